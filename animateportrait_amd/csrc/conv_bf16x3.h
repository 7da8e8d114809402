// conv_bf16x3.h -- the implicit-GEMM convolution of conv_igemm.h on the bf16 matrix pipe, at fp32-class accuracy.
//
// gfx950 has no TF32-like mode and its exact-fp32 MFMA runs at 1/16 of the bf16 rate.  This path splits
// every fp32 operand into a bf16 head and a bf16 tail (x = xh + xl, |xl| <= 2^-9 |x|) and evaluates
//     x * w  ~=  xh*wh + xh*wl + xl*wh            (the dropped xl*wl term is <= 2^-18 |x w|)
// with three v_mfma_f32_32x32x16_bf16 per tile and fp32 accumulation: 3/16 of the fp32-MFMA time per FLOP.
// bf16 keeps the fp32 exponent range, so there is no overflow / subnormal hazard (an fp16 split would need
// denormal-preserving MFMA inputs).  Measured on the full generator (ngf=64): L-inf 1.4e-4 vs the fp32
// reference, against the 1e-3 budget of BASELINE.json and 7.8e-2 for plain bf16.
//
// Data flow (same im2col-free scheme as conv_igemm.h; reference layers Module2/models/networks.py:1251, 2329-2421):
//   * split_prepass_kernel (one streaming pass per activation tensor, shared by all its consumers) applies the
//     producer's InstanceNorm + activation and writes the split tensor XS[n][head|tail][C/8][H*W + 1][8 x bf16]
//     (16-byte slots; the extra slot of every plane is all-zero and serves the zero-padding taps);
//   * the convolution stages BOTH operands with global_load_lds_dwordx4 only -- no staging registers, no VALU:
//     activation tile [head|tail][k-group][IH*IW px] slots (reflection / zero padding = per-lane source address),
//     weights pre-packed as the LDS image [head|tail][tap][k-group][cout] slots;
//   * channel chunk = 16 (one MFMA K); an A / B fragment is ONE ds_read_b128 per lane (lane = cout / pixel,
//     half-wave = k-group), conflict-free; fragments of tap t+1 are fetched while tap t multiplies;
//   * the workgroups are PERSISTENT: one per CU, each walking its share of the (image, pixel tile, cout tile)
//     list.  The (tile, chunk) stages form one flat software pipeline -- stage g+2 is issued to the LDS-DMA
//     while stage g multiplies, across tile boundaries -- so the first-stage latency of a tile and the drain of
//     the previous tile's output stores hide under MFMA work; the one barrier per stage sits in front of the
//     LAST tap of a stage (whose fragments are already in registers), so the matrix pipe never idles at it.
//     The issue window of stage g+2 is the last tap of stage g plus the first taps of stage g+1 (the buffer is free
//     from stage g's barrier on; the pieces are awaited at stage g+1's): the split 3x3 stride-1 tiles spread the
//     pieces over it, one per D MFMAs (bf3_dma_sched), the other families issue them all in the last tap of stage g;
//   * epilogue identical to the fp32 kernel (bias, activation, InstanceNorm partial statistics).
// Where the steps are: the raw LDS-DMA issue and the fragment type -- lds_dma.h; piece geometry per tile, the scalar addresses
// of a stage, the issue of a piece / a stage and the spread schedule (bf3_dma_sched) -- conv_bf3_dma.h; the stage's barrier with
// the experiment build's cycle stamps (AP_STAMP), the tile walk, fragment fetch, `stage`, the chunk loops, the epilogue and the
// tile hand-over -- the kernel below.
#pragma once
#include <type_traits>
#include <utility>

#include "conv_igemm.h"
#include "lds_dma.h"      // bf16x8, split_bf16, the raw LDS-DMA issue (glds16_sv / glds16_si, dma_wait_all), static_for

namespace apamd {

// K_ > 0: dense K x K taps.  K_ == 0: NTAP_ (1, 2 or 4) taps at run-time offsets inside a 2 x 2 window (the
// sub-pixel phases of a stride-2 transposed convolution); the count is a template parameter so that the tap
// loop unrolls with compile-time register buffers.
// ROW_ = 1: a 1 x K kernel (K horizontal taps).  The 7x7 stems (3 input channels) run this way: their input is
// expanded to "row channels" (ky, c) -- 21 of 32 channels of a split tensor -- so that the 49 x 3 products of a
// pixel become 2 channel chunks x 7 taps (ap_split_prepass_rows).
// PARTS_ = 2: split-bf16 arithmetic (head + tail of both operands staged, three MFMAs per product).
// PARTS_ = 1: plain bf16 arithmetic (AP_PRECISION_BF16, the training configurations): only the head parts are
// staged -- half the LDS image and half the LDS-DMA traffic -- and a product is ONE MFMA (fp32 accumulation).  The
// global operand layouts (XS tensors, packed weights) are the same; the kernel just skips the tail planes.
// S2D3_ = 1 (K_ == 0, NTAP_ == 4): the space-to-depth form of a 3x3 stride-2 layer with an even chunk count per input phase --
// the four phases' tap sets (4 / 2 / 2 / 1 taps) are compile-time: four chunk loops in sequence, see `stage`.
// OB16_ = 1 (plain bf16 arithmetic, dense 3x3 stride 1): the OUTPUT is stored as bf16 (round to nearest even; statistics from the
// fp32 accumulators) -- the raw outputs of the ResNet trunk and the gradients that leave its data-gradient convolutions in the
// plain-bf16 train step (ap_conv2d_fwd_bf16out): every reader of those tensors rounds them to bf16 anyway.
template <int S_, int K_, int WCO_, int MT_, int WPX_, int NT_, int NTAP_ = 0, int ROW_ = 0, int PARTS_ = 2, int S2D3_ = 0,
          int OB16_ = 0>
struct Bf3Cfg {
    static constexpr int OB16 = OB16_;
    static_assert(!OB16_ || (K_ == 3 && S_ == 1 && PARTS_ == 1 && !ROW_), "bf16 output: the plain-bf16 3x3 stride-1 tiles");
    static constexpr int CI = 16, S = S_, K = K_, WCO = WCO_, MT = MT_, WPX = WPX_, NT = NT_, ROW = ROW_, PARTS = PARTS_;
    static constexpr int S2D3 = S2D3_;
    static_assert(!S2D3_ || (K_ == 0 && NTAP_ == 4), "compile-time s2d tap sets: the 4-tap run-time-tap family");
    static_assert(PARTS == 1 || PARTS == 2, "head only, or head + tail");
    static constexpr int TMAX = K > 0 ? (ROW ? K : K * K) : NTAP_;
    static_assert(TMAX >= 1, "K == 0 needs a tap count");
    static constexpr int EXT = K > 0 ? K - 1 : 1;
    static constexpr int EXTY = (K > 0 && ROW) ? 0 : EXT;
    static constexpr int TH = WPX * NT;
    static constexpr int CO_TILE = WCO * MT * 32;
    static constexpr int IH = (TH - 1) * S + EXTY + 1;
    static constexpr int IW = 31 * S + EXT + 1;
    static constexpr int PLANE = IH * IW;                          // pixels of the staged tile
    static constexpr int XP = (2 * PLANE + 63) / 64 * 64;          // slots per part: [kgroup][pixel], padded to whole DMA pieces
    static constexpr int X_SLOTS = PARTS * XP;                     // [part][kgroup][pixel]
    static int w_slots(int ntaps) { return PARTS * ntaps * 2 * CO_TILE; }   // LDS image [part][tap][kgroup][cout], multiple of 64
    static constexpr int NIT = XP / 256 + (XP % 256 ? 1 : 0);      // DMA pieces per thread and part
    // epilogue: 32 x 36-float transposition patches (NPATCH per wave, so that two accumulator tiles are in flight
    // between the LDS write and read phases) + statistics; they live in the free stage buffer of the tile's last chunk
    static constexpr int W_BYTES_MAX = PARTS * TMAX * 2 * CO_TILE * 16;
    static constexpr int NPATCH = (NT % 2 == 0 && (8 * 32 * 36 + WPX * CO_TILE * 2) * 4 <= PARTS * XP * 16 + W_BYTES_MAX) ? 2 : 1;
    static constexpr int EPI_FLOATS = 4 * NPATCH * 32 * 36 + WPX * CO_TILE * 2;
    static_assert(WCO * WPX == 4, "4 waves per workgroup");
    static_assert(CO_TILE % 16 == 0, "weight image must be whole wave-wide LDS-DMA pieces");
    // the epilogue patches live in the (free) stage buffer of the tile's last chunk -- the LAST stage in memory, each
    // stage being one contiguous [weight image | activation image] block -- and, where a head-only stage is smaller
    // than the patches, in EPI_EXTRA bytes behind it
    static_assert(IH < 128 && IW < 256, "piece geometry is packed into 15 bits");
    // two workgroups share a CU when two stage pairs fit its 160 KB of LDS: the kernel is then compiled for <= 256 registers
    static constexpr int WG_PER_CU = (PARTS == 1 || 2 * (X_SLOTS + PARTS * TMAX * 2 * CO_TILE) * 16 + 1024 <= 80 * 1024) ? 2 : 1;
    // the LDS-DMA pieces of a stage are spread over the following stage's taps (bf3_dma_sched): the split 3x3 stride-1 tiles
    // (every other family keeps the whole issue in the stage's last tap: profiles/r07_dma_spread.md)
    static constexpr bool DMA_SPREAD = K_ == 3 && S_ == 1 && !ROW_ && PARTS_ == 2;
    static int wfloats(int ntaps) { return 2 * ntaps * 2 * CO_TILE * 4; }   // floats per packed (cout tile, chunk) weight block: always both parts
    static size_t lds_bytes(int ntaps) {                                                          // two stages (+ patches)
        const size_t stage = (size_t)(X_SLOTS + w_slots(ntaps)) * 16, epi = (size_t)EPI_FLOATS * 4;
        return 2 * stage + (epi > stage ? (epi - stage + 15) / 16 * 16 : 0);
    }
};

struct Bf3Tile {
    int n, cot, ty, tx;
};

}  // namespace apamd

// the kernel's units, each with what it reads and writes (they use Bf3Tile and take the tile configuration as C)
#include "conv_bf3_dma.h"

namespace apamd {

// seg[s].data of the bf16x3 kernel points to an XS tensor (see split_prepass_kernel); seg[s].C = channels.
// Launch with min(#tiles, #CUs) workgroups of 256 threads; needs nchunks >= 2.
// (head-only arithmetic halves the LDS image: two workgroups per CU, i.e. two waves per SIMD and <= 256 registers each)
// The DMA unit (conv_bf3_dma.h) is a struct of references into this frame -- the shape of the `[&]` closures it was, which is
// what kept every instantiation's machine code (tools/kernel_isa_diff.py is the gate for any further move).  Two things decide
// whether a lambda can leave this body unchanged.  A callee is optimised on its own before it is inlined, so what stands in
// the body itself (pgeo, woff, slots, the pending-refill set-up, the hand-over) differs once it is inside a callee, without the
// kernel's knowledge of tid and wave.  And a lambda sees `smem`, `wbuf` and `xbuf` as the LDS symbol itself (const locals with
// constant initialisers are not captured), which a unit handed them by reference does not.
// Measured, and therefore still lambdas: the epilogue (by-reference struct or function: every instantiation; naming the LDS
// symbol itself: the experiment build identical, the product build of the run-time-tap and row families not, e.g.
// Bf3Cfg<1,0,1,2,4,2,4,0,1,1,0> 25306 -> 25114 instructions), the fetch forms (both ways, e.g. Bf3Cfg<1,0,1,2,4,2,4,0,2,1,0>),
// the cycle stamps (three stamped instantiations: other register numbers).  `stage` calls all of these and stays with them.
template <class C>
__global__ __launch_bounds__(256, C::WG_PER_CU) void conv_bf16x3(const ConvKParams p) {
    constexpr int S = C::S, K = C::K, TMAX = C::TMAX, MT = C::MT, NT = C::NT, WCO = C::WCO;
    constexpr int IW = C::IW, PLANE = C::PLANE, NIT = C::NIT, CO_TILE = C::CO_TILE, XP = C::XP;
    constexpr int IWE = (IW + 1) / 2;      // even columns of a row of the LDS image (stride-2 layout, see pgeo)
    constexpr bool XPF = true;             // fragments of the next stage's tap 0 are fetched during this stage's last tap
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint4* const smem = reinterpret_cast<uint4*>(smem_raw);

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);     // scalar: LDS-DMA destinations stay in SGPRs
    const int lane = tid & 63, half = lane >> 5, l32 = lane & 31;
    const int wco = wave % WCO, wpx = wave / WCO;
    const int H = p.H, W = p.W, HW = H * W;
    const int nchunks = p.nchunks;         // even: the host pads an odd count with one all-zero weight chunk
    const int nreal = p.cin_pad >> 4;      // chunks that exist in the sources

    constexpr int T = TMAX;
    constexpr int PARTS = C::PARTS;
    constexpr int W_SLOTS = PARTS * T * 2 * CO_TILE;
    constexpr int STAGE = W_SLOTS + C::X_SLOTS;                // stage b = smem + b * STAGE: [W_SLOTS weights | X_SLOTS activations]
    uint4* const wbuf = smem;                                  // + b * STAGE
    uint4* const xbuf = smem + W_SLOTS;                        // + b * STAGE
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem_raw;

#ifdef APAMD_ABLATION
    // ---- cycle account (experiment build; tools/cycle_account.py): lane 0 of every wave records (code, s_memtime) pairs in LDS.
    // code = kind | chunk << 8 | tile ordinal << 16.  An s_memtime result is awaited with lgkmcnt(0) inside the same asm
    // statement (the compiler does not know the instruction is a scalar memory read).
    const bool stamping = p.stamps != nullptr;
    unsigned* const stamp_lds = reinterpret_cast<unsigned*>(smem_raw + p.stamp_lds_off) + wave * p.stamp_words;
    int stamp_n = 0, stamp_tile = 0;
    auto stamp_put = [&](unsigned kind, int c, unsigned long long t) __attribute__((always_inline)) {
        if (lane == 0 && stamp_n + 2 <= p.stamp_words) {
            stamp_lds[stamp_n] = kind | ((unsigned)c << 8) | ((unsigned)stamp_tile << 16);
            stamp_lds[stamp_n + 1] = (unsigned)t;
        }
        stamp_n += 2;
    };
    auto stamp_now = [&](unsigned kind, int c) __attribute__((always_inline)) {
        if (!stamping) return;
        unsigned long long t;
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
        stamp_put(kind, c, t);
    };
    // the stage's one synchronisation point, stamped: arrival (0), DMA of the next stage landed (1), barrier passed (2)
    auto stage_sync = [&](int c) __attribute__((always_inline)) {
        if (!stamping) {
            dma_wait_all();
            if (!AP_ABLATE(p, 2)) __syncthreads();
            return;
        }
        unsigned long long ta, tb, tc;
        asm volatile("s_memtime %0\n\ts_waitcnt vmcnt(0)\n\ts_memtime %1\n\ts_waitcnt lgkmcnt(0)\n\ts_barrier\n\t"
                     "s_memtime %2\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(ta), "=&s"(tb), "=&s"(tc)::"memory");
        stamp_put(0, c, ta);
        stamp_put(1, c, tb);
        stamp_put(2, c, tc);
    };
#define AP_STAMP(kind, c) stamp_now(kind, c)
#else
    auto stage_sync = [&](int) __attribute__((always_inline)) {
        dma_wait_all();
        __syncthreads();
    };
#define AP_STAMP(kind, c) ((void)0)
#endif

    // ---- this workgroup's tiles.  Workgroup b runs on XCD b % 8; each XCD owns a contiguous range of the tile
    // list (cout tile fastest, so the workgroups of an XCD share activation tiles through its L2) and its
    // workgroups walk that range in lock step.
    int tile, tile_end, tile_step;
    {
        const int G = gridDim.x, b = blockIdx.x;
        const int nx = G < 8 ? G : 8;                              // XCDs that received workgroups
        const int xcd = b % nx, idx = b / nx;
        const int ntl = p.N * p.tiles_y * p.tiles_x * p.co_tiles;
        const int q = ntl / nx, r = ntl % nx;
        const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
        tile_step = (G - xcd + nx - 1) / nx;                       // workgroups on this XCD
        tile = base + idx;
        tile_end = base + q + (xcd < r ? 1 : 0);
    }
    if (tile >= tile_end) return;

    // ---- DMA geometry: piece k of this thread covers slot it = tid + k*256 of a part = (k-group, tile pixel);
    // source = that pixel of the image (reflected) or the all-zero slot (zero padding, tile padding)
    int pgeo[NIT];      // (k-group << 15) | (ly << 8) | lx of the piece, or -1 beyond the tile
#pragma unroll
    for (int k = 0; k < NIT; ++k) {
        const int it = tid + k * 256;
        const int kg = it >= PLANE ? 1 : 0;
        const int pix = it - kg * PLANE;
        const int ly = pix / IW;
        int lx = pix - ly * IW;
        // stride 2: a row of the LDS image holds the even image columns first, then the odd ones, so that the 32
        // pixels of a fragment (image columns 2 l + kx) are CONSECUTIVE slots -- stride-2 slots are a 2-way bank
        // conflict on every ds_read_b128 (8.2 M conflict cycles per launch, profiles/r01y_pmc_mfma.md)
        if constexpr (S == 2) lx = lx < IWE ? 2 * lx : 2 * (lx - IWE) + 1;
        pgeo[k] = it < 2 * PLANE ? ((kg << 15) | (ly << 8) | lx) : -1;
    }
    using Dma = Bf3Dma<C>;                                         // locate, setup, piece, issue: conv_bf3_dma.h
    constexpr int NWP = Dma::NWP, NPIECE = Dma::NPIECE;
    unsigned woff[NWP];            // byte offset of this lane's slot in weight piece j
#pragma unroll
    for (int j = 0; j < NWP; ++j) woff[j] = ((j * 4 + wave) * 64 + lane) * 16;
    // the issue schedule (bf3_dma_sched) and the state a stage hands to the next one: conv_bf3_dma.h
    constexpr int NM_STAGE = Dma::NM_STAGE;                        // MFMA slots of a tap
    constexpr int DMA_D = Dma::DMA_D, LAST_ISSUE_TAP = Dma::LAST_ISSUE_TAP, DMA_PPT = Dma::DMA_PPT, DMA_N0 = Dma::DMA_N0;
    Bf3DmaCtx pend;
    int pig[NIT];
    int pdma;
    const Dma dma{p, wave, H, W, HW, nchunks, nreal, lds0, pgeo, woff, pend, pig, pdma};

    // fragment addresses (16-byte slots)
    const int a_slot = half * CO_TILE + wco * MT * 32 + l32;                       // + ((part*T + t)*2) * CO_TILE + m*32
    const int b_slot = half * PLANE + (wpx * NT) * S * IW + (S == 2 ? l32 : l32 * S);   // + part*XP + toff + q*S*IW

    f32x16 acc[MT][NT];
    bf16x8 ah[2][MT], al[2][MT], bh[2][NT], bl[2][NT];
    // Dense stride-1 taps share activation fragments vertically: the fragment of pixel row q at tap (ky+1, kx) is the
    // one of row q+1 at tap (ky, kx).  With the taps walked column by column (kx outer, ky inner) a wave keeps a sliding
    // window of NT + K - 1 row fragments per kx and reads ONE new row per tap (NT at a column change) instead of NT.
    // Used for the 4x4 layers (MT = 1: 22 instead of 40 ds_read_b128 per tap column, 196 -> 170..185 us on the
    // PatchGAN's 256 -> 512 layer).  The split 3x3 kernel (MT = 2: 72 instead of 108 per chunk) is no faster per launch with it
    // -- its fragment reads already hide under the MFMAs -- but a third fewer LDS reads is power the chip gives back as clock:
    // 2257 / 2258 / 2259 -> 2272 / 2275 / 2263 frames/s, same box, interleaved (round 5, gpurun_out/r05n; the kernel runs at the
    // board's power limit, profiles/r05e_power_gen.md), so it takes the window as well.
    // ... with ONE product per tap (plain bf16, PARTS = 1) it is the other way round: 6 fragment reads per 8 MFMAs and 8 waves on
    // a CU's LDS port keep that port ~75 % busy, so the head-only 3x3 kernel takes the window too (36 instead of 54 reads per chunk):
    // 132.8-134.8 -> 130.3 us per launch in the plain-bf16 train step (gpurun_out/r04ah_train_bf16_kernel_stats.md), i.e. the
    // port was not the bound either; kept because it is not slower.
    constexpr bool WIN = (K == 4 || (K == 3 && NT > 1)) && !C::ROW && S == 1;
    constexpr int WR = WIN ? NT + K - 1 : 1;
    bf16x8 wh[2][WR], wl[2][WR];                                   // [kx parity][window row]
    auto fetch_a = [&](int stage_buf, int t, int buf) __attribute__((always_inline)) {
        const uint4* Wc = wbuf + stage_buf * STAGE + a_slot;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            ah[buf][m] = *reinterpret_cast<const bf16x8*>(Wc + ((0 * T + t) * 2) * CO_TILE + m * 32);
            if constexpr (PARTS == 2) al[buf][m] = *reinterpret_cast<const bf16x8*>(Wc + ((1 * T + t) * 2) * CO_TILE + m * 32);
        }
    };
    auto fetch_brow = [&](int stage_buf, int kx, int j, int wb) __attribute__((always_inline)) {
        const uint4* Xc = xbuf + stage_buf * STAGE + b_slot + j * IW + kx;
        wh[wb][j] = *reinterpret_cast<const bf16x8*>(Xc);
        if constexpr (PARTS == 2) wl[wb][j] = *reinterpret_cast<const bf16x8*>(Xc + XP);
    };
    auto fetch = [&](int stage_buf, int t, int buf) __attribute__((always_inline)) {
        const uint4* Wc = wbuf + stage_buf * STAGE + a_slot;
        const uint4* Xc = xbuf + stage_buf * STAGE + b_slot;
        int toff;
        if constexpr (K > 0) toff = C::ROW ? t : (t / K) * IW + (S == 2 ? ((t % K) & 1) * IWE + ((t % K) >> 1) : (t % K));
        else toff = (int)((p.tap_bits >> (2 * t)) & 1u) * IW + (int)((p.tap_bits >> (2 * t + 1)) & 1u);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            ah[buf][m] = *reinterpret_cast<const bf16x8*>(Wc + ((0 * T + t) * 2) * CO_TILE + m * 32);
            if constexpr (PARTS == 2) al[buf][m] = *reinterpret_cast<const bf16x8*>(Wc + ((1 * T + t) * 2) * CO_TILE + m * 32);
        }
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            bh[buf][q] = *reinterpret_cast<const bf16x8*>(Xc + toff + q * S * IW);
            if constexpr (PARTS == 2) bl[buf][q] = *reinterpret_cast<const bf16x8*>(Xc + XP + toff + q * S * IW);
        }
    };

    // fragment r of tap t (r < 2 MT: weights head / tail alternating; then activations)
    auto fetch_one = [&](int stage_buf, int t, int buf, int r) __attribute__((always_inline)) {
        const uint4* Wc = wbuf + stage_buf * STAGE + a_slot;
        const uint4* Xc = xbuf + stage_buf * STAGE + b_slot;
        int toff;
        if constexpr (K > 0) toff = C::ROW ? t : (t / K) * IW + (S == 2 ? ((t % K) & 1) * IWE + ((t % K) >> 1) : (t % K));
        else toff = (int)((p.tap_bits >> (2 * t)) & 1u) * IW + (int)((p.tap_bits >> (2 * t + 1)) & 1u);
        if (r < PARTS * MT) {
            const int m = r / PARTS;
            if (PARTS == 2 && (r & 1)) al[buf][m] = *reinterpret_cast<const bf16x8*>(Wc + ((1 * T + t) * 2) * CO_TILE + m * 32);
            else ah[buf][m] = *reinterpret_cast<const bf16x8*>(Wc + ((0 * T + t) * 2) * CO_TILE + m * 32);
        } else {
            const int q = (r - PARTS * MT) / PARTS;
            if (PARTS == 2 && (r & 1)) bl[buf][q] = *reinterpret_cast<const bf16x8*>(Xc + XP + toff + q * S * IW);
            else bh[buf][q] = *reinterpret_cast<const bf16x8*>(Xc + toff + q * S * IW);
        }
    };
    // the same for the windowed form: fragment r of tap (0, 0) -- weights into buffer `buf`, window rows into `wb`
    auto fetch_one_win = [&](int stage_buf, int buf, int wb, int r) __attribute__((always_inline)) {
        const uint4* Wc = wbuf + stage_buf * STAGE + a_slot;
        const uint4* Xc = xbuf + stage_buf * STAGE + b_slot;
        if (r < PARTS * MT) {
            const int m = r / PARTS;
            if (PARTS == 2 && (r & 1)) al[buf][m] = *reinterpret_cast<const bf16x8*>(Wc + ((1 * T + 0) * 2) * CO_TILE + m * 32);
            else ah[buf][m] = *reinterpret_cast<const bf16x8*>(Wc + ((0 * T + 0) * 2) * CO_TILE + m * 32);
        } else {
            const int q = (r - PARTS * MT) / PARTS;
            if (PARTS == 2 && (r & 1)) wl[wb][q] = *reinterpret_cast<const bf16x8*>(Xc + XP + q * IW);
            else wh[wb][q] = *reinterpret_cast<const bf16x8*>(Xc + q * IW);
        }
    };

    Bf3Tile cur, nxt;
    int cgoff[NIT], ngoff[NIT];
    dma.locate(tile, cur, cgoff);
    AP_STAMP(7, 0);                                                // kernel entry (tile geometry done)
    dma.issue(cur, cgoff, 0, 0);
    dma.issue(cur, cgoff, 1, 1);
    dma_wait_all();
    __syncthreads();
    AP_STAMP(8, 0);                                                // first two stages landed
    // the launch's first two stages are staged whole: nothing pending.  (The carried scalars start from scalar registers, not
    // from constants: a zero shared with a vector register's initial value turns the whole carried chain into vector registers,
    // which the raw assembly of a piece cannot take.)
    if constexpr (DMA_D > 0) {
        pend = dma.setup(cur.n, cur.cot, 1, 1);
        asm volatile("s_mov_b32 %0, 0" : "=s"(pdma));
#pragma unroll
        for (int k = 0; k < NIT; ++k) pig[k] = cgoff[k];
    }

    // taps of the 2 x 2 window that exist for the current tile (fused sub-pixel phases; wave-uniform)
    auto tapmask_of = [&](const Bf3Tile& t) -> unsigned {
        if (K != 0 || p.nphase <= 1) return 0xFu;
        return (unsigned)__builtin_amdgcn_readfirstlane((int)p.ph_tapmask[t.cot / p.co_tiles_phase]);
    };
    unsigned tmask = tapmask_of(cur);
    for (;;) {
        const bool has_next = tile + tile_step < tile_end;
        dma.locate(has_next ? tile + tile_step : tile, nxt, ngoff);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
            for (int q = 0; q < NT; ++q)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[m][q][r] = 0.f;

        // one pipeline stage = one 16-channel chunk; P = its LDS stage buffer (compile-time in each copy).
        // MASK != 0 (space-to-depth 3x3 layers, K == 0 with 4 taps): the stage's taps are known at COMPILE time -- the set bits of
        // MASK -- so an absent tap costs neither MFMAs nor fragment reads.  With the run-time mask only the MFMAs were skipped:
        // a stage then issued 32 ds_read_b128 per wave for 27 MFMAs on average (4 / 2 / 2 / 1 taps of the four input phases),
        // and the LDS read port, not the matrix pipe, bounded the kernel (8 waves per CU, profiles/r03_ablate_layers.md).
        auto stage = [&](auto ptag, auto mtag, int c) __attribute__((always_inline)) {
            constexpr int P = decltype(ptag)::value;
            constexpr unsigned MASK = decltype(mtag)::value;
            static_assert(MASK == 0 || (K == 0 && (MASK & 1u)), "compile-time tap sets: run-time-tap family, tap 0 always present");
            constexpr int NREAL = MASK ? __builtin_popcount(MASK) : TMAX;
            auto tap_of = [](int i) constexpr {                   // i-th tap of the stage
                if (!MASK) return i;
                int n = 0;
                for (int b = 0; b < TMAX; ++b)
                    if ((MASK >> b) & 1u) {
                        if (n == i) return b;
                        ++n;
                    }
                return 0;
            };
            // taps of this stage: of the tile's phase, or (space-to-depth 3x3) of the chunk's input phase
            const unsigned tm = MASK ? MASK : ((K == 0 && p.s2d_div > 0) ? p.s2d_mask[c / p.s2d_div < 3 ? c / p.s2d_div : 3] : tmask);
            constexpr int FP = (XPF && (NREAL & 1)) ? P : 0;       // register buffer of tap 0
            constexpr int WP = (XPF && (K & 1)) ? P : 0;           // window buffer of kx = 0
            if (!XPF || c == 0) {
                if constexpr (WIN) {
                    fetch_a(P, 0, FP);
#pragma unroll
                    for (int q = 0; q < NT; ++q) fetch_brow(P, 0, q, WP & 1);
                } else {
                    fetch(P, 0, FP);
                }
            }
#pragma unroll
            for (int ti = 0; ti < NREAL; ++ti) {
                const int tp = tap_of(ti);
                // windowed form: taps column by column; t = the tap's index in the weight image
                constexpr int KD = K > 0 ? K : 1;                    // (K == 0 instantiations never take the windowed form)
                const int kx = WIN ? tp / KD : 0, ky = WIN ? tp % KD : 0;
                const int t = WIN ? ky * K + kx : tp;
                const int cb = (ti + FP) & 1, wb = (kx + WP) & 1;
                const bool last = ti == NREAL - 1;
                auto mfma_one = [&](int i) __attribute__((always_inline)) {
                    // the three partial products go round all MT*NT accumulators in turn, so consecutive MFMAs
                    // never wait on each other's result (small terms first)
                    const int g = PARTS == 2 ? i / (MT * NT) : 2, m = (i % (MT * NT)) / NT, q = i % NT;
                    const bf16x8 xh = WIN ? wh[wb][WIN ? ky + q : 0] : bh[cb][q];
                    const bf16x8 xl = WIN ? wl[wb][WIN ? ky + q : 0] : bl[cb][q];
                    if (g == 0) acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[cb][m], xh, acc[m][q], 0, 0, 0);
                    else if (g == 1) acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[cb][m], xl, acc[m][q], 0, 0, 0);
                    else acc[m][q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[cb][m], xh, acc[m][q], 0, 0, 0);
                };
                constexpr int NM = (PARTS == 2 ? 3 : 1) * MT * NT, NRD = PARTS * (MT + NT);
                bool spread_tap = false;
                if constexpr (DMA_D > 0) {
                    static_assert(MASK == 0 && NM == NM_STAGE, "one issue schedule for every stage of the kernel");
                    spread_tap = !last && ti <= LAST_ISSUE_TAP;
                }
                if (spread_tap) {
                    if constexpr (DMA_D > 0) {
                    // a tap that carries deferred LDS-DMA pieces of the PREVIOUS stage's refill (bf3_dma_sched).  The scalar branch
                    // of a piece ends a scheduling region, so the order is written out slot by slot: the next tap's fragment
                    // reads where the plain form below puts them (one in front of every PER-th MFMA), a piece behind every D-th MFMA.
                    constexpr int NRD1 = PARTS * (MT + 1);
                    const int kx2 = WIN ? (tp + 1) / KD : 0, ky2 = WIN ? (tp + 1) % KD : 0;
                    const bool same_col = WIN && kx2 == kx;         // (windowed form: one new window row instead of NT)
                    const int nrd = same_col ? NRD1 : NRD;
                    const int per = (NM + nrd - 1) / nrd;
                    const int tn = WIN ? ky2 * K + kx2 : t + 1;      // the next tap's index in the weight image
                    auto read_next = [&](int r) __attribute__((always_inline)) {
                        if constexpr (WIN) {
                            if (r < PARTS * MT) {
                                const uint4* Wc = wbuf + P * STAGE + a_slot + ((((PARTS == 2 && (r & 1)) ? 1 : 0) * T + tn) * 2) * CO_TILE + (r / PARTS) * 32;
                                if (PARTS == 2 && (r & 1)) al[cb ^ 1][r / PARTS] = *reinterpret_cast<const bf16x8*>(Wc);
                                else ah[cb ^ 1][r / PARTS] = *reinterpret_cast<const bf16x8*>(Wc);
                            } else {
                                const int q = (r - PARTS * MT) / PARTS;
                                const int row = same_col ? ky2 + NT - 1 : q, col = same_col ? kx : kx2, wsel = same_col ? wb : wb ^ 1;
                                const uint4* Xc = xbuf + P * STAGE + b_slot + row * IW + col;
                                if (PARTS == 2 && (r & 1)) wl[wsel][row] = *reinterpret_cast<const bf16x8*>(Xc + XP);
                                else wh[wsel][row] = *reinterpret_cast<const bf16x8*>(Xc);
                            }
                        } else {
                            fetch_one(P, tn, cb ^ 1, r);
                        }
                    };
                    static_for<NM>([&](auto it) __attribute__((always_inline)) {
                        constexpr int i = decltype(it)::value;
                        if (i % per == 0 && i / per < nrd) read_next(i / per);
                        mfma_one(i);
                        if constexpr (i % DMA_D == DMA_D - 1 && i / DMA_D < DMA_PPT) {
                            static_for<LAST_ISSUE_TAP + 1>([&](auto tt) __attribute__((always_inline)) {
                                constexpr int j = DMA_N0 + decltype(tt)::value * DMA_PPT + i / DMA_D;
                                if constexpr (j < NPIECE) {
                                    if (ti == decltype(tt)::value && pdma) dma.piece(pend, pig, pig, false, std::integral_constant<int, j>{});
                                }
                            });
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    });
                    }
                } else if (!last) {
                    int nrd = NRD;                                  // LDS reads issued for the next tap
                    if constexpr (WIN) {
                        const int kx2 = (tp + 1) / KD, ky2 = (tp + 1) % KD;
                        fetch_a(P, ky2 * K + kx2, cb ^ 1);
                        if (kx2 == kx) {
                            fetch_brow(P, kx, ky2 + NT - 1, wb);
                            nrd = PARTS * (MT + 1);
                        } else {
#pragma unroll
                            for (int q = 0; q < NT; ++q) fetch_brow(P, kx2, q, wb ^ 1);
                        }
                    } else {
                        fetch(P, MASK ? tap_of(ti + 1) : t + 1, cb ^ 1);
                    }
                    if (K != 0 || ((tm >> tp) & 1u)) {       // (an absent tap of a fused phase: zero weights, nothing to add)
#pragma unroll
                    for (int i = 0; i < NM; ++i) mfma_one(i);
                    }
                    // pin the schedule: the next tap's fragment reads are spread evenly between this tap's MFMAs
                    // (left alone, the scheduler sinks every read to just before its first use and stalls on it)
                    constexpr int PER = (NM + NRD - 1) / NRD, NRD1 = PARTS * (MT + 1), PER1 = (NM + NRD1 - 1) / NRD1;
                    if (nrd == NRD) {
#pragma unroll
                        for (int i = 0; i < NRD; ++i) {
                            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // one LDS read
                            __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);    // PER MFMAs
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < NRD1; ++i) {
                            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                            __builtin_amdgcn_sched_group_barrier(0x008, PER1, 0);
                        }
                    }
                } else {
                    // every fragment of this stage is in registers: the stage buffer can be refilled, and the
                    // next stage (issued one stage ago) has landed once everybody is past the barrier.  The DMA
                    // pieces of stage c+2 (past the tile's end: chunk 0 of the next tile) and the fragment reads of
                    // the next stage's tap 0 are issued one per MFMA slot, so the matrix pipe keeps running.
                    // The last stage of a tile issues nothing (its buffer becomes the epilogue's patch area); the last but one
                    // stages chunk 0 of the NEXT tile -- without a next tile this tile's own chunk 0 again, which nobody reads:
                    // an unconditional issue keeps the pieces free of branches.  What a piece may cost is decided here:
                    // the scalar addresses are pinned in SGPRs by dma_setup, the per-lane offset is one select,
                    // and the `more` test in front of a piece is a bare scalar branch.  (Before, the compiler put the branch, the
                    // offset select and the re-derivation of the 64-bit source address -- ten scalar multiplies / adds and a
                    // v_readlane of a spilled LDS address -- in front of EVERY piece: 74 cycles per MFMA slot of this tap
                    // instead of 32, ~1000 cycles per stage, profiles/r05_dominant_cycle_account.md.)
                    const bool more = c + 1 < nchunks;
                    const bool tail = c + 2 >= nchunks;
                    const Bf3DmaCtx d = dma.setup(tail ? nxt.n : cur.n, tail ? nxt.cot : cur.cot, tail ? 0 : c + 2, P);
                    // (the offset selects sit HERE, in front of the barrier: vector selects on SGPR-pair masks between LDS-DMA
                    // pieces and MFMAs are what makes a kernel disturb a co-resident one, profiles/r04_cohazard.md)
                    int ig[NIT];
#pragma unroll
                    for (int k = 0; k < NIT; ++k) {
                        ig[k] = tail ? ngoff[k] : cgoff[k];
                        asm volatile("" : "+v"(ig[k]));                 // (pinned here: the compiler sinks the select to its use)
                    }
                    stage_sync(c);
                    constexpr int PPS = (NPIECE + NM - 1) / NM;                 // DMA pieces per MFMA slot
                    constexpr int RPS = (NRD + NM - 1) / NM;                    // fragment reads per MFMA slot
                    constexpr int R0 = NM - (NRD + RPS - 1) / RPS;              // first slot that carries reads
                    const bool real_tap = K != 0 || ((tm >> tp) & 1u);
                    // (the MFMAs stay in straight-line code: with them inside the two arms of a branch the accumulators became phi
                    // nodes and the allocator moved all 128 between AGPRs and VGPRs every stage)
                    // (as scalar integers: left as `bool`s the compiler parks the condition in a VGPR and tests it from there)
                    const int dma_on = __builtin_amdgcn_readfirstlane((more && !AP_ABLATE(p, 1)) ? 1 : 0);
                    static_for<NM>([&](auto it) __attribute__((always_inline)) {
                        constexpr int i = decltype(it)::value;
                        if (real_tap) mfma_one(i);
                        if constexpr (DMA_D > 0) {
                            // the first N0 pieces, one behind every D-th MFMA; the others ride on the next stage's taps
                            if constexpr (i % DMA_D == DMA_D - 1 && i / DMA_D < DMA_N0) {
                                if (dma_on) dma.piece(d, ig, ig, false, std::integral_constant<int, i / DMA_D>{});
                            }
                        } else {
                            static_for<PPS>([&](auto ppt) __attribute__((always_inline)) {
                                constexpr int j = i * PPS + decltype(ppt)::value;
                                if constexpr (j < NPIECE) {
                                    if (dma_on) dma.piece(d, ig, ig, false, std::integral_constant<int, j>{});
                                }
                            });
                        }
                        if constexpr (XPF && i >= R0) {
                            if (more) {
#pragma unroll
                                for (int rr = 0; rr < RPS; ++rr)
                                    if ((i - R0) * RPS + rr < NRD) {
                                        if constexpr (WIN) fetch_one_win(P ^ 1, cb ^ 1, ((K & 1) ? (P ^ 1) : 0) & 1, (i - R0) * RPS + rr);
                                        else fetch_one(P ^ 1, 0, cb ^ 1, (i - R0) * RPS + rr);
                                    }
                            }
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    });
                    if constexpr (DMA_D > 0) {                     // the rest of this refill: the next stage's first taps
                        pend = d;
                        pdma = dma_on;
#pragma unroll
                        for (int k = 0; k < NIT; ++k) pig[k] = ig[k];
                    }
                }
            }
        };
        // nchunks is even: chunk pairs run straight-line through stage buffers 0 and 1 (a run-time choice of the
        // buffer per stage makes the register allocator shuttle all accumulators between VGPRs and AGPRs)
        using P0 = std::integral_constant<int, 0>;
        using P1 = std::integral_constant<int, 1>;
        if constexpr (C::S2D3) {
            // chunks [r * s2d_div, (r + 1) * s2d_div) belong to input phase r = (ry, rx), whose taps inside the 2 x 2 window are
            // all four / the left column / the top row / the corner: one straight-line chunk loop per phase (s2d_div is even)
            const int cpp = p.s2d_div;
            int c = 0;
            for (; c < cpp; c += 2) {
                stage(P0{}, std::integral_constant<unsigned, 0xFu>{}, c);
                stage(P1{}, std::integral_constant<unsigned, 0xFu>{}, c + 1);
            }
            for (; c < 2 * cpp; c += 2) {
                stage(P0{}, std::integral_constant<unsigned, 0x5u>{}, c);
                stage(P1{}, std::integral_constant<unsigned, 0x5u>{}, c + 1);
            }
            for (; c < 3 * cpp; c += 2) {
                stage(P0{}, std::integral_constant<unsigned, 0x3u>{}, c);
                stage(P1{}, std::integral_constant<unsigned, 0x3u>{}, c + 1);
            }
            for (; c < nchunks; c += 2) {
                stage(P0{}, std::integral_constant<unsigned, 0x1u>{}, c);
                stage(P1{}, std::integral_constant<unsigned, 0x1u>{}, c + 1);
            }
        } else {
            for (int c = 0; c < nchunks; c += 2) {
                stage(P0{}, std::integral_constant<unsigned, 0u>{}, c);
                stage(P1{}, std::integral_constant<unsigned, 0u>{}, c + 1);
            }
        }
        AP_STAMP(3, 0);                                            // last MFMA issued
        constexpr int pl = 1;                                      // stage buffer of the last chunk: free now; the
                                                                   // next tile's chunk 0 sits in buffer 0 again

        // ACT >= 0: activation known at compile time (a run-time switch per element costs scalar branches)
        auto epilogue = [&](auto atag) __attribute__((always_inline)) {
            constexpr int ACT = decltype(atag)::value;
            auto actf = [&](float v) { return ACT >= 0 ? apply_act(v, ACT) : apply_act(v, p.act); };
            // ---- epilogue.  MFMA C/D layout: column j = lane & 31 (pixel), row i = (r & 3) + 8 * (r >> 2) + 4 * half
            // (cout).  Each 32 x 32 tile is transposed through a private LDS patch so that a lane owns 4 consecutive
            // pixels of one cout row: 16-byte global stores (the dword-per-lane form is store-issue bound) and a
            // 3-step row reduction for the InstanceNorm statistics instead of a 5-step one per accumulator register.
            constexpr int TS = 36;                                            // patch row stride (floats, 16-B aligned)
            float* const epi = reinterpret_cast<float*>(smem + pl * STAGE);
            constexpr int NP = C::NPATCH;
            float* const patch0 = epi + wave * (NP * 32 * TS);
            float* const sred = epi + 4 * NP * 32 * TS;                        // [WPX][CO_TILE][2]
            const int n = cur.n;
            int cot = cur.cot, oy_off = p.oy_off, ox_off = p.ox_off, stat_off = p.stat_tile_off;
            if (p.nphase > 1) {                                // fused sub-pixel phases: (phase, cout tile of the phase)
                const int ph = cot / p.co_tiles_phase;
                cot -= ph * p.co_tiles_phase;
                oy_off = p.ph_oy[ph];
                ox_off = p.ph_ox[ph];
                stat_off = p.ph_stat[ph];
            }
            const int oy0 = cur.ty * C::TH, ox0 = cur.tx * 32;
            const int co_base = cot * CO_TILE + wco * MT * 32;
            const bool want_stats = p.stats != nullptr;
            // 16-byte fp32 stores of 4 pixels (the general loop's `full` form and fast32): every stride a multiple of 4 elements
            // and y 16-byte aligned -- an output window (ap_out_view) may have any strides
            const bool vec_ok = ((p.o_rstride | (int)p.o_cstride | (int)p.o_nstride) & 3) == 0 && p.osx == 1 && ox_off == 0 &&
                                (reinterpret_cast<uintptr_t>(p.y) & 15) == 0;
            const bool full = vec_ok && ox0 + 32 <= p.OW;                      // whole 32-pixel rows: no per-element edge tests
            const int prow = lane >> 3, pcol = (lane & 7) * 4;
            const int oxv = ox0 + pcol;
            bool octet = false;
            if constexpr (C::K == 0 || C::ROW || (C::K == 3 && C::S == 1 && C::PARTS == 2 && !C::OB16)) {
                // ---- channel-octet output y[n][Cout/8][OH*OW][8] (ap_conv2d_fwd_octet; the run-time-tap and row families
                // only: the producers of the warp kernel's input).  The MFMA layout already holds 4 consecutive couts of
                // one pixel per lane and register quad (row = (r & 3) + 8 (r >> 2) + 4 half), and the two halves of a wave
                // hold the two halves of an octet: 16-byte stores straight from the accumulators, a wave covers 32 pixels
                // x 32 bytes = 1 KiB contiguous; no LDS patch.  Row sums by a 5-step butterfly per accumulator register.
                octet = p.o_octet != 0;
                if (octet) {
                    const int ox = ox0 + l32;
                    const long long ohw = (long long)p.OH * p.OW;
                    // (round 6) every cout, row and column of the tile inside the tensor, no bias, no activation -- tested once, wave-uniform:
                    // the stores and sums below then run without the per-lane test (see fast32)
                    const bool allv = !(C::WG_PER_CU == 2 && (C::K == 0 || (C::ROW && C::MT == 2))) &&
                                      __builtin_amdgcn_readfirstlane((int)(p.bias == nullptr && ACT == 0 && co_base + MT * 32 <= p.Cout &&
                                                                           oy0 + C::TH <= p.OH && ox0 + 32 <= p.OW)) != 0;
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        float s16[16], q16[16];
#pragma unroll
                        for (int r = 0; r < 16; ++r) { s16[r] = 0.f; q16[r] = 0.f; }
                        if (allv) {
#pragma unroll
                            for (int g = 0; g < 4; ++g) {
                                const int co = co_base + m * 32 + g * 8 + 4 * half;
                                float* const ob = p.y + (long long)n * p.o_nstride + (long long)(co >> 3) * ohw * 8 + (co & 7) +
                                                  ((long long)(oy0 + wpx * NT) * p.OW + ox) * 8;
#pragma unroll
                                for (int q = 0; q < NT; ++q) {
                                    float vv[4];
#pragma unroll
                                    for (int j = 0; j < 4; ++j) {
                                        vv[j] = acc[m][q][g * 4 + j];
                                        s16[g * 4 + j] += vv[j];
                                        q16[g * 4 + j] += vv[j] * vv[j];
                                    }
                                    *reinterpret_cast<float4*>(ob + (long long)q * p.OW * 8) = make_float4(vv[0], vv[1], vv[2], vv[3]);
                                }
                            }
                        } else
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const int co = co_base + m * 32 + g * 8 + 4 * half;          // 4 consecutive couts (Cout % 8 == 0)
                            const bool cok = co < p.Cout;
                            float bv[4] = {0.f, 0.f, 0.f, 0.f};
                            if (p.bias != nullptr && cok) {
#pragma unroll
                                for (int j = 0; j < 4; ++j) bv[j] = p.bias[co + j];
                            }
                            float* const obase = p.y + (long long)n * p.o_nstride + (long long)(co >> 3) * ohw * 8 + (co & 7);
#pragma unroll
                            for (int q = 0; q < NT; ++q) {
                                const int oy = oy0 + wpx * NT + q;
                                if (cok && oy < p.OH && ox < p.OW) {
                                    float vv[4];
#pragma unroll
                                    for (int j = 0; j < 4; ++j) {
                                        vv[j] = acc[m][q][g * 4 + j] + bv[j];
                                        s16[g * 4 + j] += vv[j];
                                        q16[g * 4 + j] += vv[j] * vv[j];
                                    }
                                    *reinterpret_cast<float4*>(obase + ((long long)oy * p.OW + ox) * 8) =
                                        make_float4(actf(vv[0]), actf(vv[1]), actf(vv[2]), actf(vv[3]));
                                }
                            }
                        }
                        if (want_stats) {
                            // 16 row sums over the 32 lanes of a half-wave as a transpose-reduce: at every step a lane
                            // hands half of its rows to the partner and keeps the sums of the other half (8 + 4 + 2 + 1
                            // exchanges, then one plain step) -- 16 shuffles per quantity instead of 16 x 5
                            auto fold = [&](float (&v)[16]) {
                                const bool b16 = l32 & 16, b8 = l32 & 8, b4 = l32 & 4, b2 = l32 & 2;
                                float w8[8], w4[4], w2[2];
#pragma unroll
                                for (int i = 0; i < 8; ++i)
                                    w8[i] = (b16 ? v[i + 8] : v[i]) + __shfl_xor(b16 ? v[i] : v[i + 8], 16, 64);
#pragma unroll
                                for (int i = 0; i < 4; ++i)
                                    w4[i] = (b8 ? w8[i + 4] : w8[i]) + __shfl_xor(b8 ? w8[i] : w8[i + 4], 8, 64);
#pragma unroll
                                for (int i = 0; i < 2; ++i)
                                    w2[i] = (b4 ? w4[i + 2] : w4[i]) + __shfl_xor(b4 ? w4[i] : w4[i + 2], 4, 64);
                                float w1 = (b2 ? w2[1] : w2[0]) + __shfl_xor(b2 ? w2[0] : w2[1], 2, 64);
                                return w1 + __shfl_xor(w1, 1, 64);
                            };
                            const float s = fold(s16), q2 = fold(q16);
                            if ((l32 & 1) == 0) {
                                const int r = ((l32 >> 4) & 1) * 8 + ((l32 >> 3) & 1) * 4 + ((l32 >> 2) & 1) * 2 + ((l32 >> 1) & 1);
                                float* d = sred + ((wpx * CO_TILE) + wco * MT * 32 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * half) * 2;
                                d[0] = s;
                                d[1] = q2;
                            }
                        }
                    }
                }
            }
            bool wide16 = false;
            if constexpr (C::OB16) {
                // ---- bf16 output, whole 32-pixel rows at 16-byte aligned addresses (the forward outputs of the trunk): a lane takes
                // EIGHT consecutive pixels of a cout row from the patch (two ds_read_b128) and stores them as ONE 16-byte word --
                // 2 store instructions per 32 x 32 tile where the 4-pixel form below needs 4.  The epilogue is bound by the number
                // of store instructions a CU can retire (~115 cycles each whatever their width: MI355X_MICROARCH.md "store tail",
                // profiles/r05_dominant_cycle_account.md), so the 8-byte form was no faster than the fp32 output it replaced.
                // (every cout and row of the tile inside the tensor as well: the path below is straight-line code -- see fast32)
                wide16 = __builtin_amdgcn_readfirstlane((int)(p.osx == 1 && ox_off == 0 && ox0 + 32 <= p.OW && co_base + MT * 32 <= p.Cout &&
                         oy0 + C::TH <= p.OH && ((p.o_rstride | (int)p.o_cstride | (int)p.o_nstride) & 7) == 0 &&
                         (reinterpret_cast<uintptr_t>(p.y) & 15) == 0)) != 0;
                if (wide16) {
                    const int prow8 = lane >> 2, pcol8 = (lane & 3) * 8;
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        float s2[2] = {0.f, 0.f}, q2s[2] = {0.f, 0.f};
                        float bv2[2];
                        long long cb2[2];
                        bool cok2[2];
#pragma unroll
                        for (int ps = 0; ps < 2; ++ps) {
                            const int co = co_base + m * 32 + ps * 16 + prow8;
                            cok2[ps] = co < p.Cout;
                            bv2[ps] = (p.bias != nullptr && cok2[ps]) ? p.bias[co] : 0.f;
                            cb2[ps] = (long long)n * p.o_nstride + (long long)co * p.o_cstride + ox0 + pcol8;
                        }
#pragma unroll
                        for (int q0 = 0; q0 < NT; q0 += NP) {
#pragma unroll
                            for (int b = 0; b < NP; ++b)
#pragma unroll
                                for (int r = 0; r < 16; ++r)
                                    patch0[b * (32 * TS) + ((r & 3) + 8 * (r >> 2) + 4 * half) * TS + l32] = acc[m][q0 + b][r];
#pragma unroll
                            for (int b = 0; b < NP; ++b) {
                                const int oy = oy0 + wpx * NT + q0 + b;
                                const long long rowoff = (long long)(oy * p.osy + oy_off) * p.o_rstride;
#pragma unroll
                                for (int ps = 0; ps < 2; ++ps) {
                                    const float* src = patch0 + b * (32 * TS) + (ps * 16 + prow8) * TS + pcol8;
                                    const float4 va = *reinterpret_cast<const float4*>(src), vb = *reinterpret_cast<const float4*>(src + 4);
                                    const float bv = bv2[ps];
                                    const float vv[8] = {va.x + bv, va.y + bv, va.z + bv, va.w + bv, vb.x + bv, vb.y + bv, vb.z + bv, vb.w + bv};
                                    if (cok2[ps] && oy < p.OH) {   // (always true here.  Without the lane test the compiler hoists every patch read of the
                                                                   // round -- and this instantiation, 128 accumulators in VGPRs under a 256-register
                                                                   // cap for two workgroups per CU, spills 175 registers: measured, kept as is)
                                        s2[ps] += ((vv[0] + vv[1]) + (vv[2] + vv[3])) + ((vv[4] + vv[5]) + (vv[6] + vv[7]));
                                        q2s[ps] += ((vv[0] * vv[0] + vv[1] * vv[1]) + (vv[2] * vv[2] + vv[3] * vv[3])) +
                                                   ((vv[4] * vv[4] + vv[5] * vv[5]) + (vv[6] * vv[6] + vv[7] * vv[7]));
                                        uint4 pk;
                                        auto pack2 = [&](float a, float b2) {
                                            return (unsigned)__builtin_bit_cast(unsigned short, (__bf16)actf(a)) |
                                                   ((unsigned)__builtin_bit_cast(unsigned short, (__bf16)actf(b2)) << 16);
                                        };
                                        pk.x = pack2(vv[0], vv[1]); pk.y = pack2(vv[2], vv[3]); pk.z = pack2(vv[4], vv[5]); pk.w = pack2(vv[6], vv[7]);
                                        *reinterpret_cast<uint4*>(reinterpret_cast<__bf16*>(p.y) + cb2[ps] + rowoff) = pk;
                                    }
                                }
                            }
                        }
                        if (want_stats) {
#pragma unroll
                            for (int ps = 0; ps < 2; ++ps) {
                                float s = s2[ps], q2 = q2s[ps];
#pragma unroll
                                for (int sh = 1; sh < 4; sh <<= 1) {
                                    s += __shfl_xor(s, sh, 64);
                                    q2 += __shfl_xor(q2, sh, 64);
                                }
                                if ((lane & 3) == 0) {
                                    float* d = sred + ((wpx * CO_TILE) + wco * MT * 32 + m * 32 + ps * 16 + prow8) * 2;
                                    d[0] = s;
                                    d[1] = q2;
                                }
                            }
                        }
                    }
                }
            }
            // ---- fp32 output, the common case as STRAIGHT-LINE code (round 6): whole 32-pixel rows, every cout and every row of the
            // tile inside the tensor, no bias -- wave-uniform, tested once.  The general loop below keeps a lane-divergent
            // `cout valid && row valid` test around every 16-byte group; inside it the compiler waits for each ds_read_b128 of the
            // transposition before it issues the next one: 32 serial LDS round trips + ~130 branches per wave and tile, 14.9 k of
            // the tile's ~150 k cycles WITH OR WITHOUT the global stores (profiles/r06_epilogue_account.md: APAMD_ABLATE=16 removes
            // the stores and the segment stays at 14.9 k) -- the epilogue was bound by its own control flow, not by store issue.
            bool fast32 = false;
            // (not where two workgroups share a CU's registers and the instantiation is already at its 256-register cap: the
            // run-time-tap family and the tall row tile of plain-bf16 arithmetic spilled 230-400 bytes with the extra path --
            // tests/test_isa_cpu.py)
            constexpr bool FAST_OK = !C::OB16 && !(C::WG_PER_CU == 2 && (C::K == 0 || (C::ROW && C::MT == 2)));
            if constexpr (FAST_OK) {
                fast32 = __builtin_amdgcn_readfirstlane((int)(!octet && full && p.bias == nullptr && ACT == 0 && p.osy == 1 &&
                                                              co_base + MT * 32 <= p.Cout && oy0 + C::TH <= p.OH)) != 0;
                if (fast32) {
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
                        float s4[4] = {0.f, 0.f, 0.f, 0.f}, q4[4] = {0.f, 0.f, 0.f, 0.f};
                        float* dst0[4];
#pragma unroll
                        for (int ps = 0; ps < 4; ++ps)
                            dst0[ps] = p.y + (long long)n * p.o_nstride + (long long)(co_base + m * 32 + ps * 8 + prow) * p.o_cstride + oxv +
                                       (long long)(oy0 + wpx * NT + oy_off) * p.o_rstride;
#pragma unroll
                        for (int q0 = 0; q0 < NT; q0 += NP) {
#pragma unroll
                            for (int b = 0; b < NP; ++b)
#pragma unroll
                                for (int r = 0; r < 16; ++r)
                                    patch0[b * (32 * TS) + ((r & 3) + 8 * (r >> 2) + 4 * half) * TS + l32] = acc[m][q0 + b][r];
                            float4 v[NP][4];
#pragma unroll
                            for (int b = 0; b < NP; ++b)
#pragma unroll
                                for (int ps = 0; ps < 4; ++ps)
                                    v[b][ps] = *reinterpret_cast<const float4*>(patch0 + b * (32 * TS) + (ps * 8 + prow) * TS + pcol);
#pragma unroll
                            for (int b = 0; b < NP; ++b)
#pragma unroll
                                for (int ps = 0; ps < 4; ++ps) {
                                    const float4 t = v[b][ps];
                                    s4[ps] += (t.x + t.y) + (t.z + t.w);
                                    q4[ps] += (t.x * t.x + t.y * t.y) + (t.z * t.z + t.w * t.w);
                                    if (!AP_ABLATE(p, 16)) *reinterpret_cast<float4*>(dst0[ps] + (long long)(q0 + b) * p.o_rstride) = t;
                                }
                        }
                        if (want_stats) {
#pragma unroll
                            for (int ps = 0; ps < 4; ++ps) {
                                float s = s4[ps], q2 = q4[ps];
#pragma unroll
                                for (int sh = 1; sh < 8; sh <<= 1) {
                                    s += __shfl_xor(s, sh, 64);
                                    q2 += __shfl_xor(q2, sh, 64);
                                }
                                if ((lane & 7) == 0) {
                                    float* d = sred + ((wpx * CO_TILE) + wco * MT * 32 + m * 32 + ps * 8 + prow) * 2;
                                    d[0] = s;
                                    d[1] = q2;
                                }
                            }
                        }
                    }
                }
            }
            if (!octet && !wide16 && !fast32) {
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                float s4[4] = {0.f, 0.f, 0.f, 0.f}, q4[4] = {0.f, 0.f, 0.f, 0.f};
                float bvv[4];
                long long cbase[4];
                bool cokc[4];
#pragma unroll
                for (int ps = 0; ps < 4; ++ps) {
                    const int co = co_base + m * 32 + ps * 8 + prow;
                    cokc[ps] = co < p.Cout;
                    bvv[ps] = (p.bias != nullptr && cokc[ps]) ? p.bias[co] : 0.f;
                    cbase[ps] = (long long)n * p.o_nstride + (long long)co * p.o_cstride + oxv * p.osx + ox_off;
                }
#pragma unroll
                for (int q0 = 0; q0 < NT; q0 += NP) {
#pragma unroll
                    for (int b = 0; b < NP; ++b)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            patch0[b * (32 * TS) + ((r & 3) + 8 * (r >> 2) + 4 * half) * TS + l32] = acc[m][q0 + b][r];
#pragma unroll
                    for (int b = 0; b < NP; ++b) {
                        const int oy = oy0 + wpx * NT + q0 + b;
                        const long long rowoff = (long long)(oy * p.osy + oy_off) * p.o_rstride;
#pragma unroll
                        for (int ps = 0; ps < 4; ++ps) {
                            const float4 v = *reinterpret_cast<const float4*>(patch0 + b * (32 * TS) + (ps * 8 + prow) * TS + pcol);
                            const float bv = bvv[ps];
                            const float vv[4] = {v.x + bv, v.y + bv, v.z + bv, v.w + bv};
                            if (cokc[ps] && oy < p.OH) {
                                float* dst = p.y + cbase[ps] + rowoff;
                                if constexpr (C::OB16) {
                                    // bf16 output: the same element offsets on a 2-byte element; 8-byte stores of 4 pixels (4-byte
                                    // alignment suffices: the padded rows of a data gradient start at odd pixel pairs)
                                    typedef unsigned u32x2 __attribute__((ext_vector_type(2), aligned(4)));
                                    __bf16* d16 = reinterpret_cast<__bf16*>(p.y) + cbase[ps] + rowoff;
#pragma unroll
                                    for (int j = 0; j < 4; ++j)
                                        if (full || oxv + j < p.OW) { s4[ps] += vv[j]; q4[ps] += vv[j] * vv[j]; }
                                    // (an 8-byte store of four bf16 needs even element strides only: the 66-element rows of a padded
                                    // data gradient qualify, which the 16-byte fp32 form does not) and a 4-byte aligned y
                                    const bool v16 = p.osx == 1 && ((p.o_rstride | (int)p.o_cstride | (int)p.o_nstride | ox_off) & 1) == 0 &&
                                                     (reinterpret_cast<uintptr_t>(p.y) & 3) == 0;
                                    if (v16 && oxv + 3 < p.OW) {
                                        u32x2 pk;
                                        pk[0] = (unsigned)__builtin_bit_cast(unsigned short, (__bf16)actf(vv[0])) |
                                                ((unsigned)__builtin_bit_cast(unsigned short, (__bf16)actf(vv[1])) << 16);
                                        pk[1] = (unsigned)__builtin_bit_cast(unsigned short, (__bf16)actf(vv[2])) |
                                                ((unsigned)__builtin_bit_cast(unsigned short, (__bf16)actf(vv[3])) << 16);
                                        *reinterpret_cast<u32x2*>(d16) = pk;
                                    } else {
#pragma unroll
                                        for (int j = 0; j < 4; ++j)
                                            if (oxv + j < p.OW) d16[j * p.osx] = (__bf16)actf(vv[j]);
                                    }
                                } else if (full) {
                                    s4[ps] += (vv[0] + vv[1]) + (vv[2] + vv[3]);
                                    q4[ps] += (vv[0] * vv[0] + vv[1] * vv[1]) + (vv[2] * vv[2] + vv[3] * vv[3]);
                                    // (experiment build, APAMD_ABLATE bit 16: the epilogue without its global stores -- what is left is
                                    // the LDS transposition + statistics; profiles/r06_epilogue_account.md)
                                    if (!AP_ABLATE(p, 16))
                                    *reinterpret_cast<float4*>(dst) =
                                        make_float4(actf(vv[0]), actf(vv[1]), actf(vv[2]), actf(vv[3]));
                                } else {
#pragma unroll
                                    for (int j = 0; j < 4; ++j)
                                        if (oxv + j < p.OW) { s4[ps] += vv[j]; q4[ps] += vv[j] * vv[j]; }
                                    if (vec_ok && oxv + 3 < p.OW) {
                                        *reinterpret_cast<float4*>(dst) =
                                            make_float4(actf(vv[0]), actf(vv[1]), actf(vv[2]), actf(vv[3]));
                                    } else {
#pragma unroll
                                        for (int j = 0; j < 4; ++j)
                                            if (oxv + j < p.OW) dst[j * p.osx] = actf(vv[j]);
                                    }
                                }
                            }
                        }
                    }
                }
                if (want_stats) {
#pragma unroll
                    for (int ps = 0; ps < 4; ++ps) {
                        float s = s4[ps], q2 = q4[ps];
#pragma unroll
                        for (int sh = 1; sh < 8; sh <<= 1) {
                            s += __shfl_xor(s, sh, 64);
                            q2 += __shfl_xor(q2, sh, 64);
                        }
                        if ((lane & 7) == 0) {
                            float* d = sred + ((wpx * CO_TILE) + wco * MT * 32 + m * 32 + ps * 8 + prow) * 2;
                            d[0] = s;
                            d[1] = q2;
                        }
                    }
                }
            }
            }   // !octet
            AP_STAMP(9, 0);                                        // rows transposed, stored, row sums formed
            if (want_stats) {
                __syncthreads();
                if (tid < CO_TILE) {
                    const int co = cot * CO_TILE + tid;
                    if (co < p.Cout) {
                        float s = 0.f, q2 = 0.f;
#pragma unroll
                        for (int w = 0; w < C::WPX; ++w) {
                            s += sred[(w * CO_TILE + tid) * 2];
                            q2 += sred[(w * CO_TILE + tid) * 2 + 1];
                        }
                        float* d = p.stats + (((long long)n * p.Cout + co) * p.stat_tiles + stat_off +
                                              cur.ty * p.tiles_x + cur.tx) * 2;
                        d[0] = s;
                        d[1] = q2;
                    }
                }
            }
        };
        if (AP_ABLATE(p, 8)) {
            if (acc[0][0][0] == 123.456f) p.y[0] = 1.f;
        } else if (p.act == 0) {
            epilogue(std::integral_constant<int, 0>{});
        } else {
            epilogue(std::integral_constant<int, -1>{});
        }
        AP_STAMP(4, 0);                                            // epilogue done: every output store issued
        if (!has_next) break;
        __syncthreads();                                           // patches and statistics consumed: refill that stage
        AP_STAMP(5, 0);
        if constexpr (DMA_D > 0) {
            // the next tile's chunk 1 is "the refill of stage -1": its first N0 pieces here, the others on the taps of the
            // next tile's stage 0, like every other refill (stage_sync(0) awaits them; stage 1 reads them)
            pend = dma.setup(nxt.n, nxt.cot, 1, pl);
            pdma = __builtin_amdgcn_readfirstlane(AP_ABLATE(p, 1) ? 0 : 1);
#pragma unroll
            for (int k = 0; k < NIT; ++k) pig[k] = ngoff[k];
            static_for<DMA_N0>([&](auto jt) __attribute__((always_inline)) {
                if (pdma) dma.piece(pend, pig, pig, false, jt);
            });
        } else if (!AP_ABLATE(p, 1)) dma.issue(nxt, ngoff, 1, pl);
        AP_STAMP(6, 0);                                            // the next tile's chunk 1 is on its way
#ifdef APAMD_ABLATION
        ++stamp_tile;
#endif
        cur = nxt;
        tmask = tapmask_of(cur);
#pragma unroll
        for (int k = 0; k < NIT; ++k) cgoff[k] = ngoff[k];
        tile += tile_step;
    }
    dma_wait_all();                                                // (the last tile's tail stage staged a chunk nobody reads)
#ifdef APAMD_ABLATION
    if (stamping) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        AP_STAMP(10, 0);                                           // every store acknowledged
        __syncthreads();
        const unsigned* src = reinterpret_cast<const unsigned*>(smem_raw + p.stamp_lds_off);
        for (int i = tid; i < 4 * p.stamp_words; i += 256) p.stamps[(long long)blockIdx.x * 4 * p.stamp_words + i] = src[i];
    }
#endif
#undef AP_STAMP
}

}  // namespace apamd
