// wgrad_bf16x3.h -- the weight gradient of wgrad_igemm.h on the bf16 matrix pipe, at fp32-class accuracy
// (operands split into bf16 head + tail, three MFMAs per product, fp32 accumulation: see conv_bf16x3.h).
//
//   dW[m][ci][ky][kx] = sum_{n, oy, ox} G[n][m][oy][ox] * A[n][ci][oy + ky - pad][ox + kx - pad]        (stride 1)
//
// GEMM view: M = m (32 per wave), N = ci (32 per wave) with one accumulator tile PER TAP, K = pixels: an MFMA's
// 16-deep K step is 16 x-adjacent output pixels, 8 per half-wave.  A lane's operand fragment is therefore 8
// consecutive pixels of one channel -- for the shifted operand, at a column offset of kx pixels.  Both tensors are
// prepared once per layer (wgrad_operand.h: split_transpose_* / xs_transpose_kernel) as pixel-octet slots with the CHANNEL innermost,
//     T[n][head|tail][row][x / 8][channel][8 x bf16],
// so that (a) every LDS-DMA piece is 64 consecutive channels of one octet = 1 KiB contiguous in HBM at a scalar
// address (no per-lane address work at all), (b) fragment reads are conflict-free ds_read_b128 (lane = channel), and
// (c) a tap's fragment is a funnel shift of two neighbouring octets by kx halfwords (v_alignbit; free for even kx).
// The kx / ky shifts are register / row-index arithmetic on ONE staged tile: no im2col, no per-tap copies.
//
// Workgroup = 4 waves = 2 (m) x 2 (ci) -> 64 x 64 channels x K*K taps; one pipeline stage = 2 output rows x 32
// columns of one image (4 K steps); stages of the workgroup's pixel share are double-buffered in LDS with the same
// flat schedule as conv_bf16x3 (stage g+2 issued from inside the last MFMA group of stage g).  The pixel range is
// split over P workgroups per (m, ci) tile; the partial tiles are stored, and summed in a fixed order by wgrad_bf3_reduce_kernel,
// in wgrad_bf3_partial.h.
#pragma once
#include <type_traits>

#include "lds_dma.h"
#include "wgrad_bf3_partial.h"

namespace apamd {

struct WgradBf3Params {
    const uint4* gt;          // [N][2][GHp][GX8][Mp]  slots of 8 pixels
    const uint4* at;          // [N][2][Hp][AX8][Cp]
    int N, M, Cin, Q;         // Q = Cin * K * K
    int GHp, GX8, Mp, Hp, AX8, Cp;
    int tiles_x, tiles_y;     // pixel tiles (2 rows x 32 columns) per image
    int nstages, P;
    int m_tiles, c_tiles;
    float* partial;           // [P][tile][wave][tap][16][64]: wgrad_bf3_partial.h
    int ablate;               // debugging only (APAMD_ABLATE): 1 = no refill of the stage buffers, 2 = no barrier
};

// PARTS_ = 2: head + tail staged, three products per tap.  PARTS_ = 1 (AP_PRECISION_BF16): head planes only -- half the
// LDS stage and LDS-DMA traffic, one product per tap, two workgroups per CU.
// KY_ = 1: the ROW form of a K x K layer on few channels (the 7x7 stems): the shifted operand is prepared with one channel per
// (input channel, kernel row) -- channel ci * K + ky of row y is the padded input row y + ky (split_transpose_kernel, rows_k) --
// so the kernel sees a 1 x K layer over K * Cin channels: K taps, no row shift, and dW[m][ci * K + ky][kx] IS the OIHW tensor.
// WM_ = 4: EIGHT waves, 4 (m) x 2 (ci) -> a 128 x 64 channel tile.  With head + tail staged a 4-wave workgroup fills a CU's LDS, so
// every SIMD holds ONE wave and nothing covers its LDS / MFMA latencies; the 8-wave workgroup stages 1.3x the bytes (the shifted
// operand is shared by twice the products) for 2x the products and puts two waves on every SIMD.
template <int K_, int PARTS_ = 2, int KY_ = K_, int WM_ = 2>
struct WgradBf3Cfg {
    static constexpr int K = K_, KY = KY_, T = K * KY, PR = 2, PARTS = PARTS_, WM = WM_;
    static_assert(WM == 2 || WM == 4, "2 x 2 or 4 x 2 waves");
    static constexpr int NWAVES = 2 * WM, M_TILE = 32 * WM, MH = WM / 2;   // MH: 64-channel DMA pieces per G octet
    static_assert(PARTS == 1 || PARTS == 2, "head only, or head + tail");
    static_assert(KY == K || KY == 1, "square taps, or the row form");
    static constexpr int ROWS = PR + KY - 1;                // staged rows of the shifted operand
    static constexpr int NXG = 5;                           // staged octets per row: 4 + 1 for the column shift
    static constexpr int G_SLOTS = PARTS * PR * 4 * M_TILE; // [part][row][octet][m]
    static constexpr int A_SLOTS = PARTS * ROWS * NXG * 64; // [part][row][octet][ci]
    static constexpr int NPIECE = (G_SLOTS + A_SLOTS) / 64; // 1 KiB DMA pieces per stage
    // the LDS-DMA unit's share-out of a stage (wgrad_bf16x3: issue_piece / issue_piece8)
    static constexpr int NGP = PARTS == 2 ? 4 : 2;          // G pieces per wave and stage
    static constexpr int NAE = ROWS * NXG, NAP = PARTS == 2 ? (NAE + 1) / 2 : (NAE + 3) / 4;   // (row, octet) pairs; per wave
    static constexpr int NGPIECE = PARTS * PR * 4 * MH, NAPIECE = PARTS * ROWS * NXG;          // 8 waves: the stage's G / A piece lists
    static constexpr int NPW = WM == 2 ? NGP + NAP : (NGPIECE + NAPIECE + NWAVES - 1) / NWAVES;   // pieces per wave and stage
    static constexpr size_t lds_bytes() { return (size_t)2 * (G_SLOTS + A_SLOTS) * 16; }
    // one accumulator tile per tap: 16 K^2 registers -- with head-only staging two workgroups share a CU when that
    // leaves room for the operand registers (K <= 3; a 4x4 layer's 256 accumulators need a SIMD's whole file)
    static constexpr int WG_PER_CU = (PARTS == 1 && T * 16 <= 160 && WM == 2) ? 2 : 1;
    static_assert(K - 1 < 8, "the column shift must stay inside one extra octet");
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// 8 consecutive bf16 starting SH elements into the 16-element sequence lo ++ hi
template <int SH>
__device__ __forceinline__ bf16x8 funnel8(const u32x4 lo, const u32x4 hi) {
    unsigned c[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    u32x4 r;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        if constexpr ((SH & 1) == 0) r[d] = c[d + SH / 2];
        else r[d] = __builtin_amdgcn_alignbit(c[d + SH / 2 + 1], c[d + SH / 2], 16);
    }
    return __builtin_bit_cast(bf16x8, r);
}

// PARTS = 2: split-bf16 arithmetic (tail x head, head x tail, head x head per tap).  PARTS = 1: plain bf16 arithmetic
// (AP_PRECISION_BF16): the head x head product only, head planes only.
template <class C>
__global__ __launch_bounds__(C::NWAVES * 64, C::WG_PER_CU) void wgrad_bf16x3(const WgradBf3Params p) {
    constexpr int WM = C::WM, NWAVES = C::NWAVES, M_TILE = C::M_TILE, MH = C::MH;
    constexpr int PARTS = C::PARTS, PROD = PARTS == 1 ? 1 : 3;
    constexpr int K = C::K, KY = C::KY, T = C::T, ROWS = C::ROWS, NXG = C::NXG;
    constexpr int G_SLOTS = C::G_SLOTS, A_SLOTS = C::A_SLOTS, STAGE = G_SLOTS + A_SLOTS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const uint4* const smem = reinterpret_cast<const uint4*>(smem_raw);
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem_raw;

    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, half = lane >> 5, l32 = lane & 31;
    const int wm = wave % WM, wq = wave / WM;
    int b = blockIdx.x;
    const int split = b % p.P; b /= p.P;
    const int ct = b % p.c_tiles;
    const int mt = b / p.c_tiles;
    const int st0 = (int)((long long)p.nstages * split / p.P), st1 = (int)((long long)p.nstages * (split + 1) / p.P);

    // ---- LDS-DMA: piece j of a stage = 64 consecutive channels of one (part, row, octet); this wave issues the
    // pieces j = wave, wave + 4, ...  Source = scalar slot index, + lane.
    // Wave w moves part (w & 1); of that part, G row (w >> 1) (4 octets) and every second (row, octet) pair of the
    // shifted operand -- so a piece's kind is static and only scalar offsets depend on the wave.  The position of
    // the NEXT stage to issue advances incrementally (no divisions in the loop).
    // (Still closures: as WgradBf3Dma<C>, a struct of references into this frame with locate / advance / piece / issue_stage, six of
    // the ten instantiations changed -- WgradBf3Cfg<7,1,1> 2347 -> 2545 instructions and 78 -> 84 SGPRs, <4,1> 3005 -> 3048.)
    const unsigned lane16 = lane * 16;
    // (head-only staging: every wave moves head pieces -- G row (w >> 1), octets 2 (w & 1) and + 1; every fourth
    // (row, octet) pair of the shifted operand)
    const int dpart = PARTS == 2 ? (wave & 1) : 0, dhw = wave >> 1;
    constexpr int NGP = C::NGP, NAE = C::NAE, NPW = C::NPW, NGPIECE = C::NGPIECE, NAPIECE = C::NAPIECE;
    const long long g_row = (long long)p.GX8 * p.Mp, g_part = g_row * p.GHp;
    const long long a_row = (long long)p.AX8 * p.Cp, a_part = a_row * p.Hp;
    int in_ = 0, ity = 0, itx = 0;                                      // (image, tile row, tile column) to issue next
    {
        itx = st0 % p.tiles_x;
        const int t2 = st0 / p.tiles_x;
        ity = t2 % p.tiles_y;
        in_ = t2 / p.tiles_y;
    }
    long long gbase = 0, abase = 0;                                     // slot of (image, this wave's part, tile origin)
    auto locate = [&]() __attribute__((always_inline)) {
        if constexpr (WM == 2) {
            gbase = ((long long)(in_ * 2 + dpart) * p.GHp + ity * C::PR + dhw) * g_row + (long long)(itx * 4) * p.Mp + mt * 64;
            abase = ((long long)(in_ * 2 + dpart) * p.Hp + ity * C::PR) * a_row + (long long)(itx * 4) * p.Cp + ct * 64;
        } else {                                                      // (part 0, row 0 of the tile: the rest per piece)
            gbase = ((long long)(in_ * 2) * p.GHp + ity * C::PR) * g_row + (long long)(itx * 4) * p.Mp + mt * M_TILE;
            abase = ((long long)(in_ * 2) * p.Hp + ity * C::PR) * a_row + (long long)(itx * 4) * p.Cp + ct * 64;
        }
    };
    auto advance = [&]() __attribute__((always_inline)) {
        if (++itx == p.tiles_x) {
            itx = 0;
            if (++ity == p.tiles_y) { ity = 0; ++in_; }
        }
    };
    // 8 waves: piece j of the wave = piece (wave + 8 j) of the stage's list [G: part][row][octet][64-channel half], then
    // [A: part][row][octet]; the decode is scalar arithmetic on the wave index
    auto issue_piece8 = [&](int buf, int i) __attribute__((always_inline)) {
        const int j = wave + NWAVES * i;
        if (j < NGPIECE) {
            const int mh = j % MH, t1 = j / MH, o = t1 % 4, t2 = t1 / 4, row = t2 % C::PR, part = t2 / C::PR;
            glds16_sv(p.gt + gbase + part * g_part + row * g_row + (long long)o * p.Mp + mh * 64, lane16,
                      lds0 + (buf * STAGE + (((part * C::PR + row) * 4 + o) * MH + mh) * 64) * 16);
        } else if (j < NGPIECE + NAPIECE) {
            const int e = j - NGPIECE, o = e % NXG, t1 = e / NXG, r = t1 % ROWS, part = t1 / ROWS;
            glds16_sv(p.at + abase + part * a_part + r * a_row + (long long)o * p.Cp, lane16,
                      lds0 + (buf * STAGE + G_SLOTS + ((part * ROWS + r) * NXG + o) * 64) * 16);
        }
    };
    auto issue_piece = [&](int buf, int j) __attribute__((always_inline)) {   // uses gbase / abase of the located stage
        if constexpr (WM == 4) {
            issue_piece8(buf, j);
        } else if (j < NGP) {
            const int o = PARTS == 2 ? j : 2 * (wave & 1) + j;          // octet of the G row
            glds16_sv(p.gt + gbase + (long long)o * p.Mp, lane16,
                      lds0 + (buf * STAGE + ((dpart * C::PR + dhw) * 4 + o) * 64) * 16);
        } else {
            const int e = PARTS == 2 ? (j - NGP) * 2 + dhw : (j - NGP) * 4 + wave;   // (row, octet) pair of this wave
            if ((PARTS == 2 && (j - NGP) * 2 + 1 < NAE) || e < NAE) {
                const int r = e / NXG, o = e - r * NXG;
                glds16_sv(p.at + abase + r * a_row + (long long)o * p.Cp, lane16,
                          lds0 + (buf * STAGE + G_SLOTS + ((dpart * ROWS + r) * NXG + o) * 64) * 16);
            }
        }
    };
    auto issue_stage = [&](int buf) __attribute__((always_inline)) {    // issues the located stage and moves on
        locate();
#pragma unroll
        for (int j = 0; j < NPW; ++j) issue_piece(buf, j);
        advance();
    };

    f32x16 acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // fragment slots (16 bytes each) relative to a stage buffer
    const int ga = (half) * M_TILE + wm * 32 + l32;                    // + (part*PR*4 + py*4 + xh*2) * M_TILE
    const int ab = G_SLOTS + half * 64 + wq * 32 + l32;                // + ((part*ROWS + row)*NXG + xh*2 + j) * 64

    if (st0 < st1) {
        issue_stage(0);
        if (st0 + 1 < st1) issue_stage(1);
        dma_wait_all();
    }
    __syncthreads();

    // one group = (K step ks, kernel row ky): 4 raw octets of the shifted operand (+ 2 fragments of G at ky == 0),
    // then K taps x 3 MFMAs.  Groups run as a 3-deep software pipeline, flat across stages:
    //     while group g multiplies:  the raw octets of group g+2 are read from LDS,
    //                                the odd-shift operands of group g+1 are funnelled out of ITS raw octets,
    // so every LDS read and every vector-ALU result has a whole group (>= 9 MFMAs) before its first use, and the
    // products go round the K accumulators of the kernel row (consecutive MFMAs never wait on each other).
    // (Still closures: as WgradBf3Frags<C>, a struct of references into this frame with fetch_group / shift_group / mfma_one, the
    // register sets and NG / RB / NGF, five of the ten instantiations changed -- WgradBf3Cfg<2,1> 108 -> 110 VGPRs and 2046 -> 2063
    // instructions, <2,2> 2253 -> 2272, <7,1,1> 2347 -> 2363; the same with the struct naming the LDS symbol itself.)
    constexpr int NG = 4 * KY;
    constexpr int RB = KY == 3 ? 3 : 4;                                // raw-octet register sets (RB divides NG)
    static_assert(NG % RB == 0 && NG % 2 == 0, "register set indices must be stage-invariant");
    // G fragments by ks parity -- in the row form (one group per K step) by group index mod RB, as the raw octets: the fetch of
    // group g + 2 precedes the products of group g in program order
    constexpr int NGF = KY == 1 ? RB : 2;
    bf16x8 ah[NGF], al[NGF];
    u32x4 rh[RB][2], rl[RB][2];                                        // by group index mod RB: [octet j]
    bf16x8 sh[2][K], sl[2][K];                                         // funnelled operands by group parity (odd shifts)
    // live = false: the stage does not exist (the padding stage of an odd count, see the stage loop): its G fragments are
    // forced to zero, so its products are exact zeros whatever finite data the buffer holds
    auto fetch_group = [&](int buf, int gidx, bool live) __attribute__((always_inline)) {
        const int ks = gidx / KY, ky = gidx % KY, rb = gidx % RB;
        const int py = ks >> 1, xh = ks & 1;
        const uint4* S0 = smem + buf * STAGE;
        if (ky == 0) {
            u32x4 th = *reinterpret_cast<const u32x4*>(S0 + ga + ((0 * C::PR + py) * 4 + xh * 2) * M_TILE);
#pragma unroll
            for (int d = 0; d < 4; ++d) th[d] = live ? th[d] : 0u;
            ah[KY == 1 ? rb : (ks & 1)] = __builtin_bit_cast(bf16x8, th);
            if constexpr (PARTS == 2) {
                u32x4 tl = *reinterpret_cast<const u32x4*>(S0 + ga + ((1 * C::PR + py) * 4 + xh * 2) * M_TILE);
#pragma unroll
                for (int d = 0; d < 4; ++d) tl[d] = live ? tl[d] : 0u;
                al[KY == 1 ? rb : (ks & 1)] = __builtin_bit_cast(bf16x8, tl);
            }
        }
        const int row = py + ky;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            rh[rb][j] = *reinterpret_cast<const u32x4*>(S0 + ab + ((0 * ROWS + row) * NXG + xh * 2 + j) * 64);
            if constexpr (PARTS == 2) rl[rb][j] = *reinterpret_cast<const u32x4*>(S0 + ab + ((1 * ROWS + row) * NXG + xh * 2 + j) * 64);
        }
    };
    auto shift_group = [&](int gidx) __attribute__((always_inline)) {  // odd shifts only: even ones are register picks
        const int rb = gidx % RB, pb = gidx & 1;
        sh[pb][1] = funnel8<1>(rh[rb][0], rh[rb][1]);
        if constexpr (PARTS == 2) sl[pb][1] = funnel8<1>(rl[rb][0], rl[rb][1]);
        if constexpr (K > 3) {
            sh[pb][3] = funnel8<3>(rh[rb][0], rh[rb][1]);
            if constexpr (PARTS == 2) sl[pb][3] = funnel8<3>(rl[rb][0], rl[rb][1]);
        }
        if constexpr (K > 5) {
            sh[pb][5] = funnel8<5>(rh[rb][0], rh[rb][1]);
            if constexpr (PARTS == 2) sl[pb][5] = funnel8<5>(rl[rb][0], rl[rb][1]);
        }
    };
    auto mfma_one = [&](int gidx, int i) __attribute__((always_inline)) {
        const int ks = gidx / KY, ky = gidx % KY, rb = gidx % RB, pb = gidx & 1;
        const int pr = PROD == 1 ? 2 : i / K, kx = i % K;               // product-major: round the K accumulators
        bf16x8 bh, bl;
        if (kx == 0) { bh = funnel8<0>(rh[rb][0], rh[rb][1]); if constexpr (PARTS == 2) bl = funnel8<0>(rl[rb][0], rl[rb][1]); }
        else if (kx == 2) { bh = funnel8<2>(rh[rb][0], rh[rb][1]); if constexpr (PARTS == 2) bl = funnel8<2>(rl[rb][0], rl[rb][1]); }
        else if (kx == 4) { bh = funnel8<4>(rh[rb][0], rh[rb][1]); if constexpr (PARTS == 2) bl = funnel8<4>(rl[rb][0], rl[rb][1]); }
        else if (kx == 6) { bh = funnel8<6>(rh[rb][0], rh[rb][1]); if constexpr (PARTS == 2) bl = funnel8<6>(rl[rb][0], rl[rb][1]); }
        else { bh = sh[pb][kx]; if constexpr (PARTS == 2) bl = sl[pb][kx]; }
        f32x16& a = acc[ky * K + kx];
        const int gs = KY == 1 ? rb : (ks & 1);
        a = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pr == 0 ? al[gs] : ah[gs], pr == 1 ? bl : bh, a, 0, 0, 0);
    };

    auto stage = [&](auto ptag, int st) __attribute__((always_inline)) {
        constexpr int P = decltype(ptag)::value;                       // stage buffer
        constexpr int NM = PROD * K, PPS = (NPW + 2 * NM - 1) / (2 * NM);  // DMA pieces per MFMA slot (last two groups)
        const bool live = st < st1, more = st + 1 < st1, dma = st + 2 < st1 && !AP_ABLATE(p, 1);
        if (st == st0) {
            fetch_group(P, 0, true);
            fetch_group(P, 1, true);
            shift_group(0);
        }
        if (!live) {                                                   // (the fragments of its first groups were not fetched)
#pragma unroll
            for (int i = 0; i < NGF; ++i) {
                ah[i] = bf16x8{};
                if constexpr (PARTS == 2) al[i] = bf16x8{};
            }
        }
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
            if (gi == NG - 2) {
                // the reads of this stage's last group were issued one group ago: once everybody is past the
                // barrier the buffer can be refilled (stage st+2), and stage st+1 has landed for the reads below
                if (dma) locate();
                if (!AP_ABLATE(p, 2)) {
                    dma_wait_all();
                    __syncthreads();
                }
            }
            // (no run-time conditions in the steady-state groups: a branch would split the basic block and the
            // compiler's wait-count bookkeeping turns conservative across blocks)
            if (gi + 2 < NG) fetch_group(P, gi + 2, live);
            else if (more) fetch_group(P ^ 1, gi + 2 - NG, true);
            if (gi + 1 < NG) shift_group(gi + 1);
            else if (more) shift_group(0);
#pragma unroll
            for (int i = 0; i < NM; ++i) {
                mfma_one(gi, i);
                if (gi >= NG - 2 && dma) {
#pragma unroll
                    for (int pp = 0; pp < PPS; ++pp) {
                        const int j = ((gi - (NG - 2)) * NM + i) * PPS + pp;
                        if (j < NPW) issue_piece(P, j);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (gi < NG - 2) {
                // pin: the LDS reads go one by one after the first MFMAs (left alone, the scheduler sinks every
                // read to just before its first use and waits on it)
#pragma unroll
                for (int i = 0; i < 6; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (dma) advance();
    };
    // Stages run in PAIRS, both halves unconditionally: with the second stage behind `if (st + 1 < st1)` its MFMAs sat in a
    // conditional block, every accumulator became a phi node and the allocator moved them between AGPRs and VGPRs around it
    // (K = 4: 998 v_accvgpr moves and 128-252 bytes of scratch for 128 MFMAs; round 5).  The padding stage of an odd count
    // multiplies zeroed G fragments with whatever the buffer holds -- which must be FINITE: a workgroup with a single stage never
    // fills buffer 1, so it is cleared here.
    if (st0 + 1 == st1) {
        uint4* z = reinterpret_cast<uint4*>(smem_raw) + STAGE;
        for (int i = tid; i < STAGE; i += NWAVES * 64) z[i] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
    }
    for (int st = st0; st < st1; st += 2) {
        stage(std::integral_constant<int, 0>{}, st);
        stage(std::integral_constant<int, 1>{}, st + 1);
    }

    if (AP_ABLATE(p, 16)) {
        if (acc[0][0] == 123.456f) p.partial[0] = 1.f;
        return;
    }
    wgrad_bf3_store_partial<NWAVES, T>(p.partial, split, p.m_tiles, p.c_tiles, mt, ct, wave, lane, acc);
}

}  // namespace apamd
