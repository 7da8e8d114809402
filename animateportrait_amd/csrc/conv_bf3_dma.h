// conv_bf3_dma.h -- conv_bf16x3's LDS-DMA: where a tile's pieces come from (locate, over the kernel's pgeo), the scalar addresses
// of a stage (Bf3DmaCtx, setup), the issue of one piece or of a whole stage, and the schedule that spreads a stage's pieces over
// the following stage's taps (bf3_dma_sched).  Included by conv_bf16x3.h behind Bf3Tile.
// Reads: ConvKParams (tile counts, window origin, padding, segments, packed weights), wave, and the kernel's pgeo / woff.
// Writes: the two LDS stage buffers (through the DMA) and the tile / offsets `locate` is handed.  The refill in flight (the
// kernel's pend / pig / pdma) belongs to `stage` and the tile hand-over.  It never reads LDS and owns no fragment or accumulator.
#pragma once
#include "conv_igemm.h"
#include "lds_dma.h"

namespace apamd {

// Where the NPIECE LDS-DMA pieces of chunk c+2 are issued.  Their target, the buffer of stage c, is free from stage c's barrier
// on, and they only have to have landed at the barrier of stage c+1: the window is the last tap of stage c (NM MFMA slots) plus
// the taps of stage c+1 that leave two whole taps in front of that barrier.  D = the largest distance (in MFMA slots) at which
// one piece per D slots still fits the window; piece j < N0 goes behind slot (j + 1) * D - 1 of the last tap of stage c, piece
// N0 + t * PPT + k behind slot (k + 1) * D - 1 of tap t <= LAST_ISSUE_TAP of stage c+1.
// D == 0: no window (fewer than four taps per stage, or not enabled) -- every piece in the last tap of stage c.
struct Bf3DmaSched {
    int D, LAST_ISSUE_TAP, PPT, N0;
};
constexpr Bf3DmaSched bf3_dma_sched(bool enabled, int npiece, int nm, int nreal) {
    const int taps = nreal - 3;                                    // taps of stage c+1 that may carry pieces
    if (enabled && taps >= 1)
        for (int d = nm; d >= 1; --d) {
            const int ppt = nm / d;
            if ((taps + 1) * ppt >= npiece) {
                const int n0 = ppt < npiece ? ppt : npiece;
                return {d, (npiece - n0 + ppt - 1) / ppt - 1, ppt, n0};
            }
        }
    return {0, -1, 0, npiece};
}

// ---- LDS-DMA of one stage = NPIECE wave-wide 1 KiB pieces per wave: 2 * NIT activation pieces (head, tail) and
// the wave's share of the weight image.  Bf3DmaCtx holds the scalar part of the addresses.
// A piece is {s_mov m0; global_load_lds v_off, s[base]}: the per-lane 32-bit byte offsets are constants of the
// tile (goff) or of the kernel (woff), everything that changes per stage is scalar -- so a piece costs no
// vector ALU work and slots between two MFMAs of the stage's last tap.
struct Bf3DmaCtx {
    const unsigned char* xh;   // the chunk's first head plane of image n (scalar)
    const unsigned char* xl;   // ... and tail plane
    const unsigned char* wsrc; // the (cout tile, chunk) weight block (scalar)
    unsigned xdst, wdst;       // LDS byte addresses of the stage's activation / weight images (this wave's lane 0)
    unsigned wmask;            // S2D3: taps of the chunk's input phase -- the weight pieces of the others are not staged (the
                               // stage never reads them).  With the fragment reads of absent taps gone the kernel is bound by
                               // the LDS-DMA (1.15 MB per CU against 27 k MFMA cycles, profiles/r04p_pmc_*): 19 % fewer bytes
};

template <class C>
struct Bf3Dma {
    static constexpr int S = C::S, T = C::TMAX, PARTS = C::PARTS, IW = C::IW, PLANE = C::PLANE, NIT = C::NIT, CO_TILE = C::CO_TILE,
                         XP = C::XP;
    static constexpr int W_SLOTS = PARTS * T * 2 * CO_TILE;
    static constexpr int STAGE = W_SLOTS + C::X_SLOTS;             // stage b = smem + b * STAGE: [W_SLOTS weights | X_SLOTS activations]
    static constexpr int NWP = (W_SLOTS / 64 + 3) / 4, NPIECE = PARTS * NIT + NWP;
    // ---- the issue schedule (bf3_dma_sched) and the state a stage hands to the next one: the pieces N0 .. NPIECE-1 of the chunk
    // it staged are issued during the next stage's taps 0 .. LAST_ISSUE_TAP, from the SAME pinned scalars and per-lane offsets
    // (no select, no address arithmetic between those pieces and the MFMAs), under the same scalar flag.
    static constexpr int NM_STAGE = (PARTS == 2 ? 3 : 1) * C::MT * C::NT;       // MFMA slots of a tap
    static constexpr Bf3DmaSched SCHED = bf3_dma_sched(C::DMA_SPREAD, NPIECE, NM_STAGE, T);
    static constexpr int DMA_D = SCHED.D, LAST_ISSUE_TAP = SCHED.LAST_ISSUE_TAP, DMA_PPT = SCHED.PPT, DMA_N0 = SCHED.N0;

    const ConvKParams& p;
    // (every member a reference into the kernel's frame, as the lambdas these were captured it: the optimiser may hoist a read of
    // a by-value member where it could not hoist the read through a reference, and forms other code)
    const int& wave;           // scalar
    const int &H, &W, &HW;
    const int& nchunks;        // even: the host pads an odd count with one all-zero weight chunk
    const int& nreal;          // chunks that exist in the sources
    const unsigned& lds0;      // LDS byte address of stage buffer 0
    int (&pgeo)[NIT];          // (k-group << 15) | (ly << 8) | lx of the piece, or -1 beyond the tile
    unsigned (&woff)[NWP];     // byte offset of this lane's slot in weight piece j
    // The refill in flight, set by `stage` and the tile hand-over in the kernel; no member function touches these three.  They
    // are listed because without them three run-time-tap instantiations (Bf3Cfg<1,0,1,2,4,4,1,0,2,0,0>, <1,0,1,2,4,4,4,0,1,0,0>,
    // <1,0,1,2,4,4,4,0,2,0,0>) come out with other register numbers (tools/kernel_isa_diff.py).
    Bf3DmaCtx& pend;           // its scalars,
    int (&pig)[NIT];           // ... its per-lane offsets,
    int& pdma;                 // ... and whether it is issued at all (scalar)

    // tile number -> (image, cout tile, tile row, tile column) and the source byte offset of every piece of this thread
    __device__ __forceinline__ void locate(int logical, Bf3Tile& t, int (&goff)[NIT]) const {
        t.cot = logical % p.co_tiles;
        int t_ = logical / p.co_tiles;
        t.tx = t_ % p.tiles_x;
        t_ /= p.tiles_x;
        t.ty = t_ % p.tiles_y;
        t.n = t_ / p.tiles_y;
        int dy0 = p.dy0, dx0 = p.dx0;
        if (p.nphase > 1) {                                    // fused sub-pixel phases: the phase sets the window origin
            const int ph = t.cot / p.co_tiles_phase;
            dy0 = p.ph_dy0[ph];
            dx0 = p.ph_dx0[ph];
        }
        const int iy0 = t.ty * C::TH * S + dy0, ix0 = t.tx * 32 * S + dx0;
#pragma unroll
        for (int k = 0; k < NIT; ++k) {
            int gy = iy0 + ((pgeo[k] >> 8) & 127), gx = ix0 + (pgeo[k] & 255);
            bool ok = pgeo[k] >= 0;
            if (p.pad_mode == 1) {
                gy = reflect_clamp(gy, H);
                gx = reflect_clamp(gx, W);
            } else {
                ok = ok && gy >= 0 && gy < H && gx >= 0 && gx < W;
            }
            // byte offset from the chunk's first channel-group plane; out-of-image pixels read that plane's zero slot
            goff[k] = (ok ? ((pgeo[k] >> 15) & 1) * (HW + 1) + gy * W + gx : HW) * 16;
        }
    }
    __device__ int seg_of(int chunk) const {
        int s = 0;
        if (p.nseg > 1 && chunk >= p.seg[1].chunk_begin) s = 1;
        if (p.nseg > 2 && chunk >= p.seg[2].chunk_begin) s = 2;
        return s;
    }
    // The scalar part of a stage's addresses, computed ONCE per stage and pinned in SGPRs (the empty asm): left to itself the
    // compiler re-derived the 64-bit plane address in front of every piece (ten scalar multiplies / adds per piece).
    // The padding chunk of an odd count (chunk_ >= nreal: its weights are all zero) stages the last real chunk's activations
    // again -- finite data, so the products are exact zeros -- instead of skipping its pieces under a per-piece branch.
    __device__ __forceinline__ Bf3DmaCtx setup(int n, int cot, int chunk_, int buf) const {
        const int chunk = chunk_ < nreal ? chunk_ : nreal - 1;
        const int s = seg_of(chunk);
        const int cg0 = (chunk - p.seg[s].chunk_begin) * 2;          // first channel group of the chunk
        const int CG = p.seg[s].C >> 3;
        const unsigned char* xs = reinterpret_cast<const unsigned char*>(p.seg[s].data);
        const unsigned char* xh = xs + ((long long)(n * 2 + 0) * CG + cg0) * (HW + 1) * 16;
        const unsigned char* xl = xs + ((long long)(n * 2 + 1) * CG + cg0) * (HW + 1) * 16;
        unsigned xdst = lds0 + (buf * STAGE + W_SLOTS + wave * 64) * 16;
        const unsigned char* wsrc = reinterpret_cast<const unsigned char*>(p.wp + ((long long)cot * nchunks + chunk_) * p.wfloats);
        unsigned wdst = lds0 + (buf * STAGE + wave * 64) * 16;
        unsigned wmask = 0xFu;
        if constexpr (C::S2D3) wmask = p.s2d_mask[chunk_ / p.s2d_div < 3 ? chunk_ / p.s2d_div : 3];
        asm volatile("" : "+s"(xh), "+s"(xl), "+s"(wsrc), "+s"(xdst), "+s"(wdst));
        return Bf3DmaCtx{xh, xl, wsrc, xdst, wdst, wmask};
    }
    // piece j (a compile-time index): {s_add m0; global_load_lds v_off, s[base]} -- nothing else
    // (alt / use_alt: the tile's tail stage takes the NEXT tile's offsets; selected here, per piece, on registers -- a
    // selected copy of the array was kept in scratch memory)
    template <class JT>
    __device__ __forceinline__ void piece(const Bf3DmaCtx& d, const int (&goff)[NIT], const int (&alt)[NIT], bool use_alt, JT) const {
        constexpr int j = JT::value;
        if constexpr (j < PARTS * NIT) {
            constexpr int part = j / NIT, k = j % NIT;
            constexpr bool whole = k * 256 + 3 * 64 < XP;           // every wave's slice of the piece lies inside the part
            if (whole || k * 256 + wave * 64 < XP)                  // (wave-uniform)
                glds16_si<(part * XP + k * 256) * 16>(part ? d.xl : d.xh, (unsigned)(use_alt ? alt[k] : goff[k]), d.xdst);
        } else {
            constexpr int jj = j - PARTS * NIT;
            constexpr bool whole = jj * 4 + 3 < W_SLOTS / 64;
            bool want = whole || jj * 4 + wave < W_SLOTS / 64;
            // weight image [part][tap][k-group][CO_TILE] in 64-slot pieces: piece -> tap (wave-uniform)
            if constexpr (C::S2D3) want = want && ((d.wmask >> (((jj * 4 + wave) % (T * 2 * CO_TILE / 64)) / (2 * CO_TILE / 64))) & 1u);
            if (want) glds16_si<jj * 4096>(d.wsrc, woff[jj], d.wdst);
        }
    }
    // a whole stage at once: chunk chunk_ of tile t into stage buffer buf
    __device__ __forceinline__ void issue(const Bf3Tile& t, const int (&goff)[NIT], int chunk_, int buf) const {
        const Bf3DmaCtx d = setup(t.n, t.cot, chunk_, buf);
        static_for<NPIECE>([&](auto jt) __attribute__((always_inline)) { piece(d, goff, goff, false, jt); });
    }
};

}  // namespace apamd
