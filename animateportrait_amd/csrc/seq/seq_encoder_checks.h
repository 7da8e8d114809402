// Host side of the self-attention encoder calls of libapseq.so that needs no device: their argument checks and the launch plan
// both sides share.  Plain C++ like seq_checks.h, so that a stand-alone program can compile it with the host sanitisers.
#pragma once

#include "seq_checks.h"

namespace apq {

constexpr int kEncRows = APQ_ENC_ROWS;                  // query rows of a workgroup (the N of the 16x16x4 matrix instruction)
constexpr int kEncDk = APQ_ENC_D / APQ_ENC_HEADS;       // 32: width of a head
constexpr int kEncStride = APQ_ENC_D + kPad;            // floats of a 64-wide row in LDS
constexpr int kQkvThreads = 256;                        // 4 waves: 16 output columns of q, k and v each
constexpr int kAttnThreads = 512;                       // 8 waves
constexpr int kAttnWaves = kAttnThreads / 64;
static_assert(kEncRows == kRows, "the tile is the matrix instruction's");
static_assert(APQ_ENC_FF_CHUNK == kAttnWaves * 32, "a wave walks 32 hidden units of a chunk");
static_assert(APQ_ENC_MAX_T % kEncRows == 0 && APQ_ENC_MAX_FF % APQ_ENC_FF_CHUNK == 0, "whole tiles, whole chunks");

struct EncAttnPlan {
    int tiles;           // query tiles of a sequence: ceil(T / 16)
    long long blocks;    // workgroups: B tiles
    int ss;              // floats of a score row in LDS: T rounded up to 16, plus the pad
    int region0;         // floats of the first LDS region: the scores [2][16][ss], later the eight partial outputs [8][16][68]
    size_t lds_bytes;    // region0 and four [16][68] tiles (q, the heads' output, x + attention, Norm_2 of it)
};

inline int enc_score_stride(int T) { return (T + kEncRows - 1) / kEncRows * kEncRows + kPad; }

inline EncAttnPlan enc_attn_plan(int B, int T) {
    EncAttnPlan pl;
    pl.tiles = (T + kEncRows - 1) / kEncRows;
    pl.blocks = (long long)B * pl.tiles;
    pl.ss = enc_score_stride(T);
    const int scores = APQ_ENC_HEADS * kEncRows * pl.ss, partial = kAttnWaves * kEncRows * kEncStride;
    pl.region0 = scores > partial ? scores : partial;
    pl.lds_bytes = (size_t)(pl.region0 + 4 * kEncRows * kEncStride) * sizeof(float);
    return pl;
}

// (the largest plan: what the kernel is allowed to ask for)
constexpr size_t kEncMaxLds = (size_t)(APQ_ENC_HEADS * kEncRows * (APQ_ENC_MAX_T + kPad) + 4 * kEncRows * kEncStride) * sizeof(float);

// "<call>: <message>" into the error buffer; returns `code`
inline int enc_fail(int code, const char* what, const char* fmt, long long a = 0, long long b = 0) {
    char full[192];
    snprintf(full, sizeof full, "%s: %s", what, fmt);
    return fail(code, full, a, b);
}

// B, T and d_model of both calls
inline int check_enc_sizes(const char* what, int B, int T, int d_model) {
    if (B < 1) return enc_fail(APQ_ERR_INVALID, what, "B = %lld (at least 1)", B);
    if (T < 1) return enc_fail(APQ_ERR_INVALID, what, "T = %lld (at least 1)", T);
    if (d_model < 1) return enc_fail(APQ_ERR_INVALID, what, "d_model = %lld (at least 1)", d_model);
    if (d_model != APQ_ENC_D) return enc_fail(APQ_ERR_UNSUPPORTED, what, "d_model = %lld (built for d_model = %lld)", d_model, APQ_ENC_D);
    if (T > APQ_ENC_MAX_T) return enc_fail(APQ_ERR_UNSUPPORTED, what, "T = %lld, served: up to %lld", T, APQ_ENC_MAX_T);
    if (B > APQ_MAX_B) return enc_fail(APQ_ERR_UNSUPPORTED, what, "B = %lld, served: up to %lld", B, APQ_MAX_B);
    if ((long long)B * T * APQ_ENC_D > APQ_MAX_ELEMS)
        return enc_fail(APQ_ERR_UNSUPPORTED, what, "x of B T d_model = %lld elements, served: below 2^31", (long long)B * T * APQ_ENC_D);
    return APQ_OK;
}

struct EncPtr {
    const void* p;
    const char* name;
};

template <int N>
inline int check_enc_pointers(const char* what, const EncPtr (&ptrs)[N]) {
    for (int i = 0; i < N; ++i)
        if (!ptrs[i].p) {
            snprintf(err_buf(), 256, "%s: null %s", what, ptrs[i].name);
            return APQ_ERR_INVALID;
        }
    return APQ_OK;
}

// every tensor of both calls is moved 128 bits at a time
template <int N>
inline int check_enc_alignment(const char* what, const EncPtr (&ptrs)[N]) {
    for (int i = 0; i < N; ++i)
        if (ptrs[i].p && misaligned(ptrs[i].p, APQ_ALIGN_WIDE)) {
            snprintf(err_buf(), 256, "%s: %s is not %d-byte aligned", what, ptrs[i].name, APQ_ALIGN_WIDE);
            return APQ_ERR_UNSUPPORTED;
        }
    return APQ_OK;
}

inline int check_enc_qkv(const void* x, const void* alpha, const void* bias, const void* wq, const void* bq, const void* wk,
                         const void* bk, const void* wv, const void* bv, const void* q, const void* k, const void* v, int B, int T,
                         int d_model) {
    const char* what = "enc_qkv";
    const EncPtr ptrs[] = {{x, "x"}, {alpha, "alpha"}, {bias, "bias"}, {wq, "wq"}, {bq, "bq"}, {wk, "wk"},
                           {bk, "bk"}, {wv, "wv"}, {bv, "bv"}, {q, "q"}, {k, "k"}, {v, "v"}};
    int rc = check_enc_pointers(what, ptrs);
    if (rc != APQ_OK) return rc;
    rc = check_enc_sizes(what, B, T, d_model);
    if (rc != APQ_OK) return rc;
    return check_enc_alignment(what, ptrs);
}

inline int check_enc_attn_ff(const void* x, const void* q, const void* k, const void* v, const void* wo, const void* bo,
                             const void* alpha2, const void* bias2, const void* w1, const void* b1, const void* w2, const void* b2,
                             const void* alpha_f, const void* bias_f, const void* y, int B, int T, int d_model, int heads, int d_ff,
                             EncAttnPlan* pl) {
    const char* what = "enc_attn_ff";
    const EncPtr ptrs[] = {{x, "x"}, {q, "q"}, {k, "k"}, {v, "v"}, {wo, "wo"}, {bo, "bo"}, {alpha2, "alpha2"},
                           {bias2, "bias2"}, {w1, "w1"}, {b1, "b1"}, {w2, "w2"}, {b2, "b2"}, {y, "y"}};
    const EncPtr last[] = {{alpha_f, "alpha_f"}, {bias_f, "bias_f"}};
    int rc = check_enc_pointers(what, ptrs);
    if (rc != APQ_OK) return rc;
    if ((alpha_f == nullptr) != (bias_f == nullptr))
        return fail(APQ_ERR_INVALID, "enc_attn_ff: alpha_f and bias_f: both or neither (the closing Norm)");
    rc = check_enc_sizes(what, B, T, d_model);
    if (rc != APQ_OK) return rc;
    if (heads < 1) return fail(APQ_ERR_INVALID, "enc_attn_ff: heads = %lld (at least 1)", heads);
    if (d_ff < 1) return fail(APQ_ERR_INVALID, "enc_attn_ff: d_ff = %lld (at least 1)", d_ff);
    if (heads != APQ_ENC_HEADS) return fail(APQ_ERR_UNSUPPORTED, "enc_attn_ff: heads = %lld (built for heads = %lld)", heads, APQ_ENC_HEADS);
    if (d_ff % APQ_ENC_FF_CHUNK != 0)
        return fail(APQ_ERR_UNSUPPORTED, "enc_attn_ff: d_ff = %lld, served: multiples of %lld", d_ff, APQ_ENC_FF_CHUNK);
    if (d_ff > APQ_ENC_MAX_FF) return fail(APQ_ERR_UNSUPPORTED, "enc_attn_ff: d_ff = %lld, served: up to %lld", d_ff, APQ_ENC_MAX_FF);
    rc = check_enc_alignment(what, ptrs);
    if (rc != APQ_OK) return rc;
    rc = check_enc_alignment(what, last);
    if (rc != APQ_OK) return rc;
    *pl = enc_attn_plan(B, T);
    return APQ_OK;
}

}  // namespace apq
