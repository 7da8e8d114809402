// switches.h -- every environment variable the core library (csrc/*.hip, csrc/*.h) reads at run time, and their one reader.
//
// One parse rule (ops.py: _switch applies the same one): unset, empty, not a number or 0 means the row's default, any other
// integer means that value.  A switch is read on every call that asks for it -- tests and A/B runs flip them inside one process --
// unless its row says otherwise.
//
// Kinds (ap_switch_names lists the names of one):
//   ROUTE       read by a route decision: make_plan, make_wgrad_plan, the xs predicates, ap_instnorm_bwd_split_ok, the warp routes
//   TUNING      tile shapes and workgroup counts of a route that is already chosen
//   BUILD_ONLY  rows that exist only in an experiment build (`make ablate`: -DAPAMD_ABLATION, `make variants`: -DAPAMD_VARIANTS)
// ops.backward_switches() keys every cached route decision with the ROUTE and TUNING rows: a new switch needs its row, nothing else.
#pragma once
#include <cstdlib>
#include <cstring>

#ifdef APAMD_ABLATION
#define APAMD_SWITCHES_ABLATION(X)                                                                                                 \
    X(ABLATE, "APAMD_ABLATE", 0, BUILD_ONLY, "bits: skip the DMA refill / barriers / MFMAs / epilogue of the matrix kernels")     \
    X(STAMP_BUF, "APAMD_STAMP_BUF", 0, BUILD_ONLY, "an ADDRESS, not an integer (sw_text): the device stamp buffer of the cycle account") \
    X(STAMP_WORDS, "APAMD_STAMP_WORDS", 512, BUILD_ONLY, "dwords per wave in the stamp buffer")
#else
#define APAMD_SWITCHES_ABLATION(X)
#endif
#ifdef APAMD_VARIANTS
#define APAMD_SWITCHES_VARIANTS(X)                                                                                                 \
    X(CONV_SB, "APAMD_CONV_SB", 0, BUILD_ONLY, "the single-stage two-per-CU form of the 64-cout 3x3 stride-1 kernel")             \
    X(CONV_SB_SKEW, "APAMD_CONV_SB_SKEW", 0, BUILD_ONLY, "start delay of the second half of that kernel's grid")
#else
#define APAMD_SWITCHES_VARIANTS(X)
#endif

// X(id, variable, default, kind, meaning)
#define APAMD_SWITCHES(X)                                                                                                          \
    X(NO_BF16X3, "APAMD_NO_BF16X3", 0, ROUTE, "plan every layer on the fp32 kernels although the descriptor allows split-bf16")   \
    X(NO_SMALL, "APAMD_NO_SMALL", 0, ROUTE, "the landmark encoder's narrow 3x3 layers off their vector-ALU kernel")               \
    X(NO_SMALL_TILES, "APAMD_NO_SMALL_TILES", 0, ROUTE, "never pick the short 3x3 tile at small batch")                           \
    X(NO_S2D_WGRAD, "APAMD_NO_S2D_WGRAD", 0, ROUTE, "stride-2 weight gradients off the space-to-depth form")                      \
    X(ROWS_WGRAD, "APAMD_ROWS_WGRAD", 0, ROUTE, "opt in to the row form of the 7x7 stems' weight gradients (plain bf16)")         \
    X(NO_XS_WGRAD, "APAMD_NO_XS_WGRAD", 0, ROUTE, "the planner refuses the forward split copies as the shifted operand")          \
    X(NO_XS_DIRECT, "APAMD_NO_XS_DIRECT", 0, ROUTE, "the planner refuses ap_conv2d_wgrad_xs (both operands as split copies)")     \
    X(NO_INBWD_SPLIT, "APAMD_NO_INBWD_SPLIT", 0, ROUTE, "ap_instnorm_bwd_split_ok answers 0")                                     \
    X(WARP_BWD_PLAIN, "APAMD_WARP_BWD_PLAIN", 0, ROUTE, "tap-by-tap scatter in the warp backward (kept for comparison)")          \
    X(WARP_GATHER, "APAMD_WARP_GATHER", 0, ROUTE, "a WORD, not an integer (sw_is): quad = the quad-cooperative forward gather")   \
    X(BF3_BLOCKS, "APAMD_BF3_BLOCKS", 0, TUNING, "persistent workgroups of a split-bf16 convolution; notice on stderr")           \
    X(WGRAD_BLOCKS, "APAMD_WGRAD_BLOCKS", 0, TUNING, "workgroup target of a weight-gradient family; notice on stderr")            \
    X(CONV_COTILE, "APAMD_CONV_COTILE", 0, TUNING, "cout tile of the fp32 implicit-GEMM kernel (default: by Cout)")               \
    X(CONV_CI, "APAMD_CONV_CI", 0, TUNING, "channel chunk of the fp32 implicit-GEMM kernel (default: by segments and LDS)")       \
    X(CONV_LDS_TARGET, "APAMD_CONV_LDS_TARGET", 72 * 1024, TUNING, "LDS bytes per workgroup the channel chunk shrinks to")        \
    X(WARP_TILE, "APAMD_WARP_TILE", 5, TUNING, "READ ONCE PER PROCESS: log2 tile width of the forward warp, 4 / 5 / 6; else rows") \
    APAMD_SWITCHES_ABLATION(X)                                                                                                     \
    APAMD_SWITCHES_VARIANTS(X)

namespace apamd {
enum SwitchKind { SWK_ROUTE = 0, SWK_TUNING = 1, SWK_BUILD_ONLY = 2 };
enum Switch {
#define X(id, name, dflt, kind, meaning) SW_##id,
    APAMD_SWITCHES(X)
#undef X
    SW_COUNT
};
struct SwitchRow {
    const char* name;
    int dflt;
    SwitchKind kind;
};
inline const SwitchRow& switch_row(int s) {
    static const SwitchRow rows[] = {
#define X(id, name, dflt, kind, meaning) {name, dflt, SWK_##kind},
        APAMD_SWITCHES(X)
#undef X
    };
    return rows[s];
}
// the variable's text, or null: the only getenv of the core library
inline const char* sw_text(Switch s) { return getenv(switch_row(s).name); }
inline int sw(Switch s) {
    const char* t = sw_text(s);
    const int v = t ? atoi(t) : 0;
    return v ? v : switch_row(s).dflt;
}
inline bool sw_is(Switch s, const char* word) {
    const char* t = sw_text(s);
    return t && !strcmp(t, word);
}
}  // namespace apamd
