// conv_tapgemm_bf16x3 instantiation: the 64 -> 1 channel 7x7 output layer as a tap GEMM + shift-add (see conv_tapgemm.h)
#include "conv_tapgemm.h"
namespace apamd {
const void* tapgemm_kernel() { return reinterpret_cast<const void*>(&conv_tapgemm_bf16x3<TapGemmCfg>); }
}  // namespace apamd
