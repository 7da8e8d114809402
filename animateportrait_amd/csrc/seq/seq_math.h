// The gate non-linearities of libapseq.so: the formulas of csrc/lstm.hip (libapamd.so), so that both LSTM kernels of the
// project round alike.
#pragma once

#include <hip/hip_runtime.h>

namespace apq {

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }
__device__ __forceinline__ float tanhf_(float x) {
    // (exp-based, accurate to ~1e-7 relative over the range that matters; saturates cleanly)
    const float e = __expf(-2.f * fabsf(x));
    const float t = (1.f - e) / (1.f + e);
    return x < 0.f ? -t : t;
}

}  // namespace apq
