// Shared by the backward translation units (rpst_train.hip, rpst_conv7_train.hip): the
// fixed-order split-K reduction of the weight-gradient kernels.
#pragma once

#include "rpst_common.h"

namespace rpst {

// dw[i] = sum over splits of part[k][i], in split order. Internal linkage: the library is
// built without relocatable device code, so every translation unit that launches it carries
// its own copy.
static __global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part,
                                                                  float* __restrict__ dw,
                                                                  int64_t n, int splits) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  // 8 independent loads in flight, summed in split order
  float s = 0.f;
  int k = 0;
  for (; k + 8 <= splits; k += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(int64_t)(k + u) * n + i];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; k < splits; ++k) s += part[(int64_t)k * n + i];
  dw[i] = s;
}

}  // namespace rpst
