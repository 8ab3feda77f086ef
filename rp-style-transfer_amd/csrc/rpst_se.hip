// Squeeze-and-excitation gate of an SEBottleneck in eval mode (reference
// network/attention.py:17-22 inside :56-58): the gate of image n is
//   p    = w3 * mean_h2[n] + b3        conv3 + bn3 folded; the global average pool of a 1x1
//                                      conv's output is the conv of the pooled input, so the
//                                      conv3 output u is never formed
//   z    = relu(fc_a * p)              Linear(C, R), no bias
//   gate = sigmoid(fc_b * z)           Linear(R, C), no bias
// One workgroup of 256 threads per image. Each dot product over channels is taken by one
// wave: lane l adds elements l, l + 64, ... in order, then a butterfly over the lanes, all in
// fp64: a fixed order, no atomics. p and z stay in LDS.
#include "rpst_common.h"

namespace rpst {

constexpr int kSeMaxC = 1024, kSeMaxR = 64;

__global__ __launch_bounds__(256) void se_gate_kernel(const float* __restrict__ mean_h2,
                                                      const float* __restrict__ w3,
                                                      const float* __restrict__ b3,
                                                      const float* __restrict__ fc_a,
                                                      const float* __restrict__ fc_b,
                                                      float* __restrict__ gate, int C, int R) {
  __shared__ double p[kSeMaxC];
  __shared__ double z[kSeMaxR];
  const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* m = mean_h2 + (int64_t)n * C;
  for (int c = wave; c < C; c += 4) {
    const float* w = w3 + (int64_t)c * C;
    double s = 0.0;
    for (int k = lane; k < C; k += 64) s += (double)w[k] * (double)m[k];
    s = wave_sum(s);
    if (lane == 0) p[c] = s + (double)b3[c];
  }
  __syncthreads();
  for (int r = wave; r < R; r += 4) {
    const float* w = fc_a + (int64_t)r * C;
    double s = 0.0;
    for (int k = lane; k < C; k += 64) s += (double)w[k] * p[k];
    s = wave_sum(s);
    if (lane == 0) z[r] = s > 0.0 ? s : 0.0;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    const float* w = fc_b + (int64_t)c * R;
    double s = 0.0;
    for (int r = 0; r < R; ++r) s += (double)w[r] * z[r];
    gate[(int64_t)n * C + c] = (float)(1.0 / (1.0 + exp(-s)));
  }
}

}  // namespace rpst

using namespace rpst;

extern "C" int rpst_se_gate(const float* mean_h2, const float* w3, const float* b3,
                            const float* fc_a, const float* fc_b, float* gate, int N, int C,
                            int R, rpst_stream_t stream) {
  RPST_REQUIRE(mean_h2 && w3 && b3 && fc_a && fc_b && gate, "se_gate: null pointer");
  RPST_REQUIRE(N > 0 && C > 0 && C <= kSeMaxC, "se_gate: need 0 < N and 0 < C <= %d (C=%d)",
               kSeMaxC, C);
  RPST_REQUIRE(R >= 1 && R <= kSeMaxR, "se_gate: need 1 <= R <= %d (R=%d)", kSeMaxR, R);
  se_gate_kernel<<<N, 256, 0, as_stream(stream)>>>(mean_h2, w3, b3, fc_a, fc_b, gate, C, R);
  return launch_status("se_gate_kernel");
}
