// Segmentation-masked AdaIN (inference only).
//
//   compute_label_info                            network/base.py:421-439
//   adaptive_instance_normalization_with_segment  network/base.py:494-530
//
// For one image pair: every label l of the content map that passes the validity rule gets
// its own per-channel statistics, taken over the pixels labelled l in the content and in the
// style feature; content pixels with a valid label become (x - mean_c[l]) / std_c[l] *
// std_s[l] + mean_s[l], every other pixel is copied.
//
// Layout: NCHW fp32, one (n,c) plane = HW contiguous floats; label maps uint8 (N, HW).
// Three stream-ordered steps, none of which synchronises or reads anything back:
//   plan    one workgroup per image: LDS histograms of both maps (integer atomics, so the
//           order does not matter), the validity rule on the device-side counts.
//   params  per (n, c, split): shifted fp64 sum / sum-of-squares per label over a slice of
//           the content plane, then of the style plane. Masks are piecewise constant, so a
//           lane keeps (label, sum, sumsq) of its current run in registers and hands it over
//           only when its label changes. The hand-over is a wave reduction in a fixed order
//           into that wave's own LDS bin: no floating-point atomic anywhere, results are
//           run-to-run bit-identical. A plane is split over several workgroups (few, large
//           planes); a second kernel adds the partials in split order, forms the variance in
//           fp64, rounds it to fp32 and adds eps / takes sqrt in fp32 as torch does.
//   apply   elementwise with 16-B loads / stores and one 32-bit label load per float4; the
//           plane's 256 parameter rows sit in LDS. Contraction off (separate sub / div / mul
//           / add roundings, as plane_apply_kernel). Pass-through pixels are copied.
#include "rpst_common.h"

namespace rpst {

constexpr int kLabels = 256;
constexpr int kPlanThreads = 1024;
constexpr int kSegThreads = 256;
constexpr int kSegWaves = kSegThreads / kWave;
static_assert(kSegThreads == kLabels, "one thread per label bin");
constexpr int kMaxSplits = 16;
constexpr int kApplyElems = 16384;  // elements per apply workgroup

// plan entry: int32 x 4 per (image, label)
constexpr int kPlanC = 0;      // pixels with this label in the content map
constexpr int kPlanS = 1;      // ... in the style map
constexpr int kPlanValid = 2;  // 1 if the label is transformed
constexpr int kPlanStride = 4;

// A row whose std_c is negative is pass-through (a real std_c is a square root).
constexpr float kPassThrough = -1.0f;

// Workgroups per plane. A function of C alone, so an image's result does not depend on the
// batch it is in (the split decides the order of the additions).
__host__ __device__ inline int masked_splits(int C) {
  const int s = (512 + C - 1) / C;
  return s < 1 ? 1 : (s > kMaxSplits ? kMaxSplits : s);
}

// ---- plan -------------------------------------------------------------------------------
// Histogram of one label map into hist[256] (LDS). Each lane counts the run it is in and
// adds it to the bin only when its label changes.
__device__ __forceinline__ void histogram(const uint8_t* __restrict__ seg, int64_t HW,
                                          int* hist) {
  int cur = -1, cnt = 0;
  auto feed = [&](int lab) {
    if (lab != cur) {
      if (cnt) atomicAdd(&hist[cur], cnt);
      cur = lab;
      cnt = 0;
    }
    ++cnt;
  };
  if ((HW & 3) == 0 && (reinterpret_cast<uintptr_t>(seg) & 3) == 0) {
    const uint32_t* __restrict__ s4 = reinterpret_cast<const uint32_t*>(seg);
    for (int64_t i = threadIdx.x; i < (HW >> 2); i += kPlanThreads) {
      const uint32_t w = s4[i];
      feed(w & 255);
      feed((w >> 8) & 255);
      feed((w >> 16) & 255);
      feed(w >> 24);
    }
  } else {
    for (int64_t i = threadIdx.x; i < HW; i += kPlanThreads) feed(seg[i]);
  }
  if (cnt) atomicAdd(&hist[cur], cnt);
}

__global__ __launch_bounds__(kPlanThreads) void segment_plan_kernel(
    const uint8_t* __restrict__ c_seg, const uint8_t* __restrict__ s_seg, int64_t HWc,
    int64_t HWs, int* __restrict__ plan) {
  __shared__ int hist[2][kLabels];
  const int n = blockIdx.x, tid = threadIdx.x;
  if (tid < 2 * kLabels) (&hist[0][0])[tid] = 0;
  __syncthreads();
  histogram(c_seg + (int64_t)n * HWc, HWc, hist[0]);
  histogram(s_seg + (int64_t)n * HWs, HWs, hist[1]);
  __syncthreads();
  if (tid < kLabels) {
    const int64_t c = hist[0][tid], s = hist[1][tid];
    // c / s < 100 and s / c < 100 in integers (both counts are positive here)
    const bool valid = c > 10 && s > 10 && c < 100 * s && s < 100 * c;
    int* e = plan + ((int64_t)n * kLabels + tid) * kPlanStride;
    e[kPlanC] = (int)c;
    e[kPlanS] = (int)s;
    e[kPlanValid] = valid ? 1 : 0;
    e[3] = 0;
  }
}

// ---- params -----------------------------------------------------------------------------
struct Run {
  int label;  // -1: no run yet
  double s1, s2;
};

// Hand every lane's run whose `pend` is set to this wave's bins: one label at a time (lowest
// pending lane first), a fixed-order wave reduction, one writer. Wave-uniform control flow.
__device__ __forceinline__ void flush_runs(const Run& r, bool pend, double* bins) {
  unsigned long long m = __ballot(pend);
  while (m) {
    const int src = __ffsll((long long)m) - 1;
    const int L = __shfl(r.label, src, kWave);
    const bool mine = pend && r.label == L;
    const double a = wave_sum(mine ? r.s1 : 0.0);
    const double b = wave_sum(mine ? r.s2 : 0.0);
    if ((threadIdx.x & (kWave - 1)) == 0) {
      bins[2 * L] += a;
      bins[2 * L + 1] += b;
    }
    m &= ~__ballot(mine);
  }
}

// One element per lane (inactive lanes carry nothing); every lane of the wave calls it.
__device__ __forceinline__ void feed(Run& r, bool active, int lab, float v, float shift,
                                     double* bins) {
  const bool change = active && lab != r.label;
  flush_runs(r, change && r.label >= 0, bins);
  if (change) {
    r.label = lab;
    r.s1 = 0.0;
    r.s2 = 0.0;
  }
  if (active) {
    const double d = (double)v - shift;
    r.s1 += d;
    r.s2 += d * d;
  }
}

// Sums of slice `split` of one plane into this wave's bins.
__device__ __forceinline__ void plane_label_sums(const float* __restrict__ x,
                                                 const uint8_t* __restrict__ seg, int64_t HW,
                                                 int split, int splits, double* bins) {
  const float shift = x[0];
  const int tid = threadIdx.x;
  Run r{-1, 0.0, 0.0};
  const bool vec = (HW & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(seg) & 3) == 0;
  if (vec) {
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
    const uint32_t* __restrict__ s4 = reinterpret_cast<const uint32_t*>(seg);
    const int64_t n4 = HW >> 2;
    const int64_t per = (n4 + splits - 1) / splits;
    const int64_t lo = (int64_t)split * per;
    const int64_t hi = lo + per < n4 ? lo + per : n4;
    for (int64_t base = lo; base < hi; base += kSegThreads) {  // uniform trip count
      const int64_t i = base + tid;
      const bool active = i < hi;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      uint32_t w = 0;
      if (active) {
        v = x4[i];
        w = s4[i];
      }
      const bool same = !active || (r.label >= 0 && w == (uint32_t)r.label * 0x01010101u);
      if (__ballot(!same) == 0) {  // every lane stays in its run
        if (active) {
          const double a = (double)v.x - shift, b = (double)v.y - shift;
          const double c = (double)v.z - shift, d = (double)v.w - shift;
          r.s1 += (a + b) + (c + d);
          r.s2 += (a * a + b * b) + (c * c + d * d);
        }
      } else {
        feed(r, active, w & 255, v.x, shift, bins);
        feed(r, active, (w >> 8) & 255, v.y, shift, bins);
        feed(r, active, (w >> 16) & 255, v.z, shift, bins);
        feed(r, active, w >> 24, v.w, shift, bins);
      }
    }
  } else {
    const int64_t per = (HW + splits - 1) / splits;
    const int64_t lo = (int64_t)split * per;
    const int64_t hi = lo + per < HW ? lo + per : HW;
    for (int64_t base = lo; base < hi; base += kSegThreads) {
      const int64_t i = base + tid;
      const bool active = i < hi;
      feed(r, active, active ? seg[i] : 0, active ? x[i] : 0.f, shift, bins);
    }
  }
  flush_runs(r, r.label >= 0, bins);
}

// grid (splits, N*C). partial: [N*C][splits][256][4] doubles = (c_s1, c_s2, s_s1, s_s2);
// only rows of valid labels are written (and later read).
__global__ __launch_bounds__(kSegThreads) void masked_sums_kernel(
    const float* __restrict__ content, const float* __restrict__ style,
    const uint8_t* __restrict__ c_seg, const uint8_t* __restrict__ s_seg,
    const int* __restrict__ plan, int C, int64_t HWc, int64_t HWs,
    double* __restrict__ partial) {
  __shared__ double bins[kSegWaves][kLabels][2];
  const int split = blockIdx.x, splits = gridDim.x;
  const int plane = blockIdx.y, n = plane / C;
  const int tid = threadIdx.x, wave = tid >> 6;
  double acc[4];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
#pragma unroll
    for (int w = 0; w < kSegWaves; ++w) {
      bins[w][tid][0] = 0.0;
      bins[w][tid][1] = 0.0;
    }
    __syncthreads();
    if (half == 0)
      plane_label_sums(content + (int64_t)plane * HWc, c_seg + (int64_t)n * HWc, HWc, split,
                       splits, &bins[wave][0][0]);
    else
      plane_label_sums(style + (int64_t)plane * HWs, s_seg + (int64_t)n * HWs, HWs, split,
                       splits, &bins[wave][0][0]);
    __syncthreads();
    double t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int w = 0; w < kSegWaves; ++w) {  // fixed order
      t1 += bins[w][tid][0];
      t2 += bins[w][tid][1];
    }
    acc[2 * half] = t1;
    acc[2 * half + 1] = t2;
    __syncthreads();
  }
  if (plan[((int64_t)n * kLabels + tid) * kPlanStride + kPlanValid]) {
    double* p = partial + (((int64_t)plane * splits + split) * kLabels + tid) * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = acc[k];
  }
}

// mean and sqrt(unbiased var + eps) of `cnt` values from their shifted sums
__device__ __forceinline__ void finish_stats(double t1, double t2, int cnt, float shift,
                                             float eps, float* mean, float* stdv) {
  const double n = (double)cnt;
  const double m = t1 / n;
  const double var = (t2 - t1 * m) / (n - 1.0);
  const float varf = (float)(var < 0.0 ? 0.0 : var);
  *mean = (float)((double)shift + m);
  *stdv = __fsqrt_rn(__fadd_rn(varf, eps));
}

// grid N*C, one thread per label. params: [N*C][256] float4 = (mean_c, std_c, std_s, mean_s)
__global__ __launch_bounds__(kLabels) void masked_params_kernel(
    const float* __restrict__ content, const float* __restrict__ style,
    const int* __restrict__ plan, const double* __restrict__ partial, int C, int64_t HWc,
    int64_t HWs, int splits, float eps, float4* __restrict__ params) {
  const int plane = blockIdx.x, n = plane / C, lab = threadIdx.x;
  const int* e = plan + ((int64_t)n * kLabels + lab) * kPlanStride;
  float4 row = make_float4(0.f, kPassThrough, 1.f, 0.f);
  if (e[kPlanValid]) {
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < splits; ++s) {  // fixed order
      const double* p = partial + (((int64_t)plane * splits + s) * kLabels + lab) * 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) t[k] += p[k];
    }
    finish_stats(t[0], t[1], e[kPlanC], content[(int64_t)plane * HWc], eps, &row.x, &row.y);
    finish_stats(t[2], t[3], e[kPlanS], style[(int64_t)plane * HWs], eps, &row.w, &row.z);
  }
  params[(int64_t)plane * kLabels + lab] = row;
}

// ---- apply ------------------------------------------------------------------------------
template <bool kSkip>
__device__ __forceinline__ float masked_one(float v, float s, int lab, const float4* prm) {
#pragma clang fp contract(off)
  float r = v;
  const float4 p = prm[lab];
  if (!(p.y < 0.f)) r = (v - p.x) / p.y * p.z + p.w;
  return kSkip ? s + r : r;
}

template <bool kSkip>
__global__ __launch_bounds__(256) void masked_apply_kernel(
    const float* __restrict__ x, const float* __restrict__ skip,
    const uint8_t* __restrict__ seg, const float4* __restrict__ params,
    float* __restrict__ out, int C, int64_t HW, int chunks_per_plane, int vec) {
  __shared__ float4 prm[kLabels];
  const int plane = blockIdx.x / chunks_per_plane;
  const int chunk = blockIdx.x - plane * chunks_per_plane;
  const int n = plane / C;
  prm[threadIdx.x] = params[(int64_t)plane * kLabels + threadIdx.x];
  __syncthreads();
  const float* __restrict__ xp = x + (int64_t)plane * HW;
  const float* __restrict__ kp = kSkip ? skip + (int64_t)plane * HW : nullptr;
  const uint8_t* __restrict__ sp = seg + (int64_t)n * HW;
  float* __restrict__ op = out + (int64_t)plane * HW;
  const int64_t base = (int64_t)chunk * kApplyElems;
  if (vec) {
    const int64_t n4 = HW >> 2;
    const float4* __restrict__ x4 = reinterpret_cast<const float4*>(xp);
    const float4* __restrict__ k4 = reinterpret_cast<const float4*>(kp);
    const uint32_t* __restrict__ s4 = reinterpret_cast<const uint32_t*>(sp);
    float4* __restrict__ o4 = reinterpret_cast<float4*>(op);
#pragma unroll 4
    for (int u = 0; u < kApplyElems / 4 / 256; ++u) {
      const int64_t i = (base >> 2) + u * 256 + threadIdx.x;
      if (i < n4) {
        const float4 v = x4[i];
        const uint32_t w = s4[i];
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (kSkip) s = k4[i];
        float4 r;
        r.x = masked_one<kSkip>(v.x, s.x, w & 255, prm);
        r.y = masked_one<kSkip>(v.y, s.y, (w >> 8) & 255, prm);
        r.z = masked_one<kSkip>(v.z, s.z, (w >> 16) & 255, prm);
        r.w = masked_one<kSkip>(v.w, s.w, w >> 24, prm);
        o4[i] = r;
      }
    }
  } else {
    for (int u = 0; u < kApplyElems / 256; ++u) {
      const int64_t i = base + u * 256 + threadIdx.x;
      if (i < HW) op[i] = masked_one<kSkip>(xp[i], kSkip ? kp[i] : 0.f, sp[i], prm);
    }
  }
}

static int check_masked(int N, int C, int64_t HWc, int64_t HWs) {
  RPST_REQUIRE(N > 0 && C > 0 && HWc > 0 && HWs > 0, "bad shape N=%d C=%d HWc=%lld HWs=%lld",
               N, C, (long long)HWc, (long long)HWs);
  RPST_REQUIRE(HWc <= 0x7fffffff && HWs <= 0x7fffffff, "label map too large for int counts");
  RPST_REQUIRE((int64_t)N * C <= 65535, "too many planes (N*C > 65535)");
  return RPST_OK;
}

}  // namespace rpst

using namespace rpst;

extern "C" int rpst_segment_plan(const uint8_t* c_seg, const uint8_t* s_seg, int N,
                                 int64_t HWc, int64_t HWs, int32_t* plan,
                                 rpst_stream_t stream) {
  if (int e = check_masked(N, 1, HWc, HWs)) return e;
  RPST_REQUIRE(c_seg && s_seg && plan, "null pointer");
  segment_plan_kernel<<<N, kPlanThreads, 0, as_stream(stream)>>>(c_seg, s_seg, HWc, HWs, plan);
  return launch_status("segment_plan_kernel");
}

// one region: partial[N * C][masked_splits(C)][kLabels][4] fp64 sums
extern "C" size_t rpst_masked_adain_workspace_size(int N, int C) {
  if (N <= 0 || C <= 0) return 0;
  return (size_t)N * C * masked_splits(C) * kLabels * 4 * sizeof(double);
}

extern "C" int rpst_masked_adain_params(const float* content, const float* style,
                                        const uint8_t* c_seg, const uint8_t* s_seg,
                                        const int32_t* plan, int N, int C, int64_t HWc,
                                        int64_t HWs, float eps, float* params, void* workspace,
                                        size_t workspace_bytes, rpst_stream_t stream) {
  if (int e = check_masked(N, C, HWc, HWs)) return e;
  RPST_REQUIRE(content && style && c_seg && s_seg && plan && params, "null pointer");
  RPST_REQUIRE((reinterpret_cast<uintptr_t>(params) & 15) == 0, "params must be 16-B aligned");
  const size_t need = rpst_masked_adain_workspace_size(N, C);
  // RPST_REQUIRE_WS plus the fp64 alignment
  RPST_REQUIRE_OR(RPST_EWORKSPACE,
                  workspace && workspace_bytes >= need &&
                      (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                  "masked_adain_params: workspace %zu < %zu bytes (or unaligned)",
                  workspace_bytes, need);
  const int splits = masked_splits(C);
  hipStream_t st = as_stream(stream);
  double* partial = static_cast<double*>(workspace);
  masked_sums_kernel<<<dim3(splits, N * C), kSegThreads, 0, st>>>(
      content, style, c_seg, s_seg, plan, C, HWc, HWs, partial);
  if (int e = launch_status("masked_sums_kernel")) return e;
  masked_params_kernel<<<N * C, kLabels, 0, st>>>(content, style, plan, partial, C, HWc, HWs,
                                                  splits, eps,
                                                  reinterpret_cast<float4*>(params));
  return launch_status("masked_params_kernel");
}

extern "C" int rpst_masked_adain_apply(const float* content, const float* skip_or_null,
                                       const uint8_t* c_seg, const float* params, float* out,
                                       int N, int C, int64_t HW, rpst_stream_t stream) {
  if (int e = check_masked(N, C, HW, HW)) return e;
  RPST_REQUIRE(content && c_seg && params && out, "null pointer");
  RPST_REQUIRE((reinterpret_cast<uintptr_t>(params) & 15) == 0, "params must be 16-B aligned");
  const int64_t chunks = (HW + kApplyElems - 1) / kApplyElems;
  RPST_REQUIRE(chunks * N * C <= 0x7fffffffLL, "grid too large");
  auto al = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & a) == 0; };
  const int vec = (HW & 3) == 0 && al(content, 15) && al(out, 15) && al(c_seg, 3) &&
                  (!skip_or_null || al(skip_or_null, 15));
  const dim3 grid((unsigned)(chunks * N * C));
  const float4* p4 = reinterpret_cast<const float4*>(params);
  hipStream_t st = as_stream(stream);
  if (skip_or_null)
    masked_apply_kernel<true><<<grid, 256, 0, st>>>(content, skip_or_null, c_seg, p4, out, C, HW,
                                                    (int)chunks, vec);
  else
    masked_apply_kernel<false><<<grid, 256, 0, st>>>(content, nullptr, c_seg, p4, out, C, HW,
                                                     (int)chunks, vec);
  return launch_status("masked_apply_kernel");
}
