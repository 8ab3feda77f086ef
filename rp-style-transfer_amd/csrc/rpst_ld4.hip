// LDMSAdaINRPNet4 (`network: ld_adain4`, network/adain_rp.py:711-819): the memory traffic
// between its two encoders and its concat decoder (HBM-bound).
//
//   resize_nearest      F.interpolate(coarse, size) (default mode 'nearest') written into a
//                       channel slice of a wider tensor                  adain_rp.py:813-817
//   resized_mean_std    calc_mean_std of that resize, from the small source alone
//   ld4_fuse            cat([y, AdaIN(cat([fine, resize(coarse)]), style)]) in one pass: a decoder
//                       block's whole input                              adain_rp.py:786-798
//
// Nearest rule (ATen's nearest_neighbor_compute_source_index): per axis
//   src = min((int)floorf(dst * scale), in - 1),  scale = (float)in / (float)out,
// one fp32 product. nearest_src below is the one statement of it, for the kernels and for the
// host table (rpst_nearest_index_table); scale is formed on the host and passed in.
//
// Layout: NCHW fp32. H*W is often odd, so a plane's base is 4-byte aligned and no more: every
// destination plane is cut into a head of 0-3 elements up to the first 16-byte boundary,
// aligned quads stored with one 16-B store each, and a tail of 0-3 elements. Sources that
// stream (y, the fine feature, the statistics kernel's plane) are read as 4-byte-aligned
// 16-B vectors at the quad's own offset; the coarse source is gathered element by element
// (it is 1/4 .. 1/1024 of the destination and lives in cache). What streams once is read and
// written with nontemporal accesses. No atomics anywhere; the statistics are fp64 sums in a
// fixed order (thread-strided, wave shuffle, LDS), so a second run gives the same bits.
#include "rpst_common.h"

namespace rpst {

__host__ __device__ __forceinline__ int nearest_src(int dst, float scale, int in) {
  const int s = (int)floorf((float)dst * scale);
  return s < in - 1 ? s : in - 1;
}

// 16-B vectors: at a 16-byte boundary (stores) and at any 4-byte-aligned address (loads)
typedef float vfloat4 __attribute__((ext_vector_type(4)));
typedef float vfloat4u __attribute__((ext_vector_type(4), aligned(4)));

constexpr int kLd4Threads = 256;
constexpr int kLd4Quads = 4;                                    // quads per thread
constexpr int64_t kLd4Chunk = (int64_t)kLd4Threads * kLd4Quads * 4;  // elements per workgroup

// elements of a plane in front of its first 16-byte boundary
__device__ __forceinline__ int plane_head(const float* p, int64_t HW) {
  const int head = (int)((4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3);
  return (int64_t)head < HW ? head : (int)HW;
}

struct Resize {
  int h, w, H, W;
  float sy, sx;  // (float)h / H, (float)w / W
};

// element i of the H x W plane resized from the h x w plane src
__device__ __forceinline__ float gather1(const float* __restrict__ src, const Resize& r,
                                         int64_t i) {
  const int y = (int)(i / r.W), x = (int)(i - (int64_t)y * r.W);
  return src[(int64_t)nearest_src(y, r.sy, r.h) * r.w + nearest_src(x, r.sx, r.w)];
}

// elements i .. i + 3 (all inside the plane)
__device__ __forceinline__ float4 gather4(const float* __restrict__ src, const Resize& r,
                                          int64_t i) {
  int y = (int)(i / r.W), x = (int)(i - (int64_t)y * r.W);
  const float* __restrict__ row = src + (int64_t)nearest_src(y, r.sy, r.h) * r.w;
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    v[k] = row[nearest_src(x, r.sx, r.w)];
    if (++x == r.W) {
      x = 0;
      ++y;
      // (past the plane's last row only after the quad's last element: the row is not read)
      row = src + (int64_t)nearest_src(y < r.H ? y : r.H - 1, r.sy, r.h) * r.w;
    }
  }
  return make_float4(v[0], v[1], v[2], v[3]);
}

// NT: nontemporal, for what a kernel streams once (y, the fine feature, every output). Measured
// at N = 4, 512^2 against plain accesses: rpst_ld4_fuse 0.122 against 0.136 ms a block, test()
// 1.2-1.5 % faster on all three routes; at N = 1 the routes are level or faster
// (profiles/ld4/nt_ab.log). The coarse map is read plainly: the gather and the statistics
// share it.
template <bool NT>
__device__ __forceinline__ float4 load4u(const float* __restrict__ p) {
  const vfloat4u* q = reinterpret_cast<const vfloat4u*>(p);
  const vfloat4u v = NT ? __builtin_nontemporal_load(q) : *q;
  return make_float4(v.x, v.y, v.z, v.w);
}

template <bool NT>
__device__ __forceinline__ void store4(float* __restrict__ p, float4 v) {
  const vfloat4 u = {v.x, v.y, v.z, v.w};
  if (NT)
    __builtin_nontemporal_store(u, reinterpret_cast<vfloat4*>(p));
  else
    *reinterpret_cast<vfloat4*>(p) = u;
}

struct Affine {
  float mc, sc, ss, ms;
};

__device__ __forceinline__ float affine1(float v, const Affine& a) {
#pragma clang fp contract(off)
  // ATen's separate sub / div / mul / add roundings (base.py:410-418)
  return (v - a.mc) / a.sc * a.ss + a.ms;
}

__device__ __forceinline__ float4 affine4(float4 v, const Affine& a) {
  return make_float4(affine1(v.x, a), affine1(v.y, a), affine1(v.z, a), affine1(v.w, a));
}

// One workgroup per (destination plane, chunk of kLd4Chunk elements). MODE 0: copy of
// a streamed source plane; 1: affine of a streamed plane; 2: affine of a gathered plane;
// 3: gathered plane as it is (resize_nearest).
template <int MODE>
__device__ __forceinline__ void write_plane_chunk(const float* __restrict__ src,
                                                  float* __restrict__ dst, int64_t HW,
                                                  int chunk, const Resize& r,
                                                  const Affine& a) {
  const int head = plane_head(dst, HW);
  const int64_t nq = (HW - head) >> 2;
  const int tid = threadIdx.x;
  auto one = [&](int64_t i) {
    float v = (MODE >= 2) ? gather1(src, r, i) : src[i];
    dst[i] = (MODE == 1 || MODE == 2) ? affine1(v, a) : v;
  };
  if (chunk == 0) {  // the ragged ends: head on lanes 0-2, tail on lanes 64-66
    if (tid < head) one(tid);
    const int64_t t0 = head + 4 * nq;
    if (tid >= 64 && t0 + (tid - 64) < HW) one(t0 + (tid - 64));
  }
  const int64_t q0 = (int64_t)chunk * (kLd4Threads * kLd4Quads) + tid;
  float4 v[kLd4Quads];
#pragma unroll
  for (int u = 0; u < kLd4Quads; ++u) {
    const int64_t q = q0 + u * kLd4Threads;
    if (q < nq) {
      const int64_t i = head + 4 * q;
      v[u] = (MODE >= 2) ? gather4(src, r, i) : load4u<true>(src + i);
    }
  }
#pragma unroll
  for (int u = 0; u < kLd4Quads; ++u) {
    const int64_t q = q0 + u * kLd4Threads;
    if (q < nq) {
      const int64_t i = head + 4 * q;
      store4<true>(dst + i, (MODE == 1 || MODE == 2) ? affine4(v[u], a) : v[u]);
    }
  }
}

__global__ __launch_bounds__(kLd4Threads) void resize_nearest_kernel(
    const float* __restrict__ src, float* __restrict__ dst, int C, int c_off, int Ctot,
    Resize r, int chunks) {
  const int plane = blockIdx.x / chunks, chunk = blockIdx.x - plane * chunks;
  const int n = plane / C, c = plane - n * C;
  const int64_t HW = (int64_t)r.H * r.W;
  write_plane_chunk<3>(src + (int64_t)plane * r.h * r.w,
                       dst + ((int64_t)n * Ctot + c_off + c) * HW, HW, chunk, r, Affine{});
}

// out (N, Ca + 2h, H, W) = cat([y, affine(fine[:N]), affine(resize(coarse[:N]))]); pf / pc:
// [mean_c | mean_s | std_c | std_s], N * h each (ops.adain_params)
__global__ __launch_bounds__(kLd4Threads) void ld4_fuse_kernel(
    const float* __restrict__ y, const float* __restrict__ fine,
    const float* __restrict__ coarse, const float* __restrict__ pf,
    const float* __restrict__ pc, float* __restrict__ out, int N, int Ca, int hd, Resize r,
    int chunks) {
  const int plane = blockIdx.x / chunks, chunk = blockIdx.x - plane * chunks;
  const int Ct = Ca + 2 * hd;
  const int n = plane / Ct, co = plane - n * Ct;
  const int64_t HW = (int64_t)r.H * r.W;
  float* __restrict__ dst = out + (int64_t)plane * HW;
  if (co < Ca) {
    write_plane_chunk<0>(y + ((int64_t)n * Ca + co) * HW, dst, HW, chunk, r, Affine{});
    return;
  }
  const bool second = co >= Ca + hd;
  const int c = co - Ca - (second ? hd : 0);
  const float* __restrict__ p = second ? pc : pf;
  const int k = n * hd + c, nh = N * hd;
  const Affine a{p[k], p[2 * nh + k], p[3 * nh + k], p[nh + k]};
  if (second)
    write_plane_chunk<2>(coarse + (int64_t)k * r.h * r.w, dst, HW, chunk, r, a);
  else
    write_plane_chunk<1>(fine + (int64_t)k * HW, dst, HW, chunk, r, a);
}

// counts[s] = number of destination indices whose source is s, for the rows (the first h
// entries) and the columns (the next w). nearest_src is non-decreasing in dst, so the count
// is a difference of two lower bounds.
__device__ __forceinline__ int nearest_lower_bound(int s, float scale, int in, int out) {
  int lo = 0, hi = out;  // first dst in [0, out] with nearest_src(dst) >= s
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (nearest_src(mid, scale, in) >= s)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void nearest_counts_kernel(int* __restrict__ counts, Resize r) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= r.h + r.w) return;
  const bool col = t >= r.h;
  const int s = col ? t - r.h : t, in = col ? r.w : r.h, out = col ? r.W : r.H;
  const float scale = col ? r.sx : r.sy;
  const int hi = s + 1 < in ? nearest_lower_bound(s + 1, scale, in, out) : out;
  counts[t] = hi - nearest_lower_bound(s, scale, in, out);
}

// One workgroup per source plane: weighted, shifted fp64 sums (plane_stats_kernel's form)
__global__ __launch_bounds__(kLd4Threads) void resized_stats_kernel(
    const float* __restrict__ src, const int* __restrict__ counts, Resize r, float eps,
    float* __restrict__ mean, float* __restrict__ std_out) {
  const int p = blockIdx.x, tid = threadIdx.x;
  const int64_t hw = (int64_t)r.h * r.w;
  const float* __restrict__ x = src + (int64_t)p * hw;
  const int* __restrict__ rc = counts;
  const int* __restrict__ cc = counts + r.h;
  const float shift = x[0];
  double s1 = 0.0, s2 = 0.0;
  const int64_t nq = hw >> 2;
  for (int64_t q = tid; q < nq; q += kLd4Threads) {
    const float4 v4 = load4u<false>(x + 4 * q);
    const float v[4] = {v4.x, v4.y, v4.z, v4.w};
    int sy = (int)((4 * q) / r.w), sx = (int)(4 * q - (int64_t)sy * r.w);
    double a1 = 0.0, a2 = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double wgt = (double)rc[sy] * (double)cc[sx];
      const double d = (double)v[k] - shift;
      a1 += wgt * d;
      a2 += wgt * d * d;
      if (++sx == r.w) {
        sx = 0;
        if (sy + 1 < r.h) ++sy;  // (only after the plane's last element otherwise)
      }
    }
    s1 += a1;
    s2 += a2;
  }
  {
    const int64_t i = 4 * nq + tid;  // the 0-3 elements after the last quad
    if (tid < 4 && i < hw) {
      const int sy = (int)(i / r.w), sx = (int)(i - (int64_t)sy * r.w);
      const double wgt = (double)rc[sy] * (double)cc[sx];
      const double d = (double)x[i] - shift;
      s1 += wgt * d;
      s2 += wgt * d * d;
    }
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  __shared__ double red[2][kLd4Threads / kWave];
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = s1;
    red[1][tid >> 6] = s2;
  }
  __syncthreads();
  if (tid == 0) {
    double t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int k = 0; k < kLd4Threads / kWave; ++k) {
      t1 += red[0][k];
      t2 += red[1][k];
    }
    const double n = (double)r.H * (double)r.W;
    const double m = t1 / n;                       // mean of the shifted data
    const double var = (t2 - t1 * m) / (n - 1.0);  // NaN for n == 1, like torch.var
    float varf = (float)(var < 0.0 ? 0.0 : var);
    if ((int64_t)r.H * r.W == 1) varf = __int_as_float(0x7fc00000);
    mean[p] = (float)((double)shift + m);
    std_out[p] = __fsqrt_rn(__fadd_rn(varf, eps));
  }
}

static int check_resize(int N, int C, int h, int w, int H, int W) {
  RPST_REQUIRE(N > 0 && C > 0 && h > 0 && w > 0 && H > 0 && W > 0,
               "bad shape N=%d C=%d h=%d w=%d H=%d W=%d", N, C, h, w, H, W);
  RPST_REQUIRE(h <= H && w <= W, "resize enlarges only: source %dx%d > destination %dx%d", h,
               w, H, W);
  RPST_REQUIRE(H < (1 << 24) && W < (1 << 24), "destination %dx%d too large", H, W);
  return RPST_OK;
}

static Resize make_resize(int h, int w, int H, int W) {
  return Resize{h, w, H, W, (float)h / (float)H, (float)w / (float)W};
}

// grid of (planes x chunks of the H x W plane) workgroups -> chunks, or 0 with the error set
static int plane_chunks(int64_t planes, int64_t HW, unsigned* grid) {
  const int64_t chunks = (HW + kLd4Chunk - 1) / kLd4Chunk;
  if (planes * chunks > 0x7fffffffLL) {
    set_error("grid too large");
    return 0;
  }
  *grid = (unsigned)(planes * chunks);
  return (int)chunks;
}

}  // namespace rpst

using namespace rpst;

extern "C" int rpst_nearest_index_table(int in, int out, int* index) {
  RPST_REQUIRE(index != nullptr, "null pointer");
  RPST_REQUIRE(in > 0 && out > 0 && out < (1 << 24), "bad sizes in=%d out=%d", in, out);
  const float scale = (float)in / (float)out;
  for (int d = 0; d < out; ++d) index[d] = nearest_src(d, scale, in);
  return RPST_OK;
}

extern "C" int rpst_resize_nearest(const float* src, float* dst, int N, int C, int h, int w,
                                   int H, int W, int channel_offset, int channels_total,
                                   rpst_stream_t stream) {
  RPST_REQUIRE(src && dst, "null pointer");
  if (int e = check_resize(N, C, h, w, H, W)) return e;
  RPST_REQUIRE(channel_offset >= 0 && (int64_t)channel_offset + C <= channels_total,
               "channels [%d, %d) outside the destination's %d", channel_offset,
               channel_offset + C, channels_total);
  unsigned grid;
  const int chunks = plane_chunks((int64_t)N * C, (int64_t)H * W, &grid);
  if (!chunks) return RPST_EINVAL;
  resize_nearest_kernel<<<grid, kLd4Threads, 0, as_stream(stream)>>>(
      src, dst, C, channel_offset, channels_total, make_resize(h, w, H, W), chunks);
  return launch_status("resize_nearest_kernel");
}

// one region: how many destination rows, then columns, read each source row / column
extern "C" size_t rpst_resized_mean_std_workspace_size(int h, int w) {
  return h > 0 && w > 0 ? sizeof(int) * ((size_t)h + (size_t)w) : 0;
}

extern "C" int rpst_resized_mean_std(const float* src, float* mean, float* std_out, int N, int C,
                                     int h, int w, int H, int W, float eps, void* workspace,
                                     size_t workspace_bytes, rpst_stream_t stream) {
  RPST_REQUIRE(src && mean && std_out, "null pointer");
  if (int e = check_resize(N, C, h, w, H, W)) return e;
  RPST_REQUIRE((int64_t)N * C <= 0x7fffffff / 2, "too many planes");
  const size_t need = rpst_resized_mean_std_workspace_size(h, w);
  RPST_REQUIRE_WS(need, "resized_mean_std: workspace %zu < %zu bytes", workspace_bytes, need);
  const Resize r = make_resize(h, w, H, W);
  int* counts = static_cast<int*>(workspace);
  hipStream_t st = as_stream(stream);
  nearest_counts_kernel<<<(h + w + 255) / 256, 256, 0, st>>>(counts, r);
  if (int e = launch_status("nearest_counts_kernel")) return e;
  resized_stats_kernel<<<N * C, kLd4Threads, 0, st>>>(src, counts, r, eps, mean, std_out);
  return launch_status("resized_stats_kernel");
}

extern "C" int rpst_ld4_fuse(const float* y, const float* fine, const float* coarse,
                             const float* params_fine, const float* params_coarse, float* out,
                             int N, int Ca, int hidden, int H, int W, int h, int w,
                             rpst_stream_t stream) {
  RPST_REQUIRE(fine && coarse && params_fine && params_coarse && out, "null pointer");
  RPST_REQUIRE(Ca >= 0 && (y != nullptr) == (Ca > 0),
               "y must be given exactly when Ca > 0 (Ca=%d)", Ca);
  if (int e = check_resize(N, hidden, h, w, H, W)) return e;
  unsigned grid;
  const int chunks = plane_chunks((int64_t)N * (Ca + 2 * (int64_t)hidden), (int64_t)H * W, &grid);
  if (!chunks) return RPST_EINVAL;
  RPST_REQUIRE((int64_t)N * (Ca + 2 * (int64_t)hidden) <= 0x7fffffff, "too many planes");
  ld4_fuse_kernel<<<grid, kLd4Threads, 0, as_stream(stream)>>>(
      y, fine, coarse, params_fine, params_coarse, out, N, Ca, hidden, make_resize(h, w, H, W),
      chunks);
  return launch_status("ld4_fuse_kernel");
}
