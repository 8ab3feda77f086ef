// SANet style attention (network/sanet.py:82-99) on fp32 MFMA, gfx950.
//
//   F = f(mvn(c)), G = g(mvn(s)), H = h(s)       (1x1 convs: rpst_conv.hip)
//   S = F^T G                  (B, HW, HW)        gemm #1  M=HW, N=HW, K=C
//   m_i = max_j S_ij, l_i = sum_j exp(S_ij - m_i)  rowstats (one wave per query row)
//   O = H softmax(S)^T         (B, C, HW)         gemm #2  M=C, N=HW, K=HW, with
//       exp(S_ij - m_i) applied while the B operand is staged into LDS and the 1/l_i
//       column scale applied in the epilogue: the probability matrix is never stored.
// No 1/sqrt(d) scaling (sanet.py:90-91). With C = 512 the QK^T operand per query is
// 2 KB, so materialising S (64 MiB per image at HW = 4096, 288 GB of HBM available)
// and streaming it twice costs ~20% of the MFMA time, far less than a flash-style
// kernel would lose to a 512-wide fp32 O accumulator per query tile.
//
// GEMM tile: 128 x 128 x 32, 256 threads = 2 x 2 waves of 64 x 64, v_mfma_f32_32x32x2_f32.
// Operands are staged k-major in LDS (As[k][m], Bs[k][n]) so the MFMA fragment reads
// are lane-contiguous; global tiles are loaded with 16-B loads along whichever dim is
// contiguous (RK: row-major rows with k contiguous; KR: k-rows with m/n contiguous).
// Register prefetch of tile t+1 overlaps the MFMAs of tile t.
#include <algorithm>

#include "rpst_common.h"

namespace rpst {

// flash-style forward attention (rpst_flash.hip)
bool sanet_flash_ok(int C, int HWq, int HWk);
int sanet_flash(const float* F, const float* G, const float* H, float* O, int B, int C, int HWq,
                int HWk, hipStream_t st);
int adaptive_flash_stats(const float* F, const float* G, int B, int C, int HW, float* rm,
                         float* rinv, hipStream_t st);
int adaptive_flash_apply(const float* F, const float* G, const float* H, float* O, int B, int C,
                         int HW, const float* rm, const float* rinv, const float* clamp, int mode,
                         float scale, hipStream_t st);

enum { LAY_RK = 0, LAY_KR = 1 };

constexpr int kGBN = 128, kGBK = 32, kGPad = 4;  // M tile: 128 * MW (gemm_f32_kernel)

// B-operand staging transforms (applied to S while it is staged; row r = query index):
//   BX_NONE   v
//   BX_EXP    exp(v - m_r)                                  softmax numerator (SANet)
//   BX_AEA    sigmoid(scale (exp(v - m_r) inv_r - c_r))     AEAModule clamp (sanet.py:45-47)
//   BX_AEAR   exp(relu(exp(v - m_r) inv_r - c_r) - m2_r)    AEALReluModule (sanet.py:66-69),
//             numerator of softmax(relu(P - c)); 1/l2_r is the epilogue column scale
//   BX_PROB   exp(v - m_r) inv_r                            softmax probability (attention
//             backward: dH = dO P with P formed while S is staged, never stored)
//   BX_AEARQ  BX_AEAR * inv2_r                              the normalised AEALRelu attention
//             (AdaptiveSANet backward: dH = dO Q)
enum { BX_NONE = 0, BX_EXP = 1, BX_AEA = 2, BX_AEAR = 3, BX_PROB = 4, BX_AEARQ = 5 };
template <int BX> constexpr bool bx_inv() { return BX == BX_AEA || BX == BX_AEAR || BX == BX_PROB || BX == BX_AEARQ; }
template <int BX> constexpr bool bx_clamp() { return BX == BX_AEA || BX == BX_AEAR || BX == BX_AEARQ; }
template <int BX> constexpr bool bx_m2() { return BX == BX_AEAR || BX == BX_AEARQ; }

// Per-row vectors of the B operand's transform (each indexed batch * sV + r).
struct RowVec {
  const float* m;      // row max of S
  const float* inv;    // 1 / sum exp(S - m)
  const float* clamp;  // AEA threshold per query row
  const float* m2;     // BX_AEAR: row max of relu(P - c)
  float scale;         // BX_AEA: sigmoid slope (scale_value)
  const float* inv2;   // BX_AEARQ: 1 / sum exp(relu(P - c) - m2)
};

struct GemmArgs {
  const float* A;
  const float* B;
  float* C;
  RowVec rv;              // B-operand transform vectors (BX_* != BX_NONE)
  const float* colscale;  // optional per-n multiplier in the epilogue
  const float* colbias;   // optional per-n bias added after the scale (nn.Linear bias)
  int act;                // epilogue activation: 0 none, 1 LeakyReLU(0.2)
  int M, N, K, lda, ldb, ldc;
  int64_t sA, sB, sC, sV;  // batch strides (elements); sV for the row / column vectors
  // In-kernel split-K (BX_NONE only): grid z = batch * ks, z -> (batch z / ks, K chunk z % ks
  // of kc elements); C advances by sC per z, so each chunk writes its own partial.
  int ks = 1, kc = 0;
  int accum = 0;  // epilogue adds to C (a sum over launches, in launch order)
};

template <int BX>
__device__ __forceinline__ float bx_apply(float v, float m, float inv, float c, float m2,
                                          float scale, float inv2 = 1.f) {
  if (BX == BX_EXP) return expf(v - m);
  if (BX == BX_AEA) {
    const float p = expf(v - m) * inv;
    return 1.f / (1.f + expf(-(scale * (p - c))));
  }
  if (BX == BX_AEAR) {
    const float p = expf(v - m) * inv;
    return expf(fmaxf(p - c, 0.f) - m2);
  }
  if (BX == BX_PROB) return expf(v - m) * inv;
  if (BX == BX_AEARQ) {
    const float p = expf(v - m) * inv;
    return expf(fmaxf(p - c, 0.f) - m2) * inv2;
  }
  return v;
}

// Stage a kGBK x 128 tile of operand X (rows r0.., k0..) into registers.
template <int LAY, int BX, bool VEC>
__device__ __forceinline__ void g_load(float (&reg)[16], const float* __restrict__ X, int ld,
                                       int r0, int k0, int R, int K, const RowVec& rv,
                                       int64_t voff, int tid) {
  if (LAY == LAY_KR) {
    // thread -> (k = tid>>5 + 8p, r4 = (tid&31)*4), 4 passes of 8 k-rows
    const int kk = tid >> 5, r = r0 + (tid & 31) * 4;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int k = k0 + kk + 8 * p;
      if (VEC) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < K && r < R) v = *reinterpret_cast<const float4*>(X + (int64_t)k * ld + r);
        reg[4 * p + 0] = v.x;
        reg[4 * p + 1] = v.y;
        reg[4 * p + 2] = v.z;
        reg[4 * p + 3] = v.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          reg[4 * p + e] = (k < K && r + e < R) ? X[(int64_t)k * ld + r + e] : 0.f;
      }
      if (BX != BX_NONE) {  // KR staging: the row of S (the query) is the k index
        const int64_t q = voff + (k < K ? k : 0);
        const float mx = rv.m[q];
        const float inv = bx_inv<BX>() ? rv.inv[q] : 0.f;
        const float cl = bx_clamp<BX>() ? rv.clamp[q] : 0.f;
        const float m2 = bx_m2<BX>() ? rv.m2[q] : 0.f;
        const float i2 = BX == BX_AEARQ ? rv.inv2[q] : 1.f;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          reg[4 * p + e] = (k < K && r + e < R)
                               ? bx_apply<BX>(reg[4 * p + e], mx, inv, cl, m2, rv.scale, i2)
                               : 0.f;
      }
    }
  } else {
    // thread -> (r = tid>>3 + 32p, k4 = (tid&7)*4), 4 passes of 32 rows
    const int rr = tid >> 3, k = k0 + (tid & 7) * 4;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int r = r0 + rr + 32 * p;
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (VEC) {
        if (r < R && k < K) {
          float4 q = *reinterpret_cast<const float4*>(X + (int64_t)r * ld + k);
          v[0] = q.x;
          v[1] = q.y;
          v[2] = q.z;
          v[3] = q.w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (r < R && k + e < K) ? X[(int64_t)r * ld + k + e] : 0.f;
      }
      if (BX != BX_NONE) {
        const int64_t q = voff + (r < R ? r : 0);
        const float mx = rv.m[q];
        const float inv = bx_inv<BX>() ? rv.inv[q] : 0.f;
        const float cl = bx_clamp<BX>() ? rv.clamp[q] : 0.f;
        const float m2 = bx_m2<BX>() ? rv.m2[q] : 0.f;
        const float i2 = BX == BX_AEARQ ? rv.inv2[q] : 1.f;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          v[e] = (r < R && k + e < K) ? bx_apply<BX>(v[e], mx, inv, cl, m2, rv.scale, i2) : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) reg[4 * p + e] = v[e];
    }
  }
}

// LDS row stride of a staged operand: RK tiles are written transposed (4 k of one row per
// thread), so their stride is odd (129: 2-way bank conflicts on those scalar stores instead
// of 4-way at 132); KR tiles keep 132 for their 16-B stores. (Measured: S = F^T G + O at
// B = 32, C = 512, HW = 4096: 10.54 -> 10.33 ms, tools/bench_attn.py; a 64-deep k tile
// (11.2 ms) and double-buffered LDS with the exp applied at the LDS store (11.2 ms) were
// slower.)
template <int LAY, int W = 128>
constexpr int g_ld() { return LAY == LAY_RK ? W + 1 : W + kGPad; }

template <int LAY, int LD = g_ld<LAY>()>
__device__ __forceinline__ void g_store(float* __restrict__ Xs, const float (&reg)[16], int tid) {
  if (LAY == LAY_KR) {
    const int kk = tid >> 5, r4 = (tid & 31) * 4;
#pragma unroll
    for (int p = 0; p < 4; ++p)
      *reinterpret_cast<float4*>(Xs + (kk + 8 * p) * LD + r4) =
          make_float4(reg[4 * p], reg[4 * p + 1], reg[4 * p + 2], reg[4 * p + 3]);
  } else {
    const int rr = tid >> 3, k4 = (tid & 7) * 4;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int e = 0; e < 4; ++e) Xs[(k4 + e) * LD + rr + 32 * p] = reg[4 * p + e];
  }
}

// MW = 2: 256-row M tiles (each wave 128 x 64): the B tile (and, for the attention, its
// exp / AEA transform) is staged once per 256 rows of A instead of per 128
template <int ALAY, int BLAY, int BX, bool VECA, bool VECB, int MW>
__global__ __launch_bounds__(256, 2) void gemm_f32_kernel(GemmArgs g) {
  constexpr int BMT = 128 * MW;
  constexpr int LDA = g_ld<ALAY, BMT>(), LDB = g_ld<BLAY>();
  __shared__ float As[kGBK * LDA];
  __shared__ float Bs[kGBK * LDB];
  int b = blockIdx.z, K = g.K;
  int64_t koA = 0, koB = 0;
  if (g.ks > 1) {
    const int kb = (b % g.ks) * g.kc;
    b /= g.ks;
    K = min(g.kc, g.K - kb);
    koA = ALAY == LAY_RK ? kb : (int64_t)kb * g.lda;
    koB = BLAY == LAY_RK ? kb : (int64_t)kb * g.ldb;
  }
  const int m0 = blockIdx.y * BMT, n0 = blockIdx.x * kGBN;
  const float* A = g.A + b * g.sA + koA;
  const float* B = g.B + b * g.sB + koB;
  float* C = g.C + (int64_t)blockIdx.z * g.sC;
  const int64_t voff = (int64_t)b * g.sV;
  const float* cscale = g.colscale ? g.colscale + voff : nullptr;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, j = lane & 31;

  floatx16 acc[2 * MW][2];
#pragma unroll
  for (int mt = 0; mt < 2 * MW; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

  float ra[MW][16], rb[16];
  const int ktiles = (K + kGBK - 1) / kGBK;
#pragma unroll
  for (int i = 0; i < MW; ++i)
    g_load<ALAY, BX_NONE, VECA>(ra[i], A, g.lda, m0 + 128 * i, 0, g.M, K, g.rv, 0, tid);
  g_load<BLAY, BX, VECB>(rb, B, g.ldb, n0, 0, g.N, K, g.rv, voff, tid);
  for (int kt = 0; kt < ktiles; ++kt) {
#pragma unroll
    for (int i = 0; i < MW; ++i) g_store<ALAY, LDA>(As + 128 * i, ra[i], tid);
    g_store<BLAY, LDB>(Bs, rb, tid);
    __syncthreads();
    if (kt + 1 < ktiles) {
#pragma unroll
      for (int i = 0; i < MW; ++i)
        g_load<ALAY, BX_NONE, VECA>(ra[i], A, g.lda, m0 + 128 * i, (kt + 1) * kGBK, g.M, K,
                                    g.rv, 0, tid);
      g_load<BLAY, BX, VECB>(rb, B, g.ldb, n0, (kt + 1) * kGBK, g.N, K, g.rv, voff, tid);
    }
#pragma unroll
    for (int kk = 0; kk < kGBK / 2; ++kk) {
      float av[2 * MW], bv[2];
#pragma unroll
      for (int mt = 0; mt < 2 * MW; ++mt)
        av[mt] = As[(2 * kk + h) * LDA + wm * 64 * MW + mt * 32 + j];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) bv[nt] = Bs[(2 * kk + h) * LDB + wn * 64 + nt * 32 + j];
#pragma unroll
      for (int mt = 0; mt < 2 * MW; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
    }
    __syncthreads();
  }

#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int n = n0 + wn * 64 + nt * 32 + j;
    if (n >= g.N) continue;
    const float cs = cscale ? cscale[n] : 1.f;
    const float cb = g.colbias ? g.colbias[n] : 0.f;
#pragma unroll
    for (int mt = 0; mt < 2 * MW; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 64 * MW + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        float v = acc[mt][nt][r] * cs;
        if (g.colbias) v += cb;
        if (g.act == 1) v = v > 0.f ? v : 0.2f * v;
        if (m < g.M) {
          float* cp = C + (int64_t)m * g.ldc + n;
          *cp = g.accum ? *cp + v : v;
        }
      }
  }
}

// Row max and 1 / sum exp(x - max) of `rows` rows of length L (one wave per row).
__global__ __launch_bounds__(256) void rowstats_kernel(const float* __restrict__ S,
                                                       float* __restrict__ rmax,
                                                       float* __restrict__ rinv, int64_t rows,
                                                       int L) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* s = S + row * L;
  float mx = -INFINITY;
  if ((L & 3) == 0) {
    for (int i = lane * 4; i < L; i += 256) {
      float4 v = *reinterpret_cast<const float4*>(s + i);
      mx = fmaxf(mx, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    }
  } else {
    for (int i = lane; i < L; i += 64) mx = fmaxf(mx, s[i]);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  if ((L & 3) == 0) {
    for (int i = lane * 4; i < L; i += 256) {
      float4 v = *reinterpret_cast<const float4*>(s + i);
      sum += (expf(v.x - mx) + expf(v.y - mx)) + (expf(v.z - mx) + expf(v.w - mx));
    }
  } else {
    for (int i = lane; i < L; i += 64) sum += expf(s[i] - mx);
  }
  sum = wave_sum(sum);
  if (lane == 0) {
    rmax[row] = mx;
    rinv[row] = 1.f / sum;
  }
}

// What a call site asks of the GEMM: each operand once as pointer, leading dimension and
// batch stride (elements), the rest by name. launch_gemm lays it out as the kernel's GemmArgs.
template <class T>
struct MatT {
  T* p;
  int ld;
  int64_t stride;
};
using Mat = MatT<const float>;
struct GemmReq {
  Mat A, B;
  MatT<float> C;
  int M, N, K;
  RowVec rv = {};
  int64_t sV = 0;  // batch stride of rv's vectors and of colscale
  const float* colscale = nullptr;
  const float* colbias = nullptr;
  int act = 0;
  int ks = 1, kc = 0;
  int accum = 0;
};

template <int ALAY, int BLAY, int BX>
static void launch_gemm(const GemmReq& r, int batch, hipStream_t st) {
  const GemmArgs g{.A = r.A.p, .B = r.B.p, .C = r.C.p, .rv = r.rv, .colscale = r.colscale,
                   .colbias = r.colbias, .act = r.act, .M = r.M, .N = r.N, .K = r.K,
                   .lda = r.A.ld, .ldb = r.B.ld, .ldc = r.C.ld, .sA = r.A.stride,
                   .sB = r.B.stride, .sC = r.C.stride, .sV = r.sV, .ks = r.ks, .kc = r.kc,
                   .accum = r.accum};
  const int mw = g.M >= 256 ? 2 : 1;
  dim3 grid((g.N + kGBN - 1) / kGBN, (g.M + 128 * mw - 1) / (128 * mw), batch * g.ks);
  auto aligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  // 16-B loads need the contiguous dim, the leading dim and the batch stride % 4 == 0
  const bool va = aligned(g.A) && (g.lda % 4 == 0) && (g.sA % 4 == 0) && (g.kc % 4 == 0) &&
                  ((ALAY == LAY_KR) ? (g.M % 4 == 0) : (g.K % 4 == 0));
  const bool vb = aligned(g.B) && (g.ldb % 4 == 0) && (g.sB % 4 == 0) && (g.kc % 4 == 0) &&
                  ((BLAY == LAY_KR) ? (g.N % 4 == 0) : (g.K % 4 == 0));
  if (mw == 2) {
    if (va && vb) gemm_f32_kernel<ALAY, BLAY, BX, true, true, 2><<<grid, 256, 0, st>>>(g);
    else gemm_f32_kernel<ALAY, BLAY, BX, false, false, 2><<<grid, 256, 0, st>>>(g);
  } else {
    if (va && vb) gemm_f32_kernel<ALAY, BLAY, BX, true, true, 1><<<grid, 256, 0, st>>>(g);
    else gemm_f32_kernel<ALAY, BLAY, BX, false, false, 1><<<grid, 256, 0, st>>>(g);
  }
}


// ---- SANet attention backward (sanet.py:86-94 under autograd) ---------------------------
// dS = P (dP - rowsum(dP P)) with P = exp(S - m) inv formed from the logits (P is never
// stored); in place over dP. One wave per row, fixed-order sums. rowsum(dP P) is divided by
// the row's own sum of P (1 up to fp32 rounding), so each row of dS sums to zero to fp32
// rounding: the softmax's shift invariance (the SANet g.bias gradient is exactly zero in exact
// arithmetic) survives the recomputed P.
__global__ __launch_bounds__(256) void softmax_bwd_logits_kernel(const float* __restrict__ S,
                                                                 const float* __restrict__ rmax,
                                                                 const float* __restrict__ rinv,
                                                                 float* __restrict__ dP,
                                                                 int64_t rows, int L) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* s = S + row * L;
  float* d = dP + row * L;
  const float m = rmax[row], inv = rinv[row];
  float dot = 0.f, psum = 0.f;
  for (int i = lane; i < L; i += 64) {
    const float p = expf(s[i] - m) * inv;
    dot = fmaf(d[i], p, dot);
    psum += p;
  }
  dot = wave_sum(dot) / wave_sum(psum);
  for (int i = lane; i < L; i += 64) d[i] = expf(s[i] - m) * inv * (d[i] - dot);
}

// out[b][i] = sum_j part[b * n + j][i], j first to last (b = blockIdx.y)
__global__ void partial_sum_kernel(const float* __restrict__ part, float* __restrict__ out,
                                   int64_t per, int n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= per) return;
  const float* p = part + (int64_t)blockIdx.y * n * per + i;
  float acc = p[0];
  for (int j = 1; j < n; ++j) acc += p[j * per];
  out[blockIdx.y * per + i] = acc;
}
static int partial_sum(const float* part, float* out, int64_t per, int n, int B, const char* what,
                       hipStream_t st) {
  partial_sum_kernel<<<dim3((unsigned)((per + 255) / 256), B), 256, 0, st>>>(part, out, per, n);
  return launch_status(what);
}

// db[c] = sum_{b, p} dy[b][c][p]: one block per channel (a launch of C blocks fills the chip
// at the SANet's 512 channels; one wave per channel ran 88 us for a 64 MB read), 16-B loads
// when the planes allow, fixed order: per-thread strided sums, wave sums, then the four
// waves in order
__global__ __launch_bounds__(256) void channel_sum_kernel(const float* __restrict__ dy,
                                                          float* __restrict__ db, int nb, int C,
                                                          int64_t HW) {
  __shared__ float part[4];
  const int c = blockIdx.x;
  const int tid = threadIdx.x;
  const bool vec = (HW & 3) == 0 && (reinterpret_cast<uintptr_t>(dy) & 15) == 0;
  float s = 0.f;
  for (int b = 0; b < nb; ++b) {
    const float* p = dy + ((int64_t)b * C + c) * HW;
    if (vec) {
      for (int64_t i = 4 * tid; i < HW; i += 1024) {
        const float4 v = *reinterpret_cast<const float4*>(p + i);
        s += (v.x + v.y) + (v.z + v.w);
      }
    } else {
      for (int64_t i = tid; i < HW; i += 256) s += p[i];
    }
  }
  s = wave_sum(s);
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) db[c] = ((part[0] + part[1]) + part[2]) + part[3];
}

// chunk-local row vectors of a query chunk: dst[b][i] = src[b][q0 + i] and back
__global__ void rows_gather_kernel(const float* __restrict__ src, float* __restrict__ dst, int B,
                                   int HW, int q0, int n) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)B * n) return;
  const int64_t b = t / n;
  dst[t] = src[b * HW + q0 + (t - b * n)];
}
__global__ void rows_scatter_kernel(const float* __restrict__ src, float* __restrict__ dst, int B,
                                    int HW, int q0, int n) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)B * n) return;
  const int64_t b = t / n;
  dst[b * HW + q0 + (t - b * n)] = src[t];
}

// ---- AdaptiveSANet backward (sanet.py:100-138 under autograd; train.py:118-119 trains it) --
// Row pass from dQ (the gradient at the clamped attention) to dS (the gradient at the logits,
// in place over dQ) and dc (at the per-query clamp value):
//   aea  Q = sigmoid(scale (P - c)):      dP = dQ scale Q (1 - Q)
//   relu Q = softmax(relu(P - c)):        dR = Q (dQ - rowsum(dQ Q)), dP = dR [P > c]
//   dc = -sum_j dP, dS = P (dP - rowsum(dP P))   (P = softmax(S), from the logits)
// One wave per row; the row sums are divided by the row's own sum of P / Q (1 to rounding) as
// in softmax_bwd_logits_kernel.
__global__ __launch_bounds__(256) void aea_bwd_rows_kernel(const float* __restrict__ S,
                                                           RowVec rv, float* __restrict__ dQ,
                                                           float* __restrict__ dc, int mode,
                                                           int64_t rows, int L) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* s = S + row * L;
  float* d = dQ + row * L;
  const float m = rv.m[row], inv = rv.inv[row], c = rv.clamp[row], scale = rv.scale;
  const float m2 = mode == 1 ? rv.m2[row] : 0.f, i2 = mode == 1 ? rv.inv2[row] : 0.f;
  float dq_dot = 0.f;  // relu: rowsum(dQ Q) / rowsum(Q)
  if (mode == 1) {
    float dot = 0.f, qs = 0.f;
    for (int i = lane; i < L; i += 64) {
      const float p = expf(s[i] - m) * inv;
      const float q = expf(fmaxf(p - c, 0.f) - m2) * i2;
      dot = fmaf(d[i], q, dot);
      qs += q;
    }
    dq_dot = wave_sum(dot) / wave_sum(qs);
  }
  auto dp_of = [&](float p, float g) {
    if (mode == 0) {
      const float q = 1.f / (1.f + expf(-(scale * (p - c))));
      return g * scale * q * (1.f - q);
    }
    const float q = expf(fmaxf(p - c, 0.f) - m2) * i2;
    return p - c > 0.f ? q * (g - dq_dot) : 0.f;
  };
  float dot = 0.f, ps = 0.f, dcs = 0.f;
  for (int i = lane; i < L; i += 64) {
    const float p = expf(s[i] - m) * inv;
    const float dp = dp_of(p, d[i]);
    dot = fmaf(dp, p, dot);
    ps += p;
    dcs += dp;
  }
  dot = wave_sum(dot) / wave_sum(ps);
  dcs = wave_sum(dcs);
  for (int i = lane; i < L; i += 64) {
    const float p = expf(s[i] - m) * inv;
    d[i] = p * (dp_of(p, d[i]) - dot);
  }
  if (lane == 0) dc[row] = -dcs;
}

// f_psi backward, per query row k (= b * HW + i): t = Z_k . w2 + b2 recomputed in the order
// clamp_head_kernel used; dt = dc * head'(t) (aea: interval sigmoid'(t), relu: (1 - tanh^2)/2);
// du[k][n] = dt w2[n] LeakyReLU'(Z[k][n]) (Z = LeakyReLU(u): u > 0 iff Z > 0). One wave per row.
__global__ __launch_bounds__(256) void fpsi_bwd_rows_kernel(const float* __restrict__ Z,
                                                            const float* __restrict__ w2,
                                                            const float* __restrict__ b2,
                                                            const float* __restrict__ dc,
                                                            float* __restrict__ dt,
                                                            float* __restrict__ du, int64_t rows,
                                                            int hid, int mode, float interval) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* z = Z + row * hid;
  float acc = 0.f;
  for (int n = lane; n < hid; n += 64) acc = fmaf(z[n], w2[n], acc);
  acc = wave_sum(acc);
  const float t = acc + b2[0];
  float g;
  if (mode == 0) {
    const float sg = 1.f / (1.f + expf(-t));
    g = dc[row] * interval * sg * (1.f - sg);
  } else {
    const float th = tanhf(t);
    g = dc[row] * 0.5f * (1.f - th * th);
  }
  float* u = du + row * hid;
  for (int n = lane; n < hid; n += 64) u[n] = g * w2[n] * (z[n] > 0.f ? 1.f : 0.2f);
  if (lane == 0) dt[row] = g;
}

// Column sums of the f_psi backward over all B * HW query rows, in two fixed-order passes:
// part[(c * 3 + s) * (hid + 1) + n] over the 128-row chunk c (s = 0: sum dt Z[.][n] -> dw2,
// s = 1: sum du[.][n] -> db1, column hid of s = 2: sum dt -> db2), then the chunks in order.
// (The single-pass form ran 257 threads over all rows: latency-bound on two CUs.)
constexpr int kColChunk = 128;
__global__ __launch_bounds__(256) void fpsi_colsum_part_kernel(
    const float* __restrict__ Z, const float* __restrict__ du, const float* __restrict__ dt,
    float* __restrict__ part, int64_t rows, int hid) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int c = blockIdx.y;
  if (n > hid) return;
  const int64_t k0 = (int64_t)c * kColChunk;
  const int64_t k1 = rows < k0 + kColChunk ? rows : k0 + kColChunk;
  float a = 0.f, b = 0.f;
  if (n == hid) {
    for (int64_t k = k0; k < k1; ++k) a += dt[k];
  } else {
    for (int64_t k = k0; k < k1; ++k) {
      a = fmaf(dt[k], Z[k * hid + n], a);
      b += du[k * hid + n];
    }
  }
  float* p = part + (int64_t)c * 3 * (hid + 1);
  if (n == hid) {
    p[2 * (hid + 1) + n] = a;
  } else {
    p[n] = a;
    p[(hid + 1) + n] = b;
  }
}

__global__ void fpsi_colsum_final_kernel(const float* __restrict__ part, float* __restrict__ dw2,
                                         float* __restrict__ db1, float* __restrict__ db2,
                                         int chunks, int hid) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n > hid) return;
  float a = 0.f, b = 0.f;
  for (int c = 0; c < chunks; ++c) {
    const float* p = part + (int64_t)c * 3 * (hid + 1);
    if (n == hid) {
      a += p[2 * (hid + 1) + n];
    } else {
      a += p[n];
      b += p[(hid + 1) + n];
    }
  }
  if (n == hid) {
    db2[0] = a;
  } else {
    dw2[n] = a;
    db1[n] = b;
  }
}

// ---- AdaptiveSANet (sanet.py:12-18, 26-71, 100-138) -----------------------------------
// functional.normalize(x, dim=1): x / max(||x||_2 over channels, 1e-12), per position.
// Block = 64 consecutive positions (of one image) x 4 channel quarters (one wave each; a
// wave reads 64 consecutive positions of one channel row per load: coalesced); each lane
// sums its quarter's squares in fp64 over 4 interleaved chains, the quarters are combined in
// order through LDS, and every lane scales its quarter by the one reciprocal of the norm (one
// rounding more than the division: <= 1 ulp). (The thread-per-position form with a serial
// fp64 chain and a division per element took 0.49 ms per call at B = 32, C = 512, HW = 4096.)
__global__ __launch_bounds__(256) void colnorm_kernel(const float* __restrict__ x,
                                                      float* __restrict__ out, int B, int C,
                                                      int HW) {
  __shared__ double part[4][64];
  const int lane = threadIdx.x & 63, qtr = threadIdx.x >> 6;
  const int pblocks = (HW + 63) / 64;
  const int64_t b = blockIdx.x / pblocks;
  const int i = (int)(blockIdx.x - b * pblocks) * 64 + lane;
  const bool ok = i < HW;
  const int c0 = (int)((int64_t)C * qtr / 4), c1 = (int)((int64_t)C * (qtr + 1) / 4);
  const float* xp = x + b * C * (int64_t)HW + (ok ? i : 0);
  double ss[4] = {0.0, 0.0, 0.0, 0.0};
  if (ok) {
    int c = c0;
    for (; c + 4 <= c1; c += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double v = xp[(int64_t)(c + u) * HW];
        ss[u] = fma(v, v, ss[u]);
      }
    }
    for (; c < c1; ++c) {
      const double v = xp[(int64_t)c * HW];
      ss[0] = fma(v, v, ss[0]);
    }
  }
  part[qtr][lane] = (ss[0] + ss[1]) + (ss[2] + ss[3]);
  __syncthreads();
  if (!ok) return;
  const double tot = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
  const float r = 1.f / fmaxf((float)sqrt(tot), 1e-12f);
  float* op = out + b * C * (int64_t)HW + i;
  for (int c = c0; c < c1; ++c) op[(int64_t)c * HW] = xp[(int64_t)c * HW] * r;
}

// f_psi's last Linear(hid -> 1) + head: AEA  clamp = sigmoid(t) * interval + from
// (sanet.py:45); AEALRelu  clamp = (tanh(t) + 1) / 2 (sanet.py:66). One wave per row.
__global__ __launch_bounds__(256) void clamp_head_kernel(const float* __restrict__ Z,
                                                         const float* __restrict__ w2,
                                                         const float* __restrict__ b2,
                                                         float* __restrict__ clamp,
                                                         int64_t rows, int hid, int mode,
                                                         float from, float interval) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* z = Z + row * hid;
  float acc = 0.f;
  for (int n = lane; n < hid; n += 64) acc = fmaf(z[n], w2[n], acc);
  acc = wave_sum(acc);
  if (lane == 0) {
    const float t = acc + b2[0];
    clamp[row] = mode == 0 ? (1.f / (1.f + expf(-t))) * interval + from : (tanhf(t) + 1.f) / 2.f;
  }
}

// AEALRelu second softmax: per row, m2 = max_j relu(P_ij - c_i), inv2 = 1 / sum_j
// exp(relu(P_ij - c_i) - m2). LOGITS: the row holds S and P_ij = exp(S_ij - m_i) inv_i is
// formed exactly as the GEMM staging forms it; else the row holds P itself (a given attention
// matrix: aea_apply_kernel's mode 1; rmax and rinv unused). One wave per row.
template <bool LOGITS>
__global__ __launch_bounds__(256) void rowstats_relu_kernel(
    const float* __restrict__ S, const float* __restrict__ rmax, const float* __restrict__ rinv,
    const float* __restrict__ clamp, float* __restrict__ m2, float* __restrict__ inv2,
    int64_t rows, int L) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  const float* s = S + row * L;
  const float m = LOGITS ? rmax[row] : 0.f, inv = LOGITS ? rinv[row] : 0.f, c = clamp[row];
  auto p = [&](int i) { return LOGITS ? expf(s[i] - m) * inv : s[i]; };
  float mx = -INFINITY;
  for (int i = lane; i < L; i += 64) mx = fmaxf(mx, fmaxf(p(i) - c, 0.f));
  mx = wave_max(mx);
  float sum = 0.f;
  for (int i = lane; i < L; i += 64) sum += expf(fmaxf(p(i) - c, 0.f) - mx);
  sum = wave_sum(sum);
  if (lane == 0) {
    m2[row] = mx;
    inv2[row] = 1.f / sum;
  }
}

// Materialise P = softmax(S) (claim_before) and/or the clamped attention (claim_after)
// for callers that keep them (AdaptiveSANet.claim_before / claim_after).
// (S may be one of the outputs: the flash path forms S in the caller's claim buffer, and each
// element is read before it is overwritten)
__global__ __launch_bounds__(256) void claim_maps_kernel(
    const float* S, RowVec rv, const float* __restrict__ inv2, int mode, float* before,
    float* after, int64_t rows, int L) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * L) return;
  const int64_t r = idx / L;
  const float v = S[idx];
  const float p = expf(v - rv.m[r]) * rv.inv[r];
  if (before) before[idx] = p;
  if (after) {
    after[idx] = mode == 0
                     ? bx_apply<BX_AEA>(v, rv.m[r], rv.inv[r], rv.clamp[r], 0.f, rv.scale)
                     : bx_apply<BX_AEAR>(v, rv.m[r], rv.inv[r], rv.clamp[r], rv.m2[r], 0.f) *
                           inv2[r];
  }
}

// Elementwise AEA transform of a given attention matrix fx (AEAModule.forward's second
// half, for the function-level module API): out = f(fx, clamp_row).
__global__ __launch_bounds__(256) void aea_apply_kernel(const float* __restrict__ fx,
                                                        const float* __restrict__ clamp,
                                                        const float* __restrict__ m2,
                                                        const float* __restrict__ inv2,
                                                        float* __restrict__ out, int64_t rows,
                                                        int L, int mode, float scale) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * L) return;
  const int64_t r = idx / L;
  const float d = fx[idx] - clamp[r];
  out[idx] = mode == 0 ? 1.f / (1.f + expf(-(scale * d))) : expf(fmaxf(d, 0.f) - m2[r]) * inv2[r];
}

// f_psi's head over the B * HW rows of Z (both clamp_values* forms end here)
static int clamp_head(const float* Z, const float* w2, const float* b2, int hid, int mode,
                      float from, float interval, float* clamp, int B, int HW, hipStream_t st) {
  const int64_t rows = (int64_t)B * HW;
  clamp_head_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, st>>>(Z, w2, b2, clamp, rows, hid,
                                                               mode, from, interval);
  return launch_status("clamp_head_kernel");
}

// clamp[b, i] = head(LeakyReLU(A[b, i, :] W1^T + b1)) (AEAModule.f_psi over affinity rows)
static int clamp_values(const float* A, const float* w1, const float* b1, const float* w2,
                        const float* b2, int hid, int mode, float from, float interval,
                        float* Z, float* clamp, int B, int HW, hipStream_t st) {
  // Z[b][i][n] = sum_j A[b][i][j] W1[n][j] + b1[n]: M = HW (i), N = hid (n), K = HW (j)
  launch_gemm<LAY_RK, LAY_RK, BX_NONE>({.A = {A, HW, (int64_t)HW * HW}, .B = {w1, HW, 0},
                                        .C = {Z, hid, (int64_t)HW * hid}, .M = HW, .N = hid,
                                        .K = HW, .colbias = b1, .act = 1}, B, st);
  if (int e = launch_status("gemm_f32_kernel(Z=A W1^T)")) return e;
  return clamp_head(Z, w2, b2, hid, mode, from, interval, clamp, B, HW, st);
}

// K chunks of T = sn W1^T (C x hidden per image, K = HW): its grid is C/256 x hidden/128
// tiles per image (2 x 2 at C = 512, HW = 4096), so the pixels are split 4 ways once HW >=
// 2048 (128 -> 512 workgroups at B = 32; 0.58 ms per call before); the partials sum in order
static int clamp_t_ks(int HW) { return HW >= 2048 ? 4 : 1; }
// floats of the T region: T itself and, when split, its ks partials
static size_t clamp_t_floats(int B, int C, int HW, int hidden) {
  const int ks = clamp_t_ks(HW);
  return (size_t)B * C * hidden * (ks > 1 ? 1 + ks : 1);
}

// The clamp values without the affinity matrix: f_psi's first Linear only ever sees
// A = cn^T sn through Z = A W1^T, and Z = cn^T (sn W1^T) (sanet.py:45-66, 110): T = sn W1^T
// (C x hid per image, K = HW), then Z = cn^T T + b1 (K = C): 2 x 2 C hid HW FLOP per image
// instead of 2 HW^2 (C + hid), and the B x HW x HW affinity is never written or read (the
// same sums in another association: ~1e-7 relative from the two-GEMM form).
// T: clamp_t_floats(B, C, HW, hid) floats of scratch (T, then its K-chunk partials).
static int clamp_values_factored(const float* cn, const float* sn, const float* w1,
                                 const float* b1, const float* w2, const float* b2, int hid,
                                 int mode, float from, float interval, float* T, float* Z,
                                 float* clamp, int B, int C, int HW, hipStream_t st) {
  const int ks = clamp_t_ks(HW);
  const int kc = ks > 1 ? ((HW + ks - 1) / ks + 31) / 32 * 32 : 0;
  const int64_t per = (int64_t)C * hid, fhw = (int64_t)C * HW;
  float* Tpart = ks > 1 ? T + (size_t)B * per : T;
  // T[b][c][n] = sum_j sn[b][c][j] W1[n][j], or its ks partials over chunks of kc pixels
  launch_gemm<LAY_RK, LAY_RK, BX_NONE>({.A = {sn, HW, fhw}, .B = {w1, HW, 0},
                                        .C = {Tpart, hid, per}, .M = C, .N = hid,
                                        .K = HW, .ks = ks, .kc = kc}, B, st);
  if (int e = launch_status("gemm_f32_kernel(T=sn W1^T)")) return e;
  if (ks > 1)
    if (int e = partial_sum(Tpart, T, per, ks, B, "partial_sum_kernel(T)", st)) return e;
  // Z[b][i][n] = sum_c cn[b][c][i] T[b][c][n] + b1[n]
  launch_gemm<LAY_KR, LAY_KR, BX_NONE>({.A = {cn, HW, fhw}, .B = {T, hid, per},
                                        .C = {Z, hid, (int64_t)HW * hid}, .M = HW, .N = hid,
                                        .K = C, .colbias = b1, .act = 1}, B, st);
  if (int e = launch_status("gemm_f32_kernel(Z=cn^T T)")) return e;
  return clamp_head(Z, w2, b2, hid, mode, from, interval, clamp, B, HW, st);
}

static int col_norms(const float* c, const float* s, float* cn, float* sn, int B, int C, int HW,
                     hipStream_t st) {
  const unsigned nb = (unsigned)((int64_t)B * ((HW + 63) / 64));
  colnorm_kernel<<<nb, 256, 0, st>>>(c, cn, B, C, HW);
  colnorm_kernel<<<nb, 256, 0, st>>>(s, sn, B, C, HW);
  return launch_status("colnorm_kernel");
}

static int affinity(const float* c, const float* s, float* out, float* cn, float* sn, int B,
                    int C, int HW, hipStream_t st) {
  if (int e = col_norms(c, s, cn, sn, B, C, HW, st)) return e;
  const int64_t fhw = (int64_t)C * HW;
  // A[b][i][j] = sum_c cn[b][c][i] sn[b][c][j]
  launch_gemm<LAY_KR, LAY_KR, BX_NONE>({.A = {cn, HW, fhw}, .B = {sn, HW, fhw},
                                        .C = {out, HW, (int64_t)HW * HW}, .M = HW, .N = HW,
                                        .K = C}, B, st);
  return launch_status("gemm_f32_kernel(A=cn^T sn)");
}

// S[b][i][j] = sum_c F[b][c][i] G[b][c][j] for the n query columns i that Fq holds (all of
// them, or one chunk: F + q0), and the softmax statistics of its B * n rows
static int logits_rowstats(Mat Fq, int n, Mat G, float* S, float* rmax, float* rinv, int B, int C,
                           const char* what, hipStream_t st) {
  const int HWs = G.ld;
  launch_gemm<LAY_KR, LAY_KR, BX_NONE>({.A = Fq, .B = G, .C = {S, HWs, (int64_t)n * HWs},
                                        .M = n, .N = HWs, .K = C}, B, st);
  if (int e = launch_status(what)) return e;
  const int64_t rows = (int64_t)B * n;
  rowstats_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, st>>>(S, rmax, rinv, rows, HWs);
  return launch_status("rowstats_kernel");
}

}  // namespace rpst

using namespace rpst;

// the logits (B x HWq x HWk) and their two softmax row vectors (the two-GEMM path; the flash
// path takes none)
struct SanetLayout { float *S, *rmax, *rinv; size_t bytes; };
static SanetLayout sanet_layout(void* workspace, int B, int HWq, int HWk) {
  Carver c(workspace);
  if (B <= 0 || HWq <= 0 || HWk <= 0) return {};
  const size_t rows = (size_t)B * HWq;
  float *S = c.take(rows * HWk), *rmax = c.take(rows), *rinv = c.take(rows);
  return {S, rmax, rinv, c.bytes};
}

extern "C" size_t rpst_sanet_attention_workspace_size(int B, int HW) {
  return sanet_layout(nullptr, B, HW, HW).bytes;
}

extern "C" size_t rpst_sanet_attention_qk_workspace_size_c(int B, int C, int HWq, int HWk) {
  if (B <= 0 || C <= 0 || HWq <= 0 || HWk <= 0) return 0;
  return sanet_flash_ok(C, HWq, HWk) ? 0 : sanet_layout(nullptr, B, HWq, HWk).bytes;
}

extern "C" size_t rpst_sanet_attention_workspace_size_c(int B, int C, int HW) {
  return rpst_sanet_attention_qk_workspace_size_c(B, C, HW, HW);
}

extern "C" int rpst_sanet_attention_qk(const float* F, const float* G, const float* H, float* O,
                                       int B, int C, int HWq, int HWk, void* workspace,
                                       size_t workspace_bytes, rpst_stream_t stream) {
  RPST_REQUIRE(F && G && H && O, "sanet_attention: null pointer");
  RPST_REQUIRE(B > 0 && C > 0 && HWq > 0 && HWk > 0,
               "sanet_attention: bad shape B=%d C=%d HW=%d/%d", B, C, HWq, HWk);
  RPST_REQUIRE(B <= 65535, "sanet_attention: batch too large");
  if (sanet_flash_ok(C, HWq, HWk))
    return sanet_flash(F, G, H, O, B, C, HWq, HWk, as_stream(stream));
  const SanetLayout L = sanet_layout(workspace, B, HWq, HWk);
  RPST_REQUIRE_WS(L.bytes, "sanet_attention: workspace %zu < %zu bytes", workspace_bytes, L.bytes);
  hipStream_t st = as_stream(stream);
  const int64_t fq = (int64_t)C * HWq, fk = (int64_t)C * HWk;
  if (int e = logits_rowstats({F, HWq, fq}, HWq, {G, HWk, fk}, L.S, L.rmax, L.rinv, B, C,
                              "gemm_f32_kernel(S=F^T G)", st))
    return e;
  // O[b][c][i] = (1/l_i) sum_j H[b][c][j] exp(S[b][i][j] - m_i)
  launch_gemm<LAY_RK, LAY_RK, BX_EXP>({.A = {H, HWk, fk}, .B = {L.S, HWk, (int64_t)HWq * HWk},
                                       .C = {O, HWq, fq}, .M = C, .N = HWq, .K = HWk,
                                       .rv = {.m = L.rmax}, .sV = HWq, .colscale = L.rinv}, B, st);
  return launch_status("gemm_f32_kernel(O=H P^T)");
}

// the style at the content's size: the HWq = HWk call
extern "C" int rpst_sanet_attention(const float* F, const float* G, const float* H, float* O,
                                    int B, int C, int HW, void* workspace,
                                    size_t workspace_bytes, rpst_stream_t stream) {
  return rpst_sanet_attention_qk(F, G, H, O, B, C, HW, HW, workspace, workspace_bytes, stream);
}

// the column-normalised content and style features
struct AffinityLayout { float *cn, *sn; size_t bytes; };
static AffinityLayout affinity_layout(void* workspace, int B, int C, int HW) {
  Carver c(workspace);
  if (B <= 0 || C <= 0 || HW <= 0) return {};
  float *cn = c.take((size_t)B * C * HW), *sn = c.take((size_t)B * C * HW);
  return {cn, sn, c.bytes};
}

extern "C" size_t rpst_cosine_affinity_workspace_size(int B, int C, int HW) {
  return affinity_layout(nullptr, B, C, HW).bytes;
}

extern "C" int rpst_cosine_affinity(const float* content, const float* style, float* out,
                                    int B, int C, int HW, void* workspace,
                                    size_t workspace_bytes, rpst_stream_t stream) {
  RPST_REQUIRE(content && style && out, "cosine_affinity: null pointer");
  RPST_REQUIRE(B > 0 && C > 0 && HW > 0 && B <= 65535, "cosine_affinity: bad shape");
  const AffinityLayout L = affinity_layout(workspace, B, C, HW);
  RPST_REQUIRE_WS(L.bytes, "cosine_affinity: workspace too small");
  return affinity(content, style, out, L.cn, L.sn, B, C, HW, as_stream(stream));
}

// f_psi's hidden activations and the relu softmax's two row vectors
struct ClampLayout { float *Z, *m2, *inv2; size_t bytes; };
static ClampLayout clamp_layout(void* workspace, int B, int HW, int hidden) {
  Carver c(workspace);
  if (B <= 0 || HW <= 0 || hidden <= 0) return {};
  const size_t rows = (size_t)B * HW;
  float *Z = c.take(rows * hidden), *m2 = c.take(rows), *inv2 = c.take(rows);
  return {Z, m2, inv2, c.bytes};
}

extern "C" size_t rpst_aea_clamp_workspace_size(int B, int HW, int hidden) {
  return clamp_layout(nullptr, B, HW, hidden).bytes;
}

extern "C" int rpst_aea_clamp(const float* x, const float* fx, const float* w1,
                              const float* b1, const float* w2, const float* b2, int hidden,
                              int mode, float scale, float from, float interval, float* out_fx,
                              float* out_clamp, int B, int HW, void* workspace,
                              size_t workspace_bytes, rpst_stream_t stream) {
  RPST_REQUIRE(x && fx && w1 && b1 && w2 && b2 && out_fx && out_clamp, "aea_clamp: null pointer");
  RPST_REQUIRE(B > 0 && HW > 0 && hidden > 0 && B <= 65535, "aea_clamp: bad shape");
  RPST_REQUIRE(mode == 0 || mode == 1, "aea_clamp: mode must be 0 (aea) or 1 (relu)");
  const ClampLayout L = clamp_layout(workspace, B, HW, hidden);
  RPST_REQUIRE_WS(L.bytes, "aea_clamp: workspace too small");
  hipStream_t st = as_stream(stream);
  if (int e = clamp_values(x, w1, b1, w2, b2, hidden, mode, from, interval, L.Z, out_clamp, B,
                           HW, st))
    return e;
  const int64_t rows = (int64_t)B * HW;
  if (mode == 1) {
    rowstats_relu_kernel<false><<<(unsigned)((rows + 3) / 4), 256, 0, st>>>(
        fx, nullptr, nullptr, out_clamp, L.m2, L.inv2, rows, HW);
    if (int e = launch_status("rowstats_relu_kernel(fx)")) return e;
  }
  const int64_t n = rows * HW;
  aea_apply_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(fx, out_clamp, L.m2, L.inv2,
                                                                out_fx, rows, HW, mode, scale);
  return launch_status("aea_apply_kernel");
}

// After the logits S (B * HW rows, softmax statistics rmax / rinv) and the clamp values: the
// relu softmax statistics (mode 1; into m2 / inv2), the maps the caller keeps, its copy of the
// clamp values. S == nullptr (flash path, no map kept): the copy only.
static int adaptive_claims(const float* S, const float* rmax, const float* rinv,
                           const float* clamp, float* m2, float* inv2, float scale, int mode,
                           float* claim_value, float* claim_before, float* claim_after, int B,
                           int HW, hipStream_t st) {
  const int64_t rows = (int64_t)B * HW, n = rows * HW;
  if (S && mode == 1) {
    rowstats_relu_kernel<true><<<(unsigned)((rows + 3) / 4), 256, 0, st>>>(S, rmax, rinv, clamp,
                                                                           m2, inv2, rows, HW);
    if (int e = launch_status("rowstats_relu_kernel")) return e;
  }
  if (claim_before || claim_after) {
    const RowVec rv{.m = rmax, .inv = rinv, .clamp = clamp, .m2 = m2, .scale = scale};
    claim_maps_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(
        S, rv, inv2, mode, claim_before, claim_after, rows, HW);
    if (int e = launch_status("claim_maps_kernel")) return e;
  }
  if (claim_value &&
      hipMemcpyAsync(claim_value, clamp, sizeof(float) * rows, hipMemcpyDeviceToDevice, st) !=
          hipSuccess) {
    set_error("adaptive_attention: claim_value copy failed");
    return RPST_EHIP;
  }
  return RPST_OK;
}

struct AdaptiveLayout {
  float* S;  // T = sn W1^T (C x hidden per image) first, then the logits
  float *Z, *cn, *sn;
  float *rmax, *rinv, *clamp, *m2, *inv2;  // (B, HW) each
  float *cmax, *cinv;  // (B, HW) each: the flash path's row statistics of the kept maps
  size_t bytes;
};
static AdaptiveLayout adaptive_layout(void* workspace, int B, int C, int HW, int hidden) {
  Carver c(workspace);
  AdaptiveLayout L{};
  if (B <= 0 || C <= 0 || HW <= 0 || hidden <= 0) return L;
  const size_t rows = (size_t)B * HW, t = clamp_t_floats(B, C, HW, hidden);
  // whichever of T and S is larger; on the flash path (sanet_flash_ok) S is never formed
  L.S = c.take(sanet_flash_ok(C, HW, HW) ? t : std::max(rows * HW, t));
  L.Z = c.take(rows * hidden);
  L.cn = c.take(rows * C);
  L.sn = c.take(rows * C);
  for (float** r : {&L.rmax, &L.rinv, &L.clamp, &L.m2, &L.inv2, &L.cmax, &L.cinv})
    *r = c.take(rows);
  L.bytes = c.bytes;
  return L;
}

extern "C" size_t rpst_adaptive_attention_workspace_size(int B, int C, int HW, int hidden) {
  return adaptive_layout(nullptr, B, C, HW, hidden).bytes;
}

extern "C" int rpst_adaptive_attention(const float* F, const float* G, const float* H,
                                       const float* content, const float* style,
                                       const float* w1, const float* b1, const float* w2,
                                       const float* b2, int hidden, int mode, float scale,
                                       float from, float interval, float* O, float* claim_value,
                                       float* claim_before, float* claim_after, int B, int C,
                                       int HW, void* workspace, size_t workspace_bytes,
                                       rpst_stream_t stream) {
  RPST_REQUIRE(F && G && H && content && style && w1 && b1 && w2 && b2 && O,
               "adaptive_attention: null pointer");
  RPST_REQUIRE(B > 0 && C > 0 && HW > 0 && hidden > 0 && B <= 65535,
               "adaptive_attention: bad shape B=%d C=%d HW=%d hidden=%d", B, C, HW, hidden);
  RPST_REQUIRE(mode == 0 || mode == 1, "adaptive_attention: mode must be 0 (aea) or 1 (relu)");
  const AdaptiveLayout L = adaptive_layout(workspace, B, C, HW, hidden);
  RPST_REQUIRE_WS(L.bytes, "adaptive_attention: workspace %zu < %zu bytes", workspace_bytes,
                  L.bytes);
  hipStream_t st = as_stream(stream);
  float *S = L.S, *Z = L.Z, *cn = L.cn, *sn = L.sn;
  float *rmax = L.rmax, *rinv = L.rinv, *clamp = L.clamp, *m2 = L.m2, *inv2 = L.inv2;
  // 1. clamp values from the cosine affinity of the raw features (sanet.py:110, 45 / 66), the
  //    affinity folded into f_psi's first Linear (T in the logits' buffer, not yet written)
  if (int e = col_norms(content, style, cn, sn, B, C, HW, st)) return e;
  if (int e = clamp_values_factored(cn, sn, w1, b1, w2, b2, hidden, mode, from, interval, S, Z,
                                    clamp, B, C, HW, st))
    return e;
  const Mat Fm{F, HW, (int64_t)C * HW}, Gm{G, HW, (int64_t)C * HW}, Hm{H, HW, (int64_t)C * HW};
  if (sanet_flash_ok(C, HW, HW)) {
    // 2. pass 1: softmax row statistics of S = F^T G, S never written (rpst_flash.hip)
    if (int e = adaptive_flash_stats(F, G, B, C, HW, rmax, rinv, st)) return e;
    // the maps the caller keeps: S formed in its own (B, HW, HW) buffer and transformed in
    // place, with the row statistics of this S itself (pass 1's, from the flash kernel's
    // summation order, would put the maps ~1e-5 off the logits they transform, amplified by
    // the slope-50 sigmoid)
    float* Sx = claim_before ? claim_before : claim_after;
    if (Sx)
      if (int e = logits_rowstats(Fm, HW, Gm, Sx, L.cmax, L.cinv, B, C,
                                  "gemm_f32_kernel(S=F^T G, claims)", st))
        return e;
    if (int e = adaptive_claims(Sx, L.cmax, L.cinv, clamp, m2, inv2, scale, mode, claim_value,
                                claim_before, claim_after, B, HW, st))
      return e;
    // 3. pass 2: S recomputed per key block, Q formed in registers, O = H Q^T
    return adaptive_flash_apply(F, G, H, O, B, C, HW, rmax, rinv, clamp, mode, scale, st);
  }
  // 2. logits S = F^T G and softmax row statistics (sanet.py:114-117)
  if (int e = logits_rowstats(Fm, HW, Gm, S, rmax, rinv, B, C, "gemm_f32_kernel(S=F^T G)", st))
    return e;
  if (int e = adaptive_claims(S, rmax, rinv, clamp, m2, inv2, scale, mode, claim_value,
                              claim_before, claim_after, B, HW, st))
    return e;
  // 3. O[b][c][i] = sum_j H[b][c][j] Q[b][i][j], Q formed while S is staged (sanet.py:122-124);
  //    relu: its 1 / l2_i is the column scale
  const GemmReq g2{.A = Hm, .B = {S, HW, (int64_t)HW * HW}, .C = {O, HW, Hm.stride}, .M = C,
                   .N = HW, .K = HW,
                   .rv = {.m = rmax, .inv = rinv, .clamp = clamp, .m2 = m2, .scale = scale},
                   .sV = HW, .colscale = mode == 0 ? nullptr : inv2};
  if (mode == 0) launch_gemm<LAY_RK, LAY_RK, BX_AEA>(g2, B, st);
  else launch_gemm<LAY_RK, LAY_RK, BX_AEAR>(g2, B, st);
  return launch_status("gemm_f32_kernel(O=H Q^T)");
}

// ---- attention backward over query chunks (sanet.py:86-94, 100-138 under autograd) ------
// S and dP are formed for qc queries (full rows) at a time: per chunk S_q = F_q^T G, the row
// statistics, dH += dO_q P_q (P formed while S_q is staged), dP_q = dO_q^T H, dS_q = P (dP -
// rowsum(dP P)) in place (softmax_bwd_logits_kernel: whole rows, so every row of dS sums to
// zero to rounding), dF_q = G dS_q^T, dG += F_q dS_q; dH and dG sum the chunks in order.
// 10 HW^2 C FLOP per image whatever qc is, and S, its statistics and dS do not depend on qc
// bit for bit (the GEMM's k order does not depend on M). qc = HWc is the single pass with S and
// dP whole (rpst_sanet_attention_backward); the chunked entry points use kAttnQC and need no
// B x HW x HW workspace. (2048: the dF_q GEMM's grid is C/256 x qc/128 tiles per image -- at
// 1024 queries, C = 512 and B = 8 only 128 workgroups, and the SAModel training step ran 2.8 %
// slower than the single pass; at 2048 0.6 %, profiles/r05/attn_bwd_qc.log.)
constexpr int kAttnQC = 2048;

struct WalkScratch {
  float *S, *dP;        // [B][qc][HWs] each
  float *rmax, *rinv;   // [B][qc]
};
// The AdaptiveSANet part of the walk: the attention is Q = AEA(P, clamp), so P in the dH
// product becomes Q, and the row pass goes from dQ to dS and dc (aea_bwd_rows_kernel).
struct WalkAdaptive {
  const float* clamp;            // (B, HW) clamp values
  int mode;                      // 0 AEAModule, 1 AEALReluModule
  float scale;
  float* dc;                     // (B, HW) out: the gradient at the clamp values
  float *clq, *m2, *inv2, *dcq;  // chunk-local [B][qc] each
};
// launch_status labels of the five GEMMs, as each entry point reports them
struct WalkNames {
  const char *s, *dh, *dp, *df, *dg;
};
constexpr WalkNames kChunkNames{"gemm_f32_kernel(S_q=F_q^T G)", "gemm_f32_kernel(dH+=dO_q P_q)",
                                "gemm_f32_kernel(dP_q=dO_q^T H)",
                                "gemm_f32_kernel(dF_q=G dS_q^T)",
                                "gemm_f32_kernel(dG+=F_q dS_q)"};

static int attention_backward_walk(const float* F, const float* G, const float* H,
                                   const float* dO, float* dF, float* dG, float* dH, int B, int C,
                                   int HWc, int HWs, int qc, const WalkScratch& w,
                                   const WalkAdaptive* ad, const WalkNames& nm, hipStream_t st) {
  const int64_t fc = (int64_t)C * HWc, fs = (int64_t)C * HWs;
  const Mat Gm{G, HWs, fs}, Hm{H, HWs, fs};
  for (int q0 = 0; q0 < HWc; q0 += qc) {
    const int n = std::min(qc, HWc - q0);
    const int64_t sn = (int64_t)n * HWs, rows = (int64_t)B * n;
    const unsigned rb = (unsigned)((rows + 255) / 256), wb = (unsigned)((rows + 3) / 4);
    const Mat Fq{F + q0, HWc, fc}, dOq{dO + q0, HWc, fc}, Sq{w.S, HWs, sn}, dSq{w.dP, HWs, sn};
    if (int e = logits_rowstats(Fq, n, Gm, w.S, w.rmax, w.rinv, B, C, nm.s, st)) return e;
    RowVec rv{.m = w.rmax, .inv = w.rinv};
    if (ad) {
      rows_gather_kernel<<<rb, 256, 0, st>>>(ad->clamp, ad->clq, B, HWc, q0, n);
      if (int e = launch_status("rows_gather_kernel")) return e;
      if (ad->mode == 1) {
        rowstats_relu_kernel<true><<<wb, 256, 0, st>>>(w.S, w.rmax, w.rinv, ad->clq, ad->m2,
                                                       ad->inv2, rows, HWs);
        if (int e = launch_status("rowstats_relu_kernel")) return e;
      }
      rv = {.m = w.rmax, .inv = w.rinv, .clamp = ad->clq, .m2 = ad->m2, .scale = ad->scale,
            .inv2 = ad->inv2};
    }
    // dH += dO_q P_q (adaptive: Q_q), formed from S_q while staged (KR: its row is the k index)
    const GemmReq gh{.A = dOq, .B = Sq, .C = {dH, HWs, fs}, .M = C, .N = HWs, .K = n, .rv = rv,
                     .sV = n, .accum = q0 > 0};
    if (!ad) launch_gemm<LAY_RK, LAY_KR, BX_PROB>(gh, B, st);
    else if (ad->mode == 0) launch_gemm<LAY_RK, LAY_KR, BX_AEA>(gh, B, st);
    else launch_gemm<LAY_RK, LAY_KR, BX_AEARQ>(gh, B, st);
    if (int e = launch_status(nm.dh)) return e;
    // dP_q = dO_q^T H (adaptive: dQ_q), then the row pass writes dS_q over it
    launch_gemm<LAY_KR, LAY_KR, BX_NONE>({.A = dOq, .B = Hm, .C = {w.dP, HWs, sn}, .M = n,
                                          .N = HWs, .K = C}, B, st);
    if (int e = launch_status(nm.dp)) return e;
    if (!ad) {
      softmax_bwd_logits_kernel<<<wb, 256, 0, st>>>(w.S, w.rmax, w.rinv, w.dP, rows, HWs);
      if (int e = launch_status("softmax_bwd_logits_kernel")) return e;
    } else {
      aea_bwd_rows_kernel<<<wb, 256, 0, st>>>(w.S, rv, w.dP, ad->dcq, ad->mode, rows, HWs);
      if (int e = launch_status("aea_bwd_rows_kernel")) return e;
      rows_scatter_kernel<<<rb, 256, 0, st>>>(ad->dcq, ad->dc, B, HWc, q0, n);
      if (int e = launch_status("rows_scatter_kernel")) return e;
    }
    // dF_q = G dS_q^T
    launch_gemm<LAY_RK, LAY_RK, BX_NONE>({.A = Gm, .B = dSq, .C = {dF + q0, HWc, fc}, .M = C,
                                          .N = n, .K = HWs}, B, st);
    if (int e = launch_status(nm.df)) return e;
    // dG += F_q dS_q
    launch_gemm<LAY_RK, LAY_KR, BX_NONE>({.A = Fq, .B = dSq, .C = {dG, HWs, fs}, .M = C,
                                          .N = HWs, .K = n, .accum = q0 > 0}, B, st);
    if (int e = launch_status(nm.dg)) return e;
  }
  return RPST_OK;
}

// S_q, dP_q and their two row vectors, in this order, for chunks of qc queries
struct WalkLayout { WalkScratch w; size_t bytes; };
static WalkLayout sanet_walk_layout(void* workspace, int B, int qc, int HWs) {
  Carver c(workspace);
  if (B <= 0 || qc <= 0 || HWs <= 0) return {};
  const size_t rows = (size_t)B * qc;
  float *S = c.take(rows * HWs), *dP = c.take(rows * HWs);
  float *rmax = c.take(rows), *rinv = c.take(rows);
  return {{.S = S, .dP = dP, .rmax = rmax, .rinv = rinv}, c.bytes};
}

extern "C" size_t rpst_sanet_attention_backward_workspace_size(int B, int HWc, int HWs) {
  return sanet_walk_layout(nullptr, B, HWc, HWs).bytes;
}

extern "C" int rpst_sanet_attention_backward(const float* F, const float* G, const float* H,
                                             const float* dO, float* dF, float* dG, float* dH,
                                             int B, int C, int HWc, int HWs, void* workspace,
                                             size_t workspace_bytes, rpst_stream_t stream) {
  RPST_REQUIRE(F && G && H && dO && dF && dG && dH, "sanet_attention_backward: null pointer");
  RPST_REQUIRE(B > 0 && C > 0 && HWc > 0 && HWs > 0 && B <= 65535,
               "sanet_attention_backward: bad shape B=%d C=%d HW=%d/%d", B, C, HWc, HWs);
  const WalkLayout L = sanet_walk_layout(workspace, B, HWc, HWs);
  RPST_REQUIRE_WS(L.bytes, "sanet_attention_backward: workspace too small");
  constexpr WalkNames names{"gemm_f32_kernel(S=F^T G)", "gemm_f32_kernel(dH=dO P)",
                            "gemm_f32_kernel(dP=dO^T H)", "gemm_f32_kernel(dF=G dS^T)",
                            "gemm_f32_kernel(dG=F dS)"};
  return attention_backward_walk(F, G, H, dO, dF, dG, dH, B, C, HWc, HWs, HWc,
                                 L.w, nullptr, names, as_stream(stream));
}

extern "C" size_t rpst_sanet_attention_backward_chunked_workspace_size(int B, int C, int HWc,
                                                                       int HWs) {
  if (C <= 0) return 0;
  return sanet_walk_layout(nullptr, B, std::min(HWc, kAttnQC), HWs).bytes;
}

extern "C" int rpst_sanet_attention_backward_chunked(const float* F, const float* G,
                                                     const float* H, const float* dO, float* dF,
                                                     float* dG, float* dH, int B, int C, int HWc,
                                                     int HWs, void* workspace,
                                                     size_t workspace_bytes,
                                                     rpst_stream_t stream) {
  RPST_REQUIRE(F && G && H && dO && dF && dG && dH,
               "sanet_attention_backward_chunked: null pointer");
  RPST_REQUIRE(B > 0 && C > 0 && HWc > 0 && HWs > 0 && B <= 65535,
               "sanet_attention_backward_chunked: bad shape B=%d C=%d HW=%d/%d", B, C, HWc, HWs);
  const int qc = std::min(HWc, kAttnQC);
  const WalkLayout L = sanet_walk_layout(workspace, B, qc, HWs);
  RPST_REQUIRE_WS(L.bytes, "sanet_attention_backward_chunked: workspace too small");
  return attention_backward_walk(F, G, H, dO, dF, dG, dH, B, C, HWc, HWs, qc, L.w, nullptr,
                                 kChunkNames, as_stream(stream));
}

// K (pixel) chunks per image of the 1x1 weight gradient: the per-image GEMM has only
// ceil(Cout/256) x ceil(Cin/128) tiles (8 for the SANet's 512 x 512 convs, 64 workgroups at
// N = 8), so the pixels are split until the launch has ~512 workgroups (two per CU). A
// function of the shape only: the fixed-order partial sum stays deterministic.
static int wgrad1x1_ks(int N, int Cin, int Cout) {
  const int64_t tiles = (int64_t)((Cout + 255) / 256) * ((Cin + 127) / 128) * N;
  const int64_t ks = (512 + tiles - 1) / tiles;
  return (int)std::max<int64_t>(1, std::min<int64_t>(ks, 16));
}

// one region: part[N * wgrad1x1_ks][Cout][Cin], a dW partial per image and pixel chunk
extern "C" size_t rpst_conv1x1_wgrad_workspace_size(int N, int Cin, int Cout) {
  if (N <= 0 || Cin <= 0 || Cout <= 0) return 0;
  return sizeof(float) * (size_t)N * wgrad1x1_ks(N, Cin, Cout) * Cin * Cout;
}

extern "C" int rpst_conv1x1_wgrad(const float* x, const float* dy, float* dw, float* db, int N,
                                  int Cin, int64_t HW, int Cout, void* workspace,
                                  size_t workspace_bytes, rpst_stream_t stream) {
  RPST_REQUIRE(x && dy && dw, "conv1x1_wgrad: null pointer");
  RPST_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && HW > 0 && HW <= 0x7fffffffLL && N <= 65535,
               "conv1x1_wgrad: bad shape");
  RPST_REQUIRE_WS(rpst_conv1x1_wgrad_workspace_size(N, Cin, Cout),
                  "conv1x1_wgrad: workspace too small");
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  // part[n][co][ci] = sum_p dy[n][co][p] x[n][ci][p]
  // part[n * ks + j][co][ci] = sum over pixel chunk j of dy[n][co][p] x[n][ci][p]; chunks of
  // kc pixels (a multiple of 64, so at most ks of them and 16-B aligned)
  const int ksmax = wgrad1x1_ks(N, Cin, Cout);
  const int64_t kc = std::max<int64_t>(64, ((HW + ksmax - 1) / ksmax + 63) / 64 * 64);
  const int ks = (int)((HW + kc - 1) / kc);
  const int64_t per = (int64_t)Cout * Cin;
  launch_gemm<LAY_RK, LAY_RK, BX_NONE>({.A = {dy, (int)HW, Cout * HW}, .B = {x, (int)HW, Cin * HW},
                                        .C = {part, Cin, per}, .M = Cout, .N = Cin, .K = (int)HW,
                                        .ks = ks, .kc = (int)kc}, N, st);
  if (int e = launch_status("gemm_f32_kernel(dW=dY X^T)")) return e;
  if (int e = partial_sum(part, dw, per, N * ks, 1, "partial_sum_kernel(dW)", st)) return e;
  if (db) {
    channel_sum_kernel<<<Cout, 256, 0, st>>>(dy, db, N, Cout, HW);
    return launch_status("channel_sum_kernel");
  }
  return RPST_OK;
}

struct AdaptiveBwdLayout {
  int qc, chunks;    // queries per walk chunk; kColChunk-row chunks of the column sums
  float* Aff;        // T, then R (C x hidden per image), never the affinity
  float *Sq, *dQq;   // S and dQ of one query chunk: [B][qc][HW] each
  float *Z, *du;     // [B][HW][hidden] each
  float *cn, *sn;    // [B][C][HW] each
  float *clamp, *dc, *dt;                        // [B][HW] each
  float *rmax, *rinv, *clq, *m2, *inv2, *dcq;    // per query chunk: [B][qc] each
  float* w1part;     // [B][hidden][HW]: the per-image dW1 partials
  float* cpart;      // [chunks][3][hidden + 1]: the column-sum chunk partials
  size_t bytes;
};
static AdaptiveBwdLayout adaptive_bwd_layout(void* workspace, int B, int C, int HW,
                                             int hidden) {
  Carver c(workspace);
  AdaptiveBwdLayout L{};
  if (B <= 0 || C <= 0 || HW <= 0 || hidden <= 0) return L;
  const size_t rows = (size_t)B * HW;
  L.qc = std::min(HW, kAttnQC);
  L.chunks = (int)((rows + kColChunk - 1) / kColChunk);
  L.Aff = c.take(clamp_t_floats(B, C, HW, hidden));
  for (float** r : {&L.Sq, &L.dQq}) *r = c.take((size_t)B * L.qc * HW);
  for (float** r : {&L.Z, &L.du}) *r = c.take(rows * hidden);
  for (float** r : {&L.cn, &L.sn}) *r = c.take(rows * C);
  for (float** r : {&L.clamp, &L.dc, &L.dt}) *r = c.take(rows);
  for (float** r : {&L.rmax, &L.rinv, &L.clq, &L.m2, &L.inv2, &L.dcq})
    *r = c.take((size_t)B * L.qc);
  L.w1part = c.take(rows * hidden);
  L.cpart = c.take(3 * (size_t)(hidden + 1) * L.chunks);
  L.bytes = c.bytes;
  return L;
}

extern "C" size_t rpst_adaptive_attention_backward_workspace_size(int B, int C, int HW,
                                                                  int hidden) {
  return adaptive_bwd_layout(nullptr, B, C, HW, hidden).bytes;
}

extern "C" int rpst_adaptive_attention_backward(
    const float* F, const float* G, const float* H, const float* content, const float* style,
    const float* w1, const float* b1, const float* w2, const float* b2, int hidden, int mode,
    float scale, float from, float interval, const float* dO, float* dF, float* dG, float* dH,
    float* dw1, float* db1, float* dw2, float* db2, int B, int C, int HW, void* workspace,
    size_t workspace_bytes, rpst_stream_t stream) {
  RPST_REQUIRE(F && G && H && content && style && w1 && b1 && w2 && b2 && dO && dF && dG &&
                   dH && dw1 && db1 && dw2 && db2,
               "adaptive_attention_backward: null pointer");
  RPST_REQUIRE(B > 0 && C > 0 && HW > 0 && hidden > 0 && B <= 65535 &&
                   (int64_t)B * HW <= 0x7fffffffLL,
               "adaptive_attention_backward: bad shape B=%d C=%d HW=%d hidden=%d", B, C, HW,
               hidden);
  RPST_REQUIRE(mode == 0 || mode == 1, "adaptive_attention_backward: mode must be 0 or 1");
  const AdaptiveBwdLayout L = adaptive_bwd_layout(workspace, B, C, HW, hidden);
  RPST_REQUIRE_WS(L.bytes, "adaptive_attention_backward: workspace too small");
  hipStream_t st = as_stream(stream);
  const int64_t fhw = (int64_t)C * HW, rows = (int64_t)B * HW;
  float *Aff = L.Aff, *Z = L.Z, *du = L.du, *cn = L.cn, *sn = L.sn, *dt = L.dt;
  // forward quantities: clamp (and Z) as the forward forms them (the affinity folded into
  // f_psi's first Linear; T in the Aff region), logits, softmax / relu-softmax statistics
  if (int e = col_norms(content, style, cn, sn, B, C, HW, st)) return e;
  if (int e = clamp_values_factored(cn, sn, w1, b1, w2, b2, hidden, mode, from, interval, Aff,
                                    Z, L.clamp, B, C, HW, st))
    return e;
  // attention part over query chunks of whole rows: S_q, its softmax / relu-softmax
  // statistics, dH += dO_q Q_q, dQ_q = dO_q^T H -> dS_q and dc, dF_q = G dS_q^T, dG += F_q dS_q
  const WalkAdaptive ad{.clamp = L.clamp, .mode = mode, .scale = scale, .dc = L.dc,
                        .clq = L.clq, .m2 = L.m2, .inv2 = L.inv2, .dcq = L.dcq};
  WalkNames names = kChunkNames;
  names.dh = "gemm_f32_kernel(dH+=dO_q Q_q)";
  names.dp = "gemm_f32_kernel(dQ_q=dO_q^T H)";
  if (int e = attention_backward_walk(F, G, H, dO, dF, dG, dH, B, C, HW, HW, L.qc,
                                      {.S = L.Sq, .dP = L.dQq, .rmax = L.rmax, .rinv = L.rinv},
                                      &ad, names, st))
    return e;
  // f_psi: dt, du, then dW1 = du^T Aff over all B * HW query rows (one GEMM), the column sums
  fpsi_bwd_rows_kernel<<<(unsigned)((rows + 3) / 4), 256, 0, st>>>(Z, w2, b2, L.dc, dt, du, rows,
                                                                   hidden, mode, interval);
  if (int e = launch_status("fpsi_bwd_rows_kernel")) return e;
  // dW1 = du^T A per image with A = cn^T sn never formed: R = cn du (C x hidden, K = HW),
  // then dW1_b = R^T sn (K = C), then the B partials summed in order
  float* R = Aff;
  const int64_t nr = (int64_t)C * hidden, nw1 = (int64_t)hidden * HW;
  // R[b][c][n] = sum_i cn[b][c][i] du[b][i][n]
  launch_gemm<LAY_RK, LAY_KR, BX_NONE>({.A = {cn, HW, fhw}, .B = {du, hidden, nw1},
                                        .C = {R, hidden, nr}, .M = C, .N = hidden, .K = HW}, B,
                                       st);
  if (int e = launch_status("gemm_f32_kernel(R_b=cn_b du_b)")) return e;
  // w1part[b][n][j] = sum_c R[b][c][n] sn[b][c][j]
  launch_gemm<LAY_KR, LAY_KR, BX_NONE>({.A = {R, hidden, nr}, .B = {sn, HW, fhw},
                                        .C = {L.w1part, HW, nw1}, .M = hidden, .N = HW, .K = C}, B,
                                       st);
  if (int e = launch_status("gemm_f32_kernel(dW1_b=R_b^T sn_b)")) return e;
  if (int e = partial_sum(L.w1part, dw1, nw1, B, 1, "partial_sum_kernel(dW1)", st)) return e;
  const int chunks = L.chunks;
  fpsi_colsum_part_kernel<<<dim3((unsigned)((hidden + 1 + 255) / 256), (unsigned)chunks), 256, 0,
                            st>>>(Z, du, dt, L.cpart, rows, hidden);
  if (int e = launch_status("fpsi_colsum_part_kernel")) return e;
  fpsi_colsum_final_kernel<<<(hidden + 1 + 255) / 256, 256, 0, st>>>(L.cpart, dw2, db1, db2, chunks,
                                                                    hidden);
  return launch_status("fpsi_colsum_final_kernel");
}
