// Direct 3x3 / 1x1 convolution as an implicit GEMM on fp32 MFMA (gfx950).
//
// Replaces the ATen conv stacks of the reference hot path:
//   RP encoder / decoder  Conv2d(k3, zero pad 1) + ReLU      network/base.py:363-396
//   VGG encoder           ReflectionPad2d(1) + Conv2d + ReLU network/base.py:57-111
//                         (+ MaxPool2d(2,2,ceil) fused into the next conv's loader)
//   VGG-mirror decoder    ReflectionPad2d(1) + Conv2d [+ReLU] network/base.py:25-55,
//                         sanet.py:162-192 (+ nearest Upsample x2 fused into the loader)
//   SANet 1x1 f/g/h/out   Conv2d(k1) (+ residual add)         network/sanet.py:76-98
//   Transform merge_conv  ReflectionPad2d + Conv2d on a + up2(b) network/sanet.py:146-149
//
// GEMM view per image n:  out[co][p] = sum_k W[co][k] * X[k][p],  k = (ci, kh, kw).
//   M = Cout (block tile BM), N = pixels (block tile TH rows x 32 cols), K = Cin*KS*KS.
// Per K chunk of CK input channels the block stages into LDS
//   Ws[tap][ci][co]  : CK*KS*KS rows of BM weights (pre-packed K-major, 16-B loads)
//   Xs[ci][py][px]   : the (TH+KS-1) x (32+KS-1) input halo patch per channel, built by
//                      the loader with zero/reflect padding and pool/upsample/add applied
// and every wave runs v_mfma_f32_32x32x2_f32 over its MT x NT sub-tiles of 32x32.
// MFMA operand maps (cdna_hip_programming.md §3): lane l holds A[i=l&31][k=l>>5] and
// B[k=l>>5][j=l&31]; C row = (r&3) + 8*(r>>2) + 4*(l>>5), col = l&31. The two K values
// of one MFMA are channels ci, ci+1 at the same tap, so lane half h reads channel 2cp+h.
// Loads of chunk c+1 are issued into registers before the MFMAs of chunk c and written
// to LDS after them (issue-early / write-late), two workgroups per CU.
// Patch loader: thread -> (channel group tid>>5, column tid&31), so each half-wave reads
// a 128-B row segment and all row index math is wave-uniform (scalar).
// Numerics: exact fp32 products, fp32 accumulation (MFMA = k-ordered fmaf chain).
#include "rpst_conv.h"

#include <cstdlib>
#include <cstring>

namespace rpst {

// CKK = input channels per kernel chunk (divides the packing chunk K::CK);
// DB = double-buffered LDS (one barrier per chunk instead of two).
// GATED: the SE epilogue out = relu(gate[n][co] * (acc + bias) + res) of rpst_conv2d_gated
// (a 1x1 conv; the gate arrives in a.aux), compiled for launch_conv_gated's tiles only.
template <int KS, int BM, int TH, int WM, int WN, int INOP, int NTH, int CKK, bool DB,
          bool GATED = false>
__global__ __launch_bounds__(NTH, 2) void conv_mfma_kernel(ConvArgs a) {
  using K = ConvK<KS>;
  constexpr int PCK = K::CK, TAPS = K::TAPS;
  constexpr int CK = CKK, KCH = TAPS * CK;
  static_assert(PCK % CK == 0, "kernel chunk must divide the packing chunk");
  constexpr int OFF = (KS == 3) ? 1 : 0;
  constexpr int PH = TH + KS - 1, PW = kTW + KS - 1;
  constexpr int WTM = BM / WM;       // co per wave
  constexpr int MT = WTM / 32;       // 32-row M sub-tiles per wave
  constexpr int NT = TH / WN;        // rows (32-px N sub-tiles) per wave
  static_assert(WM * WN == NTH / kWave, "one wave per sub-tile");
  static_assert(MT >= 1 && NT >= 1 && (CK % 2) == 0, "tile");
  constexpr int NW4 = KCH * BM / 4;  // float4 weight loads per chunk
  constexpr int WLD = (NW4 + NTH - 1) / NTH;
  constexpr bool WFULL = (NW4 % NTH) == 0;
  // patch loader: NTH/32 groups of 32 lanes; a group owns CPT channels and 1/RS of
  // their rows (RS > 1 when there are more groups than channels in a chunk)
  constexpr int GROUPS = NTH / 32;
  constexpr int CPT = CK > GROUPS ? CK / GROUPS : 1;
  constexpr int RS = GROUPS > CK ? GROUPS / CK : 1;
  constexpr int CGS = GROUPS / RS;                 // distinct channel groups
  constexpr int RPT = (PH + RS - 1) / RS;          // rows per thread
  constexpr int HALO = (KS == 3) ? (2 * PH + 32 * RS - 1) / (32 * RS) : 0;  // halo loads per lane
  constexpr int XN = RPT + HALO;
  static_assert(CPT * CGS == CK, "channel split");

  constexpr int NBUF = DB ? 2 : 1;
  __shared__ float Wsb[NBUF][KCH * BM];
  __shared__ float Xsb[NBUF][CK * PH * PW];

  // block -> (co tile, image, tile row, tile col); co tile slowest so resident blocks
  // share one weight slice in L2
  int bid = blockIdx.x;
  const int tx = bid % a.tiles_x;
  bid /= a.tiles_x;
  const int ty = bid % a.tiles_y;
  bid /= a.tiles_y;
  const int n = bid % a.N;
  const int ct = bid / a.N;
  const int co0 = ct * BM;
  const int y0 = ty * TH, x0 = tx * kTW;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int h = lane >> 5, j = lane & 31;

  // ---- buffer descriptors (wave-uniform) -------------------------------------------
  const bool pooled = (INOP == RPST_IN_MAXPOOL2 || INOP == RPST_IN_UPSAMPLE2);
  const unsigned in_plane = pooled ? (unsigned)(a.Hs * a.Ws) : (unsigned)(a.H * a.W);
  const unsigned aux_plane = aux_plane_of<INOP>(a);
  const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(
      (void*)conv_in_img(a, n, (int64_t)a.Cin * in_plane), (short)0, (int)(a.Cin * in_plane * 4u),
      0x00020000);
  const __amdgpu_buffer_rsrc_t raux = aux_rsrc<INOP>(a, n);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(a.wpk + co0), (short)0, 0x7fffffff, 0x00020000);

  // weights: thread -> kernel row r = tid/(BM/4) + u*NTH/(BM/4) = (tap, cl), float4
  // column tid%(BM/4). Packed row of (tap, channel c*CK+cl) = pchunk*TAPS*PCK + tap*PCK + ci%PCK.
  // When the per-u row step RU is a multiple of CK the packed row is linear in u.
  constexpr int RU = NTH / (BM / 4);
  constexpr bool WLIN = (RU % CK) == 0;
  unsigned w_voff[WLIN ? 1 : WLD];
  unsigned w_ustride = 0;
  {
    const int r0 = tid / (BM / 4);
    if (WLIN) {
      w_voff[0] = ((unsigned)((r0 / CK) * PCK + r0 % CK) * a.Cout_pad + (tid % (BM / 4)) * 4) * 4u;
      w_ustride = (unsigned)(RU / CK) * PCK * a.Cout_pad * 4u;
    } else {
#pragma unroll
      for (int u = 0; u < (WLIN ? 1 : WLD); ++u) {
        const int r = r0 + u * RU;
        w_voff[u] = ((unsigned)((r / CK) * PCK + r % CK) * a.Cout_pad + (tid % (BM / 4)) * 4) * 4u;
      }
    }
  }

  // patch: thread -> (channel group cg, row slice rs, column jc); row math is uniform
  const int cg = (tid >> 5) % CGS, rs = (tid >> 5) / CGS, jc = tid & 31;
  int bx = x0 + jc;
  const bool bx_ok = resolve(bx, a.W, a.pad, KS == 3);
  int hy[HALO > 0 ? HALO : 1], hx[HALO > 0 ? HALO : 1];  // (HALO == 0: unused)
  bool h_ok[HALO > 0 ? HALO : 1], has_halo[HALO > 0 ? HALO : 1];
#pragma unroll
  for (int e = 0; e < HALO; ++e) {
    const int hi = jc + 32 * (rs + RS * e);
    has_halo[e] = hi < 2 * PH;
    hy[e] = y0 - OFF + (hi >> 1);
    hx[e] = (hi & 1) ? x0 + kTW : x0 - 1;
    const bool ok1 = resolve(hy[e], a.H, a.pad, true);
    const bool ok2 = resolve(hx[e], a.W, a.pad, true);
    h_ok[e] = has_halo[e] && ok1 && ok2;
  }

  floatx16 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

  constexpr int R = RawN<INOP>::R;
  u32x4 wreg[WLD];
  float xraw[CPT][XN][R];
  AdainP ap[CPT];

#define RPST_CONV_LOAD(c)                                                                   \
  {                                                                                         \
    const unsigned c0 = (unsigned)(c) * CK;                                                 \
    const unsigned wc = ((c0 / PCK) * TAPS * PCK + c0 % PCK) * a.Cout_pad * 4u;            \
    _Pragma("unroll") for (int u = 0; u < WLD; ++u) {                                       \
      const bool wv = WFULL || tid + u * NTH < NW4;                                         \
      wreg[u] = __builtin_amdgcn_raw_buffer_load_b128(                                      \
          rw, (int)(wv ? (WLIN ? w_voff[0] + u * w_ustride : w_voff[WLIN ? 0 : u]) + wc    \
                       : kOOB), 0, 0);                                                      \
    }                                                                                       \
    _Pragma("unroll") for (int q = 0; q < CPT; ++q) {                                       \
      const unsigned ch = (unsigned)((c) * CK + cg + CGS * q);                              \
      const unsigned pb = ch * in_plane * 4u, ab = ch * aux_plane * 4u;                     \
      if (INOP == RPST_IN_ADAIN || INOP == RPST_IN_ADD_ADAIN)                               \
        ap[q] = adain_params(a.aux, n, (int)ch, a);                                         \
      _Pragma("unroll") for (int i = 0; i < RPT; ++i) {                                     \
        const int py = rs * RPT + i;                                                        \
        int y = y0 - OFF + py;                                                              \
        const bool yok = resolve(y, a.H, a.pad, KS == 3) && py < PH;                        \
        fetch_raw<INOP>(xraw[q][i], rin, raux, pb, ab, y, bx, yok && bx_ok, a);             \
      }                                                                                     \
      _Pragma("unroll") for (int e = 0; e < HALO; ++e)                                      \
        fetch_raw<INOP>(xraw[q][RPT + e], rin, raux, pb, ab, hy[e], hx[e], h_ok[e], a);     \
    }                                                                                       \
  }

  const int aoff = h * BM + wm * WTM + j;
  const int boff = h * PH * PW + (wn * NT) * PW + j;

  RPST_CONV_LOAD(0)
  const int nchunks = (a.Cin + CK - 1) / CK;
  for (int c = 0; c < nchunks; ++c) {
    float* Ws = Wsb[DB ? (c & 1) : 0];
    float* Xs = Xsb[DB ? (c & 1) : 0];
#pragma unroll
    for (int u = 0; u < WLD; ++u)
      if (WFULL || tid + u * NTH < NW4)
        *reinterpret_cast<u32x4*>(Ws + 4 * (tid + u * NTH)) = wreg[u];
#pragma unroll
    for (int q = 0; q < CPT; ++q) {
      float* xs = Xs + (cg + CGS * q) * PH * PW;
      const bool chok = (int)(c * CK + cg + CGS * q) < a.Cin;
#pragma unroll
      for (int i = 0; i < RPT; ++i) {
        const int py = rs * RPT + i;
        bool ok = chok && bx_ok;
        if (INOP == RPST_IN_ADAIN || INOP == RPST_IN_ADD_ADAIN) {
          int y = y0 - OFF + py;
          ok = ok && resolve(y, a.H, a.pad, KS == 3);
        }
        const float v = combine<INOP>(xraw[q][i], ok, ap[q]);
        if ((PH % RS) == 0 || py < PH) xs[py * PW + jc + OFF] = v;
      }
#pragma unroll
      for (int e = 0; e < HALO; ++e) {
        const int hi = jc + 32 * (rs + RS * e);
        const float v = combine<INOP>(xraw[q][RPT + e], chok && h_ok[e], ap[q]);
        if (has_halo[e]) xs[(hi >> 1) * PW + ((hi & 1) ? PW - 1 : 0)] = v;
      }
    }
    __syncthreads();
    if (c + 1 < nchunks) RPST_CONV_LOAD(c + 1)
#pragma unroll
    for (int t = 0; t < TAPS; ++t) {
      const int kh = t / KS, kw = t % KS;
#pragma unroll
      for (int cp = 0; cp < CK / 2; ++cp) {
        float av[MT], bv[NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) av[mt] = Ws[aoff + (t * CK + 2 * cp) * BM + mt * 32];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          bv[nt] = Xs[boff + (2 * cp) * PH * PW + (nt + kh) * PW + kw];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt], bv[nt], acc[mt][nt],
                                                               0, 0, 0);
      }
    }
    if (!DB) __syncthreads();  // double-buffered: the next chunk's barrier suffices
  }
#undef RPST_CONV_LOAD

  // epilogue: bias, ReLU, residual, predicated coalesced stores (128 B per half-wave)
  const int x = x0 + j;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + wm * WTM + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (co >= a.Cout) continue;
      const float b = a.bias ? a.bias[co] : 0.f;
      const int64_t pbase = ((int64_t)n * a.Cout + co) * a.H * a.W;
      if constexpr (GATED) {
        // SE block tail (reference network/attention.py:58-64): one gate per (n, co) row,
        // loaded beside the bias; the residual joins before the ReLU
        const float g = a.aux[(int64_t)n * a.Cout + co];  // aux: the gate
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const int y = y0 + wn * NT + nt;
          float v = acc[mt][nt][r] + b;
          if (y < a.H && x < a.W) {
            const int64_t o = pbase + (int64_t)y * a.W + x;
            v = fmaxf(fmaf(g, v, a.res[o]), 0.f);
            a.out[o] = v;
          }
          acc[mt][nt][r] = v;
        }
        continue;
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int y = y0 + wn * NT + nt;
        float v = acc[mt][nt][r] + b;
        v = activate(v, a.relu);
        if (y < a.H && x < a.W) {
          const int64_t o = pbase + (int64_t)y * a.W + x;
          if (a.res) v += a.res[o];
          if (a.mask && !(a.mask[o] > 0.f)) v = 0.f;
          a.out[o] = v;
        }
        acc[mt][nt][r] = v;
      }
    }
  }

  // optional output statistics (AdaIN / calc_mean_std of this layer's output, fused):
  // each half-wave holds 16 output channels (r) x NT rows x 32 columns of this tile per
  // mt. Two-pass per channel: sums via a half-wave reduce-scatter (16 shuffles for 16
  // values), means broadcast back, centred sums of squares the same way -> (mean, M2)
  // per (channel, wave tile), merged in fp64 by stat_merge_kernel.
  // (compiled only for tiles with >= 4 rows per wave: with NT <= 2 hipcc keeps the
  // accumulators dynamically indexed and spills thousands of VGPRs)
  if constexpr (NT >= 4) if (a.stat_part) {
    const int rows = max(0, min(NT, a.H - (y0 + wn * NT)));
    const int cols = max(0, min(kTW, a.W - x0));
    const int cnt = rows * cols;
    const float inv = cnt > 0 ? 1.f / (float)cnt : 0.f;
    const bool xv = x < a.W;
    const int pidx = (ty * a.tiles_x + tx) * WN + wn;
    const int e = (j >> 1) & 15;  // channel index r this lane ends up holding
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      float v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float t = 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) t += (xv && nt < rows) ? acc[mt][nt][r] : 0.f;
        v[r] = t;
      }
      const float mean = halfwave_reduce_scatter16(v, j) * inv;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float mr = __shfl(mean, (h << 5) + 2 * r, 64);
        float t = 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const float d = acc[mt][nt][r] - mr;
          t += (xv && nt < rows) ? d * d : 0.f;
        }
        v[r] = t;
      }
      const float m2 = halfwave_reduce_scatter16(v, j);
      const int co = co0 + wm * WTM + mt * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
      if ((j & 1) == 0 && co < a.Cout)
        a.stat_part[((int64_t)n * a.Cout + co) * a.stat_P + pidx] = make_float2(mean, m2);
    }
  }
}

// Merge the (mean, M2) partials of one (n, c) plane in fp64 (Chan et al.), fixed order:
// lane l folds partials l, l+64, ...; then a butterfly over lanes. Writes calc_mean_std.
__global__ __launch_bounds__(256) void stat_merge_kernel(const float2* __restrict__ part,
                                                         float* __restrict__ mean,
                                                         float* __restrict__ stdv, int planes,
                                                         int P, int tiles_x, int WN, int NT,
                                                         int TW, int H, int W, float eps) {
  const int plane = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (plane >= planes) return;
  double cn = 0.0, cm = 0.0, c2 = 0.0;
  for (int p = lane; p < P; p += 64) {
    const int tile = p / WN, wn = p - tile * WN;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int rows = max(0, min(NT, H - (ty * NT * WN + wn * NT)));
    const int cols = max(0, min(TW, W - tx * TW));
    const double nb = (double)(rows * cols);
    if (nb == 0.0) continue;
    const float2 v = part[(int64_t)plane * P + p];
    const double n2 = cn + nb, d = (double)v.x - cm;
    cm += d * nb / n2;
    c2 += (double)v.y + d * d * cn * nb / n2;
    cn = n2;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double on = __shfl_xor(cn, o, 64), om = __shfl_xor(cm, o, 64), o2 = __shfl_xor(c2, o, 64);
    const double n2 = cn + on;
    if (n2 > 0.0) {
      const double d = om - cm;
      cm += d * on / n2;
      c2 += o2 + d * d * cn * on / n2;
    }
    cn = n2;
  }
  if (lane == 0) {
    float varf = (float)(cn > 1.0 ? c2 / (cn - 1.0) : __builtin_nan(""));
    mean[plane] = (float)cm;
    stdv[plane] = __fsqrt_rn(__fadd_rn(varf, eps));
  }
}

// The same merge for partials in [n][partial][co] order (ConvGeom::stat_t): a block takes 64
// consecutive channels of one image (coalesced 512-B reads per partial); its 4 waves fold
// the partials in 4 consecutive segments, each lane in order, then the 4 segment states are
// combined in segment order -- a fixed order, as above (the float2 partials are rounded the
// same; the fp64 merge tree differs from stat_merge_kernel's).
__global__ __launch_bounds__(256) void stat_merge_t_kernel(const float2* __restrict__ part,
                                                           float* __restrict__ mean,
                                                           float* __restrict__ stdv, int Cout,
                                                           int P, int tiles_x, int WN, int NT,
                                                           int TW, int H, int W, float eps) {
  const int cgroups = (Cout + 63) / 64;
  const int n = blockIdx.x / cgroups;
  const int co = (blockIdx.x - n * cgroups) * 64 + (threadIdx.x & 63);
  const int seg = threadIdx.x >> 6;
  const int per = (P + 3) / 4, p0 = seg * per, p1 = min(P, p0 + per);
  double cn = 0.0, cm = 0.0, c2 = 0.0;
  if (co < Cout) {
    const float2* pp = part + (int64_t)n * P * Cout + co;
    for (int p = p0; p < p1; ++p) {
      const int tile = p / WN, wn = p - tile * WN;
      const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
      const int rows = max(0, min(NT, H - (ty * NT * WN + wn * NT)));
      const int cols = max(0, min(TW, W - tx * TW));
      const double nb = (double)(rows * cols);
      if (nb == 0.0) continue;
      const float2 v = pp[(int64_t)p * Cout];
      const double n2 = cn + nb, d = (double)v.x - cm;
      cm += d * nb / n2;
      c2 += (double)v.y + d * d * cn * nb / n2;
      cn = n2;
    }
  }
  __shared__ double sh[3][256];
  sh[0][threadIdx.x] = cn;
  sh[1][threadIdx.x] = cm;
  sh[2][threadIdx.x] = c2;
  __syncthreads();
  if (seg != 0 || co >= Cout) return;
  for (int s = 1; s < 4; ++s) {
    const int t = s * 64 + threadIdx.x;
    const double on = sh[0][t], om = sh[1][t], o2 = sh[2][t];
    const double n2 = cn + on;
    if (n2 > 0.0) {
      const double d = om - cm;
      cm += d * on / n2;
      c2 += o2 + d * d * cn * on / n2;
    }
    cn = n2;
  }
  const float varf = (float)(cn > 1.0 ? c2 / (cn - 1.0) : __builtin_nan(""));
  mean[(int64_t)n * Cout + co] = (float)cm;
  stdv[(int64_t)n * Cout + co] = __fsqrt_rn(__fadd_rn(varf, eps));
}

// ---- weight packing: (Cout,Cin,KS,KS) -> [chunk][tap][ci_local][Cout_pad] ------------
__global__ void conv_pack_kernel(const float* __restrict__ w, float* __restrict__ pk,
                                 int Cout, int Cin, int KS, int CK, int Cout_pad,
                                 int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int taps = KS * KS;
  const int co = (int)(i % Cout_pad);
  int64_t r = i / Cout_pad;
  const int cl = (int)(r % CK);
  r /= CK;
  const int t = (int)(r % taps);
  const int c = (int)(r / taps);
  const int ci = c * CK + cl;
  float v = 0.f;
  if (ci < Cin && co < Cout) v = w[(((int64_t)co * Cin + ci) * taps) + t];
  pk[i] = v;
}

// output channels per block of the direct kernel
static int direct_bm(int Cout) { return Cout > 64 ? 128 : (Cout > 32 ? 64 : 32); }

static int pad_cout(int Cout) {
  const int bm = direct_bm(Cout);
  return (Cout + bm - 1) / bm * bm;
}

static int ck_of(int ksize) { return ksize == 3 ? ConvK<3>::CK : ConvK<1>::CK; }

// ---- narrow 3x3 layers on the VALU ------------------------------------------------------
// Cout <= 4 with Cin <= 64, or Cout <= 16 with Cin <= 4 (narrow_shape; the RP stacks'
// 3->16 input and 16->3 output convs, base.py:363-396 encoder / decoder ends, and the
// MultiScale decoder's last block 32->3, whose loader forms stylized + AdaIN(c) per element:
// INOP = RPST_IN_ADD_ADAIN, adain_rp.py:301): an MFMA tile
// pads such a layer to 32 output channels (16->3: 10x the work) or 8 input channels, so
// these run as plain FMAs instead (algorithm RPST_CONV_NARROW). Block = 4 RPT rows x 64
// columns, 256 threads (column, RPT rows); per input channel the (4 RPT+2) x 66 patch is
// staged in LDS with the padding resolved, weights [ci][tap][co] sit in LDS for the
// whole block. Same epilogue as the direct kernel: bias, activation, residual. Images go
// on grid.z: batches above 65535 images (or 65535 row tiles) take the MFMA direct path.
#ifndef RPST_NR_ALL  // 3->16 @512^2 N64 0.453 -> 0.437 (patch loads before the weight
#define RPST_NR_ALL 1  // staging) -> 0.364 ms (every channel up front): profiles/r05/narrow_ab.log
#endif
constexpr int kNrTW = 64, kNrPW = kNrTW + 2;
constexpr int kNrMaxCin = 64, kNrMaxCo = 16, kNrWl = 256 * 9;  // weight floats in LDS

static bool narrow_shape(int Cin, int Cout) {
  return (Cout <= 4 && Cin <= kNrMaxCin) || (Cout <= kNrMaxCo && Cin <= 4);
}
// the largest Cin * CO an instantiation can meet must fit the LDS weight array
static_assert(kNrMaxCin * 9 * 4 <= kNrWl && 4 * 9 * kNrMaxCo <= kNrWl, "narrow weights fit LDS");

template <int CO, int RPT, int INOP = RPST_IN_NONE>  // block = 4 RPT rows x 64 columns
__global__ __launch_bounds__(256) void conv3x3_narrow_kernel(ConvArgs a) {
  static_assert(INOP == RPST_IN_NONE || INOP == RPST_IN_ADD_ADAIN, "narrow loaders");
  constexpr bool kSkip = INOP == RPST_IN_ADD_ADAIN;
  constexpr int CK = ConvK<3>::CK, kNrTH = 4 * RPT, kNrPS = (kNrTH + 2) * kNrPW;
  __shared__ float patch[kNrPS];
  __shared__ __attribute__((aligned(8))) float wl[kNrWl];  // Cin * 9 * CO <= 2304 (narrow_shape)
  const int x0 = blockIdx.x * kNrTW, y0 = blockIdx.y * kNrTH, n = blockIdx.z;
  const int tid = threadIdx.x, col = tid & 63, rg = tid >> 6;  // output rows RPT rg ..
  // accumulators in channel pairs: one v_pk_fma_f32 per two output channels
  typedef float f2 __attribute__((ext_vector_type(2)));
  f2 acc2[RPT][CO / 2];
#pragma unroll
  for (int r = 0; r < RPT; ++r)
#pragma unroll
    for (int c2 = 0; c2 < CO / 2; ++c2) acc2[r][c2] = f2{0.f, 0.f};
  const int64_t plane = (int64_t)a.H * a.W;
  const float* in = conv_in_img(a, n, (int64_t)a.Cin * plane);
  // this thread's patch elements (slot s: element tid + 256 s), their in-plane offsets
  // resolved against the padding once (-1: zero padding / outside the patch); channel ci + 1
  // is loaded into registers while channel ci is computed (the load latency hides under
  // the FMAs instead of stalling every channel)
  constexpr int kSl = (kNrPS + 255) / 256;
  int off[kSl];
#pragma unroll
  for (int sl = 0; sl < kSl; ++sl) {
    const int i = tid + 256 * sl;
    const int r = i / kNrPW, c = i - r * kNrPW;
    int y = y0 - 1 + r, x = x0 - 1 + c;
    const bool oky = resolve(y, a.H, a.pad, true), okx = resolve(x, a.W, a.pad, true);
    off[sl] = (i < kNrPS && oky && okx) ? y * a.W + x : -1;
  }
  // ADD_ADAIN: the skip feature c (aux2) of the same shape; the element is
  // stylized + ((c - mean_c) / std_c) * std_s + mean_s (0 at zero padding)
  const float* cin = kSkip ? a.aux2 + (int64_t)n * a.Cin * plane : nullptr;
  float pre[kSl], prc[kSkip ? kSl : 1];
  auto fetch = [&](int ci) {
    const float* src = in + (int64_t)ci * plane;
#pragma unroll
    for (int sl = 0; sl < kSl; ++sl) pre[sl] = off[sl] >= 0 ? src[off[sl]] : 0.f;
    if constexpr (kSkip) {
      const float* cs = cin + (int64_t)ci * plane;
#pragma unroll
      for (int sl = 0; sl < kSl; ++sl) prc[sl] = off[sl] >= 0 ? cs[off[sl]] : 0.f;
    }
  };
  // RPST_NR_ALL: with Cin <= 4 (the 16-channel form) every channel's patch is loaded up
  // front, so no channel waits on its own loads
  constexpr bool kAll = RPST_NR_ALL && CO == 16 && !kSkip;
  float preA[kAll ? 4 : 1][kSl];
  if constexpr (kAll) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int sl = 0; sl < kSl; ++sl)
        preA[c][sl] = (c < a.Cin && off[sl] >= 0) ? in[(int64_t)c * plane + off[sl]] : 0.f;
  } else {
    fetch(0);
  }
  // direct-packed weights [ci / CK][tap][ci % CK][Cout_pad] (zero beyond Cout), staged while
  // the first patch loads are in flight
  for (int i = tid; i < a.Cin * 9 * CO; i += 256) {
    const int co = i % CO, t = (i / CO) % 9, ci = i / (9 * CO);
    wl[i] = a.wpk[((int64_t)(ci / CK) * 9 + t) * CK * a.Cout_pad + (ci % CK) * a.Cout_pad + co];
  }
  for (int ci = 0; ci < a.Cin; ++ci) {
    if constexpr (kAll) {
#pragma unroll
      for (int sl = 0; sl < kSl; ++sl)
        pre[sl] = ci == 0 ? preA[0][sl] : ci == 1 ? preA[1][sl] : ci == 2 ? preA[2][sl] : preA[3][sl];
    }
    __syncthreads();  // the previous channel's patch is consumed (first pass: weights)
    if constexpr (kSkip) {
      const AdainP pa = adain_params(a.aux, n, ci, a);
#pragma unroll
      for (int sl = 0; sl < kSl; ++sl)
        if (tid + 256 * sl < kNrPS)
          patch[tid + 256 * sl] = off[sl] >= 0 ? pre[sl] + fmaf(prc[sl] - pa.mc, pa.scale, pa.ms) : 0.f;
    } else {
#pragma unroll
      for (int sl = 0; sl < kSl; ++sl)
        if (tid + 256 * sl < kNrPS) patch[tid + 256 * sl] = pre[sl];
    }
    __syncthreads();
    if (!kAll && ci + 1 < a.Cin) fetch(ci + 1);
    float win[RPT + 2][3];
#pragma unroll
    for (int r = 0; r < RPT + 2; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) win[r][c] = patch[(RPT * rg + r) * kNrPW + col + c];
    const f2* w = reinterpret_cast<const f2*>(wl + ci * 9 * CO);
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int c2 = 0; c2 < CO / 2; ++c2) {
        const f2 wv = w[t * (CO / 2) + c2];
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
          const float xv = win[t / 3 + r][t % 3];
          acc2[r][c2] = __builtin_elementwise_fma(f2{xv, xv}, wv, acc2[r][c2]);
        }
      }
  }
  float acc[RPT][CO];
#pragma unroll
  for (int r = 0; r < RPT; ++r)
#pragma unroll
    for (int c2 = 0; c2 < CO / 2; ++c2) {
      acc[r][2 * c2] = acc2[r][c2].x;
      acc[r][2 * c2 + 1] = acc2[r][c2].y;
    }
  const int x = x0 + col;
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    const int y = y0 + RPT * rg + r;
    if (y >= a.H || x >= a.W) continue;
#pragma unroll
    for (int co = 0; co < CO; ++co) {
      if (co >= a.Cout) continue;  // (not break: the loop stays fully unrolled)
      const int64_t o = ((int64_t)n * a.Cout + co) * plane + (int64_t)y * a.W + x;
      float v = activate(acc[r][co] + (a.bias ? a.bias[co] : 0.f), a.relu);
      if (a.res) v += a.res[o];
      if (a.mask && !(a.mask[o] > 0.f)) v = 0.f;
      a.out[o] = v;
    }
  }
}

static bool heavy_loader(int in_op) {
  return in_op == RPST_IN_MAXPOOL2 || in_op == RPST_IN_ADD_UPSAMPLE2 ||
         in_op == RPST_IN_ADD_ADAIN;
}

// Direct tiles <BM, TH, WM, WN, NTH, CK, DB>: block tile BM x (TH x 32 px), WM x WN waves of
// NTH/64. BM = 128 runs 8 rows for a 3x3 conv with a one-load loader and 4 rows for a 1x1 conv
// or a 2-4-load loader (the tall tile runs out of registers there); BM = 64 / 32 run 8 rows on
// 4-channel chunks with double-buffered LDS. The measurements that settled these are in
// DESIGN.md section 3 ("Conv kernel design", the tile table).
template <int KS, int INOP>
static void launch_conv(const ConvArgs& a, int BM, hipStream_t st) {
  const int blocks = a.tiles_x * a.tiles_y * a.N * a.co_tiles;
#define RPST_LAUNCH(BM_, TH_, WM_, WN_, NTH_, CK_, DB_) \
  conv_mfma_kernel<KS, BM_, TH_, WM_, WN_, INOP, NTH_, CK_, DB_><<<blocks, NTH_, 0, st>>>(a)
  constexpr int C8 = ConvK<KS>::CK, C4 = ConvK<KS>::CK / 2;
  if (BM == 128) {
    if constexpr (KS == 1 || RawN<INOP>::R > 1) RPST_LAUNCH(128, 4, 2, 2, 256, C8, false);
    else RPST_LAUNCH(128, 8, 2, 2, 256, C8, false);
  } else if (BM == 64) {
    RPST_LAUNCH(64, 8, 1, 4, 256, C4, true);
  } else {
    RPST_LAUNCH(32, 8, 1, 4, 256, C4, true);
  }
#undef RPST_LAUNCH
}

// The gated 1x1 conv on the same tiles. tall: 16 rows for the 32 / 64-channel tiles, so a wave
// holds 4 rows and the statistics epilogue is compiled (the 8-row tile has 2 rows per wave).
// Measured at 32 -> 32, 512^2 (profiles/se_attention/stats_tile_ab.log): 0.066 / 0.538 ms at
// N = 2 / 16, against 0.066 / 0.562 ms for 8 rows on two waves of 4 rows (128 threads).
static void launch_conv_gated(const ConvArgs& a, int BM, bool tall, hipStream_t st) {
  const int blocks = a.tiles_x * a.tiles_y * a.N * a.co_tiles;
#define RPST_LAUNCH(BM_, TH_, WM_, WN_, CK_, DB_)                                           \
  conv_mfma_kernel<1, BM_, TH_, WM_, WN_, RPST_IN_NONE, 256, CK_, DB_, true><<<blocks, 256, 0, st>>>(a)
  constexpr int C8 = ConvK<1>::CK, C4 = ConvK<1>::CK / 2;
  if (BM == 128) RPST_LAUNCH(128, 4, 2, 2, C8, false);
  else if (BM == 64 && tall) RPST_LAUNCH(64, 16, 1, 4, C4, true);
  else if (tall) RPST_LAUNCH(32, 16, 1, 4, C4, true);
  else if (BM == 64) RPST_LAUNCH(64, 8, 1, 4, C4, true);
  else RPST_LAUNCH(32, 8, 1, 4, C4, true);
#undef RPST_LAUNCH
}

// the tile launch_conv runs; its statistics epilogue exists for >= 4 rows per wave only.
// tall: the 16-row tile of launch_conv_gated
static ConvTiling direct_tiling(ConvArgs& a, int ksize, int in_op, bool tall = false) {
  const int bm = direct_bm(a.Cout), ck = ck_of(ksize);
  const int th = bm == 128 ? (ksize == 1 || heavy_loader(in_op) ? 4 : 8) : (tall ? 16 : 8);
  const int wn = bm == 128 ? 2 : 4;  // waves along the tile rows
  a.Cout_pad = pad_cout(a.Cout);
  a.nchunks = (a.Cin + ck - 1) / ck;
  a.tiles_x = (a.W + kTW - 1) / kTW;
  a.tiles_y = (a.H + th - 1) / th;
  a.co_tiles = a.Cout_pad / bm;
  a.stat_P = a.tiles_x * a.tiles_y * wn;
  return {(int64_t)a.tiles_x * a.tiles_y * a.N * a.co_tiles, 256, th / wn, wn, kTW, false};
}

// Narrow kernel: 64 columns x 4 rpt rows per block, images on grid.z and row tiles on grid.y.
// rpt (rows per thread): 4 for Cout <= 4 (16->3: 0.307 vs 0.348 ms; RPST_CONV_NARROW_RPT=2
// overrides), 2 for Cout <= 16 (3->16 at 4 rows spills to scratch: 1.47 vs 0.51 ms). It reads
// the direct weight image (Cout_pad) and has no statistics epilogue.
static int narrow_rpt(int Cout, const ConvMode& m) {
  return Cout <= 4 && m.narrow_rpt != 2 ? 4 : 2;
}
static ConvTiling narrow_tiling(ConvArgs& a, int rpt) {
  const int rows = 4 * rpt;
  a.Cout_pad = pad_cout(a.Cout);
  a.nchunks = (a.Cin + ConvK<3>::CK - 1) / ConvK<3>::CK;
  a.tiles_x = (a.W + kNrTW - 1) / kNrTW;
  a.tiles_y = (a.H + rows - 1) / rows;
  a.co_tiles = 1;
  a.stat_P = 0;
  return {(int64_t)a.tiles_x * a.tiles_y * a.N, 256, 0, 0, kNrTW, false};
}

// rpst_conv2d_set_precise: at 1 this thread's launches keep to F(2x2) where F(4x4) would
// run; at 2 F(4x4) runs, on its 32-channel form only (wino4q_applies)
static thread_local int t_conv_precise = 0;
// rpst_conv2d_set_quarter: -1 (default) follows RPST_W4Q, read per launch
static thread_local int t_conv_quarter = -1;

// The calling thread's switches and the environment's, read once per ABI call.
static ConvMode conv_mode() {
  ConvMode m{};
  m.precise = t_conv_precise;
  const char* e = getenv("RPST_W4Q");
  const int q = t_conv_quarter >= 0 ? t_conv_quarter : ((e && *e) ? atoi(e) : 1);
  m.quarter = q == 2 ? 2 : q != 0;
  e = getenv("RPST_CONV_ALGO");  // direct|winograd|winograd4 (tests, A/B benches)
  m.algo = -1;
  if (e && e[0] == 'd') m.algo = RPST_CONV_DIRECT;
  else if (e && !strcmp(e, "winograd")) m.algo = RPST_CONV_WINOGRAD;
  else if (e && !strcmp(e, "winograd4")) m.algo = RPST_CONV_WINOGRAD4;
  e = getenv("RPST_CONV_NARROW");  // A/B switch
  m.narrow = !(e && *e && atoi(e) == 0);
  e = getenv("RPST_CONV_NARROW_RPT");
  m.narrow_rpt = (e && *e && atoi(e) == 2) ? 2 : 0;
  return m;
}

// Algorithm for a 3x3 conv: Winograd F(4x4,3x3) (rpst_wino4.hip) for the loader
// operators it implements, F(2x2,3x3) (rpst_wino.hip) for the others, the direct implicit
// GEMM for the 16-wide layers and every 1x1. m.algo overrides (winograd4 falls back to
// winograd where unsupported). What a launch needs may still move the choice: conv_plan.
static int conv_algo(int Cout, int Cin, int Hs, int Ws, int ksize, int in_op, const ConvMode& m) {
  if (ksize != 3) return RPST_CONV_DIRECT;
  const bool w4 = wino4_supports(in_op) && wino4_fits(1, Cin, Hs, Ws, in_op);
  const bool nr = (in_op == RPST_IN_NONE || (in_op == RPST_IN_ADD_ADAIN && Cout <= 4)) &&
                  narrow_shape(Cin, Cout) && m.narrow;
  if (m.algo == RPST_CONV_DIRECT) return nr ? RPST_CONV_NARROW : RPST_CONV_DIRECT;
  if (m.algo == RPST_CONV_WINOGRAD) return RPST_CONV_WINOGRAD;
  if (m.algo == RPST_CONV_WINOGRAD4) return w4 ? RPST_CONV_WINOGRAD4 : RPST_CONV_WINOGRAD;
  // measured (profiles/r01_bench_conv_wino4.log): F(4x4) wins every layer with >= 16 input
  // channels it supports, the 16-wide 32->16 decoder layer included; the narrow shapes
  // (3->16 / 16->3 of the RP stacks, <= 4-channel outputs) run on the VALU kernel (3->16
  // 0.44 / 16->3 0.16 ms vs 0.57 / 0.64 on MFMA tiles; the VGG decoders' 64->3 reflect at
  // 512^2, N = 32: 0.63 ms vs 1.05 on F(4x4), profiles/r04/narrow64.log); the wider 3-channel first convs
  // (VGG 3->64, MultiScale 3->32) run on F(4x4): 3->64 reflect at 512^2, N = 64: 1.25 ms vs
  // 1.59 direct and 2.49 on the VALU kernel (tools/bench_conv.py); other inputs below 16
  // channels, and precise mode, stay direct
  if (nr) return RPST_CONV_NARROW;
  if (Cin <= 4 && w4 && m.precise != 1) return RPST_CONV_WINOGRAD4;
  if (Cin < 16) return RPST_CONV_DIRECT;
  if (w4 && m.precise != 1) return RPST_CONV_WINOGRAD4;
  if (w4) return RPST_CONV_WINOGRAD;  // precise mode, same shapes as F(4x4)
  return Cout >= 32 ? RPST_CONV_WINOGRAD : RPST_CONV_DIRECT;
}

static size_t direct_packed_floats(int Cout, int Cin, int ksize) {
  const int ck = ck_of(ksize);
  const size_t nch = (size_t)(Cin + ck - 1) / ck;
  return nch * ksize * ksize * ck * (size_t)pad_cout(Cout);
}

// the shape fields of a launch: H, W are the logical (post-in_op) size
static ConvArgs conv_shape(int N, int Cin, int Hs, int Ws, int Cout, int in_op) {
  ConvArgs a{};
  a.N = N;
  a.Cin = Cin;
  a.Hs = a.H = Hs;
  a.Ws = a.W = Ws;
  a.Cout = Cout;
  if (in_op == RPST_IN_MAXPOOL2) {
    a.H = (Hs + 1) / 2;
    a.W = (Ws + 1) / 2;
  } else if (in_op == RPST_IN_UPSAMPLE2) {
    a.H = 2 * Hs;
    a.W = 2 * Ws;
  }
  return a;
}

// What a call needs of its kernel: the statistics epilogue, the residual epilogue, and
// whether it offers per-image weights to fold into (an RPST_IN_ADAIN loader with a workspace,
// or rpst_conv2d_mix's T / offset).
struct ConvNeeds {
  bool stats, residual, fold;
  bool gated;  // the SE epilogue (rpst_conv2d_gated): a 1x1 conv, always a direct tile
};

// Everything decided about one launch, in one place. The launch, the statistics merge and the
// query functions (rpst_conv2d_algorithm / _quarter / _grid_threads, workspace sizes) read it.
struct ConvPlan {
  int algo;      // the RPST_CONV_* that runs, downgrades applied
  bool quarter;  // F(4x4): the position-quarter form (rpst_wino4q.hip)
  bool fold;     // F(4x4): per-image weights and border biases (wino4_fold / wino4_mix)
  int op;        // the loader operator that launches: RPST_IN_NONE once AdaIN folds
  int rpt;       // narrow: rows per thread
  size_t wofs;   // floats from the packed buffer's start to the weight image that launches
  bool tall;     // gated conv: the 16-row tile, whose statistics epilogue exists
  ConvTiling t;
};

// a: shape fields set (conv_shape); its tiling fields are filled for the planned kernel.
static ConvPlan conv_plan(ConvArgs& a, int ksize, int in_op, const ConvMode& m, ConvNeeds need) {
  ConvPlan p{};
  p.op = in_op;
  p.algo = conv_algo(a.Cout, a.Cin, a.Hs, a.Ws, ksize, in_op, m);
  if (p.algo == RPST_CONV_NARROW) {
    p.rpt = narrow_rpt(a.Cout, m);
    p.t = narrow_tiling(a, p.rpt);
    // no statistics epilogue; grid.y / grid.z hold <= 65535 row tiles / images
    if (need.stats || a.N > 65535 || a.tiles_y > 65535) p.algo = RPST_CONV_DIRECT;
  }
  // the residual epilogue (SANet out_conv, sanet.py:97-98) exists on the direct and narrow
  // kernels only
  if (need.residual && (p.algo == RPST_CONV_WINOGRAD || p.algo == RPST_CONV_WINOGRAD4))
    p.algo = RPST_CONV_DIRECT;
  if (p.algo == RPST_CONV_WINOGRAD4) {
    // AdaIN in the weights (not with the statistics epilogue: that layer keeps the loader)
    p.fold = need.fold && !need.stats && a.H >= 2 && a.W >= 2;
    if (p.fold) p.op = RPST_IN_NONE;
    p.quarter = wino4q_applies(a.Cin, a.Cout, p.op, m);
    // the F(4x4) image follows the direct and F(2x2) ones, the quarter form's follows it
    p.wofs = direct_packed_floats(a.Cout, a.Cin, ksize) + wino_packed_floats(a.Cout, a.Cin) +
             (p.quarter ? wino4_packed_floats(a.Cout, a.Cin) : 0);
    p.t = p.quarter ? wino4q_tiling(a) : wino4_tiling(a);
  } else if (p.algo == RPST_CONV_WINOGRAD) {
    p.wofs = direct_packed_floats(a.Cout, a.Cin, ksize);
    p.t = wino_tiling(a, in_op);
  } else if (p.algo == RPST_CONV_DIRECT) {
    p.tall = need.gated && need.stats && direct_bm(a.Cout) != 128;
    p.t = direct_tiling(a, ksize, in_op, p.tall);
  }
  return p;
}

// the largest `bytes(mode)` over every precise level and quarter setting (the thread's other
// switches as they are): a workspace sized under one setting serves a launch under any other
template <class F>
static size_t max_over_modes(ConvMode m, F bytes) {
  size_t best = 0;
  for (m.precise = 0; m.precise < 3; ++m.precise)
    for (m.quarter = 0; m.quarter < 3; ++m.quarter) {
      const size_t b = bytes(m);
      best = b > best ? b : best;
    }
  return best;
}

}  // namespace rpst

using namespace rpst;

// 3x3 weights are packed three times: the direct image, the F(2x2) Winograd image and
// the F(4x4) Winograd image (the algorithm is chosen per launch; all are small).
extern "C" size_t rpst_conv2d_packed_size(int Cout, int Cin, int ksize) {
  if (Cout <= 0 || Cin <= 0 || (ksize != 1 && ksize != 3)) return 0;
  size_t f = direct_packed_floats(Cout, Cin, ksize);
  if (ksize == 3)
    f += wino_packed_floats(Cout, Cin) + wino4_packed_floats(Cout, Cin) +
         wino4q_packed_floats(Cout, Cin);
  return f * sizeof(float);
}

// the plan of a plain launch of this shape under the calling thread's mode
static ConvPlan query_plan(int N, int Cin, int Hs, int Ws, int Cout, int ksize, int in_op) {
  ConvArgs a = conv_shape(N, Cin, Hs, Ws, Cout, in_op);
  return conv_plan(a, ksize, in_op, conv_mode(), {});
}

extern "C" int64_t rpst_conv2d_grid_threads(int N, int Cin, int Hs, int Ws, int Cout,
                                            int ksize, int in_op) {
  if (N <= 0 || Cin <= 0 || Hs <= 0 || Ws <= 0 || Cout <= 0 || (ksize != 1 && ksize != 3))
    return 0;
  const ConvTiling t = query_plan(N, Cin, Hs, Ws, Cout, ksize, in_op).t;
  return t.blocks * t.nth;
}

extern "C" int rpst_conv2d_set_precise(int on) {
  const int old = t_conv_precise;
  t_conv_precise = on == 2 ? 2 : on != 0;
  return old;
}

extern "C" int rpst_conv2d_set_quarter(int mode) {
  const int old = t_conv_quarter;
  t_conv_quarter = mode < 0 ? -1 : (mode > 2 ? 2 : mode);
  return old;
}

extern "C" int rpst_conv2d_algorithm(int Cout, int Cin, int Hs, int Ws, int ksize, int in_op) {
  return query_plan(1, Cin, Hs, Ws, Cout, ksize, in_op).algo;
}

extern "C" int rpst_conv2d_quarter(int Cout, int Cin, int Hs, int Ws, int ksize, int in_op) {
  return query_plan(1, Cin, Hs, Ws, Cout, ksize, in_op).quarter ? 1 : 0;
}

extern "C" int rpst_conv2d_pack(const float* weight, float* packed, int Cout, int Cin,
                                int ksize, rpst_stream_t stream) {
  RPST_REQUIRE(weight && packed, "conv2d_pack: null pointer");
  RPST_REQUIRE(Cout > 0 && Cin > 0, "conv2d_pack: bad channels");
  RPST_REQUIRE(ksize == 1 || ksize == 3, "conv2d_pack: ksize must be 1 or 3, got %d", ksize);
  const int64_t total = (int64_t)direct_packed_floats(Cout, Cin, ksize);
  const int threads = 256;
  conv_pack_kernel<<<(unsigned)((total + threads - 1) / threads), threads, 0,
                     as_stream(stream)>>>(weight, packed, Cout, Cin, ksize, ck_of(ksize),
                                          pad_cout(Cout), total);
  if (int e = launch_status("conv_pack_kernel")) return e;
  if (ksize == 3) {
    if (int e = wino_pack(weight, packed + total, Cout, Cin, as_stream(stream))) return e;
    float* w4 = packed + total + wino_packed_floats(Cout, Cin);
    if (int e = wino4_pack(weight, w4, Cout, Cin, as_stream(stream))) return e;
    return wino4q_pack(weight, w4 + wino4_packed_floats(Cout, Cin), Cout, Cin, as_stream(stream));
  }
  return RPST_OK;
}

// out = mask > 0 ? out : 0 in place (threshold_backward after a kernel without the mask
// epilogue)
__global__ __launch_bounds__(256) void mask_apply_kernel(float* __restrict__ out,
                                                         const float* __restrict__ mask,
                                                         int64_t n) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i + 3 < n && ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(mask)) & 15) == 0) {
    float4 v = *reinterpret_cast<float4*>(out + i);
    const float4 m = *reinterpret_cast<const float4*>(mask + i);
    if (!(m.x > 0.f)) v.x = 0.f;
    if (!(m.y > 0.f)) v.y = 0.f;
    if (!(m.z > 0.f)) v.z = 0.f;
    if (!(m.w > 0.f)) v.w = 0.f;
    *reinterpret_cast<float4*>(out + i) = v;
  } else {
    for (int64_t j = i; j < n && j < i + 4; ++j)
      if (!(mask[j] > 0.f)) out[j] = 0.f;
  }
}

// One conv launch as the entry points ask for it; what a call does not set is null / zero.
struct ConvReq {
  const float* input;
  const float* aux;   // the loader operator's second tensor / AdaIN statistics
  const float* aux2;  // RPST_IN_ADD_ADAIN: the content feature
  const float* packed_weight;
  const float* bias;
  const float* residual;
  float* out;
  int N, Cin, Hs, Ws, Cout, ksize, pad_mode, in_op, relu;
  hipStream_t st;
  float2* stat_part;  // statistics partials (rpst_conv2d_stats)
  float* fold_ws;     // workspace for per-image folded weights (RPST_IN_ADAIN, or T / offset)
  int skip_from;      // ConvArgs::skip_from
  const float* in2;   // ConvArgs::in2, in2_from
  int in2_from;
  const float* mask;  // ConvArgs::mask
  int pool_out;       // ConvArgs::pool_out
  const float* gate;  // rpst_conv2d_gated: the SE gate, carried in ConvArgs::aux
  // rpst_conv2d_mix: conv(pad(T_n x + offset_n)) with both folded into fold_ws (wino4_mix);
  // the caller has checked that the plan folds
  const double* T;
  const double* offset;
};

// validates r, fills the kernel arguments and plans the launch
static int conv_prepare(const ConvReq& r, const ConvMode& m, ConvArgs& a, ConvPlan& p) {
  RPST_REQUIRE(r.input && r.packed_weight && r.out, "conv2d: null pointer");
  RPST_REQUIRE(r.N > 0 && r.Cin > 0 && r.Cout > 0 && r.Hs > 0 && r.Ws > 0, "conv2d: bad shape");
  RPST_REQUIRE(r.ksize == 1 || r.ksize == 3, "conv2d: ksize must be 1 or 3, got %d", r.ksize);
  RPST_REQUIRE(r.pad_mode == RPST_PAD_ZERO || r.pad_mode == RPST_PAD_REFLECT, "conv2d: bad pad");
  RPST_REQUIRE(r.in_op >= RPST_IN_NONE && r.in_op <= RPST_IN_ADD_ADAIN, "conv2d: bad in_op");
  RPST_REQUIRE(r.relu >= RPST_ACT_NONE && r.relu <= RPST_ACT_LRELU, "conv2d: bad activation %d", r.relu);
  RPST_REQUIRE(!(r.mask && r.stat_part), "conv2d: the mask epilogue has no statistics");
  RPST_REQUIRE(!(r.pool_out && (r.stat_part || r.mask || r.residual)),
               "conv2d: the pooled output has no statistics / mask / residual epilogue");
  if (r.in_op == RPST_IN_ADD_UPSAMPLE2) {
    RPST_REQUIRE(r.aux != nullptr, "conv2d: ADD_UPSAMPLE2 needs aux");
    RPST_REQUIRE((r.Hs % 2) == 0 && (r.Ws % 2) == 0, "conv2d: ADD_UPSAMPLE2 needs even H,W");
  } else if (r.in_op == RPST_IN_ADAIN) {
    RPST_REQUIRE(r.aux != nullptr, "conv2d: ADAIN needs aux (AdaIN statistics)");
  } else if (r.in_op == RPST_IN_ADD_ADAIN) {
    RPST_REQUIRE(r.aux != nullptr && r.aux2 != nullptr,
                 "conv2d: ADD_ADAIN needs the content feature and AdaIN statistics");
  }
  a = conv_shape(r.N, r.Cin, r.Hs, r.Ws, r.Cout, r.in_op);
  a.in = r.input;
  a.in2 = r.in2;
  a.in2_from = r.in2 ? r.in2_from : 0;
  a.aux = r.aux;
  a.aux2 = r.aux2;
  a.bias = r.bias;
  a.res = r.residual;
  a.out = r.out;
  a.pad = r.pad_mode;
  a.relu = r.relu;
  a.stat_part = r.stat_part;
  a.skip_from = r.skip_from;
  a.mask = r.mask;
  a.pool_out = r.pool_out;
  if (r.gate) a.aux = r.gate;  // the gated 1x1 kernel has no loader operand
  RPST_REQUIRE(!r.gate || (r.ksize == 1 && r.residual && r.in_op == RPST_IN_NONE && !r.mask &&
                           !r.pool_out && !r.in2),
               "conv2d_gated: a 1x1 conv with a residual and a plain input only");
  if (r.ksize == 3 && r.pad_mode == RPST_PAD_REFLECT)
    RPST_REQUIRE(a.H >= 2 && a.W >= 2, "conv2d: reflect padding needs H,W >= 2");
  RPST_REQUIRE((int64_t)r.N * (r.Cout > r.Cin ? r.Cout : r.Cin) * a.H * a.W < (1LL << 40),
               "conv2d: tensor too large");
  // per-image input (plus one chunk of channel padding) must be addressable by a 31-bit
  // buffer offset
  RPST_REQUIRE(((int64_t)r.Cin + 16) * r.Hs * r.Ws * 4 < (1LL << 31),
               "conv2d: one image's input exceeds 2 GiB");
  const bool fold = r.fold_ws && (r.in_op == RPST_IN_ADAIN || r.T);
  p = conv_plan(a, r.ksize, r.in_op, m,
                {r.stat_part != nullptr, r.residual != nullptr, fold, r.gate != nullptr});
  RPST_REQUIRE(!r.pool_out || p.algo == RPST_CONV_WINOGRAD4,
               "conv2d_pool: the pooled-output epilogue exists on the F(4x4) path only "
               "(rpst_conv2d_algorithm == RPST_CONV_WINOGRAD4)");
  RPST_REQUIRE(!r.T || p.fold, "conv2d_mix: T / offset on a launch that does not fold them");
  a.wpk = r.packed_weight + p.wofs;
  return RPST_OK;
}

template <int KS, int INOP>
static int launch_direct(const ConvArgs& a, hipStream_t st) {
  launch_conv<KS, INOP>(a, direct_bm(a.Cout), st);
  return launch_status("conv_mfma_kernel");
}

static int conv_launch(const ConvReq& r, ConvArgs& a, const ConvPlan& p) {
  hipStream_t st = r.st;
  if (p.algo == RPST_CONV_WINOGRAD4) {
    if (p.fold) {
      const int e = r.T ? wino4_mix(a, p.quarter, r.T, r.offset, r.packed_weight,
                                    pad_cout(r.Cout), r.fold_ws, st)
                        : wino4_fold(a, p.quarter, r.packed_weight, pad_cout(r.Cout), r.fold_ws, st);
      if (e) return e;
    }
    if (int e = p.quarter ? wino4q_launch(a, p.op, st) : wino4_launch(a, p.op, st)) return e;
    if (r.mask) {  // F(4x4)'s epilogue has no mask: threshold the output in a second pass
      const int64_t n = (int64_t)r.N * r.Cout * a.H * a.W;
      mask_apply_kernel<<<(unsigned)((n + 1023) / 1024), 256, 0, st>>>(r.out, r.mask, n);
      return launch_status("mask_apply_kernel");
    }
    return RPST_OK;
  }
  if (p.algo == RPST_CONV_WINOGRAD) return wino_launch(a, r.in_op, st);
  if (p.algo == RPST_CONV_NARROW) {
    RPST_REQUIRE(r.Cin * 9 * (r.Cout <= 4 ? 4 : 16) <= kNrWl, "conv2d: narrow weights exceed LDS");
    const dim3 grid((unsigned)a.tiles_x, (unsigned)a.tiles_y, r.N);
    if (r.in_op == RPST_IN_ADD_ADAIN) {
      RPST_REQUIRE(r.Cout <= 4, "conv2d: narrow skip-AdaIN conv needs Cout <= 4");
      if (p.rpt == 4) conv3x3_narrow_kernel<4, 4, RPST_IN_ADD_ADAIN><<<grid, 256, 0, st>>>(a);
      else conv3x3_narrow_kernel<4, 2, RPST_IN_ADD_ADAIN><<<grid, 256, 0, st>>>(a);
    } else if (r.Cout <= 4) {
      if (p.rpt == 4) conv3x3_narrow_kernel<4, 4><<<grid, 256, 0, st>>>(a);
      else conv3x3_narrow_kernel<4, 2><<<grid, 256, 0, st>>>(a);
    } else {
      conv3x3_narrow_kernel<16, 2><<<grid, 256, 0, st>>>(a);
    }
    return launch_status("conv3x3_narrow_kernel");
  }
  RPST_REQUIRE(p.t.blocks <= 0x7fffffffLL, "conv2d: grid too large");
  if (r.ksize == 1) {
    RPST_REQUIRE(r.in_op == RPST_IN_NONE, "conv2d: 1x1 conv supports in_op NONE only");
    if (r.gate) {
      launch_conv_gated(a, direct_bm(a.Cout), p.tall, st);
      return launch_status("conv_mfma_kernel (gated)");
    }
    return launch_direct<1, RPST_IN_NONE>(a, st);
  }
  switch (r.in_op) {
    case RPST_IN_MAXPOOL2: return launch_direct<3, RPST_IN_MAXPOOL2>(a, st);
    case RPST_IN_UPSAMPLE2: return launch_direct<3, RPST_IN_UPSAMPLE2>(a, st);
    case RPST_IN_ADD_UPSAMPLE2: return launch_direct<3, RPST_IN_ADD_UPSAMPLE2>(a, st);
    case RPST_IN_ADAIN: return launch_direct<3, RPST_IN_ADAIN>(a, st);
    case RPST_IN_ADD_ADAIN: return launch_direct<3, RPST_IN_ADD_ADAIN>(a, st);
    default: return launch_direct<3, RPST_IN_NONE>(a, st);
  }
}

static int conv_common(const ConvReq& r, const ConvMode& m) {
  ConvArgs a;
  ConvPlan p;
  if (int e = conv_prepare(r, m, a, p)) return e;
  return conv_launch(r, a, p);
}

extern "C" int rpst_conv2d(const float* input, const float* aux, const float* packed_weight,
                           const float* bias, const float* residual, float* out, int N,
                           int Cin, int Hs, int Ws, int Cout, int ksize, int pad_mode,
                           int in_op, int relu, rpst_stream_t stream) {
  RPST_REQUIRE(in_op != RPST_IN_ADD_ADAIN, "conv2d: ADD_ADAIN goes through rpst_conv2d_skip_adain");
  return conv_common({.input = input, .aux = aux, .packed_weight = packed_weight, .bias = bias,
                      .residual = residual, .out = out, .N = N, .Cin = Cin, .Hs = Hs, .Ws = Ws,
                      .Cout = Cout, .ksize = ksize, .pad_mode = pad_mode, .in_op = in_op,
                      .relu = relu, .st = as_stream(stream)},
                     conv_mode());
}

extern "C" int rpst_conv2d_pair(const float* input, const float* input2, int n1,
                                const float* packed_weight, const float* bias, float* out, int N,
                                int Cin, int Hs, int Ws, int Cout, int ksize, int pad_mode,
                                int relu, rpst_stream_t stream) {
  RPST_REQUIRE(n1 > 0 && n1 <= N, "conv2d_pair: need 0 < n1 <= N (n1=%d, N=%d)", n1, N);
  RPST_REQUIRE(n1 == N || input2, "conv2d_pair: null second input");
  return conv_common({.input = input, .packed_weight = packed_weight, .bias = bias, .out = out,
                      .N = N, .Cin = Cin, .Hs = Hs, .Ws = Ws, .Cout = Cout, .ksize = ksize,
                      .pad_mode = pad_mode, .in_op = RPST_IN_NONE, .relu = relu,
                      .st = as_stream(stream), .in2 = n1 < N ? input2 : nullptr,
                      .in2_from = n1 < N ? n1 : 0},
                     conv_mode());
}

extern "C" int rpst_conv2d_masked(const float* input, const float* packed_weight,
                                  const float* bias, const float* mask, float* out, int N,
                                  int Cin, int Hs, int Ws, int Cout, int ksize, int pad_mode,
                                  rpst_stream_t stream) {
  RPST_REQUIRE(mask, "conv2d_masked: null mask");
  return conv_common({.input = input, .packed_weight = packed_weight, .bias = bias, .out = out,
                      .N = N, .Cin = Cin, .Hs = Hs, .Ws = Ws, .Cout = Cout, .ksize = ksize,
                      .pad_mode = pad_mode, .in_op = RPST_IN_NONE, .relu = RPST_ACT_NONE,
                      .st = as_stream(stream), .mask = mask},
                     conv_mode());
}

extern "C" int rpst_conv2d_pool(const float* input, const float* aux, const float* packed_weight,
                                const float* bias, float* out, int N, int Cin, int Hs, int Ws,
                                int Cout, int ksize, int pad_mode, int in_op, int relu,
                                rpst_stream_t stream) {
  RPST_REQUIRE(in_op != RPST_IN_ADD_ADAIN, "conv2d_pool: ADD_ADAIN has no pooled form");
  return conv_common({.input = input, .aux = aux, .packed_weight = packed_weight, .bias = bias,
                      .out = out, .N = N, .Cin = Cin, .Hs = Hs, .Ws = Ws, .Cout = Cout,
                      .ksize = ksize, .pad_mode = pad_mode, .in_op = in_op, .relu = relu,
                      .st = as_stream(stream), .pool_out = 1},
                     conv_mode());
}

static bool bad_shape(int N, int Cin, int Hs, int Ws, int Cout, int ksize) {
  return N <= 0 || Cin <= 0 || Hs <= 0 || Ws <= 0 || Cout <= 0 || (ksize != 1 && ksize != 3);
}

// does a launch that offers per-image weights (an RPST_IN_ADAIN loader with a workspace, or
// rpst_conv2d_mix with in_op NONE) fold them under mode m
static bool plan_folds(int N, int Cin, int Hs, int Ws, int Cout, int ksize, int in_op,
                       const ConvMode& m) {
  ConvArgs a = conv_shape(N, Cin, Hs, Ws, Cout, in_op);
  return conv_plan(a, ksize, in_op, m, {false, false, true}).fold;
}

// workspace of the F(4x4) conv with RPST_IN_ADAIN folded into per-image weights (0 for every
// other layer): the same under every precise level and quarter setting
static size_t fold_bytes(int N, int Cin, int Hs, int Ws, int Cout, int ksize, int in_op,
                         const ConvMode& mode) {
  if (bad_shape(N, Cin, Hs, Ws, Cout, ksize) || in_op != RPST_IN_ADAIN) return 0;
  return max_over_modes(mode, [&](const ConvMode& m) {
    return plan_folds(N, Cin, Hs, Ws, Cout, ksize, in_op, m)
               ? wino4_fold_floats(N, Cin, Cout) * sizeof(float)
               : 0;
  });
}

extern "C" size_t rpst_conv2d_workspace_size(int N, int Cin, int Hs, int Ws, int Cout, int ksize,
                                             int in_op) {
  return fold_bytes(N, Cin, Hs, Ws, Cout, ksize, in_op, conv_mode());
}

extern "C" int rpst_conv2d_ws(const float* input, const float* aux, const float* packed_weight,
                              const float* bias, const float* residual, float* out, int N,
                              int Cin, int Hs, int Ws, int Cout, int ksize, int pad_mode,
                              int in_op, int relu, void* workspace, size_t workspace_bytes,
                              rpst_stream_t stream) {
  RPST_REQUIRE(in_op != RPST_IN_ADD_ADAIN, "conv2d: ADD_ADAIN goes through rpst_conv2d_skip_adain");
  const ConvMode m = conv_mode();
  const size_t need = fold_bytes(N, Cin, Hs, Ws, Cout, ksize, in_op, m);
  if (need) RPST_REQUIRE_WS(need, "conv2d: workspace %zu < %zu bytes", workspace_bytes, need);
  return conv_common({.input = input, .aux = aux, .packed_weight = packed_weight, .bias = bias,
                      .residual = residual, .out = out, .N = N, .Cin = Cin, .Hs = Hs, .Ws = Ws,
                      .Cout = Cout, .ksize = ksize, .pad_mode = pad_mode, .in_op = in_op,
                      .relu = relu, .st = as_stream(stream),
                      .fold_ws = need ? static_cast<float*>(workspace) : nullptr},
                     m);
}

// conv(pad(T_n x + c_n)): F(4x4) layers fold T_n / c_n into per-image weights and border
// biases (wino4_mix); other layers materialise z = T x + c (fp32 MFMA GEMM) and convolve it.
// The fold does not depend on the quarter setting, and neither does its size (wino4_mix_floats
// takes the larger weight image); at precise level 1 the layer runs F(2x2) on z.
// fold: the per-image weights and border biases; else z = T x + c, then wct_apply_f32's
// scratch. A ksize other than 1 or 3 sizes as 0 bytes; rpst_conv2d_mix refuses it before it
// asks for the layout.
struct MixLayout { float *fold_ws, *z, *scratch; size_t bytes; };
static MixLayout mix_layout(void* workspace, int N, int Cin, int H, int W, int Cout, int ksize,
                            const ConvMode& m) {
  Carver c(workspace);
  MixLayout L{};
  if (bad_shape(N, Cin, H, W, Cout, 1)) return L;
  if (plan_folds(N, Cin, H, W, Cout, ksize, RPST_IN_NONE, m)) {
    L.fold_ws = c.take(wino4_mix_floats(N, Cin, Cout));
  } else {
    L.z = c.take((size_t)N * Cin * H * W);
    L.scratch = c.take(wct_apply_scratch_floats(N, Cin));
  }
  c.take(64);  // spare floats the size has always carried
  L.bytes = ksize == 1 || ksize == 3 ? c.bytes : 0;
  return L;
}

extern "C" size_t rpst_conv2d_mix_workspace_size(int N, int Cin, int H, int W, int Cout,
                                                 int ksize) {
  return mix_layout(nullptr, N, Cin, H, W, Cout, ksize, conv_mode()).bytes;
}

extern "C" int rpst_conv2d_mix(const float* input, const double* T, const double* offset,
                               const float* packed_weight, const float* bias, float* out, int N,
                               int Cin, int H, int W, int Cout, int ksize, int pad_mode,
                               int relu, void* workspace, size_t workspace_bytes,
                               rpst_stream_t stream) {
  RPST_REQUIRE(input && T && offset && packed_weight && out, "conv2d_mix: null pointer");
  RPST_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, "conv2d_mix: bad shape");
  // before the layout: another ksize sizes as 0 bytes, and the fallback below writes z
  RPST_REQUIRE(ksize == 1 || ksize == 3, "conv2d_mix: ksize must be 1 or 3, got %d", ksize);
  const ConvMode m = conv_mode();
  const MixLayout L = mix_layout(workspace, N, Cin, H, W, Cout, ksize, m);
  RPST_REQUIRE_WS(L.bytes, "conv2d_mix: workspace %zu < %zu bytes", workspace_bytes, L.bytes);
  ConvReq r{.input = input, .packed_weight = packed_weight, .bias = bias, .out = out, .N = N,
            .Cin = Cin, .Hs = H, .Ws = W, .Cout = Cout, .ksize = ksize, .pad_mode = pad_mode,
            .in_op = RPST_IN_NONE, .relu = relu, .st = as_stream(stream),
            .fold_ws = L.fold_ws, .T = T, .offset = offset};
  if (L.z) {
    if (int e = wct_apply_f32(T, offset, input, L.z, N, Cin, (int64_t)H * W, L.scratch, r.st))
      return e;
    r.input = L.z;
    r.T = r.offset = nullptr;
  }
  return conv_common(r, m);
}

extern "C" int rpst_conv2d_skip_adain(const float* stylized, const float* content,
                                      const float* params, const float* packed_weight,
                                      const float* bias, float* out, int N, int Cin, int H, int W,
                                      int Cout, int ksize, int pad_mode, int relu,
                                      rpst_stream_t stream) {
  RPST_REQUIRE(ksize == 3, "conv2d_skip_adain: 3x3 convs only");
  return conv_common({.input = stylized, .aux = params, .aux2 = content,
                      .packed_weight = packed_weight, .bias = bias, .out = out, .N = N,
                      .Cin = Cin, .Hs = H, .Ws = W, .Cout = Cout, .ksize = ksize,
                      .pad_mode = pad_mode, .in_op = RPST_IN_ADD_ADAIN, .relu = relu,
                      .st = as_stream(stream)},
                     conv_mode());
}

// bytes of the statistics partials of the fused epilogue: the largest over the modes, since
// the partial count depends on the kernel that runs
static size_t stat_bytes(int N, int Cin, int Hs, int Ws, int Cout, int ksize, int in_op,
                         const ConvMode& mode) {
  if (bad_shape(N, Cin, Hs, Ws, Cout, ksize)) return 0;
  return max_over_modes(mode, [&](const ConvMode& m) {
    ConvArgs a = conv_shape(N, Cin, Hs, Ws, Cout, in_op);
    conv_plan(a, ksize, in_op, m, {true, false, false});
    return ((size_t)N * Cout * a.stat_P * sizeof(float2) + 255) / 256 * 256;
  });
}

// The partials, then the bytes of rpst_conv2d_workspace_size (kept in the size the ABI has
// always returned; a statistics launch keeps AdaIN in the loader and does not use them).
extern "C" size_t rpst_conv2d_stats_workspace_size(int N, int Cin, int Hs, int Ws, int Cout,
                                                   int ksize, int in_op) {
  const ConvMode m = conv_mode();
  return stat_bytes(N, Cin, Hs, Ws, Cout, ksize, in_op, m) +
         fold_bytes(N, Cin, Hs, Ws, Cout, ksize, in_op, m);
}

namespace rpst {
// (declared in rpst_conv.h: rpst_conv_bf16.hip's statistics epilogue ends in the same merge)
int conv_stat_merge(const float2* part, float* mean, float* std_out, int N, int Cout, int P,
                    int tiles_x, const ConvTiling& t, int H, int W, float eps, hipStream_t st) {
  const int planes = N * Cout;
  stat_merge_kernel<<<(planes + 3) / 4, 256, 0, st>>>(part, mean, std_out, planes, P, tiles_x,
                                                      t.stat_wn, t.stat_nt, t.stat_tw, H, W, eps);
  return launch_status("stat_merge_kernel");
}
}  // namespace rpst

// the partials a statistics launch left in r.stat_part -> calc_mean_std
static int stat_merge(const ConvReq& r, const ConvArgs& a, const ConvPlan& p, float* mean,
                      float* std_out, float eps) {
  const float2* part = r.stat_part;
  if (p.t.stat_t) {
    stat_merge_t_kernel<<<r.N * ((r.Cout + 63) / 64), 256, 0, r.st>>>(
        part, mean, std_out, r.Cout, a.stat_P, a.tiles_x, p.t.stat_wn, p.t.stat_nt, p.t.stat_tw,
        a.H, a.W, eps);
    return launch_status("stat_merge_t_kernel");
  }
  return conv_stat_merge(part, mean, std_out, r.N, r.Cout, a.stat_P, a.tiles_x, p.t, a.H, a.W,
                         eps, r.st);
}

static int conv2d_stats_impl(ConvReq r, float* mean, float* std_out, float eps, void* workspace,
                             size_t workspace_bytes, int store_n) {
  RPST_REQUIRE(mean && std_out, "conv2d_stats: null statistics pointer");
  RPST_REQUIRE(store_n >= 1 && store_n <= r.N, "conv2d_stats: store_n=%d outside [1, N=%d]",
               store_n, r.N);
  const ConvMode m = conv_mode();
  const size_t sb = stat_bytes(r.N, r.Cin, r.Hs, r.Ws, r.Cout, r.ksize, r.in_op, m);
  const size_t need = sb + fold_bytes(r.N, r.Cin, r.Hs, r.Ws, r.Cout, r.ksize, r.in_op, m);
  RPST_REQUIRE_WS(need, "conv2d_stats: workspace %zu < %zu bytes", workspace_bytes, need);
  r.stat_part = static_cast<float2*>(workspace);
  r.skip_from = store_n < r.N ? store_n : 0;
  ConvArgs a;
  ConvPlan p;
  if (int e = conv_prepare(r, m, a, p)) return e;
  // Tiles without the fused statistics epilogue (direct, < 4 rows per wave) convolve, then
  // reduce the output. So does a layer whose residual moved it from Winograd to a direct tile
  // with more partials than the workspace was sized for.
  if ((p.algo == RPST_CONV_DIRECT && p.t.stat_nt < 4) ||
      (size_t)r.N * r.Cout * a.stat_P * sizeof(float2) > sb) {
    r.stat_part = nullptr;
    r.skip_from = 0;
    if (int e = conv_common(r, m)) return e;
    return rpst_calc_mean_std(r.out, mean, std_out, r.N, r.Cout, (int64_t)a.H * a.W, eps,
                              (rpst_stream_t)r.st);
  }
  if (int e = conv_launch(r, a, p)) return e;
  return stat_merge(r, a, p, mean, std_out, eps);
}

extern "C" int rpst_conv2d_stats_store(const float* input, const float* aux,
                                       const float* packed_weight, const float* bias,
                                       const float* residual, float* out, int N, int Cin, int Hs,
                                       int Ws, int Cout, int ksize, int pad_mode, int in_op,
                                       int relu, float* mean, float* std_out, float eps,
                                       int store_n, void* workspace, size_t workspace_bytes,
                                       rpst_stream_t stream) {
  return conv2d_stats_impl({.input = input, .aux = aux, .packed_weight = packed_weight,
                            .bias = bias, .residual = residual, .out = out, .N = N, .Cin = Cin,
                            .Hs = Hs, .Ws = Ws, .Cout = Cout, .ksize = ksize,
                            .pad_mode = pad_mode, .in_op = in_op, .relu = relu,
                            .st = as_stream(stream)},
                           mean, std_out, eps, workspace, workspace_bytes, store_n);
}

extern "C" int rpst_conv2d_stats(const float* input, const float* aux,
                                 const float* packed_weight, const float* bias,
                                 const float* residual, float* out, int N, int Cin, int Hs,
                                 int Ws, int Cout, int ksize, int pad_mode, int in_op, int relu,
                                 float* mean, float* std_out, float eps, void* workspace,
                                 size_t workspace_bytes, rpst_stream_t stream) {
  return rpst_conv2d_stats_store(input, aux, packed_weight, bias, residual, out, N, Cin, Hs, Ws,
                                 Cout, ksize, pad_mode, in_op, relu, mean, std_out, eps, N,
                                 workspace, workspace_bytes, stream);
}

// ---- the conv that ends an SE block (reference network/attention.py:56-64) ------------
// partials of the gated conv's statistics epilogue: 0 where its tile has none (Cout > 64: the
// 128-channel 1x1 tile holds 2 rows per wave; the launch then reduces the written output)
static size_t gated_stat_bytes(int N, int Cin, int H, int W, int Cout, int ksize) {
  if (bad_shape(N, Cin, H, W, Cout, ksize) || ksize != 1) return 0;
  ConvArgs a = conv_shape(N, Cin, H, W, Cout, RPST_IN_NONE);
  const ConvPlan p = conv_plan(a, ksize, RPST_IN_NONE, conv_mode(), {true, true, false, true});
  if (p.t.stat_nt < 4) return 0;
  return ((size_t)N * Cout * a.stat_P * sizeof(float2) + 255) / 256 * 256;
}

extern "C" size_t rpst_conv2d_gated_workspace_size(int N, int Cin, int H, int W, int Cout,
                                                   int ksize) {
  return gated_stat_bytes(N, Cin, H, W, Cout, ksize);
}

extern "C" int rpst_conv2d_gated(const float* input, const float* packed_weight,
                                 const float* bias, const float* gate, const float* residual,
                                 float* out, int N, int Cin, int H, int W, int Cout, int ksize,
                                 float* mean, float* std_out, float eps, void* workspace,
                                 size_t workspace_bytes, rpst_stream_t stream) {
  RPST_REQUIRE(ksize == 1, "conv2d_gated: the gated epilogue exists for 1x1 convs only, got "
               "ksize %d", ksize);
  RPST_REQUIRE(gate && residual, "conv2d_gated: null gate / residual");
  RPST_REQUIRE((mean == nullptr) == (std_out == nullptr),
               "conv2d_gated: mean and std_out are given together or not at all");
  ConvReq r{.input = input, .packed_weight = packed_weight, .bias = bias, .residual = residual,
            .out = out, .N = N, .Cin = Cin, .Hs = H, .Ws = W, .Cout = Cout, .ksize = ksize,
            .pad_mode = RPST_PAD_ZERO, .in_op = RPST_IN_NONE, .relu = RPST_ACT_RELU,
            .st = as_stream(stream), .gate = gate};
  const ConvMode m = conv_mode();
  if (!mean) return conv_common(r, m);
  const size_t sb = gated_stat_bytes(N, Cin, H, W, Cout, ksize);
  if (sb) RPST_REQUIRE_WS(sb, "conv2d_gated: workspace %zu < %zu bytes", workspace_bytes, sb);
  if (!sb) {  // no statistics epilogue on this tile: convolve, then reduce the output
    if (int e = conv_common(r, m)) return e;
    return rpst_calc_mean_std(out, mean, std_out, N, Cout, (int64_t)H * W, eps, stream);
  }
  r.stat_part = static_cast<float2*>(workspace);
  ConvArgs a;
  ConvPlan p;
  if (int e = conv_prepare(r, m, a, p)) return e;
  if (int e = conv_launch(r, a, p)) return e;
  return stat_merge(r, a, p, mean, std_out, eps);
}

// ---- stand-alone max-pool / upsample (used where no conv follows directly) ----------
__global__ void maxpool2_kernel(const float* __restrict__ in, float* __restrict__ out,
                                int64_t planes, int H, int W, int Ho, int Wo) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= planes * Ho * Wo) return;
  const int x = (int)(i % Wo);
  const int64_t r = i / Wo;
  const int y = (int)(r % Ho);
  const int64_t p = r / Ho;
  const float* s = in + p * H * W;
  const int sy = 2 * y, sx = 2 * x;
  float v = s[(int64_t)sy * W + sx];
  if (sx + 1 < W) v = fmaxf(v, s[(int64_t)sy * W + sx + 1]);
  if (sy + 1 < H) v = fmaxf(v, s[(int64_t)(sy + 1) * W + sx]);
  if (sx + 1 < W && sy + 1 < H) v = fmaxf(v, s[(int64_t)(sy + 1) * W + sx + 1]);
  out[i] = v;
}

__global__ void upsample2_kernel(const float* __restrict__ in, float* __restrict__ out,
                                 int64_t planes, int H, int W) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int Wo = 2 * W, Ho = 2 * H;
  if (i >= planes * Ho * Wo) return;
  const int x = (int)(i % Wo);
  const int64_t r = i / Wo;
  const int y = (int)(r % Ho);
  const int64_t p = r / Ho;
  out[i] = in[p * H * W + (int64_t)(y >> 1) * W + (x >> 1)];
}

// out = a + upsample_nearest2x(b): a (planes, H, W), b (planes, H/2, W/2) read at
// (y >> 1, x >> 1), the RPST_IN_ADD_UPSAMPLE2 loader's operand, materialised
__global__ void add_upsample2_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                     float* __restrict__ out, int64_t planes, int H, int W) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= planes * H * W) return;
  const int x = (int)(i % W);
  const int64_t r = i / W;
  const int y = (int)(r % H);
  const int64_t p = r / H;
  const int Wb = W >> 1, Hb = H >> 1;
  out[i] = a[i] + b[(p * Hb + (y >> 1)) * Wb + (x >> 1)];
}

extern "C" int rpst_add_upsample_nearest2x(const float* a, const float* b, float* out, int N,
                                           int C, int H, int W, rpst_stream_t stream) {
  RPST_REQUIRE(a && b && out && N > 0 && C > 0 && H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0,
               "add_upsample2x: bad args");
  const int64_t total = (int64_t)N * C * H * W;
  add_upsample2_kernel<<<(unsigned)((total + 255) / 256), 256, 0, as_stream(stream)>>>(
      a, b, out, (int64_t)N * C, H, W);
  return launch_status("add_upsample2_kernel");
}

extern "C" int rpst_maxpool2x2_ceil(const float* in, float* out, int N, int C, int H, int W,
                                    rpst_stream_t stream) {
  RPST_REQUIRE(in && out && N > 0 && C > 0 && H > 0 && W > 0, "maxpool2x2: bad args");
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  const int64_t total = (int64_t)N * C * Ho * Wo;
  maxpool2_kernel<<<(unsigned)((total + 255) / 256), 256, 0, as_stream(stream)>>>(
      in, out, (int64_t)N * C, H, W, Ho, Wo);
  return launch_status("maxpool2_kernel");
}

extern "C" int rpst_upsample_nearest2x(const float* in, float* out, int N, int C, int H,
                                       int W, rpst_stream_t stream) {
  RPST_REQUIRE(in && out && N > 0 && C > 0 && H > 0 && W > 0, "upsample2x: bad args");
  const int64_t total = (int64_t)N * C * 4 * H * W;
  upsample2_kernel<<<(unsigned)((total + 255) / 256), 256, 0, as_stream(stream)>>>(
      in, out, (int64_t)N * C, H, W);
  return launch_status("upsample2_kernel");
}
