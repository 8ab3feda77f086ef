// Opt-in reduced-precision 3x3 convolution (stride 1, pad 1): a direct implicit GEMM on the
// bf16 MFMA (v_mfma_f32_32x32x16_bf16, gfx950) with fp32 accumulation. rpst_conv2d_bf16.
//
// Arithmetic contract (DESIGN.md "bf16 inference"):
//   * activations are fp32 in global memory, input and output;
//   * the tile loader forms the fp32 input value (the AdaIN affine first under RPST_IN_ADAIN,
//     as combine<RPST_IN_ADAIN> of rpst_conv.h), and rounds it ONCE, to nearest even, to bf16
//     while staging it to LDS (v_cvt_pk_bf16_f32);
//   * weights are rounded the same way once, by rpst_conv2d_bf16_pack;
//   * a bf16 x bf16 product is exact in fp32; accumulation is fp32 in the fixed K order
//     (16-channel chunk, kernel column, kernel row, channel), no atomics;
//   * bias, activation and the statistics epilogue are fp32 / fp64 as in conv_mfma_kernel;
//   * a block's results depend on its image alone: output bits do not depend on the batch.
//
// GEMM view per image: out[co][p] = sum_k W[co][k] X[k][p], k = (chunk c, tap t, ci in chunk).
// One MFMA takes K = 16 = the 16 channels of chunk c at one tap, so its B operand is the
// chunk's halo patch read at the tap's shift and its A operand one tap's weight rows:
//   Xs[pixel (py, px)][16 ch] : the (TH + 2) x 34 patch, pixel-major bf16, 32 B a pixel; a
//                               lane's 8 consecutive k are one ds_read_b128. The 16-B half
//                               h of pixel p sits at slot h ^ ((p >> 3) & 1): the 16 lanes a
//                               ds_read_b128 services together (columns {c..c+3, c+12..c+15,
//                               c+20..c+27}) hold no two pixels 16 apart, so they cover 16
//                               distinct 16-B slots of the 256-B bank row for every shift c.
//   Ws[tap][co][16 ch]        : the chunk's 9 x BM weight rows, the same 32-B rows and swizzle
//                               (on co), copied from the packed image [chunk][tap][Cout_pad][16]
// A block is 8 waves; a wave owns 32 MT channels x 4 rows x 32 columns. Per chunk and kernel
// column it reads its 6 patch rows once (6 B fragments) and reuses them over the 3 kernel rows:
// 36 LDS reads for 72 MFMAs at MT = 2. Ws and Xs are double-buffered (113 KB at BM = 128, one
// block a CU, two waves a SIMD): the next chunk's global loads are issued before the chunk's
// MFMAs, converted and written to the other buffer after them; one barrier per chunk.
// MFMA shape: the same wave tile on v_mfma_f32_16x16x32_bf16 (K = 2 taps x 16 channels, the
// ninth tap half empty, 60 LDS reads per 160 MFMAs, unswizzled rows) was built and timed
// against this form, interleaved, plain epilogue, N = 32, 512^2: 128->256 6.724 ms against
// 6.401 / 6.411, 256->128 5.862 against 5.631 / 5.630, 64->128 2.160 against 2.155 / 2.156
// (profiles/bf16/mfma_shape_16x16x32.jsonl; outputs 2-3e-7 apart). 32x32x16 is kept.
// Blocks: XCD x gets a contiguous range of spatial tiles, and the co tiles of one spatial tile
// run back to back on that XCD, so the second reads the input from its L2.
#include "rpst_conv.h"

namespace rpst {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kBfCK = 16;          // input channels per chunk = K of one MFMA
constexpr int kBfNTH = 512;        // threads per block
constexpr int kBfNT = 4;           // output rows per wave
constexpr int kBfPW = kTW + 2;     // patch columns
constexpr int kBfMaxCin = 256;     // AdaIN parameters staged per block

struct ConvBf16Args {
  const float* in;
  const float* in2;   // images n >= in2_from (when > 0), as ConvArgs::in2
  const float* aux;   // RPST_IN_ADAIN: [mean_c|mean_s|std_c|std_s], each N*Cin floats
  const uint4* wpk;   // [chunk][tap][Cout_pad][16] bf16
  const float* bias;
  float* out;
  float2* stat_part;  // optional (mean, M2) partials [n][co][stat_P]
  int N, Cin, H, W, Cout, Cout_pad, nchunks;
  int tiles_x, tiles_y, co_tiles;
  int spatial, per_xcd;  // spatial tiles in all, and per XCD
  int pad, act;
  int in2_from, skip_from, stat_P;
  unsigned wbytes;
};

// two floats -> packed bf16 pair, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{lo, hi}, bf16x2));
}

// 16-B unit index of half `half` of 32-B row `row` (a pixel of Xs, a (tap, co) row of Ws)
__device__ __forceinline__ int bf_slot(int row, int half) {
  return row * 2 + (half ^ ((row >> 3) & 1));
}

template <int BM, int WM, int WN, int MT, bool ADAIN>
__global__ __launch_bounds__(kBfNTH) void conv_bf16_kernel(ConvBf16Args a) {
  constexpr int NTH = kBfNTH, NT = kBfNT, CK = kBfCK, PW = kBfPW;
  constexpr int TH = WN * NT, PH = TH + 2, NPIX = PH * PW;
  constexpr int WTM = 32 * MT;
  static_assert(WM * WN == NTH / kWave && WM * WTM == BM, "one wave per sub-tile");
  constexpr int XU = NPIX * 2;  // 16-B units of the patch
  constexpr int XLD = (XU + NTH - 1) / NTH;
  constexpr int WU = 9 * BM * 2;  // 16-B units of a chunk's weights
  constexpr int WLD = (WU + NTH - 1) / NTH;

  __shared__ uint4 Wsb[2][WU];
  __shared__ uint4 Xsb[2][XU];
  __shared__ float Ps[ADAIN ? 3 * kBfMaxCin : 1];

  // block -> (spatial tile, co tile)
  const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
  const int ct = q % a.co_tiles;
  int s = xcd * a.per_xcd + q / a.co_tiles;
  if (s >= a.spatial) return;  // the last XCD's range may be short (block-uniform)
  const int tx = s % a.tiles_x;
  s /= a.tiles_x;
  const int ty = s % a.tiles_y;
  const int n = s / a.tiles_y;
  const int co0 = ct * BM;
  const int y0 = ty * TH, x0 = tx * kTW;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int h = lane >> 5, j = lane & 31;

  const unsigned plane = (unsigned)(a.H * a.W);
  const float* img = (a.in2_from > 0 && n >= a.in2_from)
                         ? a.in2 + (int64_t)(n - a.in2_from) * a.Cin * plane
                         : a.in + (int64_t)n * a.Cin * plane;
  const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(
      (void*)img, (short)0, (int)(a.Cin * plane * 4u), 0x00020000);
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
      (void*)a.wpk, (short)0, (int)a.wbytes, 0x00020000);

  if constexpr (ADAIN) {
    // fma(v - mean_c, std_s / std_c, mean_s), the parameters of adain_params (rpst_conv.h)
    const int64_t nc = (int64_t)a.N * a.Cin;
    for (int ci = tid; ci < a.Cin; ci += NTH) {
      const int64_t i = (int64_t)n * a.Cin + ci;
      Ps[ci] = a.aux[i];
      Ps[kBfMaxCin + ci] = a.aux[3 * nc + i] / a.aux[2 * nc + i];
      Ps[2 * kBfMaxCin + ci] = a.aux[nc + i];
    }
    __syncthreads();
  }

  // patch: unit u = tid + 512 i = (pixel u >> 1, channel half u & 1 = tid & 1); the byte offset
  // of its pixel in the half's first channel plane with the padding resolved once (kOOB: zero
  // padding, or past the patch). The chunk and channel go into the loads' scalar offset, so
  // these stay the only per-lane addresses (a lane's sum stays inside the image; kOOB alone is
  // already out of range)
  const int xhalf = tid & 1;
  unsigned x_voff[XLD];
#pragma unroll
  for (int i = 0; i < XLD; ++i) {
    const int pix = (tid >> 1) + (NTH / 2) * i;
    const int py = pix / PW, px = pix - py * PW;
    int y = y0 - 1 + py, x = x0 - 1 + px;
    const bool oky = resolve(y, a.H, a.pad, true), okx = resolve(x, a.W, a.pad, true);
    x_voff[i] = (pix < NPIX && oky && okx)
                    ? (unsigned)(y * a.W + x) * 4u + (unsigned)(xhalf * 8) * plane * 4u
                    : kOOB;
  }
  // weights: unit u = tid + 512 i = (row u >> 1 = tap * BM + co, half u & 1) of the chunk; a
  // step of i is 256 / BM taps
  static_assert((NTH / 2) % BM == 0, "whole taps per load step");
  const int wrow = tid >> 1;
  const unsigned w_voff =
      (unsigned)(((wrow / BM) * a.Cout_pad + co0 + wrow % BM) * 2 + (tid & 1)) * 16u;
  const unsigned w_istride = (unsigned)(NTH / 2 / BM) * (unsigned)a.Cout_pad * 32u;
  const unsigned w_cstride = 9u * (unsigned)a.Cout_pad * 32u;

  floatx16 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

  u32x4 wreg[WLD];
  float xraw[XLD][8];

  auto load_w = [&](int c) {
#pragma unroll
    for (int i = 0; i < WLD; ++i)
      wreg[i] = __builtin_amdgcn_raw_buffer_load_b128(
          rw, (int)(((WU % NTH) == 0 || tid + NTH * i < WU) ? w_voff : kOOB),
          (int)((unsigned)i * w_istride + (unsigned)c * w_cstride), 0);
  };
  auto load_x = [&](int c) {
#pragma unroll
    for (int i = 0; i < XLD; ++i)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        xraw[i][e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
            rin, (int)x_voff[i], (int)((unsigned)(c * CK + e) * plane * 4u), 0));
  };

  // operand addresses (16-B units): A rows wm WTM + mt 32 + j of a tap, B pixels of row
  // wn NT + q, column j + kw
  const int a_unit = (wm * WTM + j) * 2 + (h ^ ((j >> 3) & 1));

  // registers of chunk c -> buffer c & 1 (converted; under ADAIN the affine first)
  auto stage = [&](int c) {
    uint4* Ws = Wsb[c & 1];
    uint4* Xs = Xsb[c & 1];
#pragma unroll
    for (int i = 0; i < WLD; ++i) {
      const int u = tid + NTH * i;
      if ((WU % NTH) == 0 || u < WU)
        Ws[bf_slot(u >> 1, u & 1)] = make_uint4(wreg[i][0], wreg[i][1], wreg[i][2], wreg[i][3]);
    }
#pragma unroll
    for (int i = 0; i < XLD; ++i) {
      const int pix = (tid >> 1) + (NTH / 2) * i;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        v[e] = xraw[i][e];
        if constexpr (ADAIN) {
          const int ci = c * CK + xhalf * 8 + e;
          v[e] = x_voff[i] == kOOB
                     ? 0.f
                     : fmaf(v[e] - Ps[ci], Ps[kBfMaxCin + ci], Ps[2 * kBfMaxCin + ci]);
        }
      }
      if ((XU % NTH) == 0 || pix < NPIX)
        Xs[bf_slot(pix, xhalf)] = make_uint4(pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]),
                                             pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7]));
    }
  };

  load_w(0);
  load_x(0);
  stage(0);
  __syncthreads();
  for (int c = 0; c < a.nchunks; ++c) {
    const uint4* Ws = Wsb[c & 1];
    const uint4* Xs = Xsb[c & 1];
    const bool more = c + 1 < a.nchunks;
    if (more) {
      load_w(c + 1);
      load_x(c + 1);
    }
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      // keep one kernel column's operands live at a time (hoisting all 36 reads of the chunk
      // above its MFMAs costs 100 VGPRs and spills)
      __builtin_amdgcn_sched_barrier(0);
      bf16x8 bv[NT + 2];
#pragma unroll
      for (int qr = 0; qr < NT + 2; ++qr)
        bv[qr] = __builtin_bit_cast(bf16x8, Xs[bf_slot((wn * NT + qr) * PW + j + kw, h)]);
#pragma unroll
      for (int kh = 0; kh < 3; ++kh) {
        bf16x8 av[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
          av[mt] = __builtin_bit_cast(bf16x8, Ws[((kh * 3 + kw) * BM + mt * 32) * 2 + a_unit]);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[mt], bv[nt + kh],
                                                                  acc[mt][nt], 0, 0, 0);
      }
    }
    // buffer (c + 1) & 1 was last read before the barrier that ended chunk c - 1
    if (more) stage(c + 1);
    __syncthreads();
  }

  // epilogue: bias, activation, predicated coalesced stores (none for images >= skip_from)
  const int x = x0 + j;
  const bool store = !(a.skip_from > 0 && n >= a.skip_from);
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + wm * WTM + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      const bool cok = co < a.Cout;
      const float b = (a.bias && cok) ? a.bias[co] : 0.f;
      const int64_t pbase = ((int64_t)n * a.Cout + co) * plane;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int y = y0 + wn * NT + nt;
        const float v = activate(acc[mt][nt][r] + b, a.act);
        if (store && cok && y < a.H && x < a.W) a.out[pbase + (int64_t)y * a.W + x] = v;
        acc[mt][nt][r] = v;
      }
    }
  }

  // optional output statistics, as conv_mfma_kernel's: (mean, M2) per (channel, wave tile of
  // 4 rows x 32 columns), two-pass, merged in fp64 by stat_merge_kernel
  if (a.stat_part) {
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

// (Cout,Cin,3,3) fp32 -> [chunk][tap][Cout_pad][16] bf16 (round to nearest even), zero beyond
// Cout; one thread per channel pair
__global__ void conv_bf16_pack_kernel(const float* __restrict__ w, unsigned* __restrict__ pk,
                                      int Cout, int Cin, int Cout_pad, int64_t pairs) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pairs) return;
  const int cl = (int)(i % (kBfCK / 2)) * 2;
  int64_t r = i / (kBfCK / 2);
  const int co = (int)(r % Cout_pad);
  r /= Cout_pad;
  const int t = (int)(r % 9);
  const int ci = (int)(r / 9) * kBfCK + cl;
  const bool ok = co < Cout;
  const float lo = ok ? w[((int64_t)co * Cin + ci) * 9 + t] : 0.f;
  const float hi = ok ? w[((int64_t)co * Cin + ci + 1) * 9 + t] : 0.f;
  pk[i] = pack_bf16(lo, hi);
}

// output channels per block: 128 above 64 channels, else 64, else 32
static int bf16_bm(int Cout) { return Cout > 64 ? 128 : (Cout > 32 ? 64 : 32); }
static int bf16_cout_pad(int Cout) {
  const int bm = bf16_bm(Cout);
  return (Cout + bm - 1) / bm * bm;
}
static size_t bf16_packed_bytes(int Cout, int Cin) {
  return (size_t)(Cin / kBfCK) * 9 * (size_t)bf16_cout_pad(Cout) * kBfCK * 2;
}

// what the kernel can run
static bool bf16_capable(int Cout, int Cin, int ksize, int pad_mode, int in_op) {
  return ksize == 3 && Cin >= kBfCK && Cin % kBfCK == 0 && Cin <= kBfMaxCin && Cout >= 16 &&
         (pad_mode == RPST_PAD_ZERO || pad_mode == RPST_PAD_REFLECT) &&
         (in_op == RPST_IN_NONE || in_op == RPST_IN_ADAIN);
}

// The tiling fields of `a` (from N, H, W, Cout) and the launch shape.
static ConvTiling bf16_tiling(ConvBf16Args& a) {
  const int bm = bf16_bm(a.Cout);
  const int wn = bm == 128 ? 4 : 8;
  a.Cout_pad = bf16_cout_pad(a.Cout);
  a.co_tiles = a.Cout_pad / bm;
  a.nchunks = a.Cin / kBfCK;
  a.tiles_x = (a.W + kTW - 1) / kTW;
  a.tiles_y = (a.H + wn * kBfNT - 1) / (wn * kBfNT);
  const int64_t spatial = (int64_t)a.tiles_x * a.tiles_y * a.N;
  a.spatial = (int)spatial;
  a.per_xcd = (int)((spatial + 7) / 8);
  a.stat_P = a.tiles_x * a.tiles_y * wn;
  ConvTiling t{};
  t.blocks = spatial > 0x7fffffffLL ? -1 : (int64_t)a.per_xcd * 8 * a.co_tiles;
  t.nth = kBfNTH;
  t.stat_nt = kBfNT;
  t.stat_wn = wn;
  t.stat_tw = kTW;
  t.stat_t = false;
  return t;
}

static bool bf16_bad_shape(int N, int Cin, int H, int W, int Cout) {
  return N <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0 ||
         (int64_t)N * (Cin > Cout ? Cin : Cout) * H * W >= (1LL << 40) ||
         (int64_t)Cin * H * W * 4 >= (1LL << 31);
}

static size_t bf16_stat_bytes(int N, int Cin, int H, int W, int Cout) {
  if (bf16_bad_shape(N, Cin, H, W, Cout)) return 0;
  ConvBf16Args a{};
  a.N = N, a.Cin = Cin, a.H = H, a.W = W, a.Cout = Cout;
  bf16_tiling(a);
  return ((size_t)N * Cout * a.stat_P * sizeof(float2) + 255) / 256 * 256;
}

template <bool ADAIN>
static void bf16_launch(const ConvBf16Args& a, unsigned blocks, hipStream_t st) {
  const int bm = bf16_bm(a.Cout);
  if (bm == 128) conv_bf16_kernel<128, 2, 4, 2, ADAIN><<<blocks, kBfNTH, 0, st>>>(a);
  else if (bm == 64) conv_bf16_kernel<64, 1, 8, 2, ADAIN><<<blocks, kBfNTH, 0, st>>>(a);
  else conv_bf16_kernel<32, 1, 8, 1, ADAIN><<<blocks, kBfNTH, 0, st>>>(a);
}

}  // namespace rpst

using namespace rpst;

// Selection by measurement: the plans send a layer here only where this kernel beat the fp32
// kernel rpst_conv2d picks for it. Measured at 512^2 on one MI355X, layers launched as
// AdaINRPNet.test() (rp_blocks 5, hidden 16, N = 32 + 32) launches them, fp32 run twice
// (tools/bench_bf16.py, profiles/bf16/bench_bf16_all_layers.json; ms per call, fp32 a / b, bf16):
//   16->32   N 64   0.832 / 0.834   1.024   slower      32->16   N 32  0.581 / 0.580  0.651  slower
//   32->64   N 64   2.480 / 2.482   2.038   0.82 x      64->32   N 32  1.070 / 1.069  1.089  slower
//   64->128  N 64   7.787 / 7.796   4.713   0.61 x      128->64  N 32  3.455 / 3.453  2.257  0.65 x
//   128->256 N 64  25.81  / 25.84  13.12    0.51 x      256->128 N 32 12.67  / 12.68  6.289  0.50 x
// (128->256 with the statistics epilogue and store_n, 256->128 through the AdaIN loader). The
// fp32 spread is below 0.03 ms everywhere. Every layer of at most 32 output channels lost
// (they run at 0.31-0.39 of the HBM peak on either kernel and the 32-channel tile fills half
// an MFMA's worth of rows per wave), every layer of 64 or more won: the rule is Cout >= 64.
// Layers of 33..63 output channels were not measured and stay on fp32. rpst_conv2d_bf16
// itself runs every layer bf16_capable accepts.
extern "C" int rpst_conv2d_bf16_supports(int Cout, int Cin, int ksize, int pad_mode, int in_op) {
  return (bf16_capable(Cout, Cin, ksize, pad_mode, in_op) && Cout >= 64) ? 1 : 0;
}

extern "C" size_t rpst_conv2d_bf16_packed_size(int Cout, int Cin) {
  if (!bf16_capable(Cout, Cin, 3, RPST_PAD_ZERO, RPST_IN_NONE)) return 0;
  return bf16_packed_bytes(Cout, Cin);
}

extern "C" int rpst_conv2d_bf16_pack(const float* weight, void* packed, int Cout, int Cin,
                                     rpst_stream_t stream) {
  RPST_REQUIRE(weight && packed, "conv2d_bf16_pack: null pointer");
  RPST_REQUIRE(bf16_capable(Cout, Cin, 3, RPST_PAD_ZERO, RPST_IN_NONE),
               "conv2d_bf16_pack: Cin=%d (a multiple of 16 in [16, %d]) / Cout=%d (>= 16) "
               "unsupported", Cin, kBfMaxCin, Cout);
  const size_t bytes = bf16_packed_bytes(Cout, Cin);
  RPST_REQUIRE(bytes < (1ull << 31), "conv2d_bf16_pack: packed weights exceed 2 GiB");
  const int64_t pairs = (int64_t)(bytes / 4);
  conv_bf16_pack_kernel<<<(unsigned)((pairs + 255) / 256), 256, 0, as_stream(stream)>>>(
      weight, static_cast<unsigned*>(packed), Cout, Cin, bf16_cout_pad(Cout), pairs);
  return launch_status("conv_bf16_pack_kernel");
}

extern "C" size_t rpst_conv2d_bf16_workspace_size(int N, int Cin, int H, int W, int Cout) {
  return bf16_stat_bytes(N, Cin, H, W, Cout);
}

extern "C" int64_t rpst_conv2d_bf16_grid_threads(int N, int Cin, int H, int W, int Cout) {
  if (bf16_bad_shape(N, Cin, H, W, Cout)) return 0;
  ConvBf16Args a{};
  a.N = N, a.Cin = Cin, a.H = H, a.W = W, a.Cout = Cout;
  const ConvTiling t = bf16_tiling(a);
  return t.blocks < 0 ? 0 : t.blocks * t.nth;
}

extern "C" int rpst_conv2d_bf16(const float* input, const float* input2, int n1, const float* aux,
                                const void* packed, const float* bias, float* out, int N,
                                int Cin, int H, int W, int Cout, int pad_mode, int in_op, int act,
                                float* mean, float* std_out, float eps, int store_n,
                                void* workspace, size_t workspace_bytes, rpst_stream_t stream) {
  RPST_REQUIRE(input && packed && out, "conv2d_bf16: null pointer");
  RPST_REQUIRE(!bf16_bad_shape(N, Cin, H, W, Cout),
               "conv2d_bf16: bad shape, or one image's input exceeds 2 GiB");
  RPST_REQUIRE(bf16_capable(Cout, Cin, 3, pad_mode, in_op),
               "conv2d_bf16: unsupported layer (Cin=%d a multiple of 16 in [16, %d], Cout=%d >= "
               "16, pad %d zero / reflect, in_op %d none / AdaIN)", Cin, kBfMaxCin, Cout,
               pad_mode, in_op);
  RPST_REQUIRE(act >= RPST_ACT_NONE && act <= RPST_ACT_LRELU, "conv2d_bf16: bad activation %d",
               act);
  RPST_REQUIRE(pad_mode != RPST_PAD_REFLECT || (H >= 2 && W >= 2),
               "conv2d_bf16: reflect padding needs H,W >= 2 (got %d x %d)", H, W);
  RPST_REQUIRE((in_op == RPST_IN_ADAIN) == (aux != nullptr),
               "conv2d_bf16: aux goes with RPST_IN_ADAIN and only with it");
  RPST_REQUIRE(!(input2 && in_op != RPST_IN_NONE), "conv2d_bf16: a second input has no input op");
  RPST_REQUIRE(!input2 || (n1 > 0 && n1 < N), "conv2d_bf16: n1=%d outside (0, N=%d)", n1, N);
  RPST_REQUIRE((mean != nullptr) == (std_out != nullptr),
               "conv2d_bf16: mean and std_out go together");
  RPST_REQUIRE(mean ? (store_n >= 1 && store_n <= N) : (store_n == N || store_n == 0),
               "conv2d_bf16: store_n=%d outside [1, N=%d] (and N without statistics)", store_n, N);
  ConvBf16Args a{};
  a.in = input;
  a.in2 = input2;
  a.in2_from = input2 ? n1 : 0;
  a.aux = aux;
  a.wpk = static_cast<const uint4*>(packed);
  a.bias = bias;
  a.out = out;
  a.N = N, a.Cin = Cin, a.H = H, a.W = W, a.Cout = Cout;
  a.pad = pad_mode;
  a.act = act;
  const ConvTiling t = bf16_tiling(a);
  RPST_REQUIRE(t.blocks > 0 && t.blocks <= 0x7fffffffLL, "conv2d_bf16: grid too large");
  a.wbytes = (unsigned)bf16_packed_bytes(Cout, Cin);
  if (mean) {
    const size_t need = bf16_stat_bytes(N, Cin, H, W, Cout);
    RPST_REQUIRE_WS(need, "conv2d_bf16: workspace %zu < %zu bytes", workspace_bytes, need);
    a.stat_part = static_cast<float2*>(workspace);
    a.skip_from = store_n < N ? store_n : 0;
  }
  hipStream_t st = as_stream(stream);
  if (in_op == RPST_IN_ADAIN) bf16_launch<true>(a, (unsigned)t.blocks, st);
  else bf16_launch<false>(a, (unsigned)t.blocks, st);
  if (int e = launch_status("conv_bf16_kernel")) return e;
  if (!mean) return RPST_OK;
  return conv_stat_merge(a.stat_part, mean, std_out, N, Cout, a.stat_P, a.tiles_x, t, H, W, eps,
                         st);
}
