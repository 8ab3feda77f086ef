// Direct 7x7 convolution (stride 1, pad 3) as an implicit GEMM on fp32 MFMA (gfx950).
//
// Replaces the big-receptive-field branch of the reference's LDMSAdaINRPNet encoder:
//   Conv2dBlock(C, C, 7, 1, 3): ReflectionPad2d(3) + Conv2d(k=7) [+ 1x1s] + LeakyReLU(0.2)
//   network/adain_rp.py:513-514 (rp_enc{i}_big_revf), base.py:114-198
//
// GEMM view per image n:  out[co][p] = sum_k W[co][k] * X[k][p],  k = (ci, kh, kw), the same
// view, MFMA operand maps and k-ordered exact-fp32 accumulation as conv_mfma_kernel
// (rpst_conv.hip):  M = Cout (block tile BM), N = pixels (8 rows x 32 columns), K = Cin * 49.
// All 49 taps of an 8-channel chunk do not fit LDS beside the patch (8 x 49 x 128 x 4 B =
// 200 KB), so the K loop runs over stages s = (channel chunk c, kernel row kh):
//   Ws[s & 1][kw][ci][co] : 7 taps x 8 channels x BM weights of the stage, double-buffered
//                           (28 KB a buffer at BM = 128)
//   Xs[ci][py][px]        : the (8 + 6) x (32 + 6) halo patch of the chunk's 8 channels with
//                           the padding resolved (17 KB), staged once a chunk and kept across
//                           its 7 kernel rows
// 73 KB at BM = 128: two workgroups per CU. Staging is the direct kernel's issue-early /
// write-late form: the loads of stage s + 1 (and, on a chunk's last row, the next chunk's
// patch) are issued into registers before the MFMAs of stage s and written to LDS after them.
// A stage holds 224 MFMAs per wave (14k cycles) against 7 weight loads and, once in 7 stages,
// 17 patch loads per thread, so the global latency hides without an LDS-DMA ring.
// One barrier per stage, one more per chunk (the patch is single-buffered).
// Padding: ReflectionPad2d(3) (H, W >= 4) or zero padding 3, resolved once per thread into
// byte offsets of its patch elements; channels beyond Cin read out of the buffer's range (0).
// Epilogue: bias, activation, stores at out_channel_offset of an out_channels_total-channel
// tensor. No atomics; block results do not depend on the batch.
#include "rpst_conv.h"

namespace rpst {

constexpr int kC7K = 7, kC7Taps = 49, kC7CK = 8, kC7TH = 8;
constexpr int kC7PH = kC7TH + kC7K - 1, kC7PW = kTW + kC7K - 1;  // 14 x 38 patch

struct Conv7Args {
  const float* in;
  const float* in2;  // images n >= in2_from (when > 0), as ConvArgs::in2
  const float* wpk;
  const float* bias;
  float* out;
  int N, Cin, H, W, Cout, Cout_pad, nchunks;
  int tiles_x, tiles_y;
  int pad, act;
  int in2_from;
  int co_off, co_total;
  unsigned wbytes;  // bytes of the packed image
};

template <int BM, int WM, int WN>
__global__ __launch_bounds__(256, 2) void conv7_mfma_kernel(Conv7Args a) {
  constexpr int NTH = 256, CK = kC7CK, TH = kC7TH, PH = kC7PH, PW = kC7PW;
  constexpr int WTM = BM / WM, MT = WTM / 32, NT = TH / WN;
  static_assert(WM * WN == NTH / kWave && MT >= 1 && NT >= 1, "one wave per sub-tile");
  constexpr int KST = kC7K * CK;        // weight rows per stage (kw, ci)
  constexpr int NW4 = KST * BM / 4;     // float4 weight loads per stage
  constexpr int WLD = (NW4 + NTH - 1) / NTH;
  constexpr bool WFULL = (NW4 % NTH) == 0;
  constexpr int RU = NTH / (BM / 4);    // weight rows between a thread's loads
  constexpr int XE = CK * PH * PW;      // patch elements per chunk
  constexpr int XLD = (XE + NTH - 1) / NTH;

  __shared__ float Wsb[2][KST * BM];
  __shared__ float Xs[XE];

  // block -> (co tile, image, tile row, tile col), co tile slowest (conv_mfma_kernel)
  int bid = blockIdx.x;
  const int tx = bid % a.tiles_x;
  bid /= a.tiles_x;
  const int ty = bid % a.tiles_y;
  bid /= a.tiles_y;
  const int n = bid % a.N;
  const int co0 = (bid / a.N) * BM;
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
      (void*)(a.wpk + co0), (short)0, (int)(a.wbytes - (unsigned)co0 * 4u), 0x00020000);

  // weights: thread -> stage row tid / (BM/4) + u RU = (kw, ci), float4 column tid % (BM/4)
  const unsigned w_voff = ((unsigned)(tid / (BM / 4)) * a.Cout_pad + (tid % (BM / 4)) * 4) * 4u;
  const unsigned w_ustride = (unsigned)RU * a.Cout_pad * 4u;
  const unsigned w_sstride = (unsigned)KST * a.Cout_pad * 4u;

  // patch: element e = tid + 256 i = (ci, py, px); its byte offset in the chunk's first
  // channel plane group with the padding resolved once (kOOB: a zero-padding position)
  unsigned x_voff[XLD];
#pragma unroll
  for (int i = 0; i < XLD; ++i) {
    const int e = tid + NTH * i;
    const int cl = e / (PH * PW), r = e - cl * (PH * PW);
    const int py = r / PW, px = r - py * PW;
    int y = y0 - 3 + py, x = x0 - 3 + px;
    const bool oky = resolve(y, a.H, a.pad, true), okx = resolve(x, a.W, a.pad, true);
    x_voff[i] = (e < XE && oky && okx) ? ((unsigned)cl * plane + (unsigned)(y * a.W + x)) * 4u : kOOB;
  }

  floatx16 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

  u32x4 wreg[WLD];
  float xraw[XLD];

  auto load_w = [&](int s) {
    const unsigned sb = (unsigned)s * w_sstride;
#pragma unroll
    for (int u = 0; u < WLD; ++u) {
      const bool wv = WFULL || tid + u * NTH < NW4;
      wreg[u] = __builtin_amdgcn_raw_buffer_load_b128(
          rw, (int)(wv ? w_voff + u * w_ustride + sb : kOOB), 0, 0);
    }
  };
  auto load_x = [&](int c) {
    const unsigned cb = (unsigned)c * CK * plane * 4u;
#pragma unroll
    for (int i = 0; i < XLD; ++i) xraw[i] = bload(rin, x_voff[i] == kOOB ? kOOB : x_voff[i] + cb);
  };

  const int aoff = h * BM + wm * WTM + j;
  const int boff = h * PH * PW + (wn * NT) * PW + j;

  load_w(0);
  load_x(0);
  const int nst = a.nchunks * kC7K;
  int kh = 0, c = 0;
  for (int s = 0; s < nst; ++s) {
    float* Ws = Wsb[s & 1];
#pragma unroll
    for (int u = 0; u < WLD; ++u)
      if (WFULL || tid + u * NTH < NW4)
        *reinterpret_cast<u32x4*>(Ws + 4 * (tid + u * NTH)) = wreg[u];
    if (kh == 0) {
      if (s > 0) __syncthreads();  // the previous chunk's last row has read the patch
#pragma unroll
      for (int i = 0; i < XLD; ++i)
        if ((XE % NTH) == 0 || tid + NTH * i < XE) Xs[tid + NTH * i] = xraw[i];
    }
    __syncthreads();
    if (s + 1 < nst) {
      load_w(s + 1);
      if (kh == kC7K - 1) load_x(c + 1);
    }
    const float* xb = Xs + boff + kh * PW;
#pragma unroll
    for (int kw = 0; kw < kC7K; ++kw) {
#pragma unroll
      for (int cp = 0; cp < CK / 2; ++cp) {
        float av[MT], bv[NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) av[mt] = Ws[aoff + (kw * CK + 2 * cp) * BM + mt * 32];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bv[nt] = xb[(2 * cp) * PH * PW + nt * PW + kw];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt], bv[nt], acc[mt][nt],
                                                               0, 0, 0);
      }
    }
    if (++kh == kC7K) {
      kh = 0;
      ++c;
    }
  }

  // epilogue: bias, activation, predicated coalesced stores at the channel offset
  const int x = x0 + j;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + wm * WTM + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (co >= a.Cout) continue;
      const float b = a.bias ? a.bias[co] : 0.f;
      const int64_t pbase = ((int64_t)n * a.co_total + a.co_off + co) * plane;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int y = y0 + wn * NT + nt;
        const float v = activate(acc[mt][nt][r] + b, a.act);
        if (y < a.H && x < a.W) a.out[pbase + (int64_t)y * a.W + x] = v;
      }
    }
  }
}

// (Cout,Cin,7,7) -> [chunk][tap][ci_local][Cout_pad], zero beyond Cin / Cout
__global__ void conv7_pack_kernel(const float* __restrict__ w, float* __restrict__ pk, int Cout,
                                  int Cin, int Cout_pad, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int co = (int)(i % Cout_pad);
  int64_t r = i / Cout_pad;
  const int cl = (int)(r % kC7CK);
  r /= kC7CK;
  const int t = (int)(r % kC7Taps);
  const int ci = (int)(r / kC7Taps) * kC7CK + cl;
  pk[i] = (ci < Cin && co < Cout) ? w[((int64_t)co * Cin + ci) * kC7Taps + t] : 0.f;
}

// output channels per block: 128 above 64 channels, else 64, else 32
static int conv7_bm(int Cout) { return Cout > 64 ? 128 : (Cout > 32 ? 64 : 32); }
static int conv7_cout_pad(int Cout) {
  const int bm = conv7_bm(Cout);
  return (Cout + bm - 1) / bm * bm;
}
static size_t conv7_packed_floats(int Cout, int Cin) {
  return (size_t)((Cin + kC7CK - 1) / kC7CK) * kC7Taps * kC7CK * (size_t)conv7_cout_pad(Cout);
}

}  // namespace rpst

using namespace rpst;

extern "C" size_t rpst_conv7_packed_size(int Cout, int Cin) {
  if (Cout <= 0 || Cin <= 0) return 0;
  return conv7_packed_floats(Cout, Cin) * sizeof(float);
}

extern "C" int rpst_conv7_pack(const float* weight, float* packed, int Cout, int Cin,
                               rpst_stream_t stream) {
  RPST_REQUIRE(weight && packed, "conv7_pack: null pointer");
  RPST_REQUIRE(Cout > 0 && Cin > 0, "conv7_pack: bad channels");
  const int64_t total = (int64_t)conv7_packed_floats(Cout, Cin);
  RPST_REQUIRE(total * 4 < (1LL << 31), "conv7_pack: packed weights exceed 2 GiB");
  conv7_pack_kernel<<<(unsigned)((total + 255) / 256), 256, 0, as_stream(stream)>>>(
      weight, packed, Cout, Cin, conv7_cout_pad(Cout), total);
  return launch_status("conv7_pack_kernel");
}

extern "C" int rpst_conv7(const float* input, const float* input2, const float* packed_weight,
                          const float* bias, float* out, int N, int Cin, int H, int W, int Cout,
                          int pad_mode, int act, int out_channel_offset, int out_channels_total,
                          rpst_stream_t stream) {
  RPST_REQUIRE(input && packed_weight && out, "conv7: null pointer");
  RPST_REQUIRE(N > 0 && Cin > 0 && Cout > 0 && H > 0 && W > 0, "conv7: bad shape");
  RPST_REQUIRE(pad_mode == RPST_PAD_ZERO || pad_mode == RPST_PAD_REFLECT, "conv7: bad pad %d",
               pad_mode);
  RPST_REQUIRE(act >= RPST_ACT_NONE && act <= RPST_ACT_LRELU, "conv7: bad activation %d", act);
  RPST_REQUIRE(pad_mode != RPST_PAD_REFLECT || (H >= 4 && W >= 4),
               "conv7: reflect padding 3 needs H,W >= 4 (got %d x %d)", H, W);
  RPST_REQUIRE(out_channel_offset >= 0 && out_channels_total > 0 &&
                   (int64_t)out_channel_offset + Cout <= out_channels_total,
               "conv7: channels [%d, %d + %d) outside an output of %d channels",
               out_channel_offset, out_channel_offset, Cout, out_channels_total);
  RPST_REQUIRE(!input2 || (N % 2) == 0, "conv7: a second input needs an even batch (N=%d)", N);
  RPST_REQUIRE((int64_t)N * (out_channels_total > Cin ? out_channels_total : Cin) * H * W <
                   (1LL << 40), "conv7: tensor too large");
  // per-image input (plus one chunk of channel padding) addressable by a 31-bit buffer offset
  RPST_REQUIRE(((int64_t)Cin + kC7CK) * H * W * 4 < (1LL << 31),
               "conv7: one image's input exceeds 2 GiB");
  const size_t wfloats = conv7_packed_floats(Cout, Cin);
  RPST_REQUIRE(wfloats * 4 < (1ull << 31), "conv7: packed weights exceed 2 GiB");
  Conv7Args a{};
  a.in = input;
  a.in2 = input2;
  a.in2_from = input2 ? N / 2 : 0;
  a.wpk = packed_weight;
  a.bias = bias;
  a.out = out;
  a.N = N;
  a.Cin = Cin;
  a.H = H;
  a.W = W;
  a.Cout = Cout;
  a.Cout_pad = conv7_cout_pad(Cout);
  a.nchunks = (Cin + kC7CK - 1) / kC7CK;
  a.tiles_x = (W + kTW - 1) / kTW;
  a.tiles_y = (H + kC7TH - 1) / kC7TH;
  a.pad = pad_mode;
  a.act = act;
  a.co_off = out_channel_offset;
  a.co_total = out_channels_total;
  a.wbytes = (unsigned)(wfloats * 4);
  const int bm = conv7_bm(Cout);
  const int64_t blocks = (int64_t)a.tiles_x * a.tiles_y * N * (a.Cout_pad / bm);
  RPST_REQUIRE(blocks <= 0x7fffffffLL, "conv7: grid too large");
  hipStream_t st = as_stream(stream);
  if (bm == 128) conv7_mfma_kernel<128, 2, 2><<<(unsigned)blocks, 256, 0, st>>>(a);
  else if (bm == 64) conv7_mfma_kernel<64, 2, 2><<<(unsigned)blocks, 256, 0, st>>>(a);
  else conv7_mfma_kernel<32, 1, 4><<<(unsigned)blocks, 256, 0, st>>>(a);
  return launch_status("conv7_mfma_kernel");
}
