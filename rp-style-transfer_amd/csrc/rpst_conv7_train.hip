// Backward kernels of the 7x7 pad-3 convolution (rpst_conv7): the big-receptive-field branch
// of LDMSAdaINRPNet's encoder in training (network/adain_rp.py:513-514, base.py:114-198).
//
//   wgrad   conv7_wgrad_kernel: implicit GEMM dW[co][ci][kh][kw] = sum over (n,y,x) of
//           dY[n][co][y][x] pad3(X)[n][ci][y+kh-3][x+kw-3] on fp32 MFMA, split over K (pixels)
//           with a fixed-order reduction (wgrad_reduce_kernel, rpst_train.h); the bias gradient
//           from the staged dY tiles. The padding (reflect or zero) is resolved in the loader.
//   dgrad   = rpst_conv7 on flip-transposed weights with zero padding (rpst_conv_weight_flip,
//           rpst_conv7_pack). A reflect-padded conv runs it on dY embedded in zeros over the
//           padded domain, (H+6) x (W+6), which gives the gradient of the padded input, and
//           reflect_pad_backward_kernel sums every padded position into the pixel it mirrors.
// All reductions are fixed-order (no float atomics): results are deterministic.
#include "rpst_train.h"

namespace rpst {

// ---- conv weight gradient (7x7, stride 1, pad 3) -------------------------------------------
// The 3x3 wgrad (conv_wgrad_kernel) holds all 9 taps of a 64 co x 64 ci tile per block; 49
// taps would be 784 accumulator registers a lane, so the taps are split across blocks by
// kernel row: block = (co tile, ci tile, kh, pixel split), 256 threads (4 waves as 2 x 2 over
// the tile), 7 accumulators (the kw taps) of 32 x 32 per wave = 112 registers a lane.
// K = pixels, walked in row segments of PX = 64 columns of one output row y: LDS holds
// dY[px][co] (PX x 65) and the one input row yy = y + kh - 3 as X[col][ci] ((PX + 6) x 65,
// columns x0 - 3 .. x0 + PX + 2, padding resolved: reflected index, or 0 outside for zero
// padding). v_mfma_f32_32x32x2_f32 with A = dY (co x px) and B = X shifted by kw (px x ci): the
// 7 taps are shifted reads of the same staged row against one dY fragment.
// Staging: element e = tid + 256 i -> (channel e / width, column e % width), 4-byte buffer
// loads (16 dY + 18 X per thread a segment, coalesced along the row); the next segment's loads
// are issued into registers before the current segment's 224 MFMAs per wave and written to
// LDS after them. dY columns at or past W and channels past Cout / Cin read 0, so whatever X
// holds beside them adds nothing. Blocks of the first ci tile and kh = 0 also reduce the bias
// gradient from their dY tiles. X is read once per kh (7 times in all).
constexpr unsigned kW7OOB = 0x80000000u;
constexpr int kW7TC = 64, kW7PX = 64, kW7LD = kW7TC + 1, kW7XC = kW7PX + 6;

// index t in [-3, n + 2] of a pad-3 line of n -> source index; false: a zero
__device__ __forceinline__ bool pad3_resolve(int& t, int n, bool reflect) {
  if (t >= 0 && t < n) return true;
  if (!reflect) return false;
  t = t < 0 ? -t : 2 * n - 2 - t;
  return t >= 0 && t < n;
}

__global__ __launch_bounds__(256, 2) void conv7_wgrad_kernel(
    const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ part,
    float* __restrict__ bpart, int N, int Cin, int H, int W, int Cout, int64_t segs_per_split,
    int reflect) {
  constexpr int TC = kW7TC, PX = kW7PX, LD = kW7LD, XC = kW7XC;
  constexpr int NY = TC * PX / 256, NX = (TC * XC + 255) / 256;
  __shared__ float Ys[PX * LD];
  __shared__ float Xs[XC * LD];
  const int tilesCi = (Cin + TC - 1) / TC;
  const int tile = blockIdx.x / 7, kh = blockIdx.x % 7, split = blockIdx.y;
  const int co0 = (tile / tilesCi) * TC, ci0 = (tile % tilesCi) * TC;
  const bool bias_tile = bpart != nullptr && (tile % tilesCi) == 0 && kh == 0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int h = lane >> 5, j = lane & 31;
  const int segW = (W + PX - 1) / PX;
  const int64_t segs = (int64_t)N * H * segW;
  const int64_t s0 = (int64_t)split * segs_per_split;
  const int64_t s1 = s0 + segs_per_split < segs ? s0 + segs_per_split : segs;
  const unsigned HW = (unsigned)(H * W);

  floatx16 acc[7];
#pragma unroll
  for (int t = 0; t < 7; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bacc = 0.f;

  float ry[NY], rx[NX];
  // issue the loads of segment sg into registers (branch-free buffer loads)
  auto load = [&](int64_t sg) {
    const bool live = sg < s1;
    const int64_t sgc = live ? sg : s0;
    const int xs = (int)(sgc % segW);
    const int64_t ry_ = sgc / segW;
    const int y = (int)(ry_ % H), n = (int)(ry_ / H);
    const int x0 = xs * PX;
    const __amdgpu_buffer_rsrc_t rdy = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(dy + (int64_t)n * Cout * HW), (short)0, (int)(Cout * HW * 4u), 0x00020000);
    const __amdgpu_buffer_rsrc_t rxx = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(x + (int64_t)n * Cin * HW), (short)0, (int)(Cin * HW * 4u), 0x00020000);
#pragma unroll
    for (int i = 0; i < NY; ++i) {
      const int e = tid + 256 * i, c = e / PX, xx = x0 + e % PX;
      const bool ok = live && co0 + c < Cout && xx < W;
      const unsigned off = ((unsigned)(co0 + c) * HW + (unsigned)y * W + xx) * 4u;
      ry[i] = __uint_as_float(
          __builtin_amdgcn_raw_buffer_load_b32(rdy, (int)(ok ? off : kW7OOB), 0, 0));
    }
    int yy = y + kh - 3;
    const bool rok = pad3_resolve(yy, H, reflect != 0) && live;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int e = tid + 256 * i, c = e / XC;
      int xx = x0 - 3 + e % XC;
      const bool ok = rok && e < TC * XC && ci0 + c < Cin && pad3_resolve(xx, W, reflect != 0);
      const unsigned off = ((unsigned)(ci0 + c) * HW + (unsigned)(rok ? yy : 0) * W + xx) * 4u;
      rx[i] = __uint_as_float(
          __builtin_amdgcn_raw_buffer_load_b32(rxx, (int)(ok ? off : kW7OOB), 0, 0));
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < NY; ++i) {
      const int e = tid + 256 * i;
      Ys[(e % PX) * LD + e / PX] = ry[i];
    }
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int e = tid + 256 * i;
      if ((TC * XC) % 256 == 0 || e < TC * XC) Xs[(e % XC) * LD + e / XC] = rx[i];
    }
  };

  load(s0);
  for (int64_t sg = s0; sg < s1; ++sg) {
    store();
    __syncthreads();
    load(sg + 1);  // in flight during this segment's MFMAs
    if (bias_tile && wave == 0) {
      float t = 0.f;
      for (int px = 0; px < PX; ++px) t += Ys[px * LD + lane];
      bacc += t;
    }
#pragma unroll 4
    for (int kk = 0; kk < PX / 2; ++kk) {
      const int px = 2 * kk + h;
      const float av = Ys[px * LD + wm * 32 + j];
#pragma unroll
      for (int kw = 0; kw < 7; ++kw) {
        const float bv = Xs[(px + kw) * LD + wn * 32 + j];
        acc[kw] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[kw], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  if (bias_tile && wave == 0 && co0 + lane < Cout)
    bpart[(int64_t)split * Cout + co0 + lane] = bacc;
  // partial[split][co][ci][kh][kw]; accumulator element r of lane: row (co) =
  // (r&3) + 8(r>>2) + 4h, column (ci) = j
  const int ci = ci0 + wn * 32 + j;
  if (ci >= Cin) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    if (co >= Cout) continue;
    float* o = part + (((int64_t)split * Cout + co) * Cin + ci) * 49 + kh * 7;
#pragma unroll
    for (int kw = 0; kw < 7; ++kw) o[kw] = acc[kw][r];
  }
}

// ---- ReflectionPad2d(pad) backward -----------------------------------------------------------
// gp: planes of (H + 2 pad) x (W + 2 pad), the gradient of the padded tensor; dx[i][j] = the sum
// of gp over every padded position that reads (i, j): its own, and the mirrored ones. Along one
// axis of length n, padded index p reads t = p - pad reflected: source i is read by p = i + pad,
// by p = pad - i when 1 <= i <= pad (the leading mirror) and by p = 2 n - 2 - i + pad when
// n - 1 - pad <= i <= n - 2 (the trailing one); with n <= 2 pad both mirrors can land on the
// same i. One thread per (plane, i, j) sums its up to 3 x 3 positions in a fixed order.
__global__ __launch_bounds__(256) void reflect_pad_backward_kernel(
    const float* __restrict__ gp, float* __restrict__ dx, int64_t planes, int H, int W, int pad) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= planes * H * W) return;
  const int jx = (int)(t % W);
  const int64_t r = t / W;
  const int iy = (int)(r % H);
  const int64_t p = r / H;
  const int Wp = W + 2 * pad, Hp = H + 2 * pad;
  int rows[3], cols[3], nr = 0, nc = 0;
  rows[nr++] = iy + pad;
  if (iy >= 1 && iy <= pad) rows[nr++] = pad - iy;
  if (iy >= H - 1 - pad && iy <= H - 2) rows[nr++] = 2 * H - 2 - iy + pad;
  cols[nc++] = jx + pad;
  if (jx >= 1 && jx <= pad) cols[nc++] = pad - jx;
  if (jx >= W - 1 - pad && jx <= W - 2) cols[nc++] = 2 * W - 2 - jx + pad;
  const float* g = gp + p * Hp * Wp;
  float s = 0.f;
  for (int a = 0; a < nr; ++a)
    for (int b = 0; b < nc; ++b) s += g[(int64_t)rows[a] * Wp + cols[b]];
  dx[t] = s;
}

// The launch geometry and the partials it writes: part[splits][Cout][Cin][49], then
// bpart[splits][Cout].
struct Wgrad7Layout { int64_t tiles, sps; int splits; float *part, *bpart; size_t bytes; };
static Wgrad7Layout wgrad7_layout(void* workspace, int N, int Cin, int H, int W, int Cout) {
  Carver c(workspace);
  Wgrad7Layout L{};
  if (N <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) return L;
  L.tiles = (int64_t)((Cout + kW7TC - 1) / kW7TC) * ((Cin + kW7TC - 1) / kW7TC) * 7;
  const int64_t segs = (int64_t)N * H * ((W + kW7PX - 1) / kW7PX);
  // ~1024 workgroups in all (two a CU, two rounds), at least 4 segments each
  int64_t s = (1024 + L.tiles - 1) / L.tiles;
  if (s > segs / 4) s = segs / 4;
  if (s < 1) s = 1;
  L.sps = (segs + s - 1) / s;
  L.splits = (int)((segs + L.sps - 1) / L.sps);
  L.part = c.take((size_t)L.splits * Cout * Cin * 49);
  L.bpart = c.take((size_t)L.splits * Cout);
  L.bytes = c.bytes;
  return L;
}

}  // namespace rpst

using namespace rpst;

extern "C" size_t rpst_conv7_wgrad_workspace_size(int N, int Cin, int H, int W, int Cout) {
  return wgrad7_layout(nullptr, N, Cin, H, W, Cout).bytes;
}

extern "C" int rpst_conv7_wgrad(const float* x, const float* dy, float* dw, float* db, int N,
                                int Cin, int H, int W, int Cout, int pad_mode, void* workspace,
                                size_t workspace_bytes, rpst_stream_t stream) {
  RPST_REQUIRE(x && dy && dw, "conv7_wgrad: null pointer");
  RPST_REQUIRE(N > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0, "conv7_wgrad: bad shape");
  RPST_REQUIRE(pad_mode == RPST_PAD_ZERO || pad_mode == RPST_PAD_REFLECT,
               "conv7_wgrad: bad pad %d", pad_mode);
  RPST_REQUIRE(pad_mode != RPST_PAD_REFLECT || (H >= 4 && W >= 4),
               "conv7_wgrad: reflect padding 3 needs H,W >= 4 (got %d x %d)", H, W);
  // one image's tensors (plus a tile of channel padding) addressable by a 31-bit offset
  RPST_REQUIRE(((int64_t)(Cout > Cin ? Cout : Cin) + kW7TC) * H * W * 4 < (1LL << 31),
               "conv7_wgrad: one image's tensor exceeds 2 GiB");
  RPST_REQUIRE((int64_t)N * H * W < (1LL << 40), "conv7_wgrad: tensor too large");
  const Wgrad7Layout L = wgrad7_layout(workspace, N, Cin, H, W, Cout);
  RPST_REQUIRE_WS(L.bytes, "conv7_wgrad: workspace too small");
  RPST_REQUIRE(L.tiles <= 0x7fffffffLL && L.splits <= 65535, "conv7_wgrad: grid too large");
  hipStream_t st = as_stream(stream);
  conv7_wgrad_kernel<<<dim3((unsigned)L.tiles, (unsigned)L.splits), 256, 0, st>>>(
      x, dy, L.part, db ? L.bpart : nullptr, N, Cin, H, W, Cout, L.sps,
      pad_mode == RPST_PAD_REFLECT);
  if (int e = launch_status("conv7_wgrad_kernel")) return e;
  const int64_t n = (int64_t)Cout * Cin * 49;
  wgrad_reduce_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(L.part, dw, n, L.splits);
  if (int e = launch_status("wgrad_reduce_kernel")) return e;
  if (db) {
    wgrad_reduce_kernel<<<(unsigned)((Cout + 255) / 256), 256, 0, st>>>(L.bpart, db, Cout,
                                                                        L.splits);
    return launch_status("wgrad_reduce_kernel(bias)");
  }
  return RPST_OK;
}

extern "C" int rpst_reflect_pad_backward(const float* gp, float* dx, int64_t planes, int H,
                                         int W, int pad, rpst_stream_t stream) {
  RPST_REQUIRE(gp && dx, "reflect_pad_backward: null pointer");
  RPST_REQUIRE(planes > 0 && H > 0 && W > 0 && pad >= 0, "reflect_pad_backward: bad shape");
  RPST_REQUIRE(pad < H && pad < W,
               "reflect_pad_backward: reflect padding %d needs H,W > %d (got %d x %d)", pad, pad,
               H, W);
  const int64_t n = planes * H * W;
  RPST_REQUIRE(planes < (1LL << 40) / ((int64_t)(H + 2 * pad) * (W + 2 * pad)) &&
                   (n + 255) / 256 <= 0x7fffffffLL,
               "reflect_pad_backward: tensor too large");
  reflect_pad_backward_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(
      gp, dx, planes, H, W, pad);
  return launch_status("reflect_pad_backward_kernel");
}
