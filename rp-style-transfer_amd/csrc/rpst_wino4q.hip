// Winograd F(4x4, 3x3) on fp32 MFMA, position-quarter form (gfx950): the large 3x3 layers
// with >= 64 output channels of the reference hot path (network/base.py:25-111,363-396;
// sanet.py:162-192). Same arithmetic as rpst_wino4.hip (Y = A^T [U (.) V] A, U = G g G^T in
// fp64 rounded once, everything else fp32 on the true-fp32 MFMA); what changes is how the
// 36 transformed positions are spread over the waves.
//
// rpst_wino4.hip gives a wave 32 output channels x 18 positions x 16 tiles: each transformed
// input value V feeds 2 MFMAs (the two 16-channel halves), and the input transform (72 VALU
// per K step and wave) serialises with the fp32 MFMA on the SIMD (tools/coexec.hip) -- 20 % of
// the launch at 128->256. Here a wave owns 64 output channels x 9 positions x 16 tiles (still
// 144 accumulator registers): positions of one QUARTER of the 6x6 transformed tile (rows
// 3qr..3qr+2, columns 3qc..3qc+2), so each V value feeds 4 MFMAs and the transform is 48 VALU
// per 36 MFMAs (the column pass 3 of 6 outputs per input row, the row pass 3 of 6). The freed
// registers pay for software pipelining: the transform of K step x + 1 (its patch rows read
// and transformed one row per MFMA group) runs inside step x's MFMA stream, so no VALU chain
// and no LDS read latency sits between a step's barrier and its first MFMA.
//
// Block = 8 waves (two per SIMD), output 8 rows x 64 columns x 64 channels: wave w owns tile
// row w >> 2 and quarter w & 3. Per K step (4 input channels) the weight slice (64 co x 36
// positions x 4 ci = 36 KiB) and the patch (4 channels x 10 rows x 72) stream into an LDS ring
// (2 weight stages, 4 patch stages) by LDS-DMA: W(x + 1) and P(x + 4) are issued inside step
// x. The four quarters of a tile row meet in the epilogue: each wave sends its 9 positions of
// the other three quarters' 16-channel blocks through a weight stage (6 passes of 2
// accumulator elements x 3 positions) and finishes its own block with the full output
// transform.
#include "rpst_conv.h"

#include <type_traits>

// timing-only experiments (results wrong; tools/build_variants.sh -DRPST_W4Q_DBG=n): 1 no patch
// DMA, 2 no weight DMA, 4 no epilogue exchange, 8 no input transform, 16 no step barriers,
// 32 no epilogue at all, 64 no output stores (issued never), 128 no DMA waits. Round 6 on the
// final kernel, 128->256 @512^2 N64 (profiles/r06/epilogue_ab.log): 26.8 ms; no epilogue 25.3;
// no output stores 24.8; no exchange 25.7; no output transform (a bit since removed) 26.1
#ifndef RPST_W4Q_DBG
#define RPST_W4Q_DBG 0
#endif

namespace rpst {
namespace {

// acc += a * b on v_mfma_f32_16x16x4_f32 with the accumulator tied in place ("+v"). The
// builtin's untied form lets the register allocator rename every accumulator tuple each K
// step (dst != srcC): with 144 accumulator registers that costs 60-100 more and spills.
// hipcc pads no hazard around an asm statement (cdna_hip_programming.md 5.7): an MFMA's
// result taken whole as the next MFMA's C needs no wait states (the chain here); PAD = 1
// opens the statement with s_nop 1 (2 states: an operand a VALU wrote just before); readers
// of the results other than the chain go behind q_mfma_fence.
template <int PAD>
__device__ __forceinline__ void q_mfma(floatx4& acc, float a, float b) {
  if constexpr (PAD)
    asm volatile("s_nop 1\n\tv_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
  else
    asm volatile("v_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "v"(b));
}
// LDS-DMA issue (buffer_load ... lds) as inline asm, M0 written in the same statement
// (cdna_hip_programming.md 5.7): the compiler then tracks none of the ring's DMA, so it inserts
// no vmcnt of its own before the ring's LDS reads (its alias analysis cannot separate the
// padding pieces' dummy target from the stages and drained the ring to vmcnt(1) after every
// barrier); the ring's waits are the counted ones of wait_ring. "memory": no LDS access of
// the compiler's moves across an issue.
__device__ __forceinline__ unsigned q_lds_addr(const float* p) {
  return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) float*)p;
}
// m0: the LDS byte address lane 0 writes; OFF: the instruction offset, which gfx950 adds to the
// global and to the LDS address alike (LDS address = LDS base + M0 + OFF + 16 lane; checked by
// tests/test_gpu_conv_ring.py, which fails with M0 advanced by OFF as well), so a wave's
// contiguous pieces share one M0 value and one soffset
template <int OFF>
__device__ __forceinline__ void q_dma16(__amdgpu_buffer_rsrc_t r, unsigned m0, unsigned voff,
                                        int soff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen offset:%4 lds"
               :: "s"(m0), "v"(voff), "s"(r), "s"(soff), "i"(OFF) : "memory");
}
__device__ __forceinline__ void q_dma4(__amdgpu_buffer_rsrc_t r, unsigned m0, unsigned voff,
                                       int soff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %3 offen lds"
               :: "s"(m0), "v"(voff), "s"(r), "s"(soff) : "memory");
}
// the lane's index in its wave, derived where it is called (mbcnt over an opaque zero, 3 VALU):
// the epilogue's lane coordinates kept from the kernel's start would be live across the K
// loop, which has no VGPR to spare
__device__ __forceinline__ int q_lane_here() {
  int z = 0;
#if __HIP_DEVICE_COMPILE__
  asm volatile("" : "+v"(z));
#endif
  return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, (unsigned)z));
}
__device__ __forceinline__ void q_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

// B^T half-transform of one 6-vector: H = 0 -> outputs 0, 1, 2 (inputs 0..4); H = 1 ->
// outputs 3, 4, 5 (inputs 1..5). 6 VALU.
template <int H>
__device__ __forceinline__ void q_bt3(float d0, float d1, float d2, float d3, float d4, float d5,
                                      float& u0, float& u1, float& u2) {
  if constexpr (H == 0) {
    const float A = fmaf(-4.f, d2, d4), B = fmaf(-4.f, d1, d3);
    u0 = fmaf(4.f, d0, fmaf(-5.f, d2, d4));
    u1 = A + B;
    u2 = A - B;
  } else {
    const float C = d4 - d2, E = d3 - d1;
    u0 = fmaf(2.f, E, C);
    u1 = fmaf(-2.f, E, C);
    u2 = fmaf(4.f, d1, fmaf(-5.f, d3, d5));
  }
}

}  // namespace

constexpr int kQCo = 64;                     // output channels per co tile
constexpr int kQTH = 8, kQTW = 64;           // output rows x columns per block
// patch rows are staged from x0 - 4 (16-B aligned sources for the interior blocks' 16-B
// pieces), so column x0 - 1 sits at LDS column kQXO - 1 = 3
constexpr int kQXO = 4;                      // patch columns staged left of the tile
constexpr int kQPS = 72;                     // patch row stride (floats): columns 3 .. 68 used
constexpr int kQCS = 768;                    // patch channel stride (floats)
constexpr int kQWS = 9216;                   // weight floats per (co tile, K step)
constexpr int kQPAT = 4 * kQCS;              // patch stage: 4 channels (12 KiB)
constexpr int kQNTH = 512;
constexpr int kQMaxCo = 512;                 // output channels the LDS bias table holds
constexpr int kQWPI = 5;                     // 1-KiB weight pieces per wave and step (36 / 8)
constexpr int kQWide = 2, kQSlow = 6;        // patch pieces per wave and step: 16-B / 4-B
constexpr int kQDMA4 = 3, kQDMA = 12;        // patch pieces per channel: 16-B / 4-B
constexpr int kQRP = kQPS / 4;               // 16-B pieces per patch row
constexpr int kQXS = 4 * 3 * 3 * 64 * 2;     // epilogue exchange floats per tile row and pass
constexpr int kQWG0 = 0;  // MFMA group of a step whose issue slot takes the first W(x + 1) piece
constexpr int kQPG = 5;   // MFMA group after which the P(x + 4) pieces are issued
// MFMA groups whose A operands are read ahead: configs[1] 539.7 / 541.7 img/s at 2, 545.2 /
// 546.6 at 3 (128->256 N64 28.05 -> 27.65 ms), 537 at 4, 522 at 5 (tools/ab_bench_libs.sh,
// profiles/r05/ahead_ab.log; re-swept with kQPG and kQWG0 in profiles/r06/placement_resweep.log)
constexpr int kQAhead = 3;
static_assert(10 * kQRP <= kQDMA4 * 64 && kQDMA4 * 256 <= kQCS, "16-B pieces in a channel");
static_assert(10 * kQPS <= kQDMA * 64 && kQDMA * 64 <= kQCS, "4-B pieces in a channel");
static_assert(2 * kQWide >= kQDMA4 && 2 * kQSlow >= kQDMA && 8 * kQWPI >= 36, "coverage");
static_assert(2 * kQXS <= kQWS, "the exchange fits a weight stage");
constexpr int kQEpiB = 1024;  // epilogue context: two tile-row records + 32 row-offset vectors
static_assert((2 * kQWS + 4 * kQPAT) * 4 + 1024 + kQSlow * kQNTH * 4 + 9 * kQMaxCo * 4 + kQEpiB <=
                  163840,
              "LDS");

// ---- weight transform + packing -------------------------------------------------------
// packed[((((ct * K4 + ks) * 4 + q) * 9 + p) * 64 + l) * 4 + cb] = U_xi[co][ci] with
// xi = (3 (q >> 1) + p / 3, 3 (q & 1) + p % 3) (transformed row, column), co = 64 ct + 16 cb +
// (l & 15), ci = 4 ks + (l >> 4): lane l's A operands of position p for the four 16-channel
// blocks are one 16-B word, and one (co tile, K step) slice is contiguous (the LDS-DMA copies
// it verbatim). TW = float (the layer's weights) or double (per-image folded weights).
template <typename TW>
__global__ void wino4q_pack_kernel(const TW* __restrict__ w, float* __restrict__ pk, int Cout,
                                   int Cin, int K4, int64_t per, int64_t total, int64_t sco,
                                   int64_t sci, int64_t stap) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int64_t img = t / per;
  pk += img * per;
  w += img * (int64_t)Cout * Cin * 9;
  t -= img * per;
  const int cb = (int)(t & 3);
  int64_t r = t >> 2;
  const int l = (int)(r & 63);
  r >>= 6;
  const int p = (int)(r % 9);
  r /= 9;
  const int q = (int)(r & 3);
  r >>= 2;
  const int ks = (int)(r % K4);
  const int ct = (int)(r / K4);
  const int i = 3 * (q >> 1) + p / 3, jj = 3 * (q & 1) + p % 3;
  const int co = ct * kQCo + cb * 16 + (l & 15);
  const int ci = ks * 4 + (l >> 4);
  float v = 0.f;
  if (co < Cout && ci < Cin) {
    const double G[6][3] = {{0.25, 0, 0},
                            {-1.0 / 6, -1.0 / 6, -1.0 / 6},
                            {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                            {1.0 / 24, 1.0 / 12, 1.0 / 6},
                            {1.0 / 24, -1.0 / 12, 1.0 / 6},
                            {0, 0, 1}};
    const TW* g = w + co * sco + ci * sci;
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
      for (int s = 0; s < 3; ++s) acc += G[i][u] * (double)g[(u * 3 + s) * stap] * G[jj][s];
    v = (float)acc;
  }
  pk[t] = v;
}

size_t wino4q_packed_floats(int Cout, int Cin) {
  return (size_t)((Cout + kQCo - 1) / kQCo) * ((Cin + 3) / 4) * kQWS;
}

int wino4q_pack(const float* w, float* pk, int Cout, int Cin, hipStream_t st) {
  const int64_t t = (int64_t)wino4q_packed_floats(Cout, Cin);
  wino4q_pack_kernel<float><<<(unsigned)((t + 255) / 256), 256, 0, st>>>(
      w, pk, Cout, Cin, (Cin + 3) / 4, t, t, (int64_t)Cin * 9, 9, 1);
  return launch_status("wino4q_pack_kernel");
}

// per-image folded weights (wino4_mix): W'_n in [n][tap][co][ci] (fp64)
int wino4q_pack_mix(const double* wm, float* pk, int N, int Cout, int Cin, hipStream_t st) {
  const int64_t per = (int64_t)wino4q_packed_floats(Cout, Cin), tot = (int64_t)N * per;
  wino4q_pack_kernel<double><<<(unsigned)((tot + 255) / 256), 256, 0, st>>>(
      wm, pk, Cout, Cin, (Cin + 3) / 4, per, tot, Cin, 1, (int64_t)Cout * Cin);
  return launch_status("wino4q_pack_kernel(mix)");
}

// AdaIN folded into per-image weights: out_n = U scaled by s = std_s / std_c along ci
// (aux = [mean_c | mean_s | std_c | std_s], each N * Cin)
__global__ void wino4q_fold_w_kernel(const float4* __restrict__ pk, float4* __restrict__ out,
                                     const float* __restrict__ aux, int N, int Cin, int K4,
                                     int64_t per4) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)N * per4) return;
  const int n = (int)(t / per4);
  const int64_t u = t - (int64_t)n * per4;  // float4 index: ((ct * K4 + ks) * 36 + q * 9 + p) * 64 + l
  const int l = (int)(u & 63);
  const int ks = (int)((u / (kQWS / 4)) % K4);
  const int ci = ks * 4 + (l >> 4);
  const int64_t nc = (int64_t)N * Cin, i = (int64_t)n * Cin + (ci < Cin ? ci : 0);
  const float sc = ci < Cin ? aux[3 * nc + i] / aux[2 * nc + i] : 0.f;
  const float4 v = pk[u];
  out[t] = make_float4(v.x * sc, v.y * sc, v.z * sc, v.w * sc);
}

int wino4q_fold_w(const float* pk, float* out, const float* aux, int N, int Cout, int Cin,
                  hipStream_t st) {
  const int64_t per4 = (int64_t)wino4q_packed_floats(Cout, Cin) / 4, n4 = (int64_t)N * per4;
  wino4q_fold_w_kernel<<<(unsigned)((n4 + 255) / 256), 256, 0, st>>>(
      reinterpret_cast<const float4*>(pk), reinterpret_cast<float4*>(out), aux, N, Cin,
      (Cin + 3) / 4, per4);
  return launch_status("wino4q_fold_w_kernel");
}

// the layers this kernel takes: DMA loaders (NONE, UPSAMPLE2), >= 64 output channels (a
// 64-channel co tile; narrower layers stay on rpst_wino4.hip's 32-channel tile) and >= 128
// input channels in multiples of 16 (a co tile = a whole number of 4-step ring turns).
// Below 128 input channels a block's 8-16 K steps per co tile leave the prologue and the
// 4-way epilogue exposed: 32->64 @512^2 N64 3.12 vs 2.54 ms, 64->128 8.16 vs 8.09 on the
// 32-channel kernel (profiles/r05). ConvMode::quarter (the calling
// thread's rpst_conv2d_set_quarter, else RPST_W4Q read per launch like RPST_CONV_ALGO): 0
// off, 1 the rule above, 2 forced on for every shape it supports (Cin >= 16; parity tests,
// A/B). A training step's constant branches (rpst_conv2d_set_precise(2)) keep the 32-channel
// form: same per-conv error (tools/conv_err.py), but the gradient goldens were pinned on its
// rounding pattern.
bool wino4q_applies(int Cin, int Cout, int in_op, const ConvMode& m) {
  const int min_cin = m.quarter == 2 ? 16 : 128;
  return m.quarter && m.precise != 2 && (in_op == RPST_IN_NONE || in_op == RPST_IN_UPSAMPLE2) &&
         Cout >= 64 && Cout <= kQMaxCo &&
         Cin >= min_cin && Cin % 16 == 0;
}

// statistics partials per tile row of 4 rows x 64 columns, in [n][partial][co] order
ConvTiling wino4q_tiling(ConvArgs& a) {
  a.Cout_pad = (a.Cout + kQCo - 1) / kQCo * kQCo;
  a.nchunks = (a.Cin + 3) / 4;  // K steps of 4 channels
  a.tiles_x = (a.W + kQTW - 1) / kQTW;
  a.tiles_y = (a.H + kQTH - 1) / kQTH;
  a.co_tiles = a.Cout_pad / kQCo;
  a.stat_P = a.tiles_x * a.tiles_y * 2;
  // one block per spatial tile loops over every co tile: splitting them over 2 / 4 same-XCD
  // blocks measured 27.70 / 29.04 ms against 27.08 at 128->256 @512^2 N64 (the longer blocks
  // amortise the ring's prologue; profiles/r05/order_ab.log has the re-run under the final order)
  a.cosplit = 1;
  return {(int64_t)a.tiles_x * a.tiles_y * a.N, kQNTH, 4, kQTH / 4, kQTW, true};
}

// ---- the epilogue of one finished 4x4 tile and channel ---------------------------------
// What it needs besides the tile never changes over the life of a block, so it is derived
// once, before the ring starts (q_epi_fill), into LDS: one record per tile row wr and one
// vector of output row offsets per (wr, tn). Each channel's epilogue reads them back with LDS
// instructions only (q_finish): kept in registers across the exchange passes the context
// overflows the scalar registers, and re-derived from the kernel arguments per channel (the
// form this replaces) it cost scalar loads, three integer divisions and the flag arithmetic
// four times per co tile and wave with no MFMA in flight to hide them.
struct QEpiRec {
  float* oimg;       // bst: image n's output planes, obytes bytes (0: an image past skip_from)
  float* out;
  float2* stat;      // channel 0's statistics partial of (n, this tile row)
  unsigned obytes;
  unsigned hw4;      // bytes of one output plane (bst)
  int W, H, Cout, gy0, bx0, rows, n;
  unsigned flags;    // kQF*
  float inv, slope;
};
constexpr unsigned kQFFull = 1, kQFEdge = 2, kQFBst = 4, kQFPool = 8, kQFStore = 16;
// (a pointer read back from LDS is generic; these keep the epilogue's stores global_store)
typedef float floatx2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) floatx2 gfloatx2;
typedef __attribute__((address_space(1))) floatx4 gfloatx4;
static_assert(2 * (sizeof(QEpiRec) + 15) / 16 * 16 + 2 * 16 * 16 <= kQEpiB, "LDS");

// Block order (w4_tile; tools/ab_bench_libs.sh, profiles/r05/order_ab.log; configs[1], two
// rounds): row tile fastest with the hardware's round-robin XCD assignment (consecutive blocks
// on consecutive XCDs) 553.3 / 553.1 img/s; column tile fastest with consecutive logical blocks
// on one XCD (the round-4 choice) 548.3 / 547.3; row tile fastest on one XCD 534.7; column
// tile fastest round-robin 536.2; image-fastest orders 503-538.
//
// thread t < 32 of block (tx, ty, n) derives the context of tile (wr, tn) = (t >> 4, t & 15);
// tn = 0 writes its tile row's record
__device__ __forceinline__ void q_epi_fill(const ConvArgs& a, int tx, int ty, int n, int t,
                                           QEpiRec* recs, uint4* voffs) {
  const int wr = t >> 4, tn = t & 15;
  const int bx0 = tx * kQTW, gy0 = ty * kQTH + 4 * wr, gx0 = bx0 + 4 * tn;
  const int rows = max(0, min(4, a.H - gy0));
  unsigned vo[4];
#pragma unroll
  for (int yy = 0; yy < 4; ++yy)
    vo[yy] = (yy < rows && gx0 < a.W) ? (unsigned)(((gy0 + yy) * a.W + gx0) * 4) : 0x80000000u;
  voffs[t] = make_uint4(vo[0], vo[1], vo[2], vo[3]);
  if (tn) return;
  QEpiRec r;
  r.W = a.W;
  r.H = a.H;
  r.Cout = a.Cout;
  r.gy0 = gy0;
  r.bx0 = bx0;
  r.rows = rows;
  r.n = n;
  r.slope = a.relu == RPST_ACT_RELU ? 0.f : (a.relu == RPST_ACT_LRELU ? 0.2f : 1.f);
  const int cols = max(0, min(kQTW, a.W - bx0));
  // (v_rcp: exact for the 256-pixel full tiles)
  r.inv = rows * cols > 0 ? __builtin_amdgcn_rcpf((float)(rows * cols)) : 0.f;
  const int64_t plane = (int64_t)a.H * a.W;
  const bool full = rows == 4 && bx0 + kQTW <= a.W;
  const bool edge = gy0 == 0 || gy0 + 4 >= a.H || bx0 == 0 || bx0 + kQTW >= a.W;
  const bool pool = a.pool_out != 0;
  const bool bst = !pool && (a.W & 3) == 0 && (int64_t)a.Cout * plane * 4 < (1LL << 31);
  const bool keep = a.skip_from <= 0 || n < a.skip_from;
  r.flags = (full ? kQFFull : 0u) | (edge ? kQFEdge : 0u) | (bst ? kQFBst : 0u) |
            (pool ? kQFPool : 0u) | (keep ? kQFStore : 0u);
  r.out = a.out;
  r.oimg = a.out + (int64_t)n * a.Cout * plane;
  r.obytes = keep ? (unsigned)(a.Cout * plane * 4) : 0u;
  r.hw4 = (unsigned)(a.H * a.W) * 4u;
  const int sidx = (ty * a.tiles_x + tx) * 2 + wr;
  r.stat = a.stat_part ? a.stat_part + ((int64_t)n * a.stat_P + sidx) * a.Cout : nullptr;
  recs[wr] = r;
}

// a wave-uniform value read from LDS, moved to scalar registers (the buffer descriptor built
// from VGPRs is otherwise re-read lane by lane in a loop around every store)
__device__ __forceinline__ unsigned uni(unsigned v) {
  return (unsigned)__builtin_amdgcn_readfirstlane((int)v);
}
__device__ __forceinline__ float* uni(float* p) {
  const uint64_t u = (uint64_t)(uintptr_t)p;
  return (float*)(uintptr_t)(((uint64_t)uni((unsigned)(u >> 32)) << 32) | uni((unsigned)u));
}

// bias (interior class for BTAB) already in Y; border classes, activation, statistics
// partial, store (or 2x2 ceil-mode max pool) of channel co of this lane's tile (column tn of
// tile row r); vo = its output row offsets, cofs = co's byte offset inside the image's output
// (co hw4, a running value of the caller's). The record's fields are read where they are
// used: read ahead into one struct, the twenty of them sit in VGPRs beside the tile, and the
// statistics epilogue has none to spare.
template <bool STATS, bool BTAB, bool RELU>
__device__ __forceinline__ void q_finish(const QEpiRec& r, const uint4& vo, const float* btab,
                                         int co, unsigned cofs, float (&Y)[16], int tn) {
  const unsigned f = r.flags;
  const bool full = (f & kQFFull) != 0;
  const bool cok = co < r.Cout;
  if constexpr (BTAB) {
    if (f & kQFEdge) {
      const int gy0 = r.gy0, gx0 = r.bx0 + 4 * tn, H = r.H, W = r.W;
      const float* bt = btab + (cok ? co : 0) * 9;  // this image's table, in LDS
      float b9[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) b9[i] = cok ? bt[i] : 0.f;
      const float b4 = b9[4];
#pragma unroll
      for (int i = 0; i < 9; ++i) b9[i] -= b4;
#pragma unroll
      for (int yy = 0; yy < 4; ++yy) {
        const int gy = gy0 + yy;
        const int rc = gy == 0 ? 0 : (gy >= H - 1 ? 2 : 1);
        const float l = rc == 0 ? b9[0] : (rc == 2 ? b9[6] : b9[3]);
        const float m = rc == 0 ? b9[1] : (rc == 2 ? b9[7] : b9[4]);
        const float rr = rc == 0 ? b9[2] : (rc == 2 ? b9[8] : b9[5]);
#pragma unroll
        for (int xx = 0; xx < 4; ++xx) {
          const int gx = gx0 + xx;
          Y[yy * 4 + xx] += gx == 0 ? l : (gx >= W - 1 ? rr : m);
        }
      }
    }
  }
  if constexpr (RELU) {
#pragma unroll
    for (int i = 0; i < 16; ++i) Y[i] = __builtin_amdgcn_fmed3f(Y[i], 0.f, __builtin_inff());
  } else {
    const float slope = r.slope;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      Y[i] = __builtin_amdgcn_fmed3f(Y[i], slope * Y[i], __builtin_inff());
  }
  float sum = 0.f;
  if constexpr (STATS) {
    if (full) {
#pragma unroll
      for (int i = 0; i < 16; ++i) sum += Y[i];
    } else {
      const int rows = r.rows, gx0 = r.bx0 + 4 * tn, W = r.W;
#pragma unroll
      for (int yy = 0; yy < 4; ++yy)
#pragma unroll
        for (int xx = 0; xx < 4; ++xx) sum += (yy < rows && gx0 + xx < W) ? Y[yy * 4 + xx] : 0.f;
    }
  }
  if ((RPST_W4Q_DBG & 64) && r.H > -7) {  // timing only: the stores never taken
  } else if (f & kQFBst) {
    const auto ro = rsrc_or_zero(uni(r.oimg), uni(r.obytes), true);
    const unsigned chofs = cok ? cofs : 0x7fffffffu;
    const unsigned voff[4] = {vo.x, vo.y, vo.z, vo.w};
#pragma unroll
    for (int yy = 0; yy < 4; ++yy) {
      const floatx4 v = {Y[yy * 4], Y[yy * 4 + 1], Y[yy * 4 + 2], Y[yy * 4 + 3]};
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), ro,
                                             (int)(voff[yy] + chofs), 0, 0);
    }
  } else if (f & kQFPool) {
    // max_pool2d(2, 2, ceil_mode) of the finished tile, fmaxf in maxpool2_kernel's order
    if (cok && (f & kQFStore)) {
      const int gy0 = r.gy0, gx0 = r.bx0 + 4 * tn, rows = r.rows, H = r.H, W = r.W;
      const int Ho = (H + 1) >> 1, Wo = (W + 1) >> 1;
      gfloat* o = (gfloat*)r.out + (((int64_t)r.n * r.Cout + co) * Ho + (gy0 >> 1)) * Wo +
                  (gx0 >> 1);
#pragma unroll
      for (int py = 0; py < 2; ++py) {
        if (2 * py >= rows) continue;
        const bool y1 = 2 * py + 1 < rows;
        float pv[2];
#pragma unroll
        for (int px = 0; px < 2; ++px) {
          const bool x1 = gx0 + 2 * px + 1 < W;
          const float* t = Y + (2 * py) * 4 + 2 * px;
          float v = t[0];
          if (x1) v = fmaxf(v, t[1]);
          if (y1) v = fmaxf(v, t[4]);
          if (x1 && y1) v = fmaxf(v, t[5]);
          pv[px] = v;
        }
        if (gx0 + 3 < W && (Wo & 1) == 0) {
          *(gfloatx2*)(o + py * Wo) = floatx2{pv[0], pv[1]};
        } else {
          if (gx0 < W) o[py * Wo] = pv[0];
          if (gx0 + 2 < W) o[py * Wo + 1] = pv[1];
        }
      }
    }
  } else if (cok && (f & kQFStore)) {
    const int gy0 = r.gy0, gx0 = r.bx0 + 4 * tn, rows = r.rows, H = r.H, W = r.W;
    const bool vec = (W & 3) == 0 && gx0 + 3 < W;
    gfloat* o = (gfloat*)r.out + (((int64_t)r.n * r.Cout + co) * H + gy0) * W + gx0;
#pragma unroll
    for (int yy = 0; yy < 4; ++yy) {
      if (yy < rows) {
        if (vec) {
          *(gfloatx4*)(o + yy * W) =
              floatx4{Y[yy * 4], Y[yy * 4 + 1], Y[yy * 4 + 2], Y[yy * 4 + 3]};
        } else {
#pragma unroll
          for (int xx = 0; xx < 4; ++xx)
            if (gx0 + xx < W) o[yy * W + xx] = Y[yy * 4 + xx];
        }
      }
    }
  }
  if constexpr (STATS) {
    sum = row16_sum(sum);
    const float mean = sum * r.inv;
    float m2 = 0.f;
    if (full) {
#pragma unroll
      for (int i = 0; i < 16; ++i) m2 = fmaf(Y[i] - mean, Y[i] - mean, m2);
    } else {
      const int rows = r.rows, gx0 = r.bx0 + 4 * tn, W = r.W;
#pragma unroll
      for (int yy = 0; yy < 4; ++yy)
#pragma unroll
        for (int xx = 0; xx < 4; ++xx) {
          const float dv = Y[yy * 4 + xx] - mean;
          m2 += (yy < rows && gx0 + xx < W) ? dv * dv : 0.f;
        }
    }
    m2 = row16_sum(m2);
    // partials in [n][partial][co] order (stat_merge_t_kernel): a wave's 16 channels of one
    // partial fill whole cache lines (in [n][co][partial] order they were 8-B pieces
    // scattered over 16 planes). Statistics cost, 128->256 N64 (tools/ab_stats.py): 1.5 ms
    // of 28.4, of which the store 0.2 and the centred-square pass 0.33
    if (tn == 0 && cok) ((gfloatx2*)r.stat)[co] = floatx2{mean, m2};
  }
}

template <int INOP, bool STATS, bool BTAB, bool RELU>
__global__ __launch_bounds__(kQNTH, 1) void wino4q_mfma_kernel(ConvArgs a) {
  // ring: weights in 2 stages (W(x) in wsx % 2), patches in 4 (P(x) in ps x % 4); a co tile
  // has a multiple of 4 K steps (wino4q_applies: Cin % 16 == 0), so its steps run as a
  // 4-unrolled loop whose stage objects are fixed per position, and its last step always
  // reads ws1 -- the epilogue's exchange region. One __shared__ object per stage: the stage a
  // step reads and the ones its DMA fills are distinct objects, so the compiler's wait
  // insertion does not drain the in-flight DMA before the LDS reads.
  __shared__ __attribute__((aligned(16))) float ws0[kQWS];
  __shared__ __attribute__((aligned(16))) float ws1[kQWS];
  __shared__ __attribute__((aligned(16))) float ps0[kQPAT];
  __shared__ __attribute__((aligned(16))) float ps1[kQPAT];
  __shared__ __attribute__((aligned(16))) float ps2[kQPAT];
  __shared__ __attribute__((aligned(16))) float ps3[kQPAT];
  __shared__ __attribute__((aligned(16))) float dummy[256];  // target of padding DMA pieces
  // per-lane patch source offsets (in registers they are spilled, and every reload's vmcnt
  // wait drains the DMA ring): each lane reads only its own column
  __shared__ unsigned poffs[kQSlow][kQNTH];
  // the layer's biases (BTAB: this image's 9 border-class biases per channel), copied once
  // per block before the ring starts: a global load in the epilogue would take a
  // compiler-inserted vmcnt(0) that drains the in-flight DMA ring (wino4q_applies: Cout <= 512)
  __shared__ float btl[BTAB ? 9 * kQMaxCo : kQMaxCo];

  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  // (lane, tid: not const -- each quarter body below derives its own copies, see there)
  int lane = threadIdx.x & 63;
  const int wr = wave >> 2;

  // block -> (co-split group, row tile, column tile, image)
  int bid = (int)blockIdx.x;
  const int cog = bid % a.cosplit;
  bid /= a.cosplit;
  const int nct = a.co_tiles / a.cosplit, ct0 = cog * nct;
  int tx, ty, n;
  w4_tile(bid, a.tiles_x, a.tiles_y, tx, ty, n);
  const int K4 = a.nchunks, G = nct * K4;
  const int y0 = ty * kQTH, x0 = tx * kQTW;

  {
    const int nb = BTAB ? 9 * a.Cout : a.Cout;
    const float* src = BTAB ? a.btab + (int64_t)n * nb : a.bias;
    for (int i = threadIdx.x; i < nb; i += kQNTH) btl[i] = src ? src[i] : 0.f;
  }
  // the epilogue's context (QEpiRec, q_epi_fill), published by the prologue's barrier
  __shared__ __attribute__((aligned(16))) QEpiRec erec[2];
  __shared__ uint4 evoff[2 * 16];
  if (threadIdx.x < 32) q_epi_fill(a, tx, ty, n, (int)threadIdx.x, erec, evoff);
  constexpr bool up = INOP == RPST_IN_UPSAMPLE2;
  const unsigned in_plane = up ? (unsigned)(a.Hs * a.Ws) : (unsigned)(a.H * a.W);
  const unsigned oob = a.Cin * in_plane * 4u;  // a padding position's (out-of-range) offset
  const float* in_img = conv_in_img(a, n, (int64_t)a.Cin * in_plane);
  const unsigned wbytes = (unsigned)(nct * K4 * kQWS) * 4u;  // this block's co tiles
  const float* w_img = a.wpk + (int64_t)n * a.wstride + (int64_t)ct0 * K4 * kQWS;

  // patch of one K step: 4 channels x [10 rows][72] at channel stride 768, a row staged from
  // x0 - kQXO = x0 - 4, so the 66 window columns x0 - 1 .. x0 + 64 sit at LDS columns 3 .. 68
  // (0-2 and 69-71 are staged but never read); waves 2c, 2c + 1 fill channel c. Interior
  // blocks (every patch column inside the image, no upsampling): 16-B pieces (a 72-float row
  // = 18 pieces, 16-B aligned sources, 180 per channel, 3 wave-instructions: half 0 takes
  // 0-1, half 1 takes 2 + a padding piece); elsewhere 4-B pieces (element 64 p + lane
  // resolved against the padding, 12 per channel, 6 per half). Against 68-float rows staged
  // from x0 - 1 (4-B aligned sources) the aligned rows took 128->256 N64 from 26.69-26.94 to
  // 26.55-26.61 ms, folded 256->128 from 13.01-13.12 to 12.75-12.96
  // (profiles/r06/aligned_patch_ab.log).
  // Per-lane source offsets are resolved once per block.
  const int hf = wave & 1;
  const bool zp = a.pad == RPST_PAD_ZERO;
  const int rs = up ? a.Ws : a.W;
  // in a row of W % 4 == 0 floats a 16-B piece of the aligned rows is wholly inside or outside
  // the image, so the full-width x-edge tiles take the 16-B pieces too: outside pieces read
  // zero (zero padding), and reflect padding's one halo column is copied in after the stage
  // lands (fix_halo; profiles/r06/edge_tiles_ab.log)
  const bool w4a = (a.W & 3) == 0;
  const bool wide = !up && ((x0 >= 1 && x0 + kQTW < a.W) || (w4a && x0 + kQTW <= a.W));
  const bool fixL = wide && w4a && !zp && x0 == 0;
  const bool fixR = wide && w4a && !zp && x0 + kQTW == a.W;
  unsigned poff[kQSlow];
  int tid = threadIdx.x;
  if (wide) {
#pragma unroll
    for (int i = 0; i < kQWide; ++i) {
      const int p = kQWide * hf + i;
      const int f = 64 * p + lane, row = min(f / kQRP, 9), j = f - (f / kQRP) * kQRP;
      int y = y0 - 1 + row;
      const int xs = x0 - kQXO + 4 * j;
      const bool okx = !w4a || (xs >= 0 && xs + 3 < a.W);
      const bool ok = p < kQDMA4 && f < 10 * kQRP && resolve_bf(y, a.H, zp) && okx;
      poff[i] = ok ? ((unsigned)(y * rs) + (unsigned)xs) * 4u : oob;
    }
#pragma unroll
    for (int i = kQWide; i < kQSlow; ++i) poff[i] = oob;
  } else {
#pragma unroll
    for (int i = 0; i < kQSlow; ++i) {
      const int p = kQSlow * hf + i;
      const int f = 64 * p + lane;
      const int row = min(f / kQPS, 9), col = f - (f / kQPS) * kQPS;
      int y = y0 - 1 + row, x = x0 - kQXO + col;
      const bool oky = resolve_bf(y, a.H, zp), okx = resolve_bf(x, a.W, zp);
      const bool ok = p < kQDMA && col >= kQXO - 1 && col < kQXO + 1 + kQTW &&
                      f < 10 * kQPS && oky && okx;
      poff[i] = ok ? ((unsigned)((up ? y >> 1 : y) * rs) + (unsigned)(up ? x >> 1 : x)) * 4u : oob;
    }
  }
#pragma unroll
  for (int i = 0; i < kQSlow; ++i) poffs[i][tid] = poff[i];

  // weight slice of a step (the block's co tiles' slices are consecutive) into the stage at
  // LDS address stg: the stage is a verbatim copy of the slice's 36 1-KiB pieces, wave w
  // copies the contiguous pieces 4 w .. 4 w + 3 (i < 4: one m0, one soffset, the piece in the
  // instruction offset) and, for w < 4, piece 32 + w (i = 4); waves 4-7 issue a padding piece
  // into the dummy instead, so every wave issues kQWPI pieces and the counted waits hold.
  // Everything but the stage is wave-uniform and constant for a step: wso = the byte offset
  // of the wave's first piece (a running value, + one slice per step), live = the step
  // exists (dead steps and padding pieces read zero records; the range check takes the
  // voffset and the instruction offset, not the soffset, so that one is not masked).
  constexpr int DBG = RPST_W4Q_DBG;
  const int wl = wave * 4096;            // the wave's pieces inside a slice / a stage (bytes)
  const bool real4 = wave < 4;
  const int w4 = 32768 + wave * 1024;    // piece 32 + w
  const unsigned dummy_a = q_lds_addr(dummy);
  int wso = wl;
  auto issue_w = [&](bool live, unsigned stg, auto Ic) {
    constexpr int I = decltype(Ic)::value;
    if (DBG & 2) return;
    if constexpr (I < 4) {
      q_dma16<1024 * I>(rsrc_or_zero(w_img, wbytes, live), stg + wl, lane * 16, wso);
    } else {
      q_dma16<0>(rsrc_or_zero(w_img, wbytes, live && real4), real4 ? stg + w4 : dummy_a,
                 lane * 16, wso + (w4 - wl));
    }
  };
  // every patch piece of this wave for one step into the stage at LDS address stg; pso = the
  // byte offset of the wave's channel (a running value: + 4 channels per step, back to the
  // wave's first channel at a co tile's end; a co tile has whole K steps, Cin % 16 == 0)
  const unsigned pstep = 4u * in_plane * 4u;
  const int pbase = (int)((unsigned)(wave >> 1) * in_plane * 4u);
  const bool h1 = (wave & 1) != 0;
  const int pl = (wave >> 1) * (kQCS * 4) + (h1 ? (wide ? 2048 : kQSlow * 256) : 0);
  int pso = pbase;
  auto issue_p = [&](auto WIDEc, bool live, unsigned stg) {
    constexpr bool WIDE = decltype(WIDEc)::value;
    if (DBG & 1) return;
    const auto r = rsrc_or_zero(in_img, oob, live);
    // (pl opaque here: precomputed per stage and piece, the targets overflow the scalar
    // registers and come back by a v_readlane each; derived, a piece costs one s_add)
    const unsigned xs = stg + launder(pl);
    if constexpr (WIDE) {
      q_dma16<0>(r, xs, poffs[0][tid], pso);
      q_dma16<0>(r, h1 ? dummy_a : xs + 1024, poffs[1][tid], pso);
    } else {
#pragma unroll
      for (int i = 0; i < kQSlow; ++i) q_dma4(r, xs + 256 * i, poffs[i][tid], pso);
    }
    pso += (int)pstep;
  };
  // before step x's barrier: W(x) (issued in step x - 1 ahead of its patch group) and
  // everything older have landed; that youngest patch group (2 / 6 pieces) stays in flight
  // The first wait after an epilogue leaves its output stores in flight too: on the buffer-
  // store path (q_epi_ctx's bst, kernel-uniform) every wave issues exactly 16 (4 channels x 4
  // rows; the statistics partial stores come after them, so counting only these 16 is
  // conservative). Waiting them out (vmcnt(2)) stalled every co tile's first step on the
  // stores' write acknowledgements.
  const bool bst_all = !a.pool_out && (a.W & 3) == 0 &&
                       (int64_t)a.Cout * a.H * a.W * 4 < (1LL << 31);
  bool post_epi = false;
  auto wait_ring = [&](bool first) {
    if (DBG & 128) return;
    if (first && post_epi && bst_all) {
      if (wide) asm volatile("s_waitcnt vmcnt(18)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(22)" ::: "memory");
    } else if (wide) {
      asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    }
    if (first) post_epi = false;
  };

  // reflect halo of an x-edge tile staged from 16-B pieces: wave 0 copies column x0 + 1 (LDS
  // column kQXO + 1) into x0 - 1 (kQXO - 1), wave 1 column x0 + 62 into x0 + 64; lanes 0-39
  // take channel l / 10, row l % 10 of the stage
  auto fix_halo = [&](float* stg) {
    if ((wave == 0 && fixL) || (wave == 1 && fixR)) {
      const int l = q_lane_here();
      if (l < 40) {
        const int ch = l / 10, row = l - 10 * ch;
        float* rp = stg + ch * kQCS + row * kQPS;
        if (wave == 0) rp[kQXO - 1] = rp[kQXO + 1];
        else rp[kQXO + kQTW] = rp[kQXO + kQTW - 2];
      }
    }
  };
  // ---- prologue: P(0), P(1), W(0), P(2), P(3) -------------------------------------------
  auto prologue = [&](auto WIDEc) {
    issue_p(WIDEc, true, q_lds_addr(ps0));
    issue_p(WIDEc, true, q_lds_addr(ps1));
    issue_w(true, q_lds_addr(ws0), std::integral_constant<int, 0>{});
    issue_w(true, q_lds_addr(ws0), std::integral_constant<int, 1>{});
    issue_w(true, q_lds_addr(ws0), std::integral_constant<int, 2>{});
    issue_w(true, q_lds_addr(ws0), std::integral_constant<int, 3>{});
    issue_w(true, q_lds_addr(ws0), std::integral_constant<int, 4>{});
    issue_p(WIDEc, true, q_lds_addr(ps2));
    issue_p(WIDEc, true, q_lds_addr(ps3));
  };
  if (wide) prologue(std::true_type{});
  else prologue(std::false_type{});
  wait_ring(false);  // P(3) may stay in flight; conservative for P(2)
  q_lds_barrier();
  if (fixL || fixR) {  // P(0), P(1) (P(x + 2) is fixed in step x)
    fix_halo(ps0);
    fix_halo(ps1);
    q_lds_barrier();
  }

  auto body = [&](auto Qc) {
    constexpr int Q = decltype(Qc)::value, QR = Q >> 1, QC = Q & 1;
    // (the lane's coordinates per quarter body, the DMA issue's included: shared, they stay
    // live across the other quarters' bodies and spill)
    lane = q_lane_here();
    tid = wave * 64 + lane;
    const int k = lane >> 4, tn = lane & 15;
    floatx4 acc[9][4];
#pragma unroll
    for (int p = 0; p < 9; ++p)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) acc[p][cb] = floatx4{0.f, 0.f, 0.f, 0.f};
    // lane (k, tn) reads rows 4 wr + QR .. + 4 of channel k of a patch. Window columns
    // 4 tn .. + 5 sit at LDS columns 4 tn + 3 .. + 8: the quarter's five (QC = 0: 0-4, QC = 1:
    // 1-5) as one aligned ds_read_b128 (the empty asm keeps it whole) and a ds_read_b32 for the
    // odd one (all 64 lanes in one pass; the four channel groups k share its banks, but a
    // second whole b128 brought 13-17 VGPR spills back: profiles/r06/odd_column_read_ab.log)
    const int roff = k * kQCS + (4 * wr + QR) * kQPS + 4 * tn;
    auto read_row = [&](const float* stg, int rr, float (&d)[8]) {
      const float* rp = stg + roff + rr * kQPS;
      floatx4 u = *reinterpret_cast<const floatx4*>(rp + 4);
      const float e = QC ? rp[8] : rp[3];
      asm("" : "+v"(u));
      d[0] = QC ? 0.f : e; d[1] = u[0]; d[2] = u[1]; d[3] = u[2]; d[4] = u[3];
      d[5] = QC ? e : 0.f; d[6] = 0.f; d[7] = 0.f;
    };
    // column pass of one row (this quarter's 3 transformed columns)
    auto col_pass = [&](const float (&d)[8], float (&u)[3]) {
      if (DBG & 8) {
        u[0] = d[0]; u[1] = d[1]; u[2] = d[2];
        return;
      }
      q_bt3<QC>(d[0], d[1], d[2], d[3], d[4], d[5], u[0], u[1], u[2]);
    };
    // row pass of column j: u[rr] holds input row QR + rr, so QR = 1's half (inputs 1..5)
    // takes u[0..4] as its inputs 1..5. V[p], p = 3 i + j: transformed row 3 QR + i,
    // column 3 QC + j
    auto row_pass = [&](const float (&u)[5][3], int j, float (&v)[9]) {
      if (DBG & 8) {
        v[j] = u[0][j]; v[3 + j] = u[2][j]; v[6 + j] = u[4][j];
        return;
      }
      if constexpr (QR == 0)
        q_bt3<0>(u[0][j], u[1][j], u[2][j], u[3][j], u[4][j], 0.f, v[j], v[3 + j], v[6 + j]);
      else
        q_bt3<1>(0.f, u[0][j], u[1][j], u[2][j], u[3][j], u[4][j], v[j], v[3 + j], v[6 + j]);
    };
    float V[9];
    {  // V(0), not pipelined
      float u[5][3];
#pragma unroll
      for (int rr = 0; rr < 5; ++rr) {
        float d[8];
        read_row(ps0, rr, d);
        col_pass(d, u[rr]);
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) row_pass(u, j, V);
    }

    const int woff = Q * 9 * 256 + lane * 4;  // this wave's A operands in a weight stage
    int x = 0;                                // global K step
    // one K step: W(x) from wsx, P(x + 1) from psn (-> V(x + 1)), DMA W(x + 1) into wsn and
    // P(x + 4) into psx. MFMA groups in column-major position order, so the row pass of
    // column j overwrites V[j], V[3 + j], V[6 + j] after their last use.
    // (first: the step that may follow an epilogue, the first of an iteration)
    auto step = [&](float* wsx, float* psn, float* wsn, float* psx, float* pfx, int ks,
                    bool first) {
      wait_ring(first);
      // the step's DMA bookkeeping, once: W(x + 1) and P(x + 4) exist; their soffsets
      const bool wlive = x + 1 < G, plive = x + 4 < G;
      wso += kQWS * 4;
      if (first && ks + 4 == K4) pso = pbase;  // P(x + 4) .. P(x + 7) open the next co tile
      const unsigned wsn_a = q_lds_addr(wsn), psx_a = q_lds_addr(psx);
      if (DBG & 16) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      else q_lds_barrier();  // W(x), P(x + 1) complete; every wave is done with step x - 1
      constexpr int ord[9] = {0, 3, 6, 1, 4, 7, 2, 5, 8};
      constexpr int kA = kQAhead;  // A-operand groups read ahead
      float4 w4[9];
#pragma unroll
      for (int q = 0; q < kA; ++q)
        w4[ord[q]] = *reinterpret_cast<const float4*>(wsx + woff + ord[q] * 256);
      float d[8];
      read_row(psn, 0, d);
      float u[5][3];
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const int p = ord[q];
        if (q + kA < 9)
          w4[ord[q + kA]] = *reinterpret_cast<const float4*>(wsx + woff + ord[q + kA] * 256);
        q_mfma<1>(acc[p][0], w4[p].x, V[p]);  // V[p] / a zeroed accumulator may be fresh
        q_mfma<0>(acc[p][1], w4[p].y, V[p]);
        q_mfma<0>(acc[p][2], w4[p].z, V[p]);
        q_mfma<0>(acc[p][3], w4[p].w, V[p]);
        if (q == kQWG0) issue_w(wlive, wsn_a, std::integral_constant<int, 0>{});
        if (q == kQWG0 + 1) issue_w(wlive, wsn_a, std::integral_constant<int, 1>{});
        if (q == kQWG0 + 2) issue_w(wlive, wsn_a, std::integral_constant<int, 2>{});
        if (q == kQWG0 + 3) issue_w(wlive, wsn_a, std::integral_constant<int, 3>{});
        if (q == kQWG0 + 4) issue_w(wlive, wsn_a, std::integral_constant<int, 4>{});
        // P(x + 4): K step ks + 4 of this co tile, or of the next one
        if (q == kQPG) {
          if (wide) issue_p(std::true_type{}, plive, psx_a);
          else issue_p(std::false_type{}, plive, psx_a);
        }
        // pipelined transform of P(x + 1): rows at groups 0-4, column j's row pass at
        // groups 5, 6 and (after its MFMAs) 8
        if (q < 5) {  // row q (read one group ahead) -> u[q], then read row q + 1
          col_pass(d, u[q]);
          if (q + 1 < 5) read_row(psn, q + 1, d);
        }
        if (q == 5 || q == 6 || q == 8) row_pass(u, q == 8 ? 2 : q - 5, V);
        // P(x + 2) landed for every wave at this step's barrier and is read from step x + 1
        if (q == 7) fix_halo(pfx);
      }
      ++x;
    };

    // epilogue of co tile ctile (its last step read ws1): the quarters of a tile row exchange
    // their blocks through ws1 and each wave finishes its own 16 channels (co = 64 ctile +
    // 16 Q + 4 k + r) of tile (wr, tn)
    auto epilogue = [&](int ctile) {
      if (DBG & 32) {  // keep the accumulators live, skip the epilogue
        float t = 0.f;
#pragma unroll
        for (int p = 0; p < 9; ++p)
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) t += acc[p][cb][0];
        if (t == 1.2345f) late_args()->out[threadIdx.x] = t;
#pragma unroll
        for (int p = 0; p < 9; ++p)
#pragma unroll
          for (int cb = 0; cb < 4; ++cb) acc[p][cb] = floatx4{0.f, 0.f, 0.f, 0.f};
        return;
      }
      q_lds_barrier();  // every wave is done reading ws1
      // 12 wait states between the last MFMAs and the first reader of their results (8-pass
      // XDL), with every accumulator passed through the statements so no read moves above them
      asm volatile("s_nop 7\n\ts_nop 4" : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[0][2]),
                   "+v"(acc[0][3]), "+v"(acc[1][0]), "+v"(acc[1][1]), "+v"(acc[1][2]),
                   "+v"(acc[1][3]), "+v"(acc[2][0]), "+v"(acc[2][1]), "+v"(acc[2][2]),
                   "+v"(acc[2][3]), "+v"(acc[3][0]), "+v"(acc[3][1]), "+v"(acc[3][2]),
                   "+v"(acc[3][3]), "+v"(acc[4][0]), "+v"(acc[4][1]));
      asm volatile("" : "+v"(acc[4][2]), "+v"(acc[4][3]), "+v"(acc[5][0]), "+v"(acc[5][1]),
                   "+v"(acc[5][2]), "+v"(acc[5][3]), "+v"(acc[6][0]), "+v"(acc[6][1]),
                   "+v"(acc[6][2]), "+v"(acc[6][3]), "+v"(acc[7][0]), "+v"(acc[7][1]),
                   "+v"(acc[7][2]), "+v"(acc[7][3]), "+v"(acc[8][0]), "+v"(acc[8][1]),
                   "+v"(acc[8][2]), "+v"(acc[8][3]));
      const int el = q_lane_here(), ek = el >> 4, etn = el & 15;
      const int co0 = ctile * kQCo + 16 * Q + 4 * ek;
      unsigned cofs = (unsigned)co0 * erec[wr].hw4;  // + one plane per finished channel
      asm volatile("" : "+v"(cofs));  // (opaque: else each channel's offset is a multiply again)
      // 6 passes (accumulator element pair rp, position row pt): each wave writes its 3
      // positions of row pt of the other quarters' blocks (elements 2 rp, 2 rp + 1) into ws1
      // and, after a barrier, reads the other quarters' positions of its own block. After pass pt it holds transformed rows
      // pt and 3 + pt of M for channels co0 + 2 rp + {0, 1}: their column transform (A^T along
      // the row) runs at once, so only P = M A (6 x 4 per channel) stays live, never M.
#pragma unroll
      for (int rp = 0; rp < 2; ++rp) {
        float P[2][6][4];
#pragma unroll
        for (int pt = 0; pt < 3; ++pt) {
          float* xb = ws1 + wr * kQXS;
#pragma unroll
          for (int dq = 0; dq < 4; ++dq) {
            if (dq == Q || (DBG & 4)) continue;
            const int slot = (Q - dq - 1) & 3;
#pragma unroll
            for (int j = 0; j < 3; ++j)
              *reinterpret_cast<float2*>(xb + (((dq * 3 + slot) * 3 + j) * 64 + el) * 2) =
                  make_float2(acc[3 * pt + j][dq][2 * rp], acc[3 * pt + j][dq][2 * rp + 1]);
          }
          if (!(DBG & 4)) q_lds_barrier();
          float m[2][2][6];  // [element][row pt / 3 + pt][six columns]
#pragma unroll
          for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
              float2 v;
              if (s == Q || (DBG & 4)) {
                const int src = (DBG & 4) ? s : Q;
                v = make_float2(acc[3 * pt + j][src][2 * rp], acc[3 * pt + j][src][2 * rp + 1]);
              } else {
                v = *reinterpret_cast<const float2*>(
                    xb + (((Q * 3 + ((s - Q - 1) & 3)) * 3 + j) * 64 + el) * 2);
              }
              m[0][s >> 1][3 * (s & 1) + j] = v.x;
              m[1][s >> 1][3 * (s & 1) + j] = v.y;
            }
          }
#pragma unroll
          for (int e2 = 0; e2 < 2; ++e2) {
            at6(m[e2][0], P[e2][pt]);
            at6(m[e2][1], P[e2][3 + pt]);
          }
          if (!(DBG & 4) && (rp == 0 || pt < 2)) q_lds_barrier();  // the next pass rewrites ws1
        }
#pragma unroll
        for (int e2 = 0; e2 < 2; ++e2) {
          const int r = 2 * rp + e2;
          float bias = 0.f;
          {
            const int co = co0 + r;
            if (co < erec[wr].Cout) bias = BTAB ? btl[co * 9 + 4] : btl[co];
          }
#pragma unroll
          for (int x = 0; x < 4; ++x) P[e2][1][x] += bias;
          float Y[16];
#pragma unroll
          for (int x = 0; x < 4; ++x) {
            float c6[6], y[4];
#pragma unroll
            for (int I = 0; I < 6; ++I) c6[I] = P[e2][I][x];
            at6(c6, y);
#pragma unroll
            for (int yy = 0; yy < 4; ++yy) Y[yy * 4 + x] = y[yy];
          }
          q_finish<STATS, BTAB, RELU>(erec[wr], evoff[wr * 16 + etn], btl, co0 + r, cofs, Y, etn);
          cofs += erec[wr].hw4;
        }
      }
#pragma unroll
      for (int p = 0; p < 9; ++p)
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[p][cb] = floatx4{0.f, 0.f, 0.f, 0.f};
    };

    // one flat loop over the block's K steps, 4 per iteration (a co tile is a whole number
    // of iterations); the epilogue closes the iteration that ends a co tile (a loop over the
    // co tiles around a loop over their K steps makes the last step's accumulators two-use
    // values, and the compiler then renames every such MFMA's destination)
    int ks = 0, ct = ct0;
    for (int g = 0; g < G; g += 4) {
      step(ws0, ps1, ws1, ps0, ps2, ks, true);
      step(ws1, ps2, ws0, ps1, ps3, ks + 1, false);
      step(ws0, ps3, ws1, ps2, ps0, ks + 2, false);
      step(ws1, ps0, ws0, ps3, ps1, ks + 3, false);
      ks += 4;
      if (ks == K4) {
        epilogue(ct);
        post_epi = true;
        ks = 0;
        ++ct;
      }
    }
  };
  switch (wave & 3) {
    case 0: body(std::integral_constant<int, 0>{}); break;
    case 1: body(std::integral_constant<int, 1>{}); break;
    case 2: body(std::integral_constant<int, 2>{}); break;
    default: body(std::integral_constant<int, 3>{}); break;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the padding DMA has landed too
}

int wino4q_launch(ConvArgs& a, int in_op, hipStream_t st) {
  RPST_REQUIRE(in_op == RPST_IN_NONE || in_op == RPST_IN_UPSAMPLE2,
               "conv2d: winograd4 (quarter) does not support in_op %d", in_op);
  const ConvTiling t = wino4q_tiling(a);
  RPST_REQUIRE((int64_t)a.co_tiles * a.nchunks * kQWS * 4 < (1LL << 31),
               "conv2d: winograd4 weight image exceeds 2 GiB");
  RPST_REQUIRE(t.blocks <= 0x7fffffffLL, "conv2d: grid too large");
  const unsigned nb = (unsigned)t.blocks;
  const bool stats = a.stat_part != nullptr, btab = a.btab != nullptr;
  RPST_REQUIRE(!btab || in_op == RPST_IN_NONE, "conv2d: winograd4 bias table with a loader op");
  RPST_REQUIRE(!(stats && btab), "conv2d: winograd4 folded bias with statistics");
#define RPST_W4Q_GO(OP, S, B)                                                  \
  do {                                                                         \
    if (a.relu == RPST_ACT_RELU)                                               \
      wino4q_mfma_kernel<OP, S, B, true><<<nb, kQNTH, 0, st>>>(a);             \
    else                                                                       \
      wino4q_mfma_kernel<OP, S, B, false><<<nb, kQNTH, 0, st>>>(a);            \
  } while (0)
  if (in_op == RPST_IN_UPSAMPLE2) {
    if (stats) RPST_W4Q_GO(RPST_IN_UPSAMPLE2, true, false);
    else RPST_W4Q_GO(RPST_IN_UPSAMPLE2, false, false);
  } else {
    if (stats) RPST_W4Q_GO(RPST_IN_NONE, true, false);
    else if (btab) RPST_W4Q_GO(RPST_IN_NONE, false, true);
    else RPST_W4Q_GO(RPST_IN_NONE, false, false);
  }
#undef RPST_W4Q_GO
  return launch_status("wino4q_mfma_kernel");
}

}  // namespace rpst
