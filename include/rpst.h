/*
 * rpst.h — C ABI of the MI355X (gfx950) style-transfer forward path.
 *
 * Drop-in boundary: the reference (LuletterSoul/RP-Style-Transfer) has no FFI; its
 * boundary is the Python API of the `network` package (network/__init__.py:1-6).
 * Each entry point below replaces the ATen work behind one reference function, cited
 * as path:line relative to the reference root. The Python mirror in
 * rp-style-transfer_amd/network/ binds these symbols with ctypes.
 *
 * Conventions
 *  - All tensor pointers are DEVICE pointers to contiguous row-major (NCHW) data.
 *  - The library never allocates: ops that need scratch take (workspace, bytes) and
 *    expose a *_workspace_size() query; the caller allocates (e.g. torch caching
 *    allocator).
 *  - Every call is ordered on `stream` (a hipStream_t passed as void*; NULL = default
 *    stream) and never synchronises the device.
 *  - Return value: RPST_OK (0) or a negative RPST_E* code; rpst_last_error() returns a
 *    thread-local message describing the last failure.
 *  - fp32 in / fp32 out unless the name says f64. Results are deterministic (no float
 *    atomics; fixed-order reductions).
 */
#ifndef RPST_H_
#define RPST_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* rpst_stream_t;

#define RPST_OK 0
#define RPST_EINVAL (-1)  /* bad argument / unsupported shape            */
#define RPST_EHIP (-2)    /* HIP launch or runtime error                  */
#define RPST_EWORKSPACE (-3) /* workspace smaller than *_workspace_size() */

/* conv2d padding mode */
#define RPST_PAD_ZERO 0    /* nn.Conv2d(padding=1)            base.py:366-395            */
#define RPST_PAD_REFLECT 1 /* nn.ReflectionPad2d((1,1,1,1))   base.py:26-54, base.py:59-110 */
/* conv2d input operator applied on the fly while loading the input tile */
#define RPST_IN_NONE 0
#define RPST_IN_MAXPOOL2 1 /* nn.MaxPool2d((2,2),(2,2),(0,0),ceil_mode=True) base.py:65,72,85,98 */
#define RPST_IN_UPSAMPLE2 2 /* nn.Upsample(scale_factor=2, mode='nearest') base.py:29,42,49     */
#define RPST_IN_ADD_UPSAMPLE2 3 /* x + Upsample2(y)   sanet.py:149 (Transform merge input)   */
#define RPST_IN_ADAIN 4 /* ((x-mean_c)/std_c)*std_s+mean_s per (n,ci): AdaIN base.py:416-418 fused
                           into the consumer conv; aux = [mean_c|mean_s|std_c|std_s], N*Cin each */
#define RPST_IN_ADD_ADAIN 5 /* x + AdaIN(c): the skip fusion of MultiScaleAdaINRPNet.decode,
                           adain_rp.py:301 (rp_decoder[i+1](stylized + AdaIN(c_i, s_i)))  */

/* conv2d epilogue activation (the `relu` argument) */
#define RPST_ACT_NONE 0
#define RPST_ACT_RELU 1  /* nn.ReLU                                     */
#define RPST_ACT_LRELU 2 /* nn.LeakyReLU(0.2): Conv2dBlock base.py:147 */

/* Library version (major*10000 + minor*100 + patch). */
int rpst_version(void);
/* Message of the last failing call on this host thread ("" if none). */
const char* rpst_last_error(void);

/* ---- a1: calc_mean_std(feat, eps)  network/base.py:399-407 ----------------------
 * mean[n,c] = mean over HW; std[n,c] = sqrt(var_unbiased + eps) (eps on the variance).
 * feat (N,C,HW) -> mean, std (N,C). HW == 1 yields NaN std like torch.var. */
int rpst_calc_mean_std(const float* feat, float* mean, float* std_out, int N, int C,
                       int64_t HW, float eps, rpst_stream_t stream);

/* ---- a2: adaptive_instance_normalization(c, s)  network/base.py:410-418 ----------
 * out = (c - mean_c) / std_c * std_s + mean_s, statistics per (n,c) as in a1.
 * content/style/out (N,C,HW). Workspace: rpst_adain_workspace_size(N, C). */
size_t rpst_adain_workspace_size(int N, int C);
int rpst_adain(const float* content, const float* style, float* out, int N, int C,
               int64_t HW, float eps, void* workspace, size_t workspace_bytes,
               rpst_stream_t stream);

/* ---- a10: mean_variance_norm(feat)  network/sanet.py:20-24 -----------------------
 * out = (x - mean) / std with a1 statistics. Workspace: rpst_adain_workspace_size(N,C). */
int rpst_mean_variance_norm(const float* feat, float* out, int N, int C, int64_t HW,
                            float eps, void* workspace, size_t workspace_bytes,
                            rpst_stream_t stream);

/* ---- a2m: adaptive_instance_normalization_with_segment  network/base.py:421-530 ----
 * AdaIN per segmentation label (`use_mask: True`, inference only). Label maps are uint8
 * (N, HW), already resized to the feature size; each image uses its own pair of maps.
 *
 * rpst_segment_plan: per image, counts of every label in both maps and the validity rule of
 * compute_label_info (base.py:433-438): valid iff c > 10 and s > 10 and c/s < 100 and
 * s/c < 100. plan is int32 [N][256][4] = (content count, style count, valid flag, 0) per
 * label. It depends on the maps only, so one plan serves every feature level of that size.
 *
 * rpst_masked_adain_params: params is fp32 [N][C][256][4] = (mean_c, std_c, std_s, mean_s)
 * per (image, channel, label), statistics over that label's pixels as in a1 (fp64 sums,
 * std = sqrt(var_unbiased + eps)). Rows of invalid or absent labels are pass-through:
 * std_c = -1. content (N,C,HWc), style (N,C,HWs). params must be 16-byte aligned.
 * Workspace: rpst_masked_adain_workspace_size(N, C).
 *
 * rpst_masked_adain_apply: out = [skip +] ((x - mean_c) / std_c * std_s + mean_s) where the
 * pixel's row is not pass-through, out = [skip +] x elsewhere (bit-exact copy without skip).
 * skip_or_null: the running decoder feature of MultiScaleAdaINRPNet.decode (adain_rp.py:301)
 * or NULL. content / skip / out (N,C,HW), c_seg (N,HW). */
int rpst_segment_plan(const uint8_t* c_seg, const uint8_t* s_seg, int N, int64_t HWc,
                      int64_t HWs, int32_t* plan, rpst_stream_t stream);
size_t rpst_masked_adain_workspace_size(int N, int C);
int rpst_masked_adain_params(const float* content, const float* style, const uint8_t* c_seg,
                             const uint8_t* s_seg, const int32_t* plan, int N, int C,
                             int64_t HWc, int64_t HWs, float eps, float* params,
                             void* workspace, size_t workspace_bytes, rpst_stream_t stream);
int rpst_masked_adain_apply(const float* content, const float* skip_or_null,
                            const uint8_t* c_seg, const float* params, float* out, int N, int C,
                            int64_t HW, rpst_stream_t stream);

/* ---- a3/a5/a6/a12: Conv2d (3x3 or 1x1, stride 1) + bias [+ReLU] [+residual] -------
 * nn.Conv2d(k=3, padding=1) + ReLU         base.py:363-396 (RP encoder / decoder)
 * ReflectionPad2d(1) + Conv2d(k=3) [+ReLU] base.py:25-111, sanet.py:146-147,162-192
 * Conv2d(k=1)                              base.py:58, sanet.py:76-80
 * Weights are first repacked once into the kernel's K-major layout:
 *   rpst_conv2d_pack(weight (Cout,Cin,k,k), packed) with
 *   packed bytes = rpst_conv2d_packed_size(Cout, Cin, ksize).
 * in_op is applied to the input while it is loaded (pool / upsample / add), so
 *   RPST_IN_MAXPOOL2:     input (N,Cin,Hs,Ws), conv runs at H=ceil(Hs/2), W=ceil(Ws/2)
 *   RPST_IN_UPSAMPLE2:    input (N,Cin,Hs,Ws), conv runs at H=2Hs, W=2Ws
 *   RPST_IN_ADD_UPSAMPLE2: input (N,Cin,H,W) + aux (N,Cin,H/2,W/2) upsampled
 *   RPST_IN_ADAIN:        input (N,Cin,H,W) normalised on load with aux statistics
 *   RPST_IN_NONE:         input (N,Cin,H,W)
 * (Hs, Ws) are the dims of `input`. out (N,Cout,H,W):
 *   out = act(conv(in_op(input)) + bias) [+ residual]   (residual (N,Cout,H,W) or NULL),
 *   act = `relu`: RPST_ACT_NONE / RPST_ACT_RELU / RPST_ACT_LRELU
 * ksize 1 ignores pad_mode. Reflect padding needs H,W >= 2. */
size_t rpst_conv2d_packed_size(int Cout, int Cin, int ksize);
int rpst_conv2d_pack(const float* weight, float* packed, int Cout, int Cin, int ksize,
                     rpst_stream_t stream);
int rpst_conv2d(const float* input, const float* aux, const float* packed_weight,
                const float* bias, const float* residual, float* out, int N, int Cin,
                int Hs, int Ws, int Cout, int ksize, int pad_mode, int in_op, int relu,
                rpst_stream_t stream);

/* rpst_conv2d (in_op RPST_IN_NONE, no residual) over the batch [input; input2]: images
 * 0..n1-1 are input's, n1..N-1 are input2's (N - n1 images), read in place -- an encoder's
 * first conv over content and style without materialising torch.cat (adain_rp.py:94-95,
 * wct_rp.py:141-144, sanet.py:240-242 encode both in one pass). 0 < n1 <= N. */
int rpst_conv2d_pair(const float* input, const float* input2, int n1, const float* packed_weight,
                     const float* bias, float* out, int N, int Cin, int Hs, int Ws, int Cout,
                     int ksize, int pad_mode, int relu, rpst_stream_t stream);

/* Conv whose output only feeds a 2x2 max pool (VGG relu1_2 / relu2_2 / relu3_4 -> MaxPool2d
 * (2, 2, ceil_mode=True) -> next conv, network/base.py vgg, sanet.py:195-199 enc_2..enc_5):
 * out (N, Cout, (H+1)/2, (W+1)/2) = max_pool2d(act(conv(in_op(input)) + bias)), the pool
 * taken on the finished output tiles in the F(4x4) epilogue, so the full-resolution map is
 * never written. Bit-identical to rpst_conv2d followed by rpst_maxpool2x2_ceil. Only for
 * layers whose rpst_conv2d_algorithm is RPST_CONV_WINOGRAD4 (RPST_EINVAL otherwise: run
 * the two calls). */
int rpst_conv2d_pool(const float* input, const float* aux, const float* packed_weight,
                     const float* bias, float* out, int N, int Cin, int Hs, int Ws, int Cout,
                     int ksize, int pad_mode, int in_op, int relu, rpst_stream_t stream);

/* Conv (in_op NONE, no activation) whose output is zeroed where mask <= 0 (mask has the
 * output's shape): the input gradient of a conv whose input is a ReLU output y, dgrad and
 * threshold_backward(., y) in one pass (torch.autograd's ConvolutionBackward + ReluBackward
 * under total_loss.backward(), train.py:186-189). Bit-identical to rpst_conv2d followed by
 * rpst_relu_backward; the F(4x4) path thresholds in a second pass. */
int rpst_conv2d_masked(const float* input, const float* packed_weight, const float* bias,
                       const float* mask, float* out, int N, int Cin, int Hs, int Ws, int Cout,
                       int ksize, int pad_mode, rpst_stream_t stream);

/* Same conv with a caller-provided workspace (rpst_conv2d_workspace_size bytes, 0 when the
 * layer needs none). With RPST_IN_ADAIN on the F(4x4) path the workspace holds per-image
 * weights with the AdaIN scale std_s/std_c folded in along Cin and a per-(n, co) bias by
 * border class carrying mean_s - mean_c*std_s/std_c, so the conv streams the raw feature
 * (conv(pad0(s*x + b)) = conv_{W*s}(pad0(x)) + sum over in-image taps of W*b). Same result
 * as rpst_conv2d within fp32 rounding; rpst_conv2d applies the affine in its tile loader.
 * The size does not depend on the calling thread's rpst_conv2d_set_precise /
 * rpst_conv2d_set_quarter settings (it is the largest over all of them), so a workspace sized
 * under one setting serves a launch under any other. */
size_t rpst_conv2d_workspace_size(int N, int Cin, int Hs, int Ws, int Cout, int ksize,
                                  int in_op);
int rpst_conv2d_ws(const float* input, const float* aux, const float* packed_weight,
                   const float* bias, const float* residual, float* out, int N, int Cin,
                   int Hs, int Ws, int Cout, int ksize, int pad_mode, int in_op, int relu,
                   void* workspace, size_t workspace_bytes, rpst_stream_t stream);

/* Same conv, additionally returning calc_mean_std (base.py:399-407) of its OUTPUT per
 * (n, co): the statistics are reduced in the conv epilogue from registers and merged in
 * fp64, so an AdaIN consumer never re-reads the feature. mean/std_out: N*Cout floats.
 * Workspace: rpst_conv2d_stats_workspace_size(N, Cin, Hs, Ws, Cout, ksize, in_op), likewise
 * independent of the precise level and the quarter setting. */
size_t rpst_conv2d_stats_workspace_size(int N, int Cin, int Hs, int Ws, int Cout, int ksize,
                                        int in_op);
int rpst_conv2d_stats(const float* input, const float* aux, const float* packed_weight,
                      const float* bias, const float* residual, float* out, int N, int Cin,
                      int Hs, int Ws, int Cout, int ksize, int pad_mode, int in_op, int relu,
                      float* mean, float* std_out, float eps, void* workspace,
                      size_t workspace_bytes, rpst_stream_t stream);
/* Same, writing `out` for images n < store_n only (1 <= store_n <= N); the statistics cover
 * all N images. For a batch whose tail images are needed only through their statistics
 * (AdaINRPNet.test, adain_rp.py:94-101: the style half of the encoder output feeds
 * calc_mean_std alone). Images >= store_n of `out` are left unspecified. Same workspace. */
int rpst_conv2d_stats_store(const float* input, const float* aux, const float* packed_weight,
                            const float* bias, const float* residual, float* out, int N,
                            int Cin, int Hs, int Ws, int Cout, int ksize, int pad_mode,
                            int in_op, int relu, float* mean, float* std_out, float eps,
                            int store_n, void* workspace, size_t workspace_bytes,
                            rpst_stream_t stream);

/* SE channel attention of Conv2dBlock(attention='se') in eval mode (SEBottleneck,
 * network/attention.py:25-66, built at network/base.py:177-179). With every BatchNorm folded
 * into the conv before it (running statistics), the block is
 *   h1 = relu(conv1(x)), h2 = relu(conv2(h1)), u = conv3(h2),
 *   gate = sigmoid(fc_b relu(fc_a mean_HW(u))), out = relu(gate * u + x),
 * and runs as rpst_conv2d (1x1), rpst_conv2d_stats (3x3; its `mean` is mean_HW(h2)), then the
 * two calls below. u is never written: the pool of a 1x1 conv's output is the conv of the
 * pooled input.
 *
 * The gate (SELayer, attention.py:17-22): mean_h2 (N, C) = per-(n, c) mean of h2; w3 (C, C)
 * and b3 (C) = conv3 with bn3 folded, unpacked; fc_a (R, C), fc_b (C, R) = se.fc.0 / se.fc.2
 * weights, R >= 1. gate (N, C) = sigmoid(fc_b relu(fc_a (w3 mean_h2 + b3))), accumulated in
 * fp64 in a fixed order (no atomics): one launch, one workgroup per image. C <= 1024,
 * R <= 64. */
int rpst_se_gate(const float* mean_h2, const float* w3, const float* b3, const float* fc_a,
                 const float* fc_b, float* gate, int N, int C, int R, rpst_stream_t stream);

/* The conv that ends the block (attention.py:56-64): out = relu(gate[n, co] * (conv(input) +
 * bias[co]) + residual), gate (N, Cout), residual and out (N, Cout, H, W). The gate is loaded
 * once per output row beside the bias and the residual joins before the ReLU, in the direct
 * kernel's epilogue. mean / std_out (N*Cout floats each; both NULL: not computed) receive
 * calc_mean_std (base.py:399-407) of `out` as rpst_conv2d_stats returns it: from the
 * statistics epilogue for Cout <= 64, from a reduction of the written output above that.
 * Workspace: rpst_conv2d_gated_workspace_size bytes (may be 0; unused when mean is NULL).
 * ksize must be 1 (RPST_EINVAL otherwise: no other gated kernel is built). */
size_t rpst_conv2d_gated_workspace_size(int N, int Cin, int H, int W, int Cout, int ksize);
int rpst_conv2d_gated(const float* input, const float* packed_weight, const float* bias,
                      const float* gate, const float* residual, float* out, int N, int Cin,
                      int H, int W, int Cout, int ksize, float* mean, float* std_out, float eps,
                      void* workspace, size_t workspace_bytes, rpst_stream_t stream);

/* ---- f7: 7x7 conv, stride 1, padding 3 (LDMSAdaINRPNet's big-receptive-field branch) ----
 * Conv2dBlock(C, C, 7, 1, 3): ReflectionPad2d(3) + Conv2d(k=7) + LeakyReLU(0.2)
 *   adain_rp.py:513-514 (rp_enc{i}_big_revf), base.py:114-198
 * Weights are repacked once into the K-major image [ceil(Cin/8)][49 taps][8][Cout_pad]
 * (channel chunk CK = 8; Cout_pad = Cout rounded up to the kernel's output-channel tile: 32
 * for Cout <= 32, 64 for Cout <= 64, else 128), zero beyond Cin / Cout:
 *   packed bytes = rpst_conv7_packed_size(Cout, Cin) = 4 * ceil(Cin/8) * 49 * 8 * Cout_pad.
 * rpst_conv7: out[n, out_channel_offset + co, y, x] = act(bias[co] + sum w[co, ci, kh, kw] *
 *   pad3(x)[n, ci, y + kh - 3, x + kw - 3]); input (N,Cin,H,W); out is a tensor of
 *   out_channels_total channels per image of which only channels [out_channel_offset,
 *   out_channel_offset + Cout) are written (a branch lands in its half of a concatenated
 *   feature without a copy). pad_mode RPST_PAD_REFLECT = ReflectionPad2d(3), H, W >= 4;
 *   RPST_PAD_ZERO = zero padding 3, any size. act: RPST_ACT_*. bias may be NULL.
 *   input2 (may be NULL; otherwise N must be even): images n >= N/2 are read from it, image
 *   N/2 first, as rpst_conv2d_pair reads its second input. The padding is resolved in the tile loader; no
 *   padded copy is written. fp32 MFMA, exact products, k-ordered accumulation, no atomics:
 *   deterministic, and image k's bits do not depend on the batch. */
size_t rpst_conv7_packed_size(int Cout, int Cin);
int rpst_conv7_pack(const float* weight, float* packed, int Cout, int Cin,
                    rpst_stream_t stream);
int rpst_conv7(const float* input, const float* input2, const float* packed_weight,
               const float* bias, float* out, int N, int Cin, int H, int W, int Cout,
               int pad_mode, int act, int out_channel_offset, int out_channels_total,
               rpst_stream_t stream);

/* ---- bf16: opt-in reduced-precision 3x3 conv (stride 1, pad 1) on the bf16 MFMA ----
 * A second precision for inference, chosen per call: no thread switch, no environment
 * variable, and nothing above changes with it. Activations stay fp32 in memory (input and
 * output). The tile loader forms the fp32 input value (under RPST_IN_ADAIN the affine of
 * rpst_conv2d first) and rounds it once, to nearest even, to bf16; the weights are rounded the
 * same way once, by rpst_conv2d_bf16_pack. Products of two bf16 values are exact in fp32;
 * accumulation is fp32 in a fixed K order without atomics; bias, activation and statistics are
 * fp32 / fp64 as for rpst_conv2d_stats. Image n's output bits do not depend on the batch.
 * Runs: ksize 3, Cin a multiple of 16 in [16, 256], Cout >= 16, pad_mode RPST_PAD_ZERO /
 * RPST_PAD_REFLECT (H, W >= 2), in_op RPST_IN_NONE / RPST_IN_ADAIN, act RPST_ACT_*, any
 * H, W >= 1 with one image's input below 2 GiB. Everything else: RPST_EINVAL.
 *   rpst_conv2d_bf16_supports (host only): 1 for a layer rpst_conv2d_bf16 runs AND runs faster
 *     than rpst_conv2d's fp32 kernel (measured at 512^2: Cout >= 64; the rule and its numbers
 *     stand beside the function), else 0. The plans lower a conv to bf16 only where it says 1.
 *   packed: the bf16 image [Cin/16][9 taps][Cout_pad][16] of fp32 (Cout,Cin,3,3) weights,
 *     rpst_conv2d_bf16_packed_size bytes (0 for an unsupported layer); Cout_pad as rpst_conv7.
 *   input2 (may be NULL): images n >= n1 are read from it, as rpst_conv2d_pair (RPST_IN_NONE
 *     only; n1 is ignored without it). aux: the AdaIN parameters of rpst_conv2d, non-NULL
 *     exactly under RPST_IN_ADAIN. bias may be NULL.
 *   mean / std_out (both or neither; may be NULL): calc_mean_std of `out` from the epilogue
 *     as rpst_conv2d_stats returns it; then store_n in [1, N] and images n >= store_n are not
 *     written, only reduced (rpst_conv2d_stats_store), and the workspace holds
 *     rpst_conv2d_bf16_workspace_size bytes. Without statistics store_n is N (or 0) and the
 *     workspace is unused.
 *   rpst_conv2d_bf16_grid_threads: total threads of the launch, for profilers. */
int rpst_conv2d_bf16_supports(int Cout, int Cin, int ksize, int pad_mode, int in_op);
size_t rpst_conv2d_bf16_packed_size(int Cout, int Cin);
int rpst_conv2d_bf16_pack(const float* weight, void* packed, int Cout, int Cin,
                          rpst_stream_t stream);
size_t rpst_conv2d_bf16_workspace_size(int N, int Cin, int H, int W, int Cout);
int rpst_conv2d_bf16(const float* input, const float* input2, int n1, const float* aux,
                     const void* packed, const float* bias, float* out, int N, int Cin, int H,
                     int W, int Cout, int pad_mode, int in_op, int act, float* mean,
                     float* std_out, float eps, int store_n, void* workspace,
                     size_t workspace_bytes, rpst_stream_t stream);
int64_t rpst_conv2d_bf16_grid_threads(int N, int Cin, int H, int W, int Cout);

/* ---- LDMSAdaINRPNet4 (`network: ld_adain4`, adain_rp.py:711-819): coarse pyramid + concat ----
 * Nearest rule of F.interpolate(x, size) in its default mode, per axis:
 *   src = min((int)floorf(dst * ((float)in / (float)out)), in - 1), the product in fp32.
 * rpst_nearest_index_table (host only): index[dst] for dst in [0, out), by the statement of the
 *   rule the kernels share.
 * rpst_resize_nearest: src (N,C,h,w) -> channels [channel_offset, channel_offset + C) of dst
 *   (N,channels_total,H,W), h <= H, w <= W (the identity included); a pure gather, the other
 *   channels are left alone.
 * rpst_resized_mean_std: calc_mean_std (unbiased variance + eps, sqrt) of that resize without
 *   writing it: each source pixel weighted by the number of destination pixels that read it;
 *   mean / std_out (N,C). fp64 shifted sums in a fixed order: two calls give the same bits.
 *   H*W = 1 as rpst_calc_mean_std. Workspace: rpst_resized_mean_std_workspace_size(h, w).
 * rpst_ld4_fuse: a decoder block's input in one pass, out (N, Ca + 2*hidden, H, W):
 *   channels [0, Ca): y (N,Ca,H,W) copied (Ca = 0 with y NULL: the first block);
 *   [Ca, Ca + hidden): (v - mean_c) / std_c * std_s + mean_s of fine (N,hidden,H,W);
 *   [Ca + hidden, Ca + 2*hidden): the same of coarse (N,hidden,h,w) gathered by the rule.
 *   params_fine / params_coarse = [mean_c | mean_s | std_c | std_s], N*hidden floats each (as
 *   RPST_IN_ADAIN). fine / coarse may point at a [content; style] batch of 2N images: the
 *   first N are read. No atomics; plane bases need 4-byte alignment only. */
int rpst_nearest_index_table(int in, int out, int* index);
int rpst_resize_nearest(const float* src, float* dst, int N, int C, int h, int w, int H, int W,
                        int channel_offset, int channels_total, rpst_stream_t stream);
size_t rpst_resized_mean_std_workspace_size(int h, int w);
int rpst_resized_mean_std(const float* src, float* mean, float* std_out, int N, int C, int h,
                          int w, int H, int W, float eps, void* workspace,
                          size_t workspace_bytes, rpst_stream_t stream);
int rpst_ld4_fuse(const float* y, const float* fine, const float* coarse,
                  const float* params_fine, const float* params_coarse, float* out, int N,
                  int Ca, int hidden, int H, int W, int h, int w, rpst_stream_t stream);

/* MultiScaleAdaINRPNet skip fusion (adain_rp.py:301): out = act(conv(pad(x + AdaIN(c))) +
 * bias), x = `stylized` and c = `content` both (N,Cin,H,W), AdaIN with the calc_mean_std
 * statistics `params` = [mean_c | mean_s | std_c | std_s] (4*N*Cin floats, as
 * RPST_IN_ADAIN). The sum is formed while the conv stages its input tile. */
int rpst_conv2d_skip_adain(const float* stylized, const float* content, const float* params,
                           const float* packed_weight, const float* bias, float* out, int N,
                           int Cin, int H, int W, int Cout, int ksize, int pad_mode, int relu,
                           rpst_stream_t stream);

/* Launch geometry (total threads) rpst_conv2d would use for this shape under the calling
 * thread's settings — host-only, read from the same plan the launch reads; lets profilers
 * match rocprofv3 per-dispatch records (Grid_Size) to a layer. */
int64_t rpst_conv2d_grid_threads(int N, int Cin, int Hs, int Ws, int Cout, int ksize,
                                 int in_op);

/* Algorithm rpst_conv2d uses for this layer — host-only: RPST_CONV_NARROW (VALU kernel for
 * 3x3 layers with loader NONE and Cout <= 4, Cin <= 16 or Cout <= 16, Cin <= 4: the RP
 * stacks' 3->16 / 16->3 convs; batches above 65535 images and the statistics entry point
 * take the direct path instead), RPST_CONV_DIRECT (implicit GEMM: every 1x1 layer and the
 * other 3x3 layers with < 16 input channels), RPST_CONV_WINOGRAD4 (F(4x4,3x3) in fp32: 3x3
 * layers with >= 16 input channels whose loader operator is NONE / ADAIN / UPSAMPLE2) or
 * RPST_CONV_WINOGRAD (F(2x2,3x3) in fp32: the other 3x3 layers with >= 16 input and >= 32
 * output channels). The environment variable RPST_CONV_ALGO=direct|winograd|winograd4
 * overrides ("direct" keeps the narrow kernel for narrow shapes; RPST_CONV_NARROW=0 turns
 * it off). */
#define RPST_CONV_DIRECT 0
#define RPST_CONV_WINOGRAD 1
#define RPST_CONV_WINOGRAD4 2
#define RPST_CONV_NARROW 3
int rpst_conv2d_algorithm(int Cout, int Cin, int Hs, int Ws, int ksize, int in_op);

/* Precise mode for the CALLING THREAD (host-only): while on, the default choice never picks
 * F(4x4,3x3) (its fp32 rounding, ~1e-6 per conv, compounds through the ~30 convolutions of
 * a training step's backward chain); F(2x2) runs instead. Returns the previous setting.
 * on = 2: F(4x4) allowed, on its 32-channel form only (not the position-quarter kernel):
 * a training step's constant branches. The training autograd path (rpst/autograd.py)
 * sets it; an explicit RPST_CONV_ALGO still wins. */
int rpst_conv2d_set_precise(int on);

/* Position-quarter F(4x4) kernel (rpst_wino4q.hip) for the CALLING THREAD (host-only): mode
 * 0 off (every F(4x4) layer on the 32-channel kernel), 1 the default rule (Cin >= 128, Cin %
 * 16 == 0, 64 <= Cout <= 512, loader NONE / UPSAMPLE2 or the folded AdaIN), 2 forced on for
 * every shape it supports (Cin >= 16), -1 back to the RPST_W4Q environment variable (read
 * per launch; unset = 1). Same arithmetic as the 32-channel kernel within fp32 rounding.
 * Returns the previous setting. Workspace-size queries cover every setting.
 * rpst_conv2d_quarter reports whether a layer runs on it under the current settings. */
int rpst_conv2d_set_quarter(int mode);
int rpst_conv2d_quarter(int Cout, int Cin, int Hs, int Ws, int ksize, int in_op);

/* ---- stand-alone pool / upsample (same semantics as the conv input operators) ----- */
int rpst_maxpool2x2_ceil(const float* in, float* out, int N, int C, int H, int W,
                         rpst_stream_t stream);
int rpst_upsample_nearest2x(const float* in, float* out, int N, int C, int H, int W,
                            rpst_stream_t stream);
/* out (N,C,H,W) = a + upsample_nearest2x(b), b (N,C,H/2,W/2), H and W even: the merge
 * conv's input of Transform.forward (sanet.py:140-149) when that conv runs on F(4x4). */
int rpst_add_upsample_nearest2x(const float* a, const float* b, float* out, int N, int C, int H,
                                int W, rpst_stream_t stream);

/* ---- a11: SANet attention core  network/sanet.py:86-94 ------------------------------
 * O[b] = H[b] softmax_rows(F[b]^T G[b])^T  for F, G, H, O of shape (B, C, HW):
 *   S = F^T G (HW x HW, no 1/sqrt(C) scale), row softmax over keys, O = H S^T.
 * The 1x1 convs f/g/h/out_conv and mean_variance_norm run through rpst_conv2d /
 * rpst_mean_variance_norm. C in {64, 128, 256, 512} with HW % 4 == 0 runs flash-style (S
 * is never written: the keys stream through a double-buffered LDS ring with an online
 * softmax; no workspace); other shapes materialise S (B*HW*HW floats).
 * Workspace: rpst_sanet_attention_workspace_size_c(B, C, HW) (0 on the flash path);
 * rpst_sanet_attention_workspace_size(B, HW) is the materialised-S size (always enough). */
size_t rpst_sanet_attention_workspace_size(int B, int HW);
size_t rpst_sanet_attention_workspace_size_c(int B, int C, int HW);
int rpst_sanet_attention(const float* F, const float* G, const float* H, float* O, int B,
                         int C, int HW, void* workspace, size_t workspace_bytes,
                         rpst_stream_t stream);

/* The same with a style of another size (SANet.forward reads G's own size, sanet.py:86-94):
 * F and O are (B, C, HWq), G and H are (B, C, HWk); S = F^T G is HWq x HWk, the row softmax
 * runs over the HWk keys, O = H S^T. rpst_sanet_attention is the HWq = HWk call of this entry
 * (one body, the same bits).
 * Flash path: C in {64, 128, 256, 512} and HWk % 4 == 0 (16-byte key rows for the LDS DMA).
 * HWq needs no alignment (F and O are scalar accesses), so an odd HWq runs flash-style too.
 * Each operand's own (C, HW) plane must stay under 2^31 bytes for the flash path. Every other
 * shape materialises S: B*HWq*HWk floats plus 2*B*HWq of row statistics.
 * Workspace: rpst_sanet_attention_qk_workspace_size_c(B, C, HWq, HWk) (0 on the flash path).
 * RPST_EINVAL for a count < 1, RPST_EWORKSPACE for a short workspace, before any launch. */
size_t rpst_sanet_attention_qk_workspace_size_c(int B, int C, int HWq, int HWk);
int rpst_sanet_attention_qk(const float* F, const float* G, const float* H, float* O, int B,
                            int C, int HWq, int HWk, void* workspace, size_t workspace_bytes,
                            rpst_stream_t stream);

/* ---- f3: AdaptiveSANet  network/sanet.py:12-18, 26-71, 100-138 ----
 * cal_affinity_matrix(c, s) (sanet.py:12-18): out[b] = normalize(c[b])^T normalize(s[b]),
 * normalize = x / max(||x||_2 over channels, 1e-12). c, s (B, C, HW) -> out (B, HW, HW).
 * Workspace: rpst_cosine_affinity_workspace_size(B, C, HW). */
size_t rpst_cosine_affinity_workspace_size(int B, int C, int HW);
int rpst_cosine_affinity(const float* content, const float* style, float* out, int B, int C,
                         int HW, void* workspace, size_t workspace_bytes, rpst_stream_t stream);

/* AEAModule.forward (mode 0, sanet.py:42-47) / AEALReluModule.forward (mode 1, :63-69):
 * clamp[b,i] = head(w2 . LeakyReLU_0.2(W1 x[b,i,:] + b1) + b2), head = sigmoid(t)*interval
 * + from (mode 0) or (tanh(t)+1)/2 (mode 1); out_fx = sigmoid(scale (fx - clamp)) (mode 0)
 * or softmax_rows(relu(fx - clamp)) (mode 1). x, fx, out_fx (B, HW, HW); W1 (hidden, HW),
 * b1 (hidden), w2 (hidden), b2 (1) device pointers; out_clamp (B, HW).
 * Workspace: rpst_aea_clamp_workspace_size(B, HW, hidden). */
size_t rpst_aea_clamp_workspace_size(int B, int HW, int hidden);
int rpst_aea_clamp(const float* x, const float* fx, const float* w1, const float* b1,
                   const float* w2, const float* b2, int hidden, int mode, float scale,
                   float from, float interval, float* out_fx, float* out_clamp, int B, int HW,
                   void* workspace, size_t workspace_bytes, rpst_stream_t stream);

/* AdaptiveSANet attention core (sanet.py:106-124): with S = F^T G and P = softmax_rows(S),
 * O[b] = H[b] Q^T with Q = AEA(cal_affinity_matrix(content, style), P) as rpst_aea_clamp
 * (mode/scale/from/interval). For C in {64, 128, 256, 512} and HW % 4 == 0 S is never
 * stored: a flash pass forms each query's softmax statistics, a second recomputes S per key
 * block and applies P and Q in registers (no B x HW x HW workspace); other shapes form S in
 * the workspace and apply P and Q while staging it into the second GEMM. claim_before /
 * claim_after (B, HW, HW) are written only when non-null; claim_value (B, HW) receives the
 * clamp values when non-null.
 * Workspace: rpst_adaptive_attention_workspace_size(B, C, HW, hidden). */
size_t rpst_adaptive_attention_workspace_size(int B, int C, int HW, int hidden);
int rpst_adaptive_attention(const float* F, const float* G, const float* H,
                            const float* content, const float* style, const float* w1,
                            const float* b1, const float* w2, const float* b2, int hidden,
                            int mode, float scale, float from, float interval, float* O,
                            float* claim_value, float* claim_before, float* claim_after, int B,
                            int C, int HW, void* workspace, size_t workspace_bytes,
                            rpst_stream_t stream);

/* ---- f4: host I/O pixel conversions  test.py:49-54, 139-149 ------
 * transforms.ToTensor: in (N, H, W, 3) uint8 -> out (N, 3, H, W) fp32 = u8 / 255. */
int rpst_u8hwc_to_f32nchw(const uint8_t* in, float* out, int N, int H, int W,
                          rpst_stream_t stream);
/* torchvision.utils.save_image's pixel path: in (N, 3, H, W) fp32 -> uint8 of
 * clamp(x * 255 + 0.5, 0, 255) written as the tile at (y0, x0) of each of N canvases
 * (canvas_h, canvas_w, 3) HWC. make_grid's padding is the caller's memset of the canvas. */
int rpst_f32nchw_to_u8_tile(const float* in, uint8_t* canvas, int N, int H, int W,
                            int canvas_h, int canvas_w, int y0, int x0, rpst_stream_t stream);

/* PNG "Up" filter of N 8-bit images of H rows x rowbytes bytes (e.g. rpst_f32nchw_to_u8_tile's
 * canvases, rowbytes = 3 W): out (N, H, rowbytes + 1) = per row the filter-type byte 2 then
 * (row y - row y-1) mod 256 (row -1 = 0), i.e. the PNG IDAT scanlines before zlib, so the host
 * side of save_image (test.py:139-149) is only the deflate (rpst.imageio.write_png). */
int rpst_png_filter_up(const uint8_t* in, uint8_t* out, int N, int H, int rowbytes,
                       rpst_stream_t stream);

/* ---- f2: training backward  AdaINRPNet.forward adain_rp.py:110-138 +
 * total_loss.backward() train.py:186-189. Conv dgrad runs on rpst_conv2d with weights from
 * rpst_conv_weight_flip (packed by rpst_conv2d_pack); reflect-padded convs then add
 * rpst_reflect_pad_border_grad.
 * w (Cout, Cin, k, k) -> wt (Cin, Cout, k, k), wt[ci][co][a][b] = w[co][ci][k-1-a][k-1-b]. */
int rpst_conv_weight_flip(const float* w, float* wt, int Cout, int Cin, int ksize,
                          rpst_stream_t stream);
/* ReLU backward: out = y > 0 ? g : 0 (y = the ReLU output), n elements. */
int rpst_relu_backward(const float* g, const float* y, float* out, int64_t n,
                       rpst_stream_t stream);
/* LeakyReLU(slope) backward (Conv2dBlock's activation, base.py:147; slope > 0):
 * out = y > 0 ? g : slope * g (y = the activation output, same sign as its input). */
int rpst_leaky_relu_backward(const float* g, const float* y, float* out, int64_t n, float slope,
                             rpst_stream_t stream);
/* MaxPool2d(2, 2, ceil_mode=True) backward: x (N,C,H,W) the pool input, g the gradient at
 * its output -> dx (N,C,H,W) (argmax as ATen: first max in window order, NaN wins);
 * relu_mask = 1 also applies ReLU backward with y = x (x is a ReLU output). */
int rpst_maxpool2x2_ceil_backward(const float* x, const float* g, float* dx, int N, int C,
                                  int H, int W, int relu_mask, rpst_stream_t stream);
/* ReflectionPad2d(1) + conv3x3 backward, border part: dy (N,Cout,H,W), w (Cout,Cin,3,3);
 * dx (N,Cin,H,W) holds the zero-padded dgrad and receives the padded border's gradient
 * folded onto the rows / columns it reflects. H, W >= 2.
 * Workspace: rpst_reflect_pad_border_grad_workspace_size(N, Cin, H, W). */
size_t rpst_reflect_pad_border_grad_workspace_size(int N, int Cin, int H, int W);
int rpst_reflect_pad_border_grad(const float* dy, const float* w, float* dx, int N, int Cin,
                                 int Cout, int H, int W, void* workspace, size_t workspace_bytes,
                                 rpst_stream_t stream);
/* The same, for a conv whose input is a ReLU output y (mask = y, N x Cin x H x W): the border
 * gradient is added only where y > 0, so with dx from rpst_conv2d_masked the result equals
 * rpst_relu_backward(dgrad + border, y) bit for bit (threshold_backward fused, train.py:186-189
 * backward through the decoders' Conv2d -> ReLU chains). mask may be NULL. */
int rpst_reflect_pad_border_grad_masked(const float* dy, const float* w, const float* mask,
                                        float* dx, int N, int Cin, int Cout, int H, int W,
                                        void* workspace, size_t workspace_bytes,
                                        rpst_stream_t stream);
/* conv3x3 (stride 1, zero pad 1) weight / bias gradient: x (N,Cin,H,W) the conv input, dy
 * (N,Cout,H,W) the gradient at its output -> dw (Cout,Cin,3,3), db (Cout) (db may be NULL).
 * Workspace: rpst_conv_wgrad_workspace_size(N, Cin, H, W, Cout). */
size_t rpst_conv_wgrad_workspace_size(int N, int Cin, int H, int W, int Cout);
int rpst_conv_wgrad(const float* x, const float* dy, float* dw, float* db, int N, int Cin,
                    int H, int W, int Cout, void* workspace, size_t workspace_bytes,
                    rpst_stream_t stream);
/* the same with the conv's padding: RPST_PAD_ZERO, or RPST_PAD_REFLECT (ReflectionPad2d(1) +
 * conv3x3 pad 0, the decoders of sanet.py:162-192 / base.py Conv2dBlock 'reflect'; H, W >= 2),
 * read in the loader (no padded copy). Same workspace. */
int rpst_conv_wgrad_pad(const float* x, const float* dy, float* dw, float* db, int N, int Cin,
                        int H, int W, int Cout, int pad, void* workspace,
                        size_t workspace_bytes, rpst_stream_t stream);
/* conv7x7 (stride 1, pad 3: rpst_conv7) weight / bias gradient, LDMSAdaINRPNet's big branch
 * (adain_rp.py:513-514) in training: x (N,Cin,H,W) the conv input, dy (N,Cout,H,W) the gradient
 * at its (pre-activation) output -> dw[co][ci][kh][kw] = sum over (n,y,x) of dy[n][co][y][x] *
 * pad3(x)[n][ci][y+kh-3][x+kw-3] (Cout,Cin,7,7), db[co] = sum dy (db may be NULL). pad_mode
 * RPST_PAD_REFLECT (ReflectionPad2d(3); H, W >= 4) or RPST_PAD_ZERO (any size), resolved in the
 * loader (no padded copy). fp32 MFMA, exact products, split over pixels with the partials
 * summed in a fixed order, no atomics: two calls give the same bits. Any Cin, Cout >= 1.
 * Workspace: rpst_conv7_wgrad_workspace_size(N, Cin, H, W, Cout).
 * The data gradient is rpst_conv7 with zero padding on the weights of rpst_conv_weight_flip
 * (ksize 7) packed by rpst_conv7_pack; for a reflect-padded conv it runs on dy embedded in zeros
 * over the padded domain (H+6) x (W+6) and rpst_reflect_pad_backward folds the result. */
size_t rpst_conv7_wgrad_workspace_size(int N, int Cin, int H, int W, int Cout);
int rpst_conv7_wgrad(const float* x, const float* dy, float* dw, float* db, int N, int Cin,
                     int H, int W, int Cout, int pad_mode, void* workspace,
                     size_t workspace_bytes, rpst_stream_t stream);
/* ReflectionPad2d(pad) backward: gp (planes, H + 2 pad, W + 2 pad) the gradient of the padded
 * tensor -> dx (planes, H, W), every padded position summed into the pixel it reflects, in a
 * fixed order (pad < H, W; with H or W <= 2 pad both mirrors reach the same pixels). */
int rpst_reflect_pad_backward(const float* gp, float* dx, int64_t planes, int H, int W, int pad,
                              rpst_stream_t stream);
/* adaptive_instance_normalization backward (base.py:410-418): g the gradient at the AdaIN
 * output, c / s the content / style features (planes x HW), stats = [mean_c | std_c |
 * mean_s | std_s] (planes each) -> dc, ds. Workspace: 2*planes floats. */
int rpst_adain_backward(const float* g, const float* c, const float* s, const float* stats,
                        float* dc, float* ds, int planes, int64_t HW, void* workspace,
                        size_t workspace_bytes, rpst_stream_t stream);
/* Gradient of weights[0] * calc_style_loss(F, target) (+ weights[1] * mse(F, Fc) when Fc is
 * non-NULL) w.r.t. F (planes x HW), adain_rp.py:84-88 / 131-136 with MSELoss (mean);
 * stats = [mean | std | mean_t | std_t] (planes each); weights is a DEVICE pointer;
 * accumulate = 1 adds into out. */
int rpst_style_content_loss_grad(const float* F, const float* Fc, const float* stats,
                                 const float* weights, float* out, int planes, int64_t HW,
                                 int accumulate, rpst_stream_t stream);
/* ---- SAModel training (network/sanet.py:248-275): the extra backward pieces --------
 * 1-pixel pad of `planes` H x W planes to (H+2) x (W+2): reflect = 1 ReflectionPad2d(1)
 * (H, W >= 2), 0 zeros. A reflect-padded conv's weight gradient is rpst_conv_wgrad of the
 * padded input against the zero-padded output gradient. */
int rpst_pad1(const float* x, float* out, int64_t planes, int H, int W, int reflect,
              rpst_stream_t stream);
/* nn.Upsample(scale_factor=2, mode='nearest') backward: g (planes, 2H, 2W) -> dx (planes,
 * H, W), each dx the sum of its 2x2 block of g (sanet.py:145,166,179,186). */
int rpst_upsample_nearest2x_backward(const float* g, float* dx, int64_t planes, int H, int W,
                                     rpst_stream_t stream);
/* mean_variance_norm backward (sanet.py:20-24): y the normalised output, dy its gradient,
 * std (planes) = sqrt(var_unbiased + eps) -> dx = (dy - mean(dy) - y sum(dy y)/(HW-1))/std
 * (accumulate = 1 adds into dx). */
int rpst_mean_variance_norm_backward(const float* y, const float* dy, const float* std,
                                     float* dx, int64_t planes, int64_t HW, int accumulate,
                                     rpst_stream_t stream);
/* Row softmax (sanet.py:92-93, dim=-1) and its backward dS = P (dP - rowsum(dP P)), for
 * `rows` rows of `cols` contiguous floats (dS may alias dP). */
int rpst_softmax_rows(const float* S, float* P, int64_t rows, int cols, rpst_stream_t stream);
int rpst_softmax_rows_backward(const float* P, const float* dP, float* dS, int64_t rows,
                               int cols, rpst_stream_t stream);
/* SANet attention backward (sanet.py:86-94 under autograd; the rocBLAS batched GEMMs of
 * round 2 replaced): for F (B,C,HWc), G, H (B,C,HWs) and dO (B,C,HWc), with S = F^T G and
 * P = softmax_rows(S): dH = dO P, dP = dO^T H, dS = P (dP - rowsum(dP P)), dF = G dS^T,
 * dG = F dS. P is formed from S while staged, never stored. Workspace:
 * rpst_sanet_attention_backward_workspace_size(B, HWc, HWs) (S and dP). */
size_t rpst_sanet_attention_backward_workspace_size(int B, int HWc, int HWs);
int rpst_sanet_attention_backward(const float* F, const float* G, const float* H,
                                  const float* dO, float* dF, float* dG, float* dH, int B, int C,
                                  int HWc, int HWs, void* workspace, size_t workspace_bytes,
                                  rpst_stream_t stream);
/* The same gradients without the B x HWc x HWs terms (the training path): S and dP exist for
 * 2048 queries (whole rows) at a time; dF is written per query chunk, dH and dG are summed
 * over the chunks in order. S, its row statistics and dS are the single pass's bit for bit.
 * Workspace: rpst_sanet_attention_backward_chunked_workspace_size(B, C, HWc, HWs) =
 * 4 (2 B q HWs + 2 B q) bytes, q = min(HWc, 2048). */
size_t rpst_sanet_attention_backward_chunked_workspace_size(int B, int C, int HWc, int HWs);
int rpst_sanet_attention_backward_chunked(const float* F, const float* G, const float* H,
                                          const float* dO, float* dF, float* dG, float* dH,
                                          int B, int C, int HWc, int HWs, void* workspace,
                                          size_t workspace_bytes, rpst_stream_t stream);
/* AdaptiveSANet attention backward (sanet.py:100-138 under autograd; AdaptiveSAModel trains
 * through it, train.py:118-119): with A the cosine affinity of content / style, c the f_psi
 * clamp, S = F^T G, P = softmax_rows(S) and Q = AEA(P) (mode 0 aea: sigmoid(scale (P - c)),
 * mode 1 relu: softmax_rows(relu(P - c))), O = H Q^T: from dO (B,C,HW) -> dF, dG, dH (B,C,HW)
 * and the f_psi gradients dw1 (hidden,HW), db1 (hidden), dw2 (hidden), db2 (1). Q and P are
 * formed from S where staged, never stored; S and dQ exist for 2048 queries (whole rows) at
 * a time (no B x HW x HW term; dH, dG summed over the query chunks in order). Workspace:
 * rpst_adaptive_attention_backward_workspace_size(B, C, HW, hidden). */
size_t rpst_adaptive_attention_backward_workspace_size(int B, int C, int HW, int hidden);
int rpst_adaptive_attention_backward(const float* F, const float* G, const float* H,
                                     const float* content, const float* style, const float* w1,
                                     const float* b1, const float* w2, const float* b2,
                                     int hidden, int mode, float scale, float from,
                                     float interval, const float* dO, float* dF, float* dG,
                                     float* dH, float* dw1, float* db1, float* dw2, float* db2,
                                     int B, int C, int HW, void* workspace,
                                     size_t workspace_bytes, rpst_stream_t stream);
/* 1x1 conv weight / bias gradient over a batch (sanet.py:76-80, 97 f / g / h / out_conv):
 * dw (Cout,Cin) = sum_n dy_n x_n^T, db (Cout, may be NULL) = sum over n and pixels of dy.
 * Per-image products then a fixed-order batch sum. Workspace:
 * rpst_conv1x1_wgrad_workspace_size(N, Cin, Cout). */
size_t rpst_conv1x1_wgrad_workspace_size(int N, int Cin, int Cout);
int rpst_conv1x1_wgrad(const float* x, const float* dy, float* dw, float* db, int N, int Cin,
                       int64_t HW, int Cout, void* workspace, size_t workspace_bytes,
                       rpst_stream_t stream);
/* *out = scale * sum (a - b)^2 over n elements (fp64 accumulation, fixed order).
 * Workspace: rpst_sq_diff_workspace_size(). */
size_t rpst_sq_diff_workspace_size(void);
int rpst_sq_diff_sum(const float* a, const float* b, int64_t n, double scale, float* out,
                     void* workspace, size_t workspace_bytes, rpst_stream_t stream);

/* ---- a7: matrix_sqrt / matrix_inv_sqrt  network/wct_rp.py:7-40 ----------------------
 * out[b] = (A[b] + 1e-4 I)^(+1/2) (inverse = 0) or ^(-1/2) (inverse = 1), fp64 n x n,
 * batch of `batch`: the reference's SVD form V diag(s^p) V^T with singular values < 1e-5
 * dropped, for any input. One persistent launch runs coupled Newton-Schulz per matrix
 * (stop at the product's rounding floor, max(1e-10, 8 eps n ||Y||_F ||Z||_F), or on
 * stagnation; at most 64 steps) -- equal to the SVD form on symmetric inputs whose smallest
 * eigenvalue is provably >= 1e-5; a matrix that is not symmetric, may be truncated or did
 * not converge is recomputed by a one-sided Jacobi SVD (n <= 1024). residual (batch doubles,
 * may be NULL) receives each matrix's last Newton-Schulz residual (informational). Fully
 * asynchronous on `stream` (no host synchronisation).
 * Workspace: rpst_matrix_power_workspace_size(n, batch). */
size_t rpst_matrix_power_workspace_size(int n, int batch);
int rpst_matrix_power_psd_f64(const double* A, double* out, int n, int batch, int inverse,
                              double* residual, void* workspace, size_t workspace_bytes,
                              rpst_stream_t stream);

/* ---- a8: WCTRPNet.whiten_and_color(cF, sF, 'closed-form')  network/wct_rp.py:82-114 ---
 * cF, sF, out: (C, HW) fp64. out = T (cF - mu_c) + mu_s with the closed-form T.
 * residual (2 doubles or NULL): Newton-Schulz residuals of Cc + 1e-4 I and of Mid's argument
 * (informational; a non-finite input gives NaN in out).
 * Workspace: rpst_wct_workspace_size(1, C, HW). */
size_t rpst_wct_workspace_size(int n, int C, int64_t HW);
int rpst_whiten_and_color_f64(const double* cF, const double* sF, double* out, int C,
                              int64_t HW, double* residual, void* workspace,
                              size_t workspace_bytes, rpst_stream_t stream);

/* whiten_and_color(cF, sF, 'original') (Li et al., wct_rp.py:96-101): out =
 * matrix_sqrt(Cs) matrix_inv_sqrt(Cc + I) (cF - mu_c) + mu_s, both matrix functions in the
 * reference's SVD form (as rpst_matrix_power_psd_f64, including the 1e-5 truncation), with
 * Cc, Cs the covariances of wct_rp.py:89-94 (the content one + I). Same shapes and workspace
 * as rpst_whiten_and_color_f64. */
int rpst_whiten_and_color_original_f64(const double* cF, const double* sF, double* out, int C,
                                       int64_t HW, void* workspace, size_t workspace_bytes,
                                       rpst_stream_t stream);

/* ---- a9: WCTRPNet.fuse(content_feats, style_feats)  network/wct_rp.py:157-166 --------
 * content, style, out: (n, C, HW) fp32. Per image: widen to fp64, whiten_and_color, round
 * to fp32 — all n images in one set of launches. residual: 2n doubles or NULL (as a8, per
 * image). Workspace: rpst_wct_workspace_size(n, C, HW). */
int rpst_wct_fuse(const float* content, const float* style, float* out, int n, int C,
                  int64_t HW, double* residual, void* workspace, size_t workspace_bytes,
                  rpst_stream_t stream);

/* ---- a9 split for the fused WCTRPNet.test: the closed-form matrices without the product
 * T: (n, C, C) fp64 and offset c = mu_s - T mu_c: (n, C) fp64, so that the fused feature
 * T (cF - mu_c) + mu_s = T cF + c (wct_rp.py:109-113) is formed inside the decoder's first
 * conv (rpst_conv2d_mix) instead of being written. means: optional fp32 row means (2n x C,
 * content rows then style rows, e.g. the encoder's statistics epilogue); NULL computes them.
 * Workspace: rpst_wct_workspace_size(n, C, HW). */
int rpst_wct_params(const float* content, const float* style, const float* means, double* T,
                    double* offset, int n, int C, int64_t HW, double* residual, void* workspace,
                    size_t workspace_bytes, rpst_stream_t stream);

/* Per-image status of the last rpst_wct_fuse / rpst_wct_params call on `workspace` (same n,
 * C, HW), copied asynchronously on `stream` into status (n ints, device memory): 0 = valid,
 * otherwise a bit mask of RPST_WCT_NOCONV (a Newton-Schulz iteration did not converge:
 * non-finite features) and RPST_WCT_TIMEOUT (a group barrier of the persistent matrix-function
 * launch timed out, e.g. its workgroups were not all resident beside other work). Any non-zero
 * status comes with NaN in that image's T / offset / output — never a silently wrong finite
 * value. Read it at the caller's next natural synchronisation.
 * rpst_whiten_and_color_status: the same for the last rpst_whiten_and_color_f64 call. */
#define RPST_WCT_NOCONV 1
#define RPST_WCT_TIMEOUT 4
int rpst_wct_status(const void* workspace, int n, int C, int64_t HW, int* status,
                    rpst_stream_t stream);
int rpst_whiten_and_color_status(const void* workspace, int C, int64_t HW, int* status,
                                 rpst_stream_t stream);

/* ---- a9 with a style of another size (fuse flattens cf and sf independently, wct_rp.py:
 * 157-166; whiten_and_color divides each covariance by its own pixel count - 1, :89-94).
 * content and out: (n, C, HWc) fp32; style: (n, C, HWs) fp32. Per image:
 *   mu_c, Cc = (cF - mu_c)(cF - mu_c)^T / (HWc - 1) + I   over the content's HWc pixels
 *   mu_s, Cs = (sF - mu_s)(sF - mu_s)^T / (HWs - 1)       over the style's HWs pixels
 *   T, the offset c = mu_s - T mu_c and out = T (cF - mu_c) + mu_s over the HWc pixels.
 * The covariance's split-K is a function of each side's own pixel count, so an image's bits
 * do not depend on its batch. means, T, offset, residual and status are as in the one-count
 * entries (means: 2n x C, content rows first). rpst_wct_workspace_size, rpst_wct_fuse,
 * rpst_wct_params and rpst_wct_status are the HWc = HWs calls of these (one body, the same
 * bits). The fp64 entries (rpst_whiten_and_color_f64 / _original_f64) stay one-count.
 * Workspace: rpst_wct_workspace_size_cs(n, C, HWc, HWs). RPST_EINVAL for a count < 2,
 * RPST_EWORKSPACE for a short workspace, before any launch. */
size_t rpst_wct_workspace_size_cs(int n, int C, int64_t HWc, int64_t HWs);
int rpst_wct_fuse_cs(const float* content, const float* style, float* out, int n, int C,
                     int64_t HWc, int64_t HWs, double* residual, void* workspace,
                     size_t workspace_bytes, rpst_stream_t stream);
int rpst_wct_params_cs(const float* content, const float* style, const float* means, double* T,
                       double* offset, int n, int C, int64_t HWc, int64_t HWs, double* residual,
                       void* workspace, size_t workspace_bytes, rpst_stream_t stream);
int rpst_wct_status_cs(const void* workspace, int n, int C, int64_t HWc, int64_t HWs,
                       int* status, rpst_stream_t stream);

/* Measurement (bench.py): while armed (rpst_wct_phase_timing(1); returns the previous
 * setting), rpst_wct_params / rpst_wct_fuse record HIP events around their covariance phase
 * (means + SYRK + reduce) and their matrix-function launch; rpst_wct_phase_ms waits for the
 * last armed call and returns the two durations in milliseconds. */
int rpst_wct_phase_timing(int on);
int rpst_wct_phase_ms(float* cov_ms, float* matfun_ms);

/* out = act(conv(pad(T_n x + c_n)) + bias) per image n: the WCT colour transform fused into
 * the consumer conv. F(4x4) layers fold T_n into per-image weights W T_n (fp64, rounded
 * once) and c_n into per-(n, co) border-class biases; other layers materialise T x + c.
 * x: (N, Cin, H, W) fp32; T: (N, Cin, Cin) fp64; offset: (N, Cin) fp64.
 * Workspace: rpst_conv2d_mix_workspace_size(N, Cin, H, W, Cout, ksize). It does not depend on
 * the quarter setting but does on the precise level: at rpst_conv2d_set_precise(1) the layer
 * leaves F(4x4) and the workspace holds T x + c (N*Cin*H*W floats), which every inference
 * workspace would otherwise carry. Query it at the level the launch runs under. ksize is 1
 * or 3: another one sizes as 0 bytes and is refused (RPST_EINVAL) before any launch. */
size_t rpst_conv2d_mix_workspace_size(int N, int Cin, int H, int W, int Cout, int ksize);
int rpst_conv2d_mix(const float* input, const double* T, const double* offset,
                    const float* packed_weight, const float* bias, float* out, int N, int Cin,
                    int H, int W, int Cout, int ksize, int pad_mode, int relu, void* workspace,
                    size_t workspace_bytes, rpst_stream_t stream);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RPST_H_ */
