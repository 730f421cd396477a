/* hydranet_hip.h -- C ABI of libhydranet_hip.so, the MI355X (gfx950) kernels behind the HydraNet forward/backward hot path.
 *
 * Drop-in boundary.  The reference (FlowEternal/multitask-hydranet) has no FFI of its own: its hot path is the ATen op layer
 * underneath model/model.py:159-264 and the one torch.autograd.Function it authors (SwishImplementation, model/net/common.py:11-22).
 * Each entry point below replaces the ATen/cuDNN call(s) named in its comment (paths relative to /root/reference/model).
 *
 * Conventions
 *   - Activations are NHWC ("channels last") bf16: a tensor is [rows = N*H*W][C] with an explicit row stride `ld*` in ELEMENTS so
 *     producers can write channel slices of a concatenation buffer.  C and every ld must be a multiple of 8 (16-byte pieces).
 *   - Parameters and statistics are fp32.  Packed weight operands are bf16 (see hn_pack_weight / hn_gconv_pack / hn_dw_pack).
 *   - Every buffer is owned by the caller (PyTorch's caching allocator) and only borrowed for the call; the library keeps no state.
 *   - Every function only enqueues kernels on `stream` (no allocation, no synchronisation => hipGraph-capturable) and returns
 *     0 on success, 1 = bad argument, 2 = launch failure, 3 = unsupported shape.  No C++ exceptions cross the boundary.
 *   - Activation codes: 0 none, 1 ReLU, 2 Swish, 3 ELU, 4 sigmoid.
 */
#ifndef HYDRANET_HIP_H
#define HYDRANET_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t;

/* ---- dense contractions on MFMA (hn_gemm.hip) ------------------------------------------------------------------------------- */

/* fp32 conv weight [Cout][Cin][taps] -> bf16 forward operand wp[Cout][taps][KP(Cin)] and (optional) dgrad operand
 * wt[Cin][taps][KP(Cout)], KP(x) = x rounded up to 32, zero filled.  Replaces the implicit weight cast of autocast convs. */
int hn_gconv_pack_diag(const float* w, void* wk, void* wd, int C, hipStream_t stream);
int hn_pack_weight(const float* w, void* wp, void* wt, int Cout, int Cin, int taps, hipStream_t stream);
/* hn_pack_weight for a channel slice [ci0, ci0+Cin) of w [Cout][Cin_total][taps] (phase = 0), or (phase = 1, taps = 9) the PHASE-FORM
 * effective weights of that slice: a 3x3 conv over a nearest-x2 up-sampled map (head_seg/segmentation.py:92-104: Upsample -> ReflectionPad2d
 * -> Conv2d) evaluated on the low-resolution grid has 4*Cout outputs (one Cout-vector per output phase), each tap of which is the sum of
 * the original taps that land on it: wp [4*Cout][9][KP(Cin)], wt [Cin][9][KP(4*Cout)], b_eff [4*Cout] (optional) = bias per phase. */
int hn_pack_weight_ex(const float* w, void* wp, void* wt, int Cout, int Cin_total, int ci0, int Cin, int taps, int phase, const float* bias,
                      float* b_eff, hipStream_t stream);
/* the transpose: dw [K][C0+C1][3][3] (db [K], optional) from the effective-weight gradient dw_eff [4K][C0][3][3] (db_eff [4K]); channels
 * [C0, C0+C1) are copied from the skip operand's own gradient dw1 [K][C1][3][3] */
int hn_phase_fold(const float* dw_eff, const float* dw1, const float* db_eff, float* dw, float* db, int K, int C0, int C1, hipStream_t stream);
/* every conv weight of a model in one launch: jobs = DEVICE table njobs x 8 int64 {w, wp, wt, Cout, Cin, taps, first_block, ci_tiles}; job j
 * owns one block per 32 x 32 (cout, cin) tile -- (KP(Cout)/32) * ci_tiles blocks with ci_tiles = KP(Cin)/32 -- starting at first_block;
 * the tile passes through LDS so that both operand layouts are written in contiguous runs.  taps = 1 or 9 (a job with any other value packs nothing).  block_job (optional, DEVICE
 * int32 [total_blocks]) = job index of every block (otherwise each block searches the table). */
int hn_pack_weights_batched(const long* jobs, int njobs, long total_blocks, const int* block_job, hipStream_t stream);
/* the remaining per-step packs of a model (depthwise taps = hn_dw_pack, grouped-conv stencil operands = hn_gconv_pack, block-diagonal MFMA
 * operands = hn_gconv_pack_diag, channel-slice / phase-form packs = hn_pack_weight_ex) in one launch: jobs = DEVICE table njobs x 16 int64
 * {w, out0, out1, out2, bias, kind 1..4, first_block, p0..p5, 0, 0, 0} with the parameters of the single-weight entry point of that kind,
 * one thread per output element; block_job = DEVICE int32 [total_blocks].  Kind 3 writes only the 8 x 8 diagonal blocks of the block-diagonal
 * operands: the caller's (persistent) buffers must have been zero-filled once. */
int hn_pack_small_batched(const long* jobs, const int* block_job, long total_blocks, hipStream_t stream);

/* out[pixel][cout] = act(bias[cout] + sum_{tap,c} X(pixel, tap)[c] * w[cout][tap][c]); X is gathered on the fly:
 *   mode 0: X = x0 rows (1x1 conv; also every dgrad of a 1x1 conv)            nn.Conv2d k=1: net/anynet.py:29-33,52-60;
 *           net/bifpn.py:58-102; net/common.py:95; head_lane/lanedetect.py:45-64
 *   mode 1: 1x1 conv stride 2 (XBlock shortcut)                                 net/anynet.py:57-60
 *   mode 2: 3x3 conv over reflect-pad-1 of cat[nearest_up2(x0) if up else x0, x1]   head_seg/segmentation.py:16-48,84-105
 *   mode 3: 3x3 "full" correlation of zero-extended x0 (dgrad of mode 2 on the padded (H+2)x(W+2) grid; H, W passed here are the
 *           PADDED sizes); fold back with hn_seg_fold.
 *   mode 4: mode 2 with replicate (clamp) padding, no up-sampling / concat: the low-resolution form of a 3x3 reflect-pad conv over a
 *           nearest-x2 up-sampled map (reflection of the up-sampled index == clamping of the source index); used with 4-phase
 *           effective weights for the final seg conv (head_seg/segmentation.py:101-104).  With out_f32 and
 *           img_stride = -k (k = Nout / 4) the epilogue stores depth-to-space itself: out is fp32 [N][2H][2W][k].
 *   mode 5: grouped 3x3 conv, group width 8, stride 1, zero padding 1 (XBlock conv_block_2, net/anynet.py:34-38) on MFMA: cout tile t
 *           (64 couts = 8 groups) contracts only over input channels [64t, 64t+64) with block-diagonal weights from
 *           hn_gconv_pack_diag (w = wk for the forward, wd for the data gradient); Nout == C0, KP == 64, no statistics.
 * (n_img, H, W) describe the OUTPUT pixel grid, M = n_img*H*W rows.  psum/psq (optional) receive per-wave partial sums / sums of
 * squares of the bf16-rounded outputs, [hn_nt_stat_rows(M, Nout)][Nout], for training-mode BatchNorm (F.batch_norm statistics); with
 * act != 0 they are taken before the activation (of bf16(bias + sum), fp32 outputs unrounded).
 * rpi/img_stride (optional, 0 = off): out offset(pixel) = (pixel / rpi) * img_stride + (pixel % rpi) * ldc, which writes a pyramid
 * level straight into the per-image concatenation of head_detect/detection.py:37-44,74-83. */
int hn_conv_gemm_nt(const void* x0, const void* x1, int mode, int n_img, int H, int W, int C0, int C1, int ld0, int ld1, int up, long M,
                    const void* w, int Nout, int KP, int taps, const float* bias, int act, void* out, int out_f32, int ldc, long rpi,
                    long img_stride, float* psum, float* psq, hipStream_t stream);
int hn_nt_stat_rows(long M, int Nout);
/* pixel rows summed into one partial row (64 or 128; the last tile may be ragged): a caller that reads the rows per IMAGE (the SE
 * gate-gradient partials, emode 1) needs H*W to be a multiple of it -- M / hn_nt_stat_rows is NOT the tile size when M is ragged */
int hn_nt_stat_tile(long M, int Nout);
/* hn_conv_gemm_nt for large maps of plain pixel rows with a short K (mode 0, one tap, one operand, bf16 output, no rpi mapping), as a
 * persistent streaming launch: the [Nout][KP] weights stay in LDS, each workgroup walks 64-row pixel tiles of a static partition with the
 * next tiles' operand DMA under the current tile's MFMAs and epilogue (no workgroup ever waits for another).
 * Domain: hn_nt_stream_ok(M, C0, Nout, KP) -- KP <= 128, KP % 32 == 0, 64 < Nout <= 128, Nout % 8 == 0, C0 % 8 == 0, C0 <= KP and M in the
 * range where hn_nt_stat_tile(M, Nout) == 64 -- with ld0 % 8 == 0, ldc % 8 == 0 and 16-byte aligned x, w, out.  Anything else returns
 * HN_ERR_UNSUPPORTED and nothing is written.
 * Contract: hn_conv_gemm_nt's on that domain, BIT FOR BIT: out = act(bf16(sum + bias)) with the same MFMA K order and rounding points, and
 * psum / psq (optional) = the same [hn_nt_stat_rows(M, Nout)][Nout] partial rows -- row t = the sums over the live rows of pixel tile t
 * (rows [64 t, 64 t + 64)) of q and q^2, q = bf16(sum + bias) before the activation, in the same summation order.
 * wg_limit: 0 = a grid sized from the device (two workgroups per CU, at most one per tile); k > 0 = k workgroups, capped by that device
 * size (tests: multi-tile walks, uneven shares and idle workgroups on tiny shapes; a tuning handle). */
int hn_conv_gemm_nt_stream(const void* x, int ld0, long M, int C0, const void* w, int Nout, int KP, const float* bias, int act, void* out,
                           int ldc, float* psum, float* psq, int wg_limit, hipStream_t stream);
int hn_nt_stream_ok(long M, int C0, int Nout, int KP);
/* mode 5 with psum/psq: one partial row per 16x16 output patch */
int hn_direct_stat_rows(int n_img, int H, int W);
/* Plain-rows 1x1 GEMM (hn_conv_gemm_nt mode 0, one tap, bf16 out) with ONE PACKED WEIGHT MATRIX PER IMAGE: rows [n * rows_per_image,
 * (n + 1) * rows_per_image) of x0 use w + n * w_img_stride ([Nout][KP] bf16 each; rows_per_image % 128 == 0).  addend (optional): added
 * BEFORE the activation.  hn_scale_weight_gate makes such operands: out[n][co][k] = bf16(wp[co][k] * gate[n][k]).  Inference: an XBlock's
 * conv_block_3 with the SE gate folded into its weights per image (net/anynet.py:68-75) instead of a b * gate pass over the activation. */
int hn_conv_gemm_nt_imgw(const void* x0, int ld0, long M, int C0, const void* w, long w_img_stride, long rows_per_image, int Nout, int KP,
                         const float* bias, int act, void* out, int ldc, const void* addend, int ld_add, hipStream_t stream);
int hn_scale_weight_gate(const void* wp, const float* gate, void* out, int N, int Cout, int C, int KP, hipStream_t stream);
/* The same plain-rows GEMM on LEVEL-PACKED rows with the per-level eval-mode BatchNorm + activation of the det towers in the epilogue
 * (head_detect/detection.py:60-75): out = act(coef[l][0][c] * (x W^T + bias) + coef[l][1][c]), l = the level of the row; rows [nlev] =
 * rows of every level (multiples of 128: hn_bn_act_levels' argument), coef [nlev][4][Nout].  Inference: one launch per tower layer's
 * pointwise conv + BatchNorm + Swish instead of two. */
int hn_conv_gemm_nt_lvl(const void* x0, int ld0, long M, int C0, const void* w, int Nout, int KP, const float* bias, int act, void* out,
                        int ldc, const float* coef, int nlev, const long* rows, hipStream_t stream);
/* hn_conv_gemm_nt for level-packed plain rows whose fp32 output is the per-image concatenation of the pyramid levels (Regressor / Classifier,
 * head_detect/detection.py:36-60: the same convs on every level, torch.cat along the anchor axis): row image * H_l W_l + pixel of level l ->
 * out + image * img_stride + (sum_{k<l} H_k W_k + pixel) * ldc.  Levels start on row_align-aligned rows (a multiple of 128); alignment rows
 * are not stored.  M = the packed tensor's rows.  One launch instead of one hn_conv_gemm_nt per level. */
int hn_conv_gemm_nt_lvlout(const void* x0, int ld0, long M, int C0, const void* w, int Nout, int KP, const float* bias, int act, float* out,
                           int ldc, long img_stride, int n_img, int nlev, const int* H, const int* W, int row_align, hipStream_t stream);

/* hn_conv_gemm_nt with (a) an operand transform for modes 0/1 (bf16 output): the pixel operand is act(xscale[c]*x + xshift[c]) rounded to
 * bf16 and optionally multiplied by xgate[row / xhw][c] -- BatchNorm apply (+ReLU, + SE gate) of the producer folded into this conv's
 * operand path (net/anynet.py:67-70: conv_block_3 consumes SE(relu(bn2(conv_block_2)))), nothing materialised; and (b) an addend for the
 * staged bf16 epilogue: out = bf16(bf16(acc) + addend[pixel][cout]) (the residual-gradient add of an XBlock's conv_block_1 dgrad); with
 * ld_add < 0 the addend (row stride -ld_add) goes in BEFORE the activation: out = act(acc + bias + addend) -- inference with folded
 * BatchNorm: conv_block_3 + identity branch + ReLU of an XBlock in one launch (net/anynet.py:70-76).  add_mode 1 (mode 0, ld_add > 0,
 * even H, W): the addend lives on the stride-2 sub-grid [N][H/2][W/2] and is added at even (y, x) only -- the data gradient of a
 * stride-2 XBlock's shortcut conv joins the data gradient of its conv_block_1 (both read the same input, net/anynet.py:65-76) without a
 * zero-filled full-resolution tensor and a separate addition. */
int hn_conv_gemm_nt_ex(const void* x0, const void* x1, int mode, int n_img, int H, int W, int C0, int C1, int ld0, int ld1, int up, long M,
                       const void* w, int Nout, int KP, int taps, const float* bias, int act, void* out, int out_f32, int ldc, long rpi,
                       long img_stride, float* psum, float* psq, const float* xscale, const float* xshift, const float* xgate, long xhw,
                       int xact, const void* addend, int ld_add, int add_mode, hipStream_t stream);
/* hn_conv_gemm_nt_ex (no operand transform) whose statistics rows carry a backward reduction over (output, ez) instead of the output's
 * BatchNorm statistics, so that the reduce pass that would follow the launch is not needed (net/anynet.py:50-78 XBlock backward):
 *   emode 1: psum[tile][c] = sum_rows q * bf16(relu(ecoef[0][c] * ez + ecoef[1][c]))   the SE gate-gradient partials of dbg = dz3 W3
 *            (what hn_se_bwd_reduce_fused computes; psq may be NULL);
 *   emode 2: g = q * [ecoef[0][c] * ez + ecoef[1][c] > 0];  psum = sum g,  psq = sum g * (ez - ecoef[2][c]) * ecoef[3][c]
 *            (the partial sums of hn_bn_bwd_reduce_fused with ReLU; modes 0/1: one row per pixel tile, hn_nt_stat_rows; mode 5: one row
 *            per 16x16 patch, hn_direct_stat_rows), consumed by hn_bn_bwd_apply_fused.
 * q = the bf16-rounded output; ez = bf16 [M][ld_ez] on the output's pixel rows; ecoef = fp32 [4][Nout]; bf16 output, no activation. */
int hn_conv_gemm_nt_stat(const void* x0, const void* x1, int mode, int n_img, int H, int W, int C0, int C1, int ld0, int ld1, int up, long M,
                         const void* w, int Nout, int KP, int taps, const float* bias, int act, void* out, int out_f32, int ldc, long rpi,
                         long img_stride, float* psum, float* psq, const void* addend, int ld_add, int add_mode, int emode, const void* ez,
                         int ld_ez, const float* ecoef, hipStream_t stream);
/* Data-gradient GEMM of an identity XBlock's conv_block_1 (dx = dz1 W1 + g, the addend joining after the rounding), whose statistics rows
 * are the reduce pass of the PREVIOUS block's masked BatchNorm-3 backward over the dx it produces: psum / psq [ceil(M / 64)][Nout] =
 * sum g', sum g' (ez - mean) rstd with g' = dx [ey > 0] (ez = that block's conv_block_3 output, ey = its output, ecoef fp32 [4][Nout] its
 * BatchNorm-3 coefficients).  Consumed by hn_bn_bwd_apply_fused.  Only where hn_nt_stat_rows(M, Nout) == ceil(M / 64) (the 64 x 64 tiling);
 * HN_ERR_ARG otherwise.  Replaces the first pass of aten::native_batch_norm_backward of net/anynet.py:65-76's last BatchNorm. */
int hn_conv_gemm_nt_stat3(const void* x0, int ld0, long M, int C0, const void* w, int Nout, int KP, void* out, int ldc, float* psum, float* psq,
                          const void* addend, int ld_add, const void* ez, int ld_ez, const void* ey, int ld_ey, const float* ecoef,
                          hipStream_t stream);
/* wgrad: dw[Cout][Cin][taps] (PyTorch layout, fp32) = sum_pixel dz[pixel][cout] * X(pixel, tap)[c]; X modes 0..2 as above.
 * dz rows must be zero padded up to ldz >= Nout rounded up to 8.  workspace: fp32, size from hn_wgrad_plan.
 * Replaces aten::convolution_backward's weight gradient. */
int hn_wgrad_plan(int mode, int n_img, int H, int W, long M, int Nout, int KP, int taps, int* splits, long* rows_per_split, long* ws_bytes);
int hn_conv_gemm_tn(const void* x0, const void* x1, int mode, int n_img, int H, int W, int C0, int C1, int ld0, int ld1, int up, long M,
                    const void* dz, int ldz, int Nout, int KP, int taps, float* workspace, float* dw, hipStream_t stream);

/* ---- NHWC stencils (hn_stencil.hip) ----------------------------------------------------------------------------------------- */

/* Stem: x NCHW fp32 [N,3,H,W], w fp32 [32][3][3][3] -> z NHWC bf16 [N,H/2,W/2,32] (conv 3x3 s2 p1, net/anynet.py:12,17).
 * patches (optional): bf16 im2col rows [N*H/2*W/2][32] (27 taps in weight order + 5 zeros) so that the weight gradient is one
 * hn_conv_gemm_tn(mode 0) call on MFMA. */
int hn_stem_fwd(const float* x, const float* w, void* z, void* patches, int N, int H, int W, hipStream_t stream);

/* Grouped 3x3 conv, group width 8, pad 1, stride 1|2 (XBlock conv_block_2, net/anynet.py:34-35).
 * hn_gconv_pack: fp32 [C][8][3][3] -> wk[tap][i][G][o] and wd (o/i swapped; flip=1 also flips the taps for stride-1 dgrad).
 * The stride-2 kernels contract with packed bf16 dot products and want the CONTRACTION index contiguous: hn_gconv_fwd(stride 2) takes the
 * pack whose last index is the input channel = `wd` of hn_gconv_pack(flip = 0); hn_gconv_dgrad_s2 takes the pack whose last index is the
 * output channel = `wk`.  (stride 1, the VALU form: hn_gconv_fwd takes `wk`, its data gradient = hn_gconv_fwd on dz with `wd` of flip = 1.) */
int hn_gconv_pack(const float* w, void* wk, void* wd, int C, int flip, hipStream_t stream);
int hn_gconv_fwd(const void* in, int ldi, const void* wk, void* out, int ldo, int N, int Hi, int Wi, int C, int stride, hipStream_t stream);
int hn_gconv_dgrad_s2(const void* dz, int ldz, const void* wd, void* dx, int ldx, int N, int Hi, int Wi, int C, hipStream_t stream);
long hn_wgrad_chunks(long pixels, long items);
int hn_gconv_wgrad(const void* x, int ldx, const void* dz, int ldz, float* part, int N, int Hi, int Wi, int C, int stride,
                   hipStream_t stream);

/* Depthwise 3x3, stride 1, zero pad 1 (SeparableConvBlock.depthwise_conv, net/common.py:91-92,104). */
int hn_dw_pack(const float* w, void* wk, void* wkf, int C, hipStream_t stream);
int hn_dwconv_fwd(const void* in, int ldi, const void* wk, void* out, int ldo, int N, int H, int W, int C, hipStream_t stream);
/* level-packed form: rows of nlev (<= 5) pyramid levels [N,H[l],W[l],C] stacked in one tensor, one launch (the det-head towers apply the
 * same SeparableConvBlock to every level, head_detect/detection.py:30-35,67-72) */
/* row_align (>= 1): every level starts on a multiple of row_align rows ("ragged" packing: levels whose row count is not a multiple of the
 * 128-row GEMM / BatchNorm blocks are padded; this kernel writes ZEROS to the alignment rows so downstream sums can be corrected exactly).
 * accumulate = 1: out += (used as the data gradient of a packed map that feeds both det towers: the second tower adds in place). */
int hn_dwconv_fwd_levels(const void* in, int ldi, const void* wk, void* out, int ldo, int N, int C, int nlev, const int* H, const int* W,
                         int row_align, int accumulate, hipStream_t stream);
/* partial rows of hn_dwconv_wgrad*: strips = sum over levels of N * H * ceil(W / 4) (the kernel walks 4-pixel strips) */
long hn_dwconv_wgrad_blocks(long strips, int C);
int hn_dwconv_wgrad(const void* x, int ldx, const void* dz, int ldz, float* part, int N, int H, int W, int C, hipStream_t stream);
/* level-packed: part is fp32 [hn_dwconv_wgrad_blocks(total pixels, C)][C*9] */
int hn_dwconv_wgrad_levels(const void* x, int ldx, const void* dz, int ldz, float* part, int N, int C, int nlev, const int* H, const int* W,
                           int row_align, hipStream_t stream);
/* depthwise 3x3 backward in one pass over (dz, x): dx (optional; `accumulate`: added to an existing tensor) = conv(dz, flipped weights wf
 * [9][C] bf16) and the weight-gradient partial rows part [hn_dwconv_bwd_blocks(strips, C)][C*9] (strips = sum over levels of
 * N * H * ceil(W / 4)); reduce with hn_rows_reduce.  Reference: the backward of SeparableConvBlock.depthwise_conv (net/common.py:91-92,104). */
long hn_dwconv_bwd_blocks(long strips, int C);
/* ... for these maps, whichever form of the kernel hn_dwconv_bwd_levels takes (strips walked by lanes, or -- C <= 120, >= 512 tiles -- 8 x 16-pixel
 * tiles staged in LDS: two workgroups per CU, one partial row each); -1: bad argument.  Callers size `part` with THIS. */
long hn_dwconv_bwd_blocks_levels(int N, int C, int nlev, const int* H, const int* W);
int hn_dwconv_bwd_levels(const void* dz, int ldz, const void* x, int ldx, const void* wf, void* dx, int lddx, float* part, int N, int C,
                         int nlev, const int* H, const int* W, int row_align, int accumulate, hipStream_t stream);

/* 3x3/s2 max pools: mode 0 = zero pad right/bottom, zeros take part in the max (MaxPool2dStaticSamePadding, net/common.py:138-151);
 * mode 1 = nn.MaxPool2d(3,2,1) (head_lane/lanedetect.py:40).  Backward recomputes the arg-max (first maximum wins). */
int hn_maxpool_fwd(const void* in, int ldi, void* out, int ldo, int N, int H, int W, int C, int mode, hipStream_t stream);
int hn_maxpool_bwd(const void* in, int ldi, const void* dout, int ldd, void* dx, int ldx, const float* wscale, int N, int H, int W, int C,
                   int mode, hipStream_t stream);
/* two-pass form of the same backward (arg-max bytes of every window in arg_ws = N*(H/2)*(W/2)*C bytes, then a gather per input pixel) */
int hn_maxpool_bwd2(const void* in, int ldi, const void* dout, int ldd, void* dx, int ldx, const float* wscale, void* arg_ws, int N, int H,
                    int W, int C, int mode, int accumulate, hipStream_t stream);

/* Nearest x2 up-sampling and its backward (F.interpolate / nn.Upsample, net/bifpn.py:43-46, head_lane/lanedetect.py:10-13). */
int hn_up2_fwd(const void* in, int ldi, void* out, int ldo, int N, int H, int W, int C, hipStream_t stream);
int hn_sum2x2(const void* g, int ldg, void* out, int ldo, const float* wscale, int N, int H, int W, int C, int accumulate, hipStream_t stream);

/* BiFPN fusion node out = swish(sum_i w[i]*T_i(in_i)) (net/bifpn.py:177-231); mode[i]: 0 absent, 1 same res, 2 nearest x2 of a
 * half-res map, 3 zero-pad-same max-pool of a double-res map.  w: 3 fp32 in device memory. */
/* backward of w = relu(p)/(sum relu(p)+eps) (net/bifpn.py:179-180; the forward normalisation runs inside hn_fuse_fwd) from the per-block
 * partials of hn_fuse_bwd */
int hn_fuse_dweights(const float* pw, int blocks, const float* praw, int nw, float eps, float* dp, hipStream_t stream);
int hn_fuse_fwd(const void* const* in, const int* ld, const int* mode, const float* w, void* out, int ldo, int N, int H, int W, int C,
                hipStream_t stream);
/* the same with the normalisation of the raw fusion parameters inside the kernel (wn [3] is written for the backward pass) */
int hn_fuse_fwd_raw(const void* const* in, const int* ld, const int* mode, const float* praw, int nw, float eps, float* wn, void* out, int ldo,
                    int N, int H, int W, int C, hipStream_t stream);
/* `accumulate` / acc[i] = 1 in hn_fuse_bwd, hn_sum2x2 and hn_maxpool_bwd2: the destination already holds the gradient another consumer of
 * the same tensor wrote (a BiFPN map feeds 2-3 nodes, net/bifpn.py:186-231) and this consumer's contribution is added in place (fp32 add,
 * one bf16 rounding) -- the autograd engine's separate gradient-accumulation kernels disappear (ops.Share / ops.GradSlot). */
/* hn_fuse_bwd, din[i]: destination of input i's gradient for mode 1 (same grid) AND mode 2 inputs (nearest x2 of a half-resolution map:
 * din[i] is [N][H/2][W/2][.], the kernel walks the output in 2x2 quads and writes w_i * the quad sum itself; NULL: the caller runs
 * hn_sum2x2 over g); mode 3 (max-pooled) inputs: NULL, routed by hn_maxpool_bwd2. */
int hn_fuse_bwd_blocks(int N, int H, int W, int C);
int hn_fuse_bwd(const void* const* in, const int* ld, const int* mode, const float* w, const void* dout, int ldd, void* g, int ldg,
                void* const* din, const int* ldin, const int* acc, float* pw, int N, int H, int W, int C, hipStream_t stream);
/* hn_fuse_bwd that also writes the arg-max bytes of the pooling windows of every mode-3 input i with arg_out[i] != NULL ([N][H][W][C] uint8:
 * the kernel recomputes those windows anyway), and the second pass of hn_maxpool_bwd2 on its own, fed with such bytes (H, W = the pool's
 * INPUT resolution): one launch per pooled fusion input in the backward pass instead of two (net/bifpn.py:206-231) */
int hn_fuse_bwd_arg(const void* const* in, const int* ld, const int* mode, const float* w, const void* dout, int ldd, void* g, int ldg,
                    void* const* din, const int* ldin, const int* acc, float* pw, void* const* arg_out, int N, int H, int W, int C,
                    hipStream_t stream);
int hn_maxpool_bwd_from_arg(const void* arg, const void* dout, int ldd, void* dx, int ldx, const float* wscale, int N, int H, int W, int C,
                            int mode, int accumulate, hipStream_t stream);

/* Data gradient of a 3x3 conv over a reflection-padded (clamp = 0: ConvBlock / Conv3x3, head_seg/segmentation.py:40-58) or, in phase form,
 * replicate-padded (clamp = 1) input, written straight to the unpadded gradient: dx [N][H][W][Nout] (row stride ldo) = fold(full
 * correlation of dz with the transposed weights) [* ELU'(yprev)].  Replaces hn_conv_gemm_nt(mode 3) on the padded grid + hn_seg_fold:
 * the conv epilogue writes the interior of the padded grid in place and the one-pixel ring to `ring`
 * [N][hn_fold_ring_rows(H, W)][Nout] bf16; a border fix-up adds the ring to the 2 (H + W) pixels per image it mirrors onto.
 * phase_k = 0: dz [N][H][W][Cz], wt [Nout][9][KP];  phase_k > 0: dz = space-to-depth gradient [N][H][W][4 k], wt = transposed effective
 * weights.  HN_ERR_UNSUPPORTED (3) unless Nout % 8 == 0, Nout > 32, H, W >= 4 -- callers keep the two-pass path for those shapes. */
long hn_fold_ring_rows(int H, int W);
int hn_conv3x3_dgrad_fold(const void* dz, int ldz, int Cz, int n_img, int H, int W, const void* wt, int Nout, int KP, int phase_k, int clamp,
                          void* out, int ldo, const void* yprev, int ldy, void* ring, hipStream_t stream);
/* The same gradient (also) in SPACE-TO-DEPTH order: out_s2d [N][H/2][W/2][4 Nout] (row stride ld_s2d >= 4 Nout; H, W even), pixel (y, x)
 * channel c at row (y/2, x/2), channel ((y&1) 2 + (x&1)) Nout + c -- the form in which the phase-form block that produced this conv's input
 * consumes its gradient (that block's hn_space_to_depth_bf16 pass is not needed; head_seg/segmentation.py:92-104).  out = NULL: only that
 * form (a block without a skip operand reads nothing else); otherwise both.  yprev stays [N][H][W] (row stride ldy). */
int hn_conv3x3_dgrad_fold_s2d(const void* dz, int ldz, int Cz, int n_img, int H, int W, const void* wt, int Nout, int KP, int phase_k, int clamp,
                              void* out, int ldo, void* out_s2d, int ld_s2d, const void* yprev, int ldy, void* ring, hipStream_t stream);
/* Backward of ReflectionPad2d(1) (+ nearest x2, + channel split of the concat) for the seg decoder (head_seg/segmentation.py:40,92-99). */
int hn_seg_fold(const void* dvp, int ldv, int c0, void* out, int ldo, const void* yprev, int ldy, int N, int H, int W, int C, int up,
                hipStream_t stream);
/* up = 2 selects the replicate-padding fold (backward of mode 4). */

/* Pixel shuffle of the phase-decomposed final seg conv, gradient side: fp32 [N][2h][2w][k] -> zero-padded bf16 [N][h][w][ldo] with channel
 * (py*2+px)*k + o (the forward shuffle is the output conv's own epilogue, mode 4 above). */
int hn_space_to_depth(const float* dy, void* out, int ldo, int N, int h, int w, int k, hipStream_t stream);

/* bf16 form: in [N][2h][2w][k] (row stride ldi) -> out [N][h][w][4k], phase-major channels (the operand layout of the phase-form convs);
 * psum (optional, fp32 [hn_space_to_depth_blocks][k], needs 256 % (k/2) == 0): per-block channel sums of the tensor on its way through =
 * partial rows of the conv's bias gradient (head_seg/segmentation.py:60-67 ConvBlock bias), reduce with hn_rows_reduce */
int hn_space_to_depth_blocks(int N, int h, int w, int k);
int hn_space_to_depth_bf16(const void* in, int ldi, void* out, int N, int h, int w, int k, float* psum, hipStream_t stream);

/* Phase form of Conv3x3(ReflectionPad2d(1)(nearest_up2(x0))) (head_seg/segmentation.py:92-104, decoder blocks 1/3/5/7) on the LOW-resolution
 * grid: effective weights W_eff[(py,px,o)][c][dy][dx] = sum of the original taps that land on low-res offset (dy, dx) for output phase
 * (py, px); phase (py, px) is non-zero only on ky in {py, py+1}, kx in {px, px+1}, and only those 4 taps are visited (16 instead of 36
 * tap products per low-res pixel = 2.25x fewer MACs than convolving the up-sampled map).
 *   mode 4 (forward): x0 [N][H][W][C0] (low-res), w = packed W_eff [4k][9][KP(C0)], bias [4k], out bf16 [N][2H][2W][k] (row stride ldc),
 *           addend (optional, row stride ld_add, the output's layout) = pre-activation partial result of the full-resolution skip operand;
 *   mode 3 (data gradient): x0 = space-to-depth output gradient [N][H-2][W-2][4k] (H, W are the PADDED sizes), w = packed transposed
 *           weights [C][9][KP(4k)], out = padded-grid gradient [N][H][W][Nout] (fold with hn_seg_fold, up = 2).
 * hn_conv_gemm_tn_phase: gradient of W_eff (fp32 [4k][C0][3][3], zeros at unused taps) from x0 and the space-to-depth output gradient. */
int hn_conv3x3_phase(const void* x0, int mode, int n_img, int H, int W, int C0, int ld0, const void* w, int Nout, int KP, const float* bias,
                     int act, void* out, int ldc, int k, const void* addend, int ld_add, hipStream_t stream);
/* deploy forward of the seg head's output layer: Conv3x3(ReflectionPad2d(1)(nearest_up2(x0))) (head_seg/segmentation.py:101-104, phase
 * form: w = effective weights [4k][9][KP] from hn_pack_weight_ex, bias [4k]) fused with torch.argmax over the k classes
 * (model/model.py:197): mask int64 [N][2H][2W], first maximum wins; the fp32 logits are never written.  C0 <= 64, KP == 64, 4k <= 32,
 * W * k even (the staged tile's rows of 2 W k floats are whole 16-byte pieces), mask 16-byte aligned; HN_ERR_ARG otherwise. */
int hn_conv3x3_out_argmax(const void* x0, int n_img, int H, int W, int C0, int ld0, const void* w, int k, int KP, const float* bias, long* mask,
                          hipStream_t stream);
int hn_wgrad_plan_phase(int n_img, int H, int W, int Nout, int KP, int phase_span, int* splits, long* rows_per_split, long* ws_bytes);
int hn_conv_gemm_tn_phase(const void* x0, int n_img, int H, int W, int C0, int ld0, const void* dz, int ldz, int Nout, int KP, int phase_span,
                          float* workspace, float* dw, float* dbias_eff, hipStream_t stream);
/* hn_conv_gemm_tn without its slab reduce: job [8] (HOST array) receives {part, dw, splits, Nout, Cin, KP, taps, kind}; hn_wgrad_reduce_jobs
 * reduces up to four such jobs (njobs x 8 longs, host) in ONE launch -- the weight gradients of an XBlock's conv_block_1 / 2 / 3 / shortcut
 * (net/anynet.py:25-76) each had their own 5-7 us reduce launch.  dw is complete only after hn_wgrad_reduce_jobs. */
int hn_conv_gemm_tn_deferred(const void* x0, const void* x1, int mode, int n_img, int H, int W, int C0, int C1, int ld0, int ld1, int up, long M,
                             const void* dz, int ldz, int Nout, int KP, int taps, float* workspace, float* dw, long* job, hipStream_t stream);
int hn_wgrad_reduce_jobs(const long* jobs, int njobs, hipStream_t stream);
/* Deferred, grouped weight gradients of grouped 3x3 convs (group width 8, stride 1): up to 32 dw_j [C][8][3][3] (fp32) in one launch of the
 * patch kernel + one extract launch -- the conv_block_2 weight gradients of the identity XBlocks of one backbone stage (net/anynet.py:34-38).
 * jobs: HOST table, 9 int64 per job {x, dz, dw, n_img, H, W, C, ldx, ldz}; workspace: hn_gconv_wgrad_group_ws_bytes() bytes. */
long hn_gconv_wgrad_group_ws_bytes(const long* jobs, int njobs);
int hn_gconv_wgrad_group(const long* jobs, int njobs, float* workspace, hipStream_t stream);

/* Deferred parameter-gradient tails in ONE launch (ops.GradQueue): up to 64 small reductions that finish parameter gradients off the
 * backward pass's critical path.  jobs: HOST table, 8 int64 per job {kind, a, b, out, out2, n0, n1, n2}:
 *   kind 0: out[c] = sum_r a[r][c], a fp32 [n0 rows][n1 cols] -- partial-row folds of depthwise / stride-2 grouped conv weight gradients
 *           (reference ops: the weight gradient of net/common.py:85-95 depthwise convs, net/anynet.py:34-38 grouped convs);
 *   kind 1: BiFPN fusion-weight Jacobian (net/bifpn.py:179-180): a = per-block sums [n0][3], b = raw parameter [n1 <= 3], out = gradient
 *           [n1], n2 = float bits of eps;
 *   kind 2: SE MLP outer product (net/anynet.py:43-47): out[i][j] = sum_n a[n][i] * b[n][j], out2[i] = sum_n a[n][i]; a [n2][n0], b [n2][n1]. */
int hn_grad_tail(const long* jobs, int njobs, hipStream_t stream);

/* Deferred, grouped 1x1 weight gradients: up to 32 independent dw_j [Nout][Cin] (fp32) = dz_j^T . x_j in ONE GEMM launch (+ one slab-reduce
 * launch only when the jobs cannot fill the chip without a pixel split).  Replaces, for a whole backbone stage, the per-conv weight
 * gradients autograd's convolution_backward produces one by one (reference: conv_block_1 / conv_block_3 / shortcut of every XBlock,
 * net/anynet.py:29-33,52-60).  jobs: HOST table, 12 int64 per job {x0, dz, dw, mode, n_img, H, W, Cin, ld0, ldz, Nout, M}: x0 bf16 rows
 * (row stride ld0), dz bf16 [M][ldz], dw fp32 [Nout][Cin] out; mode 0: x rows = dz rows; mode 1: x is the [n_img][2H][2W] input of a
 * stride-2 1x1 conv with output grid [n_img][H][W] (M = n_img*H*W).  workspace: hn_wgrad_group_ws_bytes() bytes (-1: bad job table). */
long hn_wgrad_group_ws_bytes(const long* jobs, int njobs);
int hn_wgrad_group(const long* jobs, int njobs, float* workspace, hipStream_t stream);

/* hn_conv_gemm_tn (any mode but the grouped mode 5) that also returns the conv's bias gradient dbias [Nout] = column sums of dz (ConvBlock /
 * Conv3x3 bias, head_seg/segmentation.py:40-58; head output convs): one extra MFMA per k-step against an all-ones operand while the dz
 * fragments are in registers; the launch that reduces the weight-gradient slabs reduces the bias partials.
 * (dbias_eff of hn_conv_gemm_tn_phase: the same for the 4 k effective outputs, optional.) */
int hn_conv_gemm_tn_bias(const void* x0, const void* x1, int mode, int n_img, int H, int W, int C0, int C1, int ld0, int ld1, int up, long M,
                         const void* dz, int ldz, int Nout, int KP, int taps, float* workspace, float* dw, float* dbias, hipStream_t stream);

/* fp32 head-output gradient [N][rows][Nout] -> zero padded bf16 dz [N*rpi][ldz] (optionally times sigmoid'). */
int hn_head_grad(const float* dy, const float* y, long rpi, long img_stride, int lds, int Nout, void* dz, int ldz, long M, int sigmoid,
                 hipStream_t stream);

/* Stacks the pyramid levels a shared-weight head runs on (head_detect/detection.py:36-60 loops over them) into the level-packed operand of
 * the *_levels entry points: src[l] bf16 [N][H_l][W_l][C] (row stride ld[l]); level l's rows start at the row_align-aligned offset of dst
 * (row stride ldd); alignment rows are not written. */
int hn_pack_levels(const void* const* src, const int* ld, void* dst, int ldd, int N, int C, int nlev, const int* H, const int* W, int row_align,
                   hipStream_t stream);
/* hn_head_grad for every pyramid level of a level-packed head output in one launch: dy / y fp32 [N][sum_l H_l W_l][lds] (the per-image
 * concatenation of head_detect/detection.py:36-60), dz bf16 with level l's N*H_l*W_l rows at the row_align-aligned offsets of the packing
 * (as hn_dwconv_fwd_levels); alignment rows are not written. */
int hn_head_grad_levels(const float* dy, const float* y, long img_stride, int lds, int Nout, void* dz, int ldz, int N, int nlev, const int* H,
                        const int* W, int row_align, int sigmoid, hipStream_t stream);

/* ---- reductions, BatchNorm, SE, elementwise (hn_norm.hip) ------------------------------------------------------------------- */

long hn_colred_rows(long M, long align);
/* per-channel partial sums / sums of squares over row blocks of R rows: psum, psq are [ceil(M/R)][C] */
int hn_col_stats(const void* x, int ldx, long M, int C, long R, float* psum, float* psq, hipStream_t stream);
int hn_col_dot(const void* a, int lda, const void* b, int ldb, long M, int C, long R, float* pdot, float* psum, hipStream_t stream);
int hn_rows_reduce(const float* in, float* out, int G, int S, int C, float alpha, hipStream_t stream);
/* two arrays at once with ragged groups: outK[g][c] = sum of inK rows [g*S, min((g+1)*S, rows)), S = ceil(rows/G); folds the per-wave
 * partial statistic rows of a GEMM epilogue (or of hn_bn_bwd_reduce) before hn_bn_finalize / hn_bn_bwd_finalize */
int hn_rows_reduce2(const float* in1, const float* in2, float* out1, float* out2, int rows, int G, int C, hipStream_t stream);

/* Training-mode nn.BatchNorm2d (F.batch_norm): statistics -> (scale, shift, mean, rstd) + running-stat update. */
int hn_bn_finalize(const float* psum, const float* psq, int prows, int C, long count, const float* gamma, const float* beta, float eps,
                   float momentum, float* running_mean, float* running_var, float* scale, float* shift, float* mean, float* rstd,
                   hipStream_t stream);
int hn_bn_eval_coeff(const float* gamma, const float* beta, const float* rm, const float* rv, float eps, int C, float* scale, float* shift,
                     hipStream_t stream);
/* out = act(scale*z + shift [+ (rscale*res + rshift | res)])   (BN apply + ReLU/Swish + residual add, net/anynet.py:65-76) */
int hn_bn_act(const void* z, int ldz, const float* scale, const float* shift, const void* res, int ldr, const float* rscale,
              const float* rshift, int act, void* out, int ldo, long M, int C, hipStream_t stream);
/* BN backward: g = dout*act'(pre) (or dout*[y>0] when the saved post-ReLU output y is given); partial sums of g and g*xhat */
int hn_bn_bwd_reduce(const void* dout, int ldd, const void* z, int ldz, const void* y, int ldy, const float* scale, const float* shift,
                     const float* mean, const float* rstd, int act, long M, int C, long R, float* pg, float* pgx, hipStream_t stream);
int hn_bn_bwd_finalize(const float* pg, const float* pgx, int prows, int C, long count, float* dgamma, float* dbeta, float* mg, float* mgx,
                       hipStream_t stream);
int hn_bn_bwd_apply(const void* dout, int ldd, const void* z, int ldz, const void* y, int ldy, const float* scale, const float* shift,
                    const float* mean, const float* rstd, const float* mg, const float* mgx, int act, void* dz, int lddz, void* gout, int ldg,
                    long M, int C, hipStream_t stream);

/* Level-packed BatchNorm with per-level parameters (bn_list[level][i] of the det towers, head_detect/detection.py:23,31-35,60,68-72).
 * rows[l] = tensor rows of level l INCLUDING its alignment rows (each a multiple of 128), count[l] = real rows; the alignment rows of the
 * conv output hold bf16(conv_bias) exactly and are subtracted from the statistics; coef = [nlev][4][C] (scale, shift, mean, rstd), red = [nlev][2][C].
 * gamma/beta/running_*/dgamma/dbeta are HOST arrays of nlev device pointers.  Partial-row inputs hold one row per `div` tensor rows. */
int hn_bn_finalize_levels(const float* psum, const float* psq, int div, int C, int nlev, const long* rows, const long* count,
                          const void* const* gamma, const void* const* beta, void* const* running_mean, void* const* running_var, float eps,
                          float momentum, const float* conv_bias, float* coef, hipStream_t stream);
int hn_bn_act_levels(const void* z, int ldz, const float* coef, int act, void* out, int ldo, int C, int nlev, const long* rows,
                     hipStream_t stream);
int hn_bn_bwd_reduce_levels(const void* dout, int ldd, const void* z, int ldz, const void* y, int ldy, const float* coef, int act, int C,
                            long R, int nlev, const long* rows, float* pg, float* pgx, hipStream_t stream);
int hn_bn_bwd_finalize_levels(const float* pg, const float* pgx, int div, int C, int nlev, const long* rows, const long* count,
                              void* const* dgamma, void* const* dbeta, float* red, float* zero_c, hipStream_t stream);
int hn_bn_bwd_apply_levels(const void* dout, int ldd, const void* z, int ldz, const void* y, int ldy, const float* coef, const float* red,
                           int act, void* dz, int lddz, int C, int nlev, const long* rows, hipStream_t stream);

/* ---- fused BatchNorm passes (hn_fused.hip) ----------------------------------------------------------------------------------
 * The finalize step of a training-mode nn.BatchNorm2d (partial statistics -> scale/shift/mean/rstd + running statistics; partial gradient
 * sums -> dgamma/dbeta + the two means) runs in the PROLOGUE of the elementwise kernel that consumes it: grid = (64-channel chunks,
 * row blocks of RB rows), every workgroup reduces the P partial rows of its own 64 channels.  Replaces hn_bn_finalize + hn_bn_act and
 * hn_bn_bwd_finalize + hn_bn_bwd_apply (and the hn_rows_reduce2 folds in front of them) for net/anynet.py:31,36,54,59,65-76,
 * net/common.py:98, net/bifpn.py:58-102, head_lane/lanedetect.py:45-64. */
/* rows per row block for M rows x C channels.  kind 0: apply passes (P = partial rows their prologue reduces); kind 1: reduce passes (their
 * row-block count becomes the P of the apply that follows).  align > 0 (rows per image): RB divides align, <= 8 row blocks per image. */
long hn_fused_row_block(long M, int C, long align, int P, int kind);
/* out = act(bn(z) [+ res]) [* gate[row / HW][c]].  P > 0: training mode, statistics from psum/psq [P][C] (count = rows normalised over),
 * row block 0 writes coef [4][C] (scale, shift, mean, rstd) and updates rm/rv; P == 0: use coef as is (null = identity); P < 0: eval mode
 * (running statistics).  out may be null when only pool is wanted; pool (optional) [ceil(M/RB)][C] = per-row-block channel sums of the
 * bf16-rounded output (SE squeeze, net/anynet.py:42,68); gate (optional, RB divides HW): SE excite applied to the rounded output. */
int hn_bn_apply_fused(const void* z, int ldz, long M, int C, const float* psum, const float* psq, int P, long count, const float* gamma,
                      const float* beta, float eps, float momentum, float* rm, float* rv, float* coef, const void* res, int ldr, int act,
                      void* out, int ldo, float* pool, const float* gate, long HW, long RB, hipStream_t stream);
/* SE excite + gated apply in one launch (net/anynet.py:44-48,68-69: the second nn.Conv2d of the SE block, its Sigmoid and the
 * `x * se(x)` product together with the BatchNorm + ReLU in front of them): gate[n][c] = sigmoid(b2[c] + sum_j w2[c][j] hid[n][j]) (stored
 * to `gate` [N][C] when non-null), out[row][c] = bf16(act(coef[0][c] z + coef[1][c])) * gate[row / HW][c]; coef null = identity */
int hn_se_gate_apply(const void* z, int ldz, const float* coef, int act, const float* hid, const float* w2, const float* b2, float* gate,
                     void* out, int ldo, int N, long HW, int C, int Cs, hipStream_t stream);
/* BatchNorm backward.  g = dout * act'(scale*z+shift), or dout * [y > 0] when the saved block output y is given (ReLU after the residual
 * add), or, with gate/dpool (SE, RB divides HW): g = (dout*gate[n][c] + dpool[n][c]/HW) * [scale*z+shift > 0] where dout is the gradient of
 * the gated tensor.  reduce: pg/pgx [ceil(M/RB)][C] partial sums of g and g*xhat.  apply: dz = scale*(g - mean g - xhat*mean(g*xhat)),
 * dgamma/dbeta written by row block 0, gout (optional) = g in bf16 (the residual branch's gradient), zero_c (optional) = C zeros (the
 * gradient of a conv bias that feeds this BatchNorm: written here instead of by a fill launch). */
int hn_bn_bwd_reduce_fused(const void* dout, int ldd, const void* z, int ldz, const void* y, int ldy, const float* coef, int act,
                           const float* gate, const float* dpool, long HW, long M, int C, long RB, float* pg, float* pgx, hipStream_t stream);
int hn_bn_bwd_apply_fused(const void* dout, int ldd, const void* z, int ldz, const void* y, int ldy, const float* coef, int act,
                          const float* gate, const float* dpool, long HW, const float* pg, const float* pgx, int P, long count, float* dgamma,
                          float* dbeta, void* dz, int lddz, void* gout, int ldg, long M, int C, long RB, float* zero_c, hipStream_t stream);
/* per-row-block channel sums / sums of squares [ceil(M/RB)][C] of a bf16 tensor (statistics of convs without a statistics epilogue) */
int hn_col_stats_fused(const void* x, int ldx, long M, int C, long RB, float* psum, float* psq, hipStream_t stream);
/* SE backward, first pass over (dbg = gradient of the gated tensor, z = pre-BN conv_block_2 output): b = relu(scale*z+shift),
 * pdot [ceil(M/RB)][C] = per-row-block sums of dbg*b (gate gradient), bg (optional) = b*gate[n][c] in bf16 (operand of conv_block_3's
 * weight gradient). */
int hn_se_bwd_reduce_fused(const void* dbg, int ldd, const void* z, int ldz, const float* coef, const float* gate, long HW, void* bg, int ldb,
                           float* pdot, long M, int C, long RB, hipStream_t stream);

/* SE gating x * gate[n][c] and its data-path backward (net/anynet.py:40-48,68-69). */
int hn_scale_rows(const void* x, int ldx, const float* gate, long HW, void* out, int ldo, long M, int C, hipStream_t stream);
int hn_se_bwd_apply(const void* dout, int ldd, const float* gate, const float* dpool, long HW, void* db, int ldb, long M, int C,
                    hipStream_t stream);

/* SE excitation MLP on the pooled [N,C] vectors: hid = relu(W1 p + b1) [N,Cs], gate = sigmoid(W2 hid + b2) [N,C]; backward gives dpool and
 * the four parameter gradients (dpre2 [N,C], dpre1 [N,Cs] are scratch).  Replaces the two 1x1 nn.Conv2d of net/anynet.py:44-47. */
int hn_se_mlp_fwd(const float* pooled, const float* w1, const float* b1, const float* w2, const float* b2, float* hid, float* gate, int N,
                  int C, int Cs, hipStream_t stream);
/* forms fed by partial rows (S per image): pooled = alpha * sum of the squeeze partials of hn_bn_apply_fused (stored to `pooled`), and
 * dgate = sum of the partials of hn_se_bwd_reduce_fused -- the reductions ride on the first MLP kernel instead of their own launches.
 * hn_se_mlp_fwd_parts with gate == NULL runs the first layer only (w2 / b2 unused): the second one is hn_se_gate_apply's prologue */
int hn_se_mlp_fwd_parts(const float* pool_part, int S, float alpha, const float* w1, const float* b1, const float* w2, const float* b2,
                        float* pooled, float* hid, float* gate, int N, int C, int Cs, hipStream_t stream);
int hn_se_mlp_bwd_parts(const float* dgate_part, int S, const float* gate, const float* hid, const float* pooled, const float* w1,
                        const float* w2, float* dpre2, float* dpre1, float* dpool, float* dw1, float* db1, float* dw2, float* db2, int N,
                        int C, int Cs, hipStream_t stream);
int hn_se_mlp_bwd(const float* dgate, const float* gate, const float* hid, const float* pooled, const float* w1, const float* w2,
                  float* dpre2, float* dpre1, float* dpool, float* dw1, float* db1, float* dw2, float* db2, int N, int C, int Cs,
                  hipStream_t stream);

/* ---- persistent stage kernel (hn_xstage.hip) ----------------------------------------------------------------------------------- */

/* The stride-1 identity XBlocks 1..d-1 of a backbone stage (net/anynet.py:65-76,84-86; training mode) as ONE launch: 256 workgroups of 512
 * threads, workgroup = (image, channel slice), the workgroups of an image on one XCD (read from HW_REG_XCC_ID), in-image exchanges through
 * that XCD's L2, BatchNorm statistics exchanged device-wide as tagged 8-byte granules.  Replaces nb x the 8 launches of ops/backbone.py
 * XBlockFn.forward and leaves every tensor that node saves: z1 / a / z2 / bg / z3 / out [nb][N*H*W][C] bf16 (dense rows), coef [nb][3][4][C]
 * (scale, shift, mean, rstd of BatchNorm 1 / 2 / 3), pooled / gate [nb][N][C], hid [nb][N][Cs]; running statistics updated in place.
 * tab = HOST table nb x 19 int64: {w1 packed [C][KP], w2 block-diagonal pack (hn_gconv_pack_diag wk), w3 packed, se.1.weight [Cs][C],
 * se.1.bias, se.3.weight [C][Cs], se.3.bias, then (gamma, beta, running_mean, running_var) of BatchNorm 1, 2, 3}.  x0 = input of the first
 * block [N*H*W][C].  alpha = 1 / (H*W).  ws = hn_xstage_ws_bytes() bytes, ZEROED ONCE when allocated and then owned by these launches
 * (counters / tags continue across launches; one workspace per device, launches on it serialised).  ws word 64 (uint32) is the status word:
 * 0 = every launch so far completed; non-zero = a bounded wait expired (the launch could not become co-resident): outputs invalid.
 * stamps (optional) = [nb][16] uint64 real-time-counter stamps of one workgroup.  mode 0: XCD-local counters; 1: agent-scope counters +
 * release / acquire fences (placement independent).  hn_xstage_supported: 0 = shape not covered (caller keeps the launch chain). */
long hn_xstage_ws_bytes(void);
int hn_xstage_supported(int N, int H, int W, int C, int Cs);
int hn_xstage_fwd(const long* tab, int nb, const void* x0, void* z1, void* a, void* z2, void* bg, void* z3, void* out, float* coef,
                  float* pooled, float* hid, float* gate, int N, int H, int W, int C, int Cs, float eps, float momentum, float alpha,
                  void* ws, long* stamps, int mode, hipStream_t stream);
/* The backward of the same blocks (ops/backbone.py XBlockFn.backward, 21 launches per block), last block first, in ONE launch of the same
 * shape: BatchNorm-backward sums cross XCDs as granules, dz3 / dz1 (the operands of the two data-gradient GEMMs) and the SE partials stay in
 * the image's XCD, a block's dx is the next block's dout of the same workgroup.  tab = HOST table nb x 5 int64 per block, forward block
 * order: {wt1 (transposed pack of conv_block_1, hn_pack_weight), wd2 (hn_gconv_pack_diag's data-gradient operand), wt3, se.1.weight,
 * se.3.weight}.  Inputs: dout = gradient of the last block's output [N*H*W][C] bf16 (dense rows); the forward's stacked tensors z1 / z2 /
 * z3 / out, coef, hid, gate.  Outputs: dz1 / dz2 / dz3 [nb][N*H*W][C] bf16 (operands of the weight gradients, which stay separate launches),
 * dx [N*H*W][C] (gradient of the first block's input), dgb [nb][3][2][C] = (dgamma, dbeta) of BatchNorm 1 / 2 / 3, dpre2 [nb][N][C] and
 * dpre1 [nb][N][Cs] = pre-activation gradients of the two SE layers (their outer products with hid / pooled are the SE weight gradients).
 * ws, stamps, mode: as hn_xstage_fwd (the same workspace). */
int hn_xstage_bwd(const long* tab, int nb, const void* dout, const void* z1, const void* z2, const void* z3, const void* out,
                  const float* coef, const float* hid, const float* gate, void* dz1, void* dz2, void* dz3, void* dx, float* dgb,
                  float* dpre2, float* dpre1, int N, int H, int W, int C, int Cs, void* ws, long* stamps, int mode, hipStream_t stream);

/* out += b0 [+ b1] [+ b2] (bf16 [M][C] tensors, fp32 sum, one rounding): the gradient sum of a multi-consumer map whose consumers return
 * separate gradients (ops.Share.backward; net/bifpn.py outputs feed three heads) in one launch instead of one per extra consumer */
int hn_add_n(void* out, int ldo, const void* b0, int ld0, const void* b1, int ld1, const void* b2, int ld2, long M, int C, hipStream_t stream);
/* op 0: a+b, 1: a*act'(b = post-activation; ELU/ReLU), 2: alpha*a, 3: act(a), 4: a*act'(b = pre-activation) */
int hn_eltwise(int op, const void* a, int lda, const void* b, int ldb, void* out, int ldo, long M, int C, int act, float alpha,
               hipStream_t stream);
int hn_add_strided2(void* dx, int ldx, const void* dxs, int lds, int N, int Ho, int Wo, int C, hipStream_t stream);
int hn_cast_f32_to_bf16_pad(const float* src, int lds, void* dst, int ldo, long M, int C, hipStream_t stream);

/* ---- losses (hn_loss.hip; the detection losses: hn_det_loss.hip) ------------------------------------------------------------- */

/* Weighted cross entropy with ignore_index and optional top-k hardest pixels per image (CrossEntropyLoss.forward, use_focal=False,
 * head_seg/segmentation_loss.py:48-65).  logits: fp32 NHWC [N*HW][C] (row stride ldl); target: int64 or float32 class ids [N*HW];
 * k = int(top_k_ratio * HW).  The per-image k-th largest loss is found with an exact 3-level radix select instead of torch.sort.
 * ws: hn_seg_loss_ws_bytes(N, HW) bytes, written by fwd and read by bwd.  out[0] = mean loss; bwd writes dlogits (fp32, row stride ldd). */
long hn_seg_loss_ws_bytes(int N, long HW);
int hn_seg_loss_fwd(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* cw, int ignore_index, int N,
                    long HW, int use_topk, long k, void* ws, float* out, hipStream_t stream);
int hn_seg_loss_bwd(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* cw, int ignore_index, int N,
                    long HW, int use_topk, long k, const void* ws, const float* gout, float* dlogits, int ldd, hipStream_t stream);
/* the same gradient in the layout the phase-form 5-class output conv's backward consumes (hn_space_to_depth of dlogits, rounded to bf16):
 * dz bf16 [N][H/2][W/2][ldz], channel (py*2+px)*C + c of low-res pixel (y, x) = dlogits(2y+py, 2x+px, c), zeros in [4C, ldz) -- the fp32
 * dlogits tensor and the pass over it are skipped (head_seg/segmentation.py:101-104 -> segmentation_loss.py:48-65 chain) */
int hn_seg_loss_bwd_s2d(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* class_weights,
                        int ignore_index, int N, int H, int W, int use_topk, long k, const void* ws, const float* gout, void* dz, int ldz,
                        hipStream_t stream);
/* Focal variant of the seg loss (CrossEntropyLoss.forward with use_focal, head_seg/segmentation_loss.py:31-46; cfgs/hydranet_joint_small_backbone.yml):
 * p = softmax + 1e-8, t = one_hot + 1e-8, loss = mean over all N*HW pixels of sum_c t_c * (-alpha (1-p_c)^gamma log(p_c) w_c).  logits fp32
 * [N*HW][ldl], target float32 / int64 class ids (no ignore_index on this path, as in the reference); ws: fp32 [hn_seg_loss_blocks(N, HW)]. */
int hn_seg_loss_blocks(int N, long HW);
int hn_seg_focal_fwd(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* class_weights, float gamma,
                     float alpha, int N, long HW, void* ws, float* out, hipStream_t stream);
int hn_seg_focal_bwd(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* class_weights, float gamma,
                     float alpha, int N, long HW, const float* gout, float* dlogits, int ldd, hipStream_t stream);
/* Lovasz-softmax variant of the seg loss (segment.use_lovasz: head_seg/loss_lovasz.py lovasz_softmax(softmax(logits), gt, ignore=255),
 * classes='present', per_image=False; hn_lovasz.hip).  logits fp32 [N*HW][ldl], target int64 / float32 class ids; labels == ignore_index
 * are dropped, other labels outside [0, C) are background for every class.  Per-class sort order: error descending, then pixel index
 * ascending (deterministic; the reference's unstable sort leaves ties unspecified).  2 <= C <= 16.  ws: hn_seg_lovasz_ws_bytes(N, HW, C)
 * bytes, written by fwd and read by bwd (per-pixel gradient w.r.t. the probabilities, class counts).  out[0] = loss (0 when no class is
 * present); bwd writes dlogits (fp32, row stride ldd), bwd_s2d the space-to-depth bf16 operand of hn_seg_loss_bwd_s2d's layout. */
long hn_seg_lovasz_ws_bytes(int N, long HW, int C);
int hn_seg_lovasz_fwd(const float* logits, int ldl, int C, const void* target, int target_is_float, int ignore_index, int N, long HW,
                      void* ws, float* out, hipStream_t stream);
int hn_seg_lovasz_bwd(const float* logits, int ldl, int C, const void* target, int target_is_float, int ignore_index, int N, long HW,
                      const void* ws, const float* gout, float* dlogits, int ldd, hipStream_t stream);
int hn_seg_lovasz_bwd_s2d(const float* logits, int ldl, int C, const void* target, int target_is_float, int ignore_index, int N, int H,
                          int W, const void* ws, const float* gout, void* dz, int ldz, hipStream_t stream);
/* Detection loss (FocalLoss.forward, head_detect/detection_loss.py:132-267): cls fp32 [N][A][K] (post-sigmoid), reg [N][A][4], anchors
 * [A][4] (y1,x1,y2,x2), ann [N][Mx][5] (x1,y1,x2,y2,class; rows with class -1 are padding).  out[0] / out[1] = batch-mean classification /
 * regression loss.  assign: int16 [N][A]; part: fp32 [N][hn_det_loss_blocks(A)][3]; npos: fp32 [N] (all written by fwd, read by bwd). */
int hn_det_loss_blocks(int A);
int hn_det_loss_fwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx, void* assign,
                    float* part, float* npos, float* out, hipStream_t stream);
int hn_det_loss_bwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                    const void* assign, const float* npos, const float* gout, float* dcls, float* dreg, hipStream_t stream);
/* The same loss with an IoU-family regression term (detection.loss_reg_type; hn_det_loss.hip): kind 1 GIoU, 2 DIoU, 3 CIoU between the
 * deploy-mode decode of a positive anchor's (dy, dx, dh, dw) (exp clipped at log(1000/16)) and its annotation (sides clamped to >= 1),
 * per image the mean over its positives, then the batch mean.  Assignment and the classification loss are hn_det_loss_fwd's, bit for bit.
 * out[0] / out[1] = classification / regression loss, out[2] = mean IoU of the positives (reduced like the loss).  assign: int16 [N][A];
 * part: fp32 [N][hn_det_loss_blocks(A)][4]; npos: fp32 [N].  gout[2] = gradients of out[0], out[1]. */
int hn_det_loss_iou_fwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx, int kind,
                        void* assign, float* part, float* npos, float* out, hipStream_t stream);
int hn_det_loss_iou_bwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx, int kind,
                        const void* assign, const float* npos, const float* gout, float* dcls, float* dreg, hipStream_t stream);
/* ATSS anchor assignment (detection.assigner = atss; hn_det_atss.hip, the rule is stated there and in ops.det_atss_assign): per box the
 * topk * anchors_per_location nearest anchors (centre distance, ties to the lower index) on every level are its candidates, the threshold
 * is mean + std of their IoUs, a candidate at or above it whose centre lies inside the box is positive, conflicts go to the larger IoU.
 * level_sizes: HOST int [n_levels] (<= 8 levels, read during the call), the contiguous anchor ranges, summing to A; topk *
 * anchors_per_location <= 1024.  ws: hn_det_atss_ws_bytes(...) bytes (-1 for arguments the call would reject).  Writes assign int16 [N][A]
 * (>= 0 annotation index, -1 background; never -2) and thr fp32 [N][Mx] (rows of padding annotations are left unwritten).  Three launches. */
long hn_det_atss_ws_bytes(int N, int A, int Mx, const int* level_sizes, int n_levels, int topk, int anchors_per_location);
int hn_det_atss_assign(const float* anchors, const float* ann, int N, int A, int Mx, const int* level_sizes, int n_levels, int topk,
                       int anchors_per_location, void* ws, void* assign, float* thr, hipStream_t stream);
/* hn_det_loss_fwd / hn_det_loss_iou_fwd with assign [N][A] as an INPUT (e.g. hn_det_atss_assign's) instead of computing the max-IoU
 * assignment; values outside -2 .. Mx - 1 count as ignored.  The backward entry points above read the same assign. */
int hn_det_loss_fwd_assigned(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                             const void* assign, float* part, float* npos, float* out, hipStream_t stream);
int hn_det_loss_iou_fwd_assigned(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                                 int kind, const void* assign, float* part, float* npos, float* out, hipStream_t stream);
/* Detection loss with a quality classification term (detection.loss_cls_type = qfl | vfl; hn_det_loss.hip) and an IoU-family
 * regression term (kind 1 giou, 2 diou, 3 ciou).  The target of a positive anchor's class is the IoU q of its decoded prediction with its
 * annotation (the iou of hn_det_loss_iou_fwd, a constant in the backward), every other target is 0; with p^ = clamp(p, 1e-4, 1 - 1e-4),
 * BCE = -(y ln p^ + (1 - y) ln(1 - p^)): cls_kind 1 (qfl) l = (y - p^)^2 BCE; cls_kind 2 (vfl) l = y BCE for y > 0 and
 * 0.75 p^2 (-ln(1 - p^)) for y = 0; reduced like the focal term.  One pair for every variant: valid = the det row of the task masks or
 * NULL (every image labelled); assign_given = 0: the max-IoU assignment is computed and written to assign, 1: assign is read (values
 * outside -2 .. Mx - 1 count as ignored) and not written.  Regression loss, out[2], npos, dreg and part[..][1..3] are
 * hn_det_loss_iou_fwd / _bwd's, bit for bit.  Buffers as there; K <= 32.  Two launches forward, one backward. */
int hn_det_loss_quality_fwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx, int kind,
                            int cls_kind, const unsigned char* valid, int assign_given, void* assign, float* part, float* npos, float* out,
                            hipStream_t stream);
int hn_det_loss_quality_bwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx, int kind,
                            int cls_kind, const unsigned char* valid, const void* assign, const float* npos, const float* gout, float* dcls,
                            float* dreg, hipStream_t stream);
/* Task-aligned anchor assignment (detection.assigner = tal; hn_det_tal.hip, the rule is stated there and in ops.det_tal_assign): per box
 * the topk anchors with the largest metric t = score * IoU^6 among those whose centre lies inside the box, IoU being the iou of
 * hn_det_loss_iou_fwd for the anchor's own regression; conflicts go to the larger IoU.  regression fp32 [N][A][4] and classification fp32
 * [N][A][K] (post-sigmoid, K <= 32) are read as constants; anchors and regression 16-byte aligned; N <= 65535, Mx <= 32767,
 * 1 <= topk <= 2048.  ws: hn_det_tal_ws_bytes(...) bytes (-1 for arguments the call would reject).  Writes assign int16 [N][A] (>= 0
 * annotation index, -1 background; never -2) and target fp32 [N][A]: (t / tmax) * umax of an assigned anchor with the maxima taken over its
 * box's assigned anchors, else 0.  Three launches. */
long hn_det_tal_ws_bytes(int N, int A, int Mx, int topk);
int hn_det_tal_assign(const float* anchors, const float* regression, const float* classification, const float* ann, int N, int A, int K, int Mx,
                      int topk, void* ws, void* assign, float* target, hipStream_t stream);
/* hn_det_loss_quality_fwd / _bwd with the positives' classification target handed in: y = target[n][a] (fp32 [N][A], e.g.
 * hn_det_tal_assign's) instead of the box's IoU, in the forward and in the backward.  assign_given must be 1.  The regression loss, out[2],
 * npos and dreg are hn_det_loss_quality_fwd / _bwd's on the same assign, bit for bit. */
int hn_det_loss_aligned_fwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx, int kind,
                            int cls_kind, const unsigned char* valid, int assign_given, void* assign, const float* target, float* part,
                            float* npos, float* out, hipStream_t stream);
int hn_det_loss_aligned_bwd(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx, int kind,
                            int cls_kind, const unsigned char* valid, const void* assign, const float* target, const float* npos,
                            const float* gout, float* dcls, float* dreg, hipStream_t stream);
/* torch.argmax(seg, dim=1) of deploy mode (model/model.py:197): fp32 NHWC logits -> int64 class ids, first maximum wins. */
/* Lane losses (head_lane/lanedetect_loss.py:18-78).  cls: logits / one-hot target fp32 [M][2]; out[0] = positive term, out[1] = OHEM
 * negative term (NEGATIVE_RATIO 15, ALPHA 10: the k-th smallest background log-prob is found by a radix select, not a sort);
 * lsm [M][2], pmask [M] bytes and aux[4] = {threshold, max(#pos,1), #pos, #neg} are kept for the backward pass and the location loss.
 * loc: pred / target fp32 [M][L]; the x`alpha` weights sit at columns wcol, wcol+1 (the reference hard-codes wcol = 160). */
int hn_lane_cls_loss_fwd(const float* logits, const float* target, long M, float neg_ratio, float alpha, float* lsm, void* pmask,
                         float* out, float* aux, hipStream_t stream);
int hn_lane_cls_loss_bwd(const float* lsm, const void* pmask, const float* aux, const float* gpos, const float* gneg, float alpha, long M,
                         float* dlogits, hipStream_t stream);
int hn_lane_loc_loss_fwd(const float* pred, const float* target, const void* pmask, const float* aux, long M, int L, int wcol, float alpha,
                         float* rowloss, float* rownorm, float* out, hipStream_t stream);
int hn_lane_loc_loss_bwd(const float* pred, const float* target, const void* pmask, const float* rownorm, const float* aux,
                         const float* gout, long M, int L, int wcol, float alpha, float* dpred, hipStream_t stream);
/* Lane line-IoU location loss (lane.loss_loc_type: liou; CLRNet, CVPR 2022, section 3.4; DESIGN 4y) in place of the loc pair above.
 * pred / target fp32 [M][L] with L = 2 P + 2 (else 1): x-offsets at columns [0, P) and [P + 2, L), the two lengths at P and P + 1; a column
 * is valid iff target != 0.  e > 0 (finite, else 1) is the half width in target units.  Per positive row with n valid x-columns and
 * d = |pred - target|: I = sum (2e - d), U = sum (2e + d), term 1 - I / U (0 when n = 0), plus the loc loss's own term of the two length
 * columns (x`alpha` huber over nrm = max(#valid columns of the row, 1)).  out[0] = the sum over the positive rows / aux[1], out[1] = the
 * mean I / U over the positive rows with n > 0 (0 without one).  rowI, rowU, rownorm, rowloss: fp32 [M] workspace, all written for every
 * row (I = U = 0 on a row that is not positive); bwd reads rowU and rownorm and writes all of dpred [M][L], exactly 0 at invalid columns
 * and on rows that are not positive.  pmask / aux as left by hn_lane_cls_loss_fwd or its _masked twin, which already carry a task mask.
 * Two launches forward, one backward; no atomics (two runs give the same bits). */
int hn_lane_liou_loss_fwd(const float* pred, const float* target, const void* pmask, const float* aux, long M, int L, int P, float e,
                          float alpha, float* rowI, float* rowU, float* rownorm, float* rowloss, float* out, hipStream_t stream);
int hn_lane_liou_loss_bwd(const float* pred, const float* target, const void* pmask, const float* rowU, const float* rownorm,
                          const float* aux, const float* gout, long M, int L, int P, float e, float alpha, float* dpred, hipStream_t stream);
/* Per-image task masks (gt_dict["task_valid"], DESIGN 4u): every loss entry point above has a `_masked` twin that also takes `valid`, one
 * contiguous uint8 row of N bytes on the device (1 = image n is labelled for the task; NULL returns 1 before any launch).  The rule: the
 * losses equal the unmasked losses of the sub-batch of labelled images, taken in batch order; without a labelled image every loss is 0;
 * the gradient with respect to an unlabelled image's predictions is written as exactly 0.  The same kernels and the same number of
 * launches as the unmasked call; the mask is read on the device (no synchronisation, capturable); an all-ones mask gives the unmasked
 * call's bits.
 *   seg CE / top-k: sum over labelled images of their top-k sums / (N_valid k); focal: the mean over N_valid HW pixels; Lovasz: an
 *     unlabelled image's pixels are dropped like ignored pixels.  The workspaces are the unmasked calls' and go to the matching bwd.
 *   det: an unlabelled image's anchors are all ignored (its row of a computed assign is -2 throughout, npos = 0; a given assign is read
 *     only for labelled images and never written); the batch means, out[2] included, are taken over N_valid.  bwd takes the same mask.
 *   lane cls: M = N x rows; the rows of an unlabelled image are neither positive nor negative: they stay out of #pos, #neg, the rank, the
 *     select and both sums (lsm is still written, pmask is 0).  M % rows != 0 returns 1.  The location loss follows through pmask and aux
 *     and needs no twin. */
int hn_seg_loss_fwd_masked(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* class_weights,
                           int ignore_index, int N, long HW, int use_topk, long k, const unsigned char* valid, void* ws, float* out,
                           hipStream_t stream);
int hn_seg_loss_bwd_masked(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* class_weights,
                           int ignore_index, int N, long HW, int use_topk, long k, const unsigned char* valid, const void* ws,
                           const float* gout, float* dlogits, int ldd, hipStream_t stream);
int hn_seg_loss_bwd_s2d_masked(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* class_weights,
                               int ignore_index, int N, int H, int W, int use_topk, long k, const unsigned char* valid, const void* ws,
                               const float* gout, void* dz, int ldz, hipStream_t stream);
int hn_seg_focal_fwd_masked(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* class_weights,
                            float gamma, float alpha, int N, long HW, const unsigned char* valid, void* ws, float* out, hipStream_t stream);
int hn_seg_focal_bwd_masked(const float* logits, int ldl, int C, const void* target, int target_is_float, const float* class_weights,
                            float gamma, float alpha, int N, long HW, const unsigned char* valid, const float* gout, float* dlogits, int ldd,
                            hipStream_t stream);
int hn_seg_lovasz_fwd_masked(const float* logits, int ldl, int C, const void* target, int target_is_float, int ignore_index, int N, long HW,
                             const unsigned char* valid, void* ws, float* out, hipStream_t stream);
int hn_seg_lovasz_bwd_masked(const float* logits, int ldl, int C, const void* target, int target_is_float, int ignore_index, int N, long HW,
                             const unsigned char* valid, const void* ws, const float* gout, float* dlogits, int ldd, hipStream_t stream);
int hn_seg_lovasz_bwd_s2d_masked(const float* logits, int ldl, int C, const void* target, int target_is_float, int ignore_index, int N,
                                 int H, int W, const unsigned char* valid, const void* ws, const float* gout, void* dz, int ldz,
                                 hipStream_t stream);
int hn_det_loss_fwd_masked(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                           const unsigned char* valid, void* assign, float* part, float* npos, float* out, hipStream_t stream);
int hn_det_loss_fwd_assigned_masked(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                                    const unsigned char* valid, const void* assign, float* part, float* npos, float* out,
                                    hipStream_t stream);
int hn_det_loss_bwd_masked(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                           const unsigned char* valid, const void* assign, const float* npos, const float* gout, float* dcls, float* dreg,
                           hipStream_t stream);
int hn_det_loss_iou_fwd_masked(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                               int kind, const unsigned char* valid, void* assign, float* part, float* npos, float* out, hipStream_t stream);
int hn_det_loss_iou_fwd_assigned_masked(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K,
                                        int Mx, int kind, const unsigned char* valid, const void* assign, float* part, float* npos,
                                        float* out, hipStream_t stream);
int hn_det_loss_iou_bwd_masked(const float* cls, const float* reg, const float* anchors, const float* ann, int N, int A, int K, int Mx,
                               int kind, const unsigned char* valid, const void* assign, const float* npos, const float* gout, float* dcls,
                               float* dreg, hipStream_t stream);
int hn_lane_cls_loss_fwd_masked(const float* logits, const float* target, long M, int rows, const unsigned char* valid, float neg_ratio,
                                float alpha, float* lsm, void* pmask, float* out, float* aux, hipStream_t stream);
int hn_lane_cls_loss_bwd_masked(const float* lsm, const void* pmask, const float* aux, const float* gpos, const float* gneg, float alpha,
                                long M, int rows, const unsigned char* valid, float* dlogits, hipStream_t stream);
/* Greedy NMS on the device for the detection post-process (head_detect/detection_loss.py:70-108; torchvision batched_nms semantics):
 * boxes fp32 [K][4] (x1,y1,x2,y2) sorted by descending score with their class offsets added; suppress j > i when IoU > threshold, IoU in
 * separately rounded fp32 ops (bit-identical decisions to the host path).  mask: hn_nms_mask_words(K) uint64 scratch; keep: K bytes. */
long hn_nms_mask_words(int K);
int hn_nms_sorted(const float* boxes, int K, float iou_threshold, void* mask, void* keep, hipStream_t stream);
/* ---- stages either side of the hot path (hn_post.hip; SURVEY.md section 8(f)) ---------------------------------------------------- */

/* Detection post-process for a whole batch on the device (head_detect/detection_loss.py:7-108 BBoxTransform + ClipBoxes + postprocess;
 * torchvision.ops.batched_nms semantics restated: stable descending-score order, suppress when IoU > threshold, classes separated by an
 * offset of class_id * (max kept coordinate + 1)).  anchors fp32 [A][4] (y1,x1,y2,x2), regression [N][A][4], classification [N][A][K]
 * (post-sigmoid).  cap <= 32768 = per-image capacity.  Per image n: kept[n] boxes in descending-score order in rois [N][cap][4] (x1,y1,x2,y2),
 * class_ids int64 [N][cap], scores [N][cap]; total[n] = anchors over the threshold (total[n] > cap: overflow, results invalid).
 * ws: hn_det_post_ws_bytes(N, cap) bytes of scratch. */
long hn_det_post_ws_bytes(int N, int cap);
int hn_det_postprocess(const float* anchors, const float* regression, const float* classification, int N, int A, int K, int img_h, int img_w,
                       float threshold, float iou_threshold, int cap, void* ws, float* rois, long* class_ids, float* scores, int* kept,
                       int* total, hipStream_t stream);
/* The same pipeline with the suppression rule as an option (DESIGN.md 4z).  nms_kind: 0 hard (the rule above), 1 diou (suppress when
 * IoU - rho^2 / c^2 > iou_threshold: rho = distance of the centres, c = diagonal of the enclosing box), 2 soft_linear, 3 soft_gaussian
 * (Soft-NMS: the highest working score is emitted and decays every other by 1 - IoU when IoU > iou_threshold, or by exp(-IoU^2 / sigma);
 * a box leaves when its score is no longer > score_floor; scores holds the decayed scores, still in descending order).  max_det: at most
 * that many boxes per image (0: no limit; total keeps its meaning).  class_agnostic != 0: no class offset.  nms_kind 0, max_det 0,
 * class_agnostic 0 give hn_det_postprocess's outputs bit for bit.  ws: hn_det_post_ws_bytes_ex(N, cap, nms_kind) bytes of scratch. */
long hn_det_post_ws_bytes_ex(int N, int cap, int nms_kind);
int hn_det_postprocess_ex(const float* anchors, const float* regression, const float* classification, int N, int A, int K, int img_h,
                          int img_w, float threshold, float iou_threshold, int cap, void* ws, float* rois, long* class_ids, float* scores,
                          int* kept, int* total, int nms_kind, float sigma, float score_floor, int max_det, int class_agnostic,
                          hipStream_t stream);

/* Lane decode + lane NMS (LaneHeader.decode, head_lane/lanedetect.py:103-116 = softmax + LaneCodec.decode_lane, lane_codec.py:116-219 +
 * nms_with_pos, lane_codec_utils.py:487-543) for a batch: one workgroup per image.  predict_cls fp32 [N][hw][2] (logits), predict_loc fp32
 * [N][hw][2*ppl+2], hw = (W/stride)*(H/stride) <= 7168 (anchors are walked with a workgroup stride; 1152x1920 has 2160).  Outputs: X [N][hw][ppl] = x of anchor a at line position p (start[a] <= p < end[a]),
 * prob / start / end [N][hw] per anchor, order [N][hw] = candidates in descending-prob order (counts[n] of them), keep [N][hw] = 1 for the
 * candidates that survive. */
int hn_lane_decode_nms(const float* predict_cls, const float* predict_loc, int N, int W, int H, int stride, int ppl, float exist_threshold,
                       float nms_threshold, int use_mean, float margin, float* X, float* prob, int* start, int* end, int* order, int* keep,
                       int* counts, hipStream_t stream);
/* Lane filter by the seg head's marking class (deploy/src/model/hydranet_model.cpp:546-607; hn_lane_filter.hip, DESIGN.md 4n), on
 * hn_lane_decode_nms's device outputs as they are.  Per image: the first top_k (1 .. 64) entries of order[0 .. counts[n]) with keep != 0 are
 * selected (n_sel[n] of them; every other candidate is dropped).  A selected candidate of anchor a has the points (rn(X[n][a][p]), H - 1 -
 * p * interval), start[a] <= p < end[a]: x rounded to nearest, ties to even, clamped to +-16383; fewer than two points or a non-finite x
 * paint nothing.  Its mask is the union of its segments painted with thickness line_width by hn_draw's kind 0 rule (pixel centres within
 * line_width / 2 of the segment, the integer distance test), clipped to the image; area = its pixels, inter = those where mask == lane_class
 * (mask: int64 [N][H][W] arg-max class map of the net input size).  Kept iff (float)inter / (float)area > min_ratio (one fp32 division;
 * 0 / 0 drops).  stats int32 [N][top_k][4] = {position j in order, area, inter, kept} (rows from n_sel[n] on: zero); keep_out int32 [N][hw],
 * hw = (W/stride)*(H/stride): 1 at the positions j of the kept candidates, 0 everywhere else.  All three outputs are written completely.
 * ws: hn_lane_seg_filter_ws_bytes(N, top_k, ppl) bytes (-1: N < 1, top_k outside 1 .. 64 or ppl outside 1 .. 1024).  Returns 1 before any
 * HIP call for a null pointer, top_k or line_width (1 .. 16384) out of range, W or H not a multiple of stride or above 16384, interval < 1
 * or a workspace that is too small.  Three launches, no memset, no allocation, no synchronisation. */
long hn_lane_seg_filter_ws_bytes(int N, int top_k, int ppl);
int hn_lane_seg_filter(const float* X, const int* start, const int* end, const int* order, const int* keep, const int* counts, int N, int W,
                       int H, int stride, int ppl, int interval, const long* mask, int lane_class, int line_width, float min_ratio, int top_k,
                       void* ws, long ws_bytes, int* keep_out, int* stats, int* n_sel, hipStream_t stream);

/* Input pre-processing (demo.py:26-50,186-196; dataset/utility.py:213-227): uint8 BGR frames [N][Hs][Ws][3] -> bilinear resize (cv2.resize
 * INTER_LINEAR fixed-point form for 8-bit images) -> RGB -> (v/255 - mean)/std -> fp32 [N][3][Hd][Wd]. */
int hn_preprocess_bgr(const void* src, int N, int Hs, int Ws, float* dst, int Hd, int Wd, hipStream_t stream);
/* The same resize up to its 8-bit value (cv2.resize of a BGR frame, INTER_LINEAR; preprocess.resize_bgr): a ragged batch of uint8 BGR
 * frames, frame n of desc[n].H x desc[n].W at src + desc[n].off (desc = DEVICE array of N 16-byte records {long off; int H, W}) -> uint8
 * dst [N][Hd][Wd][3].  A frame that has the output size is copied; a record that does not fit [src, src + src_bytes) leaves its frame
 * unwritten.  One launch, no allocation, no synchronisation.  N, Hd <= 65535. */
int hn_resize_bgr8(const void* src, long src_bytes, const void* desc, int N, void* dst, int Hd, int Wd, hipStream_t stream);

/* Segmentation overlay = SegmentHeader.decode (head_seg/segmentation.py:107-125; deploy/src/model/hydranet_model.cpp:758) after the
 * arg-max: mask int64 [N][H][W] -> colour LUT uint8 [ncls][3] (ids without a colour stay black) -> cv2.resize to the frame size (the
 * reference passes cv2.INTER_NEAREST in the `dst` position, so the resize is the default 8-bit INTER_LINEAR) -> cv2.addWeighted(frame,
 * 0.8, colours, 0.5, 0) with float32 arithmetic, round-half-even, saturation.  frames / out: uint8 [N][Ho][Wo][3]. */
int hn_seg_overlay(const long* mask, int N, int H, int W, const void* lut, int ncls, const void* frames, void* out, int Ho, int Wo,
                   hipStream_t stream);

/* Lane F1 (head_lane/lane_metric.py:166-266, used by train.py:188,397,433): the bitwise IoU of lanes drawn as thick polylines.
 * hn_lane_raster paints every segment (p_i, p_{i+1}) of every lane's spline-interpolated polyline with width lane_width into the lane's
 * uint8 mask (cv2.line restated as "pixel centre within lane_width / 2 of the segment": parity with OpenCV's fill rules unpinned);
 * hn_lane_iou counts |mask_g & mask_p| and |mask| for ground-truth lanes g < G and predictions p < P (G, P <= 32) with integer atomics.
 * pts int32 [npts][2]; seg_lane / seg_first int32 [nseg]; masks uint8 [lanes][H][W] zeroed by the caller; inter uint64 [G][P] and area
 * uint64 [G + P] zeroed by the caller. */
int hn_lane_raster(const int* pts, const int* seg_lane, const int* seg_first, int nseg, int lane_width, int H, int W, void* masks,
                   hipStream_t stream);
int hn_lane_iou(const void* masks, int G, int P, long HW, void* inter, void* area, hipStream_t stream);
/* The same counts for a ragged batch of images, from the lanes' float64 points, without a mask in HBM (hn_lane_metric.hip, DESIGN.md 4i):
 * natural cubic spline per lane in float64 (calc_params, every operation rounded once), unit-step samples truncated toward zero, thick
 * lines painted per 64 x 64 tile in LDS (the distance test of hn_lane_raster), integer atomics into the images' tables.
 * pts: DEVICE fp64 [n_points][2] = x, y of every lane's points, lanes back to back.  tab: DEVICE int32, back to back: lane_off
 * [n_lanes + 1] (CSR offsets of the lanes' points), img_lane [N + 1] (CSR offsets of the images' lanes, an image's ground truths first),
 * img_g [N] (ground-truth lanes per image), img_h [N], img_w [N], cnt_off [N] (the image's tables in counts), work [n_work][4] = {image, g0,
 * p0, first tile}: one block of up to 32 x 32 pairs of one image, ceil(H / 64) * ceil(W / 64) tiles each; n_tiles = their sum.  counts: uint64
 * [n_counts], zeroed here: image b holds |g & p| [G][P], |g| [G], |p| [P] at cnt_off[b]; counts[n_counts - 1] is a status word (0, or
 * non-zero when a segment is longer than 1e9 or the batch has more than sample_cap samples: the tables are then incomplete).  ws:
 * hn_lane_metric_ws_bytes(n_lanes, n_points, sample_cap) bytes, 16-byte aligned (-1: sizes out of range).  Two memsets, four launches. */
long hn_lane_metric_ws_bytes(int n_lanes, long n_points, long sample_cap);
int hn_lane_metric_batch(const double* pts, const int* tab, int N, int n_lanes, long n_points, int n_work, long n_tiles, long sample_cap,
                         int lane_width, void* ws, long ws_bytes, void* counts, long n_counts, hipStream_t stream);

/* Streaming confusion counts for the segmentation mIoU (head_seg/seg_metrics.py:12-47): conf uint64 [(C+1)*(C+1)] += counts of
 * (pred, target) pairs, both clamped to C (the ignore bucket): an id above C or below 0 counts there (the reference raises on a
 * negative id).  pred int64 [M]; target int64 or float32 [M] (truncated toward zero).  1 <= C <= 63. */
int hn_seg_confusion(const long* pred, const void* target, int target_is_float, long M, int C, void* conf, hipStream_t stream);

int hn_argmax_channels(const float* logits, int ldl, int C, long M, long* out, hipStream_t stream);

/* HydraTrainer.cal_total_loss (model/train.py:192-203) in one launch: total = sum_g (sum_{i in g} x_i*w_i) * gw_g, left to right in fp32
 * without fused multiply-add (the reference rounds after every mul / add); xs = HOST array of n <= 8 device pointers to fp32 scalars,
 * w [n], gw [number of groups], grp [n] (non-decreasing group id per term) = HOST arrays.  out (optional) = total; grads (optional, needs
 * gout = d loss / d total on the device) [n] = (gout * gw_g) * w_i. */
int hn_weighted_sum(const void* const* xs, const float* w, const float* gw, const int* grp, int n, const float* gout, float* out, float* grads,
                    hipStream_t stream);

/* The same sum under learned homoscedastic-uncertainty weights (train.loss_balance: uncertainty; Kendall, Gal and Cipolla 2018), one
 * launch of one wave, no atomics, no allocation: with s~_i = min(max(s[slot_i], -clamp), clamp) and e_i = expf(-s~_i),
 *   total = [ sum_g ( sum_{i in g, active} (x_i*w_i)*e_i ) * gw_g ] + sum_{i active} s~_i      (term i is active when x_i != 0)
 * in hn_weighted_sum's order, the s~ added last in term order, every operation rounded on its own; at s = 0 total and grads are
 * hn_weighted_sum's bits.  slot (HOST [n], strictly increasing, < n_slots <= 8): the entry of s / ds that term i owns; s (DEVICE fp32
 * [n_slots]) is read at those entries only.  0 < clamp <= 80.  record (DEVICE fp32 [16], always): e_i by term, then 1.0 / 0.0 = term i
 * active, the rest 0.0 -- written by a call with `out`, read by a call without.  With grads (needs gout and ds): grads [n] =
 * ((gout * gw_g) * w_i) * e_i; ds (DEVICE fp32 [2 * n_slots]), every entry written: ds[slot_i] = gout * (1 - t_i * gw_g) for an active
 * term whose s is inside the clamp, or at / outside it when a descent step moves it back inside, else 0.0; ds[n_slots + slot] = 1.0 for
 * the slot of an active term, else 0.0. */
int hn_balanced_sum(const void* const* xs, const float* w, const float* gw, const int* grp, const int* slot, int n, int n_slots,
                    const float* s, float clamp, const float* gout, float* out, float* record, float* grads, float* ds, hipStream_t stream);

/* Before / after the Adam step of the log-variances: hold (DEVICE fp32 [3 * n]) takes s, m, v (act == NULL), or gives them back to every
 * slot i with !(act[i] > 0) (act: DEVICE fp32 [n], hn_balanced_sum's activity or its mean over accumulated micro-batches), so that an
 * inactive or untrained slot keeps its value and both moments to the bit.  n <= 8. */
int hn_balance_hold(float* s, float* m, float* v, float* hold, const float* act, int n, hipStream_t stream);

/* Adam step of all parameters in one launch (torch.optim.Adam as model/train.py:147 constructs it: L2 weight decay on the gradient, bias
 * correction, eps outside the square root; not amsgrad).  jobs (DEVICE) = n x 6 int64 {p, g, m, v (fp32 pointers), numel, first_block};
 * a block = 256 threads x 4 consecutive elements of one tensor; block_job (DEVICE int32 [total_blocks]) = job index of every block;
 * step = 1-based iteration count (bias corrections are computed on the host in double). */
int hn_adam_step(const long* jobs, const int* block_job, long total_blocks, double lr, double beta1, double beta2, double eps,
                 double weight_decay, long step, hipStream_t stream);

/* Global gradient norm, clipping coefficient and a non-finite step guard, decided on the device (no host synchronisation, no allocation,
 * graph-capturable; three launches, none of whose workgroups waits on another).  jobs / block_job / total_blocks are hn_adam_step's tables
 * (n_jobs rows; only g, numel and first_block are read).  record (DEVICE, 32 bytes, zeroed once by the caller):
 *   word 0 float norm = (float)sqrt(total)       word 1 float coef       word 2 int skip (bit mask)       word 3 int steps
 *   word 4 int skipped       word 5 int skipped_consecutive       words 6-7 pad
 * Reduction order: a thread adds the squares of its 4 elements left to right in fp32 (products rounded, no fused multiply-add; the same
 * instruction stream for 16-byte vector loads and element loads); a block's value is a fixed tree over its 256 thread values (DPP inside
 * each wave, then (w0 + w1) + (w2 + w3) through LDS); a job's sum is formed in double by one workgroup (thread t adds blocks t, t + 256,
 * ... in ascending order, then a fixed 256-leaf tree), and the total over the jobs the same way.  The order depends on the job table
 * alone: no floating-point atomics, no dependence on which workgroup finishes first.
 * coef = min(1.0f, (float)max_norm / (norm + 1e-6f)) in rounded fp32 operations (torch.nn.utils.clip_grad_norm_; a NaN stays a NaN as under
 * torch.clamp); exactly 1.0f when max_norm <= 0.
 * skip: bit 1 = the total is not finite or exceeds fp32's range, bit 2 = one of `losses` is not finite (both only when flags & 1; without
 * it a non-finite norm just flows through the formula, as in torch), bit 4 = one of `words` is non-zero (always).  steps += 1 on every
 * call; skip != 0: skipped += 1, skipped_consecutive += 1; else skipped_consecutive = 0.
 * losses: HOST array of n_losses <= 8 DEVICE fp32 scalars; words: HOST array of n_words <= 4 DEVICE int32 words (both read at launch
 * time into the kernel's arguments); ws: DEVICE, 16-byte aligned, >= hn_grad_guard_ws_bytes(total_blocks, n_jobs) bytes; job_sq (optional,
 * DEVICE double [n_jobs]) receives the per-job sums of squares.  Writes go to ws, job_sq and record only.
 * hn_grad_guard_ws_bytes: -1 unless 1 <= n_jobs <= total_blocks <= 2^31 - 1. */
long hn_grad_guard_ws_bytes(long total_blocks, long n_jobs);
int hn_grad_guard(const long* jobs, const int* block_job, long total_blocks, long n_jobs, double max_norm, int flags,
                  const void* const* losses, int n_losses, const void* const* words, int n_words, void* ws, long ws_bytes, double* job_sq,
                  void* record, hipStream_t stream);

/* hn_adam_step that obeys `record` (written by hn_grad_guard earlier on the same stream): every thread reads it first; skip != 0: the
 * kernel returns before its first store (p, m, v untouched bit for bit); otherwise the gradient is multiplied by coef (rounded) before the
 * weight-decay term, which is clipping in place and then stepping -- but the gradient tensors are not written.  coef == 1.0f gives
 * hn_adam_step's result bit for bit (one shared kernel body). */
int hn_adam_step_guarded(const long* jobs, const int* block_job, long total_blocks, double lr, double beta1, double beta2, double eps,
                         double weight_decay, long step, const void* record, hipStream_t stream);

/* hn_adam_step (record == NULL) or hn_adam_step_guarded (record = hn_grad_guard's) that also keeps an exponential moving average of every
 * parameter, in the same launch and the same kernel body: p, m and v come out bit-identical to those entry points.  jobs / block_job /
 * total_blocks are hn_adam_step's tables, unchanged; ema (DEVICE long [n_jobs]) = one fp32 pointer per job, numel elements each, not
 * overlapping p, g, m or v.  With the new parameter value p' in its register, e' = e + w * (p' - e), w = (float)(1.0 - ema_decay) formed
 * in double on the host and rounded once; subtraction, product and sum are each rounded (no fused multiply-add), and whole aligned float4s
 * (p, g, m, v and e all 16-byte aligned) and single elements go through one instruction stream.  A skipped step (record->skip != 0) returns
 * before any store: e stays untouched too.  HN_ERR "bad argument" unless 0 <= ema_decay < 1 (a NaN fails) and ema is non-NULL.  Plain
 * vector loads and stores only; no workgroup waits on another, nothing is allocated or synchronised: graph-capturable. */
int hn_adam_step_ema(const long* jobs, const int* block_job, long total_blocks, const long* ema, double lr, double beta1, double beta2,
                     double eps, double weight_decay, long step, double ema_decay, const void* record, hipStream_t stream);

/* Many contiguous tensors copied in one launch (the gather of a gradient bucket before its all-reduce, train.py:130-137's DDP buckets):
 * jobs (DEVICE) = n x 4 int64 {src, dst, numel, first_block}, block = 256 threads x 4 elements, block_job (DEVICE int32) = job of every
 * block; kind 0: fp32 -> fp32, 1: fp32 -> bf16 (reduced-precision payload), 2: bf16 -> fp32. */
int hn_copy_many(const long* jobs, const int* block_job, long total_blocks, int kind, hipStream_t stream);

/* Many pairs of contiguous fp32 tensors exchanged in one launch: jobs / block_job in hn_copy_many's layout, n x 4 int64 {a, b, numel,
 * first_block}; afterwards a holds what b held and b what a held.  32-bit words are moved, not floats (NaN payloads and -0 survive), 16
 * bytes at a time where both pointers allow.  a and b of one job must NOT overlap, and no tensor may appear in two jobs.  Plain vector
 * loads and stores; no workgroup waits on another, nothing is allocated or synchronised: graph-capturable. */
int hn_swap_many(const long* jobs, const int* block_job, long total_blocks, hipStream_t stream);

/* State a training step writes outside the optimizer (BatchNorm running statistics and their batch counters), kept in step with
 * hn_grad_guard's decision and averaged next to the weights; one launch over many small tensors (hn_state.hip).  jobs (DEVICE) = n x 6
 * int64 {live, shadow, avg, words, first_block, kind}: `words` counts 32-bit words (an fp32 statistic of C channels: C; an int64 counter:
 * 2), a block = 256 threads x 4 consecutive words of one job, block_job (DEVICE int32) = job of every block (hn_copy_many's idiom);
 * kind 0: fp32 values, kind 1: raw words, never read as floats; a shadow / avg pointer of 0: the job has none and is not touched for it.
 * live, shadow and avg of a job do not overlap, and no tensor appears in two jobs.
 *   mode 0, snapshot: shadow = live for every job that has a shadow; record and ema_decay are ignored.
 *   mode 1, settle: record = hn_grad_guard's 32-byte record, written earlier on the same stream, or NULL = "not skipped"; every thread
 *     reads skip first.  skip != 0: live = shadow for every job that has a shadow, and nothing else is written (averages stay untouched,
 *     as hn_adam_step_ema leaves e); skip == 0: nothing is written.
 *   mode 2, settle and average: as mode 1 when skipped; otherwise, for every job that has an average, kind 0: avg' = avg + w * (live -
 *     avg), w = (float)(1.0 - ema_decay) formed in double on the host and rounded once, subtraction, product and sum each rounded (no fused
 *     multiply-add; hn_adam_step_ema's formulation), aligned float4s and single elements through one instruction stream; kind 1: avg =
 *     live (the average of a counter is the counter).
 * Snapshots and restores move 32-bit words (NaN payloads, -0 and denormals survive), 16 bytes at a time where both pointers allow.
 * HN_ERR "bad argument", before any HIP call: NULL jobs / block_job, total_blocks outside 1 .. 2^31 - 1, mode outside {0, 1, 2}, and in
 * mode 2 ema_decay outside [0, 1) (a NaN fails).  Plain vector loads and stores only; no workgroup waits on another, nothing is allocated
 * or synchronised: graph-capturable. */
int hn_state_guard(const long* jobs, const int* block_job, long total_blocks, int mode, const void* record, double ema_decay,
                   hipStream_t stream);

/* Gradient accumulation over several backward passes: the running mean of a group's micro-batch gradients, one launch per micro-batch
 * over all gradient tensors (hn_accum.hip).  jobs (DEVICE) = n x 4 int64 {g, acc, numel, first_block} in hn_copy_many's layout (fp32
 * pointers; a block = 256 threads x 4 consecutive elements of one tensor; block_job (DEVICE int32) = job of every block); g and acc of a
 * job do not overlap and no tensor appears in two jobs.  j = 1-based index of this micro-batch within its group:
 *   j == 1: acc = g, moved as 32-bit words (NaN payloads, -0 and denormals survive); acc is NOT read.
 *   j  > 1: acc' = acc + w * (g - acc), w = (float)(1.0 / j) formed in double on the host and rounded once; subtraction, product and sum
 *           are each rounded (no fused multiply-add; hn_adam_step_ema's formulation).
 * After every call acc holds the mean of the micro-batches seen so far.  Whole float4s where g and acc are both 16-byte aligned, single
 * elements otherwise, through one instruction stream: the bits do not depend on alignment.  g is only read.  A NaN or Inf of any
 * micro-batch leaves a non-finite value in acc at that element.
 * One thread of block 0, with plain stores: loss_mean[i] (DEVICE float [n_losses]) follows the same rule over losses (HOST array of
 * n_losses <= 8 DEVICE fp32 scalars, read at launch time into the kernel's arguments, as hn_grad_guard takes them); sticky (DEVICE int32)
 * = bits when j == 1, else sticky | bits, where bits = 2 if any of losses is not finite, | 4 if any of words (HOST array of n_words <= 4
 * DEVICE int32 words) is non-zero -- the word to hand to hn_grad_guard's `words` at the group's end.  n_losses == 0 and n_words == 0 are
 * allowed; loss_mean (n_losses == 0) and sticky (both counts 0) may then be NULL; a non-NULL sticky is written even then.
 * HN_ERR "bad argument", before any HIP call: NULL jobs / block_job, total_blocks outside 1 .. 2^31 - 1, j < 1, n_losses outside 0 .. 8,
 * n_words outside 0 .. 4, NULL losses / loss_mean with n_losses > 0, NULL words with n_words > 0, NULL sticky with either count > 0, a
 * NULL entry of losses / words.  Plain vector loads and stores only; no atomics, no workgroup waits on another, nothing is allocated
 * or synchronised: graph-capturable (j is baked into a captured launch). */
int hn_grad_accum(const long* jobs, const int* block_job, long total_blocks, long j, const void* const* losses, int n_losses,
                  float* loss_mean, const void* const* words, int n_words, int* sticky, hipStream_t stream);

/* Full-state training checkpoints: many tensors gathered into a staging buffer with a checksum per tensor, verified, and scattered back
 * in place (hn_ckpt.hip; checkpoint.StatePacker).  jobs (DEVICE) = n_jobs x 4 int64 {src, dst, words, first_block} in hn_copy_many's
 * layout: `words` counts 32-bit words (an int64 counter is two), a block = 256 threads x 4 consecutive words of one job, block_job
 * (DEVICE int32 [total_blocks]) = job of every block.  Words are moved, never floats: NaN payloads, -0 and denormals survive.  Whole
 * 16-byte vectors where a pointer allows and single words otherwise, into the same registers: the bits do not depend on alignment.
 * src and dst of a job do not overlap, and no dst appears in two jobs.
 * Checksum of a job with words w[0 .. W-1], each a uint32 zero-extended to 64 bits:
 *     s1 = sum of w[i] mod 2^64          s2 = sum of (i + 1) * w[i] mod 2^64
 * Integer arithmetic: the value does not depend on the order of the additions.  Formed without atomics: one {s1, s2} partial per block in
 * ws (DEVICE, 8-byte aligned, total_blocks * 16 bytes; every block writes its own, so nothing is zeroed by the caller), folded per job by
 * a second launch of n_jobs workgroups.  sums / expect: DEVICE uint64 [n_jobs][2] = {s1, s2}, 8-byte aligned.
 *   hn_state_pack:   dst = src for every job; sums receives the checksums of the words read.  src is only read.
 *   hn_state_verify: no copy; the checksums of the src column go to sums and are compared with expect.  verdict (DEVICE int32 [4]) =
 *     {number of jobs that differ, index of the first such job or -1, 0, 0}, written in full by every call (a third launch of one
 *     workgroup): the caller zeroes nothing.
 *   hn_state_unpack: dst = src for every job -- unless verdict (hn_state_verify's, written earlier on the same stream) is non-NULL and
 *     verdict[0] != 0: every thread reads it first and returns before its first store, so every dst keeps its bits.
 *   hn_state_checksum_host: the same {s1, s2} of n_words words of HOST memory (4-byte aligned) into out[2]; a host function, no GPU call.
 * HN_ERR "bad argument", before any HIP call: NULL jobs / block_job, total_blocks or n_jobs outside 1 .. 2^31 - 1, a NULL or misaligned
 * ws / sums / expect, a NULL verdict for hn_state_verify; for hn_state_checksum_host n_words < 0, NULL out, NULL words with n_words > 0.
 * Plain vector loads and stores only; no atomics, no workgroup waits on another, nothing is allocated or synchronised: graph-capturable. */
int hn_state_pack(const long* jobs, const int* block_job, long total_blocks, long n_jobs, void* ws, void* sums, hipStream_t stream);
int hn_state_verify(const long* jobs, const int* block_job, long total_blocks, long n_jobs, const void* expect, void* ws, void* sums,
                    int* verdict, hipStream_t stream);
int hn_state_unpack(const long* jobs, const int* block_job, long total_blocks, const int* verdict, hipStream_t stream);
int hn_state_checksum_host(const void* words, long n_words, unsigned long long* out);

/* COCO box mAP (pycocotools COCOeval(..., 'bbox') evaluate + accumulate; hn_coco.hip, parity rules in its header comment).
 * hn_coco_match: one workgroup per (image, category) cell.  cells (DEVICE int32 [n_cells][4]) = {gt cell = image order * K + category,
 * first detection, detection count, first output record}; dets fp64 [n][5] = x, y, w, h, score (an fp32 value); gt_off int32
 * [images * K + 1] = CSR offsets of gt fp64 [G][5] = x, y, w, h, area (annotation order per cell); prm fp64 = T IoU thresholds
 * (min(iouThr, 1 - 1e-10)) then the 4 area ranges [4][2]; T <= 16; gtm_ws: hn_coco_match_ws_bytes(G) bytes (matched flags of cells with
 * more than 256 GTs).  Writes min(count, 100) records of 8 int32 per cell: {score fp32 bits, image order * 128 + rank, category, 0,
 * per area range (matched bits 0..T-1 | ignored bits 16..16+T-1)}.
 * hn_coco_accumulate: rec [N][8] (N < 2^31), iprm (DEVICE int32) = category starts [K + 1] of the records in category order, npig [K][4],
 * maxDets [M]; rec_thrs fp64 [R <= 128]; seq_bits >= bit length of the largest record sequence; ws: hn_coco_accumulate_ws_bytes(N).
 * precision fp64 [T][R][K][4][M], recall [T][K][4][M] (-1 where npig == 0). */
long hn_coco_match_ws_bytes(long n_gt);
int hn_coco_match(const int* cells, int n_cells, const double* dets, const int* gt_off, const double* gt, const double* prm, int K, int T,
                  void* gtm_ws, int* rec, hipStream_t stream);
long hn_coco_accumulate_ws_bytes(long N);
int hn_coco_accumulate(const int* rec, long N, int K, int seq_bits, const int* iprm, const double* rec_thrs, int T, int R, int M, void* ws,
                       double* precision, double* recall, hipStream_t stream);

/* Lane ground-truth encoding (head_lane/lane_codec.py LaneCodec.encode_lane + dataset/dataloader.py:343-352's scale-invariance division;
 * hn_lane_encode.hip, parity rules in its header comment and DESIGN.md 4e).  pts (DEVICE fp64 [n_points][2] = x, y) = every lane's points
 * scaled to the W x H input, deduplicated on y, y descending (>= 2 per lane); lane_off int32 [n_lanes + 1] = CSR offsets of the lanes' points;
 * img_lane int32 [N + 1] = CSR offsets of every image's lanes (annotation order).  Geometry: anchor grid fw x fh = int(W / stride) x
 * int(H / stride), F = fw * fh, P points per line, interval = H / P; div_interval = the dataset's divisor for columns [0, P) and
 * [P + 2, 2P + 2) when scale_invariance.  Writes gt_cls fp32 [N][F][2] and gt_loc fp32 [N][F][2P + 2] completely (background rows
 * included).  ws: hn_lane_encode_ws_bytes(n_lanes, n_points, W, H, stride, P) bytes.  Two launches. */
long hn_lane_encode_ws_bytes(int n_lanes, long n_points, int W, int H, int stride, int P);
int hn_lane_encode(const double* pts, const int* lane_off, const int* img_lane, int N, int n_lanes, long n_points, int W, int H, int stride,
                   int P, int interpolate, int scale_invariance, float div_interval, void* ws, float* gt_cls, float* gt_loc, hipStream_t stream);

/* Training-batch augmentation (augment.py; hn_augment.hip, semantics in augment.py's docstring and DESIGN.md 4f).  src: uint8 BGR source
 * frames packed back to back (ragged: every image's byte offset, Hs, Ws in its descriptor); desc: DEVICE array of N 176-byte AugDesc
 * (F^-1, photometric op + parameters, noise key, blur weights, offsets; layout in hn_augment.hip and augment.py DESC_DTYPE).
 * hn_augment_photometric writes the photometric result of every image with ws_off >= 0 into ws at that offset (Hs * Ws * 3 bytes each);
 * the grid covers max_hs x max_ws.  hn_augment_image: warp + INTER_AREA resize + BGR->RGB + ImageNet normalisation -> fp32 [N][3][Hd][Wd]
 * (it samples ws for images with ws_off >= 0, src otherwise).  hn_augment_seg: uint8 label maps (packed, seg_off) -> uint8 [N][Hd][Wd]. */
int hn_augment_photometric(const void* src, const void* desc, int N, int max_hs, int max_ws, void* ws, hipStream_t stream);
int hn_augment_image(const void* src, const void* ws, const void* desc, int N, int Hd, int Wd, float* dst, hipStream_t stream);
int hn_augment_seg(const void* seg, const void* desc, int N, int Hd, int Wd, void* dst, hipStream_t stream);

/* Baseline JPEG decode, entropy stage on the host and the rest on the device (jpeg.py; hn_jpeg.hip, semantics in DESIGN.md 4g).
 * Supported: 8-bit Huffman SOF0 / SOF1, one interleaved scan, 1 component or YCbCr with luma 1x1 / 2x1 / 2x2 and chroma 1x1, restart
 * intervals.  hn_jpeg_parse and hn_jpeg_entropy_decode are HOST functions (no HIP runtime call, no allocation; they run without a GPU):
 * status 3 = outside the supported set, 1 = not a well-formed JPEG (or a corrupt / truncated scan).  head: a 432-byte JpegHead record
 * (width, height, components, sampling, MCU counts, restart interval, coef_bytes, quantisation tables in natural order; layout in
 * hn_jpeg.hip and jpeg.py HEAD_DTYPE).  hn_jpeg_entropy_decode writes head.coef_bytes bytes of quantised int16 coefficients into the
 * caller's buffer: one de-zigzagged 64-entry block per 8x8 block, component plane after component plane, blocks in raster order of the
 * plane padded to whole MCUs; no read leaves [data, data + len) and no write leaves [coefs, coefs + coef_bytes). */
int hn_jpeg_parse(const void* data, long len, void* head);
int hn_jpeg_entropy_decode(const void* data, long len, const void* head, void* coefs, long coef_bytes);
/* Device stage for a ragged batch: desc = DEVICE array of N 440-byte JpegDesc (offsets into coefs / planes / dst, geometry, quantisation
 * tables).  Dequantise + libjpeg's accurate integer IDCT into uint8 sample planes (planes: scratch, 64 bytes per block, 16-byte aligned,
 * as coefs), then libjpeg's fancy chroma up-sampling + YCbCr -> BGR uint8 H x W x 3 at dst + dst_off (augment.pack's frame layout).
 * max_blocks / max_h / max_w: the largest block count / height / width of the batch (grid extents).  The three byte counts bound every
 * access: an image whose descriptor does not fit them is left unwritten.  Two launches, no allocation, no synchronisation. */
int hn_jpeg_decode(const void* coefs, long coef_bytes, const void* desc, int N, long max_blocks, int max_h, int max_w, void* planes,
                   long plane_bytes, void* dst, long dst_bytes, hipStream_t stream);
/* The entropy stage on the device instead (jpeg.entropy_decode_device; hn_jpeg_scan.hip, semantics in DESIGN.md 4g).
 * hn_jpeg_scan_prepare is a HOST function (no HIP runtime call, no allocation), statuses as hn_jpeg_parse, 1 also for a head that is not
 * this stream's: it fills an 8576-byte JpegScanRec (layout in hn_jpeg_scan.h and jpeg.py SCAN_DTYPE) with the scan's offset and length,
 * the geometry and the Huffman tables its components select; the caller adds stream_off / coef_off (multiples of 16) when it packs a batch.
 * hn_jpeg_scan_decode: streams = the batch's files at their stream_off (stream_bytes a multiple of 4), desc = DEVICE array of N records
 * -> coefs, exactly what hn_jpeg_entropy_decode writes for each image at its coef_off, and status: N int32, 0 or 1 (a corrupt or truncated
 * scan, or a record that does not fit the buffers; that image's coefficients are then undefined, but inside its slot).  coefs
 * [0, coef_bytes) is zeroed first.  Self-synchronising parallel Huffman decoding over subsequences of hn_jpeg_scan_subseq_bytes() raw bytes;
 * max_scan_bytes / max_blocks: the batch's largest scan length and block count (grid extents and the workspace, hn_jpeg_scan_ws_bytes, -1
 * for arguments out of range; ws 16-byte aligned).  Two memsets and three launches, no allocation, no synchronisation. */
int hn_jpeg_scan_prepare(const void* data, long len, const void* head, void* rec);
long hn_jpeg_scan_ws_bytes(int N, long max_scan_bytes, long max_blocks);
int hn_jpeg_scan_subseq_bytes(void);
int hn_jpeg_scan_decode(const void* streams, long stream_bytes, const void* desc, int N, long max_scan_bytes, long max_blocks, void* ws,
                        long ws_bytes, void* coefs, long coef_bytes, void* status, hipStream_t stream);

/* PNG label decode on the device (png.py; hn_png.hip, semantics in DESIGN.md 4j): inflate (RFC 1950 / 1951: stored, fixed and dynamic
 * blocks) and the five PNG row filters.  data = the batch's zlib streams (every image's IDAT payloads concatenated; data_bytes a multiple
 * of 4, data 16-byte aligned); desc = DEVICE array of N 48-byte PngDesc {long idat_off (a multiple of 4), idat_len; long raw_off (into ws, a
 * multiple of 16: H (1 + W bpp) bytes of filtered scanlines, rounded up to 16); long out_off (into out: H W bytes); int W, H, bpp (1 or 3),
 * pad} (png.py DESC_DTYPE).  out + out_off receives channel 0 of every pixel, H x W uint8 (what dataset.imread_label returns).  max_idat_bytes
 * / max_raw_bytes: the batch's largest stream and largest raw size (< 2^28 / < 2^30).  ws: hn_png_ws_bytes (-1 for arguments out of
 * range) bytes, 16-byte aligned: the raw regions live in its first N * round16(max_raw_bytes) bytes, the library's own scratch behind them.
 * status: N int32, written for every image:
 *   0 decoded                        1 reserved block type             2 stored block LEN / NLEN mismatch
 *   3 code lengths over-subscribed, incomplete, too many, a repeat out of range or no end-of-block code
 *   4 invalid litlen / distance symbol     5 distance reaches before the start of the output      6 input exhausted
 *   7 more or fewer raw bytes than H (1 + W bpp)     8 filter byte > 4     9 Adler-32 mismatch     10 bad zlib header (CMF / FLG)
 *   11 the record does not fit the buffers (nothing written)
 * A rejected image leaves its out region in any state; nothing outside an image's own ws / out regions (and the library's scratch in ws)
 * is written.  Three launches, no allocation, no synchronisation. */
long hn_png_ws_bytes(int N, long max_idat_bytes, long max_raw_bytes);
int hn_png_decode(const void* data, long data_bytes, const void* desc, int N, long max_idat_bytes, long max_raw_bytes, void* ws,
                  long ws_bytes, void* out, long out_bytes, void* status, hipStream_t stream);

/* PNG label encode on the device, the mirror image (png_encode.py; hn_png_enc.hip, semantics in DESIGN.md 4l): class maps -> per image a
 * complete zlib stream (header 78 01, fixed-Huffman deflate blocks of hn_png_enc_chunk_bytes() raw bytes each, big-endian Adler-32) of the
 * filtered scanlines of the map resized to (Ho, Wo) with cv2's INTER_NEAREST index rule: the payload of a PNG file's IDAT chunk (bit
 * depth 8, one byte per pixel).  src = int64 class ids (src_is_int64 = 1; 8-byte aligned) or uint8 maps (0), src_elems elements; desc =
 * DEVICE array of N 64-byte PngEncDesc {long src_off (elements); long raw_off (into ws, a multiple of 16: Ho (1 + Wo) bytes of filtered
 * scanlines, rounded up to 16); long out_off (into out, a multiple of 4), out_cap (bytes the stream may use, a multiple of 4); int Hs, Ws,
 * Ho, Wo (1..65535); long pad[2]} (png_encode.py DESC_DTYPE).  result = DEVICE array of N 16-byte records {long stream_bytes; int status,
 * pad}, written for every image:
 *   0 encoded      1 an int64 value outside 0..255 among the values the resize samples      2 the stream is longer than out_cap
 *   3 the record does not fit the buffers
 * An image with a non-zero status has stream_bytes 0 and nothing written to out; no write ever lands at or past an image's out_cap, or
 * outside [ws, ws + hn_png_enc_ws_bytes(...)).  hn_png_enc_cap_bytes(raw): a capacity no stream of `raw` filtered bytes exceeds, 2 +
 * ceil((9 raw + 10 ceil(raw / chunk)) / 8) + 4 rounded up to 16 (-1 out of range).  max_out_h / max_raw_bytes: the batch's largest Ho and
 * Ho (1 + Wo) (< 2^30); they size the grids and the workspace (hn_png_enc_ws_bytes, -1 for arguments out of range; 16-byte aligned, the
 * raw regions in its first N * round16(max_raw_bytes) bytes; it needs no clearing).  One memset of N words and four launches, no
 * allocation, no synchronisation; no workgroup waits on another. */
int hn_png_enc_chunk_bytes(void);
long hn_png_enc_cap_bytes(long raw_bytes);
long hn_png_enc_ws_bytes(int N, long max_raw_bytes);
int hn_png_encode(const void* src, long src_elems, int src_is_int64, const void* desc, int N, int max_out_h, long max_raw_bytes, void* ws,
                  long ws_bytes, void* out, long out_bytes, void* result, hipStream_t stream);

/* The same encode with dynamic-Huffman deflate blocks (png_encode.py huffman="dynamic"; restated in tests/png_enc_dyn_ref.py): arguments,
 * descriptors, result records and status codes are hn_png_encode's.  The stream: 78 01, then ONE deflate block for every
 * hn_png_enc_block_chunks() (16) chunks of hn_png_enc_chunk_bytes() raw bytes -- the last block holds the remaining 1..16 chunks and
 * carries BFINAL -- then the big-endian Adler-32.  The token parse is per chunk, as in hn_png_encode.  Every block is written with the
 * smaller of two codes: a literal/length Huffman code built from the block's own tokens (at most 15 bits; the header's code-length code at
 * most 7) with a two-entry distance code (distance 1 and the row distance Wo + 1, one bit each), or the fixed code when the dynamic
 * block, its header included, is not strictly smaller.  So a stream is never longer than hn_png_encode's, and hn_png_enc_cap_bytes bounds
 * it.  The workspace is larger (hn_png_enc_dyn_ws_bytes, -1 for arguments out of range): hn_png_encode's layout, then 292 words per chunk
 * and 440 per block.  One memset of N words and five launches (filter, per-chunk counts, per-block code, scan, emit), no allocation, no
 * synchronisation; no workgroup waits on another; integer atomics and OR into zeroed words only, so the bytes are deterministic.  A
 * non-zero status leaves stream_bytes 0 and nothing written to out; no write lands at or past an image's out_cap or outside the
 * workspace. */
int hn_png_enc_block_chunks(void);
long hn_png_enc_dyn_ws_bytes(int N, long max_raw_bytes);
int hn_png_encode_dyn(const void* src, long src_elems, int src_is_int64, const void* desc, int N, int max_out_h, long max_raw_bytes, void* ws,
                      long ws_bytes, void* out, long out_bytes, void* result, hipStream_t stream);

/* Baseline JPEG encode, the mirror image (jpeg_encode.py; hn_jpeg_enc.hip, semantics in DESIGN.md 4h): libjpeg's default compressor, all
 * integer.  Device stage for a ragged batch: desc = DEVICE array of N 432-byte JpegEncDesc (offsets into frames / coefs, geometry,
 * quantisation tables in natural order).  frames: packed BGR uint8 H x W x 3 frames (augment.pack's layout; a 1-component image encodes
 * channel 0); coefs: quantised int16 coefficients in hn_jpeg_entropy_decode's layout, blocks that only fill an MCU written as zeros.
 * max_mcus_y / max_wpad: the largest MCU-row count and MCU-padded width of the batch (grid extents).  Both pointers 16-byte aligned.  The
 * two byte counts bound every access: an image whose descriptor does not fit them is left unwritten.  One launch, no allocation, no
 * synchronisation. */
int hn_jpeg_encode(const void* frames, long frames_bytes, const void* desc, int N, int max_mcus_y, int max_wpad, void* coefs,
                   long coef_bytes, hipStream_t stream);
/* HOST function (no HIP runtime call, no allocation): coefficients + a 432-byte JpegHead record (restart_interval 0, 8-bit tables,
 * qt[1] == qt[2]) -> a complete JFIF stream (SOI, APP0, DQT, SOF0, DHT with the Annex K tables, one interleaved SOS, EOI) in out.  Returns
 * the stream's length; -4 when `capacity` is too small (nothing is written at or past out + capacity: call again with a larger buffer);
 * -1 for a bad argument or a coefficient no baseline table can code.  The blocks that only fill an MCU are synthesised (AC zero, DC of
 * the preceding block), whatever the buffer holds there. */
long hn_jpeg_entropy_encode(const void* coefs, long coef_bytes, const void* head, void* out, long capacity);
/* HOST function (no HIP runtime call, no allocation): exactly the bytes hn_jpeg_entropy_encode writes before the first scan bit (SOI, APP0,
 * DQT, SOF0, four DHT -- two for a 1-component image -- and SOS) for the same 432-byte JpegHead record.  Returns their count; -4 when
 * `capacity` is too small (nothing is written at or past out + capacity); -1 for a bad argument. */
long hn_jpeg_write_header(const void* head, void* out, long capacity);
/* The entropy stage on the device (jpeg_encode.entropy_encode_device; hn_jpeg_huff.hip, semantics in DESIGN.md 4h): coefs in the layout
 * hn_jpeg_encode writes -> every image's byte-stuffed scan, the last byte padded with one-bits, bit for bit what hn_jpeg_entropy_encode
 * writes between its header and its EOI (neither of which is written here).  desc = DEVICE array of N 56-byte JpegHuffDesc {long coef_off
 * (multiple of 16), out_off, out_cap; int W, H, ncomp, hs, vs, mcus_x, mcus_y, pad}: the image's scan goes to out + out_off and may use
 * out_cap bytes.  result = DEVICE array of N 16-byte records {long scan_bytes; int status, pad}: status 0 and the scan's length; -4 when
 * the stuffed scan is longer than out_cap; -1 for a descriptor that does not fit coef_bytes / out_bytes / max_blocks / max_cap or a
 * coefficient no baseline table can code (a DC difference of more than 11 bits, an AC value of more than 10: what the host stage refuses).
 * An image with a non-zero status has scan_bytes 0 and nothing written to out; no write ever lands at or past its out_cap, or outside
 * [ws, ws + hn_jpeg_huff_ws_bytes(...)).  The blocks that only fill an MCU are not read.  max_blocks / max_cap: the largest block count
 * (coefficient bytes / 128) and capacity of the batch; they size the grids and the workspace, whose size hn_jpeg_huff_ws_bytes returns
 * (-1 for arguments out of range).  ws needs no clearing, before the first call or between calls.  coefs and ws 16-byte aligned, result
 * 8-byte.  Six launches, no allocation, no synchronisation, no memset; no workgroup waits on another. */
long hn_jpeg_huff_ws_bytes(int N, long max_blocks, long max_cap);
int hn_jpeg_huff_encode(const void* coefs, long coef_bytes, const void* desc, int N, long max_blocks, long max_cap, void* ws, long ws_bytes,
                        void* out, long out_bytes, void* result, hipStream_t stream);

/* Drawing on packed BGR frames, in place (draw.py; hn_draw.hip): imgs = DEVICE array of N 24-byte DrawImage (frame offset, W, H, its range
 * of the primitive list), prims = DEVICE array of 32-byte DrawPrim (kind 0 thick segment / 1 filled rectangle / 2 glyph bitmap, colour).  A
 * pixel takes the colour of the LAST primitive of its image's range that covers it.  Coordinates within +-16384.  frames_bytes / nprims
 * bound every access: an image whose record does not fit them is left untouched.  One launch, no allocation, no synchronisation. */
int hn_draw(void* frames, long frames_bytes, const void* imgs, int N, int max_h, int max_w, const void* prims, int nprims,
            hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
