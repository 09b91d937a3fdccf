/*
 * vlp_hip.h — C ABI of libvlp_hip.so, the MI355X (gfx950) implementation of the
 * CLIP-style contrastive pretraining step of
 * schusterbenjamin/Vision-Language-Pretraining-for-Bone-Tumor-Detection.
 *
 * The reference is pure Python: its hot path is VisionLanguageModule
 * (src/models/pretrain/VisionLanguageModule.py) whose arithmetic is delegated to
 * timm resnet34 (:30-35), HF BertModel/TinyBERT (:38-60), the head in forward
 * (:441-461), _compute_loss (:532-554) and torch.optim.AdamW (:130-184).  Each
 * entry point below replaces one of the device operations those calls dispatch
 * to; the Python host layer (vlp_amd/, src/models/pretrain/VisionLanguageModule.py
 * in this package) binds them with ctypes exactly as INTEGRATION.md shows.
 *
 * Conventions
 *  - All tensor arguments are DEVICE pointers (caller-allocated, e.g. by the
 *    PyTorch caching allocator); `stream` is a hipStream_t passed as void*.
 *    Every call only enqueues work on `stream`; none synchronises.
 *  - `dtype`: 0 = fp32 (parity mode), 1 = bf16 (throughput mode) storage of
 *    activations/gradients.  Weight gradients, BN statistics, and optimizer
 *    state are always fp32 (fp64 for BN sums).
 *  - Activations are NHWC ([N][H][W][C], C innermost); token hidden states are
 *    row-major [B*T][D].
 *  - Return value: 0 on success, otherwise a hipError_t code.
 *  - Stateless and re-entrant; "accumulate" outputs require the caller to zero
 *    them first (documented per call).
 */
#ifndef VLP_HIP_H
#define VLP_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* 3 since r5 (r4's 2 plus role_w on vlp_clip_loss_fused / vlp_ce_sym; the dy^T
 * operands of vlp_conv_wgrad / vlp_stem_wgrad / vlp_bn_bwd_apply removed); the
 * Python binding refuses any other value. */
int vlp_abi_version(void);
/* Diagnostic: register-only v_mfma_f32_16x16x32_bf16 chains (8 independent
 * accumulators per wave, 4 waves per block) to measure the card's dense bf16
 * MFMA ceiling next to the vendor figure.
 * FLOP = blocks * 4 * iters * 8 * 16384; out: blocks * 256 floats. */
int vlp_mfma_peak_probe(int blocks, int iters, float* out, void* stream);
/* Diagnostic: an empty kernel dispatch (end = 0: begin marker, 1: end marker)
 * that brackets bench.py's isolated roofline pass in a rocprofv3 kernel trace
 * (tools/roofline_window.py).  No reference counterpart. */
int vlp_trace_marker(int end, void* stream);

/* ---------------- image tower: convolutions ----------------
 * Replace the cuDNN conv fwd/dgrad/wgrad calls made by timm resnet34
 * (VisionLanguageModule.py:30-35 -> ImageEncoder.forward).
 * Weight operands are produced by vlp_pack_conv:
 *   wp = [Co][KH][KW][C]   (forward),  wt = [C][KH][KW][Co]   (data gradient).
 * Channel counts: C and Co must both be whole 16-byte chunks -- multiples of 8 in
 * bf16, of 4 in fp32.  The loaders resolve (pixel, filter tap) from a chunk's first
 * element and the epilogues store 4- or 8-column groups, so any other count would
 * mix the neighbouring pixel's channels into the sum; vlp_conv_fwd, vlp_conv_dgrad,
 * vlp_conv_dgrad_relu, vlp_conv_wgrad and vlp_conv_wgrad_ws return
 * hipErrorInvalidValue for it (the stem, with 3 input channels, has its own entry
 * points below).  The bf16 data gradients further need Co % 64 == 0 (one filter tap
 * per 64-deep K-step); the fused variants state their own shapes.
 * Operand sizes: every activation tensor must stay below 2 GiB (32-bit buffer
 * offsets); the forward and data-gradient entry points do not check this.
 */
/* y[N][Ho][Wo][Co] = conv(x, w); optionally x := relu(in_scale*x + in_shift)
 * per input channel on load (previous BN+ReLU); accumulates per-channel
 * sum / sum of squares of y into stat_sum / stat_sumsq (fp64, zeroed by caller). */
int vlp_conv_fwd(int dtype, const void* x, const void* wp, void* y, int N, int H, int W, int C,
                 int Co, int KH, int KW, int S, int P, const float* in_scale,
                 const float* in_shift, double* stat_sum, double* stat_sumsq, int stat_rep,
                 void* stream);
/* Conv forward with BN-apply + ReLU of its input fused (timm BasicBlock
 * act1(bn1(conv1(x))) -> conv2, VisionLanguageModule.py:30-32): x is the raw
 * output of the previous conv; each input element becomes
 * relu(in_scale[c]*x + in_shift[c]) once, and that activation is also written to
 * x_act (what this conv's weight gradient reads), so no separate BN pass runs.
 * Bit-identical to vlp_bn_add_relu (no residual) followed by vlp_conv_fwd.
 * Layer-1 geometry only: vlp_conv_fwd_act_ok(...) = 1 when the shape is taken
 * (bf16, C = Co = 64, 3x3, stride 1, pad 1, W = 128); otherwise
 * vlp_conv_fwd_act returns hipErrorInvalidValue. */
int vlp_conv_fwd_act_ok(int dtype, int N, int H, int W, int C, int Co, int KH, int KW, int S, int P);
int vlp_conv_fwd_act(int dtype, const void* x, const void* wp, void* y, void* x_act, int N, int H, int W,
                     int C, int Co, int KH, int KW, int S, int P, const float* in_scale,
                     const float* in_shift, double* stat_sum, double* stat_sumsq, int stat_rep,
                     void* stream);
/* dx[N][H][W][C] = conv^T(dy, w).  If y_bn != NULL: dx := dx * (bn_scale*y_bn +
 * bn_shift > 0) (ReLU mask of the producing BN+ReLU) and stat1 += sum(dx),
 * stat2 += sum(dx * (y_bn - bn_mean) * bn_invstd); else if addend != NULL:
 * dx += addend (residual-branch gradient). */
int vlp_conv_dgrad(int dtype, const void* dy, const void* wt, void* dx, int N, int H, int W, int C,
                   int Co, int KH, int KW, int S, int P, const void* addend, const void* y_bn,
                   const float* bn_scale, const float* bn_shift, const float* bn_mean,
                   const float* bn_invstd, double* stat1, double* stat2, int stat_rep,
                   void* stream);
/* dgrad fused with the next block's output ReLU and BN2 backward sums:
 * g = (dgrad + addend) * (relu_out > 0); stat1 += sum g, stat2 += sum g*(y-mean)*invstd
 * (replaces the separate bn_bwd_reduce pass over dx, out, y2).  Exactly one of
 * relu_out (the activation) and relu_mask (its sign bits as written by
 * vlp_bn_add_relu / vlp_maxpool_fwd: bit e&7 of byte e>>3 for element e) is given. */
int vlp_conv_dgrad_relu(int dtype, const void* dy, const void* wt, void* g, int N, int H, int W,
                        int C, int Co, int KH, int KW, int S, int P, const void* addend,
                        const void* relu_out, const uint8_t* relu_mask, const void* y,
                        const float* mean, const float* invstd, double* stat1, double* stat2,
                        int stat_rep, void* stream);
/* Layer-1 data gradients with their input's BatchNorm backward folded in (timm
 * BasicBlock backward, VisionLanguageModule.py:30-32; replaces vlp_bn_bwd_apply +
 * vlp_conv_dgrad / vlp_conv_dgrad_relu).  The input dy = k*g_in + b*y_in + c (per
 * channel, in_coef = [k | b | c] from vlp_bn_bwd_coef) is formed once per input row
 * in the rows kernel's LDS ring and written to dy_out (the weight gradient's
 * operand); the epilogues are those of vlp_conv_dgrad (y_bn) and vlp_conv_dgrad_relu.
 * Shapes: vlp_conv_dgrad_act_ok (bf16, C = Co = 64, 3x3 stride 1 pad 1, W = 128),
 * else hipErrorInvalidValue.  Bit-identical to the separate pass + data gradient. */
int vlp_conv_dgrad_act_ok(int dtype, int N, int H, int W, int C, int Co, int KH, int KW, int S, int P);
int vlp_conv_dgrad_bn_act(int dtype, const void* g_in, const void* y_in, const float* in_coef, void* dy_out,
                          const void* wt, void* dx, int N, int H, int W, int C, int Co, int KH, int KW,
                          int S, int P, const void* y_bn, const float* bn_scale, const float* bn_shift,
                          const float* bn_mean, const float* bn_invstd, double* stat1, double* stat2,
                          int stat_rep, void* stream);
int vlp_conv_dgrad_relu_act(int dtype, const void* g_in, const void* y_in, const float* in_coef,
                            void* dy_out, const void* wt, void* gout, int N, int H, int W, int C, int Co,
                            int KH, int KW, int S, int P, const void* addend, const void* relu_out,
                            const uint8_t* relu_mask, const void* y, const float* mean,
                            const float* invstd, double* stat1, double* stat2, int stat_rep, void* stream);
/* Second block of layers 2-4 (timm BasicBlock backward, VisionLanguageModule.py:30-32): conv1's
 * data gradient (+ addend) through the previous block's output ReLU (relu_mask sign bits),
 * with that block's bn2 (y, mean, invstd) and downsample-BN (yd, meand, invstdd) backward
 * sums stat1 = sum g, stat2 = sum g*xhat, stat3 = sum g*xhatd in the epilogue (replaces
 * vlp_bn_bwd_reduce over dout, out, y2, yd).  bf16, stride 1, C >= 128, C % 64 == 0. */
int vlp_conv_dgrad_relu2(int dtype, const void* dy, const void* wt, void* g, int N, int H, int W, int C, int Co,
                         int KH, int KW, int S, int P, const void* addend, const uint8_t* relu_mask, const void* y,
                         const float* mean, const float* invstd, const void* yd, const float* meand,
                         const float* invstdd, double* stat1, double* stat2, double* stat3, int stat_rep,
                         void* stream);
/* First block of layers 2-4 (timm BasicBlock with downsample, VisionLanguageModule.py:30-32):
 * conv1's 3x3/2 data gradient with the 1x1/2 downsample's data gradient folded into
 * pixel-parity class (0, 0) as extra K-steps -- replaces vlp_conv_dgrad of the
 * downsample and the addend of vlp_conv_dgrad_relu.  dyd = dy + N*Ho*Wo*Co and
 * wtd = wt + C*KH*KW*Co (one allocation each), bf16, KH = KW = 3, S = 2, P = 1. */
int vlp_conv_dgrad_relu_ds(int dtype, const void* dy, const void* dyd, const void* wt, const void* wtd, void* g,
                           int N, int H, int W, int C, int Co, int KH, int KW, int S, int P,
                           const void* relu_out, const uint8_t* relu_mask, const void* y, const float* mean,
                           const float* invstd, double* stat1, double* stat2, int stat_rep, void* stream);
/* Weight gradient as split-K fp32 slabs: split s of the pixel reduction writes
 * split_ws[s][Co][KH][KW][C] (plain stores, no atomics); *nsplit receives the
 * split count (<= ws_floats / (Co*KH*KW*C)).  vlp_conv_wgrad_fold then sums the
 * slabs into grad[Co][C][KH][KW], the layout of the reference's conv weight
 * gradient (timm resnet34 convs, VisionLanguageModule.py:34-35), overwriting it.
 * Replaces vlp_conv_wgrad + vlp_unpack_conv_grad on the training path. */
int vlp_conv_wgrad_ws(int dtype, const void* dy, const void* x, float* split_ws, long long ws_floats,
                      int* nsplit, int N, int H, int W, int C, int Co, int KH, int KW, int S, int P,
                      void* stream);
int vlp_conv_wgrad_fold(int Co, int C, int KH, int KW, int nsplit, const float* split_ws, float* grad,
                        void* stream);
/* vlp_conv_wgrad_ws takes the layer-1 row-streaming kernel (bf16, C = Co = 64,
 * 3x3/1 pad 1, W = 128; one workgroup per image, one slab each) when the batch
 * holds at least this many images, else the im2col GEMM.  n < 0 restores the
 * default (3/4 of the device's CUs: below it the per-image workgroups leave the
 * chip idle).  *prev (may be null) receives the previous setting (-1 = default).
 * Returns 0.  Host-only, no GPU work. */
int vlp_set_wgrad_rows_min_images(int n, int* prev);
/* dw_ws[Co][KH][KW][C] += sum over pixels dy x_patch (fp32 atomics; zero first).
 * Optional BN+ReLU-on-load of x as in vlp_conv_fwd. */
int vlp_conv_wgrad(int dtype, const void* dy, const void* x, float* dw_ws, int N, int H, int W,
                   int C, int Co, int KH, int KW, int S, int P, const float* in_scale,
                   const float* in_shift, void* stream);

/* stem conv 7x7/2 pad 3, 3 -> 64 channels (timm resnet34 conv1, called from
 * ImageEncoder.forward, VisionLanguageModule.py:34-35), on a zero-padded NHWC4
 * image xp of size [N][Hp][Wp][4] (vlp_stem_geom); the caller zeroes xp once.
 * vlp_stem_prep_u8 also folds the collation's normalise + 3-channel replicate
 * (PretrainDataModule.py:167-171) into the upload of 1-channel uint8 images. */
void vlp_stem_geom(int H, int W, int* Ho, int* Wo, int* Hp, int* Wp);
int vlp_stem_prep(int dtype, const float* x_nchw, void* xp, int N, int H, int W, void* stream);
int vlp_stem_prep_u8(int dtype, const uint8_t* x_u8, void* xp, int N, int H, int W, float mean,
                     float std, void* stream);
int vlp_stem_fwd(int dtype, const void* xp, const void* wp, void* y, int N, int H, int W,
                 double* stat_sum, double* stat_sumsq, int stat_rep, void* stream);
int vlp_stem_wgrad(int dtype, const void* dy, const void* xp, float* dw_ws, int N, int H, int W,
                   void* stream);
/* the same through per-split fp32 slabs split_ws[s][64][256] (plain stores, no
 * atomics; *nsplit receives the split count), then vlp_stem_wgrad_fold sums
 * them into grad[64][3][7][7] (timm conv1.weight layout), overwriting it */
int vlp_stem_wgrad_ws(int dtype, const void* dy, const void* xp, float* split_ws, long long ws_floats,
                      int* nsplit, int N, int H, int W, void* stream);
int vlp_stem_wgrad_fold(int nsplit, const float* split_ws, float* grad, void* stream);

/* single-channel stem for the 1-channel uint8 upload (the reference replicates
 * the grayscale radiograph to 3 identical channels, PretrainDataModule.py:167-171,
 * so conv1 = a 1-channel 7x7/2 conv with the channel-summed weights: K = 64
 * instead of 256).  Image: 4 copies shifted by 0/2/4/6 pixels,
 * xs[4][N][Hp][Wp1] (vlp_stem1_geom; returns non-zero when Wo % 4 != 0, then the
 * caller uses the 3-channel path); weights W1[64][8][8] (vlp_pack_stem1);
 * vlp_stem1_wgrad_ws + vlp_stem1_wgrad_fold give the [64][3][7][7] gradient
 * (identical for the three channels). */
int vlp_stem1_geom(int H, int W, int* Ho, int* Wo, int* Hp, int* Wp1);
int vlp_stem1_prep_u8(int dtype, const uint8_t* x_u8, void* xs, int N, int H, int W, float mean, float std,
                      void* stream);
int vlp_pack_stem1(int dtype, const float* w, void* wp, void* stream);
int vlp_stem1_fwd(int dtype, const void* xs, const void* wp, void* y, int N, int H, int W,
                  double* stat_sum, double* stat_sumsq, int stat_rep, void* stream);
int vlp_stem1_wgrad_ws(int dtype, const void* dy, const void* xs, float* split_ws, long long ws_floats,
                       int* nsplit, int N, int H, int W, void* stream);
int vlp_stem1_wgrad_fold(int nsplit, const float* split_ws, float* grad, void* stream);
/* Fused stem (bf16, single-channel upload): replaces timm's conv1 -> bn1 ->
 * act1 -> maxpool (VisionLanguageModule.py:30-32) without ever writing the
 * full-resolution conv output.  vlp_stem1_pool_fwd computes the conv per
 * output row on MFMA, the BatchNorm sums (stat_* may be NULL: eval mode) and
 * the 3x3/2 pad-1 max-pool of sign(gamma)*y0, i.e. the window's max (gamma >= 0)
 * or min (gamma < 0) of y0, which is where relu(bn(y0)) peaks; it stores the
 * raw y0 there (yarg [N][Ho/2][Wo/2][64]) and the tap kh*3+kw (idx).  Then
 * p = relu(sc*yarg + sh) is vlp_bn_add_relu over the pooled tensor.
 * vlp_stem1_route_bwd writes dy = dBN(route(dp)) for the stem weight gradient,
 * recomputing y0 instead of reading it; dp must be ReLU-masked (p > 0, as the
 * layer-1 data-gradient epilogue produces it).  vlp_stem1_fused_ok(H, W) = 1 when the
 * shape qualifies (Wo a multiple of 64 up to 256, Ho even). */
int vlp_stem1_fused_ok(int H, int W);
int vlp_stem1_pool_fwd(const void* xs, const void* wp1, const float* gamma, void* yarg, uint8_t* idx, int N,
                       int H, int W, double* stat_sum, double* stat_sumsq, int stat_rep, void* stream);
int vlp_stem1_route_bwd(const void* xs, const void* wp1, const void* dp, const uint8_t* idx, const float* sc,
                        const float* sh, const float* mean, const float* istd, const float* gamma,
                        const double* sum_g, const double* sum_gx, void* dy, int N, int H, int W, void* stream);
/* The whole stem backward in one pass (routing + BN backward + weight gradient;
 * replaces the stem's autograd backward behind VisionLanguageModule.py:30-32):
 * dW1 = k R + b W1 G + c S with R = sum g P^T (the pooled gradient routed to its
 * arg-max pixel), G = sum P P^T, S = sum P over the conv-output pixels, so neither
 * y0 nor dy is formed.  grad [64][3][7][7] is overwritten (the same gradient for
 * the 3 identical input channels).  dp ReLU-masked as above; ws holds
 * vlp_stem1_bwd_fused_ws_floats fp32 elements. */
int vlp_stem1_bwd_fused_ws_floats(int N, int H, int W, long long* n);
int vlp_stem1_bwd_fused(const void* xs, const void* wp1, const void* dp, const uint8_t* idx, const float* mean,
                        const float* istd, const float* gamma, const double* sum_g, const double* sum_gx, float* ws,
                        long long ws_floats, float* grad, int N, int H, int W, void* stream);

/* ---------------- image tower: BatchNorm / residual / pooling ----------------
 * Replace timm resnet34's BatchNorm2d (train-mode batch statistics), ReLU,
 * residual add, maxpool 3x3/2 and global average pool (VisionLanguageModule.py:30-35).
 * Per-channel statistic outputs (fp64) are REPLICATED: a producer called with
 * stat_rep = R adds into R copies laid out [R][C] (copy = workgroup % R) so
 * that ~1e5 workgroups do not serialise on C addresses; vlp_stat_reduce folds
 * them into copy 0, which is what every consumer reads.  stat_rep = 1 means a
 * plain [C] buffer. */
int vlp_stat_reduce(int rep, int C, double* a, double* b, double* c, void* stream);
int vlp_bn_finalize(int C, double count, const double* sum, const double* sumsq,
                    const float* gamma, const float* beta, float eps, float momentum,
                    float* running_mean, float* running_var, float* scale, float* shift,
                    float* mean, float* invstd, void* stream);
/* vlp_stat_reduce + vlp_bn_finalize in one launch (sum / sumsq: [rep][C]
 * replicas, folded into copy 0 as a side effect) */
int vlp_bn_finalize_rep(int rep, int C, double count, double* sum, double* sumsq,
                        const float* gamma, const float* beta, float eps, float momentum,
                        float* running_mean, float* running_var, float* scale, float* shift,
                        float* mean, float* invstd, void* stream);
/* vlp_stat_reduce + vlp_bn_param_grad in one launch: dgamma = sum g*xhat,
 * dbeta = sum g; sum_gxd / dgamma_d / dbeta_d (all or none): the downsample BN
 * that shares g (BasicBlock bn2 + downsample.1).  Sums folded into copy 0. */
int vlp_bn_grad_rep(int rep, int C, double* sum_g, double* sum_gx, double* sum_gxd, float* dgamma,
                    float* dbeta, float* dgamma_d, float* dbeta_d, void* stream);
int vlp_bn_eval_coeffs(int C, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* scale, float* shift,
                       void* stream);
/* Shapes of the streaming passes (vlp_bn_add_relu, vlp_bn_bwd_reduce, vlp_bn_bwd_apply,
 * vlp_maxpool_bwd, vlp_maxpool_bwd_apply): a thread keeps one 16-byte channel chunk
 * (8 bf16 / 4 fp32 elements), so C must be a multiple of the chunk, at least one chunk,
 * with a chunk count C / chunk that divides 256 (bf16 C <= 2048, fp32 C <= 1024), and
 * M (N, H, W) >= 1; anything else is hipErrorInvalidValue before any launch. */
/* out = relu(sc*y + sh + idt'), idt' = idt (scd == NULL) or scd*idt + shd; idt == NULL: relu(sc*y + sh).
 * relu_mask (optional, bf16 only, else hipErrorInvalidValue): out's sign bits,
 * byte e>>3 bit e&7 = (out[e] > 0) */
int vlp_bn_add_relu(int dtype, long long M, int C, const void* y, const float* sc, const float* sh,
                    const void* idt, const float* scd, const float* shd, void* out, uint8_t* relu_mask,
                    void* stream);
/* g = dout * (mask > 0) (dout may be a broadcast [N][C]/HW gradient `dbc`);
 * sum_g += sum g, sum_ga += sum g*xhat(ya), sum_gb += sum g*xhat(yb) (yb optional).
 * mask, ya, mean_a, istd_a and one of dout / dbc are required, HW >= 1 with dbc:
 * hipErrorInvalidValue otherwise. */
int vlp_bn_bwd_reduce(int dtype, long long M, int C, const void* dout, const float* dbc, int HW,
                      const void* mask, const void* ya, const float* mean_a, const float* istd_a,
                      const void* yb, const float* mean_b, const float* istd_b, double* sum_g,
                      double* sum_ga, double* sum_gb, int stat_rep, void* stream);
/* coef[3][C] = (k, b, c) of dy = k*g + b*y + c over M rows (the folded BN backward;
 * sums already folded, as vlp_bn_bwd_apply reads them) */
int vlp_bn_bwd_coef(long long M, int C, const float* gamma, const float* istd, const float* mean,
                    const double* sum_g, const double* sum_gx, float* coef, void* stream);
/* dy_s = gamma_s*istd_s*(g - mean(g) - xhat_s*mean(g*xhat_s)) for sides a, b; g_out = g.
 * Side a (ya, dy_a) and one of dout / dbc are required (HW >= 1 with dbc); side b is
 * selected by dy_b and then needs yb: hipErrorInvalidValue otherwise. */
int vlp_bn_bwd_apply(int dtype, long long M, int C, const void* dout, const float* dbc, int HW,
                     const void* mask, const void* ya, const float* mean_a, const float* istd_a,
                     const float* gamma_a, const double* sum_g_a, const double* sum_gx_a,
                     void* dy_a, const void* yb, const float* mean_b, const float* istd_b,
                     const float* gamma_b, const double* sum_g_b, const double* sum_gx_b,
                     void* dy_b, void* g_out, void* stream);
int vlp_bn_param_grad(int C, const double* sum_g, const double* sum_gx, float* dgamma,
                      float* dbeta, void* stream);
/* out = maxpool3x3/2(relu(sc*y + sh)), idx = argmax tap (0..8) per element;
 * yarg (optional): y at the argmax, so the stem BN's backward sums can be taken
 * per pooled output (g*[out>0]*xhat(yarg)) by the layer-1 data-gradient
 * epilogue (vlp_conv_dgrad_relu with relu_out = out, y = yarg) instead of a
 * pass over the full-resolution y */
int vlp_maxpool_fwd(int dtype, int N, int H, int W, int C, const void* y, const float* sc,
                    const float* sh, void* out, uint8_t* idx, void* yarg, uint8_t* relu_mask,
                    void* stream);
/* stem backward, pass 1: g = dp routed to each window's recorded argmax, masked by
 * the stem ReLU; accumulates sum g and sum g*xhat(y) (g itself is not stored) */
int vlp_maxpool_bwd(int dtype, int N, int H, int W, int C, const void* dp, const uint8_t* idx,
                    const void* y, const float* sc, const float* sh, const float* mean,
                    const float* istd, double* sum_g, double* sum_gx, int stat_rep,
                    void* stream);
/* stem backward, pass 2: recomputes g and writes the BatchNorm input gradient
 * dy = gamma*istd*(g - mean(g) - xhat*mean(g*xhat)) in one stream over y */
int vlp_maxpool_bwd_apply(int dtype, int N, int H, int W, int C, const void* dp,
                          const uint8_t* idx, const void* y, const float* sc, const float* sh,
                          const float* mean, const float* istd, const float* gamma,
                          const double* sum_g, const double* sum_gx, void* dy, void* stream);
int vlp_avgpool_fwd(int dtype, int N, int HW, int C, const void* x, void* feat, void* stream);

/* ---------------- text towers (TinyBERT, DistilBERT) ----------------
 * Replace the cuBLAS/ATen kernels of HF BertModel / DistilBertModel
 * (VisionLanguageModule.py:43-45, :57-60). */
/* y = x W^T + bias; mode 0 plain, 1 aux = pre-activation & y = gelu(aux),
 * 2 y = dropout_p(x W^T + bias) + res.  bf16 (also _rs and vlp_linear_dgrad): the
 * output width and every output/operand leading dimension a multiple of 8 and the
 * rows 16-byte aligned (8-column epilogue groups), else hipErrorInvalidValue. */
int vlp_linear_fwd(int dtype, int M, int N, int K, const void* x, int ldx, const void* w,
                   const float* bias, void* y, int ldy, int mode, void* aux, const void* res,
                   int ldr, float p, unsigned long long seed, void* stream);
/* y = res + rscale[row / rps] * (x W^T + bias): a residual branch under DropPath (NesT
 * TransformerLayer, timm nest.py: x + drop_path(attn(norm1(x))); per-sample scale 0 or 1/(1-p)) */
int vlp_linear_fwd_rs(int dtype, int M, int N, int K, const void* x, int ldx, const void* w,
                      const float* bias, void* y, int ldy, const void* res, int ldr, const float* rscale,
                      int rps, void* stream);
/* dx = dy W; mode 1: dx *= gelu'(aux); mode 0: dx += addend (if non-NULL) */
int vlp_linear_dgrad(int dtype, int M, int Kin, int Nout, const void* dy, int lddy, const void* w,
                     void* dx, int lddx, int mode, const void* aux, int ldaux, const void* addend,
                     int ldad, void* stream);
/* dw[Nout][Kin] += dy^T x (fp32 atomics; zero first) */
int vlp_linear_wgrad(int dtype, int M, int Nout, int Kin, const void* dy, int lddy, const void* x,
                     int ldx, float* dw, void* stream);
/* the same through a split-K workspace ws[ks][Nout][Kin] fp32 (bf16 only, Kin % 4 == 0):
 * split partials are plain stores, then one pass folds them into dw (no atomics) */
int vlp_linear_wgrad_ws(int dtype, int M, int Nout, int Kin, const void* dy, int lddy, const void* x,
                        int ldx, float* dw, float* ws, long long ws_elems, void* stream);
/* fp32 elements of the workspace vlp_linear_wgrad_ws uses at its full split count
 * for this shape (host-side query; a smaller workspace trims the splits) */
int vlp_linear_wgrad_ws_floats(int M, int Nout, int Kin, long long* n);
/* out[n] += sum_m x[m][n] (bias gradients; fp32 atomics) */
int vlp_colsum(int dtype, int M, int N, const void* x, int ld, float* out, void* stream);
/* LayerNorm over rows of D <= 1024 (D a multiple of 8 for bf16, 4 for fp32), else
 * hipErrorInvalidValue.  A dropout probability (p, p_out, p_in) outside [0, 1) is refused with
 * hipErrorInvalidValue (1 / (1 - p) would be infinite), M < 1 is a no-op that returns 0, and with
 * M >= 1 a NULL x, gamma, beta, y, mean, rstd (forward) or dy, x, mean, rstd, gamma, dx, dgamma,
 * dbeta (backward) is refused with hipErrorInvalidValue; dxd and addend may be NULL.  Nothing is
 * launched by a refused call. */
int vlp_layernorm_fwd(int dtype, int M, int D, const void* x, const float* gamma,
                      const float* beta, float eps, void* y, float* mean, float* rstd, float p,
                      unsigned long long seed, void* stream);
int vlp_layernorm_bwd(int dtype, int M, int D, const void* dy, float p_out,
                      unsigned long long seed_out, const void* x, const float* mean,
                      const float* rstd, const float* gamma, void* dx, void* dxd, float p_in,
                      unsigned long long seed_in, float* dgamma, float* dbeta, void* stream);
/* dx = LayerNorm backward + addend (pre-norm residual: NesT's x + attn(norm1(x))) */
int vlp_layernorm_bwd_add(int dtype, int M, int D, const void* dy, const void* x, const float* mean,
                          const float* rstd, const float* gamma, const void* addend, void* dx,
                          float* dgamma, float* dbeta, void* stream);
/* the same, also writing dxs = rscale[row / rps] * dx: the DropPath-scaled gradient of the
 * residual branch that produced x (NesT; saves a separate scaling pass) */
int vlp_layernorm_bwd_add_rs(int dtype, int M, int D, const void* dy, const void* x, const float* mean,
                             const float* rstd, const float* gamma, const void* addend, void* dx, void* dxs,
                             const float* rscale, int rps, float* dgamma, float* dbeta, void* stream);
/* softmax attention of one (sequence, head) per workgroup: T <= 64, 1 <= dh <= 64 (head
 * channels padded to 32 or 64 in LDS), else hipErrorInvalidValue.  Also refused with
 * hipErrorInvalidValue, before any launch: a dropout probability p outside [0, 1), a NULL qkv,
 * ctx or P (forward), a NULL qkv, P, dctx or dqkv (backward).  amask may be NULL (no key masked). */
int vlp_attn_fwd(int dtype, int B, int T, int H, int dh, const void* qkv, const long long* amask,
                 void* ctx, float* P, float scale, float p, unsigned long long seed, void* stream);
int vlp_attn_bwd(int dtype, int B, int T, int H, int dh, const void* qkv, const float* P,
                 const void* dctx, void* dqkv, float scale, float p, unsigned long long seed,
                 void* stream);
/* temb / dtemb NULL: a model without a token-type table (DistilBERT); tt given without a table
 * is ignored.  Refused with hipErrorInvalidValue before any division or launch: M < 1, T < 1,
 * D < 1, M % T != 0, a NULL ids, wemb, pemb or e_out (forward), a NULL ids, de, dwemb or dpemb
 * (backward). */
int vlp_embed_fwd(int dtype, int M, int T, int D, const long long* ids, const long long* tt,
                  const float* wemb, const float* pemb, const float* temb, void* e_out,
                  void* stream);
int vlp_embed_bwd(int dtype, int M, int T, int D, const long long* ids, const long long* tt,
                  const void* de, float* dwemb, float* dpemb, float* dtemb, void* stream);
/* out[r * ldo + c] = in[r * ldi + c], r < R, c < D.  R < 1, D < 1, ldi < D, ldo < D or a NULL
 * pointer: hipErrorInvalidValue, nothing launched. */
int vlp_scatter_rows(int dtype, int R, int D, const void* in, int ldi, void* out, int ldo,
                     void* stream);

/* ---------------- retrieval metrics ----------------
 * Replace the topk over the full similarity matrix in
 * precision_at_k_on_image_embeddings (VisionLanguageModule.py:364-400) and
 * recall_at_k_on_image_text_retreival (:402-439).  vals/idx[R][K] = the K
 * largest entries of each row x[r][0..N) in descending order, ties to the
 * lower column; K <= 16.  The caller builds x one query chunk at a time
 * (fp32 vlp_linear_fwd of normalised embeddings). */
int vlp_row_topk(int R, int N, const float* x, long long ldx, int K, float* vals, int* idx, void* stream);

/* ---------------- post-fit silhouette scores ----------------
 * Replace sklearn's silhouette_score over the best checkpoint's cached features in
 * plot_tsne_and_calculate_silhouette.py:56-60 (called from train.py:179-183 and :261-327):
 * sums[q][c] (fp32, [Q][C] dense) = sum over keys j with key_label[j] == c of
 * ||xq[q] - xk[j]||_2, each distance sqrtf(sum_d (a_d - b_d)^2) from direct fp32 differences
 * (a row against itself or a duplicate is exactly 0).  One launch for all of Q, nothing of
 * size Q x N is stored, no atomics: two calls agree bit for bit and equal query rows give
 * equal bits.  A key whose label is outside [0, C) adds to no column (callers validate the
 * labels); Q == 0 returns 0 with no launch, N == 0 writes zeros.  hipErrorInvalidValue before
 * any launch: C < 1, C > 8, D < 1, ldq < D, ldk < D, a negative Q or N, Q or N within 128 of
 * INT_MAX, a NULL xq or sums, a NULL xk or key_label with N > 0. */
int vlp_cluster_dist_sums(int Q, int N, int D, const float* xq, long long ldq, const float* xk,
                          long long ldk, const int* key_label, int C, float* sums, void* stream);

/* ---------------- post-fit t-SNE ----------------
 * Replace sklearn.manifold.TSNE(method="exact") over the best checkpoint's cached features in
 * plot_tsne_and_calculate_silhouette.py:62-66.  Every N below is at most 32768 (P [N][N] fp32
 * stays within 4 GB); no atomics, every sum in one fixed order: two runs agree bit for bit.  A NULL
 * pointer or a size out of range is hipErrorInvalidValue with nothing launched.
 *
 * vlp_tsne_sqdist: d2[i][j] = sum_d (x[i][d] - x[j][d])^2 from direct fp32 differences, any D >= 1:
 * an exactly zero diagonal (and zeros between duplicate rows), nothing negative, symmetric bit for
 * bit.  ldx >= D, ldd >= N.
 *
 * vlp_tsne_affinities: sklearn's _joint_probabilities on d2 [N][ldd].  Per row (one wave each)
 * _binary_search_perplexity in fp64: beta from 1, infinite bounds doubled / halved, at most 100
 * steps, |H - log(perplexity)| <= 1e-5, no diagonal, a zero row sum replaced by 1e-8.  cond [N][N]
 * fp32 (dense, written) is the conditional matrix, ws holds N + 1 doubles of scratch, and
 * P[i][j] = max((cond[i][j] + cond[j][i]) / max(sum, eps), eps) with eps = 2^-52 and a zero
 * diagonal (dense [N][N] fp32; symmetric bit for bit).  2 <= N, 0 < perplexity < N.
 *
 * vlp_tsne_pairs: the all-pairs pass of one iteration over Y [N][2] and P [N][N].  With
 * d = y_i - y_j and q = 1 / (1 + |d|^2) (fp32), the sums over j != i, accumulated in fp64:
 * parts[i][0..7) = { q, p q d_0, p q d_1, q^2 d_0, q^2 d_1, p (log p + log(1 + |d|^2)), p };
 * the last two only when check != 0 (0 otherwise), from a second instantiation of the kernel.
 *
 * vlp_tsne_update: one step of sklearn's _gradient_descent from parts (one workgroup).
 * Z = sum_i parts[i][0]; grad = (float)(4 (exag attr - rep / Z)); where update * grad < 0 the
 * gain += 0.2, elsewhere *= 0.8, floored at 0.01; grad *= gain; update = momentum * update -
 * lr * grad; Y += update -- every fp32 operation rounded on its own, as numpy's.  exag is the
 * early exaggeration of this iteration (P is never rescaled).  When check != 0, stats[0] = the KL
 * divergence sum_i parts[i][5] + log(Z) sum_i parts[i][6] of the Y the step started from, and
 * stats[1] = the norm of the gained gradient (what _gradient_descent compares with
 * min_grad_norm); these two doubles are the only values the host reads during the descent. */
int vlp_tsne_sqdist(int N, int D, const float* x, long long ldx, float* d2, long long ldd, void* stream);
int vlp_tsne_affinities(int N, const float* d2, long long ldd, double perplexity, float* cond,
                        double* ws, float* P, void* stream);
int vlp_tsne_pairs(int N, const float* Y, const float* P, double* parts, int check, void* stream);
int vlp_tsne_update(int N, const double* parts, float* Y, float* update, float* gains, float exag,
                    float momentum, float lr, int check, double* stats, void* stream);

/* ---------------- the linear probe's logistic regression ----------------
 * Replace sklearn.linear_model.LogisticRegression (and decision_function / predict) over the
 * image features in LinearProbeCallback.py:72-85.  The objective is sklearn's binary L2 one with
 * an unpenalised intercept, scaled as sklearn >= 1.4 scales it:
 *   f(w, b) = (1/N) sum_i [softplus(z_i) - y_i z_i] + (lambda / 2) |w|^2,  z_i = x_i . w + b,
 *   lambda = 1 / (C N),
 * solved by a truncated Newton method (conjugate gradients on Hessian-vector products).  x [N][ldx]
 * is fp32 as the encoders return it, y [N] holds 0.0 / 1.0, everything else is fp64: the
 * coefficient vectors are D + 1 doubles (the intercept last; x~ = (x, 1) below).  No atomics, every
 * sum in one fixed order: two fits agree bit for bit.  hipErrorInvalidValue before any launch:
 * a NULL pointer that the call uses, N < 1, N > 2^30, D < 1, D > 2048, ldx < D, C <= 0 (or NaN),
 * a mode outside 0 .. 3.
 *
 * vlp_logreg_pass: one pass over X; workgroup g owns rows [32 g, 32 g + 32) and writes
 * parts[g][0 .. D + 2), with G = ceil(N / 32) partials in all.  With t_i = x~_i . u:
 *   mode 0 GRAD   s[i] = p_i (1 - p_i) (written), c_i = p_i - y_i with p_i = sigmoid(t_i),
 *                 l_i = softplus(t_i) - y_i t_i; parts[g] = { sum c_i x_i, sum c_i, sum l_i }
 *   mode 1 HVP    c_i = s[i] t_i (s read); parts[g] = { sum c_i x_i, sum c_i, 0 }; returns at
 *                 entry where state is non-NULL and its done flag is set
 *   mode 2 LOSS   parts[g][D + 1] = sum l_i, the rest of parts untouched
 *   mode 3 SCORES z[i] = t_i, nothing else (decision_function)
 * sigmoid and softplus are the overflow-safe forms in e = exp(-|t|): softplus(750) = 750 exactly,
 * p is exactly 1 from t = 37 up and exactly 0 once e^t underflows, s is exactly 0 there, and no
 * inf or NaN arises from finite inputs.  Pointers a mode does not use may be NULL.
 *
 * The four kernels below run in one workgroup.  vec holds { g, d, r, q }, 4 (D + 1) doubles;
 * state holds 10 doubles of which the host reads the first five, 40 bytes per outer iteration and
 * the fit's only device-to-host traffic: [0] f(w), [1] |g|_inf, [2] g . d, [3] f(wt), [4] CG steps
 * taken, [5] the penalty of wt, [6] r . r, [7] the CG tolerance, [8] the done flag, [9] |g|_2.
 * `fold` is (parts[0][j] + parts[1][j] + ...) / N in ascending g; products are rounded on their
 * own (no multiply-add), vector sums run thread-strided (entries t, t + 1024, t + 2048) and then
 * through a halving tree over 1024 slots, so a numpy evaluation in that order gives the same bits.
 *
 * vlp_logreg_newton_begin (after a GRAD pass at w): g = fold + lambda (w, 0); [0] = fold of the
 * losses + (lambda / 2) |w|^2; [1]; [9]; d = 0, r = q = -g; [2] = [4] = 0; [6] = g . g;
 * [7] = min(0.5, sqrt |g|_2) |g|_2; [8] = 1 where |g|_inf <= tol or g = 0, else 0.
 * vlp_logreg_cg_step (after an HVP pass at q): returns at entry where [8] is set.  Hq = fold +
 * lambda (q, 0); alpha = [6] / q . Hq; d += alpha q; r -= alpha Hq; beta = r . r / [6]; q = r + beta q;
 * [2] = g . d; [4] += 1; [6] = r . r; [8] = 1 where sqrt(r . r) <= [7].  A curvature q . Hq that is not
 * positive (rounding only: the objective is strictly convex) sets [8] and changes nothing else.
 * vlp_logreg_trial: wt = w + t d; [5] = (lambda / 2) |wt[0 .. D)|^2.
 * vlp_logreg_trial_loss (after a LOSS pass at wt): [3] = fold of the losses + [5]. */
int vlp_logreg_pass(int mode, int N, int D, const float* x, long long ldx, const double* y,
                    const double* u, double* s, double* parts, double* z, const double* state,
                    void* stream);
int vlp_logreg_newton_begin(int N, int D, double C, const double* parts, const double* w, double tol,
                            double* vec, double* state, void* stream);
int vlp_logreg_cg_step(int N, int D, double C, const double* parts, double* vec, double* state,
                       void* stream);
int vlp_logreg_trial(int N, int D, double C, const double* w, double t, const double* vec, double* wt,
                     double* state, void* stream);
int vlp_logreg_trial_loss(int N, int D, const double* parts, double* state, void* stream);

/* ---------------- the baselines' binary classification metrics ----------------
 * Replace torchmetrics' Binary{Accuracy, Precision, Recall, F1Score, AUROC} (threshold 0.5) of
 * FusionModule.py:251-286 / :393-504 and OnlyImagingModule.py:305-430 with an integer
 * accumulator on the device.  The device
 * compares fp32 scores and adds integers, nothing else: no sum depends on its order, and the host
 * derives the five values from six integers.  No atomics; the calls of one accumulator belong on
 * one stream.  hipErrorInvalidValue before any launch: a NULL pointer that the call uses, a
 * negative size, a label_kind outside 0 .. 2, offset + n > capacity, n > 2^18 or splits outside
 * 1 .. ceil(n / 256) for the pair count.
 *
 * vlp_binmetric_append (one workgroup): scores[offset + i] = prob[i] and labels[offset + i] = the
 * label of row i for i < n -- 1 where the input is 1, 0 where it is 0, else 2, which is counted
 * nowhere -- and counts[0 .. 4) += the batch's tp, fp, fn, tn with the prediction prob >= 0.5f.
 * label_kind: 0 int64, 1 int32, 2 uint8 (bool).  prob is the probability, not the logit.  n = 0
 * returns without a launch.
 * vlp_binmetric_pairs: over i with labels[i] = 1 and j with labels[j] = 0 among the first n rows,
 * wins = #{scores[i] > scores[j]} and ties = #{scores[i] == scores[j]}, so that
 * AUROC = (2 wins + ties) / (2 n1 n0), the Mann-Whitney statistic with tie-averaged ranks.  Grid
 * (ceil(n / 256), splits): a workgroup keeps 256 values of i in registers and streams its share of
 * the j range through LDS; parts[(by * ceil(n / 256) + bx)][2] = its { wins, ties }.  O(n^2) pairs:
 * meant for n <= 2^18.  A NaN score is out of contract (it is counted in no pair).
 * vlp_binmetric_fold (one workgroup): out[0 .. 4) = counts, out[4] = sum of parts[.][0], out[5] =
 * sum of parts[.][1]: the 48 bytes the host reads.  nparts = 0 gives zero pair counts. */
int vlp_binmetric_append(int n, const float* prob, const void* label, int label_kind, float* scores,
                         unsigned char* labels, long long offset, long long capacity, long long* counts,
                         void* stream);
int vlp_binmetric_pairs(int n, const float* scores, const unsigned char* labels, int splits,
                        unsigned long long* parts, void* stream);
int vlp_binmetric_fold(int nparts, const unsigned long long* parts, const long long* counts, long long* out,
                       void* stream);

/* ---------------- the test-set evaluation's per-subgroup counts ----------------
 * Replace the boolean-mask subsets of scripts/test_eval_downstream.py:120-236 (evaluate_results:
 * about 40 subsets per fold, six sklearn calls each) with one device op that counts every group of
 * every level at once.  n rows: scores [n] fp32 (probabilities: finite, a NaN is out of contract as
 * above), labels [n] uint8 in vlp_binmetric_append's encoding (1, 0, or 2 = counted nowhere), and
 * for each of L levels (1 .. 8) a group code per row, codes [L][n] uint8: 0 .. G_l - 1, or 255 for
 * "in no group of this level".  cell_base [L + 1] (HOST memory) holds the prefix sums of the G_l
 * (1 .. 255 each, cell_base[0] = 0); cells = cell_base[L].
 *   out [cells][6] int64: for level l and group g, at cell_base[l] + g, over the rows with
 *   codes[l][.] == g: tp, fp, fn, tn with the prediction score >= 0.5f, and over positive i and
 *   negative j among them wins = #{s_i > s_j}, ties = #{s_i == s_j}
 * -- vlp_binmetric_*'s six integers for that subset; a level with G = 1 and all codes 0 returns
 * exactly what they return.  A pair belongs to a level's group when both rows carry its code, so
 * one pass over the pairs serves all levels.  Two launches: the pair kernel on a grid
 * (ceil(n / 256), splits) -- 256 rows i in registers with their codes packed in 64 bits, the j
 * range streamed through LDS as (score or NaN, packed codes), per pair two fp32 compares and per
 * level a byte compare and two 32-bit adds; each workgroup folds its threads by cell through LDS
 * and writes its own [cells][6] partial into ws -- and a one-workgroup fold.  Integers only, no
 * atomics, bitwise reproducible.  ws: vlp_groupmetric_ws_bytes(n, L, cells) bytes of scratch that
 * need no initialisation.  hipErrorInvalidValue before any launch: a NULL pointer, n < 1,
 * n > 2^18, L outside 1 .. 8, cell_base[0] != 0, a G_l outside 1 .. 255 (a cell_base that does not
 * increase), ws_bytes below vlp_groupmetric_ws_bytes. */
int vlp_groupmetric_ws_bytes(int n, int L, int cells, long long* bytes);
int vlp_groupmetric_counts(int n, const float* scores, const unsigned char* labels, int L,
                           const unsigned char* codes, const int* cell_base, long long* out, void* ws,
                           long long ws_bytes, void* stream);

/* ---------------- the baselines' weighted BCE + CORAL loss ----------------
 * Replace FusionModule.py:341-390 (_compute_loss, shared by OnlyImagingModule) and
 * coral_loss/coral.py:5-37 with one device op in fp64 that returns the three logged losses and
 * both gradients: no boolean-mask index, nothing read back.  With x_i row i of feat, c_i =
 * domain[i] (0 INTERNAL / source, 1 BTXRD / target, anything else takes no part in CORAL but counts
 * in the BCE), n_s, n_t the two counts, mu_s, mu_t the domains' column means and
 * w_i = +1 / (n_s - 1) (source), -1 / (n_t - 1) (target), 0 (else):
 *   Delta = sum_i w_i x_i x_i^T - mu_s mu_s^T / (n_s - 1) + mu_t mu_t^T / (n_t - 1)      [D][D]
 *   coral = lambda ||Delta||_F^2 / (4 D^2)
 *   d coral / d x_i = (lambda w_i / D^2) (x_i - mu_dom(i) / n_dom(i)) Delta
 * -- the reference's "covariance" subtracts the mean outer product once, not n times
 * (coral.py:31-35), which is kept.  coral and its gradient are exactly 0 where n_s <= 1, n_t <= 1 or
 * lambda == 0 (:375-376); the device decides that from the codes.  With z_i = logits[i], y_i =
 * label[i] and u_i = w0 where y_i == 0, else w1:
 *   cls = (1 / N) sum_i u_i (max(z_i, 0) - z_i y_i + log1p(exp(-|z_i|)))
 *   d cls / d z_i = u_i (sigmoid(z_i) - y_i) / N
 * out[3] (fp64, written on the device) = { cls + coral, cls, coral }; g_feat [N][D] fp32 =
 * d coral / d x and g_logits [N] fp32 = d cls / d z, each rounded once from fp64.  A NULL g_feat
 * skips the gradient pass (and Delta's store), a NULL g_logits that store; out's bits do not
 * depend on either.  feat [N][ldf] fp32; label_kind as vlp_binmetric_append (0 int64, 1 int32,
 * 2 uint8); ws: vlp_domain_loss_ws_bytes(N, D) bytes of scratch that need no initialisation.
 *
 * At most four launches (three without g_feat, two at lambda == 0 without it): the statistics
 * (per chunk of 256 rows: per-domain column sums, counts, the BCE sum, g_logits), the 64 x 64
 * tiles of Delta with their Frobenius partials, the 32 x 64 tiles of g_feat, and a one-workgroup
 * fold into out.  fp64 FMA throughout, no atomics; every sum runs in one order fixed by N and D
 * (rows in ascending index, Delta's rows in ascending index, partials thread-strided and then a
 * halving tree), so two calls on the same inputs return the same bits.
 * hipErrorInvalidValue before any launch: a NULL pointer that the call uses (out always; feat,
 * logits, label, domain, ws when N > 0), N < 0, N > 2^18, D < 1, D > 2048, ldf < D, a label_kind
 * outside 0 .. 2, ws_bytes below vlp_domain_loss_ws_bytes.  N = 0 launches nothing and zeroes out. */
int vlp_domain_loss_ws_bytes(int N, int D, long long* bytes);
int vlp_domain_loss(int N, int D, const float* feat, long long ldf, const float* logits, const void* label,
                    int label_kind, const unsigned char* domain, double w0, double w1, double coral_lambda,
                    double* out, float* g_feat, float* g_logits, double* ws, long long ws_bytes, void* stream);

/* ---------------- NesT image encoder (BASELINE configs[3]) ----------------
 * Replace timm nest.py's pieces behind ImageEncoder's timm.create_model("nest_small", ...)
 * (VisionLanguageModule.py:27-35).  Blocked local attention: qkv[BT*N][3C] rows (q | k | v,
 * head h at h*32), out[BT*N][C] head-major (h*32 + d; timm's d*H + h order is folded into
 * the proj weight with vlp_nest_permute_cols), lse[BT*H*N] (log2 domain), head dim 32.
 * Backward: delta[BT*H*N] scratch; writes every column of dqkv.  A NULL qkv, out, lse (forward)
 * or qkv, out, dout, lse, delta, dqkv (backward) is refused with hipErrorInvalidValue before any
 * launch, here and in vlp_vit_attn_*. */
int vlp_nest_attn_fwd(int dtype, int BT, int H, int N, int dh, const void* qkv, void* out, float* lse,
                      float scale, void* stream);
int vlp_nest_attn_bwd(int dtype, int BT, int H, int N, int dh, const void* qkv, const void* out,
                      const void* dout, const float* lse, float* delta, void* dqkv, float scale, void* stream);
/* blockify (timm nest.blockify, + pos[Hg*Wg][bs*bs][C] when non-NULL): NHWC image
 * x[B][Hg*bs][Wg*bs][C] -> tokens y[B][Hg*Wg][bs*bs][C]; inverse = deblockify (y <- x tokens) */
int vlp_nest_blockify(int dtype, int B, int Hg, int Wg, int bs, int C, const void* x, const float* pos,
                      void* y, int inverse, void* stream);
/* dpos[t][c] = sum_b dy[b][t][c] over the B samples of a level input [B][TN][C] */
int vlp_nest_pos_grad(int dtype, int B, int TN, int C, const void* dy, float* dpos, void* stream);
/* ConvPool's max pool 3x3 / 2, padding 1 (NHWC); idx = window tap 0..8 */
int vlp_nest_maxpool_fwd(int dtype, int B, int H, int W, int C, const void* x, void* y, uint8_t* idx,
                         void* stream);
int vlp_nest_maxpool_bwd(int dtype, int B, int H, int W, int C, const void* dy, const uint8_t* idx,
                         void* dx, void* stream);
/* patch-embed im2col: 4x4/4 patches -> out[B*(H/4)*(W/4)][48] in level-0 blocked token order;
 * exactly one of x (fp32 [B][3][H][W], normalised) / x_u8 ([B][1][H][W], (v-mean)/std) */
int vlp_nest_patch_prep(int dtype, int B, int H, int W, int bs, const float* x, const uint8_t* x_u8,
                        float mean, float std_, void* out, void* stream);
/* y[m][n] += bias[n] */
int vlp_nest_add_bias(int dtype, long long M, int N, void* y, const float* bias, void* stream);
/* proj weight input columns: dst[n][h*Dh + d] = src[n][d*H + h] (fp32 -> dtype_out), and back */
int vlp_nest_permute_cols(int dtype_out, int Nr, int H, int Dh, const float* src, void* dst, void* stream);
int vlp_nest_unpermute_cols(int Nr, int H, int Dh, const float* src, float* dst, void* stream);
/* DropPath: mode 0 x += s[m / rows] * y; mode 1 y = s[m / rows] * x */
int vlp_nest_rowscale(int dtype, long long M, int N, int rows, const float* s, void* x, void* y, int mode,
                      void* stream);
/* global average pool backward: dy[b*HW + p][c] = dfeat[b][c] * inv */
int vlp_nest_bcast(int dtype, int B, int HW, int C, const float* dfeat, float inv, void* dy, void* stream);

/* ---------------- ViT image encoder (vit_base_patch16_224, vit_large_patch16_224) ----------------
 * Replace timm vision_transformer.py's pieces behind timm.create_model(model, ...)
 * (OnlyImagingModule.py:73; ImageEncoder, VisionLanguageModule.py:30-32).  The blocks run on
 * vlp_layernorm_* / vlp_linear_* and on the NesT flash-attention kernels at head dim 64.
 * Attention over B images of N >= 1 tokens: qkv[B*N][3C] rows (q | k | v, head h at h*64),
 * out[B*N][C] head-major (h*64 + d, timm's own order: no proj-weight permutation),
 * lse[B*H*N] (log2 domain), head dim 64 only.  Backward: delta[B*H*N] scratch; writes
 * every column of dqkv.  No atomics: results are bitwise reproducible. */
int vlp_vit_attn_fwd(int dtype, int B, int H, int N, int dh, const void* qkv, void* out, float* lse,
                     float scale, void* stream);
int vlp_vit_attn_bwd(int dtype, int B, int H, int N, int dh, const void* qkv, const void* out,
                     const void* dout, const float* lse, float* delta, void* dqkv, float scale, void* stream);
/* patch-embed im2col: 16x16/16 patches -> out[B*(H/16)*(W/16)][768], raster patch order, columns
 * (c, ky, kx) as patch_embed.proj.weight[D][3][16][16] flattens; H, W multiples of 16; exactly
 * one of x (fp32 [B][3][H][W], normalised) / x_u8 ([B][1][H][W], (v-mean)/std, channel replicated) */
int vlp_vit_patch_prep(int dtype, int B, int H, int W, const float* x, const uint8_t* x_u8, float mean,
                       float std_, void* out, void* stream);
/* tok[b][0] = cls + pos[0], tok[b][1+p] = patch[b][p] + pos[1+p]: patch[B*(N-1)][D], cls[D] and
 * pos[N][D] fp32, tok[B*N][D]; D a multiple of the 16-B chunk (8 bf16 / 4 fp32) */
int vlp_vit_assemble(int dtype, int B, int N, int D, const void* patch, const float* cls, const float* pos,
                     void* tok, void* stream);

/* ---------------- contrastive head ----------------
 * Replace VisionLanguageModule.forward (VisionLanguageModule.py:441-461: projections,
 * F.normalize, logit_scale.exp().clamp(max=100) * img @ txt.T) and
 * VisionLanguageModule._compute_loss (VisionLanguageModule.py:532-554: symmetric CE). */
int vlp_l2norm_fwd(int R, int E, const float* x, float* y, float* norm, void* stream);
/* dx = gscale[0] * d normalize(x) (gscale may be NULL = 1); optional compute-dtype copy */
int vlp_l2norm_bwd(int dtype, int R, int E, const float* y, const float* norm, const float* dy,
                   const float* gscale, float* dx, void* dx_t, void* stream);
/* y = x * s[0] (+ y if accumulate); s may be NULL (= 1) */
int vlp_scale(int n, const float* x, const float* s, float* y, int accumulate, void* stream);
/* out[3] = {(parts0 + parts1) / (2N), parts0 / N, parts1 / N} */
int vlp_clip_loss_finish(const float* parts, int N, float* out, void* stream);
/* Fused global-batch symmetric InfoNCE, forward + backward (replaces the
 * logits matmul and the two F.cross_entropy calls of VisionLanguageModule.py
 * :456-459 / :550-552 with their autograd backward).  img_all/txt_all: [N][E]
 * gathered normalised embeddings (E <= 256, E % 4 == 0); this rank owns rows
 * [offset, offset+B).  Written (not accumulated): g_img_all/g_txt_all, d loss /
 * d embeddings for all N rows; d_logit_scale; loss_parts[0] the sum of the
 * image->text CE terms of the local rows, loss_parts[1] text->image; lse_out
 * (optional) [2][B].  role_w (optional, device, 2 floats): the gradients are those
 * of (role_w[0] image_loss + role_w[1] text_loss) / 2 (NULL: {1, 1}, the
 * reference's loss; other weights carry gradients of image_loss / text_loss).  ws: vlp_clip_loss_ws_floats(B, N, E) floats of scratch
 * (cosines / softmax weights, split-key partials, dq slabs; every product on fp32
 * MFMA; no atomics, bitwise reproducible).  ABI 3 (vlp_abi_version). */
int vlp_clip_loss_ws_floats(int B, int N, int E, long long* n);
int vlp_clip_loss_fused(int B, int N, int E, int offset, const float* img_all,
                        const float* txt_all, const float* logit_scale, float* g_img_all,
                        float* g_txt_all, float* d_logit_scale, float* loss_parts,
                        float* lse_out, const float* role_w, float* ws, long long ws_floats,
                        void* stream);
/* vlp_clip_loss_fused with duplicate-caption negatives masked out (the global batch of a
 * data-parallel job holds captions more than once; the reference's sampler rules that out
 * per process only, and its own masked / deduplicate branches of _compute_loss,
 * VisionLanguageModule.py:506-530 / :532-554, are retired).  cid_all: [N] device ints, one
 * caption id per gathered row.  An entry (i, j), i != j, with cid_all[i] == cid_all[j] is
 * left out of both softmaxes as if its logit were -inf (not the retired logits * mask, which
 * keeps exp(0) in the denominator): nothing in either log-sum-exp, zero gradient, no part in
 * d_logit_scale; the diagonal always stays, and a row left with its diagonal alone gives
 * exactly 0 loss and 0 gradient.  Losses stay means over all N rows / columns.  Same
 * workspace (vlp_clip_loss_ws_floats), outputs and role_w as vlp_clip_loss_fused, and with
 * all ids distinct the same bits. */
int vlp_clip_loss_fused_masked(int B, int N, int E, int offset, const float* img_all,
                               const float* txt_all, const float* logit_scale, const int* cid_all,
                               float* g_img_all, float* g_txt_all, float* d_logit_scale,
                               float* loss_parts, float* lse_out, const float* role_w, float* ws,
                               long long ws_floats, void* stream);
/* symmetric CE over explicit logits [B][B]: out = {loss, image_loss, text_loss} (+=);
 * dlogits (+=, optional) = d (role_w[0] image_loss + role_w[1] text_loss) / 2 / d logits
 * (role_w NULL: {1, 1}, the reference's loss, :550-552) */
int vlp_ce_sym(int B, const float* logits, float* out, float* dlogits, const float* role_w, void* stream);
/* vlp_ce_sym under vlp_clip_loss_fused_masked's rule: cid [B] device ints, entries (i, j),
 * i != j, with cid[i] == cid[j] are left out of both softmaxes and get no gradient */
int vlp_ce_sym_masked(int B, const float* logits, const int* cid, float* out, float* dlogits,
                      const float* role_w, void* stream);
/* C[M][N] (=|+=) alpha * sum_k A(m,k) B(n,k) on MFMA; a_kc / b_kc: K-contiguous
 * operand ([rows][ld]) else MN-contiguous ([K][ld]).  Every contiguous extent and
 * leading dimension a multiple of 16 B (4 fp32 / 8 bf16), N and ldc multiples of 4;
 * otherwise hipErrorInvalidValue */
int vlp_matmul(int dtype, int M, int N, int K, const void* A, int lda, int a_kc, const void* B,
               int ldb, int b_kc, void* C, int ldc, int out_f32, float alpha, int accumulate,
               void* stream);
int vlp_cast(int dtype, long long n, const float* x, void* y, void* stream);

/* ---------------- optimizer / packing ----------------
 * Replace torch.optim.AdamW as built by configure_optimizers
 * (VisionLanguageModule.py:130-184, configs/optimizer/adamw.yaml:1-3).
 * step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t) come from the host.  g is only
 * read.  vlp_adamw and the three step entry points below are one kernel and one set of checks:
 * 16-B vector accesses where p, g, m, v (and acc) share their 16-B misalignment, scalar ones
 * otherwise; a NULL or not 4-B aligned p / g / m / v with n > 0 is hipErrorInvalidValue with
 * nothing launched; n <= 0 launches nothing and returns 0. */
int vlp_adamw(long long n, float* p, const float* g, float* m, float* v, float lr, float beta1,
              float beta2, float eps, float wd, float step_size, float bc2_sqrt, void* stream);
/* Gradient clipping on the device: replace torch.nn.utils.clip_grad_norm_ / clip_grad_value_
 * as Lightning's Trainer applies them for gradient_clip_val / gradient_clip_algorithm
 * (configs/experiment/baseline_only_imaging/baseline_only_imaging_vit_base_16_only_100_samples.yaml:16).
 * No host synchronisation and no atomics: every sum has a fixed order, so the norm and the
 * step that uses it are bitwise reproducible.
 *
 * vlp_grad_sumsq: partials[s] = sum of g[i]^2 (squares and sums in fp64) over segment s of the
 * span, elements [16384 s, 16384 (s + 1)); *nparts (host memory, written during the call) =
 * ceil(n / 16384), a function of n alone, so several spans can be laid end to end in one
 * partials buffer.  g needs only 4-B alignment.  n <= 0: *nparts = 0, nothing launched, returns 0;
 * a NULL pointer or a g that is not 4-B aligned: hipErrorInvalidValue, nothing launched.
 * vlp_grad_sumsq_nparts: the same count without a launch (to size the partials buffer). */
int vlp_grad_sumsq_nparts(long long n, int* nparts);
int vlp_grad_sumsq(long long n, const float* g, double* partials, int* nparts, void* stream);
/* one workgroup: out[0] = (float)sqrt(sum of partials[0 .. nparts)) (fp64 sum, fixed order),
 * out[1] = min(1, max_norm / (out[0] + 1e-6f)): clip_grad_norm_'s total_norm and clamped
 * coefficient (error_if_nonfinite=False: non-finite values propagate as in torch) */
int vlp_clip_coef(int nparts, const double* partials, float max_norm, float* out, void* stream);
/* vlp_adamw on the clipped gradient gi, which is also stored back to g (what torch leaves in
 * p.grad).  mode 1: gi = g[i] * coef[0], coef a DEVICE pointer (vlp_clip_coef's out + 1);
 * mode 2: gi = clamp(g[i], -clip_value, clip_value) (gradient_clip_algorithm: value).
 * The update after that is vlp_adamw's; with coef[0] == 1 the results are its bits. */
int vlp_adamw_clip(long long n, float* p, float* g, float* m, float* v, float lr, float beta1,
                   float beta2, float eps, float wd, float step_size, float bc2_sqrt, int mode,
                   const float* coef, float clip_value, void* stream);
/* Gradient accumulation on the device (Lightning's accumulate_grad_batches): the backward
 * overwrites the flat gradient arena, so the micro-batches of one optimizer step are summed in
 * an accumulator of the same layout.  Same conventions as above: no host synchronisation, no
 * atomics, bitwise reproducible; 16-B vector accesses where the operands share their 16-B
 * misalignment (spans at equal offsets of equally laid out arenas do), scalar ones otherwise;
 * every pointer needs 4-B alignment (hipErrorInvalidValue if not, or if NULL with n > 0);
 * n <= 0 launches nothing.
 *
 * vlp_grad_accum: acc[i] = (first ? 0 : acc[i]) + w * g[i], one fused multiply-add per element.
 * first != 0 does not read acc, which may hold anything (no memset is needed).
 * vlp_grad_accum_sumsq: vlp_grad_sumsq of s[i] = fmaf(w, g[i], acc[i]), the accumulated gradient
 * including a last micro-batch that is never stored; same segments, partials layout and *nparts,
 * so vlp_clip_coef consumes the partials unchanged.
 * vlp_adamw_clip_accum: the vlp_adamw update on the gradient s[i] = fmaf(w, g[i], acc[i]) (the
 * value vlp_grad_accum_sumsq squared), after mode 1: s * coef[0], mode 2: clamp(s, +-clip_value),
 * mode 0: nothing.  One pass reads p, g, acc, m, v and writes p, m, v; g and acc are left alone.
 * acc == NULL: vlp_adamw_clip with the same arguments, bit for bit (g written back, modes 1 / 2). */
int vlp_grad_accum(long long n, float* acc, const float* g, float w, int first, void* stream);
int vlp_grad_accum_sumsq(long long n, const float* acc, const float* g, float w, double* partials,
                         int* nparts, void* stream);
int vlp_adamw_clip_accum(long long n, float* p, float* g, float* m, float* v, float lr, float beta1,
                         float beta2, float eps, float wd, float step_size, float bc2_sqrt, int mode,
                         const float* coef, float clip_value, const float* acc, float w,
                         void* stream);
/* Replace torch.optim.Adam (configs/optimizer/adam.yaml:3, the `optimizer: adam` experiments;
 * built by the reference's configure_optimizers, VisionLanguageModule.py:130-184, from the same
 * parameter groups) with clipping and accumulation fused as above.  Adam differs from AdamW in
 * the weight decay alone: it is an L2 term of the gradient, not a decay of the parameter.
 * Arguments as vlp_adamw_clip_accum; per element
 *   s  = acc ? fmaf(w, g[i], acc[i]) : g[i]
 *   c  = mode 1: s * coef[0] (coef a DEVICE pointer) | mode 2: clamp(s, +-clip_value) | mode 0: s
 *   gd = fmaf(wd, p[i], c)           (torch: grad + weight_decay * param, after the clipping)
 *   m, v, p: vlp_adamw's moment and parameter update on gd, without its p *= 1 - lr * wd
 * (lr enters through step_size alone).  With wd == 0 the results are the bits of vlp_adamw
 * (acc == NULL, mode 0), vlp_adamw_clip (acc == NULL, modes 1 / 2) or vlp_adamw_clip_accum.
 * All six combinations of mode 0..2 with and without acc are valid.  With acc, g and acc are left
 * alone; without, modes 1 / 2 store c back to g (what torch leaves in p.grad: the clipped
 * gradient, never gd) and mode 0 only reads g.  One pass over 4 or 5 fp32 streams in and 3 or 4
 * out, the bytes vlp_adamw_clip_accum moves for the same case.  Same conventions: no host
 * synchronisation, no atomics, bitwise reproducible; 16-B vector accesses where the operands share
 * their 16-B misalignment, scalar ones otherwise; every pointer needs 4-B alignment.
 * hipErrorInvalidValue with nothing launched: a NULL or misaligned p / g / m / v with n > 0, a
 * misaligned acc, a NULL coef in mode 1, a mode outside 0..2.  n <= 0 launches nothing, returns 0. */
int vlp_adam_step(long long n, float* p, float* g, float* m, float* v, float lr, float beta1,
                  float beta2, float eps, float wd, float step_size, float bc2_sqrt, int mode,
                  const float* coef, float clip_value, const float* acc, float w, void* stream);
int vlp_pack_conv(int dtype, int Co, int C, int KH, int KW, const float* w, void* wp, void* wt,
                  void* stream);
/* vlp_pack_conv for n <= 48 convolutions in one launch: desc holds n rows of
 * 6 values {w, wp, wt (device pointers; wp / wt may be 0), Co, C, KH*KW}
 * (host memory, read during the call) */
int vlp_pack_conv_batch(int dtype, int n, const long long* desc, void* stream);
int vlp_pack_stem(int dtype, const float* w, void* wp, void* stream);
int vlp_unpack_conv_grad(int Co, int C, int KH, int KW, const float* ws, float* g, void* stream);
int vlp_unpack_stem_grad(const float* ws, float* g, void* stream);

/* ---------------- radiograph preprocessing / augmentation ----------------
 * Replace the reference's CPU DataLoader transforms (src/data/PretrainDataModule.py:157-198).
 * vlp_prep_images: n grayscale images of any size packed back to back in src (uint8 when
 * src_u8, else fp32; element offsets off[n] and sizes hw[n][2] in DEVICE memory) ->
 * HistogramNormalized (MONAI, 256 bins) -> CropLargerDimension(0.05) ->
 * PadToSquaredEdgeAverage -> Resized(S, area) -> (x - mean) / std, written to out fp32
 * [n][C][S][S] (channels identical, as the reference's 3-channel repeat).
 * work: n * 1544 bytes of device scratch. */
int vlp_prep_images(int n, const void* src, int src_u8, const long long* off, const int* hw, int S,
                    float mean, float std_, int C, float* out, void* work, void* stream);
/* One resample per sample for RandAffined + RandRotated + RandFlipd + RandZoomd, then
 * RandGaussianNoised: out[b][c] = bilinear(in[b][ci]) at source (row, col) =
 * M_b (p - centre) + centre + t_b (border clamp) + N(0, noise_std[b]);
 * maps[b] = {m00, m01, t0, m10, m11, t1} drawn on the host.  in: fp32 [B][Cin][H][W]
 * (Cin 1 or C), or uint8 [B][1][H][W] normalised on load with (v - mean) / std. */
int vlp_aug_warp(int B, int Cin, int C, int H, int W, const void* in, int in_u8, float mean, float std_,
                 const float* maps, const float* noise_std, unsigned long long seed, float* out,
                 void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VLP_HIP_H */
