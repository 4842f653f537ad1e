/*
 * t2i_hip.h — C ABI of libt2i_hip.so: the MI355X (gfx950) kernels behind the reference's operator surface.
 *
 * The reference (crisbodnar/text-to-image) has no FFI/plugin layer: its operator API is the Python wrappers in
 * utils/ops.py, which hand the arithmetic to TensorFlow-1.4 kernels (Eigen / cuDNN).  This library is what sits
 * under those wrappers instead.  Each entry point cites the reference interface it serves.
 *
 * Conventions (all entry points):
 *   - extern "C"; return 0 on success, a negative T2I_ERR_* otherwise; never throw.  t2i_last_error() gives the
 *     thread-local message of the last failure.
 *   - every pointer is a DEVICE pointer owned by the caller; the library never allocates or frees device memory.
 *     Scratch comes from the caller's workspace (size from the matching *_workspace_bytes query; 256-byte aligned); the
 *     optional transformed-filter cache lives in an arena the caller attaches (t2i_filter_cache_attach).
 *   - tensors are dense NHWC fp32 ("[B,H,W,C]", C fastest); conv filters are TF "HWIO" [KH,KW,Cin,Cout];
 *     dense kernels are [in,out].  No tensor may exceed 2^30-16 elements (4 GiB: buffer addressing).
 *   - every call is asynchronous on the given hipStream_t (void* here so the header needs no HIP include) and is
 *     safe to capture into a hipGraph: no allocation, no synchronisation.  Host-side state is limited to (a) the tuning
 *     switches, read from the T2I_* environment once at first use and changed afterwards only through t2i_tuning_set, and
 *     (b) the bookkeeping (not the storage) of the filter cache, mutex-guarded; the planner never consults the environment
 *     at call time, so equal descriptors take equal paths for the life of the process.  There is NO per-thread hand-over
 *     state: everything a call reads or writes besides its tensors travels in its own arguments (t2i_conv_opts for the
 *     conv family, an explicit image pointer for the elementwise producers) — ABI v5 removed the one-shot "arm the next
 *     call" entry points of v4 (t2i_conv2d_operand_images, t2i_output_image, t2i_conv2d_input_transform, *_written, *_kept).
 */
#ifndef T2I_HIP_H
#define T2I_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T2I_OK 0
#define T2I_ERR_INVALID (-1)   /* bad descriptor / null pointer / unsupported geometry */
#define T2I_ERR_WORKSPACE (-2) /* workspace too small or misaligned */
#define T2I_ERR_LAUNCH (-3)    /* HIP launch failure (message holds hipGetErrorString) */

/* activation fused into an epilogue (reference utils/ops.py `act=` argument; model.py:110,131 lrelu 0.2) */
#define T2I_ACT_NONE 0
#define T2I_ACT_LRELU 1 /* max(x, alpha*x) */
#define T2I_ACT_RELU 2
#define T2I_ACT_TANH 3

typedef void* t2i_stream_t; /* a hipStream_t */

/* Element type of the ACTIVATION tensors of a call (v6).  T2I_DT_F32: dense fp32, the reference's dtype and the default everywhere.
 * T2I_DT_BF16: the tensors are bf16 in memory (BASELINE config 3 end to end: activations and activation gradients travel between
 * kernels as bf16; weights, biases, optimizer state, batch-norm statistics, every reduction result and all accumulators stay
 * fp32).  Entry points with a `dtype` argument read AND write all their activation tensors in that type (pointers are void* for
 * that reason); bf16 tensors need 16-byte aligned pointers and a channel / element count that is a multiple of 4, and there is no
 * separate bf16 twin then (the y_h arguments must be NULL).  Arithmetic is fp32 either way: a bf16 tensor is widened exactly on load
 * and rounded to nearest even on store. */
enum { T2I_DT_F32 = 0, T2I_DT_BF16 = 1 };

/* Geometry of one 2-D convolution, already resolved from the TF padding string (SAME/VALID -> pad_t/pad_l, Ho/Wo):
 * y[b,oh,ow,co] = sum_{kh,kw,ci} x[b, oh*SH-pad_t+kh, ow*SW-pad_l+kw, ci] * w[kh,kw,ci,co]. */
typedef struct t2i_conv_desc {
  int32_t B, H, W, Cin;  /* input  [B,H,W,Cin]   */
  int32_t Ho, Wo, Cout;  /* output [B,Ho,Wo,Cout] */
  int32_t KH, KW, SH, SW;
  int32_t pad_t, pad_l;  /* TF SAME puts the odd pixel bottom/right, so only top/left are needed */
  int32_t math;          /* T2I_MATH_F32 (0): exact fp32 matrix pipe.  T2I_MATH_BF16 (1): operands rounded to bf16 (RNE),
                          * v_mfma_*_bf16 with fp32 accumulation; the tensors at this interface stay fp32 (BASELINE
                          * config 3).  Where the gathered tensor has a multiple of 64 channels the forward conv and the
                          * input gradient first stage bf16 copies of their operands (activation: workspace; filter:
                          * workspace or the filter cache) and run a GEMM whose operands are bf16 in memory; elsewhere
                          * the rounding happens on the way into LDS.  Same arithmetic either way.  The direct kernels for
                          * thin layers (Cin or Cout <= 4, the logit head) compute in fp32 in both modes. */
} t2i_conv_desc;
enum { T2I_MATH_F32 = 0, T2I_MATH_BF16 = 1 };

/* ---- library ------------------------------------------------------------------------------------------------ */
#define T2I_ABI_VERSION 13        /* what t2i_version() returns and what the Python binding, which reads this header, expects */
int t2i_version(void);            /* ABI version, currently 13 (v13: t2i_cosine_distance added, then t2i_bn_infer and t2i_bytescale_nearest (+ workspace query) — no existing signature changed; v12: t2i_pool_dropout, t2i_softmax_ce_head (+ workspace query), t2i_pooled_grad_scatter and t2i_rmsprop_tf added — no existing signature changed; v11: t2i_resample_bilinear, t2i_pool2d, t2i_channel_slice_copy, t2i_gram_accumulate and their workspace queries added — no existing signature changed; v10: t2i_nearest_images and t2i_nearest_images_workspace_bytes added — no existing signature changed; v9: t2i_conv_opts gained xform_valid_rows / xform_plane_rows, t2i_bn_train_fwd_grouped gained moving_groups, t2i_trunc_normal and t2i_zero_ranges added; v8: t2i_sigmoid_ce_head, t2i_bn_train_fwd_grouped, t2i_bn_bwd_grouped, t2i_bn_grouped_workspace_bytes added — no existing signature changed; v7: v7: t2i_conv2d_bwd_pair, t2i_row_scale_div, t2i_stat, t2i_filter_cache_assume added, t2i_adam_tf takes m == NULL at beta1 == 0 — no existing signature changed; v2: t2i_conv_desc.math; v3: caller-owned filter-cache arena,
                                   * t2i_tuning_set, t2i_kt_sgd; v4: t2i_filter_cache_refresh, bf16 operand images; v5: t2i_conv_opts
                                   * and explicit image arguments instead of thread-local one-shot hand-overs; v6: bf16 STORAGE —
                                   * activation tensors may be bf16 at this interface: t2i_dtype arguments, t2i_conv_opts.in_dtype /
                                   * out_dtype) */
const char* t2i_last_error(void); /* thread-local, never NULL */
long long t2i_stat(const char* key); /* process-wide counters for tests / diagnostics: "pair_fused" = t2i_conv2d_bwd_pair calls issued as one launch; -1: unknown key */
/* CU count, clock (kHz) and gcnArchName of `device` into caller buffers; used by bench.py to re-derive peaks. */
int t2i_device_info(int device, int32_t* cu_count, int32_t* clock_khz, char* arch, size_t arch_len);

/* Tuning / diagnostic switch `key` := value (tests, sweeps: tools/sweep_conv.py).  Keys and their T2I_* environment
 * defaults: force_tile (T2I_FORCE_TILE: 22, 21, 12, 11 = 128x128 ... 64x64; 0 = planner), force_splitk, debug_plan, group_n,
 * no_ut, no_thin, winograd, winograd_minc, winograd_maxhw, winograd_k4s2, winograd_k4s2_minc, winograd_k4s2_bwd_minc,
 * winograd_k4s2_bwdf, adam_blocks, max_chain (longest unsplit fp32 reduction chain, default 8192), split_cost, bf16_operands, cache_refresh, thin_parts.
 * Not a hot-path call; changes apply to launches planned afterwards (workspace queries included). */
int t2i_tuning_set(const char* key, double value);

/* ---- convolution family: reference utils/ops.py:58-63 (conv2d) and :66-71 (conv2d_transpose) ------------------ */
size_t t2i_conv2d_workspace_bytes(const t2i_conv_desc* d); /* upper bound for fwd / bwd_data / bwd_filter */

/* Optional side inputs / outputs of ONE conv call (pass NULL for none).  Plain data, owned by the caller, read at entry and
 * written (the two out-flags) before the call returns; the library keeps no pointer to it.  Results of the convolution are
 * identical with and without any of these.
 *   a_image / b_image   bf16 math: bf16 images (same shape and layout, made by t2i_cast_bf16 or written as a twin by the
 *                       producer) of the call's first / second ACTIVATION operand (fwd: x; bwd_data: dy; bwd_filter: x, dy).
 *                       An activation feeds up to three convs of a training step and a gradient two, so the caller that keeps
 *                       the image saves the repeated casts.  Paths that do not read bf16 operands from memory ignore them.
 *   out_image           bf16 math, fwd / fwd_stats / bwd_data: also write the bf16 image of the output tensor here (16-byte
 *                       aligned), in the epilogue's own pass; out_image_written tells whether the path taken did.
 *   xform, xform_bytes, xform_mode
 *                       fp32 Winograd: the forward conv of a layer and its filter gradient transform the same x (V = B^T x B
 *                       per tile, 4x resp. 2.25x the size of x).  T2I_XFORM_KEEP on t2i_conv2d_fwd / _fwd_stats leaves V in
 *                       `xform` (>= t2i_conv2d_input_transform_bytes(d) bytes; xform_kept tells whether the call took a path
 *                       that has one); T2I_XFORM_HAVE on t2i_conv2d_bwd_filter (same d, same unchanged x) reads V from there
 *                       instead of transforming x again; xform_valid_rows (below) restricts what is trusted to the leading images of the
 *                       batch — the stacked critic step (text-to-image_amd/stacked.py) replaces the x_hat rows of a layer's input by
 *                       the gradient penalty's tangent before its ONE filter-gradient launch over all 4B rows.
 *   in_dtype, out_dtype bf16 STORAGE: the activation tensors of the call are bf16 in memory.  The bf16-operand GEMMs and the
 *                       3 -> 128 stem read and write them directly (no cast, no fp32 copy anywhere); the remaining paths (thin /
 *                       head kernels, the generic kernel for channel counts that are not multiples of 64) run on fp32 staging copies
 *                       carved from the workspace — t2i_conv2d_workspace_bytes includes the room for them. */
enum { T2I_XFORM_NONE = 0, T2I_XFORM_KEEP = 1, T2I_XFORM_HAVE = 2 };
typedef struct t2i_conv_opts {
  const void* a_image;
  const void* b_image;
  void* out_image;
  void* xform;
  size_t xform_bytes;
  int32_t xform_mode;
  int32_t out_image_written; /* out */
  int32_t xform_kept;        /* out */
  int32_t in_dtype;          /* bf16 storage (needs math = T2I_MATH_BF16): bit 0 / bit 1 set = the call's first / second ACTIVATION operand
                              * (the pointer argument itself) is a bf16 tensor; a_image / b_image are then not consulted for it */
  int32_t out_dtype;         /* T2I_DT_BF16: the output pointer (y / dx) is a bf16 tensor and is the only thing written */
  int32_t xform_valid_rows;  /* v9, T2I_XFORM_HAVE: `xform` is current for the first xform_valid_rows images of the batch only (the caller
                              * changed the images behind them since the forward conv); t2i_conv2d_bwd_filter regenerates the transform of
                              * the remaining images from x, in place in `xform`.  0 (or >= B): all of it is current.  (v8: `reserved`, 0) */
  int32_t xform_plane_rows;  /* v9, T2I_XFORM_HAVE: `xform` was kept by the forward conv of a LARGER batch of that many images whose leading B
                              * images are this call's x (a stacked pass of which only the leading part is differentiated).  0: the batch is d->B.
                              * Honoured by the 3x3 Winograd form; other forms transform x anew. */
  int32_t reserved;
} t2i_conv_opts;
size_t t2i_conv2d_input_transform_bytes(const t2i_conv_desc* d);   /* > 0: fwd and bwd_filter of `d` both take a Winograd path */

/* y = act(conv(x, w) + bias).  bias may be NULL.  Serves ops.conv2d (utils/ops.py:58-63), ops.fc as a 1x1 conv on
 * [B,1,1,in] (utils/ops.py:84-87), and the double-backward term adj_gy = conv(ggx, w) of the gradient penalty. */
int t2i_conv2d_fwd(const t2i_conv_desc* d, const void* x, const float* w, const float* bias, void* y, int act,
                   float alpha, t2i_conv_opts* opts, void* ws, size_t ws_bytes, t2i_stream_t stream);

/* t2i_conv2d_fwd that also hands the batch norm behind it its statistics: if the launch takes the unsplit path,
 * *chunks = number of M-tiles, *tile_rows = their height and stats = [2][chunks][Cout]: per tile the column sums of y and
 * the second moment of y ABOUT THE TILE'S OWN MEAN (finish with t2i_bn_stats_tiles(stats, stats + chunks*Cout, chunks,
 * tile_rows, B*Ho*Wo, Cout, sum, m2, ...)); otherwise *chunks = 0 and the caller computes the statistics itself
 * (t2i_bn_stats).  stats must hold t2i_conv2d_stats_bytes(d). */
size_t t2i_conv2d_stats_bytes(const t2i_conv_desc* d);
int t2i_conv2d_fwd_stats(const t2i_conv_desc* d, const void* x, const float* w, const float* bias, void* y, int act,
                         float alpha, float* stats, size_t stats_bytes, int32_t* chunks, int32_t* tile_rows, t2i_conv_opts* opts,
                         void* ws, size_t ws_bytes, t2i_stream_t stream);

/* dx = conv^T(dy, w) (+ bias over Cin if non-NULL, then act).  This IS ops.conv2d_transpose (utils/ops.py:66-71):
 * TF stores the deconv filter as [KH,KW,Cout_deconv,Cin_deconv], i.e. the HWIO filter of the adjoint conv, so the
 * descriptor is that adjoint conv's (d->Cin = deconv output channels) and no re-layout is needed. */
int t2i_conv2d_bwd_data(const t2i_conv_desc* d, const void* dy, const float* w, const float* bias, void* dx,
                        int act, float alpha, t2i_conv_opts* opts, void* ws, size_t ws_bytes, t2i_stream_t stream);

/* dw = x (*) dy over all B*Ho*Wo positions (tf.gradients wrt `weights`, reference models/wgancls/model.py:94-106);
 * accumulate != 0: dw += x (*) dy in the epilogue, i.e. the gradient is summed straight into the optimizer's arena. */
int t2i_conv2d_bwd_filter(const t2i_conv_desc* d, const void* x, const void* dy, float* dw, int accumulate,
                          t2i_conv_opts* opts, void* ws, size_t ws_bytes, t2i_stream_t stream);

/* One layer's backward on bf16 tensors in (possibly) ONE launch (v7).  In tf.gradients' walk of the reference graph
 * (models/wgancls/model.py:94-106) every conv2d (utils/ops.py:58-63) contributes an input gradient conv^T(g, w) AND a filter
 * gradient x (*) g, every conv2d_transpose (utils/ops.py:66-71) contributes conv(g, w) AND a filter gradient g (*) saved dy: two
 * independent GEMMs on the same incoming gradient.  first = T2I_PAIR_BWD_DATA: out1 = conv^T(g, w);  T2I_PAIR_FWD: out1 = conv(g, w)
 * (no bias, no activation);  then dw = fx (*) fdy (accumulate != 0: dw += ...).  The results are the SAME SUMS as those of
 * t2i_conv2d_bwd_data / t2i_conv2d_fwd followed by t2i_conv2d_bwd_filter with the same opts (same operand rounding, same fp32
 * accumulation inside a K range) but not necessarily the same bits: a shared launch plans each GEMM for its share of the chip
 * (tuning pair_cus, default half), which may choose another split-K grouping, i.e. another order of the fp32 partial sums
 * (tests/test_storage_gpu.py bounds the difference at the fp32 GEMM tolerance).  Hence bf16-storage results depend on whether the
 * pair path is taken (kernels.pair_calls, and autograd takes it only on one stream): runs are bit-reproducible for a FIXED
 * setting, the side-stream / pair toggles are not bit-neutral in bf16.  Where both GEMMs run on the
 * bf16-operand kernels they share one launch (a B = 64 layer leaves each of them one workgroup per CU; two streams of a captured
 * graph do not overlap on this stack).  opts1 (in_dtype bit 0: g, out_dtype: out1) and opts2 (bit 0: fx, bit 1: fdy) are
 * required; ws1 / ws2 (each t2i_conv2d_workspace_bytes(d)) are in use at the same time and must not overlap. */
enum { T2I_PAIR_FWD = 0, T2I_PAIR_BWD_DATA = 1 };
int t2i_conv2d_bwd_pair(const t2i_conv_desc* d, int first, const void* g, const float* w, void* out1, t2i_conv_opts* opts1,
                        const void* fx, const void* fdy, float* dw, int accumulate, t2i_conv_opts* opts2,
                        void* ws1, size_t ws1_bytes, void* ws2, size_t ws2_bytes, t2i_stream_t stream);

/* ---- column reductions over a [rows, C] view ------------------------------------------------------------------ */
size_t t2i_col_reduce_workspace_bytes(int64_t rows, int32_t C);
/* out0[c] = sum_r a[r,c];  out1[c] = sum_r a[r,c]*(b[r,c] - center[c])  (b == NULL -> a*a; center == NULL -> 0;
 * out1 == NULL -> skipped).  Bias gradients (db = colsum(dy)) and the batch-norm backward sums (sum dy, sum dy*(x - mean):
 * centred inside the reduction — sum(dy*x) - mean*sum(dy) would cancel). */
int t2i_col_reduce(const void* a, const void* b, const float* center, int64_t rows, int32_t C, float* out0, float* out1,
                   int accumulate, void* ws, size_t ws_bytes, int32_t dtype /* of a and b */,
                   t2i_stream_t stream); /* accumulate != 0: out += (gradient arena) */

/* ---- batch norm, training mode: reference utils/ops.py:7-29 (tf.contrib.layers.batch_norm fused, scale=True) --- */
/* Second stage alone: out0[c] = sum_k part0[k*C + c] (k < chunks, fixed order), same for part1/out1 when given. */
int t2i_col_reduce_partials(const float* part0, const float* part1, int32_t chunks, int32_t C, float* out0, float* out1,
                            int accumulate, t2i_stream_t stream);
/* Batch statistics of x [rows, C], numerically stable: sum[c] = sum_r x[r,c] and m2[c] = sum_r (x[r,c] - mean[c])^2, from
 * per-chunk moments about a sample of the chunk merged with Chan's update — NOT from sum(x^2) - sum(x)^2/n, which loses the
 * variance to cancellation when |mean| >> std (a rank-2 batch norm over a batch of 2; deep batch-normed stacks at batch 2).
 * Workspace as t2i_col_reduce.  t2i_bn_stats_tiles: the same from the per-tile partials of t2i_conv2d_fwd_stats. */
int t2i_bn_stats(const float* x, int64_t rows, int32_t C, float* sum, float* m2, void* ws, size_t ws_bytes, t2i_stream_t stream);
int t2i_bn_stats_tiles(const float* part_sum, const float* part_m2, int32_t chunks, int32_t tile_rows, int64_t rows, int32_t C,
                       float* sum, float* m2, t2i_stream_t stream);
/* Statistics AND the finalize step in one chain (stage 1 + one stage-2 launch): exactly one of x (the tensor, [rows, C];
 * workspace as t2i_col_reduce) or the tile partials of t2i_conv2d_fwd_stats (part_sum / part_m2 / chunks / tile_rows;
 * chunks = ceil(rows / tile_rows) as for t2i_bn_stats_tiles, anything else is refused).
 * Outputs as t2i_bn_finalize.  What the training-mode batch norm of utils/ops.py:7-29 launches in front of t2i_bn_apply. */
int t2i_bn_train_fwd_stats(const void* x, const float* part_sum, const float* part_m2, int32_t chunks, int32_t tile_rows, int64_t rows,
                           int32_t C, const float* gamma, const float* beta, float eps, float decay, float* mean, float* rstd,
                           float* scale, float* shift, float* moving_mean, float* moving_var, void* ws, size_t ws_bytes,
                           int32_t dtype /* of x */, t2i_stream_t stream);
/* From sum and the centred second moment m2 over n rows: mean, rstd = 1/sqrt(m2/n + eps) (biased variance);
 * scale = gamma*rstd, shift = beta-mean*scale; and, if moving_mean != NULL,
 * moving = decay*moving + (1-decay)*{mean, var_biased*n/(n-1)} in place. */
int t2i_bn_finalize(const float* sum, const float* m2, int64_t n, int32_t C, const float* gamma,
                    const float* beta, float eps, float decay, float* mean, float* rstd, float* scale, float* shift,
                    float* moving_mean, float* moving_var, t2i_stream_t stream);
/* y = act(x*scale[c] + shift[c])  (normalise + affine + activation in one pass; also eval-mode BN).
 * y_h (here and in t2i_bn_bwd_fused, t2i_act_fwd, t2i_act_bwd, t2i_act_bwd_colsum, t2i_add_act): NULL, or a buffer that receives
 * the bf16 image (round to nearest even) of the output tensor in the same pass — the "twin" a bf16-math conv reading that
 * tensor next takes as its operand image (t2i_conv_opts.a_image), so that no cast launch is needed.  Requires the vectorised
 * path: every tensor and y_h 16-byte aligned and C % 4 == 0 (n % 4 == 0); otherwise the call fails with T2I_ERR_INVALID
 * instead of silently not writing it. */
int t2i_bn_apply(const void* x, const float* scale, const float* shift, int64_t rows, int32_t C, int act,
                 float alpha, void* y, void* y_h, int32_t dtype, t2i_stream_t stream);
/* Inference batch norm in one launch: y = res_act(residual + act(x*scale[c] + shift[c])) over x [rows, C], with
 * scale = gamma / sqrt(moving_variance + eps) and shift = beta - moving_mean * scale formed inside the kernel from the four [C]
 * vectors (any C: the channels are tiled).  residual: NULL, or a tensor of x's shape and dtype — then res_act is applied to the
 * sum (the closing join of a residual block); without it res_act / res_alpha are ignored.  dtype: x, residual and y are fp32 or
 * bf16 tensors (bf16: 16-byte aligned, C % 4 == 0).  16-byte accesses when C % 4 == 0 and the tensors are 16-byte aligned, a
 * scalar form otherwise.  Added within ABI v13: no existing argument list changed. */
int t2i_bn_infer(const void* x, const float* gamma, const float* beta, const float* moving_mean, const float* moving_variance, float eps,
                 int64_t rows, int32_t C, int act, float alpha, const void* residual, int res_act, float res_alpha, void* y, int32_t dtype,
                 t2i_stream_t stream);
/* dx = gamma*rstd*(dy - sum_dy/n - xhat*sum_dy_xhat/n), xhat = (x-mean)*rstd, sum_dy_xhat = rstd * sum_dy_x with
 * sum_dy_x = sum dy*(x - mean) (t2i_col_reduce / t2i_act_bwd_colsum with center = mean).  Also emits dgamma, dbeta. */
int t2i_bn_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
               const float* sum_dy, const float* sum_dy_x, int64_t rows, int32_t C, float* dx, float* dgamma,
               float* dbeta, int accumulate /* dgamma/dbeta += */, void* ws /* >= 3*C floats */, size_t ws_bytes,
               t2i_stream_t stream);

/* The whole training-mode batch-norm backward in three launches: [g = dy*act'(y) and the reductions sum g, sum g*(x - mean),
 * stage 1] -> [stage 2 + dgamma/dbeta + the coefficients of dx] -> [dx = k_dy*g + k_x*x + k_0].  y == NULL: no activation
 * behind the batch norm (g = dy, gmask unused).  gmask: caller's [rows, C] buffer for g.  C % 4 == 0, 16-byte alignment. */
size_t t2i_bn_bwd_fused_workspace_bytes(int64_t rows, int32_t C);
int t2i_bn_bwd_fused(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, const float* gamma, int64_t rows,
                     int32_t C, int act, float alpha, void* gmask, void* dx, void* dx_h, float* dgamma, float* dbeta, int accumulate, void* ws,
                     size_t ws_bytes, int32_t dtype /* of dy, y, x, gmask, dx */, t2i_stream_t stream);

/* Batch norm of a STACKED batch (v8).  The reference evaluates its batch-normalised critic three times per sess.run with shared variables
 * (models/gancls/model.py:48-51: fake / match / mismatch images; models/stackgan/stageI/model.py:44-48): convolutions, activations and the text
 * projection are per-sample, so the three passes can run as ONE batch of groups * B samples — except batch norm, which must keep each pass's own
 * statistics.  x is [groups * rows_per_group, C], group g = rows [g * rows_per_group, (g + 1) * rows_per_group) (contiguous: the batch axis is the
 * slowest).  Forward: statistics per group (mean / rstd / scale / shift are [groups][C]), moving averages updated once per group in group order
 * (what `groups` sequential passes do), y = act(x * scale_g + shift_g) — three launches for all groups.  Backward: dx with the group's own
 * statistics, dgamma / dbeta summed over the groups (accumulate != 0: += into the arena slots) — three launches.  groups = 1 is the ordinary
 * training-mode batch norm.  C % 4 == 0, 16-byte aligned tensors; ws >= t2i_bn_grouped_workspace_bytes(...) for either call.
 * tile_sum / tile_m2 (optional): the per-tile partials the producing conv's epilogue left (t2i_conv2d_fwd_stats: tile_chunks tiles of tile_rows rows
 * per group) — the statistics' first pass over x is then skipped.  With at most 64 partial rows per column and group the second stage runs in the
 * prologue of the normalisation / dx kernel (two launches, one with tile partials; T2I_BN_FUSE=0: always three).
 * moving_groups (v9; 0 = all): only the first moving_groups groups move the moving averages — a stacked pass whose later groups are evaluations
 * outside UPDATE_OPS (the generator's critic-step evaluation stacked behind its generator-step evaluation).
 * moving_updates (>= 1): how many sequential exponential-average steps the moving statistics take with this batch's statistics per group — 2 when
 * ONE evaluation of a network stands for two identical evaluations of the reference graph (gancls: the generator in the D run and in the G run of
 * one iteration, models/gancls/trainer.py:115-134: same feed, no noise, weights unchanged in between; both runs sit under UPDATE_OPS). */
size_t t2i_bn_grouped_workspace_bytes(int64_t rows_per_group, int32_t C, int32_t groups);
int t2i_bn_train_fwd_grouped(const void* x, int64_t rows_per_group, int32_t C, int32_t groups, const float* gamma, const float* beta, float eps,
                             float decay, float* mean, float* rstd, float* scale, float* shift, float* moving_mean, float* moving_var, int act,
                             float alpha, void* y, void* y_h, const float* tile_sum, const float* tile_m2, int32_t tile_chunks, int32_t tile_rows,
                             int32_t moving_updates, int32_t moving_groups, void* ws, size_t ws_bytes, int32_t dtype, t2i_stream_t stream);
int t2i_bn_bwd_grouped(const void* dy, const void* y, const void* x, const float* mean, const float* rstd, const float* gamma, int64_t rows_per_group,
                       int32_t C, int32_t groups, int act, float alpha, void* gmask, void* dx, void* dx_h, float* dgamma, float* dbeta, int accumulate,
                       void* ws, size_t ws_bytes, int32_t dtype, t2i_stream_t stream);

/* ---- elementwise ----------------------------------------------------------------------------------------------- */
/* y = act(x) */
int t2i_act_fwd(const void* x, int64_t n, int act, float alpha, void* y, void* y_h, int32_t dtype, t2i_stream_t stream);
/* dx = dy * act'(.) with the derivative taken from the OUTPUT y (lrelu/relu are sign preserving, tanh' = 1-y^2). */
int t2i_act_bwd(const void* dy, const void* y, int64_t n, int act, float alpha, void* dx, void* dx_h, int32_t dtype, t2i_stream_t stream);
/* Fused activation backward + column sums: dx = dy * act'(y), colsum[c] = sum_r dx[r,c] and, if x2 != NULL,
 * colsum_x2[c] = sum_r dx[r,c]*(x2[r,c] - center[c]) (center NULL = 0), in ONE pass over a [rows, C] view (C % 4 == 0,
 * 16-byte aligned).  Serves the bias gradient of a conv layer and the two reductions of the batch-norm backward (x2 = the
 * layer input, center = its batch mean).  accumulate: sums are added to the outputs.  Workspace as t2i_col_reduce. */
int t2i_act_bwd_colsum(const void* dy, const void* y, const void* x2, const float* center, int64_t rows, int32_t C, int act,
                       float alpha, void* dx, void* dx_h, float* colsum, float* colsum_x2, int accumulate, void* ws, size_t ws_bytes,
                       int32_t dtype, t2i_stream_t stream);
/* y = act(a + b): residual joins (reference models/wgancls/model.py:145-146, 190-191, 206-207). */
int t2i_add_act(const void* a, const void* b, int64_t n, int act, float alpha, void* y, void* y_h, int32_t dtype, t2i_stream_t stream);
/* y = alpha*a + beta*b (b may be NULL). */
int t2i_axpby(const void* a, float alpha, const void* b, float beta, int64_t n, void* y, int32_t dtype, t2i_stream_t stream);
/* x_hat[b,:] = eps[b]*g[b,:] + (1-eps[b])*x[b,:]   (reference models/wgancls/model.py:53). */
int t2i_interp(const float* eps, const float* g, const float* x, int32_t B, int64_t per_sample, float* xhat,
               t2i_stream_t stream);
/* out[b,p,:] = concat(feat[b,p,:Cf], emb[b,:Ce]) for p < P: tile the compressed text embedding over the 4x4 map
 * and concatenate on channels (reference models/wgancls/model.py:153-155).  bwd splits the gradient back. */
int t2i_concat_tile_fwd(const void* feat, const void* emb, int32_t B, int32_t P, int32_t Cf, int32_t Ce,
                        void* out, int32_t dtype, t2i_stream_t stream);
int t2i_concat_tile_bwd(const void* dout, int32_t B, int32_t P, int32_t Cf, int32_t Ce, void* dfeat, void* demb,
                        int32_t dtype, t2i_stream_t stream);
/* NCHW <-> NHWC physical transposes: reference utils/ops.py:129-134 (to_nchw / to_nhwc) and the dense_2 reshape. */
int t2i_nchw_to_nhwc(const void* x, int32_t B, int32_t C, int32_t HW, void* y, int32_t dtype, t2i_stream_t stream);
int t2i_nhwc_to_nchw(const void* x, int32_t B, int32_t C, int32_t HW, void* y, int32_t dtype, t2i_stream_t stream);

/* ---- gradient penalty: reference models/wgancls/model.py:62-70 -------------------------------------------------- */
/* slopes[b] = sqrt(sum_j g[b,j]^2); one wavefront-shuffle reduction per sample. */
int t2i_gp_slopes(const void* g, int32_t B, int64_t per_sample, float* slopes, int32_t dtype, t2i_stream_t stream);
/* out[b,:] = coef[b] * g[b,:]  (per-sample scaling: backward of the slope norm, and its own double backward). */
int t2i_row_scale(const void* g, const float* coef, int32_t B, int64_t per_sample, void* out, int32_t dtype, t2i_stream_t stream);
/* out[b,:] = (den[b] > 0 ? num[b] / max(den[b], 1e-30) : 0) * g[b,:]: the slope norm's backward with its coefficient d / ||g_b|| formed
 * in the kernel (v7; tf.gradients of tf.sqrt(tf.reduce_sum(tf.square(.))), model.py:64,69). */
int t2i_row_scale_div(const void* g, const float* num, const float* den, int32_t B, int64_t per_sample, void* out, int32_t dtype, t2i_stream_t stream);

/* ---- loss heads: reference models/wgancls/model.py:72-92 (critic losses) and :117-127 (conditioning augmentation) --- */
/* From the critic's 3B logits (fake | real | mismatch, each B) and the two per-sample slope vectors: the loss scalars
 *   scalars[0..11] = D_loss, D_loss_real, D_loss_fake, D_loss_mismatch, wdist, wdist2, real_gp, real_gp2, reg_loss,
 *                    balance_loss, d balance_loss / d kt, kt
 * with D_loss = -wdist - kt*wdist2 + gp_coeff*(real_gp + real_gp2), real_gp = mean(max(0, slope-1)^2), and the seeds
 * of the backward pass dD_loss/dlogits [3B], dD_loss/dslopes1 [B], dD_loss/dslopes2 [B].  kt_dev: device scalar, or NULL
 * for kt = 1 (models/pggan/pggan.py:104).  One workgroup; replaces ~40 elementwise launches. */
int t2i_wgan_d_head(const float* logits, const float* slopes1, const float* slopes2, const float* kt_dev, int32_t B,
                    float gp_coeff, float* seed_logits, float* seed_slopes1, float* seed_slopes2, float* scalars,
                    t2i_stream_t stream);
/* Sigmoid cross-entropy heads: reference models/gancls/trainer.py:20-34 (tf.nn.sigmoid_cross_entropy_with_logits on the critic's fake /
 * match / mismatch logits with constant labels 0 / 0.9 / 0, weighted 1-alpha / 1 / alpha; G_loss with label 1) and
 * models/stackgan/stageI/trainer.py:53-77.  For each head k < 3 with logits l_k[B] (l1, l2 may be NULL):
 *   losses[1+k] = mean_i [max(l,0) - l y_k + log1p(exp(-|l|))],  losses[0] = sum_k w_k losses[1+k],
 *   seed_k[i] = w_k (sigmoid(l) - y_k) / B  (= d losses[0] / d l_k[i]),  prob_k[i] = sigmoid(l)   (seed_k / prob_k may be NULL).
 * One workgroup; replaces ~25 elementwise / reduction launches per set of heads. */
int t2i_sigmoid_ce_head(const float* l0, const float* l1, const float* l2, float y0, float y1, float y2, float w0, float w1, float w2, int32_t B,
                        float* seed0, float* seed1, float* seed2, float* prob0, float* prob1, float* prob2, float* losses, t2i_stream_t stream);
/* code = mean + exp(log_sigma)*eps (eps: the truncated-normal draw) and kl[0] = mean(-ls + .5(-1 + exp(2 ls) + mean^2))
 * over the n = B*D elements; bwd: dmean = dcode + dkl/n * mean, dlog_sigma = dcode*eps*exp(ls) + dkl/n * (exp(2 ls) - 1)
 * (dcode and/or dkl may be NULL = zero). */
int t2i_ca_kl_fwd(const float* mean, const float* log_sigma, const float* eps, int64_t n, float* code, float* kl, t2i_stream_t stream);
int t2i_ca_kl_bwd(const float* mean, const float* log_sigma, const float* eps, const float* dcode, const float* dkl, int64_t n,
                  float* dmean, float* dlog_sigma, t2i_stream_t stream);

/* ---- optimizer: tf.train.AdamOptimizer as used at reference models/wgancls/model.py:94-106 ---------------------- */
/* m = b1*m+(1-b1)*g; v = b2*v+(1-b2)*g*g; w -= lr_t*m/(sqrt(v)+eps), lr_t = lr*sqrt(1-b2^t)/(1-b1^t) computed by the
 * caller (epsilon outside the bias correction).  One launch over a flat parameter arena. grad_scale multiplies g
 * first (1/world_size for summed data-parallel gradients).  If lr_t_dev != NULL the step size is read from that device
 * scalar instead of lr_t, so a hipGraph that captured the launch can be replayed with the next step's bias correction.
 * m may be NULL when beta1 == 0 (v7): m_t = g_t * grad_scale whatever m_{t-1} was, so it is neither read nor written. */
int t2i_adam_tf(float* w, const float* g, float* m, float* v, int64_t n, float lr_t, const float* lr_t_dev, float beta1,
                float beta2, float eps, float grad_scale, t2i_stream_t stream);
/* t2i_adam_tf plus tf.train.ExponentialMovingAverage of the updated weights, in the same launch (v13, added without a version
 * change: no existing argument list moved).  w, m, v after the call are bit for bit what t2i_adam_tf writes from the same inputs
 * (the three Adam entries launch instantiations of one kernel template, whose update statements are written once);
 * then, per element, in fp32 and without fma contraction,
 *   omd = 1 - decay;  ema = ema - omd * (ema - w_new)
 * so the shadow equals a step-by-step fp32 restatement on the host bit for bit.  decay is read from *ema_decay_dev when that
 * pointer is non-NULL (as lr_t_dev: a captured launch replays with a changed decay), else it is ema_decay, which must lie in
 * [0, 1].  ema: n floats, 16-byte aligned, overlapping none of w, g, m, v.  Everything t2i_adam_tf refuses is refused here, and
 * every refusal returns T2I_ERR_INVALID before any launch.  Enqueues one kernel on `stream`, allocates and synchronises nothing,
 * graph-capturable; treats the filter cache as t2i_adam_tf does for the arena it updates (the tuning key cache_refresh included).
 * The shadow is not filter memory to the cache: whoever copies it into an arena is a writer of filter memory like any other. */
int t2i_adam_tf_ema(float* w, const float* g, float* m, float* v, float* ema, int64_t n, float lr_t, const float* lr_t_dev,
                    float beta1, float beta2, float eps, float grad_scale, float ema_decay, const float* ema_decay_dev,
                    t2i_stream_t stream);
/* The same update with two multipliers per arena slot (v13, added without a version change): the arena is a sequence of n_slots
 * slots, slot s ending (exclusive, in elements) at slot_end_dev[s]; per slot, two fp32 products are formed once,
 *   gs = grad_scale * slot_mult_dev[2 s]       lr_s = lr_t * slot_mult_dev[2 s + 1]
 * and the slot's elements are updated by t2i_adam_tf's statements with gs in place of grad_scale and lr_s in place of lr_t.  With
 * every multiplier 1.0f the result is bit for bit t2i_adam_tf's (t2i_adam_tf_ema's with a shadow); with a general table it is bit
 * for bit one such launch per slot that is handed those two products.  Training w-hat ~ N(0, 1) with Adam and using c * w-hat (the
 * equalized learning rate) is Adam on w = c * w-hat with (grad_mult, lr_mult) = (c, c); a per-layer learning rate is (1, k).
 * ema: NULL for no shadow, else t2i_adam_tf_ema's shadow with ema_decay / ema_decay_dev (both ignored when ema is NULL).
 * n: a positive multiple of 4.  slot_end_dev: device int64[n_slots], 8-byte aligned, ascending, each a multiple of 4 (a float4
 * lies in one slot), the last equal to n.  slot_mult_dev: device float[2 n_slots].  1 <= n_slots <= T2I_ADAM_MAX_SLOTS (the
 * table is staged in LDS, 16 bytes per slot).  The tables only select multipliers: whatever they hold, no address is formed
 * from them and the kernel stays inside the arenas; elements past the last slot end use the last slot's multipliers.  Neither
 * table may overlap an arena.  Everything t2i_adam_tf_ema refuses is refused here in the same form (T2I_ERR_INVALID before any
 * launch, no buffer touched); graph-capturable; the filter cache is treated as by t2i_adam_tf. */
#define T2I_ADAM_MAX_SLOTS 2048
int t2i_adam_tf_slots(float* w, const float* g, float* m, float* v, float* ema, int64_t n, const int64_t* slot_end_dev,
                      const float* slot_mult_dev, int32_t n_slots, float lr_t, const float* lr_t_dev, float beta1, float beta2,
                      float eps, float grad_scale, float ema_decay, const float* ema_decay_dev, t2i_stream_t stream);

/* kt <- kt - lr * 2 (kt*wd2 - wd) * wd2, the SGD step on balance_loss = (kt*wdist2 - wdist)^2 (reference
 * models/wgancls/model.py:85,100: GradientDescentOptimizer(0.001) minimising balance_loss over kt).  wdist_sums = device
 * [2] holding wdist and wdist2 SUMMED over the data-parallel ranks (each rank's value being its batch mean) and
 * scale = 1/ranks, so that wd, wd2 are the global-batch means (the loss is quadratic in them: averaging per-rank
 * gradients would not be its gradient).  Single rank: the two means and scale = 1. */
int t2i_kt_sgd(float* kt, const float* wdist_sums, float scale, float lr, t2i_stream_t stream);
/* v9.  base[start_r + i] = 0 for every range r < n of the DEVICE table ranges[n][2] = (start, length) in elements: the small slots of a gradient arena
 * whose large filter slots take their first contribution of a step as a plain store (accumulate = 0) and therefore need no zero-fill. */
int t2i_zero_ranges(float* base, const int64_t* ranges, int32_t n, t2i_stream_t stream);
/* v9.  out[i] = mean + std * t_i, t_i ~ N(0, 1) truncated to [lo, hi] (tf.truncated_normal: reference models/wgancls/model.py:119, the
 * conditioning-augmentation noise redrawn on every run), by CDF inversion of Philox4x32-10 uniforms keyed by (seed, offset + i / 4): the
 * draw is a pure function of (seed, offset, i).  The caller advances offset by (n + 3) / 4 per call.  One launch (the tensor library's
 * trunc_normal_ is eight). */
int t2i_trunc_normal(float* out, int64_t n, uint64_t seed, uint64_t offset, float mean, float std, float lo, float hi, t2i_stream_t stream);

/* ---- PGGAN operators: reference utils/ops.py:74-81 (layer_norm), :100-101 (pool), :109-111 (upscale) ------------ */
/* y[b,h,w,:] = scale * sum of the 2x2 window of x [B,H,W,C] (H, W even) -> [B,H/2,W/2,C].  scale = 1/4 is
 * ops.pool(x, 2) (AVG, SAME, even extents); scale = 1 is the backward of t2i_upscale2. */
int t2i_pool2_sum(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, float scale, float* y, t2i_stream_t stream);
/* y[b,2h+i,2w+j,:] = scale * x[b,h,w,:]: ops.upscale(x, 2) (nearest neighbour) for scale = 1; scale = 1/4 is the
 * backward of the average pool. */
int t2i_upscale2(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, float scale, float* y, t2i_stream_t stream);
/* s1[b] = sum_i a[b,i]; s2[b] = sum_i a[b,i]*b[b,i] (b = a when NULL): the per-sample moments of layer norm. */
size_t t2i_row_moments_workspace_bytes(int32_t B);
int t2i_row_moments(const float* a, const float* b, int32_t B, int64_t per_sample, float* s1, float* s2, void* ws,
                    size_t ws_bytes, t2i_stream_t stream);
/* out[b,i] = a[b,i]*alpha[b] + b[b,i]*gamma[b] + delta[b]  (b/gamma and delta optional): layer-norm normalise and its
 * backward. */
int t2i_row_fma2(const float* a, const float* b, const float* alpha, const float* gamma, const float* delta, int32_t B,
                 int64_t per_sample, float* out, t2i_stream_t stream);

/* Fade-in mix with the weight t in device memory (reference models/pggan/pggan.py:267,314 reads the `alpha_tra` variable):
 * mode 0: out = (1-t)*a + t*b;  mode 1: out = t*a;  mode 2: out = (1-t)*a  (modes 1, 2 = the backward of mode 0). */
int t2i_lerp_dev(const float* a, const float* b, const float* t_dev, int32_t mode, int64_t n, float* out, t2i_stream_t stream);

/* Which algorithm the three conv entry points pick for this descriptor (which: 0 = t2i_conv2d_fwd, 1 = t2i_conv2d_bwd_data,
 * 2 = t2i_conv2d_bwd_filter), assuming 16-byte aligned tensors.  For tests, benchmarks and roofline accounting: the
 * Winograd paths execute 1/2.25 (F(2x2,3x3)) resp. 9/16 (F(2x2,2x2), 4x4 stride 2) of the direct convolution's
 * multiply-adds.  Returns -1 for an invalid descriptor. */
enum {
  T2I_ALGO_IMPLICIT_GEMM = 0,        /* igemm_kernel on the direct convolution */
  T2I_ALGO_WINOGRAD_F2X2_3X3 = 1,    /* 3x3 stride 1: transforms + 16 batched GEMMs */
  T2I_ALGO_WINOGRAD_F2X2_2X2 = 2,    /* 4x4 stride 2: space-to-depth / per-phase F(2x2,2x2), 9 or 36 batched GEMMs */
  T2I_ALGO_DIRECT_SMALL = 3,         /* thin / tiny / head kernels of the 3-channel and 1-output layers */
  T2I_ALGO_IMPLICIT_GEMM_BF16_OPERANDS = 4 /* math = BF16, gathered channels % 64 == 0 (fwd, bwd_data): the gathered tensor and
                                      * the filter are first copied to bf16 (workspace / filter cache), then igemm_h_kernel */
};
int t2i_conv2d_algo(const t2i_conv_desc* d, int32_t which);

/* ---- transformed-filter cache (optional) -------------------------------------------------------------------------
 * The Winograd paths of the three conv entry points transform the filter (U = G g G^T) on every call.  A training step
 * uses each critic filter in up to six convs between two optimizer updates; with the cache on, the transform is kept in
 * a slot of a CALLER-OWNED arena, keyed by (filter pointer, transform kind, Cin, Cout), and reused until the filter changes.
 * t2i_filter_cache_attach(buf, bytes) hands the library that arena (device memory, 16-byte aligned, on the device the
 * convs run on); slots are carved from it in order and never moved; when it is full, further filters are simply
 * transformed per call.  attach(NULL, 0) detaches (all entries dropped); the caller frees the arena only after that and
 * after every graph captured with the cache on has been destroyed.  The wgancls step at the reference's widths needs 0.65 GB.
 * CONTRACT when enabled: filter memory may be modified only by t2i_adam_tf (which drops the entries of the arena it
 * updates) or must be followed by t2i_filter_cache_invalidate(ptr, bytes) (ptr NULL = everything) — this includes
 * initialisation, checkpoint loads, broadcasts, and replaying a captured graph that contains t2i_adam_tf from a process
 * that also issues eager convs.  Launches captured into a hipGraph reuse only transforms filled in the same capture, so a
 * graph always contains every transform it depends on; an image filled lazily by one captured stream is not handed to another
 * stream of the same capture (no dependency between them) — only images regenerated by t2i_filter_cache_refresh, which must be
 * issued before the capture's streams fork, are shared across its streams.  Results are bit-identical with and without the cache.  Off by
 * default; t2i_filter_cache_enable returns the previous state. */
int t2i_filter_cache_attach(void* buf, size_t bytes);
int t2i_filter_cache_enable(int on);
void t2i_filter_cache_invalidate(const void* ptr, size_t bytes);
size_t t2i_filter_cache_bytes(void);            /* bytes of the attached arena handed out so far */
/* Regenerates, in ONE launch per 80 entries, every cached image whose filter lies inside [ptr, ptr + bytes) (ptr NULL: all —
 * only if every filter the cache has ever seen is still allocated: entries outlive their filters) and is
 * stale in the launch context of `stream` (eager, or the capture active on it), and marks it filled for that context.
 * Call it behind t2i_adam_tf for the arena it updated (or set the tuning key cache_refresh = 1 and t2i_adam_tf does), and at
 * the head of a capture with (NULL, 0): an iteration then holds one batched regeneration per optimizer step instead of one
 * small fill per (filter, kind) at its first use — ~60 launches.  The bytes moved are the same as with lazy fills as long as
 * an image is not regenerated twice between two updates of its filter. */
int t2i_filter_cache_refresh(const void* ptr, size_t bytes, t2i_stream_t stream);
/* v7: marks every cached image whose filter lies inside [ptr, ptr + bytes) as filled for the launch context of `stream` WITHOUT
 * regenerating it — the caller's promise that, whenever the work issued (or captured) after this call runs, the images in the
 * cache arena are those of the current filters.  For a captured iteration that regenerates an arena's images behind its own
 * t2i_adam_tf (mid-graph t2i_filter_cache_refresh): every replay then finds them as the previous replay left them, and the
 * regeneration at the head of the graph (one read of every filter per iteration) is redundant.  The caller must regenerate
 * them eagerly (t2i_filter_cache_refresh outside the capture, same stream as the replay) before the first replay and after any
 * other writer touched the filters (the writers that must call t2i_filter_cache_invalidate).  Launches nothing. */
int t2i_filter_cache_assume(const void* ptr, size_t bytes, t2i_stream_t stream);

/* ---- bf16 operand images (T2I_MATH_BF16) --------------------------------------------------------------------------
 * out[i] = bf16(x[i]), round to nearest even; n % 8 == 0, both buffers 16-byte aligned.  The image of an activation tensor
 * is handed to the convs that read it through t2i_conv_opts.a_image / b_image. */
int t2i_cast_bf16(const float* x, int64_t n, void* out, t2i_stream_t stream);
/* out[i] = float(x[i]) for a bf16 tensor x (exact widening; any n and alignment): a bf16 activation handed to fp32 code. */
int t2i_cast_f32(const void* x_bf16, int64_t n, float* out, t2i_stream_t stream);
/* 0 for an eager stream, else a number unique to the capture active on `stream`: a caller that keeps bf16 images (or any
 * derived buffer) across calls must not let a capture reuse one made outside it — the graph would not contain its producer. */
uint64_t t2i_capture_id(t2i_stream_t stream);

/* ---- data pipeline: reference preprocess/dataset.py ------------------------------ */
/* out[b] = crop/flip/normalise of stored image ids[b] (reference Dataset.next_batch + transform, dataset.py:83-96,150):
 * src [N,S,S,3] uint8 resident on the device; out [B,out_size,out_size,3] float32 with
 *   out[b,r,c,:] = u8 * (2/255) - 1  at  src[ids[b], row0[b]+r, col0[b] + (flip[b] ? out_size-1-c : c), :]
 * in float32 without fused multiply-add, i.e. bit-identical to NumPy's `images.astype(float32) * (2./255) - 1.`.
 * ids/row0/col0/flip are device int32[B]; the caller guarantees ids < N and row0/col0 + out_size <= S (the reference
 * draws them as floor((S - out_size) * U[0,1))). */
int t2i_crop_flip_normalize(const uint8_t* src, int64_t N, int32_t S, const int32_t* ids, const int32_t* row0,
                            const int32_t* col0, const int32_t* flip, int32_t B, int32_t out_size, float* out,
                            t2i_stream_t stream);
/* out[b,:] = mean_j emb[ids[b], choice[b,j], :]  (reference Dataset.sample_embeddings, dataset.py:98-120: mean of `k`
 * of the image's caption embeddings).  emb [N,En,D] float32, choice device int32[B,k]; sequential fp32 sum in choice
 * order then division by k — bit-identical to np.mean(e[choice], axis=0). */
int t2i_gather_mean(const float* emb, int64_t N, int32_t En, int32_t D, const int32_t* ids, const int32_t* choice, int32_t B,
                    int32_t k, float* out, t2i_stream_t stream);

/* ---- caption visualiser: reference utils/visualize.py closest_image --------------------------------------------- */
/* Closest training image of each of Q generated images.  For every query q and stored image n:
 *   real[r,c,ch] = fl32(fl32(u8 * fl32(2/255)) - 1)   (no fused multiply-add: exactly t2i_crop_flip_normalize's value) of
 *                  src[n, row0[q,n]+r, flip[q,n] ? col0[q,n]+out_size-1-c : col0[q,n]+c, ch]
 *   fake         = min(max(queries[q], lo), hi)        in fp32 (the reference's np.clip(samples, -1, 1))
 *   d2[q,n]      = sum ((double)fake - (double)real)^2 accumulated in fp64
 * idx[q] = the smallest n with minimal d2[q,n], dist2[q] = that minimum.  src [N,S,S,3] uint8; queries [Q,out_size,out_size,3]
 * float32; row0/col0/flip device int32 [Q,N] each, or all three NULL for the identity crop (then S == out_size); idx int32 [Q],
 * dist2 double [Q].  The caller guarantees row0/col0 + out_size <= S.  N <= INT32_MAX.  Scratch: the workspace query (Q*N
 * doubles).  No atomics: results are bitwise identical from call to call. */
size_t t2i_nearest_images_workspace_bytes(int32_t Q, int64_t N);
int t2i_nearest_images(const uint8_t* src, int64_t N, int32_t S, const int32_t* row0, const int32_t* col0, const int32_t* flip,
                       const float* queries, int32_t Q, int32_t out_size, float lo, float hi, int32_t* idx, double* dist2,
                       void* ws, size_t ws_bytes, t2i_stream_t stream);

/* ---- evaluator: Inception score and FID (reference evaluation/, utils/utils.py prep_incep_img) ------------------------- */
/* Pillow's 8-bit bilinear Image.resize, bit for bit, of B images [Hi, Wi, 3] into [B, Ho, Wo, 3].  Image b is row rows[b] of
 * the source store [N, Hi, Wi, 3] (rows == NULL: row b); a row outside [0, N) gives black.  src_f32 == 0: the store is uint8;
 * src_f32 == 1: it is fp32 generator output in [-1, 1], read as ((x + 1) * 127.5).astype(uint8) (truncating, saturated to
 * [0, 255]).  The filter tables are Pillow's precompute_coeffs + normalize_coeffs_8bpc for (Wi -> Wo) and (Hi -> Ho), made by
 * the caller: xb int32 [Wo, 2] (first source column, tap count <= kx), xk int32 [Wo, kx] (22-bit fixed-point weights); yb / yk
 * the same for rows.  Horizontal pass into a uint8 intermediate (workspace), then the vertical pass; every pass rounds with
 * 2^21 and clips to [0, 255].  out_u8 == 0: y is fp32 u / 127.5 - 1; out_u8 == 1: y is the uint8 pixel. */
size_t t2i_resample_bilinear_workspace_bytes(int32_t B, int32_t Hi, int32_t Wo);
int t2i_resample_bilinear(const void* src, int32_t src_f32, int64_t N, int32_t Hi, int32_t Wi, const int32_t* rows, int32_t B,
                          int32_t Ho, int32_t Wo, const int32_t* xb, const int32_t* xk, int32_t kx, const int32_t* yb,
                          const int32_t* yk, int32_t ky, void* y, int32_t out_u8, void* ws, size_t ws_bytes, t2i_stream_t stream);

/* TF max / average pooling of x [B, H, W, C] fp32 with a KH x KW window, strides SH, SW <= 4, TF SAME (same != 0) or VALID
 * padding.  Output [B, Ho, Wo] pixels of C channels go to y[pixel * y_ld + y_c0 + c] (a channel slice of a concatenation
 * buffer; y_c0 + C <= y_ld).  MAX ignores padded taps; AVG divides the fp32 sum of the in-bounds taps by their count, as TF
 * does.  op: T2I_POOL_MAX or T2I_POOL_AVG. */
enum { T2I_POOL_MAX = 0, T2I_POOL_AVG = 1 };
int t2i_pool2d(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t KH, int32_t KW, int32_t SH, int32_t SW,
               int32_t same, int32_t op, float* y, int32_t y_ld, int32_t y_c0, t2i_stream_t stream);

/* y[r * y_ld + y_c0 + c] = x[r * C + c] for r < rows, c < C (y_c0 + C <= y_ld): one branch of a channel concatenation. */
int t2i_channel_slice_copy(const float* x, int64_t rows, int32_t C, float* y, int32_t y_ld, int32_t y_c0, t2i_stream_t stream);

/* FID statistics, streamed: for X fp32 [n, d] and a shift s fp32 [d], sum[j] += sum_k (double)(X[k][j] - s[j]) and
 * G[i][j] += sum_k (X[k][i] - s[i]) (X[k][j] - s[j]) with sum fp64 [d] and G fp64 [d, d].  The products run on the fp32
 * matrix pipe (exact fp32 fma chains over runs of 64 rows), the runs and the calls accumulate in fp64.  No atomics: results
 * are bitwise identical from call to call.  The workspace query returns 0 (no scratch); ws may be NULL. */
size_t t2i_gram_accumulate_workspace_bytes(int64_t n, int32_t d);
int t2i_gram_accumulate(const float* X, int64_t n, int32_t d, const float* s, double* sum, double* G, void* ws, size_t ws_bytes,
                        t2i_stream_t stream);

/* IMD (reference evaluation/imd.py): for n row pairs of a fp32 [n, d] (row stride lda >= d) and b fp32 [n, d] (ldb >= d),
 * out[i] (fp64) = clip(1 - uv / sqrt(uu * vv), 0, 2) with uv = a_i . b_i, uu = |a_i|^2, vv = |b_i|^2 — scipy's
 * spatial.distance.cosine — and NaN when uu or vv is 0.  Products and sums in fp64; one wave64 per pair, each lane a fixed
 * stride of columns (16-byte reads where d, lda, ldb are multiples of 4 and a, b are 16-byte aligned), then a fixed-order
 * butterfly across the wave: no atomics, bitwise-repeatable.  Any d.  Bad arguments (n <= 0, d <= 0, ld < d, a NULL
 * pointer) return T2I_ERR_INVALID before anything is launched. */
int t2i_cosine_distance(const float* a, int64_t lda, const float* b, int64_t ldb, int64_t n, int32_t d, double* out,
                        t2i_stream_t stream);

/* ---- caption sheets: scipy.misc.imresize(float image, (size, size), interp='nearest') -------------------------------------- */
/* The reference's gen_multiple_stage_img / gen_pggan_sample resize FLOAT images with scipy.misc.imresize, i.e. scipy's bytescale
 * per image, Pillow's NEAREST resize, and (on the host, not here) / 127.5 - 1.  x fp32 [N, h, w, C] (contiguous, C in 1..4) ->
 * y uint8 [N, size, size, C].  Per image n, every operation rounded to fp32 on its own, in this order, no fused multiply-add:
 *   v = fl32(fl32(x + 1) * 127.5);  cmin, cmax = min, max of v over the whole image, all channels;
 *   cscale = fl32(cmax - cmin), replaced by 1 when it is 0;  scale = fl32(255 / cscale);
 *   u8 = (uint8) trunc(clip(fl32(fl32(v - cmin) * scale), 0, 255) + 0.5)
 * Output pixel (r, c) reads source pixel (floor((r + 0.5) * h / size), floor((c + 0.5) * w / size)), computed in integers.
 * Inputs are finite by contract (a generator's tanh output, clipped or not); there is no NaN policy.
 * Two launches: partial min / max per (image, chunk) into the workspace (16-byte loads where h*w*C % 4 == 0 and x is 16-byte
 * aligned), then per (image, tile of output rows) a fold of that image's partials and the gather, which quantises only the source
 * pixels it reads.  No atomics: results are bitwise identical from call to call.  An image holds at most 2^30 elements on either
 * side.  Bad arguments (a NULL pointer, N, h, w or size <= 0, C outside 1..4) return T2I_ERR_INVALID and a workspace that is NULL,
 * misaligned or smaller than the query T2I_ERR_WORKSPACE, before anything is launched.  Added within ABI v13: no existing
 * argument list changed. */
size_t t2i_bytescale_nearest_workspace_bytes(int64_t N, int32_t h, int32_t w, int32_t C);
int t2i_bytescale_nearest(const float* x, int64_t N, int32_t h, int32_t w, int32_t C, int32_t size, uint8_t* y, void* ws,
                          size_t ws_bytes, t2i_stream_t stream);

/* ---- load-size image stores: reference preprocess/utils.py transform (colorize, custom_crop, imresize 'bicubic') --------- */
/* Pillow's precompute_coeffs + normalize_coeffs_8bpc (libImaging/Resample.c) formed on the device in fp64, every operation
 * rounded on its own, in the order of evaluation/resize.py: for each of N axes, axis i resizing in_sizes[i] -> out_size,
 * bounds int32 [N, out_size, 2] = (first input index, tap count) and coeffs int32 [N, out_size, kmax] = the 22-bit fixed-point
 * weights, zero beyond the tap count.  in_sizes is a DEVICE int32 array.  An axis needs 2 * ceil(support * max(in / out, 1)) + 1
 * taps (support 1 for T2I_FILTER_BILINEAR, 2 for T2I_FILTER_BICUBIC); an axis that needs more than kmax, or whose size is
 * outside 1 .. T2I_PREPROCESS_MAX_SIDE, gets empty rows (count 0, weights 0).  out_size <= T2I_PREPROCESS_MAX_OUT. */
#define T2I_PREPROCESS_MAX_SIDE 16384 /* largest stored height / width of a source image */
#define T2I_PREPROCESS_MAX_OUT 2048   /* largest output side S */
enum { T2I_FILTER_BILINEAR = 0, T2I_FILTER_BICUBIC = 1 };
int t2i_pillow_tables(int32_t filter, const int32_t* in_sizes, int64_t N, int32_t out_size, int32_t* bounds, int32_t* coeffs,
                      int32_t kmax, t2i_stream_t stream);

/* One image of a ragged batch: uint8 [height, width, channels] stored at packed + offset, rows [y1, y2) and columns [x1, x2)
 * of it taken.  channels 1 (grey: read for all three output channels), 3, or 4 (the fourth is never read). */
typedef struct t2i_image_desc {
  int64_t offset;
  int32_t height, width, channels;
  int32_t y1, y2, x1, x2;
  int32_t reserved;
} t2i_image_desc;

/* scipy.misc.imresize(float image, [S, S], 'bicubic') of N cropped images, bit for bit, into y uint8 [N, S, S, 3].  Per image:
 * cmin, cmax = min, max over the crop (the channels that are read); scipy's bytescale as a 256-entry table in fp64,
 *   lut[u] = (uint8) trunc(clip((u - cmin) * (255.0 / cscale), 0, 255) + 0.5),  cscale = cmax - cmin, or 1 when that is 0
 * (a constant image comes out black); then Pillow's 8-bit BICUBIC resize of lut[pixel] with the tables above for
 * (crop width -> S) and (crop height -> S): horizontal pass into a uint8 intermediate, vertical pass, each
 * clip8(2^21 + sum).  No atomics: results are bitwise identical from call to call.
 * packed is device memory of packed_bytes bytes.  desc is a HOST array of N descriptors: the call checks every one, copies them
 * to the device on `stream`, enqueues its kernels behind the copy and then waits for the copy alone, so desc may be changed or
 * freed as soon as the call returns while the kernels may still be running.  (It is therefore the one entry point that waits on
 * the stream's earlier work, and it cannot be captured into a graph.)
 * The uint8 intermediate holds exactly the batch's rows: the workspace query takes total_rows, the sum of the crops' heights
 * y2 - y1, and max_side, the largest crop height or width.  The filter tables are NOT ragged: every image's two tables have
 * the tap count of max_side, N * 2 * S * taps * 4 bytes in all, so one extreme downscale in a batch of many images is paid for
 * by all of them (batch such images apart).  Limits: stored sides
 * <= T2I_PREPROCESS_MAX_SIDE, S <= T2I_PREPROCESS_MAX_OUT, N <= 2^24, N * S < 2^31, total_rows < 2^31.
 * Bad arguments (a NULL pointer, N or S <= 0 or above the limits, channels outside {1, 3, 4}, a crop that
 * is empty or leaves its image, an image that ends past packed_bytes) return T2I_ERR_INVALID and a workspace that is NULL,
 * misaligned (16 bytes) or smaller than the query T2I_ERR_WORKSPACE, before anything is launched.  Added within ABI v13: no
 * existing argument list changed. */
size_t t2i_preprocess_images_workspace_bytes(int64_t N, int64_t total_rows, int32_t max_side, int32_t S);
int t2i_preprocess_images(const uint8_t* packed, size_t packed_bytes, const t2i_image_desc* desc, int64_t N, int32_t S, uint8_t* y,
                          void* ws, size_t ws_bytes, t2i_stream_t stream);

/* ---- InceptionV3 fine-tuning (reference models/inception/trainer.py) -------------------------------------------------- */
/* AvgPool_1a_8x8 + Dropout_1b of slim inception_v3(is_training=True): x fp32 [B, HW, D] (the Mixed_7c output, HW = 64) ->
 * pre[b, d] = (sum_p x[b, p, d]) / HW (fp32, taps in order: t2i_pool2d's AVG), mask[b, d] = floor(keep + U) in {0, 1} and
 * y[b, d] = pre / keep * mask (tf.nn.dropout).  U in [0, 1) has 24 bits from Philox4x32-10 with key seed and counter
 * (element / 4, step): the mask is a pure function of (seed, step, b, d).  D % 4 == 0, 16-byte aligned tensors. */
int t2i_pool_dropout(const float* x, int32_t B, int32_t HW, int32_t D, float keep, uint64_t seed, uint64_t step, float* pre,
                     float* mask, float* y, t2i_stream_t stream);
/* The logits head and its mean sparse softmax cross-entropy, forward and backward, in two launches: logits = y W + bias
 * (y fp32 [B, D], W [D, C], bias [C], labels int32 [B] in [0, C)), prob = softmax(logits), loss[0] = mean_b (logsumexp -
 * logit[label]), acc[0] = mean_b (argmax prob == label; the first maximum), and with dz = (prob - onehot) / B: dW = y^T dz,
 * db = colsum dz (accumulate != 0: +=), dy = dz W^T.  Each output element is summed by one thread in a fixed order: no
 * atomics, bitwise-repeatable.  Any C <= 1024 with B * C <= 16384 and D + C <= 16384: the forward stages (D + C) floats and
 * the backward B * C floats in LDS, each within the 64 KiB a launch gets without asking for more. */
size_t t2i_softmax_ce_head_workspace_bytes(int32_t B, int32_t C);
int t2i_softmax_ce_head(const float* y, const float* W, const float* bias, const int32_t* labels, int32_t B, int32_t D, int32_t C,
                        float* logits, float* prob, float* loss, float* acc, float* dW, float* db, int32_t accumulate, float* dy,
                        void* ws, size_t ws_bytes, t2i_stream_t stream);
/* Gradient of the n <= T2I_MAX_SCATTER_BRANCHES Mixed_7c branch outputs from the gradient g [B, D] of the dropout output:
 * outs[i] [B, HW, C[i]] (device pointers in a HOST array) receives g[b, c0[i] + c] * mask[b, c0[i] + c] / keep / HW at every
 * pixel — the backward of t2i_pool_dropout, sliced into the branches of the concatenation.  C[i] % 4 == 0, c0[i] % 4 == 0. */
#define T2I_MAX_SCATTER_BRANCHES 8
int t2i_pooled_grad_scatter(const float* g, const float* mask, int32_t B, int32_t HW, int32_t D, float keep, int32_t n,
                            float* const* outs, const int32_t* c0, const int32_t* C, t2i_stream_t stream);
/* tf.train.RMSPropOptimizer (ApplyRMSProp) over a flat arena of n floats: ms += (g^2 - ms)(1 - rho);
 * mom = momentum * mom + lr * g / sqrt(ms + eps); w -= mom.  One launch. */
int t2i_rmsprop_tf(float* w, const float* g, float* ms, float* mom, int64_t n, float lr, float rho, float momentum, float eps,
                   t2i_stream_t stream);

/* ---- the rest of the operator surface: reference utils/ops.py:94-97 (pixel_norm), :100-101 (pool, any window), :104-116
 * (resize_nearest_neighbor / upscale / downscale), :145-148 (gn).  Added within ABI v13: no existing argument list changed.
 * fp32 tensors; 16-byte accesses when C % 4 == 0 and the tensors are 16-byte aligned, a scalar form for any other C; no atomics,
 * every sum in a fixed order: results repeat bit for bit. ---------------------------------------------------------------- */
/* u = act(x), y = u / sqrt(mean_c(u^2) + eps) over x [rows, C]; rnorm[rows] = 1 / sqrt(mean_c(u^2) + eps) is kept for the
 * backward.  One launch: a row is reduced by a power-of-two group of lanes of one wave through cross-lane shuffles and stays
 * in registers up to the scaling (rows of up to 2048 floats in the 16-byte form; wider rows are read twice). */
int t2i_pixel_norm_fwd(const float* x, int64_t rows, int32_t C, float eps, int act, float alpha, float* y, float* rnorm,
                       t2i_stream_t stream);
/* dx = du * act'(.), du = s (g - y mean_c(g y)), s = rnorm: u is recovered as y / s, so no x is needed (lrelu / relu read the
 * derivative from the sign of y, tanh is 1 - u^2).  The sign of y is the sign of x only for a slope alpha >= 0: both entry
 * points return T2I_ERR_INVALID for T2I_ACT_LRELU with alpha < 0.  One launch. */
int t2i_pixel_norm_bwd(const float* g, const float* y, const float* rnorm, int64_t rows, int32_t C, int act, float alpha, float* dx,
                       t2i_stream_t stream);
/* The double backward of pixel_norm: for the cotangent v of dx (t2i_pixel_norm_bwd) it writes dg = dL/dg and dxx = dL/dx of
 * L = <v, dx>, from v, g, y and rnorm alone.  With d = act'(.) read from the sign of y, w = v d and the per-pixel means m_wy, m_gy, m_wg:
 * dg = s (w - y m_wy), dxx = -s^2 (y m_wg + w m_gy + g m_wy - 3 y m_wy m_gy) d.  act: T2I_ACT_NONE, T2I_ACT_RELU or T2I_ACT_LRELU
 * with alpha >= 0 (piecewise linear: no second-derivative term); T2I_ACT_TANH and a negative slope return T2I_ERR_INVALID.
 * One launch, the lane-group scheme of the two kernels above. */
int t2i_pixel_norm_bwd2(const float* v, const float* g, const float* y, const float* rnorm, int64_t rows, int32_t C, int act, float alpha,
                        float* dg, float* dx, t2i_stream_t stream);
/* The double backward of layer_norm (per sample over per_sample elements, per-channel gamma over the last axis of C channels;
 * xhat and rstd as the forward left them, y = the activation's output or NULL for T2I_ACT_NONE, act as for t2i_pixel_norm_bwd2).
 * With g = gamma_c gy act'(.):  _sums writes sums [B,5] = per-sample (sum v, sum v xhat, sum g, sum g xhat, sum v g), each sample
 * split over up to 256 workgroups and finished in a fixed order (workspace: t2i_layer_norm_bwd2_workspace_bytes(B); two launches);
 * _apply reads the same tensors plus rstd and sums and writes dgy = dL/dgy and dx = dL/dx of L = <v, dx_first_order> in one launch,
 * and, if hgz is not NULL, hgz = (dL/dg) gy act'(.), whose column sums (t2i_col_reduce) are dL/dgamma.  B <= 65535. */
size_t t2i_layer_norm_bwd2_workspace_bytes(int32_t B);
int t2i_layer_norm_bwd2_sums(const float* v, const float* gy, const float* xhat, const float* y, const float* gamma, int32_t B,
                             int64_t per_sample, int32_t C, int act, float alpha, float* sums, void* ws, size_t ws_bytes,
                             t2i_stream_t stream);
int t2i_layer_norm_bwd2_apply(const float* v, const float* gy, const float* xhat, const float* y, const float* gamma, const float* rstd,
                              const float* sums, int32_t B, int64_t per_sample, int32_t C, int act, float alpha, float* dgy, float* dx,
                              float* hgz, t2i_stream_t stream);
/* Minibatch standard deviation (the critic layer of the progressive-growing paper) over x [B,H,W,C], fp32: sample n belongs to group
 * n / G (contiguous rows), channel c to chunk c / (C/F).  Per column (h, w, c) of a group: mu = mean_g x, d_g = x_g - mu,
 * sigma = sqrt(mean_g d_g^2 + eps) (biased, two passes over registers); stat [B,F]: row n, chunk f = the mean of sigma over the
 * Nf = H W C/F columns of chunk f of group n / G.  _bwd: dx_g = k d_g / sigma with k = (sum of gs over the group's rows) / (Nf G).
 * _bwd2, for the cotangent v of dx: dgs = dL/dgs = (1 / (Nf G)) sum_{g,j} v_g d_g / sigma (the same in every row of a group) and
 * dxx = dL/dx_g = k [(v_g - mean_g v) / sigma - d_g (sum_g v_g d_g) / (G sigma^3)].  G = 1: stat = sqrt(eps), dx = dxx = 0 exactly.
 * 1 <= G <= 16 dividing B, F >= 1 dividing C, B / G and F <= 65535, eps > 0 (sigma is a divisor); anything else, a NULL pointer or a workspace smaller than
 * t2i_minibatch_stddev_workspace_bytes (0 for a refused shape) returns T2I_ERR_INVALID before anything is launched.  A 16-byte form
 * where (C/F) % 4 == 0 and the tensors are 16-byte aligned, a scalar form otherwise.  No atomics; a group's work is cut by the
 * sample's shape alone, so the results for a batch are bit for bit those of its groups taken in separate calls.  _fwd and _bwd2
 * are two launches (partials in the workspace, then their fixed-order sum), _bwd is one.  Added within ABI v13. */
size_t t2i_minibatch_stddev_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t G, int32_t F);
int t2i_minibatch_stddev_fwd(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t G, int32_t F, float eps, float* stat,
                             void* ws, size_t ws_bytes, t2i_stream_t stream);
int t2i_minibatch_stddev_bwd(const float* gs, const float* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t G, int32_t F, float eps,
                             float* dx, t2i_stream_t stream);
int t2i_minibatch_stddev_bwd2(const float* v, const float* x, const float* gs, int32_t B, int32_t H, int32_t W, int32_t C, int32_t G,
                              int32_t F, float eps, float* dxx, float* dgs, void* ws, size_t ws_bytes, t2i_stream_t stream);
/* tf.image.resize_nearest_neighbor(align_corners = False): y[b,r,q,:] = x[b, src_h(r), src_w(q), :] with
 * src_h(r) = min(int(floorf(r * hs)), H - 1), hs = float(H) / float(Ho) in fp32, columns alike.  x [B,H,W,C] -> y [B,Ho,Wo,C]. */
int t2i_resize_nearest(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo, float* y, t2i_stream_t stream);
/* Its adjoint, also a gather (the map is monotone): dx[b,h,w,:] = the sum of g [B,Ho,Wo,C] over the contiguous block of output
 * rows and columns whose source is (h, w), rows outer, columns inner. */
int t2i_resize_nearest_adj(const float* g, int32_t B, int32_t H, int32_t W, int32_t C, int32_t Ho, int32_t Wo, float* dx,
                           t2i_stream_t stream);
/* tf.nn.pool, window = stride = s (1 <= s <= 32768), SAME: x [B,H,W,C] -> y [B,Ho,Wo,C], Ho = ceil(H / s), the padding
 * Ho s - H split with the smaller half in front.  op = T2I_POOL_AVG: sum of the taps inside the image (row-major) / their
 * count; idx must be NULL.  T2I_POOL_MAX: padding ignored; idx (int32 [B,Ho,Wo,C] or NULL) receives the window offset
 * ky * s + kx of the FIRST maximum in row-major window order. */
int t2i_pool_same_fwd(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, int32_t s, int32_t op, float* y, int32_t* idx,
                      t2i_stream_t stream);
/* Backward as a per-input gather (windows do not overlap): g [B,Ho,Wo,C] -> dx [B,H,W,C]; AVG: g of the pixel's window / that
 * window's count; MAX: g of the pixel's window where idx holds this pixel's offset, else 0. */
int t2i_pool_same_bwd(const float* g, const int32_t* idx, int32_t B, int32_t H, int32_t W, int32_t C, int32_t s, int32_t op, float* dx,
                      t2i_stream_t stream);
/* y[b,oh,ow,c] = x at offset idx[b,oh,ow,c] of that window (0 where the offset leaves the image): MAX pooling as the linear map
 * it is for fixed offsets — the backward of the MAX backward. */
int t2i_pool_same_take(const float* x, const int32_t* idx, int32_t B, int32_t H, int32_t W, int32_t C, int32_t s, float* y,
                       t2i_stream_t stream);
/* y = x * f, f = exp(nrm * log_m), nrm ~ N(0, 1) per element (log_m = log(noise magnitude) >= 0; 0 gives f = 1 and y = x bit
 * for bit).  Normals by Box-Muller from Philox4x32-10 keyed by seed and counted by (offset + i / 4) in a counter subsequence of
 * its own (third counter word non-zero; t2i_trunc_normal uses 0): a pure function of (seed, offset, i).  The caller advances
 * offset by (n + 3) / 4 per call.  f may be NULL (no backward will follow): the factor is then not written, y is the same.
 * One launch. */
int t2i_gn_fwd(const float* x, int64_t n, float log_m, uint64_t seed, uint64_t offset, float* y, float* f, t2i_stream_t stream);
/* y = a * b, n elements: the backward (and every further derivative) of gn. */
int t2i_mul(const float* a, const float* b, int64_t n, float* y, t2i_stream_t stream);

/* ---- sliced Wasserstein distance of Laplacian-pyramid patch descriptors (Karras et al., progressive growing of GANs; the reference
 * has no such metric).  Added within ABI v13: no existing argument list changed.  fp32 tensors, C in 1..4, every tensor below 2^31
 * elements.  No atomics: every sum in a fixed order, results bitwise identical from call to call; every entry only enqueues kernels
 * on `stream` (capturable).  Bad arguments (a NULL or misaligned pointer, a non-positive size, overlapping input / output /
 * workspace ranges, and what each entry names) return T2I_ERR_INVALID, a workspace that is NULL, misaligned (16 bytes) or smaller
 * than its query T2I_ERR_WORKSPACE, before anything is launched. ------------------------------------------------------------- */
/* x [N, H, W, C] -> out: the `levels` levels back to back, level i = [N, H >> i, W >> i, C] at element offset
 * N * C * sum_{j < i} (H >> j)(W >> j).  With k = [1, 4, 6, 4, 1] / 16, F = outer(k, k), g_0 = x:
 * g_{i+1} = convolve(g_i, F, 'mirror')[::2, ::2] (scipy.ndimage's mirror: reflection about the centre of the edge pixel),
 * lap_i = g_i - convolve(zero_insert_x2(g_{i+1}), 4 F, 'mirror') for i < levels - 1 and lap_{levels-1} = g_{levels-1}.  The
 * filters run separably in fp32 (rows then columns of an LDS tile; the up-sampling in its polyphase form), the Gaussian chain
 * g_1 .. g_{levels-2} lives in the workspace.  H and W must be multiples of 2^(levels-1) with H >> (levels-1) and W >> (levels-1)
 * at least 7; N <= 65535.  levels == 1 copies x. */
size_t t2i_laplacian_pyramid_workspace_bytes(int64_t N, int32_t H, int32_t W, int32_t C, int32_t levels);
int t2i_laplacian_pyramid(const float* x, int64_t N, int32_t H, int32_t W, int32_t C, int32_t levels, float* out, void* ws,
                          size_t ws_bytes, t2i_stream_t stream);
/* Rows row0 + n P + p of the descriptor store out [rows_total, 49 C]: the 7 x 7 x C neighbourhood of level [N, h, w, C] around
 * (y, x) = pos[n, p] (int32 [N, P, 2]), flattened in the order (c, dy, dx).  A pure gather, bit-exact.  Centres belong in
 * [3, side - 3); the kernel clamps them into that range, so no address is formed from an unchecked value.  row0 + N P <=
 * rows_total. */
int t2i_swd_descriptors(const float* level, int64_t N, int32_t h, int32_t w, int32_t C, const int32_t* pos, int32_t P, float* out,
                        int64_t row0, int64_t rows_total, t2i_stream_t stream);
/* mean64[c], std64[c] (fp64 [C]) of channel c of A [rows, 49 C]: over all rows and the channel's 49 columns, the mean and the
 * population standard deviation (ddof 0).  Two passes in fp64, the mean and then the centred squares, each leaving at most 1024
 * per-workgroup partials that one workgroup folds in a fixed order (four launches). */
size_t t2i_swd_channel_stats_workspace_bytes(int64_t rows, int32_t C);
int t2i_swd_channel_stats(const float* A, int64_t rows, int32_t C, double* mean64, double* std64, void* ws, size_t ws_bytes,
                          t2i_stream_t stream);
/* out[s][r] = sum_j ((A[r][j] - mean64[c(j)]) / std64[c(j)]) dirs[j][s], c(j) = j / 49, for A [rows, 49 C], dirs fp32 [49 C, S],
 * out fp32 [S, rows_pad]: the operand is standardised in fp64 as it is loaded and rounded once to fp32 (the standardised matrix
 * never exists in memory), then one fp32 fma chain over j in order.  The output is transposed, so a slice is one contiguous run;
 * entries rows <= r < rows_pad are +inf.  rows_pad: a power of two >= rows.  std64 must be non-zero (the caller checks). */
int t2i_swd_project(const float* A, int64_t rows, int32_t C, const double* mean64, const double* std64, const float* dirs, int32_t S,
                    float* out, int64_t rows_pad, t2i_stream_t stream);
/* Ascending bitonic sort of every segment of data [segments, len], in place; len a power of two, segments <= 65535 (a grid
 * dimension), data 16-byte aligned.  Chunks of T2I_SORT_CHUNK floats are sorted entirely in LDS by one launch; for each larger
 * merge size, global compare-exchange passes (16-byte accesses, up to three strides per pass) take the strides >= the chunk and
 * one LDS launch finishes all strides below it.  Inputs hold no NaN by contract (there is no NaN policy); +inf is legal and sorts
 * last.  t2i_segmented_sort_chunk() returns T2I_SORT_CHUNK. */
#define T2I_SORT_CHUNK 4096
int32_t t2i_segmented_sort_chunk(void);
int t2i_segmented_sort_f32(float* data, int32_t segments, int64_t len, t2i_stream_t stream);
/* out64[0] = (sum over segments and the first `rows` entries of each of |a - b|) / (segments * rows), a and b fp32
 * [segments, len], in fp64 and in a fixed order (two launches).  Entries rows <= r < len (the padding) are never read. */
size_t t2i_sorted_l1_mean_workspace_bytes(int32_t segments, int64_t rows);
int t2i_sorted_l1_mean(const float* a, const float* b, int32_t segments, int64_t len, int64_t rows, double* out64, void* ws,
                       size_t ws_bytes, t2i_stream_t stream);

/* ---- multi-scale structural similarity (Karras et al., ms_ssim.py = the TensorFlow-compression msssim; the reference has no such
 * metric).  Added within ABI v13: no existing argument list changed. -------------------------------------------------------------- */
/* One scale for N pairs a[n], b[n] of fp32 [H, W, C] images (levels 0..255 held as floats, C in 1..4, N H W C < 2^31):
 * with g = window_host[0..S) (S <= T2I_SSIM_MAX_WINDOW doubles ON THE HOST, copied into the kernel's arguments: the entry only
 * enqueues work and can be captured), mu1, mu2, E[a^2], E[b^2], E[ab] the VALID correlations with outer(g, g) per channel
 * ((H - S + 1) x (W - S + 1) x C maps, every moment accumulated in fp64), s11 = E[a^2] - mu1^2, s22 = E[b^2] - mu2^2,
 * s12 = E[ab] - mu1 mu2, v1 = 2 s12 + c2, v2 = s11 + s22 + c2:
 *   cs[n] = mean(v1 / v2),   ssim[n] = mean((2 mu1 mu2 + c1) v1 / ((mu1^2 + mu2^2 + c1) v2))      (device fp64 [N] each)
 * over the whole map, channels included.  Sums run in a fixed order (one fp64 partial pair per workgroup in the workspace, folded
 * per pair by a second launch; no atomics): results repeat bit for bit.  With a_half and b_half (both or neither) the same launch
 * writes the next scale [N, ceil(H/2), ceil(W/2), C]: out[i, j] = ((x[2i, 2j] + x[2i, j']) + (x[i', 2j] + x[i', j'])) * 0.25 in
 * fp32, i' = min(2i + 1, H - 1), j' = min(2j + 1, W - 1) (scipy.ndimage.convolve(x, ones(2, 2) / 4, 'reflect')[::2, ::2]).
 * Every refusal, a short workspace included, returns T2I_ERR_INVALID before anything is launched: a NULL a, b, ssim, cs,
 * window_host or workspace; N <= 0, H < 1, W < 1; C outside 1..4; S < 1, S > T2I_SSIM_MAX_WINDOW or S > min(H, W);
 * N H W C >= 2^31; exactly one of a_half / b_half NULL; an output or the workspace overlapping an input or another output (a and
 * b may be the same tensor); a workspace smaller than the query; a non-finite window entry, c1 or c2, or c2 <= 0; a misaligned
 * pointer (4 bytes for fp32, 8 for fp64 and the workspace). */
#define T2I_SSIM_MAX_WINDOW 11
size_t t2i_ssim_scale_workspace_bytes(int64_t N, int32_t H, int32_t W, int32_t C);
int t2i_ssim_scale(const float* a, const float* b, int64_t N, int32_t H, int32_t W, int32_t C, const double* window_host, int32_t S,
                   double c1, double c2, double* ssim, double* cs, float* a_half, float* b_half, void* workspace,
                   size_t workspace_bytes, t2i_stream_t stream);

/* ---- k-nearest-neighbour distances and ball counts in fp64 (evaluation/prdc.py: improved precision and recall, Kynkaanniemi et al.
 * 2019; density and coverage, Naeem et al. 2020; the reference has no such metric).  Added within ABI v13: no existing argument list
 * changed. ------------------------------------------------------------------------------------------------------------------------ */
/* Q [M, D] and R [N, D] are dense row-major fp32 on the device.  d2(m, n) = max(|Q_m|^2 + |R_n|^2 - 2 Q_m.R_n, 0), the three sums
 * accumulated in fp64 from the inputs widened exactly, each pair over the whole D in one fixed order: results are bit-identical for
 * every value of `segments` and from call to call (no atomics).  `segments` >= 1 splits the candidate range over workgroups (partial
 * results in the workspace, folded in segment order by a second launch); 0 lets the library choose.
 *   t2i_knn_dist2:   out[m, 0..k) = the k smallest d2(m, .) in ascending order (device fp64 [M, k]).  With exclude_self = 1 (M == N)
 *                    candidate n == m is skipped by INDEX: a duplicate row of the query still counts as a neighbour.
 *   t2i_ball_counts: count[m] = #{n : d2(m, n) <= r2[n]} (device int32 [M], r2 device fp64 [N]), dmin[m] = min_n d2(m, n) (fp64 [M]).
 * A NaN distance is never selected or counted (d2 < worst, d2 <= r2); a slot with no candidate holds +inf.
 * Every refusal returns T2I_ERR_INVALID before anything is launched: a NULL pointer; M, N or D < 1; k outside 1..T2I_KNN_MAX_K or
 * k > N - exclude_self; exclude_self not 0 / 1, or 1 with M != N; segments < 0, > N or > 65536; M D or N D >= 2^31 * 64; M k beyond
 * int64; a workspace smaller than the query; an output overlapping an input, another output or the workspace (Q and R may be the same
 * tensor); a misaligned pointer (4 bytes for fp32 and int32, 8 for fp64 and the workspace).  The entries only enqueue work. */
#define T2I_KNN_MAX_K 8
size_t t2i_knn_dist2_workspace_bytes(int64_t M, int64_t N, int32_t D, int32_t k, int32_t segments);
int t2i_knn_dist2(const float* Q, int64_t M, const float* R, int64_t N, int32_t D, int32_t k, int32_t exclude_self, int32_t segments,
                  double* out, void* workspace, size_t workspace_bytes, t2i_stream_t stream);
size_t t2i_ball_counts_workspace_bytes(int64_t M, int64_t N, int32_t D, int32_t segments);
int t2i_ball_counts(const float* Q, int64_t M, const float* R, int64_t N, int32_t D, const double* r2, int32_t segments, int32_t* count,
                    double* dmin, void* workspace, size_t workspace_bytes, t2i_stream_t stream);

/* ---- the kernel sums of the polynomial-kernel MMD^2 (evaluation/mmd.py: the Kernel Inception distance of Binkowski et al. 2018,
 * "Demystifying MMD GANs"; the reference has no such metric).  Added within ABI v13: no existing argument list changed. ------------- */
/* X [NX, D] and Y [NY, D] are dense row-major fp32 on the device (they may be one tensor); ix and iy are device int32 [S, m]: subset s
 * is the rows ix[s, 0..m) of X and iy[s, 0..m) of Y.  With k(a, b) = (gamma a.b + coef0)^degree, every a.b one fp64 sum over ascending
 * d of the inputs widened exactly, t = fma(gamma, a.b, coef0) and degree - 1 multiplications by t:
 *   sums[s, 0] = P_xx = sum_{i<j} k(x_i, x_j)     sums[s, 1] = P_yy likewise     sums[s, 2] = S_xy = sum_{i,j} k(x_i, y_j)
 * with i and j POSITIONS in the subset: a row named twice forms a pair with itself, a position never does.  No m x m matrix and no
 * copy of a subset is written; tiles of the two symmetric products below the diagonal are not computed.  One double per tile goes to the
 * workspace and a second launch adds each sum's tiles in ascending order: no atomics, results are bit-identical from call to call.
 * An index outside 0..N-1 is not dereferenced: its row counts as NaNs, so exactly the sums of its subset that it enters are NaN.
 * Every refusal returns T2I_ERR_INVALID before anything is launched: a NULL pointer; NX, NY, D or S < 1; m < 2; degree outside 1..8;
 * gamma or coef0 not finite; NX D or NY D >= 2^31 * 64; more than 2^30 work items (tiles of all subsets and products: the grid of the
 * one launch); a workspace smaller than the query; sums or the workspace overlapping an input, an index table or each other; a
 * misaligned pointer (4 bytes for fp32 and int32, 8 for fp64 and the workspace).  The entry only enqueues work. */
size_t t2i_poly_mmd_sums_workspace_bytes(int64_t NX, int64_t NY, int32_t D, int32_t S, int32_t m);
int t2i_poly_mmd_sums(const float* X, int64_t NX, const float* Y, int64_t NY, int32_t D, const int32_t* ix, const int32_t* iy, int32_t S,
                      int32_t m, int32_t degree, double gamma, double coef0, double* sums, void* workspace, size_t workspace_bytes,
                      t2i_stream_t stream);

/* ---- differentiable augmentation (Zhao et al., "Differentiable Augmentation for Data-Efficient GAN Training", NeurIPS 2020; the
 * reference has no such layer).  Added within ABI v13: no existing argument list changed. ------------------------------------------- */
/* x [B,H,W,C] fp32 and one row of params [B,9] fp32 = (b, s, c, ty, tx, y0, y1, x0, x1) per sample, the six geometric entries
 * integer-valued floats (the kernels clamp them to the image's extents before any index is formed, so no table can move an address out
 * of the tensors), the rectangle clipped to the image, y0 == y1 = no cutout.  With m_pix = the mean over a pixel's channels and M = the mean
 * over the sample:
 *   colour       u1 = u + b (only with offset != 0);  u2 = s u1 + (1 - s) m_pix(u1);  u3 = c u2 + (1 - c) M(u2),  M(u2) = M(u) + b
 *   translation  u4[y, x, :] = u3[y - ty, x - tx, :] inside the image, else 0
 *   cutout       u5[y, x, :] = 0 for y0 <= y < y1 and x0 <= x < x1, else u4[y, x, :]
 * policy: a non-empty mask of T2I_DIFFAUG_*; the columns of a policy outside the mask are not read (identity).  Both blends are
 * evaluated as k a + (1 - k) mean: s = 1 and c = 1 return the input bit for bit.  _adj is the adjoint of the linear part: g masked by
 * the rectangle, gathered at [y + ty, x + tx] (0 outside the image), then c g3 + (1 - c) M(g3) and s g2 + (1 - s) m_pix(g2).  The
 * backward of _adj is _fwd with offset = 0, so the pair is closed under differentiation of any order.
 * With T2I_DIFFAUG_COLOR each entry is two launches: per-sample partial sums (of x, or of the masked, shifted cotangent) into the
 * workspace in a fixed order, one partial per 4096 floats of a sample, then the apply kernel, which adds a sample's partials itself
 * in a fixed order; without it one launch and no workspace (the query returns 0; it also returns 0 for a refused shape).  No
 * atomics; a sample's work is cut by H, W and C alone, so its result is the same bits in whatever batch it sits and calls repeat bit
 * for bit.  Any C >= 1 (a thread keeps a pixel in registers for C = 3 and 4).  1 <= B <= 65535, 1 <= H, W <= 32768; anything else, a
 * NULL or misaligned (4 bytes) pointer, an unknown policy bit, an output overlapping its input or a workspace that is NULL or
 * smaller than the query returns T2I_ERR_INVALID before anything is launched. */
enum { T2I_DIFFAUG_COLOR = 1, T2I_DIFFAUG_TRANSLATION = 2, T2I_DIFFAUG_CUTOUT = 4 };
size_t t2i_diff_augment_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t policy);
int t2i_diff_augment_fwd(const float* x, const float* params, int32_t B, int32_t H, int32_t W, int32_t C, int32_t policy, int32_t offset,
                         float* y, void* ws, size_t ws_bytes, t2i_stream_t stream);
int t2i_diff_augment_adj(const float* g, const float* params, int32_t B, int32_t H, int32_t W, int32_t C, int32_t policy, float* dx,
                         void* ws, size_t ws_bytes, t2i_stream_t stream);

/* ---- the parameter table drawn on the device with probability p, and p steered from the critic's outputs (Karras et al., "Training
 * Generative Adversarial Networks with Limited Data", NeurIPS 2020).  Added within ABI v13: no existing argument list changed. --------
 * t2i_diffaug_state: sixteen 32-bit words (64 bytes) of device memory, 16-byte aligned, written by the host once and by the two
 * kernels afterwards:
 *   word 0, 1   seed lo, hi (u32)                      word 7      calls (u32): observe calls since the last adjustment
 *   word 2, 3   call counter lo, hi (u32)              word 8      last_r (f32): the statistic at the last adjustment, 0 before the first
 *   word 4      p (f32, in [0, 1])                     word 9      updates (u32): adjustments so far
 *   word 5      acc_sign (f32): running sum of signs   word 10-15  reserved: 0 from the host, left alone by the kernels
 *   word 6      acc_n (f32): real logits seen
 * t2i_diff_augment_draw writes params_out [n, 9] fp32, the table of t2i_diff_augment_fwd for H x W images, and advances the call
 * counter by one (64-bit, the carry from word 2 into word 3 included); it writes no other word.  Row i of call k takes three blocks
 * of Philox4x32-10 (multipliers D2511F53, CD9E8D57; Weyl constants 9E3779B9, BB67AE85; ten rounds) with key (seed lo, seed hi) and
 * counter (i, j, k lo, k hi), j = 0 colour, 1 translation, 2 cutout.  With u(w) = float(w >> 8) * 2^-24 and below(w, m) =
 * (uint64(w) * m) >> 32:
 *   j = 0   b = u(w1) - 0.5f,  s = 2 u(w2),  c = u(w3) + 0.5f
 *   j = 1   ty = below(w1, 2 r_H + 1) - r_H,  tx = below(w2, 2 r_W + 1) - r_W,  r_size = int(size / 8 + 0.5)
 *   j = 2   offset = below(w1 | w2, size - extent % 2 + 1) - extent / 2 along y | x, extent = int(size / 2 + 0.5); the rectangle is
 *           [max(offset, 0), min(offset + extent, size))
 * A transform is applied to a row iff its bit is in `policy` and u(w0) of its block < p (p = 0 never, p = 1 always); otherwise its
 * columns are the identity's (b 0, s 1, c 1, no shift, an empty rectangle), under which t2i_diff_augment_fwd returns the sample bit
 * for bit.  Every float is one rounding of an exact value, so the stream of tables is a pure function of (seed, call, row) that any
 * IEEE implementation reproduces bit for bit.  One launch of one workgroup, no host work: it may be captured in a graph, and every
 * replay draws the next call's table.  1 <= n <= 65535, 1 <= H, W <= 32768; anything else, a NULL pointer, a state not aligned to
 * 16 bytes, a table not aligned to 4 or an unknown or empty policy mask returns T2I_ERR_INVALID before anything is launched.
 * t2i_diffaug_observe adds sum_i sign(d_real[i] - theta) to acc_sign (sign(0) = 0), n to acc_n and 1 to calls; theta = 0 under
 * T2I_ADA_LOGIT (the publication's r_t for a critic with a logistic loss; d_fake may be NULL) and (mean d_real + mean d_fake) / 2
 * under T2I_ADA_MIDPOINT (the same statistic for a critic whose outputs have no fixed zero).  On the call that brings calls to
 * `interval`:  r = acc_sign / acc_n;  p <- clamp(p + sign(r - target) acc_n / ramp_images, 0, 1);  last_r <- r;  updates += 1;
 * acc_sign, acc_n and calls <- 0.  Words 0-3 and 10-15 are not written.  One launch of one workgroup, every sum in a fixed order.
 * A NULL state or d_real, a NULL d_fake under T2I_ADA_MIDPOINT, n outside 1..65535, an unknown mode, interval < 1, ramp_images not
 * positive and finite, target outside (-1, 1), a state not aligned to 16 bytes or a logit vector not to 4 returns T2I_ERR_INVALID
 * before anything is launched. */
enum { T2I_ADA_LOGIT = 0, T2I_ADA_MIDPOINT = 1 };
int t2i_diff_augment_draw(void* state, int32_t n, int32_t H, int32_t W, int32_t policy, float* params_out, t2i_stream_t stream);
int t2i_diffaug_observe(void* state, const float* d_real, const float* d_fake, int32_t n, int32_t mode, float target, int32_t interval,
                        float ramp_images, t2i_stream_t stream);

/* ---- spectral normalisation of the matrices of an arena (Miyato et al., "Spectral Normalization for Generative Adversarial
 * Networks", ICLR 2018).  Added within ABI v13: no existing argument list changed. ------------------------------------------------
 * An arena of n floats (a positive multiple of 4) holds n_slots normalised matrices, 1 <= n_slots <= T2I_SPECTRAL_MAX_SLOTS.  Row s
 * of table_dev (device int64 [n_slots, T2I_SPECTRAL_COLS], 8-byte aligned) is
 *   (off, R, C, u_off, v_off, part_off, iterate)
 * the row-major matrix M [R, C] at element `off` of the arena, its u [C] at u_off of `u` (nu floats), its v [R] at v_off of `v` (nv
 * floats), its partial sums at part_off of the workspace and whether the power iteration advances it.  off, u_off and v_off are
 * multiples of 4; the slots ascend and do not overlap; sigma is float [n_slots].  A matrix is cut into work items of
 * rb = min(R, clamp(8192 / C, 1, 2048)) rows, ceil(R / rb) of them: max_items is the largest count of any slot and max_col_blocks
 * the largest ceil(C / 64) (both at most T2I_SPECTRAL_MAX_ITEMS), a slot needs items * C + items + ceil(C / 64) floats of workspace at
 * part_off (column partials, the items' |t|^2, the column blocks' |s|^2), and part_floats is the end of the last such region.  The table lives in device memory, so the entries cannot read it: THE CALLER validates its rows before the upload (the
 * package does, in kernels.spectral_table), and a kernel forms addresses from rows that passed there.
 * t2i_spectral_grad: grad <- (grad - <grad, flat>_s v_s u_s^T) / max(sigma_s, 1e-12) inside every slot, in place; <,>_s the sum of
 * the slot's products, from per-item partials added in ascending order.  Elements outside the slots are left alone.  Two launches.
 * t2i_spectral_normalize: `iterations` (0..T2I_SPECTRAL_MAX_ITERATIONS) times, for every slot with iterate != 0:
 *   t = M u;  v = t / max(|t|, 1e-12);  s = M^T v;  sigma = |s|;  u = s / max(sigma, 1e-12)         (M read from `raw`)
 * then flat[i] = raw[i] / max(sigma_s, 1e-12) for every element of every slot (iterate or not) and flat[i] = raw[i] elsewhere: the
 * other variables of the arena and the padding.  3 iterations + 1 launches; treats the filter cache as t2i_adam_tf does for `flat`.
 * Both: no floating-point atomics and every sum in a fixed order, so a call repeats bit for bit and a matrix gives the same bits
 * whatever else its table holds; graph-capturable, no allocation, no synchronisation.  Refused with T2I_ERR_INVALID before any launch:
 * a NULL pointer; n, nu or nv not a positive multiple of 4, nu or nv above n; n_slots, max_items, max_col_blocks or iterations out of
 * range; part_floats < 1 or above 4 n + 8 n_slots; an arena, u, v or the workspace not 16-byte aligned, the table not 8-byte, sigma not 4-byte; a workspace smaller than
 * t2i_spectral_workspace_bytes(part_floats) (0 for a refused count); any two of the buffers, the table and the workspace overlapping. */
#define T2I_SPECTRAL_MAX_SLOTS 2048
#define T2I_SPECTRAL_MAX_ITEMS (1 << 22)
#define T2I_SPECTRAL_MAX_ITERATIONS 64
#define T2I_SPECTRAL_COLS 7
size_t t2i_spectral_workspace_bytes(int64_t part_floats);
int t2i_spectral_grad(float* grad, const float* flat, int64_t n, const int64_t* table_dev, int32_t n_slots, int32_t max_items, const float* u,
                      int64_t nu, const float* v, int64_t nv, const float* sigma, int64_t part_floats, void* ws, size_t ws_bytes,
                      t2i_stream_t stream);
int t2i_spectral_normalize(float* flat, const float* raw, int64_t n, const int64_t* table_dev, int32_t n_slots, int32_t max_items,
                           int32_t max_col_blocks, float* u, int64_t nu, float* v, int64_t nv, float* sigma, int32_t iterations,
                           int64_t part_floats, void* ws, size_t ws_bytes, t2i_stream_t stream);

/* ---- anti-aliased resampling: upsample by zero insertion, pad or crop, FIR filter, decimate (the upfirdn2d of Karras et al., "A
 * Style-Based Generator Architecture for Generative Adversarial Networks", CVPR 2019, with the taps of Zhang, "Making Convolutional
 * Networks Shift-Invariant Again", ICML 2019).  Added within ABI v13: no existing argument list changed. ---------------------------------
 * x [B,H,W,C] -> y [B,Ho,Wo,C], contiguous NHWC fp32.  taps: n floats in HOST memory, 1 <= n <= T2I_UPFIRDN_MAX_TAPS, read during the
 * call and used on both axes; u, d in {1, 2}; the pads p0 (front) and p1 (back) may be negative, which crops.  Per axis, with
 * z[j] = x[j / u] where 0 <= j < H u and u divides j, else 0:
 *   Ho = floor((H u + p0 + p1 - n) / d) + 1 = t2i_upfirdn2d_extent(H, u, d, p0, p1, n)        (0 for a refused shape)
 *   y[o] = sum_{t = 0}^{n - 1} g[n - 1 - t] z[o d + t - p0],     g = taps, or taps reversed when flip != 0
 * a true convolution.  The adjoint for an input of extent H and output extent Ho is the same entry on [B,Ho,Wo,C] with
 *   u' = d, d' = u, p0' = n - 1 - p0, p1' = H u - Ho d + p0 - u + 1, flip' = !flip
 * and returns extent H exactly.  One launch; both axes in it, the input window of a T2I_UPFIRDN_TILE x T2I_UPFIRDN_TILE output tile staged
 * once in LDS; with u = 2 only the taps that meet a stored sample are read (the inserted zeros exist nowhere).  A 16-byte form when
 * C % 4 == 0 and x, y are 16-byte aligned, a scalar form otherwise.  An output is sum_t w_t (sum_s w_s x), both sums by fma in
 * ascending tap order: no atomics, calls repeat bit for bit, a sample's bits do not depend on its batch.  The taps travel as kernel
 * arguments: graph-capturable, no device table, no allocation, no synchronisation.  Refused with T2I_ERR_INVALID before any launch: a
 * NULL pointer; a size < 1; n outside 1..8; u or d outside {1, 2}; |p0| or |p1| above 32768; an extent < 1; x or y of 2^31 elements or
 * more; x and y overlapping; a tap that is not finite. */
#define T2I_UPFIRDN_TILE 8
#define T2I_UPFIRDN_MAX_TAPS 8
int32_t t2i_upfirdn2d_extent(int32_t H, int32_t u, int32_t d, int32_t p0, int32_t p1, int32_t n);
int t2i_upfirdn2d(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, const float* taps, int32_t n, int32_t u, int32_t d,
                  int32_t p0, int32_t p1, int32_t flip, float* y, t2i_stream_t stream);
/* The same with a back pad per axis, p1_h along H and p1_w along W (t2i_upfirdn2d passes p1 for both): where d = 2 and H and W leave
 * different remainders, the adjoint's p1' differs between the axes by one. */
int t2i_upfirdn2d_axes(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, const float* taps, int32_t n, int32_t u, int32_t d,
                       int32_t p0, int32_t p1_h, int32_t p1_w, int32_t flip, float* y, t2i_stream_t stream);

/* ---- the style-based generator's layer epilogue: per-pixel noise, activation, instance norm and the style's affine map (AdaIN; Karras
 * et al., CVPR 2019).  csrc/t2i_style.hip, DESIGN.md section 4.42.  Added within ABI v13: no existing argument list changed. ------------
 * x [B,R,C] (R = H W, contiguous NHWC fp32), noise [B,R] and strength [C] (both or neither: NULL), ys and yb [B,C] whose rows lie
 * style_stride >= C floats apart (the two halves of one dense layer's [B,2C] output need no copy):
 *   u = act(x + strength[c] noise[b,r])     act: T2I_ACT_NONE, T2I_ACT_RELU or T2I_ACT_LRELU with alpha >= 0; without noise u = act(x)
 *   mean[b,c], var[b,c] = the biased moments of u over r,    rstd = rsqrt(var + eps)
 *   y = (u - mean) rstd (1 + ys[b,c]) + yb[b,c]
 * _stats  (2 launches) per-chunk (mean, M2) by Welford's update for each (b, chunk of T2I_ADAIN_CHUNK_ROWS rows, c) into the workspace, then
 *         their merge in ascending chunk order by Chan's update -> mean [B,C], rstd [B,C]; never E[u^2] - mean^2.
 * _apply  (1 launch) recomputes u and writes y; no plane of u or of the normalised u is ever stored.
 * _bwd_sums (2 launches) for the cotangent g of y: dyb [B,C] = sum_r g, dys [B,C] = sum_r g uh, uh = (u - mean) rstd recomputed.
 * _bwd_apply (1 launch, 2 with dstrength) dx = act'(u) rstd (1 + ys) (g - dyb / R - uh dys / R), act' from the sign of the recomputed
 *         pre-activation; dstrength [C] (or NULL; needs noise) = sum_{b,r} dx noise, per-item partials summed in a fixed order.  noise gets
 *         no gradient.
 * A 16-byte form when C % 4 == 0 and the [B,R,C] tensors of the call are 16-byte aligned, a scalar form otherwise.  A grid of at most 65535
 * workgroups walks the items with a stride.  No atomics; the split depends on R and C alone: mean, rstd, y, dx, dys and dyb of a sample do
 * not depend on its batch, and calls repeat bit for bit.  Graph-capturable: no allocation, no synchronisation, nothing read back.
 * Refused with T2I_ERR_INVALID before any launch: a NULL pointer (noise, strength and dstrength apart); a size < 1; 2^31 elements or more;
 * another activation or a negative slope; noise without strength or the reverse; dstrength without noise; style_stride < C; eps negative or
 * not finite; an output overlapping x or g.  A workspace that is NULL, not 16-byte aligned or smaller than t2i_adain_workspace_bytes
 * (0 for a refused shape) returns T2I_ERR_WORKSPACE (_bwd_apply reads it only with dstrength). */
#define T2I_ADAIN_CHUNK_ROWS 64
int32_t t2i_adain_chunk_rows(void);
size_t t2i_adain_workspace_bytes(int32_t B, int64_t R, int32_t C);
int t2i_adain_stats(const float* x, const float* noise, const float* strength, int32_t B, int64_t R, int32_t C, int act, float alpha,
                    float eps, float* mean, float* rstd, void* ws, size_t ws_bytes, t2i_stream_t stream);
int t2i_adain_apply(const float* x, const float* noise, const float* strength, const float* mean, const float* rstd, const float* ys,
                    const float* yb, int32_t style_stride, int32_t B, int64_t R, int32_t C, int act, float alpha, float* y,
                    t2i_stream_t stream);
int t2i_adain_bwd_sums(const float* g, const float* x, const float* noise, const float* strength, const float* mean, const float* rstd,
                       int32_t B, int64_t R, int32_t C, int act, float alpha, float* dys, float* dyb, void* ws, size_t ws_bytes,
                       t2i_stream_t stream);
int t2i_adain_bwd_apply(const float* g, const float* x, const float* noise, const float* strength, const float* mean, const float* rstd,
                        const float* ys, int32_t style_stride, const float* dys, const float* dyb, int32_t B, int64_t R, int32_t C,
                        int act, float alpha, float* dx, float* dstrength, void* ws, size_t ws_bytes, t2i_stream_t stream);

/* ---- weight-demodulated convolutions (Karras et al., CVPR 2020): what surrounds the convolution.  csrc/t2i_modconv.hip, DESIGN.md section
 * 4.45.  Added within ABI v13: no existing argument list changed. -------------------------------------------------------------------------
 * With s [B,Cin] (rows style_stride >= Cin floats apart) and W [T,Cin,Cout] (T = KH KW taps of an HWIO filter), the modulated layer
 *   y[b] = conv(x[b], W s[b,:] d[b,:]),  d[b,o] = rsqrt(sum_{t,i} (W[t,i,o] s[b,i])^2 + eps)
 * equals d[b,o] conv(x[b] s[b,:], W)[.,.,o] exactly, and d = rsqrt(sum_i s[b,i]^2 q[i,o] + eps) with q[i,o] = sum_t W[t,i,o]^2.  The
 * convolution is t2i_conv2d_fwd as it is; these calls are the rest.  fp32 only.  R = H W rows per sample.
 * t2i_demod_coef (2 launches): q [Cin,Cout] (t ascending) and d [B,Cout] (input channels in 4 fixed lanes, merged in ascending order).
 * t2i_demod_coef_bwd (a launch per wanted output): for the cotangent gd of d, with e = -d^3 gd / 2:  ds [B,Cin] (dense; or NULL; needs q)
 *         = 2 s sum_o q[i,o] e[b,o];  dW [T,Cin,Cout] (or NULL; needs W) = 2 W[t,i,o] sum_b s[b,i]^2 e[b,o], b ascending;
 *         accumulate != 0 adds that to what dW holds (a gradient arena slot that the convolution's filter gradient shares).
 * t2i_modulate (1 launch): xs[b,r,c] = x[b,r,c] s[b,c]; with the cotangent of xs in place of x it is its own adjoint for dx.
 * t2i_modulate_bwd_scale (2 launches): ds [B,C] = sum_r g[b,r,c] x[b,r,c]: partials per chunk of T2I_MODCONV_CHUNK_ROWS rows in the
 *         workspace, then their sum in a fixed order.
 * t2i_demod_act (1 launch): out = act(p), p = fmaf(strength[c], noise[b,r], fmaf(d[b,c], c[b,r,c], bias[c])).  d NULL: coefficient 1; bias
 *         NULL: 0; noise [B,R] and strength [C] both or neither (without them the outer fmaf is not taken).  act: T2I_ACT_NONE, T2I_ACT_RELU
 *         or T2I_ACT_LRELU with alpha >= 0.
 * t2i_demod_act_bwd (1 launch, 2 with any of the sums): recomputes p by the same sequence; gp = act'(p) g; dc (or NULL) = gp d;
 *         dd [B,C] (or NULL; needs d) = sum_r gp c;  dbias [C] (or NULL) = sum_{b,r} gp;  dstrength [C] (or NULL; needs noise) = sum_{b,r} gp
 *         noise.  Per-item partials in the workspace (read only when a sum is wanted), summed in a fixed order.  noise gets no gradient.
 * A 16-byte form when C % 4 == 0 and the [B,R,C] tensors of the call are 16-byte aligned, a scalar form otherwise.  A grid of at most 65535
 * workgroups walks the items with a stride.  No atomics; every split depends on the shape without B: a sample's d, xs, out, dc, dd and ds
 * do not depend on its batch, and calls repeat bit for bit.  Graph-capturable: no allocation, no synchronisation, nothing read back.
 * Refused with T2I_ERR_INVALID before any launch: a NULL pointer (the optional ones above apart; _act_bwd with no output at all); a size < 1;
 * 2^31 elements or more; style_stride below the channel count; eps negative or not finite; another activation or a negative slope; noise
 * without strength or the reverse; dstrength without noise; dd without d; an output overlapping an input or another output.  A workspace
 * that is NULL, not 16-byte aligned or smaller than the call's *_workspace_bytes (0 for a refused shape) returns T2I_ERR_WORKSPACE.
 * t2i_demod_coef, its backward, t2i_modulate and t2i_demod_act need no workspace and take none. */
#define T2I_MODCONV_CHUNK_ROWS 64
int32_t t2i_modconv_chunk_rows(void);
int t2i_demod_coef(const float* W, const float* s, int32_t style_stride, int32_t T, int32_t Cin, int32_t Cout, int32_t B, float eps, float* q,
                   float* d, t2i_stream_t stream);
int t2i_demod_coef_bwd(const float* gd, const float* d, const float* s, int32_t style_stride, const float* W, const float* q, int32_t T,
                       int32_t Cin, int32_t Cout, int32_t B, float* ds, float* dW, int32_t accumulate, t2i_stream_t stream);
int t2i_modulate(const float* x, const float* s, int32_t style_stride, int32_t B, int64_t R, int32_t C, float* xs, t2i_stream_t stream);
size_t t2i_modulate_bwd_scale_workspace_bytes(int32_t B, int64_t R, int32_t C);
int t2i_modulate_bwd_scale(const float* g, const float* x, int32_t B, int64_t R, int32_t C, float* ds, void* ws, size_t ws_bytes,
                           t2i_stream_t stream);
int t2i_demod_act(const float* c, const float* d, const float* bias, const float* noise, const float* strength, int32_t B, int64_t R, int32_t C,
                  int act, float alpha, float* out, t2i_stream_t stream);
size_t t2i_demod_act_bwd_workspace_bytes(int32_t B, int64_t R, int32_t C);
int t2i_demod_act_bwd(const float* g, const float* c, const float* d, const float* bias, const float* noise, const float* strength, int32_t B,
                      int64_t R, int32_t C, int act, float alpha, float* dc, float* dd, float* dbias, float* dstrength, void* ws,
                      size_t ws_bytes, t2i_stream_t stream);

/* ---- the backward of that backward (path-length regularisation differentiates the generator twice).  csrc/t2i_modconv.hip, DESIGN.md
 * section 4.46.  Added within ABI v13: no existing argument list changed.  Same items, forms, grid, order of sums and refusals as above.
 * t2i_demod_act_bwd2 (1 launch, 2 with gd): with m = act'(p), p recomputed by the forward's sequence, the first backward gave dc = m g d
 *         and dd = sum_r m g c.  For the cotangents vc [B,R,C] of dc and vd [B,C] of dd (each may be NULL, not both; vd needs d):
 *           gg [B,R,C] (or NULL) = m (d vc + c vd)     gc [B,R,C] (or NULL; needs vd) = m g vd     gd [B,C] (or NULL; needs vc and d) = sum_r m g vc
 *         g is read only for gc and gd (it may be NULL without them).  bias, strength and noise get nothing: act'' is zero almost everywhere.
 * t2i_modulate2 (1 launch): the first backward gave dx = g s and ds = sum_r g x.  For the cotangents vx [B,R,C] and vs [B,C] (dense; each
 *         may be NULL, not both; vx comes with s, vs with x):  gg = s vx + x vs.  (g vs is t2i_modulate, sum_r vx g is t2i_modulate_bwd_scale.)
 * t2i_demod_coef_bwd2 (a launch for gg_d / gd_d, a launch for dW): the first backward gave ds = 2 s sum_o q e, e = -d^3 gd / 2.  For the
 *         cotangent vs [B,Cin] (dense) of ds, with r[b,o] = sum_i vs[b,i] s[b,i] q[i,o] (input channels in 4 fixed lanes, ascending):
 *           gg_d [B,Cout] (or NULL; needs q) = -d^3 r           (to gd)
 *           gd_d [B,Cout] (or NULL; needs q) = -3 d^2 gd r      (to d)
 *           dW [T,Cin,Cout] (or NULL; needs W) (+)= 4 W[t,i,o] sum_b vs[b,i] s[b,i] e[b,o], b ascending; accumulate as in t2i_demod_coef_bwd
 *         (the term to s is t2i_demod_coef_bwd's ds with vs in place of s). */
size_t t2i_demod_act_bwd2_workspace_bytes(int32_t B, int64_t R, int32_t C);
int t2i_demod_act_bwd2(const float* g, const float* c, const float* d, const float* bias, const float* noise, const float* strength,
                       const float* vc, const float* vd, int32_t B, int64_t R, int32_t C, int act, float alpha, float* gg, float* gc, float* gd,
                       void* ws, size_t ws_bytes, t2i_stream_t stream);
int t2i_modulate2(const float* s, int32_t style_stride, const float* vx, const float* x, const float* vs, int32_t B, int64_t R, int32_t C,
                  float* gg, t2i_stream_t stream);
int t2i_demod_coef_bwd2(const float* vs, const float* gd, const float* d, const float* s, int32_t style_stride, const float* W, const float* q,
                        int32_t T, int32_t Cin, int32_t Cout, int32_t B, float* gg_d, float* gd_d, float* dW, int32_t accumulate,
                        t2i_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* T2I_HIP_H */
