/* vltf.h -- C-ABI of libvltf_hip.so: the MI355X (gfx950) hot path of npit/video-learning-tf.
 *
 * The reference has no FFI: every FLOP of its hot path runs inside two TensorFlow executor calls,
 *   train:   sess.run([summaries, loss, lr, global_step, optimizer], feed_dict)   run_task.py:29,44
 *   forward: sess.run(model.logits, feed_dict)                                     run_task.py:95
 * over a graph assembled from stock TF ops (models/alexnet/alexnet.py, models/lstm/lstm.py,
 * tf_util.py, train.py).  Each entry point below replaces one of those TF ops (cited per
 * function); the Python host (video-learning-tf_amd/) composes them exactly where the
 * reference composes the TF ops, so the two sess.run calls become two host functions.
 *
 * Conventions
 *   - extern "C"; every function returns 0 on success, non-zero on failure;
 *     vl_last_error() returns a thread-local human readable message for the last failure.
 *   - Every data pointer is a DEVICE pointer owned by the caller (torch-ROCm tensors are used
 *     only as allocations).  Nothing is allocated after vl_conv_create(); workspaces are
 *     caller provided.  All work is enqueued asynchronously on `stream` (a hipStream_t).
 *   - Activations are NCHW fp32.  Parameters keep the reference's layouts: conv kernels HWIO
 *     [kh][kw][cin/group][cout] (alexnet.py:73,113), fc weights [in][out] (alexnet.py:225),
 *     LSTM kernel [D+H][4H] with gate order i, j, f, o (TF BasicLSTMCell; lstm.py:17).
 *   - Thread-compatible: one stream/descriptor set per host thread (exceptions, both process-wide words: vl_set_conv_math
 *     and the test hooks vl_lstm_seq_test_hooks, vl_pool_lrn_bwd_test_ranges, vl_conv_set_row_classes,
 *     vl_conv_set_stage_depth / vl_conv_last_launch).
 */
#ifndef VLTF_H
#define VLTF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vl_stream_t;                 /* hipStream_t */
typedef struct vl_conv_desc vl_conv_desc;  /* opaque convolution descriptor */

/* Device-resident scalars of one training step (a block in device memory, vl_step_state_bytes() bytes, caller allocated).  The
 * _st entry points read them when they run instead of taking them as kernel arguments, so that a captured step (hipGraph) replays
 * with the values of the current step: the host writes the block with vl_step_state_set on the stream before each replay. */
typedef struct vl_step_state {
    int64_t step;          /* the step count BEFORE the step's update: the dropout seed is (step << 20) ^ 0x5DEECE66D */
    float lr;              /* learning rate */
    uint32_t tag_origin;   /* origin of the LSTM exchange tags of vl_lstm_seq_*_st */
    float adam_lr;         /* Adam's bias-corrected step size for count step + 1 (written by vl_step_state_set, see there) */
    float ema_rate;        /* 1 - decay of this update's weight average (written by vl_step_state_set_ema alone, see vl_ema_update) */
    uint32_t reserved[2];  /* LAMB's bias corrections as fp32 bit patterns: word VL_STEP_STATE_LAMB_C1 = c1, word VL_STEP_STATE_LAMB_C2 =
                              c2 (bytes 24 and 28; written by vl_step_state_set_lamb alone, see vl_lamb_moments); 0 until then */
} vl_step_state;
#define VL_STEP_STATE_LAMB_C1 0
#define VL_STEP_STATE_LAMB_C2 1

const char* vl_last_error(void);
int vl_version(void);
/* Number of HIP devices visible; <0 on error.  Does not create a context. */
int vl_device_count(void);

/* ---- input preparation: Dataset.process_image (dataset_.py:481-501) on device ------------------
 * src: uint8 [n][raw_h][raw_w][3] HWC, BGR (the TFRecord 'image_raw' bytes, dataset_.py:125-126).
 * dst: fp32  [n][3][out_h + 2*dst_halo][out_w + 2*dst_halo] NCHW; the interior ROWS are written whole -- their halo (and, in the
 * phase-split layout, padding) columns with the 0.0 a halo holds -- the halo rows above and below are not touched (they must have
 * been zeroed once: the halo is conv1's SAME padding, see vl_conv_set_halo).  n <= 65535.  crop_y/crop_x: int32[n] top-left crop offsets
 * (center: floor((raw-want)/2), dataset_.py:572-573); mirror: uint8[n] flips the W axis
 * (dataset_.py:497-499); mean_bgr: float[3] subtracted per channel (dataset_.py:521-530), may be NULL.
 * crop_y, crop_x, mirror may be NULL (= 0).  dst_phase = 1, or the consuming conv's vl_conv_x_phase(): dst is then the
 * column-phase-split layout [n][3][phase][out_h + 2*dst_halo][ceil((out_w + 2*dst_halo) / phase)]. */
int vl_input_prep_u8(const uint8_t* src, float* dst, int n, int raw_h, int raw_w, int out_h, int out_w,
                     const int32_t* crop_y, const int32_t* crop_x, const uint8_t* mirror,
                     const float* mean_bgr, int dst_halo, int dst_phase, vl_stream_t stream);
/* Random resized crop: the same destination contract (interior rows whole, halo / padding columns 0.0, halo rows untouched,
 * n <= 65535), the source a box per frame.  box: DEVICE int32 [n][4] = {y0, x0, bh, bw} in pixels of the raw_h x raw_w frame; the
 * kernel clamps bh, bw into [1, raw] and then y0, x0 into [0, raw - b] before use, so no box value reads outside the frame.  Output
 * pixel (oy, ox) is the bilinear sample of the box (half-pixel centres, clamped to the box's edge, no antialiasing), taps and weights
 * from integers:  num = max((2 oy + 1) bh - out_h, 0); i0 = min(num / (2 out_h), bh - 1); i1 = min(num / (2 out_h) + 1, bh - 1);
 * fy = (num % (2 out_h)) / (2 out_h) (taken as 0 where i0 == i1); columns alike; value = lerp(lerp(p[i0][j0], p[i0][j1], fx),
 * lerp(p[i1][j0], p[i1][j1], fx), fy) - mean[c], lerp(a, b, f) = a (1 - f) + b f.  mirror flips the output W axis after sampling.
 * out_h / out_w may exceed raw_h / raw_w (a box may be upsampled); bh == out_h and bw == out_w give vl_input_prep_u8's crop at
 * (y0, x0) bit for bit.  mirror, mean_bgr may be NULL; src, dst, box may not. */
int vl_input_prep_u8_box(const uint8_t* src, float* dst, int n, int raw_h, int raw_w, int out_h, int out_w, const int32_t* box,
                         const uint8_t* mirror, const float* mean_bgr, int dst_halo, int dst_phase, vl_stream_t stream);
/* The reference's own feed format: fp32 NHWC placeholder (models/model.py:54) -> NCHW (+halo, dst_phase as above).  A copy of the
 * pixels, bit for bit, and of nothing else: unlike vl_input_prep_u8 it writes NO halo or phase-padding column, in the interior rows
 * either -- the whole halo must have been zeroed once (tests/test_feed_geometry_gpu.py holds it to that). */
int vl_nhwc_to_nchw(const float* src, float* dst, int n, int h, int w, int c, int dst_halo, int dst_phase, vl_stream_t stream);
int vl_nchw_to_nhwc(const float* src, float* dst, int n, int c, int h, int w, vl_stream_t stream);

/* ---- convolution: dcnn.conv (alexnet.py:15-31) = tf.nn.conv2d 'SAME' per group + bias_add ------
 * The descriptor fixes geometry and owns small device index tables (allocated at create). */
int vl_conv_create(vl_conv_desc** out, int cin, int h, int w, int cout, int kh, int kw, int stride, int groups);
void vl_conv_destroy(vl_conv_desc* d);
int vl_conv_out_hw(const vl_conv_desc* d, int* oh, int* ow);
/* Padded ("halo") activation layout.  A tensor with halo p is stored [n][c][H + 2p][W + 2p] with p zero
 * pixels on every side of each plane; only interiors are ever written.  When the gathered operand's halo
 * covers the SAME padding, the im2col gather needs no bounds test at all (every tap is in-bounds and the
 * padding taps read the zeros), which removes all vector-ALU address work from the kernel's steady state.
 *   x_halo : layout of x (vl_conv_fwd / vl_conv_wgrad input; also of vl_conv_dgrad's relu_mask)
 *   y_halo : layout of y written by vl_conv_fwd
 *   dy_halo: layout of dy read by vl_conv_dgrad / vl_conv_wgrad
 *   dx_halo: layout of dx written by vl_conv_dgrad
 * Default 0 everywhere (dense NCHW; bounds-tested gather).  Rebuilds the index tables (setup time only). */
int vl_conv_set_halo(vl_conv_desc* d, int x_halo, int y_halo, int dy_halo, int dx_halo);
/* Column-phase-split x for a strided conv in the padded layout (conv1, stride 4): x is stored
 * [n][c][phase = stride][H + 2p][ceil((W + 2p) / stride)], physical column iw at [iw % stride][iw / stride].  The taps of
 * consecutive output columns are then CONSECUTIVE addresses (a 64-lane gather touches 2 cache lines instead of 8), for
 * vl_conv_fwd and vl_conv_wgrad alike.  on = 0 restores plain [n][c][H + 2p][W + 2p].  Call after vl_conv_set_halo; no-op
 * for stride 1.  vl_conv_x_phase returns the phase count in force (1 = plain). */
int vl_conv_set_x_phase_split(vl_conv_desc* d, int on);
int vl_conv_x_phase(const vl_conv_desc* d);
/* Arithmetic of the contraction in vl_conv_fwd / vl_conv_dgrad / vl_conv_wgrad and, given the workspace of
 * vl_gemm_split_ws_bytes, of the large vl_gemm products (process-wide):
 *   0  fp32 MFMA (default; the reference's arithmetic, alexnet.py:21 tf.nn.conv2d on float32)
 *   3  "bf16x3": each fp32 operand is split into a bf16 head and tail (x = hi + lo + O(2^-17 |x|)) and a product is
 *      hi*hi + hi*lo + lo*hi on the bf16 matrix pipe with fp32 accumulation -- results agree with mode 0 to ~5e-6
 *      relative L2 per layer, inside every parity tolerance of tests/, but it is NOT fp32 arithmetic and is opt-in.
 *      Applies to layers in the padded layout with >= 96 output channels per group and unit column stride in memory
 *      (stride 1, or the phase-split x of a strided conv); other layers keep mode 0.
 *   6  "bf16x6": three bf16 pieces per operand and the six products above 2^-23 -- agrees with mode 0 to ~1e-7 relative L2 per
 *      layer, i.e. to fp32 rounding (as close as two fp32 summation orders are to each other); opt-in like mode 3.
 *   1  plain bf16 products (heads only), fp32 accumulation: ~2.3e-3 relative L2 per layer -- the reduced-precision conv path
 *      of BASELINE config 5; outside the fp32 parity tolerances by design (tests hold it to 3e-2 on logits).
 * The environment variable VL_CONV_MATH=bf16x3 | bf16x6 | bf16 presets mode 3 | 6 | 1.
 * NOT thread-safe: the mode is ONE process-wide word read by every later launch call, the only exception to this header's
 * "thread-compatible" convention.  A process that mixes arithmetics sets it before each group of launches from the one thread
 * that issues them (LRCNEngine does, at the top of every forward and backward pass); two host threads launching with
 * different modes need an external lock around (set, launches). */
int vl_set_conv_math(int math);
int vl_conv_math(void);
/* Test hook of vl_conv_fwd / vl_conv_dgrad in fp32 arithmetic, process-wide, default on.  A stride-1 layer with kh > 1 in the padded
 * layout whose launch has many frames enumerates its output pixels by ROW CLASS (runs of output rows that share one set of in-range
 * kernel rows: 3 x 3 pad 1 gives {0}, {1 .. OH-2}, {OH-1}), every 128-pixel tile inside one class, and a tile's reduction leaves out
 * the kernel rows that lie in the SAME-padding halo for all of its pixels.  Those terms are w * (+0) added to a sum that starts at +0:
 * for finite weights the results are bitwise those of on = 0, which enumerates pixels flat and multiplies the halo's zeros like data.
 * The one difference: with on = 0 a non-finite weight reaches every output through its padding taps as well (inf * 0 = NaN); with
 * on = 1 it no longer poisons the border rows through the kernel rows left out. */
int vl_conv_set_row_classes(int on);
/* Test hook of the same launches, process-wide, default 0.  The 16x16-MFMA LDS-DMA kernel (48- and 96-channel tiles: conv1 / conv4
 * forward, conv2 / conv4 / conv5 dgrad) exists with reduction stages of 32 rows (two workgroups per CU) and of 16 rows (three).
 * rows = 16 or 32 forces that form on every launch of the kernel, 0 returns the choice to the dispatcher.  The stage depth moves
 * barriers only, never the order of a sum: the two forms agree bit for bit.  Launches of other kernels ignore it. */
int vl_conv_set_stage_depth(int rows);
/* Kernel form of the latest vl_conv_fwd / vl_conv_dgrad call in fp32 arithmetic: tile height * 100 + stage depth for an LDS-DMA
 * launch (4816, 4832, 9616, 9632: the 16x16-MFMA kernel; 12832: the 32x32-MFMA kernel), 0 for any other kernel.  A call that splits
 * into two launches reports the second. */
int vl_conv_last_launch(void);
/* y[n][cout][oh][ow] = conv(x[n][cin][h][w], w_hwio) + bias, optional fused ReLU (alexnet.py:77). */
int vl_conv_fwd(const vl_conv_desc* d, const float* x, const float* w_hwio, const float* bias, float* y,
                int n, int relu, vl_stream_t stream);
/* wt = flipped/transposed copy of w used by vl_conv_dgrad: wt[kh'][kw'][co][g*cin_g+ci] =
 * w[KH-1-kh'][KW-1-kw'][ci][g*cout_g+co].  Same element count as w. */
int vl_conv_wt_transpose(const vl_conv_desc* d, const float* w_hwio, float* wt, vl_stream_t stream);
/* dx = d(loss)/dx given dy (stride-1 layers only; conv1 never needs it).  If relu_mask != NULL
 * (same shape as dx) the ReluGrad of the producing layer is fused: dx = relu_mask > 0 ? dx : 0. */
int vl_conv_dgrad(const vl_conv_desc* d, const float* dy, const float* wt, float* dx, const float* relu_mask,
                  int n, vl_stream_t stream);
/* dw (HWIO) = d(loss)/dw.  Deterministic split reduction through `ws` (>= vl_conv_wgrad_ws_bytes).
 * db (optional, [cout]): the bias gradient sum_{n,h,w} dy, accumulated from the dy tiles the kernel streams
 * anyway (no second pass over dy); available when vl_conv_wgrad_fuses_bias() != 0 (padded layout), else pass
 * NULL and use vl_bias_grad_nchw. */
size_t vl_conv_wgrad_ws_bytes(const vl_conv_desc* d, int n);
int vl_conv_wgrad_fuses_bias(const vl_conv_desc* d);
int vl_conv_wgrad(const vl_conv_desc* d, const float* x, const float* dy, float* dw, float* db, void* ws,
                  size_t ws_bytes, int n, vl_stream_t stream);
/* ---- the bf16 conv PATH (BASELINE config 5; csrc/conv_c8.hip) --------------------------------------
 * Same arithmetic as vl_set_conv_math(1) -- operands rounded to bf16 (nearest even), fp32 accumulation, fp32 bias / ReLU -- but the
 * operands ARE bf16 in memory, in the "c8" layout: a tensor [n][c][h][w] with halo p is stored
 * [n][ceil(c/8)][h + 2p][w + 2p][8] bf16 (8 consecutive channels of a pixel = one 16-byte chunk = one MFMA operand; zero halo, zero
 * beyond c).  Kernels fetch 16 bytes per lane straight into LDS and run v_mfma_f32_32x32x16_bf16 with no conversion in the loop.
 * Layers: channels per group a multiple of 8, padded layout (vl_conv_set_halo), not phase split; dgrad / wgrad: stride 1, wgrad
 * additionally x_halo == dy_halo (every SAME layer with an odd kernel).  Halos are those of the descriptor, as for the fp32 calls.
 * PRECONDITION on every c8 tensor handed to these calls: halo chunks and channels beyond c hold ZEROS.  No kernel here writes them
 * (only interiors are ever written), so a buffer zeroed once at allocation stays valid; a caller that recycles memory must zero it
 * first.  vl_conv_c8_wgrad (it sweeps each image's plane linearly, halo columns included: their dy must be 0) and vl_bias_grad_c8
 * (it sums whole rows) return WRONG dw / db on a dirty halo, without any check; forward / dgrad read halo taps as the padding zeros.
 *   vl_c8_bytes            bytes of a c8 tensor (allocate zeroed once: only interiors are ever written)
 *   vl_pack_c8             fp32 NCHW (x_halo) -> c8 (xb_halo): the stand-alone producer
 *   vl_conv_c8_pack_w      HWIO fp32 weights -> the packed operand of vl_conv_c8_fwd (bwd = 0) / vl_conv_c8_dgrad (bwd = 1);
 *                          wb: vl_conv_c8_w_bytes(d, bwd) bytes
 *   vl_conv_c8_fwd         y (fp32 NCHW, y_halo; may be NULL) and / or yb (c8, y_halo; may be NULL) = conv(xb) + bias (ReLU)
 *   vl_conv_c8_dgrad       dx (fp32 NCHW, dx_halo) and / or dxb (c8, dx_halo) from dyb (c8, dy_halo); ReluGrad of the producing layer
 *                          from relu_mask (fp32, as vl_conv_dgrad) or relu_mask_c8 (the layer's own packed input xb, x_halo)
 *   vl_bias_grad_c8        db[c] = sum_{n,h,w} dy from the packed gradient (c8, halo); ws: float[64 * 8 * ceil(c/8)]
 *   vl_conv_c8_wgrad       dw (HWIO fp32) from xb and dyb; deterministic slab reduction through ws (vl_conv_c8_wgrad_ws_bytes) */
size_t vl_c8_bytes(int n, int c, int h, int w, int halo);
int vl_pack_c8(const float* x, void* xb, int n, int c, int h, int w, int x_halo, int xb_halo, vl_stream_t stream);
size_t vl_conv_c8_w_bytes(const vl_conv_desc* d, int bwd);
int vl_conv_c8_pack_w(const vl_conv_desc* d, const float* w_hwio, void* wb, int bwd, vl_stream_t stream);
int vl_conv_c8_fwd(vl_conv_desc* d, const void* xb, const void* wb, const float* bias, float* y, void* yb, int n, int relu,
                   vl_stream_t stream);
int vl_conv_c8_dgrad(vl_conv_desc* d, const void* dyb, const void* wbt, float* dx, void* dxb, const float* relu_mask,
                     const void* relu_mask_c8, int n, vl_stream_t stream);
size_t vl_conv_c8_wgrad_ws_bytes(const vl_conv_desc* d, int n);
int vl_conv_c8_wgrad(vl_conv_desc* d, const void* xb, const void* dyb, float* dw, void* ws, size_t ws_bytes, int n,
                     vl_stream_t stream);
int vl_bias_grad_c8(const void* dyb, float* db, float* ws, int n, int c, int h, int w, int halo, vl_stream_t stream);
/* Dense products on the same pipeline (fc6 of the bf16 path): c[m][n] = sum_k a[k][m] b[k][n] (+ bias[n]) (ReLU) with both operands
 * reduction-major in 8-channel blocks, "kc8" = [ceil(channels / 8)][k][8] bf16 -- what the wgrad kernel consumes.
 *   vl_pack_kc8   dst = src[position * pos_stride + channel * ch_stride] (fp32, any strides: a matrix or its transpose) in kc8
 *   vl_gemm_kc8   the product (fp32 out, row-major; m, n multiples of 8); ws: vl_gemm_kc8_ws_bytes (split-k slabs, fixed order)
 * A kc8 address (dst, a_kc8, b_kc8) is a multiple of 16 -- 16-byte stores and fetches -- or the call is refused. */
int vl_pack_kc8(const float* src, void* dst, int64_t positions, int channels, int64_t pos_stride, int64_t ch_stride, vl_stream_t stream);
size_t vl_gemm_kc8_ws_bytes(int m, int n, int k);
int vl_gemm_kc8(const void* a_kc8, const void* b_kc8, float* c, int m, int n, int k, const float* bias, int relu, void* ws,
                size_t ws_bytes, vl_stream_t stream);
/* A strided first layer (conv1: 11 x 11 / 4 over 3 channels) on the same kernels: with kh = s a + py, kw = s b + px it is a ka x ka
 * (ka = ceil(k / s), odd) STRIDE-1 layer over the cin s^2 channels (c, py, px) of the space-to-depth input -- identical products and
 * sums, plus multiplies by zero where s a + py >= k.  The caller creates that layer's descriptor (cin s^2, oh, ow, cout, ka, ka, 1, 1;
 * x_halo = dy_halo = (ka - 1) / 2) and runs vl_conv_c8_fwd / vl_conv_c8_wgrad on it with
 *   vl_s2d_c8_from_x0   x0 (fp32, as the strided layer d's vl_conv_fwd takes it) -> packed input [n][cin s^2 / 8][oh + ka - 1][ow + ka - 1][8]
 *   vl_s2d_weights      grad = 0: w [k][k][cin][cout] -> [ka][ka][cin s^2][cout];  grad = 1: the stride-1 layer's dw -> dw
 *   vl_input_prep_u8_s2d  the uint8 frames straight into that packed input (arguments as vl_input_prep_u8; the crop is d's h x w):
 *                       the same values as vl_input_prep_u8 followed by vl_s2d_c8_from_x0
 *   vl_input_prep_u8_box_s2d  likewise for vl_input_prep_u8_box (box: device int32 [n][4], clamped by the kernel; out size d's h x w;
 *                       n <= 65535): bit for bit vl_input_prep_u8_box followed by vl_s2d_c8_from_x0 */
int vl_s2d_c8_from_x0(const vl_conv_desc* d, const float* x0, void* xb, int n, vl_stream_t stream);
int vl_input_prep_u8_s2d(const vl_conv_desc* d, const uint8_t* src, void* xb, int n, int raw_h, int raw_w, const int32_t* crop_y,
                         const int32_t* crop_x, const uint8_t* mirror, const float* mean_bgr, vl_stream_t stream);
int vl_input_prep_u8_box_s2d(const vl_conv_desc* d, const uint8_t* src, void* xb, int n, int raw_h, int raw_w, const int32_t* box,
                             const uint8_t* mirror, const float* mean_bgr, vl_stream_t stream);
int vl_s2d_weights(const vl_conv_desc* d, const float* src, float* dst, int grad, vl_stream_t stream);
/* db[c] = sum_{n,h,w} dy[n][c][h][w]  (gradient of tf.nn.bias_add, alexnet.py:31).
 * ws: float[64*c] scratch. */
int vl_bias_grad_nchw(const float* dy, float* db, float* ws, int n, int c, int hw, vl_stream_t stream);

/* ---- tf.nn.local_response_normalization (alexnet.py:79-89,120-130), across channels ------------
 * y = x / (bias + alpha * sum_{|c'-c|<=radius} x^2)^beta   (alpha not divided by the window). */
int vl_lrn_fwd(const float* x, float* y, int n, int c, int hw, int radius, float alpha, float beta, float bias,
               vl_stream_t stream);
/* dx for the above; relu_fused != 0 additionally applies the ReluGrad of the layer that produced
 * x (x is a ReLU output, alexnet.py:77): dx = x > 0 ? dx : 0.  x and dy are dense; dx may carry a halo
 * (plane width w, hw = h*w): it is the dy of the conv that produced x. */
int vl_lrn_bwd(const float* x, const float* dy, float* dx, int n, int c, int hw, int radius, float alpha,
               float beta, float bias, int relu_fused, int w, int dx_halo, vl_stream_t stream);

/* Fused backward of [LRN -> max_pool 3x3/2 VALID] (alexnet.py:79-98,120-139): dx = LRN'(x) applied to the
 * pooled gradient routed through argmax, + optional ReluGrad of x; the gradient wrt the LRN output is never
 * written.  x dense NCHW [n][c][h][w] (the LRN input); dp / argmax: pool-output layout NCHW with p_halo;
 * dx: NCHW with dx_halo; its interior ROWS are written whole (the halo columns of those rows receive the 0.0 a zero halo holds). */
int vl_pool_lrn_bwd(const float* x, const float* dp, const uint8_t* argmax, float* dx, int n, int c, int h, int w,
                    int p_halo, int radius, float alpha, float beta, float bias, int relu_fused, int dx_halo,
                    vl_stream_t stream);

/* vl_pool_lrn_bwd with the gradient written as packed bf16 (dxb: "c8" layout of the bf16 conv path, dxb_halo; rounded to nearest
 * even) instead of fp32 dx -- the only form that path's wgrad / dgrad / bias gradient read.  x_packed != 0: x (the LRN input) is packed
 * as well, c8 without a halo, as the producing conv's epilogue writes it. */
int vl_pool_lrn_bwd_c8(const void* x, int x_packed, const float* dp, const uint8_t* argmax, void* dxb, int n, int c, int h, int w,
                       int p_halo, int radius, float alpha, float beta, float bias, int relu_fused, int dxb_halo, vl_stream_t stream);

/* Test hook of vl_pool_lrn_bwd / vl_pool_lrn_bwd_c8, process-wide: force the number of channel ranges a (band, image) is split into
 * (1..4; fewer where the channel count does not allow it); 0 = the launcher's cost model (the default). */
int vl_pool_lrn_bwd_test_ranges(int ranges);

/* Fused forward of [LRN -> max_pool 3x3/2 VALID] (alexnet.py:79-98,120-139): p = max_pool(lrn(x)), argmax = window-local
 * index (0..8) of the first maximum in scan order; the LRN output is never written (vl_pool_lrn_bwd needs only x).
 * x dense NCHW [n][c][h][w]; p / argmax: NCHW with p_halo.  The interior ROWS are written whole: the halo columns of those rows
 * receive 0.0 in p (what a zero halo holds anyway) and unspecified bytes in argmax (its halo is never read); halo rows are not touched. */
int vl_lrn_pool_fwd(const float* x, float* p, uint8_t* argmax, int n, int c, int h, int w, int p_halo, int radius,
                    float alpha, float beta, float bias, vl_stream_t stream);

/* vl_lrn_pool_fwd with the pooled output written as packed bf16 (pb: "c8" layout of the bf16 conv path, p_halo) instead of fp32 p:
 * the next conv's operand.  argmax as vl_lrn_pool_fwd.  x_packed != 0: x is packed as well (c8 without a halo). */
int vl_lrn_pool_fwd_c8(const void* x, int x_packed, void* pb, uint8_t* argmax, int n, int c, int h, int w, int p_halo, int radius,
                       float alpha, float beta, float bias, vl_stream_t stream);

/* ---- tf.nn.max_pool k x k, stride s, VALID (alexnet.py:91-98,132-139,204-211) ------------------
 * x NCHW [n][c][h][w]; y element (n,c,oh,ow) is stored at y[n*ys_n + c*ys_c + oh*ys_h + ow*ys_w]
 * (NCHW: ys = {c*oh*ow, oh*ow, ow, 1}; (h,w,c)-flat for fc6, alexnet.py:228: {oh*ow*c, 1, ow*c, c}).
 * argmax: uint8 per output element, stored with the same strides: window-local index of the
 * first maximum in scan order (TF-CPU MaxPoolGrad target). */
int vl_maxpool_fwd(const float* x, float* y, uint8_t* argmax, int n, int c, int h, int w, int k, int s,
                   int64_t ys_n, int64_t ys_c, int64_t ys_h, int64_t ys_w, vl_stream_t stream);
/* dx NCHW with dx_halo (interior fully written).  relu_mask (the pool input, dense NCHW) optional: fused ReluGrad. */
int vl_maxpool_bwd(const float* dy, const uint8_t* argmax, float* dx, const float* relu_mask, int n, int c,
                   int h, int w, int k, int s, int64_t ys_n, int64_t ys_c, int64_t ys_h, int64_t ys_w,
                   int dx_halo, vl_stream_t stream);

/* ---- dense GEMM on fp32 MFMA: tf.nn.relu_layer / xw_plus_b / matmul gradients ------------------
 * C[m][n] = sum_k opA(m,k) * opB(k,n) (+ bias[n]) (ReLU) ; then C = relu_mask>0 ? C : 0 if given.
 * transa == 0: A is [m][k] row-major (lda);  transa != 0: A is stored [k][m] (lda).
 * transb == 0: B is [k][n] row-major (ldb);  transb != 0: B is stored [n][k] (ldb).
 * relu_mask has C's layout (ldc).  ws/ws_bytes: scratch for split-K (may be NULL/0: no split). */
int vl_gemm(int transa, int transb, int m, int n, int k, const float* a, int64_t lda, const float* b, int64_t ldb,
            float* c, int64_t ldc, const float* bias, int relu, const float* relu_mask, void* ws, size_t ws_bytes,
            vl_stream_t stream);
/* Workspace (bytes) with which vl_gemm runs an m x n x k product in the split-bf16 arithmetic selected by vl_set_conv_math
 * (operand images + split-K slabs); with a smaller workspace, or in mode 0, vl_gemm is the fp32 MFMA kernel. */
size_t vl_gemm_split_ws_bytes(int m, int n, int k);
/* out[n] = sum_m a[m][n] (bias gradients of fc layers); ws: float[64*n]. */
int vl_colsum(const float* a, int64_t lda, float* out, float* ws, int m, int n, vl_stream_t stream);

/* ---- LSTM: tf.contrib.rnn.BasicLSTMCell under tf.nn.dynamic_rnn (lstm.py:9-20,102-143) ---------
 * Rows are clip-major: row r = b*T + t.  gx = X @ kernel[:D] + bias for all rows is hoisted into one
 * vl_gemm; per step the host calls vl_gemm for gh = h_{t-1} @ kernel[D:] and then this kernel:
 *   z = gx[r] + gh[b];  i,j,f,o = split(z);  c = c_prev*sigmoid(f+forget_bias) + sigmoid(i)*tanh(j);
 *   h = tanh(c)*sigmoid(o).
 * act[r][4H] receives the activated gates (i, j, f, o), cseq[r][H] the cell state, hseq[r][H] the
 * output, hprev[r][H] a copy of h_{t-1} (zeros at t == 0).  gh may be NULL at t == 0. */
int vl_lstm_step_fwd(const float* gx, const float* gh, float* act, float* cseq, float* hseq, float* hprev,
                     int batch, int T, int t, int H, float forget_bias, vl_stream_t stream);
/* BPTT step t: dh = dout[r] + dh_next[b] (dh_next may be NULL at t == T-1); writes dz[r][4H] and
 * dc (in/out, [batch][H], zero before t == T-1). */
int vl_lstm_step_bwd(const float* dout, const float* dh_next, const float* act, const float* cseq, float* dc,
                     float* dz, int batch, int T, int t, int H, vl_stream_t stream);

/* The whole recurrence in ONE launch per direction (csrc/lstm_cluster.hip).  kh = kernel[D:] ([H][4H], row stride 4H).
 * Same outputs as T x {vl_gemm + vl_lstm_step_fwd}.  H <= 1024.
 *   h0, c0 (nullable, [batch][H]): initial output and cell state -- the reference's get_state_tuple (lstm.py:34-42) passes ONE
 *   vector as both (c = h = init), from input_state_fc (lstm.py:74-77); NULL = dynamic_rnn's zero state.  hprev[r] at t == 0 is h0.
 * H <= 512: weight-stationary cluster form -- ceil(H/16) workgroups per group of <= 8 clips keep their 64 gate columns of kh in
 * LDS for the whole sequence and exchange h_t (forward) / partial dh_{t-1} (backward) through tagged 8-byte words in `ws`
 * (agent-scope atomics, bounded spins); larger H: one workgroup per clip streaming kh every step.
 * ws: device scratch of vl_lstm_seq_ws_bytes(batch, T, H) bytes, ZEROED ONCE by the caller when it is allocated: its first word is
 * the sticky time-out flag of vl_lstm_seq_status, which no launch clears; the rest holds the exchange words, whose tags are unique
 * per launch within the process (no launch zeroes them), so it must not be handed anything else to scribble on. */
size_t vl_lstm_seq_ws_bytes(int batch, int T, int H);
/* vl_lstm_seq_fwd / vl_lstm_seq_bwd take each launch's tag base from a process-wide host counter and pass it as a kernel argument: a
 * captured launch would replay the same tags over the words its previous replay left behind and read stale values.  So both return
 * an error, and launch nothing, when `stream` is being captured (hipStreamIsCapturing); a graph uses the _st variants below. */
int vl_lstm_seq_fwd(const float* gx, const float* kh, const float* h0, const float* c0, float* act, float* cseq, float* hseq,
                    float* hprev, int batch, int T, int H, float forget_bias, void* ws, size_t ws_bytes, vl_stream_t stream);
/* BPTT over all steps: dout may be NULL; writes dz[r][4H]; c0 as given to the forward call (NULL = zero state);
 * dh0 / dc0 (nullable, [batch][H]) receive the gradients w.r.t. the initial output / cell state. */
int vl_lstm_seq_bwd(const float* dout, const float* kh, const float* act, const float* cseq, const float* c0, float* dz,
                    float* dh0, float* dc0, int batch, int T, int H, void* ws, size_t ws_bytes, vl_stream_t stream);
/* ---- per-clip sequence lengths (tf.nn.dynamic_rnn(sequence_length=...), lstm.py:132-142) ------------------------------------------
 * seq_len: device int32 [batch], one entry per sequence; steps t >= seq_len[b] of clip b are DEAD (values are clamped to 0..T on
 * the device; callers validate 1..T).  NULL = the call without _len.  The recurrence is dynamic_rnn's:
 *   - state is copied through a dead step (c_t = c_{t-1}, h_t = h_{t-1}), so cseq[b][T-1] is still the final cell state, and the
 *     output of a dead step is zero;
 *   - backward: dout of a dead row is ignored, its dz is exactly 0, nothing flows into dh / dc there (dead steps are a suffix and
 *     there is no gradient into the final state); dh0 / dc0 are the gradients of the live prefix.
 * THE DEAD-ROW CONTRACT: every row of every output is written, and no output depends on a dead row of gx or dout, not even as
 * 0 * x -- they may hold NaN.  Dead rows get act = 0, cseq = the carried c, hseq = 0, hprev = the carried h, dz = 0, so the
 * whole-sequence GEMMs that follow (x^T dz, hprev^T dz, dz K^T) can sum over them.
 * The cluster form's exchange does not depend on the lengths: every workgroup publishes and gathers at every step.
 * Like the eager pair, these refuse a stream that is being captured. */
int vl_lstm_seq_fwd_len(const float* gx, const float* kh, const float* h0, const float* c0, float* act, float* cseq, float* hseq,
                        float* hprev, int batch, int T, int H, float forget_bias, const int32_t* seq_len, void* ws, size_t ws_bytes,
                        vl_stream_t stream);
int vl_lstm_seq_bwd_len(const float* dout, const float* kh, const float* act, const float* cseq, const float* c0, float* dz,
                        float* dh0, float* dc0, int batch, int T, int H, const int32_t* seq_len, void* ws, size_t ws_bytes,
                        vl_stream_t stream);
/* Replay-safe variants (capturable): the tag base of launch k of the call is state->tag_origin, read from device memory when the
 * kernel runs, + tag_offset + k (T + 1).  A call uses the tags origin + tag_offset + 1 .. origin + tag_offset +
 * vl_lstm_seq_tag_span(batch, T, H) - 1 (span 0: the per-clip form, no tags).  The caller owns the tag stream: `ws` must not be
 * used by the eager variants, every replay needs an origin above the tags of the previous replays on `ws`, and before the origin
 * starts over the exchange words are zeroed (vl_lstm_seq_ws_clear).  The eager variants' limit of the tag range is 0xfff00000. */
size_t vl_lstm_seq_tag_span(int batch, int T, int H);
int vl_lstm_seq_fwd_st(const float* gx, const float* kh, const float* h0, const float* c0, float* act, float* cseq, float* hseq,
                       float* hprev, int batch, int T, int H, float forget_bias, void* ws, size_t ws_bytes, const vl_step_state* state,
                       uint32_t tag_offset, vl_stream_t stream);
int vl_lstm_seq_bwd_st(const float* dout, const float* kh, const float* act, const float* cseq, const float* c0, float* dz,
                       float* dh0, float* dc0, int batch, int T, int H, void* ws, size_t ws_bytes, const vl_step_state* state,
                       uint32_t tag_offset, vl_stream_t stream);
/* ---- bidirectional layer: both directions in ONE launch (tf.nn.bidirectional_dynamic_rnn, outputs concatenated) -------------------------
 * A forward cell (_fw) and a backward cell (_bw) of the same hidden size H read the same clips.  The backward cell runs over the reversed
 * live prefix (tf.reverse_sequence with seq_len): its processing step s of clip b works on time index L_b - 1 - s for s < L_b, and every
 * per-row tensor of the _bw set is addressed by that TIME index, so row r of hseq_fw and of hseq_bw belong to the same frame.  Steps
 * s >= L_b are dead and sit on row s: the dead-row contract above holds for both sets (every row written, dead rows of gx / dout never
 * read).  hprev_bw[r] is the h that entered the step of row r -- the backward cell's output of the row AFTER it in time, h0_bw on the last
 * live row -- so hprev_bw^T dz_bw is the recurrent weight gradient; the cell-state predecessor in the backward launch is likewise the
 * previous processing step.  seq_len == NULL: L_b = T.
 * Each argument set is dense as in vl_lstm_seq_fwd / _bwd, except hseq_fw / hseq_bw (written) and dout_fw / dout_bw (read, nullable),
 * whose rows are hseq_ld / dout_ld floats apart (>= H): with hseq_bw = hseq_fw + H and a stride of 2H a layer's output is one
 * [batch T][2H] tensor, and its gradient is read in place.
 * H <= 512 only (the cluster form; no per-clip form), and the device must hold both directions of one group: CUs >= 2 ceil(H/16).
 * Otherwise the calls return an error and launch nothing.  A launch runs 2 G ceil(H/16) workgroups, G <= CUs / (2 ceil(H/16)) groups of
 * <= 8 clips per direction; larger batches take further launches.  `ws` is a workspace of vl_lstm_seq_ws_bytes (the exchange words of the
 * two directions are disjoint slices of it); a launch uses T + 1 tags.  The eager pair refuses a stream that is being captured. */
int vl_lstm_seq_bi_fwd(const float* gx_fw, const float* gx_bw, const float* kh_fw, const float* kh_bw, const float* h0_fw,
                       const float* h0_bw, const float* c0_fw, const float* c0_bw, float* act_fw, float* act_bw, float* cseq_fw,
                       float* cseq_bw, float* hseq_fw, float* hseq_bw, int64_t hseq_ld, float* hprev_fw, float* hprev_bw, int batch, int T,
                       int H, float forget_bias, const int32_t* seq_len, void* ws, size_t ws_bytes, vl_stream_t stream);
int vl_lstm_seq_bi_bwd(const float* dout_fw, const float* dout_bw, int64_t dout_ld, const float* kh_fw, const float* kh_bw,
                       const float* act_fw, const float* act_bw, const float* cseq_fw, const float* cseq_bw, const float* c0_fw,
                       const float* c0_bw, float* dz_fw, float* dz_bw, float* dh0_fw, float* dh0_bw, float* dc0_fw, float* dc0_bw, int batch,
                       int T, int H, const int32_t* seq_len, void* ws, size_t ws_bytes, vl_stream_t stream);
/* Replay-safe forms (no lengths), tags as vl_lstm_seq_fwd_st: launch k of a call uses base origin + tag_offset + k (T + 1);
 * vl_lstm_seq_bi_tag_span = launches x (T + 1), launches = ceil(batch / (8 (CUs / (2 ceil(H/16))))); 0 where the calls are refused. */
size_t vl_lstm_seq_bi_tag_span(int batch, int T, int H);
int vl_lstm_seq_bi_fwd_st(const float* gx_fw, const float* gx_bw, const float* kh_fw, const float* kh_bw, const float* h0_fw,
                          const float* h0_bw, const float* c0_fw, const float* c0_bw, float* act_fw, float* act_bw, float* cseq_fw,
                          float* cseq_bw, float* hseq_fw, float* hseq_bw, int64_t hseq_ld, float* hprev_fw, float* hprev_bw, int batch,
                          int T, int H, float forget_bias, void* ws, size_t ws_bytes, const vl_step_state* state, uint32_t tag_offset,
                          vl_stream_t stream);
int vl_lstm_seq_bi_bwd_st(const float* dout_fw, const float* dout_bw, int64_t dout_ld, const float* kh_fw, const float* kh_bw,
                          const float* act_fw, const float* act_bw, const float* cseq_fw, const float* cseq_bw, const float* c0_fw,
                          const float* c0_bw, float* dz_fw, float* dz_bw, float* dh0_fw, float* dh0_bw, float* dc0_fw, float* dc0_bw,
                          int batch, int T, int H, void* ws, size_t ws_bytes, const vl_step_state* state, uint32_t tag_offset,
                          vl_stream_t stream);
/* ---- GRU recurrence, reset-after form (Keras GRU(reset_after=True), CudnnGRU, torch.nn.GRU), gate blocks z | r | n of width H -------------
 *   gh_t = h_{t-1} . rk + rb        z = sigmoid(gx_z + gh_z)   r = sigmoid(gx_r + gh_r)   n = tanh(gx_n + r * gh_n)
 *   h_t  = z * h_{t-1} + (1 - z) * n
 * gx [batch T][3H]: the input projections x . kernel + bias of all rows (one GEMM, the caller's); rk = recurrent_kernel [H][3H];
 * rb = recurrent_bias [3H] (nullable: zeros); h0 (nullable, [batch][H]: zeros).  The forward writes act [batch T][3H] (the ACTIVATED
 * z, r, n), hcand [batch T][H] (= gh_n with its bias: the backward needs it for the reset gate), hseq and hprev (h_{t-1} of every row).
 * The backward, with din = dout_t + dh (dout nullable: zeros):
 *   dn = din (1 - z)(1 - n^2)   dz' = din (h_{t-1} - n) z (1 - z)   dr' = dn gh_n r (1 - r)
 *   dgx_t = [dz', dr', dn]   dgh_t = [dz', dr', dn r]   dh_{t-1} = din z + dgh_t . rk^T
 * writes dgx and dgh [batch T][3H] (the caller's GEMMs give d kernel = x^T dgx, d bias = colsum dgx, d rk = hprev^T dgh,
 * d rb = colsum dgh, dx = dgx kernel^T) and, when asked, dh0 [batch][H].
 * The cluster form of vl_lstm_seq_fwd only, H <= 512 (larger: an error, nothing launched; there is no per-clip form): a workgroup keeps the
 * 48 columns of rk of its 16 units in LDS.  Launch plan, workspace (vl_lstm_seq_ws_bytes), status word (vl_lstm_seq_status) and test
 * hooks are the LSTM's, and a launch takes its T + 1 tags from the SAME process-wide counter as the LSTM launches, so GRU and LSTM
 * launches may share a workspace.  seq_len (nullable, device int32 [batch]): the dead-row contract above -- a dead step carries h,
 * writes act = hcand = hseq = dgx = dgh = 0 and hprev = the carried h, and never reads its row of gx or dout.
 * The eager pair refuses a stream that is being captured; the _st pair (no lengths) takes its tags as vl_lstm_seq_fwd_st does, and
 * vl_gru_seq_tag_span = launches x (T + 1) counts them (0 where the calls are refused). */
int vl_gru_seq_fwd(const float* gx, const float* rk, const float* rb, const float* h0, float* act, float* hcand, float* hseq,
                   float* hprev, int batch, int T, int H, const int32_t* seq_len, void* ws, size_t ws_bytes, vl_stream_t stream);
int vl_gru_seq_bwd(const float* dout, const float* rk, const float* act, const float* hcand, const float* hprev, float* dgx, float* dgh,
                   float* dh0, int batch, int T, int H, const int32_t* seq_len, void* ws, size_t ws_bytes, vl_stream_t stream);
size_t vl_gru_seq_tag_span(int batch, int T, int H);
int vl_gru_seq_fwd_st(const float* gx, const float* rk, const float* rb, const float* h0, float* act, float* hcand, float* hseq,
                      float* hprev, int batch, int T, int H, void* ws, size_t ws_bytes, const vl_step_state* state, uint32_t tag_offset,
                      vl_stream_t stream);
int vl_gru_seq_bwd_st(const float* dout, const float* rk, const float* act, const float* hcand, const float* hprev, float* dgx,
                      float* dgh, float* dh0, int batch, int T, int H, void* ws, size_t ws_bytes, const vl_step_state* state,
                      uint32_t tag_offset, vl_stream_t stream);
/* Zeroes the exchange words of `ws` (not its time-out word), on the stream: lets the owner of a workspace restart its tags. */
int vl_lstm_seq_ws_clear(void* ws, size_t ws_bytes, vl_stream_t stream);
/* Synchronous read-and-reset of the time-out flag in `ws`: *timed_out = 1 if a workgroup of ANY cluster-form launch on `ws` since
 * the last call of this function gave up waiting for its peers (the cluster form needs all its workgroups resident at once: one
 * per CU; a launch that shares the device with another kernel holding CUs can starve).  Results are then invalid -- it never
 * hangs -- and the caller must discard the step (LRCNEngine / GraphEngine raise). */
int vl_lstm_seq_status(void* ws, int* timed_out);
/* Test hooks of the cluster form, process-wide: spin_limit polls before a gather gives up (0 = the default 2^18);
 * mute_workgroup >= 0: that workgroup of every launch publishes nothing, so its peers time out (-1 = off). */
int vl_lstm_seq_test_hooks(unsigned spin_limit, int mute_workgroup);
/* dst[cols][rows] = src[rows][cols]^T (src row stride ld). */
int vl_transpose(const float* src, int64_t ld, float* dst, int rows, int cols, vl_stream_t stream);

/* ---- apply_temporal_fusion (tf_util.py:4-30) over x[batch][T][H] ---------------------------------
 * method 0 = avg, 1 = last. */
int vl_temporal_fusion_fwd(const float* x, float* y, int batch, int T, int H, int method, vl_stream_t stream);
int vl_temporal_fusion_bwd(const float* dy, float* dx, int batch, int T, int H, int method, vl_stream_t stream);
/* With per-clip lengths (seq_len as above, clamped to 1..T; NULL = the calls above): a clip of length L in a T-step batch gives what it
 * gives in an L-step model.  last = step L - 1 (dynamic_rnn's final output; NOT what tf_util.py would read from the zero-filled
 * output at step T - 1, a zero row: the reference never combines the two, and nobody wants that artefact); avg = the mean over
 * the first L steps (not sum / T).  The backward writes zeros to the dead rows of dx. */
int vl_temporal_fusion_fwd_len(const float* x, float* y, int batch, int T, int H, int method, const int32_t* seq_len,
                               vl_stream_t stream);
int vl_temporal_fusion_bwd_len(const float* dy, float* dx, int batch, int T, int H, int method, const int32_t* seq_len,
                               vl_stream_t stream);

/* ---- attention pooling over time (fusion `attn`: Raffel & Ellis 2015, Yang et al. 2016) ------------------------------
 * Per clip b with L = min(max(seq_len[b], 1), T) live steps (seq_len NULL: L = T), rows h[b][t][HO] and projections u[b][t][A]
 * (u = h W + bias, vl_gemm):  s = tanh(u),  e_t = s_t . c,  alpha = softmax(e_0 .. e_{L-1}) (max-subtracted),  y = sum_t alpha_t h_t.
 * fwd writes s [batch][T][A] (may alias u; dead rows zero), alpha [batch][T] (dead steps zero) and y [batch][HO].
 * bwd reads dy [batch][HO] and writes du [batch][T][A] = de_t c_a (1 - s^2) with de_t = alpha_t (dy . h_t - sum_r alpha_r dy . h_r),
 * dh [batch][T][HO] = alpha_t dy (the direct term only: du W^T is the caller's product) and dcp [batch][A] = sum_t de_t s[t][a], the
 * per-clip partials of c's gradient (vl_colsum them); dead rows of du and dh are zeros.
 * One workgroup per clip, no atomics: a clip's outputs depend on that clip's inputs alone, bit for bit, in any batch.  Rows t >= L of
 * h, u and s are never read.  T <= 1024 (the scores of a clip live in LDS). */
int vl_attn_pool_fwd(const float* u, const float* c, const float* h, const int32_t* seq_len, float* s, float* alpha, float* y,
                     int batch, int T, int HO, int A, vl_stream_t stream);
int vl_attn_pool_bwd(const float* dy, const float* h, const float* s, const float* alpha, const float* c, const int32_t* seq_len,
                     float* du, float* dh, float* dcp, int batch, int T, int HO, int A, vl_stream_t stream);

/* ---- NetVLAD pooling over time (fusion `vlad`: Arandjelovic et al. 2016, Girdhar et al. 2017, Miech et al. 2017; csrc/netvlad.hip,
 * DESIGN 4.30).  Per clip b with L = min(max(seq_len[b], 1), T) live steps (seq_len NULL: L = T), rows h[b][t][HO], K centres c[k][HO]
 * and projections s[b][t][K] (s = h W + beta, vl_gemm):
 *   a_t = softmax_k(s_t) for t < L (max-subtracted), 0 for t >= L;   m_k = sum_t a_tk;   V_k = sum_t a_tk h_t - m_k c_k (t ascending);
 *   r_k = rsqrt(max(|V_k|^2, 1e-12)) (tf.nn.l2_normalize's rule and epsilon);   y[k HO + j] = V_k[j] r_k / sqrt(K) (cluster-major).
 * The whole-descriptor L2 normalisation of the papers is the CONSTANT 1 / sqrt(K), on purpose: behind the intra-normalisation every
 * |U_k| is 1, so the descriptor's norm is sqrt(K), and the radial term of that norm's backward is annihilated by the
 * intra-normalisation's projection.  Clusters are therefore independent of each other in both directions.  A cluster whose |V_k|^2 is
 * not above the epsilon is scaled by the constant 1e6 (stored in r exactly) and shrinks smoothly to nothing.
 * fwd writes a [batch][T][K] (may alias s; dead rows zero), r [batch][K] and y [batch][K HO].
 * bwd reads dy [batch][K HO] and the stored a, r, y; with U_k = sqrt(K) y_k and dU_k = dy_k / sqrt(K),
 *   dV_k = r_k (dU_k - U_k (U_k . dU_k)) where r_k < 1e6, else r_k dU_k;   da_tk = dV_k . (h_t - c_k);
 *   dh [batch][T][HO] = sum_k a_tk dV_k (the direct term only: ds W^T is the caller's product);
 *   ds [batch][T][K] = a_t o (da_t - sum_k a_tk da_tk);   dcp [batch][K HO] = -m_k dV_k, the per-clip partials of c's gradient
 *   (vl_colsum them); dead rows of ds and dh are zeros.  ds, dh and dcp must not overlap an input.
 * One workgroup per clip, no atomics, every sum in a fixed order: a clip's outputs depend on that clip's inputs alone, bit for bit, in
 * any batch.  Rows t >= L of h and s are never read (they may hold NaN).  No host-varying scalar: a captured step replays the launches
 * as they are.  Limits (an error names the one missed, nothing is launched): 2 <= K <= 64, 1 <= HO <= 1024, K HO <= 16384,
 * 1 <= T <= 1024. */
int vl_netvlad_fwd(const float* s, const float* c, const float* h, const int32_t* seq_len, float* a, float* r, float* y, int batch,
                   int T, int HO, int K, vl_stream_t stream);
int vl_netvlad_bwd(const float* dy, const float* h, const float* a, const float* r, const float* y, const float* c,
                   const int32_t* seq_len, float* ds, float* dh, float* dcp, int batch, int T, int HO, int K, vl_stream_t stream);

/* ---- multi-head self-attention over the frames of a clip (rnn_cell `mhsa`; csrc/self_attention.hip) --------------------
 * qkv [batch T][3H]: a row is Q(H) | K(H) | V(H) (the caller's projection x Wqkv + bqkv, vl_gemm); head h of `heads` owns columns
 * h dh .. (h + 1) dh of each block, dh = H / heads.  Per clip b with L = min(max(seq_len[b], 0), T) live steps (seq_len NULL: L = T)
 * and per head:
 *   S[q][k] = (Q_q . K_k) / sqrt(dh) + pos[h][k - q + T - 1]      pos [heads][2T - 1], nullable: no position term
 *   P[q]    = softmax over the live keys k < L of S[q]            (max-subtracted)
 *   ctx_q   = sum_k P[q][k] V_k                                    head h writes its dh columns of ctx [batch T][H]
 * fwd writes P [batch][heads][T][T] and ctx; a dead query row (q >= L) and a dead key column (k >= L) of P are zeros, a dead row of ctx
 * is zeros.  bwd reads dctx [batch T][H], qkv and P as the forward stored it and writes
 *   dV = P^T dctx,  dP = dctx V^T,  dS = P o (dP - rowsum(dP o P)),  dQ = dS K / sqrt(dh),  dK = dS^T Q / sqrt(dh)
 * into dqkv [batch T][3H] (dead rows zeros) and, when dposp is not NULL, dposp [batch][heads][2T - 1][r] = sum over q, k with
 * k - q + T - 1 = r of dS[q][k]: the per-clip partials of pos's gradient (vl_colsum them over the batch rows).
 * DEAD-ROW CONTRACT: rows t >= L of qkv and dctx are never read (they may hold NaN).  One workgroup per (clip, head), no atomics,
 * every sum in a fixed order: a clip's outputs depend on that clip's inputs alone, bit for bit, in any batch.
 * Limits (an error names the one missed, nothing is launched): 1 <= T <= 64, H <= 1024, heads divides H, 8 <= dh <= 128.
 * The launches take no host-varying scalar (1 / sqrt(dh) follows from the shape), so a captured step replays them as they are: there
 * is no _st form. */
int vl_mhsa_fwd(const float* qkv, const float* pos, const int32_t* seq_len, float* P, float* ctx, int batch, int T, int H, int heads,
                vl_stream_t stream);
int vl_mhsa_bwd(const float* dctx, const float* qkv, const float* P, const int32_t* seq_len, float* dqkv, float* dposp, int batch, int T,
                int H, int heads, vl_stream_t stream);
/* y = x in the live rows t < L of x [batch T][W] and 0 in the dead ones (L as above; seq_len not NULL): the input of the first
 * self-attention layer under seq_len, so that a padded frame's features reach no product (x^T dqkv reads every row). */
int vl_live_rows(const float* x, const int32_t* seq_len, float* y, int batch, int T, int W, vl_stream_t stream);

/* ---- the taps of a dilated 1-D convolution over the frames of a clip (rnn_cell `tcn`; csrc/temporal_conv.hip) ----------
 * x [batch T][C], rows clip-major r = b T + t; L = min(max(seq_len[b], 0), T) live steps of clip b (seq_len NULL: L = T).  Tap j of
 * `taps` reads at offset off_j = (j - (taps - 1) / 2) dilation, or, causal, off_j = (j - (taps - 1)) dilation (a step sees itself and
 * the past only).
 *   fwd: cols[b T + t][j C + c] = x[b T + t + off_j][c]  where t < L and 0 <= t + off_j < L, +0.0f everywhere else (dead rows, taps
 *        before the clip's first step or at or behind its L-th): a clip of length L in a T-step batch gives what it gives in an
 *        L-step model with zero padding.  Every element of cols [batch T][taps C] is written; nothing is read where a zero is stored.
 *        The convolution is then the product cols W with W the (taps C, out) flat form of a (taps, C, out) kernel (vl_gemm).
 *   bwd: for t < L, dx[b T + t][c] = dres[b T + t][c] + sum over j ASCENDING with 0 <= t - off_j < L of dcols[b T + t - off_j][j C + c]:
 *        plain fp32 adds in that order, starting from the dres term (the gradient of a residual path around the convolution), or from
 *        +0.0f when dres is NULL.  Dead rows of dx are +0.0f.  A gather per output element: no atomics.
 * DEAD-ROW CONTRACT: rows t >= L of x, dcols and dres are never read (they may hold NaN).  A clip's outputs depend on that clip's
 * inputs alone, bit for bit, in any batch.  16-byte loads and stores where C % 4 == 0 and every pointer is 16-byte aligned, a scalar
 * path otherwise.  Index arithmetic is 64-bit.
 * Limits (an error names the one missed, nothing is launched): batch, T, C >= 1; 1 <= taps <= 9, odd unless causal;
 * 1 <= dilation <= 65536 (a dilation of T or more is legal: only the zero-offset tap is live); C <= 1024; seq_len and dres alone may
 * be NULL.  The launches take no host-varying scalar, so a captured step replays them as they are: there is no _st form. */
int vl_tconv_cols_fwd(const float* x, const int32_t* seq_len, float* cols, int batch, int T, int C, int taps, int dilation, int causal,
                      vl_stream_t stream);
int vl_tconv_cols_bwd(const float* dcols, const float* dres, const int32_t* seq_len, float* dx, int batch, int T, int C, int taps,
                      int dilation, int causal, vl_stream_t stream);

/* ---- the encoder block around the self-attention layer (sa_block `encoder`; csrc/layer_norm.hip) -----------------------
 * Rows are [clips T][W], 8 <= W <= 1024; L = min(max(seq_len[b], 0), T) live steps of clip b (seq_len NULL: L = T).
 * vl_add_layer_norm_fwd: s = x + r (r NULL: s = x), stored to `sum` where it is not NULL; y = (s - mean) rstd gamma + beta with
 *   mean = sum(s) / W, rstd = 1 / sqrt(sum((s - mean)^2) / W + eps) (the variance of the CENTRED values); stats [clips T][2] = mean,
 *   rstd.  One launch is a layer norm, or a residual add with the norm that follows it.
 * vl_layer_norm_bwd: from s and stats as the forward stored them, with x^ = (s - mean) rstd and dy^ = dy gamma:
 *   dx = rstd (dy^ - mean(dy^) - x^ mean(dy^ x^)) + dres (dres NULL: no such term; it is the gradient that arrives on the residual
 *   stream beside the norm), and dgb_partial [clips][2W] = the clip's sums over its live rows, t ascending, of dy x^ (columns 0 .. W:
 *   gamma's gradient) and dy (columns W .. 2W: beta's); vl_colsum them over the clips.
 * DEAD-ROW CONTRACT: rows t >= L of x, r, dy, s, stats and dres are never read (they may hold NaN); dead rows of y, sum, stats and dx
 * are zeros, a clip of length 0 has a zero partial row.  One wave per row, no atomics, every sum in a fixed order: a clip's outputs
 * depend on that clip's inputs alone, bit for bit, in any batch.  x, r, sum, y (dy, s, dres, dx) must not overlap one another.
 * vl_gelu_fwd: f = u Phi(u), the exact (erf) form; vl_gelu_bwd: du = df (Phi(u) + u phi(u)); du may be df.  Finite for every finite u,
 * the gradient 0 and 1 where erf saturates.
 * A refused call (a null required pointer, a size outside the limits, eps not positive) launches nothing.  No host-varying argument
 * but eps, a constant of the model: a captured step replays the launches as they are; there is no _st form. */
int vl_add_layer_norm_fwd(const float* x, const float* r, float* sum, float* y, const float* gamma, const float* beta, float* stats,
                          int clips, int T, int W, float eps, const int32_t* seq_len, vl_stream_t stream);
int vl_layer_norm_bwd(const float* dy, const float* s, const float* gamma, const float* stats, const float* dres, float* dx,
                      float* dgb_partial, int clips, int T, int W, const int32_t* seq_len, vl_stream_t stream);
int vl_gelu_fwd(const float* u, float* f, int64_t count, vl_stream_t stream);
int vl_gelu_bwd(const float* df, const float* u, float* du, int64_t count, vl_stream_t stream);

/* ---- dropout of the self-attention model: weights, residual branches, drop path (sa_attn_dropout, sa_dropout, sa_drop_path;
 * csrc/self_attention.hip, csrc/layer_norm.hip).  No mask buffer: every draw is a function of counters.
 * MASK DEFINITION.  The generator of vl_fc_dropout_fwd under a stream constant of its own:
 *   s = seed ^ splitmix64(0x5AD000000000 + salt);  h = splitmix64(s ^ splitmix64(e));  kept = (h >> 40) * 2^-24 < keep
 * The constant is above 2^45, so with a 32-bit salt no stream is one of vl_fc_dropout_fwd's (0xFC00 + salt) and none is the bare
 * seed of vl_dropout_fwd.  The engines pack salt = node << 12 | layer << 2 | site with site 0 = attention weights, 1 = elements of
 * the attention branch, 2 = elements of the feed-forward branch, 3 = path draws: every (node, layer, site) is a stream of its own.
 * Counters e are GLOBAL: clip0 is the index in the whole batch of the launch's first clip, so clip g of the batch draws the same
 * masks whichever rank or launch holds it (0 <= clip0 < 2^31 - clips):
 *   weights          e = (((clip0 + b) heads + h) T + q) T + k
 *   branch elements  e = ((clip0 + b) T + t) W + col
 *   path             e = 2 (clip0 + b) + branch            branch 0 = attention, 1 = feed-forward
 * Under seq_len the dead rows' and keys' draws are simply unused.  keep and keep_path lie in (0, 1] (NaN refused); a keep of exactly 1
 * draws nothing.  The _st forms take seed = (state->step << 20) ^ 0x5DEECE66D from the step state when the kernel runs.
 * vl_mhsa_drop_fwd: vl_mhsa_fwd with ctx = (P o F) V, F = kept ? fl(1 / keep) : 0, one fp32 product per weight; P is stored UNDROPPED.
 * vl_mhsa_drop_bwd: F drawn again; dV = (P o F)^T dctx, dP = (dctx V^T) o F, dS = P o (dP - rowsum(dP o P)), the rest as vl_mhsa_bwd.
 *   Same launch shape, LDS and dead-row contract as vl_mhsa_fwd / _bwd, and at keep = 1 their bits.
 * BRANCH FACTOR, in fp32 so that a host restatement gives the same bits:  fe = kept_e ? 1.0f / keep : 0,  fp = path_kept ? 1.0f /
 *   keep_path : 0,  f = fmul(fe, fp)  (a factor whose keep is 1 is exactly 1).
 * vl_add_layer_norm_drop_fwd: vl_add_layer_norm_fwd with s = fadd(x, fmul(r, f)), no fma (r required); `sum` receives the dropped sum,
 *   so vl_layer_norm_bwd needs no change.  With both keeps 1 it is vl_add_layer_norm_fwd bit for bit.
 * vl_branch_drop_grad: dr = fmul(ds, f) over [clips T][W], zeros in the dead rows (ds is not read there): the gradient that enters a
 *   dropped branch.  16-byte accesses where both pointers are 16-byte aligned; the bits do not depend on alignment.  dr must not
 *   overlap ds.
 * A refused call (null pointer, a size outside the limits of the sibling launch, a keep outside (0, 1], clip0 out of range) launches
 * nothing. */
int vl_mhsa_drop_fwd(const float* qkv, const float* pos, const int32_t* seq_len, float* P, float* ctx, int batch, int T, int H, int heads,
                     float keep, uint64_t seed, uint32_t salt, int64_t clip0, vl_stream_t stream);
int vl_mhsa_drop_fwd_st(const float* qkv, const float* pos, const int32_t* seq_len, float* P, float* ctx, int batch, int T, int H,
                        int heads, float keep, const vl_step_state* state, uint32_t salt, int64_t clip0, vl_stream_t stream);
int vl_mhsa_drop_bwd(const float* dctx, const float* qkv, const float* P, const int32_t* seq_len, float* dqkv, float* dposp, int batch,
                     int T, int H, int heads, float keep, uint64_t seed, uint32_t salt, int64_t clip0, vl_stream_t stream);
int vl_mhsa_drop_bwd_st(const float* dctx, const float* qkv, const float* P, const int32_t* seq_len, float* dqkv, float* dposp, int batch,
                        int T, int H, int heads, float keep, const vl_step_state* state, uint32_t salt, int64_t clip0,
                        vl_stream_t stream);
int vl_add_layer_norm_drop_fwd(const float* x, const float* r, float* sum, float* y, const float* gamma, const float* beta, float* stats,
                               int clips, int T, int W, float eps, const int32_t* seq_len, float keep, float keep_path, uint64_t seed,
                               uint32_t salt_elem, uint32_t salt_path, int branch, int64_t clip0, vl_stream_t stream);
int vl_add_layer_norm_drop_fwd_st(const float* x, const float* r, float* sum, float* y, const float* gamma, const float* beta,
                                  float* stats, int clips, int T, int W, float eps, const int32_t* seq_len, float keep, float keep_path,
                                  const vl_step_state* state, uint32_t salt_elem, uint32_t salt_path, int branch, int64_t clip0,
                                  vl_stream_t stream);
int vl_branch_drop_grad(const float* ds, float* dr, int clips, int T, int W, const int32_t* seq_len, float keep, float keep_path,
                        uint64_t seed, uint32_t salt_elem, uint32_t salt_path, int branch, int64_t clip0, vl_stream_t stream);
int vl_branch_drop_grad_st(const float* ds, float* dr, int clips, int T, int W, const int32_t* seq_len, float keep, float keep_path,
                           const vl_step_state* state, uint32_t salt_elem, uint32_t salt_path, int branch, int64_t clip0,
                           vl_stream_t stream);

/* ---- imresize: scipy.misc.imresize(image, shape) of Dataset.process_image (dataset_.py:481-495: imgproc `raw_resize` to the raw
 * shape, `resize` to the network input size; also serialize.py:424-425) = PIL Image.resize(BILINEAR) on uint8, bit-exact:
 * Pillow's two-pass fixed-point resample (22-bit coefficients, uint8 intermediate, horizontal pass first; csrc/resize.hip).
 * The descriptor holds the coefficient tables of one (h, w) -> (oh, ow) pair on the device.  Images are uint8 [n][h][w][3] (HWC). */
typedef struct vl_resize_desc vl_resize_desc;
int vl_resize_create(vl_resize_desc** out, int h, int w, int oh, int ow, int channels);
void vl_resize_destroy(vl_resize_desc* d);
/* bytes of the uint8 intermediate vl_resize_u8 needs for n images (0 when at most one axis changes size) */
size_t vl_resize_tmp_bytes(const vl_resize_desc* d, int n);
int vl_resize_u8(const vl_resize_desc* d, const uint8_t* src, uint8_t* tmp, uint8_t* dst, int n, vl_stream_t stream);

/* ---- tensor-list plumbing of multi-input pipelines (tf_util.py:99-192) ------------------------------------------------
 * vl_copy2d: dst[r][c] = src[r][c] for r < rows, c < cols with row strides src_ld / dst_ld (src_ld 0 repeats one row).
 * tf.concat / vec_seq_concat (tf_util.py:99-124), the ibias insertion (tf_util.py:154-176) and replicate_auxilliary_tensor
 * (tf_util.py:182-192) are such block copies, forward and backward. */
int vl_copy2d(const float* src, int64_t src_ld, float* dst, int64_t dst_ld, int rows, int cols, vl_stream_t stream);
/* op 0: a + b; 1: mean of the two (tf.reduce_mean, fusion avg, tf_util.py:142-143); 2: max (fusion maximum, :144-145). */
int vl_eltwise2(const float* a, const float* b, float* out, int64_t count, int op, vl_stream_t stream);
/* gradient of max(a, b) w.r.t. both: the larger input takes d, equal inputs share it evenly (tf.reduce_max's _MinOrMaxGrad). */
int vl_max2_grad(const float* a, const float* b, const float* d, float* da, float* db, int64_t count, vl_stream_t stream);
/* apply_tensor_list_fusion avg | maximum over a LIST of n <= 8 equally shaped tensors (tf.reduce_mean / tf.reduce_max over the
 * stacked list, tf_util.py:142-145).  ins / dins: HOST arrays of n device pointers.  op 0: mean, 1: maximum.
 * vl_fuse_n_grad writes dins[i] (null entries are skipped): d / n for the mean; for the maximum the inputs equal to it share d
 * evenly (ins may be null for op 0). */
int vl_fuse_n(const float* const* ins, int n, float* out, int64_t count, int op, vl_stream_t stream);
int vl_fuse_n_grad(const float* const* ins, int n, const float* d, float* const* dins, int64_t count, int op, vl_stream_t stream);

/* ---- tf.nn.dropout (lstm.py:50-56): y = x * mask / keep, mask ~ Bernoulli(keep) ------------------
 * Counter-based RNG keyed by (seed, element index); mask (uint8) is written for the backward. */
int vl_dropout_fwd(const float* x, float* y, uint8_t* mask, int64_t count, float keep, uint64_t seed, vl_stream_t stream);
int vl_dropout_bwd(const float* dy, const uint8_t* mask, float* dx, int64_t count, float keep, vl_stream_t stream);
/* vl_dropout_fwd with seed = (state->step << 20) ^ 0x5DEECE66D, read from the step state when the kernel runs. */
int vl_dropout_fwd_st(const float* x, float* y, uint8_t* mask, int64_t count, float keep, const vl_step_state* state,
                      vl_stream_t stream);

/* ---- dropout on the ReLU'd fc layers of the tower (Caffe AlexNet's drop6 / drop7), in place, no mask buffer ----------------------
 * y[e] = kept(e) ? y[e] / keep : 0 over `count` floats, any count >= 1, any 4-byte aligned pointer (16-byte accesses over the part
 * of the range that is 16-byte aligned, scalar head and tail).  kept(e) is a function of (seed, salt, e) alone, e counted from the
 * pointer given:   s = seed ^ splitmix64(0xFC00 + salt);  h = splitmix64(s ^ splitmix64(e));  kept = (h >> 40) * 2^-24 < keep
 * (splitmix64: the generator of vl_dropout_fwd; the salt separates the layers' and towers' masks from each other and from
 * vl_dropout_fwd's, which uses the bare seed).  y being a ReLU output, y > 0 afterwards means "ReLU active and kept": */
int vl_fc_dropout_fwd(float* y, int64_t count, float keep, uint64_t seed, uint32_t salt, vl_stream_t stream);
/* The same with seed = (state->step << 20) ^ 0x5DEECE66D, read from the step state when the kernel runs (as vl_dropout_fwd_st). */
int vl_fc_dropout_fwd_st(float* y, int64_t count, float keep, const vl_step_state* state, uint32_t salt, vl_stream_t stream);
/* ... so ReluGrad and the dropout's gradient are one pass over the dropped output: d[e] = y[e] > 0 ? d[e] / keep : 0, in place. */
int vl_relu_dropout_grad(float* d, const float* y, int64_t count, float keep, vl_stream_t stream);

/* ---- loss: mean_b softmax_cross_entropy_with_logits (train.py:120-123) + accuracy (142-149) ----
 * labels: int32 one/multi-hot [batch][classes] (the reference's labels placeholder, train.py:117).
 * dlogits = (softmax - labels) * grad_scale   (grad_scale = 1/global_batch); may be NULL.
 * stats[0] += sum_b loss_b, stats[1] += number of rows with argmax(logits) == argmax(labels);
 * zero `stats` first (vl_fill).  rows: float[2*batch] workspace receiving the per-row losses and hits (one wave per row over
 * the whole chip, summed in a fixed order); NULL walks every row in one workgroup (same result, for small batches only). */
int vl_softmax_xent(const float* logits, const int32_t* labels, float* dlogits, float* stats, float* rows,
                    int batch, int classes, float grad_scale, vl_stream_t stream);
/* Rows are the steps of batch / T sequences (row r = b T + t) with per-clip lengths seq_len[batch / T]: a row with t >= seq_len[b]
 * is padding (the reference's non_padding_index, dataset_.py:327-383).  It is not read (it may hold NaN), adds nothing to `stats`
 * and gets dlogits = 0.  The caller divides by the live-row count: grad_scale = 1 / sum(seq_len).  seq_len NULL = vl_softmax_xent. */
int vl_softmax_xent_len(const float* logits, const int32_t* labels, float* dlogits, float* stats, float* rows,
                        int batch, int classes, float grad_scale, const int32_t* seq_len, int T, vl_stream_t stream);
/* vl_softmax_xent_len with label smoothing and top-k hits, one launch (tf.losses.softmax_cross_entropy(label_smoothing=smoothing)):
 * y'_c = labels_c (1 - smoothing) + smoothing / classes takes the labels' place, per element, in the row loss sum_c y'_c (lse - z_c)
 * and in dlogits = (softmax - y') * grad_scale; smoothing == 0 gives vl_softmax_xent_len's bits.  0 <= smoothing < 1.
 * stats is float[3]: [0] += row losses, [1] += top-1 hits, [2] += top-k hits (top_k == 0: untouched).  With t the first arg-max of a
 * label row, rank = #{c : z_c > z_t} + #{c < t : z_c == z_t}; the row is a top-k hit iff rank < top_k (top_k == 1: the top-1 hit;
 * top_k >= classes: every live row).  rows: float[3*batch] (losses | top-1 hits | top-k hits) or NULL, as above.  seq_len NULL:
 * every row is live.  No atomics: the sums are bitwise reproducible. */
int vl_softmax_xent_ls(const float* logits, const int32_t* labels, float* dlogits, float* stats, float* rows,
                       int batch, int classes, float grad_scale, const int32_t* seq_len, int T, float smoothing, int top_k,
                       vl_stream_t stream);

/* ---- mixup (Zhang et al. 2018): clip i is paired with clip clips - 1 - i --------------
 * vl_mixup_pairs: x is [clips][clip_elems], blended in place per pair: x_i' = lam x_i + (1 - lam) x_p, x_p' = lam x_p + (1 - lam) x_i,
 * whatever the layout inside a clip (halo and padding zeros blend to zero).  dtype 0: fp32; 1: packed bf16, blended in fp32 and
 * rounded to nearest even (clip_elems a multiple of 8).  lam_dev != NULL: *lam_dev is read when the kernel runs (capturable) and lam
 * is ignored; else 0 <= lam <= 1.  lam == 1 leaves every bit.  The middle clip of an odd count is not touched; clips <= 1 launches
 * nothing. */
int vl_mixup_pairs(void* x, int dtype, int clips, int64_t clip_elems, float lam, const float* lam_dev, vl_stream_t stream);
/* vl_softmax_xent_ls (without lengths) on the labels of the blended clips: y' = lam y_r + (1 - lam) y_p, then the smoothing.  Rows are
 * batch / rows_per_clip clips of rows_per_clip rows; the partner of row r is row r % rows_per_clip of clip
 * batch / rows_per_clip - 1 - r / rows_per_clip (a row that is its own partner reads one label row).  Hits are counted against the
 * row's OWN labels.  lam / lam_dev as above; lam == 1 gives vl_softmax_xent_ls's bits.  stats, rows, both launch forms: as there. */
int vl_softmax_xent_mix(const float* logits, const int32_t* labels, float* dlogits, float* stats, float* rows, int batch, int classes,
                        float grad_scale, int rows_per_clip, float smoothing, int top_k, float lam, const float* lam_dev,
                        vl_stream_t stream);
/* Class weights and the focal loss (Lin et al. 2017) on top of both, one launch.  With p = softmax(z), y' the label row
 * after the mixup blend and then the smoothing exactly as above, w = class_weights (float[classes] on the device, read when the
 * kernel runs; NULL = all ones) and m_c = (1 - p_c)^gamma (gamma == 0: m_c = 1 exactly, no pow):
 *     loss = sum_c w_c y'_c m_c (-log p_c)
 *     a_c  = w_c y'_c (m_c - gamma (1 - p_c)^(gamma - 1) p_c log p_c),  A = sum_c a_c,  dlogits_j = (p_j A - a_j) * grad_scale
 * with log p_c = z_c - lse, 1 - p_c = -expm1(log p_c), and the second term of a_c 0 where 1 - p_c == 0 (its limit: a saturated row
 * stays finite at every gamma).  The weights sit inside the class sum (PyTorch's rule for probability targets), so a smoothed or
 * mixed row is weighted by the classes it carries.  The normaliser stays the row count: grad_scale is the caller's 1 / live rows
 * (Keras' class_weight, tf.losses' SUM_OVER_BATCH_SIZE), NOT 1 / sum of the rows' weights as in PyTorch's hard-label mean.
 * seq_len / T as in vl_softmax_xent_ls; rows_per_clip, lam, lam_dev as in vl_softmax_xent_mix (rows_per_clip 1, lam 1 and lam_dev
 * NULL: no partner row is read); lengths together with rows_per_clip > 1 or a lambda are refused.  gamma must be finite and >= 0.
 * Hits and top-k hits are unweighted, against the row's own labels.  stats float[3], rows float[3*batch] or NULL, both launch forms,
 * no atomics: as there.  All weights 1 and gamma 0 computes what _ls / _mix compute (not bit for bit: p A and p round differently). */
int vl_softmax_xent_wf(const float* logits, const int32_t* labels, float* dlogits, float* stats, float* rows, int batch, int classes,
                       float grad_scale, const int32_t* seq_len, int T, int rows_per_clip, float smoothing, int top_k, float lam,
                       const float* lam_dev, const float* class_weights, float gamma, vl_stream_t stream);
/* The multi-label loss: independent sigmoids per class on multi-hot labels (0 / 1 per class, any number of ones, none
 * included), one launch in the form of the softmax ones.  Per element, z the logit, y the label, yp the partner row's label as in
 * vl_softmax_xent_mix, q = pos_weights[c] (float[classes] on the device, read when the kernel runs; NULL = ones):
 *     t = lam y + (1 - lam) yp  (lam 1 or a row that is its own partner: y exactly),  then  t = t (1 - smoothing) + smoothing / 2
 *     log p = -(max(-z, 0) + sp),  log(1 - p) = -(max(z, 0) + sp),  sp = log1p(exp(-|z|))
 *   gamma == 0:  l = -(q t log p + (1 - t) log(1 - p))             (tf.nn.weighted_cross_entropy_with_logits; q = 1: torch's
 *                dl/dz = p (q t + 1 - t) - q t                      BCEWithLogitsLoss, with pos_weight = q otherwise)
 *   gamma > 0:   l = q t (1 - p)^g (-log p) + (1 - t) p^g (-log(1 - p))        (Lin et al. 2017, the sigmoid form)
 *                dl/dz = q t (1 - p)^g (g p log p - (1 - p)) + (1 - t) p^g (p - g (1 - p) log(1 - p)),  finite at any z and gamma
 * The row loss is the MEAN over the classes and dlogits = dl/dz * grad_scale / classes: with the caller's grad_scale = 1 / live rows
 * the summed loss over the rows is the element mean of Keras / torch / tf.losses, and the gradients are `classes` times smaller than
 * a softmax row's.  stats float[3] += {row losses, hit@1 rows (the first arg-max of the logits is a class with y > 0, the row's OWN
 * labels), exact-match rows ((z_c > 0) == (y_c > 0) for every class; z == 0 predicts negative; a row without labels is never a hit
 * and is exact iff no logit is positive)}, in xent_sum_kernel's fixed order; rows float[3*batch] or NULL (one workgroup walks the
 * batch); no atomics, bitwise reproducible.  seq_len / T: the dead-row contract of vl_softmax_xent_ls (not read, nothing added,
 * dlogits row zeros); lengths together with rows_per_clip > 1 or a lambda are refused.  dlogits may be NULL.  smoothing in [0, 1),
 * lam in [0, 1] unless lam_dev is given, gamma finite and >= 0. */
int vl_sigmoid_xent(const float* logits, const int32_t* labels, float* dlogits, float* stats, float* rows, int batch, int classes,
                    float grad_scale, const int32_t* seq_len, int T, int rows_per_clip, float smoothing, float lam, const float* lam_dev,
                    const float* pos_weights, float gamma, vl_stream_t stream);

/* ---- CutMix / VideoMix (Yun et al. 2019, 2020): one box swapped between clip i and clip clips - 1 - i ---------------
 * The box is {t0, t1, y0, y1, x0, x1}, half-open, in frames of the clip and pixels of the out_h x out_w frame conv1 sees; all channels
 * are swapped, frame t of clip i with frame t of its partner, bit for bit, in place; no byte outside the box changes (halo, phase
 * padding, unused channel slots).  box_dev != NULL: six device words read when the kernel runs (capturable, the grid does not depend
 * on them; box_host is ignored); every bound is clamped to its axis and a reversed or empty range swaps nothing.  Else box_host: six
 * host ints inside [0, fpc] x [0, out_h] x [0, out_w], no reversed range.  The middle clip of an odd count is not touched; clips <= 1
 * or an empty host box launches nothing.
 * vl_cutmix_pairs: x0 is vl_input_prep_u8's destination for clips * fpc frames (dst_halo = halo, dst_phase = phase): pixel (y, x) of
 * channel c is in plane c * phase + (x + halo) % phase, row y + halo, column (x + halo) / phase. */
int vl_cutmix_pairs(float* x0, int clips, int fpc, int out_h, int out_w, int halo, int phase, const int32_t* box_host,
                    const int32_t* box_dev, vl_stream_t stream);
/* The same on vl_input_prep_u8_s2d's destination for the descriptor d (the frame is d's h x w): element j of chunk (cb, R, S) is
 * channel cp = 8 cb + j with px = cp % s, py = (cp / s) % s, c = cp / s^2, at pixel (s R + py - pt, s S + px - pl). */
int vl_cutmix_pairs_s2d(const vl_conv_desc* d, void* xb, int clips, int fpc, const int32_t* box_host, const int32_t* box_dev,
                        vl_stream_t stream);

/* ---- random erasing (Zhong et al. 2017): every clip's own box overwritten in place, write-only ----------------------
 * table_dev: DEVICE int32 [clips][8] = {t0, t1, y0, y1, x0, x1, key_lo, key_hi} per clip, read when the kernel runs (capturable; the
 * grid depends on clips, fpc and the frame height only).  The box is half-open, in frames of the clip and pixels of the frame conv1
 * sees; every bound is clamped to its axis as a CutMix device box is, and a reversed or empty range writes nothing for that clip.
 * All channels of the box are overwritten; no byte outside it changes (halo, phase padding, unused channel slots, other clips).
 * mode 0 (zero): +0.0f, the mean colour of a mean-subtracted input (0x0000 packed).
 * mode 1 (clip): one value per (clip, channel c), noise(key, 2^40 + c).
 * mode 2 (pixel): noise(key, ((t C + c) H + y) W + x) with t the frame within the clip, c the stored channel, (y, x) the logical pixel
 *   and C, H, W the channel count and frame size (3, out_h, out_w for x0; d's cin, h, w for the packed form) -- a function of the
 *   logical coordinates, never of an address.
 * noise(key, e): key = key_hi << 32 | key_lo (both as unsigned words); h = splitmix64(key ^ splitmix64(e)) with the splitmix64 of
 *   vl_dropout_fwd; s = the sum of the four 16-bit fields of h; noise = (float)(s - 131070) * scale: an integer and ONE fp32 multiply.
 *   s has mean 131070 and standard deviation sqrt(4 (65536^2 - 1) / 12) = 37837.22723720648, so scale = std / 37837.22723720648.
 * The packed form rounds each value to bf16 to nearest even; a 16-byte chunk wholly inside the box is stored without being read, a
 * chunk cut by a box edge is read, selected per element and written back.
 * Contract: vl_erase_boxes followed by vl_s2d_c8_from_x0 equals vl_input_prep_u8_s2d followed by vl_erase_boxes_s2d bit for bit.
 * Refused without a launch: null pointers, clips < 0, fpc outside [1, 65535], a bad size, mode outside 0..2, a non-finite scale.
 * clips == 0 launches nothing.
 * vl_erase_boxes: x0 is vl_input_prep_u8's destination for clips * fpc frames (dst_halo = halo, dst_phase = phase; the layout is
 * stated at vl_cutmix_pairs). */
int vl_erase_boxes(float* x0, int clips, int fpc, int out_h, int out_w, int halo, int phase, const int32_t* table_dev, int mode,
                   float scale, vl_stream_t stream);
/* The same on vl_input_prep_u8_s2d's destination for the descriptor d (the element map is stated at vl_cutmix_pairs_s2d). */
int vl_erase_boxes_s2d(const vl_conv_desc* d, void* xb, int clips, int fpc, const int32_t* table_dev, int mode, float scale,
                       vl_stream_t stream);

/* ---- optimizer: clip_by_global_norm + GradientDescentOptimizer (train.py:199-222) ---------------
 * vl_sumsq: out[0] (+)= sum g^2 over count elements (ws: float[1024]); accumulate != 0 adds to out. */
int vl_sumsq(const float* g, int64_t count, float* out, float* ws, int accumulate, vl_stream_t stream);
/* w -= lr * gscale * clip_scale * g with clip_scale = clip_norm / max(gscale*sqrt(*sumsq), clip_norm)
 * (1 if clip_norm <= 0 or sumsq == NULL).  gscale folds the 1/world averaging of DP all-reduce.
 * skip (device word, may be NULL): when *skip != 0 at execution time the launch changes nothing -- the step's gradients are invalid
 * (a cluster-form LSTM launch of the step timed out, vl_status_or) and must not reach the weights; the host raises when it next reads
 * the status (vl_lstm_seq_status). */
int vl_sgd_apply(float* w, const float* g, int64_t count, float lr, float clip_norm, const float* sumsq,
                 float gscale, const uint32_t* skip, vl_stream_t stream);
/* tf.train.AdamOptimizer (train.py:205-206) with TF defaults beta1=.9 beta2=.999 eps=1e-8; step >= 1.  skip: as vl_sgd_apply (m, v
 * stay untouched too). */
int vl_adam_apply(float* w, const float* g, float* m, float* v, int64_t count, float lr, float clip_norm,
                  const float* sumsq, float gscale, int step, const uint32_t* skip, vl_stream_t stream);
/* *dst = (init ? 0 : *dst) | (the sticky time-out word of an LSTM cluster workspace != 0), on the stream: collects the `skip` word of a
 * step without a host round trip (init != 0 for the step's first workspace; the workspace's own word stays set until
 * vl_lstm_seq_status reads it). */
int vl_status_or(uint32_t* dst, const void* lstm_ws, int init, vl_stream_t stream);

/* ---- step state (vl_step_state above) ---------------------------------------------------------------------------------------
 * vl_step_state_set: one single-lane launch that writes step, lr and tag_origin, and adam_lr = lr sqrt(1 - 0.999^(step+1)) /
 * (1 - 0.9^(step+1)) computed on the HOST by the same code as vl_adam_apply (device pow need not round like the host's: the
 * replayed update must equal the eager one bit for bit).  step >= 0. */
size_t vl_step_state_bytes(void);
int vl_step_state_set(vl_step_state* state, int64_t step, float lr, uint32_t tag_origin, vl_stream_t stream);
/* The same for a micro-step of an accumulated update (vl_grad_accumulate): state->step = draw_step, the dropout seed's input, while
 * adam_lr comes from update_step by the code above.  vl_step_state_set(s, step, ...) is vl_step_state_set_micro(s, step, step, ...). */
int vl_step_state_set_micro(vl_step_state* state, int64_t update_step, int64_t draw_step, float lr, uint32_t tag_origin,
                            vl_stream_t stream);
/* One single-lane launch that writes state->ema_rate and nothing else (vl_step_state_set and _set_micro never touch that field).
 * 0 < rate <= 1, finite. */
int vl_step_state_set_ema(vl_step_state* state, float rate, vl_stream_t stream);
/* vl_sgd_apply with lr = state->lr; vl_adam_apply with the step size state->adam_lr (= count state->step + 1). */
int vl_sgd_apply_st(float* w, const float* g, int64_t count, const vl_step_state* state, float clip_norm, const float* sumsq,
                    float gscale, const uint32_t* skip, vl_stream_t stream);
int vl_adam_apply_st(float* w, const float* g, float* m, float* v, int64_t count, const vl_step_state* state, float clip_norm,
                     const float* sumsq, float gscale, const uint32_t* skip, vl_stream_t stream);

/* ---- tiered update: per-range learning-rate multipliers, untouched gaps ------------------------------------------------------
 * A tier table lists the half-open element ranges [begin, end) of the flat buffers that an update touches, each with the multiplier
 * of its learning rate.  The table is sorted and disjoint, lies inside [0, count), has 1 .. VL_MAX_LR_TIERS entries and multipliers
 * that are finite and > 0; anything else is refused on the host.  It is read on the host and travels BY VALUE in the launch arguments:
 * the caller's array may be freed as soon as the call returns, and a captured step needs no device table.
 * Elements outside every tier are neither loaded nor stored (w, g and Adam's m, v alike: they may hold anything, NaN included).
 * Inside a tier with multiplier mult the arithmetic is that of the plain call with lr replaced by the fp32 product lr * mult (Adam:
 * step size adam_lr * mult), so the tier's elements get, bit for bit, what the plain entry point gives on that sub-range with
 * lr' = (float)(lr * mult).  sumsq and clip_norm mean what they mean there: ONE global norm, whatever the table.  One launch per call,
 * with the plain call's grid.  The plain entry points above are the table {0, count, 1.0f} of the same kernels. */
#define VL_MAX_LR_TIERS 16
typedef struct vl_lr_tier {
    int64_t begin, end;
    float lr_mult;
} vl_lr_tier;
int vl_sgd_apply_tiers(float* w, const float* g, int64_t count, float lr, float clip_norm, const float* sumsq,
                       float gscale, const uint32_t* skip, const vl_lr_tier* tiers, int n_tiers, vl_stream_t stream);
int vl_adam_apply_tiers(float* w, const float* g, float* m, float* v, int64_t count, float lr, float clip_norm,
                        const float* sumsq, float gscale, int step, const uint32_t* skip, const vl_lr_tier* tiers, int n_tiers,
                        vl_stream_t stream);
int vl_sgd_apply_tiers_st(float* w, const float* g, int64_t count, const vl_step_state* state, float clip_norm, const float* sumsq,
                          float gscale, const uint32_t* skip, const vl_lr_tier* tiers, int n_tiers, vl_stream_t stream);
int vl_adam_apply_tiers_st(float* w, const float* g, float* m, float* v, int64_t count, const vl_step_state* state, float clip_norm,
                           const float* sumsq, float gscale, const uint32_t* skip, const vl_lr_tier* tiers, int n_tiers,
                           vl_stream_t stream);
/* out[0] = sum g^2 over the elements inside the tiers (the multipliers are ignored; elements outside are not read); ws: float[1024].
 * Two stages in a fixed order like vl_sumsq: the same bits from run to run.  Not the summation order of vl_sumsq: callers whose table
 * is the single full range call vl_sumsq. */
int vl_sumsq_tiers(const float* g, int64_t count, const vl_lr_tier* tiers, int n_tiers, float* out, float* ws, vl_stream_t stream);

/* ---- SGD with momentum / Nesterov: tf.train.MomentumOptimizer(lr, momentum, use_nesterov) -------------------------------------------
 * (= torch.optim.SGD(momentum, dampening=0, nesterov)).  The learning rate stays OUTSIDE the accumulator, so a schedule that changes
 * lr rescales no history; clipping and gscale scale the gradient BEFORE it is accumulated.  Per element, every step one fp32 rounding,
 * in this order (no contraction is left to the compiler, and the scalar and 16-byte loops share the element function):
 *     sc   = the clip scale of vl_sgd_apply (gscale * clip_norm / max(gscale*sqrt(*sumsq), clip_norm), or gscale)
 *     gi   = g * sc
 *     a'   = fma(momentum, a, gi)                      the accumulator `accum`, count floats, zero before the first step
 *     w'   = fma(-lr_k, a', w)                         nesterov == 0
 *     w'   = fma(-lr_k, fma(momentum, a', gi), w)      nesterov != 0
 *     lr_k = (float)(lr * tier.lr_mult)                the tier changes lr only, never the accumulator
 * tiers == NULL && n_tiers == 0 is the full range {0, count, 1.0f}; any other table obeys the rules above, and elements outside every
 * tier are neither loaded nor stored (w, g and accum alike).  accum != NULL, 0 < momentum < 1 (momentum 0 is vl_sgd_apply's job: this
 * rule at 0 does not round as that one does).  skip: as vl_sgd_apply (accum stays untouched too).  One launch, the grid of
 * vl_sgd_apply; it moves 5 floats per element (reads w, g, accum; writes w, accum), all of the interior as 16-byte accesses.
 * vl_momentum_apply_st: lr = state->lr; momentum and nesterov are constants of a run and stay launch arguments. */
int vl_momentum_apply(float* w, const float* g, float* accum, int64_t count, float lr, float momentum, int nesterov,
                      float clip_norm, const float* sumsq, float gscale, const uint32_t* skip,
                      const vl_lr_tier* tiers, int n_tiers, vl_stream_t stream);
int vl_momentum_apply_st(float* w, const float* g, float* accum, int64_t count, const vl_step_state* state, float momentum,
                         int nesterov, float clip_norm, const float* sumsq, float gscale, const uint32_t* skip,
                         const vl_lr_tier* tiers, int n_tiers, vl_stream_t stream);

/* ---- L2 weight decay: the regulariser's gradient and both sums in the launch that was the global norm ---------------------------------
 * loss_total = loss + sum_k (decay_k / 2) |w_k|^2 (tf.nn.l2_loss, Caffe weight_decay, torch.optim.SGD(weight_decay=)): the gradient
 * every later stage sees -- the global-norm clip, SGD, momentum, Adam (so Adam gets coupled L2, not AdamW; LAMB's decoupled decay,
 * vl_lamb_moments below, does not use this call) -- is g + decay w.  This call
 * REPLACES vl_sumsq / vl_sumsq_tiers in a step: it writes the regularised gradient over g IN PLACE and returns the two sums; the update
 * entry points above then run unchanged on g, with out as their sumsq.
 * The range table obeys the rules of vl_lr_tier: sorted, disjoint, inside [0, count), 1 .. VL_MAX_DECAY_RANGES entries; decay finite and
 * >= 0; anything else is refused on the host with the entry's index in the message.  It is read on the host and travels BY VALUE in the
 * launch arguments (64 x 24 bytes), so a captured step needs no device table.  Per element, no contraction left to the compiler, one
 * element function for the scalar head / tail and the 16-byte interior:
 *     decay_k > 0:   g' = fma(decay_k, w, g), stored;   out[0] += g' * g';   out[1] += ((0.5f * decay_k) * w) * w
 *     decay_k == 0:  out[0] += g * g;   w is NOT loaded and g is NOT stored (biases cost one read, as in vl_sumsq_tiers)
 *     outside every range: neither loaded nor stored (w and g may hold anything there, NaN included)
 * out: float[2], out[0] = sum g'^2 over every range, out[1] = sum (decay_k / 2) w^2, both overwritten.  ws: float[2048].  Two stages in
 * a fixed order (per-block partials, then one 256-thread block): the same bits from run to run, no float atomics.  w and g that
 * disagree in 16-byte phase take the scalar loops.  g must be written afresh by every backward pass: a caller that accumulates into g
 * across steps would decay it twice (vl_grad_accumulate below: the engines regularise only the final sum of an accumulated update).  Over decayed elements the launch moves 3 floats each (reads w, g; writes g): vl_sgd_apply's traffic. */
#define VL_MAX_DECAY_RANGES 64
typedef struct vl_decay_range {
    int64_t begin, end;
    float decay;
} vl_decay_range;
int vl_l2_regularize(const float* w, float* g, int64_t count, const vl_decay_range* ranges, int n_ranges, float* out /* [2] */,
                     float* ws /* float[2048] */, vl_stream_t stream);

/* ---- gradient accumulation: k micro-batches per update, one ranged launch per micro-step ------------------------------------------------
 * mode 0 (store): acc = g, the first micro-step (no fill is ever needed);  mode 1 (add): acc = acc + g;  mode 2 (final): g = acc + g,
 * acc left as it is.  One fp32 add per element, the same element function for the scalar head / tail and the 16-byte interior: the
 * result is bit for bit the IEEE single sum, and an update's gradient is ((g1 + g2) + g3) + ... in call order, the same from run to run.
 * The range table obeys the rules of vl_lr_tier (sorted, disjoint, inside [0, count), 1 .. VL_MAX_LR_TIERS entries; lr_mult must be valid
 * and is ignored, as in vl_sumsq_tiers); ranges == NULL && n_ranges == 0 is the full range.  It travels BY VALUE in the launch arguments.
 * Elements outside every range are neither loaded nor stored, in acc and in g alike (they may hold NaN).  acc and g that disagree in
 * 16-byte phase take the scalar loops.  One launch, the grid of vl_sgd_apply; per element in range it moves 2 floats (store) or 3 (add,
 * final), i.e. vl_sgd_apply's traffic.  Refused on the host: a null pointer, count <= 0, an unknown mode, a bad table.
 * This is the accumulating caller vl_l2_regularize warns about: the engines regularise only the FINAL sum (mode 2 first, then
 * vl_l2_regularize on g, once per update), so the decay enters once however many micro-steps there were. */
int vl_grad_accumulate(float* acc, float* g, int64_t count, int mode, const vl_lr_tier* ranges, int n_ranges, vl_stream_t stream);

/* ---- exponential moving average of the weights: tf.train.ExponentialMovingAverage's shadow variables, one ranged launch ------------------
 * shadow -= (1 - decay) * (shadow - w), restated with rate = 1 - decay so that nothing cancels near decay = 1.  Per element inside a range,
 * two fp32 roundings in this order (no contraction is left to the compiler, and the scalar head / tail and the 16-byte interior share the
 * element function, so an element's bits do not depend on which loop reached it):
 *     d  = w - s
 *     s' = fma(rate, d, s)
 * The range table obeys the rules of vl_lr_tier (sorted, disjoint, inside [0, count), 1 .. VL_MAX_LR_TIERS entries; lr_mult must be valid
 * and is ignored, as in vl_grad_accumulate); ranges == NULL && n_ranges == 0 is the full range.  It travels BY VALUE in the launch
 * arguments.  Elements outside every range are neither loaded nor stored, in shadow and in w alike (they may hold NaN).  shadow and w that
 * disagree in 16-byte phase take the scalar loops.  skip: as vl_sgd_apply -- when *skip != 0 at execution time the launch changes nothing.
 * One launch, the grid of vl_sgd_apply; per element in range it moves 3 floats (reads w, shadow; writes shadow): vl_sgd_apply's traffic.
 * Refused on the host: a null shadow or w, count <= 0, a rate outside (0, 1] or not finite, a bad table.
 * vl_ema_update_st: rate = state->ema_rate, written by vl_step_state_set_ema.  The rate is NOT derived from state->step on the device:
 * under accumulation that field holds the draw step, not the update count, and the warm-up rate max(1 - decay, 9 / (10 + n)) is computed
 * on the host by one function for the eager and the replayed form, which therefore agree bit for bit (as adam_lr does). */
int vl_ema_update(float* shadow, const float* w, int64_t count, float rate, const uint32_t* skip, const vl_lr_tier* ranges,
                  int n_ranges, vl_stream_t stream);
int vl_ema_update_st(float* shadow, const float* w, int64_t count, const vl_step_state* state, const uint32_t* skip,
                     const vl_lr_tier* ranges, int n_ranges, vl_stream_t stream);

/* ---- per-variable gradient and weight statistics: one segmented, fixed-order reduction over the flat buffers -------------------------------
 * One launch returns a row of statistics per segment (= per variable), whether the segment is fc6W or a 96-float bias.  READ-ONLY on w
 * and g.  The segment table obeys the rules of vl_lr_tier: sorted, disjoint, inside [0, count), 1 .. VL_MAX_STAT_SEGMENTS entries, each of
 * 1 .. 2^32 - 1 elements; anything else is refused on the host with the entry's index in the message.  It is read on the host and travels BY
 * VALUE in the launch arguments together with each segment's first chunk index, so a captured step needs no device table.  Elements outside
 * every segment are neither loaded nor stored (they may hold NaN; frozen ranges of g do).
 * Per element x of w and of g:  finite -> sum += (double)x, sumsq += (double)x * (double)x (the square is exact), min / max;  NaN or +-Inf ->
 * counted in *_nonfinite and left out of the sums and of min / max.  A denormal is finite and is not zero; g_zero counts +0 and -0.  Every
 * sum of a segment of N elements is within N 2^-53 sum|term| of the exact sum; min, max and the counts are exact (of +0 and -0 the
 * minimum is -0 and the maximum +0).
 * Order: a segment is cut into chunks of VL_STAT_CHUNK elements (chunks never span segments, a segment's last chunk is short).  Stage 1:
 * one workgroup per chunk finds its segment by a uniform scan of the table and writes one partial row to ws.  The element at index j of its
 * chunk is added, in order of j, to accumulator j mod 1024 of that chunk, and the 1024 accumulators are reduced in a fixed tree: where a
 * 16-byte load happens to begin plays no part.  Stage 2: one workgroup per segment reduces the segment's rows in a fixed order into out[s].
 * So the result is the same bits from run to run and depends on the table and on VL_STAT_CHUNK alone -- not on a grid size, not on the
 * pointers' alignment; no float atomics.  Interior elements are read as 16-byte loads where w and g agree in 16-byte phase, else by the
 * same element function through 4-byte loads.  The launch reads w and g once inside the segments: 8 bytes per element.
 * out: device, [n_segs], every byte overwritten.  ws: device, vl_tensor_stats_ws_bytes(segs, n_segs) bytes (one row per chunk; 0 when the
 * table would be refused), overwritten; 8-byte aligned like out.  Nothing needs zeroing first. */
#define VL_MAX_STAT_SEGMENTS 64
#define VL_STAT_CHUNK 16384
typedef struct vl_stat_segment {
    int64_t begin, end;
} vl_stat_segment;
typedef struct vl_tensor_stat {
    double g_sum, g_sumsq, w_sum, w_sumsq;
    float g_min, g_max, w_min, w_max;
    uint32_t g_nonfinite, w_nonfinite, g_zero;
    uint32_t reserved;
} vl_tensor_stat;
size_t vl_tensor_stats_ws_bytes(const vl_stat_segment* segs, int n_segs);
int vl_tensor_stats(const float* w, const float* g, int64_t count, const vl_stat_segment* segs, int n_segs, vl_tensor_stat* out,
                    void* ws, size_t ws_bytes, vl_stream_t stream);

/* ---- LARS: layer-wise adaptive learning rates for the momentum update (tf.contrib.opt.LARSOptimizer; You, Gitman, Ginsburg 2017) ---------
 * Two calls behind a vl_tensor_stats launch over the RAW gradient (after accumulation and exchange, before vl_l2_regularize): the rows
 * stay on the device, so does the trust table, and a captured step replays all of it.
 *
 * vl_lars_trust: trust[k] for the n_segs rows of a vl_tensor_stats launch, one workgroup, lane k = row k.  In double, rounded to float once:
 *     sc      = the clip scale of vl_sgd_apply, from clip_norm, *sumsq and gscale as the update launches take them
 *     wn      = sqrt(rows[k].w_sumsq)              gn = sc * sqrt(rows[k].g_sumsq)
 *     trust   = eeta * wn / (gn + decay[k] * wn + eps)     if wn > 0 and gn > 0 and the row counts no non-finite element of w or g
 *             = 1                                          otherwise (TF's where(w_norm > 0, where(g_norm > 0, .., 1), 1); a NaN travels
 *                                                          through the update exactly as it does without LARS)
 * decay: HOST array of n_segs coefficients (the one vl_l2_regularize gives the variable, 0 without weight decay); it travels by value in
 * the launch arguments like eeta and eps.  Read-only on rows; every one of the n_segs entries of trust is overwritten.  Refused on the
 * host: a null pointer, n_segs outside 1 .. VL_MAX_STAT_SEGMENTS, eeta not finite or <= 0, eps or a decay negative or not finite.
 *
 * vl_lars_apply: vl_momentum_apply over a range table whose entries carry a trust index.  Inside an entry the element rule is
 * vl_momentum_apply's (the same element function) with
 *     lr_k = (float)((float)(lr * lr_mult) * t),   t = 1 for trust_index == -1 (not read), else trust[trust_index] read when the kernel runs
 * so an entry's elements get, bit for bit, what vl_momentum_apply gives on that sub-range with that lr.  The accumulator never sees lr_k.
 * The table obeys the rules of vl_lr_tier (sorted, disjoint, inside [0, count), lr_mult finite and > 0) with 1 .. VL_MAX_STAT_SEGMENTS
 * entries, travels BY VALUE, and every trust_index is -1 or in [0, n_trust); anything else is refused on the host.  trust may be NULL when
 * n_trust == 0.  Elements outside every range are neither loaded nor stored (w, g and accum alike).  skip, gscale, clip_norm, sumsq,
 * nesterov, the scalar head / tail and the 16-byte interior: as vl_momentum_apply.  One launch, the grid of vl_sgd_apply, 5 floats per
 * element; the trust value is one uniform load per range.  vl_lars_apply_st: lr = state->lr. */
typedef struct vl_lars_range {
    int64_t begin, end;
    float lr_mult;
    int32_t trust_index;
} vl_lars_range;
int vl_lars_trust(const vl_tensor_stat* rows, int n_segs, double eeta, double eps, const float* decay, float clip_norm,
                  const float* sumsq, float gscale, float* trust, vl_stream_t stream);
int vl_lars_apply(float* w, const float* g, float* accum, int64_t count, float lr, float momentum, int nesterov, float clip_norm,
                  const float* sumsq, float gscale, const uint32_t* skip, const vl_lars_range* ranges, int n_ranges,
                  const float* trust, int n_trust, vl_stream_t stream);
int vl_lars_apply_st(float* w, const float* g, float* accum, int64_t count, const vl_step_state* state, float momentum,
                     int nesterov, float clip_norm, const float* sumsq, float gscale, const uint32_t* skip,
                     const vl_lars_range* ranges, int n_ranges, const float* trust, int n_trust, vl_stream_t stream);

/* ---- LAMB: layer-wise trust ratios and decoupled decay for the Adam update (You et al. 2019, "Large Batch Optimization for Deep
 * Learning"; tfa.optimizers.LAMB) ------------------------------------------------------------------------------------------------------
 * Two calls in the place of vl_adam_apply.  Element rule, fp32, contraction off, one element function for the scalar head / tail and
 * the 16-byte interior; sc = the clip scale of vl_sgd_apply (clip_norm, *sumsq, gscale), decay = the range's coefficient:
 *     gi = g * sc
 *     m' = fma(0.9f, m, 0.1f * gi)                 v' = fma(0.999f, v, gi * (0.001f * gi))       (vl_adam_apply's two lines: the same bits)
 *     mh = m' * c1        vh = v' * c2             r = mh / (sqrtf(vh) + eps)
 *     u  = decay > 0 ? fma(decay, w, r) : r        (decoupled decay, AdamW-style: it never enters g, m or v)
 * c1 = fl32(1 / (1 - 0.9^t)), c2 = fl32(1 / (1 - 0.999^t)) for update t >= 1 come from the caller (ONE host function computes them for
 * the eager and the replayed form; they are not derived from state->step, which holds the draw step under accumulation).
 * Per range with trust_index k >= 0 (a weight tensor), in double and rounded to float once:
 *     wn = sqrt(sum w^2)   un = sqrt(sum u^2)
 *     trust[k] = wn / un   if wn > 0 and un > 0 and no element of w or u in the range is non-finite,   else 1       (no clamp)
 * (TF's where(w_norm > 0, where(g_norm > 0, .., 1), 1); a NaN then travels through the update as it does under Adam.)
 *
 * vl_lamb_moments: inside every range m <- m', v <- v'; w and g are never written, w is read only inside ranges with trust_index >= 0
 * (a range with index -1 needs neither norms nor u).  For each range with an index it overwrites rows[index] and trust[index].  The
 * reduction order is vl_tensor_stats's: chunks of VL_STAT_CHUNK that never span ranges, element j of a chunk into accumulator j mod 1024,
 * the fixed tree, one workgroup per range for stage 2 (which also forms the trust value), squares formed in double, a non-finite element
 * adds +0 and counts.  So the bits depend on the table alone and rows[k].w_sumsq equals, bit for bit, the w_sumsq vl_tensor_stats
 * returns for the same segment.  No atomics.  *skip != 0 when the launch runs: m, v, rows and trust stay untouched.  Elements outside
 * every range are neither loaded nor stored.  Traffic: 6 floats per element (w, g, m, v read, m, v written).
 * ws: vl_lamb_moments_ws_bytes(ranges, n_ranges) bytes, 8-byte aligned (one vl_lamb_row per chunk; 0 = the table was refused).
 *
 * vl_lamb_apply: w' = fma(-a, u, w), a = (float)((float)(lr * lr_mult) * t), t = 1 for trust_index -1 (nothing read) else
 * trust[trust_index], one uniform load per range; u is recomputed from the stored m', v' and the unchanged w by the element function
 * above.  m and v are read-only.  The grid of vl_sgd_apply; 4 floats per element.  *skip != 0: nothing is touched.
 *
 * The table obeys the rules of vl_lr_tier (sorted, disjoint, inside [0, count), lr_mult finite and > 0) with 1 .. VL_MAX_STAT_SEGMENTS
 * entries, travels BY VALUE; decay finite and >= 0; trust_index -1 or in [0, n_trust); `reserved` is ignored.  rows and trust may be NULL
 * when n_trust == 0.  Refused on the host, each with a message that names the argument: null pointers, count <= 0, a bad table, an index
 * outside the trust array, eps not finite or <= 0 (it keeps 0 / 0 out where v' = 0), c1 or c2 not finite or < 1, a workspace too small.
 * The _st forms read c1, c2 (vl_lamb_moments_st) and lr, c1, c2 (vl_lamb_apply_st) from the step state when they run.
 * vl_step_state_set_lamb: one single-lane launch that writes the two words and nothing else; no other setter touches them. */
typedef struct vl_lamb_range {
    int64_t begin, end;
    float lr_mult;
    float decay;
    int32_t trust_index;
    int32_t reserved;
} vl_lamb_range;
typedef struct vl_lamb_row {
    double w_sumsq, u_sumsq;
    uint32_t nonfinite, reserved;
} vl_lamb_row;
size_t vl_lamb_moments_ws_bytes(const vl_lamb_range* ranges, int n_ranges);
int vl_lamb_moments(const float* w, const float* g, float* m, float* v, int64_t count, float c1, float c2, float eps, float clip_norm,
                    const float* sumsq, float gscale, const uint32_t* skip, const vl_lamb_range* ranges, int n_ranges, vl_lamb_row* rows,
                    float* trust, int n_trust, void* ws, size_t ws_bytes, vl_stream_t stream);
int vl_lamb_moments_st(const float* w, const float* g, float* m, float* v, int64_t count, const vl_step_state* state, float eps,
                       float clip_norm, const float* sumsq, float gscale, const uint32_t* skip, const vl_lamb_range* ranges, int n_ranges,
                       vl_lamb_row* rows, float* trust, int n_trust, void* ws, size_t ws_bytes, vl_stream_t stream);
int vl_lamb_apply(float* w, const float* m, const float* v, int64_t count, float lr, float c1, float c2, float eps, const uint32_t* skip,
                  const vl_lamb_range* ranges, int n_ranges, const float* trust, int n_trust, vl_stream_t stream);
int vl_lamb_apply_st(float* w, const float* m, const float* v, int64_t count, const vl_step_state* state, float eps, const uint32_t* skip,
                     const vl_lamb_range* ranges, int n_ranges, const float* trust, int n_trust, vl_stream_t stream);
int vl_step_state_set_lamb(vl_step_state* state, float c1, float c2, vl_stream_t stream);

/* ---- utilities ------------------------------------------------------------------------------- */
int vl_fill(float* p, int64_t count, float value, vl_stream_t stream);
/* ReluGrad in place: d[i] = y[i] > 0 ? d[i] : 0 (y = the ReLU's forward output, alexnet.py:228,248). */
int vl_relu_grad(float* d, const float* y, int64_t count, vl_stream_t stream);
/* truncated-normal / uniform parameter initialisers are host side; nothing here. */

#ifdef __cplusplus
}
#endif
#endif /* VLTF_H */
