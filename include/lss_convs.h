/*
 * lss_convs.h -- C ABI of the conv-stack kernels beside the Lift-Splat hot path (same library,
 * liblss_hip.so). Not part of the reference's hot-path boundary (lss_hip.h): these replace MIOpen
 * for the depthwise convolutions of CamEncode's EfficientNet-B0 trunk (src/models.py:43, 63-84),
 * which MIOpen runs on naive kernels for bf16 NCHW.
 *
 * Depthwise (groups = C) 2-D convolution, no bias, dilation 1, NCHW contiguous activations of
 * element type dtype (fp32 or bf16), fp32 weights (C, 1, K, K), fp32 accumulation; K in {3, 5},
 * stride in {1, 2}. Padding is given as the top / left pads; the bottom / right pads are implied
 * by (Ho, Wo): taps that fall outside the input read zero (TF "same" static padding, asymmetric
 * for the stride-2 layers). Asynchronous on the stream; 0 on success, a positive hipError_t on a
 * launch failure, LSS_CONV_EINVAL for bad arguments.
 *
 * Alignment contract (whole header). Pointers are bare addresses: a function cannot see the tensor's
 * dtype, strides or storage offset, so each one states the alignment its vector accesses need and
 * checks it on the host, before any HIP call -- a pointer that misses it is LSS_CONV_EINVAL, never a
 * launch (there is no scalar fallback; a caller holding a dense view at an odd offset copies it first,
 * as lss_carla_amd._lib.aligned does). fp32 arrays (weights, statistics, partials) are read by element.
 * The lss_dwconv_* functions: x, y, dy, dx 16-B aligned (the LDS-staged and the plane kernels load and
 * store 16-B vectors).
 */
#ifndef LSS_CONVS_H
#define LSS_CONVS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { LSS_CONV_F32 = 0, LSS_CONV_BF16 = 1 };
enum { LSS_CONV_NCHW = 0, LSS_CONV_NHWC = 1 };
enum { LSS_ACT_NONE = 0, LSS_ACT_RELU = 1, LSS_ACT_SWISH = 2 };
enum { LSS_CONV_EINVAL = -1 };

/* Which kernel a depthwise pass launches (ABI 27; host only: no HIP call, no allocation -- the launchers
 * switch on the same rule). pass: the entry point; the other arguments as that entry point's (ngroups is
 * read for LSS_DW_BWD_WEIGHT only). The rule depends on the shape alone: every lss_dwconv_* entry point
 * already refuses pointers that are not 16-B aligned. Families:
 *   LSS_DW_LDS_SEG    LDS-staged, segment map: forward (and stride-1 backward-data) of every (K, stride) but (3, 1)
 *   LSS_DW_LDS_TILE   LDS-staged, tile map: forward / stride-1 backward-data of (3, 1); every weight gradient
 *     both where Wo % 4 == 0 and the output reaches the whole padded input, (Wo - 1) stride + K >= pad_left + Wi
 *     (rows alike); seg = 8 (Wo % 8 == 0) or 4 outputs per vector store; banded = 1 when a plane's staged rows
 *     pass the LDS budget and it is cut into bands of rows (then pb = 1), else pb = planes per block
 *   LSS_DW_PLANES22 / LSS_DW_PLANES11  whole narrow planes (Wo = 22 / 11) through LDS, pb planes per block:
 *     forward with stride 1, every weight gradient, within the LDS budget
 *   LSS_DW_REG        the register-tiled kernels: everything else (seg = banded = pb = 0)
 *   LSS_DW_S2_PAR0..3 stride-2 backward-data, index 2 (pad_top & 1) + (pad_left & 1)
 * Stride-1 backward-data is the forward on (Ho, Wo) -> (Hi, Wi) with paddings K - 1 - pad: the forward
 * families, chosen for that mirrored shape. Returns 0, or LSS_CONV_EINVAL as the entry point would. */
enum { LSS_DW_FWD = 0, LSS_DW_BWD_DATA = 1, LSS_DW_BWD_WEIGHT = 2 };
enum { LSS_DW_LDS_SEG = 0, LSS_DW_LDS_TILE = 1, LSS_DW_PLANES22 = 2, LSS_DW_PLANES11 = 3, LSS_DW_REG = 4,
       LSS_DW_S2_PAR0 = 5, LSS_DW_S2_PAR1 = 6, LSS_DW_S2_PAR2 = 7, LSS_DW_S2_PAR3 = 8, LSS_DW_FAMILIES = 9 };
typedef struct lss_dw_arm {
    int32_t family, seg, banded, pb;
} lss_dw_arm_t;
int lss_dwconv_arm(int32_t pass, int32_t dtype, int32_t N, int32_t C, int32_t Hi, int32_t Wi, int32_t K,
                   int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo, int32_t ngroups,
                   lss_dw_arm_t* arm);

/* y (N, C, Ho, Wo) = depthwise_conv(x (N, C, Hi, Wi), w) */
int lss_dwconv_fwd(const void* x, int32_t dtype, const float* w, int32_t N, int32_t C, int32_t Hi, int32_t Wi,
                   int32_t K, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo, void* y,
                   void* stream);

/* dx (N, C, Hi, Wi) = d loss / d x given dy (N, C, Ho, Wo); shapes and pads of the forward conv */
int lss_dwconv_bwd_data(const void* dy, int32_t dtype, const float* w, int32_t N, int32_t C, int32_t Hi, int32_t Wi,
                        int32_t K, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo, void* dx,
                        void* stream);

/* partial (C, ngroups, K*K) fp32: the weight gradient of images [N*q/ngroups, N*(q+1)/ngroups) in
 * slot q (1 <= ngroups <= N); the caller sums the groups (fixed order, deterministic). */
int lss_dwconv_bwd_weight(const void* x, const void* dy, int32_t dtype, int32_t N, int32_t C, int32_t Hi, int32_t Wi,
                          int32_t K, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho, int32_t Wo,
                          int32_t ngroups, float* partial, void* stream);
/* (ABI 23) lss_dwconv_bwd_weight that also folds the partials: the last of each channel's ngroups blocks
 * to finish sums them in group order into dw (C, K*K) fp32 -- no separate reduction launch. sync: the
 * batch-norm sync workspace (lss_bn_sync_words int32, zero-filled; left zero-filled), C <= 4096. */
int lss_dwconv_bwd_weight2(const void* x, const void* dy, int32_t dtype, int32_t N, int32_t C, int32_t Hi,
                           int32_t Wi, int32_t K, int32_t stride, int32_t pad_top, int32_t pad_left, int32_t Ho,
                           int32_t Wo, int32_t ngroups, float* partial, uint32_t* sync, float* dw, void* stream);

/* 1x1 convolution to one output channel (BevEncode's last conv, up2.4: 128 -> outC = 1,
 * src/models.py:115) over channels-last bf16 rows x (P, C), C % 8 == 0 and 64 % (C / 8) == 0:
 * y[r] = bf16(sum_c x[r, c] * w[c] + bias[0]) (fp32 accumulation; w holds the bf16-rounded weights
 * as fp32, as autocast's conv operands; bias is a device scalar, nullable). Backward: dx[r, c] = bf16(dy[r] * w[c]) and partial
 * (lss_head1_blocks(P), C + 1) fp32 = per block of rows, sum_r dy[r] * x[r, c] (columns 0..C-1) and
 * sum_r dy[r] (column C); the caller sums the blocks (fixed order).
 * Alignment: x and dx 16-B aligned (rows are read as 16-B vectors); y and dy by element (2 B). */
int lss_head1_blocks(int32_t P);
int lss_head1_fwd(const void* x, const float* w, const float* bias, int32_t P, int32_t C, void* y, void* stream);
int lss_head1_bwd(const void* x, const void* dy, const float* w, int32_t P, int32_t C, void* dx, float* partial,
                  void* stream);
/* (ABI 23) BevEncode's up2 tail -- BN + ReLU + the one-channel head -- without the normalised map:
 * lss_head1_fwd2 / lss_head1_bwd2 with bn_stats = the batch norm's saved (4, C) statistics (mean, rstd,
 * scale, shift; from lss_bn_fwd2 with y = NULL) read x as the batch norm's INPUT and use
 * bf16(relu(fmaf(x, scale, shift))) -- the value lss_bn_fwd's ReLU apply would have stored -- in its
 * place (bn_stats = NULL: lss_head1_fwd / lss_head1_bwd). lss_head1_bwd2 with dx = NULL writes no input
 * gradient (bn_stats required): lss_bn_bwd_rank1 takes it as bf16(dy[r] w[c]) itself. Bit-identical to
 * the unfused sequence (tests/test_gpu_convs.py). */
int lss_head1_fwd2(const void* x, const float* w, const float* bias, int32_t P, int32_t C, const float* bn_stats,
                   void* y, void* stream);
int lss_head1_bwd2(const void* x, const void* dy, const float* w, int32_t P, int32_t C, const float* bn_stats,
                   void* dx, float* partial, void* stream);

/* (ABI 25) The same head with K = 2..8 output channels (a multi-class BevEncode, outC = K), x as above:
 * channels-last bf16 rows (P, C), P = N * HW, C % 8 == 0 and 64 % (C / 8) == 0. The logits y and their
 * gradient dy are NCHW contiguous (N, K, H, W) bf16 -- the layout the loss, the metric and the labels use --
 * so row r = n * HW + q holds its K values at (n * K + k) * HW + q; HW and P need not be multiples of
 * anything (a block of rows may straddle an image boundary).
 *   y[n, k, q] = bf16(sum_c in[r, c] * w[k, c] + bias[k])    w (K, C) fp32 holding bf16-rounded weights,
 *                                                            bias K device floats, nullable
 *   dx[r, c]   = bf16(sum_k dy[n, k, q] * w[k, c])           fp32, k ascending, rounded once; always written
 *   partial    (lss_head1_blocks(P), K, C + 1) fp32: per block of rows, sum_r dy[r, k] * in[r, c] and
 *              (column C) sum_r dy[r, k]; the caller sums the blocks (fixed order)
 * in = x, or with bn_stats (a batch norm's saved (4, C) statistics, as lss_head1_fwd2)
 * bf16(relu(fmaf(x, scale, shift))) of the batch norm's INPUT x: the normalised map is never written, and
 * dx is then the gradient of that map (lss_bn_bwd2's NHWC path with y = NULL takes it from there). Per
 * channel k the arithmetic and its order are lss_head1_*'s: with w[k] = w1, bias[k] = b1 channel k of y is
 * lss_head1_fwd2's output bit for bit, and a dy that is zero outside channel k gives lss_head1_bwd2's dx
 * and partials. Alignment: x and dx 16 B; y and dy by element (2 B). One launch each; LSS_CONV_EINVAL
 * (before any launch) for K outside 2..8, P % HW != 0 or a pointer that misses its alignment. */
int lss_headk_fwd(const void* x, const float* w, const float* bias, int32_t P, int32_t HW, int32_t C, int32_t K,
                  const float* bn_stats, void* y, void* stream);
int lss_headk_bwd(const void* x, const void* dy, const float* w, int32_t P, int32_t HW, int32_t C, int32_t K,
                  const float* bn_stats, void* dx, float* partial, void* stream);

/* Weight gradient of a 1x1 convolution (no bias, stride 1) over NCHW contiguous bf16 activations:
 * dw (Cout, Cin) = sum over n < N, q < HW of dy[n][co][q] * x[n][ci][q], fp32 accumulation, written as
 * dw_dtype (LSS_CONV_BF16: rounded once; LSS_CONV_F32). HW % 4 == 0, 8-B aligned x / dy. workspace:
 * at least lss_pw_wrw_workspace_bytes(N, Cin, Cout, HW) bytes of device memory (per-split fp32
 * partials, summed in split order: deterministic). Two launches on the stream. */
int64_t lss_pw_wrw_workspace_bytes(int32_t N, int32_t Cin, int32_t Cout, int32_t HW);
int lss_pw_wrw(const void* x, const void* dy, int32_t N, int32_t Cin, int32_t Cout, int32_t HW, void* dw,
               int32_t dw_dtype, void* workspace, int64_t workspace_bytes, void* stream);

/* 1x1 convolution (no bias, stride 1) over NCHW contiguous bf16 activations, fp32 accumulation:
 * y[n][m][q] = bf16(sum_k A(m, k) * x[n][k][q]) for n < N, m < M, q < HW, with A(m, k) = a[m * K + k]
 * (LSS_PW_MK: the conv weight (M, K), the forward) or a[k * M + m] (LSS_PW_KM: the weight (K, M) read
 * transposed, the backward-data dx = W^T dy). HW % 4 == 0, K % 8 == 0, M % 8 == 0, 16-B aligned pointers. */
enum { LSS_PW_MK = 0, LSS_PW_KM = 1 };
int lss_pw_conv(const void* x, const void* a, int32_t a_layout, int32_t N, int32_t K, int32_t M, int32_t HW, void* y,
                void* stream);

/* Per-sample scale (+ residual) over N samples of `per` contiguous bf16 elements each (any memory
 * format that is sample-major: NCHW or channels-last), per % 8 == 0, 16-B aligned pointers:
 * y = bf16(x * scale[n] + res) (res nullable: y = bf16(x * scale[n])), scale[n] = mask[n] / keep with
 * mask[n] = floor(bf16(keep + u[n])), u the N bf16 uniform draws (torch.rand in the activations'
 * dtype), 0 < keep <= 1. The MBConv residual with stochastic depth (efficientnet_pytorch
 * drop_connect: inputs / keep_prob * floor(keep_prob + rand), then the skip add; the reference's
 * trunk, src/models.py:43) in one pass, the mask computed in the kernel; its backward is the
 * res == NULL form on the output gradient with the same draws. */
int lss_scale_add(const void* x, const void* u, float keep, const void* res, int64_t N, int64_t per, void* y,
                  void* stream);

/* (ABI 23) The weight of a stride-1, padding-(K-1)/2 transposed convolution as a forward one:
 * wt[i][o][a][b] = w[o][i][K-1-a][K-1-b], written channels-last ((I, O, K, K) with memory order
 * i, a, b, o). w is (O, I, K, K), NCHW (contiguous) or NHWC (channels-last) per w_layout; dtype fp32 or
 * bf16. dx = conv2d(dy, wt) is the backward-data of y = conv2d(x, w) (models._Conv3x3: MIOpen's forward
 * kernels instead of its backward-data ones). Replaces w.transpose(0, 1).flip(2, 3).contiguous(...),
 * two torch kernels. */
int lss_conv_flip_weight(const void* w, int32_t dtype, int32_t O, int32_t I, int32_t K, int32_t w_layout,
                         void* wt, void* stream);

/* Dropout (CamEncode.dropout = nn.Dropout(0.2), src/models.py:44, 53), training mode: y = x / keep where
 * a counter-based draw keeps the element (probability keep), else 0; n elements of dtype (fp32 or bf16)
 * in memory order (any memory format), n * sizeof(dtype) % 16 == 0, 16-B aligned. The mask is a pure
 * function of (*seed, element index) -- Philox4x32-10, key = the 64-bit seed (device memory, so a
 * captured graph draws a new one per replay), counter = (16-B vector index, block) -- so the backward is
 * the same call on dy with the same seed. Blocks write the tensor in 8 XCD-contiguous eighths (the
 * fused lift's layout) and, when `prefetch` is non-NULL, also read its `prefetch_bytes` (the lift's
 * packed depthnet weights) into every XCD's L2. */
int lss_dropout(const void* x, int32_t dtype, int64_t n, const uint64_t* seed, float keep, void* y,
                const void* prefetch, int64_t prefetch_bytes, void* stream);

/* SimpleLoss (src/tools.py:222-230: BCEWithLogitsLoss(pos_weight=[pos_weight]), reduction mean) and its
 * input gradient in one pass: loss[0] = mean over the n elements of
 *   (1 - t) x + (1 + (pw - 1) t) (log1p(exp(-|x|)) + max(-x, 0)),
 * grad = ((1 + (pw - 1) t) sigmoid(x) - pw t) / n (the gradient for d loss = 1; the caller scales it by
 * the incoming gradient). x, grad: n logits of dtype (fp32 or bf16), 16-B aligned; target: n fp32,
 * 16-B aligned; arithmetic fp32. partial: lss_bce_partials(n) fp32 scratch. Deterministic (fixed-order
 * sums). Two launches, no host synchronisation. */
int lss_bce_logits(const void* x, int32_t dtype, const float* target, int64_t n, float pos_weight, float* partial,
                   float* loss, void* grad, void* stream);
int64_t lss_bce_partials(int64_t n);
/* Backward of lss_bce_logits: dx = grad * grad_loss[0] (grad_loss: the loss's incoming gradient, one fp32
 * in device memory), computed in fp32 and rounded once to dtype; grad and dx 16-B aligned. */
int lss_bce_logits_bwd(const void* grad, int32_t dtype, int64_t n, const float* grad_loss, void* dx, void* stream);

/* Validation metrics of one batch (get_val_info, src/tools.py:243-270), over the first n_valid[0] samples
 * only (n_valid: one int32 in device memory, clamped to [0, batch]; NULL = batch), accumulated:
 *   totals[0] += sum of l(x, t) / per_sample   (l: lss_bce_logits's per-element fp32 term; this is the
 *                                               batch's mean loss times its valid sample count)
 *   totals[1] += #(x > 0 and t != 0),  totals[2] += #(x > 0 or t != 0)
 * x: batch * per_sample logits of dtype (fp32 or bf16), target: as many fp32; per_sample need not be a
 * multiple of anything (the mask is per element); 16-byte loads are used when both are 16-B aligned.
 * totals: 3 doubles in device memory; partial: lss_bce_iou_partial_bytes(batch * per_sample) bytes of
 * 8-B aligned scratch. Per-element arithmetic fp32, sums fp64 and counts integer in a fixed order: two
 * launches (block records, a one-block fold), no atomics, no host read; graph-capturable, and one captured
 * launch serves any n_valid. */
int lss_bce_iou_accum(const void* x, int32_t dtype, const float* target, int64_t per_sample, int32_t batch,
                      const int32_t* n_valid, float pos_weight, double* totals, void* partial, void* stream);
int64_t lss_bce_iou_partial_bytes(int64_t n);

/* (ABI 25) Per-class forms for logits (N, K, H, W) contiguous, plane = H * W: element i takes
 * pw = pos_weight[(i / plane) % K], K floats in DEVICE memory (a captured graph replays with the current
 * weights; BCEWithLogitsLoss(pos_weight = w.view(K, 1, 1)), mean over all n). plane need not be a multiple
 * of 8: the weight is looked up per element. Otherwise lss_bce_logits -- same partition, per-element
 * expression, fold, alignment, scratch (lss_bce_partials(n)) and two launches; with K equal weights, its
 * loss and grad bit for bit. The backward is lss_bce_logits_bwd. */
int lss_bce_logits_pc(const void* x, int32_t dtype, const float* target, int64_t n, int64_t plane, int32_t K,
                      const float* pos_weight, float* partial, float* loss, void* grad, void* stream);
/* lss_bce_iou_accum with the counts kept per class (per_sample = K * plane, K <= 32):
 *   totals[0] += sum of l(x, t) / per_sample,  totals[1 + k] += intersection of class k,
 *   totals[1 + K + k] += union of class k      (1 + 2 K doubles)
 * partial: lss_bce_iou_pc_partial_bytes(batch * per_sample, K) bytes, 8-B aligned. Same n_valid masking,
 * same fixed-order sums (integer counts, fp64 loss), two launches, capturable; K = 1 gives
 * lss_bce_iou_accum's three totals bit for bit. */
int lss_bce_iou_accum_pc(const void* x, int32_t dtype, const float* target, int64_t per_sample, int32_t batch,
                         const int32_t* n_valid, int64_t plane, int32_t K, const float* pos_weight, double* totals,
                         void* partial, void* stream);
int64_t lss_bce_iou_pc_partial_bytes(int64_t n, int32_t K);

/* (ABI 29) Focal loss for imbalanced classes, loss and input gradient in one pass. params: K x 3 fp32 in DEVICE
 * memory, row k = (w_pos, w_neg, gamma) of class k = (i / plane) % K (a captured graph replays with the current
 * values). Labels are hard, q = (t != 0). With softplus(z) = log1p(exp(-|z|)) + max(z, 0) and p = sigmoid(x):
 *   q = 1:  l = exp(-gamma softplus(x)) w_pos softplus(-x),
 *           dl/dx = -exp(-gamma softplus(x)) w_pos (gamma p softplus(-x) + sigmoid(-x))
 *   q = 0:  l = exp(-gamma softplus(-x)) w_neg softplus(x),
 *           dl/dx = exp(-gamma softplus(-x)) w_neg (gamma sigmoid(-x) softplus(x) + p)
 * i.e. (1 - p_t)^gamma times the weighted BCE, the power written as exp(gamma log(1 - p_t)): no division and no
 * difference of near-equal terms, so 0 < gamma < 1 is finite at saturated logits. (pw, 1, 0) is lss_bce_logits_pc's
 * loss for hard labels; focal(alpha, gamma) is (alpha, 1 - alpha, gamma). loss[0] = mean over the n elements,
 * grad = dl/dx / n in the logits' type (rounded once). Otherwise lss_bce_logits_pc's contract: fp32 arithmetic,
 * x / grad / target 16-B aligned, partial = lss_bce_partials(n) fp32, fixed-order folds (two runs give equal
 * bits), two launches. K = 1: plane = the elements of a sample. The backward is lss_bce_logits_bwd. */
int lss_focal_logits_pc(const void* x, int32_t dtype, const float* target, int64_t n, int64_t plane, int32_t K,
                        const float* params, float* partial, float* loss, void* grad, void* stream);
/* (ABI 29) Validation in one pass for either loss and a ladder of thresholds: thetas = T ascending fp32 logit
 * thresholds in device memory (1 <= T <= 16), params as above (K <= 32, per_sample = K * plane). Over the first
 * n_valid[0] samples (as lss_bce_iou_accum), for class k and threshold j, compared in fp32 with a strict >:
 *   P_k = #(t != 0),  TP_kj = #(x > theta_j and t != 0),  PP_kj = #(x > theta_j)
 * totals (1 + K + 2 K T doubles in device memory, +=):
 *   [0] the sum of lss_focal_logits_pc's per-element l (fp64) / per_sample,  [1 + k] P_k,
 *   [1 + K + k T + j] TP_kj,  [1 + K + K T + k T + j] PP_kj
 * so the intersection at j is TP and the union PP + P - TP. Counts are exact integers. partial:
 * lss_seg_metrics_partial_bytes(batch * per_sample, K, T) bytes (0 for sizes out of range), 8-B aligned. Each element
 * adds one to its block's histogram over (class, #thresholds below x, label); the fold kernel takes suffix sums.
 * Two launches, no host read, capturable; one captured launch serves any n_valid. */
int lss_seg_metrics_accum(const void* x, int32_t dtype, const float* target, int64_t per_sample, int32_t batch,
                          const int32_t* n_valid, int64_t plane, int32_t K, const float* params, const float* thetas,
                          int32_t T, double* totals, void* partial, void* stream);
int64_t lss_seg_metrics_partial_bytes(int64_t n, int32_t K, int32_t T);

/* (ABI 32) The masked forms: losses and metrics over the cells a uint8 mask marks valid (e.g. lss_simbev_valid_mask's,
 * include/lss_simbev.h). valid: (batch, plane) bytes in device memory, any value != 0 = valid, one plane shared by the K
 * classes of a sample: element i of the (batch, K, plane) logits reads valid[(i / (K plane)) plane + i % plane]
 * (n = batch K plane). The existing entries and their kernels are untouched.
 *
 * lss_seg_loss_masked: lss_focal_logits_pc's per-element term (rows (w_pos, w_neg, gamma); (pw, 1, 0) is SimpleLoss)
 * over the valid elements only. An element whose mask byte is 0 is selected out, not multiplied out: it adds nothing
 * and its gradient is exactly 0, whatever its logit (NaN, +-Inf). With M the number of valid elements (K per valid
 * cell), counted as integers in the same pass:
 *   loss[0] = sum of l / max(M, 1),   scale[0] = n / max(M, 1),   grad = dl/dx / n in the logits' type
 * -- M is not known while the gradient is written, so grad is what lss_focal_logits_pc stores and the backward applies
 * the rest; scale is exactly 1 when every element is valid, and an all-ones mask then gives lss_focal_logits_pc's loss
 * gradient bit for bit (a bf16 gradient takes the same two roundings). M = 0 gives loss 0 and a zero gradient. partial:
 * 2 * lss_bce_partials(n) 4-byte words (the block sums, then the block counts). Partition, loads, fixed-order folds and
 * alignment rules are lss_focal_logits_pc's; two launches, capturable; the mask is read on the device, so a replay
 * follows an in-place change of it. -1 also for n not a multiple of K * plane.
 * lss_seg_loss_masked_bwd: dx = grad * (grad_loss[0] * scale[0]), both scalars read on the device, rounded once. */
int lss_seg_loss_masked(const void* x, int32_t dtype, const float* target, const uint8_t* valid, int64_t n,
                        int64_t plane, int32_t K, const float* params, float* partial, float* loss, float* scale,
                        void* grad, void* stream);
int lss_seg_loss_masked_bwd(const void* grad, int32_t dtype, int64_t n, const float* grad_loss, const float* scale,
                            void* dx, void* stream);
/* lss_seg_metrics_accum with the mask: only valid elements of the first n_valid[0] samples enter the counts and the
 * fp64 loss sum. With M the number of those elements and nv the clamped n_valid:
 *   totals[0] += nv * (sum of l) / max(M, 1)     (the masked batch mean times the batch size, as get_val_info
 *                                                 weights it);  totals[1..]: as lss_seg_metrics_accum, same layout
 *   valid_cells[0] += M / K                      (one double in device memory, 8-B aligned; may be NULL)
 * partial: lss_seg_metrics_masked_partial_bytes(batch * per_sample, K, T) bytes (0 for sizes out of range), 8-B
 * aligned. Two launches, no host read, capturable. */
int lss_seg_metrics_accum_masked(const void* x, int32_t dtype, const float* target, const uint8_t* valid,
                                 int64_t per_sample, int32_t batch, const int32_t* n_valid, int64_t plane, int32_t K,
                                 const float* params, const float* thetas, int32_t T, double* totals,
                                 double* valid_cells, void* partial, void* stream);
int64_t lss_seg_metrics_masked_partial_bytes(int64_t n, int32_t K, int32_t T);

/* (ABI 34) Exclusive classes: every cell has exactly one of C classes (2 <= C <= 8; class 0 is the background). x and
 * grad are (batch, C, plane) contiguous logits, fp32 or bf16 (the K-channel head's NCHW output with K = C); labels is a
 * (batch, plane) uint8 class map in device memory, a value >= C (255 by convention) meaning "ignore"; valid is NULL or a
 * (batch, plane) uint8 mask as above. A cell counts iff its label is < C and (valid == NULL or its mask byte != 0). A cell
 * that does not count is selected out, not multiplied out: it adds nothing to any sum or count and its C gradient
 * elements are exactly 0, whatever its logits (NaN, +-Inf) -- lss_seg_loss_masked's rule. The existing entries and
 * their kernels are untouched.
 *
 * lss_softmax_ce: F.cross_entropy(x, labels, weight = w, ignore_index, reduction = "mean") and its input gradient in one
 * pass. weight: C fp32 class weights in DEVICE memory. Per counted cell, fp32 arithmetic, channel sums in ascending c:
 *   m = max_c x_c,  e_c = exp(x_c - m),  S = sum_c e_c,  p_c = e_c / S,  l = w_y ((m - x_y) + log S)
 *   dl/dx_c = w_y (p_c - [c = y]), the c = y element written as -w_y (sum_{c != y} e_c) / S (no cancellation at p_y ~ 1)
 *   loss[0] = sum l / max(W, tiny),  W = sum of w_y over the counted cells
 * W is not known while the gradient is written, so grad = dl/dx_c / n_cells (n_cells = batch * plane) in the logits'
 * type, rounded once, scale[0] = n_cells / W, and the backward is lss_seg_loss_masked_bwd over the batch * C * plane
 * gradient elements (dx = grad * (grad_loss[0] * scale[0])). W = 0 gives loss 0, scale 0 and so a zero gradient.
 * partial: lss_softmax_ce_partials(n_cells) fp32 (the block sums of l, then of w_y), folded in a fixed order by a
 * one-wave kernel: two runs give equal bits. Two launches, no atomics, no host read, capturable; weight, valid and labels
 * are read on the device, so a replay follows an in-place change of any of them. valid == NULL gives the bits of an
 * all-ones mask. Two arms, the same arithmetic (lss_softmax_ce_arm says which one a call takes):
 *   LSS_CE_ARM_VECTOR  plane % 8 == 0, x and grad 16-B aligned, labels and valid 8-B aligned: a thread takes 8
 *                      consecutive cells -- one 8-B label load, one 8-B mask load and C vector loads of the logits, all
 *                      from unconditional addresses and issued before the first use; one instantiation per C.
 *   LSS_CE_ARM_SCALAR  anything else: one cell per thread, a channel past C read from a clamped address.
 * LSS_CONV_EINVAL without launching: a NULL pointer (valid excepted), another dtype, batch or plane < 1, C outside 2..8,
 * batch * C * plane not addressable, x or grad not aligned to its element, weight / partial / loss / scale to 4 B. */
enum { LSS_CE_ARM_SCALAR = 0, LSS_CE_ARM_VECTOR = 1 };
int lss_softmax_ce(const void* x, int32_t dtype, const uint8_t* labels, const uint8_t* valid, int32_t batch,
                   int64_t plane, int32_t C, const float* weight, float* partial, float* loss, float* scale, void* grad,
                   void* stream);
int lss_softmax_ce_arm(const void* x, int32_t dtype, const uint8_t* labels, const uint8_t* valid, int32_t batch,
                       int64_t plane, int32_t C, const void* grad);
int64_t lss_softmax_ce_partials(int64_t n_cells);
/* The prediction: out (batch, plane) uint8 = argmax_c x_c, compared in fp32 with a strict > scanning c upwards from
 * channel 0 against a running best that starts at -inf: ties go to the lowest class, a NaN never wins, all-NaN gives 0
 * (torch.argmax differs on NaN). One launch; 8 cells and one 8-B store per thread when plane % 8 == 0, x is 16-B and
 * out 8-B aligned, else a cell per thread. LSS_CONV_EINVAL as above. */
int lss_argmax_classes(const void* x, int32_t dtype, int32_t batch, int64_t plane, int32_t C, uint8_t* out,
                       void* stream);
/* Validation: the C x C confusion matrix of exact integer counts conf[y][pred] (pred: lss_argmax_classes' rule, the
 * same device function) over the counted cells of the first n_valid[0] samples (one int32 in device memory, clamped to
 * 0..batch; NULL = batch), and the loss. totals: 1 + C * C doubles in device memory, +=:
 *   [0] nv * (sum l) / max(W, tiny) over those cells (the batch's mean loss times its sample count, as
 *       lss_seg_metrics_accum_masked weights it; l and w_y summed in fp64),   [1 + y * C + pred] the counts
 * Each block keeps an LDS histogram of C * C int32; a block record is two doubles plus the histogram, and a one-block
 * kernel folds the records in block order. partial: lss_confusion_partial_bytes(batch * plane, C) bytes (0 for sizes
 * out of range), 8-B aligned as totals. Two launches, no host read, capturable; one captured launch serves any n_valid. */
int lss_confusion_accum(const void* x, int32_t dtype, const uint8_t* labels, const uint8_t* valid, int32_t batch,
                        int64_t plane, int32_t C, const int32_t* n_valid, const float* weight, double* totals,
                        void* partial, void* stream);
int64_t lss_confusion_partial_bytes(int64_t n_cells, int32_t C);

/* out[c] = sum over (n, pixel) of x[n][c][pixel] (fp32, fixed order), x (N, C, HW) NCHW fp32 or bf16: the
 * bias gradient of the fused lift's depthnet conv (src/models.py:47) from d(logits). One launch. */
int lss_channel_sums(const void* x, int32_t dtype, int32_t N, int32_t C, int32_t HW, float* out, void* stream);

/* The training step's update (train_simbev.py:245-248): clip_grad_norm_(params, max_norm) fused with
 * torch.optim.Adam (L2 weight_decay added to the clipped gradient, no amsgrad) over `count` fp32 tensors
 * (params[k], grads[k], exp_avg[k], exp_avg_sq[k]: numel[k] elements each; step[k]: the tensor's
 * device-resident fp32 step count, advanced by one; all distinct). The clip factor is
 * min(max_norm / (||all grads||_2 + 1e-6), 1); the gradients are not modified. partial:
 * lss_clip_adam_partials() fp32 scratch. Two launches, no host synchronisation (graph-capturable);
 * deterministic. */
#define LSS_ADAM_MAX_TENSORS 32
int lss_clip_adam_partials(void);
int lss_clip_adam(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, float* const* step, const int64_t* numel, float max_norm, float lr,
                  float beta1, float beta2, float eps, float weight_decay, float* partial, void* stream);
/* lss_clip_adam that survives a non-finite gradient. When the gradient norm is finite it computes exactly
 * what lss_clip_adam computes, bit for bit. When it is not (a NaN or an infinity among the gradients, or a
 * sum of squares that overflows), nothing is written -- parameters, exp_avg, exp_avg_sq and every step
 * count keep their bits -- and skipped[0] (one int32 in device memory) is advanced by one. Every block
 * folds the same partials in the same order, so the decision is the same everywhere. Three launches (the
 * third, one block, advances the step counts or the skip counter), no host synchronisation
 * (graph-capturable); deterministic. */
int lss_clip_adam_guarded(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                          float* const* exp_avg_sq, float* const* step, const int64_t* numel, float max_norm,
                          float lr, float beta1, float beta2, float eps, float weight_decay, float* partial,
                          int32_t* skipped, void* stream);
/* (ABI 30) Either update with the learning rate computed on the device and, optionally, an exponential moving
 * average (EMA) of the weights, so that a captured update follows a schedule. skipped: NULL = lss_clip_adam's
 * form (two launches), else lss_clip_adam_guarded's (three). lr is the base rate; with t the value Adam's bias
 * correction uses for this update (each tensor's own count, after its advance) and s = t - 1, in fp32:
 *   warm  = warmup_steps > 0 ? warmup_factor + (1 - warmup_factor) * min(s, W) / W : 1
 *   x     = clamp((s - W) / (T - W), 0, 1)            W = warmup_steps, T = total_steps, m = min_factor
 *   decay = 1 (kind 0, constant) | m + (1 - m)(1 - x) (1, linear) | m + (1 - m) * 0.5 * (1 + cos(pi x)) (2, cosine)
 *   lr_t  = lr * warm * decay                          (past T: lr * m)
 * (the cosine is evaluated as sin^2(pi (1 - x) / 2), the same function without the cancellation at x -> 1).
 * A skipped step does not advance t, hence not the schedule; a constant schedule without warm-up, ema = NULL,
 * computes what the entries above compute, bit for bit. lr_out (device, nullable): tensor 0's lr_t of the
 * update just applied, written by one thread of the Adam pass; a skipped step leaves it alone.
 * ema (NULL, or `count` device pointers, ema[k] of numel[k] fp32, distinct from each other and from every
 * params / exp_avg / exp_avg_sq pointer): after the parameter's update, same thread, same pass,
 *   e = fmaf(1 - d, p_new - e, e),  d = ema_warmup ? min(ema_decay, (1 + t) / (10 + t)) : ema_decay;
 * a skipped step writes no EMA element; a tensor whose EMA is not 16-B aligned takes the scalar loop.
 * LSS_CONV_EINVAL before any launch: kind outside 0..2, warmup_steps < 0, warmup_factor or min_factor outside
 * [0, 1], kind != 0 with total_steps <= warmup_steps, ema_decay outside [0, 1), a NULL or repeated ema entry,
 * an ema pointer equal to a params / exp_avg / exp_avg_sq pointer, and what the entries above refuse. */
int lss_clip_adam_sched(int32_t count, float* const* params, const float* const* grads, float* const* exp_avg,
                        float* const* exp_avg_sq, float* const* step, const int64_t* numel, float max_norm,
                        float lr, float beta1, float beta2, float eps, float weight_decay, float* partial,
                        int32_t* skipped, int32_t kind, int32_t warmup_steps, float warmup_factor,
                        int32_t total_steps, float min_factor, float* lr_out, float* const* ema, float ema_decay,
                        int32_t ema_warmup, void* stream);

/* Training-mode batch norm fused with an activation (and, for ReLU, a residual add), for
 * nn.BatchNorm2d followed by swish (EfficientNet-B0, src/models.py:68 and the MBConv blocks) or
 * ReLU (CamEncode.up1, BevEncode, src/models.py:15-34, 92-130):
 *   y = act(x * scale_c + shift_c [+ residual]),  scale_c = gamma_c / sqrt(var_c + eps),
 *   shift_c = beta_c - mean_c * scale_c, mean / biased var over (N, H, W); running_mean / running_var
 *   (nullable) updated with `momentum` and the unbiased variance, as nn.BatchNorm2d does.
 * x, residual, y: (N, C, H, W) with HW = H*W, NCHW or channels-last (LSS_CONV_NHWC: C a multiple
 * of 8 with 256 % (C / 8) == 0), element type dtype; gamma, beta and every statistic fp32.
 * partial: (C, ngroups, 2) fp32 scratch, ngroups from lss_bn_groups. save_mean, save_rstd, scale,
 * shift are the four rows of one (4, C) fp32 array (outputs kept for lss_bn_bwd).
 * num_batches_tracked (nullable): the module's int64 counter, incremented on the device (no
 * separate launch per BN layer).
 * Alignment of x, residual, y (and dy, dx, dresidual in the backward): the width of the vector the
 * kernels pick from the layout and HW -- LSS_CONV_NHWC: 16 B; LSS_CONV_NCHW: 16 B for fp32 with
 * HW % 4 == 0 and bf16 with HW % 8 == 0, 8 B for bf16 with HW % 8 == 4, else one element. gamma, beta,
 * the statistics and scratch: 4 B; num_batches_tracked: 8 B. */
int lss_bn_groups(int32_t N, int32_t C, int32_t HW, int32_t layout);
int lss_bn_fwd(const void* x, const void* residual, int32_t dtype, int32_t layout, int32_t N, int32_t C, int32_t HW,
               const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
               float* running_var, long long* num_batches_tracked, int32_t act, int32_t ngroups, float* partial,
               float* save_mean, float* save_rstd, float* scale, float* shift, void* y, void* stream);

/* Backward of lss_bn_fwd: dx (and dresidual = the gradient of the residual, nullable) of element
 * type dtype; dgamma, dbeta fp32 (nullable). y is the forward output (needed for ReLU). With
 * LSS_CONV_NHWC and a forward WITHOUT a residual, y may be NULL for ReLU: the kernels then recompute
 * it from x and the saved scale / shift exactly as the forward rounded it (one tensor read less).
 * Swish takes its slope at the pre-activation recomputed from x, scale and shift alone, so the backward of a
 * forward with LSS_ACT_SWISH AND a residual does not exist: LSS_ACT_SWISH with dresidual != NULL is
 * LSS_CONV_EINVAL (ABI 35), and a caller that gave such a forward a residual must not call this.
 * coef: (C, 2) fp32 scratch. */
int lss_bn_bwd(const void* dy, const void* x, const void* y, int32_t dtype, int32_t layout, int32_t N, int32_t C,
               int32_t HW, const float* scale, const float* shift, const float* save_mean, const float* save_rstd,
               int32_t act, int32_t ngroups, float* partial, float* coef, float* dgamma, float* dbeta, void* dx,
               void* dresidual, void* stream);

/* lss_bn_fwd / lss_bn_bwd with a sync workspace (lss_bn_sync_words() uint32, zero-filled once; every
 * call leaves it zero-filled; one call at a time per workspace; NULL = the calls above). For NCHW bf16
 * maps with several groups per channel (lss_bn_groups > 1), statistics and apply then run in ONE launch:
 * the blocks of a channel hold their groups in registers and meet on the channel's counters in the
 * workspace (bounded waits; a block that gives up recomputes the statistics itself). Same outputs,
 * bit for bit. The workspace's last word overrides the wait bound (0: built in; s > 0: s - 1 polls). */
int lss_bn_sync_words(void);
int lss_bn_fwd2(const void* x, const void* residual, int32_t dtype, int32_t layout, int32_t N, int32_t C, int32_t HW,
                const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                float* running_var, long long* num_batches_tracked, int32_t act, int32_t ngroups, float* partial,
                float* save_mean, float* save_rstd, float* scale, float* shift, void* y, uint32_t* sync,
                void* stream);
int lss_bn_bwd2(const void* dy, const void* x, const void* y, int32_t dtype, int32_t layout, int32_t N, int32_t C,
                int32_t HW, const float* scale, const float* shift, const float* save_mean, const float* save_rstd,
                int32_t act, int32_t ngroups, float* partial, float* coef, float* dgamma, float* dbeta, void* dx,
                void* dresidual, uint32_t* sync, void* stream);
/* (ABI 23) NHWC bf16 batch-norm backward whose incoming gradient is the rank-1 product
 * dy[p][c] = bf16(g1[p] * w1[c]) (g1: N*HW bf16, w1: C fp32), computed in the kernels instead of read --
 * the gradient the one-channel head hands back (lss_head1_bwd2 with dx = NULL). Otherwise lss_bn_bwd's
 * NHWC path with y = NULL, no residual; act LSS_ACT_NONE or LSS_ACT_RELU. And lss_bn_fwd / lss_bn_fwd2
 * accept y = NULL for LSS_CONV_NHWC: statistics, saved stats and running stats only, no apply pass.
 * Alignment: x and dx 16 B, g1 by element (2 B), the fp32 arrays 4 B. */
int lss_bn_bwd_rank1(const void* g1, const float* w1, const void* x, int32_t N, int32_t C, int32_t HW,
                     const float* scale, const float* shift, const float* save_mean, const float* save_rstd,
                     int32_t act, int32_t ngroups, float* partial, float* coef, float* dgamma, float* dbeta, void* dx,
                     void* stream);

/* (ABI 28) Eval-mode batch norm fused with an activation and a residual add, for inference
 * (model.eval() under no_grad, then out.sigmoid(): src/explore.py:244-246 eval_model_iou and 317-328
 * viz_model_preds) over the same layers as lss_bn_fwd (Up's BN + ReLU, src/models.py:22-28, and BevEncode,
 * src/models.py:97-115, and the EfficientNet-B0 trunk):
 *   y = act(fmaf(x, scale_c, shift_c) [+ residual]), rounded to the element type once,
 *   scale_c = gamma_c * rsqrtf(running_var_c + eps), shift_c = beta_c - running_mean_c * scale_c
 * -- the training kernels' expression with the running statistics in place of the batch's. act is
 * LSS_ACT_NONE, LSS_ACT_RELU or LSS_ACT_SWISH; residual (nullable) is allowed with each. One launch: the
 * kernel computes the coefficients it needs from the four arrays itself. Nothing but y is written:
 * gamma, beta (both nullable: 1 and 0) and the running statistics are read-only.
 * Layouts, element types and alignment of x, residual, y: exactly lss_bn_fwd's (NCHW any C; LSS_CONV_NHWC
 * with C % 8 == 0 and 256 % (C / 8) == 0; 16 B, 8 B for NCHW bf16 with HW % 8 == 4, else one element);
 * the fp32 arrays 4 B. LSS_CONV_EINVAL before any launch for anything else. */
int lss_bn_eval(const void* x, const void* residual, int32_t dtype, int32_t layout, int32_t N, int32_t C, int32_t HW,
                const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                float eps, int32_t act, void* y, void* stream);
/* (ABI 28) The same coefficients as the (4, C) fp32 array lss_head1_fwd2 / lss_headk_fwd take as bn_stats
 * (rows: running_mean, rstd, scale, shift): BevEncode's tail (src/models.py:111-115) in eval mode without
 * the normalised map, as src/explore.py:244-246, 317-328 run it. One small launch. */
int lss_bn_eval_coef(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                     float eps, int32_t C, float* stats /* (4, C) */, void* stream);

/* Which kernels a batch-norm entry point launches (ABI 35; host only: no HIP call, no allocation -- lss_bn_fwd2,
 * lss_bn_bwd2 and lss_bn_eval switch on the same rule, so it reports what this build launches). pass: the entry
 * point; dtype, layout, N, C, HW, act, ngroups as that entry point's (ngroups is not read for LSS_BN_EVAL);
 * has_sync: whether a sync workspace is passed (lss_bn_fwd / lss_bn_bwd: 0). The rule depends on these alone:
 * every entry point already refuses pointers off the alignment above. Families:
 *   LSS_BN_ARM_NHWC       channels-last training: statistics (ngroups blocks), fold, row-walking apply; v = 8,
 *     launches = 3 (the forward with y = NULL skips the apply: 2)
 *   LSS_BN_ARM_CLUSTER    NCHW bf16, HW % 8 == 0, a sync workspace, 2 <= ngroups <= 64, N / ngroups >= 2,
 *     C * ngroups <= 1024 (forward) / 2304 (backward), C <= 4096, and the largest group's 16-B vectors fit 8 per
 *     thread: one launch, it = 6 (at most 6 vectors per thread) or 8; relu = 1 for the backward's ReLU form
 *   LSS_BN_ARM_FUSED_REG  NCHW bf16, ngroups = 1, v in {8, 4}, cnt = N * HW / v <= 2048 vectors held in registers:
 *     (v, it) = (8, 4) cnt <= 1024, (8, 5) cnt <= 1280, (8, 8); (4, 4) cnt <= 1024, (4, 8)
 *   LSS_BN_ARM_FUSED      NCHW, ngroups = 1, anything else: one launch, v in {8, 4, 1}
 *   LSS_BN_ARM_TWO_PASS   NCHW, ngroups > 1 and no cluster: statistics + apply, v in {8, 4, 1}
 *   LSS_BN_ARM_EVAL_NCHW  lss_bn_eval: v as above except fp32 with HW % 8 == 0 takes 4; chunks = pieces of
 *     1024 vectors a channel is cut into
 *   LSS_BN_ARM_EVAL_NHWC  lss_bn_eval, channels-last: v = 8
 * v = elements per vector access (HW % 8 == 0: 8; HW % 4 == 0: 4; else 1); it, relu, chunks are 0 where the
 * kernel has none; blocks = the grid of the first launch. ngroups may exceed N (NCHW) or N * HW (NHWC): the
 * groups then left without an image or row publish zero sums, which is defined behaviour (lss_bn_groups never
 * picks such a count). Returns 0, or LSS_CONV_EINVAL as the entry point would for these arguments. */
enum { LSS_BN_FWD = 0, LSS_BN_BWD = 1, LSS_BN_EVAL = 2 };
enum { LSS_BN_ARM_NHWC = 0, LSS_BN_ARM_CLUSTER = 1, LSS_BN_ARM_FUSED_REG = 2, LSS_BN_ARM_FUSED = 3,
       LSS_BN_ARM_TWO_PASS = 4, LSS_BN_ARM_EVAL_NCHW = 5, LSS_BN_ARM_EVAL_NHWC = 6, LSS_BN_ARM_FAMILIES = 7 };
typedef struct lss_bn_arm {
    int32_t family, v, it, relu, launches, chunks, blocks;
} lss_bn_arm_t;
int lss_bn_arm(int32_t pass, int32_t dtype, int32_t layout, int32_t N, int32_t C, int32_t HW, int32_t act,
               int32_t ngroups, int32_t has_sync, lss_bn_arm_t* arm);

/* Bilinear upsampling with align_corners=True (nn.Upsample(mode="bilinear", align_corners=True),
 * src/models.py:19, 109) fused with Up's channel concatenation (torch.cat([x2, x1], 1),
 * src/models.py:33). All tensors channels-last bf16, 16-byte aligned, C1 and C2 multiples of 8,
 * upsampling only (Ho >= Hi > 1, Wo >= Wi > 1):
 *   y (N, Ho, Wo, C2 + C1) = cat([skip (N, Ho, Wo, C2), up(x (N, Hi, Wi, C1))]) -- skip may be NULL
 *   when C2 == 0; the blend is fp32 in PyTorch's order, rounded to bf16 once (the value the bf16
 *   autocast cast of the reference's fp32 upsample + cat produces). */
int lss_upsample_cat_fwd(const void* x, const void* skip, int32_t N, int32_t Hi, int32_t Wi, int32_t C1, int32_t C2,
                         int32_t Ho, int32_t Wo, void* y, void* stream);

/* dx (N, Hi, Wi, C1) bf16 = the upsample's backward applied to channels [C2, C2 + C1) of dy
 * (N, Ho, Wo, C2 + C1) bf16: a gather (each input element sums its weighted output gradients in
 * fp32, fixed order), no atomics. The skip's gradient is dy's first C2 channels (a view). */
int lss_upsample_bwd(const void* dy, int32_t N, int32_t Hi, int32_t Wi, int32_t C1, int32_t C2, int32_t Ho,
                     int32_t Wo, void* dx, void* stream);
/* (ABI 23) The same with chan_scale (nullable, N x C1 fp32): x's channel c of image n scaled by
 * chan_scale[n C1 + c] after the interpolation, and the input gradient by the same factor -- BevEncode's
 * Dropout2d (src/models.py:110: a per-(image, channel) 0 or 1 / (1 - p)) folded into up2's upsample. */
int lss_upsample_cat_fwd2(const void* x, const void* skip, int32_t N, int32_t Hi, int32_t Wi, int32_t C1, int32_t C2,
                          int32_t Ho, int32_t Wo, const float* chan_scale, void* y, void* stream);
int lss_upsample_bwd2(const void* dy, int32_t N, int32_t Hi, int32_t Wi, int32_t C1, int32_t C2, int32_t Ho,
                      int32_t Wo, const float* chan_scale, void* dx, void* stream);

/* Squeeze-and-excitation of an MBConv block (efficientnet_pytorch MBConvBlock, used by CamEncode's
 * trunk, src/models.py:43): y = x * sigmoid(W2 swish(W1 mean_hw(x) + b1) + b2), x / y (N, C, HW)
 * NCHW bf16 (HW % 4 == 0, C <= 2048, sq <= 64), W1 (sq, C), b1 (sq), W2 (C, sq), b2 (C) fp32
 * masters. Weights and values are rounded to bf16 where bf16 autocast rounds them (conv operands,
 * pooled map, both conv outputs, swish, sigmoid). Saved for the backward: m (N, C) pooled means, r / h (N, sq) reduce-conv output and
 * its swish, sig (N, C); all fp32 buffers. Alignment: x, y (and dy, dx of lss_se_bwd) 8-B aligned
 * (four bf16 per access).
 * (ABI 26) With the MLP tails (lss_se_tails) two launches: the plane means, whose last block of each image
 * to finish also runs both 1x1 convs for that image (the arithmetic and its order are those of the separate MLP launches, so the
 * values are the same bit for bit), then the scale pass. The hand-off is a ticket per image on a
 * counter the library owns (zero between calls), with no waiting; see lss_se_tails. */
int lss_se_fwd(const void* x, int32_t N, int32_t C, int32_t HW, const float* w1, const float* b1, const float* w2,
               const float* b2, int32_t sq, float* m, float* r, float* h, float* sig, void* y, void* stream);

/* Backward: dx (bf16) = dy * sig + dm / HW (the excitation and the pooling paths), and the
 * per-image gradients the caller turns into parameter gradients with small GEMMs: de (N, C) =
 * d(expand-conv output), dr (N, sq) = d(reduce-conv output), dm (N, C) = d(pooled means).
 * Scratch: t (N, C) fp32 (sum over HW of dy * x), dh_part (N, ceil(C / 64), sq) fp32.
 * (ABI 26) With the MLP tails two launches, as the forward: the plane sums t with the MLP backward in each image's last
 * block, then dx. The per-chunk partials of dh then stay on chip: dh_part must still be a valid buffer
 * of that size, its contents after the call are unspecified (the tails leave it untouched, the fallback
 * sequence of lss_se_tails stores the partials in it). */
int lss_se_bwd(const void* dy, const void* x, int32_t N, int32_t C, int32_t HW, const float* w1, const float* w2,
               int32_t sq, const float* r, const float* sig, float* t, float* dh_part, float* de, float* dr, float* dm,
               void* dx, void* stream);

/* The SE convs' parameter gradients from the backward's per-image values, in one launch (fp32, the N
 * images summed in order): dw1 (sq, C) = dr^T m, db1 (sq) = sum_n dr, dw2 (C, sq) = de^T h,
 * db2 (C) = sum_n de. */
int lss_se_wgrad(const float* de, const float* h, const float* dr, const float* m, int32_t N, int32_t C, int32_t sq,
                 float* dw1, float* db1, float* dw2, float* db2, void* stream);

/* (ABI 26) Switch of the per-image MLP tails in lss_se_fwd / lss_se_bwd. Settings:
 *   0  off: the earlier sequence of four launches each (mean / dot, two MLP kernels, scale / dx);
 *   1  on (the default): two launches each for the shapes where that measured faster -- small weight
 *      matrices, C * sq <= 1024 forward and <= 4096 backward -- and the earlier sequence for the rest;
 *   2  on for every shape (tests, tuning).
 * N > LSS_SE_TAIL_MAX_IMAGES (one counter word per image) always takes the earlier sequence. The results
 * are equal bit for bit whichever sequence runs. Sets the process-wide setting (on <= 0: 0, on >= 2: 2)
 * and returns the previous one; a captured graph keeps the sequence it was captured with.
 * Streams: the counters are per device, in a few banks that successive calls take in turn. That makes
 * two calls in flight at once on two streams of one device unlikely to share counters, not unable to:
 * the supported use is one stream per device, as for the batch-norm sync workspace. */
#define LSS_SE_TAIL_MAX_IMAGES 4096
int lss_se_tails(int on);

/* What lss_se_fwd / lss_se_bwd launch for a shape under the current lss_se_tails setting (ABI 37; host only: no HIP
 * call, no allocation -- both entry points read the same rule, so it reports what this build launches). pass: the
 * entry point; N, C, HW, sq as that entry point's. Returns 0, or LSS_CONV_EINVAL where the entry point would for these
 * sizes (and for an unknown pass or arm == NULL). The report:
 *   tails       1: the reduction with the per-image MLP tail, then scale / dx (launches = 2); 0: the sequence of four
 *   grid        blocks of each launch in order (zero past `launches`)
 *   bpi, cpb    tails: blocks per image and channels per block (cpb % 16 == 0; bpi = 1 once N > 512); sequence: 0
 *   planes_max, planes_min   the most and the fewest planes one wave of one block takes. Tails: a block of nch
 *               channels gives wave w ceil((nch - w) / 16) of them, the mean loading them four at a time and the dot
 *               two at a time; sequence: 1, or 0 for the idle waves of a last block (N * C % 4 != 0)
 *   w2_chunks   forward: pieces W2 goes through LDS in -- tails ceil(C / min(1024, 16384 / (sq + 1))), sequence
 *               ceil(C / 256); backward: 0
 *   chunks64    backward: ceil(C / 64), the 64-channel chunks (four 16-channel units each); forward: 0
 * and the classes these form -- every combination below that the sizes admit is a distinct path through the kernels:
 *   planes_class  min(planes_max, 5): 1 one plane a wave (the unbatched body); 2, 3, 4 one batch of the mean with that
 *               many live planes (the dot: 2; 2 + 1; 2 + 2); LSS_SE_PLANES_MANY = 5 several batches. Sequence: 1.
 *   ragged      planes_min < planes_max: a block whose waves do not all take the same number of planes
 *   chunk_class forward  LSS_SE_FWD_ONE_CHUNK   W2 staged once
 *                        LSS_SE_FWD_CHUNKS      several chunks, C <= 1024
 *                        LSS_SE_FWD_TWO_PASSES  tails only: C > 1024, so also a second pass of the block over the means
 *               backward LSS_SE_BWD_ONE_CHUNK   C <= 64
 *                        LSS_SE_BWD_UNIT_A_WAVE 2 to 4 chunks: each wave of the tail takes at most one unit
 *                        LSS_SE_BWD_UNITS_A_WAVE 5 to 16 chunks: a wave of the tail takes several units
 *                        LSS_SE_BWD_TWO_PASSES  C > 1024: also a second pass of the tail's block over t / de / dm
 *               (the sequence runs one block per chunk and sums as many partials, so the classes bound it as well)
 * The finite set: tails in {0, 1}; with the tails planes_class x ragged in {1..5} x {0, 1} and bpi = 1 or more, the
 * forward's three and the backward's four chunk classes; in the sequence ragged in {0, 1}, the forward's first two
 * and the backward's four chunk classes. */
enum { LSS_SE_FWD = 0, LSS_SE_BWD = 1 };
enum { LSS_SE_PLANES_MANY = 5 };
enum { LSS_SE_FWD_ONE_CHUNK = 0, LSS_SE_FWD_CHUNKS = 1, LSS_SE_FWD_TWO_PASSES = 2 };
enum { LSS_SE_BWD_ONE_CHUNK = 0, LSS_SE_BWD_UNIT_A_WAVE = 1, LSS_SE_BWD_UNITS_A_WAVE = 2, LSS_SE_BWD_TWO_PASSES = 3 };
typedef struct lss_se_arm {
    int32_t tails, launches, grid[4], bpi, cpb, planes_max, planes_min, w2_chunks, chunks64;
    int32_t planes_class, ragged, chunk_class;
} lss_se_arm_t;
int lss_se_arm(int32_t pass, int32_t N, int32_t C, int32_t HW, int32_t sq, lss_se_arm_t* arm);

#ifdef __cplusplus
}
#endif
#endif /* LSS_CONVS_H */
