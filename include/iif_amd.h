/*
 * iif_amd.h — C ABI of libiif_amd.so: the MI355X (gfx950) kernels behind the IIF
 * training hot path.  Plain pointers and sizes only; no torch / C++ types.
 *
 * Conventions
 *   - every `d_*` / device pointer is BORROWED: owned by the caller, must stay
 *     alive until the work enqueued on `stream` has completed; nothing is
 *     allocated or freed inside the library and no call synchronises.
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *     All work is enqueued on it; calls are re-entrant across streams and keep
 *     no global or thread-local state, so they may be captured into a hipGraph.
 *   - return value: IIF_OK (0) or a negative IIF_E* code; nothing throws.
 *   - dtype codes: IIF_F32 / IIF_BF16.  Activations are NHWC ("channels last"),
 *     weights KRSC ([Cout][R][S][Cin/groups]); this is the layout the kernels
 *     are tiled for (16-byte channel vectors feed the MFMA K dimension).
 *
 * Each entry point names the reference interface it replaces (file:line under
 * kostas1515/iif).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 */
#ifndef IIF_AMD_H
#define IIF_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IIF_OK 0
#define IIF_EINVAL (-1)       /* bad argument (null pointer, size <= 0, bad enum) */
#define IIF_EUNSUPPORTED (-2) /* shape / alignment the kernels are not built for */
#define IIF_ELAUNCH (-3)      /* hipLaunch / hip runtime error */

#define IIF_F32 0
#define IIF_BF16 1

/* table variants: classification/custom.py:16-23 */
#define IIF_RAW 0
#define IIF_SMOOTH 1
#define IIF_REL 2
#define IIF_NORMIT 3
#define IIF_GOMBIT 4
#define IIF_BASE2 5
#define IIF_BASE10 6

/* library / build info: "iif_amd <version> gfx950" */
const char* iif_version(void);

/* ------------------------------------------------------------------ IIF head */

/* HOST.  Per-class IIF weights from class counts.
 * Replaces the table construction of classification/custom.py:14-26
 * (float64 arithmetic, one cast to float32, optional division by the p-norm
 * of the float32 vector when norm_p > 0).  out_host: float[C]. */
int iif_build_table(const int64_t* counts_host, int C, int variant, int norm_p, float* out_host);

/* Fused IIF softmax cross-entropy, forward + gradient in ONE pass over logits.
 * Replaces classification/custom.py:28-36 (pred*iif -> CrossEntropyLoss('none',
 * weight) -> mean/sum), custom.py:116-117 (mixup criterion: pass targets_b and
 * lam) and mmdet/models/losses/iif_loss.py:184-202 + losses/utils.py:42-55
 * (row weights, ignore_index, avg_factor folded into `scale`).
 *
 *   z_i      = logits_i * table                               (row i, C classes)
 *   nll(i,t) = logsumexp(z_i) - z_i[t]   (0 if t == ignore_index)
 *   r_i      = row_weight_i * ( lam*cw[ta_i]*nll(i,ta_i) + (1-lam)*cw[tb_i]*nll(i,tb_i) )
 *   loss     = scale * sum_i r_i            (scale = 1/B for 'mean', 1 for 'sum',
 *                                            loss_weight/avg_factor for mmdet)
 *   dlogits[i,c] = scale * d r_i / d logits[i,c]
 *
 * logits/dlogits: [B, C] row-major with leading dimensions ld_logits / ld_dlogits
 * (elements), dtype IIF_F32 or IIF_BF16 (math is fp32 either way).
 * targets_b == NULL means no mixup (lam ignored).  row_weight / class_weight may
 * be NULL (= ones).  loss_per_row: float[B] (required; receives r_i, the
 * reduction='none' value).  loss_out: float[1] or NULL.  dlogits may be NULL
 * (loss only).  d_status: int32[1] or NULL; set to 1 if any target is outside
 * [0,C) and != ignore_index (such rows contribute 0).
 * d_workspace: IIF_CE_WORKSPACE_BYTES of device memory or NULL.  Its first int32 is a
 * ticket that must be ZERO on entry (zero it once; the kernel leaves it zero again),
 * the rest holds one partial sum per block.  With a workspace the scalar loss comes
 * out of the SAME launch (the last block to finish sums the per-block partials);
 * without it a second, one-block launch sums loss_per_row.  A workspace must not be
 * shared by calls that can run concurrently (one per stream).
 * Deterministic either way (fixed-order trees, no float atomics); the two paths
 * associate the sum differently and may differ in the last fp32 bits.
 * The softmax runs in base 2 on v_exp_f32 / v_log_f32 (~1 ulp each). */
int iif_ce_fwd_bwd(const void* logits, int dtype, int64_t ld_logits,
                   const float* table, const int64_t* targets_a, const int64_t* targets_b,
                   float lam, const float* row_weight, const float* class_weight,
                   int64_t ignore_index, float scale, int B, int C,
                   float* loss_per_row, float* loss_out,
                   void* dlogits, int64_t ld_dlogits, int32_t* d_status, void* d_workspace, void* stream);
#define IIF_CE_WORKSPACE_BYTES (4 * (1 + 2048))

/* Fused sigmoid BCE / focal loss, forward + gradient in ONE pass over logits.
 * Replaces classification/custom.py:42-89 (FocalLoss: one-hot targets, sigmoid,
 * BCELoss / BCEWithLogitsLoss, modulating factor, class weights, alpha_t, reduction)
 * and custom.py:116-117 (mixup criterion: pass targets_b and lam).
 *
 *   y        = one-hot of the row's target,  s = sigmoid(x),  w_c = class_weight[c] (1 if NULL)
 *   gamma==0: l(x,y) = softplus(x) - x*y                      (alpha ignored, as the reference)
 *   gamma >0: l(x,y) = BCE(s,y) * (1-p_t)^gamma * alpha_t,   p_t = s*y + (1-s)*(1-y),
 *             alpha_t = alpha*y + (1-alpha)*(1-y) if use_alpha, else 1
 *   r_i      = sum_c w_c * ( lam*l(x_ic, [c==ta_i]) + (1-lam)*l(x_ic, [c==tb_i]) )
 *   loss     = scale * sum_i r_i   (scale = 1/(B*C) for 'mean' / 'none', 1/B for 'sum')
 *   dlogits[i,c] = scale * d r_i / d logits[i,c]
 *
 * The function is evaluated exactly at every |x| (stable softplus forms); the
 * reference's nn.BCELoss path saturates once sigmoid(x) rounds to 1 in fp32.
 * logits/dlogits: [B, C] row-major with leading dimensions ld_logits / ld_dlogits
 * (elements), dtype IIF_F32 or IIF_BF16 (math is fp32; dlogits in the logits'
 * dtype); both pointers element-aligned.  targets_b == NULL means no mixup (lam
 * ignored).  class_weight: float[C] or NULL.  gamma >= 0 and finite; 1 and 2 are
 * evaluated as multiplies.  loss_per_row: float[B] (required; receives r_i).
 * loss_out: float[1] or NULL.  dlogits may be NULL (loss only).  d_status: int32[1]
 * or NULL; set to 1 if any target is outside [0,C) (such rows contribute 0; there
 * is no ignore index).  d_workspace: IIF_CE_WORKSPACE_BYTES with the same contract
 * as iif_ce_fwd_bwd's (ticket zero on entry and exit, one workspace per stream);
 * with it the scalar loss comes out of the same launch.  Deterministic (fixed-order
 * sums, no float atomics).  B == 0 writes a zero loss. */
int iif_sigmoid_focal_fwd_bwd(const void* logits, int dtype, int64_t ld_logits,
                              const int64_t* targets_a, const int64_t* targets_b, float lam,
                              const float* class_weight, float gamma, int use_alpha, float alpha,
                              float scale, int B, int C, float* loss_per_row, float* loss_out,
                              void* dlogits, int64_t ld_dlogits, int32_t* d_status, void* d_workspace,
                              void* stream);

/* Detection-style sigmoid BCE (mmdet's binary_cross_entropy), forward + gradient in ONE launch, no host round trip.
 * Replaces mmdet/models/losses/cross_entropy_loss.py:53-111 (_expand_onehot_labels, binary_cross_entropy) +
 * losses/utils.py:29-55 (weight_reduce_loss).
 *
 * Label mode (labels != NULL, targets == NULL), element (i, c) of pred [N, C]:
 *   valid_i = labels_i >= 0 and labels_i != ignore_index
 *   y_ic    = [labels_i == c]          (a valid label >= C is an all-zero row: background, not an error)
 *   w_ic    = valid_i * (row_weight_i, 1 if NULL)
 * Dense mode (targets != NULL, labels == NULL; the reference's pred.dim() == label.dim() branch):
 *   y_ic = targets[i, c],  w_ic = elem_weight[i, c] (1 if NULL); float [N, C] contiguous; no ignore index.
 * Either mode, pw_c = class_weight[c] as torch's pos_weight (1 if NULL):
 *   l_ic     = (1 - y) x + (1 + (pw_c - 1) y) softplus(-x)     (evaluated as (1 - y) softplus(x) + pw_c y softplus(-x):
 *                                                               exact at every |x|)
 *   loss     = scale * sum_ic w_ic l_ic      (scale = loss_weight / (N C) for 'mean', loss_weight for 'sum',
 *                                             loss_weight / avg_factor with an avg_factor)
 *   dpred_ic = scale * w_ic * ((1 - y) sigmoid(x) - pw_c y (1 - sigmoid(x)))
 *
 * pred / dpred: [N, C] row-major with leading dimensions ld_pred / ld_dpred (elements), IIF_F32 or IIF_BF16 (math is
 * fp32; dpred in the dtype of pred), element-aligned; dpred may be NULL (loss only).  loss_elems: float [N, C]
 * contiguous or NULL, receives the unscaled w_ic l_ic (reduction 'none').  loss_out: float[1] or NULL; with it
 * d_workspace is required: IIF_CE_WORKSPACE_BYTES under iif_ce_fwd_bwd's contract (ticket zero on entry and exit, one
 * workspace per stream), and the scalar leaves the same launch.  Deterministic (fixed-order sums, no float atomics).
 * The kernel walks the flat element range in 16-byte pieces and carries each piece's (row, column) along: any C >= 1
 * (C = 1 with N in the hundreds of thousands is the RPN shape), 64-bit indexing.  That form needs ld == C and element
 * h of every array on a 16-byte boundary, h = the first element of pred that is; any other pitch or phase runs the
 * same arithmetic one element per lane.  N == 0 writes a zero loss without a launch. */
int iif_bce_det_fwd_bwd(const void* pred, int dtype, int64_t ld_pred, const int64_t* labels, const float* row_weight,
                        int64_t ignore_index, const float* targets, const float* elem_weight,
                        const float* class_weight, float scale, int N, int C, float* loss_elems, float* loss_out,
                        void* dpred, int64_t ld_dpred, void* d_workspace, void* stream);

/* Box-regression loss (mmdet's l1_loss / smooth_l1_loss), forward + COMPACT gradient in ONE launch, no host round trip.
 * Replaces mmdet/models/losses/smooth_l1_loss.py:10-52 + losses/utils.py:29-55 and, in gather mode, the positive-row
 * selection of mmdet/models/roi_heads/bbox_heads/bbox_head.py:284-311 (pos_inds.any(), three boolean indexings).
 *
 * Plain mode (labels == NULL, C == 1): pred, target and weight are the same flat range of n elements (pred contiguous;
 *   ld_pred, num_classes and N are not read); n >= 0, not necessarily a multiple of 4.
 * Gather mode (labels != NULL: int64[N], n == 4N): pred is [N, 4C] with leading dimension ld_pred >= 4C (elements);
 *   row i is positive iff 0 <= labels_i < num_classes, and its four predictions are pred[i, 4 labels_i .. 4 labels_i + 3]
 *   (C > 1; num_classes <= C) or pred[i, 0 .. 3] (C == 1: a class-agnostic head, any num_classes >= 1).  target /
 *   weight / dsel / loss_elems are [N, 4] contiguous; a row that is not positive reads nothing of pred and contributes
 *   nothing: its dsel and loss_elems are exact zeros.
 * Per element, d = p - t, a = |d|:
 *   beta == 0 (L1):        l = a,                  dl = sign(d), sign(0) = 0
 *   beta  > 0 (smooth L1): a < beta (strict) ?  l = 0.5 a a / beta,  dl = d / beta  :  l = a - 0.5 beta,  dl = sign(d)
 *   loss = scale * sum w l   (w = weight, 1 if NULL; scale = loss_weight / n for 'mean', loss_weight for 'sum',
 *                             loss_weight / avg_factor with an avg_factor)
 *   dsel[e]       = scale * w * dl      (float[n] or NULL: the gradient w.r.t. the SELECTED predictions, fp32)
 *   loss_elems[e] = w * l               (float[n] or NULL: unscaled, reduction 'none')
 * pred: IIF_F32 or IIF_BF16 (math is fp32), element-aligned.  loss_out: float[1] or NULL; with it d_workspace is
 * required: IIF_CE_WORKSPACE_BYTES under iif_ce_fwd_bwd's contract (ticket zero on entry and exit, one workspace per
 * stream), and the scalar leaves the same launch.  Deterministic (fixed-order sums, no float atomics): bit-identical
 * from call to call.  A lane takes one box (four elements: 16 bytes of every fp32 array, 16 / 8 bytes of pred) when
 * pred's boxes sit on a 4-element boundary (base and, in gather mode, ld_pred % 4 == 0) and every fp32 array on a
 * 16-byte one; any other phase runs one element per lane.  64-bit indexing.  n == 0 writes a zero loss without a
 * launch.  Backward in plain mode is iif_scale_by_device_scalar on dsel; in gather mode iif_bbox_reg_scatter_grad. */
int iif_bbox_reg_fwd(const void* pred, int dtype, int64_t ld_pred, const int64_t* labels, int num_classes, int C,
                     const float* target, const float* weight, float beta, float scale, int64_t n, int N,
                     float* loss_elems, float* loss_out, float* dsel, void* d_workspace, void* stream);

/* The dense gradient of gather mode in ONE launch, a pure store stream: dpred [N, 4C] (dtype IIF_F32 or IIF_BF16,
 * leading dimension ld_dpred >= 4C elements, element-aligned) receives *g * dsel[i, 0..3] at row i, columns
 * 4 labels_i .. 4 labels_i + 3 (C == 1: columns 0 .. 3) for the positive rows (0 <= labels_i < num_classes) and exact
 * zero in every other column of [0, 4C).  Columns beyond 4C of a wider pitch are not touched.  g: the upstream
 * gradient of the scalar loss, a DEVICE float (NULL = 1), so nothing synchronises.  Every byte has exactly one writer
 * within the launch: no memset, no fill-then-overwrite.  dpred on a 16-byte boundary with ld_dpred == 4C is written in
 * 16-byte pieces (one class of fp32, two classes of bf16 - with odd C a piece straddles two rows); any other base or
 * pitch goes one element per lane.  N == 0 is a no-op. */
int iif_bbox_reg_scatter_grad(const float* dsel, const int64_t* labels, int num_classes, int N, int C, const float* g,
                              void* dpred, int dtype, int64_t ld_dpred, void* stream);

/* The classification half of BBoxHead.loss (mmdet/models/roi_heads/bbox_heads/bbox_head.py:266-283) in ONE launch and with NO
 * host read (csrc/head_loss.hip): the softmax cross entropy of iif_ce_fwd_bwd with avg_factor = max(#{label_weights > 0}, 1)
 * counted on the device, and the top-1 accuracy (mmdet/models/losses/accuracy.py:7-51) of the rows that count.
 * scores [N, C], row pitch ld_scores >= C (elements), IIF_F32 or IIF_BF16 (math is fp32), element-aligned;
 * l_i = labels[i] (int64), w_i = label_weights[i] (NULL = ones), cw = class_weight (NULL = ones), table NULL = ones:
 *   z_i    = scores_i * table
 *   nll_i  = cw[l_i] * (logsumexp(z_i) - z_i[l_i])           0 if l_i == ignore_index
 *   V      = #{ i : w_i > 0 },  avg = max(V, 1)
 *   loss   = loss_weight * (sum_i w_i nll_i) / avg
 *   hit_i  = no column of the RAW scores_i outranks column l_i (greater, or equal at a lower index: iif_topk_hits' tie rule)
 *   acc    = float(sum_{w_i > 0} hit_i) * float(100.0 / avg)   0 when V == 0
 *   dscores[i, c] = w_i * cw[l_i] * table[c] * (softmax(z_i)[c] - [c == l_i])     WITHOUT loss_weight / avg: iif_head_loss_bwd
 * The scores of a row with w_i == 0 are NOT READ and its label is not looked at: its dscores row is zeros and it takes no part in loss, V
 * or acc (the padded rows of iif_roi_stage_targets; the reference computes 0 * nll there, NaN for a non-finite row).  A row
 * with w_i < 0 enters the loss but not V, as in the reference.  Of a row with w_i != 0, a label equal to ignore_index, or
 * outside [0, C), contributes 0, is never a hit and gets a zero dscores row; the latter also sets d_status (int32[1] or NULL)
 * to 1, as iif_ce_fwd_bwd does.
 * loss_out, acc_out, avg_out: DEVICE floats, all required.  dscores: [N, C] in the scores' dtype, pitch ld_dscores >= C, or
 * NULL (loss only).  d_workspace: IIF_HEAD_LOSS_WORKSPACE_BYTES (the IIF_CE_WORKSPACE_BYTES buffer of a stream is large
 * enough and may be shared: same contract - its first int32 zero on entry, zero again on exit; nothing else has to be zero).
 * V and the hit count are integer sums, the float sum is added in an order fixed by N: the same bits from call to call.
 * N == 0 writes loss 0, acc 0, avg 1 (one launch).
 * Before anything is launched: IIF_EINVAL for N outside 0 .. IIF_HEAD_LOSS_MAX_ROWS, C < 2, an unknown dtype, a null or
 * misaligned output / workspace / scores / labels, a pitch smaller than C; IIF_EUNSUPPORTED for C > IIF_HEAD_LOSS_MAX_CLASSES. */
#define IIF_HEAD_LOSS_MAX_ROWS 65535
#define IIF_HEAD_LOSS_MAX_CLASSES 2048
#define IIF_HEAD_LOSS_WORKSPACE_BYTES (4 * (4 + 3 * 512))
int iif_head_loss_fwd(const void* scores, int dtype, int64_t ld_scores, const float* table, const int64_t* labels,
                      const float* label_weights, const float* class_weight, int64_t ignore_index, float loss_weight, int N, int C,
                      void* dscores, int64_t ld_dscores, float* loss_out, float* acc_out, float* avg_out, int32_t* d_status,
                      void* d_workspace, void* stream);

/* Backward of iif_head_loss_fwd in ONE launch: out[e] = dscores[e] * (*d_upstream * loss_weight / *d_avg) over n contiguous
 * elements (IIF_F32 / IIF_BF16, element-aligned; 16-byte pieces when both bases allow).  d_upstream (the gradient of the
 * scalar loss) and d_avg (iif_head_loss_fwd's avg_out) are DEVICE floats, so nothing synchronises; dscores is left intact
 * (backward may run twice).  n == 0 is a no-op.  IIF_EINVAL: n < 0, a null or misaligned pointer, an unknown dtype. */
int iif_head_loss_bwd(const void* dscores, int dtype, int64_t n, const float* d_upstream, const float* d_avg, float loss_weight,
                      void* out, void* stream);

/* iif_head_loss_fwd for the SIGMOID head, CrossEntropyLoss(use_sigmoid=True): mmdet's binary_cross_entropy with one class index
 * per row (mmdet/models/losses/cross_entropy_loss.py:53-111, the element loss of iif_bce_det_fwd_bwd) in ONE launch and with NO
 * host read (csrc/head_loss.hip).  scores [N, C], 1 <= C <= IIF_HEAD_LOSS_MAX_CLASSES, row pitch ld_scores >= C, IIF_F32 or
 * IIF_BF16 (math is fp32), element-aligned; l_i = labels[i], w_i = label_weights[i] (NULL = ones), pw = class_weight (torch's
 * pos_weight, NULL = ones); sp = softplus, s = sigmoid:
 *   valid_i = l_i >= 0 and l_i != ignore_index,   y_ic = [l_i == c]   (a valid label >= C is a background row, not an error)
 *   l_ic    = (1 - y_ic) sp(x_ic) + pw_c y_ic sp(-x_ic)
 *   V       = #{ i : w_i > 0 },  avg = max(V, 1)
 *   loss    = loss_weight * (sum_i w_i valid_i sum_c l_ic) / avg
 *   hit_i   = l_i in [0, C) and no column of the RAW scores_i outranks column l_i (iif_topk_hits' tie rule)
 *   acc     = float(sum_{w_i > 0} hit_i) * float(100.0 / avg)   0 when V == 0
 *   dscores[i, c] = w_i valid_i ((1 - y_ic) s(x_ic) - pw_c y_ic (1 - s(x_ic)))       WITHOUT loss_weight / avg: iif_head_loss_bwd
 * A row with w_i == 0 is NOT READ, its label included: its dscores row is zeros and it takes no part in loss, V or acc.  A row
 * with w_i < 0 enters the loss but not V or acc.  dscores equals iif_bce_det_fwd_bwd's dpred at scale 1 bit for bit (fp32).
 * loss_out, acc_out, avg_out, dscores, d_workspace (IIF_HEAD_LOSS_WORKSPACE_BYTES) and the order of the sums: as
 * iif_head_loss_fwd's.  N == 0 writes loss 0, acc 0, avg 1 (one launch).
 * Before anything is launched: IIF_EINVAL for N outside 0 .. IIF_HEAD_LOSS_MAX_ROWS, C < 1, an unknown dtype, a null or
 * misaligned output / workspace / scores / labels, a pitch smaller than C; IIF_EUNSUPPORTED for C > IIF_HEAD_LOSS_MAX_CLASSES. */
int iif_head_bce_loss_fwd(const void* scores, int dtype, int64_t ld_scores, const int64_t* labels, const float* label_weights,
                          const float* class_weight, int64_t ignore_index, float loss_weight, int N, int C, void* dscores,
                          int64_t ld_dscores, float* loss_out, float* acc_out, float* avg_out, void* d_workspace, void* stream);

/* ---- Box overlaps and max-IoU assignment (csrc/assign.hip): mmdet/core/bbox/iou_calculators/iou2d_calculator.py:75-261 and
 * mmdet/core/bbox/assigners/max_iou_assigner.py:61-213 without the [G, N] overlap matrix.
 *
 * Boxes are float32 rows <x1, y1, x2, y2> with a row pitch in ELEMENTS (>= 4: an [n, 5] array with a score column is read in
 * place), element-aligned.  Each step is one IEEE float32 operation in the reference's order, the division correctly rounded:
 *   area = (x2 - x1) * (y2 - y1);  w, h = max(min(rb) - max(lt), 0);  overlap = w * h
 *   mode 0 'iou':  overlap / max(area1 + area2 - overlap, eps)      mode 1 'iof':  overlap / max(area1, eps)
 *   mode 2 'giou': iou - (max(enclose, eps) - union) / max(enclose, eps)
 * so the results are the reference's float32 numbers bit for bit (NaN coordinates excepted).
 *
 * iif_bbox_overlaps: out is float[m, n] contiguous (aligned == 0) or float[n] for the pairs (i, i) (aligned != 0: m == n).
 * One launch; m == 0 or n == 0 is a no-op. */
int iif_bbox_overlaps(const float* bboxes1, int64_t ld1, int64_t m, const float* bboxes2, int64_t ld2, int64_t n, int mode,
                      int aligned, float eps, float* out, void* stream);

/* MaxIoUAssigner.assign for N candidate boxes and G ground-truth boxes (eps = 1e-6, the calculator's default):
 *   overlap(i, j) = iou(gt i, candidate j), or -1 for every i if candidate j is IGNORED: ignore_bboxes != NULL, I > 0,
 *     ignore_iof_thr > 0 and max over the ignore boxes k of iof > ignore_iof_thr, where iof = iof(candidate j, ignore k) if
 *     ignore_wrt_candidates else iof(ignore k, candidate j);
 *   max_overlaps[j] = max_i overlap(i, j), argmax the LOWEST such i;  gt_max[i] = max_j overlap(i, j), gt_argmax[i] the
 *     LOWEST such j;
 *   gt_inds[j] = -1;  = 0 where neg_lo <= max_overlaps[j] < neg_hi (a single threshold t is (0, t));  = argmax + 1 where
 *     max_overlaps[j] >= pos_iou_thr;  then, if match_low_quality, for i ascending with gt_max[i] >= min_pos_iou:
 *     gt_inds[j] = i + 1 for every j with overlap(i, j) == gt_max[i] (gt_max_assign_all) or for j = gt_argmax[i] only;
 *   labels[j] = gt_labels[gt_inds[j] - 1] where gt_inds[j] > 0, else -1  (labels NULL: not wanted; else gt_labels is required).
 * All comparisons are float32.  G == 0: gt_inds 0, max_overlaps 0, labels -1.  N == 0: a no-op.
 * d_workspace: IIF_ASSIGN_WORKSPACE_BYTES(G) of device memory on an 8-byte boundary, required when match_low_quality and G > 0;
 * it belongs to this call until the stream has run it (contents on entry do not matter: the call clears it) - calls on
 * different streams need different workspaces.  At most three operations are enqueued (the clear and two launches; one launch
 * without match_low_quality), nothing is allocated, nothing synchronises; the [G, N] matrix is never stored.  Integer atomics
 * only: the result does not depend on arrival order.  N, G, I < 2^31. */
#define IIF_ASSIGN_WORKSPACE_BYTES(G) (8 * ((int64_t)(G) + 1))
int iif_max_iou_assign(const float* bboxes, int64_t ld_bboxes, int64_t N, const float* gt_bboxes, int64_t ld_gt, int64_t G,
                       const float* ignore_bboxes, int64_t ld_ignore, int64_t I, float pos_iou_thr, float neg_lo, float neg_hi,
                       float min_pos_iou, float ignore_iof_thr, int gt_max_assign_all, int ignore_wrt_candidates,
                       int match_low_quality, const int64_t* gt_labels, int64_t* gt_inds, float* max_overlaps, int64_t* labels,
                       void* d_workspace, int64_t workspace_bytes, void* stream);

/* ---- Box sampling, the delta coder and the target builders (csrc/targets.hip): what lies between the assigner above and the
 * losses - mmdet/core/bbox/coder/delta_xywh_bbox_coder.py:98-272, core/bbox/samplers/base_sampler.py:35-102 with
 * random_sampler.py:32-82 and sampling_result.py, dense_heads/anchor_head.py:224-265, roi_heads/bbox_heads/bbox_head.py:122-186.
 * Every entry enqueues on `stream`, allocates nothing, reads nothing back to the host.  Boxes are float32 rows with a pitch in
 * ELEMENTS (>= 4), element-aligned, as in iif_bbox_overlaps.  means / stds: HOST pointers to four floats each, read during the
 * call.  Dense float outputs ([.., 4] targets, weights, decoded boxes) are contiguous and 16-byte aligned.
 *
 * iif_bbox2delta: out [n, 4] = ((dx, dy, dw, dh) - means) / stds with px = (x1 + x2) * 0.5, pw = x2 - x1 (likewise g),
 *   dx = (gx - px) / pw, dw = logf(gw / pw): each step one IEEE float32 operation in the reference's order, so dx, dy are
 *   the reference's bit for bit and dw, dh up to the logarithm's rounding; zero-width boxes give the reference's infinities and
 *   NaNs.  One launch, one lane per row; n == 0 is a no-op. */
int iif_bbox2delta(const float* proposals, int64_t ld_proposals, const float* gt, int64_t ld_gt, int64_t n, const float* means,
                   const float* stds, float* out, void* stream);

/* iif_delta2bbox: rois [n, >= 4], deltas [n, 4 num_classes] (pitch ld_deltas), out [n, 4 num_classes]; one lane per (row, class):
 *   d = delta * std + mean (two operations);  dxw = pw * dx;  add_ctr_clamp: dxw, dyh clamped to [-ctr_clamp, ctr_clamp] and
 *   dw, dh to (.., max_ratio], otherwise dw, dh to [-max_ratio, max_ratio];  gw = pw * expf(dw);  gx = px + dxw;
 *   x1 = gx - gw * 0.5, x2 = gx + gw * 0.5;  clip != 0: x < 0 ? 0 : x, then x > max ? max : x against max_w (x) and max_h (y).
 *   A NaN passes through the clamps and the clip as in torch.  max_ratio: float(abs(log(wh_ratio_clip))), computed in double
 *   by the caller.  clip == 0 is the reference's clip_border=False or max_shape=None.  No batch dimensions. */
int iif_delta2bbox(const float* rois, int64_t ld_rois, const float* deltas, int64_t ld_deltas, int64_t n, int num_classes,
                   const float* means, const float* stds, float max_ratio, int add_ctr_clamp, float ctr_clamp, int clip,
                   float max_h, float max_w, float* out, void* stream);

/* RandomSampler.sample on the assigner's gt_inds [N] (> 0 positive, 0 negative, < 0 ignored) with one random key per
 * candidate, keys [N] int32 >= 0 (the sign bit is not read):
 *   positives: all if at most num_expected_pos, else the num_expected_pos SMALLEST (key, index) pairs - equal keys go to the
 *     lower index;  negatives: budget num - (positives kept), capped at int(neg_pos_ub * max(1, kept)) when neg_pos_ub >= 0
 *     (a double, multiplied and truncated as Python does); the same rule.
 *   pos_inds [num_expected_pos], neg_inds [num]: the kept indices ascending (the reference's unique() sorts), unused tails -1;
 *   counts [2]: positives, negatives kept;  flags [N] int8: 0 not sampled, 1 positive, 2 negative.
 * With keys[gallery[j]] = inverse_permutation[j] per class this selects exactly the reference's gallery[randperm[:k]].
 * Three enqueued operations (a clear of 32 KiB + 16 bytes and two launches), no host read; gt_inds and keys are each read twice;
 * integer atomics only, so the result does not depend on arrival order and is correct for any keys, all equal included.
 * d_workspace: IIF_SAMPLE_WORKSPACE_BYTES(N) on a 16-byte boundary; it belongs to the call until the stream has run it
 * (contents on entry do not matter).  N < 2^31 - 4, 0 <= num_expected_pos <= num.  N == 0: the tails and zero counts are written. */
#define IIF_SAMPLE_WORKSPACE_BYTES(N) (4 * (int64_t)(N) + 65536)
int iif_random_sample(const int64_t* gt_inds, const int32_t* keys, int64_t N, int64_t num_expected_pos, int64_t num,
                      double neg_pos_ub, int64_t* pos_inds, int64_t* neg_inds, int64_t* counts, int8_t* flags, void* d_workspace,
                      int64_t workspace_bytes, void* stream);

/* AnchorHead._get_targets_single after assign and sample, with unmap_outputs=True, in one launch over the FULL anchor set [A]:
 *   row = compact_index ? compact_index[a] : a  (compact_index: -1 for an anchor that took no part - outside the image - else its
 *   row in flags / gt_inds [rows]; NULL: identity, rows == A);
 *   flags[row] == 1: labels = gt_labels ? gt_labels[gt_inds[row] - 1] : 0, label_weights = pos_weight <= 0 ? 1 : pos_weight,
 *     bbox_targets = reg_decoded_bbox ? gt box : bbox2delta(anchor, gt box) (iif_bbox2delta's arithmetic), bbox_weights = 1;
 *   flags[row] == 2: label_weights = 1;  otherwise and elsewhere: labels = background_label, zeros.
 * Rows and gt indices out of range are treated as "took no part". */
int iif_anchor_targets(const float* anchors, int64_t ld_anchors, int64_t A, const int8_t* flags, const int64_t* gt_inds,
                       int64_t rows, const float* gt_bboxes, int64_t ld_gt, int64_t G, const int64_t* gt_labels,
                       const int64_t* compact_index, int64_t background_label, float pos_weight, int reg_decoded_bbox,
                       const float* means, const float* stds, int64_t* labels, float* label_weights, float* bbox_targets,
                       float* bbox_weights, void* stream);

/* BBoxHead._get_target_single on the padded lists of iif_random_sample (pos_inds [cap_pos], neg_inds [cap], counts [2]), with
 * SamplingResult's gathers and bbox2roi; one lane per output row r < cap:
 *   r < counts[0]: candidate pos_inds[r], a positive: labels = labels_in[candidate] (the assigner's per-candidate labels; NULL: 0),
 *     label_weights = pos_weight <= 0 ? 1 : pos_weight, bbox_targets as in iif_anchor_targets, bbox_weights = 1,
 *     pos_assigned_gt_inds = gt_inds[candidate] - 1;
 *   r < counts[0] + counts[1]: candidate neg_inds[r - counts[0]]: labels = num_classes, label_weights = 1, zeros, -1;
 *   beyond: padding - a zero box, labels = num_classes, all weights 0, -1: it adds nothing to a loss.
 *   rois [cap, 5] = (img_index, the candidate's box). */
int iif_roi_targets(const float* bboxes, int64_t ld_bboxes, int64_t N, const int64_t* gt_inds, const int64_t* labels_in,
                    const float* gt_bboxes, int64_t ld_gt, int64_t G, const int64_t* pos_inds, const int64_t* neg_inds,
                    const int64_t* counts, int64_t cap, int64_t cap_pos, int img_index, int64_t num_classes, float pos_weight,
                    int reg_decoded_bbox, const float* means, const float* stds, float* rois, int64_t* labels,
                    float* label_weights, float* bbox_targets, float* bbox_weights, int64_t* pos_assigned_gt_inds, void* stream);

/* ---- The RoI stage in one launch (csrc/roi_stage.hip): assign, add the ground truth, sample and build the targets for all B
 * images of a batch, reading each image's number of valid proposals from DEVICE memory - what roi_heads/standard_roi_head.py:85-100
 * and BBoxHead.get_targets do per image.  One workgroup per image.
 *
 * images: HOST array of B descriptors, copied into the launch: the image's ground-truth boxes [G, >= 4] (pitch ld_gt elements)
 *   and labels [G] on the device, G (known from the shapes: no read) and the image index written into the rois.
 * proposals: float32 rows <x1, y1, x2, y2, ...>; row i of image b at proposals + b * ld_image + i * ld_row (ld_row >= 4: dets
 *   [B, P, 5] and refined boxes [B, P, 4] both go in unchanged).  n_b = clamp(proposal_counts[b], 0, P), or P when
 *   proposal_counts is NULL; rows at or beyond n_b are NEVER READ.
 * Candidates of image b: the ground-truth boxes, then the n_b proposals, when add_gt_as_proposals and G > 0 (front = G), else the
 *   proposals alone (front = 0); M_b = front + n_b, candidate c < front is gt c.
 * Assignment: iif_max_iou_assign's definition above on the PROPOSALS (no ignore boxes; the low-quality match never sees the gt
 *   boxes as candidates; lowest gt on equal overlaps, lowest proposal for a gt's maximum), then the gt candidates get
 *   gt_inds c + 1 and their own labels, as AssignResult.add_gt_ does.  Per-gt maxima are 64-bit integer maxima in LDS.
 * Sampling: iif_random_sample's rule with the key of candidate c of image b at keys[b * ld_keys + c] (ld_keys >= max front + P):
 *   the num_expected_pos smallest (key, index) pairs of the positives, the negative budget num - kept positives capped by
 *   neg_pos_ub in the same double arithmetic; index lists ascending; correct for any keys, all equal included.
 * Rows [b * num, (b + 1) * num) of rois [B num, 5], labels, label_weights, bbox_targets [B num, 4], bbox_weights,
 *   pos_assigned_gt_inds: positives, negatives, padding - iif_roi_targets' rows for that image, bit for bit.
 * counts [B, 2]: positives, negatives kept.  pos_is_gt [B num] uint8: 1 where the row is a ground-truth box (0 on negatives and
 *   padding).  Rows [b * num_expected_pos, ..) of pos_rois [.., 5], pos_gt_inds, pos_labels: the positives alone, for the mask
 *   branch; unused rows carry image index -1, gt index -1, label num_classes.
 * Limits: 1 <= B <= 16, P <= 4096, G <= 1024, num <= 1024, 0 <= num_expected_pos <= num; beyond them IIF_EINVAL.
 * One launch, nothing allocated, nothing synchronises, no workspace; integer atomics only: no result depends on arrival order. */
typedef struct iif_roi_image {
    const float* gt_bboxes;
    int64_t ld_gt;
    const int64_t* gt_labels;
    int32_t G;
    int32_t img_index;
} iif_roi_image;
int iif_roi_stage_targets(const iif_roi_image* images, int B, const float* proposals, int64_t ld_row, int64_t ld_image, int64_t P,
                          const int64_t* proposal_counts, const int32_t* keys, int64_t ld_keys, float pos_iou_thr, float neg_lo,
                          float neg_hi, float min_pos_iou, int gt_max_assign_all, int match_low_quality, int add_gt_as_proposals,
                          int64_t num_expected_pos, int64_t num, double neg_pos_ub, int64_t num_classes, float pos_weight,
                          int reg_decoded_bbox, const float* means, const float* stds, float* rois, int64_t* labels,
                          float* label_weights, float* bbox_targets, float* bbox_weights, int64_t* pos_assigned_gt_inds,
                          int64_t* counts, uint8_t* pos_is_gt, float* pos_rois, int64_t* pos_gt_inds, int64_t* pos_labels,
                          void* stream);

/* BBoxHead.refine_bboxes + regress_by_class (bbox_heads/bbox_head.py:380-496) on the padded rows of one stage, one workgroup
 * per image.  Of image b the rows r < clamp(counts[2 b] + counts[2 b + 1], 0, num) are valid; rows beyond are NEVER READ.
 *   A valid row whose pos_is_gt is set is dropped.  Every other valid row is decoded with iif_delta2bbox's arithmetic from
 *   rois[row, 1:5] and the four deltas at bbox_preds[row, 4 label ..] (at 0 when reg_class_agnostic; a label outside
 *   [0, num_classes) reads nothing and decodes zero deltas), clipped to img_hw[b] = (h, w) (HOST array [B, 2]) when clip != 0.
 *   proposals [B, num, 4]: the kept boxes compacted in their original order, zero rows behind them; proposal_counts [B]: their
 *   number - the (proposals, proposal_counts) input of iif_roi_stage_targets.
 * Limits: 1 <= B <= 16, num <= 1024.  One launch, nothing allocated, nothing synchronises, no atomics. */
int iif_refine_bboxes(const float* rois, int64_t ld_rois, const int64_t* labels, const float* bbox_preds, int64_t ld_preds,
                      int num_classes, int reg_class_agnostic, const uint8_t* pos_is_gt, const int64_t* counts, int B, int64_t num,
                      const float* img_hw, const float* means, const float* stds, float max_ratio, int add_ctr_clamp,
                      float ctr_clamp, int clip, float* proposals, int64_t* proposal_counts, void* stream);

/* ---- The training side of the RPN head (csrc/rpn_stage.hip): anchors from a formula, batch targets without stored anchors, the
 * loss at the sampled anchors only - what AnchorGenerator (core/anchor/anchor_generator.py) and AnchorHead.get_anchors /
 * get_targets / loss (dense_heads/anchor_head.py:142-491) do.
 *
 * iif_rpn_grid: a HOST description of the anchor grid, copied into every launch.  Level l has H[l] x W[l] cells (both <= 65535),
 *   num_base[l] <= 16 base anchors base[l][a] = <x1, y1, x2, y2> and integer strides; at most 8 levels.  Flat anchor index
 *   i = start_l + (y W + x) num_base + a over the concatenated levels, A = sum of the levels < 2^31.  Anchor (l, y, x, a) is
 *   base[l][a] + (x stride_w, y stride_h, x stride_w, y stride_h): one float32 add per coordinate (x stride_w < 2^24). */
typedef struct iif_rpn_grid {
    int32_t num_levels;
    int32_t W[8], H[8], num_base[8], stride_w[8], stride_h[8];
    float base[8][16][4];
} iif_rpn_grid;
/* anchors [A, 4] float32 on a 16-byte boundary, all levels in one launch. */
int iif_grid_anchors(const iif_rpn_grid* grid, float* anchors, void* stream);
/* flags [A] uint8 (0 / 1): x < valid_wh[2 l] and y < valid_wh[2 l + 1] (HOST array [num_levels, 2]: the valid width and height
 * of each level in cells), all levels in one launch. */
int iif_grid_valid_flags(const iif_rpn_grid* grid, const int32_t* valid_wh, uint8_t* flags, void* stream);

/* Assign (iif_max_iou_assign's definition, no ignore boxes), sample (iif_random_sample's rule) and encode for all B images at
 * once; the anchors are generated from their index and never read.
 *   images: HOST array of B iif_roi_image (gt_bboxes, ld_gt, G; gt_labels and img_index are not read).  Any G.
 *   Candidate i of image b takes part only if its cell is valid - x < valid_wh[(b L + l) 2], y < valid_wh[(b L + l) 2 + 1]
 *   (HOST array [B, L, 2], each <= 65535) - and, when use_border, x1 >= border_lo, y1 >= border_lo, x2 < border_hi[2 b],
 *   y2 < border_hi[2 b + 1] (HOST array [B, 2]: img_w + border, img_h + border; border_lo = -border).  Every other candidate
 *   takes no part at all: not in a gt's maximum, not as a negative, not in the sampler.
 *   keys [B, A] int32: the key of flat anchor i of image b.
 *   pos_inds [B, num_expected_pos] / neg_inds [B, num]: flat indices, ascending, tails -1; counts [B, 2]; pos_assigned_gt_inds
 *   [B, num_expected_pos] (tail -1); pos_bbox_targets [B, num_expected_pos, 4] (iif_bbox2delta's arithmetic, tail 0);
 *   num_total_samples: one float32 = sum_b max(pos_b, 1) + max(neg_b, 1).
 *   d_workspace: iif_rpn_stage_workspace_bytes(B, A, sum of G) on a 16-byte boundary; it belongs to the call until the stream
 *   has run it.
 * Limits: 1 <= B <= 16, num <= 1024, 0 <= num_expected_pos <= num.  FIVE enqueued operations whatever the shapes and the data:
 * one clear of the head of the workspace, two assignment passes, the selection, the total.  Phases meet at launch boundaries;
 * integer atomics only: no result depends on arrival order. */
int64_t iif_rpn_stage_workspace_bytes(int B, int64_t A, int64_t total_G);
int iif_rpn_stage_targets(const iif_rpn_grid* grid, const iif_roi_image* images, int B, const int32_t* valid_wh, int use_border,
                          float border_lo, const float* border_hi, const int32_t* keys, float pos_iou_thr, float neg_lo,
                          float neg_hi, float min_pos_iou, int gt_max_assign_all, int match_low_quality, int64_t num_expected_pos,
                          int64_t num, double neg_pos_ub, const float* means, const float* stds, int64_t* pos_inds,
                          int64_t* neg_inds, int64_t* counts, int64_t* pos_assigned_gt_inds, float* pos_bbox_targets,
                          float* num_total_samples, void* d_workspace, int64_t workspace_bytes, void* stream);

/* The dense targets of AnchorHead.get_targets after images_to_levels from the lists above, one launch, every element written
 * once: each of labels (int64), label_weights, bbox_targets [.., 4], bbox_weights [.., 4] holds the levels one after the other,
 * level l as [B, A_l(, 4)] at element offset B start_l.  Positives: label 0, weight pos_weight (1 when <= 0), their targets,
 * box weights 1; negatives: label num_classes, weight 1; the rest: label num_classes, zeros. */
int iif_rpn_stage_dense(const iif_rpn_grid* grid, int B, const int64_t* pos_inds, const int64_t* neg_inds, const int64_t* counts,
                        const float* pos_bbox_targets, int64_t num_expected_pos, int64_t num, int64_t num_classes, float pos_weight,
                        int64_t* labels, float* label_weights, float* bbox_targets, float* bbox_weights, void* stream);

/* The RPN loss at the sampled anchors only.  levels: HOST array, one per level: the float32 score map [B, num_base, H, W] and
 * delta map [B, 4 num_base, H, W] with their element strides (any memory format; read in place at channel a / 4 a + j), and for
 * the backward the gradient maps with theirs.
 *   forward (one launch, one workgroup per level, fixed summation order): loss_cls[l] = cls_loss_weight / num_total_samples *
 *   sum over the level's sampled anchors of w BCE_with_logits(x, [positive]) (w = pos_weight on positives when > 0, else 1);
 *   loss_bbox[l] = bbox_loss_weight / num_total_samples * sum over its positives and the four deltas of |p - t| (beta <= 0) or
 *   SmoothL1(beta).  num_total_samples is read on the device.
 *   backward (one launch): plain stores at the sampled positions of gradient maps THE CALLER HAS CLEARED. */
typedef struct iif_rpn_loss_level {
    const float* scores;
    const float* deltas;
    float* grad_scores;
    float* grad_deltas;
    int64_t score_strides[4], delta_strides[4], grad_score_strides[4], grad_delta_strides[4];
} iif_rpn_loss_level;
int iif_rpn_loss_fwd(const iif_rpn_grid* grid, const iif_rpn_loss_level* levels, int B, const int64_t* pos_inds,
                     const int64_t* neg_inds, const int64_t* counts, const float* pos_bbox_targets, int64_t num_expected_pos,
                     int64_t num, const float* num_total_samples, float pos_weight, float cls_loss_weight, float bbox_loss_weight,
                     float beta, float* loss_cls, float* loss_bbox, void* stream);
int iif_rpn_loss_bwd(const iif_rpn_grid* grid, const iif_rpn_loss_level* levels, int B, const int64_t* pos_inds,
                     const int64_t* neg_inds, const int64_t* counts, const float* pos_bbox_targets, int64_t num_expected_pos,
                     int64_t num, const float* num_total_samples, float pos_weight, float cls_loss_weight, float bbox_loss_weight,
                     float beta, const float* grad_loss_cls, const float* grad_loss_bbox, void* stream);

/* ---- The RPN head's backward at the sampled pixels only (csrc/rpn_head_sampled.hip).  RPNHead.forward_single
 * (dense_heads/rpn_head.py:38-44) is relu(rpn_conv(x)) followed by the 1x1 convolutions rpn_cls and rpn_reg; the gradient that
 * iif_rpn_loss_bwd leaves in the maps is zero outside the pixels of the sampled anchors, so the three convolutions' backward is
 * formed from those pixels alone.
 *
 * iif_rpn_sampled_pixels: slot e of the B (num_expected_pos + num) entries of the lists above -> its pixel.
 *   owner [B, P] int32, P = sum_l H_l W_l, pixel (l, y, x) of image b at b P + sum_{l' < l} H_l' W_l' + y W_l + x: the lowest slot
 *   index whose anchor lies on the pixel (flat index -> pixel: (i - start_l) / num_base[l]), -1 where nothing was sampled.
 *   slots [B (num_expected_pos + num), 4] int32: <image, level, y, x> of a slot that owns its pixel, level -1 for every other slot
 *   (unused, or a second sampled anchor of a pixel).  THREE enqueued operations whatever the data: the clear of owner, an integer
 *   atomicMin per entry, the slot records. */
int iif_rpn_sampled_pixels(const iif_rpn_grid* grid, int B, const int64_t* pos_inds, const int64_t* neg_inds, const int64_t* counts,
                           const float* pos_bbox_targets, int64_t num_expected_pos, int64_t num, int32_t* owner, int32_t* slots,
                           void* stream);

/* One level of the head's backward: the float32 feature map [B, Ci, H, W] the head read, the gradient map of the same shape THE
 * CALLER HAS CLEARED (NULL on every level: the features' gradient is not wanted), and the gradients of the score map
 * [B, A, H, W] and delta map [B, 4 A, H, W]; each with its element strides (any memory format). */
typedef struct iif_rpn_head_level {
    const float* feat;
    float* grad_feat;
    const float* grad_scores;
    const float* grad_deltas;
    int64_t feat_strides[4], grad_feat_strides[4], grad_score_strides[4], grad_delta_strides[4];
} iif_rpn_head_level;

/* The gradients of rpn_conv [Co, Ci, 3, 3] (stride 1, pad 1; b_conv nullable), rpn_cls [A, Co] and rpn_reg [4 A, Co] and of the
 * features, from the `slots` records of iif_rpn_sampled_pixels.  CONTRACT: grad_scores / grad_deltas are zero outside the pixels
 * of the active slots (they are read nowhere else).
 *   d_w_conv [Co, Ci, 3, 3], d_b_conv [Co], d_w_cls [A, Co], d_b_cls [A], d_w_reg [4 A, Co], d_b_reg [4 A]: each nullable, every
 *   element written (a product none of whose results is wanted is not launched).  grad_feat: every pixel within the 3x3 neighbourhood of an active slot's pixel written once (all Ci
 *   channels); nothing else is touched.
 *   d_workspace: iif_rpn_head_sampled_workspace_bytes(slots, ci, co, A) on a 16-byte boundary (the patches, the hidden rows and
 *   their gradients, the per-range partials); it belongs to the call until the stream has run it.
 * Exact float32 products on v_mfma_f32_32x32x2_f32, fixed summation order (the slots in at most 16 ranges, partials added in range
 * order), no float atomics: the same bits from call to call.  NINE launches whatever the data (seven without grad_feat).
 * IIF_EINVAL before any launch: a required pointer NULL or misaligned, B outside 1 .. 16, slots < 1, ci or co < 1, a negative
 * stride, a workspace too small.  IIF_EUNSUPPORTED: ci or co not a multiple of 8 or above 2048, slots > 32768, levels with
 * different num_base, w_conv or d_workspace not 16-byte aligned. */
int64_t iif_rpn_head_sampled_workspace_bytes(int slots, int ci, int co, int num_base);
int iif_rpn_head_sampled_bwd(const iif_rpn_grid* grid, const iif_rpn_head_level* levels, int B, int slots_n, const int32_t* owner,
                             const int32_t* slots, const float* w_conv, const float* b_conv, const float* w_cls, const float* w_reg,
                             int ci, int co, float* d_w_conv, float* d_b_conv, float* d_w_cls, float* d_b_cls, float* d_w_reg,
                             float* d_b_reg, void* d_workspace, int64_t workspace_bytes, void* stream);

/* out = logits * table. Replaces classification/custom.py:37-39 (infer=True). */
int iif_scale_logits(const void* logits, int dtype, int64_t ld_logits, const float* table,
                     int B, int C, void* out, int64_t ld_out, void* stream);

/* out = softmax(logits * table, dim=-1), fp32 out.
 * Replaces mmdet/models/losses/iif_loss.py:65-78 (get_activation). */
int iif_softmax(const void* logits, int dtype, int64_t ld_logits, const float* table,
                int B, int C, float* out, int64_t ld_out, void* stream);

/* Top-k hit counts.  hits[j] += #rows whose target ranks < k[j] in
 * logits*table (table NULL = raw logits); rank = #greater + #equal-with-lower-index.
 * Replaces classification/utils.py:165-179 and mmdet/models/losses/accuracy.py:7-51
 * (callers turn counts into percent).  hits: int32[nk], zeroed by the caller;
 * integer atomics => exact and order independent.  nk <= 4. */
int iif_topk_hits(const void* logits, int dtype, int64_t ld_logits, const float* table,
                  const int64_t* targets, int B, int C, const int32_t* k_host, int nk,
                  int32_t* hits, void* stream);

/* Evaluation statistics of logits*table (table NULL = raw logits), accumulated into acc (int64, device,
 * zeroed by the caller, layout below).  One read of each row.  Integer atomics only => exact and
 * independent of launch order, batch split and rank count.  nk <= 4; 1 <= nb <= 256.
 * bin_edges: device float64[nb+1], ascending (the caller passes np.linspace(0, 1, nb+1)).
 * pred_out (int64[B]) and conf_out (float[B]) are optional per-row outputs.
 * acc = [rows | out_of_range | hits_k[nk] | n_test[C] | n_hit[C] | bin_count[nb] | bin_hit[nb] | bin_conf[nb]]:
 * rank of the target as iif_topk_hits; prediction = first index of the maximum (torch.argmax); confidence = the
 * softmax maximum; bin b holds edges[b] < conf <= edges[b+1] (np.digitize(..., right=True)); bin_conf sums
 * llrint(conf * 2^32).  A target outside [0, C) counts in rows, out_of_range and the bins (as a miss) only. */
int iif_eval_accumulate(const void* logits, int dtype, int64_t ld_logits, const float* table,
                        const int64_t* targets, int B, int C, const int32_t* k_host, int nk,
                        const double* bin_edges, int nb, int64_t* acc,
                        int64_t* pred_out, float* conf_out, void* stream);

/* out[i] = x[i] * *d_scalar (device scalar; out may alias x).  Used by the autograd
 * bridge to apply the upstream gradient of the scalar loss without a host sync. */
int iif_scale_by_device_scalar(const void* x, int dtype, int64_t n, const float* d_scalar, void* out, void* stream);

/* ------------------------------------------------------------- Seesaw head (LVIS) */

/* Fused Seesaw loss, forward + gradient.  Replaces mmdet/models/losses/seesaw_loss.py:12-76,199-262
 * (SeesawLoss.forward: the host loop over labels.unique(), the [C, C] ratio matrix, two softmaxes, pow, log,
 * cross entropy on the positive rows and the objectness cross entropy) by TWO launches and no host round trip.
 *
 * cls_score: [N, C + 2] fp32, leading dimension ld_score >= C + 2 (elements), element-aligned: C class columns z
 * and two objectness columns o.  labels: int64[N] in [0, C], C = background.  label_weights: float[N] or NULL.
 *
 *   launch 1   cum_samples[l] += (float)count(labels == l) when update_counts != 0: an integer histogram, ONE fp32
 *              addition per class (exact and order independent, also above 2^24); the number of positive rows
 *   launch 2   with the UPDATED cum_samples[:C], for a positive row (t = label < C), in the log domain:
 *                a_j = min(0, p * (log max(cum_j, 1) - log max(cum_t, 1)))                          (p > 0)
 *                b_j = max(0, q * (z_j - lse(z) - max(z_t - lse(z), log eps)))                      (q > 0)
 *                z'_j = z_j + a_j + b_j (j != t), z'_t = z_t
 *                class loss_i = w_i * (lse(z') - z_t),  d z = scale_cls' * w_i * (softmax(z') - onehot_t)
 *              background rows: class loss 0 and a zero class gradient.  Every row: objectness loss_i =
 *              w_i * (lse(o) - o[label == C]), gradient scale_obj * w_i * (softmax(o) - onehot) in the last two columns.
 *   loss_out[0] = scale_cls' * sum class loss_i,  loss_out[1] = scale_obj * sum objectness loss_i,
 *   scale_cls' = scale_cls / (positive rows) when div_by_pos != 0 (reduction 'mean' without avg_factor; no positive
 *   row: loss 0, gradient 0), else scale_cls.
 *
 * cum_samples: float[C + 1], state, updated in place.  loss_rows_cls / loss_rows_obj: float[N], required (the
 * unscaled loss_i).  loss_out: float[2].  dscore: [N, C + 2] fp32 with ld_dscore, or NULL (losses only); every
 * element of a row is written.  A label outside [0, C] counts nowhere, zeroes its row (losses and gradient) and sets
 * d_status (int32[1] or NULL) to 1, as iif_ce_fwd_bwd does.
 * d_workspace: IIF_SEESAW_WORKSPACE_BYTES of device memory, ZERO on first use; the kernels leave its tickets and
 * histogram zero again.  One workspace per stream.  Deterministic (integer atomics, fixed-order float sums).
 * dtype must be IIF_F32 (IIF_EINVAL otherwise); C + 2 > 2048 is IIF_EUNSUPPORTED (the row is register resident).
 * N == 0 writes two zero losses without a launch and leaves cum_samples alone. */
int iif_seesaw_fwd_bwd(const void* cls_score, int dtype, int64_t ld_score, const int64_t* labels,
                       const float* label_weights, float* cum_samples, int update_counts,
                       float p, float q, float eps, float scale_cls, int div_by_pos, float scale_obj,
                       int N, int C, float* loss_rows_cls, float* loss_rows_obj, float* loss_out,
                       void* dscore, int64_t ld_dscore, int32_t* d_status, void* d_workspace, void* stream);
#define IIF_SEESAW_WORKSPACE_BYTES (4 * (4 + 2048 + 2 * 1024))

/* iif_seesaw_fwd_bwd as the classification half of BBoxHead.loss (bbox_head.py:266-283 with SeesawLoss.forward and
 * SeesawLoss.get_accuracy, seesaw_loss.py:177-262) with NO host read: avg_factor = max(#{label_weights > 0}, 1) is counted on
 * the device and both accuracies leave the loss launch.  TWO launches.  cls_score [N, C + 2] fp32 (IIF_F32 only), C + 2 <= 2048,
 * N <= IIF_HEAD_LOSS_MAX_ROWS, pitch ld_score >= C + 2; labels, label_weights (NULL = ones), cum_samples, p, q, eps as above.
 *   launch 1   the histogram over the rows with w_i != 0 and a label in [0, C], added to cum_samples as one fp32 addition per
 *              class; V = #{w_i > 0} and P = #{w_i > 0, label_i < C}, as integers
 *   launch 2   the row arithmetic of iif_seesaw_fwd_bwd with the updated cum_samples; avg = max(V, 1)
 *   loss_out[0] = loss_weight * (sum class loss_i) / avg       an exact 0 without a positive row
 *   loss_out[1] = loss_weight * (sum objectness loss_i) / avg
 *   loss_out[2] = loss_out[0] + loss_out[1]                     (return_dict=False)
 *   acc_out[0]  = float(objectness hits over w_i > 0) * float(100 / avg)          0 when V == 0
 *   acc_out[1]  = float(class hits over the positive rows with w_i > 0) * float(100 / P)          0 when P == 0
 *   avg_out     = avg
 *   dscore      = w_i * (softmax(z') - onehot_t | softmax(o) - onehot) at UNIT scale: iif_seesaw_fwd_bwd's at scale_cls =
 *                 scale_obj = 1, div_by_pos = 0, bit for bit; iif_seesaw_head_bwd applies the rest
 * A row with w_i == 0 is NOT READ, its label included: its dscore row is zeros and it enters neither the losses, V, the
 * accuracies nor cum_samples (the padded rows of iif_roi_stage_targets; the reference counts every one of them into
 * cum_samples[C]).  A row with w_i < 0 enters the losses and the histogram but not V or the accuracies.  A label outside [0, C]
 * of a row with w_i != 0 zeroes the row, is not counted in the histogram, is never a hit and sets d_status, as above.
 * loss_out float[3], acc_out float[2], avg_out float[1]: DEVICE memory, all required.  dscore [N, C + 2] or NULL.
 * d_workspace: IIF_SEESAW_HEAD_WORKSPACE_BYTES, ZERO on first use; its tickets, histogram and accumulators are zero again on
 * exit.  One per stream.  Integer counts, float sums in an order fixed by N: the same bits from call to call.
 * N == 0 writes losses 0, accuracies 0, avg 1 (two launches) and leaves cum_samples alone.
 * Before anything is launched: IIF_EINVAL for N outside 0 .. IIF_HEAD_LOSS_MAX_ROWS, C < 1, a dtype other than IIF_F32, p or q
 * negative, eps <= 0 with q > 0, a null or misaligned output / cum_samples / workspace / cls_score / labels, a pitch smaller
 * than C + 2; IIF_EUNSUPPORTED for C + 2 > 2048. */
#define IIF_SEESAW_HEAD_WORKSPACE_BYTES (4 * (4 + 2048 + 4 + 4 * 1024))
int iif_seesaw_head_fwd(const void* cls_score, int dtype, int64_t ld_score, const int64_t* labels, const float* label_weights,
                        float* cum_samples, float p, float q, float eps, float loss_weight, int N, int C, void* dscore,
                        int64_t ld_dscore, float* loss_out, float* acc_out, float* avg_out, int32_t* d_status, void* d_workspace,
                        void* stream);

/* Backward of iif_seesaw_head_fwd in ONE launch: out = dscore * (*d_g_cls * loss_weight / *d_avg) on the C class columns and
 * dscore * (*d_g_obj * loss_weight / *d_avg) on the two objectness columns.  d_g_cls / d_g_obj (the gradients of loss_out[0] /
 * loss_out[1]; the same pointer twice for loss_out[2]) and d_avg (avg_out) are DEVICE floats; dscore is left intact (backward
 * may run twice).  N == 0 is a no-op.  IIF_EINVAL: N < 0, C < 1, a null or misaligned pointer, a pitch smaller than C + 2. */
int iif_seesaw_head_bwd(const float* dscore, int64_t ld_dscore, int N, int C, const float* d_g_cls, const float* d_g_obj,
                        const float* d_avg, float loss_weight, float* out, int64_t ld_out, void* stream);

/* out[:, :C] = softmax(z) * softmax(o)[0], out[:, C] = softmax(o)[1]; out: [N, C + 1] fp32 with ld_out >= C + 1.
 * Replaces seesaw_loss.py:157-175 (get_activation).  One launch.  fp32 only, C + 2 <= 2048. */
int iif_seesaw_activation(const void* cls_score, int dtype, int64_t ld_score, int N, int C,
                          float* out, int64_t ld_out, void* stream);

/* out[0] = objectness top-1 accuracy over all rows, out[1] = class top-1 accuracy over the positive rows, in percent
 * (seesaw_loss.py:177-197 + accuracy.py:7-51: float32 hit count times float32(100 / rows); 0 when there is no
 * positive row, and both 0 for N == 0).  Integer counts and the division on the device, one launch; rank rule of
 * iif_topk_hits.  d_workspace: int32[4], zero on first use and left zero.  A label outside [0, C] is no positive row. */
int iif_seesaw_accuracy(const void* cls_score, int dtype, int64_t ld_score, const int64_t* labels, int N, int C,
                        float* out, int32_t* d_workspace, void* stream);

/* Backward of the two Seesaw losses: out = dscore * g_cls on the C class columns and dscore * g_obj on the two
 * objectness columns.  g_cls / g_obj: device float[1] (per_row == 0) or float[N] (per_row != 0, reduction 'none').
 * out may alias dscore. */
int iif_seesaw_scale_grad(const float* dscore, int64_t ld_dscore, int N, int C, const float* g_cls, const float* g_obj,
                          int per_row, float* out, int64_t ld_out, void* stream);

/* out[b,:] = lam*x[b,:] + (1-lam)*x[perm[b],:], rows of n elements.
 * Replaces the image blend of classification/custom.py:112 (Mixup.__call__). */
int iif_mix_rows(const void* x, int dtype, const int64_t* perm, float lam, int B, int64_t n,
                 void* out, void* stream);

/* ------------------------------------------------------- ResNet forward/backward */

/* Geometry of one convolution-shaped contraction (all tensors NHWC).
 * "source" is what the taps gather from, "destination" is the output grid. */
typedef struct iif_conv_desc {
    int32_t n, hs, ws, cs;   /* source      [n, hs, ws, cs]                       */
    int32_t hd, wd, cd;      /* destination [n, hd, wd, cd]                       */
    int32_t r, s;            /* taps                                               */
    int32_t stride, pad;     /* of the FORWARD convolution (stride 1 or 2)         */
    int32_t transposed;      /* 0: ys = y*stride - pad + r   (forward)             */
                             /* 1: ys = (y + pad - r)/stride (data gradient)       */
    int32_t ldw;             /* weight row pitch in elements (>= r*s*cs, 16-B mult) */
    int32_t dtype;           /* IIF_F32 / IIF_BF16 of src and wgt                  */
    int32_t dst_dtype;       /* dtype of dst / res: == dtype, or IIF_F32           */
    int32_t groups;          /* 0/1: dense.  G > 1: cs / cd are PER-GROUP widths, the   */
                             /* tensors hold G*cs / G*cd channels per pixel, wgt is G   */
                             /* consecutive [cd][ldw] matrices (grouped convolution,    */
                             /* resnet_pytorch.py:137,141 ResNeXt)                      */
    const void* wgt_frag;    /* nullable: the SAME weights as MFMA fragments            */
                             /* (iif_conv_pack_fragments); used by the 3x3 / stride-1   */
                             /* kernel where iif_conv3x3_frag_ok(d) says so, ignored    */
                             /* elsewhere.  wgt must be valid either way.               */
    int32_t wgt_frag_kind;   /* 0: iif_conv_pack_fragments' format.  1 (round 6): the  */
                             /* grouped 16-channel format of iif_conv_pack_fragments_g16 */
                             /* (groups > 1, cs = cd = 64, every group <= 16 channels). */
} iif_conv_desc;

/* Implicit-GEMM convolution on the matrix cores:
 *   dst[m, k] = sum_{r,s,c} gather(src)[m; r,s,c] * wgt[k][r][s][c]  (+ bias[k]) (+ res[m, k])
 * wgt: [cd][ldw] rows of r*s*cs K-contiguous elements.  With transposed=0 and
 * KRSC weights this is conv2d forward (resnet_pytorch.py:46-62 conv3x3/conv1x1,
 * resnet_cifar.py:112-115); with transposed=1 and [cin][R][S][cout] weights it is
 * the data gradient; r=s=1 on a [B,1,1,C] tensor is the fully connected layer
 * (resnet_pytorch.py:219, resnet_cifar.py:192) with `bias`.  res (nullable, same
 * shape/dtype as dst, may alias dst) is added in the epilogue: gradient
 * accumulation at residual joins.  bf16 inputs multiply on v_mfma_f32_16x16x32_bf16
 * with fp32 accumulation; f32 inputs on v_mfma_f32_16x16x4_f32 (exact fp32). */
int iif_conv_igemm(const iif_conv_desc* d, const void* src, const void* wgt, void* dst,
                   const void* res, const float* bias, void* stream);

/* iif_conv_igemm that also emits batch-norm statistics of its (bf16) output from the
 * epilogue: bn_partial[t][0][k] / [t][1][k] = sum / sum of squares of the stored output
 * over pixel tile t (128 consecutive pixels) for channel k; *n_partials (host int,
 * nullable) receives the tile count.  Feed them to iif_bn_finalize_stats: no separate
 * pass over the activation.  bf16 in/out, cd % 8 == 0, no bias/res; otherwise
 * IIF_EUNSUPPORTED.  bn_partial must hold >= ceil(m/128)*2*cd floats. */
int iif_conv_igemm_bnstats(const iif_conv_desc* d, const void* src, const void* wgt, void* dst,
                           const void* res, const float* bias, float* bn_partial,
                           int64_t bn_partial_floats, int32_t* n_partials, void* stream);

/* Weight gradient: dw[k][r][s][c] = sum_m dy[m, k] * gather(x)[m; r,s,c], fp32 out.
 * d describes the FORWARD convolution (source = x, destination = dy grid,
 * transposed must be 0).  dw: float [cd][ldw] (columns >= r*s*cs are not
 * written).  The pixel reduction is split over `splits` workgroup rows
 * (0 = choose: one co-resident round of workgroups on the whole device; -n =
 * choose for 1/n of the device, for a caller that runs n weight gradients side
 * by side on n streams - every workgroup writes its accumulator tile once, so
 * n half-size rounds write 1/n of the slab bytes each) into fp32 slabs in
 * `workspace` (>= splits*cd*ldw*4 bytes; fewer
 * splits are used if it is smaller, NULL = no split) that are then summed in
 * fixed order: deterministic, no float atomics.  bf16 fragments are formed by
 * ds_read_b64_tr_b16.  Replaces the wgrad half of autograd's conv backward for
 * resnet_pytorch.py:46-62 / resnet_cifar.py:112-115 and the fc layer. */
int iif_conv_wgrad(const iif_conv_desc* d, const void* x, const void* dy, float* dw,
                   void* workspace, int64_t workspace_bytes, int splits, void* stream);

/* 1x1 weight gradient against TWO gradient tensors stacked along the channels, one pass over x (bf16):
 *   out[k][:] = sum_m dy[m][k] x[m][:] for k < cd1,   out[cd1 + j][:] = sum_m dy2[m][j] x[m][:] for j < cd2;
 * out float [cd1 + cd2][ldw], split-K slabs and `splits` as iif_conv_wgrad.  The BN-by-algebra backward
 * (iif_bn3_algebra_*) takes P = g~^T a2 and the Gram matrix a2^T a2 from one launch this way (dy = g~, dy2 = x = a2).
 * cd1 % 128 == 0, cs % 8 == 0, cd2 % 8 == 0; otherwise IIF_EUNSUPPORTED. */
int iif_wgrad1x1_stacked(const void* x, const void* dy, const void* dy2, int64_t m, int cs, int cd1, int cd2,
                         int ldw, float* out, void* workspace, int64_t workspace_bytes, int splits,
                         void* stream);

/* The split-K decision of a weight-gradient launch as a value: what iif_conv_wgrad(d, ..., workspace_bytes, splits) would
 * launch, decided on the host, nothing launched, no device needed.  cd2 = 0: iif_conv_wgrad; cd2 = -1: the same with x and dy
 * one tensor (the Gram matrix; cs == cd); cd2 > 0: iif_wgrad1x1_stacked with d its 1x1 descriptor (n * hd * wd = m, cd = cd1).
 * workspace_bytes = 0 stands for no workspace.  The argument checks are the entry's own (operand pointers aside).
 *
 * The rule.  With groups = max(d->groups, 1), K = r * s * cs, M = n * hd * wd, and unless IIF_CONV_REGSTAGE is set or an operand
 * (n * hs * ws * groups * cs, or M * groups * cd, elements) reaches 0x7ffffff0 bytes - then every launch is REGSTAGE - bf16 takes
 *   NINETAP  3 x 3 / stride 1 / pad 1 with hs x ws = hd x wd, wd <= 61, dense channels in 64s or grouped 64 -> 64 chunks with
 *            ldw >= 576; tiles = (cs / 64) * (cd / 64) (grouped: groups) of 64 x 64; steps of 32 PADDED pixels,
 *            nsteps = ceil(n * (hd + 2) * (wd + 2) / 32); 2 blocks per CU;
 *   STEM     4 x 4 / stride 1 / pad 2, dense 16 -> 64 with hs x ws = hd x wd and a window that fits the ring:
 *            ceil((2 * (wd + 3) + 2) / 32) + floor((wd + 35) / 32) <= 12; one 64 x 256 tile, nsteps = ceil(n * (hd + 3) * (wd + 3) / 32);
 *            2 blocks per CU;
 *   1X1      1 x 1 / stride 1 / pad 0, dense: output-channel tile 256 (cd a multiple of 256; stacked: cd1 is), 64 (cd <= 64; never
 *            stacked) or 128; input-column tile 64 (64-channel tile and cs <= 64), 256 (64-channel tile, cs a multiple of 256;
 *            not under IIF_WGRAD_NO_64X256) or 128; tiles = ceil(cd_total / bc) * ceil(cs / bnw); nsteps = ceil(M / 32);
 *            blocks per CU: 1 (256), 3 (128), 2 (64 x 256), 4;
 * and everything else, fp32 included, takes
 *   DMA / REGSTAGE  output-channel tile 256 (DMA, bf16, dense, cd a multiple of 256), 64 (cd <= 64) or 128, by 128 of the K columns;
 *            tiles = ceil(cd / bc) * ceil(K / 128) PER GROUP; nsteps = ceil(M / 32) (fp32: 16); blocks per CU: 1, 4, 3.
 *            (REGSTAGE has no grouped form: IIF_EUNSUPPORTED.)
 * A NINETAP / STEM shape with more than 0x7fff0000 padded pixels falls through to the families below it.
 * splits > 0 is the request.  splits <= 0 asks for one co-resident round of 1 / max(1, -splits) of the device:
 *   256 * blocks_per_cu / share / (tiles * groups), at least 1 and at most max(1, nsteps / 8) (integer divisions, left to right;
 *   the NINETAP tile count already counts the groups, the STEM has no lower clamp to apply);
 *   NINETAP divides that by IIF_WGRAD_HALO_DIV (1), grouped by IIF_WGRAD_HALO_GROUPED_DIV (4), before the two clamps;
 *   1X1, after the clamps and if more than 8 are left, divides by IIF_WGRAD_GRAM_DIV (8) for the Gram matrix, else by
 *   IIF_WGRAD_SMALL_DIV (2) for a slab of at most IIF_WGRAD_SMALL_KB (256) KiB, else by IIF_WGRAD_MID_DIV (2) for one of at most
 *   4 MiB - but never to fewer than 8.  (These switches are read once per process.)
 * Then, with slab = groups * cd_total * ldw floats: at most workspace_bytes / (slab * 4) splits, at least 1, at most nsteps and
 * 65 535; steps_per_split = ceil(nsteps / splits), and the realised count is ceil(nsteps / steps_per_split): the last split may
 * be shorter, none is empty.  One split writes dw itself.  The grid is padded to tiles * (splits rounded up to 8) blocks, DMA: times
 * groups (REGSTAGE: tiles x splits, unpadded); the padding blocks write nothing.
 * More than one split: the slabs are summed in slab order by one pass, or - splits > 32, ceil(slab / 1024) < 256 (a slab under
 * about 1 MiB) and (splits + chunks) * slab * 4 <= workspace_bytes with chunks = ceil(splits / 16) - in two stages: chunk c of 16
 * consecutive slabs into slab c of a stage area BEHIND the splits slabs, then the chunk sums in order.
 *
 * out[10] = { family, output-channel tile, input-column tile, tiles (as counted above), nsteps, realised splits, steps_per_split,
 *             blocks launched, reduction stages (0: one split, 1, 2), chunks of the first stage (0 unless 2 stages) }. */
#define IIF_WGRAD_REGSTAGE 0
#define IIF_WGRAD_DMA 1
#define IIF_WGRAD_1X1 2
#define IIF_WGRAD_NINETAP 3
#define IIF_WGRAD_STEM 4
int iif_conv_wgrad_plan(const iif_conv_desc* d, int cd2, int64_t workspace_bytes, int splits, int32_t* out);

/* Training-mode batch norm, NHWC activation viewed as x[m, c] (m = N*H*W).
 * Replaces F.batch_norm(training=True) + ReLU + residual add and their autograd
 * backward under resnet_pytorch.py:152-167 / resnet_cifar.py:133-138.
 *
 * forward_stats: batch mean / biased variance per channel (fixed-order partial
 *   sums, fp64 finalisation), running stats updated in place with `momentum`
 *   (unbiased variance, as torch), and `stats` = float[4*c]:
 *   mean | invstd | a = gamma*invstd | b = beta - mean*a.
 * apply: y = act(a*x + b + R) with R = 0, `residual`, or a2*residual + b2 when
 *   residual_stats (another BN's stats block) is given; act = ReLU if relu.
 * backward: given gy = dL/dy (y = the activated output), y_mask (the stored
 *   activated output; NULL = no ReLU), the BN input x and `stats`:
 *   dy = gy*[y_mask>0]; dgamma = sum dy*xhat; dbeta = sum dy;
 *   dx = gamma*invstd*(dy - mean(dy) - xhat*mean(dy*xhat)).
 *   gmasked (nullable, may alias gy) receives dy — the gradient that also flows
 *   into the residual branch.  dx may alias gy when gmasked is NULL.
 * relu_bits (apply: nullable output, backward: nullable input that replaces y_mask): one byte per
 *   16-byte channel vector (8 bf16 / 4 f32 channels), bit k = [pre-activation k > 0] — the backward
 *   passes then read 1/16 of the mask bytes.  m*c/8 (bf16) or m*c/4 (f32) bytes.
 * workspace: iif_bn_workspace_bytes(m, c) bytes. */
int64_t iif_bn_workspace_bytes(int64_t m, int c);
int iif_bn_forward_stats(const void* x, int dtype, int64_t m, int c, const float* gamma,
                         const float* beta, float eps, float momentum, float* running_mean,
                         float* running_var, float* stats, void* workspace,
                         int64_t workspace_bytes, void* stream);
int iif_bn_apply(const void* x, int dtype, int64_t m, int c, const float* stats,
                 const void* residual, const float* residual_stats, int relu, void* y,
                 uint8_t* relu_bits, void* stream);
/* Inference-mode BN of every layer of a network in ONE launch: for each table entry (a device array of n_layers
 * descriptors) the `stats` rows iif_bn_apply reads are written from the affine parameters and the running statistics,
 * (mean, invstd = rsqrt(running_var + eps), a = gamma * invstd, b = beta - mean * a), each operation rounded on its own -
 * bit for bit the [C]-vector arithmetic torch does for model.eval().  Runs once per evaluation forward: nothing is cached,
 * so a write to running_mean needs no invalidation. */
typedef struct iif_bn_fold_desc {
    const float* gamma; const float* beta; const float* running_mean; const float* running_var;
    float* stats;          /* [4][c] */
    int32_t c, reserved;
} iif_bn_fold_desc;
int iif_bn_fold(const iif_bn_fold_desc* table, int n_layers, float eps, void* stream);
/* second half of iif_bn_forward_stats on externally produced partial sums
 * (partial[t][0][k] = sum, [t][1][k] = sum of squares; fixed-order fp64 reduction).
 * scratch (nullable, >= 128*c floats) lets > 512 partial rows be reduced in two
 * parallel stages instead of one serial walk. */
int iif_bn_finalize_stats(const float* partial, int n_partials, int64_t m, int c, const float* gamma,
                          const float* beta, float eps, float momentum, float* running_mean,
                          float* running_var, float* stats, float* scratch, int64_t scratch_floats,
                          void* stream);
/* iif_bn_finalize_stats with both reduction stages in ONE launch when there are > 512 partial rows: the 64 slice sums
 * are published with agent-scope atomics and the last block of every 32-channel group (a ticket per group) finishes
 * the statistics.  tickets: int32[64], ZERO on entry (zero it once; the kernel leaves it zero), not shared by calls
 * that can run concurrently; NULL = the two-launch path.  Same arithmetic (fixed-order fp64 sums). */
int iif_bn_finalize_stats_fused(const float* partial, int n_partials, int64_t m, int c, const float* gamma,
                                const float* beta, float eps, float momentum, float* running_mean,
                                float* running_var, float* stats, float* scratch, int64_t scratch_floats,
                                int32_t* tickets, void* stream);
/* Round 6: iif_bn_finalize_stats_fused plus a second, independent job in the same launch: sums2[2][c2] = column sums of the partial
 * rows partial2 [n_partials2][2][c2] (iif_bn_partial_sums' result) - the column sums of a2 that conv3's prologue emits
 * (iif_conv_igemm_bnstats_pro's act_csum) are reduced by the finalisation that follows that launch anyway. */
int iif_bn_finalize_stats_sums(const float* partial, int n_partials, int64_t m, int c, const float* gamma, const float* beta,
                               float eps, float momentum, float* running_mean, float* running_var, float* stats,
                               float* scratch, int64_t scratch_floats, int32_t* tickets, const float* partial2, int n_partials2,
                               int c2, float* sums2, void* stream);
int iif_bn_backward(const void* gy, const void* y_mask, const uint8_t* relu_bits, const void* x,
                    int dtype, int64_t m, int c, const float* stats, const float* gamma, float* dgamma,
                    float* dbeta, void* dx, void* gmasked, void* workspace, int64_t workspace_bytes,
                    void* stream);

/* Max pooling k x k / stride / pad on NHWC (resnet_pytorch.py:206 MaxPool2d(3,2,1)).
 * argmax: uint8 per output element = kh*k + kw of the first maximum in scan
 * order (torch's tie rule); backward routes gy to that input position. */
int iif_maxpool_forward(const void* x, int dtype, int n, int h, int w, int c, int k, int stride,
                        int pad, void* y, uint8_t* argmax, void* stream);
int iif_maxpool_backward(const void* gy, const uint8_t* argmax, int dtype, int n, int h, int w, int c,
                         int k, int stride, int pad, void* dx, void* stream);

/* Global average pooling over hw pixels (resnet_pytorch.py:211 AdaptiveAvgPool2d(1),
 * resnet_cifar.py:209 avg_pool2d). */
int iif_avgpool_forward(const void* x, int dtype, int n, int hw, int c, void* y, void* stream);
int iif_avgpool_backward(const void* gy, int dtype, int n, int hw, int c, void* dx, void* stream);

/* Stem patches: NCHW fp32 image -> [n*ho*wo][kp] matrix, column (r*S+s)*cin + c,
 * zero padded to kp, so the few-channel first convolution (resnet_pytorch.py:203
 * 7x7/2, resnet_cifar.py:179 3x3) runs as a K-contiguous MFMA GEMM. */
int iif_im2col_nchw(const float* img, int n, int cin, int h, int w, int r, int s, int stride, int pad,
                    int kp, int out_dtype, void* out, void* stream);

/* Element-wise precision cast (f32 -> bf16 | f32, bf16 -> f32). */
int iif_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);

/* fp32 master weights [cout][ldw] (r,s,cin order) -> [cin][ldwt] (r,s,cout order) in
 * out_dtype: the operand layout of the data-gradient contraction. */
int iif_weight_transpose(const float* w, int cout, int cin, int rs, int ldw, int ldwt, int out_dtype,
                         void* wt, void* stream);

/* Option-A shortcut of the CIFAR ResNet (resnet_cifar.py:125-126):
 * y[n,y,x,c] = x[n,2y,2x,c-(cout-cin)/2] inside the channel band, else 0;
 * backward_acc adds g back into dx at the even pixels. */
int iif_shortcut_a_forward(const void* x, int dtype, int n, int h, int w, int cin, int cout, void* y,
                           void* stream);
int iif_shortcut_a_backward_acc(const void* g, int dtype, int n, int h, int w, int cin, int cout,
                                void* dx, void* stream);

/* out[c] = sum_r a[r*ld + c] (bias gradient of the fc layer). */
int iif_colsum_f32(const float* a, int rows, int cols, int64_t ld, float* out, void* stream);

/* One fused SGD update over a flat fp32 arena (all parameters of the model in
 * one launch).  torch.optim.SGD semantics as used at classification/train.py:199-204
 * (dampening 0; a zero-initialised momentum buffer reproduces buf = grad on the
 * first step): d = grad_scale*g + wd*p; buf = m*buf + d;
 * p -= lr*(nesterov ? d + m*buf : buf).  d_lr (nullable) overrides lr with a
 * device scalar so a captured graph can follow the schedule. */
int iif_sgd_step(float* params, const float* grads, float* momentum_buf, int64_t n, float lr,
                 const float* d_lr, float momentum, float weight_decay, int nesterov,
                 float grad_scale, void* stream);
/* Planning query of the streaming kernels: the launch decisions that depend only on the SIZE of the tensor, answered by the
 * functions the launches themselves call (a host function; it touches no operand and launches nothing).  `work` is the number of
 * work items as the entry counts them:
 *   IIF_PLAN_BN_STREAM      16-byte vectors m * c / V of iif_bn_apply and of the normalisation pass of every iif_bn_backward*
 *                           entry; follows IIF_BN_GRID_CAP / IIF_BN_UNROLL / IIF_BN_NT_STORES as the process read them;
 *   IIF_PLAN_GRID_STRIDE    the grid-stride kernels of the pooling / cast / shortcut / im2col / transpose entries: output vectors
 *                           (pools, im2col), elements (casts, shortcut, transpose), n / 4 + 1 for iif_sgd_step;
 *   IIF_PLAN_RMSPROP        n / 4 + 1 for iif_rmsprop_step;
 *   IIF_PLAN_SE_STREAM      vectors n * hw * c / V of iif_se_apply and iif_se_backward_form;
 *   IIF_PLAN_STEM_POOL_ROWS pooled rows n * ho of iif_maxpool_bn_forward (3 x 3 / 2 / 1 with 256 % (c / V) == 0);
 *   IIF_PLAN_POOL_FUSED     image rows n * h of iif_bn_backward_pool_fused, with w and cv = c / V (unused by the others).
 * out[4] = { blocks, vectors per thread and trip (U), non-temporal stores (0 / 1), trips of the grid-stride loop } and for
 * IIF_PLAN_POOL_FUSED { row groups = blocks, image rows per block, XCD remap (0 / 1), rows of the last group }.
 * For tests: a case asks on which side of a threshold it lies instead of repeating the arithmetic. */
#define IIF_PLAN_BN_STREAM 0
#define IIF_PLAN_GRID_STRIDE 1
#define IIF_PLAN_RMSPROP 2
#define IIF_PLAN_SE_STREAM 3
#define IIF_PLAN_STEM_POOL_ROWS 4
#define IIF_PLAN_POOL_FUSED 5
int iif_stream_plan(int family, int64_t work, int w, int cv, int32_t* out);

/* One fused RMSprop update over a flat fp32 arena.  torch.optim.RMSprop
 * semantics as used at classification/train.py:205-207 (eps 0.0316, alpha 0.9;
 * zero-initialised state reproduces torch's lazy initialisation):
 * g = grad_scale*grad + wd*p; sq = alpha*sq + (1-alpha)*g*g;
 * avg = sqrt(sq - ga*ga) + eps with ga = lerp(ga, g, 1-alpha) if centered, else
 * sqrt(sq) + eps; momentum > 0: buf = m*buf + g/avg, p -= lr*buf; else
 * p -= lr*g/avg.  momentum_buf is read only when momentum > 0 and grad_avg only
 * when centered (NULL otherwise).  d_lr (nullable) overrides lr with a device
 * scalar.  IIF_EINVAL: n < 0, a required pointer NULL, or lr / eps / alpha /
 * momentum / weight_decay negative or not finite (checked before n == 0, which
 * is IIF_OK); IIF_EUNSUPPORTED: an arena pointer not 16-byte aligned. */
int iif_rmsprop_step(float* params, const float* grads, float* square_avg,
                     float* momentum_buf, float* grad_avg,
                     int64_t n, float lr, const float* d_lr, float alpha, float eps,
                     float weight_decay, float momentum, int centered,
                     float grad_scale, void* stream);

/* Cosine / normed classifier heads (resnet_cifar.py:38-78 CosNorm_Classifier,
 * NormedLinear; mmdet normed_predictor.py).  Row maps and their backward; the
 * products run on iif_conv_igemm / iif_conv_wgrad.
 *   mode 0: out = x * scale/(1+|x|)           (cosine feature squashing)
 *   mode 1: out = x / max(|x|, eps)           (F.normalize; zero rows stay zero)
 * norms (nullable in forward) receives |x| per row, fp32.
 * backward: dx = d(out)/dx^T g given the forward input x and its stored norms. */
int iif_rowmap_forward(const void* x, int x_dtype, int rows, int cols, int64_t ldx, int mode,
                       float scale, float eps, void* out, int out_dtype, int64_t ldo, float* norms,
                       void* stream);
int iif_rowmap_backward(const void* x, int x_dtype, const float* norms, const void* g, int g_dtype,
                        int rows, int cols, int64_t ldx, int64_t ldg, int mode, float scale, float eps,
                        void* dx, int dx_dtype, int64_t lddx, void* stream);
/* out[c][r] = in[r][c] (fp32); NormedLinear keeps its weight [in][out]. */
int iif_transpose_f32(const float* in, int rows, int cols, int64_t ldi, float* out, int64_t ldo,
                      void* stream);
/* out[0] = alpha / (*d_alpha_div or 1) * sum_{r<rows,c<cols} a[r][c]*b[r][c], fixed order
 * (gradient of the learnable cosine scale). */
int iif_dot_window_f32(const float* a, const float* b, int rows, int cols, int64_t lda, int64_t ldb,
                       float alpha, const float* d_alpha_div, float* out, void* stream);

/* Grouped convolution (ResNeXt, resnet_pytorch.py:137,141) on the MFMA kernels: channels are
 * cut into chunks of `chunk` (64) and each chunk runs as a dense convolution whose weights are
 * block-diagonal over the groups inside it (iif_conv_desc.groups = channels/chunk, cs = cd = chunk).
 * iif_group_pack: fp32 master weights [channels][ldm] (rows of (tap, cin_local < cg)) -> packed
 * [channels][ldp] rows of (tap, chunk-local channel); transposed=1 gives the data-gradient operand
 * (rows = input channels, columns = (tap, chunk-local output channel)).
 * iif_group_unpack_grad: dense-in-chunk weight gradient -> master layout (in-group entries). */
int iif_group_pack(const float* master, int channels, int cg, int chunk, int rs, int ldm, int ldp,
                   int transposed, int out_dtype, void* out, void* stream);
int iif_group_unpack_grad(const float* packed, int channels, int cg, int chunk, int rs, int ldp,
                          int ldm, float* master, void* stream);
/* iif_group_pack for every grouped layer in ONE launch: `table` = `entries` device-resident
 * iif_group_pack_entry records (all outputs of dtype out_dtype), `blocks_per_entry` 256-thread
 * blocks walk each entry.  Same arithmetic as iif_group_pack, entry by entry. */
typedef struct iif_group_pack_entry {
    const float* master;   /* fp32 [channels][ldm] */
    void* out;             /* [channels][ldp] */
    int32_t channels, cg, chunk, rs, ldm, ldp, transposed, reserved;
} iif_group_pack_entry;
int iif_group_pack_batched(const void* table, int entries, int blocks_per_entry, int out_dtype,
                           void* stream);

/* Stem as a space-to-depth convolution: the RxR / stride-2 / pad-(R-1)/2 convolution on a c-channel
 * NCHW fp32 image (resnet_pytorch.py:203: 7x7/2 on 3 channels) equals an AxA / stride-1 / pad-A/2
 * convolution, A = (R+1)/2, on the 2x2 space-to-depth image [n, h/2, w/2, cpad] (channel (di*2+dj)*c + ch,
 * zero padded to cpad), with output grid h/2 x w/2.  No patch matrix is written.
 * iif_space_to_depth_nchw builds that image, iif_stem_s2d_pack the [k][A*A*cpad] weight rows from the
 * master [k][ldm] (r, s, c) rows, iif_stem_s2d_unpack_grad maps the weight gradient back. */
int iif_space_to_depth_nchw(const float* img, int n, int c, int h, int w, int cpad, int out_dtype,
                            void* out, void* stream);
int iif_stem_s2d_pack(const float* master, int k, int c, int r, int ldm, int cpad, int out_dtype,
                      void* out, void* stream);
int iif_stem_s2d_unpack_grad(const float* packed, int k, int c, int r, int cpad, int ldm, float* master,
                             void* stream);

/* Squeeze-and-excitation around the last BN of a residual block (SE_Block.forward,
 * classification/resnet_pytorch.py:313-317 / resnet_cifar.py:102-106, inside SEBottleneck.forward :358-381
 * and Se_Block.forward resnet_cifar.py:163-169).  x is the raw convolution output [n, hw, c] (NHWC), stats
 * the BN stats block (scale at [2c], shift at [3c]), excite / offset fp32 [n, c].
 *   iif_se_squeeze        sums[n,c] = sum_hw x
 *   iif_se_apply          y = relu((a*x + b) * excite[n,c] + identity), identity = residual or
 *                         a2*residual + b2 (residual_stats), relu_bits = 1 bit per element
 *   iif_se_backward_sums  g <- g * [y > 0] in place; s1[n,c] = sum_hw g; s2[n,c] = sum_hw g*x
 *   iif_se_backward_form  out = g * excite[n,c] + offset[n,c]  (gradient w.r.t. the BN output)
 * The [n, c]-sized excitation (two bias-free linears, ReLU, sigmoid; resnet_pytorch.py:306-311, 315), fp32:
 *   iif_se_excite_forward   q = a * sums / hw + b (mean of the BN output);  h = relu(W1 q);  e = sigmoid(W2 h)
 *   iif_se_excite_backward  from s1 / s2 of iif_se_backward_sums: dz2, dz1 (scratch [n,c] / [n,hid]), offset = (dz1 W1) / hw
 *                           (the `offset` of iif_se_backward_form) and the weight gradients dw1 [hid][ldg1], dw2 [c][ldg2]
 * w1 is W1 [hid][ld1]; w2t is the TRANSPOSE of W2, [hid][ldt] (iif_transpose_f32), so both matrices are read along c. */
int iif_se_squeeze(const void* x, int dtype, int n, int hw, int c, float* sums, void* stream);
int iif_se_apply(const void* x, int dtype, int n, int hw, int c, const float* stats, const float* excite,
                 const void* residual, const float* residual_stats, void* y, unsigned char* relu_bits,
                 void* stream);
int iif_se_backward_sums(void* g, const unsigned char* relu_bits, const void* x, int dtype, int n, int hw,
                         int c, float* s1, float* s2, void* stream);
int iif_se_backward_form(const void* g, int dtype, int n, int hw, int c, const float* excite,
                         const float* offset, void* out, void* stream);
int iif_se_excite_forward(const float* sums, const float* stats, int n, int hw, int c, int hid, const float* w1, int ld1,
                          const float* w2t, int ldt, float* q, float* h, float* e, void* stream);
int iif_se_excite_backward(const float* s1, const float* s2, const float* stats, int n, int hw, int c, int hid, const float* w1,
                           int ld1, const float* w2t, int ldt, const float* e, const float* h, const float* q, float* dz2,
                           float* dz1, float* offset, float* dw1, int ldg1, float* dw2, int ldg2, void* stream);

/* mmdet normed predictors (instance_segmentation/mmdet/models/utils/normed_predictor.py: NormedLinear :34-40,
 * IIFNormedLinear :67-73, NormedConv2d with a 1x1 kernel :104-112), fp32:
 *   v = row_scale[row] * x[row] (row_scale nullable = 1);  out = v * scale / (|v|^power + eps);  norms[row] = |v|
 * backward: dx = d(out)/dx^T g.  The products run on iif_conv_igemm / iif_conv_wgrad. */
int iif_rownorm_forward(const float* x, const float* row_scale, int rows, int cols, int64_t ldx, float power,
                        float scale, float eps, float* out, int64_t ldo, float* norms, void* stream);
int iif_rownorm_backward(const float* x, const float* row_scale, const float* norms, const float* g, int rows,
                         int cols, int64_t ldx, int64_t ldg, float power, float scale, float eps, float* dx,
                         int64_t lddx, void* stream);

/* All dense convolutions' transposed copies ([cin][rs*cout], for the data gradient) in ONE launch.  `table` is a
 * DEVICE array of n_desc descriptors sorted by block_start; descriptor i owns the blocks
 * [block_start_i, block_start_{i+1}): rs * ceil(cin/32) * ceil(cout/32) of them, one 32x32 tile of one tap each
 * (tap-major, then cin tiles, then cout tiles).
 * src_off / dst_off are element offsets into the fp32 parameter arena / the output arena. */
typedef struct iif_wt_desc {
    int64_t src_off, dst_off;
    int32_t cout, cin, rs, ldw, ldwt, block_start;
} iif_wt_desc;
int iif_weight_transpose_batched(const float* arena, const iif_wt_desc* table, int n_desc, int total_blocks,
                                 int out_dtype, void* out, void* stream);

/* Weights as ready-made MFMA fragments for the 3x3 / stride-1 / pad-1 bf16 kernel (conv3x3 of resnet_pytorch.py:46-57,
 * forward and data gradient).  Source: bf16 rows [rows][ld] of `taps` x `k` channels — the forward weights
 * [cout][9 * cin] or the transposed copy [cin][9 * cout] of iif_weight_transpose.  Destination, rows * taps * k elements:
 * fragment (row / 16, tap, channel / 32) = 1 KB, lane l's 16 bytes (row l & 15, channels (l >> 4) * 8 .. + 8) at l * 16,
 * so that a wavefront fetches one operand of v_mfma_f32_16x16x32_bf16 with one coalesced load and the weights never pass
 * through LDS.  rows % 16 == 0, k % 32 == 0.  `table` is a DEVICE array of descriptors (element offsets into src_base /
 * dst_base, block_start = first 256-thread block of the descriptor, ascending); total_blocks = sum of
 * ceil(rows * taps * k / 8 / 256).  iif_conv3x3_frag_ok: 1 when a convolution with this descriptor (wgt_frag set) runs on
 * the fragment kernel, 0 when it would take the row-weights path. */
typedef struct iif_pack_desc {
    int64_t src_off, dst_off;
    int32_t rows, taps, k, ld, block_start, reserved;
} iif_pack_desc;
int iif_conv_pack_fragments(const void* src_base, const iif_pack_desc* table, int n_desc, int total_blocks, void* dst_base,
                            void* stream);
int iif_conv3x3_frag_ok(const iif_conv_desc* d);
/* Round 6, ResNeXt's narrow groups (resnet_pytorch.py:137,141 with groups = 32, base width 4: 4 / 8 / 16 channels per group): the
 * block-diagonal 64-channel chunk matrices of iif_group_pack re-packed as 20 fragments per chunk (4 output tiles x 5 tap PAIRS:
 * K of an MFMA = two taps x the tile's own 16 input channels), for iif_conv_desc.wgt_frag with wgt_frag_kind = 1.  Table entries
 * as for iif_conv_pack_fragments (rows = channels of the layer, taps = 9, k = 64, ld = row pitch of the chunk matrix); one
 * 256-thread block per 4 fragments: blocks of an entry = ceil(rows / 64 * 20 / 4).  Valid where every group is <= 16 channels wide. */
int iif_conv_pack_fragments_g16(const void* src_base, const iif_pack_desc* table, int n_desc, int total_blocks, void* dst_base,
                                void* stream);

/* Batch-norm backward through the expanding 1x1 convolution of a bottleneck (conv3 -> bn3 -> += identity -> relu,
 * classification/resnet_pytorch.py:160-167) WITHOUT re-reading the convolution's output y = a2 W^T.  BN backward is affine per
 * channel in (g~, y), dy = A o g~ + B o y + D, with g~ the block-output gradient already gated by the block's ReLU bits, so
 * with P = g~^T a2 (iif_conv_wgrad), Gram = a2^T a2 (iif_conv_wgrad of a2 with itself) and csum = colsum(a2) (iif_bn_stats_sums):
 *   sum g~ y = rowdot(P, W);  dW = diag(A) P + diag(B) W Gram + D (x) csum;  da2 = [g~ | a2] [A o W ; W^T diag(B) W]^T + D W.
 *   iif_conv_igemm_dgrad_masksum  the data gradient that PRODUCES the block-output gradient stores it gated by up_bits and
 *                                 emits per tile into `partial` either (sum dst, 0) (up_x NULL: no read of y) or, with up_x /
 *                                 up_stats (y and its batch statistics), (sum dst, sum dst * xhat) as iif_conv_igemm_dgrad_bnbwd;
 *   iif_bn3_algebra_prep          those partial rows, W (the bf16 copy the forward used) and EITHER P (sum g~ y = rowdot(P, W):
 *                                 y is never read, but P is needed before the data gradient) OR P = NULL (sum g~ xhat from the
 *                                 second half of the rows: y is read once by the producer and P is only needed for dW, off the
 *                                 critical path) -> coef [3][C] = (A, B, D), dgamma, dbeta and the stacked bf16 weights
 *                                 wt [c][ldwt >= C + c]: wt[j][ch] = A[ch] W[ch][j], wt[j][C + i] = sum_ch bf16(B[ch] W[ch][j]) W[ch][i],
 *                                 and bias[j] = sum_ch D[ch] W[ch][j].  Two launches (one ticketed kernel over channel groups x row
 *                                 slices, one slab sum); scratch: iif_bn3_algebra_prep_scratch_floats(C, c) floats; tickets:
 *                                 int32[64], zero on entry, zero again on exit.  c in {64, 128, 256}, C <= 4096.  With colsum2
 *                                 (sum over the pixels of the second K source of the data gradient, i.e. of a2) the bias also absorbs
 *                                 what the bf16 rounding of wt adds to the COLUMN SUMS of the data gradient (exactly zero in exact
 *                                 arithmetic): bias[j] -= (sum_i colsum2[i] d2[j][i] + sum_ch sum(g~)[ch] d1[j][ch]) / m;
 *   iif_conv_igemm_dgrad2_bnbwd   dst = [src | src2] wgt^T + bias (1x1, stride 1, bf16; K runs over src's cs then src2's cs2
 *                                 channels), optionally with the upstream BN-backward sums of iif_conv_igemm_dgrad_bnbwd;
 *   iif_bn3_algebra_dw            dW [C][lddw] from P, W, Gram, csum, coef.
 * c in {64, 128, 256} (the 56x56 ... 14x14 stages of the ImageNet networks).  Everything sums in a fixed order. */
/* Two-pass forward of conv + BN (+ identity) + ReLU for the expanding 1x1 layer of a bottleneck (resnet_pytorch.py:160-167),
 * bf16, 1x1 / stride 1: the raw convolution output is never stored.
 *   iif_conv_igemm_stats_only   pass 1: the per-tile (sum, sum of squares) partial rows of iif_conv_igemm_bnstats — same
 *                               bf16 rounding of the tile, same sums — without the store;
 *   iif_conv_igemm_bn_relu      pass 2 (after iif_bn_finalize_stats): dst = relu(fma(a, bf16(conv), b) + res), a / b at
 *                               stats[2 Cd + c] / stats[3 Cd + c], one byte of ReLU decisions per 8 channels into relu_bits
 *                               (nullable): bit-identical to iif_conv_igemm followed by iif_bn_apply with that residual. */
int iif_conv_igemm_stats_only(const iif_conv_desc* d, const void* src, const void* wgt, float* bn_partial,
                              int64_t bn_partial_floats, int32_t* n_partials, void* stream);
int iif_conv_igemm_bn_relu(const iif_conv_desc* d, const void* src, const void* wgt, void* dst, const void* res,
                           const float* stats, unsigned char* relu_bits, void* stream);
/* Round 6: the same two passes on the register-weight kernel (cs in {64, 128, 256}, cd a multiple of 256, n*hd*wd a multiple
 * of 64; iif_conv_fwdbn_ok says whether a descriptor qualifies), which is what makes the never-stored forward pay
 * (resnet_pytorch.py:160-167: conv3 -> bn3 -> += identity -> relu):
 *   iif_conv_igemm_stats_acc    pass 1: (sum, sum of squares) of the UNROUNDED fp32 accumulators, one partial row per tile
 *                               sequence, nothing staged or stored (the statistics of the convolution itself rather than of
 *                               its bf16 rounding; feed iif_bn_finalize_stats as usual);
 *   iif_conv_igemm_bn_relu2     pass 2: as iif_conv_igemm_bn_relu; with res_stats the residual is the RAW output of the
 *                               block's convolutional shortcut and is normalised on the way in, fma(a2, res, b2) with a2 / b2 at
 *                               res_stats[2 Cd + c] / [3 Cd + c] (iif_bn_apply's residual_stats arithmetic).  relu_bits required. */
int iif_conv_fwdbn_ok(const iif_conv_desc* d);
/* Inference forward: the convolution with a FIXED per-channel affine (eval-mode BN), the residual and the ReLU in its epilogue,
 *   dst = relu(fmaf(a, bf16(conv), b) + r),   r = nothing | res | fmaf(a2, res, b2) with res_affine (the block's convolutional
 * shortcut, stored raw).  affine / res_affine are laid out like the `stats` rows of iif_bn_apply (a at [2 C + c], b at [3 C + c],
 * C = cd * groups), so iif_bn_fold's output serves both routes.  The accumulator tile is rounded to bf16 before the affine,
 * exactly as the stored tensor would have been: the result is bit-identical to iif_conv_igemm followed by
 * iif_bn_apply(relu = 1, res, res_affine); relu_bits (nullable) receives the same decision bytes.  bf16 in and out; 1x1 and
 * 3x3, stride 1 and 2, dense and grouped, any m.  iif_conv_affine_ok (host only, launches nothing) says whether a descriptor
 * has a fused instance with the given residual form; where it says 0, iif_conv_igemm_affine returns IIF_EUNSUPPORTED. */
int iif_conv_affine_ok(const iif_conv_desc* d, int has_res, int has_res_affine);
/* Which kernel family iif_conv_igemm_affine launches for this descriptor and operand set: the answer of the selection step
 * the launch itself starts with (a host function of the descriptor and of WHICH operands there are; it touches no operand
 * and launches nothing): 0 none, 1 tile (three LDS stages), 2 tile (two stages, 4 blocks per CU), 3 tile with general
 * addressing (source channels not in 32s), 4 256-row tile, 5 3x3 halo, 6 3x3 fragment weights, 7 3x3 grouped 16-channel
 * fragments, 8 streaming 1x1, 9 register-weight 1x1, 10 register-weight 3x3, 11 register-staged tile.  d->wgt_frag only
 * has to be non-null where fragments would be supplied.  Follows the IIF_CONV_* switches and the CU budget; the persistent
 * kernels size themselves by the device's compute units (256 assumed where there is no device).  For tests and route
 * listings. */
int iif_conv_affine_route(const iif_conv_desc* d, int has_res, int has_res_affine, int has_relu_bits);
/* The same for every other call of the convolution entry (forward, statistics, data gradient, two-source ...): which launches
 * it makes for this descriptor and this set of operands, answered by the selection step the launch starts with.  Host only: it
 * touches no operand, launches nothing and needs no device.  `operands`: IIF_CONV_OP_* bits, one per operand or option the call
 * would pass (d->transposed says forward or data gradient); cs2: channels of the second source (IIF_CONV_OP_SRC2) or of the
 * recomputed upstream a2 (IIF_CONV_OP_RX), else ignored.  Operands count as 16-byte aligned and the partial buffer as large
 * enough.  Returns the number of launches (1; up to 4 for a stride-2 data gradient launched class by class) and writes, for
 * each launch that fits `cap` int32 of `out`, the nine values {family (as iif_conv_affine_route; 12 stem, 13 all parity
 * classes in one grid), instance (columns per tile of the tile families, rows per tile of the halo kernel, slice width of the
 * streaming kernel, index of the register-weight instance), parity class or -1, pixel tiles, column tiles, grid x, grid y,
 * threads per block, partial rows written}.  A call the entry would refuse returns that negative status code. */
enum { IIF_CONV_OP_RES = 1, IIF_CONV_OP_RES_IS_DST = 2 /* dst += ... */, IIF_CONV_OP_RES_BITS = 4 /* ReLU bits gate the residual */,
       IIF_CONV_OP_BIAS = 8, IIF_CONV_OP_PARTIAL = 16 /* partial rows: forward statistics, or with UP_* the backward sums */,
       IIF_CONV_OP_UP_X = 32, IIF_CONV_OP_UP_BITS = 64, IIF_CONV_OP_UP_STATS = 128, IIF_CONV_OP_SRC2 = 256,
       IIF_CONV_OP_SRC_BIAS = 512, IIF_CONV_OP_GATED_STORE = 1024, IIF_CONV_OP_NO_STORE = 2048 /* iif_conv_igemm_stats_only */,
       IIF_CONV_OP_NO_STORE_ACC = 4096 /* iif_conv_igemm_stats_acc */, IIF_CONV_OP_RX = 8192 /* ..._dgrad_masksum_rx */,
       IIF_CONV_OP_PROLOGUE = 16384 /* iif_conv_igemm_bnstats_pro */ };
int iif_conv_route(const iif_conv_desc* d, unsigned operands, int cs2, int32_t* out, int cap);
int iif_conv_igemm_affine(const iif_conv_desc* d, const void* src, const void* wgt, void* dst, const void* res,
                          const float* res_affine, const float* affine, unsigned char* relu_bits, void* stream);
int iif_conv_igemm_stats_acc(const iif_conv_desc* d, const void* src, const void* wgt, float* bn_partial,
                             int64_t bn_partial_floats, int32_t* n_partials, void* stream);
int iif_conv_igemm_bn_relu2(const iif_conv_desc* d, const void* src, const void* wgt, void* dst, const void* res,
                            const float* res_stats, const float* stats, unsigned char* relu_bits, void* stream);
int iif_conv_igemm_dgrad_masksum(const iif_conv_desc* d, const void* src, const void* wgt, void* dst, const void* res,
                                 const unsigned char* res_bits, const void* up_x, const unsigned char* up_bits,
                                 const float* up_stats, float* partial, int64_t partial_floats, int32_t* n_partials,
                                 void* stream);
/* Round 6: the batch norm + ReLU of the PREVIOUS unit applied in the convolution's operand path (resnet_pytorch.py:157-160:
 * bn2 -> relu -> conv3).  src_raw is that unit's raw convolution output [n, h, w, cs] and src_stats its statistics as
 * iif_bn_finalize_stats wrote them; each tile is normalised in LDS (iif_bn_apply's arithmetic) before the matrix pipe reads
 * it, and the activated tensor is written out as a by-product - act_out [n, h, w, cs] bf16 and act_bits (one byte per 8
 * channels), bit-identical to iif_bn_apply's - because backward needs it; act_csum (nullable) receives per partial row one
 * row [2][cs] = (its column sums, zeros), the layout iif_bn_partial_sums reduces.  dst NULL: the statistics-only pass of iif_conv_igemm_stats_acc; otherwise the stored forward
 * with statistics of iif_conv_igemm_bnstats.  One launch and one pass over the activation less per bottleneck.
 * iif_conv_pro_ok(d, stats_only) says whether the register-weight kernel has the instance. */
int iif_conv_pro_ok(const iif_conv_desc* d, int stats_only);
int iif_conv_igemm_bnstats_pro(const iif_conv_desc* d, const void* src_raw, const float* src_stats, void* act_out,
                               unsigned char* act_bits, float* act_csum, const void* wgt, void* dst, float* bn_partial,
                               int64_t bn_partial_floats, int32_t* n_partials, void* stream);
/* Round 6: iif_conv_igemm_dgrad_masksum whose (sum dst, sum dst * xhat) rows are formed WITHOUT the upstream block's conv3 output:
 * each tile of it is recomputed on the matrix pipe from that block's a2 (up_a2, [n*h*w, up_c2] bf16) and conv3 weights as the
 * forward multiplied them (up_w3, [cd, up_ldw3] bf16), rounded to bf16 as the stored tensor would have been.  Together with
 * iif_conv_igemm_stats_acc / iif_conv_igemm_bn_relu2 this lets the forward pass never store that output, with "sums from the
 * producer" (P and Gram off the critical path).  Register-weight kernel only: iif_conv_dgrad_rx_ok(d, up_c2) says whether the
 * (cs, up_c2) pair has an instance ((64, 64), (128, 64), (128, 128), (256, 128)). */
int iif_conv_dgrad_rx_ok(const iif_conv_desc* d, int up_c2);
int iif_conv_igemm_dgrad_masksum_rx(const iif_conv_desc* d, const void* src, const void* wgt, void* dst, const void* res,
                                    const unsigned char* res_bits, const void* up_a2, int up_c2, const void* up_w3, int up_ldw3,
                                    const unsigned char* up_bits, const float* up_stats, float* partial, int64_t partial_floats,
                                    int32_t* n_partials, void* stream);
/* ... and with the two small matrices the algebraic BN3 backward of that upstream block needs as BY-PRODUCTS of the same launch
 * (classification/resnet_pytorch.py:162-163, conv3 + bn3 backward as autograd derives them): P = dst^T a2 ([cd, up_c2]: what the
 * conv3 weight-gradient GEMM computes) and Gram = a2^T a2 ([up_c2, up_c2]).  The block that forms a tile of dst holds it in its
 * staging buffers and the a2 tile in LDS; it accumulates both products over its tiles and writes ONE fp32 slab
 * [(cd + up_c2), pg_ld] (P rows first) per tile sequence into pg_slabs (pg_floats floats available; *n_slabs receives the slab count).
 * iif_slab_sum adds the slabs in sequence order (deterministic).  The stacked weight-gradient launch that re-read dst and a2 from
 * memory (0.5 GB per bottleneck at 56 x 56) is not needed.  iif_conv_dgrad_rx_pg_ok: up_c2 = 64, cd = 256, cs in {64, 128}. */
int iif_conv_dgrad_rx_pg_ok(const iif_conv_desc* d, int up_c2);
int iif_conv_igemm_dgrad_masksum_rx_pg(const iif_conv_desc* d, const void* src, const void* wgt, void* dst, const void* res,
                                       const unsigned char* res_bits, const void* up_a2, int up_c2, const void* up_w3, int up_ldw3,
                                       const unsigned char* up_bits, const float* up_stats, float* partial, int64_t partial_floats,
                                       int32_t* n_partials, float* pg_slabs, int64_t pg_floats, int pg_ld, int32_t* n_slabs,
                                       void* stream);
/* out[r][c] = sum over the n slabs [rows, ld] of slabs[s][r][c], c < cols, in slab order (the split-K reduction of
 * iif_conv_wgrad for slabs another kernel wrote).  slab_floats: floats available behind `slabs`; with room for ceil(n / 16)
 * more slabs behind the n the reduction runs in two parallel stages (n > 32 and a slab under about 1 MiB, as iif_conv_wgrad_plan
 * describes).  Columns >= cols of out are not written.  ld % 4 == 0 and cols % 4 == 0 (the sum moves 4-float vectors), slabs and
 * out 16-byte aligned; otherwise IIF_EINVAL. */
int iif_slab_sum(float* slabs, int64_t slab_floats, int n, int rows, int ld, int cols, float* out, void* stream);
int iif_conv_igemm_dgrad2_bnbwd(const iif_conv_desc* d, const void* src, const void* src2, int cs2, const void* wgt,
                                const float* bias, void* dst, const void* up_x, const unsigned char* up_bits,
                                const float* up_stats, float* partial, int64_t partial_floats, int32_t* n_partials,
                                void* stream);
int64_t iif_bn3_algebra_prep_scratch_floats(int C, int c);
int iif_bn3_algebra_prep(const float* P, int ldp, const void* w_bf16, int ldw, const float* partial, int n_partials,
                         const float* stats, const float* gamma, int C, int c, int64_t m, float* coef, float* dgamma, float* dbeta,
                         void* wt, int ldwt, float* bias, float* scratch, int64_t scratch_floats, int32_t* tickets,
                         const float* colsum2 /* nullable: colsum of the data gradient's second source, [c] */, void* stream);
int iif_bn3_algebra_dw(const float* P, int ldp, const void* w_bf16, int ldw, const float* gram, int ldg, const float* csum,
                       const float* coef, int C, int c, float* dW, int lddw, void* stream);

/* The convolution library reads its experiment / test switches (IIF_CONV_NO_STREAM1X1, IIF_CONV_STREAM1X1_FORCE,
 * IIF_CONV_NO_SHORTK, IIF_CONV_TWOSTAGE_K, IIF_CONV_FORCE_BN64, IIF_CONV_REGSTAGE, IIF_CONV_NO_V2) from the environment once, when it is
 * loaded: nothing on the launch path calls getenv.  A harness that changes one of them afterwards calls this to have them
 * read again.  Not needed (and not used) by the product path. */
int iif_conv_reload_env(void);

/* Data gradient with a MASKED residual: dst = dgrad(src, wgt) + res * [bit], where res_bits holds one ReLU
 * decision bit per element of res (the relu_bits of iif_bn_apply: one byte per 16-byte vector).  This is the
 * identity path of a residual block in backward (resnet_pytorch.py:163-167: out += identity; relu): the
 * gradient of the block output is gated by the block's ReLU while it is added, so no masked copy is ever
 * written.  transposed=1, stride 1 only. */
int iif_conv_igemm_masked_res(const iif_conv_desc* d, const void* src, const void* wgt, void* dst,
                              const void* res, const unsigned char* res_bits, void* stream);

/* Mask-side class-channel selection.  pred is [n, c, hw] (NCHW mask logits / probabilities,
 * fp32 or bf16), labels int64 [n] the IIF-derived class of every RoI.
 *   iif_mask_gather       out[n, hw] = pred[i, labels[i], :]        (FCNMaskHead.get_seg_masks,
 *                         mmdet/models/roi_heads/mask_heads/fcn_mask_head.py:289-290)
 *   iif_mask_bce_fwd_bwd  loss = mean_i,p BCEWithLogits(pred[i, labels[i], p], target[i, p])   (mask_cross_entropy,
 *                         mmdet/models/losses/cross_entropy_loss.py:158-162); dpred (nullable, fp32 [n, c, hw],
 *                         ZERO-FILLED by the caller) receives grad_scale * d loss / d pred in the selected
 *                         channels only.  row_loss: [n] scratch.  An out-of-range label sets bit 0 of *status
 *                         (device int, caller-zeroed) and contributes nothing. */
int iif_mask_gather(const void* pred, int dtype, const int64_t* labels, int n, int c, int hw, float* out,
                    int* status, void* stream);
int iif_mask_bce_fwd_bwd(const void* pred, int dtype, const float* target, const int64_t* labels, int n, int c,
                         int hw, float grad_scale, float* row_loss, float* loss, float* dpred, int* status,
                         void* stream);

/* FASA side outputs of the IIF classifier loss (instance_segmentation/mmdet).
 *   iif_class_accumulate  FasaIIFLoss.forward with use_cums (losses/fasa_iif_loss.py:154-160): for every class
 *                         c in [0, C): cum_labels[c] += #{labels == c}, cum_losses[c] += sum of rows over them
 *                         (row order; labels outside [0, C) are skipped).
 *   iif_fasa_update       fa_update / fa_update_push (roi_heads/bbox_heads/fasa_bbox_head.py:118-147): per-class mean
 *                         and unbiased variance of embedding [n, d] rows, first sight -> copy, afterwards
 *                         exponential moving average with `decay`; feature_used[c] becomes 1.
 *   iif_fasa_generate     fa_generate (:149-172) with the random numbers supplied by the caller: classes with
 *                         rnd[c] < prob[c] and feature_used[c] > 0, ascending, get out[k] = mean + sqrt(var) *
 *                         normal[c], out_labels[k] = c; *count (device) = number of rows written (<= c).
 *                         slot_class: int32 [c] scratch. */
int iif_class_accumulate(const float* rows, const int64_t* labels, int n, int c, float* cum_losses,
                         float* cum_labels, void* stream);
int iif_fasa_update(const float* embedding, const int64_t* labels, int n, int d, int64_t ld, int c, float decay,
                    float* feature_mean, float* feature_var, float* feature_used, void* stream);
int iif_fasa_generate(const float* rnd, const float* prob, const float* feature_used, const float* feature_mean,
                      const float* feature_var, const float* normal, int c, int d, int* slot_class, int* count,
                      float* out, int64_t* out_labels, void* stream);

/* FasaBBoxHead.loss without a host read (csrc/fasa_head.hip, csrc/head_loss.hip; ConvFCFASABBoxHead.loss,
 * roi_heads/bbox_heads/fasa_bbox_head.py:217-300).
 *   iif_fasa_update_rows      iif_fasa_update on the rows with 0 <= labels[i] < c of a PADDED batch, selected on the device:
 *                             feature_mean / feature_var / feature_used end with the very bits iif_fasa_update gives on
 *                             embedding[pos], labels[pos] (one shared __device__ function, sums in ascending row order).
 *                             A row whose label is outside [0, c) is never dereferenced; no atomics; two launches (the
 *                             statistics, then feature_used).  present: int32 [c] scratch.  n <= IIF_FASA_ROWS_MAX_ROWS and
 *                             c <= IIF_FASA_ROWS_MAX_CLASSES, else IIF_EUNSUPPORTED; any d, any ld >= d.
 *   iif_fasa_generate_padded  iif_fasa_generate with a fixed shape, ONE launch: out [capacity, d], out_labels [capacity],
 *                             out_weights [capacity].  Row k below count[0] = min(#drawn, capacity) holds the k-th drawn
 *                             class (ascending) exactly as iif_fasa_generate writes it, weight aug_weight; the rows from
 *                             count[0] on hold zeros, label c and weight 0.  count: device int32 [2] = (rows written,
 *                             drawn classes dropped because capacity was smaller).
 *   iif_head_loss_cums_fwd    iif_head_loss_fwd for FasaIIFLoss with OPEN accumulators (reduction 'none', then .mean();
 *                             losses/fasa_iif_loss.py:145-160): rows_out[i] = loss_weight * w_i * cw[l_i] * nll_i,
 *                             *loss_out = sum_i rows_out[i] / avg with avg = max(#{w_i != 0}, 1), *acc_out the top-1
 *                             accuracy over the rows with w_i != 0, and in a second launch cum_losses[l] += the sum of
 *                             rows_out over the rows of label l in ascending row order, cum_labels[l] += their number.
 *                             A row of weight 0 is not read and enters none of these.  dscores as iif_head_loss_fwd's,
 *                             to be finished by iif_head_loss_bwd with loss_weight and *avg_out.  Arguments are checked
 *                             as iif_head_loss_fwd's. */
#define IIF_FASA_ROWS_MAX_ROWS 65535
#define IIF_FASA_ROWS_MAX_CLASSES 4096
int iif_fasa_update_rows(const float* embedding, const int64_t* labels, int n, int d, int64_t ld, int c, float decay,
                         float* feature_mean, float* feature_var, float* feature_used, int32_t* present, void* stream);
int iif_fasa_generate_padded(const float* rnd, const float* prob, const float* feature_used, const float* feature_mean,
                             const float* feature_var, const float* normal, int c, int d, int capacity, float aug_weight,
                             float* out, int64_t* out_labels, float* out_weights, int32_t* count, void* stream);
int iif_head_loss_cums_fwd(const void* scores, int dtype, int64_t ld_scores, const float* table, const int64_t* labels,
                           const float* label_weights, const float* class_weight, int64_t ignore_index, float loss_weight,
                           int N, int C, void* dscores, int64_t ld_dscores, float* rows_out, float* cum_losses,
                           float* cum_labels, float* loss_out, float* acc_out, float* avg_out, int32_t* d_status,
                           void* d_workspace, void* stream);

/* Data gradient that also emits the batch-norm BACKWARD partial sums of the upstream unit.  dst (= dL/dy of the
 * unit that produced this convolution's input) is gated by that unit's ReLU bits `up_bits` (nullable: no ReLU) and
 * reduced per pixel tile against its pre-normalisation output `up_x` (same shape as dst) and statistics
 * `up_stats` (mean at [c], invstd at [cd + c]): partial[t] = (sum g, sum g * xhat) per channel, *n_partials rows.
 * iif_bn_backward_partials then finishes that unit's BN backward without the reduction pass over dst and up_x
 * (what F.batch_norm's backward re-reads in resnet_pytorch.py:152-167).  bf16, cd % 8 == 0, dense;
 * res / res_bits as in iif_conv_igemm / iif_conv_igemm_masked_res; stride-2 launches visit every pixel once. */
int iif_conv_igemm_dgrad_bnbwd(const iif_conv_desc* d, const void* src, const void* wgt, void* dst, const void* res,
                               const unsigned char* res_bits, const void* up_x, const unsigned char* up_bits,
                               const float* up_stats, float* partial, int64_t partial_floats, int32_t* n_partials,
                               void* stream);
int iif_bn_backward_partials(const void* gy, const uint8_t* relu_bits, const void* x, int dtype, int64_t m, int c,
                             const float* stats, const float* gamma, const float* partial, int n_partials,
                             float* dgamma, float* dbeta, void* dx, void* workspace, int64_t workspace_bytes,
                             void* stream);
/* Cross-replica batch statistics (nn.SyncBatchNorm, classification/train.py:190-191): reduction and normalisation as
 * separate calls so that the host can all-reduce the per-channel sums of all ranks in between.
 *   iif_bn_partial_sums         sums[0][c] / sums[1][c] = column sums of partial rows [n][2][c] (fixed order, fp64)
 *   iif_bn_stats_sums           the same straight from x [m, c]: (sum x, sum x^2); workspace as iif_bn_forward_stats
 *   forward: all-reduce sums, then iif_bn_finalize_stats(sums, 1, m * world, ...) (one "partial row", global count)
 *   iif_bn_backward_sums        (sum g, sum g*xhat) of this rank, g gated by y_mask > 0 or relu_bits
 *   iif_bn_backward_apply_sums  dgamma / dbeta from the LOCAL sums (the gradient all-reduce averages them as it does every
 *                               parameter gradient), dx with mean(g), mean(g*xhat) from the all-reduced total_sums and
 *                               total_count = m * world; gmasked nullable; coef_scratch: 3*c floats */
int iif_bn_partial_sums(const float* partial, int n_partials, int c, float* sums, void* stream);
int iif_bn_stats_sums(const void* x, int dtype, int64_t m, int c, float* sums, void* workspace, int64_t workspace_bytes,
                      void* stream);
int iif_bn_backward_sums(const void* gy, const void* y_mask, const uint8_t* relu_bits, const void* x, int dtype, int64_t m,
                         int c, const float* stats, float* sums, void* workspace, int64_t workspace_bytes, void* stream);
int iif_bn_backward_apply_sums(const void* gy, const void* y_mask, const uint8_t* relu_bits, const void* x, int dtype,
                               int64_t m, int c, const float* stats, const float* gamma, const float* local_sums,
                               const float* total_sums, double total_count, float* dgamma, float* dbeta, void* dx,
                               void* gmasked, float* coef_scratch, void* stream);
/* the same with the slice reduction and the finalisation of > 512 partial rows in one launch (tickets as above) */
int iif_bn_backward_partials_fused(const void* gy, const uint8_t* relu_bits, const void* x, int dtype, int64_t m, int c,
                                   const float* stats, const float* gamma, const float* partial, int n_partials,
                                   float* dgamma, float* dbeta, void* dx, void* workspace, int64_t workspace_bytes,
                                   int32_t* tickets, void* stream);

/* Stem without a stored activation (resnet_pytorch.py:284-287: bn1 -> relu -> maxpool):
 *   iif_maxpool_bn_forward           max pool over relu(a*x + b) of the RAW convolution output x (stats: scale at [2c],
 *                                    shift at [3c]); candidates are rounded to the storage type first, so value and
 *                                    argmax equal iif_bn_apply followed by iif_maxpool_forward
 *   iif_bn_backward_relu_recompute   iif_bn_backward with the ReLU mask recomputed as a*x + b > 0 (same fmaf)
 *   iif_bn_backward_relu_recompute_pooled   the same, its two column sums taken from the POOLED gradient g_pool and the RAW stem
 *                                    output at each window's arg max, pool_x ([pool_pixels][c] each; written by
 *                                    iif_maxpool_bn_forward when its pool_x argument is given) instead of a reduction pass over
 *                                    gy and x: sum g = sum g_pool [a x* + b > 0], sum g xhat = sum g_pool [a x* + b > 0] (x* - mean) invstd
 *                                    - term for term what the reduction pass adds, in another order.  gy is the pooled gradient
 *                                    already scattered to the stem's resolution (iif_maxpool_backward) */
int iif_maxpool_bn_forward(const void* x, int dtype, const float* stats, int n, int h, int w, int c, int k, int stride,
                           int pad, void* y, uint8_t* argmax, void* pool_x /* nullable */, void* stream);
int iif_bn_backward_relu_recompute(const void* gy, const void* x, int dtype, int64_t m, int c, const float* stats,
                                   const float* gamma, float* dgamma, float* dbeta, void* dx, void* workspace,
                                   int64_t workspace_bytes, void* stream);
int iif_bn_backward_relu_recompute_pooled(const void* gy, const void* x, int dtype, int64_t m, int c, const float* stats,
                                          const float* gamma, float* dgamma, float* dbeta, void* dx, void* workspace,
                                          int64_t workspace_bytes, const void* g_pool, const void* pool_x, int64_t pool_pixels,
                                          void* stream);
/* iif_maxpool_backward (3x3 / stride 2 / pad 1) + iif_bn_backward_relu_recompute_pooled in one: the pooled gradient g_pool
 * [n][ho][wo][c] is gathered through `argmax` inside the normalisation pass, the scattered gradient at the stem's resolution
 * [n][h][w][c] is never formed.  dx and dgamma / dbeta bit-identical to the two calls (the gathered value is rounded to the
 * storage type as the stored tensor was).  workspace >= (min(512, ceil(n*ho*wo/64)) * 2c + 3c) * 4 bytes. */
int iif_bn_backward_pool_fused(const void* g_pool, const uint8_t* argmax, const void* pool_x, const void* x, int dtype, int n,
                               int h, int w, int c, int ho, int wo, const float* stats, const float* gamma, float* dgamma,
                               float* dbeta, void* dx, void* workspace, int64_t workspace_bytes, void* stream);

/* SingleRoIExtractor (mmdet roi_heads/roi_extractors/single_level_roi_extractor.py with mmcv's RoIAlign, pool_mode 'avg') in ONE
 * launch over all FPN levels; iif_amd/mmdet_roi_extractor.py.  levels: a HOST array of num_levels (1 .. 8) descriptors, copied
 * into the launch: ptr = the level's features, fp32 NHWC [N][H][W][C] (torch's channels_last), the same N and C on every level.
 * rois [K] rows of (batch index, x1, y1, x2, y2) fp32, ld_rois floats apart (>= 5), read in place.  Per roi, in float32 with
 * the reference's operations in its order:
 *   level   num_levels > 1: clamp(floorf(log2f(sqrtf((x2 - x1) * (y2 - y1)) / finest_scale + 1e-6f)), 0, num_levels - 1), from
 *           the roi as given; a NaN scale is a zero row without gradient (lvl_out -1).  One level: no mapping.
 *   rescale roi_scale_factor > 0: base_roi_extractor.py roi_rescale, after the level is chosen (<= 0: none).
 *   RoIAlign  off = aligned ? .5f : 0; start = coord * spatial_scale - off; roi = end - start (not aligned: at least 1);
 *           bin = roi / pooled; grid = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(roi / pooled) per axis;
 *           sample y = start_h + ph * bin_h + (iy + .5f) * bin_h / grid_h; y < -1 || y > H || x < -1 || x > W adds nothing; else
 *           y = max(y, 0), y_low = (int)y, y_low >= H - 1 ? y_low = y_high = H - 1, y = y_low; four-corner bilinear weights;
 *           out = sum / max(grid_h * grid_w, 1); grid <= 0 on an axis: a zero bin.  The bin is summed in separable form (per-axis
 *           pixel weights from those samples), so only the summation order differs from mmcv's loop.
 *   A batch index < 0 or >= N (or NaN), a non-finite coordinate or a grid count above 65536: a zero row without gradient.
 * out: fp32 [K][C][pooled_h][pooled_w] (out_channels_last: [K][pooled_h][pooled_w][C]).  lvl_out (nullable): int32 [K].
 * Allocates nothing, reads nothing back.  IIF_EINVAL before any launch: a null or misaligned (4 bytes) pointer, num_levels
 * outside 1 .. 8, N / C / H / W / pooled_h / pooled_w <= 0 (pooled > 1024), spatial_scale or (num_levels > 1) finest_scale not
 * positive, ld_rois < 5, K < 0.  K == 0: IIF_OK, nothing is enqueued. */
typedef struct iif_roi_level {
    void* ptr;
    int32_t H, W;
    float spatial_scale;
} iif_roi_level;
int iif_roi_extract_forward(const iif_roi_level* levels, int num_levels, int N, int C, const float* rois, int64_t ld_rois,
                            int64_t K, int pooled_h, int pooled_w, int sampling_ratio, int aligned, float finest_scale,
                            float roi_scale_factor /* <= 0: none */, float* out, int out_channels_last,
                            int32_t* lvl_out /* int32 [K] or NULL */, void* stream);
/* The gradient of iif_roi_extract_forward with respect to the features: one clear of `arena` (arena_bytes; every
 * grad_levels[i].ptr, fp32 NHWC like the features, must lie inside it with its N * H * W * C floats) and one launch that adds
 * grad_out[k, c, ph, pw] * weight / count into the roi's level with float atomics, 256 contiguous bytes per wave-instruction
 * - so sums depend on arrival order in their last bits, and a level no roi maps to comes back all zero.  grad_out: the layout
 * of `out` (grad_channels_last).  The same geometry arguments and checks as the forward entry; K == 0: nothing is enqueued
 * (the arena is not cleared). */
int iif_roi_extract_backward(const iif_roi_level* grad_levels, int num_levels, int N, int C, const float* rois, int64_t ld_rois,
                             int64_t K, int pooled_h, int pooled_w, int sampling_ratio, int aligned, float finest_scale,
                             float roi_scale_factor, const float* grad_out, int grad_channels_last, void* arena,
                             int64_t arena_bytes, void* stream);

/* The two ends of the Mask R-CNN mask branch (csrc/mask_ops.hip; iif_amd/mmdet_mask_target.py, iif_amd/mmdet_mask_loss.py).
 *
 * iif_mask_targets: mask_target (mmdet core/mask/mask_target.py:7-127) with BitmapMasks.crop_and_resize
 * (core/mask/structures.py:333-367) for all images of a batch in ONE launch.  images: a HOST array of num_images (1 .. 16)
 * descriptors, copied into the launch: ptr = the image's gt masks, uint8 (any non-zero byte is "inside"), G masks of H x W, rows
 * ld_row bytes apart (>= W), masks ld_mask bytes apart (>= (H - 1) * ld_row + W): masks are read IN PLACE through the gt index,
 * no float copy of a mask is formed.  G == 0 (ptr may be NULL): every roi of that image is a zero row.
 * rois [K] rows of (image index, x1, y1, x2, y2) fp32, ld_rois floats apart (>= 5): what iif_roi_targets returns.
 * gt_inds int64 [K].  Per roi, in float32 with the reference's operations in its order:
 *   clip      x = fminf(fmaxf(x, 0), W), y likewise with H (np.clip on the float32 proposal)
 *   RoIAlign  the definition at iif_roi_extract_forward with spatial_scale 1, sampling_ratio 0, aligned, pooled = (mask_h, mask_w)
 *             on the image  m[y, x] = (byte != 0);  summed in the separable form, so only the summation order differs
 *   out       binarize != 0: value >= 0.5f ? 1.0f : 0.0f; else the value (soft_mask_target)
 *   A zero row: an image index outside [0, num_images) (NaN included; the -1 padding rows of the padded samplings), a gt index
 *   outside [0, G), a non-finite coordinate, a grid count above 65536.
 * out: fp32 [K][mask_h][mask_w].  The result is a pure function of the arguments' values: no atomics, and the same bits wherever
 * the masks lie in memory and whatever their pitches.  Allocates nothing, reads nothing back.
 * IIF_EINVAL before any launch: a null or misaligned pointer (rois / out 4 bytes, gt_inds 8), num_images outside 1 .. 16, G < 0,
 * H / W / mask_h / mask_w <= 0, ld_row < W, ld_mask too small, ld_rois < 5, K < 0.  IIF_EUNSUPPORTED: W > 4096 or mask_h /
 * mask_w > 64 (the per-axis weights and the output tile live in LDS).  K == 0: IIF_OK, nothing is enqueued. */
typedef struct iif_mask_image {
    const uint8_t* ptr;
    int32_t G, H, W;
    int64_t ld_row, ld_mask;
} iif_mask_image;
int iif_mask_targets(const iif_mask_image* images, int num_images, const float* rois, int64_t ld_rois, const int64_t* gt_inds,
                     int64_t K, int mask_h, int mask_w, int binarize, float* out, void* stream);
/* iif_paste_masks: FCNMaskHead.get_seg_masks between the logits and the boolean image (fcn_mask_head.py:228-306 with
 * _do_paste_mask, :344-412, skip_empty=False) in ONE launch.  mask_pred [N][C][h][w], dtype IIF_F32 or IIF_BF16 (widened to
 * float32): logits, or with activated != 0 probabilities.  labels int64 [N], or NULL: channel 0 (class-agnostic heads).
 * boxes [N] rows of (x0, y0, x1, y1, ...) fp32, ld_boxes floats apart (>= 4): det_bboxes [N, 5] is read in place.
 * Per detection and pixel (py, px) of the img_h x img_w image, in float32 with the reference's operations in its order:
 *   value   p = 1 / (1 + expf(-logit)) of the label's channel (activated: the value itself)
 *   grid    gx = ((px + .5f) - x0) / (x1 - x0) * 2 - 1, +-inf replaced by 0; gy likewise
 *   sample  grid_sample, bilinear, align_corners=False, zero padding: ix = ((gx + 1) * w - 1) / 2, x_nw = floorf(ix), weights
 *           (x_nw + 1 - ix) and (ix - x_nw) per axis, the four taps added in the order nw, ne, sw, se, taps outside the tile add
 *           nothing
 *   out     value >= threshold ? 1 : 0 (uint8; torch.bool's storage).  A pixel whose four taps lie outside is 0 >= threshold.
 *   A label outside [0, C): an all-zero mask.  A NaN coordinate (0 / 0: a zero-size box edge exactly at a pixel centre) is not
 *   offered: such a pixel is treated as one with its four taps outside.
 * out: uint8 [N][img_h][img_w], any alignment.  Allocates nothing, reads nothing back.
 * IIF_EINVAL before any launch: a null or misaligned pointer, an unknown dtype, C / h / w / img_h / img_w <= 0, ld_boxes < 4,
 * N < 0 or > 65535, threshold < 0 (the reference's uint8 visualisation branch) or NaN.  IIF_EUNSUPPORTED: h or w > 64, img_h *
 * img_w >= 2^31.  N == 0: IIF_OK, nothing is enqueued. */
int iif_paste_masks(const void* mask_pred, int dtype, int activated, const int64_t* labels /* NULL: channel 0 */,
                    const float* boxes, int64_t ld_boxes, int64_t N, int C, int h, int w, int img_h, int img_w, float threshold,
                    uint8_t* out, void* stream);
/* COCO run-length encoding on the device (csrc/mask_rle.hip; iif_amd/mmdet_mask_loss.py: paste_masks_rle, encode_masks,
 * get_seg_masks_rle): what pycocotools' mask.encode returns for each mask, without the host loop and - for pasted masks - without
 * the boolean image.  A mask of H x W is read in column-major order, pixel j = x * H + y; its counts alternate run lengths
 * starting with a run of zeros (which may be 0 long), so they are the differences of successive transition positions (j with
 * M[j] != M[j - 1], M[-1] := 0), opened by 0 and closed by H * W.
 *
 * Two steps, with one small read by the caller between them:
 *   ..._count  transitions per (mask, column, row segment) into `workspace`, their exclusive scan in place, totals[n] = the
 *              number of counts of mask n (int32 [N]) and the masks' offsets in the flat run buffer (kept in the workspace)
 *   (caller)   reads totals, total = their sum, allocates positions and runs: uint32 [total] each
 *   ..._fill   the same pixels again: transition positions into `positions`, then runs[k] = positions[k] - positions[k - 1]
 *              within each mask.  runs holds the counts of mask 0, then of mask 1, ...; positions is scratch.
 * workspace: iif_rle_workspace_bytes(N, H, W) bytes, 8-byte aligned, the SAME buffer untouched between the two steps; the fill
 * step must get the arguments of the count step.  No atomics: the same bytes from call to call.  A `total` below the true sum
 * is not an overrun: what does not fit is dropped.
 *
 * iif_paste_rle_*: the masks iif_paste_masks would write, decided pixel by pixel by the same definition (csrc/mask_paste.h), but
 * evaluated only inside the conservative rectangle around each box - outside it the mask is the constant 0 >= threshold; the
 * arguments, limits and checks of iif_paste_masks (H = img_h, W = img_w).
 * iif_mask_rle_*: masks uint8 (any non-zero byte is 1; torch.bool's storage), N masks of H x W read IN PLACE, rows ld_row bytes
 * apart (>= W), masks ld_mask bytes apart (>= (H - 1) * ld_row + W).  IIF_EINVAL: N < 0 or > 65535, H / W <= 0, a pitch too
 * small, a null pointer; IIF_EUNSUPPORTED: H * W >= 2^31.
 * Both: IIF_EINVAL for a null or misaligned workspace / totals / positions / runs (4 bytes), a workspace below
 * iif_rle_workspace_bytes, total < N.  N == 0: IIF_OK, nothing is enqueued. */
int64_t iif_rle_workspace_bytes(int64_t N, int H, int W);
int iif_paste_rle_count(const void* mask_pred, int dtype, int activated, const int64_t* labels /* NULL: channel 0 */,
                        const float* boxes, int64_t ld_boxes, int64_t N, int C, int h, int w, int img_h, int img_w, float threshold,
                        void* workspace, int64_t workspace_bytes, int32_t* totals, void* stream);
int iif_paste_rle_fill(const void* mask_pred, int dtype, int activated, const int64_t* labels, const float* boxes, int64_t ld_boxes,
                       int64_t N, int C, int h, int w, int img_h, int img_w, float threshold, void* workspace,
                       int64_t workspace_bytes, const int32_t* totals, int64_t total, uint32_t* positions, uint32_t* runs,
                       void* stream);
int iif_mask_rle_count(const uint8_t* masks, int64_t ld_row, int64_t ld_mask, int64_t N, int H, int W, void* workspace,
                       int64_t workspace_bytes, int32_t* totals, void* stream);
int iif_mask_rle_fill(const uint8_t* masks, int64_t ld_row, int64_t ld_mask, int64_t N, int H, int W, void* workspace,
                      int64_t workspace_bytes, const int32_t* totals, int64_t total, uint32_t* positions, uint32_t* runs,
                      void* stream);
/* iif_rle_to_string (host code: the runs are on the host by then): pycocotools' rleToString of m counts.  Count i is written as
 * x = counts[i] - (i > 2 ? counts[i - 2] : 0) in signed 64-bit, five bits at a time from the low end: c = x & 0x1f, x >>= 5
 * (arithmetic), more = (c & 0x10) ? x != -1 : x != 0, byte = (c | (more ? 0x20 : 0)) + 48.  out: `cap` bytes, no terminator;
 * *len (nullable) = the length of the string, also when it does not fit.  7 * m bytes always suffice.  IIF_EINVAL: m < 0, cap < 0,
 * a null counts with m > 0, a null out with cap > 0, and a string longer than cap - then nothing is written past out[cap - 1]. */
int iif_rle_to_string(const uint32_t* counts, int64_t m, char* out, int64_t cap, int64_t* len);

/* The class-selected mask predictor (csrc/mask_predictor.hip; iif_amd/mmdet_mask_predictor.py): FCNMaskHead's conv_logits
 * (fcn_mask_head.py:135, a 1x1 convolution to C channels) evaluated at each RoI's label channel only - the one channel that
 * mask_cross_entropy (cross_entropy_loss.py:158-162) and get_seg_masks (fcn_mask_head.py:289-290) keep.  The [N, C, HW] logits
 * are never formed.  x [n][cin][hw], IIF_F32 or IIF_BF16, NCHW-contiguous; weight fp32 rows of cin values, ld_w floats apart
 * (>= cin; the row of class k starts at weight + k * ld_w); bias fp32 [c] or NULL; labels int64 [n].  With l = labels[i]:
 *
 * iif_mask_predict_fwd (one launch; two with a target)
 *   z[i, p] = bias[l] + sum_k weight[l, k] * x[i, k, p]           fp32 [n][hw], nullable when a target is given
 *   target (fp32 [n][hw], nullable):  *loss = 1 / (n hw) * sum BCEWithLogits(z, target) (row partials in fp32, their sum in
 *   double), g0[i, p] = (sigmoid(z) - target) / (n hw) (fp32 [n][hw], nullable: the compact gradient the two backward entries
 *   take).  row_loss: scratch of n * ((hw + 63) / 64) floats.  Without a target row_loss and loss are not touched and g0 must be
 *   NULL.  A label outside [0, c) sets bit 0 of *status (device int, caller-zeroed); that RoI gets z = 0, g0 = 0 and adds nothing
 *   to the loss, whose divisor stays n * hw.
 * iif_mask_predict_bwd_input (one launch, no clearing launch)
 *   dx[i, k, p] = up * g[i, p] * weight[l, k]                     dx [n][cin][hw] in `dtype`, EVERY element written once
 *   g fp32 [n][hw]; up: a DEVICE scalar (the upstream gradient of the loss), NULL = 1.  Reads no x.  A label outside [0, c): a
 *   zero slice.
 * iif_mask_predict_bwd_weight (two launches)
 *   scratch[i, k] = up * sum_p g[i, p] * x[i, k, p], scratch[i, cin] = up * sum_p g[i, p]      fp32 [n][cin + 1]
 *   dweight[j, k] = sum over the RoIs with labels[i] == j, in ascending i, of scratch[i, k];  dbias[j] likewise of scratch[i, cin]
 *   dweight fp32 [c][cin] and dbias fp32 [c], either nullable: EVERY row is written, zeros for a class no RoI has.  A label
 *   outside [0, c) contributes nothing.
 * All sums are fp32 in a fixed order without float atomics: the same bits from call to call.  Nothing is allocated or read back.
 * IIF_EINVAL before any launch: a required pointer NULL, n < 0 or > 65535, c < 1, cin outside 1 .. 2048, hw outside 1 .. 4096,
 * ld_w < cin, an unknown dtype.  n == 0: IIF_OK, nothing is enqueued (dweight / dbias are not written). */
int iif_mask_predict_fwd(const void* x, int dtype, const float* weight, int64_t ld_w, const float* bias /* nullable */,
                         const int64_t* labels, const float* target /* nullable */, int n, int c, int cin, int hw,
                         float* z /* nullable */, float* g0 /* nullable */, float* row_loss, float* loss, int* status,
                         void* stream);
int iif_mask_predict_bwd_input(const float* g, const float* up /* nullable */, const float* weight, int64_t ld_w,
                               const int64_t* labels, int n, int c, int cin, int hw, void* dx, int dtype, void* stream);
int iif_mask_predict_bwd_weight(const void* x, int dtype, const float* g, const float* up /* nullable */, const int64_t* labels,
                                int n, int c, int cin, int hw, float* scratch, float* dweight /* nullable */,
                                float* dbias /* nullable */, void* stream);

/* The same predictor fused with the loss, the divisor left to the device (the padded RoI pipeline: rows with a label outside
 * [0, c) are padding).  Operands, limits, errors and launch counts as for the three entries above, with these differences:
 *
 * iif_mask_predict_loss_fwd (two launches): target is required, no z.  g[i, p] = sigmoid(z) - target (fp32 [n][hw], nullable, NOT
 *   divided), *loss = sum BCEWithLogits(z, target) / divisor and *inv_div = 1 / divisor, a device scalar for the backward
 *   entries.  divisor = n * hw, or with valid_rows != 0 max(1, #{i : 0 <= labels[i] < c}) * hw, counted on the device (the
 *   finishing kernel the normed family uses).  A RoI with a label outside [0, c) gets g = 0 and adds nothing to the loss;
 *   its x and target are not read.  No status word.
 * iif_mask_predict_loss_bwd_input / iif_mask_predict_loss_bwd_weight: iif_mask_predict_bwd_input / _bwd_weight with u = up *
 *   inv_div (DEVICE scalars, each nullable = 1) in place of up; the product is formed inside the kernels.
 * In the grids of these three entries block y works on the y-th RoI with a label in [0, c) (the others follow), so the blocks
 * with work are dispatched first; every result is the one the RoI order would give, to the bit. */
int iif_mask_predict_loss_fwd(const void* x, int dtype, const float* weight, int64_t ld_w, const float* bias /* nullable */,
                              const int64_t* labels, const float* target, int n, int c, int cin, int hw, int valid_rows,
                              float* g /* nullable */, float* row_loss, float* loss, float* inv_div, void* stream);
int iif_mask_predict_loss_bwd_input(const float* g, const float* up /* nullable */, const float* inv_div /* nullable */,
                                    const float* weight, int64_t ld_w, const int64_t* labels, int n, int c, int cin, int hw,
                                    void* dx, int dtype, void* stream);
int iif_mask_predict_loss_bwd_weight(const void* x, int dtype, const float* g, const float* up /* nullable */,
                                     const float* inv_div /* nullable */, const int64_t* labels, int n, int c, int cin, int hw,
                                     float* scratch, float* dweight /* nullable */, float* dbias /* nullable */, void* stream);

/* The class-selected mask predictor of the cosine-norm heads (csrc/normed_mask_predictor.hip;
 * iif_amd/mmdet_normed_mask_predictor.py): predictor_cfg=dict(type='NormedConv2d', tempearture=20) - normed_predictor.py:104-124,
 * a 1x1 kernel - evaluated at each RoI's label channel only.  Operands as for iif_mask_predict_*.  With l = labels[i],
 * T = temperature, q = power:  r = |x[i, :, p]|_2, rho = |weight[l, :]|_2, s_x = T / (r^q + eps), s_w = 1 / (rho^q + eps),
 * what = weight[l] * s_w, d = sum_k what[k] * x[i, k, p].
 *
 * iif_normed_mask_predict_fwd (one launch; two with a target)
 *   z[i, p] = s_x * d + bias[l]                                    fp32 [n][hw], nullable when a target is given
 *   coef_a[i, p] = s_x,  coef_b[i, p] = d * T * q * r^(q-2) / (r^q + eps)^2, exactly 0 where r == 0      fp32 [n][hw], nullable:
 *   what the backward entries take.  target (fp32 [n][hw], nullable): g[i, p] = sigmoid(z) - target (fp32 [n][hw], nullable,
 *   NOT divided), *loss = sum BCEWithLogits(z, target) / divisor (row partials in fp32, their sum in double) and
 *   *inv_div = 1 / divisor, a device scalar for the backward entries.  divisor = n * hw, or with valid_rows != 0
 *   max(1, #{i : 0 <= labels[i] < c}) * hw, counted on the device.  row_loss: scratch of n * ((hw + 63) / 64) floats.  Without a
 *   target row_loss, loss and inv_div are not touched and g must be NULL.  A RoI with a label outside [0, c) gets z = g =
 *   coef_a = coef_b = 0, adds nothing to the loss, and its x is not read.
 * iif_normed_mask_predict_bwd_input (one launch)
 *   dx[i, k, p] = u * g[i, p] * (coef_a[i, p] * what[k] - coef_b[i, p] * x[i, k, p]),  u = up * inv_div (DEVICE scalars, each
 *   nullable = 1).  dx [n][cin][hw] in x's dtype, EVERY element written once; x is read once.  A label outside [0, c): a zero
 *   slice, x not read.
 * iif_normed_mask_predict_bwd_weight (two launches)
 *   scratch[i, k] = u * sum_p g[i, p] * coef_a[i, p] * x[i, k, p],  scratch[i, cin] = u * sum_p g[i, p]       fp32 [n][cin + 1]
 *   dwhat[j] = sum over the RoIs with labels[i] == j, in ascending i, of scratch[i, :cin];  dbias[j] likewise of scratch[i, cin]
 *   dweight[j] = s_w * dwhat[j] - (<dwhat[j], weight[j]> * q * rho^(q-2) / (rho^q + eps)^2) * weight[j]   (no second term at rho == 0)
 *   dweight fp32 [c][cin] and dbias fp32 [c], either nullable: EVERY row is written, zeros for a class no RoI has.
 * All sums are fp32 in a fixed order without float atomics: the same bits from call to call.  power == 1 calls no powf.  Nothing
 * is allocated or read back.  IIF_EINVAL before any launch: a required pointer NULL, n < 0 or > 65535, c < 1, cin outside
 * 1 .. 2048, hw outside 1 .. 4096, ld_w < cin, an unknown dtype, power <= 0.  n == 0: IIF_OK, nothing is enqueued. */
int iif_normed_mask_predict_fwd(const void* x, int dtype, const float* weight, int64_t ld_w, const float* bias /* nullable */,
                                const int64_t* labels, const float* target /* nullable */, int n, int c, int cin, int hw,
                                float temperature, float power, float eps, int valid_rows, float* z /* nullable */,
                                float* g /* nullable */, float* coef_a /* nullable */, float* coef_b /* nullable */,
                                float* row_loss, float* loss, float* inv_div, void* stream);
int iif_normed_mask_predict_bwd_input(const void* x, int dtype, const float* g, const float* coef_a, const float* coef_b,
                                      const float* up /* nullable */, const float* inv_div /* nullable */, const float* weight,
                                      int64_t ld_w, const int64_t* labels, int n, int c, int cin, int hw, float power, float eps,
                                      void* dx, void* stream);
int iif_normed_mask_predict_bwd_weight(const void* x, int dtype, const float* g, const float* coef_a,
                                       const float* up /* nullable */, const float* inv_div /* nullable */, const float* weight,
                                       int64_t ld_w, const int64_t* labels, int n, int c, int cin, int hw, float power, float eps,
                                       float* scratch, float* dweight /* nullable */, float* dbias /* nullable */, void* stream);

/* The mask head's tail fused (csrc/mask_tail.hip; iif_amd/mmdet_mask_tail.py): FCNMaskHead's upsample (a ConvTranspose2d with
 * kernel = stride = 2, no padding), its ReLU and conv_logits at each RoI's label channel (fcn_mask_head.py:131-136), on the
 * fp32-input MFMA.  The [n][co][2h][2w] activation between the two layers and its gradient are never stored.
 * f [n][ci][h][w], IIF_F32 or IIF_BF16, NCHW-contiguous; up_weight fp32 [ci][co][2][2] contiguous; up_bias fp32 [co] or NULL;
 * weight fp32 rows of co values, ld_w floats apart (>= co); bias fp32 [c] or NULL; labels int64 [n].  With l = labels[i],
 * P = (2y + a, 2x + b):
 *   pre[i, k, P] = up_bias[k] + sum_m f[i, m, y, x] * up_weight[m, k, a, b],   z[i, P] = bias[l] + sum_k weight[l, k] * max(pre, 0)
 *
 * iif_mask_tail_fwd (one launch; two with a target)
 *   z fp32 [n][2h][2w], nullable when a target is given.  target (fp32 [n][2h][2w], nullable): *loss = 1 / (4 n h w) * sum
 *   BCEWithLogits(z, target), g0 = (sigmoid(z) - target) / (4 n h w) (fp32 [n][2h][2w], nullable).  row_loss: scratch of
 *   n * ((h w + 63) / 64) floats.  Without a target row_loss and loss are not touched and g0 must be NULL.  A label outside
 *   [0, c) sets bit 0 of *status (device int, caller-zeroed); that RoI gets z = 0, g0 = 0 and adds nothing to the loss, whose
 *   divisor stays 4 n h w.
 * iif_mask_tail_bwd_rows (one launch): recomputes pre for the gradient g fp32 [n][2h][2w] (times the DEVICE scalar up, NULL = 1)
 *   signs[i][t][j]: bit q of the word is pre[i, k, P] > 0 for input pixel 32 t + q and j = 4 k + 2 a + b;
 *                   n * ((h w + 31) / 32) * 4 co words, which the two entries below read
 *   rows[i, k] = up * sum_P g[i, P] * max(pre[i, k, P], 0), rows[i, co] = up * sum_P g[i, P]      fp32 [n][co + 1], nullable
 * iif_mask_tail_bwd_input (one launch, no clearing launch)
 *   df[i, m, y, x] = sum_{k,a,b} dpre[i, k, P] * up_weight[m, k, a, b],  dpre = up * g[i, P] * weight[l, k] * [pre > 0]
 *   df [n][ci][h][w] in `dtype`, EVERY element written once.  up_weight must be 16-byte aligned (IIF_EUNSUPPORTED otherwise).
 * iif_mask_tail_bwd_params (two launches)
 *   dup_weight[m, k, a, b] = sum_{i,y,x} f * dpre, dup_bias[k] = sum dpre (either nullable): the RoIs are cut into
 *   iif_mask_tail_splits(n, ci, co) ranges, one partial each, summed in range order.  partial: scratch of
 *   splits * (ci + 1) * 4 co floats.
 * iif_mask_tail_bwd_classes (one launch): dweight[j, k] = sum over the RoIs with labels[i] == j, in ascending i, of rows[i, k];
 *   dbias[j] likewise of rows[i, co].  dweight fp32 [c][co], dbias fp32 [c], either nullable: EVERY row is written.
 * A label outside [0, c) gives a zero df slice and contributes nothing to any parameter gradient.  All sums are fp32 in a fixed
 * order without float atomics: the same bits from call to call.  Nothing is allocated or read back.
 * IIF_EINVAL before any launch: a required pointer NULL, n < 0 or > 65535, c < 1, ci or co outside 1 .. 1024, h or w < 1,
 * h * w > 1024, ld_w < co, a dtype other than IIF_F32 / IIF_BF16.  n == 0: IIF_OK, nothing enqueued. */
int iif_mask_tail_fwd(const void* f, int dtype, const float* up_weight, const float* up_bias /* nullable */, const float* weight,
                      int64_t ld_w, const float* bias /* nullable */, const int64_t* labels, const float* target /* nullable */,
                      int n, int c, int ci, int co, int h, int w, float* z /* nullable */, float* g0 /* nullable */,
                      float* row_loss, float* loss, int* status, void* stream);
int iif_mask_tail_bwd_rows(const void* f, int dtype, const float* up_weight, const float* up_bias /* nullable */, const float* g,
                           const float* up /* nullable */, const int64_t* labels, int n, int c, int ci, int co, int h, int w,
                           unsigned int* signs, float* rows /* nullable */, void* stream);
int iif_mask_tail_bwd_input(const float* g, const float* up /* nullable */, const float* up_weight, const float* weight,
                            int64_t ld_w, const int64_t* labels, const unsigned int* signs, int n, int c, int ci, int co, int h,
                            int w, void* df, int dtype, void* stream);
int iif_mask_tail_splits(int n, int ci, int co);
int iif_mask_tail_bwd_params(const void* f, int dtype, const float* g, const float* up /* nullable */, const float* weight,
                             int64_t ld_w, const int64_t* labels, const unsigned int* signs, int n, int c, int ci, int co, int h,
                             int w, float* partial, float* dup_weight /* nullable */, float* dup_bias /* nullable */,
                             void* stream);
int iif_mask_tail_bwd_classes(const float* rows, const int64_t* labels, int n, int c, int co, float* dweight /* nullable */,
                              float* dbias /* nullable */, void* stream);

/* The tail fused with the loss, the divisor left to the device, as iif_mask_predict_loss_* above.  Operands, limits, errors and
 * launch counts as for the iif_mask_tail_* entries, with these differences:
 *
 * iif_mask_tail_loss_fwd (two launches): target is required, no z.  g = sigmoid(z) - target (fp32 [n][2h][2w], nullable, NOT
 *   divided), *loss = sum BCEWithLogits(z, target) / divisor, *inv_div = 1 / divisor (device scalar).  divisor = 4 n h w, or with
 *   valid_rows != 0 max(1, #{i : 0 <= labels[i] < c}) * 4 h w, counted on the device.  A RoI with a label outside [0, c) gets
 *   g = 0 and adds nothing; its f and target are not read.  No status word.
 * iif_mask_tail_loss_bwd_rows / _bwd_input / _bwd_params: the iif_mask_tail_bwd_* entries with u = up * inv_div (DEVICE scalars,
 *   each nullable = 1) in place of up; the product is formed inside the kernels.  iif_mask_tail_bwd_classes and
 *   iif_mask_tail_splits serve both.  Forward, rows and df put the RoIs with a label in [0, c) first in their grids, as above. */
int iif_mask_tail_loss_fwd(const void* f, int dtype, const float* up_weight, const float* up_bias /* nullable */,
                           const float* weight, int64_t ld_w, const float* bias /* nullable */, const int64_t* labels,
                           const float* target, int n, int c, int ci, int co, int h, int w, int valid_rows, float* g /* nullable */,
                           float* row_loss, float* loss, float* inv_div, void* stream);
int iif_mask_tail_loss_bwd_rows(const void* f, int dtype, const float* up_weight, const float* up_bias /* nullable */,
                                const float* g, const float* up /* nullable */, const float* inv_div /* nullable */,
                                const int64_t* labels, int n, int c, int ci, int co, int h, int w, unsigned int* signs,
                                float* rows /* nullable */, void* stream);
int iif_mask_tail_loss_bwd_input(const float* g, const float* up /* nullable */, const float* inv_div /* nullable */,
                                 const float* up_weight, const float* weight, int64_t ld_w, const int64_t* labels,
                                 const unsigned int* signs, int n, int c, int ci, int co, int h, int w, void* df, int dtype,
                                 void* stream);
int iif_mask_tail_loss_bwd_params(const void* f, int dtype, const float* g, const float* up /* nullable */,
                                  const float* inv_div /* nullable */, const float* weight, int64_t ld_w, const int64_t* labels,
                                  const unsigned int* signs, int n, int c, int ci, int co, int h, int w, float* partial,
                                  float* dup_weight /* nullable */, float* dup_bias /* nullable */, void* stream);

/* Non-maximum suppression (mmcv 1.3.8 ops/nms.py nms / batched_nms; iif_amd/mmdet_nms.py) in 5 enqueued operations for any N and
 * any data: a 4 KiB clear, the sort keys, the rank, the suppression bit matrix, the greedy scan (csrc/nms.hip).
 * boxes [N] rows of (x1, y1, x2, y2, ...) fp32, ld_boxes floats apart (>= 4), read in place; scores [N] fp32.
 *   rank     score descending, equal scores to the LOWER index (mmcv's sort is unstable: any tie order is one of its outputs).
 *   test     box b is suppressed by a kept box a of higher rank when inter / (Sa + Sb - inter) > iou_threshold, with
 *            w = max(min(a.x2, b.x2) - max(a.x1, b.x1) + offset, 0), h likewise, inter = w * h, S = (x2 - x1 + offset) *
 *            (y2 - y1 + offset): single float32 operations in this order; a NaN quotient does not suppress.  offset: 0 or 1.
 *   scan     mmcv's: walk the ranked list, keep a box unless a box KEPT earlier suppresses it.
 *   ids      int64 [N], read for id_mode != 0.  1: every coordinate gets id * (max over all coordinates of `boxes` + 1) added in
 *            float32 (the maximum is reduced on the device) and every pair is tested on the shifted boxes - batched_nms below
 *            split_thr, including its quirk that boxes of different ids can meet when coordinates lie below -1.  2: the same
 *            shifted boxes, pairs of equal id only - batched_nms at or above split_thr (a plain NMS per id, merged by rank).
 *            Ids must lie in the int32 range: they are narrowed to int32 before the conversion to float (mmcv converts the int64
 *            directly); the module's callers pass class or level numbers.  The maximum is reduced with fmaxf: a NaN coordinate
 *            is dropped from it, where torch's max would make every shift NaN.  NaN coordinates are not reproduced.
 *   score_threshold > 0: boxes with score <= score_threshold take no part (mmcv filters only for a threshold above 0).
 *   max_num > 0: the scan stops after max_num kept boxes.
 * keep: int64 [cap], cap = max_num > 0 ? min(max_num, N) : N: the kept input indices in rank order, then -1.  dets (nullable):
 * fp32 [cap][5] = the kept boxes as given (unshifted) and their scores, then zeros.  count: int64 [1].
 * d_workspace: IIF_NMS_WORKSPACE_BYTES(1, N) on a 16-byte boundary; it belongs to the call until the stream has run it.  Its
 * contents on entry do not matter.  Allocates nothing, reads nothing back; integer atomics only.
 * IIF_EINVAL before anything is enqueued: N < 0 or > IIF_NMS_MAX_BOXES (the matrix is N^2 / 8 bytes: 32 MiB there), ld_boxes < 4,
 * id_mode outside 0 .. 2, offset outside 0 .. 1, a NaN threshold, a null or misaligned count, and for N > 0 a null boxes / scores /
 * keep (ids with id_mode != 0) or a null, misaligned or short workspace.  N == 0: count = 0 (one operation). */
#define IIF_NMS_MAX_BOXES 16384
#define IIF_NMS_WORKSPACE_BYTES(B, N) (4096 + (int64_t)(B) * (659456 + (((int64_t)(N) + 63) / 64 * 64) * (64 + (((int64_t)(N) + 63) / 64 * 64) / 8)))
int iif_nms(const float* boxes, int64_t ld_boxes, const float* scores, const int64_t* ids /* int64 [N] or NULL */, int64_t N,
            int id_mode, float iou_threshold, int offset, float score_threshold, int64_t max_num, int64_t* keep,
            float* dets /* nullable */, int64_t* count, void* d_workspace, int64_t workspace_bytes, void* stream);

/* The RPN proposal step (mmdet models/dense_heads/rpn_head.py:79-225 with the sigmoid classifier) for B images and all levels
 * in 10 enqueued operations, whatever B, the number of levels and the data: a clear, five radix-select passes, the gather with
 * decode, then the rank, matrix and scan of the NMS entry for all images at once.
 * levels: a HOST array of num_levels (1 .. 8) descriptors, copied into the launches.  scores is the head's [B, A, H, W] output and
 * deltas its [B, 4 A, H, W] output, both fp32 and read IN PLACE through their four element strides (NCHW and channels_last both
 * work); anchors [A H W] rows of 4 floats, ld_anchors apart, in the order of the flattened index (h * W + w) * A + a.
 * Per image and level the nms_pre largest logits are taken, equal logits to the lower flattened index; a level with at most nms_pre
 * anchors, or nms_pre <= 0, gives all of them.  (Sigmoid is monotone, so this is the reference's selection by score wherever the
 * float32 sigmoid keeps distinct logits distinct.)  The candidates are decoded with the arithmetic of the delta2bbox entry (the
 * same device function) against max_shape = img_hw[b] (a HOST array of B pairs (max_h, max_w); clip: the coder's clip_border);
 * score = 1 / (1 + expf(-logit)); with min_bbox_size >= 0 a candidate takes part only if w > min_bbox_size && h > min_bbox_size.
 * The NMS is batched_nms with the level as id, ALWAYS id_mode 1 above (the reference switches to a per-level NMS when split_thr
 * or more candidates take part: the caller keeps Ncand below its split_thr, as iif_amd/mmdet_nms.py does; the maximum runs over
 * the candidates that take part), ranked by
 * (logit descending, index into the concatenated anchors ascending).
 * dets: fp32 [B][max_per_img][5], the kept boxes and scores in rank order, then zeros; counts: int64 [B].
 * cand_* (cand_index NULL: none; the others nullable): the RANKED candidates of every image, Ncand = sum over the levels of
 * min(nms_pre, A H W) each, those that take no part behind the others: cand_index int64 [B][Ncand] (index into the concatenated
 * anchors), cand_boxes fp32 [B][Ncand][4] (16-byte aligned), cand_scores fp32, cand_level int32, cand_valid int8.
 * d_workspace: IIF_NMS_WORKSPACE_BYTES(B, Ncand) on a 16-byte boundary, contents on entry do not matter.
 * IIF_EINVAL before anything is enqueued: a null levels / img_hw / means / stds / dets / counts, num_levels outside 1 .. 8, B outside
 * 1 .. 16, max_per_img < 1, offset outside 0 .. 1, a NaN threshold or size, a level with a null or misaligned pointer, A / H / W < 1
 * or ld_anchors < 4, Ncand > IIF_NMS_MAX_BOXES, 2^24 or more anchors per image, a null, misaligned or short workspace. */
typedef struct iif_rpn_level {
    const float* scores;
    const float* deltas;
    const float* anchors;
    int64_t score_strides[4];
    int64_t delta_strides[4];
    int64_t ld_anchors;
    int32_t A, H, W, reserved;
} iif_rpn_level;
int iif_rpn_proposals(const iif_rpn_level* levels, int num_levels, int B, const float* img_hw, int nms_pre, int max_per_img,
                      float min_bbox_size, float iou_threshold, int offset, const float* means, const float* stds, float max_ratio,
                      int add_ctr_clamp, float ctr_clamp, int clip, float* dets, int64_t* counts, int64_t* cand_index /* nullable */,
                      float* cand_boxes, float* cand_scores, int32_t* cand_level, int8_t* cand_valid, void* d_workspace,
                      int64_t workspace_bytes, void* stream);

/* mmdet's multiclass_nms (core/post_processing/bbox_nms.py:8-95; iif_amd/mmdet_multiclass_nms.py) for B images of R padded rows
 * and C foreground classes each, in 12 enqueued operations whatever the sizes and the data (csrc/multiclass_nms.hip): a clear,
 * the filter, the rank and walk of the all-pairs regime, the per-class walk, six selection passes, the finish.
 * scores fp32 [B][R] rows of C + 1 values, ld_scores floats apart (>= C + 1); the last column (background) is never read.
 * boxes fp32 [B][R] rows, ld_boxes floats apart: 4 C values (boxes_per_class != 0, box c at 4 c) or 4 values shared by the classes.
 * score_factors (nullable) fp32 [B][R]; row_counts (nullable) int64 [B] on the DEVICE: rows at or beyond it take no part.
 *   candidates  (r, c) with flat index f = r * C + c takes part iff score[r, c] > score_thr (strict, the raw score).  Its ranked
 *               score is score[r, c] * factor[r] (one float32 multiply; the score itself without factors).  M = how many take part.
 *   regime      decided on the device.  0 < M < split_thr: mmcv's nms over ALL pairs of the shifted boxes box + float(c) * (max + 1),
 *               max over all coordinates of the boxes that take part, formed in float32 - including mmcv's quirk that boxes of
 *               different classes can meet when coordinates lie below -1.  M >= split_thr: one plain NMS per class on the same
 *               shifted boxes, merged by score.  The rank, the overlap test and the walk are those of iif_nms above: ranked score
 *               descending, equal scores to the lower f; single float32 operations; a NaN quotient does not suppress.
 *   cap         the result is the first cap of the ranked kept candidates (the caller folds nms_cfg['max_num'] and max_num into it).
 * dets fp32 [B][cap][5]: the kept UNSHIFTED boxes and ranked scores in rank order, then zeros.  labels int64 [B][cap]: c, then
 * -1.  inds int64 [B][cap]: f, then -1.  counts int64 [B].  num_candidates (nullable) int64 [B]: M.
 * d_workspace: IIF_MULTICLASS_NMS_WORKSPACE_BYTES(B, R, C, cap) on a 16-byte boundary; it belongs to the call until the stream has
 * run it; its contents on entry do not matter.  Allocates nothing, reads nothing back; integer atomics only; the result does not
 * depend on their arrival order.
 * IIF_EINVAL before anything is enqueued: B outside 1 .. 16, R outside 0 .. IIF_MULTICLASS_NMS_MAX_ROWS, C outside
 * 1 .. IIF_MULTICLASS_NMS_MAX_CLASSES, R C >= 2^24, cap outside 1 .. IIF_MULTICLASS_NMS_MAX_CAP, offset outside 0 .. 1, a NaN
 * threshold, a row pitch smaller than the row, split_thr > IIF_NMS_MAX_BOXES while R C exceeds it (the all-pairs regime holds
 * IIF_NMS_MAX_BOXES candidates), a null or misaligned scores / boxes / output, a null, misaligned or short workspace. */
#define IIF_MULTICLASS_NMS_MAX_ROWS 1024
#define IIF_MULTICLASS_NMS_MAX_CLASSES 4096
#define IIF_MULTICLASS_NMS_MAX_CAP 4096
#define IIF_MULTICLASS_NMS_WORKSPACE_BYTES(B, R, C, cap) (4096 + (int64_t)(B) * (212992 + 4 * (((int64_t)(C) + 3) / 4 * 4) + 16 * (int64_t)(R) * (int64_t)(C) + 8 * (int64_t)(cap)))
int iif_multiclass_nms(const float* boxes, int64_t ld_boxes, int boxes_per_class, const float* scores, int64_t ld_scores,
                       const float* score_factors /* nullable */, const int64_t* row_counts /* nullable */, int B, int64_t R, int64_t C,
                       float score_thr, float iou_threshold, int offset, int64_t split_thr, int64_t cap, float* dets,
                       int64_t* labels, int64_t* inds, int64_t* counts, int64_t* num_candidates /* nullable */, void* d_workspace,
                       int64_t workspace_bytes, void* stream);

/* CIFAR training input (iif_amd/cifar.py DeviceCIFARLoader): ONE launch per batch builds out[b] (fp32 NCHW [batch][3][32][32])
 * and targets[b] = labels[index[b]] from the device-resident dataset data (uint8 [n][3][32][32], the planar rows of the
 * CIFAR files) and labels (int64 [n]).  flags select the stages, applied in the reference's order (initialisers.py:116-134):
 *   IIF_CIFAR_CROP_FLIP  pad 4 with 0, random 32x32 crop, horizontal flip with p 0.5
 *   IIF_CIFAR_POLICY     on the [0, 1] image, one of the 25 CIFAR10Policy sub-policies of iif_amd/augment.py; policy is the
 *                        device table of per-(sub-policy, op, sign) constants, uint32 [25][2][2][8] (cifar.policy_table)
 *   IIF_CIFAR_CUTOUT     Cutout(1, 16): centre uniform in 0..31, the clipped 16x16 box set to 0 before normalisation
 * then always (x - mean) / std with the reference's CIFAR mean (0.4914, 0.4822, 0.4465) and std (0.2023, 0.1994, 0.2010).
 * Randomness: a counter-based hash (splitmix64 finaliser) of (seed, epoch, rank, pos0 + b, draw slot): no host RNG, the
 * same arguments give the same batch.  params (nullable) receives the draws, int32 [batch][10]: crop y, crop x, flip,
 * sub-policy, op 0 applied, op 0 sign positive, op 1 applied, op 1 sign positive, cutout centre y, x.
 * An index outside [0, n) reads nothing: out[b] = 0 and targets[b] = -1.
 * IIF_EINVAL before any launch: a null data / labels / index / out / targets (or policy with IIF_CIFAR_POLICY), n <= 0,
 * batch < 0, pos0 < 0, unknown flag bits. */
#define IIF_CIFAR_CROP_FLIP 1u
#define IIF_CIFAR_POLICY 2u
#define IIF_CIFAR_CUTOUT 4u
int iif_cifar_augment(const uint8_t* data, int64_t n, const int64_t* labels, const int64_t* index, int64_t batch,
                      int64_t pos0, uint64_t seed, int64_t epoch, int64_t rank, uint32_t flags, const uint32_t* policy,
                      float* out, int64_t* targets, int32_t* params, void* stream);

/* List-dataset input (ImageNet-LT / Places-LT / iNaturalist-18; iif_amd/lt_device.py DeviceLTLoader): ONE launch per batch
 * builds out[b] (fp32 NCHW [batch][size][size] per channel, 3 channels) from source regions the host decoded and cut out,
 * in TensorTransform's order (iif_amd/imbalanced_dataset.py):
 *   antialiased bilinear resize of the region to rh x rw (interpolate(mode="bilinear", antialias=True,
 *   align_corners=False): triangle filter of support max(scale, 1), window clipped to the region, weights renormalised),
 *   of which only the size x size window at (oy, ox) is formed; then the horizontal flip of that window;
 *   IIF_LT_JITTER        on the [0, 1] image (clamped), ColorJitter's brightness / contrast / saturation / hue in the
 *                        recorded order with the recorded factors (augment.ColorJitter.apply; contrast blends toward the
 *                        grey mean of the image as it stands when contrast runs; a zero hue shift is skipped)
 * then always (x - mean) / std.
 * pool: uint8, every region HWC with 3 channels, packed back to back; pool_bytes its size.
 * desc: int64 [batch][8] = byte offset in pool, region height, width, rh, rw, oy, ox, flip (non-zero: flipped).
 * jitter (needed with IIF_LT_JITTER): uint32 [batch][8] = the order (bits 2k..2k+1: the op at position k; 0 brightness,
 *   1 contrast, 2 saturation, 3 hue), then the fp32 bits of fb, 1 - fb, fc, 1 - fc, fs, 1 - fs, fh.  Factor 1 (and
 *   1 - f = 0) leaves brightness / contrast / saturation out; fh = 0 leaves hue out.
 * mean_std: 6 floats in HOST memory, mean then std per channel.
 * A descriptor that reaches outside the pool, has a non-positive size, or a window outside rh x rw reads nothing: out[b] = 0.
 * IIF_EINVAL before any launch: a null pool / desc / mean_std / out (or jitter with IIF_LT_JITTER), pool_bytes < 0,
 * batch < 0, size <= 0 or > 16384, unknown flag bits. */
#define IIF_LT_JITTER 1u
int iif_lt_augment(const uint8_t* pool, int64_t pool_bytes, const int64_t* desc, const uint32_t* jitter, int64_t batch,
                   int size, const float* mean_std, uint32_t flags, float* out, void* stream);

/* List-dataset training input with an auto-augment policy (iif_amd/lt_device.py DeviceLTLoader(policy=...)): ONE launch per
 * batch builds out[b] as iif_lt_augment does without IIF_LT_JITTER, with up to two auto-augment operations between the flip
 * and Normalize, in TensorTransform's order:
 *   resize / window / flip (the same values as iif_lt_augment) -> clamp(0, 1) -> the op of record slot 0, then of slot 1
 *   (augment.apply_op_signed: the affine ops as PIL's nearest-neighbour mapping at pixel centres with grey 128 / 255 fill;
 *   Posterize / Solarize / Equalize through uint8 levels, Equalize by PIL's LUT rule; AutoContrast by channel min / max;
 *   Contrast toward the grey mean; Sharpness with the (1 1 1; 1 5 1; 1 1 1) / 13 blur, borders kept) -> (x - mean) / std.
 * pool, desc, mean_std: as iif_lt_augment.
 * ops: uint32 [batch][2][8], one record per op slot: word 0 the op code (the index in iif_amd/cifar.py OPS: ShearX, ShearY,
 *   TranslateX, TranslateY, Rotate, Color, Posterize, Solarize, Contrast, Sharpness, Brightness, AutoContrast, Equalize,
 *   Invert) or IIF_LT_OP_NONE; words 1..6 its constants as cifar.policy_table encodes them at h = w = size (the fp32 bits of
 *   the affine a .. f or of the blend's (f, 1 - f); the posterize mask or solarize threshold as an integer); word 7 unused.
 * work, out: fp32 [batch][3][size][size] each, distinct; work is scratch (the block keeps its image there between sweeps).
 * A malformed descriptor (as iif_lt_augment) or an unknown op code reads nothing: out[b] = 0.
 * IIF_EINVAL before any launch: a null pool / desc / ops / mean_std / work / out, pool_bytes < 0, batch < 0,
 * size <= 0 or > 16384.  batch == 0: IIF_OK, no launch. */
#define IIF_LT_OP_NONE 0xFFu
int iif_lt_augment_policy(const uint8_t* pool, int64_t pool_bytes, const int64_t* desc, const uint32_t* ops, int64_t batch,
                          int size, const float* mean_std, float* work, float* out, void* stream);

/* Baseline JPEG decoding (iif_amd/jpeg.py; DeviceLTLoader(decode="device"), --device-decode): TWO launches turn the
 * entropy-coded scans of n images into uint8 HWC regions with 3 channels, equal byte for byte to libjpeg's default decode
 * (ISLOW IDCT, fancy upsampling, jdcolor's YCbCr -> RGB; grey repeated), each cropped to its record's box:
 *   one workgroup per image destuffs its scan, decodes it in parallel (one thread per restart interval, or self-synchronising
 *   bit subsequences of subseq_bits bits), dequantises and inverse-transforms the blocks the box needs; then the pixel
 *   launch upsamples the chroma, converts and stores.
 * data: uint8, data_bytes long, 16-byte aligned: what the records point into.
 * rec: int64 [n][IIF_JPEG_REC_WORDS] (device memory): byte offset in data of the scan (16-aligned; the bytes after the SOS
 *   header, markers and stuffing included) and its length, offset of the table block (16-aligned: int16 [3][64]
 *   quantisation tables in natural order, then 6 Huffman lookup tables of 1424 bytes: uint16 [512] 9-bit table (code
 *   length << 8 | symbol, 0: a longer code), int32 [18] maxcode, int32 [18] symbol offset, uint8 [256] symbols), height,
 *   width, components (1, or 3 in one interleaved YCbCr scan), the luma sampling factors h, v (1x1, 2x1, 2x2), restart
 *   interval in MCUs (0: none), box top, left, height, width, byte offset of the region in out, byte offset of the image's
 *   scratch (16-aligned) and its size (iif_amd/jpeg.py scratch_bytes), then one word per component: DC slot | AC slot << 4;
 *   the other words are unused.
 * scratch: uint8, 16-byte aligned, scratch_bytes long.  out: uint8, out_bytes long.  status: int32 [n], written for every
 *   image: IIF_JPEG_OK or why it was not decoded.
 * A record that reaches outside data, out or scratch, or whose geometry is invalid, reads nothing and gets the status
 * IIF_JPEG_BAD_RECORD; its region is filled with IIF_JPEG_FILL when the region's offset and size lie inside out.  A malformed scan (an invalid code, a coefficient index past 63, a scan that ends before the
 * box's last MCU, a missing restart marker) fills that image's region with IIF_JPEG_FILL; the other images are exact.
 * IIF_EINVAL before any launch: a null pointer, data or scratch not 16-byte aligned, a negative size, n < 0 or > 65535,
 * subseq_bits < 32 or > 2^24.  n == 0: IIF_OK, no launch. */
#define IIF_JPEG_REC_WORDS 32
#define IIF_JPEG_FILL 128
#define IIF_JPEG_OK 0
#define IIF_JPEG_BAD_RECORD 1
#define IIF_JPEG_BAD_CODE 2
#define IIF_JPEG_OVERFLOW 3
#define IIF_JPEG_TRUNCATED 4
#define IIF_JPEG_NO_RESTART 5
int iif_jpeg_decode(const uint8_t* data, int64_t data_bytes, const int64_t* rec, int64_t n, uint8_t* scratch,
                    int64_t scratch_bytes, uint8_t* out, int64_t out_bytes, int subseq_bits, int32_t* status, void* stream);

/* Compute-unit budget of the persistent grids (the weights-in-registers kernels, the stem, the streaming 1x1 kernel size their
 * grids to one or two resident blocks per CU).  Process-wide, default 0 = every CU of the device; a rank whose gradient
 * all-reduce (RCCL kernels, classification/train.py:230-234 DDP) overlaps backward sets e.g. 240 so that the reduction's
 * channels find free CUs instead of queueing behind a resident grid.  Rounded down to a multiple of 8, at least 64.
 * iif_get_cu_budget: the count the next persistent launch will use. */
int iif_set_cu_budget(int cus);
int iif_get_cu_budget(void);
/* Blocks of a persistent grid that is launched in whole units of `unit` blocks (8 * S: the S column slices of eight tile
 * sequences, one sequence per XCD), before the layer's own tile and row counts bound it.  With n = the device's CUs and
 * b = iif_get_cu_budget(): g = b / unit * unit, the largest whole-unit count within the budget - unless that rounding gives up
 * more CUs than the reservation asked for, b - g > n - b, in which case the launch keeps the device's whole-unit grid,
 * n / unit * unit.  (n = 256, b = 240: units of 8, 16, 32 give 240, 240, 224; units of 64 and 128 keep 256.)  The result may
 * be 0 (b = 64, unit 128): such a launch takes the tile kernels.  unit <= 0: b.  A host function; no device is needed (256 CUs
 * are assumed without one). */
int iif_persistent_grid_blocks(int unit);

#ifdef __cplusplus
}
#endif
#endif /* IIF_AMD_H */
