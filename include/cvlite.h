/*
 * cvlite — C ABI of the MI355X (gfx950) detector-training hot path.
 *
 * Drop-in boundary for the numeric work that WD-Leong/CV-Lite-Object-Detection does in
 * TF2-eager ops and numpy loops (the reference has no FFI of its own).  Each entry
 * point below names the reference function it replaces.  The Python host layer
 * (cv-lite-object-detection_amd/cvlite) binds these with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions (all functions):
 *  - every pointer is a DEVICE pointer unless the parameter says "host";
 *  - the caller allocates every buffer, including workspaces (query *_workspace_size first);
 *    the library allocates nothing and keeps no pointer past return;
 *  - all work is enqueued on `stream` (a hipStream_t); nothing synchronises;
 *  - return value: CVL_OK, CVL_EINVAL (bad argument; nothing enqueued) or CVL_EHIP + hipError_t;
 *  - stateless and re-entrant; safe to capture into a hipGraph.
 *  - tensors are row-major; activations NHWC; "bf16" = raw uint16 bfloat16 bits.
 */
#ifndef CVLITE_H_
#define CVLITE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* cvl_stream_t; /* hipStream_t */

enum { CVL_OK = 0, CVL_EINVAL = 1, CVL_EHIP = 1000 };

int cvl_version(void);

/* ------------------------------------------------------------------------------------------
 * FCOS target assignment.  Replaces FCOS/fcos.py:136-378 `format_data` (per image, numpy loops)
 * with one batched launch.  boxes[b, i] = (yc, xc, h, w, class) normalised to img_dim[b] (the
 * unpadded size, fp32, as data_preprocess.resize_and_pad_image returns it); only the first
 * nbox[b] rows of image b are used.  Output targets[b, p, 0:5+C] float32, p running level-major
 * over the 5 maps of size (pad_h/stride_l) x (pad_w/stride_l) (row-major inside a level); this is
 * the reference's list of 5 float64 maps rounded to fp32 (bit-exact).  num_targets[b, l] int32.
 * strides[5], size_bounds[4] are host arrays (reference defaults {8,16,32,64,128}, {32,64,128,256}).
 * ---------------------------------------------------------------------------------------- */
int cvl_fcos_assign(const float* boxes, const int32_t* nbox, const float* img_dim, int B, int n_max,
                    int pad_h, int pad_w, int num_classes, const int32_t* strides /*host[5]*/,
                    const float* size_bounds /*host[4]*/, float* targets, int32_t* num_targets,
                    cvl_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused FCOS loss forward + backward.  Replaces FCOS/fcos.py:380-496 (`focal_loss`,
 * `smooth_l1_loss`, `iou_loss`, `model_loss`; alpha 0.25, gamma 2, plain sums) and the matching
 * GradientTape backward.  Per cell p of image b:
 *   reg_pred[(b*P+p)*ld_reg + 0..4] = (t, b, l, r, centerness-logit)
 *   cls_pred[(b*P+p)*ld_cls + 0..C-1] = class logits
 *   targets[(b*P+p)*(5+C) + ...] as produced by cvl_fcos_assign.
 * losses[b*3 + {0,1,2}] = (cls, reg, cen) float32 sums for image b (model_loss's tuple).
 * If d_reg / d_cls are non-null, writes grad_scale * d(cls+reg+cen)/d(pred) with the same
 * strides (padding channels zeroed); *_dtype 0 = float32, 1 = bf16.
 * reg_type bits 0-1: 0 = "l1" (smooth-L1), 1 = "iou"; flags for the centre variants: +4 focal
 * centerness (fcos_center.py:386-389 cen_type="focal", fcos_center_v1.py:305-307), +8 smooth-L1 on
 * sigmoid(reg[:4]) (fcos_center_v1.py:115, l1 only), +16 the centerness logit / gradient is column
 * round_up(C, 8) of the class rows (cen_output_l lives on the cls tower).
 * `workspace` >= cvl_fcos_loss_workspace_size(B, P) bytes, passed as `workspace_bytes`
 * (CVL_EINVAL when smaller: the size grew in round 5 to 64-cell tiles, so a buffer sized by an
 * older formula is rejected instead of overrun).
 * ---------------------------------------------------------------------------------------- */
size_t cvl_fcos_loss_workspace_size(int B, int P);
int cvl_fcos_loss(const float* reg_pred, int ld_reg, const float* cls_pred, int ld_cls,
                  const float* targets, int B, int P, int num_classes, int reg_type,
                  float grad_scale, float* losses, void* d_reg, int ld_dreg, int dreg_dtype,
                  void* d_cls, int ld_dcls, int dcls_dtype, void* workspace, size_t workspace_bytes,
                  cvl_stream_t stream);
/* cvl_fcos_loss with the loss keywords of FCOS/fcos.py:380 smooth_l1_loss(delta) and :443-444
 * focal_loss(alpha, gamma) (RetinaNet/retinanet_module.py:367-401 has the same two), and one more
 * reg_type flag: +32 the regression mask is the float value targets[5] itself instead of
 * (max class target >= 1) -- the drop-in smooth_l1_loss / iou_loss(mask=<float map>) (C = 1).
 * cvl_fcos_loss(...) == cvl_fcos_loss_ex(..., 0.25f, 2.0f, 1.0f, ...).  gamma >= 0, delta > 0. */
int cvl_fcos_loss_ex(const float* reg_pred, int ld_reg, const float* cls_pred, int ld_cls,
                     const float* targets, int B, int P, int num_classes, int reg_type,
                     float grad_scale, float alpha, float gamma, float delta, float* losses, void* d_reg,
                     int ld_dreg, int dreg_dtype, void* d_cls, int ld_dcls, int dcls_dtype, void* workspace,
                     size_t workspace_bytes, cvl_stream_t stream);

/* FCOS/fcos.py:112-134 prediction_to_corners: pred [S0][S1][ld>=4] (t, b, l, r) fp32 ->
 * out [S0][S1][4] float64 = stride * (y_lo, x_lo, y_hi, x_hi) around cell centres (fp32 math). */
int cvl_fcos_decode(const float* pred, int ld, int S0, int S1, double stride, double* out,
                    cvl_stream_t stream);
/* FCOS/fcos_center_v1.py:124-147 prediction_to_corners(xy_pred, box_sc, stride): pred [S0][S1][ld>=4]
 * (y_off, x_off, h, w) fp32 -> out [S0][S1][4] float64 corners of the box centred at
 * ((cell + off) * stride) with size (h, w) * box_sc (fp32 arithmetic, stored as float64). */
int cvl_fcos_v1_decode(const float* pred, int ld, int S0, int S1, float box_sc, float stride, double* out,
                       cvl_stream_t stream);


/* FCOS/fcos_center.py:149-317 format_data (the variant of train_fcos_center_voc.py): level by
 * max(h, w) px against b_dim [4] (HOST, reference default {32,64,128,256}); per level, boxes in
 * ascending area paint the 3x3 cells around int(centre * img_dim / stride + 0.5) (only the centre
 * cell when center_only): centerness = max(1 / 0.5 / 0.25), ltrb = last box's offsets about the
 * cell centre (unclamped), class bits OR-ed.  Layout as cvl_fcos_assign: targets [B][P][5+C]
 * level-major over (pad_h/stride) x (pad_w/stride) maps, num_targets [B][5]; strides [5] HOST. */
int cvl_fcos_center_assign(const float* boxes, const int32_t* nbox, const float* img_dim, int B, int n_max,
                           int pad_h, int pad_w, int num_classes, const int32_t* strides, const float* b_dim,
                           int center_only, float* targets, int32_t* num_targets, cvl_stream_t stream);
/* FCOS/fcos_center_v1.py:149-281 format_data (train_fcos_center_v1_voc.py): same level selection and
 * ascending-area order as cvl_fcos_center_assign; each box writes ONLY its centroid cell
 * (int(centre * img_dim / stride)): (y_off, x_off, h / box_sc, w / box_sc) of the last box there,
 * centre score 1, class bits OR-ed; box_sc = b_dim[l] (l < 4) or max(img_dim) (l = 4). */
int cvl_fcos_center_v1_assign(const float* boxes, const int32_t* nbox, const float* img_dim, int B, int n_max,
                              int pad_h, int pad_w, int num_classes, const int32_t* strides, const float* b_dim,
                              float* targets, int32_t* num_targets, cvl_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The FCOS recipe of the FCOS papers (Tian et al., ICCV 2019 / TPAMI 2020): an extension beyond the
 * reference, whose own recipe is cvl_fcos_assign / cvl_fcos_loss above.
 *
 * cvl_fcos_paper_assign: inputs, layout and channel order of cvl_fcos_assign (targets [B][P][5+C] =
 * (top, bottom, left, right) in stride units, centerness, C class values; n_max <= 256; the staged
 * tile limits C to 219) plus center_radius.  num_targets [B][5] is the number of POSITIVE CELLS per
 * level (cvl_fcos_assign counts boxes).  All fp32, in this operation order (no contraction):
 *   box i < clamp(nbox[b], 0, n_max) with (int)label in [0, C) (others are skipped entirely):
 *     yc = r0*H, xc = r1*W, hp = r2*H, wp = r3*W; y0 = yc - hp*0.5f, y1 = yc + hp*0.5f,
 *     x0 = xc - wp*0.5f, x1 = xc + wp*0.5f; area = hp*wp
 *   cell (cy, cx) of level l, sf = (float)stride_l: gy = ((float)cy + 0.5f)*sf, gx likewise;
 *     t = gy - y0, b = y1 - gy, l = gx - x0, r = x1 - gx, m = max(t, b, l, r)
 *   inside: center_radius <= 0: min(t, b, l, r) > 0; otherwise rs = center_radius*sf,
 *     sy0 = fmaxf(y0, yc - rs), sy1 = fminf(y1, yc + rs), the same in x, and
 *     min(gy - sy0, sy1 - gy, gx - sx0, sx1 - gx) > 0
 *   range: lo_l <= m <= hi_l, lo = (-1, size_bounds[0..3]), hi = (size_bounds[0..3], +inf), both
 *     ends inclusive (m exactly on a bound is a candidate on both levels)
 *   winner among the candidates: smallest area, ties to the lowest box index
 *   values: (t, b, l, r)/sf; centerness = (float)sqrt((min(t,b)/max(t,b)) * (min(l,r)/max(l,r))) with
 *     the four pixel distances cast to double first; a one-hot class.  Cells without a candidate are
 *     all zero.
 *
 * cvl_fcos_target_norm: norm[b] = (n_pos, sum of targets[4] over the positive cells) of image b, a cell
 * being positive when max_c targets[5+c] >= 1 (the mask of cvl_fcos_loss); summed in float64 in a
 * fixed order.  workspace >= cvl_fcos_target_norm_workspace_size(B, P) bytes.
 *
 * cvl_fcos_paper_loss: fused forward + backward with the conventions of cvl_fcos_loss (reg_pred
 * [B][P][ld_reg >= 5], cls_pred [B][P][ld_cls >= C], optional d_reg / d_cls fp32 (0) or bf16 (1) with
 * padding columns zeroed, grad_scale, losses [B][3] = (cls, reg, cen), workspace >=
 * cvl_fcos_loss_workspace_size(B, P) bytes).  norm [B][2] as cvl_fcos_target_norm writes it, or null.
 * Per image, N = max(norm[b][0], 1), Wsum = max(norm[b][1], 1e-6f) (null norm: N = Wsum = 1):
 *   cls = (1/N) sum_cells sum_c focal(y, x)              (the focal term of cvl_fcos_loss_ex)
 *   cen = (1/N) sum_pos [max(x,0) - x t4 + log1p(exp(-|x|))], x = reg_pred[4]; d/dx = sigmoid(x) - t4
 *   reg = (1/Wsum) sum_pos t4 (1 - GIoU)
 * GIoU on d_j = max(p_j, 0) (gradient 0 where p_j <= 0); th = t0+t1, tw = t2+t3, ph = d0+d1, pw = d2+d3:
 *   I = (min(t0,d0)+min(t1,d1)) (min(t2,d2)+min(t3,d3)), U = th tw + ph pw - I + 1e-12,
 *   E = (max(t0,d0)+max(t1,d1)) (max(t2,d2)+max(t3,d3)) + 1e-12, GIoU = I/U - (E - U)/E.
 * Non-positive cells contribute nothing to cen / reg and get zero box gradients.  Per-image sums are
 * deterministic (float64 per-tile partials, fixed-order second pass).
 * ---------------------------------------------------------------------------------------- */
int cvl_fcos_paper_assign(const float* boxes, const int32_t* nbox, const float* img_dim, int B, int n_max,
                          int pad_h, int pad_w, int num_classes, const int32_t* strides /*host[5]*/,
                          const float* size_bounds /*host[4]*/, float center_radius, float* targets,
                          int32_t* num_targets, cvl_stream_t stream);
size_t cvl_fcos_target_norm_workspace_size(int B, int P);
int cvl_fcos_target_norm(const float* targets, int B, int P, int num_classes, float* norm, void* workspace,
                         size_t workspace_bytes, cvl_stream_t stream);
int cvl_fcos_paper_loss(const float* reg_pred, int ld_reg, const float* cls_pred, int ld_cls,
                        const float* targets, const float* norm, int B, int P, int num_classes,
                        float grad_scale, float alpha, float gamma, float* losses, void* d_reg, int ld_dreg,
                        int dreg_dtype, void* d_cls, int ld_dcls, int dcls_dtype, void* workspace,
                        size_t workspace_bytes, cvl_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ATSS target assignment for FCOS (Zhang et al., CVPR 2020, "Bridging the Gap Between Anchor-based and
 * Anchor-free Detection via Adaptive Training Sample Selection"): an extension beyond the reference.
 * Its targets feed cvl_fcos_target_norm and cvl_fcos_paper_loss above, the loss ATSS trains FCOS with.
 *
 * cvl_fcos_atss_assign: inputs, target layout and channel order of cvl_fcos_paper_assign (boxes
 * [B][n_max][5] = (yc, xc, h, w, label) normalised, nbox [B], img_dim [B][2], strides HOST [5]; targets
 * [B][P][5+C] level-major over the (pad_h/stride) x (pad_w/stride) maps; num_targets [B][5] = POSITIVE
 * CELLS per level; n_max <= 256; the staged tile limits C to 219).  topk in 1..16 (the papers' 9),
 * anchor_scale > 0 (the papers' 8); anything outside these limits returns the invalid-argument status
 * and writes nothing.  fp32 in this operation order (no contraction) except where float64 is named:
 *   box i < clamp(nbox[b], 0, n_max): yc, xc, hp, wp, y0, y1, x0, x1, area as in cvl_fcos_paper_assign;
 *     the box is skipped entirely unless (int)label is in [0, C) (tested as -1 < label < C, so a NaN
 *     label is skipped) and area > 0 (which drops a NaN size)
 *   1 candidates, per level l with Hs x Ws cells, sf = (float)stride_l: gy = ((float)cy + 0.5f)*sf, gx
 *     likewise; dy = gy - yc, dx = gx - xc, d2 = dy*dy + dx*dx; the candidates are the
 *     k_l = min(topk, Hs*Ws) cells with the smallest d2, ties to the lowest row-major cell index,
 *     ranked in that order (d2 orders by its bit pattern, a NaN above +inf)
 *   2 anchor IoU of a candidate: ha = anchor_scale*sf*0.5f;
 *     ih = fmaxf(fminf(y1, gy+ha) - fmaxf(y0, gy-ha), 0), iw likewise in x; inter = ih*iw;
 *     uni = ((ha+ha)*(ha+ha) + area) - inter; iou = (float)((double)inter / (double)uni)
 *   3 threshold, float64, over the n = sum_l k_l candidates level-major and then by rank:
 *     mean = (sum iou)/n; var = sum (iou-mean)^2 / (n-1); std = sqrt(var) (the sample standard
 *     deviation, as the published implementations; 0 for n < 2); thr = mean + std
 *   4 positive pair (box, cell): the cell is a candidate of the box, (double)iou >= thr, and each of
 *     t = gy - y0, b = y1 - gy, l = gx - x0, r = x1 - gx is > 0.01f (so min(t, b, l, r) > 0.01f, and a
 *     NaN distance is never positive).  A pair with iou == 0 that passes both is still positive.
 *   per cell: among its positive pairs the largest iou wins, ties to the lowest box index; values as
 *     cvl_fcos_paper_assign: (t, b, l, r)/sf, centerness = (float)sqrt((min(t,b)/max(t,b)) *
 *     (min(l,r)/max(l,r))) in float64, a one-hot class.  Cells without a positive pair are all zero.
 * Optional outputs (null: not written), how the tests see inside the assignment: cand_cells int32
 * [B][n_max][5*topk] = the global cell index in [0, P) by level and rank, or -1; cand_iou float, the same
 * shape, 0 where cand_cells is -1; cand_thr double [B][n_max]; boxes that are skipped or past nbox get
 * -1 / 0 / 0.  workspace >= cvl_fcos_atss_workspace_size(B, P) bytes, 8-byte aligned (one 64-bit contest
 * key per cell).  Graph-safe: no host synchronisation, no allocation; its clears are memset nodes.
 * Bit-identical from run to run (the contest is an integer max, the counts integer adds).
 * ---------------------------------------------------------------------------------------- */
size_t cvl_fcos_atss_workspace_size(int B, int P);
int cvl_fcos_atss_assign(const float* boxes, const int32_t* nbox, const float* img_dim, int B, int n_max,
                         int pad_h, int pad_w, int num_classes, const int32_t* strides /*host[5]*/, int topk,
                         float anchor_scale, float* targets, int32_t* num_targets, int32_t* cand_cells,
                         float* cand_iou, double* cand_thr, void* workspace, size_t workspace_bytes,
                         cvl_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ATSS target assignment and a per-image normalised loss for RetinaNet (the same paper: ATSS was
 * published to bridge RetinaNet and FCOS): an extension beyond the reference.  The targets are compact,
 * 8 floats per anchor in the row order of the head outputs, instead of cvl_retina_assign's one-hot rows.
 *
 * cvl_retina_atss_assign: inputs of cvl_retina_assign (boxes [B][n_max][5] = (yc, xc, h, w, label)
 * normalised, nbox [B], img_dim [B][2], a square pad, anchor_dims DEVICE [5][A][2] = (h, w), strides HOST
 * [5]) plus topk.  targets [B][P][A][8], 16-byte aligned: cell-major over the level-major cells (level l
 * has S = pad/stride_l cells a side, cell = u*S + v, P = sum_l S*S), anchor-minor.  num_targets [B][5] =
 * POSITIVE ANCHORS per level.  Limits: n_max <= 256, 1 <= A <= 16, 1 <= topk <= 144 and
 * ceil(topk/A) <= 16, pad a positive multiple of 128 and of every stride, 1 <= C <= 256; anything else
 * returns the invalid-argument status and writes nothing.  fp32 in this operation order (no
 * contraction) except where float64 is named:
 *   box i < clamp(nbox[b], 0, n_max): yc, xc, hp, wp, y0, y1, x0, x1, area and the validity test exactly
 *     as in cvl_fcos_atss_assign (skipped unless -1 < label < C and area > 0)
 *   anchor positions as cvl_retina_assign / cvl_retina_decode: the A anchors of cell (u, v) of level l
 *     are centred at c0 = (float)(u*s) in y, c1 = (float)(v*s) in x (no +0.5), with dims
 *     (ah, aw) = anchor_dims[l][an]
 *   1 candidates, per level: dy = c0 - yc, dx = c1 - xc, d2 = dy*dy + dx*dx (ordered by its bit pattern,
 *     a NaN above +inf); the candidates are the k_l = min(topk, A*S*S) anchors with the smallest d2, ties
 *     to the lowest cell*A + an, ranked in that order.  All A anchors of a cell tie, so these are the
 *     ceil(k_l/A) nearest cells, each in full except possibly the last: rank j is anchor j % A of the
 *     cell of rank j / A
 *   2 IoU of a candidate: ih = fmaxf(fminf(y1, c0+ah*0.5f) - fmaxf(y0, c0-ah*0.5f), 0), iw likewise in x
 *     with aw; inter = ih*iw; uni = (ah*aw + area) - inter; iou = (float)((double)inter / (double)uni)
 *   3 threshold, float64, over the n = sum_l k_l candidates level-major and then by rank: mean + sample
 *     standard deviation, exactly as step 3 of cvl_fcos_atss_assign
 *   4 positive pair (box, anchor): the anchor is a candidate of the box, (double)iou >= thr, and each of
 *     c0 - y0, y1 - c0, c1 - x0, x1 - c1 is > 0.01f
 *   per anchor: among its positive pairs the largest iou wins, ties to the lowest box index (a 64-bit
 *     integer max of iou bits << 32 | ~box).  The row of a positive anchor: slots 0..3 the linear box
 *     targets of cvl_retina_assign in float64 rounded to fp32, (c0 - yc)/ah, (c1 - xc)/aw, hp/ah, wp/aw;
 *     slot 4 (float)label; slot 5 the winning iou; slot 6 (float)box index; slot 7 zero.  The row of any
 *     other anchor is 0, 0, 0, 0, -1, 0, -1, 0.
 * Optional outputs (null: not written): cand_idx int32 [B][n_max][5*topk] = the target row
 * (off_l + cell)*A + an in [0, P*A) by level and rank, or -1; cand_iou float, the same shape, 0 where
 * cand_idx is -1; cand_thr double [B][n_max]; boxes that are skipped or past nbox get -1 / 0 / 0.
 * workspace >= cvl_retina_atss_workspace_size(B, P, A) bytes, 8-byte aligned (one 64-bit contest key per
 * anchor).  Graph-safe: no host synchronisation, no allocation; its clears are memset nodes.
 * Bit-identical from run to run.
 *
 * cvl_retina_atss_loss: fused forward + backward on those targets.  reg_pred [B][P][ld_reg >= 4A] with
 * anchor a at channels 4a..4a+3, cls_pred [B][P][ld_cls >= A*C] with anchor a at channels aC..aC+C-1
 * (the grouped heads' rows); targets / num_targets as the assign call writes them; img_weight [B] or null
 * (= 1).  Per element, fp32: class = the focal term of cvl_fcos_paper_loss with y = 1 iff the anchor's
 * label (slot 4) equals the class; box = the smooth-L1 element of cvl_retina_loss between slots 0..3 and
 * the four box outputs, on the positive anchors only (label >= 0; the box slots of the others are never
 * read).  Per image, N_b = max(sum_l num_targets[b][l], 1), wb = img_weight[b]:
 *   losses[b] = (cls, reg) = (float)(wb * sum / (double)N_b), the sums as float64 per-tile partials and
 *     a fixed-order second pass (no float atomics: bit-identical from run to run)
 *   a gradient element is g * gs with gs = (grad_scale * wb) / (float)N_b; the box gradient of a
 *     non-positive anchor is written as 0; channels at or beyond 4A / A*C are not touched.
 * d_reg / d_cls: fp32 (dtype 0) or bf16 (1) with leading dimensions of their own, or null for forward
 * only.  workspace >= cvl_retina_atss_loss_workspace_size(B, P, A) bytes, 8-byte aligned; targets 16-byte
 * aligned.  Arguments out of range return the invalid-argument status and write nothing.  Graph-safe.
 * ---------------------------------------------------------------------------------------- */
size_t cvl_retina_atss_workspace_size(int B, int P, int n_anchors);
int cvl_retina_atss_assign(const float* boxes, const int32_t* nbox, const float* img_dim, int B, int n_max, int pad,
                           int num_classes, const float* anchor_dims, int n_anchors,
                           const int32_t* strides /*host[5]*/, int topk, float* targets, int32_t* num_targets,
                           int32_t* cand_idx, float* cand_iou, double* cand_thr, void* workspace,
                           size_t workspace_bytes, cvl_stream_t stream);
size_t cvl_retina_atss_loss_workspace_size(int B, int P, int n_anchors);
int cvl_retina_atss_loss(const float* reg_pred, int ld_reg, const float* cls_pred, int ld_cls, const float* targets,
                         const int32_t* num_targets, const float* img_weight, int B, int P, int n_anchors,
                         int num_classes, float grad_scale, float alpha, float gamma, float* losses, void* d_reg,
                         int ld_dreg, int dreg_dtype, void* d_cls, int ld_dcls, int dcls_dtype, void* workspace,
                         size_t workspace_bytes, cvl_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Generalized Focal Loss for the FCOS head (Li et al., NeurIPS 2020, "Generalized Focal Loss: Learning
 * Qualified and Distributed Bounding Boxes for Dense Object Detection"): an extension beyond the
 * reference, trained on the targets of cvl_fcos_atss_assign (or cvl_fcos_paper_assign).  The
 * centerness output is gone: the class target of a positive is the IoU of its decoded box (Quality
 * Focal Loss), and each box side is a discrete distribution over R + 1 bins (Distribution Focal Loss)
 * whose expectation is the distance.  Compiled without contraction; fp32 unless float64 is named.
 *
 * Layout as cvl_fcos_paper_loss except for the box rows: R = reg_max, 1 <= R <= 16; cls_pred
 * [B][P][ld_cls >= C]; reg_pred [B][P][ld_reg >= 4(R+1)] with z[j][i] = reg_pred[.. + j*(R+1) + i], side
 * j = 0..3 = (top, bottom, left, right) in the order of targets[0..3], bin i = 0..R in stride units;
 * targets [B][P][5+C] as the assign entries write them (targets[4] is not read).  A cell is positive
 * when max_c targets[5+c] >= 1.
 *   every cell, every class c: s_c = sigmoid(x_c); y_c = q if the cell is positive and targets[5+c] >= 1,
 *     else 0;  QFL_c = |y_c - s_c|^beta * (max(x_c,0) - x_c*y_c + log1p(exp(-|x_c|)))
 *     (beta = 2 is evaluated as a product, other values through powf)
 *   positive cells, all softmaxes max-subtracted: p[j] = softmax(z[j]), d_j = sum_i i*p[j][i], t_j =
 *     targets[j]; th = t0+t1, tw = t2+t3, ph = d0+d1, pw = d2+d3,
 *     I = (min(t0,d0)+min(t1,d1)) (min(t2,d2)+min(t3,d3)), U = th tw + ph pw - I + 1e-12,
 *     E = (max(t0,d0)+max(t1,d1)) (max(t2,d2)+max(t3,d3)) + 1e-12, GIoU = I/U - (E - U)/E
 *     (the expressions of cvl_fcos_paper_loss with d_j in the place of max(p_j, 0));
 *     q = I/U and w = sigmoid(max_c x_c), BOTH constants for the gradient;
 *     tc_j = fminf(fmaxf(t_j, 0), (float)R - 0.1f), yl = floorf(tc_j), wl = (yl + 1) - tc_j, wr = tc_j - yl,
 *     dfl_cell = 0.25 * sum_j [wl*(lse(z[j]) - z[j][yl]) + wr*(lse(z[j]) - z[j][yl+1])]
 *   per image, losses [B][3] = (qfl, box, dfl) with N = max(norm[b][0], 1), Wsum = max(norm[b][1], 1e-6f)
 *     (null norm: N = Wsum = 1):  qfl = (1/N) sum_cells sum_c QFL_c;  box = (w_box/Wsum) sum_pos w*(1 - GIoU);
 *     dfl = (w_dfl/Wsum) sum_pos w*dfl_cell.  The published values are beta = 2, w_box = 2, w_dfl = 0.25.
 *   gradients = grad_scale * d(qfl + box + dfl)/d(pred): d_cls from QFL only, d_reg from box and DFL
 *     only; non-positive cells get all-zero box rows (their box logits are never read); the padding
 *     columns of both gradient rows are zeroed.  d_reg / d_cls: fp32 (dtype 0) or bf16 (1), or null for
 *     forward only.
 * Per-image sums are float64 per-tile partials and a fixed-order second pass: a call is bit-identical
 * from run to run.  The normalisation is per image (the published code normalises over the batch).
 *
 * cvl_fcos_gfl_norm: norm[b] = (number of positive cells, sum over them of sigmoid(max_c x_c)), summed
 * in float64 in a fixed order and stored as fp32; it needs the class outputs, so it runs after the
 * forward.  workspace >= cvl_fcos_gfl_norm_workspace_size(B, P) bytes.
 * cvl_fcos_gfl_loss: workspace >= cvl_fcos_gfl_loss_workspace_size(B, P) bytes.
 * cvl_fcos_gfl_decode: out[row][0..3] = d_j of reg_pred row `row` (rows = B*P), columns 4..ld_out-1
 * zero, ld_out >= 8: what cvl_fcos_detect with center = 0 reads as (t, b, l, r).
 * Arguments out of range (R outside 1..16, an ld too small, beta < 0, a dtype other than 0 / 1, a
 * workspace too small) return the invalid-argument status and write nothing.  All three are graph-safe:
 * no host synchronisation, no allocation.
 * ---------------------------------------------------------------------------------------- */
size_t cvl_fcos_gfl_norm_workspace_size(int B, int P);
int cvl_fcos_gfl_norm(const float* cls_pred, int ld_cls, const float* targets, int B, int P, int num_classes,
                      float* norm, void* workspace, size_t workspace_bytes, cvl_stream_t stream);
size_t cvl_fcos_gfl_loss_workspace_size(int B, int P);
int cvl_fcos_gfl_loss(const float* reg_pred, int ld_reg, const float* cls_pred, int ld_cls,
                      const float* targets, const float* norm, int B, int P, int num_classes, int reg_max,
                      float grad_scale, float beta, float w_box, float w_dfl, float* losses, void* d_reg,
                      int ld_dreg, int dreg_dtype, void* d_cls, int ld_dcls, int dcls_dtype, void* workspace,
                      size_t workspace_bytes, cvl_stream_t stream);
int cvl_fcos_gfl_decode(const float* reg_pred, int ld_reg, int rows, int reg_max, float* out, int ld_out,
                        cvl_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Task-aligned assignment for the FCOS head (Feng et al., ICCV 2021, "TOOD: Task-aligned One-stage
 * Object Detection") and its loss: an extension beyond the reference, the step after the geometric
 * assigners above.  The network's own outputs choose its positives: a cell is positive for a box when
 * its class score and the IoU of its predicted box are jointly high, and the class target of a positive
 * is that alignment value instead of a one-hot 1.  The assignment therefore runs AFTER the forward.
 * Compiled without contraction; fp32 in this operation order unless float64 is named.
 *
 * cvl_fcos_tal_assign: boxes, validity, cell positions, the target layout and num_targets exactly as
 * cvl_fcos_atss_assign (boxes [B][n_max][5] = (yc, xc, h, w, label) normalised, skipped unless
 * -1 < label < C and area > 0; gy = ((float)cy + 0.5f)*sf; targets [B][P][5+C] level-major; num_targets
 * [B][5] = POSITIVE CELLS per level; n_max <= 256; the staged tile limits C to 219).
 * dist [B][P][ld_dist >= 4] = the predicted distances (top, bottom, left, right) in stride units: with
 * clamp != 0, d_j = fmaxf(v_j, 0) (the 5-output head's raw reg_pred is passed directly); with clamp == 0,
 * d_j = v_j (the layout cvl_fcos_gfl_decode writes).  cls_pred [B][P][ld_cls >= C] = fp32 class logits.
 * topk in 1..32 (the papers' 13), alpha >= 0 and beta >= 0 (the papers' 1 and 6); anything outside
 * these limits returns the invalid-argument status and writes nothing.
 *   per (box i, cell p):
 *     inside: t = gy - y0, b = y1 - gy, l = gx - x0, r = x1 - gx, each > 0.01f (rule 4 of ATSS); the
 *       predictions of a cell are read only for the boxes it lies inside, so cells outside every valid
 *       box may hold anything, a NaN included
 *     predicted box: py0 = gy - d0*sf, py1 = gy + d1*sf, px0 = gx - d2*sf, px1 = gx + d3*sf;
 *       ih = fmaxf(fminf(y1, py1) - fmaxf(y0, py0), 0), iw likewise in x; inter = ih*iw;
 *       uni = ((py1 - py0)*(px1 - px0) + area) - inter;
 *       u = uni > 0 ? (float)((double)inter / (double)uni) : 0
 *     score: s = 1/(1 + expf(-x)), x = cls_pred[b][p][(int)label]
 *     metric: m = pow_a(s) * pow_b(u); alpha == 1 is evaluated as s, beta == 6 as u2 = u*u, (u2*u2)*u2,
 *       other exponents through powf
 *   candidates of box i: the inside cells with m > 0 (a NaN metric is never a candidate); selected: the
 *     min(topk, #candidates) candidates with the largest m, ties to the lowest global cell index, ranked
 *     in that order (the inside-first order of PP-YOLOE / YOLOv8)
 *   per cell: among the boxes that selected it the largest u wins, ties to the lowest box index (a
 *     64-bit integer max of u bits << 32 | ~box, as the ATSS contest)
 *   per box: max_m and max_u over the cells it won (integer max of the bit patterns; both are >= 0)
 *   the row of a won cell: (t, b, l, r)/sf; slot 4 = (float)((double)m * (double)max_u /
 *     ((double)max_m + 1e-9)); a one-hot class.  All other rows are zero.
 * Optional outputs (null: not written): cand_cells int32 [B][n_max][topk] = the selected global cell
 * by rank, or -1; cand_metric and cand_iou fp32 of the same shape, 0 where the cell is -1; box_max float
 * [B][n_max][2] = (max_m, max_u), 0 for a box that won nothing.  workspace >=
 * cvl_fcos_tal_workspace_size(B, P, n_max) bytes, 8-byte aligned.  Graph-safe: no host synchronisation,
 * no allocation; its clears are memset nodes.  Bit-identical from run to run (the contests are integer
 * maxima, the counts integer adds), whatever path the selection takes: a box's candidate keys are staged
 * in LDS, and a box with more candidates than the stage holds recomputes them in every round.
 *
 * cvl_fcos_tal_loss: fused forward + backward with the conventions, argument order and workspace rule
 * of cvl_fcos_paper_loss (reg_pred [B][P][ld_reg >= 5], cls_pred [B][P][ld_cls >= C], optional d_reg /
 * d_cls fp32 (0) or bf16 (1) with padding columns zeroed, grad_scale, losses [B][3], workspace >=
 * cvl_fcos_loss_workspace_size(B, P) bytes), with qfl_beta >= 0 and w_box (the papers' 2 and 2) in the
 * place of alpha and gamma.  A cell is positive when max_c targets[5+c] >= 1; y_c = targets[4] where
 * targets[5+c] >= 1 (such a cell is positive), else 0.  W = max(norm[b][1], 1) with norm [B][2] as
 * cvl_fcos_target_norm writes it (count, sum of slot 4); a null norm gives W = 1.
 *   cls = (1/W) sum_cells sum_c |y_c - s_c|^qfl_beta * (max(x,0) - x*y_c + log1p(exp(-|x|))), the QFL term
 *     of cvl_fcos_gfl_loss with y a constant for the gradient
 *   box = (w_box/W) sum_pos targets[4] * (1 - GIoU), GIoU exactly the expressions of cvl_fcos_paper_loss
 *     on d_j = max(p_j, 0)
 *   losses[b] = (cls, box, 0)
 * Column 4 and up of d_reg is zero (the head's centerness output gets no gradient); non-positive cells
 * get all-zero box rows, and their box outputs are not read.  Per-image sums are float64 per-tile
 * partials and a fixed-order second pass.  The normalisation is per image (the published code
 * normalises over the batch).  Arguments out of range return the invalid-argument status and write
 * nothing.  Graph-safe.
 * ---------------------------------------------------------------------------------------- */
size_t cvl_fcos_tal_workspace_size(int B, int P, int n_max);
int cvl_fcos_tal_assign(const float* boxes, const int32_t* nbox, const float* img_dim, int B, int n_max,
                        int pad_h, int pad_w, int num_classes, const int32_t* strides /*host[5]*/,
                        const float* dist, int ld_dist, int clamp, const float* cls_pred, int ld_cls, int topk,
                        float alpha, float beta, float* targets, int32_t* num_targets, int32_t* cand_cells,
                        float* cand_metric, float* cand_iou, float* box_max, void* workspace,
                        size_t workspace_bytes, cvl_stream_t stream);
int cvl_fcos_tal_loss(const float* reg_pred, int ld_reg, const float* cls_pred, int ld_cls,
                      const float* targets, const float* norm, int B, int P, int num_classes,
                      float grad_scale, float qfl_beta, float w_box, float* losses, void* d_reg, int ld_dreg,
                      int dreg_dtype, void* d_cls, int ld_dcls, int dcls_dtype, void* workspace,
                      size_t workspace_bytes, cvl_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * CenterNet as the paper trains it (Zhou et al., 2019, "Objects as Points"): an extension beyond the
 * reference.  Gaussian heat about every object centre, the penalty-reduced focal loss, L1 on the box
 * channels of the centres, every sum divided by the image's number of objects.  The reference's recipe
 * (cvl_centernet_assign / cvl_centernet_loss: one-hot centres, full-weight negatives, plain sums) is
 * unchanged.  The model output keeps the reference's ltrb box channels (no size / offset heads), so
 * cvl_centernet_decode and cvl_centernet_peak_decode read it as before.  Compiled without contraction;
 * fp32 unless float64 is named.
 *
 * cvl_centernet_gauss_assign: boxes [B][n_max][5] = (yc, xc, h, w, label) normalised, nbox [B], img_dim
 * [B][2] = (H, W), n_max <= 256, num_classes = C <= 256, 0 < min_overlap < 1 -> targets
 * [B][hm = pad_h/stride][wm = pad_w/stride][4+C], rows along y.  (cvl_centernet_assign keeps the
 * reference's swap of the two pads; the two layouts and paddings coincide when pad_h == pad_w and
 * H == W.)  Per box, in fp32 with s = (float)stride, the expressions of cvl_centernet_assign:
 *   c0 = (yc - 0.5f h) H, c1 = (xc - 0.5f w) W, c2 = (yc + 0.5f h) H, c3 = (xc + 0.5f w) W;
 *   pad_y = (float)(int)((pad_h - H) / 2.0f), pad_x = (float)(int)((pad_w - W) / 2.0f);
 *   ycf = (c0 + c2) / 2.0f, xcf = (c1 + c3) / 2.0f; cy = (int)((pad_y + ycf) / s), cx = (int)((pad_x + xcf) / s);
 *   off4 = ((float)((double)cy + 0.5) - (pad_y + c0)/s, ((pad_y + c2)/s - (float)cy) - 0.5f,
 *           (float)((double)cx + 0.5) - (pad_x + c1)/s, ((pad_x + c3)/s - (float)cx) - 0.5f).
 *   A box whose (cy, cx) lies outside the map, or whose label lies outside [0, C), is skipped entirely.
 *   Radius, float64 (mmdet's gaussian_radius, the corrected roots), m = min_overlap,
 *     h = ceilf((c2 - c0)/s), w = ceilf((c3 - c1)/s) widened:
 *     b1 = h + w, k1 = w h (1 - m)/(1 + m), r1 = (b1 - sqrt(b1 b1 - 4 k1)) / 2;
 *     b2 = 2 (h + w), k2 = (1 - m) w h, r2 = (b2 - sqrt(b2 b2 - 16 k2)) / 8;
 *     a3 = 4 m, b3 = -2 m (h + w), k3 = (m - 1) w h, r3 = (b3 + sqrt(b3 b3 - 4 a3 k3)) / (2 a3);
 *     r = max(0, (int)min(r1, r2, r3)).
 *   Heat, fp32: sigma = (float)(2r + 1) / 6.0f, two_s2 = 2.0f * sigma * sigma; for integer offsets
 *     |dy| <= r, |dx| <= r from (cy, cx): g = expf(-(float)(dy dy + dx dx) / two_s2) (1.0f at the centre).
 *   targets[cell][4+c] = max of g over the image's kept boxes of label c, 0 where no disc reaches.
 *   targets[cell][0..3] = off4 of the last kept box centred on the cell in the stable ascending order of
 *     the areas (h H)(w W) (the reference's rule: the largest box wins), 0 on every other cell.
 * cvl_centernet_gauss_norm: targets [B][P][4+C] -> npos[b] (int32) = number of (cell, class) entries of
 *   image b equal to 1.0f (two same-class boxes on one centre cell count once).  Any target map.
 * cvl_centernet_gauss_loss: pred [B*P][ld_pred >= 4+C] fp32 (box 0..3, class logits 4..4+C), targets
 *   [B*P][4+C], N = max(npos[b], 1).  Per class entry with y = its target, e = expf(-|x|),
 *   L = log1pf(e), p = sigmoid(x) and q = 1 - p formed from e without cancellation,
 *   -log p = L - min(x, 0), -log q = L + max(x, 0):
 *     y == 1.0f:  q^alpha (-log p);   otherwise:  (1 - y)^beta p^alpha (-log q)
 *     (an exponent of 2 or 4 is evaluated as products, any other through powf);
 *   per box channel j of a cell with some class target == 1.0f: |t_j - x_j|, gradient sign(x_j - t_j), 0
 *   at equality, applied by selection: the box predictions of every other cell are not used at all.
 *   losses [B][2] = (cls, reg) = the image's two sums / N, not scaled by the lambdas (the paper's values
 *   are alpha 2, beta 4); d_pred bf16 [B*P][ld_d >= 4+C] = d(cls_scale*cls + reg_scale*reg)/d(pred),
 *   channels >= 4+C zeroed.  An image without positives: its negative class sum with N = 1, no box term.
 *   Sums are float64 per-tile partials and a fixed-order second pass.
 *   workspace >= cvl_centernet_gauss_loss_workspace_size(B, P) bytes, 8-byte aligned.
 * Arguments out of range return the invalid-argument status and write nothing.  All three are
 * graph-safe (no host synchronisation, no allocation, no floating-point atomics) and bit-identical
 * from run to run.
 * ---------------------------------------------------------------------------------------- */
int cvl_centernet_gauss_assign(const float* boxes, const int32_t* nbox, const float* img_dim, int B, int n_max,
                               int pad_h, int pad_w, int num_classes, int stride, float min_overlap,
                               float* targets, cvl_stream_t stream);
int cvl_centernet_gauss_norm(const float* targets, int B, int P, int num_classes, int32_t* npos,
                             cvl_stream_t stream);
size_t cvl_centernet_gauss_loss_workspace_size(int B, int P);
int cvl_centernet_gauss_loss(const float* pred, int ld_pred, const float* targets, const int32_t* npos, int B,
                             int P, int num_classes, float alpha, float beta, float cls_scale, float reg_scale,
                             float* losses, void* d_pred, int ld_d, void* workspace, cvl_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Segmented implicit-GEMM convolution (bf16 MFMA, fp32 accumulate).  Replaces every Conv2D of
 * the reference graphs (Keras ResNet50 backbone; FCOS/fcos.py:49-101 FPN, towers and heads;
 * RetinaNet/retinanet_module.py:74-148) forward (mode FWD) and backward-input (mode DGRAD).
 * A "segment" is one feature map of B images: rows of image b live at source/destination rows
 * base + b*img_stride + (y*W + x), each row holding `Cin` (source) / `ld_dst` (dest) channels.
 * Several segments in one call share the forward geometry (kernel/stride/pad) but may each have
 * their own packed weights and bias: the five FPN levels through a shared tower, or the five
 * per-level heads, are one launch.
 * Weights: FWD  -> packed [Npad][KH*KW*Cin]   (cvl_pack_conv_weights w_fwd)
 *          DGRAD-> packed [Npad=Cin_pad][KH*KW*Cout_pad] (w_dgrad); then `Cin` = Cout_pad.
 * TF "same" padding: pad_t/pad_l = floor(total/2) (asymmetric for stride 2).
 * bn_stats (nullable) receives per-(image, out channel) (sum, sumsq) as BN accumulators (below;
 * zero it first), which requires H*W % 4 == 0.
 *
 * BN accumulators (cvl_bn_acc): the statistics many workgroups add into one (image, channel) --
 * (sum, sumsq) of a conv output, (sum g, sum g*xhat) of a BN backward.  Two modes, chosen for the
 * whole library by cvl_bn_set_exact() before any buffer is made (cvl_bn_acc_slots() = S reports it):
 *  - default (S = 1): one float64 per statistic, fp64 atomic adds of fp32 partials (the order of
 *    the adds can change the last bits of a sum);
 *  - exact (S = 8, cvl_bn_set_exact(1)): each fp32 partial is added as an integer into one of 7
 *    uint64 bins chosen by its exponent (bin k holds multiples of 2^(22k - 123); partials below
 *    2^-100 are dropped, slot 7 counts non-finite ones), so the result is bit-identical whatever
 *    order the atomics land in.  The value of a statistic is
 *    sum_k (double)(int64)slot[k] * 2^(22k - 123) over k = 0..6 in that order (NaN if slot[7] != 0).
 *    The consumers (cvl_bn_finalize[_apply], cvl_bn_backward_*_sums) first DECODE THE BUFFER IN
 *    PLACE -- slot 0 of each statistic becomes its float64 value and slot 7 the marker ~0 -- so each
 *    statistic is decoded once; a decoded buffer stays valid input for every reader.
 * Layout: uint64 [B][C][2][S] (zero it before the producer); cvl_bn_acc_decode writes the values of
 * n statistics as float64 [n] in either mode.
 * ---------------------------------------------------------------------------------------- */
#define CVL_BN_ACC_SLOTS 8          /* S of the exact mode */
int cvl_bn_set_exact(int on);
int cvl_bn_acc_slots(void);
int cvl_bn_acc_decode(const uint64_t* acc, double* out, int64_t n, cvl_stream_t stream);
#define CVL_CONV_MAX_SEG 10
enum { CVL_CONV_FWD = 0, CVL_CONV_DGRAD = 1 };

typedef struct {
  int Hr, Wr;          /* spatial size of the GEMM rows: FWD output map / DGRAD input map */
  int Hs, Ws;          /* spatial size of the gathered source: FWD input map / DGRAD dY map */
  int64_t src_base, src_img;  /* source row of image 0 and rows per image */
  int64_t dst_base, dst_img;  /* destination row of image 0 and rows per image */
  const void* w;       /* packed bf16 weights for this segment */
  const float* bias;   /* per output channel, or NULL */
} cvl_conv_seg;

typedef struct {
  int mode;            /* CVL_CONV_FWD / CVL_CONV_DGRAD */
  int B;               /* images per segment */
  int Cin;             /* channels of each gathered source row (multiple of 32) */
  int KH, KW, stride, pad_t, pad_l;   /* FORWARD conv geometry */
  int Npad;            /* GEMM columns = packed weight rows (multiple of 32) */
  int n_store;         /* columns written (<= Npad) */
  int ld_dst, dst_coff;/* destination row pitch and channel offset (elements) */
  int dst_f32;         /* 1: fp32 destination, 0: bf16 */
  int relu_out;        /* ReLU on the result */
  int relu_in;         /* ReLU on the gathered source values */
  float beta;          /* dst = result + beta * dst */
  int nseg;
  cvl_conv_seg seg[CVL_CONV_MAX_SEG];
  int prec;            /* CVL_PREC_BF16 (0): bf16 source / weights / destination (dst_f32 aside),
                          bf16 MFMA.  CVL_PREC_F32 (1): the fp32 parity mode -- fp32 source, fp32
                          packed weights (cvl_pack_item.f32_out), fp32 destination, fp32 FMA,
                          deterministic; bn_stats then needs nseg == 1 (cvl_conv_wgrad* take the
                          same field for x / dy). */
} cvl_conv_desc;
enum { CVL_PREC_BF16 = 0, CVL_PREC_F32 = 1 };

/* workspace (optional, >= cvl_conv_igemm_workspace_size(d) bytes) enables split-K for grids too
 * small to fill the GPU (fp32 partial slabs + a finishing pass); NULL = no split. */
size_t cvl_conv_igemm_workspace_size(const cvl_conv_desc* d);
int cvl_conv_igemm(const cvl_conv_desc* d, const void* src, void* dst, uint64_t* bn_stats,
                   void* workspace, size_t workspace_bytes, cvl_stream_t stream);
/* A data gradient through a ReLU (the TF gradient of the FCOS towers' final ReLU behind the heads,
 * FCOS/fcos.py:16-27, 76-101): dst = conv data gradient of src (mode CVL_CONV_DGRAD, prec bf16, beta 0,
 * no relu_out) masked by y > 0, y [rows][ld_dst] laid out as dst.  The tower kernel applies the mask
 * in its register epilogue; otherwise the plain launch is followed by cvl_relu_backward (then dst
 * must be dense: ld_dst == n_store, dst_coff 0).  Bit-identical to cvl_conv_igemm + cvl_relu_backward. */
int cvl_conv_igemm_relu_mask(const cvl_conv_desc* d, const void* src, void* dst, const void* y, void* workspace,
                             size_t workspace_bytes, cvl_stream_t stream);
/* A residual unit whose BatchNorm is folded into the conv (inference; no reference counterpart: Keras
 * runs conv, BN, Add, ReLU as four ops): dst = relu(conv(src) + bias + dst), mode CVL_CONV_FWD, prec bf16,
 * beta 1, no relu_out, bf16 dst.  Where the plan is the persistent 1x1 kernel's accumulate form (64- /
 * 128-wide tiles) its epilogue applies the ReLU right after the accumulate; any other plan runs the
 * beta = 1 launch followed by cvl_relu_ over the destination rows (then dst must be dense: ld_dst ==
 * n_store, dst_coff 0 -- checked before anything is launched; CVL_DISPATCH=no_res_relu_fuse forces this
 * form).  ReLU of a bf16 value is exact: the two forms are bit-identical.  dst may not alias src. */
int cvl_conv_igemm_res_relu(const cvl_conv_desc* d, const void* src, void* dst, void* workspace,
                            size_t workspace_bytes, cvl_stream_t stream);
/* Test and profiling hook, as cvl_conv_igemm_plan: the kernel family (*kernel) a cvl_conv_igemm_res_relu
 * call would use and whether its epilogue applies the ReLU (*fused = 1) or the separate pass follows
 * (0).  Host only, no launch.  CVL_EINVAL where the call would reject d. */
int cvl_conv_igemm_res_relu_plan(const cvl_conv_desc* d, size_t workspace_bytes, int32_t* kernel, int32_t* fused);

/* Test / profiling hook: the kernel variant the last cvl_conv_igemm / cvl_conv_wgrad* call on THIS
 * host thread launched.  CVL_CK_* codes; cvl_conv_kernel_name(code) is a static string.  Codes 6
 * (X256) and 12 (X32H) belong to retired kernels and are no longer returned. */
enum { CVL_CK_NONE = 0, CVL_CK_BASE = 1, CVL_CK_BASE_SPLITK = 2, CVL_CK_L64 = 3, CVL_CK_L128 = 4,
       CVL_CK_L256 = 5, CVL_CK_X256 = 6, CVL_CK_X32 = 7,
       CVL_CK_WG_S = 8, CVL_CK_WG_L128 = 9, CVL_CK_WG_L256 = 10, CVL_CK_WG_X = 11, CVL_CK_X32H = 12, CVL_CK_WG_SN = 13,
       CVL_CK_H64 = 14, CVL_CK_WG_H = 15, CVL_CK_P = 16 };
int cvl_conv_igemm_last_kernel(void);
/* K-tile depth (32 or 64 bf16) of the last launch of the tower kernel (CVL_CK_X32) or the persistent
 * 1x1 kernel (CVL_CK_P) on this host thread; 0 before the first one. */
int cvl_conv_igemm_last_ktile(void);
/* Test and profiling hook: the kernel family (*kernel, a CVL_CK_* code) and K-tile depth (*ktile, as
 * cvl_conv_igemm_last_ktile reports it) that cvl_conv_igemm would use for d with these options
 * (BN statistics requested or not; workspace_bytes 0 = no workspace).  Runs the launch planner only:
 * host code, no device memory, no launch.  CVL_EINVAL where cvl_conv_igemm would reject d. */
int cvl_conv_igemm_plan(const cvl_conv_desc* d, int with_bn_stats, size_t workspace_bytes, int32_t* kernel,
                        int32_t* ktile);
/* The same query with the launch geometry: *grid = the workgroups the launch would have (per K split),
 * *ntile = its N-tile width in channels.  bsum_offer 0: a cvl_conv_igemm call; 1 / 2 / 3: a
 * cvl_conv_igemm_dgrad_bnsum / _res / _res_bits call offering that fused BN-sums form (as
 * cvl_conv_igemm_plan_bnsum; a declined offer reports the plain data gradient's plan).  For the
 * persistent 1x1 kernel (CVL_CK_P) a workgroup walks ceil(m_tiles / (grid / (Npad / ntile))) 256-row
 * tiles, so tests derive "several tiles per workgroup" from the planner's own answer.  Host only. */
int cvl_conv_igemm_plan_grid(const cvl_conv_desc* d, int with_bn_stats, int bsum_offer, size_t workspace_bytes,
                             int32_t* kernel, int32_t* ktile, int32_t* grid, int32_t* ntile);
const char* cvl_conv_kernel_name(int code);

/* Measurement hook (no reference counterpart: bench.py's in-step roofline timing).  cvl_probe_arm
 * hands slot (uint64 x4 device buffer, zero it first) to the NEXT cvl_conv_igemm call: when that
 * call runs the tower kernel (cvl_conv_igemm_last_kernel() == CVL_CK_X32) the kernel times itself
 * (workgroup 0's start to the last workgroup's end): slot[1] += elapsed ticks, slot[2] += 1 (slot[0]
 * / slot[3]: start stamp / workgroup counter); any other kernel leaves the slot untouched.  The slot
 * travels in the launch arguments, so graph capture keeps it.  cvl_probe_clock_hz = ticks per
 * second of the GPU wall clock. */
int cvl_probe_arm(uint64_t* slot);
double cvl_probe_clock_hz(void);

/* Weight gradient (replaces Conv2DBackpropFilter + the per-image gradient accumulation of
 * FCOS/train_fcos.py:173-176): dw[KH][KW][Cin][n_store] (HWIO fp32) = beta*dw + sum over all
 * rows of all segments of im2col(x) * dy.  `d` is the FORWARD descriptor (its ld_dst/dst_coff
 * address dy; all segments must share one weight pointer).  workspace >= *_workspace_size(d). */
size_t cvl_conv_wgrad_workspace_size(const cvl_conv_desc* d);
int cvl_conv_wgrad(const cvl_conv_desc* d, const void* x, const void* dy, float* dw, float beta,
                   void* workspace, size_t workspace_bytes, cvl_stream_t stream);

/* Grouped weight gradient: the segments of `d` split into `ngroups` consecutive equal groups (each
 * sharing one weight pointer), group g summed into dw[g] (a HOST array of device pointers).  The
 * FCOS cls and reg tower layers (FCOS/fcos.py:16-27, 76-101: same geometry, own weights) are one
 * call with 10 segments and 2 groups.  workspace >= cvl_conv_wgrad_grouped_workspace_size(d, ngroups). */
/* Deferred split reductions of the weight gradients.  cvl_wgrad_defer(1): the split-M weight
 * gradients (cvl_conv_wgrad / _grouped) leave their fp32 slabs pending instead of reducing them into
 * dW at once; cvl_wgrad_flush reduces everything pending in ONE batched launch (deterministic, the
 * same arithmetic as the immediate form).  The caller keeps every pending call's workspace alive and
 * dW unread until the flush; cvl_wgrad_defer(0) flushes and turns deferral off.  A reduction or
 * unsplit write into a dW that is already pending flushes first. */
int cvl_wgrad_defer(int on, cvl_stream_t stream);
int cvl_wgrad_flush(cvl_stream_t stream);
size_t cvl_conv_wgrad_grouped_workspace_size(const cvl_conv_desc* d, int ngroups);
int cvl_conv_wgrad_grouped(const cvl_conv_desc* d, int ngroups, const void* x, const void* dy, float* const* dw,
                           float beta, void* workspace, size_t workspace_bytes, cvl_stream_t stream);

/* Batched weight gradients (round 6): the weight gradients of n independent convolutions, d / x /
 * dy / dw HOST arrays of n entries (dw pairwise distinct), each as cvl_conv_wgrad(d[i], x[i], dy[i],
 * dw[i], beta) would form it -- the per-image gradient accumulation of FCOS/train_fcos.py:173-176 for
 * every 1x1 and 3x3 conv of a ResNet stage at once.  The 1x1 bf16 single-segment problems (pad 0,
 * stride 1 or 2, dense rows) share ONE launch per <= 16 and tile width, the 3x3 stride-1 problems the
 * halo weight-gradient kernel takes ONE launch per <= 12 (each problem its own tile grid, a common
 * rows-per-workgroup chunk chosen for the whole launch), with their split reductions deferred as by
 * cvl_wgrad_defer; any other problem runs as its own cvl_conv_wgrad.  Sums are fixed-order
 * (deterministic); the chunking differs from the one-conv calls, so results agree with them to fp32
 * rounding, not bit for bit.  workspace >= cvl_conv_wgrad_batch_workspace_size(d, n). */
size_t cvl_conv_wgrad_batch_workspace_size(const cvl_conv_desc* const* d, int n);
int cvl_conv_wgrad_batch(const cvl_conv_desc* const* d, int n, const void* const* x, const void* const* dy,
                         float* const* dw, float beta, void* workspace, size_t workspace_bytes, cvl_stream_t stream);

/* Test and profiling hooks: what cvl_conv_wgrad_grouped(d, ngroups, ...) would launch, as
 * cvl_conv_igemm_plan for the other half.  Host only: no device memory, no launch.  *kernel (a
 * CVL_CK_WG_* code), *tile (its co tile width) and *nsplit describe the call's LAST launch -- what
 * cvl_conv_igemm_last_kernel() shows after it -- and *workspace is the call's workspace size.  A
 * descriptor the call rejects gets the same status; prec == CVL_PREC_F32 reports CVL_CK_NONE. */
int cvl_conv_wgrad_plan(const cvl_conv_desc* d, int ngroups, int32_t* kernel, int32_t* tile, int32_t* nsplit,
                        size_t* workspace);
/* ... and of cvl_conv_wgrad_batch(d, n, ...), per problem (arrays of n): its kernel, the index of
 * the launch group that runs it (in launch order) and its split count. */
int cvl_conv_wgrad_batch_plan(const cvl_conv_desc* const* d, int n, int32_t* kernel_of, int32_t* launch_of,
                              int32_t* nsplit_of);

/* fp32 HWIO [KH][KW][Cin][Cout] master weights -> bf16 forward pack [Npad][KH*KW*Cin_k]
 * (zero rows >= Cout and channels >= Cin) and/or dgrad pack [Cin_pad][KH*KW*Cout_pad]. */
int cvl_pack_conv_weights(const float* w_hwio, int KH, int KW, int Cin, int Cout, int Cin_k, int Npad,
                          void* w_fwd, int Cin_pad, int Cout_pad, void* w_dgrad, cvl_stream_t stream);

/* Batched form of cvl_pack_conv_weights: every conv of a network in ONE launch (run after each
 * optimizer step).  items: DEVICE array of cvl_pack_item; tiles: DEVICE int32 [ntiles][4] =
 * (item, tap, ci0, co0), one per 64x64 (Cin x Cout) block of each tap, covering ci < max(Cin_k,
 * Cin_pad) and co < max(Npad, Cout_pad) (multiples of 64 from 0).  Cin_k, Cin_pad, Cout_pad % 8 == 0. */
typedef struct {
  const float* w;      /* HWIO fp32 master [KH*KW][Cin][Cout] */
  void* w_fwd;         /* bf16 [Npad][KHW*Cin_k] or NULL */
  void* w_dgrad;       /* bf16 [Cin_pad][KHW*Cout_pad] or NULL */
  int KHW, Cin, Cout, Cin_k, Npad, Cin_pad, Cout_pad;
  int f32_out;         /* 1: w_fwd / w_dgrad are fp32 (the CVL_PREC_F32 parity mode; any Cin_k) */
} cvl_pack_item;
int cvl_pack_conv_weights_multi(const cvl_pack_item* items, const int32_t* tiles, int ntiles,
                                cvl_stream_t stream);
/* The batched forward re-pack with a per-output-channel scale (BatchNorm folded into the conv for
 * inference, ConvBN.fold): w_fwd[co][tap * Cin_k + ci] = bf16_rne(w[tap][ci][co] * scale[co]) (one fp32
 * multiply), zero rows >= Cout and channels >= Cin.  Forward pack only.  tiles as above, covering
 * ci < Cin_k and co < Npad; Cin_k % 8 == 0. */
typedef struct {
  const float* w;      /* HWIO fp32 master [KH*KW][Cin][Cout] */
  const float* scale;  /* fp32 [Cout] */
  void* w_fwd;         /* bf16 [Npad][KHW*Cin_k] */
  int KHW, Cin, Cout, Cin_k, Npad;
} cvl_pack_scaled_item;
int cvl_pack_conv_weights_scaled_multi(const cvl_pack_scaled_item* items, const int32_t* tiles, int ntiles,
                                       cvl_stream_t stream);

/* ResNet stem straight from the image (Keras ResNet50 conv1: ZeroPadding2D(3) + Conv2D(64, 7,
 * strides=2) + bias, behind FCOS/fcos.py:30-46 and RetinaNet/retinanet_module.py:39-72; no im2col
 * matrix in HBM).  img fp32 NHWC [B][H][W][3]; Ho = (H-1)/2+1, Wo = (W-1)/2+1.  K order k = ky*24 +
 * kx*3 + c (each kernel row's 21 taps x channels padded to 24): w_packed = cvl_pack_conv_weights of
 * the HWIO [7][7][3][64] kernel viewed as KH=7, KW=1, Cin=21, Cin_k=24, Npad=64 ([64][168] bf16).
 * Forward: z [B][Ho][Wo][64] bf16 = bf16(conv(bf16(img)) + bias), bn_stats (nullable) = the BN
 * accumulators of z.  Weight gradient: dw [192][64] fp32 = beta*dw + sum over pixels, rows in the
 * same padded K order (HWIO row ky*21+kx*3+c = dw row ky*24+kx*3+c; pad rows 0); deterministic. */
int cvl_stem_conv7x7s2(const float* img, int B, int H, int W, const void* w_packed, const float* bias, void* z,
                       uint64_t* bn_stats, cvl_stream_t stream);
size_t cvl_stem_wgrad_workspace_size(int B, int H, int W);
int cvl_stem_wgrad(const float* img, int B, int H, int W, const void* dz, float* dw, float beta, void* workspace,
                   size_t workspace_bytes, cvl_stream_t stream);

/* fp32 NHWC image -> bf16 im2col rows [B*Ho*Wo][Kp] (ResNet50 conv1 after ZeroPadding2D(3)). */
int cvl_im2col(const float* x, int B, int H, int W, int C, int KH, int KW, int stride, int pad_t,
               int pad_l, int Ho, int Wo, int Kp, void* out, cvl_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * BatchNormalization in training mode with per-image statistics (the reference forwards one
 * image at a time, train_fcos.py:137-153; Keras eps 1.001e-5, momentum 0.99, running variance
 * unbiased as TF's fused kernel).  stats: BN accumulators [B][C][2][S] from cvl_conv_igemm(bn_stats)
 * or cvl_bn_stats; mean_rstd [B][C][2].
 * ---------------------------------------------------------------------------------------- */
int cvl_bn_finalize(uint64_t* stats, float* mean_rstd, float* run_mean, float* run_var, int B,
                    int C, int HW, float eps, float momentum, cvl_stream_t stream);
int cvl_bn_apply(const void* z, const float* mean_rstd, const float* gamma, const float* beta,
                 const void* residual, void* y, int B, int HW, int C, int relu, cvl_stream_t stream);
/* cvl_bn_finalize + cvl_bn_apply in ONE launch (bit-identical results): every block derives the
 * (mean, rstd) of its image from stats; mean_rstd is still written for the backward and the running
 * statistics advanced (run_mean/run_var NULL together: inference-style, no EMA). */
int cvl_bn_finalize_apply(uint64_t* stats, float* mean_rstd, float* run_mean, float* run_var,
                          const void* z, const float* gamma, const float* beta, const void* residual, void* y,
                          int B, int HW, int C, int relu, float eps, float momentum, cvl_stream_t stream);
/* cvl_bn_finalize_apply whose residual is ANOTHER BN's output that was never stored: the projection
 * shortcut of a Keras ResNet block1, y = act(BN_3(z) + BN_0(res_z)).  Both finalizes run in the one
 * launch (res_mean_rstd written, res running statistics advanced with res_eps / res_momentum), and the
 * residual term is bf16(BN_0(res_z)) rounded as the stored shortcut output was: bit-identical to
 * cvl_bn_finalize_apply(res) + cvl_bn_finalize_apply(z, residual) without writing or re-reading it.
 * Replaces the shortcut's apply of resnet.py block1 (Keras applications, behind FCOS/fcos.py:30-35). */
int cvl_bn_finalize_apply_bnres(uint64_t* stats, float* mean_rstd, float* run_mean, float* run_var,
                                const void* z, const float* gamma, const float* beta, uint64_t* res_stats,
                                float* res_mean_rstd, float* res_run_mean, float* res_run_var,
                                const void* res_z, const float* res_gamma, const float* res_beta,
                                float res_eps, float res_momentum, void* y, int B, int HW, int C, int relu,
                                float eps, float momentum, cvl_stream_t stream);
/* dy: grad of y; y_relu: y when the unit ends in ReLU (mask), else NULL; writes dz (bf16),
 * optionally g_out = masked dy (the residual branch's gradient), dgamma/dbeta (= + beta_acc*old)
 * and, if conv_dbias != NULL, the gradient of the preceding conv's bias, which is exactly 0
 * behind training-mode BN (the per-image mean subtraction cancels any constant shift of z).  workspace >= cvl_bn_backward_workspace_size(B, HW, C) bytes; reductions are
 * deterministic (per-block partials summed in a fixed order, no atomics). */
size_t cvl_bn_backward_workspace_size(int B, int HW, int C);
int cvl_bn_backward(const void* dy, const void* y_relu, const void* z, const float* mean_rstd,
                    const float* gamma, void* workspace, size_t workspace_bytes, void* dz, void* g_out,
                    float* dgamma, float* dbeta, float beta_acc, float* conv_dbias, int B, int HW, int C,
                    cvl_stream_t stream);
/* cvl_bn_backward for a unit that ends in ReLU WITHOUT a residual add (the conv1/conv2 units of a
 * Keras ResNet bottleneck, the stem): the ReLU mask is recomputed from z as
 * fma(gamma, (z - mean) * rstd, beta) > 0 -- the forward's own arithmetic (cvl_bn_apply) -- so y
 * is not read (two passes read 2 tensors instead of 3).  beta = the BN's beta parameter. */
int cvl_bn_backward_relu(const void* dy, const void* z, const float* mean_rstd, const float* gamma,
                         const float* beta, void* workspace, size_t workspace_bytes, void* dz, float* dgamma,
                         float* dbeta, float beta_acc, float* conv_dbias, int B, int HW, int C,
                         cvl_stream_t stream);
/* Fused BN-backward first pass.  cvl_conv_igemm_dgrad_bnsum runs a DGRAD conv (beta 0) whose
 * result is dy of a BN -> ReLU (act_hi = INFINITY) / ReLU6 (act_hi = 6) unit without a residual
 * (the bottleneck's conv1 / conv2 units: their dy has one producer) and, when the 256-row
 * LDS-DMA kernel takes the launch with one image per tile, adds per (image, channel)
 * (sum g, sum g*xhat), g = dy * mask(bn(z)), into sums (BN accumulators [B][C][2][S], zero them first) and sets
 * *fused (HOST) = 1; otherwise it runs the plain data gradient and sets *fused = 0.  z / mean_rstd
 * / gamma / beta are the unit's pre-BN conv output (same layout as dst), (mean, rstd) [B][C][2]
 * and BN parameters.  cvl_bn_backward_relu_sums is cvl_bn_backward_relu's second pass from those
 * sums (the first pass and its reduction are skipped). */
int cvl_conv_igemm_dgrad_bnsum(const cvl_conv_desc* d, const void* src, void* dst, const void* z,
                               const float* mean_rstd, const float* gamma, const float* beta, float act_hi,
                               uint64_t* sums, int32_t* fused, void* workspace, size_t workspace_bytes,
                               cvl_stream_t stream);
int cvl_bn_backward_relu_sums(const void* dy, const void* z, const float* mean_rstd, const float* gamma,
                              const float* beta, uint64_t* sums, void* dz, float* dgamma, float* dbeta,
                              float beta_acc, float* conv_dbias, float act_hi, int B, int HW, int C,
                              cvl_stream_t stream);
/* The residual-unit form (a bottleneck's BN3: BN -> + shortcut -> ReLU, the block output y).  The
 * block-input gradient of the NEXT block is completed by its first 1x1 data gradient accumulating
 * into dst (d->beta != 0); cvl_conv_igemm_dgrad_bnsum_res runs that launch and, on the persistent
 * 1x1 kernel, adds (sum g, sum g*xhat), g = final dst * (y > 0), into sums (zeroed) and sets
 * *fused = 1 (else the plain data gradient, *fused = 0).  cvl_bn_backward_res_sums is then that BN
 * backward's second pass from the sums: dz, g_out (= g, the shortcut's gradient) and dgamma/dbeta
 * (replaces cvl_bn_backward with y_relu given). */
int cvl_conv_igemm_dgrad_bnsum_res(const cvl_conv_desc* d, const void* src, void* dst, const void* y, const void* z,
                                   const float* mean_rstd, const float* gamma, const float* beta, uint64_t* sums,
                                   int32_t* fused, void* workspace, size_t workspace_bytes, cvl_stream_t stream);
int cvl_bn_backward_res_sums(const void* dy, const void* y, const void* z, const float* mean_rstd, const float* gamma,
                             uint64_t* sums, void* dz, void* g_out, float* dgamma, float* dbeta, float beta_acc,
                             float* conv_dbias, int B, int HW, int C, cvl_stream_t stream);
/* A projection block's residual unit (Keras ResNet50 block1: conv3 BN -> + shortcut BN -> ReLU, the
 * TF gradient through both BNs behind FCOS/fcos.py:30-35): cvl_bn_backward_res_sums that also forms
 * the shortcut BN backward's first pass on the same masked gradient (the shortcut's dy is g_out) from
 * the shortcut's pre-BN z_sc and (mean, rstd) -- per-block partials in `workspace`, then a fixed-order
 * column sum into sc_sums [B][C][2] (float64 values, slot mode 1); cvl_bn_backward_sums then runs the
 * shortcut's second pass.  The separate first pass over g_out and z_sc is gone. */
size_t cvl_bn_backward_res_sums_sc_workspace_size(int B, int HW, int C);
int cvl_bn_backward_res_sums_sc(const void* dy, const void* y, const void* z, const float* mean_rstd,
                                const float* gamma, uint64_t* sums, void* dz, void* g_out, float* dgamma,
                                float* dbeta, float beta_acc, float* conv_dbias, const void* z_sc,
                                const float* mean_rstd_sc, void* workspace, size_t workspace_bytes,
                                uint64_t* sc_sums, int B, int HW, int C, cvl_stream_t stream);
/* The same when the residual unit's first pass is not fused upstream: cvl_bn_backward (mask y > 0,
 * g_out) whose second pass also forms the shortcut BN's first pass into sc_sums. */
size_t cvl_bn_backward_sc_workspace_size(int B, int HW, int C);
int cvl_bn_backward_sc(const void* dy, const void* y, const void* z, const float* mean_rstd, const float* gamma,
                       void* workspace, size_t workspace_bytes, void* dz, void* g_out, float* dgamma, float* dbeta,
                       float beta_acc, float* conv_dbias, const void* z_sc, const float* mean_rstd_sc,
                       uint64_t* sc_sums, int B, int HW, int C, cvl_stream_t stream);
/* Second pass only of a BN without ReLU from first-pass sums [B][C][2] (slot mode 1). */
int cvl_bn_backward_sums(const void* dy, const void* z, const float* mean_rstd, const float* gamma,
                         const uint64_t* sums, void* dz, float* dgamma, float* dbeta, float beta_acc,
                         float* conv_dbias, int B, int HW, int C, cvl_stream_t stream);

/* The ReLU sign bitmap of a residual unit's output (no reference counterpart: the backward of
 * y = relu(BN(z) + shortcut) uses only the sign of y).  relu_bits: uint8 [B*HW][C/8], dense; bit u of
 * byte [row][c] is 1 where the STORED (bf16-rounded) y[row][8c + u] > 0.  bf16, relu == 1 only.
 * cvl_bn_finalize_apply_bits / _bnres_bits: their namesakes, which also write relu_bits (y is
 * bit-identical).  The *_bits backward entries: their namesakes with relu_bits in y's place (1/16 of
 * the bytes; dz, g_out, sc_sums, dgamma, dbeta bit-identical).
 * cvl_conv_igemm_dgrad_bnsum_res_bits: cvl_conv_igemm_dgrad_bnsum_res with the mask of the fused sums
 * read from relu_bits (laid out as dst: byte (row * ld_dst + dst_coff + n) / 8, so ld_dst and
 * dst_coff must be multiples of 8 -- otherwise the y form runs, hence y is still passed); *form
 * (optional) = 3 bitmap form / 2 y form / 0 not fused.
 * cvl_conv_igemm_plan_bnsum: host-only query, as cvl_conv_igemm_plan, for a fused BN-sums offer
 * (1 z mask, 2 y mask, 3 bitmap): the form that would run (*form, 0 = none: the plain data gradient),
 * kernel family and K-tile. */
int cvl_bn_finalize_apply_bits(uint64_t* stats, float* mean_rstd, float* run_mean, float* run_var, const void* z,
                               const float* gamma, const float* beta, const void* residual, void* y,
                               uint8_t* relu_bits, int B, int HW, int C, int relu, float eps, float momentum,
                               cvl_stream_t stream);
int cvl_bn_finalize_apply_bnres_bits(uint64_t* stats, float* mean_rstd, float* run_mean, float* run_var,
                                     const void* z, const float* gamma, const float* beta, uint64_t* res_stats,
                                     float* res_mean_rstd, float* res_run_mean, float* res_run_var,
                                     const void* res_z, const float* res_gamma, const float* res_beta,
                                     float res_eps, float res_momentum, void* y, uint8_t* relu_bits, int B, int HW,
                                     int C, int relu, float eps, float momentum, cvl_stream_t stream);
int cvl_bn_backward_bits(const void* dy, const uint8_t* relu_bits, const void* z, const float* mean_rstd,
                         const float* gamma, void* workspace, size_t workspace_bytes, void* dz, void* g_out,
                         float* dgamma, float* dbeta, float beta_acc, float* conv_dbias, int B, int HW, int C,
                         cvl_stream_t stream);
int cvl_bn_backward_res_sums_bits(const void* dy, const uint8_t* relu_bits, const void* z, const float* mean_rstd,
                                  const float* gamma, uint64_t* sums, void* dz, void* g_out, float* dgamma,
                                  float* dbeta, float beta_acc, float* conv_dbias, int B, int HW, int C,
                                  cvl_stream_t stream);
int cvl_bn_backward_res_sums_sc_bits(const void* dy, const uint8_t* relu_bits, const void* z, const float* mean_rstd,
                                     const float* gamma, uint64_t* sums, void* dz, void* g_out, float* dgamma,
                                     float* dbeta, float beta_acc, float* conv_dbias, const void* z_sc,
                                     const float* mean_rstd_sc, void* workspace, size_t workspace_bytes,
                                     uint64_t* sc_sums, int B, int HW, int C, cvl_stream_t stream);
int cvl_bn_backward_sc_bits(const void* dy, const uint8_t* relu_bits, const void* z, const float* mean_rstd,
                            const float* gamma, void* workspace, size_t workspace_bytes, void* dz, void* g_out,
                            float* dgamma, float* dbeta, float beta_acc, float* conv_dbias, const void* z_sc,
                            const float* mean_rstd_sc, uint64_t* sc_sums, int B, int HW, int C, cvl_stream_t stream);
int cvl_conv_igemm_dgrad_bnsum_res_bits(const cvl_conv_desc* d, const void* src, void* dst, const void* y,
                                        const uint8_t* relu_bits, const void* z, const float* mean_rstd,
                                        const float* gamma, const float* beta, uint64_t* sums, int32_t* fused,
                                        int32_t* form, void* workspace, size_t workspace_bytes, cvl_stream_t stream);
int cvl_conv_igemm_plan_bnsum(const cvl_conv_desc* d, int offer, size_t workspace_bytes, int32_t* form,
                              int32_t* kernel, int32_t* ktile);

/* BN -> ReLU6 unit without a residual (MobileNetV2: Keras ReLU(6.)): as cvl_bn_backward_relu with
 * the TF Relu6Grad mask 0 < bn(z) < 6 rebuilt from z in fp32 (the forward's exact pre-clamp value);
 * cvl_bn_apply / cvl_bn_finalize_apply take relu = 2 for ReLU6. */
int cvl_bn_backward_relu6(const void* dy, const void* z, const float* mean_rstd, const float* gamma,
                          const float* beta, void* workspace, size_t workspace_bytes, void* dz, float* dgamma,
                          float* dbeta, float beta_acc, float* conv_dbias, int B, int HW, int C, cvl_stream_t stream);

/* ResNet50 pool1: ZeroPadding2D(1) + MaxPooling2D(3, 2); argmax [B][Ho][Wo][C] uint8 (0..8). */
/* Stem BN -> ReLU -> ZeroPadding2D(1) -> MaxPool 3x3/2 fused (Keras ResNet50 conv1_bn .. pool1_pool):
 * from the pre-BN z [B,H,W,C] bf16 and (mean, rstd) [B][C][2]; writes the pooled y and argmax as
 * cvl_maxpool3x3s2 would from the stored BN output (bit-identical), without that full-size output. */
int cvl_bn_relu_maxpool3x3s2(const void* z, const float* mean_rstd, const float* gamma, const float* beta, void* y,
                             uint8_t* argmax, int B, int H, int W, int C, cvl_stream_t stream);
int cvl_maxpool3x3s2(const void* x, void* y, uint8_t* argmax, int B, int H, int W, int C,
                     cvl_stream_t stream);
int cvl_maxpool3x3s2_backward(const void* dy, const uint8_t* argmax, void* dx, int B, int H, int W,
                              int C, cvl_stream_t stream);
/* The stem's backward front (pool1_pool -> conv1_relu -> conv1_bn backward, the TF gradient of
 * Keras ResNet50's first block behind FCOS/fcos.py:30): max-pool backward of dp [B,Ho,Wo,64] through
 * argmax into dy [B,H,W,64] (bit-identical to cvl_maxpool3x3s2_backward) with the BN -> ReLU
 * backward's first pass (mask rebuilt from z) fused into that kernel, then the second pass as
 * cvl_bn_backward_relu (dz, dgamma, dbeta, conv_dbias = 0).  C = 64 (ResNet conv1) only. */
size_t cvl_maxpool3x3s2_backward_bn_relu_workspace_size(int B, int H, int W, int C);
int cvl_maxpool3x3s2_backward_bn_relu(const void* dp, const uint8_t* argmax, const void* z, const float* mean_rstd,
                                      const float* gamma, const float* beta, void* workspace,
                                      size_t workspace_bytes, void* dy, void* dz, float* dgamma, float* dbeta,
                                      float beta_acc, float* conv_dbias, int B, int H, int W, int C,
                                      cvl_stream_t stream);
/* FPN top-down (fcos.py:57-60): out[B,H,W,C] = a + nearest_up2(b[B,H/2,W/2,C]); backward:
 * db = sum of dout over each 2x2 block (+ beta*db). */
int cvl_upsample2x_add(const void* a, const void* b, void* out, int B, int H, int W, int C,
                       cvl_stream_t stream);
int cvl_upsample2x_backward(const void* dout, void* db, int B, int H, int W, int C, float beta,
                            cvl_stream_t stream);
int cvl_relu_backward(const void* dy, const void* y, void* dx, long n, float beta, cvl_stream_t stream);
/* In-place ReLU of n bf16 values (16-byte vectors, any n). */
int cvl_relu_(void* x, long n, cvl_stream_t stream);
int cvl_add(const void* a, const void* b, void* out, long n, cvl_stream_t stream);
/* bias gradient over a segment's rows: db[c] = beta*db + sum dy[row][coff + c] (rows base +
 * b*img_stride + q, q < HW); deterministic (per-block partials summed in a fixed order).  Needs
 * ld, coff % 8 == 0 and coff + round_up(ncol, 8) <= ld; workspace >= *_workspace_size bytes. */
size_t cvl_bias_grad_workspace_size(int ncol, int HW, int B);
int cvl_bias_grad(const void* dy, int ld, int coff, int ncol, int64_t base, int64_t img_stride, int HW,
                  int B, void* workspace, size_t workspace_bytes, float* db, float beta, cvl_stream_t stream);
/* Batched form of cvl_bias_grad: up to CVL_BIAS_MAX_ITEMS bias gradients (e.g. the per-level
 * heads `logits_output_l` / `reg_output_l` of FCOS/fcos.py:85-101, the FPN convs of fcos.py:49-74)
 * in ONE partial-sum launch + ONE fixed-order finish launch.  items: HOST array (passed by value to
 * the kernels, so the call is graph-capturable); same per-item contract as cvl_bias_grad with
 * ncol <= 2048; workspace >= cvl_bias_grad_multi_workspace_size(items, n) bytes. */
#define CVL_BIAS_MAX_ITEMS 16
typedef struct {
  const void* dy;      /* bf16 rows [*][ld] */
  float* db;           /* fp32 [ncol] */
  int64_t base, img_stride;
  int ld, coff, ncol, HW, B;
  float beta;
} cvl_bias_item;
size_t cvl_bias_grad_multi_workspace_size(const cvl_bias_item* items, int n);
int cvl_bias_grad_multi(const cvl_bias_item* items, int n, void* workspace, size_t workspace_bytes,
                        cvl_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * fp32 parity mode (SURVEY.md §8b "Parity modes", CVL_PRECISION=fp32): the same training graph
 * with fp32 activations and activation gradients, for whole-graph parity with the reference's
 * fp32 Keras graph (FCOS/fcos.py:6-110, RetinaNet/retinanet_module.py:8-159).  Convolutions take
 * cvl_conv_desc.prec = CVL_PREC_F32; the memory-bound ops below are the fp32 forms of the
 * entry points of the same names (same arguments, float tensors; every reduction fixed-order).
 * cvl_bn_backward_f32 covers cvl_bn_backward (y_relu = the ReLU output, bn_beta NULL) and
 * cvl_bn_backward_relu (y_relu NULL, bn_beta = the BN's beta: mask rebuilt from z), act_hi =
 * INFINITY (ReLU) or 6 (ReLU6); workspace >= cvl_bn_backward_f32_workspace_size(B, C).
 * cvl_bias_grad_multi_f32 takes cvl_bias_item rows of fp32 dy (no workspace).
 * ---------------------------------------------------------------------------------------- */
int cvl_bn_apply_f32(const float* z, const float* mean_rstd, const float* gamma, const float* beta,
                     const float* residual, float* y, int B, int HW, int C, int relu, cvl_stream_t stream);
int cvl_bn_finalize_apply_f32(uint64_t* stats, float* mean_rstd, float* run_mean, float* run_var,
                              const float* z, const float* gamma, const float* beta, const float* residual,
                              float* y, int B, int HW, int C, int relu, float eps, float momentum,
                              cvl_stream_t stream);
size_t cvl_bn_backward_f32_workspace_size(int B, int C);
int cvl_bn_backward_f32(const float* dy, const float* y_relu, const float* z, const float* mean_rstd,
                        const float* gamma, const float* bn_beta, void* workspace, size_t workspace_bytes,
                        float* dz, float* g_out, float* dgamma, float* dbeta, float beta_acc,
                        float* conv_dbias, float act_hi, int B, int HW, int C, cvl_stream_t stream);
int cvl_maxpool3x3s2_f32(const float* x, float* y, uint8_t* argmax, int B, int H, int W, int C,
                         cvl_stream_t stream);
int cvl_maxpool3x3s2_backward_f32(const float* dy, const uint8_t* argmax, float* dx, int B, int H, int W,
                                  int C, cvl_stream_t stream);
int cvl_upsample2x_add_f32(const float* a, const float* b, float* out, int B, int H, int W, int C,
                           cvl_stream_t stream);
int cvl_upsample2x_backward_f32(const float* dout, float* db, int B, int H, int W, int C, float beta,
                                cvl_stream_t stream);
int cvl_relu_backward_f32(const float* dy, const float* y, float* dx, long n, float beta, cvl_stream_t stream);
int cvl_add_f32(const float* a, const float* b, float* out, long n, cvl_stream_t stream);
int cvl_bias_grad_multi_f32(const cvl_bias_item* items, int n, cvl_stream_t stream);
/* cvl_retina_loss with fp32 gradient outputs (the parity mode's RetinaNet heads). */
int cvl_retina_loss_f32(const float* reg_pred, int ld_reg, const float* cls_pred, int ld_cls, const float* targets,
                        int B, const int32_t* level_cells, int n_anchors, int num_classes, const float* img_weight,
                        float grad_scale, float* losses, float* d_reg, int ld_dreg, float* d_cls, int ld_dcls,
                        void* workspace, cvl_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer (train_fcos.py:179-185): g <- (g * inv_bs) clipped by global norm `clip`
 * (tf.clip_by_global_norm), then Keras SGD momentum v = m*v - lr*g; w += v.  Flat fp32 buffers;
 * lr read from device memory (graph-capturable); sumsq_ws: CVL_SUMSQ_WS float64 (total + the
 * per-block partials of the deterministic norm reduction); w / g / v 16-byte aligned.
 * cvl_lr_schedule: lr = max(init*rate^floor(step/decay_step), min_lr); step += 1 (device ints).
 * cvl_lr_schedule_capped: the same with the exponent capped at max_decays (>= 0): the centre
 * variants' step schedule (FCOS/train_fcos_center_voc.py:150-157: init_lr below step 8000, init/10
 * from then on -- its init/100 branch is unreachable) is rate 0.1, decay_step 8000, max_decays 1.
 * ---------------------------------------------------------------------------------------- */
#define CVL_SUMSQ_WS 1025
int cvl_sgd_clip_update(float* w, const float* g, float* v, int64_t n, const float* lr_dev,
                        float momentum, float inv_bs, float clip, double* sumsq_ws, cvl_stream_t stream);
int cvl_lr_schedule(int32_t* step, float* lr, double init_lr, double min_lr, double decay_rate,
                    int decay_step, cvl_stream_t stream);
int cvl_lr_schedule_capped(int32_t* step, float* lr, double init_lr, double min_lr, double decay_rate,
                           int decay_step, int max_decays, cvl_stream_t stream);

/* l2_params_reg of train_fcos.py:118-120 = sum over tensors v of sqrt(sum(tf.nn.l2_loss(v)))
 * = sum_v sqrt(0.5 * sum(v^2)), over the tensors at device offsets[i] / sizes[i] of the flat
 * parameter buffer; terms: n_tensors floats of workspace; *out (device float).  The reference
 * computes it outside the GradientTape, so it enters the reported loss, not the gradient. */
int cvl_l2_params_reg(const float* flat, const int64_t* offsets, const int64_t* sizes, int n_tensors,
                      float* terms, float* out, cvl_stream_t stream);

/* RetinaNet candidate selection (train_retinanet_coco.py:190-209: images without matches are
 * skipped, the first batch_size usable candidates are trained on): idx[k] = the first k indices
 * i < n (in order) with counts[i] > 0, weight[k] = 1 for a filled slot and 0 for an empty one.
 * cvl_gather_rows: dst row i = src row idx[i], rows of row_bytes (multiple of 16). */
int cvl_select_first_nonzero(const int32_t* counts, int n, int k, int32_t* idx, float* weight,
                             cvl_stream_t stream);
int cvl_gather_rows(const void* src, int64_t row_bytes, const int32_t* idx, int n, void* dst, cvl_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * RetinaNet target assignment.  Replaces RetinaNet/retinanet_module.py:205-365
 * (`RetinaNet.__init__` anchor dims are passed in; `get_anchors` + `format_data` + utils.compute_iou
 * run per output cell): anchor_dims [5][n_anchors][2] fp32 (h, w); square pad (pad x pad);
 * output targets [B][sum_l n_anchors*S_l^2][4+C] ordered (level, anchor, u, v), the reference's
 * nested [5][9] maps of [S,S,4+C] (float64 there) rounded to fp32, bit-exact; match iff fp32
 * IoU > iou_thresh; num_targets[b] = number of (box, anchor) matches. */
int cvl_retina_assign(const float* boxes, const int32_t* nbox, const float* img_dim, int B, int n_max,
                      int pad, int num_classes, const float* anchor_dims, int n_anchors,
                      const int32_t* strides /*host[5]*/, float iou_thresh, float* targets,
                      int32_t* num_targets, cvl_stream_t stream);

/* CenterNet (hourglass) centroid targets: CenterNet/tf_centernet_hourglass.py:379-456.
 * Output [B][pad_w/stride][pad_h/stride][4+C] (the reference's h_max/w_max swap kept). */
int cvl_centernet_assign(const float* boxes, const int32_t* nbox, const float* img_dim, int B, int n_max,
                         int pad_h, int pad_w, int num_classes, int stride, float* targets,
                         cvl_stream_t stream);

/* CenterNet centre "splat": CenterNet/tf_centernet.py:152-342 (inverse-power kernel, spread 8,
 * sigma sub-box).  Output [B][pad_h/stride][pad_w/stride][5+C]. */
int cvl_centernet_splat(const float* boxes, const int32_t* nbox, const float* img_dim, int B, int n_max,
                        int pad_h, int pad_w, int num_classes, int stride, float sigma, float* targets,
                        cvl_stream_t stream);
/* CenterNet/tf_centernet.py:6-19 center_dist_1d (grid_y NULL) / center_dist_2d: out[i] =
 * g[i] / max(g), g = 1 / (grid_x - mu_x)^spread [* 1 / (grid_y - mu_y)^spread], float64, n points. */
int cvl_center_dist(const double* grid_x, const double* grid_y, int n, double mu_x, double mu_y, double spread,
                    double* out, cvl_stream_t stream);

/* Focal (alpha .25, gamma 2) on C class logits + smooth-L1 on 4 box channels masked by
 * max(class target) > 0: CenterNet model_loss (tf_centernet_hourglass.py:492-505) and one
 * (level, anchor) term of RetinaNet.train_loss (retinanet_module.py:403-426).  targets
 * [B][P][4+C]; losses [B][2] = (cls, reg); d_reg / d_cls (fp32, same strides) nullable. */
size_t cvl_det_loss_workspace_size(int B, int P);
int cvl_det_loss(const float* reg_pred, int ld_reg, const float* cls_pred, int ld_cls, const float* targets,
                 int B, int P, int num_classes, float grad_scale_cls, float grad_scale_reg, float* losses,
                 float* d_reg, float* d_cls, void* workspace, cvl_stream_t stream);

/* RetinaNet.train_loss fwd + bwd over all (level, anchor) terms (retinanet_module.py:367-426) in
 * one launch.  reg_pred / cls_pred: the grouped head outputs [B][P][ld] fp32 (P = sum of
 * level_cells, level-major cells; anchor a's boxes at channels 4a..4a+3, its classes at
 * aC..aC+C-1); targets: cvl_retina_assign's [B][n_anchors*P][4+C] in (level, anchor, cell) order.
 * losses [B][2] = (cls, reg) sums; d_reg / d_cls (nullable): bf16 grad_scale * dloss/dpred at the
 * prediction positions (other channels untouched).  img_weight [B] (nullable) multiplies image b's
 * loss and gradient (0 = an image the reference loop skipped for having no matches). */
size_t cvl_retina_loss_workspace_size(int B, int P, int n_anchors);
int cvl_retina_loss(const float* reg_pred, int ld_reg, const float* cls_pred, int ld_cls, const float* targets,
                    int B, const int32_t* level_cells /*host[5]*/, int n_anchors, int num_classes,
                    const float* img_weight, float grad_scale, float* losses, void* d_reg, int ld_dreg,
                    void* d_cls, int ld_dcls, void* workspace, cvl_stream_t stream);

/* Greedy per-class NMS (CenterNet/tf_centernet_hourglass.py:44-85, method 'nms'): boxes [n][6] =
 * (x1, y1, x2, y2, score, cls) float64; classes [ncls] processed in the given order; keep
 * [ncls][n] indices in selection order (first maximum among survivors), nkeep [ncls]. */
size_t cvl_nms_workspace_size(int n, int ncls);
int cvl_nms(const double* boxes, int n, const double* classes, int ncls, double iou_threshold,
            int32_t* keep, int32_t* nkeep, void* workspace, cvl_stream_t stream);
/* Soft-NMS (tf_centernet_hourglass.py:44-85, method 'soft-nms'; Bodla et al. 2017, Gaussian
 * decay): per class, emit the first maximum of the running scores, then scale every survivor's
 * score by exp(-(iou^2 / sigma)) (float64) and drop scores that are no longer > 0.  Same layout as
 * cvl_nms plus keep_score [ncls][n] = the emitted (decayed) score of each kept row. */
size_t cvl_soft_nms_workspace_size(int n, int ncls);
int cvl_soft_nms(const double* boxes, int n, const double* classes, int ncls, double sigma, int32_t* keep,
                 double* keep_score, int32_t* nkeep, void* workspace, cvl_stream_t stream);

/* ==========================================================================================
 * CenterNet hourglass training path (CenterNet/tf_centernet_hourglass.py:87-353 build_model,
 * :492-564 model_loss / train_step).
 * ========================================================================================== */

/* BatchNormalization over sub-batches: train_step (:527-545) runs one Keras training-mode forward
 * per sub-batch of `group` images, so statistics span the sub-batch (groups [g*G, min(g*G+G, B)),
 * the last may be short); running stats are updated once per group, in order.
 * cvl_bn_stats: stats[b][c] = (sum, sum of squares) over H*W of a bf16 NHWC tensor (BN
 *   accumulators [B][C][2][S], deterministic), the input of cvl_bn_finalize[_grouped].
 * cvl_bn_backward_grouped: as cvl_bn_backward (no ReLU output / conv bias terms) with group
 *   statistics; dz = BN-backward + dz_beta * dz (accumulate into an existing gradient). */
size_t cvl_bn_stats_workspace_size(int B, int HW, int C);
int cvl_bn_stats(const void* x, int B, int HW, int C, uint64_t* stats, void* workspace, size_t workspace_bytes,
                 cvl_stream_t stream);
int cvl_bn_finalize_grouped(const uint64_t* stats, float* mean_rstd, float* run_mean, float* run_var, int B, int C,
                            int HW, int group, float eps, float momentum, cvl_stream_t stream);
size_t cvl_bn_backward_grouped_workspace_size(int B, int HW, int C);
int cvl_bn_backward_grouped(const void* dy, const void* y_relu, const void* z, const float* mean_rstd,
                            const float* gamma, void* workspace, size_t workspace_bytes, void* dz, float dz_beta,
                            float* dgamma, float* dbeta, int B, int HW, int C, int group, cvl_stream_t stream);

/* downsample_block (:158-161): MaxPooling2D(2, 2, "same") -> [B][ceil(H/2)][ceil(W/2)][C];
 * argmax [B][Ho][Wo][C] uint8 (0..3, first maximum in window order). */
int cvl_maxpool2x2(const void* x, void* y, uint8_t* argmax, int B, int H, int W, int C, cvl_stream_t stream);
int cvl_maxpool2x2_backward(const void* dy, const uint8_t* argmax, void* dx, int B, int H, int W, int C,
                            cvl_stream_t stream);

/* Decoder merge (:276-284): out[B][2h][2w][C] = other + UpSampling2D(bilinear)(prev[B][h][w][C]),
 * TF resize_bilinear with half-pixel centres.  Backward: dprev = adjoint(dout) (+ beta * dprev). */
int cvl_upsample_bilinear2x_add(const void* prev, const void* other, void* out, int B, int h, int w, int C,
                                cvl_stream_t stream);
int cvl_upsample_bilinear2x_backward(const void* dout, void* dprev, int B, int h, int w, int C, float beta,
                                     cvl_stream_t stream);

/* Depthwise convolution (Keras DepthwiseConv2D, depth_multiplier 1, no bias; the MobileNetV2
 * backbone of FCOS/fcos.py:36-41 and its siblings): x [B][H][W][C] bf16, w [k][k][C] fp32 (Keras
 * depthwise_kernel [k][k][C][1]), y [B][Ho][Wo][C] bf16, explicit top/left padding (TF "same" or
 * ZeroPadding2D(correct_pad) + "valid"), C % 8 == 0.  dgrad: dx = beta*dx + conv^T(dy).  wgrad
 * (k = 3): dw = beta*dw + sum over all output pixels, deterministic; workspace >= *_size. */
int cvl_depthwise_fwd(const void* x, const float* w, void* y, int B, int H, int W, int C, int k, int stride,
                      int pad_t, int pad_l, int Ho, int Wo, cvl_stream_t stream);
int cvl_depthwise_dgrad(const void* dy, const float* w, void* dx, int B, int H, int W, int C, int k, int stride,
                        int pad_t, int pad_l, int Ho, int Wo, float beta, cvl_stream_t stream);
size_t cvl_depthwise_wgrad_workspace_size(int B, int Ho, int Wo, int C, int k);
int cvl_depthwise_wgrad(const void* x, const void* dy, float* dw, float beta, int B, int H, int W, int C, int k,
                        int stride, int pad_t, int pad_l, int Ho, int Wo, void* workspace, size_t workspace_bytes,
                        cvl_stream_t stream);

/* Grouped 3x3 convolution (the 32-group 3x3 of the ResNeXt bottleneck; the ResNeXt50 / ResNeXt101
 * branch of RetinaNet/retinanet_module.py:53-66): x [B][H][W][C] bf16, fp32 master kernel
 * w [3][3][Cg][C] (output channel o is in group o / Cg and reads input channels (o / Cg) * Cg .. + Cg),
 * y [B][Ho][Wo][C] bf16, ZeroPadding2D(1) + "valid" (pad 1 top / left), Ho = (H - 1) / stride + 1.
 * C % 32 == 0, Cg in {4, 8, 16, 32}, stride 1 or 2; anything else is CVL_EINVAL.
 * The kernels read bf16 slab images of the kernel: *_pack writes the forward image and / or the
 * data-gradient image (either may be null), each *_packed_bytes large
 * (retinanet_module.py:53-66). */
size_t cvl_gconv3x3_packed_bytes(int C);
int cvl_gconv3x3_pack(const float* w, int C, int Cg, void* w_fwd, void* w_dgrad, cvl_stream_t stream);
/* y = conv(x); bn_stats (or null): BN accumulators [B][C][2][S] of the rounded outputs, added to
 * (retinanet_module.py:53-66). */
int cvl_gconv3x3_fwd(const void* x, const void* w_fwd, void* y, uint64_t* bn_stats, int B, int H, int W, int C, int Cg,
                     int stride, int Ho, int Wo, cvl_stream_t stream);
/* dx [B][H][W][C] = beta*dx + conv^T(dy [B][Ho][Wo][C]) on the data-gradient image
 * (retinanet_module.py:53-66). */
int cvl_gconv3x3_dgrad(const void* dy, const void* w_dgrad, void* dx, int B, int H, int W, int C, int Cg, int stride,
                       int Ho, int Wo, float beta, cvl_stream_t stream);
/* dw [3][3][Cg][C] fp32 = beta*dw + sum over all output pixels of x (x) dy; partial sums reduced in a
 * fixed order (bit-identical run to run); workspace >= *_size (retinanet_module.py:53-66). */
size_t cvl_gconv3x3_wgrad_workspace_size(int B, int H, int W, int C, int Cg, int stride);
int cvl_gconv3x3_wgrad(const void* x, const void* dy, float* dw, float beta, int B, int H, int W, int C, int Cg,
                       int stride, int Ho, int Wo, void* workspace, size_t workspace_bytes, cvl_stream_t stream);
/* What the next launch with these arguments would use, CVL_DISPATCH hooks (gc_tpw, gw_wgs) included;
 * host only, touches no device.  kind 0 = fwd, 1 = dgrad, 2 = wgrad.  fwd / dgrad: tpw (destination
 * tiles a workgroup walks down a column), ychunks = ceil(tiles_y / tpw), the destination tile grid;
 * wgrad: the output tile grid, tpc (pixel tiles a workgroup accumulates) and nchunk (partials the
 * reduce sums; workspace = nchunk * 9 * Cg * C * 4 bytes).  Fields that do not apply are written
 * as 0; any pointer may be null.  CVL_EINVAL for the geometries the kernels reject. */
int cvl_gconv3x3_plan(int kind, int B, int H, int W, int C, int Cg, int stride, int* tpw, int* ychunks, int* tiles_x,
                      int* tiles_y, int* tpc, int* nchunk);

/* bn_data: the BatchNormalization(scale=False) on the fp32 input image [B][H][W][3] in front of the
 * ResNeXt stem (retinanet_module.py:53-66).  *_stats: per-image (mean, rstd) [B][3][2] and the
 * moving-average update of run_mean / run_var [3] (either may be null), deterministic; *_apply:
 * out = (img - mean) * rstd + beta. */
size_t cvl_bn_data_stats_workspace_size(int B);
int cvl_bn_data_stats(const float* img, int B, int H, int W, float eps, float momentum, float* mean_rstd,
                      float* run_mean, float* run_var, void* workspace, size_t workspace_bytes, cvl_stream_t stream);
int cvl_bn_data_apply(const float* img, const float* mean_rstd, const float* beta, float* out, int B, int H, int W,
                      cvl_stream_t stream);

/* CenterNet v2 (CenterNet/tf_hourglass_net.py:115-449, n_filters 12 in train_hourglass_voc.py:298-331)
 * --------------------------------------------------------------------------------------------
 * out = UpSampling2D(bilinear)(a + b) (:252-305; b nullable): taps of a + b in fp32, one pass. */
int cvl_upsample_bilinear2x_sum(const void* a, const void* b, void* out, int B, int h, int w, int C,
                                cvl_stream_t stream);
/* The "pass through" reshape-concat (:307-344): map k [B][hw][c_ld] bf16 (c real channels, pads
 * zero) is tf.reshape'd to [B][S2][c*hw/S2] (row-major reinterpretation, Q36) and the maps are
 * concatenated on channels into dst [B][S2][ld_dst] (columns past the sum zeroed).  c % 4 == 0,
 * (c*hw/S2) % 4 == 0.  Backward: dsrc = beta*dsrc + the inverse gather of d_dst (pads of dsrc
 * written zero when beta == 0).  items: HOST array. */
#define CVL_RC_MAX_ITEMS 16
typedef struct {
  const void* src;     /* forward source map */
  void* dsrc;          /* backward destination (gradient of the map) */
  int c, c_ld, hw;     /* real channels, channel pitch, pixels per image */
  float beta;          /* backward accumulate factor */
} cvl_rc_item;
int cvl_reshape_concat(const cvl_rc_item* items, int n_items, int B, int S2, void* dst, int ld_dst,
                       cvl_stream_t stream);
int cvl_reshape_concat_backward(const cvl_rc_item* items, int n_items, int B, int S2, const void* d_dst,
                                int ld_dst, cvl_stream_t stream);
/* b_focal on every scale's class channels (:380-385): b_eff[c] = bias[c] + ((c % period) >= c0 ?
 * *scalar : 0); unfold: g_bias = g_eff, *g_scalar = sum over those channels (fixed order). */
int cvl_bias_scalar_fold_periodic(const float* bias, const float* scalar, float* b_eff, int n, int period, int c0,
                                  cvl_stream_t stream);
int cvl_bias_scalar_unfold_periodic(const float* g_eff, float* g_bias, float* g_scalar, int n, int period, int c0,
                                    cvl_stream_t stream);
/* Targets of train_hourglass_voc.py train() :96-160 for one batch: boxes [B][n_max][5] = the
 * dataset's corner rows + label (utils.convert_to_xywh :16-27 applied inside), one (raw_dims,
 * img_dims) per batch (pad_dims = (img - raw) / 2); targets [B][S][S][4][5+C] fp32, S = img/8:
 * ascending w*h*100, last writer per (cell, scale) sets (y_off, x_off, h_reg, w_reg, 1), class
 * bits OR'd.  Bit-exact to the reference's float32 arithmetic. */
int cvl_hourglass_v2_assign(const float* boxes, const int32_t* nbox, int B, int n_max, int raw_dims, int img_dims,
                            int num_classes, float* targets, cvl_stream_t stream);
/* model_loss (:398-413) fwd + bwd off the head conv: pred [B*P][ld_pred] fp32 (channel sc*(5+C)+j,
 * b_focal folded), targets [B*P][4][5+C]; loss_type bit 0: sigmoid cross-entropy (else focal) on
 * channels 4..4+C; L1 on sigmoid(pred[0..3]) masked by t[4] (bit 1: pred[0..3] are already the
 * model's sigmoid outputs, as model_loss receives them).  losses [B][2] = (cls, reg); d_pred bf16
 * [B*P][ld_d] = d(cls_scale*cls + reg_scale*reg)/d(pred).  workspace >= *_workspace_size(B, P). */
/* CenterNet ResNet stride-8 multi-scale (CenterNet/tf_centernet_resnet_s8.py) targets, format_data
 * (:243-330) batched: boxes [B][n_max][5] normalised (y, x, h, w, cls) fp32, img_dim [B][2] the
 * resized size, (pad_h, pad_w) the padded size, box_scales HOST [n_scales] (<= 8), stride 8 in the
 * reference.  targets [B][pad_w/stride][pad_h/stride][n_scales][4+C] fp32; float64 arithmetic
 * (the reference's gt_labels are float64), bit-exact. */
int cvl_centernet_s8_assign(const float* boxes, const int32_t* nbox, const float* img_dim, int B, int n_max,
                            int pad_h, int pad_w, int num_classes, const float* box_scales, int n_scales, int stride,
                            float* targets, cvl_stream_t stream);
/* model_loss (:368-385) fwd + bwd off the two head convs: reg_pred [B*P][ld_reg] (n_scales x 4 raw
 * box logits per cell, sigmoid applied here), cls_pred [B*P][ld_cls] (n_scales x C logits),
 * targets [B*P][n_scales][4+C]; focal + smooth-L1 of sigmoid(box) masked by max(class) > 0.
 * losses [B][2] = (cls, reg); d_reg / d_cls bf16 (pitches ld_dreg / ld_dcls, pads zeroed). */
size_t cvl_centernet_s8_loss_workspace_size(int B, int P, int n_scales);
int cvl_centernet_s8_loss(const float* reg_pred, int ld_reg, const float* cls_pred, int ld_cls, const float* targets,
                          int B, int P, int n_scales, int num_classes, float cls_scale, float reg_scale, float* losses,
                          void* d_reg, int ld_dreg, void* d_cls, int ld_dcls, void* workspace, cvl_stream_t stream);
size_t cvl_hourglass_v2_loss_workspace_size(int B, int P);
int cvl_hourglass_v2_loss(const float* pred, int ld_pred, const float* targets, int B, int P, int num_classes,
                          int loss_type, float cls_scale, float reg_scale, float* losses, void* d_pred, int ld_d,
                          void* workspace, cvl_stream_t stream);

/* SeparableConv2D (:110-123, :178-181; depth_multiplier 1) runs as ONE dense conv on the MFMA
 * conv kernels with the folded kernel W[t][ci][co] = D[t][ci] * P[ci][co] (t = kh*kw taps; D =
 * Keras depthwise_kernel [kh][kw][Cin][1], P = pointwise_kernel [1][1][Cin][Cout]).
 * cvl_sep_fold_multi writes weff (fp32 HWIO) for every item; cvl_sep_unfold_multi turns the dense
 * kernel gradient gweff into gdw / gpw (weff / gweff [t][cin_ld][cout_ld] when the pitches are set,
 * pads untouched).  rows: DEVICE int32 [nrows][2] = (item, ci), one row per
 * input channel of every item.  items: DEVICE array. */
typedef struct {
  const float* dw;
  const float* pw;
  float* weff;
  const float* gweff;
  float* gdw;
  float* gpw;
  int taps, cin, cout;
  int cin_ld, cout_ld;  /* weff / gweff channel pitches (0 = cin / cout): padded dense kernels */
  int pad_;
} cvl_sep_item;
int cvl_sep_fold_multi(const cvl_sep_item* items, const int32_t* rows, int nrows, cvl_stream_t stream);
int cvl_sep_unfold_multi(const cvl_sep_item* items, const int32_t* rows, int nrows, cvl_stream_t stream);

/* BiasLayer b_focal (tf_bias_layer.py:4-14; :347) folded into the output conv bias:
 * b_eff[c] = bias[c] + (c >= c0 ? *scalar : 0); unfold: g_bias = g_eff, *g_scalar = sum_{c>=c0} g_eff. */
int cvl_bias_scalar_fold(const float* bias, const float* scalar, float* b_eff, int n, int c0, cvl_stream_t stream);
int cvl_bias_scalar_unfold(const float* g_eff, float* g_bias, float* g_scalar, int n, int c0, cvl_stream_t stream);

/* model_loss (:492-505) fwd + bwd off the output conv: pred [B*P][ld_pred] fp32 (reg 0..3, class
 * logits 4..4+C), targets [B*P][4+C] (cvl_centernet_assign); losses [B][2] = (cls, reg) sums;
 * d_pred bf16 [B*P][ld_d] = d(cls_scale*cls + reg_scale*reg)/d(pred), channels >= 4+C zeroed.
 * workspace >= cvl_det_loss_workspace_size(B, P). */
int cvl_centernet_loss(const float* pred, int ld_pred, const float* targets, int B, int P, int num_classes,
                       float cls_scale, float reg_scale, float* losses, void* d_pred, int ld_d, void* workspace,
                       cvl_stream_t stream);

/* obj_detect_results decode (tf_centernet_hourglass.py:576-650, before `nms`): pred [H][W][ld] fp32
 * (one image of the model output: ltrb 0..3, class logits 4..4+C) -> rows [n][6] float64 =
 * (x_low, y_low, w, h, int(100 * max prob), argmax class) for every cell whose max sigmoid
 * probability >= thresh, in np.nonzero (row-major) order; *count = n (<= H*W).  stride = the
 * reference's `downsample`; w_ratio = img_width / img_rows, h_ratio = img_height / img_cols with
 * img_width/img_height the source image's shape[0]/shape[1] (as the reference names them). */
int cvl_centernet_decode(const float* pred, int ld, int H, int W, int num_classes, double stride, float thresh,
                         double w_ratio, double h_ratio, double img_width, double img_height, double* rows,
                         int32_t* count, cvl_stream_t stream);

/* The variant CenterNets' obj_detect_results decodes (one image, before any plotting): pred
 * [H][W][ld] fp32 with scale s's channels at s*ch_per_scale (4 box channels, the class logits at
 * cls0 .. cls0+num_classes-1); rows [n][6] float64 for every (scale, cell) whose max sigmoid class
 * probability >= thresh, scale-major and np.nonzero order within a scale; *count = n (<= n_scales*H*W).
 * box_mode 1 = CenterNet/tf_centernet_resnet_s8.py:446-547 (prediction_to_corners :210-241 with
 *   box_scales[s] and `stride` = downsample, then (x_low, y_low, w, h, int(100 p), argmax class):
 *   the input of `nms` :44-85, iou 0.213);
 * box_mode 2 = CenterNet/tf_hourglass_net.py:517-578 (stride 8, box_scales[s] = the per-scale box
 *   scale of :518-524): (x_lower, y_lower, box_width, box_height, int(100 p), class index) of the
 *   drawn rectangles (x = the row axis, as the reference names it; cls0 = 5 skips channel 4 when the
 *   model has more than one class channel).
 * w_ratio = img_width / img_rows, h_ratio = img_height / img_cols (the source image's shape[0] /
 * shape[1], as the reference names them).  n_scales <= 16. */
int cvl_centernet_scale_decode(const float* pred, int ld, int H, int W, int n_scales, int ch_per_scale, int cls0,
                               int num_classes, int box_mode, const double* box_scales /*host[n_scales]*/,
                               float stride, float thresh, double w_ratio, double h_ratio, double img_width,
                               double img_height, double* rows, int32_t* count, cvl_stream_t stream);

/* CenterNet 3x3 max-pool peak decode (the north_star's peak decode; the reference's own decode is
 * cvl_centernet_decode above): pred [B][H][W][ld] fp32 (ltrb 0..3, class logits 4..4+C).  A
 * (cell, class) is a peak when sigmoid(logit) equals the 3x3 max-pool of its class map (-inf
 * padding, ties kept) and >= thresh; per image the K highest (probability desc, flat index
 * cell*C+class asc) peaks -> dets [B][K][6] float64 = (y_lo, x_lo, y_hi, x_hi, prob, class), the
 * corners as prediction_to_corners (tf_centernet_hourglass.py:355-377) x stride in fp32;
 * count [B] = rows written (<= K).  Sigmoid in float64 rounded to fp32.  Deterministic.
 * workspace >= cvl_centernet_peak_decode_workspace_size(B, H, W, C). */
size_t cvl_centernet_peak_decode_workspace_size(int B, int H, int W, int num_classes);
int cvl_centernet_peak_decode(const float* pred, int ld, int B, int H, int W, int num_classes, float stride,
                              float thresh, int K, double* dets, int32_t* count, void* workspace,
                              size_t workspace_bytes, cvl_stream_t stream);

/* train_step update (:555-563) with tf.keras.optimizers.Adam (train_hourglass_voc.py:330):
 * g <- clip_by_global_norm(g * inv_bs, clip); t = *iterations + 1;
 * m += (g - m)(1 - b1); v += (g^2 - v)(1 - b2); w -= lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps);
 * then *iterations += 1.  lr read from device memory; sumsq_ws: one float64. */
int cvl_adam_clip_update(float* w, const float* g, float* m, float* v, int64_t n, const float* lr_dev,
                         int32_t* iterations, float beta1, float beta2, float eps, float inv_bs, float clip,
                         double* sumsq_ws, cvl_stream_t stream);

/* ==========================================================================================
 * RetinaNet inference decode (RetinaNet/retinanet_module.py:428-529).
 * ========================================================================================== */

/* prediction_to_corners (:428-451) of one (level, anchor) map: xy [H][W][ld] fp32 (t_y, t_x, t_h,
 * t_w at 0..3) -> out [H][W][4] = (y1, x1, y2, x2) fp32, centre = (col|row) * stride - t * anchor
 * (no +0.5, Q21), size = t * anchor; the reference's fp32 operation order. */
int cvl_retina_corners(const float* xy, int ld, int H, int W, float anchor_h, float anchor_w, int stride,
                       float* out, cvl_stream_t stream);

/* image_detections (:483-520) up to cpu_nms, for B images of the fused head outputs
 * (reg [B][P][ld_reg]: anchor a at 4a..4a+3; cls [B][P][ld_cls]: anchor a at aC..aC+C-1; rows
 * level-major, P = sum h*w).  level_hw [5][2] and strides [5] are HOST arrays; anchor_dims
 * [5][A][2] fp32 (h, w) on the device.  dets [B][A*P][6] fp32 = (y1, x1, y2, x2, max sigmoid
 * prob, first-argmax class) for the rows with prob >= cls_thresh, in the reference's
 * concatenation order (level, anchor, row-major cell); count [B] (device). */
size_t cvl_retina_decode_workspace_size(int B, const int32_t* level_hw, int n_anchors);
int cvl_retina_decode(const float* reg_pred, int ld_reg, const float* cls_pred, int ld_cls, int B,
                      const int32_t* level_hw, const int32_t* strides, const float* anchor_dims, int n_anchors,
                      int num_classes, float cls_thresh, float* dets, int32_t* count, void* workspace,
                      size_t workspace_bytes, cvl_stream_t stream);

/* cpu_nms (:453-481) per image over the first min(count[b], n_cap) rows of dets + b*rows_per_img*6
 * (count on the device: chains after cvl_retina_decode with no host sync): greedy, class-agnostic,
 * highest score first (lowest row among equal scores), survivors kept iff
 * inter / (a_i + a_j - inter + 1e-8) <= iou_thresh in fp32.  keep [B][n_cap] = selected rows in
 * selection order, nkeep [B]. */
size_t cvl_retina_nms_workspace_size(int B, int n_cap);
int cvl_retina_nms(const float* dets, int rows_per_img, const int32_t* count, int B, int n_cap, float iou_thresh,
                   int32_t* keep, int32_t* nkeep, void* workspace, cvl_stream_t stream);

/* FCOS/infer_fcos.py:27-62 image_detections for B images of the FCOS head outputs (reg [B][P][ld_reg]
 * = t, b, l, r, centerness; cls [B][P][ld_cls]; rows level-major, P = sum h*w <= 16384; level_hw
 * [5][2] and strides [5] HOST arrays): boxes = fcos.prediction_to_corners rounded to fp32, scores =
 * sigmoid(cls) (center != 0: sigmoid(centerness) * sigmoid(cls)), then
 * tf.image.combined_non_max_suppression(max_output_size_per_class = max_per_class, max_total_size =
 * max_total, clip_boxes=False): out_boxes [B][max_total][4] (y1, x1, y2, x2), out_scores /
 * out_classes [B][max_total] (zero padded), valid [B].  TF's op is restated (parity unpinned at
 * the reference level; equal-score order: lower box index, then lower class). */
size_t cvl_fcos_detect_workspace_size(int B, int P, int num_classes, int max_per_class);
int cvl_fcos_detect(const float* reg_pred, int ld_reg, const float* cls_pred, int ld_cls, int B,
                    const int32_t* level_hw, const int32_t* strides, int num_classes, int center, float iou_thresh,
                    float score_thresh, int max_per_class, int max_total, float* out_boxes, float* out_scores,
                    float* out_classes, int32_t* valid, void* workspace, size_t workspace_bytes,
                    cvl_stream_t stream);

/* ==========================================================================================
 * Detection evaluation: VOC AP (VOCdevkit VOCevaldet) and COCO-style mAP (pycocotools evaluateImg /
 * accumulate, area range "all").  The reference has no evaluator; the semantics are
 * this project's contract (INTEGRATION.md "Evaluation"; numpy restatement tests/eval_ref.py).
 * Deviations from the two tools: boxes are continuous (no "+1 pixel" of the VOC devkit); recall
 * levels are compared in integers (a point reaches k / n iff n * tp >= k * npos, no float
 * linspace); cvl_eval_match / cvl_eval_ap score COCO's area range "all" at one max_dets, and
 * cvl_eval_match_areas / cvl_eval_ap_views add the small / medium / large ranges and AR@1/10/100
 * (there "all" is unbounded, not [0, 1e10], and areas are box areas unless gt_area is given).
 * Every entry needs no workspace (the per-image state lives in LDS), launches one kernel, is
 * stateless and capturable.
 * ========================================================================================== */
#define CVL_EVAL_MAX_T 1024          /* detection slots per image */
#define CVL_EVAL_MAX_G 1024          /* ground-truth slots per image */
#define CVL_EVAL_MAX_THRESHOLDS 16   /* IoU thresholds K (one bit each in the uint16 bit sets) */
#define CVL_EVAL_MAX_CLASSES 65535
#define CVL_EVAL_MAX_B 65535         /* images per call */
#define CVL_EVAL_AP_CHUNK 1024       /* records per step of cvl_eval_ap's walk over a class segment */
enum { CVL_EVAL_VOC = 0, CVL_EVAL_COCO = 1 };                            /* matching protocol */
enum { CVL_EVAL_AP_VOC07 = 0, CVL_EVAL_AP_VOC12 = 1, CVL_EVAL_AP_COCO = 2 }; /* AP mode */

/* Matches one batch.  boxes [B][T][4] fp32 (y1, x1, y2, x2), scores [B][T], classes [B][T] (fp32
 * class values, as cvl_fcos_detect emits them), valid [B]; gt_boxes [B][G][4], gt_labels [B][G]
 * int32, gt_flags [B][G] bytes (VOC difficult / COCO iscrowd; NULL = none set), gt_count [B] (all
 * three may be NULL when G == 0); image_ids [B] int64 in [0, 2^31); thresholds: HOST double [K].
 * A detection is dropped when its slot >= valid[b], its score is NaN or its class is outside
 * [0, num_classes); with CVL_EVAL_COCO also when max_dets detections of its (image, class) rank
 * before it.  Ground truths with a label outside [0, num_classes) are left out.  IoU in float64:
 * inter / ((ad + ag) - inter), 0 when the denominator <= 0; with CVL_EVAL_COCO against a flagged
 * (crowd) ground truth inter / ad, 0 when ad <= 0.  Per (image, class) the detections are visited
 * by score descending, lower slot first among equal scores, separately for each threshold k:
 *   CVL_EVAL_VOC   jmax = the first ground truth of the class with the strictly largest IoU; IoU >=
 *                  thr: flagged -> ignored, else unused -> TP (marks it used), else FP; IoU < thr: FP;
 *   CVL_EVAL_COCO  ground truths non-crowd first, then crowd, each group in the given order; best =
 *                  min(thr, 1 - 1e-10), m = none; skip a used non-crowd; stop at the crowds when m is
 *                  set; skip when IoU < best; else best = IoU, m = g (later ties win).  m set: marked
 *                  used, ignored when m is a crowd, TP otherwise; m unset: FP.
 * Record i = rec_offset + b * T + t of every slot (the caller provides rec_offset + B * T elements
 * in each array): rec_score (0 when dropped), rec_class (num_classes when dropped), rec_key =
 * image_id << 32 | t, rec_tp / rec_ign: bit k = TP / ignored at threshold k.  npos [num_classes]
 * int32 += the unflagged ground truths per class (integer atomics; the caller zeroes it once).
 * CVL_EINVAL: B, T, G, K, num_classes outside the limits above (T, K, B, num_classes >= 1, G >= 0),
 * an unknown protocol, max_dets < 1, rec_offset < 0, a NULL array. */
int cvl_eval_match(const float* boxes, const float* scores, const float* classes, const int32_t* valid,
                   const float* gt_boxes, const int32_t* gt_labels, const uint8_t* gt_flags,
                   const int32_t* gt_count, const int64_t* image_ids, int B, int T, int G, int num_classes,
                   const double* thresholds /*host[K]*/, int K, int protocol, int max_dets, float* rec_score,
                   int32_t* rec_class, int64_t* rec_key, uint16_t* rec_tp, uint16_t* rec_ign, int64_t rec_offset,
                   int32_t* npos, cvl_stream_t stream);

/* AP of every (class, threshold) over n_records records sorted by (class, score descending, key):
 * rec_tp / rec_ign in that order, seg_offsets [num_classes + 1] int64 (DEVICE) = where each class
 * starts (the dropped records, class num_classes, sort last), npos as accumulated above.  One
 * workgroup per (class, threshold) walks its segment in chunks of CVL_EVAL_AP_CHUNK (a segment may
 * hold many chunks): the TP / FP totals forward, then backward the cumulative counts, precision =
 * tp / (tp + fp) in float64 and its running maximum from the right (the envelope); ignored records
 * are skipped.  mode CVL_EVAL_AP_VOC07: the mean over k = 0..10 of the envelope at the first point
 * with 10 * tp >= k * npos (0 when none); CVL_EVAL_AP_COCO: the same with k = 0..100 and 100;
 * CVL_EVAL_AP_VOC12: (the sum over the points where tp rises of the envelope) / npos.  ap [K][C]
 * float64 (NaN where npos == 0, 0 for a class with ground truth and no detections), tp_total [K][C]
 * int32 = the final TP count.  Deterministic (no floating-point atomics). */
int cvl_eval_ap(const uint16_t* rec_tp, const uint16_t* rec_ign, const int64_t* seg_offsets, const int32_t* npos,
                int64_t n_records, int num_classes, int K, int mode, double* ap, int32_t* tp_total,
                cvl_stream_t stream);

/* ---- COCO area ranges and detection-count views (pycocotools evaluateImg per areaRng, accumulate
 * per maxDets): the twelve-number summary AP, AP50, AP75, APs, APm, APl, AR@1, AR@10, AR@100, ARs,
 * ARm, ARl.  Two entries beside the two above, which are unchanged. ---- */
#define CVL_EVAL_MAX_AREAS 4         /* area ranges A per cvl_eval_match_areas call */
#define CVL_EVAL_MAX_VIEWS 8         /* (area index, max_rank) views R per cvl_eval_ap_views call */

/* cvl_eval_match under CVL_EVAL_COCO (the only protocol; another one is CVL_EINVAL), once per area
 * range a < A (1 <= A <= CVL_EVAL_MAX_AREAS): the inputs, the dropping, the ranking, the max_dets
 * cut per (image, class) -- one cut, the same for every range -- and the IoU arithmetic are
 * cvl_eval_match's.  area_ranges: HOST double [A][2] = (lo, hi); a value v is outside range a iff
 * v < lo || v > hi (both ends inclusive, as pycocotools: an area of exactly 1024 is small and
 * medium; -inf / +inf leave a side open).  Areas in float64: a detection's is (y2 - y1) * (x2 - x1)
 * from its fp32 corners; a ground truth's is the same expression on its box, or (double)
 * gt_area[b][g] when gt_area [B][G] is not NULL (COCO's `area` is the mask area).  area_scale [B]
 * (NULL = none): every box-derived area is multiplied once by (double)area_scale[b] -- original
 * pixels^2 per network pixel^2 when the boxes live on a resized input; a supplied gt_area is used
 * as is.  Per range a and threshold k, with their own used flags:
 *   ign_a[g] = crowd[g] || area_g outside a; the class's ground truths are visited not-ignored
 *   first, then ignored, each group in the given order; npos[a][c] += the ground truths with !ign_a.
 *   Per detection in rank order: best = min(thr, 1 - 1e-10), m = none; per g in that order: skip
 *   when used[g] && !crowd[g]; stop when m is set, !ign_a[m] and ign_a[g]; IoU in the crowd form iff
 *   crowd[g]; skip when IoU < best; else best = IoU, m = g (later ties win).  m set: used[m] = 1,
 *   the detection is ignored iff ign_a[m], else a TP.  m unset: ignored iff the detection's own area
 *   is outside a, else an FP.
 * With A = 1 and the range (-inf, +inf) the records equal cvl_eval_match's bit for bit.
 * Outputs at record i = rec_offset + b * T + t (rec_offset counts records): rec_score / rec_class /
 * rec_key as cvl_eval_match; rec_tp / rec_ign [n][A] uint16, record-major (element i * A + a: bit k
 * = TP / ignored at threshold k in range a); rec_rank [n] uint16 = the detection's rank inside its
 * (image, class), counted before the max_dets cut (0xffff for every dropped slot, those the cut
 * drops included); npos [A][num_classes] int32 += (integer atomics).
 * One workgroup per image, one launch, all state in LDS (63 KiB at T = G = 1024, K = 16, A = 4: one
 * lane per (class present, threshold) walks the ranges serially, the range bits of a ground truth
 * share its used byte), no workspace.  CVL_EINVAL: as cvl_eval_match, and a protocol other than
 * CVL_EVAL_COCO, A outside [1, 4], area_ranges or rec_rank NULL. */
int cvl_eval_match_areas(const float* boxes, const float* scores, const float* classes, const int32_t* valid,
                         const float* gt_boxes, const int32_t* gt_labels, const uint8_t* gt_flags,
                         const int32_t* gt_count, const int64_t* image_ids, int B, int T, int G, int num_classes,
                         const double* thresholds /*host[K]*/, int K, int protocol, int max_dets,
                         const double* area_ranges /*host[A][2]*/, int A, const float* gt_area /*[B][G] or NULL*/,
                         const float* area_scale /*[B] or NULL*/, float* rec_score, int32_t* rec_class,
                         int64_t* rec_key, uint16_t* rec_tp, uint16_t* rec_ign, uint16_t* rec_rank,
                         int64_t rec_offset, int32_t* npos, cvl_stream_t stream);

/* cvl_eval_ap in mode CVL_EVAL_AP_COCO over R views of the same sorted records, one launch with
 * grid (class, threshold, view): views HOST int32 [R][2] = (area index a in [0, A), max_rank >= 1),
 * 1 <= R <= CVL_EVAL_MAX_VIEWS.  View r walks bit k of rec_tp / rec_ign [n][A] at element i * A + a
 * against npos[a][c]; a record is skipped when its ignored bit is set or rec_rank[i] >= max_rank
 * (matching is greedy in rank order, so a rank prefix is pycocotools' maxDets slice).  ap
 * [R][K][C] float64 (NaN where npos[a][c] == 0), tp_total [R][K][C] int32.  Same walk and fixed-
 * order block reductions as cvl_eval_ap.  CVL_EINVAL: the limits of cvl_eval_ap, A outside [1, 4],
 * R outside [1, 8], a view with an area index outside [0, A) or max_rank < 1, a NULL array. */
int cvl_eval_ap_views(const uint16_t* rec_tp, const uint16_t* rec_ign, const uint16_t* rec_rank,
                      const int64_t* seg_offsets, const int32_t* npos, int64_t n_records, int num_classes, int K,
                      int A, const int32_t* views /*host[R][2]*/, int R, double* ap, int32_t* tp_total,
                      cvl_stream_t stream);

/* ==========================================================================================
 * Input pipeline (FCOS/data_preprocess.py:24-133): resize_and_pad_image + random_flip_horizontal.
 * ========================================================================================== */

/* One decoded image src [H][W][C] (uint8 when src_u8, else fp32; C <= 4) -> out [pad_h][pad_w][C]
 * fp32 = (flip == 1 ? flip_left_right(src) : src) resized to out_h x out_w by TF2's bilinear
 * tf.image.resize (half-pixel centres, antialias off; restated), flip == 2: the resized image's
 * left-right flip (preprocess_data pad_flag=False: resize, then flip), then / 127.5 - 1, zero padded
 * bottom/right (tf.image.pad_to_bounding_box).  out may point into a batch slot. */
int cvl_resize_pad_normalize(const void* src, int src_u8, int H, int W, int C, int flip, int out_h, int out_w,
                             int pad_h, int pad_w, float* out, cvl_stream_t stream);

/* CenterNet/train_hourglass_voc.py:24-67 image_augment over a batch, the draws made by the caller
 * (cvlite.train_hourglass_v2.draw_augment): ops[b] / params[b] DEVICE int32 / fp32 per image,
 * 0 none, 1 brightness (x + params[b]), 2 contrast ((x - mean_c) * params[b] + mean_c, mean over
 * the N x N pixels of channel c), 3 flip left-right, 4 transpose (90 degrees), 5 transpose + flip
 * up-down (270 degrees); other codes copy.  img [B][N][N][3] fp32 (square padded images); tgt
 * [B][S][S][4][T] fp32 target maps (T = 5 + C), moved with the image (3: channel 1 := 1 - v;
 * 4 / 5: channels 0 := 1 and 2 := 3 of the transposed cell, the reference's aliased swap; 5: then
 * channel 0 := 1 - v) -- tgt_src = tgt_dst = NULL skips them.  src and dst must not overlap.
 * workspace: cvl_image_augment_workspace_size(B, N) bytes.  Two launches, deterministic. */
size_t cvl_image_augment_workspace_size(int B, int N);
int cvl_image_augment(const float* img_src, float* img_dst, const float* tgt_src, float* tgt_dst,
                      const int32_t* ops, const float* params, int B, int N, int S, int T, void* workspace,
                      size_t workspace_bytes, cvl_stream_t stream);

/* Batched training augmentation (cvlite extension, beyond the reference; cvlite/augment.py): one
 * descriptor per image.  The image's result is defined as this staged fp32 pipeline:
 *   1. zoom-out: src [H][W][3] (uint8 when src_u8, else fp32) at integer offset (oy, ox) on a canvas
 *      ch x cw filled with fill[3] (source units); no zoom-out: ch = H, cw = W, oy = ox = 0;
 *   2. crop: the integer rectangle (y0, x0, hh, ww) of the canvas;
 *   3. flip: the crop mirrored left-right when flip == 1;
 *   4. resize: the bilinear resize of cvl_resize_pad_normalize (the same fp32 arithmetic) of the crop
 *      to oh x ow;
 *   5. colour: v' = M v + t per pixel, m row-major [3][3], row c = ((m[c][0] * r + m[c][1] * g) +
 *      m[c][2] * b) + t[c] in fp32 -- the fill goes through it like any other pixel, nothing is clipped;
 *   6. / 127.5 - 1, zero padded bottom / right to ph x pw, written to dst [ph][pw][3] fp32 (dst may
 *      point into a batch slot; 16-byte aligned with pw % 4 == 0 takes the 16-byte store path). */
typedef struct cvl_augment_desc {
  const void* src;               /* DEVICE [H][W][3] */
  float* dst;                    /* DEVICE [ph][pw][3] */
  int32_t src_u8, H, W;
  int32_t ch, cw, oy, ox;        /* canvas size, source offset on it */
  int32_t y0, x0, hh, ww;        /* crop rectangle on the canvas */
  int32_t flip;
  int32_t oh, ow, ph, pw;        /* resized size, padded size */
  float m[9], t[3], fill[3];
  int32_t reserved;              /* 0 (keeps the size a multiple of 8: 144 bytes) */
} cvl_augment_desc;
#define CVL_AUGMENT_MAX_BATCH 4096
#define CVL_AUGMENT_MAX_SIDE 32768

/* Augments B images in ONE launch.  table: HOST array of B descriptors (read here, for the checks and
 * the grid); table_dev: the same B descriptors in DEVICE memory, copied there by the caller on `stream`
 * ahead of this call (a pinned host table and one asynchronous copy).  Images of different source, crop
 * and padded sizes mix; destinations must not overlap each other or a source.  No atomics: deterministic.
 * Kernel only, no allocation or synchronisation inside.  CVL_EINVAL: B outside [1,
 * CVL_AUGMENT_MAX_BATCH], a NULL pointer, src_u8 or flip not 0 / 1, a source or a crop that does not
 * lie inside its canvas, an empty crop, oh > ph or ow > pw, a canvas or padded side above
 * CVL_AUGMENT_MAX_SIDE, ph * pw >= 2^31. */
int cvl_augment_batch(const cvl_augment_desc* table /*host[B]*/, const cvl_augment_desc* table_dev, int B,
                      cvl_stream_t stream);

/* ==========================================================================================
 * JPEG decode (FCOS/data_preprocess.py:5-9 `_parse_image`, tf.image.decode_jpeg): the file bytes
 * -> [H][W][3] uint8 RGB, bit-identical to libjpeg's default decode (islow IDCT, fancy upsampling),
 * i.e. to PIL's Image.open(...).convert("RGB").  Hybrid: the Huffman bit stream is decoded on the
 * host (std::threads, several images at once), dequantise + inverse DCT + chroma upsampling +
 * YCbCr->RGB + crop run on the GPU, two launches per batch.
 *
 * Supported files: baseline (SOF0) 8-bit, one interleaved scan of all components, greyscale or
 * YCbCr with luma sampling 1x1 (4:4:4), 2x1 (4:2:2) or 2x2 (4:2:0) and 1x1 chroma, 8-bit
 * quantisation tables, 1 <= width, height <= 8192, restart intervals allowed.  Everything else
 * (progressive, arithmetic, 12-bit, CMYK / YCCK, RGB-coded, other samplings, several scans, not a
 * JPEG) is CVL_JPEG_UNSUPPORTED; a truncated or inconsistent stream, or one libjpeg would only
 * decode with warnings, is CVL_JPEG_CORRUPT.  Neither reads or writes out of range.
 * ========================================================================================== */
enum { CVL_JPEG_UNSUPPORTED = 2, CVL_JPEG_CORRUPT = 3 };
#define CVL_JPEG_MAX_BATCH 4096

/* Host only: parses the segments up to the scan.  data: HOST bytes of the file.  info: HOST int32
 * [8] = {status, width, height, components (1 or 3), hmax, vmax (luma sampling), restart interval
 * in MCUs (0 = none), coefficient count (int16 elements, blocks padded to whole MCUs)}; all but
 * the status are 0 when the status (also the return value) is not CVL_OK. */
int cvl_jpeg_info(const uint8_t* data, size_t nbytes, int32_t* info /*host[8]*/);

/* Host only, no GPU call: the entropy decode of one file.  coef: HOST int16, the quantised (not
 * dequantised) coefficients in natural (de-zigzagged) order, component-planar
 * [comp][block_row][block_col][64]; coef_cap = its capacity in elements (CVL_EINVAL when below the
 * coefficient count of cvl_jpeg_info).  qt: HOST uint16 [3][64], the quantisation table of each
 * component in natural order (rows of absent components zero).  Returns CVL_OK or the file's
 * status; coef / qt hold partial data after CVL_JPEG_CORRUPT. */
int cvl_jpeg_entropy_decode(const uint8_t* data, size_t nbytes, int16_t* coef, size_t coef_cap,
                            uint16_t* qt /*host[3][64]*/);

/* Host only: the buffer sizes of cvl_jpeg_decode_batch for n images whose coefficient counts
 * (cvl_jpeg_info; 0 for an image that is not CVL_OK) are coef_counts (HOST). */
int cvl_jpeg_batch_sizes(const int32_t* coef_counts, int n, size_t* staging_bytes, size_t* workspace_bytes);

/* Decodes n files in one call.  data / nbytes: HOST arrays of n HOST byte pointers and lengths;
 * out: HOST array of n DEVICE pointers, image i written as [H_i][W_i][3] uint8 (sizes from
 * cvl_jpeg_info); staging: a PINNED HOST buffer and workspace a DEVICE buffer of at least the
 * cvl_jpeg_batch_sizes bytes, both 16-byte aligned; status: HOST int32 [n], the status of each
 * image.  The call entropy-decodes on min(n, CVL_JPEG_THREADS) threads (environment, default 8,
 * clamped to 1..16) into staging, then enqueues on `stream` one copy of the used staging bytes into
 * workspace and the two kernels over the whole batch (images of different sizes and samplings mix).
 * An image whose status is not CVL_OK is skipped -- its output is untouched -- and the call still
 * returns CVL_OK.  No allocation of device or pinned memory and no device synchronisation inside:
 * staging and workspace are in use until the enqueued work has run, so the caller must not reuse
 * them (another batch included) before that (record an event on `stream`, wait for it).  Unlike the
 * kernels-only entries this one runs host work and a copy; it is not for capture into a hipGraph. */
int cvl_jpeg_decode_batch(const uint8_t* const* data, const size_t* nbytes, int n, uint8_t* const* out,
                          void* staging, size_t staging_bytes, void* workspace, size_t workspace_bytes,
                          int32_t* status, cvl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CVLITE_H_ */
