/*
 * brcnn_hip.h -- C ABI of libbrcnn_hip.so: the MI355X (gfx950) kernels of the
 * Boosting R-CNN hot path.
 *
 * Conventions (the same the reference's operator seam uses):
 *   - every pointer is a DEVICE pointer unless the name ends in `_host`;
 *   - the caller owns and pre-allocates every buffer (mmcv does
 *     `output = input.new_zeros(...)` before calling its native op);
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); all
 *     work is enqueued on it, nothing synchronises unless stated;
 *   - return value: 0 on success, -22 (EINVAL) for a rejected argument,
 *     -(1000 + hipError_t) when a HIP call failed, -62 (BRCNN_EHANDOVER) when an
 *     EARLIER conv launch reported a lost stream-K hand-over (its results are
 *     invalid; see brcnn_conv_handover_status).  No exceptions cross the ABI;
 *   - thread-safe for calls on distinct streams with distinct workspaces
 *     (brcnn_conv_set_workspace); the `brcnn_*_set_*` tuning hooks are
 *     process-wide test / benchmarking switches: set them from one thread while
 *     no other thread is inside the library.
 *
 * Each entry cites the reference interface it replaces.  The reference tree has
 * no native code: those interfaces are the `mmcv.ops` Python functions
 * (mmcv-full 1.4.0, un-vendored) whose call sites are given as
 * /root/reference file:line.
 */
#ifndef BRCNN_HIP_H
#define BRCNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BRCNN_LAYOUT_NCHW 0 /* (N,C,H,W) contiguous, the reference's layout      */
#define BRCNN_LAYOUT_NHWC 1 /* (N,H,W,C) contiguous == torch.channels_last       */

#define BRCNN_DT_F32 0
#define BRCNN_DT_BF16 1          /* bf16 operands, fp32 accumulate, bf16 result */
#define BRCNN_DT_BF16_OUT_F32 2  /* bf16 operands, fp32 accumulate, fp32 result  */
#define BRCNN_DT_F16 3           /* IEEE fp16 operands, fp32 accumulate, fp16 result (the recipes' `fp16 =
                                    dict(loss_scale=512.)`, mmdet/apis/train.py:115-119) */
#define BRCNN_DT_F16_OUT_F32 4   /* fp16 operands, fp32 accumulate, fp32 result  */

#define BRCNN_MAX_LEVELS 8
#define BRCNN_MAX_IMAGES 64      /* images per call of the whole-batch train-step entries */

/* library / device info -------------------------------------------------------- */
int brcnn_version(void);

/* Measurement aid: a one-lane kernel that spins for `wall_ticks_100mhz` ticks of the constant
 * 100 MHz counter and writes {elapsed wall ticks, elapsed shader cycles} to out2 (device, 2 x
 * int64).  Launched on a second stream beside a workload it gives the effective shader clock
 * under that load (cycles / ticks * 0.1 GHz) without a profiler attached (tools/clock_under_load.py). */
int brcnn_clock_probe(int64_t *out2, int64_t wall_ticks_100mhz, void *stream);

/* number of HIP devices visible, or a negative status */
int brcnn_device_count(void);

/* ------------------------------------------------------------------------------
 * RoIAlign.  Replaces mmcv.ops.roi_align_forward / roi_align_backward, reached at
 * mmdet/models/roi_heads/roi_extractors/base_roi_extractor.py:54-60 (construction,
 * `getattr(ops, 'RoIAlign')`) and single_level_roi_extractor.py:103 (call).
 *   input  (N,C,H,W) logical shape, memory per `layout`
 *   rois   (K,5) fp32 [batch_index, x1, y1, x2, y2]
 *   output (K,C,ph,pw) logical shape, memory per `layout` ((K,ph,pw,C) for NHWC)
 *   pool_mode 0 = max (argmax_y/argmax_x (K,C,ph,pw) required), 1 = avg
 *   sampling_ratio 0 = adaptive grid ceil(roi_size / pooled_size)
 * -------------------------------------------------------------------------- */
int brcnn_roi_align_forward(const float *input, const float *rois, float *output,
                            float *argmax_y, float *argmax_x, int batch, int channels,
                            int height, int width, int n_rois, int pooled_h, int pooled_w,
                            float spatial_scale, int sampling_ratio, int pool_mode, int aligned,
                            int layout, void *stream);

/* avg-mode backward; grad_input must be zero-filled by the caller. */
int brcnn_roi_align_backward(const float *grad_output, const float *rois, float *grad_input,
                             int batch, int channels, int height, int width, int n_rois,
                             int pooled_h, int pooled_w, float spatial_scale, int sampling_ratio,
                             int aligned, int layout, void *stream);

/* Fused SingleRoIExtractor.forward (single_level_roi_extractor.py:57-115 with
 * map_roi_levels :36-55): every RoI picks its pyramid level
 * clamp(floor(log2(sqrt(w*h)/finest_scale + 1e-6)), 0, L-1) in-kernel and is
 * pooled from that level's map; NHWC only, avg, aligned.
 *   feats[l]  (N,H_l,W_l,C) device pointers (host array of L pointers)
 *   output    (K,ph,pw,C)
 *   levels_out optional (K) int32: the level each RoI was mapped to */
int brcnn_roi_extract_forward(const void *const *feats_host, const int *heights_host,
                              const int *widths_host, const float *scales_host, int num_levels,
                              const float *rois, void *output, int32_t *levels_out, int batch,
                              int channels, int n_rois, int pooled_h, int pooled_w,
                              int sampling_ratio, float finest_scale,
                              int dtype /* of feats and output: BRCNN_DT_F32 | BRCNN_DT_BF16 */,
                              void *stream);
/* The same with `order_ws` (n_rois int32, caller-owned; NULL = visit the RoIs as given): from ~12000 RoIs on the
 * kernel visits them sorted by (image, level, 12-row band of the RoI's centre) -- one small counting-sort launch --
 * so that the bin rows an XCD has in flight stay inside what its L2 holds.  Results are those of
 * brcnn_roi_extract_forward bit for bit. */
int brcnn_roi_extract_forward_ordered(const void *const *feats_host, const int *heights_host,
                              const int *widths_host, const float *scales_host, int num_levels,
                              const float *rois, void *output, int32_t *levels_out, int batch,
                              int channels, int n_rois, int pooled_h, int pooled_w,
                              int sampling_ratio, float finest_scale,
                              int dtype /* of feats and output */, int32_t *order_ws, void *stream);

/* Round 5: the same with `prep_ws` -- brcnn_roi_extract_prep_workspace_bytes(n_rois) bytes of caller-owned scratch,
 * 256-byte aligned, or NULL.  With it the level mapping (single_level_roi_extractor.py:36-55), the RoI geometry and the
 * per-axis bilinear weights are computed once per RoI by a small first launch and handed to the gather through a
 * 576-byte record per RoI, instead of once per bin row inside the gather.  Results: those of the footprint form (bit
 * for bit on the bin rows that take its streaming path; the others run the reference's sample loop).  Measured
 * (profiles/r05_notes.md) faster only from ~1000 RoIs per image on, so the form is OFF by default
 * (brcnn_roi_align_set_exact(31) switches it on): brcnn_roi_extract_prep_workspace_bytes returns 0 while it is off. */
size_t brcnn_roi_extract_prep_workspace_bytes(int n_rois);
int brcnn_roi_extract_forward_prepared(const void *const *feats_host, const int *heights_host,
                              const int *widths_host, const float *scales_host, int num_levels,
                              const float *rois, void *output, int32_t *levels_out, int batch,
                              int channels, int n_rois, int pooled_h, int pooled_w,
                              int sampling_ratio, float finest_scale,
                              int dtype /* of feats and output */, int32_t *order_ws, void *prep_ws,
                              size_t prep_bytes, void *stream);
/* the RoI count from which a non-NULL `order_ws` is used (below it the RoIs are visited as given) */
int brcnn_roi_extract_order_min_rois(void);

int brcnn_roi_extract_backward(float *const *grad_feats_host, const int *heights_host,
                               const int *widths_host, const float *scales_host, int num_levels,
                               const float *rois, const float *grad_output, int batch,
                               int channels, int n_rois, int pooled_h, int pooled_w,
                               int sampling_ratio, float finest_scale, void *stream);

/* The same gradient as a GATHER: every pixel of every grad_feats level is written exactly once (no
 * pre-zeroing, no atomics, a fixed summation order: deterministic).  One workgroup per 8x8 tile of a
 * (level, image) map collects the RoIs whose footprint touches the tile and accumulates
 * dX[h,w] += sum_bins Wy[ph][h] * Wx[pw][w] * dY[roi,ph,pw] / count with the separable bilinear footprint
 * weights.  workspace: brcnn_roi_extract_backward_workspace_bytes(n_rois).  pooled_h, pooled_w <= 7.
 * dtype: element type of grad_output AND of the grad_feats maps (BRCNN_DT_F32, or the 16-bit compute dtype of
 * the pyramid in training: fp32 accumulation, one rounding at the store). */
size_t brcnn_roi_extract_backward_workspace_bytes(int n_rois);
/* ... plus room for the fp32 partials of the hit-chunked form: a map with at most 32 tiles of 8 x 8 pixels per image (the
 * coarse pyramid levels) is touched by most of its level's RoIs in every tile, and one workgroup per tile walks those hits
 * one after the other -- that chain, not the bytes, is the launch (512 RoIs / image of 450-800 px: 2.0 ms, of 16-110 px:
 * 0.22 ms).  With a workspace of this size the gather entries give such tiles n_rois / batch / 48 (<= 16) workgroups, each
 * taking every n-th hit in RoI order, and add their partials in a fixed order in a second launch (reproducible; not the
 * one-workgroup chain's association).  With the smaller workspace above they run the one-workgroup form. */
size_t brcnn_roi_extract_backward_workspace_bytes_ex(int n_rois, int batch, int channels, int num_levels,
                                                     const int *heights_host, const int *widths_host);
int brcnn_roi_extract_backward_gather(void *const *grad_feats_host, const int *heights_host,
                                      const int *widths_host, const float *scales_host, int num_levels,
                                      const float *rois, const void *grad_output, int batch, int channels,
                                      int n_rois, int pooled_h, int pooled_w, int sampling_ratio,
                                      float finest_scale, void *workspace, size_t workspace_bytes,
                                      int dtype, void *stream);
/* ... with one more operand per level: grad_feats[l] = gather + addends[l] (NULL array or NULL entries: none), the
 * addend in the maps' dtype, added in fp32 before the store's one rounding.  What autograd does with a separate add
 * over the whole map when a pyramid level has a second consumer besides the RoI extractor (here: the RPN branch's
 * gradient, kept from its own earlier backward pass -- detectors.py, early_rpn_backward). */
int brcnn_roi_extract_backward_gather_add(void *const *grad_feats_host, const void *const *addends_host,
                                          const int *heights_host, const int *widths_host,
                                          const float *scales_host, int num_levels, const float *rois,
                                          const void *grad_output, int batch, int channels, int n_rois,
                                          int pooled_h, int pooled_w, int sampling_ratio, float finest_scale,
                                          void *workspace, size_t workspace_bytes, int dtype, void *stream);
/* NHWC RoIAlign forward variants: 0 (default) = footprint form, column streaming (one wavefront per row of bins
 * reads every pixel of the ROW's footprint once, rows reduced first, then spread over the bins with their x weights;
 * bin rows dealt to the XCDs in contiguous eighths; equal to the reference to fp32 round-off), 1 = the reference's
 * sample-order accumulation (bit-identical to mmcv's CPU kernel; ~1.5x the L2 reads), 2 = the footprint form of
 * rounds 1-2 (per-bin loop, round-robin rows), 3 = column streaming with round-robin rows (tuning / A-B hooks).
 * 60 .. 63 (tests) RETURN a host-side count and clear it: forward launches that visited the RoIs in band order (60) /
 * took the prepared-record form (61), gradient gathers that ran chunked (62), the chunks per coarse tile of the last
 * of them (63). */
int brcnn_roi_align_set_exact(int exact);

/* The policy switches of the library as ONE documented struct (round 5; VERDICT r04: the integer hooks had become what
 * product defaults depend on).  Process-wide, unsynchronised: read / written from one thread while no other thread is
 * inside the library.  Every choice yields the same results bit for bit EXCEPT conv_split_k (the association of the K
 * sum changes: results then depend on the tile count, i.e. on the batch size), roi_exact_order (the footprint form
 * equals the exact form to fp32 round-off) and wgrad_slab_reduction = 0 (fp32 atomics: order-dependent sums).
 * `size` must be sizeof(brcnn_tuning) (a caller built against another layout gets BRCNN_EINVAL).
 * The integer hooks (brcnn_conv_set_tile*, brcnn_roi_align_set_exact) stay as the fine-grained test / tuning interface;
 * both interfaces write one table (csrc/policy.h), which lists every switch and its default. */
typedef struct brcnn_tuning {
    int size;
    int conv_stream_k;                /* chained stream-K schedule of the conv kernels: 0 off, 1 by the heuristic (default), 2 wherever the tile count allows */
    int conv_split_k;                 /* split-K of launches with fewer tiles than CUs: 0 off (default), 1 heuristic, 2 forced */
    int conv_eight_phase_16bit;       /* eight-phase 256x256 kernel for bf16 / fp16: 0 never, 1 heuristic (default) */
    int conv_persistent_1x1;          /* persistent LDS-resident-weights kernel for the short-K 1x1 layers: 0 never, 1 heuristic (default), 2 forced */
    int conv_eight_phase_f32;         /* fp32 eight-phase kernel: 0 never, 1 heuristic (default), 2 forced, 128 / 256 forced with that tile height */
    int wgrad_slab_reduction;         /* weight gradient over the M slices: 0 fp32 atomics, 1 slabs + fixed-order second stage (default: deterministic) */
    int wgrad_eight_phase;            /* eight-phase weight-gradient kernel: 0 never, 1 heuristic (default), 2 wherever the shape allows */
    int wgrad_reduce_in_launch;       /* its slab reduction: 0 separate launches (default), 1 inside the producing launch (measured slower) */
    int wgrad_generation_percent;     /* two-buffer weight-gradient launches: percent of one generation of resident workgroups (default 75: they share the device with the main stream) */
    int wgrad_eight_phase_cu_percent; /* eight-phase weight-gradient launches: percent of the CUs (default 75) */
    int roi_exact_order;              /* RoIAlign forward: 0 footprint form (default), 1 the reference's sample order bit for bit */
    int roi_rows_per_wave;            /* bin rows per wavefront: 0 heuristic (default), 1, 7 */
    int roi_visit_order;              /* band-ordered visit of the RoIs: 0 off, 1 from brcnn_roi_extract_order_min_rois() RoIs on (default), 2 always */
    int roi_prepared_records;         /* per-RoI records written by a first launch: 0 off (default), 1 on where the caller gives the scratch */
} brcnn_tuning;
int brcnn_get_tuning(brcnn_tuning *t);          /* t->size set by the caller */
int brcnn_set_tuning(const brcnn_tuning *t);

/* Whole-batch candidate preparation / collection around brcnn_nms for fixed per-image slots of
 * `slot` candidates (the device-resident form of mmcv.ops.batched_nms below split_thr, called per
 * image by atss_rpn_head.py:756 and bbox_nms.py:86): brcnn_nms_prepare compacts the valid rows of
 * every slot in order (zeros behind them), writes `nms_boxes = box + float(id) * (max + 1)` with
 * max = the slot's largest surviving coordinate (mmcv's class / level separation, same fp32
 * operations) and the slot's [begin, end) range; brcnn_nms_collect gathers the first
 * min(num[b], max_keep) survivors of each slot into dets (batch, max_keep, 5) / ids_kept (zeros / -1
 * behind them).  ids int64, valid one byte per row. */
int brcnn_nms_prepare(const float *boxes, const float *scores, const int64_t *ids, const uint8_t *valid,
                      float *c_boxes, float *c_scores, int64_t *c_ids, float *nms_boxes, int32_t *ranges,
                      int batch, int slot, void *stream);
int brcnn_nms_collect(const int64_t *keep, const int32_t *num, const float *c_boxes, const float *c_scores,
                      const int64_t *c_ids, float *dets, int64_t *ids_kept, int batch, int slot,
                      int max_keep, void *stream);

/* The same for mmcv batched_nms at or above split_thr (its per-id branch, mmcv/ops/nms.py; the training
 * proposal stage has 15 150 candidates per image, atss_rpn_head.py:756, and the 80-class second stage
 * 256 x 80): candidate columns [sum level_sizes[:l], +level_sizes[l]) of a slot carry id l, so after
 * the order-preserving compaction every (image, id) is one segment -- ranges is (batch*num_levels, 2).
 * brcnn_nms_collect_sorted then re-sorts an image's survivors of all ids by score (descending, ties by
 * ascending candidate position) and keeps the first max_keep: dets (batch, max_keep, 5) zero padded,
 * ids_kept (batch, max_keep) (-1 padded) or NULL, n_kept (batch).  new_scores5: rows of 5 floats aligned
 * with `keep` whose column 4 replaces the score (soft-NMS picks), or NULL.  slot <= 16384. */
int brcnn_nms_prepare_levels(const float *boxes, const float *scores, const int64_t *ids, const uint8_t *valid,
                             float *c_boxes, float *c_scores, int64_t *c_ids, float *nms_boxes,
                             int32_t *ranges, int batch, int slot, int num_levels,
                             const int *level_sizes_host, void *stream);
int brcnn_nms_collect_sorted(const int64_t *keep, const int32_t *num, const int32_t *ranges,
                             const float *c_boxes, const float *c_scores, const int64_t *c_ids,
                             const float *new_scores5, float *dets, int64_t *ids_kept, int32_t *n_kept,
                             int batch, int slot, int num_levels, int max_keep, void *stream);

/* ------------------------------------------------------------------------------
 * NMS.  Replaces mmcv.ops.nms (ext `nms(boxes, scores, iou_threshold, offset)`),
 * reached through mmcv batched_nms at atss_rpn_head.py:756, rpn_head.py:245 and
 * core/post_processing/bbox_nms.py:86.
 * Segmented form: `num_segments` independent problems (images, or levels of the
 * split_thr path) in one launch; segment s owns boxes [seg_begin[s], seg_end[s])
 * (for back-to-back segments pass offsets and offsets+1; gaps are allowed).  Semantics per segment = mmcv nms_cpu: order by score
 * descending (ties: ascending index), greedy suppress when
 * inter/(area_i+area_j-inter) > iou_threshold.
 *   boxes (n,4) fp32, scores (n) fp32, seg_begin/seg_end (S) int32 on device
 *   keep  (n) int64: for segment s the kept ORIGINAL global indices in score
 *         order are written at keep[seg_begin[s] ...]; num_keep (S) int32
 *   max_keep > 0 stops each segment after that many survivors (mmcv `max_num`)
 *   max_segment_len: an upper bound on the longest segment (sizes the bit mask:
 *         n * ceil(max_segment_len/64) * 8 bytes)
 *   workspace: brcnn_nms_workspace_bytes(n, S, max_segment_len) bytes of scratch
 * -------------------------------------------------------------------------- */
size_t brcnn_nms_workspace_bytes(int64_t n, int num_segments, int64_t max_segment_len);
int brcnn_nms(const float *boxes, const float *scores, const int32_t *seg_begin,
              const int32_t *seg_end, int num_segments, int64_t n, int64_t max_segment_len, float iou_threshold,
              int offset, int max_keep, int64_t *keep, int32_t *num_keep, void *workspace,
              size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------
 * Soft-NMS.  Replaces mmcv.ops.soft_nms (ext `softnms`, CPU-only in mmcv),
 * selected by `nms=dict(type='soft_nms', ...)`
 * (configs/boosting_rcnn/boosting_rcnn_r2_101_dcn_pafpn_mstrain_3x_coco.py:27)
 * through bbox_nms.py:86.  Sequential pick-max / decay / discard semantics of
 * softnms_cpu reproduced exactly, one workgroup per segment.
 *   dets (n,5) out [x1,y1,x2,y2,decayed score] in pick order per segment
 *   inds (n) int64 out: original global indices in pick order
 *   method 0 naive, 1 linear, 2 gaussian
 * -------------------------------------------------------------------------- */
size_t brcnn_softnms_workspace_bytes(int64_t n, int num_segments);
int brcnn_softnms(const float *boxes, const float *scores, const int32_t *seg_begin,
                  const int32_t *seg_end, int num_segments, int64_t n, float iou_threshold, float sigma, float min_score,
                  int method, int offset, float *dets, int64_t *inds, int32_t *num_keep,
                  void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------
 * Sigmoid focal loss, element-wise (reduction 'none').  Replaces
 * mmcv.ops.sigmoid_focal_loss_forward/_backward reached at
 * mmdet/models/losses/focal_loss.py:86.  input (n,c) fp32, target (n) int64 in
 * [0,c] (c = background), weight (c) or NULL.
 * -------------------------------------------------------------------------- */
int brcnn_sigmoid_focal_loss_forward(const float *input, const int64_t *target,
                                     const float *weight, float *output, int64_t n, int64_t c,
                                     float gamma, float alpha, void *stream);
int brcnn_sigmoid_focal_loss_backward(const float *input, const int64_t *target,
                                      const float *weight, float *grad_input, int64_t n,
                                      int64_t c, float gamma, float alpha, void *stream);

/* ------------------------------------------------------------------------------
 * Convolution / linear stack (no mmcv counterpart: torch.nn.Conv2d/Linear +
 * BatchNorm(eval)/ReLU/residual in mmdet/models/backbones/resnet.py:263-302,
 * necks/pafpn.py:100-158, dense_heads/atss_rpn_head.py:207-215,
 * roi_heads/bbox_heads/convfc_bbox_head.py:154-192).
 * Implicit-GEMM on MFMA, NHWC activations:
 *   x  (N,H,W,Cin)   w (Cout,KH,KW,Cin)   y (N,Ho,Wo,Cout)
 *   y = act( conv(x,w) * scale[c] + shift[c] + residual ),  act = relu if `relu`
 *   scale/shift/residual may be NULL (scale -> 1, shift -> 0).
 *   dtype BRCNN_DT_F32: fp32 operands on v_mfma_f32_32x32x2_f32 (exact fp32 FMA
 *   chain); BRCNN_DT_BF16: bf16 operands, fp32 accumulate, bf16 output.
 * A linear layer is the 1x1 case with H=W=1.
 * -------------------------------------------------------------------------- */
int brcnn_conv2d_nhwc(const void *x, const void *w, const float *scale, const float *shift,
                      const void *residual, void *y, int batch, int height, int width, int cin,
                      int cout, int kh, int kw, int stride, int pad, int relu, int dtype,
                      void *stream);

/* Stride-1 convolution whose output is scattered with stride 2: output pixel (a, b) of the
 * (height + 2 pad - kh + 1) x (width + 2 pad - kw + 1) result goes to pixel
 * (2 (a - origin) + ph, 2 (b - origin) + pw) of y (batch, out_height, out_width, cout); pixels that
 * fall outside y are dropped, pixels of y of other parities are not touched.  It is one parity
 * class of the data gradient of a stride-2 convolution (x = dy, w = the class's taps as
 * (Cin_of_the_layer, KH', KW', Cout_of_the_layer)): the four classes of a 3x3 / pad 1 layer have
 * 1 + 2 + 2 + 4 = 9 taps, against 36 for the full kernel over the zero-stuffed dy that
 * brcnn_conv2d_dgrad_nhwc_multi runs (the reference gets the same effect from cuDNN's strided
 * dgrad).  cin % 32 == 0 (fp32) / % 64 (bf16). */
int brcnn_conv2d_nhwc_scatter2(const void *x, const void *w, void *y, int batch, int height, int width,
                               int cin, int cout, int kh, int kw, int pad, int out_height,
                               int out_width, int ph, int pw, int origin, int dtype, void *stream);

/* Scratch of the convolution launches of ONE stream -- the stream-K hand-over slots (fp32 accumulators of the tiles
 * cut between two workgroups), their flags, and the slabs of the sliced 16-bit weight gradient -- is CALLER-OWNED like
 * every other buffer: allocate brcnn_conv_workspace_bytes() bytes (256-byte aligned), register them for the stream
 * once, keep them alive until brcnn_conv_set_workspace(stream, NULL, 0).  The registration enqueues a memset of the
 * flag area on `stream`.  A stream that never registered gets a library-side hipMalloc on its first convolution
 * (fallback for plain C callers; released by the NULL call, which synchronises that stream). */
size_t brcnn_conv_workspace_bytes(void);
int brcnn_conv_set_workspace(void *stream, void *workspace, size_t bytes);

/* 0, or BRCNN_EHANDOVER (-62) if a K tail of a stream-K launch gave up waiting for its head since the last call
 * (reported once, then cleared).  Every conv launch checks the same word first, so the error also surfaces as the
 * status of the NEXT convolution; call this after a synchronisation to vet the launches already finished. */
#define BRCNN_EHANDOVER (-62)
int brcnn_conv_handover_status(void);

/* Tuning hook: force the workgroup tile (wm: 2 -> 128 rows, 4 -> 256 rows; nt: 1 -> 64
 * columns, 2 -> 128 columns; 0 -> built-in heuristic).  Process-wide; used by the
 * benchmarking scripts (tools/conv_bench.py).  (-1, 0/1/2): register-staged / heuristic / LDS-DMA
 * staging.  (-2, 0 / 1 / 2 / 128 / 256): the eight-phase fp32 kernel (csrc/conv_pp_f32.hip: 256- or
 * 128-row x 256-column tiles, two wave groups alternating MFMA and load blocks, chained stream-K) never /
 * by the heuristic / forced, forced with 128- / 256-row tiles.  (-3, 0 / 1 / 2): its 256 x 128 form for layers with 128
 * output channels never / by the heuristic / forced.  (-4, 0 / 1): test hook -- 1 = every conv launch (all dtypes) takes the
 * general set-up and read-out instead of the straight-line forms of full tiles and plain 1x1 layers.  (-5, 0 / 1 / 2): the
 * persistent launch of the fp32 64 x 64 kernel (exactly the resident workgroups, one contiguous range of tile x K-tile
 * iterations each, chained hand-over of the tiles a range boundary cuts) never / by the heuristic / wherever the schedule
 * allows (not under stream capture, with fewer than two tiles per CU, on one-K-tile, grouped, scattering or zero-stuffed
 * launches; a launch with fewer tiles than resident workgroups runs tiles / CUs workgroups per CU).  (-6, 0) returns the
 * number of persistent launches so far (>= 0), (-6, 1) the workgroups of the last one.  (-7, n): at most n workgroups per
 * CU in the persistent launch, 0 = as many as are resident (tools/f32_tile_persistent_bench.py).
 * Every choice gives the same bits.
 * (-9, n), tests: which route the conv launches took -- returns host-side counter n and clears it, (-9, -1) clears all:
 * n = 0 fp32 eight-phase launches, 1 / 2 tile rows / columns of the last one; 3 / 4 / 5 launches of the 256 x 256
 * eight-phase, 256 x 128 two-group and persistent 1x1 16-bit kernels; 6 / 7 launches planned as chained stream-K /
 * split-K, 8 the workgroups of the last of them; 9 launches of the two-buffer / ring 16-bit tile kernel, 10 .. 13 the
 * last one's tile rows, tile columns, waves per workgroup, ring stages; 14 launches of the 16-bit weight gradient's tile
 * kernel (csrc/conv_wgrad_bf16.hip), 15 the tile code (1, 2, 4) of the last one (csrc/policy.h: Counters).
 * (-11, 0 / 1): Winograd F(2x2,3x3) for the fp32 3x3 layers whose caller prepared the transformed filter never / yes;
 * (-11, 2) RETURNS the setting (the caller reads it: the Winograd entry point never falls back by itself); (-11, 11 .. 18):
 * 1 .. 8 transform + GEMM launch pairs per call.  (-12, 0) returns and clears the number of Winograd calls that launched,
 * (-12, 1) the 2x2 tiles of the last one; (-9, -1) clears both as well.
 * (-13, 0 / 1 / 2): route of the 16-bit deformable convs (brcnn_deform_conv_route) im2col + GEMM always / the measured
 * rule / fused wherever accepted; (-13, 3) RETURNS the setting; (-13, 10) / (-13, 11) return and clear the launches of the
 * fused deformable kernel / of the deformable im2col kernels ((-9, -1) clears them too).
 * (-14, 0 / 1 / 2): Winograd single-layer route of the frozen fp32 3x3 layers (brcnn_winograd_layer_route) never / the
 * measured rule / wherever the entry accepts the shape; (-14, 3) RETURNS the setting; (-14, 10) / (-14, 11) return and clear
 * the launches of brcnn_conv3x3_winograd_f32_layer / the GEMM tile of the last one (1 = 64 x 128, 2 = 32 x 128,
 * 3 = 64 x 64; (-9, -1) clears them too); (-14, 20 + v): that entry's GEMM tile by the measured rule (v = 0) or forced
 * (v = 1 .. 3), (-14, 24) RETURNS it.  (-11, 0) switches this route off as well.  Every tile gives the same bits.
 * (-16, 0 / 1 / 2): persistent, balanced launch of the Winograd GEMM (both Winograd entries) never / by the measured rule
 * (brcnn_winograd_persistent_rule) / wherever the schedule allows; (-16, 3) RETURNS the setting; (-16, 10) / (-16, 11) /
 * (-16, 12) / (-16, 13) return and clear the persistent launches / the workgroups of the last one / the GEMM tile of the
 * last tower call / the LDS ring stages of the last GEMM launch ((-9, -1) clears them too); (-16, 40 / 42 / 43): LDS ring
 * stages of the GEMM's K loop by the measured rule / 2 / 3, (-16, 49) RETURNS it; (-16, 20 + v): the tower entry's GEMM tile by the measured rule (v = 0) or forced (1 = 64 x 128,
 * 3 = 64 x 64), (-16, 24) RETURNS it; (-16, 30 + n), n = 0 .. 8: at most n workgroups per CU in a persistent launch (0: the
 * occupancy query's), (-16, 39) RETURNS it; (-16, 1000 + n), n = 0 .. 2048: at most n workgroups in all (a test hook: small
 * maps then straddle tiles; 0: no cap), (-16, 999) RETURNS it.  Both launch forms give the same bits. */
int brcnn_conv_set_tile(int wm, int nt);

/* Tuning hook of the bf16 kernel: 0 heuristic; 11 / 21 / 22 = 64x64 / 128x64 / 128x128 tile on
 * 4 waves; 81 / 82 / 164 / 42 = 128x64 / 128x128 (8 waves) / 128x128 (16 waves) / 256x128 (8
 * waves); 381 / 382 / 3164 / 322 / 342 = the same tiles on a 3-deep LDS ring with counted
 * vmcnt waits, 482 = 4-deep (measured slower than two double-buffered workgroups per CU:
 * profiles/r01_notes.md).  -1 / -2: spread the LDS-DMA pieces of the next K tile between the MFMA
 * groups / issue them in front of the tile (default).  8844: the 256x256 eight-phase kernel
 * (csrc/conv_pp_bf16.hip).  -3 / -4 / -5: chained stream-K schedule (a tile cut between two workgroups
 * continues from the stored fp32 accumulators; bit-identical) off / by the heuristic / wherever the
 * tile count allows it.  -6 / -7: eight-phase kernel never / by the heuristic.  -11 / -12 (test hook): stream-K heads
 * stop / resume publishing and tails give up after 256 polls -- a lost hand-over on demand, to exercise
 * BRCNN_EHANDOVER.  -15 / -16 / -17: the persistent kernel of the plain K = 64 / 128 1x1 layers (csrc/conv1x1_stream_bf16.hip:
 * weights resident in LDS, x / residual tiles through LDS-DMA rings) never / by the heuristic (default) / wherever the shape
 * allows; bit-identical.  8842: the 256x128 two-group kernel (csrc/conv_pp128_bf16.hip) wherever its shape rules allow.
 * fp16 operands run the production tiles whatever the code, except that 8844 / 8842 force the two eight-phase kernels
 * for fp16 as for bf16; any non-zero code keeps the persistent 1x1 kernel out (both types). */
int brcnn_conv_set_tile_bf16(int mtnt);

/* The same convolution over `num_segments` feature maps that share one set of weights (the
 * RetinaRPN tower and heads run over 5 pyramid levels, atss_rpn_head.py:296-297): x and y hold
 * the segments back to back ((N,H_s,W_s,Cin) then the next), one launch covers all of them. */
int brcnn_conv2d_nhwc_multi(const void *x, const void *w, const float *scale, const float *shift,
                            const void *residual, void *y, int batch, int num_segments,
                            const int *heights_host, const int *widths_host, int cin, int cout,
                            int kh, int kw, int stride, int pad, int relu, int dtype,
                            void *stream);

/* Winograd F(2x2,3x3) form of the fp32 3x3 stride-1 pad-1 convolution over the same segment table
 * (csrc/conv_winograd_f32.hip): 4 multiplies per output and input channel instead of 9.
 *   brcnn_winograd_filter_f32: w (Cout,3,3,Cin) packed fp32 -> u (16,Cout,Cin) = G g G^T, once per weight.
 *   ..._workspace_bytes: the V planes (16, tiles, cin) of the input transform, tiles = sum over the segments of
 *     batch * ceil(H/2) * ceil(W/2); 0 for arguments the conv would refuse (host arithmetic only, no device call).
 *   brcnn_conv3x3_winograd_f32_multi: y (rows, cout) = [relu](conv3x3(x') * scale + shift), scale / shift NULL = none;
 *     x' = x, or with gn_stats != NULL x' = [relu_in](groupnorm(x)) from the finalized (mean, rstd) pairs a GroupNorm
 *     call over the same segments left in its stats_ws, with gamma / beta (cin) and `groups` -- the expression of the
 *     GroupNorm apply pass, so the result has the bits of GroupNorm launch -> this call without gn_stats; the zero
 *     padding surrounds the NORMALISED tensor.
 * fp32 only (dtype BRCNN_DT_F32), kh = kw = 3, stride 1, pad 1, cin % 32 == 0, cout % 64 == 0, a workspace of at least
 * ..._workspace_bytes: anything else is BRCNN_EINVAL and launches nothing (no fall-back inside the entry point).
 * Results differ from brcnn_conv2d_nhwc_multi by fp32 round-off (about 2.5x its error against float64). */
int brcnn_winograd_filter_f32(const void *w, void *u, int cout, int cin, int kh, int kw, int dtype, void *stream);
size_t brcnn_conv3x3_winograd_f32_multi_workspace_bytes(int batch, int num_segments, const int *heights_host,
                                                        const int *widths_host, int cin);
int brcnn_conv3x3_winograd_f32_multi(const void *x, const void *u, const void *gn_stats, const float *gamma,
                                     const float *beta, int groups, int relu_in, const float *scale,
                                     const float *shift, int relu, void *y, void *workspace, size_t workspace_bytes,
                                     int batch, int num_segments, const int *heights_host, const int *widths_host,
                                     int cin, int cout, int kh, int kw, int stride, int pad, int dtype, void *stream);

/* The same form for ONE frozen conv + folded-BN / bias (+ ReLU) layer: x (batch, height, width, cin) -> y (batch, height,
 * width, cout) = [relu](conv3x3(x) * scale + shift), u from brcnn_winograd_filter_f32, the workspace of
 * ..._multi_workspace_bytes(batch, 1, &height, &width, cin).  The GEMM's workgroup tile (64 x 128, 32 x 128 or 64 x 64 tiles x
 * channels; equal bits) follows the measured rule or the hook (-14, 20 + v).  Same refusals as the entry above, no fall-back.
 *   brcnn_winograd_layer_route: host arithmetic only, launches nothing.  1 when the policy sends a layer of `tiles` =
 *     batch * ceil(H/2) * ceil(W/2) output tiles and this form to brcnn_conv3x3_winograd_f32_layer, else 0: always 0 for
 *     anything but 3x3, stride 1, pad 1, dilation 1, groups 1, cin % 32 == 0, cout % 64 == 0, BRCNN_DT_F32, and while
 *     (-11, 0) or (-14, 0) is set; (-14, 2): 1 for every such layer; (-14, 1), the default: the rule measured on MI355X
 *     (profiles/f32_winograd_layers.txt).  The caller must hold the transformed filter of the layer.
 *   brcnn_winograd_layer_gemm_variant: the GEMM tile (1 / 2 / 3) the layer entry would launch for (tiles, cout). */
int brcnn_conv3x3_winograd_f32_layer(const void *x, const void *u, const float *scale, const float *shift, int relu,
                                     void *y, void *workspace, size_t workspace_bytes, int batch, int height, int width,
                                     int cin, int cout, int kh, int kw, int stride, int pad, int dtype, void *stream);
int brcnn_winograd_layer_route(int tiles, int cin, int cout, int kh, int kw, int stride, int pad, int dilation,
                               int groups, int dtype);
int brcnn_winograd_layer_gemm_variant(int tiles, int cout);
/* The measured rule of the persistent launch of the Winograd GEMM (host arithmetic only): 1 when a launch of
 * `workgroup_tiles` GEMM tiles of `units` xi planes each runs as `per_cu` balanced workgroups on each of `cus` CUs, 0 when it
 * stays one workgroup per tile (profiles/f32_winograd_persistent.txt). */
int brcnn_winograd_persistent_rule(int workgroup_tiles, int units, int cus, int per_cu);

/* Grouped convolution (ResNeXt bottleneck conv2, mmdet/models/backbones/resnext.py:10-84).
 * x (N,H,W,Cin) fp32; w_tiles (Cout,KH,KW,window) block-diagonal per 64-channel output tile
 * (tile t = co/64 reads input channels [t*window, (t+1)*window), window = 64*cg_in/cg_out,
 * a multiple of 32; Cout % 64 == 0); same fused epilogue as brcnn_conv2d_nhwc. */
int brcnn_conv2d_nhwc_grouped(const void *x, const void *w_tiles, const float *scale,
                              const float *shift, const void *residual, void *y, int batch,
                              int height, int width, int cin, int cout, int kh, int kw, int stride,
                              int pad, int window, int relu, int dtype, void *stream);
/* its backward: dgrad with w_t_tiles = the grouped packing of the flipped, (co<->ci)-transposed
 * per-group filters; wgrad into dw_tiles (Cout,KH,KW,window) (zero-filled by the caller, fp32
 * atomics), of which the block-diagonal entries are the parameter gradient. */
int brcnn_conv2d_dgrad_nhwc_grouped(const void *dy, const void *w_t_tiles, void *dx, int batch,
                                    int in_height, int in_width, int out_height, int out_width, int cin,
                                    int cout, int kh, int kw, int stride, int pad, int window, int dtype,
                                    void *stream);
int brcnn_conv2d_wgrad_nhwc_grouped(const void *x, const void *dy, void *dw_tiles, int batch, int height,
                                    int width, int cin, int cout, int kh, int kw, int stride, int pad,
                                    int window, int dtype, void *stream);

/* Backward of the convolution (autograd of the trainable convs / FCs; the reference gets these
 * from cuDNN/cuBLAS through torch autograd).
 * dgrad: dx (N,H,W,Cin) from dy (N,Ho,Wo,Cout) and w_t (Cin,KH,KW,Cout) =
 *   flipped + transposed weights (w_t[ci,a,b,co] = w[co,KH-1-a,KW-1-b,ci]); in_* are the
 *   forward-input sizes (of dx), out_* the forward-output sizes (of dy).
 * wgrad: dw (Cout,KH,KW,Cin) += sum over pixels of dy x im2col(x); dw must be zero-filled
 *   by the caller (fp32 atomics across the slices of the pixel dimension). */
int brcnn_conv2d_dgrad_nhwc_multi(const void *dy, const void *w_t, void *dx, int batch,
                                  int num_segments, const int *in_heights_host,
                                  const int *in_widths_host, const int *out_heights_host,
                                  const int *out_widths_host, int cin, int cout, int kh, int kw,
                                  int stride, int pad, int dtype, void *stream);
int brcnn_conv2d_wgrad_nhwc_multi(const void *x, const void *dy, void *dw, int batch,
                                  int num_segments, const int *heights_host,
                                  const int *widths_host, int cin, int cout, int kh, int kw,
                                  int stride, int pad, int dtype, void *stream);
/* Deferred second stage of the sliced 16-bit weight gradients (csrc/wgrad_defer.hip).  A sliced launch of
 * brcnn_conv2d_wgrad_nhwc_multi / _grouped (bf16, fp16) writes one fp32 slab per slice of the pixel dimension and adds the
 * slabs into dw with a second launch.  After brcnn_wgrad_defer_begin(stream, arena, bytes, max_items) the launches on
 * `stream` take their slabs from the caller-owned `arena` (device memory, 256-byte aligned, >= 1 MiB; a launch whose slabs
 * exceed it keeps the immediate form) and the second stages of up to `max_items` (<= 64; <= 0: 64) launches wait for
 * brcnn_wgrad_defer_flush(stream): ONE table-driven launch with the same additions in the same order -- dw is bit for bit
 * the immediate result, but complete only after the flush.  A full arena / table flushes by itself before the next
 * producing launch.  arena NULL: deferral off (pending items are flushed first).  _flush returns the number of items
 * reduced (>= 0) or an error; _pending the number waiting.  The reference has no counterpart (cuDNN's weight gradient is
 * one call, mmdet/models/backbones/resnet.py:263-302 via torch.nn.Conv2d). */
int brcnn_wgrad_defer_begin(void *stream, void *arena, size_t bytes, int max_items);
int brcnn_wgrad_defer_flush(void *stream);
int brcnn_wgrad_defer_pending(void *stream);
int brcnn_wgrad_defer_stats(void *stream, long long *flushes, long long *items);
/* per-step operand preparation of a trainable conv: weight (Cout,Cin,KH,KW) fp32 (the reference's
 * parameter layout) -> fwd (Cout,KH,KW,Cin) and / or dgrad (Cin,KH,KW,Cout) with flipped taps, in
 * `dtype`; either output may be NULL. */
int brcnn_pack_conv_weights(const float *weight, void *fwd, void *dgrad, int cout, int cin, int kh, int kw,
                            int dtype, void *stream);
/* tuning hook of the bf16 wgrad kernel: 0 heuristic, 1 = 64x64 output tile, 2 = 128x128, 4 = 256x256 (16 waves);
 * 10 / 11: the M slices of a tile are reduced with fp32 atomics / through per-workgroup slabs and a fixed-order
 * second stage (default: reproducible bit for bit, faster) */
int brcnn_conv_set_tile_wgrad_bf16(int wt);

/* ResNet stem: 7x7 / stride 2 / pad 3 convolution of the 3-channel NCHW image + folded BN +
 * ReLU (resnet.py:599-611,631-636) -> y (N,Ho,Wo,Cout) NHWC.  w_packed fp32: (Cout,7,1,32) with
 * w_packed[co,kh,0,kw*4+c] = w[co,c,kh,kw]; 16-bit: (Cout,4,1,64) with w_packed[co,t,0,r*32+kw*4+c] =
 * w[co,c,2t+r,kw] (two filter rows per 128-byte K row); zeros elsewhere.  workspace:
 * brcnn_stem_workspace_bytes() bytes (zero-bordered NHWC4 repack of the image). */
size_t brcnn_stem_workspace_bytes(int batch, int height, int width);
int brcnn_stem7x7s2_nchw(const float *img, const void *w_packed, const float *scale,
                         const float *shift, void *y, void *workspace, int batch, int height,
                         int width, int cout, int relu, int dtype, void *stream);

/* The same stem followed by its 3x3/s2/p1 max-pool (resnet.py:611,631-636) in ONE launch, 64 output channels, ReLU
 * always: y (N,Hp,Wp,64) NHWC in `dtype` (BRCNN_DT_F32 / BF16 / F16).  The image tile of a workgroup's 7 x 8 pooled
 * outputs is staged in LDS once; the conv output never reaches memory.  w_packed: K index of filter row kh, tap kw,
 * channel c = kh*22 + kw*3 + c (fp32; stored [k/2][co/32][k%2][co%32], 154 x 64 floats) or kh*32 + kw*4 + c (16-bit;
 * stored [co][232]), zeros elsewhere.  cout must be 64. */
int brcnn_stem7x7s2_pool_nchw(const float *img, const void *w_packed, const float *scale, const float *shift,
                              void *y, int batch, int height, int width, int cout, int dtype, void *stream);

/* Tail of a frozen stage-1 Bottleneck (resnet.py Bottleneck.forward:263-302) in one fp32 launch:
 * y = relu(bn3(conv3_1x1(relu(bn2(conv2_3x3(x))))) + identity), x (N,H,W,64), w2 (64,3,3,64), w3 (256,1,1,64) packed
 * (Cout,KH,KW,Cin), scale / shift = the folded eval-mode BatchNorms (NULL: 1 / 0), identity / y (N,H,W,256); N*H*W must be
 * a multiple of 64.  The 64-channel intermediate stays in LDS; bit-identical to the two brcnn_conv2d_nhwc launches. */
int brcnn_bottleneck_tail_f32(const float *x, const float *w2, const float *scale2, const float *shift2, const float *w3,
                              const float *scale3, const float *shift3, const float *identity, float *y, int batch,
                              int height, int width, void *stream);
/* ... and with 16-bit tensors (dtype BRCNN_DT_BF16 / BRCNN_DT_F16: x, w2, w3, identity, y; fp32 accumulation, the
 * intermediate rounded to the 16-bit type as the two-launch form stores it); N*H*W must be a multiple of 128. */
int brcnn_bottleneck_tail_16(const void *x, const void *w2, const float *scale2, const float *shift2, const void *w3,
                             const float *scale3, const float *shift3, const void *identity, void *y, int batch,
                             int height, int width, int dtype, void *stream);

/* 3x3/s2/p1 max-pool of the ResNet stem (resnet.py:611), NHWC fp32/bf16 */
int brcnn_maxpool3x3s2_nhwc(const void *x, void *y, int batch, int height, int width,
                            int channels, int dtype, void *stream);
/* its backward (a trainable stem: frozen_stages < 0): dx[n,h,w,c] = sum of dy over the windows whose first
 * maximum (row-major scan, torch's argmax rule) is (h,w); x / y are the forward's input / output */
int brcnn_maxpool3x3s2_nhwc_backward(const void *x, const void *y, const void *dy, void *dx, int batch,
                                     int height, int width, int channels, int dtype, void *stream);

/* GroupNorm(+ReLU) over NHWC (RPN tower ConvModule norm, atss_rpn_head.py:118,150-190):
 * y = relu?((x-mean_g)/sqrt(var_g+eps)*gamma[c]+beta[c]); stats per (n, group). */
int brcnn_groupnorm_nhwc(const void *x, const float *gamma, const float *beta, void *y,
                         void *stats_ws /* batch*groups*2 doubles of device scratch */,
                         int batch, int hw, int channels, int groups, float eps, int relu,
                         int dtype, void *stream);

int brcnn_groupnorm_nhwc_multi(const void *x, const float *gamma, const float *beta, void *y,
                               void *stats_ws /* batch*num_segments*groups*2 doubles */,
                               int batch, int num_segments, const int *hw_host, int channels,
                               int groups, float eps, int relu, int dtype, void *stream);
/* its statistics alone (fp32 only): stats_ws as the full call leaves it, no y -- for a consumer that applies the
 * normalisation while it loads its operand (the gn_stats argument of the Winograd conv above) */
int brcnn_groupnorm_nhwc_multi_stats(const void *x, void *stats_ws, int batch, int num_segments, const int *hw_host,
                                     int channels, int groups, float eps, int dtype, void *stream);

/* Backward of brcnn_groupnorm_nhwc_multi (training of the RPN tower: GroupNorm(32) + ReLU of
 * mmcv's ConvModule, atss_rpn_head.py:150-170; torch's native group-norm backward needs NCHW
 * and costs two layout copies per layer and direction).  `x` is the forward input, `stats` the
 * forward's stats_ws (mean / rstd per (segment, image, group) after the forward call), `relu`
 * the forward's flag (the clipped positions are recomputed from x).  Writes dx (same layout and
 * dtype as x), dgamma / dbeta (channels, fp32, overwritten).  Deterministic except for the
 * double-precision group sums (atomics).  Accepts what the forward accepts, in every dtype:
 * channels <= 256, channels % 4 == 0, channels % groups == 0; anything else is BRCNN_EINVAL
 * and writes nothing. */
size_t brcnn_groupnorm_nhwc_multi_backward_workspace_bytes(int batch, int num_segments, const int *hw_host,
                                                           int channels, int groups);
int brcnn_groupnorm_nhwc_multi_backward(const void *dy, const void *x, const void *stats, const float *gamma,
                                        const float *beta, void *dx, float *dgamma, float *dbeta,
                                        void *workspace, size_t workspace_bytes, int batch, int num_segments,
                                        const int *hw_host, int channels, int groups, int relu, int dtype,
                                        void *stream);

/* Element-wise tail of a trainable conv block in training (eval-mode BatchNorm = per-channel
 * affine whose gamma / beta still train, resnet.py:263-302 with norm_eval=True):
 *   forward   out = [relu](z * scale[c] + shift[c] [+ residual])          (rows, C) NHWC rows
 *   backward  dpre = dout * (out > 0);  dz = dpre * scale[c];  dres = dpre (optional);
 *             dscale[c] = sum_rows dpre * z;  dshift[c] = sum_rows dpre    (fp32; two-stage,
 *             deterministic: per-strip partials in `workspace`, then a column reduction)
 * C % 4 == 0 (fp32) / C % 8 == 0 (bf16); backward needs C/vec to be a power of two or >= 256. */
int brcnn_bn_act_forward(const void *z, const float *scale, const float *shift, const void *residual,
                         void *out, int64_t rows, int channels, int relu, int dtype, void *stream);
size_t brcnn_bn_act_backward_workspace_bytes(int64_t rows, int channels, int dtype);
int brcnn_bn_act_backward(const void *dout, const void *out, const void *z, const float *scale,
                          void *dz, void *dres, float *dscale, float *dshift, void *workspace,
                          size_t workspace_bytes, int64_t rows, int channels, int relu, int dtype,
                          void *stream);

/* Training forward of conv -> eval-mode BatchNorm [-> + residual] [-> ReLU] in one launch (the trainable
 * Bottleneck layers, backbones/resnet.py:263-302 with norm_eval=True): z_out receives the raw conv output
 * (what brcnn_bn_eval_act_backward needs for dgamma and for the recomputed ReLU mask), y the activation;
 * both (rows, cout) in `dtype`.  mean / var NULL: gamma / beta are a plain per-channel scale / shift.
 * 16-bit dtypes (BRCNN_DT_BF16 / BRCNN_DT_F16), cout % 8 == 0; geometry as brcnn_conv2d_nhwc_multi. */
int brcnn_conv2d_bn_act_nhwc_multi(const void *x, const void *w, const float *gamma, const float *beta,
                                   const float *mean, const float *var, float eps, const void *residual,
                                   void *z_out, void *y, int batch, int num_segments,
                                   const int *heights_host, const int *widths_host, int cin, int cout,
                                   int kh, int kw, int stride, int pad, int relu, int dtype, void *stream);

/* Data gradient of a conv whose input came out of conv -> eval-BN -> [ReLU] (conv2 / conv3 of a Bottleneck,
 * backbones/resnet.py:263-302), with THAT BatchNorm's backward folded into the epilogue: what leaves is
 * dz_prev = (dx masked by the producer's ReLU, z_prev * scale + shift > 0) * scale -- the gradient of the
 * producer's raw conv output -- plus dgamma / dbeta of the producer's BatchNorm (per-row-tile partial sums in
 * `workspace`, summed in a fixed order).  dy (batch, out_h, out_w, cout), w_t (cin, kh, kw, cout) flipped /
 * transposed as for brcnn_conv2d_dgrad_nhwc_multi, z_prev / dz_prev (batch, in_h, in_w, cin).  16-bit dtypes,
 * cin % 64 == 0, cout % 64 == 0.  Values equal brcnn_conv2d_dgrad_nhwc_multi followed by
 * brcnn_bn_eval_act_backward (dz bit for bit; dgamma / dbeta up to the summation order).
 * Residual producer (bn3 of the previous Bottleneck, whose output is this conv's input AND the identity of this
 * block): dskip = the identity branch's gradient (added to the data gradient first, as
 * brcnn_conv2d_nhwc's residual operand does), prev_out = the producer's output (ReLU mask: > 0 instead of the
 * recomputed z * scale + shift), dres receives the masked sum -- the previous block's identity gradient.  All
 * three NULL for a producer without residual. */
size_t brcnn_conv2d_dgrad_bn_backward_workspace_bytes(int batch, int in_height, int in_width, int cin);
int brcnn_conv2d_dgrad_bn_backward_nhwc(const void *dy, const void *w_t, const void *z_prev, const float *gamma,
                                        const float *beta, const float *mean, const float *var, float eps, int relu,
                                        const void *dskip, const void *prev_out, void *dres,
                                        void *dz_prev, float *dgamma, float *dbeta, void *workspace,
                                        size_t workspace_bytes, int batch, int in_height, int in_width,
                                        int out_height, int out_width, int cin, int cout, int kh, int kw, int stride,
                                        int pad, int dtype, void *stream);

/* The same pair with the eval-mode BatchNorm parameters themselves (norm_eval=True,
 * backbones/resnet.py:648-657): scale = gamma / sqrt(var + eps), shift = beta - mean * scale are formed
 * inside the kernels (the reference spends ~5 element-wise torch launches per layer and direction on
 * them), and the backward returns dgamma = (sum dpre*z - mean * sum dpre) / sqrt(var + eps),
 * dbeta = sum dpre directly. */
int brcnn_bn_eval_act_forward(const void *z, const float *gamma, const float *beta, const float *mean,
                              const float *var, float eps, const void *residual, void *out, int64_t rows,
                              int channels, int relu, int dtype, void *stream);
/* `out` (the forward output, read for the ReLU mask) may be NULL when the forward had NO residual and
 * `beta` is given: the mask is then recomputed as z * scale + shift > 0 and one of the four streams
 * of the backward pass is not read at all. */
int brcnn_bn_eval_act_backward(const void *dout, const void *out, const void *z, const float *gamma,
                               const float *beta, const float *mean, const float *var, float eps, void *dz, void *dres,
                               float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes,
                               int64_t rows, int channels, int relu, int dtype, void *stream);
/* Deferred second stage.  Both backward entries above end with a small launch that turns the per-strip partial sums
 * in `workspace` into dgamma / dbeta (16 - 128 workgroups, ~7 us): a backward pass issues ~40 of them, serial on
 * the launching stream, and nothing reads their results before the optimizer.  With defer_second_stage != 0 the `_ex`
 * forms record that stage instead (workspace, dgamma, dbeta, mean, var must stay valid until the flush) and
 * brcnn_bn_reduce_flush(stream) runs everything recorded for `stream` in one launch per 48 layers -- same sums in the
 * same order, same bits; returns the number of stages it ran, < 0 on error.  brcnn_bn_reduce_pending: recorded, not yet
 * run (all streams). */
int brcnn_bn_eval_act_backward_ex(const void *dout, const void *out, const void *z, const float *gamma,
                                  const float *beta, const float *mean, const float *var, float eps, void *dz, void *dres,
                                  float *dgamma, float *dbeta, void *workspace, size_t workspace_bytes,
                                  int64_t rows, int channels, int relu, int dtype, void *stream, int defer_second_stage);
int brcnn_conv2d_dgrad_bn_backward_nhwc_ex(const void *dy, const void *w_t, const void *z_prev, const float *gamma,
                                           const float *beta, const float *mean, const float *var, float eps, int relu,
                                           const void *dskip, const void *prev_out, void *dres,
                                           void *dz_prev, float *dgamma, float *dbeta, void *workspace,
                                           size_t workspace_bytes, int batch, int in_height, int in_width,
                                           int out_height, int out_width, int cin, int cout, int kh, int kw, int stride,
                                           int pad, int dtype, void *stream, int defer_second_stage);
int brcnn_bn_reduce_flush(void *stream);
int brcnn_bn_reduce_pending(void);

/* Training-mode BatchNorm (norm_eval=False: F.batch_norm(training=True)) over (rows, C) NHWC rows in fp32 / bf16 /
 * fp16; gamma, beta, the statistics and the running buffers are fp32 (C each).
 *   brcnn_bn_train_stats: per channel mean and biased var over the rows of the STORED z (two stages: per-strip partial
 *     sums as doubles in `workspace`, then one launch that adds them in a fixed order and finalizes); writes
 *       save_mean, save_rstd = 1 / sqrt(var + eps)           (for the backward)
 *       scale = gamma save_rstd, shift = beta - mean scale    (the apply pass is brcnn_bn_act_forward on these)
 *       batch_var (may be NULL): the biased variance
 *     and updates in place  running_mean <- (1 - momentum) running_mean + momentum mean,
 *                           running_var  <- (1 - momentum) running_var  + momentum var rows / (rows - 1).
 *   brcnn_bn_train_backward: dpre = dout * (out > 0) (relu; `out` = the saved forward output, ignored without relu),
 *       dbeta = sum dpre,  dgamma = save_rstd sum dpre (z - save_mean)    (same two stages, same workspace size)
 *       dz = gamma save_rstd (dpre - dbeta / rows - xh dgamma / rows),  xh = (z - save_mean) save_rstd
 *       dres = dpre (optional: NULL without a residual)
 * No atomics: results are bit-identical from run to run.  C % 4 == 0 (fp32) / C % 8 == 0 (16-bit) and C / vec a power of
 * two (what brcnn_bn_act_backward takes below 256 vectors); rows >= 2 (one value per channel has no variance); rows * C * 16
 * must fit int64.  Anything else: BRCNN_EINVAL, and the workspace query returns 0.  `workspace` 8-byte aligned. */
size_t brcnn_bn_train_workspace_bytes(int64_t rows, int channels, int dtype);
int brcnn_bn_train_stats(const void *z, const float *gamma, const float *beta, float eps, float momentum,
                         float *running_mean, float *running_var, float *save_mean, float *save_rstd,
                         float *batch_var, float *scale, float *shift, void *workspace, size_t workspace_bytes,
                         int64_t rows, int channels, int dtype, void *stream);
int brcnn_bn_train_backward(const void *dout, const void *out, const void *z, const float *gamma,
                            const float *save_mean, const float *save_rstd, void *dz, void *dres, float *dgamma,
                            float *dbeta, void *workspace, size_t workspace_bytes, int64_t rows, int channels,
                            int relu, int dtype, void *stream);

/* Res2Net / DCNv2 rows (the r2_101 recipes): NHWC average pooling with torch.nn.AvgPool2d's
 * window / divisor rules (res2net.py:52-54, 173-178), and mmcv's modulated deformable im2col
 * (ModulatedDeformConv2dPack, deform_groups 1): col (N*Ho*Wo, KH*KW*channels_padded) with K
 * order (tap, c); `offset_mask` is the raw conv_offset output (N,Ho,Wo,>=3*KH*KW) NHWC with
 * om_stride floats per pixel: [2t] = dy, [2t+1] = dx of tap t, [2*KH*KW + t] = mask logit. */
int brcnn_avgpool_nhwc(const float *x, float *y, int batch, int height, int width, int channels,
                       int kernel, int stride, int pad, int ceil_mode, int count_include_pad,
                       void *stream);
int brcnn_deform_im2col_nhwc(const float *x, const float *offset_mask, float *col, int batch,
                             int height, int width, int channels, int kh, int kw, int stride, int pad,
                             int dilation, int om_stride, int channels_padded, void *stream);
/* backward of the above: dx (zero-filled by the caller, fp32 atomics) and d_offset_mask (N,Ho,Wo,
 * 3*KH*KW; every entry written) from dcol; the mask sigmoid's derivative is included. */
int brcnn_deform_col2im_nhwc(const float *x, const float *offset_mask, const float *dcol, float *dx,
                             float *d_offset_mask, int batch, int height, int width, int channels, int kh,
                             int kw, int stride, int pad, int dilation, int om_stride, int channels_padded,
                             void *stream);
/* 16-bit forms (dtype BRCNN_DT_BF16 | BRCNN_DT_F16; BRCNN_DT_F32 runs the fp32 entries above unchanged).  x / y / col
 * in the 16-bit type, offset_mask and every gradient in fp32.  avgpool: fp32 sums and divisor, one rounding.  im2col:
 * channels and channels_padded multiples of 8; each sample is the fp32 value of the fp32 im2col on the widened input,
 * rounded once to nearest even.  col2im: dcol (N*Ho*Wo, KH*KW*channels_padded) fp32 -> dx fp32 (zero-filled by the
 * caller, atomics; the caller converts it) and d_offset_mask fp32. */
int brcnn_avgpool_nhwc_ex(const void *x, void *y, int batch, int height, int width, int channels, int kernel,
                          int stride, int pad, int ceil_mode, int count_include_pad, int dtype, void *stream);
int brcnn_deform_im2col_nhwc_ex(const void *x, const float *offset_mask, void *col, int batch, int height,
                                int width, int channels, int kh, int kw, int stride, int pad, int dilation,
                                int om_stride, int channels_padded, int dtype, void *stream);
int brcnn_deform_col2im_nhwc_ex(const void *x, const float *offset_mask, const float *dcol, float *dx,
                                float *d_offset_mask, int batch, int height, int width, int channels, int kh,
                                int kw, int stride, int pad, int dilation, int om_stride, int channels_padded,
                                int dtype, void *stream);
/* Fused modulated deformable 3x3 conv (csrc/deform_conv_bf16.hip), 16-bit only (dtype BRCNN_DT_BF16 | BRCNN_DT_F16):
 * y = [relu](scale * (im2col16(x, offset_mask) . w^T) + shift) in one launch, the columns never stored.
 * x (N,H,W,channels) with channels % 64 == 0; offset_mask (N,Ho,Wo,om_stride >= 27) fp32 raw conv_offset output;
 * w (cout,3,3,channels) with cout in {64, 128, 256}; stride 1 or 2; scale / shift (cout) fp32 or NULL (shift alone:
 * a bias); y (N,Ho,Wo,cout) 16-bit.  The A operand equals brcnn_deform_im2col_nhwc_ex's columns bit for bit. */
int brcnn_deform_conv_nhwc(const void *x, const float *offset_mask, const void *w, const float *scale,
                           const float *shift, void *y, int batch, int height, int width, int channels, int cout,
                           int stride, int pad, int relu, int om_stride, int dtype, void *stream);
/* Deform groups and the unmodulated form (mmcv DeformConv2dPack, `type='DCN'`; ResNet dconv_c3-c5 backbones).  With
 * T = KH*KW taps and G = deform_groups (channels % G == 0; channel c belongs to group c / (channels / G); the pad
 * channels c >= channels stay zero and belong to no group) an offset row of a pixel holds [2 T g + 2 t] = dy and
 * [2 T g + 2 t + 1] = dx of tap t in group g and, when `modulated`, the mask logit at [2 T G + T g + t] -- mmcv's
 * `o1, o2, mask = chunk(out, 3); offset = cat(o1, o2)`; G = 1 is the layout of the entries above.  modulated = 0: the
 * mask factor is identically 1, no sigmoid is evaluated, rows have 2 T G entries (v1 is DEFINED as the v2
 * restatement with that factor).  dtype BRCNN_DT_F32 | _BF16 | _F16; (channels / G) % 4 == 0 in fp32, % 8 == 0 in 16 bits.
 * im2col: om_stride >= (modulated ? 3 : 2) T G; col2im: om_stride equal to it, every entry of d_offset_mask written.
 * With G = 1, modulated = 1 they equal the entries above bit for bit (dx: up to the order of its atomics). */
int brcnn_deform_im2col_nhwc_g(const void *x, const float *offset_mask, void *col, int batch, int height, int width,
                               int channels, int kh, int kw, int stride, int pad, int dilation, int om_stride,
                               int channels_padded, int deform_groups, int modulated, int dtype, void *stream);
int brcnn_deform_col2im_nhwc_g(const void *x, const float *offset_mask, const float *dcol, float *dx,
                               float *d_offset_mask, int batch, int height, int width, int channels, int kh, int kw,
                               int stride, int pad, int dilation, int om_stride, int channels_padded, int deform_groups,
                               int modulated, int dtype, void *stream);
/* brcnn_deform_col2im_nhwc_g whose dx carries the same bits from run to run: the contributions are added as 64-bit integers
 * (integer addition does not depend on the order the waves arrive in; fp32 atomics do) and converted once.  The grid comes
 * from the data of the call: a pre-pass takes m = max |dcol| and its binary exponent ex (m < 2^ex); a contribution (dcol *
 * mask * corner weight, at most m in magnitude) is scaled by 2^(S - ex), S = 62 - ceil(log2(Ho * Wo * kh * kw * 4)), so that
 * even every sample of an image on one pixel sums below 2^62: no overflow at any finite input.  Precision: a contribution is
 * rounded to a multiple of 2^(ex - S), an absolute error of at most m * 2^-S each (S = 41 for a 100 x 168 map, 50 for
 * 6 x 7); one of at least m * 2^(24 - S) keeps all 24 bits of fp32, one below m * 2^(-S - 1) is dropped -- where the fp32
 * atomics of the other entry keep the relative precision of every partial sum instead.  A dcol or a contribution that is
 * not finite makes every element of dx NaN.  d_offset_mask is the other entry's, bit for bit.  workspace:
 * brcnn_deform_col2im_ordered_workspace_bytes (8 bytes per element of dx + 8).  The star deformable convs of VFNetHead train
 * through this entry. */
size_t brcnn_deform_col2im_ordered_workspace_bytes(int batch, int height, int width, int channels);
int brcnn_deform_col2im_nhwc_ordered(const void *x, const float *offset_mask, const float *dcol, float *dx,
                                     float *d_offset_mask, int batch, int height, int width, int channels, int kh, int kw,
                                     int stride, int pad, int dilation, int om_stride, int channels_padded, int deform_groups,
                                     int modulated, int dtype, void *workspace, size_t workspace_bytes, void *stream);
/* The fused 16-bit deformable 3x3 conv with deform groups, modulated or not, any cout % 64 == 0 (output-channel blocks in
 * the grid).  Requires (channels / deform_groups) % 64 == 0 (a K step -- one tap x 64 channels -- then lies inside one
 * group) and om_stride >= (modulated ? 27 : 18) * deform_groups; anything else is refused with BRCNN_EINVAL and the
 * caller runs brcnn_deform_im2col_nhwc_g + the GEMM.  The A operand equals brcnn_deform_im2col_nhwc_g's 16-bit columns
 * bit for bit; modulated = 0 loads no mask and evaluates no sigmoid. */
int brcnn_deform_conv_nhwc_g(const void *x, const float *offset_mask, const void *w, const float *scale,
                             const float *shift, void *y, int batch, int height, int width, int channels, int cout,
                             int stride, int pad, int relu, int om_stride, int deform_groups, int modulated, int dtype,
                             void *stream);
/* Which route a caller takes for a 16-bit deformable conv of this shape: 1 = brcnn_deform_conv_nhwc_g, 0 = im2col + GEMM
 * (also for every shape the fused entry refuses).  Reads the policy switch brcnn_conv_set_tile(-13, 0 / 1 / 2): im2col +
 * GEMM always / the measured rule (default) / fused wherever accepted; (-13, 3) returns the setting; (-13, 10) and
 * (-13, 11) return and clear the launches of the fused kernel and of the deformable im2col kernels (tests). */
int brcnn_deform_conv_route(int batch, int height, int width, int channels, int cout, int stride, int pad,
                            int deform_groups, int dtype);

/* FPN top-down path: dst[n,y,x,c] += src[n, y*Hs/Hd, x*Ws/Wd, c]  (nearest,
 * F.interpolate(size=...) at necks/pafpn.py:113-115, fpn.py:178-181) */
int brcnn_upsample_nearest_add_nhwc(void *dst, const void *src, int batch, int hd, int wd,
                                    int hs, int ws, int channels, int dtype, void *stream);
/* differentiable form: out = dst + nearest_upsample(src) into a separate tensor, and the gradient w.r.t.
 * src (every source pixel sums the gradient of the destination pixels that read it; d/d dst is dout) */
int brcnn_upsample_nearest_add_nhwc_out(const void *dst, const void *src, void *out, int batch, int hd,
                                        int wd, int hs, int ws, int channels, int dtype, void *stream);
int brcnn_upsample_nearest_add_nhwc_backward(const void *dout, void *dsrc, int batch, int hd, int wd, int hs,
                                             int ws, int channels, int dtype, void *stream);

/* column sums of a (rows, channels) fp32 / bf16 tensor into fp32 (bias gradients of the convs / FCs:
 * db = sum_rows dy), two fixed-order stages (deterministic); channels / 4 a power of two or >= 256 */
size_t brcnn_colsum_workspace_bytes(int64_t rows, int channels);
int brcnn_colsum(const void *x, float *out, void *workspace, size_t workspace_bytes, int64_t rows,
                 int channels, int dtype, void *stream);

/* layout shuffles between the reference's NCHW boundary and the NHWC interior */
int brcnn_nchw_to_nhwc(const float *src, void *dst, int batch, int channels, int hw,
                       int dst_dtype, void *stream);
int brcnn_nhwc_to_nchw(const void *src, float *dst, int batch, int channels, int hw,
                       int src_dtype, void *stream);

/* ------------------------------------------------------------------------------
 * RetinaRPN proposal stage (ATSSRPNHead._get_bboxes_single,
 * atss_rpn_head.py:688-760, with AnchorGenerator.single_level_grid_anchors
 * core/anchor/anchor_generator.py:336-381 and delta2bbox
 * core/bbox/coder/delta_xywh_bbox_coder.py:145-272 fused in).
 *
 * brcnn_rpn_score: score[r*A + a] = sqrt(sigmoid(cls)*sigmoid(iou)) over `rows` pixels of
 *   NHWC head output; consecutive pixels are cls_stride / iou_stride floats apart (A when the
 *   tensor is dense, 54 when the fused cls|reg|iou head output is read in place).
 *   bbox_pred likewise has pred_stride floats per pixel and is multiplied by pred_scale
 *   (the level's learnable Scale) before decoding.
 * brcnn_rpn_decode: for `count` selected anchors (flat index into (H*W*A) of one
 *   level) regenerate the anchor from base_anchors (A,4) + stride, apply
 *   delta2bbox(means 0, stds `std4`, wh_ratio_clip) with max_shape clipping; writes
 *   proposals (count,4) and valid (count) uint8 = w > min_size && h > min_size.
 * brcnn_rpn_topk: for every (image, level) the `k` best scores of the level's `n` anchors in
 *   (score descending, index ascending) order -- the reference sorts the whole level and keeps
 *   nms_pre (atss_rpn_head.py:727-737); exact radix select + an in-LDS sort of the winners.
 *   score_levels / out_score / out_idx are HOST arrays of device pointers, one per level:
 *   score (batch, n_l), out_score / out_idx (batch, min(k, n_l)).  A level with n_l <= k is
 *   passed through in index order, as the reference does.  k <= 4096.  Levels of >= 32768 anchors
 *   are selected in up to 8 parts and merged (two launches; device scratch in `workspace`).
 * -------------------------------------------------------------------------- */
int brcnn_rpn_score(const float *cls, const float *iou, float *score, int64_t rows,
                    int num_anchors, int cls_stride, int iou_stride, void *stream);
int brcnn_rpn_decode(const int64_t *topk_inds, const float *bbox_pred, int pred_stride,
                     float pred_scale, const float *base_anchors,
                     int batch, int count, int height, int width, int num_anchors, int stride_w,
                     int stride_h, const float *means4_host, const float *stds4_host,
                     double wh_ratio_clip, float max_h, float max_w, float min_size,
                     float *proposals, uint8_t *valid, void *stream);

/* brcnn_rpn_decode for all pyramid levels in one launch: level l's picked anchors (topk_inds[l],
 * (batch, counts[l])) are decoded into columns [sum counts[:l], +counts[l]) of proposals
 * (batch, T, 4) / valid (batch, T) / ids (batch, T) (ids = the level index: the `level_ids` of
 * atss_rpn_head.py:738-740 that batched_nms separates by).  Host arrays of device pointers. */
int brcnn_rpn_decode_levels(const int64_t *const *topk_inds, const float *const *bbox_pred,
                            const int *pred_strides, const float *pred_scales,
                            const float *const *base_anchors, int batch, int num_levels, const int *counts,
                            const int *heights, const int *widths, int num_anchors, const int *strides_w,
                            const int *strides_h, const float *means4_host, const float *stds4_host,
                            double wh_ratio_clip, float max_h, float max_w, float min_size,
                            float *proposals, uint8_t *valid, int64_t *ids, void *stream);
/* the same with the per-level scales read from DEVICE memory (num_levels floats): the training
 * proposal stage decodes with the live Scale parameters without reading them back to the host;
 * max_shape_dev (batch, 2) [h, w] device = per-image clip border (img_shape differs inside a
 * training batch), or NULL to use max_h / max_w */
int brcnn_rpn_decode_levels_dscale(const int64_t *const *topk_inds, const float *const *bbox_pred,
                                   const int *pred_strides, const float *pred_scales_dev,
                                   const float *max_shape_dev, const float *const *base_anchors, int batch, int num_levels, const int *counts,
                                   const int *heights, const int *widths, int num_anchors, const int *strides_w,
                                   const int *strides_h, const float *means4_host, const float *stds4_host,
                                   double wh_ratio_clip, float max_h, float max_w, float min_size,
                                   float *proposals, uint8_t *valid, int64_t *ids, void *stream);

/* Second-stage candidates of a whole batch in one launch: the score fusion of
 * prob_roi_head.py:232-240 and ProbConvFCBBoxHead.get_bboxes (convfc_bbox_head.py:294-330) up to
 * the NMS call.  probs (batch*per_image, C+1) softmax outputs, bbox_pred (batch*per_image, 4C),
 * proposals (batch, per_image, 5) [x1,y1,x2,y2,prior] zero padded with num[b] real rows,
 * max_shape (batch, 2) [h, w], scale_factor (batch, 4) or NULL.  Writes, in (proposal, class)
 * order, boxes (batch, per_image*C, 4), scores = sqrt(prob * prior), labels = class, valid =
 * score > score_thr and the row is real. */
int brcnn_rcnn_decode(const float *probs, const float *bbox_pred, const float *proposals, const int32_t *num,
                      const float *max_shape, const float *scale_factor, int batch, int per_image,
                      int num_classes, float score_thr, const float *means4_host, const float *stds4_host,
                      double wh_ratio_clip, float *boxes, float *scores, int64_t *labels, uint8_t *valid,
                      void *stream);

/* The un-fused form for the standard head (BBoxHead.get_bboxes, bbox_heads/bbox_head.py:317-379): same
 * layout and outputs as brcnn_rcnn_decode, but scores = prob (the softmax alone; column 4 of the
 * proposals is not read), and with reg_class_agnostic != 0 bbox_pred is (batch*per_image, 4) and every
 * class of a proposal reads that one box. */
int brcnn_rcnn_decode_plain(const float *probs, const float *bbox_pred, const float *proposals, const int32_t *num,
                            const float *max_shape, const float *scale_factor, int batch, int per_image,
                            int num_classes, int reg_class_agnostic, float score_thr, const float *means4_host,
                            const float *stds4_host, double wh_ratio_clip, float *boxes, float *scores,
                            int64_t *labels, uint8_t *valid, void *stream);

/* ------------------------------------------------------------------------------
 * Cascade R-CNN (CascadeRoIHead, mmdet/models/roi_heads/cascade_roi_head.py): handing boxes from one stage to
 * the next, one launch each on the padded (batch, per_image, 5) layout, no host read.  fp32 only: the heads'
 * last GEMM writes fp32 logits and deltas in every compute mode.  cls_score / bbox_pred are read in place:
 * cls_stride / reg_stride are the floats between two consecutive rows (>= C+1, >= 4 | 4C), so the two column
 * blocks of the heads' fused output need no copy.  Plain stores, no float atomics: two runs give the same bits.
 *
 * brcnn_cascade_refine_test -- the between-stage step of CascadeRoIHead.simple_test (cascade_roi_head.py:342-372)
 *   over BBoxHead.regress_by_class (roi_heads/bbox_heads/bbox_head.py:461-496).  dets (batch, per_image, 5) zero
 *   padded with num[b] real rows, cls_score (batch*per_image, C+1) raw logits, bbox_pred (batch*per_image, 4 | 4C),
 *   max_shape (batch, 2) [h, w]; means / stds / wh_ratio_clip of THIS stage's coder.  Per real row: label =
 *   argmax over the C foreground columns (:368; the lowest index on ties, torch's rule; the background column
 *   takes no part), delta2bbox of the row's 4 deltas (reg_class_agnostic) or the label's 4 (:482-485), clipped
 *   to max_shape (:488-495).  Writes dets_out (batch, per_image, 5): boxes in columns 0-3, column 4 zero,
 *   padded rows zero.  The same launch accumulates the logits the row has just read (:357 ms_scores):
 *   first != 0: logit_sum = cls_score, else logit_sum += cls_score (one fp32 add, stage order); logit_sum is
 *   (batch*per_image, C+1) dense, every row.
 *
 * brcnn_cascade_mean_softmax -- the ensemble of cascade_roi_head.py:374-378 and the softmax of
 *   BBoxHead.get_bboxes (bbox_head.py:354-355): probs (rows, C+1) = softmax((logit_sum + cls_score_last) /
 *   float(num_stages)); the sum in stage order, ONE fp32 division (no reciprocal).  num_stages == 1 reads
 *   cls_score_last alone (logit_sum may be NULL).  probs feeds brcnn_rcnn_decode_plain.  mean_logits (rows, C+1) or
 *   NULL: the averaged logits themselves, for inspection (the tests pin them bit for bit).
 *
 * brcnn_cascade_refine_train -- BBoxHead.refine_bboxes (bbox_head.py:382-458) as CascadeRoIHead.forward_train
 *   calls it (cascade_roi_head.py:264-284): rois (N, 5) / labels (N) int64 / gt_flags (N) int32 as
 *   brcnn_rcnn_sample_gt wrote them, image b owning rows [row_offsets_host[b], row_offsets_host[b+1]) (HOST,
 *   batch+1 ints, at most 2048 rows per image).  A background row (label == C) takes the arg-max foreground
 *   class (:279-281), every other row keeps its label; decode + clip as above; the rows with gt_flags set are
 *   dropped (:451-456) wherever they sit, the survivors keep their order.  Writes props_out (batch, rows_out, 5)
 *   zero padded (column 4 zero) and num_out (batch) int32 on the device: the next stage's proposals for
 *   brcnn_assign_max_iou / brcnn_rcnn_sample.  rows_out >= the largest per-image row count. */
int brcnn_cascade_refine_test(const float *dets, const int32_t *num, const float *cls_score, int cls_stride,
                              const float *bbox_pred, int reg_stride, const float *max_shape, int batch,
                              int per_image, int num_classes, int reg_class_agnostic, int first,
                              const float *means4_host, const float *stds4_host, double wh_ratio_clip,
                              float *dets_out, float *logit_sum, void *stream);
int brcnn_cascade_mean_softmax(const float *logit_sum, const float *cls_score_last, int cls_stride, int64_t rows,
                               int num_classes, int num_stages, float *probs, float *mean_logits, void *stream);
int brcnn_cascade_refine_train(const float *rois, const int64_t *labels, const int32_t *gt_flags,
                               const int *row_offsets_host, int batch, const float *cls_score, int cls_stride,
                               const float *bbox_pred, int reg_stride, const float *max_shape, int num_classes,
                               int reg_class_agnostic, const float *means4_host, const float *stds4_host,
                               double wh_ratio_clip, int rows_out, float *props_out, int32_t *num_out,
                               void *stream);

/* ------------------------------------------------------------------------------
 * Test-time augmentation (multi-scale + flip), whole batch, no host round trip: the device form of
 * TwoStageDetector.aug_test (detectors/two_stage.py:184-193).  Per-(aug, image) geometry is one device
 * table geom (num_augs, batch, 8) = [img_h, img_w, sf0, sf1, sf2, sf3, flip, 0] built by the host from
 * img_metas (scale_factor as the meta carries it, [sx, sy, sx, sy]; flip 0 none, 1 horizontal, 2
 * vertical, 3 diagonal).  Coordinates are mapped with the reference's fp32 operations in its order
 * (core/bbox/transforms.py:6-56: `w - x2`, true division by the scale factor), bit for bit.
 * -------------------------------------------------------------------------- */
#define BRCNN_TTA_MAX_AUGS 16
#define BRCNN_TTA_FUSED 0 /* per aug sqrt(softmax(cls_score) * prior) (prob_roi_head.py:232-240), then the mean */
#define BRCNN_TTA_RAW 1   /* the mean of the logits, prior ignored: aug_test_bboxes as the reference runs it    */

/* merge_aug_proposals up to its NMS call (core/post_processing/merge_augs.py:61-72).  proposals[a]
 * (batch, per_aug_host[a], 5) [x1,y1,x2,y2,score] zero padded with num[a][b] real rows (host arrays of
 * num_augs device pointers).  Writes the T = sum per_aug_host candidate slots of every image, aug-major
 * (the reference's torch.cat order = the tie order of the NMS), mapped back to the original image
 * (bbox_mapping_back): candidates (batch, T, 5), valid (batch, T) = the row is real (others are zero),
 * and, where not NULL, the same rows split as boxes (batch, T, 4) / scores (batch, T) for
 * brcnn_nms_prepare. */
int brcnn_tta_gather_proposals(const float *const *proposals, const int32_t *const *num, const int *per_aug_host,
                               int num_augs, const float *geom, int batch, float *candidates, float *boxes,
                               float *scores, uint8_t *valid, void *stream);

/* bbox_mapping (transforms.py:35-44) of the merged proposals into every aug's frame, as RoIs (the loop
 * head of aug_test_bboxes, roi_heads/test_mixins.py:142-151): merged (batch, per_image, 5) in the
 * original frame -> rois (num_augs, batch*per_image, 5) [image, x1, y1, x2, y2], x scale factor then
 * flip. */
int brcnn_tta_map_rois(const float *merged, const float *geom, int num_augs, int batch, int per_image,
                       float *rois, void *stream);

/* The TTA form of brcnn_rcnn_decode: aug_test_bboxes + merge_aug_bboxes (test_mixins.py:138-165,
 * merge_augs.py:84-110) up to the NMS call.  cls_score (num_augs, batch*per_image, C+1) RAW logits,
 * bbox_pred (num_augs, batch*per_image, 4C), merged (batch, per_image, 5) proposals in the original
 * frame with num[b] real rows, out_scale (batch, 4) or NULL (aug 0's scale factor: results in the frame
 * of imgs[0], prob_roi_head.py:190-193).  Per (proposal, class), over the augs in order: the score
 * (mode BRCNN_TTA_FUSED: max-subtracted fp32 softmax of the row, sqrt(p * prior); BRCNN_TTA_RAW: the
 * logit) and delta2bbox of the proposal as mapped into the aug's frame, clipped at the aug's img_shape
 * and mapped back; sums divided by num_augs.  Outputs as brcnn_rcnn_decode: boxes (batch, per_image*C,
 * 4), scores, labels = class, valid = score > score_thr and the row is real. */
int brcnn_rcnn_decode_tta(const float *cls_score, const float *bbox_pred, const float *merged, const int32_t *num,
                          const float *geom, const float *out_scale, int num_augs, int batch, int per_image,
                          int num_classes, int mode, float score_thr, const float *means4_host,
                          const float *stds4_host, double wh_ratio_clip, float *boxes, float *scores,
                          int64_t *labels, uint8_t *valid, void *stream);

size_t brcnn_rpn_topk_workspace_bytes(const int *n_host, int num_levels, int batch, int k);
int brcnn_rpn_topk(const float *const *score_levels, const int *n_host, int num_levels,
                   int batch, int k, float *const *out_score, int64_t *const *out_idx,
                   void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------
 * Input front door: the reference's Resize -> RandomFlip -> Normalize -> Pad
 * transforms (mmdet/datasets/pipelines/transforms.py:31-315,318-470,700-739,625-697; the image
 * arithmetic is mmcv.imresize = cv2.resize INTER_LINEAR on uint8, mmcv.imflip,
 * mmcv.imnormalize, mmcv.impad) of ONE decoded image as one pass.
 *   src  (src_h, src_w, 3) uint8, BGR, dense        dst (3, pad_h, pad_w) fp32, CHW
 *   the image is resized to (new_h, new_w) with OpenCV's 8-bit fixed-point bilinear, flipped
 *   (flip: 0 none, 1 horizontal, 2 vertical, 3 diagonal), converted BGR->RGB when to_rgb,
 *   normalised (v - mean[c]) * fp32(1/std[c]) (mean/std in the OUTPUT channel order, host
 *   arrays of 3) and zero-padded at the bottom / right to (pad_h, pad_w).
 * -------------------------------------------------------------------------- */
int brcnn_preprocess_u8(const uint8_t *src, int src_h, int src_w, float *dst, int new_h,
                        int new_w, int pad_h, int pad_w, int flip, const float *mean3_host,
                        const float *std3_host, int to_rgb, void *stream);

/* ------------------------------------------------------------------------------
 * Batched input front door: the same transform chain for a whole (augmentations x images) batch
 * in ONE launch (test pipelines: MultiScaleFlipAug over a batch of decoded images).
 *   src       ONE device buffer of src_bytes bytes: the source images back to back, each
 *             (src_h, src_w, 3) uint8 BGR dense, ragged sizes; uploaded once whatever the number of augs
 *   jobs_dev  device copy of the job table, one row per (aug a, image b), 8-byte aligned
 *   jobs_host the host copy of the same num_jobs rows (<= BRCNN_PRE_MAX_JOBS): every row is
 *             validated on it before anything is queued (sizes, flip, both blocks' bounds, the
 *             scales, first_block), and the grid is sized from it -- the kernel trusts the table
 *   dst       device buffer of dst_elems floats, 16-byte aligned; job (a, b) writes EVERY element of
 *             the (3, pad_h, pad_w) fp32 CHW image at dst + dst_off: pixels, then zeros -- with
 *             dst_off = off_a + b * 3 * pad_h * pad_w and (pad_h, pad_w) the aug's batch shape, aug a's
 *             rows form one contiguous (B, 3, pad_h, pad_w) tensor
 *   a row:    src_off (bytes into src), dst_off (floats into dst), scale_x = 1.0 / ((double)new_w /
 *             (double)src_w) and scale_y likewise (exactly these doubles, as brcnn_preprocess_u8
 *             computes them), src_h, src_w, new_h, new_w, pad_h, pad_w, flip (0-3 as above), and
 *             first_block = the sum of brcnn_preprocess_u8_batch_blocks(pad_h, pad_w) of the rows before it
 *   mean / std / to_rgb as above, per launch.  16-byte stores where pad_w % 4 == 0 and dst_off % 4 == 0,
 *   4-byte stores otherwise.  Every image equals brcnn_preprocess_u8's bit for bit.
 * -------------------------------------------------------------------------- */
#define BRCNN_PRE_MAX_JOBS 4096
typedef struct brcnn_pre_job {
    int64_t src_off, dst_off;
    double scale_x, scale_y;
    int32_t src_h, src_w, new_h, new_w, pad_h, pad_w, flip, first_block;
} brcnn_pre_job;                                   /* 64 bytes */

int64_t brcnn_preprocess_u8_batch_blocks(int pad_h, int pad_w);
int brcnn_preprocess_u8_batch(const uint8_t *src, size_t src_bytes, const brcnn_pre_job *jobs_dev,
                              const brcnn_pre_job *jobs_host, int num_jobs, float *dst,
                              size_t dst_elems, const float *mean3_host, const float *std3_host,
                              int to_rgb, void *stream);

/* ------------------------------------------------------------------------------
 * Training front door of the multi-scale recipes: AutoAugment's crop policy
 * [RandomFlip ->] Resize -> RandomCrop -> Resize(override) [-> RandomFlip] -> Normalize -> Pad
 * (mmdet/datasets/pipelines/auto_augment.py:44-109, transforms.py:742-896 and the lines cited above) of ONE
 * decoded image as one pass.
 *   src  (src_h, src_w, 3) uint8, BGR, dense        dst (3, pad_h, pad_w) fp32, CHW, every element written
 *   the source, mirrored by src_flip (0-3 as above: a RandomFlip in FRONT of the policies), is resized to a
 *   virtual (mid_h, mid_w) uint8 image that is never stored; its window [top, top + crop_h) x [left, left +
 *   crop_w) is resized to (new_h, new_w) -- both with OpenCV's 8-bit fixed-point bilinear, both rounded to
 *   uint8, the second with its taps clamped to the window -- then flipped by `flip` (a RandomFlip BEHIND the
 *   policies), converted, normalised and zero-padded as brcnn_preprocess_u8 does.  A stage whose sizes match
 *   is the identity: mid = src gives crop + resize, window = whole and new = crop gives brcnn_preprocess_u8
 *   (bit for bit).  The host draws every random number; the launch only sees the geometry.
 *   -22 and no launch for: a NULL pointer, a size <= 0, a window that leaves the virtual image, pad < new, a
 *   flip code outside 0-3, a zero std, a source of 2 GiB or more.
 * -------------------------------------------------------------------------- */
int brcnn_preprocess_u8_chain(const uint8_t *src, int src_h, int src_w, int src_flip, int mid_h, int mid_w,
                              int top, int left, int crop_h, int crop_w, float *dst, int new_h, int new_w,
                              int pad_h, int pad_w, int flip, const float *mean3_host,
                              const float *std3_host, int to_rgb, void *stream);

/* ------------------------------------------------------------------------------
 * Train step: whole-batch target assignment, RoI sampling and the fused losses.
 * The reference runs these per image / per level as chains of small torch ops with host
 * synchronisations (nonzero / unique / .item()); each entry below serves the whole batch.
 * Ground truth is passed flat: gts (sum G, 4) [+ gt_labels (sum G) int64], image b owning rows
 * [gt_offsets_host[b], gt_offsets_host[b+1]) (HOST array of batch+1 ints; batch <= BRCNN_MAX_IMAGES).
 *
 * brcnn_assign_max_iou -- MaxIoUAssigner.assign (mmdet/core/bbox/assigners/max_iou_assigner.py:61-213)
 *   over BboxOverlaps2D (core/bbox/iou_calculators/iou2d_calculator.py:30-261, mode 'iou').
 *   boxes: image b's n rows start at boxes + b*box_batch_stride (0: shared anchors), box_row_stride
 *   floats per row (5 for proposals with a score column); num_boxes (batch) real rows or NULL.
 *   num_levels > 0 describes RPN anchors (level_start_host[L+1] first anchor of each level,
 *   level_width_host[L] cells per row, anchors_per_cell): valid_hw (batch, L, 2) device
 *   [valid_h, valid_w] in cells reproduces AnchorGenerator.valid_flags
 *   (core/anchor/anchor_generator.py:383-440), img_hw (batch, 2) + allowed_border >= 0
 *   anchor_inside_flags (core/anchor/utils.py:21-47); either may be NULL.  Boxes that fail take no
 *   part and come out as -1.  neg_iou_thr as [neg_iou_lo, neg_iou_hi) (a float thr is [0, thr)).
 *   gt_max_ws (sum G) uint32 scratch for match_low_quality.  Writes gt_inds (batch, n) int32
 *   (-1 ignore, 0 negative, k matched to gt k-1), max_overlaps (batch, n) or NULL, counts (batch, 2)
 *   [#positive, #negative] or NULL.  Index-exact with the reference on the host (first maximum on
 *   ties, later ground truth overriding earlier in the low-quality pass).
 *
 * brcnn_rcnn_sample -- RandomSampler.sample (core/bbox/samplers/base_sampler.py:35-102,
 *   random_sampler.py:32-82), SamplingResult (sampling_result.py:26-55), the prior extraction of
 *   ProbRoIHead.forward_train (models/roi_heads/prob_roi_head.py:51-64), bbox2roi
 *   (core/bbox/transforms.py:59-78) and BBoxHead._get_target_single (bbox_heads/bbox_head.py:122-196).
 *   proposals (batch, per_image, 5) zero padded with num_props[b] real rows; gt_inds / max_overlaps
 *   from brcnn_assign_max_iou on them.  perm (batch, num_expected_pos + num) int32: image b's first
 *   num_expected_pos entries are torch.randperm(n_pos)[:num_expected_pos] when n_pos exceeds it, the
 *   rest randperm(n_neg)[:expected_neg] likewise (drawn on the host: the reference's seeded stream);
 *   row_offsets_host (batch+1): first output row of each image (host knows the counts).
 *   list_ws (batch, 2, list_stride) int32 scratch, list_stride >= per_image + max G.
 *   Writes rois (N,5), labels (N) int64 (background = num_classes), bbox_targets (N,4) (encoded
 *   with means / stds, or the matched gt box when reg_decoded_bbox), priors (N), ious (N) or NULL
 *   (`quality`), pos_flags (N) int32 or NULL; rows of an image are [positives | negatives], each
 *   ascending in candidate index.
 *
 * brcnn_rpn_loss_* -- ATSSRPNHead.loss / loss_single (models/dense_heads/atss_rpn_head.py:299-464)
 *   for every RPN loss configuration of the recipes: reg_decoded_bbox=True with IoULoss(mode 'log')
 *   [+ MSELoss aug] or reg_decoded_bbox=False with CIoULoss on the raw deltas (:361-374, the FPN
 *   recipe); FocalLoss or VarifocalLoss (:393-400, the VOC recipe); sigmoid-BCE IoU branch.
 *   y (rows, ystride) is the fused head output of all levels, level-major rows
 *   (level l: batch*H_l*W_l rows), channels [cls A | reg 4A | iou A | padding]; scales (L) the
 *   per-level Scale parameters (device); gt_inds (batch, anchors per image) from
 *   brcnn_assign_max_iou.  cfg20_host = [focal_gamma, focal_alpha, pos_weight, iou_gamma(self.gamma),
 *   mean4, std4, max_ratio |ln(wh_ratio_clip)|, with_aug, lw_cls, lw_bbox, lw_aug, lw_iou,
 *   cls_mode (0 FocalLoss, 1 VarifocalLoss iou_weighted, 2 VarifocalLoss not iou_weighted; gamma /
 *   alpha are then the varifocal ones), reg_mode (0 decoded IoU-log, 1 CIoU on raw deltas)].
 *   forward: sums (L, 6) [focal, iou-loss, mse, bce, iou_target, n_pos] and totals (2)
 *   [n_pos, sum iou_target] of THIS rank; the caller averages totals over ranks (reduce_mean,
 *   :440-444,458-460) and calls finalize: losses3 = [loss_rpn_cls, loss_rpn_bbox, loss_rpn_iou]
 *   summed over levels, per_level (3, L), coef2 = the two reciprocal normalisers the backward uses.
 *   backward: grad3 (3) device = dLoss/dlosses3; writes dy (rows, ystride) and dscales (L).
 *   Deterministic (fixed-order partial sums, no float atomics).
 *
 * brcnn_boost_loss_* -- ProbRoIHead._bbox_forward_train_boost + norm_loss
 *   (models/roi_heads/prob_roi_head.py:107-154) over ProbConvFCBBoxHead.loss
 *   (bbox_heads/convfc_bbox_head.py:332-418; CrossEntropyLoss + L1Loss, reduction 'none').
 *   cfg6_host = [gamma, alpha, iou_gamma, loss_cls weight, loss_bbox weight, reg_norm == 'mean'].
 *   out3 = [loss_cls, loss_bbox, acc]; backward: dcls (n, C+1), dbbox (n, 4C | 4).
 * -------------------------------------------------------------------------- */
/* bbox_overlaps (mmdet/core/bbox/iou_calculators/iou2d_calculator.py:75-261): mode 0 'iou', 1 'iof',
 * 2 'giou'; out (n1, n2), or (n1) when is_aligned (n1 == n2).  stride = floats per box row (4, or 5 with a
 * score column, which BboxOverlaps2D.__call__ strips, :30-66).  union / enclosing area clamped at eps. */
int brcnn_bbox_overlaps(const float *bboxes1, int stride1, int n1, const float *bboxes2, int stride2, int n2,
                        int mode, int is_aligned, float eps, float *out, void *stream);
int brcnn_assign_max_iou(const float *boxes, int64_t box_batch_stride, int box_row_stride,
                         const int32_t *num_boxes, int n, int batch, const float *gts,
                         const int *gt_offsets_host, int num_levels, const int *level_start_host,
                         const int *level_width_host, int anchors_per_cell, const int32_t *valid_hw,
                         const float *img_hw, float allowed_border, float pos_iou_thr, float neg_iou_lo,
                         float neg_iou_hi, float min_pos_iou, int match_low_quality, uint32_t *gt_max_ws,
                         int32_t *gt_inds, float *max_overlaps, int32_t *counts, void *stream);
int brcnn_rcnn_sample(const float *proposals, const int32_t *num_props, int per_image, int batch,
                      const int32_t *gt_inds, const float *max_overlaps, const float *gts,
                      const int64_t *gt_labels, const int *gt_offsets_host, int add_gt_as_proposals,
                      int num, int num_expected_pos, float neg_pos_ub, const int32_t *perm,
                      const int *row_offsets_host, int num_classes, int reg_decoded_bbox,
                      const float *means4_host, const float *stds4_host, int32_t *list_ws,
                      int list_stride, float *rois, int64_t *labels, float *bbox_targets, float *priors,
                      float *ious, int32_t *pos_flags, void *stream);
/* brcnn_rcnn_sample_gt -- the same launch and the same outputs, bit for bit, plus gt_flags (N) int32: 1 where the
 * row is a ground truth box the sampler added as a proposal (add_gt_as_proposals; SamplingResult.pos_is_gt,
 * core/bbox/samplers/sampling_result.py:32), wherever in the image's positives it sits.  These are the rows
 * BBoxHead.refine_bboxes drops between two cascade stages (brcnn_cascade_refine_train). */
int brcnn_rcnn_sample_gt(const float *proposals, const int32_t *num_props, int per_image, int batch,
                         const int32_t *gt_inds, const float *max_overlaps, const float *gts,
                         const int64_t *gt_labels, const int *gt_offsets_host, int add_gt_as_proposals,
                         int num, int num_expected_pos, float neg_pos_ub, const int32_t *perm,
                         const int *row_offsets_host, int num_classes, int reg_decoded_bbox,
                         const float *means4_host, const float *stds4_host, int32_t *list_ws,
                         int list_stride, float *rois, int64_t *labels, float *bbox_targets, float *priors,
                         float *ious, int32_t *pos_flags, int32_t *gt_flags, void *stream);
/* The sampled RPN loss of the Faster R-CNN baseline (RPNHead: AnchorHead.loss with a RandomSampler,
 * dense_heads/anchor_head.py:373-497, samplers/random_sampler.py:32-82).  y (rows, ystride) is the fused
 * head output of all levels, level-major rows, columns [objectness A | deltas 4A | padding]; gt_inds
 * (batch, n) from brcnn_assign_max_iou on the n anchors of an image.
 *   brcnn_rpn_sampled_draw: compacts every image's positive / negative candidates in index order and
 *     gathers the host-drawn picks (perm (batch, num_expected_pos + num) int32, the contract of
 *     brcnn_rcnn_sample) into drawn (batch, num) int32: positives, then negatives, then -1.
 *   brcnn_rpn_sampled_loss_forward / _finalize: losses2 = [loss_rpn_cls, loss_rpn_bbox] =
 *     loss_weight * sum over the drawn anchors of [w * bce_with_logits(x, is_pos), is_pos * sum_4
 *     l1 | smooth_l1_beta(pred - bbox2delta(anchor, gt))] / num_total_samples; coef2 keeps the two scale
 *     factors for the backward pass.  Fixed summation order, no float atomics.
 *   brcnn_rpn_sampled_loss_backward: dy (rows, ystride), zero wherever no drawn anchor reads y.
 * cfg13_host = [pos_weight (<= 0: 1), smooth_l1_beta (0: L1), means x4, stds x4, loss_weight_cls,
 * loss_weight_bbox, num_total_samples].  workspace: brcnn_rpn_sampled_workspace_bytes, shared by draw,
 * forward and finalize of one step. */
size_t brcnn_rpn_sampled_workspace_bytes(int batch, int anchors_per_image, int num);
int brcnn_rpn_sampled_draw(const int32_t *gt_inds, int anchors_per_image, int batch, int num,
                           int num_expected_pos, float neg_pos_ub, const int32_t *perm, void *workspace,
                           size_t workspace_bytes, int32_t *drawn, void *stream);
int brcnn_rpn_sampled_loss_forward(const float *y, int ystride, int batch, int num_levels, const int *heights,
                                   const int *widths, const int *strides_w, const int *strides_h,
                                   const float *const *base_anchors, int anchors_per_cell,
                                   const int32_t *gt_inds, const float *gts, const int *gt_offsets_host,
                                   const int32_t *drawn, int num, const float *cfg13_host, void *workspace,
                                   size_t workspace_bytes, void *stream);
int brcnn_rpn_sampled_loss_finalize(const void *workspace, int batch, int anchors_per_image, int num,
                                    const float *cfg13_host, float *losses2, float *coef2, void *stream);
int brcnn_rpn_sampled_loss_backward(const float *y, int ystride, int batch, int num_levels, const int *heights,
                                    const int *widths, const int *strides_w, const int *strides_h,
                                    const float *const *base_anchors, int anchors_per_cell,
                                    const int32_t *gt_inds, const float *gts, const int *gt_offsets_host,
                                    const int32_t *drawn, int num, const float *cfg13_host, const float *g2,
                                    const float *coef2, float *dy, void *stream);
size_t brcnn_rpn_loss_workspace_bytes(int batch, int num_levels, const int *heights, const int *widths,
                                      int anchors_per_cell);
int brcnn_rpn_loss_forward(const float *y, int ystride, int batch, int num_levels, const int *heights,
                           const int *widths, const int *strides_w, const int *strides_h,
                           const float *const *base_anchors, int anchors_per_cell, const float *scales,
                           const int32_t *gt_inds, const float *gts, const int *gt_offsets_host,
                           const float *cfg20_host, void *workspace, size_t workspace_bytes, float *sums,
                           float *totals, void *stream);
int brcnn_rpn_loss_finalize(const float *sums, const float *totals, int num_levels, const float *cfg20_host,
                            float *losses3, float *per_level, float *coef2, void *stream);
int brcnn_rpn_loss_backward(const float *y, int ystride, int batch, int num_levels, const int *heights,
                            const int *widths, const int *strides_w, const int *strides_h,
                            const float *const *base_anchors, int anchors_per_cell, const float *scales,
                            const int32_t *gt_inds, const float *gts, const int *gt_offsets_host,
                            const float *cfg20_host, const float *grad3, const float *coef2,
                            void *workspace, size_t workspace_bytes, float *dy, float *dscales,
                            void *stream);
size_t brcnn_boost_loss_workspace_bytes(int n);
int brcnn_boost_loss_forward(const float *cls_score, const float *bbox_pred, const int64_t *labels,
                             const float *priors, const float *ious, const float *bbox_targets, int n,
                             int num_classes, int reg_class_agnostic, const float *cfg6_host,
                             void *workspace, size_t workspace_bytes, float *out3, float *coef2,
                             void *stream);
int brcnn_boost_loss_backward(const float *cls_score, const float *bbox_pred, const int64_t *labels,
                              const float *priors, const float *ious, const float *bbox_targets, int n,
                              int num_classes, int reg_class_agnostic, const float *cfg6_host,
                              const float *grad3, const float *coef2, float *dcls, float *dbbox,
                              void *stream);
/* the same kernels with two more switches, cfg8_host = cfg6 + [plain, beta]:
 *   plain != 0: the boosted weights are LABEL WEIGHTS of the head's own loss -- loss_cls = sum(w * ce) / max(#{w > 0}, 1)
 *     (DyProbRoIHead._bbox_forward_train_boost, models/roi_heads/prob_roi_head.py:604-623 over
 *     bbox_heads/bbox_head.py loss; also gamma = 0 for its un-boosted branch) instead of norm_loss;
 *   beta > 0: SmoothL1Loss(beta) for the box term (models/losses/smooth_l1_loss.py:9-32; Dynamic R-CNN moves beta
 *     every update_iter_interval iterations), beta <= 0: L1Loss. */
int brcnn_boost_loss_forward_ex(const float *cls_score, const float *bbox_pred, const int64_t *labels,
                                const float *priors, const float *ious, const float *bbox_targets, int n,
                                int num_classes, int reg_class_agnostic, const float *cfg8_host,
                                void *workspace, size_t workspace_bytes, float *out3, float *coef2,
                                void *stream);
int brcnn_boost_loss_backward_ex(const float *cls_score, const float *bbox_pred, const int64_t *labels,
                                 const float *priors, const float *ious, const float *bbox_targets, int n,
                                 int num_classes, int reg_class_agnostic, const float *cfg8_host,
                                 const float *grad3, const float *coef2, float *dcls, float *dbbox,
                                 void *stream);

/* ------------------------------------------------------------------------------
 * The dense (single-stage) detection head: RetinaHead over AnchorHead (models/dense_heads/anchor_head.py), csrc/dense_head.hip.
 * Head outputs are NHWC and read in place: `rows` pixels with A * C class logits (anchor-major) resp. 4A deltas each,
 * consecutive pixels `*_stride` floats apart.
 *   brcnn_dense_score: score[r * A + a] = max_c sigmoid(cls[r, a * C + c]) (anchor_head.py:646-669), the maximum over the
 *     fp32 sigmoid VALUES; the dense (rows, A) result feeds brcnn_rpn_topk.
 *   brcnn_dense_decode_levels: everything between the top-k and multiclass_nms (anchor_head.py:672-710,
 *     core/post_processing/bbox_nms.py) for all levels and images in one launch.  Per level l: topk_inds[l] (batch,
 *     counts[l]) int64 flat anchor indices as brcnn_rpn_decode_levels takes them, cls[l] / bbox_pred[l] the level's head
 *     outputs (batch, h, w, stride).  max_shape (batch, 2) [h, w] the clip border, scale_factor (batch, 4) or NULL (a true
 *     fp32 division).  With T = sum(counts), in (level, pick, class) order -- the order of the reference's `nonzero`:
 *     boxes (batch, T*C, 4), scores (batch, T*C) the class sigmoid, labels (batch, T*C), valid (batch, T*C) = score >
 *     score_thr, and n_valid (batch) the number of valid candidates per image.
 *   brcnn_dense_loss_forward / _finalize / _backward: AnchorHead.loss without a sampler (anchor_head.py:373-491 with
 *     PseudoSampler).  cls (rows, cls_stride) / reg (rows, reg_stride): the head outputs of all levels, level-major rows
 *     (level l: batch * h_l * w_l rows).  gt_inds (batch, anchors per image) from brcnn_assign_max_iou: k > 0 positive
 *     (label gt_labels[gt_offsets[b] + k - 1]), 0 negative (background), < 0 label weight 0.  losses (2, L) =
 *     [loss_cls per level, loss_bbox per level]: loss_weight * sum / num_total_pos with the sigmoid focal term of
 *     brcnn_sigmoid_focal_loss_forward over every weighted (anchor, class) pair and L1 | SmoothL1 on pred -
 *     bbox2delta(anchor, gt) over the positives; num_total_pos = sum over images of max(n_pos, 1) is counted by forward
 *     and inverted by finalize on the device.  coef3 = [loss_weight_cls / num_total_pos, loss_weight_bbox /
 *     num_total_pos, num_total_pos] goes to backward, which writes every element of dcls / dreg (padding columns: 0).
 *     Fixed summation order, no float atomics.
 * cfg14_host = [focal gamma, focal alpha, pos_weight (<= 0: 1), smooth_l1_beta (0: L1), means x4, stds x4,
 * loss_weight_cls, loss_weight_bbox].  workspace: brcnn_dense_loss_workspace_bytes, shared by forward and finalize.
 * -------------------------------------------------------------------------- */
int brcnn_dense_score(const float *cls, float *score, int64_t rows, int num_anchors, int num_classes, int cls_stride,
                      void *stream);
int brcnn_dense_decode_levels(const int64_t *const *topk_inds, const float *const *cls, const int *cls_strides,
                              const float *const *bbox_pred, const int *pred_strides,
                              const float *const *base_anchors, int batch, int num_levels, const int *counts,
                              const int *heights, const int *widths, int num_anchors, int num_classes,
                              const int *strides_w, const int *strides_h, const float *max_shape,
                              const float *scale_factor, const float *means4_host, const float *stds4_host,
                              double wh_ratio_clip, float score_thr, float *boxes, float *scores, int64_t *labels,
                              uint8_t *valid, int32_t *n_valid, void *stream);
size_t brcnn_dense_loss_workspace_bytes(int batch, int num_levels, const int *heights, const int *widths,
                                        int anchors_per_cell, int num_classes);
int brcnn_dense_loss_forward(const float *cls, int cls_stride, const float *reg, int reg_stride, int batch,
                             int num_levels, const int *heights, const int *widths, const int *strides_w,
                             const int *strides_h, const float *const *base_anchors, int anchors_per_cell,
                             int num_classes, const int32_t *gt_inds, const float *gts, const int64_t *gt_labels,
                             const int *gt_offsets_host, const float *cfg14_host, void *workspace,
                             size_t workspace_bytes, void *stream);
int brcnn_dense_loss_finalize(const void *workspace, size_t workspace_bytes, int batch, int num_levels,
                              const int *heights, const int *widths, int anchors_per_cell, int num_classes,
                              const float *cfg14_host, float *losses, float *coef3, void *stream);
int brcnn_dense_loss_backward(const float *cls, int cls_stride, const float *reg, int reg_stride, int batch,
                              int num_levels, const int *heights, const int *widths, const int *strides_w,
                              const int *strides_h, const float *const *base_anchors, int anchors_per_cell,
                              int num_classes, const int32_t *gt_inds, const float *gts, const int64_t *gt_labels,
                              const int *gt_offsets_host, const float *cfg14_host, const float *grad_losses,
                              const float *coef3, float *dcls, float *dreg, void *stream);

/* ------------------------------------------------------------------------------
 * The anchor-free dense head: FCOSHead (models/dense_heads/fcos_head.py), csrc/fcos_head.hip.  The candidates are the cell
 * centres: level l with stride s, cell (y, x) is the point (x*s + s/2, y*s + s/2), s/2 an integer division.  The head
 * outputs are two fp32 row tensors over all levels (level-major rows, level l: batch * h_l * w_l rows), read in place:
 * A (rows, stride_a) holds the C class logits at column cls_off, R (rows, stride_r) the 4 RAW distances at column reg_off,
 * and the centerness logit is column ctr_off of A, or of R when ctr_in_r.  layout8_host = [stride_a, cls_off, stride_r,
 * reg_off, ctr_in_r, ctr_off, norm_on_bbox, giou].  scales: (L) floats ON THE DEVICE, the per-level Scale; the distance
 * is expf(scale_l * raw), or under norm_on_bbox max(scale_l * raw, 0) (times stride_l at test time only).
 *   brcnn_fcos_score: score[row] = max_c(sigmoid(cls_c) * sigmoid(ctr)) (fcos_head.py:396), the maximum over the fp32
 *     products; equal products tie and brcnn_rpn_topk's ascending-index rule decides.  Feeds brcnn_rpn_topk.
 *   brcnn_fcos_decode_levels: everything between the top-k and multiclass_nms(score_factors=centerness) for all levels and
 *     images in one launch.  topk_inds[l] (batch, counts[l]) int64 cell indices of level l.  Box (px - d0, py - d1,
 *     px + d2, py + d3) clipped to max_shape (batch, 2) [h, w], divided by scale_factor (batch, 4) unless NULL.  With T =
 *     sum(counts), in (level, pick, class) order: boxes (batch, T*C, 4), scores = sigmoid(cls_c) * sigmoid(ctr), labels,
 *     valid = sigmoid(cls_c) > score_thr (the class score BEFORE the centerness factor), n_valid (batch).
 *   brcnn_fcos_assign: _get_target_single (fcos_head.py:546-628) for every (image, point): gt_inds (batch, points per
 *     image) int32, the index of the smallest-area ground truth of the image whose box (or centre box of radius
 *     stride_l * center_sample_radius, clipped to the box, under center_sampling) strictly contains the point and whose
 *     largest side distance lies in [ranges[2l], ranges[2l+1]]; ties go to the lowest index; -1 background.
 *   brcnn_fcos_loss_forward / _finalize / _backward: FCOSHead.loss (fcos_head.py:164-261).  forward leaves block partials
 *     in the workspace and norm2 = [n_pos, sum of the centerness targets] on the device (the caller may average norm2 over
 *     ranks); finalize forms N = max(norm2[0], 1), S = max(norm2[1], 1e-6), losses3 = [lw_cls * sum_focal / N, lw_bbox *
 *     sum(ctr_target * box_loss) / S, lw_ctr * sum_bce / N] and coef3 = [lw_cls / N, lw_bbox / S, lw_ctr / N]; backward
 *     writes every element of dA (rows, stride_a) and dR (rows, stride_r) (w.r.t. the RAW outputs; other columns 0) and
 *     dscale (L).  box_loss is -log(max(iou, eps_loss)) or, with giou, 1 - giou of the aligned bbox_overlaps with eps_overlap.
 *     Fixed summation order, no float atomics.  At most BRCNN_MAX_LEVELS levels and BRCNN_MAX_IMAGES images.
 * cfg7_host = [focal gamma, focal alpha, eps_overlap, eps_loss, loss_weight_cls, loss_weight_bbox, loss_weight_centerness].
 * workspace: brcnn_fcos_loss_workspace_bytes, shared by forward and finalize; backward takes one of the same size.
 * -------------------------------------------------------------------------- */
int brcnn_fcos_score(const float *a, const float *r, const int *layout8_host, int num_classes, int64_t rows, float *score,
                     void *stream);
int brcnn_fcos_decode_levels(const int64_t *const *topk_inds, const int *counts, const float *a, const float *r,
                             const int *layout8_host, const float *scales, int batch, int num_levels, const int *heights,
                             const int *widths, const int *strides, int num_classes, const float *max_shape,
                             const float *scale_factor, float score_thr, float *boxes, float *scores, int64_t *labels,
                             uint8_t *valid, int32_t *n_valid, void *stream);
int brcnn_fcos_assign(const float *gts, const int *gt_offsets_host, int batch, int num_levels, const int *heights,
                      const int *widths, const int *strides, const float *ranges_host, int center_sampling,
                      double center_sample_radius, int32_t *gt_inds, void *stream);
size_t brcnn_fcos_loss_workspace_bytes(int batch, int num_levels, const int *heights, const int *widths, int num_classes);
int brcnn_fcos_loss_forward(const float *a, const float *r, const int *layout8_host, const float *scales, int batch,
                            int num_levels, const int *heights, const int *widths, const int *strides, int num_classes,
                            const int32_t *gt_inds, const float *gts, const int64_t *gt_labels, const int *gt_offsets_host,
                            const float *cfg7_host, void *workspace, size_t workspace_bytes, float *norm2, void *stream);
int brcnn_fcos_loss_finalize(const void *workspace, size_t workspace_bytes, const float *norm2, int batch, int num_levels,
                             const int *heights, const int *widths, int num_classes, const float *cfg7_host,
                             float *losses3, float *coef3, void *stream);
int brcnn_fcos_loss_backward(const float *a, const float *r, const int *layout8_host, const float *scales, int batch,
                             int num_levels, const int *heights, const int *widths, const int *strides, int num_classes,
                             const int32_t *gt_inds, const float *gts, const int64_t *gt_labels, const int *gt_offsets_host,
                             const float *cfg7_host, const float *grad_losses3, const float *coef3, void *workspace,
                             size_t workspace_bytes, float *da, float *dr, float *dscale, void *stream);

/* ------------------------------------------------------------------------------
 * The ATSS head: ATSSHead + ATSSAssigner (models/dense_heads/atss_head.py, core/bbox/assigners/atss_assigner.py),
 * csrc/atss_head.hip.  ONE anchor per cell, never materialised: level l, cell (y, x) has the anchor base_l + (x * stride_l,
 * y * stride_l, x * stride_l, y * stride_l), base_anchors_host (L, 4) the generator's base anchors -- exact in fp32.  The head
 * outputs are FCOSHead's two row tensors A / R with their layout8_host (norm_on_bbox and giou are not read): RAW values,
 * level-major rows, the centerness wherever the layout puts it.  scales: (L) floats ON THE DEVICE; delta = scale_l * raw.
 * The per-anchor ranking score max_c(sigmoid(cls_c) * sigmoid(ctr)) is brcnn_fcos_score.
 *   brcnn_atss_assign: ATSSAssigner.assign (atss_assigner.py:34-179) for a whole batch.  gts (sum G, 4) packed with host
 *     offsets; valid_hw (batch, L, 2) int32 [valid_h, valid_w] in cells as brcnn_assign_max_iou takes it, or NULL = every
 *     cell valid (allowed_border < 0: inside flags = valid flags).  Per (ground truth, level) the candidates are the
 *     min(topk, VALID cells of the level) anchors nearest to the box centre by sqrt(dx*dx + dy*dy) of the fp32 centres
 *     (x1 + x2) / 2; EQUAL DISTANCES RANK BY ASCENDING ANCHOR INDEX (the reference leaves that tie to torch.topk, whose
 *     choice is unspecified; this rule is the library's own).  thr = mean + unbiased std of the candidates' IoUs
 *     (BboxOverlaps2D, eps 1e-6), summed sequentially in (level, rank) order; a candidate is positive when iou >= thr and
 *     min(cx - x1, cy - y1, x2 - cx, y2 - cy) > 0.01 (a NaN thr -- a single candidate -- makes none).  An anchor positive
 *     for several ground truths goes to the highest IoU, equal IoUs to the lowest index (an integer atomic max on
 *     (IoU bits << 32 | ~index): order-independent).  gt_inds (batch, anchors per image) int32: k > 0 positive for ground
 *     truth k - 1 of the image, 0 negative, -1 invalid cell; max_overlaps (same shape) or NULL: the winner's IoU, -1e8
 *     elsewhere.  workspace: batch * anchors per image * 8 bytes.  0 < topk <= 16.
 *   brcnn_atss_decode_levels: everything between the top-k and multiclass_nms(score_factors=centerness)
 *     (atss_head.py:372-504) as brcnn_fcos_decode_levels does it, the box being delta2bbox(anchor, scale_l * raw, means,
 *     stds, wh_ratio_clip) in brcnn_dense_decode_levels' operation order, clipped to max_shape, divided by scale_factor.
 *     valid = sigmoid(cls_c) > score_thr (BEFORE the centerness factor), score = sigmoid(cls_c) * sigmoid(ctr).
 *   brcnn_atss_loss_forward / _finalize / _backward: ATSSHead.loss (atss_head.py:143-310), the targets formed in the kernel
 *     from gt_inds (brcnn_atss_assign's convention; < 0: weight 0).  Per positive: target = bbox2delta(anchor, gt), gt' =
 *     delta2bbox(anchor, target) (the reference's round trip), centerness target sqrt(min(l,r)/max(l,r) * min(t,b)/max(t,b))
 *     from the anchor centre to gt', box loss (1 - giou(delta2bbox(anchor, scale_l * raw), gt')) * centerness target,
 *     centerness BCE.  forward leaves block partials and norm2 = [sum over images of max(n_pos, 1), sum of the centerness
 *     targets] on the device (the caller may average norm2 over ranks); finalize forms N = max(norm2[0], 1), S =
 *     max(norm2[1], 1), losses (3, L) = [lw_cls * focal_l / N | lw_bbox * box_l / S | lw_ctr * bce_l / N] per level and
 *     coef3 = [lw_cls / N, lw_bbox / S, lw_ctr / N]; backward takes grad_losses (3, L) and writes every element of dA and
 *     dR (w.r.t. the RAW outputs, through the scale, the decode, its exp and its clamp -- zero where the clamp is active;
 *     other columns 0) and dscale (L).  Fixed summation order, no float atomics.
 * cfg15_host = [focal gamma, focal alpha, giou eps, loss_weight_cls, loss_weight_bbox, loss_weight_centerness, means x4,
 * stds x4, |log(wh_ratio_clip)|].  workspace: brcnn_atss_loss_workspace_bytes, shared by forward and finalize; backward takes one
 * of the same size.  At most BRCNN_MAX_LEVELS levels and BRCNN_MAX_IMAGES images.
 * -------------------------------------------------------------------------- */
int brcnn_atss_assign(const float *gts, const int *gt_offsets_host, int batch, int num_levels, const int *heights,
                      const int *widths, const int *strides, const float *base_anchors_host, const int32_t *valid_hw,
                      int topk, void *workspace, size_t workspace_bytes, int32_t *gt_inds, float *max_overlaps,
                      void *stream);
int brcnn_atss_decode_levels(const int64_t *const *topk_inds, const int *counts, const float *a, const float *r,
                             const int *layout8_host, const float *scales, int batch, int num_levels, const int *heights,
                             const int *widths, const int *strides, const float *base_anchors_host, int num_classes,
                             const float *max_shape, const float *scale_factor, const float *means4_host,
                             const float *stds4_host, double wh_ratio_clip, float score_thr, float *boxes, float *scores,
                             int64_t *labels, uint8_t *valid, int32_t *n_valid, void *stream);
size_t brcnn_atss_loss_workspace_bytes(int batch, int num_levels, const int *heights, const int *widths, int num_classes);
int brcnn_atss_loss_forward(const float *a, const float *r, const int *layout8_host, const float *scales, int batch,
                            int num_levels, const int *heights, const int *widths, const int *strides,
                            const float *base_anchors_host, int num_classes, const int32_t *gt_inds, const float *gts,
                            const int64_t *gt_labels, const int *gt_offsets_host, const float *cfg15_host, void *workspace,
                            size_t workspace_bytes, float *norm2, void *stream);
int brcnn_atss_loss_finalize(const void *workspace, size_t workspace_bytes, const float *norm2, int batch, int num_levels,
                             const int *heights, const int *widths, int num_classes, const float *cfg15_host, float *losses,
                             float *coef3, void *stream);
int brcnn_atss_loss_backward(const float *a, const float *r, const int *layout8_host, const float *scales, int batch,
                             int num_levels, const int *heights, const int *widths, const int *strides,
                             const float *base_anchors_host, int num_classes, const int32_t *gt_inds, const float *gts,
                             const int64_t *gt_labels, const int *gt_offsets_host, const float *cfg15_host,
                             const float *grad_losses, const float *coef3, void *workspace, size_t workspace_bytes,
                             float *da, float *dr, float *dscale, void *stream);

/* ------------------------------------------------------------------------------
 * The GFL head: GFLHead with QualityFocalLoss / DistributionFocalLoss (models/dense_heads/gfl_head.py,
 * models/losses/gfocal_loss.py), csrc/gfl_head.hip.  ONE anchor per cell as for the ATSS head (base_anchors_host (L, 4)); only
 * its centre ((x1 + x2) / 2, (y1 + y2) / 2) is used.  The head outputs are two fp32 row tensors over all levels, level-major
 * rows, read in place: A (rows, stride_a) with the C class logits at column cls_off, R (rows, stride_r) with the 4 *
 * (reg_max + 1) RAW box logits at column reg_off, side-major [left | top | right | bottom].  layout4_host = [stride_a,
 * cls_off, stride_r, reg_off].  scales: (L) floats ON THE DEVICE; logit = scale_l * raw.  A side's distance is the
 * expectation sum p_i * i of the max-subtracted softmax over its reg_max + 1 logits; the exp sum and the expectation are
 * accumulated in bin order.  1 <= reg_max <= 16.  The per-anchor ranking score max_c sigmoid(cls_c) is brcnn_dense_score
 * with one anchor per cell, reading A in place; the assignment is brcnn_atss_assign.
 *   brcnn_gfl_decode_levels: everything between the top-k and multiclass_nms (gfl_head.py:373-472) as
 *     brcnn_fcos_decode_levels does it: box = (cx - d0 * s, cy - d1 * s, cx + d2 * s, cy + d3 * s) with s = stride_l, clipped
 *     to max_shape, divided by scale_factor; score = sigmoid(cls_c), valid = score > score_thr; (level, pick, class) order.
 *   brcnn_gfl_loss_forward / _finalize / _backward: GFLHead.loss (gfl_head.py:211-371), the targets formed in the kernel from
 *     gt_inds (brcnn_atss_assign's convention; < 0: weight 0), everything in units of the stride.  Per positive: centre /
 *     stride, target = gt / stride, decoded box from the four integrals, quality = aligned bbox_overlaps(decoded, target)
 *     (eps 1e-6) and weight = max_c sigmoid(cls_c), both constants; box loss weight * (1 - giou); DFL with t =
 *     clamp(distance to the target side, 0, reg_max - 0.1), left = floor(t): (CE(left) * (left + 1 - t) + CE(left + 1) *
 *     (t - left)) summed over the sides, * weight / 4.  Class term over every (anchor, class) of a valid cell: BCE(x, 0) *
 *     sigmoid(x)^beta, at a positive's label BCE(x, quality) * |quality - sigmoid(x)|^beta; beta >= 1.  forward leaves block
 *     partials and norm2 = [sum over images of max(n_pos, 1), sum of the positives' weights] on the device (the caller may
 *     average norm2 over ranks); finalize forms N = max(norm2[0], 1), S = max(norm2[1], 1), losses (3, L) = [lw_cls * qfl_l
 *     / N | lw_bbox * box_l / S | lw_dfl * dfl_l / S] per level and coef3 = [lw_cls / N, lw_bbox / S, lw_dfl / S]; backward
 *     takes grad_losses (3, L) and writes every element of dA and dR (w.r.t. the RAW outputs: the GIoU gradient through
 *     decode, expectation, softmax and scale, the DFL gradient through the log-softmax and the scale; padding columns and
 *     rows of invalid cells exactly 0) and dscale (L).  Fixed summation order, no float atomics.
 * cfg5_host = [QFL beta, giou eps, loss_weight_cls, loss_weight_bbox, loss_weight_dfl].  workspace:
 * brcnn_gfl_loss_workspace_bytes, shared by forward and finalize; backward takes one of the same size.  At most
 * BRCNN_MAX_LEVELS levels and BRCNN_MAX_IMAGES images.
 * -------------------------------------------------------------------------- */
int brcnn_gfl_decode_levels(const int64_t *const *topk_inds, const int *counts, const float *a, const float *r,
                            const int *layout4_host, const float *scales, int batch, int num_levels, const int *heights,
                            const int *widths, const int *strides, const float *base_anchors_host, int num_classes,
                            int reg_max, const float *max_shape, const float *scale_factor, float score_thr, float *boxes,
                            float *scores, int64_t *labels, uint8_t *valid, int32_t *n_valid, void *stream);
size_t brcnn_gfl_loss_workspace_bytes(int batch, int num_levels, const int *heights, const int *widths, int num_classes);
int brcnn_gfl_loss_forward(const float *a, const float *r, const int *layout4_host, const float *scales, int batch,
                           int num_levels, const int *heights, const int *widths, const int *strides,
                           const float *base_anchors_host, int reg_max, int num_classes, const int32_t *gt_inds,
                           const float *gts, const int64_t *gt_labels, const int *gt_offsets_host, const float *cfg5_host,
                           void *workspace, size_t workspace_bytes, float *norm2, void *stream);
int brcnn_gfl_loss_finalize(const void *workspace, size_t workspace_bytes, const float *norm2, int batch, int num_levels,
                            const int *heights, const int *widths, int num_classes, const float *cfg5_host, float *losses,
                            float *coef3, void *stream);
int brcnn_gfl_loss_backward(const float *a, const float *r, const int *layout4_host, const float *scales, int batch,
                            int num_levels, const int *heights, const int *widths, const int *strides,
                            const float *base_anchors_host, int reg_max, int num_classes, const int32_t *gt_inds,
                            const float *gts, const int64_t *gt_labels, const int *gt_offsets_host, const float *cfg5_host,
                            const float *grad_losses, const float *coef3, void *workspace, size_t workspace_bytes, float *da,
                            float *dr, float *dscale, void *stream);

/* ------------------------------------------------------------------------------
 * The VFNet head: VFNetHead with VarifocalLoss (models/dense_heads/vfnet_head.py, models/losses/varifocal_loss.py),
 * csrc/vfnet_head.hip.  ONE anchor per cell as for the ATSS head (base_anchors_host (L, 4)); only its centre is used: it is
 * the reference's point (x * s, y * s) + s * center_offset.  Row tensors over all levels, level-major rows, fp32, read in
 * place: A (rows, stride_a) with the C class logits at cls_off; R0 / R1 (rows, stride_r) with the 4 RAW distance logits
 * (l, t, r, b) at reg_off; D0 / D1 dense (rows, 4) distances in pixels.  scales / scales_refine: (L) floats ON THE DEVICE.
 * layout4_host = [stride_a, cls_off, stride_r, reg_off].
 *   brcnn_vfnet_star_offsets: D0 = exp(scale_l * raw0) * denoms_host[l], and offsets (rows, 18) in the row layout of
 *     brcnn_deform_im2col_nhwc_g ([2t] = dy, [2t + 1] = dx of tap t) in star_dcn_offset's order: q = (f0 * D0 + f1 * D0) /
 *     stride_l, the signed entries (taps 0..8 sample top-left, top, top-right, left, centre, right, bottom-left, bottom,
 *     bottom-right of the box), minus the base offset (ty - 1, tx - 1).  f0 = (float)(1 - gradient_mul), f1 =
 *     (float)gradient_mul.  The offsets are not clamped: the deformable kernels compare a sample coordinate with (-1, H) x
 *     (-1, W) in fp32 before any conversion to int, so a huge or non-finite offset samples zero.
 *   brcnn_vfnet_star_offsets_backward: dD0 (rows, 4) and d_offsets (rows, 18), each may be NULL (zeros) -> g = dD0 + f1 *
 *     (signed sums of the three entries per side / stride_l); d raw0 = g * D0 * scale_l written to every element of dr0
 *     (rows, stride_r), zeros outside the 4 columns; dscale (L) from block partials summed in a fixed order.
 *   brcnn_vfnet_refine / _backward: D1 = exp(scale_refine_l * raw1) * D0 with D0 a constant; d raw1 = dD1 * D1 *
 *     scale_refine_l, dscale (L) likewise.  workspace of both backward entries: brcnn_vfnet_rows_workspace_bytes.
 *   brcnn_vfnet_decode_levels: everything between the top-k and multiclass_nms (vfnet_head.py:463-595): D1 of the picked row,
 *     box = (px - l, py - t, px + r, py + b) clipped to max_shape, divided by scale_factor; score = sigmoid(cls_c), valid =
 *     score > score_thr; (level, pick, class) order.  The ranking score is brcnn_dense_score on A in place.
 *   brcnn_vfnet_loss_forward / _finalize / _backward: VFNetHead.loss (vfnet_head.py:315-461) on gt_inds (brcnn_atss_assign's
 *     convention; <= 0 and invalid cells are background: the reference passes no weight to loss_cls).  Per positive: target =
 *     bbox2distance(point, gt), gt' = distance2bbox(point, target), the boxes of D0 and D1, w_ini = max(aligned
 *     bbox_overlaps(box0, gt'), 1e-6), w_rf likewise (constants); sums of w_ini * (1 - giou0) and w_rf * (1 - giou1).  Class
 *     term over every (row, class): at a positive's label q = w_rf, q * BCE(x, q) (iou_weighted) or BCE(x, q); elsewhere
 *     alpha * sigmoid(x)^gamma * softplus(x); gamma >= 1.  forward leaves block partials and norm3 = [n_pos of the batch, sum
 *     w_ini, sum w_rf] on the device (the caller may average norm3 over ranks); finalize clamps each to >= 1 (N, S0, S1) and
 *     leaves losses (3) = [lw_cls * vfl / N, lw_bbox * box0 / S0, lw_rf * box1 / S1] and coef3 = [lw_cls / N, lw_bbox / S0,
 *     lw_rf / S1]; backward takes grad_losses (3) and writes every element of dA (rows, stride_a), dD0 and dD1 (rows, 4),
 *     padding columns and non-positive rows of dD0 / dD1 exactly 0.  Fixed summation order, no float atomics.
 * cfg7_host = [VFL alpha, VFL gamma, iou_weighted, giou eps, loss_weight_cls, loss_weight_bbox, loss_weight_bbox_refine].
 * At most BRCNN_MAX_LEVELS levels and BRCNN_MAX_IMAGES images.
 * -------------------------------------------------------------------------- */
size_t brcnn_vfnet_rows_workspace_bytes(int batch, int num_levels, const int *heights, const int *widths);
int brcnn_vfnet_star_offsets(const float *r0, int stride_r, int reg_off, const float *scales, int batch, int num_levels,
                             const int *heights, const int *widths, const int *strides, const float *denoms_host, float f0,
                             float f1, float *d0, float *offsets, void *stream);
int brcnn_vfnet_star_offsets_backward(const float *r0, int stride_r, int reg_off, const float *scales, int batch,
                                      int num_levels, const int *heights, const int *widths, const int *strides, float f1,
                                      const float *d0, const float *dd0, const float *doffsets, void *workspace,
                                      size_t workspace_bytes, float *dr0, float *dscale, void *stream);
int brcnn_vfnet_refine(const float *r1, int stride_r, int reg_off, const float *scales_refine, int batch, int num_levels,
                       const int *heights, const int *widths, const float *d0, float *d1, void *stream);
int brcnn_vfnet_refine_backward(const float *r1, int stride_r, int reg_off, const float *scales_refine, int batch,
                                int num_levels, const int *heights, const int *widths, const float *d1, const float *dd1,
                                void *workspace, size_t workspace_bytes, float *dr1, float *dscale, void *stream);
int brcnn_vfnet_decode_levels(const int64_t *const *topk_inds, const int *counts, const float *a, const float *r1,
                              const int *layout4_host, const float *scales_refine, int batch, int num_levels,
                              const int *heights, const int *widths, const int *strides, const float *base_anchors_host,
                              const float *d0, int num_classes, const float *max_shape, const float *scale_factor,
                              float score_thr, float *boxes, float *scores, int64_t *labels, uint8_t *valid, int32_t *n_valid,
                              void *stream);
size_t brcnn_vfnet_loss_workspace_bytes(int batch, int num_levels, const int *heights, const int *widths, int num_classes);
int brcnn_vfnet_loss_forward(const float *a, int stride_a, int cls_off, const float *d0, const float *d1, int batch,
                             int num_levels, const int *heights, const int *widths, const int *strides,
                             const float *base_anchors_host, int num_classes, const int32_t *gt_inds, const float *gts,
                             const int64_t *gt_labels, const int *gt_offsets_host, const float *cfg7_host, void *workspace,
                             size_t workspace_bytes, float *norm3, void *stream);
int brcnn_vfnet_loss_finalize(const void *workspace, size_t workspace_bytes, const float *norm3, int batch, int num_levels,
                              const int *heights, const int *widths, int num_classes, const float *cfg7_host, float *losses,
                              float *coef3, void *stream);
int brcnn_vfnet_loss_backward(const float *a, int stride_a, int cls_off, const float *d0, const float *d1, int batch,
                              int num_levels, const int *heights, const int *widths, const int *strides,
                              const float *base_anchors_host, int num_classes, const int32_t *gt_inds, const float *gts,
                              const int64_t *gt_labels, const int *gt_offsets_host, const float *cfg7_host,
                              const float *grad_losses, const float *coef3, float *da, float *dd0, float *dd1, void *stream);

/* ------------------------------------------------------------------------------
 * Optimizer step of the train loop: SGD with momentum and weight decay after clipping the global gradient
 * norm (torch.optim.SGD + mmcv OptimizerHook grad_clip; configs/_base_/schedules/schedule_1x.py:2-3,
 * configs/boosting_rcnn/boosting_rcnn_r50_pafpn_1x_utdac.py:130), as three stages over tables of tensors
 * passed by value (HOST arrays of device pointers; fp32 dense tensors):
 *   ctl3 = [ ||g||_2 / loss_scale, applied factor, skipped ]; with skip_nonfinite the step is skipped when the norm
 *   is not finite (GradScaler.step, the fp16 recipes); without it the update runs as clip_grad_norm_ + SGD would
 *   d = g * factor + wd * w;  buf = has_buf ? momentum * buf + d : d;  w -= lr * buf   (dampening 0, no nesterov)
 * brcnn_pack_conv_weights_batch: forward (Cout,KH,KW,Cin) and data-gradient (Cin,KH,KW,Cout, taps flipped)
 * operands of many conv weights in one launch per 64 tensors (dims_host: cout, cin, kh, kw each;
 * channels_last_host[i] != 0: master weight i is stored with torch.channels_last strides -- the layout the
 * weight-gradient kernel writes, so that its result IS the parameter's gradient without a layout copy; NULL =
 * all contiguous); with ctl3 the packing follows the step it belongs to (skipped together).
 * -------------------------------------------------------------------------- */
size_t brcnn_sgd_workspace_bytes(int num_tensors, const int64_t *numel_host);
int brcnn_sgd_step(float *const *params, const float *const *grads, float *const *bufs, const int64_t *numel_host,
                   const float *lr_host, const float *wd_host, const int *has_buf_host, int num_tensors,
                   float momentum, float max_norm, float inv_scale, int skip_nonfinite, void *workspace,
                   size_t workspace_bytes, float *ctl3, void *stream);
int brcnn_pack_conv_weights_batch(const float *const *weights, void *const *fwd, void *const *dgrad,
                                  const int *dims_host, const int *channels_last_host, int num, int dtype,
                                  const float *ctl3, void *stream);
/* The first FC of the box head (convfc_bbox_head.py:154-192 flattens the RoI features as (C, ph, pw)): master weight
 * (out_features, channels, positions) fp32 -> forward operand (out_features, positions, channels) in `dtype` -- the K
 * order of the NHWC RoI features -- and, when dgrad != NULL, the data-gradient operand (positions * channels,
 * out_features).  channels % 64 == 0, positions <= 255; ctl3 as above. */
int brcnn_pack_fc_weight_permuted(const float *weight, void *fwd, void *dgrad, int out_features, int channels,
                                  int positions, int dtype, const float *ctl3, void *stream);

/* ------------------------------------------------------------------------------
 * COCO bbox / proposal evaluation (evaluation.py: COCOeval.evaluateImg / accumulate) on the device.
 * Pairs are dense: pair = category * num_imgs + image (images in sorted-id order; one category when
 * categories are pooled).  gt_off / det_off (num_cats*num_imgs + 1) are the CSR offsets of the pair-major
 * ground-truth and detection tables: gt_box (G, 4) fp64 xywh, gt_area (G) fp64, gt_flags (G) bit 0 iscrowd,
 * bit 1 "id != 0"; det (D, 5) fp32 x1 y1 x2 y2 score, inside a pair in descending-score order and already
 * cut to the largest maxDet.  Every result is bit-equal to the host evaluator's.
 *
 * brcnn_coco_match: one launch for all pairs.  iou_thrs (num_thrs <= 16), area_rng (num_areas, 2) fp64 on
 * the device, num_thrs * num_areas <= 64; max_gt_per_pair (host-known) <= 1024.  Writes per detection and
 * area range the matched / ignored bits of every threshold (bit t) into dt_matched / dt_ignored
 * (D, num_areas) uint16, per ground truth its ignore bits (bit a) into gt_ignored (G), the number of
 * ground truths that count into num_gt (num_cats, num_areas), and for the later stages det_rank (D) and
 * det_key (D) = category << 32 | score bits flipped for an ascending sort.
 * brcnn_coco_order: stable LSD radix sort of det_key -> order (D) uint32, the detection indices by
 * (category, descending score), ties in table order; workspace from brcnn_coco_order_workspace_bytes.
 * brcnn_coco_accumulate: precision / scores (T, R, K, A, M) and recall (T, K, A, M) fp64 with the host's
 * conventions (-1: nothing to find; 0: nothing found); rec_thrs (num_recs <= 1024, ascending) fp64 and
 * max_dets (num_max_dets) int32 on the device. */
size_t brcnn_coco_order_workspace_bytes(int64_t num_dets);
int brcnn_coco_match(const double *gt_box, const double *gt_area, const uint8_t *gt_flags, const int32_t *gt_off,
                     const float *det, const int32_t *det_off, int num_cats, int num_imgs, const double *iou_thrs,
                     int num_thrs, const double *area_rng, int num_areas, int max_gt_per_pair, uint16_t *dt_matched,
                     uint16_t *dt_ignored, uint8_t *gt_ignored, int32_t *num_gt, int32_t *det_rank, uint64_t *det_key,
                     void *stream);
int brcnn_coco_order(const uint64_t *det_key, int64_t num_dets, int num_cats, uint32_t *order, void *workspace,
                     size_t workspace_bytes, void *stream);
int brcnn_coco_accumulate(const uint32_t *order, const int32_t *det_off, int num_imgs, const float *det,
                          const int32_t *det_rank, const uint16_t *dt_matched, const uint16_t *dt_ignored,
                          const int32_t *num_gt, const double *rec_thrs, const int32_t *max_dets, int num_thrs,
                          int num_recs, int num_cats, int num_areas, int num_max_dets, double *precision,
                          double *scores, double *recall, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BRCNN_HIP_H */
