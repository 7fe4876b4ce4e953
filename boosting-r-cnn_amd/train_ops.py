"""Train-step operators on libbrcnn_hip.so: whole-batch target assignment, RoI sampling and the
fused losses (C ABI: `brcnn_assign_max_iou`, `brcnn_rcnn_sample`, `brcnn_rpn_loss_*`,
`brcnn_boost_loss_*`, include/brcnn_hip.h).

The reference does this work per image and per level with chains of small torch ops and host
synchronisations (mmdet/core/bbox/assigners/max_iou_assigner.py:61-213,
core/bbox/samplers/random_sampler.py:32-82, models/dense_heads/atss_rpn_head.py:299-464,
models/roi_heads/prob_roi_head.py:23-154).  Here the batch is one unit: ground truth travels as
one flat (sum G, 4) tensor plus host-side offsets, every entry is one or two launches, and the
only device->host read of a train step is the (batch, 2) positive / negative counts the seeded
host `randperm` of the RandomSampler needs.

Device tensors only; a CPU tensor raises (there is no fallback).
"""
import ctypes
import math

import torch
import torch.distributed as dist
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import lib as _L
from .ops import _ptr, _require_gpu, _stream

MAX_IMAGES = 64


def _ints(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def _floats(vals):
    return (ctypes.c_float * len(vals))(*[float(v) for v in vals])


def flatten_gts(gt_bboxes, gt_labels=None):
    """list of (G_b, 4) [+ (G_b,)] -> flat (sum G, 4) fp32, (sum G,) int64 or None, host offsets"""
    offs = [0]
    for g in gt_bboxes:
        offs.append(offs[-1] + int(g.shape[0]))
    gts = torch.cat([g.reshape(-1, 4) for g in gt_bboxes], 0).float().contiguous()
    labels = None
    if gt_labels is not None:
        labels = torch.cat([l.reshape(-1) for l in gt_labels], 0).long().contiguous()
    return gts, labels, offs


def bbox_overlaps(bboxes1, bboxes2, mode='iou', is_aligned=False, eps=1e-6):
    """bbox_overlaps of two (n, 4|5) device box lists on the HIP kernel (values only, no autograd)"""
    _require_gpu(bboxes1, bboxes2)
    b1, b2 = bboxes1.detach().float().contiguous(), bboxes2.detach().float().contiguous()
    n1, n2 = b1.shape[0], b2.shape[0]
    out = torch.empty((n1,) if is_aligned else (n1, n2), dtype=torch.float32, device=b1.device)
    st = _L.load().brcnn_bbox_overlaps(_ptr(b1), b1.shape[1] if n1 else 4, n1, _ptr(b2), b2.shape[1] if n2 else 4, n2,
                                       {'iou': 0, 'iof': 1, 'giou': 2}[mode], int(bool(is_aligned)), float(eps), _ptr(out),
                                       _stream())
    _L.check(st, 'brcnn_bbox_overlaps')
    return out


def _neg_range(neg_iou_thr):
    if isinstance(neg_iou_thr, (tuple, list)):
        assert len(neg_iou_thr) == 2
        return float(neg_iou_thr[0]), float(neg_iou_thr[1])
    return 0.0, float(neg_iou_thr)


def assign_max_iou(boxes, gts, gt_offsets, pos_iou_thr, neg_iou_thr, min_pos_iou=0.0, match_low_quality=True,
                   num_boxes=None, batch=None, geom=None, valid_hw=None, img_hw=None, allowed_border=-1,
                   want_overlaps=False, want_counts=False):
    """MaxIoUAssigner for a whole batch.

    boxes: (n, 4|5) shared by every image (RPN anchors; `batch` given) or (B, n, 4|5) per image
    (proposals, `num_boxes` (B,) int32 real rows).  geom = (level_starts[L+1], level_widths[L], A)
    with valid_hw (B, L, 2) int32 / img_hw (B, 2) + allowed_border for the anchor validity flags.
    Returns gt_inds (B, n) int32 [, max_overlaps (B, n)] [, counts (B, 2) int32]."""
    _require_gpu(boxes, gts, num_boxes, valid_hw, img_hw)
    assert boxes.dtype == torch.float32 and boxes.is_contiguous()
    if boxes.dim() == 2:
        assert batch is not None
        B, n, bstride = int(batch), boxes.shape[0], 0
    else:
        B, n = boxes.shape[:2]
        bstride = boxes.stride(0)
    rstride = boxes.shape[-1]
    assert B <= MAX_IMAGES and len(gt_offsets) == B + 1
    dev = boxes.device
    total_gt = gt_offsets[-1]
    gt_inds = torch.empty((B, n), dtype=torch.int32, device=dev)
    mo = torch.empty((B, n), dtype=torch.float32, device=dev) if want_overlaps else None
    counts = torch.empty((B, 2), dtype=torch.int32, device=dev) if want_counts else None
    ws = torch.empty((max(total_gt, 1),), dtype=torch.int32, device=dev) if match_low_quality else None
    if geom is not None:
        starts, widths, A = geom
        L = len(widths)
        ls, lw = _ints(starts), _ints(widths)
    else:
        L, A, ls, lw = 0, 1, None, None
    lo, hi = _neg_range(neg_iou_thr)
    st = _L.load().brcnn_assign_max_iou(
        _ptr(boxes), bstride, rstride, _ptr(num_boxes), n, B, _ptr(gts) if total_gt else None, _ints(gt_offsets), L,
        ls, lw, int(A), _ptr(valid_hw), _ptr(img_hw), float(allowed_border), float(pos_iou_thr), lo, hi,
        float(min_pos_iou), int(bool(match_low_quality)), _ptr(ws), _ptr(gt_inds), _ptr(mo), _ptr(counts), _stream())
    _L.check(st, 'brcnn_assign_max_iou')
    out = (gt_inds,)
    if want_overlaps:
        out += (mo,)
    if want_counts:
        out += (counts,)
    return out if len(out) > 1 else gt_inds


def sample_counts(n_pos, n_neg, num, num_expected_pos, neg_pos_ub=-1):
    """rows the RandomSampler keeps for an image with n_pos / n_neg candidates
    (base_sampler.py:78-100): (sampled_pos, sampled_neg, expected_neg)"""
    spos = min(n_pos, num_expected_pos)
    eneg = num - spos
    if neg_pos_ub >= 0:
        eneg = min(eneg, int(neg_pos_ub * max(1, spos)))
    return spos, min(n_neg, eneg), eneg


def draw_sampler_perms(counts, num, num_expected_pos, neg_pos_ub=-1):
    """The host random stream of RandomSampler.random_choice (random_sampler.py:58,
    `torch.randperm(gallery.numel())[:num]`) for every image in the reference's order (positives
    then negatives, image by image), as one (B, num_expected_pos + num) int32 tensor, plus the
    (B+1) output row offsets.  `counts`: [(n_pos, n_neg)] host ints."""
    B = len(counts)
    perm = torch.zeros((B, num_expected_pos + num), dtype=torch.int32)
    rows = [0]
    for b, (n_pos, n_neg) in enumerate(counts):
        spos, sneg, eneg = sample_counts(n_pos, n_neg, num, num_expected_pos, neg_pos_ub)
        if n_pos > num_expected_pos:
            perm[b, :num_expected_pos] = torch.randperm(n_pos)[:num_expected_pos].to(torch.int32)
        if n_neg > eneg:
            perm[b, num_expected_pos:num_expected_pos + eneg] = torch.randperm(n_neg)[:eneg].to(torch.int32)
        rows.append(rows[-1] + spos + sneg)
    return perm, rows


def rcnn_sample(proposals, num_props, gt_inds, max_overlaps, gts, gt_labels, gt_offsets, perm, row_offsets, num,
                num_expected_pos, neg_pos_ub, num_classes, means, stds, add_gt_as_proposals=True,
                reg_decoded_bbox=False, want_ious=False, want_pos_flags=False, want_gt_flags=False):
    """Sampled RoIs + targets of the second stage for the whole batch in one launch.
    Returns dict(rois (N,5), labels (N) int64, bbox_targets (N,4), priors (N) [, ious (N)] [, pos_flags (N) int32]
    [, gt_flags (N) int32: the ground truths the sampler added, brcnn_rcnn_sample_gt])."""
    _require_gpu(proposals, num_props, gt_inds, max_overlaps, gts, gt_labels, perm)
    B, K, five = proposals.shape
    assert five == 5 and proposals.is_contiguous() and proposals.dtype == torch.float32
    assert gt_inds.shape == (B, K) and gt_inds.dtype == torch.int32 and gt_inds.is_contiguous()
    assert perm.dtype == torch.int32 and perm.shape == (B, num_expected_pos + num) and perm.is_contiguous()
    dev = proposals.device
    N = int(row_offsets[-1])
    gmax = max(gt_offsets[b + 1] - gt_offsets[b] for b in range(B))
    stride = K + gmax
    lists = torch.empty((B, 2, stride), dtype=torch.int32, device=dev)
    out = dict(rois=torch.empty((N, 5), dtype=torch.float32, device=dev),
               labels=torch.empty((N,), dtype=torch.int64, device=dev),
               bbox_targets=torch.empty((N, 4), dtype=torch.float32, device=dev),
               priors=torch.empty((N,), dtype=torch.float32, device=dev))
    if want_ious:
        assert max_overlaps is not None
        out['ious'] = torch.empty((N,), dtype=torch.float32, device=dev)
    if want_pos_flags:
        out['pos_flags'] = torch.empty((N,), dtype=torch.int32, device=dev)
    if want_gt_flags:
        out['gt_flags'] = torch.empty((N,), dtype=torch.int32, device=dev)
    if N == 0:
        return out
    total_gt = gt_offsets[-1]
    entry, more = ('brcnn_rcnn_sample_gt', (_ptr(out['gt_flags']),)) if want_gt_flags else ('brcnn_rcnn_sample', ())
    st = getattr(_L.load(), entry)(
        _ptr(proposals), _ptr(num_props), K, B, _ptr(gt_inds), _ptr(max_overlaps), _ptr(gts) if total_gt else None,
        _ptr(gt_labels) if total_gt else None, _ints(gt_offsets), int(bool(add_gt_as_proposals)), int(num),
        int(num_expected_pos), float(neg_pos_ub), _ptr(perm), _ints(row_offsets), int(num_classes),
        int(bool(reg_decoded_bbox)), _floats(means), _floats(stds), _ptr(lists), stride, _ptr(out['rois']),
        _ptr(out['labels']), _ptr(out['bbox_targets']), _ptr(out['priors']), _ptr(out.get('ious')),
        _ptr(out.get('pos_flags')), *more, _stream())
    _L.check(st, entry)
    return out


CASCADE_MAX_ROWS = 2048         # rows of one image brcnn_cascade_refine_train serves (the sampler's limit)


def cascade_refine_train(rois, labels, gt_flags, row_offsets, cls_score, bbox_pred, max_shape, num_classes, means, stds,
                         reg_class_agnostic=False, wh_ratio_clip=16 / 1000):
    """BBoxHead.refine_bboxes for the whole batch in one launch (brcnn_cascade_refine_train): the sampled rois (N,5) /
    labels (N) int64 / gt_flags (N) int32 of `rcnn_sample(..., want_gt_flags=True)` with their host row offsets, this
    stage's cls_score (N, C+1) and bbox_pred (N, 4 | 4C), max_shape (B,2).  Background rows are regressed by their
    arg-max class, the others by their label; added ground truths are dropped, order kept.
    Returns (props (B, Kout, 5) zero padded, num (B,) int32): the next stage's proposals, on the device."""
    _require_gpu(rois, labels, gt_flags, cls_score, bbox_pred, max_shape)
    from .ops import _rows_in_place
    B = len(row_offsets) - 1
    N, C = int(row_offsets[-1]), int(num_classes)
    assert 1 <= B <= MAX_IMAGES and rois.shape == (N, 5) and rois.dtype == torch.float32 and rois.is_contiguous()
    assert labels.shape == (N,) and labels.dtype == torch.int64 and labels.is_contiguous()
    assert gt_flags.shape == (N,) and gt_flags.dtype == torch.int32 and gt_flags.is_contiguous()
    assert cls_score.shape == (N, C + 1) and bbox_pred.shape == (N, 4 if reg_class_agnostic else 4 * C)
    assert max_shape.shape == (B, 2) and max_shape.dtype == torch.float32 and max_shape.is_contiguous()
    kout = max(1, max(row_offsets[b + 1] - row_offsets[b] for b in range(B)))
    cls_score, cs = _rows_in_place(cls_score.detach())
    bbox_pred, rs = _rows_in_place(bbox_pred.detach())
    props = torch.empty((B, kout, 5), dtype=torch.float32, device=rois.device)
    num = torch.empty((B,), dtype=torch.int32, device=rois.device)
    st = _L.load().brcnn_cascade_refine_train(_ptr(rois), _ptr(labels), _ptr(gt_flags), _ints(row_offsets), B, _ptr(cls_score),
                                              cs, _ptr(bbox_pred), rs, _ptr(max_shape), C, int(bool(reg_class_agnostic)),
                                              _floats(means), _floats(stds), float(wh_ratio_clip), kout, _ptr(props),
                                              _ptr(num), _stream())
    _L.check(st, 'brcnn_cascade_refine_train')
    return props, num


# ----------------------------------------------------------------------------- RPN loss
class RPNLossMeta:
    """host-side description of one fused RPN loss call (shapes, anchors, loss configuration)"""

    def __init__(self, batch, sizes, strides, base_anchors, num_anchors, gt_offsets, focal_gamma, focal_alpha,
                 pos_weight, iou_gamma, means, stds, wh_ratio_clip, with_aug, lw_cls, lw_bbox, lw_aug, lw_iou,
                 cls_mode=0, reg_mode=0):
        """cls_mode: 0 FocalLoss, 1 / 2 VarifocalLoss (iou_weighted / not; focal_gamma / focal_alpha are then
        the varifocal ones); reg_mode: 0 decoded boxes with IoULoss('log') [+ MSE aug], 1 CIoULoss on the raw
        deltas (reg_decoded_bbox=False)"""
        self.batch, self.sizes, self.A = int(batch), [tuple(s) for s in sizes], int(num_anchors)
        self.L = len(self.sizes)
        self.hs, self.ws = _ints([h for h, _ in self.sizes]), _ints([w for _, w in self.sizes])
        self.sw = _ints([s if isinstance(s, int) else s[0] for s in strides])
        self.sh = _ints([s if isinstance(s, int) else s[1] for s in strides])
        self.base = base_anchors                      # list of (A,4) device tensors (kept alive here)
        self.base_ptrs = (ctypes.c_void_p * self.L)(*[b.data_ptr() for b in base_anchors])
        self.gt_offsets = _ints(gt_offsets)
        self.total_gt = int(gt_offsets[-1])
        self.cfg = _floats([focal_gamma, focal_alpha, pos_weight, iou_gamma] + list(means) + list(stds) +
                           [abs(math.log(wh_ratio_clip)), 1.0 if with_aug else 0.0, lw_cls, lw_bbox, lw_aug, lw_iou,
                            float(cls_mode), float(reg_mode)])
        self.rows = sum(self.batch * h * w for h, w in self.sizes)
        self.anchors_per_image = sum(h * w for h, w in self.sizes) * self.A


def _reduce_mean_(t):
    """mean over ranks in place (mmdet/core/utils/dist_utils.py:67-73); identity when not distributed"""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(t.div_(dist.get_world_size()), op=dist.ReduceOp.SUM)
    return t


class RPNLossFunction(Function):
    """losses3 = [loss_rpn_cls, loss_rpn_bbox, loss_rpn_iou] (summed over the pyramid levels) from the
    fused head output y (rows, ystride) of all levels and the per-level Scale parameters."""

    @staticmethod
    def forward(ctx, y, scales, gt_inds, gts, meta):
        _require_gpu(y, scales, gt_inds, gts)
        assert y.dim() == 2 and y.dtype == torch.float32 and y.is_contiguous() and y.shape[0] == meta.rows
        assert gt_inds.dtype == torch.int32 and gt_inds.shape == (meta.batch, meta.anchors_per_image)
        lib = _L.load()
        dev = y.device
        sc = scales.detach().float().contiguous()
        nb = lib.brcnn_rpn_loss_workspace_bytes(meta.batch, meta.L, meta.hs, meta.ws, meta.A)
        ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=dev)
        small = torch.empty((meta.L * 6 + 2,), dtype=torch.float32, device=dev)
        sums, coef = small[:meta.L * 6], small[meta.L * 6:]
        totals = torch.empty((2,), dtype=torch.float32, device=dev)
        losses3 = torch.empty((3,), dtype=torch.float32, device=dev)
        per_level = torch.empty((3 * meta.L,), dtype=torch.float32, device=dev)
        gp = _ptr(gts) if meta.total_gt else None
        st = lib.brcnn_rpn_loss_forward(_ptr(y), y.shape[1], meta.batch, meta.L, meta.hs, meta.ws, meta.sw, meta.sh,
                                        meta.base_ptrs, meta.A, _ptr(sc), _ptr(gt_inds), gp, meta.gt_offsets, meta.cfg,
                                        _ptr(ws), nb, _ptr(sums), _ptr(totals), _stream())
        _L.check(st, 'brcnn_rpn_loss_forward')
        _reduce_mean_(totals)           # ONE collective for both normalisers (num_pos, sum iou_target)
        st = lib.brcnn_rpn_loss_finalize(_ptr(sums), _ptr(totals), meta.L, meta.cfg, _ptr(losses3), _ptr(per_level),
                                         _ptr(coef), _stream())
        _L.check(st, 'brcnn_rpn_loss_finalize')
        ctx.save_for_backward(y, sc, gt_inds, gts, coef)
        ctx.meta = meta
        ctx.scales_dtype = scales.dtype
        per_level = per_level.view(3, meta.L)
        ctx.mark_non_differentiable(per_level, totals)
        return losses3, per_level, totals

    @staticmethod
    @once_differentiable
    def backward(ctx, g3, _gl, _gt):
        y, sc, gt_inds, gts, coef = ctx.saved_tensors
        meta = ctx.meta
        lib = _L.load()
        nb = lib.brcnn_rpn_loss_workspace_bytes(meta.batch, meta.L, meta.hs, meta.ws, meta.A)
        ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=y.device)
        dy = torch.empty_like(y)
        dsc = torch.empty((meta.L,), dtype=torch.float32, device=y.device)
        g3 = g3.float().contiguous()
        gp = _ptr(gts) if meta.total_gt else None
        st = lib.brcnn_rpn_loss_backward(_ptr(y), y.shape[1], meta.batch, meta.L, meta.hs, meta.ws, meta.sw, meta.sh,
                                         meta.base_ptrs, meta.A, _ptr(sc), _ptr(gt_inds), gp, meta.gt_offsets, meta.cfg,
                                         _ptr(g3), _ptr(coef), _ptr(ws), nb, _ptr(dy), _ptr(dsc), _stream())
        _L.check(st, 'brcnn_rpn_loss_backward')
        return dy, dsc.to(ctx.scales_dtype), None, None, None


def rpn_loss(y, scales, gt_inds, gts, meta):
    """(losses3 (3,), per_level (3, L), totals (2,) = rank means of [num_pos, sum iou_target])"""
    return RPNLossFunction.apply(y, scales, gt_inds, gts, meta)


# ----------------------------------------------------------------------------- sampled RPN loss (Faster R-CNN baseline)
class RPNSampledMeta:
    """host-side description of one sampled RPN loss call (RPNHead: RandomSampler over the assigned anchors)"""

    def __init__(self, batch, sizes, strides, base_anchors, num_anchors, gt_offsets, num, num_expected_pos, neg_pos_ub,
                 pos_weight, smooth_l1_beta, means, stds, lw_cls, lw_bbox):
        self.batch, self.sizes, self.A = int(batch), [tuple(s) for s in sizes], int(num_anchors)
        self.L = len(self.sizes)
        self.hs, self.ws = _ints([h for h, _ in self.sizes]), _ints([w for _, w in self.sizes])
        self.sw = _ints([s if isinstance(s, int) else s[0] for s in strides])
        self.sh = _ints([s if isinstance(s, int) else s[1] for s in strides])
        self.base = base_anchors                      # list of (A,4) device tensors (kept alive here)
        self.base_ptrs = (ctypes.c_void_p * self.L)(*[b.data_ptr() for b in base_anchors])
        self.gt_offsets = _ints(gt_offsets)
        self.total_gt = int(gt_offsets[-1])
        self.num, self.num_pos, self.neg_pos_ub = int(num), int(num_expected_pos), float(neg_pos_ub)
        self.head = [float(pos_weight), float(smooth_l1_beta)] + [float(v) for v in means] + [float(v) for v in stds] + \
            [float(lw_cls), float(lw_bbox)]
        self.rows = sum(self.batch * h * w for h, w in self.sizes)
        self.anchors_per_image = sum(h * w for h, w in self.sizes) * self.A

    def cfg(self, num_total_samples):
        return _floats(self.head + [float(num_total_samples)])


def rpn_num_total_samples(counts, num, num_expected_pos, neg_pos_ub=-1):
    """AnchorHead.get_targets' normaliser (anchor_head.py:354-355, :469-470): per image max(#drawn positives, 1) +
    max(#drawn negatives, 1), from the host-side candidate counts"""
    total = 0
    for n_pos, n_neg in counts:
        spos, sneg, _ = sample_counts(n_pos, n_neg, num, num_expected_pos, neg_pos_ub)
        total += max(spos, 1) + max(sneg, 1)
    return total


def rpn_sampled_draw(gt_inds, perm, meta):
    """drawn (B, num) int32: per image the drawn positives, then the drawn negatives (flat anchor indices), -1 after;
    also returns the workspace the loss call goes on with"""
    _require_gpu(gt_inds, perm)
    assert gt_inds.dtype == torch.int32 and gt_inds.shape == (meta.batch, meta.anchors_per_image) and gt_inds.is_contiguous()
    assert perm.dtype == torch.int32 and perm.shape == (meta.batch, meta.num_pos + meta.num) and perm.is_contiguous()
    lib = _L.load()
    nb = lib.brcnn_rpn_sampled_workspace_bytes(meta.batch, meta.anchors_per_image, meta.num)
    ws = torch.empty((nb + 3) // 4, dtype=torch.int32, device=gt_inds.device)
    drawn = torch.empty((meta.batch, meta.num), dtype=torch.int32, device=gt_inds.device)
    st = lib.brcnn_rpn_sampled_draw(_ptr(gt_inds), meta.anchors_per_image, meta.batch, meta.num, meta.num_pos,
                                    meta.neg_pos_ub, _ptr(perm), _ptr(ws), nb, _ptr(drawn), _stream())
    _L.check(st, 'brcnn_rpn_sampled_draw')
    return drawn, ws


class RPNSampledLossFunction(Function):
    """losses2 = [loss_rpn_cls, loss_rpn_bbox] over the drawn anchors, from the fused head output y (rows, ystride)"""

    @staticmethod
    def forward(ctx, y, gt_inds, gts, drawn, ws, meta, num_total_samples):
        _require_gpu(y, gt_inds, gts, drawn)
        assert y.dim() == 2 and y.dtype == torch.float32 and y.is_contiguous() and y.shape[0] == meta.rows
        assert y.shape[1] >= 5 * meta.A
        assert drawn.dtype == torch.int32 and drawn.shape == (meta.batch, meta.num) and drawn.is_contiguous()
        lib = _L.load()
        cfg = meta.cfg(num_total_samples)
        nb = lib.brcnn_rpn_sampled_workspace_bytes(meta.batch, meta.anchors_per_image, meta.num)
        if ws is None:
            ws = torch.empty((nb + 3) // 4, dtype=torch.int32, device=y.device)
        out = torch.empty((4,), dtype=torch.float32, device=y.device)
        losses2, coef = out[:2], out[2:]
        gp = _ptr(gts) if meta.total_gt else None
        st = lib.brcnn_rpn_sampled_loss_forward(_ptr(y), y.shape[1], meta.batch, meta.L, meta.hs, meta.ws, meta.sw, meta.sh,
                                                meta.base_ptrs, meta.A, _ptr(gt_inds), gp, meta.gt_offsets, _ptr(drawn),
                                                meta.num, cfg, _ptr(ws), nb, _stream())
        _L.check(st, 'brcnn_rpn_sampled_loss_forward')
        st = lib.brcnn_rpn_sampled_loss_finalize(_ptr(ws), meta.batch, meta.anchors_per_image, meta.num, cfg,
                                                 _ptr(losses2), _ptr(coef), _stream())
        _L.check(st, 'brcnn_rpn_sampled_loss_finalize')
        ctx.save_for_backward(y, gt_inds, gts, drawn, coef)
        ctx.meta, ctx.cfg = meta, cfg
        return losses2

    @staticmethod
    @once_differentiable
    def backward(ctx, g2):
        y, gt_inds, gts, drawn, coef = ctx.saved_tensors
        meta = ctx.meta
        dy = torch.empty_like(y)
        g2 = g2.float().contiguous()
        gp = _ptr(gts) if meta.total_gt else None
        st = _L.load().brcnn_rpn_sampled_loss_backward(
            _ptr(y), y.shape[1], meta.batch, meta.L, meta.hs, meta.ws, meta.sw, meta.sh, meta.base_ptrs, meta.A,
            _ptr(gt_inds), gp, meta.gt_offsets, _ptr(drawn), meta.num, ctx.cfg, _ptr(g2), _ptr(coef), _ptr(dy), _stream())
        _L.check(st, 'brcnn_rpn_sampled_loss_backward')
        return dy, None, None, None, None, None, None


def rpn_sampled_loss(y, gt_inds, gts, drawn, meta, num_total_samples, workspace=None):
    """(2,) tensor [loss_rpn_cls, loss_rpn_bbox], differentiable w.r.t. y"""
    return RPNSampledLossFunction.apply(y, gt_inds, gts, drawn, workspace, meta, num_total_samples)


# ----------------------------------------------------------------------------- dense head loss (RetinaNet baseline)
class DenseLossMeta:
    """host-side description of one dense-head loss call (RetinaHead: focal loss over every anchor, no sampler)"""

    def __init__(self, batch, sizes, strides, base_anchors, num_anchors, num_classes, gt_offsets, focal_gamma, focal_alpha,
                 pos_weight, smooth_l1_beta, means, stds, lw_cls, lw_bbox):
        self.batch, self.sizes, self.A, self.C = int(batch), [tuple(s) for s in sizes], int(num_anchors), int(num_classes)
        self.L = len(self.sizes)
        self.hs, self.ws = _ints([h for h, _ in self.sizes]), _ints([w for _, w in self.sizes])
        self.sw = _ints([s if isinstance(s, int) else s[0] for s in strides])
        self.sh = _ints([s if isinstance(s, int) else s[1] for s in strides])
        self.base = base_anchors                      # list of (A,4) device tensors (kept alive here)
        self.base_ptrs = (ctypes.c_void_p * self.L)(*[b.data_ptr() for b in base_anchors])
        self.gt_offsets = _ints(gt_offsets)
        self.total_gt = int(gt_offsets[-1])
        self.cfg = _floats([focal_gamma, focal_alpha, pos_weight, smooth_l1_beta] + list(means) + list(stds) +
                           [lw_cls, lw_bbox])
        self.rows = sum(self.batch * h * w for h, w in self.sizes)
        self.anchors_per_image = sum(h * w for h, w in self.sizes) * self.A


class DenseLossFunction(Function):
    """losses (2, L) = [loss_cls per level, loss_bbox per level] from the head outputs of all levels: cls (rows, >= A*C),
    reg (rows, >= 4A), level-major rows"""

    @staticmethod
    def forward(ctx, cls, reg, gt_inds, gts, gt_labels, meta):
        _require_gpu(cls, reg, gt_inds, gts, gt_labels)
        for t, need in ((cls, meta.A * meta.C), (reg, 4 * meta.A)):
            assert t.dim() == 2 and t.dtype == torch.float32 and t.is_contiguous() and t.shape[0] == meta.rows
            assert t.shape[1] >= need
        assert gt_inds.dtype == torch.int32 and gt_inds.shape == (meta.batch, meta.anchors_per_image) and gt_inds.is_contiguous()
        if meta.total_gt:
            assert gts.dtype == torch.float32 and gts.shape == (meta.total_gt, 4) and gts.is_contiguous()
            assert gt_labels.dtype == torch.int64 and gt_labels.shape == (meta.total_gt,) and gt_labels.is_contiguous()
        lib = _L.load()
        dev = cls.device
        nb = lib.brcnn_dense_loss_workspace_bytes(meta.batch, meta.L, meta.hs, meta.ws, meta.A, meta.C)
        ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=dev)
        out = torch.empty((2 * meta.L + 3,), dtype=torch.float32, device=dev)
        losses, coef = out[:2 * meta.L], out[2 * meta.L:]
        gp, lp = (_ptr(gts), _ptr(gt_labels)) if meta.total_gt else (None, None)
        st = lib.brcnn_dense_loss_forward(_ptr(cls), cls.shape[1], _ptr(reg), reg.shape[1], meta.batch, meta.L, meta.hs,
                                          meta.ws, meta.sw, meta.sh, meta.base_ptrs, meta.A, meta.C, _ptr(gt_inds), gp, lp,
                                          meta.gt_offsets, meta.cfg, _ptr(ws), nb, _stream())
        _L.check(st, 'brcnn_dense_loss_forward')
        st = lib.brcnn_dense_loss_finalize(_ptr(ws), nb, meta.batch, meta.L, meta.hs, meta.ws, meta.A, meta.C, meta.cfg,
                                           _ptr(losses), _ptr(coef), _stream())
        _L.check(st, 'brcnn_dense_loss_finalize')
        ctx.save_for_backward(cls, reg, gt_inds, gts, gt_labels, coef)
        ctx.meta = meta
        ctx.mark_non_differentiable(coef)
        return losses.view(2, meta.L), coef

    @staticmethod
    @once_differentiable
    def backward(ctx, g2, _gc):
        cls, reg, gt_inds, gts, gt_labels, coef = ctx.saved_tensors
        meta = ctx.meta
        dcls, dreg = torch.empty_like(cls), torch.empty_like(reg)
        g2 = g2.float().contiguous()
        gp, lp = (_ptr(gts), _ptr(gt_labels)) if meta.total_gt else (None, None)
        st = _L.load().brcnn_dense_loss_backward(
            _ptr(cls), cls.shape[1], _ptr(reg), reg.shape[1], meta.batch, meta.L, meta.hs, meta.ws, meta.sw, meta.sh,
            meta.base_ptrs, meta.A, meta.C, _ptr(gt_inds), gp, lp, meta.gt_offsets, meta.cfg, _ptr(g2), _ptr(coef),
            _ptr(dcls), _ptr(dreg), _stream())
        _L.check(st, 'brcnn_dense_loss_backward')
        return dcls, dreg, None, None, None, None


def dense_loss(cls, reg, gt_inds, gts, gt_labels, meta):
    """(losses (2, L), coef3 = [loss_weight_cls / num_total_pos, loss_weight_bbox / num_total_pos, num_total_pos]);
    the losses are differentiable w.r.t. cls and reg"""
    return DenseLossFunction.apply(cls, reg, gt_inds, gts, gt_labels, meta)


# ----------------------------------------------------------------------------- FCOS head: targets and loss
class CenternessLossMeta:
    """host-side description of one loss call of a centerness head (FCOS, ATSS): the pyramid, the ground-truth offsets and
    the loss settings.  A head names its entry points (`brcnn_<kind>_loss_*`), the arguments it adds after the strides
    (`extra`) and whether the losses come back per level ((3, L)) or summed ((3,))."""

    kind, per_level, extra = None, False, ()

    def __init__(self, batch, sizes, strides, num_classes, gt_offsets, cfg):
        self.batch, self.sizes, self.C = int(batch), [tuple(int(v) for v in s) for s in sizes], int(num_classes)
        self.L = len(self.sizes)
        if self.batch > MAX_IMAGES:
            raise ValueError(f'{self.kind} loss: batch {self.batch} exceeds {MAX_IMAGES} images per call')
        self.hs, self.ws = _ints([h for h, _ in self.sizes]), _ints([w for _, w in self.sizes])
        self.strides = _ints([s if isinstance(s, int) else s[0] for s in strides])
        self.gt_offsets = _ints(gt_offsets)
        self.total_gt = int(gt_offsets[-1])
        self.cfg = _floats(cfg)
        self.rows = sum(self.batch * h * w for h, w in self.sizes)
        self.per_image = sum(h * w for h, w in self.sizes)        # points resp. anchors of one image

    def entry(self, lib, what):
        return getattr(lib, f'brcnn_{self.kind}_loss_{what}')

    def workspace(self, lib, device):
        nb = self.entry(lib, 'workspace_bytes')(self.batch, self.L, self.hs, self.ws, self.C)
        return torch.empty((nb + 3) // 4, dtype=torch.float32, device=device), nb


class FcosLossMeta(CenternessLossMeta):
    """the FCOS loss call (include/brcnn_hip.h: cfg7_host)"""

    kind = 'fcos'

    def __init__(self, batch, sizes, strides, num_classes, gt_offsets, focal_gamma, focal_alpha, eps_overlap, eps_loss,
                 lw_cls, lw_bbox, lw_ctr):
        super().__init__(batch, sizes, strides, num_classes, gt_offsets,
                         [focal_gamma, focal_alpha, eps_overlap, eps_loss, lw_cls, lw_bbox, lw_ctr])


def fcos_assign(gts, gt_offsets, batch, sizes, strides, regress_ranges, center_sampling=False, center_sample_radius=1.5):
    """FCOSHead._get_target_single for the whole batch (brcnn_fcos_assign): gts (sum G, 4) fp32 packed, host offsets ->
    gt_inds (batch, points per image) int32, the image-local index of the ground truth each point takes, -1 background"""
    _require_gpu(gts)
    L = len(sizes)
    assert len(strides) == L and len(regress_ranges) == L and len(gt_offsets) == batch + 1
    total = int(gt_offsets[-1])
    if total:
        assert gts.dtype == torch.float32 and gts.shape == (total, 4) and gts.is_contiguous()
    n = sum(int(h) * int(w) for h, w in sizes)
    out = torch.empty((batch, n), dtype=torch.int32, device=gts.device)
    ranges = _floats([v for lo_hi in regress_ranges for v in lo_hi])
    st = _L.load().brcnn_fcos_assign(_ptr(gts) if total else None, _ints(gt_offsets), int(batch), L,
                                     _ints([h for h, _ in sizes]), _ints([w for _, w in sizes]), _ints(strides), ranges,
                                     int(bool(center_sampling)), float(center_sample_radius), _ptr(out), _stream())
    _L.check(st, 'brcnn_fcos_assign')
    return out


def _centerness_loss_args(a, r, layout, scales, gt_inds, gts, gt_labels, meta):
    """the arguments the forward and backward entry points of a centerness head share"""
    gp, lp = (_ptr(gts), _ptr(gt_labels)) if meta.total_gt else (None, None)
    return (_ptr(a), _ptr(r), layout.arr, _ptr(scales), meta.batch, meta.L, meta.hs, meta.ws, meta.strides, *meta.extra,
            meta.C, _ptr(gt_inds), gp, lp, meta.gt_offsets, meta.cfg)


def _centerness_loss_partials(a, r, layout, scales, gt_inds, gts, gt_labels, meta):
    """brcnn_<kind>_loss_forward: (workspace holding the block partials, norm2 = [n_pos, sum of centerness targets]) on the
    device; the caller may average norm2 over ranks before the finalize step"""
    _require_gpu(a, r, scales, gt_inds, gts, gt_labels)
    assert layout.rows == meta.rows and layout.C == meta.C
    assert scales.dtype == torch.float32 and scales.shape == (meta.L,) and scales.is_contiguous()
    assert gt_inds.dtype == torch.int32 and gt_inds.shape == (meta.batch, meta.per_image) and gt_inds.is_contiguous()
    if meta.total_gt:
        assert gts.dtype == torch.float32 and gts.shape == (meta.total_gt, 4) and gts.is_contiguous()
        assert gt_labels.dtype == torch.int64 and gt_labels.shape == (meta.total_gt,) and gt_labels.is_contiguous()
    lib = _L.load()
    ws, nb = meta.workspace(lib, a.device)
    norm2 = torch.empty((2,), dtype=torch.float32, device=a.device)
    st = meta.entry(lib, 'forward')(*_centerness_loss_args(a, r, layout, scales, gt_inds, gts, gt_labels, meta), _ptr(ws), nb,
                                    _ptr(norm2), _stream())
    _L.check(st, f'brcnn_{meta.kind}_loss_forward')
    return ws, norm2


def _centerness_loss_finalize(ws, norm2, meta):
    """brcnn_<kind>_loss_finalize: (losses (3,) or (3, L), coef3 = [lw_cls / N, lw_bbox / S, lw_ctr / N]), one allocation"""
    n = 3 * meta.L if meta.per_level else 3
    out = torch.empty((n + 3,), dtype=torch.float32, device=ws.device)
    st = meta.entry(_L.load(), 'finalize')(_ptr(ws), ws.numel() * 4, _ptr(norm2), meta.batch, meta.L, meta.hs, meta.ws,
                                           meta.C, meta.cfg, _ptr(out[:n]), _ptr(out[n:]), _stream())
    _L.check(st, f'brcnn_{meta.kind}_loss_finalize')
    return (out[:n].view(3, meta.L) if meta.per_level else out[:n]), out[n:]


def fcos_loss_partials(a, r, layout, scales, gt_inds, gts, gt_labels, meta):
    """brcnn_fcos_loss_forward, see `_centerness_loss_partials`"""
    return _centerness_loss_partials(a, r, layout, scales, gt_inds, gts, gt_labels, meta)


def fcos_loss_finalize(ws, norm2, meta):
    """brcnn_fcos_loss_finalize: out6 = [loss_cls, loss_bbox, loss_centerness | lw_cls / N, lw_bbox / S, lw_ctr / N]"""
    return _centerness_loss_finalize(ws, norm2, meta)


class CenternessLossFunction(Function):
    """losses = [loss_cls, loss_bbox, loss_centerness] ((3,) for FCOS, (3, L) per level for ATSS) from the head outputs of
    all levels, differentiable w.r.t. A, R (the raw outputs) and the per-level scales; `meta` selects the head's kernels"""

    @staticmethod
    def forward(ctx, a, r, scales, gt_inds, gts, gt_labels, layout, meta, norm_hook):
        scales = scales.detach().float().contiguous()
        ws, norm2 = _centerness_loss_partials(a, r, layout, scales, gt_inds, gts, gt_labels, meta)
        if norm_hook is not None:
            norm_hook(norm2)
        losses, coef = _centerness_loss_finalize(ws, norm2, meta)
        ctx.save_for_backward(a, r, scales, gt_inds, gts, gt_labels, coef)
        ctx.layout, ctx.meta = layout, meta
        ctx.mark_non_differentiable(coef, norm2)
        return losses, coef, norm2

    @staticmethod
    @once_differentiable
    def backward(ctx, g3, _gc, _gn):
        a, r, scales, gt_inds, gts, gt_labels, coef = ctx.saved_tensors
        meta, layout = ctx.meta, ctx.layout
        da, dr = torch.empty_like(a), torch.empty_like(r)
        dscale = torch.empty_like(scales)
        g3 = g3.float().contiguous()
        lib = _L.load()
        ws, nb = meta.workspace(lib, a.device)
        st = meta.entry(lib, 'backward')(*_centerness_loss_args(a, r, layout, scales, gt_inds, gts, gt_labels, meta), _ptr(g3),
                                         _ptr(coef), _ptr(ws), nb, _ptr(da), _ptr(dr), _ptr(dscale), _stream())
        _L.check(st, f'brcnn_{meta.kind}_loss_backward')
        return da, dr, dscale, None, None, None, None, None, None


def fcos_loss(a, r, scales, gt_inds, gts, gt_labels, layout, meta, norm_hook=None):
    """(losses (3,), coef3, norm2); `norm_hook(norm2)` may change norm2 in place between the sums and the division (the
    mean over ranks)"""
    return CenternessLossFunction.apply(a, r, scales, gt_inds, gts, gt_labels, layout, meta, norm_hook)




# ----------------------------------------------------------------------------- ATSS head: assignment and loss
ATSS_MAX_TOPK = 16


def atss_assign(gts, gt_offsets, batch, sizes, strides, base_anchors, topk, valid_hw=None, want_overlaps=False):
    """ATSSAssigner.assign for the whole batch (brcnn_atss_assign): gts (sum G, 4) fp32 packed, host offsets, base_anchors
    from `ops.atss_base_anchors`, valid_hw (batch, L, 2) int32 or None -> gt_inds (batch, anchors per image) int32: k > 0
    positive for ground truth k - 1 of the image, 0 negative, -1 invalid cell [, max_overlaps]"""
    _require_gpu(gts, valid_hw)
    L = len(sizes)
    if not 0 < int(topk) <= ATSS_MAX_TOPK:
        raise ValueError(f'atss_assign: topk={topk} outside (0, {ATSS_MAX_TOPK}]')
    if L > 8:
        raise ValueError(f'atss_assign: {L} pyramid levels, at most 8 are supported')
    if batch > MAX_IMAGES:
        raise ValueError(f'atss_assign: batch {batch} exceeds {MAX_IMAGES} images per call')
    assert len(strides) == L and len(base_anchors) == 4 * L and len(gt_offsets) == batch + 1
    total = int(gt_offsets[-1])
    if total:
        assert gts.dtype == torch.float32 and gts.shape == (total, 4) and gts.is_contiguous()
    if valid_hw is not None:
        assert valid_hw.dtype == torch.int32 and valid_hw.shape == (batch, L, 2) and valid_hw.is_contiguous()
    n = sum(int(h) * int(w) for h, w in sizes)
    dev = gts.device
    out = torch.empty((batch, n), dtype=torch.int32, device=dev)
    ov = torch.empty((batch, n), dtype=torch.float32, device=dev) if want_overlaps else None
    ws = torch.empty((batch, n), dtype=torch.int64, device=dev)
    st = _L.load().brcnn_atss_assign(_ptr(gts) if total else None, _ints(gt_offsets), int(batch), L,
                                     _ints([h for h, _ in sizes]), _ints([w for _, w in sizes]), _ints(strides), base_anchors,
                                     _ptr(valid_hw), int(topk), _ptr(ws), ws.numel() * 8, _ptr(out), _ptr(ov), _stream())
    _L.check(st, 'brcnn_atss_assign')
    return (out, ov) if want_overlaps else out


class AtssLossMeta(CenternessLossMeta):
    """the ATSS loss call: adds the base anchors of the pyramid; per-level losses (include/brcnn_hip.h: cfg15_host)"""

    kind, per_level = 'atss', True

    def __init__(self, batch, sizes, strides, base_anchors, num_classes, gt_offsets, focal_gamma, focal_alpha, eps, lw_cls,
                 lw_bbox, lw_ctr, means, stds, wh_ratio_clip=16 / 1000):
        super().__init__(batch, sizes, strides, num_classes, gt_offsets,
                         [focal_gamma, focal_alpha, eps, lw_cls, lw_bbox, lw_ctr] + list(means) + list(stds) +
                         [abs(math.log(wh_ratio_clip))])
        assert len(base_anchors) == 4 * self.L
        self.base = base_anchors
        self.extra = (base_anchors,)


def atss_loss(a, r, scales, gt_inds, gts, gt_labels, layout, meta, norm_hook=None):
    """(losses (3, L), coef3, norm2); `norm_hook(norm2)` may change norm2 in place between the sums and the division (the
    mean over ranks)"""
    return CenternessLossFunction.apply(a, r, scales, gt_inds, gts, gt_labels, layout, meta, norm_hook)




# ----------------------------------------------------------------------------- GFL head: loss
class GflLossMeta(CenternessLossMeta):
    """the GFL loss call: the base anchors of the pyramid and reg_max; per-level losses [loss_cls, loss_bbox, loss_dfl]
    (include/brcnn_hip.h: cfg5_host).  The assignment is `atss_assign`; `layout` is an `ops.GflLayout`."""

    kind, per_level = 'gfl', True

    def __init__(self, batch, sizes, strides, base_anchors, reg_max, num_classes, gt_offsets, beta, eps, lw_cls, lw_bbox,
                 lw_dfl):
        super().__init__(batch, sizes, strides, num_classes, gt_offsets, [beta, eps, lw_cls, lw_bbox, lw_dfl])
        assert len(base_anchors) == 4 * self.L
        self.base, self.reg_max = base_anchors, int(reg_max)
        self.extra = (base_anchors, self.reg_max)


def gfl_loss(a, r, scales, gt_inds, gts, gt_labels, layout, meta, norm_hook=None):
    """(losses (3, L), coef3, norm2 = [sum of max(n_pos, 1), sum of the positives' weights]); `norm_hook(norm2)` may change
    norm2 in place between the sums and the division (the mean over ranks)"""
    assert layout.reg_max == meta.reg_max
    return CenternessLossFunction.apply(a, r, scales, gt_inds, gts, gt_labels, layout, meta, norm_hook)


# ----------------------------------------------------------------------------- VFNet head: distances, star offsets, loss
def _vfnet_rows_workspace(lib, batch, sizes, device):
    L = len(sizes)
    hs, ws = _ints([h for h, _ in sizes]), _ints([w for _, w in sizes])
    nb = lib.brcnn_vfnet_rows_workspace_bytes(int(batch), L, hs, ws)
    return torch.empty((nb + 3) // 4, dtype=torch.float32, device=device), nb, L, hs, ws


class VfnetStarOffsetsFunction(Function):
    """(D0 (rows, 4), offsets of level 0, ..., offsets of level L - 1) from the raw output of `vfnet_reg` and the per-level
    scales (brcnn_vfnet_star_offsets): the offsets of a level are a (B, h, w, 18) view of one tensor, the input both star
    deformable convs of the level read.  Backward takes dD0 and the offset gradients of all levels (each possibly absent)
    and leaves d raw0 (every element written) and dscale (L,)"""

    @staticmethod
    def forward(ctx, r0, scales, batch, sizes, strides, denoms, gradient_mul, reg_off):
        from . import ops
        scales = scales.detach().float().contiguous()
        d0, off = ops.vfnet_star_offsets(r0, scales, batch, sizes, strides, denoms, gradient_mul, reg_off)
        ctx.save_for_backward(r0, scales, d0)
        ctx.cfg = (int(batch), [tuple(int(v) for v in s) for s in sizes], [int(s) for s in strides], float(gradient_mul),
                   int(reg_off))
        outs, r = [], 0
        for h, w in ctx.cfg[1]:
            n = batch * h * w
            outs.append(off[r:r + n].view(batch, h, w, 18))
            r += n
        return (d0,) + tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, dd0, *doffs):
        r0, scales, d0 = ctx.saved_tensors
        batch, sizes, strides, gm, reg_off = ctx.cfg
        doff = None
        if any(g is not None for g in doffs):
            doff = torch.cat([(g.float().reshape(-1, 18) if g is not None else r0.new_zeros((batch * h * w, 18)))
                              for g, (h, w) in zip(doffs, sizes)], 0).contiguous()
        dd0 = dd0.float().contiguous() if dd0 is not None else None
        lib = _L.load()
        ws, nb, L, hs, wds = _vfnet_rows_workspace(lib, batch, sizes, r0.device)
        dr0, dscale = torch.empty_like(r0), torch.empty_like(scales)
        st = lib.brcnn_vfnet_star_offsets_backward(_ptr(r0), int(r0.shape[1]), reg_off, _ptr(scales), batch, L, hs, wds,
                                                   _ints(strides), ctypes.c_float(gm).value, _ptr(d0), _ptr(dd0), _ptr(doff),
                                                   _ptr(ws), nb, _ptr(dr0), _ptr(dscale), _stream())
        _L.check(st, 'brcnn_vfnet_star_offsets_backward')
        return dr0, dscale, None, None, None, None, None, None


def vfnet_star_offsets(r0, scales, batch, sizes, strides, denoms, gradient_mul, reg_off=0):
    """(D0, [offsets per level]), differentiable w.r.t. r0 and scales"""
    out = VfnetStarOffsetsFunction.apply(r0, scales, batch, sizes, strides, denoms, gradient_mul, reg_off)
    return out[0], list(out[1:])


class VfnetRefineFunction(Function):
    """D1 = exp(scale_refine_l * raw1) * D0 with D0 a constant (brcnn_vfnet_refine), differentiable w.r.t. raw1 and the
    scales"""

    @staticmethod
    def forward(ctx, r1, scales_refine, d0, batch, sizes, reg_off):
        from . import ops
        scales_refine = scales_refine.detach().float().contiguous()
        d1 = ops.vfnet_refine(r1, scales_refine, batch, sizes, d0, reg_off)
        ctx.save_for_backward(r1, scales_refine, d1)
        ctx.cfg = (int(batch), [tuple(int(v) for v in s) for s in sizes], int(reg_off))
        return d1

    @staticmethod
    @once_differentiable
    def backward(ctx, dd1):
        r1, scales, d1 = ctx.saved_tensors
        batch, sizes, reg_off = ctx.cfg
        lib = _L.load()
        ws, nb, L, hs, wds = _vfnet_rows_workspace(lib, batch, sizes, r1.device)
        dd1 = dd1.float().contiguous()
        dr1, dscale = torch.empty_like(r1), torch.empty_like(scales)
        st = lib.brcnn_vfnet_refine_backward(_ptr(r1), int(r1.shape[1]), reg_off, _ptr(scales), batch, L, hs, wds, _ptr(d1),
                                             _ptr(dd1), _ptr(ws), nb, _ptr(dr1), _ptr(dscale), _stream())
        _L.check(st, 'brcnn_vfnet_refine_backward')
        return dr1, dscale, None, None, None, None


def vfnet_refine(r1, scales_refine, d0, batch, sizes, reg_off=0):
    return VfnetRefineFunction.apply(r1, scales_refine, d0.detach(), batch, sizes, reg_off)


class VfnetLossMeta(CenternessLossMeta):
    """the VFNet loss call: the base anchors of the pyramid (their centres are the points); scalar losses [loss_cls,
    loss_bbox, loss_bbox_rf] (include/brcnn_hip.h: cfg7_host).  The assignment is `atss_assign`."""

    kind = 'vfnet'

    def __init__(self, batch, sizes, strides, base_anchors, num_classes, gt_offsets, alpha, gamma, iou_weighted, eps, lw_cls,
                 lw_bbox, lw_refine):
        super().__init__(batch, sizes, strides, num_classes, gt_offsets,
                         [alpha, gamma, 1.0 if iou_weighted else 0.0, eps, lw_cls, lw_bbox, lw_refine])
        assert len(base_anchors) == 4 * self.L
        self.base = base_anchors


class VfnetLossFunction(Function):
    """losses (3,) = [loss_cls, loss_bbox, loss_bbox_rf] from A (rows, stride_a) and the distances D0, D1 (rows, 4),
    differentiable w.r.t. all three (brcnn_vfnet_loss_*); also coef3 and norm3 = [n_pos, sum w_ini, sum w_rf]"""

    @staticmethod
    def forward(ctx, a, d0, d1, gt_inds, gts, gt_labels, cls_off, meta, norm_hook):
        _require_gpu(a, d0, d1, gt_inds, gts, gt_labels)
        assert a.dim() == 2 and a.dtype == torch.float32 and a.is_contiguous() and a.shape[0] == meta.rows
        assert 0 <= cls_off and cls_off + meta.C <= a.shape[1]
        d0, d1 = d0.detach().float().contiguous(), d1.detach().float().contiguous()
        assert d0.shape == (meta.rows, 4) and d1.shape == (meta.rows, 4)
        assert gt_inds.dtype == torch.int32 and gt_inds.shape == (meta.batch, meta.per_image) and gt_inds.is_contiguous()
        if meta.total_gt:
            assert gts.dtype == torch.float32 and gts.shape == (meta.total_gt, 4) and gts.is_contiguous()
            assert gt_labels.dtype == torch.int64 and gt_labels.shape == (meta.total_gt,) and gt_labels.is_contiguous()
        lib = _L.load()
        ws, nb = meta.workspace(lib, a.device)
        out = torch.empty((9,), dtype=torch.float32, device=a.device)
        norm3, losses, coef = out[:3], out[3:6], out[6:]
        st = lib.brcnn_vfnet_loss_forward(*VfnetLossFunction._args(a, cls_off, d0, d1, gt_inds, gts, gt_labels, meta), _ptr(ws),
                                          nb, _ptr(norm3), _stream())
        _L.check(st, 'brcnn_vfnet_loss_forward')
        if norm_hook is not None:
            norm_hook(norm3)
        st = lib.brcnn_vfnet_loss_finalize(_ptr(ws), nb, _ptr(norm3), meta.batch, meta.L, meta.hs, meta.ws, meta.C, meta.cfg,
                                           _ptr(losses), _ptr(coef), _stream())
        _L.check(st, 'brcnn_vfnet_loss_finalize')
        ctx.save_for_backward(a, d0, d1, gt_inds, gts, gt_labels, coef)
        ctx.cls_off, ctx.meta = int(cls_off), meta
        ctx.mark_non_differentiable(coef, norm3)
        return losses, coef, norm3

    @staticmethod
    def _args(a, cls_off, d0, d1, gt_inds, gts, gt_labels, meta):
        gp, lp = (_ptr(gts), _ptr(gt_labels)) if meta.total_gt else (None, None)
        return (_ptr(a), int(a.shape[1]), int(cls_off), _ptr(d0), _ptr(d1), meta.batch, meta.L, meta.hs, meta.ws, meta.strides,
                meta.base, meta.C, _ptr(gt_inds), gp, lp, meta.gt_offsets, meta.cfg)

    @staticmethod
    @once_differentiable
    def backward(ctx, g3, _gc, _gn):
        a, d0, d1, gt_inds, gts, gt_labels, coef = ctx.saved_tensors
        meta = ctx.meta
        da, dd0, dd1 = torch.empty_like(a), torch.empty_like(d0), torch.empty_like(d1)
        g3 = g3.float().contiguous()
        st = _L.load().brcnn_vfnet_loss_backward(*VfnetLossFunction._args(a, ctx.cls_off, d0, d1, gt_inds, gts, gt_labels, meta),
                                                 _ptr(g3), _ptr(coef), _ptr(da), _ptr(dd0), _ptr(dd1), _stream())
        _L.check(st, 'brcnn_vfnet_loss_backward')
        return da, dd0, dd1, None, None, None, None, None, None


def vfnet_loss(a, d0, d1, gt_inds, gts, gt_labels, meta, cls_off=0, norm_hook=None):
    """(losses (3,), coef3, norm3); `norm_hook(norm3)` may change norm3 in place between the sums and the division (the mean
    over ranks)"""
    return VfnetLossFunction.apply(a, d0, d1, gt_inds, gts, gt_labels, cls_off, meta, norm_hook)


# ----------------------------------------------------------------------------- boosting loss
class BoostLossFunction(Function):
    """out3 = [loss_cls, loss_bbox, acc] of the boosting-reweighted R-CNN loss
    (prob_roi_head.py:107-154 over convfc_bbox_head.py:332-418)."""

    @staticmethod
    def forward(ctx, cls_score, bbox_pred, labels, priors, ious, bbox_targets, num_classes, agnostic, cfg6):
        _require_gpu(cls_score, bbox_pred, labels, priors, ious, bbox_targets)
        n = cls_score.shape[0]
        assert cls_score.shape == (n, num_classes + 1) and labels.dtype == torch.int64
        assert bbox_pred.shape == (n, 4 if agnostic else 4 * num_classes)
        cls_c, bb_c = cls_score.detach().float().contiguous(), bbox_pred.detach().float().contiguous()
        labels, priors = labels.contiguous(), priors.detach().float().contiguous()
        tg = bbox_targets.detach().float().contiguous()
        io = ious.detach().float().contiguous() if ious is not None else None
        lib = _L.load()
        dev = cls_score.device
        nb = lib.brcnn_boost_loss_workspace_bytes(n)
        ws = torch.empty((nb + 3) // 4, dtype=torch.float32, device=dev)
        out3 = torch.empty((3,), dtype=torch.float32, device=dev)
        coef = torch.empty((2,), dtype=torch.float32, device=dev)
        cfg = _floats(cfg6)
        st = lib.brcnn_boost_loss_forward_ex(_ptr(cls_c), _ptr(bb_c), _ptr(labels), _ptr(priors), _ptr(io), _ptr(tg), n,
                                             int(num_classes), int(bool(agnostic)), cfg, _ptr(ws), nb, _ptr(out3),
                                             _ptr(coef), _stream())
        _L.check(st, 'brcnn_boost_loss_forward_ex')
        ctx.save_for_backward(cls_c, bb_c, labels, priors, tg, coef, *([io] if io is not None else []))
        ctx.cfg = (n, int(num_classes), bool(agnostic), tuple(cfg6), cls_score.dtype, bbox_pred.dtype)
        return out3

    @staticmethod
    @once_differentiable
    def backward(ctx, g3):
        cls_c, bb_c, labels, priors, tg, coef, *rest = ctx.saved_tensors
        io = rest[0] if rest else None
        n, num_classes, agnostic, cfg6, cdt, bdt = ctx.cfg
        dcls, dbb = torch.empty_like(cls_c), torch.empty_like(bb_c)
        g3 = g3.float().contiguous()
        st = _L.load().brcnn_boost_loss_backward_ex(_ptr(cls_c), _ptr(bb_c), _ptr(labels), _ptr(priors), _ptr(io), _ptr(tg),
                                                    n, num_classes, int(agnostic), _floats(cfg6), _ptr(g3), _ptr(coef),
                                                    _ptr(dcls), _ptr(dbb), _stream())
        _L.check(st, 'brcnn_boost_loss_backward_ex')
        return dcls.to(cdt), dbb.to(bdt), None, None, None, None, None, None, None


def boost_loss(cls_score, bbox_pred, labels, priors, bbox_targets, num_classes, gamma, alpha=0.0, ious=None,
               iou_gamma=0.0, loss_cls_weight=1.0, loss_bbox_weight=1.0, reg_norm='bbox_num', reg_class_agnostic=False,
               plain_label_weights=False, smooth_l1_beta=0.0):
    """[loss_cls, loss_bbox, acc] as a (3,) tensor (differentiable w.r.t. cls_score and bbox_pred).
    `plain_label_weights`: the boosted weights enter the head's own loss as label weights (DyProbRoIHead,
    prob_roi_head.py:604-623) instead of ProbRoIHead's norm_loss; `smooth_l1_beta` > 0: SmoothL1Loss box term"""
    cfg8 = (float(gamma), float(alpha), float(iou_gamma), float(loss_cls_weight), float(loss_bbox_weight),
            1.0 if reg_norm == 'mean' else 0.0, 1.0 if plain_label_weights else 0.0, float(smooth_l1_beta))
    return BoostLossFunction.apply(cls_score, bbox_pred, labels, priors, ious, bbox_targets, int(num_classes),
                                   bool(reg_class_agnostic), cfg8)
