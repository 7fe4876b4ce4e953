"""Float64 restatements of the three cascade kernels (csrc/cascade.hip), written from the reference's definitions
(cascade_roi_head.py:264-284 / :342-378, bbox_head.py:382-498, delta_xywh_bbox_coder.py:145-272) and sharing no code with
the kernels or with the torch host path.  Decisions (arg-max, kept rows, order) are exact; values are float64."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)


def argmax_fg(cls_score):
    """arg-max over the foreground columns (all but the last), the LOWEST index on ties (torch's rule)"""
    fg = np.asarray(cls_score)[:, :-1]
    best = fg.max(axis=1, keepdims=True)
    return (fg == best).argmax(axis=1).astype(np.int64)         # (argmax of a boolean row = its first True)


def gather_deltas(bbox_pred, labels, agnostic):
    p = np.asarray(bbox_pred, dtype=np.float64)
    if agnostic:
        assert p.shape[1] == 4
        return p
    idx = labels[:, None] * 4 + np.arange(4)[None, :]
    return np.take_along_axis(p, idx, axis=1)


def delta2bbox(boxes, deltas, means, stds, max_shape_hw, wh_ratio_clip=16 / 1000):
    """boxes (n, 4), deltas (n, 4), max_shape_hw (n, 2) [h, w] per row; float64 throughout; the coder constants and the
    ratio clip are the fp32 numbers the kernel holds"""
    b, d = np.asarray(boxes, dtype=np.float64), np.asarray(deltas, dtype=np.float64)
    means = np.asarray(means, dtype=np.float32).astype(np.float64)
    stds = np.asarray(stds, dtype=np.float32).astype(np.float64)
    d = d * stds + means
    limit = float(np.float32(abs(np.log(wh_ratio_clip))))
    ctr, size = (b[:, :2] + b[:, 2:]) * 0.5, b[:, 2:] - b[:, :2]
    new_size = size * np.exp(np.clip(d[:, 2:], -limit, limit))
    new_ctr = ctr + size * d[:, :2]
    out = np.concatenate([new_ctr - new_size * 0.5, new_ctr + new_size * 0.5], axis=1)
    hw = np.asarray(max_shape_hw, dtype=np.float64)
    upper = np.stack([hw[:, 1], hw[:, 0], hw[:, 1], hw[:, 0]], axis=1)
    return np.minimum(np.maximum(out, 0.0), upper)


def box_bound(boxes):
    """(n, 4) bound on |fp32 decode - float64 decode|, per coordinate: 8 * EPS32 * (|centre| + size) along the coordinate's
    axis, the bound test_rcnn_decode_plain_against_float64 derives for the same arithmetic (six fp32 operations from the
    proposal to the corner, expf to 2 ulp; the clip does not enlarge an error).  `boxes` are the UNCLIPPED float64 boxes."""
    b = np.asarray(boxes, dtype=np.float64)
    mag = np.abs((b[:, :2] + b[:, 2:]) * 0.5) + (b[:, 2:] - b[:, :2])
    return 8 * EPS32 * np.concatenate([mag, mag], axis=1)


def refine_test(dets, num, cls_score, bbox_pred, max_shape, means, stds, agnostic):
    """-> dets_out (B, K, 5) float64, labels (B*K,), bound (B, K, 4) (zero on padded rows)"""
    dets = np.asarray(dets, dtype=np.float64)
    B, K, _ = dets.shape
    labels = argmax_fg(cls_score)
    rows_hw = np.repeat(np.asarray(max_shape, dtype=np.float64), K, axis=0)
    deltas = gather_deltas(bbox_pred, labels, agnostic)
    flat = dets.reshape(B * K, 5)[:, :4]
    boxes = delta2bbox(flat, deltas, means, stds, rows_hw)
    bound = box_bound(delta2bbox(flat, deltas, means, stds, np.full_like(rows_hw, np.inf)))
    valid = (np.arange(K)[None, :] < np.asarray(num)[:, None]).reshape(B * K)
    out = np.zeros((B * K, 5))
    out[valid, :4] = boxes[valid]
    bound = np.where(valid[:, None], bound, 0.0)
    return out.reshape(B, K, 5), labels, bound.reshape(B, K, 4)


def refine_train(rois, labels, gt_flags, row_offsets, cls_score, bbox_pred, max_shape, means, stds, agnostic, num_classes):
    """-> per image (kept boxes (n_b, 4) float64 in their original order, bound (n_b, 4)), and the labels used (N,)"""
    rois, labels = np.asarray(rois, dtype=np.float64), np.asarray(labels).astype(np.int64)
    used = np.where(labels == num_classes, argmax_fg(cls_score), labels)
    deltas = gather_deltas(bbox_pred, used, agnostic)
    out = []
    for b in range(len(row_offsets) - 1):
        r0, r1 = row_offsets[b], row_offsets[b + 1]
        hw = np.repeat(np.asarray(max_shape, dtype=np.float64)[b:b + 1], r1 - r0, axis=0)
        boxes = delta2bbox(rois[r0:r1, 1:], deltas[r0:r1], means, stds, hw)
        bound = box_bound(delta2bbox(rois[r0:r1, 1:], deltas[r0:r1], means, stds, np.full_like(hw, np.inf)))
        keep = np.asarray(gt_flags[r0:r1]) == 0
        out.append((boxes[keep], bound[keep]))
    return out, used


def mean_logits32(stage_scores):
    """the fp32 mean as the reference forms it: fp32 adds in stage order, then one fp32 division by float(stages)"""
    acc = np.asarray(stage_scores[0], dtype=np.float32).copy()
    for s in stage_scores[1:]:
        acc = (acc + np.asarray(s, dtype=np.float32)).astype(np.float32)
    return (acc / np.float32(len(stage_scores))).astype(np.float32)


def softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def flags_from_pos_is_gt(pos_is_gts, row_offsets):
    """the reference's per-image pos_is_gt lists (flags of an image's LEADING positives) -> gt_flags (N,) int32"""
    flags = np.zeros(row_offsets[-1], dtype=np.int32)
    for b, f in enumerate(pos_is_gts):
        f = np.asarray(f).astype(np.int32)
        flags[row_offsets[b]:row_offsets[b] + len(f)] = f
    return flags
