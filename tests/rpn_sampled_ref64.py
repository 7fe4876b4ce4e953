"""float64 numpy reference of the sampled RPN loss (RPNHead over AnchorHead.loss with a RandomSampler:
mmdet/models/dense_heads/anchor_head.py:373-497) and of its gradient, written from the formulas, sharing no code with
the kernels (csrc/rpn_sampled.hip) or with the torch host path:

    loss_rpn_cls  = lw_cls  * sum_{drawn}           w * bce_with_logits(x, is_pos)              / num_total_samples
    loss_rpn_bbox = lw_bbox * sum_{drawn positives} sum_4 l(pred - bbox2delta(anchor, gt))      / num_total_samples

with w = pos_weight for a positive when pos_weight > 0, else 1; l = |d| (L1) or SmoothL1(beta).

Besides the values it returns what a test needs to state an fp32 tolerance instead of tuning one: the sums of the
absolute terms and a bound on the fp32 evaluation error of the encoded targets.
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)


def flatten_outputs(cls, reg):
    """per-level (B, A, h, w) / (B, 4A, h, w) arrays -> x (B, n), pred (B, n, 4) in the reference's anchor order
    (level, cell row-major, anchor)"""
    B = cls[0].shape[0]
    x = np.concatenate([np.asarray(c, np.float64).transpose(0, 2, 3, 1).reshape(B, -1) for c in cls], 1)
    p = np.concatenate([np.asarray(r, np.float64).transpose(0, 2, 3, 1).reshape(B, -1, 4) for r in reg], 1)
    return x, p


def unflatten_grads(dx, dp, sizes, A):
    """inverse of flatten_outputs for the gradients: lists of (B, A, h, w) / (B, 4A, h, w)"""
    B = dx.shape[0]
    dcls, dreg, o = [], [], 0
    for h, w in sizes:
        n = h * w * A
        dcls.append(dx[:, o:o + n].reshape(B, h, w, A).transpose(0, 3, 1, 2))
        dreg.append(dp[:, o:o + n].reshape(B, h, w, 4 * A).transpose(0, 3, 1, 2))
        o += n
    return dcls, dreg


def encode(anchors, gt, means, stds):
    """bbox2delta (delta_xywh_bbox_coder.py:99-141) and a bound on the error of its fp32 evaluation"""
    px, py = (anchors[:, 0] + anchors[:, 2]) * 0.5, (anchors[:, 1] + anchors[:, 3]) * 0.5
    pw, ph = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    gx, gy = (gt[:, 0] + gt[:, 2]) * 0.5, (gt[:, 1] + gt[:, 3]) * 0.5
    gw, gh = gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]
    raw = np.stack([(gx - px) / pw, (gy - py) / ph, np.log(gw / pw), np.log(gh / ph)], 1)
    m, s = np.asarray(means, np.float64), np.asarray(stds, np.float64)
    t = (raw - m) / s
    # fp32: centres and sizes carry an absolute rounding error of ~eps * (largest coordinate) each (two of them meet in
    # every difference), the quotient 2 roundings, log / subtraction / division by std ~4 more
    X = np.maximum(np.abs(anchors).max(1), np.abs(gt).max(1))
    size = np.stack([pw, ph, np.minimum(gw, pw), np.minimum(gh, ph)], 1)
    err = EPS32 * (4.0 * X[:, None] / size + 4.0 * np.abs(raw) + 4.0 + 2.0 * np.abs(m)) / s + 2.0 * EPS32 * np.abs(t)
    return t, err


def sampled_rpn_loss(x, pred, anchors, gt_inds, gts, gt_offsets, drawn, num_total_samples, pos_weight=-1.0, beta=0.0,
                     means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.), lw_cls=1.0, lw_bbox=1.0):
    """x (B, n) logits, pred (B, n, 4) deltas, anchors (n, 4), gt_inds (B, n) (-1 / 0 / k), gts (sum G, 4),
    gt_offsets (B + 1), drawn: per image an int array of drawn anchor indices (entries < 0 are padding).
    Returns a dict: loss_cls, loss_bbox, dx (B, n), dpred (B, n, 4), and for tolerances n_cls / n_bbox (terms summed),
    abs_cls / abs_bbox (sums of |terms|, already scaled), err_bbox (scaled bound of the targets' fp32 error), terr
    (B, n, 4) per-coordinate target error (unscaled)."""
    x, pred = np.asarray(x, np.float64), np.asarray(pred, np.float64)
    anchors, gts = np.asarray(anchors, np.float64), np.asarray(gts, np.float64).reshape(-1, 4)
    B, n = x.shape
    k_cls, k_bbox = lw_cls / num_total_samples, lw_bbox / num_total_samples
    dx, dp, terr = np.zeros_like(x), np.zeros_like(pred), np.zeros_like(pred)
    out = dict(loss_cls=0.0, loss_bbox=0.0, n_cls=0, n_bbox=0, abs_cls=0.0, abs_bbox=0.0, err_bbox=0.0)
    for b in range(B):
        idx = np.asarray(drawn[b], np.int64).reshape(-1)
        idx = idx[idx >= 0]
        assert len(np.unique(idx)) == len(idx), 'an anchor is drawn once'
        gi = np.asarray(gt_inds[b], np.int64)[idx]
        assert (gi >= 0).all(), 'ignored anchors are never drawn'
        pos = gi > 0
        w = np.where(pos & (pos_weight > 0), pos_weight, 1.0)
        xi = x[b, idx]
        bce = np.maximum(xi, 0.0) - xi * pos + np.log1p(np.exp(-np.abs(xi)))
        out['loss_cls'] += k_cls * float((w * bce).sum())
        out['abs_cls'] += k_cls * float((w * (np.abs(xi) + np.log(2.0))).sum())
        out['n_cls'] += len(idx)
        dx[b, idx] = k_cls * w * (1.0 / (1.0 + np.exp(-xi)) - pos)
        if pos.any():
            pi = idx[pos]
            t, e = encode(anchors[pi], gts[gt_offsets[b] + gi[pos] - 1], means, stds)
            d = pred[b, pi] - t
            ad = np.abs(d)
            if beta > 0:
                l = np.where(ad < beta, 0.5 * ad * ad / beta, ad - 0.5 * beta)
                g = np.where(ad < beta, d / beta, np.sign(d))
            else:
                l, g = ad, np.sign(d)
            out['loss_bbox'] += k_bbox * float(l.sum())
            out['abs_bbox'] += k_bbox * float(l.sum())
            out['err_bbox'] += k_bbox * float((e + 2.0 * EPS32 * ad).sum())
            out['n_bbox'] += 4 * len(pi)
            dp[b, pi] = k_bbox * g
            terr[b, pi] = e
    out.update(dx=dx, dpred=dp, terr=terr)
    return out


def loss_tolerance(ref):
    """fp32 bounds for (loss_cls, loss_bbox) of a kernel that sums its terms in any fixed order:
    n * eps * sum|terms| for the summation (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4: any order),
    plus the evaluation error of a term -- 8 eps relative for max(x,0) - x*t + log1p(exp(-|x|)) (exp and log1p to a
    few ulp each, two additions), and the encoded targets' error for the box term"""
    tol_cls = (ref['n_cls'] + 8) * EPS32 * ref['abs_cls']
    tol_bbox = (ref['n_bbox'] + 8) * EPS32 * ref['abs_bbox'] + ref['err_bbox']
    return tol_cls, tol_bbox
