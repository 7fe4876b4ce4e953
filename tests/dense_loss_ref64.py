"""float64 numpy reference of the dense head's loss (RetinaHead over AnchorHead.loss with a PseudoSampler:
mmdet/models/dense_heads/anchor_head.py:373-491) and of its gradient, written from the formulas, sharing no code with the
kernels (csrc/dense_head.hip) or with the torch host path:

    loss_cls[l]  = lw_cls  * sum_{anchors of level l, classes c} w * focal(x_c, label == c)      / num_total_pos
    loss_bbox[l] = lw_bbox * sum_{positives of level l}          sum_4 l(pred - bbox2delta(anchor, gt)) / num_total_pos

    focal(x, hit) = -alpha (1 - p)^gamma log p  if hit  else  -(1 - alpha) p^gamma log(1 - p),   p = sigmoid(x)
    w = 0 for an anchor with gt_inds < 0 (ignore band, outside the image), pos_weight for a positive when pos_weight > 0,
    else 1;  l = |d| (L1) or SmoothL1(beta);  num_total_pos = sum over images of max(number of positives, 1).

Besides the values it returns what a test needs to state an fp32 tolerance instead of tuning one: the sums of the absolute
terms and bounds on the fp32 evaluation error of every term and of every gradient element.
"""
import numpy as np

from tests.rpn_sampled_ref64 import EPS32, encode


def flatten_outputs(cls, reg, num_classes):
    """per-level (B, A*C, h, w) / (B, 4A, h, w) arrays -> x (B, n, C), pred (B, n, 4) in the reference's anchor order
    (level, cell row-major, anchor), and the number of anchors of every level"""
    B, C = cls[0].shape[0], num_classes
    xs = [np.asarray(c, np.float64).transpose(0, 2, 3, 1).reshape(B, -1, C) for c in cls]
    ps = [np.asarray(r, np.float64).transpose(0, 2, 3, 1).reshape(B, -1, 4) for r in reg]
    return np.concatenate(xs, 1), np.concatenate(ps, 1), [x.shape[1] for x in xs]


def unflatten(dx, dp, sizes, A):
    """inverse of flatten_outputs (gradients, error bounds): lists of (B, A*C, h, w) / (B, 4A, h, w)"""
    B, C = dx.shape[0], dx.shape[2]
    dcls, dreg, o = [], [], 0
    for h, w in sizes:
        n = h * w * A
        dcls.append(dx[:, o:o + n].reshape(B, h, w, A * C).transpose(0, 3, 1, 2))
        dreg.append(dp[:, o:o + n].reshape(B, h, w, 4 * A).transpose(0, 3, 1, 2))
        o += n
    return dcls, dreg


def _softplus(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def focal(x, hit, gamma, alpha):
    """(term, d term / dx, fp32 error bound of the term, of the derivative) of the sigmoid focal loss, element-wise.

    The bounds follow the fp32 evaluation p = 1 / (1 + exp(-x)), q = 1 - p, pow, log (csrc/focal_loss.hip): p carries a
    relative error of 3 eps (exp to 2 ulp, one addition, one division), hence q = 1 - p an ABSOLUTE error dq = 3 eps p +
    eps q -- the cancellation that dominates for confident predictions -- and every pow / log / product a further
    relative 2 eps, counted as 6 eps (term) resp. 8 eps (derivative) on the whole expression."""
    p = 1.0 / (1.0 + np.exp(-x))
    q = 1.0 / (1.0 + np.exp(x))
    lp, lq = -_softplus(-x), -_softplus(x)              # log p, log(1 - p)
    dp_, dq = 3.0 * EPS32 * p, 3.0 * EPS32 * p + EPS32 * q
    tiny = np.finfo(np.float64).tiny
    qg1 = gamma * np.power(np.maximum(q, tiny), gamma - 1.0) if gamma > 0 else 0.0 * q      # d q^gamma / dq
    pg1 = gamma * np.power(np.maximum(p, tiny), gamma - 1.0) if gamma > 0 else 0.0 * p
    # hit:  T = alpha q^g (-lp);  G = -alpha q^g (q - g p lp)
    t_pos = alpha * np.power(q, gamma) * (-lp)
    br_pos = q + gamma * p * (-lp)
    g_pos = -alpha * np.power(q, gamma) * br_pos
    e_t_pos = alpha * (qg1 * dq * (-lp) + np.power(q, gamma) * dp_ / p) + 6.0 * EPS32 * t_pos
    e_g_pos = alpha * ((qg1 * dq + 2.0 * EPS32 * np.power(q, gamma)) * br_pos +
                       np.power(q, gamma) * (dq + gamma * dp_ * (1.0 - lp))) + 8.0 * EPS32 * np.abs(g_pos)
    # miss: T = (1 - alpha) p^g (-lq);  G = (1 - alpha) p^g (g q (-lq) + p)
    t_neg = (1.0 - alpha) * np.power(p, gamma) * (-lq)
    br_neg = gamma * q * (-lq) + p
    g_neg = (1.0 - alpha) * np.power(p, gamma) * br_neg
    e_t_neg = (1.0 - alpha) * (pg1 * dp_ * (-lq) + np.power(p, gamma) * dq / q) + 6.0 * EPS32 * t_neg
    e_g_neg = (1.0 - alpha) * ((pg1 * dp_ + 2.0 * EPS32 * np.power(p, gamma)) * br_neg +
                               np.power(p, gamma) * (gamma * dq * (1.0 - lq) + dp_)) + 8.0 * EPS32 * np.abs(g_neg)
    return (np.where(hit, t_pos, t_neg), np.where(hit, g_pos, g_neg), np.where(hit, e_t_pos, e_t_neg),
            np.where(hit, e_g_pos, e_g_neg))


def dense_loss(x, pred, level_sizes, anchors, gt_inds, gts, gt_labels, gt_offsets, gamma=2.0, alpha=0.25, pos_weight=-1.0,
               beta=0.0, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.), lw_cls=1.0, lw_bbox=1.0):
    """x (B, n, C) logits, pred (B, n, 4) deltas, level_sizes: anchors per level (sum = n), anchors (n, 4), gt_inds (B, n)
    (< 0 ignored / 0 background / k matched to ground truth k - 1 of the image), gts (sum G, 4), gt_labels (sum G),
    gt_offsets (B + 1).
    Returns a dict: loss_cls / loss_bbox (L,), tol_cls / tol_bbox (L,) fp32 bounds of a kernel that sums in any fixed order,
    dx (B, n, C) / dpred (B, n, 4) with their element-wise bounds dx_err / dpred_err, dpred_sure (B, n, 4) False where the
    sign of pred - target is not determined in fp32, num_total_pos and n_pos (B,), and the targets it formed: hit (B, n, C)
    (the anchor's label is this class) and weight (B, n)."""
    x, pred = np.asarray(x, np.float64), np.asarray(pred, np.float64)
    anchors, gts = np.asarray(anchors, np.float64), np.asarray(gts, np.float64).reshape(-1, 4)
    gt_inds, gt_labels = np.asarray(gt_inds, np.int64), np.asarray(gt_labels, np.int64).reshape(-1)
    B, n, C = x.shape
    L = len(level_sizes)
    bounds = np.concatenate([[0], np.cumsum(level_sizes)])
    assert bounds[-1] == n
    n_pos = (gt_inds > 0).sum(1)
    total = int(np.maximum(n_pos, 1).sum())
    # the kernel forms 1 / total and lw / total in fp32 (2 roundings), then one product per loss or gradient element
    k_cls, k_bbox, k_err = lw_cls / total, lw_bbox / total, 3.0 * EPS32
    hits, ws = np.zeros(x.shape, bool), np.zeros((B, n))
    dx, dxe = np.zeros_like(x), np.zeros_like(x)
    dp, dpe, sure = np.zeros_like(pred), np.zeros_like(pred), np.ones(pred.shape, bool)
    out = dict(loss_cls=np.zeros(L), loss_bbox=np.zeros(L), tol_cls=np.zeros(L), tol_bbox=np.zeros(L))
    for b in range(B):
        gi = gt_inds[b]
        pos = gi > 0
        label = np.full(n, C, np.int64)                 # background
        label[pos] = gt_labels[gt_offsets[b] + gi[pos] - 1]
        w = np.where(gi < 0, 0.0, np.where(pos & (pos_weight > 0), pos_weight, 1.0))
        hit = label[:, None] == np.arange(C)[None, :]
        hits[b], ws[b] = hit, w
        t, g, te, ge = focal(x[b], hit, gamma, alpha)
        dx[b] = k_cls * w[:, None] * g
        dxe[b] = k_cls * w[:, None] * (ge + (k_err + EPS32) * np.abs(g))
        tt = np.zeros((n, 4))
        terr = np.zeros((n, 4))
        if pos.any():
            tt[pos], terr[pos] = encode(anchors[pos], gts[gt_offsets[b] + gi[pos] - 1], means, stds)
        d = (pred[b] - tt) * pos[:, None]
        ad = np.abs(d)
        derr = (terr + 2.0 * EPS32 * ad) * pos[:, None]      # fp32 error of pred - target
        if beta > 0:
            lt = np.where(ad < beta, 0.5 * ad * ad / beta, ad - 0.5 * beta)
            gt_ = np.where(ad < beta, d / beta, np.sign(d))
            gerr = np.where(ad < beta + derr, derr / beta + 2.0 * EPS32 * np.abs(gt_), 0.0)
            lerr = np.where(ad < beta, ad * derr / beta + 4.0 * EPS32 * lt, derr + 2.0 * EPS32 * lt)
        else:
            lt, gt_, gerr, lerr = ad, np.sign(d), np.zeros_like(d), derr
            sure[b] = ~pos[:, None] | (ad > derr)
        lt, gt_ = lt * pos[:, None], gt_ * pos[:, None]
        dp[b] = k_bbox * gt_
        dpe[b] = k_bbox * (gerr + k_err * np.abs(gt_))
        for l in range(L):
            s = slice(bounds[l], bounds[l + 1])
            terms = w[s, None] * t[s]
            n_terms = int((w[s] > 0).sum()) * C
            out['loss_cls'][l] += k_cls * terms.sum()
            out['tol_cls'][l] += k_cls * ((w[s, None] * te[s]).sum() + k_err * terms.sum())
            out.setdefault('_abs_cls', np.zeros(L))[l] += k_cls * terms.sum()
            out.setdefault('_n_cls', np.zeros(L))[l] += n_terms
            out['loss_bbox'][l] += k_bbox * lt[s].sum()
            out['tol_bbox'][l] += k_bbox * (lerr[s].sum() + k_err * lt[s].sum())
            out.setdefault('_abs_bbox', np.zeros(L))[l] += k_bbox * lt[s].sum()
            out.setdefault('_n_bbox', np.zeros(L))[l] += 4 * int(pos[s].sum())
    # summation in any fixed order: n * eps * sum|terms| (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4)
    out['tol_cls'] += (out['_n_cls'] + 8) * EPS32 * out['_abs_cls']
    out['tol_bbox'] += (out['_n_bbox'] + 8) * EPS32 * out['_abs_bbox']
    out.update(dx=dx, dx_err=dxe, dpred=dp, dpred_err=dpe, dpred_sure=sure, num_total_pos=total, n_pos=n_pos, hit=hits,
               weight=ws)
    return out
