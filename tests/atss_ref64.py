"""Float64 restatement of what csrc/atss_head.hip computes: the adaptive assignment (with the library's tie rules), the
candidate decode and the loss with its gradients (torch autograd in float64).  Written from the definitions (ATSS: per
ground truth and level the k anchors nearest to the box centre, positives where the IoU reaches mean + std of the
candidates' IoUs and the anchor centre lies inside the box; focal loss over every anchor, centerness-weighted GIoU loss on
anchor-decoded boxes, centerness BCE); tests/test_atss_cpu.py pins it to the reference's fixture before the GPU tests lean
on it.

Tie rules: equal distances rank by ascending anchor index; an anchor claimed by several ground truths goes to the highest
IoU, equal IoUs to the lowest index.

`assign` takes a dtype: its comparisons are decided by fp32 values in the reference, so the tests run it in float32 for
exactness and in float64 to show that no decision of their inputs sits on a rounding edge."""
import math

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
MAX_RATIO = abs(math.log(16 / 1000))


def anchors(sizes, strides, octave, dtype=torch.float64):
    """per level (h*w, 4): the one square anchor of `octave` strides per cell, centred on the cell's origin (x*s, y*s)"""
    out = []
    for (h, w), s in zip(sizes, strides):
        ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing='ij')
        x, y, half = xs.reshape(-1) * s, ys.reshape(-1) * s, s * octave / 2
        out.append(torch.stack([x - half, y - half, x + half, y + half], -1))
    return out


def valid_mask(sizes, valid_hw):
    """(anchors,) bool from per-level [valid_h, valid_w] in cells (None: all)"""
    out = []
    for l, (h, w) in enumerate(sizes):
        vh, vw = (h, w) if valid_hw is None else valid_hw[l]
        m = torch.zeros(h, w, dtype=torch.bool)
        m[:vh, :vw] = True
        out.append(m.reshape(-1))
    return torch.cat(out)


def iou_table(an, gt, eps=1e-6):
    a, b = an[:, None, :], gt[None, :, :]
    area_a, area_b = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]), (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    wh = (torch.minimum(a[..., 2:], b[..., 2:]) - torch.maximum(a[..., :2], b[..., :2])).clamp(min=0)
    ov = wh[..., 0] * wh[..., 1]
    return ov / (area_a + area_b - ov).clamp(min=eps)


def assign(gt_bboxes, sizes, strides, octave, topk, valid_hws=None, dtype=torch.float64, details=False):
    """per image (anchors,) int64 in the kernel's convention: k > 0 positive for ground truth k - 1, 0 negative, -1 invalid
    cell.  valid_hws: per image None or per-level [valid_h, valid_w].  With `details`, also per image a dict of the
    candidates (M, G), their IoUs, distances, the thresholds, the side minima, the positive mask and, per (ground truth,
    level), the distance gap between ranks k and k + 1 (inf where the level has no more valid cells)."""
    an_l = anchors(sizes, strides, octave, dtype)
    an = torch.cat(an_l)
    starts = np.cumsum([0] + [len(a) for a in an_l])
    out, info = [], []
    for b, gt in enumerate(gt_bboxes):
        gt = gt.to(dtype)
        valid = valid_mask(sizes, None if valid_hws is None else valid_hws[b])
        G = len(gt)
        if G == 0:
            out.append(torch.where(valid, 0, -1).long())
            info.append(None)
            continue
        iou = iou_table(an, gt)
        ctr, gctr = (an[:, :2] + an[:, 2:]) / 2, (gt[:, :2] + gt[:, 2:]) / 2
        dx, dy = ctr[:, None, 0] - gctr[None, :, 0], ctr[:, None, 1] - gctr[None, :, 1]
        dist = (dx * dx + dy * dy).sqrt()
        picks, gaps = [], []
        for l in range(len(sizes)):
            idx = torch.arange(starts[l], starts[l + 1])[valid[starts[l]:starts[l + 1]]]
            k = min(topk, len(idx))
            srt, order = dist[idx].sort(dim=0, stable=True)          # ties: ascending anchor index
            picks.append(idx[order[:k]])
            gaps.append(srt[k] - srt[k - 1] if 0 < k < len(idx) else torch.full((G,), float('inf'), dtype=dtype))
        cand = torch.cat(picks, 0)                                   # (M, G)
        ci, cd = iou.gather(0, cand), dist.gather(0, cand)
        thr = ci.mean(0) + ci.std(0)
        cc = ctr[cand]                                               # (M, G, 2)
        side = torch.stack([cc[..., 0] - gt[:, 0], cc[..., 1] - gt[:, 1], gt[:, 2] - cc[..., 0], gt[:, 3] - cc[..., 1]], -1).min(-1)[0]
        pos = (ci >= thr[None, :]) & (side > 0.01)
        claimed = torch.full_like(iou, float('-inf'))
        cols = torch.arange(G)[None, :].expand_as(cand)
        claimed[cand[pos], cols[pos]] = iou[cand[pos], cols[pos]]
        best = claimed.max(1)[0]
        first = (claimed == best[:, None]).float().argmax(1)         # equal IoUs: the lowest index
        gi = torch.where(torch.isinf(best), torch.zeros_like(first), first + 1)
        out.append(torch.where(valid, gi, torch.full_like(gi, -1)))
        info.append(dict(cand=cand, iou=ci, dist=cd, thr=thr, side=side, pos=pos, gaps=torch.stack(gaps), claimed=claimed,
                         max_overlaps=torch.where(torch.isinf(best), torch.full_like(best, -1e8), best)))
    return (out, info) if details else out


def _rows(levels):
    """per-level (B, c, h, w) -> level-major rows (sum B*h*w, c)"""
    return torch.cat([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in levels])


def decode(an, d, means, stds, max_ratio=MAX_RATIO):
    """delta2bbox without the clip to the image: (n, 4) anchors and deltas -> corner boxes"""
    m, s = torch.as_tensor(means, dtype=d.dtype), torch.as_tensor(stds, dtype=d.dtype)
    dn = d * s + m
    ctr, size = (an[..., :2] + an[..., 2:]) * 0.5, an[..., 2:] - an[..., :2]
    new_size = size * dn[..., 2:].clamp(min=-max_ratio, max=max_ratio).exp()
    new_ctr = ctr + size * dn[..., :2]
    return torch.cat([new_ctr - new_size * 0.5, new_ctr + new_size * 0.5], -1)


def encode(an, gt, means, stds):
    m, s = torch.as_tensor(means, dtype=gt.dtype), torch.as_tensor(stds, dtype=gt.dtype)
    ctr, size = (an[..., :2] + an[..., 2:]) * 0.5, an[..., 2:] - an[..., :2]
    gctr, gsize = (gt[..., :2] + gt[..., 2:]) * 0.5, gt[..., 2:] - gt[..., :2]
    return (torch.cat([(gctr - ctr) / size, (gsize / size).log()], -1) - m) / s


def candidates(cls, raw, ctr, scales, sizes, strides, octave, means, stds, img_shapes, scale_factors=None):
    """per level float64 (B, hw) anchor scores = max_c sigmoid(cls) * sigmoid(ctr), (B, hw, C) class sigmoids, (B, hw)
    centerness sigmoids and (B, hw, 4) decoded, clipped (and rescaled) boxes"""
    out = []
    an_l = anchors(sizes, strides, octave)
    for l, (h, w) in enumerate(sizes):
        B = cls[l].shape[0]
        c = cls[l].double().permute(0, 2, 3, 1).reshape(B, h * w, -1).sigmoid()
        ct = ctr[l].double().permute(0, 2, 3, 1).reshape(B, h * w).sigmoid()
        v = raw[l].double().permute(0, 2, 3, 1).reshape(B, h * w, 4) * float(scales[l])
        bx = decode(an_l[l][None].expand(B, -1, -1), v, means, stds)
        for b in range(B):
            ih, iw = img_shapes[b][:2]
            hi = torch.tensor([iw, ih, iw, ih], dtype=torch.float64)
            bx[b] = torch.minimum(bx[b].clamp(min=0), hi)
            if scale_factors is not None:
                bx[b] = bx[b] / torch.as_tensor(scale_factors[b], dtype=torch.float64)
        out.append(((c * ct[..., None]).max(-1)[0], c, ct, bx))
    return out


def loss(cls, raw, ctr, scales, gt_inds, gt_bboxes, gt_labels, sizes, strides, octave, means, stds, gamma=2.0, alpha=0.25,
         eps=1e-6, weights=(1.0, 1.0, 1.0), norm2=None, grads=True):
    """cls / raw / ctr: per-level (B, c, h, w) fp32 RAW head outputs; scales (L,); gt_inds: per image (anchors,) as `assign`
    gives them.  Returns dict(losses (3, L) float64, norm2 = [sum_b max(n_pos_b, 1), sum of centerness targets], and with
    `grads` dcls / draw / dctr per level and dscale (L,)).  `norm2`: override of the two normalisers (as a mean over ranks
    would)."""
    L, B = len(sizes), cls[0].shape[0]
    C = cls[0].shape[1]
    leaf = lambda lst: [t.detach().double().requires_grad_(grads) for t in lst]     # noqa: E731
    cls64, raw64, ctr64 = leaf(cls), leaf(raw), leaf(ctr)
    sc64 = torch.as_tensor(scales, dtype=torch.float64).clone().requires_grad_(grads)
    n_l = [h * w for h, w in sizes]
    an_l = anchors(sizes, strides, octave)
    f_cls, f_ctr = _rows(cls64), _rows(ctr64).reshape(-1)
    f_v = torch.cat([_rows([raw64[l]]) * sc64[l] for l in range(L)])
    f_an = torch.cat([a.repeat(B, 1) for a in an_l])
    f_level = torch.cat([torch.full((B * n,), l) for l, n in enumerate(n_l)])
    gi = torch.cat([torch.cat([gt_inds[b].split(n_l)[l] for b in range(B)]) for l in range(L)])
    img = torch.cat([torch.cat([torch.full((n,), b) for b in range(B)]) for n in n_l])
    pos = (gi > 0).nonzero().reshape(-1)
    boxes = torch.zeros(len(gi), 4, dtype=torch.float64)
    labels = torch.full((len(gi),), C, dtype=torch.long)
    for i in pos.tolist():
        boxes[i] = gt_bboxes[int(img[i])][int(gi[i]) - 1].double()
        labels[i] = int(gt_labels[int(img[i])][int(gi[i]) - 1])
    weight = (gi >= 0).double()
    # focal loss over every (anchor, class) of a valid cell
    p = f_cls.sigmoid()
    hot = torch.nn.functional.one_hot(labels, C + 1)[:, :C].double()
    pt = (1 - p) * hot + p * (1 - hot)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(f_cls, hot, reduction='none')
    focal = bce * (alpha * hot + (1 - alpha) * (1 - hot)) * pt.pow(gamma) * weight[:, None]
    # positives.  Every intermediate the fp32 kernel rounds is recorded with the number of roundings (in units of eps,
    # exp / log / sqrt counted as 2) that produce it from its operands: the first-order error bounds below are
    # sum |d out / d z| |z| c eps over them.  Anchors are exact in fp32, and so are their centres and sizes.
    Z = []

    def rec(z, c):
        Z.append((z, c))
        return z
    m, s = torch.as_tensor(means, dtype=torch.float64), torch.as_tensor(stds, dtype=torch.float64)
    an = f_an[pos]
    a_ctr, a_size = (an[:, :2] + an[:, 2:]) * 0.5, an[:, 2:] - an[:, :2]

    def dec(d):
        dn = rec(d * s + m, 2)
        shift = rec(a_size * dn[:, :2], 1)
        e = rec(dn[:, 2:].clamp(min=-MAX_RATIO, max=MAX_RATIO).exp(), 2)
        size = rec(a_size * e, 1)
        c = rec(a_ctr + shift, 1)
        return rec(torch.cat([c - size * 0.5, c + size * 0.5], -1), 1), dn
    # the target round trip: bbox2delta (5 roundings per component), then the same decode
    t = rec(encode(an, boxes[pos], means, stds).detach().requires_grad_(grads), 5)
    tb, _ = dec(t)
    side = rec(torch.stack([a_ctr[:, 0] - tb[:, 0], a_ctr[:, 1] - tb[:, 1], tb[:, 2] - a_ctr[:, 0], tb[:, 3] - a_ctr[:, 1]], -1), 1)
    ctr_t = rec(torch.sqrt((torch.minimum(side[:, 0], side[:, 2]) / torch.maximum(side[:, 0], side[:, 2])) *
                           (torch.minimum(side[:, 1], side[:, 3]) / torch.maximum(side[:, 1], side[:, 3]))), 5)
    v = rec(f_v[pos], 1)
    pb, dn_p = dec(v)
    pwh, twh = rec(pb[:, 2:] - pb[:, :2], 1), rec(tb[:, 2:] - tb[:, :2], 1)
    a1, a2 = rec(pwh[:, 0] * pwh[:, 1], 1), rec(twh[:, 0] * twh[:, 1], 1)
    wh = rec((torch.minimum(pb[:, 2:], tb[:, 2:]) - torch.maximum(pb[:, :2], tb[:, :2])).clamp(min=0), 1)
    inter = rec(wh[:, 0] * wh[:, 1], 1)
    union = rec((a1 + a2 - inter).clamp(min=eps), 2)
    iou = rec(inter / union, 1)
    ewh = rec((torch.maximum(pb[:, 2:], tb[:, 2:]) - torch.minimum(pb[:, :2], tb[:, :2])).clamp(min=0), 1)
    hull = rec((ewh[:, 0] * ewh[:, 1]).clamp(min=eps), 1)
    box_l = rec(1 - (iou - (hull - union) / hull), 4)
    box_w = rec(box_l * ctr_t, 1)
    xc = f_ctr[pos]
    bce_c = torch.nn.functional.binary_cross_entropy_with_logits(xc, ctr_t.detach(), reduction='none')
    lv_pos = f_level[pos]
    per_level = lambda x, lv: torch.stack([x[lv == l].sum() for l in range(L)])      # noqa: E731
    n_img = [int(((gt_inds[b] > 0)).sum()) for b in range(B)]
    n2 = [float(sum(max(n, 1) for n in n_img)), float(ctr_t.detach().sum())] if norm2 is None else [float(v_) for v_ in norm2]
    N, S = max(n2[0], 1.0), max(n2[1], 1.0)
    sum_cls, sum_box, sum_ctr = per_level(focal.sum(1), f_level), per_level(box_w, lv_pos), per_level(bce_c, lv_pos)
    losses = torch.stack([weights[0] * sum_cls / N, weights[1] * sum_box / S, weights[2] * sum_ctr / N])
    out = dict(losses=losses.detach(), norm2=n2, n_pos=len(pos), ctr_targets=ctr_t.detach(), iou=iou.detach(), pos=pos,
               pos_level=lv_pos, scaled=f_v.detach()[pos], dn=dn_p.detach(), labels=labels, weight=weight, level=f_level,
               box_terms=box_w.detach(), ctr_terms=bce_c.detach(),
               edge_gap=float(torch.cat([(pb - tb).abs().reshape(-1), wh.reshape(-1) + (wh.reshape(-1) == 0) * 1e9]).detach().min())
               if len(pos) else float('inf'))
    if grads and len(pos):
        def first_order(vec):
            """per positive: sum over the recorded intermediates of |d vec_i / d z| |z| c eps"""
            gs = torch.autograd.grad(vec.sum(), [z for z, _ in Z], retain_graph=True, allow_unused=True)
            e = torch.zeros(len(pos), dtype=torch.float64)
            for (z, c), g in zip(Z, gs):
                if g is not None and c:
                    e = e + (g * z).abs().reshape(len(pos), -1).sum(1).detach() * c * EPS32
            return e
        gv = torch.autograd.grad(box_w.sum(), v, create_graph=True)[0]              # d sum_box / d(scale * raw), (P, 4)
        out['box_value_err'] = first_order(box_w)
        out['dv'] = gv.detach()
        out['dv_err'] = torch.stack([first_order(gv[:, k]) for k in range(4)], 1)
        # centerness BCE: (1 - t) x - log_sigmoid(x): 4 roundings on values of size <= |x| + 2, and the target's own error
        dt = first_order(ctr_t)
        out['ctr_target_err'] = dt
        out['ctr_value_err'] = EPS32 * 4 * (xc.detach().abs() + 2) + xc.detach().abs() * dt
        out['dctr_elem_err'] = 4 * EPS32 * xc.detach().sigmoid() + dt
    if grads:
        losses.sum().backward()
        zero = lambda lst: [torch.zeros_like(t_) if t_.grad is None else t_.grad for t_ in lst]     # noqa: E731
        out.update(dcls=zero(cls64), draw=zero(raw64), dctr=zero(ctr64),
                   dscale=torch.zeros_like(sc64) if sc64.grad is None else sc64.grad)
    return out
