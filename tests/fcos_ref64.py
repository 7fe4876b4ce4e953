"""Float64 restatement of what csrc/fcos_head.hip computes: the point assignment, the candidate decode and the loss with
its gradients (torch autograd in float64).  Written from the definitions (FCOS: focal loss over every point, the smallest
ground truth whose box / centre box contains the point and whose largest side distance lies in the level's range,
centerness-weighted IoU-log | GIoU loss, centerness BCE); tests/test_fcos_cpu.py pins it to the reference's fixture before
the GPU tests lean on it.

`assign` takes a dtype: the comparisons of the assignment (strict inside test, inclusive range test, smallest area) are
decided by fp32 values in the reference, so the tests run it in float32 for exactness and in float64 to show that no
decision of their inputs sits on a rounding edge."""
import numpy as np
import torch

INF = 1e8
EPS32 = float(np.finfo(np.float32).eps)


def points(sizes, strides, dtype=torch.float64):
    out = []
    for (h, w), s in zip(sizes, strides):
        ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype), torch.arange(w, dtype=dtype), indexing='ij')
        out.append(torch.stack([xs.reshape(-1) * s + s // 2, ys.reshape(-1) * s + s // 2], -1))
    return out


def assign(gt_bboxes, sizes, strides, ranges, center_sampling=False, radius=1.5, dtype=torch.float64):
    """per image (points,) int64: index of the ground truth each point takes, -1 background (points level-major)"""
    pts_l = points(sizes, strides, dtype)
    pts = torch.cat(pts_l)
    lo = torch.cat([torch.full((len(p),), float(r[0]), dtype=dtype) for p, r in zip(pts_l, ranges)])
    hi = torch.cat([torch.full((len(p),), float(r[1]), dtype=dtype) for p, r in zip(pts_l, ranges)])
    rad = torch.cat([torch.full((len(p),), float(s * radius), dtype=dtype) for p, s in zip(pts_l, strides)])
    out = []
    for gt in gt_bboxes:
        gt = gt.to(dtype)
        if len(gt) == 0:
            out.append(torch.full((len(pts),), -1, dtype=torch.long))
            continue
        x, y = pts[:, 0:1], pts[:, 1:2]
        t = torch.stack([x - gt[:, 0], y - gt[:, 1], gt[:, 2] - x, gt[:, 3] - y], -1)          # (P, G, 4)
        if center_sampling:
            cx, cy = (gt[:, 0] + gt[:, 2]) / 2, (gt[:, 1] + gt[:, 3]) / 2
            r = rad[:, None]
            x0, y0 = torch.maximum(cx - r, gt[:, 0]), torch.maximum(cy - r, gt[:, 1])
            x1, y1 = torch.minimum(cx + r, gt[:, 2]), torch.minimum(cy + r, gt[:, 3])
            inside = torch.stack([x - x0, y - y0, x1 - x, y1 - y], -1).min(-1)[0] > 0
        else:
            inside = t.min(-1)[0] > 0
        far = t.max(-1)[0]
        ok = inside & (far >= lo[:, None]) & (far <= hi[:, None])
        area = ((gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]))[None].expand_as(far)
        area = torch.where(ok & (area < INF), area, torch.full_like(area, float('inf')))
        best, idx = area.min(1)             # the first of equal minima
        first = (area == best[:, None]).float().argmax(1)
        out.append(torch.where(torch.isinf(best), torch.full_like(idx, -1), first))
    return out


def _rows(levels):
    """per-level (B, c, h, w) -> level-major rows (sum B*h*w, c)"""
    return torch.cat([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in levels])


def candidates(cls, raw, ctr, scales, sizes, strides, norm_on_bbox, img_shapes, scale_factors=None):
    """per level float64 (B, hw) point scores = max_c sigmoid(cls) * sigmoid(ctr), (B, hw, C) class sigmoids, (B, hw)
    centerness sigmoids and (B, hw, 4) decoded, clipped (and rescaled) boxes"""
    out = []
    for l, ((h, w), s) in enumerate(zip(sizes, strides)):
        B = cls[l].shape[0]
        c = cls[l].double().permute(0, 2, 3, 1).reshape(B, h * w, -1).sigmoid()
        ct = ctr[l].double().permute(0, 2, 3, 1).reshape(B, h * w).sigmoid()
        v = raw[l].double().permute(0, 2, 3, 1).reshape(B, h * w, 4) * float(scales[l])
        d = v.clamp(min=0) * s if norm_on_bbox else v.exp()
        p = points([(h, w)], [s])[0][None]
        bx = torch.stack([p[..., 0] - d[..., 0], p[..., 1] - d[..., 1], p[..., 0] + d[..., 2], p[..., 1] + d[..., 3]], -1)
        for b in range(B):
            ih, iw = img_shapes[b][:2]
            hi = torch.tensor([iw, ih, iw, ih], dtype=torch.float64)
            bx[b] = torch.minimum(bx[b].clamp(min=0), hi)
            if scale_factors is not None:
                bx[b] = bx[b] / torch.as_tensor(scale_factors[b], dtype=torch.float64)
        out.append(((c * ct[..., None]).max(-1)[0], c, ct, bx))
    return out


def loss(cls, raw, ctr, scales, gt_inds, gt_bboxes, gt_labels, sizes, strides, norm_on_bbox=False, giou=False, gamma=2.0,
         alpha=0.25, eps=1e-6, weights=(1.0, 1.0, 1.0), norm2=None, grads=True):
    """cls / raw / ctr: per-level (B, c, h, w) fp32 RAW head outputs; scales (L,); gt_inds: per image (points,) as `assign`
    gives them.  Returns dict(losses (3,) float64, norm2 = [n_pos, sum of centerness targets], and with `grads` dcls / draw /
    dctr per level and dscale (L,)).  `norm2`: override of the two normalisers (as a mean over ranks would)."""
    L, B = len(sizes), cls[0].shape[0]
    C = cls[0].shape[1]
    leaf = lambda lst: [t.detach().double().requires_grad_(grads) for t in lst]     # noqa: E731
    cls64, raw64, ctr64 = leaf(cls), leaf(raw), leaf(ctr)
    sc64 = torch.as_tensor(scales, dtype=torch.float64).clone().requires_grad_(grads)
    n_l = [h * w for h, w in sizes]
    pts_l = points(sizes, strides)
    f_cls, f_ctr = _rows(cls64), _rows(ctr64).reshape(-1)
    f_v = torch.cat([_rows([raw64[l]]) * sc64[l] for l in range(L)])
    f_d = f_v.clamp(min=0) if norm_on_bbox else f_v.exp()
    # per row: the point, its level's stride, its ground truth
    f_pts = torch.cat([p.repeat(B, 1) for p in pts_l])
    f_stride = torch.cat([torch.full((B * n,), float(s), dtype=torch.float64) for n, s in zip(n_l, strides)])
    gi = torch.cat([torch.cat([gt_inds[b].split(n_l)[l] for b in range(B)]) for l in range(L)])
    img = torch.cat([torch.cat([torch.full((n,), b) for b in range(B)]) for n in n_l])
    pos = (gi >= 0).nonzero().reshape(-1)
    boxes = torch.zeros(len(gi), 4, dtype=torch.float64)
    labels = torch.full((len(gi),), C, dtype=torch.long)
    for i in pos.tolist():
        boxes[i] = gt_bboxes[int(img[i])][int(gi[i])].double()
        labels[i] = int(gt_labels[int(img[i])][int(gi[i])])
    # focal loss over every (point, class)
    p = f_cls.sigmoid()
    hot = torch.nn.functional.one_hot(labels, C + 1)[:, :C].double()
    pt = (1 - p) * hot + p * (1 - hot)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(f_cls, hot, reduction='none')
    sum_cls = (bce * (alpha * hot + (1 - alpha) * (1 - hot)) * pt.pow(gamma)).sum()
    # positives.  Every intermediate the fp32 kernel rounds is recorded with the number of roundings (in units of eps,
    # exp / log / sqrt counted as 2) that produce it from its operands: the first-order error bounds below are
    # sum |d out / d z| |z| c eps over them
    Z = []

    def rec(z, c):
        Z.append((z, c))
        return z
    x, y = f_pts[pos, 0], f_pts[pos, 1]
    t = torch.stack([x - boxes[pos, 0], y - boxes[pos, 1], boxes[pos, 2] - x, boxes[pos, 3] - y], -1)
    if norm_on_bbox:
        t = t / f_stride[pos, None]
    t = rec(t.detach().requires_grad_(grads), 2)
    ctr_t = rec(torch.sqrt((torch.minimum(t[:, 0], t[:, 2]) / torch.maximum(t[:, 0], t[:, 2])) *
                           (torch.minimum(t[:, 1], t[:, 3]) / torch.maximum(t[:, 1], t[:, 3]))), 5)
    v = rec(f_v[pos], 1)
    d = rec(v.clamp(min=0) if norm_on_bbox else v.exp(), 0 if norm_on_bbox else 2)
    pb = rec(torch.stack([x - d[:, 0], y - d[:, 1], x + d[:, 2], y + d[:, 3]], -1), 1)
    tb = rec(torch.stack([x - t[:, 0], y - t[:, 1], x + t[:, 2], y + t[:, 3]], -1), 1)
    pwh, twh = rec(pb[:, 2:] - pb[:, :2], 1), rec(tb[:, 2:] - tb[:, :2], 1)
    a1, a2 = rec(pwh[:, 0] * pwh[:, 1], 1), rec(twh[:, 0] * twh[:, 1], 1)
    wh = rec((torch.minimum(pb[:, 2:], tb[:, 2:]) - torch.maximum(pb[:, :2], tb[:, :2])).clamp(min=0), 1)
    inter = rec(wh[:, 0] * wh[:, 1], 1)
    union = rec((a1 + a2 - inter).clamp(min=eps), 2)
    iou = rec(inter / union, 1)
    if giou:
        ewh = rec((torch.maximum(pb[:, 2:], tb[:, 2:]) - torch.minimum(pb[:, :2], tb[:, :2])).clamp(min=0), 1)
        hull = rec((ewh[:, 0] * ewh[:, 1]).clamp(min=eps), 1)
        box_l = rec(1 - (iou - (hull - union) / hull), 4)
    else:
        box_l = rec(-iou.clamp(min=eps).log(), 2)
    box_w = rec(box_l * ctr_t, 1)
    sum_box = box_w.sum()
    xc = f_ctr[pos]
    bce_c = torch.nn.functional.binary_cross_entropy_with_logits(xc, ctr_t, reduction='none')
    sum_ctr = bce_c.sum()
    n2 = [float(len(pos)), float(ctr_t.detach().sum())] if norm2 is None else [float(v_) for v_ in norm2]
    N, S = max(n2[0], 1.0), max(n2[1], 1e-6)
    losses = torch.stack([weights[0] * sum_cls / N, weights[1] * sum_box / S, weights[2] * sum_ctr / N])
    out = dict(losses=losses.detach(), norm2=n2, n_pos=len(pos), ctr_targets=ctr_t.detach(), iou=iou.detach(),
               pos=pos, scaled=f_v.detach()[pos], labels=labels, abs_terms=[float(sum_cls.detach()), float(box_w.detach().abs().sum()),
                                                                             float(bce_c.detach().sum())],
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
        gv = torch.autograd.grad(sum_box, v, create_graph=True)[0]              # d sum_box / d(scale * raw), (P, 4)
        out['box_value_err'] = first_order(box_w)
        out['dv'] = gv.detach()
        out['dv_err'] = torch.stack([first_order(gv[:, k]) for k in range(4)], 1)
        # centerness BCE: (1 - t) x - log_sigmoid(x): 4 roundings on values of size <= |x| + 2, and the target's own error
        dt = 5 * EPS32 * ctr_t.detach()
        out['ctr_value_err'] = EPS32 * 4 * (xc.detach().abs() + 2) + xc.detach().abs() * dt
        out['dctr_elem_err'] = 4 * EPS32 * xc.detach().sigmoid() + dt
    if grads:
        losses.sum().backward()
        zero = lambda lst: [torch.zeros_like(t_) if t_.grad is None else t_.grad for t_ in lst]     # noqa: E731
        out.update(dcls=zero(cls64), draw=zero(raw64), dctr=zero(ctr64),
                   dscale=torch.zeros_like(sc64) if sc64.grad is None else sc64.grad)
    return out
