"""Float64 restatement of the GFL head's test-time decode, loss and gradients, written from the formulas of
include/brcnn_hip.h (brcnn_gfl_*) and the reference's definitions (gfl_head.py, gfocal_loss.py, transforms.py), not from the
kernels.  The assignment is tests/atss_ref64.assign.  tests/test_gfl_cpu.py pins it to the fixture; tests/test_gfl_gpu.py holds
the kernels to it, with bounds built from the first-order error records kept here.

The one anchor of a cell is centred on the cell's origin (x * s, y * s) (tests/atss_ref64.anchors), so the centre is an integer,
exact in fp32."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import atss_ref64 as RA

EPS32 = float(np.finfo(np.float32).eps)
_rows = RA._rows


def centers(sizes, strides, octave=2):
    """per level (h*w, 2) float64 anchor centres"""
    return [(a[:, :2] + a[:, 2:]) / 2 for a in RA.anchors(sizes, strides, octave)]


def integral(x):
    """(..., n + 1) logits -> expectation of the softmax over {0 .. n}"""
    p = F.softmax(x, -1)
    return (p * torch.arange(x.shape[-1], dtype=x.dtype)).sum(-1)


def clamp_hi(reg_max):
    """reg_max - 0.1 as the fp32 value the clamp compares with"""
    return float(np.float32(reg_max - 0.1))


def candidates(cls, raw, scales, sizes, strides, img_shapes, scale_factors=None, reg_max=16):
    """per level float64: (B, hw) anchor scores = max_c sigmoid(cls), (B, hw, C) class sigmoids, (B, hw, 4) decoded, clipped
    (and rescaled) boxes, and (B, hw) the bound of the fp32 kernel's box error (see `box_bound`)"""
    out = []
    n = reg_max + 1
    for l, (c, r, ctr) in enumerate(zip(cls, raw, centers(sizes, strides))):
        B = c.shape[0]
        s = c.double().permute(0, 2, 3, 1).reshape(B, -1, c.shape[1]).sigmoid()
        x = r.double().permute(0, 2, 3, 1).reshape(B, -1, 4, n) * float(scales[l])
        d = integral(x) * strides[l]
        box = torch.stack([ctr[None, :, 0] - d[..., 0], ctr[None, :, 1] - d[..., 1], ctr[None, :, 0] + d[..., 2],
                           ctr[None, :, 1] + d[..., 3]], -1)
        bound = box_bound(x.abs().amax((-1, -2)), strides[l], reg_max, float(ctr.abs().max()) + reg_max * strides[l])
        for b in range(B):
            h, w = img_shapes[b][:2]
            box[b, :, 0::2] = box[b, :, 0::2].clamp(0, w)
            box[b, :, 1::2] = box[b, :, 1::2].clamp(0, h)
            if scale_factors is not None:
                sf = torch.as_tensor(scale_factors[b], dtype=torch.float64)
                box[b] = box[b] / sf
                bound[b] = bound[b] / float(sf.min()) + EPS32 * float(box[b].abs().max())
        out.append((s.max(-1)[0], s, box, bound))
    return out


def box_bound(xmax, stride, reg_max, coord):
    """the fp32 error of a decoded coordinate.  A scaled logit x = scale * raw carries 1 rounding, x - max another: the
    argument of exp is off by <= 2 eps * 2|x|max, and exp adds 2 eps: every e_i has a relative error <= (4 |x|max + 2) eps.
    The n + 1 sequential additions of Z add (n + 1) eps, the division 1, the product with the bin 1, the n + 1 additions of
    the expectation (positive terms) n + 1: the distance, at most reg_max strides, is off by <= reg_max * stride * (2 * (4
    |x|max + 2) + 2 (n + 1) + 2) eps.  The product with the stride and the sum with the centre add 2 eps of the coordinate."""
    n = reg_max + 1
    return reg_max * stride * (2 * (4 * xmax + 2) + 2 * n + 2) * EPS32 + 2 * EPS32 * coord


def loss(cls, raw, scales, gt_inds, gt_bboxes, gt_labels, sizes, strides, octave=2, reg_max=16, beta=2.0, eps=1e-6,
         weights=(1.0, 1.0, 1.0), norm2=None, grads=True, bounds=True):
    """cls / raw: per-level (B, c, h, w) fp32 RAW head outputs; scales (L,); gt_inds: per image (anchors,) in
    brcnn_atss_assign's convention.  Returns dict(losses (3, L) float64 [qfl, bbox, dfl], norm2 = [sum_b max(n_pos_b, 1), sum
    of the positives' weights], and with `grads` dcls / draw per level and dscale (L,); with `bounds` the first-order error
    records the GPU test builds its bounds from).  `norm2`: override of the two normalisers (as a mean over ranks would)."""
    L, B, C, n = len(sizes), cls[0].shape[0], cls[0].shape[1], reg_max + 1
    leaf = lambda lst: [t.detach().double().requires_grad_(grads) for t in lst]     # noqa: E731
    cls64, raw64 = leaf(cls), leaf(raw)
    sc64 = torch.as_tensor(scales, dtype=torch.float64).clone().requires_grad_(grads)
    n_l = [h * w for h, w in sizes]
    f_cls = _rows(cls64)
    f_x = torch.cat([_rows([raw64[l]]) * sc64[l] for l in range(L)])
    f_ctr = torch.cat([c.repeat(B, 1) for c in centers(sizes, strides, octave)])
    f_level = torch.cat([torch.full((B * m,), l) for l, m in enumerate(n_l)])
    f_stride = torch.cat([torch.full((B * m,), float(s), dtype=torch.float64) for m, s in zip(n_l, strides)])
    gi = torch.cat([torch.cat([gt_inds[b].split(n_l)[l] for b in range(B)]) for l in range(L)])
    img = torch.cat([torch.cat([torch.full((m,), b) for b in range(B)]) for m in n_l])
    pos = (gi > 0).nonzero().reshape(-1)
    P = len(pos)
    boxes = torch.zeros(len(gi), 4, dtype=torch.float64)
    labels = torch.full((len(gi),), C, dtype=torch.long)
    for i in pos.tolist():
        boxes[i] = gt_bboxes[int(img[i])][int(gi[i]) - 1].double()
        labels[i] = int(gt_labels[int(img[i])][int(gi[i]) - 1])
    valid = (gi >= 0).double()
    # Every intermediate the fp32 kernel rounds is recorded with the number of roundings (in units of eps; exp / log / pow
    # counted as 2) that produce it from its operands: the first-order error bounds are sum |d out / d z| |z| c eps.
    Z = []

    def rec(z, c):
        Z.append((z, c))
        return z
    st = f_stride[pos]
    ctr = rec((f_ctr[pos] / st[:, None]).requires_grad_(grads), 1)
    tb = rec((boxes[pos] / st[:, None]).requires_grad_(grads), 1)
    x = rec(f_x[pos].reshape(P, 4, n), 1)
    u = rec(x - x.max(-1, keepdim=True)[0].detach(), 1)
    e = rec(u.exp(), 2)
    zs = rec(e.sum(-1), n)
    p = rec(e / zs[..., None], 1)
    pi = rec(p * torch.arange(n, dtype=torch.float64), 1)
    d = rec(pi.sum(-1), n)
    pb = rec(torch.stack([ctr[:, 0] - d[:, 0], ctr[:, 1] - d[:, 1], ctr[:, 0] + d[:, 2], ctr[:, 1] + d[:, 3]], -1), 1)
    pwh, twh = rec(pb[:, 2:] - pb[:, :2], 1), rec(tb[:, 2:] - tb[:, :2], 1)
    a1, a2 = rec(pwh[:, 0] * pwh[:, 1], 1), rec(twh[:, 0] * twh[:, 1], 1)
    wh = rec((torch.minimum(pb[:, 2:], tb[:, 2:]) - torch.maximum(pb[:, :2], tb[:, :2])).clamp(min=0), 1)
    inter = rec(wh[:, 0] * wh[:, 1], 1)
    union = rec((a1 + a2 - inter).clamp(min=eps), 2)
    iou = rec(inter / union, 1)
    ewh = rec((torch.maximum(pb[:, 2:], tb[:, 2:]) - torch.minimum(pb[:, :2], tb[:, :2])).clamp(min=0), 1)
    hull = rec((ewh[:, 0] * ewh[:, 1]).clamp(min=eps), 1)
    box_l = rec(1 - (iou - (hull - union) / hull), 4)
    wt = rec(f_cls[pos].detach().sigmoid().max(1)[0].requires_grad_(grads and bounds), 4)
    box_w = rec(box_l * wt, 1)
    # DFL
    side = torch.stack([ctr[:, 0] - tb[:, 0], ctr[:, 1] - tb[:, 1], tb[:, 2] - ctr[:, 0], tb[:, 3] - ctr[:, 1]], -1)
    t = rec(side.clamp(min=0, max=clamp_hi(reg_max)), 1)
    left = t.detach().floor().long()
    wl, wr = rec((left + 1).double() - t, 1), rec(t - left.double(), 1)
    lz = rec(zs.log(), 2)
    ce_l = rec(-(u.gather(-1, left[..., None])[..., 0] - lz), 1)
    ce_r = rec(-(u.gather(-1, left[..., None] + 1)[..., 0] - lz), 1)
    dfl_side = rec(ce_l * wl + ce_r * wr, 3)
    dfl = rec(dfl_side.sum(-1), 3)
    dfl_w = rec(dfl * wt * 0.25, 2)
    # QFL: every (anchor, class) of a valid cell against quality 0, the label of a positive against its quality
    q = iou.detach()
    sg = f_cls.sigmoid()
    qfl = F.binary_cross_entropy_with_logits(f_cls, torch.zeros_like(f_cls), reduction='none') * sg.pow(beta)
    hot = torch.zeros_like(qfl, dtype=torch.bool)
    hot[pos, labels[pos]] = True
    xh = f_cls[pos, labels[pos]]
    qz = rec(iou.detach().clone().requires_grad_(grads and bounds), 0)        # the quality as an input of the class term
    ph = rec(xh.sigmoid(), 4)
    ce_h = rec(rec((1 - qz) * xh, 2) - rec(F.logsigmoid(xh), 5), 1)
    diff = rec(qz - ph, 1)
    mod = rec(diff.abs().pow(beta), 2)
    hit_term = rec(ce_h * mod, 1)
    qfl = torch.where(hot, torch.zeros_like(qfl), qfl) * valid[:, None]
    per_level = lambda v, lv: torch.stack([v[lv == l].sum() for l in range(L)])      # noqa: E731
    lv_pos = f_level[pos]
    n_img = [int((gt_inds[b] > 0).sum()) for b in range(B)]
    n2 = [float(sum(max(m, 1) for m in n_img)), float(wt.detach().sum())] if norm2 is None else [float(v_) for v_ in norm2]
    N, S = max(n2[0], 1.0), max(n2[1], 1.0)
    sum_cls = per_level(qfl.sum(1), f_level) + per_level(hit_term, lv_pos)
    sum_box, sum_dfl = per_level(box_w, lv_pos), per_level(dfl_w, lv_pos)
    losses = torch.stack([weights[0] * sum_cls / N, weights[1] * sum_box / S, weights[2] * sum_dfl / S])
    out = dict(losses=losses.detach(), norm2=n2, n_pos=P, pos=pos, pos_level=lv_pos, labels=labels, valid=valid, level=f_level,
               hot=hot, quality=q, weight=wt.detach(), target=t.detach(), left=left, side=side.detach(), dist=d.detach(),
               box_terms=box_w.detach(), dfl_terms=dfl_w.detach(), hit_terms=hit_term.detach(), neg_terms=qfl.detach(),
               xmax=float(x.detach().abs().max()) if P else 0.0,
               edge_gap=float(torch.cat([(pb - tb).abs().reshape(-1), wh.reshape(-1) + (wh.reshape(-1) == 0) * 1e9]).detach().min())
               if P else float('inf'))
    if grads and bounds and P:
        def first_order(vec):
            """per positive: sum over the recorded intermediates of |d vec_i / d z| |z| c eps"""
            gs = torch.autograd.grad(vec.sum(), [z for z, _ in Z], retain_graph=True, allow_unused=True)
            err = torch.zeros(P, dtype=torch.float64)
            for (z, c), g in zip(Z, gs):
                if g is not None and c:
                    err = err + (g * z).abs().reshape(P, -1).sum(1).detach() * c * EPS32
            return err
        out['box_value_err'], out['dfl_value_err'] = first_order(box_w), first_order(dfl_w)
        out['quality_err'], out['weight_err'] = first_order(iou), 4 * EPS32 * wt.detach()
        # the class term at the label: its own intermediates, and the quality's error through d term / d quality
        gq = torch.autograd.grad(hit_term.sum(), qz, create_graph=True)[0]
        out['hit_value_err'] = first_order(hit_term) + gq.detach().abs() * out['quality_err']
        gh = torch.autograd.grad(hit_term.sum(), xh, create_graph=True)[0]
        gqh = torch.autograd.grad(gh.sum(), qz, retain_graph=True)[0]
        out['dhit'] = gh.detach()
        out['dhit_err'] = first_order(gh) + gqh.abs() * out['quality_err']
        # d (sum of the weighted box terms) / d x and d (sum of the weighted DFL terms) / d x, x the scaled logits (P, 4, n)
        for name, vec in (('box', box_w), ('dfl', dfl_w)):
            g = torch.autograd.grad(vec.sum(), x, create_graph=True)[0]
            out[f'dx_{name}'] = g.detach()
            out[f'dx_{name}_err'] = torch.stack([torch.stack([first_order(g[:, k, i]) for i in range(n)], 1) for k in range(4)], 1)
    if grads:
        losses.sum().backward()
        zero = lambda lst: [torch.zeros_like(t_) if t_.grad is None else t_.grad for t_ in lst]     # noqa: E731
        out.update(dcls=zero(cls64), draw=zero(raw64), dscale=torch.zeros_like(sc64) if sc64.grad is None else sc64.grad)
    return out


def qfl_background(x, beta):
    """float64 value and derivative of the class term off the label, softplus(x) * sigmoid(x)^beta, and the bounds of their
    fp32 evaluation.  Both are products / sums of positive factors: sigmoid carries 4 eps, its power beta times that + 2,
    softplus (max(x, 0) + log1p(exp(-|x|)), no cancellation) 5, the products and the sum of the derivative's two terms 4
    more: (4 beta + 16) eps relative.  The derivative sigmoid^beta (sigmoid + beta (1 - sigmoid) softplus) also holds 1 -
    sigmoid, whose error is the sigmoid's own, 4 eps sigmoid, in absolute terms"""
    x = np.asarray(x, dtype=np.float64)
    s = 1 / (1 + np.exp(-x))
    sp = np.logaddexp(0, x)
    val = sp * s ** beta
    der = s ** beta * (s + beta * (1 - s) * sp)
    rel = (4 * beta + 16) * EPS32
    return val, der, rel * val, rel * der + s ** beta * beta * sp * 4 * EPS32 * s
