"""Restatement of the VFNet head's star offsets, DCN v1 deformable conv, test-time decode, loss and gradients on torch ops with
autograd, written from the formulas of include/brcnn_hip.h (brcnn_vfnet_*) and the reference's definitions (vfnet_head.py,
varifocal_loss.py, transforms.py, mmcv's deform_conv), not from the kernels.  Every function computes in the dtype of its
inputs: float64 is the reference the GPU tests hold the kernels to, float32 the measure of what one fp32 evaluation in another
order differs by.  The assignment is tests/atss_ref64.assign.  tests/test_vfnet_cpu.py pins it to the fixture.

The point of a cell is the centre of its anchor, (x * s, y * s) for the recipe's center_offset = 0: an integer, exact in fp32."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import atss_ref64 as RA

EPS32 = float(np.finfo(np.float32).eps)
_rows = RA._rows


def points(sizes, strides, dtype=torch.float64):
    """per level (h*w, 2) [x, y] points"""
    out = []
    for (h, w), s in zip(sizes, strides):
        y, x = torch.meshgrid(torch.arange(h, dtype=dtype) * s, torch.arange(w, dtype=dtype) * s, indexing='ij')
        out.append(torch.stack([x.reshape(-1), y.reshape(-1)], -1))
    return out


def distances(raw, scale, denom):
    """exp(scale * raw) * denom, elementwise (denom a number or a tensor)"""
    return (raw * scale).exp() * denom


def star_offsets(d, gradient_mul, stride):
    """(..., 4) distances (l, t, r, b) in pixels -> (..., 18) offsets, [2t] = dy, [2t + 1] = dx of tap t: the nine star points
    (corners, side midpoints, centre of the box in cells) minus the regular 3 x 3 grid.  The gradient reaches `d` through
    the gradient_mul share only"""
    g = ((1 - gradient_mul) * d.detach() + gradient_mul * d) / stride
    left, top, right, bottom = g[..., 0], g[..., 1], g[..., 2], g[..., 3]
    zero = torch.zeros_like(left)
    dy = [-top, zero, bottom]
    dx = [-left, zero, right]
    out = []
    for t in range(9):
        out += [dy[t // 3] - (t // 3 - 1), dx[t % 3] - (t % 3 - 1)]
    return torch.stack(out, -1)


def sample_points(offsets):
    """(N, H, W, 18) offsets -> (N, H, W, 9, 2) sample coordinates (y, x) in cells"""
    N, H, W, _ = offsets.shape
    gy, gx = torch.meshgrid(torch.arange(H, dtype=offsets.dtype), torch.arange(W, dtype=offsets.dtype), indexing='ij')
    pts = []
    for t in range(9):
        pts.append(torch.stack([gy + (t // 3 - 1) + offsets[..., 2 * t], gx + (t % 3 - 1) + offsets[..., 2 * t + 1]], -1))
    return torch.stack(pts, 3)


def deform_conv_v1(x, offsets, weight):
    """DCN v1, 3 x 3, stride 1, padding 1, one group, no bias: x (N, H, W, C), offsets (N, H, W, 18), weight (O, C, 3, 3) ->
    (N, H, W, O).  mmcv's sampling: a point outside (-1, H) x (-1, W) is zero, else bilinear with zero beyond the map.
    Differentiable w.r.t. all three (the floor has no gradient)"""
    N, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))                       # a ring of zeros: corner -1 -> 0, corner H -> H + 1
    n_idx = torch.arange(N).view(N, 1, 1)
    p = sample_points(offsets)
    cols = []
    for t in range(9):
        py, px = p[..., t, 0], p[..., t, 1]
        inside = (py > -1) & (px > -1) & (py < H) & (px < W)
        py, px = torch.where(inside, py, torch.zeros_like(py)), torch.where(inside, px, torch.zeros_like(px))
        y0, x0 = py.detach().floor(), px.detach().floor()
        fy, fx = (py - y0)[..., None], (px - x0)[..., None]
        iy, ix = y0.long() + 1, x0.long() + 1
        v = xp[n_idx, iy, ix] * ((1 - fy) * (1 - fx)) + xp[n_idx, iy, ix + 1] * ((1 - fy) * fx) + \
            xp[n_idx, iy + 1, ix] * (fy * (1 - fx)) + xp[n_idx, iy + 1, ix + 1] * (fy * fx)
        cols.append(v * inside[..., None].to(x.dtype))
    col = torch.stack(cols, 3)                                                      # (N, H, W, 9, C)
    return torch.einsum('nhwkc,ock->nhwo', col, weight.reshape(weight.shape[0], C, 9))


def integer_margin(offsets):
    """the smallest distance of a star sample coordinate to an integer (the bilinear gradient w.r.t. the offset has a kink
    there), over the points inside the sampling range and the twelve coordinates that depend on the distances: the y of the
    middle row and the x of the middle column are the cell's own, integers by construction, and carry no gradient"""
    N, H, W, _ = offsets.shape
    p = sample_points(offsets.double())
    inside = (p[..., 0] > -1) & (p[..., 1] > -1) & (p[..., 0] < H) & (p[..., 1] < W)
    signed = torch.tensor([[t // 3 != 1, t % 3 != 1] for t in range(9)])
    frac = (p - p.round()).abs()[inside[..., None] & signed]
    return float(frac.min()) if frac.numel() else 1.0


def star_chain(raw0, scales, x_reg, x_cls, w_reg, w_cls, strides, denoms, gradient_mul):
    """raw0 -> D0 -> offsets -> relu(star dconv) of both towers, per level: raw0[l] (B, h, w, 4), x_*[l] (B, h, w, C), scales
    (L,) tensor, w_* (O, C, 3, 3).  Returns per level (D0, offsets, y_reg, y_cls)"""
    out = []
    for l, (r, xr, xc) in enumerate(zip(raw0, x_reg, x_cls)):
        d0 = distances(r, scales[l], denoms[l])
        off = star_offsets(d0, gradient_mul, strides[l])
        out.append((d0, off, deform_conv_v1(xr, off, w_reg).relu(), deform_conv_v1(xc, off, w_cls).relu()))
    return out


def corner_boxes(pts, d):
    return torch.stack([pts[..., 0] - d[..., 0], pts[..., 1] - d[..., 1], pts[..., 0] + d[..., 2], pts[..., 1] + d[..., 3]], -1)


def aligned_iou(a, b, eps=1e-6):
    wh = (torch.minimum(a[..., 2:], b[..., 2:]) - torch.maximum(a[..., :2], b[..., :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    area = lambda t: (t[..., 2] - t[..., 0]) * (t[..., 3] - t[..., 1])       # noqa: E731
    return inter / (area(a) + area(b) - inter).clamp(min=eps)


def giou_loss(a, b, eps=1e-6):
    wh = (torch.minimum(a[..., 2:], b[..., 2:]) - torch.maximum(a[..., :2], b[..., :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    area = lambda t: (t[..., 2] - t[..., 0]) * (t[..., 3] - t[..., 1])       # noqa: E731
    union = (area(a) + area(b) - inter).clamp(min=eps)
    ewh = (torch.maximum(a[..., 2:], b[..., 2:]) - torch.minimum(a[..., :2], b[..., :2])).clamp(min=0)
    hull = (ewh[..., 0] * ewh[..., 1]).clamp(min=eps)
    return 1 - (inter / union - (hull - union) / hull)


def candidates(cls, d1, sizes, strides, img_shapes, scale_factors=None):
    """per level float64: (B, hw) ranking scores = max_c sigmoid(cls), (B, hw, C) class sigmoids, (B, hw, 4) boxes of the
    refined distances d1[l] (B, 4, h, w), clipped (and rescaled)"""
    out = []
    for l, (c, d, pts) in enumerate(zip(cls, d1, points(sizes, strides))):
        B = c.shape[0]
        s = c.double().permute(0, 2, 3, 1).reshape(B, -1, c.shape[1]).sigmoid()
        box = corner_boxes(pts[None], d.double().permute(0, 2, 3, 1).reshape(B, -1, 4))
        for b in range(B):
            h, w = img_shapes[b][:2]
            box[b, :, 0::2] = box[b, :, 0::2].clamp(0, w)
            box[b, :, 1::2] = box[b, :, 1::2].clamp(0, h)
            if scale_factors is not None:
                box[b] = box[b] / torch.as_tensor(scale_factors[b], dtype=torch.float64)
        out.append((s.max(-1)[0], s, box))
    return out


def loss(cls, d0, d1, gt_inds, gt_bboxes, gt_labels, sizes, strides, alpha=0.75, gamma=2.0, iou_weighted=True,
         weights=(1.0, 1.5, 2.0), eps=1e-6, norm3=None, grads=True, dtype=torch.float64):
    """cls (B, C, h, w), d0 / d1 (B, 4, h, w) per level (distances in pixels); gt_inds: per image (anchors,) in
    brcnn_atss_assign's convention (<= 0: background, invalid cells included).  Returns dict(losses (3,) [loss_cls, loss_bbox,
    loss_bbox_rf], norm3 = [n_pos, sum w_ini, sum w_rf] before the clamp, and with `grads` dcls / dd0 / dd1 per level).  The
    target box of a positive is the reference's fp32 round trip distance2bbox(point, bbox2distance(point, gt)), taken as data.
    `norm3`: override of the three normalisers (as a mean over ranks would)."""
    L, B, C = len(sizes), cls[0].shape[0], cls[0].shape[1]
    leaf = lambda lst: [t.detach().to(dtype).requires_grad_(grads) for t in lst]     # noqa: E731
    cls64, d064, d164 = leaf(cls), leaf(d0), leaf(d1)
    n_l = [h * w for h, w in sizes]
    f_cls, f_d0, f_d1 = _rows(cls64), _rows(d064), _rows(d164)
    f_pts = torch.cat([p.repeat(B, 1) for p in points(sizes, strides, torch.float32)])
    gi = torch.cat([torch.cat([gt_inds[b].split(n_l)[l] for b in range(B)]) for l in range(L)])
    img = torch.cat([torch.cat([torch.full((m,), b) for b in range(B)]) for m in n_l])
    pos = (gi > 0).nonzero().reshape(-1)
    P = len(pos)
    gt = torch.zeros(P, 4, dtype=torch.float32)
    labels = torch.zeros(P, dtype=torch.long)
    for j, i in enumerate(pos.tolist()):
        gt[j] = gt_bboxes[int(img[i])][int(gi[i]) - 1].float()
        labels[j] = int(gt_labels[int(img[i])][int(gi[i]) - 1])
    pp = f_pts[pos]
    t32 = torch.stack([pp[:, 0] - gt[:, 0], pp[:, 1] - gt[:, 1], gt[:, 2] - pp[:, 0], gt[:, 3] - pp[:, 1]], -1)
    tb = corner_boxes(pp, t32).to(dtype)                                            # the fp32 round trip, as data
    pp = pp.to(dtype)
    b0, b1 = corner_boxes(pp, f_d0[pos]), corner_boxes(pp, f_d1[pos])
    w0, w1 = aligned_iou(b0, tb).clamp(min=1e-6).detach(), aligned_iou(b1, tb).clamp(min=1e-6).detach()
    box0, box1 = (giou_loss(b0, tb, eps) * w0).sum(), (giou_loss(b1, tb, eps) * w1).sum()
    sg = f_cls.sigmoid()
    terms = F.softplus(f_cls) * (alpha * sg.pow(gamma))
    hot = torch.zeros_like(terms, dtype=torch.bool)
    hot[pos, labels] = True
    xh = f_cls[pos, labels]
    bce = (1 - w1) * xh + F.softplus(-xh)
    hit = bce * w1 if iou_weighted else bce
    vfl = torch.where(hot, torch.zeros_like(terms), terms).sum() + hit.sum()
    n3 = [float(P), float(w0.sum()), float(w1.sum())] if norm3 is None else [float(v) for v in norm3]
    N, S0, S1 = (max(v, 1.0) for v in n3)
    losses = torch.stack([weights[0] * vfl / N, weights[1] * box0 / S0, weights[2] * box1 / S1])
    neg = torch.where(hot, torch.zeros_like(terms), terms).detach()
    out = dict(losses=losses.detach(), norm3=n3, n_pos=P, pos=pos, labels=labels, w_ini=w0, w_rf=w1, hot=hot,
               target_boxes=tb, boxes0=b0.detach(), boxes1=b1.detach(), giou0=giou_loss(b0, tb, eps).detach(),
               giou1=giou_loss(b1, tb, eps).detach(), x_hit=xh.detach(), bce_hit=bce.detach(), hit=hit.detach(), neg=neg,
               sigmoid=sg.detach(), softplus=F.softplus(f_cls).detach(), neg_abs=float(torch.where(hot, torch.zeros_like(terms), terms).abs().sum().detach()),
               hit_abs=float(hit.abs().sum().detach()))
    if grads:
        losses.sum().backward()
        zero = lambda lst: [torch.zeros_like(t_) if t_.grad is None else t_.grad for t_ in lst]     # noqa: E731
        out.update(dcls=zero(cls64), dd0=zero(d064), dd1=zero(d164))
    return out
