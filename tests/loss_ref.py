"""A dtype-generic restatement of the two fused train losses (`brcnn_rpn_loss_*`, `brcnn_boost_loss_*`), written from
the formulas in the header of csrc/train_loss.hip and the published definitions of the losses (focal, varifocal,
IoU / Complete-IoU, smooth-L1, softmax cross entropy).  Plain torch + autograd, no project kernel and no project loss
module: `float64` is the reference of tests/test_loss_edges_gpu.py, `float32` its round-off yardstick (how much fp32
round-off the chosen inputs amplify), and tests/test_loss_ref_cpu.py pins the fp32 run to the project's CPU chain.

torch semantics throughout: `torch.max` / `torch.min` of two tensors split the gradient evenly at a tie, `clamp`
passes the gradient at the bound, `abs` has gradient 0 at 0; iou_target, the CIoU alpha, the weights and the
normalisers are detached.

The focal term alone is not left to autograd.  It is the closed form of the native op of the reference,

    p = 1 / (1 + exp(-x)),   pos: -alpha (1 - p)^g log(max(p, FLT_MIN)),   neg: -(1 - alpha) p^g log(max(1 - p, FLT_MIN))

with that op's own analytic backward (which does not differentiate the `max`), so that the fp32 run carries the same
cancellation in `1 - p` and the same saturation at -log(FLT_MIN) as the kernel.
"""
import math

import torch
import torch.nn.functional as F

FLT_MIN = 1.1754943508222875e-38          # smallest normal fp32
WEIGHT_FLOOR = 1e-12                      # clamp(iou_target ** gamma, min=1e-12)

# ----------------------------------------------------------------------------- the bound of the GPU comparisons
K, ULPS, EPS32 = 4.0, 4.0, 2.0 ** -23
CEILING = 1e-4          # err32 above this: the inputs sit on an ill-conditioned point and the yardstick says nothing
# focal gradient of ONE logit, relative to itself, on |x| <= 12: 1 - p >= 6.1e-6 carries half an ulp of p ~ 1 (3e-8),
# 5e-3 relative, and enters to the third power (gamma 2 plus the bracket): 1.5e-2; the library calls add a few ulps
CEILING_FOCAL_ELEMENT = 5e-2
# focal loss VALUE of a call whose negatives reach x = 12: -log(1 - p) = 12 with an absolute error of 3e-8 / 6.1e-6 =
# 4.9e-3, 4.1e-4 relative, and those anchors dominate the sum
CEILING_FOCAL_SUM = 5e-4


def check_against_fp64(tag, got, r64, r32, mag=None, ceiling=CEILING):
    """kernel_err = |got - r64| <= K * max(err32) + ULPS fp32 ulps, err32 = |r32 - r64|, every error relative to `mag`
    (default: the element's own |r64|; broadcastable); where r64 is exactly 0, `got` must be exactly 0; max(err32)
    itself must stay below `ceiling`, so that a vacuous yardstick fails.  Prints the figures before it asserts."""
    got, r32, r64 = got.detach().cpu().double(), r32.detach().double(), r64.detach().double()
    assert got.shape == r64.shape == r32.shape, (tag, got.shape, r64.shape, r32.shape)
    assert torch.isfinite(got).all(), (tag, 'not finite')
    mag = r64.abs() if mag is None else mag.expand_as(r64)
    nz = mag > 0
    one = torch.ones_like(mag)
    rel_k = torch.where(nz, (got - r64).abs() / torch.where(nz, mag, one), torch.zeros_like(mag))
    rel_32 = torch.where(nz, (r32 - r64).abs() / torch.where(nz, mag, one), torch.zeros_like(mag))
    mk, m32 = rel_k.max().item() if rel_k.numel() else 0.0, rel_32.max().item() if rel_32.numel() else 0.0
    bound = K * m32 + ULPS * EPS32
    print(f'MEASURED {tag}: kernel_err {mk:.3e} max_err32 {m32:.3e} ratio '
          f'{(mk / m32) if m32 > 0 else float("nan"):.3f} of_bound {mk / bound:.3f}')
    assert m32 <= ceiling, (tag, 'err32 of the yardstick above its ceiling', m32, ceiling)
    zero = r64 == 0
    assert (got[zero] == 0).all(), (tag, 'reference exactly 0, kernel not', got[zero].abs().max().item())
    assert mk <= bound, (tag, mk, bound, m32)
    return mk, m32


RPN_DEFAULTS = dict(focal_gamma=2.0, focal_alpha=0.25, pos_weight=-1.0, iou_gamma=0.5, means=(0., 0., 0., 0.),
                    stds=(1., 1., 1., 1.), wh_ratio_clip=16 / 1000, with_aug=True, lw_cls=1.0, lw_bbox=1.0, lw_aug=1.0,
                    lw_iou=1.0, cls_mode=0, reg_mode=0)
BOOST_DEFAULTS = dict(gamma=0.5, alpha=0.0, iou_gamma=0.0, lw_cls=1.0, lw_bbox=1.0, reg_norm='bbox_num', agnostic=False,
                      plain=False, beta=0.0)


def rpn_cfg(**kw):
    assert set(kw) <= set(RPN_DEFAULTS), set(kw) - set(RPN_DEFAULTS)
    return dict(RPN_DEFAULTS, **kw)


def boost_cfg(**kw):
    assert set(kw) <= set(BOOST_DEFAULTS), set(kw) - set(BOOST_DEFAULTS)
    return dict(BOOST_DEFAULTS, **kw)


# ----------------------------------------------------------------------------- element-wise terms
class _FocalClosedForm(torch.autograd.Function):
    """sigmoid focal loss per logit, forward and backward as closed forms (see the module docstring)"""

    @staticmethod
    def forward(ctx, x, is_pos, gamma, alpha):
        p = 1 / (1 + torch.exp(-x))
        log_p, log_q = torch.log(p.clamp(min=FLT_MIN)), torch.log((1 - p).clamp(min=FLT_MIN))
        ctx.save_for_backward(p, log_p, log_q, is_pos)
        ctx.gamma, ctx.alpha = gamma, alpha
        return torch.where(is_pos, -alpha * (1 - p) ** gamma * log_p, -(1 - alpha) * p ** gamma * log_q)

    @staticmethod
    def backward(ctx, g):
        p, log_p, log_q, is_pos = ctx.saved_tensors
        gamma, alpha = ctx.gamma, ctx.alpha
        term_p = (1 - p) ** gamma * (1 - p - gamma * p * log_p)
        term_n = p ** gamma * (gamma * (1 - p) * log_q - p)
        return g * torch.where(is_pos, -alpha * term_p, -(1 - alpha) * term_n), None, None, None


def focal_closed_form(x, is_pos, gamma, alpha):
    return _FocalClosedForm.apply(x, is_pos, float(gamma), float(alpha))


def bce_with_logits(x, t):
    """-t log(sigmoid(x)) - (1 - t) log(1 - sigmoid(x)) = softplus(x) - x t (log1p(exp(.)) inside: no cancellation)"""
    return F.softplus(x) - x * t


def varifocal(x, t, gamma, alpha, iou_weighted):
    """BCE-with-logits(x, t) * (t [or 1] where t > 0, alpha |sigmoid(x) - t|^gamma elsewhere); t is a constant"""
    t = t.detach()
    pos = t > 0
    w_pos = t if iou_weighted else torch.ones_like(t)
    w = torch.where(pos, w_pos, alpha * (torch.sigmoid(x) - t).abs() ** gamma)
    return bce_with_logits(x, t) * w


def decode(anchors, deltas, means, stds, limit):
    """delta (dx, dy, dw, dh) -> corner box: centre + size * d, size * exp(clamp(d, +-limit)); no border clip"""
    px, py = (anchors[:, 0] + anchors[:, 2]) * 0.5, (anchors[:, 1] + anchors[:, 3]) * 0.5
    pw, ph = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    dx, dy = deltas[:, 0] * stds[0] + means[0], deltas[:, 1] * stds[1] + means[1]
    dw = (deltas[:, 2] * stds[2] + means[2]).clamp(min=-limit, max=limit)
    dh = (deltas[:, 3] * stds[3] + means[3]).clamp(min=-limit, max=limit)
    gw, gh = pw * torch.exp(dw), ph * torch.exp(dh)
    gx, gy = px + pw * dx, py + ph * dy
    return torch.stack([gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5], 1)


def encode(anchors, gt, means, stds):
    """corner boxes -> ((g_ctr - p_ctr) / p_size, log(g_size / p_size)), normalised"""
    px, py = (anchors[:, 0] + anchors[:, 2]) * 0.5, (anchors[:, 1] + anchors[:, 3]) * 0.5
    pw, ph = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    gx, gy = (gt[:, 0] + gt[:, 2]) * 0.5, (gt[:, 1] + gt[:, 3]) * 0.5
    gw, gh = gt[:, 2] - gt[:, 0], gt[:, 3] - gt[:, 1]
    return torch.stack([((gx - px) / pw - means[0]) / stds[0], ((gy - py) / ph - means[1]) / stds[1],
                        (torch.log(gw / pw) - means[2]) / stds[2], (torch.log(gh / ph) - means[3]) / stds[3]], 1)


def aligned_iou(a, b, eps=1e-6):
    """IoU of row-aligned corner boxes, union floored at eps"""
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    w = (torch.min(a[:, 2], b[:, 2]) - torch.max(a[:, 0], b[:, 0])).clamp(min=0)
    h = (torch.min(a[:, 3], b[:, 3]) - torch.max(a[:, 1], b[:, 1])).clamp(min=0)
    ov = w * h
    union = torch.max(area_a + area_b - ov, torch.full_like(ov, eps))
    return ov / union


def iou_log_loss(pred, target, eps=1e-6):
    return -torch.log(aligned_iou(pred, target).clamp(min=eps))


def ciou_parts(p, q, eps=1e-6):
    """Complete-IoU of row-aligned corner boxes: (loss, iou, alpha, ci) with
    ci = IoU - rho^2 / c^2 - alpha v,  v = 4 / pi^2 (atan(w_q / (h_q + eps)) - atan(w_p / (h_p + eps)))^2,
    alpha = [IoU > 0.5] v / (1 - IoU + v) (a constant),  loss = 1 - clamp(ci, -1, 1)"""
    w = (torch.min(p[:, 2], q[:, 2]) - torch.max(p[:, 0], q[:, 0])).clamp(min=0)
    h = (torch.min(p[:, 3], q[:, 3]) - torch.max(p[:, 1], q[:, 1])).clamp(min=0)
    ov = w * h
    w1, h1 = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    w2, h2 = q[:, 2] - q[:, 0], q[:, 3] - q[:, 1]
    iou = ov / (w1 * h1 + w2 * h2 - ov + eps)
    cw = (torch.max(p[:, 2], q[:, 2]) - torch.min(p[:, 0], q[:, 0])).clamp(min=0)
    ch = (torch.max(p[:, 3], q[:, 3]) - torch.min(p[:, 1], q[:, 1])).clamp(min=0)
    c2 = cw * cw + ch * ch + eps
    rho2 = ((q[:, 0] + q[:, 2]) - (p[:, 0] + p[:, 2])) ** 2 / 4 + ((q[:, 1] + q[:, 3]) - (p[:, 1] + p[:, 3])) ** 2 / 4
    v = (4 / math.pi ** 2) * (torch.atan(w2 / (h2 + eps)) - torch.atan(w1 / (h1 + eps))) ** 2
    alpha = (torch.where(iou > 0.5, v / (1 - iou + v), torch.zeros_like(v))).detach()
    ci = iou - (rho2 / c2 + alpha * v)
    return 1 - ci.clamp(min=-1.0, max=1.0), iou, alpha, ci


def ciou_loss(p, q, eps=1e-6):
    return ciou_parts(p, q, eps)[0]


# ----------------------------------------------------------------------------- RPN loss
def level_anchors(size, stride, base, dtype):
    """(h*w*A, 4) anchors of one level in (cell, a) order: base anchor + (x * stride_w, y * stride_h)"""
    h, w = size
    sw, sh = (stride, stride) if isinstance(stride, int) else stride
    xs = (torch.arange(w) * sw).repeat(h)
    ys = (torch.arange(h) * sh).repeat_interleave(w)
    shifts = torch.stack([xs, ys, xs, ys], 1).to(dtype)
    return (shifts[:, None, :] + base.detach().cpu().to(dtype)[None, :, :]).reshape(-1, 4)


def rpn_pos_details(y, scales, gt_inds, gts, gt_offsets, sizes, strides, base_anchors, A, cfg, dtype):
    """per level: dict of the positives' (row, a) indices and their detached intermediates -- what the tests read their
    coverage conditions from (iou_target, which side of the dw / dh clamp, the delta-box IoU and ci of the CIoU branch)"""
    return _rpn(y, scales, gt_inds, gts, gt_offsets, sizes, strides, base_anchors, A, cfg, dtype)[3]


def rpn_loss_ref(y, scales, gt_inds, gts, gt_offsets, sizes, strides, base_anchors, A, cfg, dtype):
    """losses3 = [loss_cls, loss_bbox, loss_iou] summed over the levels, per_level (3, L), totals = [num_pos,
    sum iou_target]; differentiable w.r.t. `y` (rows, ystride) = [cls A | raw deltas 4A | iou A | padding] and `scales`
    (L).  gt_inds (B, anchors per image): -1 ignored, 0 negative, k matched to row gt_offsets[b] + k - 1 of `gts`."""
    return _rpn(y, scales, gt_inds, gts, gt_offsets, sizes, strides, base_anchors, A, cfg, dtype)[:3]


def _rpn(y, scales, gt_inds, gts, gt_offsets, sizes, strides, base_anchors, A, cfg, dtype):
    y = y if y.dtype == dtype else y.to(dtype)
    scales = scales if scales.dtype == dtype else scales.to(dtype)
    gts = gts.detach().cpu().to(dtype).reshape(-1, 4)
    gt_inds = gt_inds.detach().cpu().long()
    B, L = gt_inds.shape[0], len(sizes)
    means, stds = cfg['means'], cfg['stds']
    limit = abs(math.log(cfg['wh_ratio_clip']))
    reg_mode, cls_mode = cfg['reg_mode'], cfg['cls_mode']
    with_aug = bool(cfg['with_aug']) and reg_mode == 0
    zero = torch.zeros((), dtype=dtype)
    s_cls, s_box, s_aug, s_bce, s_iout, details = [], [], [], [], [], []
    num_pos, row0, start = 0, 0, 0
    for l, (h, w) in enumerate(sizes):
        hw = h * w
        rows = y[row0:row0 + B * hw]
        cls, raw, iou_pred = rows[:, :A], rows[:, A:5 * A].reshape(B * hw, A, 4), rows[:, 5 * A:6 * A]
        gi = gt_inds[:, start:start + hw * A].reshape(B * hw, A)
        anchors = level_anchors((h, w), strides[l], base_anchors[l], dtype).reshape(hw, A, 4).repeat(B, 1, 1)
        pr, pa = torch.nonzero(gi > 0, as_tuple=True)
        iou_full = torch.zeros((B * hw, A), dtype=dtype)
        det = dict(rows=pr, a=pa)
        if pr.numel():
            img = pr // hw
            g = gts[torch.tensor(gt_offsets)[img] + gi[pr, pa] - 1]
            anc = anchors[pr, pa]
            d = raw[pr, pa] * scales[l]
            enc = encode(anc, g, means, stds)
            box = decode(anc, d, means, stds, limit)
            target_box = g if reg_mode == 0 else decode(anc, enc, means, stds, limit)
            iou_t = aligned_iou(box.detach(), target_box).detach()
            wgt = (iou_t ** cfg['iou_gamma']).clamp(min=WEIGHT_FLOOR).detach()
            if reg_mode == 0:
                s_box.append((iou_log_loss(box, g) * wgt).sum())
                s_aug.append((((d - enc) ** 2) * wgt[:, None]).sum() if with_aug else zero)
            else:
                loss, d_iou, d_alpha, d_ci = ciou_parts(d, enc, 1e-6)
                s_box.append((loss * wgt).sum())
                s_aug.append(zero)
                det.update(delta_iou=d_iou.detach(), alpha=d_alpha, ci=d_ci.detach())
            s_bce.append(bce_with_logits(iou_pred[pr, pa], iou_t).sum())
            s_iout.append(iou_t.sum())
            num_pos += pr.numel()
            iou_full[pr, pa] = iou_t
            dd = d.detach()
            det.update(iou_target=iou_t, weight=wgt, enc=enc.detach(), box=box.detach(), gt=g,
                       dw=dd[:, 2] * stds[2] + means[2], dh=dd[:, 3] * stds[3] + means[3])
        else:
            for s in (s_box, s_aug, s_bce, s_iout):
                s.append(zero)
        if cls_mode:
            s_cls.append(varifocal(cls, iou_full, cfg['focal_gamma'], cfg['focal_alpha'], cls_mode == 1).sum())
        else:
            f = focal_closed_form(cls, gi > 0, cfg['focal_gamma'], cfg['focal_alpha'])
            if cfg['pos_weight'] > 0:
                f = torch.where(gi > 0, f * cfg['pos_weight'], f)
            s_cls.append(torch.where(gi >= 0, f, torch.zeros_like(f)).sum())
        details.append(det)
        row0 += B * hw
        start += hw * A
    totals = torch.stack([torch.tensor(float(num_pos), dtype=dtype), torch.stack(s_iout).sum()]).detach()
    nts, baf = totals[0].clamp(min=1.0), totals[1].clamp(min=1.0)
    lc = cfg['lw_cls'] * (torch.stack(s_cls) / nts)
    lb = cfg['lw_bbox'] * torch.stack(s_box)
    if with_aug:
        lb = (lb + cfg['lw_aug'] * torch.stack(s_aug)) * 0.5
    lb = lb / baf
    li = cfg['lw_iou'] * (torch.stack(s_bce) / nts)
    per_level = torch.stack([lc, lb, li])
    return per_level.sum(1), per_level, totals, details


# ----------------------------------------------------------------------------- boosting loss
def boost_loss_ref(cls, bbox, labels, priors, ious, targets, C, cfg, dtype):
    """out3 = [loss_cls, loss_bbox, top-1 accuracy in percent] of the boosting-reweighted second-stage loss:
    L_i = lw_cls CE_i,  w_i = (1 - prior_i)^gamma [* |iou_i - p_i[label]|^iou_gamma] [* alpha]  (a constant);
    norm form: sum_i L_i w_i (sum L / sum w L) / N;  plain form: sum_i L_i w_i / max(#{w > 0}, 1);
    box term over the rows with a foreground label: L1 or smooth-L1(beta) of pred[label] - target, summed, times lw_bbox,
    over N ('bbox_num') or 4 n_pos ('mean'), 0 without a foreground row.  Differentiable w.r.t. `cls` and `bbox`."""
    cls = cls if cls.dtype == dtype else cls.to(dtype)
    bbox = bbox if bbox.dtype == dtype else bbox.to(dtype)
    priors, targets = priors.detach().to(dtype), targets.detach().to(dtype)
    n = cls.shape[0]
    logp = torch.log_softmax(cls, 1)
    L = cfg['lw_cls'] * -logp.gather(1, labels[:, None]).squeeze(1)
    p_label = torch.softmax(cls, 1).gather(1, labels[:, None]).squeeze(1).detach()
    w = (1 - priors) ** cfg['gamma']
    if ious is not None:
        w = (ious.detach().to(dtype) - p_label).abs() ** cfg['iou_gamma'] * w
    if cfg['alpha'] != 0:
        w = w * cfg['alpha']
    w = w.detach()
    if cfg['plain']:
        loss_cls = (L * w).sum() / max(float((w > 0).sum()), 1.0)
    else:
        loss_cls = (L * (w * (L.sum() / (w * L).sum())).detach()).sum() / n
    pos = labels < C
    n_pos = int(pos.sum())
    if n_pos:
        pred = bbox[pos] if cfg['agnostic'] else bbox.reshape(n, C, 4)[pos, labels[pos]]
        d = (pred - targets[pos]).abs()
        beta = cfg['beta']
        term = torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta) if beta > 0 else d
        loss_bbox = cfg['lw_bbox'] * term.sum() / (4 * n_pos if cfg['reg_norm'] == 'mean' else n)
    else:
        loss_bbox = bbox.sum() * 0
    acc = (cls.detach().argmax(1) == labels).to(dtype).sum() * (100.0 / n)
    return torch.stack([loss_cls, loss_bbox, acc])
