"""CPU tests: pin tests/loss_ref.py, the dtype-generic restatement of the fused RPN / boosting losses that
tests/test_loss_edges_gpu.py holds the HIP kernels against.  Its fp32 run must equal the project's CPU chain
(`head.loss`, pinned to the reference by fixtures g6 / g11 / g15) and the golden values of fixture g7 at the tolerances
the GPU tests already use for the same comparisons; its elementary terms must equal closed forms that need no code."""
import itertools
import math
import os

import pytest
import torch

import brcnn  # noqa: F401
from brcnn import Config
from tests import loss_ref as R
from tests import util
from tests.test_host_cpu import ROOT, T, _rpn_head, load

SIZES = [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]


def _head(recipe):
    if recipe is None:
        return _rpn_head()[0]
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'boosting_rcnn', recipe))
    c = cfg.model.rpn_head.copy()
    c.update(train_cfg=cfg.model.train_cfg.rpn, test_cfg=cfg.model.test_cfg.rpn)
    return brcnn.build_head(c)


def _ref_cfg(head):
    cls_mode, reg_mode = head._fused_loss_modes()
    return R.rpn_cfg(focal_gamma=head.loss_cls.gamma, focal_alpha=head.loss_cls.alpha, pos_weight=head.train_cfg.pos_weight,
                     iou_gamma=head.gamma, means=tuple(head.bbox_coder.means), stds=tuple(head.bbox_coder.stds),
                     with_aug=head.with_aug_loss, lw_cls=head.loss_cls.loss_weight, lw_bbox=head.loss_bbox.loss_weight,
                     lw_aug=head.aug_loss.loss_weight if head.with_aug_loss else 0.0,
                     lw_iou=head.loss_centerness.loss_weight, cls_mode=cls_mode, reg_mode=reg_mode)


@pytest.mark.parametrize('recipe,modes', [(None, (0, 0)),                                       # IoU-log + MSE aug, focal
                                          ('boosting_rcnn_r50_fpn_1x_coco.py', (0, 1)),         # CIoU on raw deltas
                                          ('boosting_rcnn_r50_pafpn_1x_voc.py', (1, 0))])       # VarifocalLoss
def test_rpn_loss_ref_fp32_equals_cpu_chain(recipe, modes):
    """fp32 restatement == autograd of the CPU `head.loss` on the g6 inputs (raw deltas under a per-level Scale),
    gt_inds from the CPU assigner; tolerances of test_rpn_loss_variants_equal_cpu_chain"""
    g = load('g6_rpn_loss')
    head = _head(recipe)
    assert head._fused_loss_modes() == modes
    A = head.num_anchors
    _, metas, _, _ = util.demo_inputs(2, 128, 192, seed=6)
    gts = [T(g['gt0']), T(g['gt1'])]
    sc = torch.tensor([1.3, 0.7, 1.1, 0.9, 1.5])
    if g['cls0'].shape[1] == A:
        cls, raw, iou = ([T(g[f'{k}{i}']).clone().requires_grad_() for i in range(5)] for k in ('cls', 'reg', 'iou'))
    else:       # the fixture's head outputs are 9 anchors wide; this recipe's head is not: seeded outputs on the fixture's gts
        gen = torch.Generator().manual_seed(21)
        cls = [(torch.randn(2, A, h, w, generator=gen) - 2).requires_grad_() for h, w in SIZES]
        raw = [(torch.randn(2, 4 * A, h, w, generator=gen) * 0.3).requires_grad_() for h, w in SIZES]
        iou = [torch.randn(2, A, h, w, generator=gen).requires_grad_() for h, w in SIZES]
    scp = sc.clone().requires_grad_()
    out = head.loss(cls, [r * scp[i] for i, r in enumerate(raw)], iou, gts, metas)
    assert sum(out['loss_rpn_bbox']).item() > 0
    tot = sum(sum(v) for v in out.values())
    ref_g = torch.autograd.grad(tot, cls + raw + iou + [scp])

    anchors = torch.cat(head.anchor_generator.grid_anchors(SIZES, 'cpu'), 0)
    gt_inds = torch.stack([head.assigner.assign(anchors, b).gt_inds for b in gts]).to(torch.int32)
    assert (gt_inds > 0).sum() > 0 and (gt_inds == 0).sum() > 0
    rows = [torch.cat([t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in (c_, r_, i_)], 1)
            for c_, r_, i_ in zip(cls, raw, iou)]
    y = torch.cat(rows, 0)
    y = torch.cat([y, torch.full((y.shape[0], 64 - 6 * A), 7.0)], 1).requires_grad_()
    s2 = sc.clone().requires_grad_()
    offs = [0, gts[0].shape[0], gts[0].shape[0] + gts[1].shape[0]]
    losses3, per_level, totals = R.rpn_loss_ref(y, s2, gt_inds, torch.cat(gts), offs, SIZES,
                                                head.anchor_generator.strides, head.anchor_generator.base_anchors, A,
                                                _ref_cfg(head), torch.float32)
    assert totals[0].item() == (gt_inds > 0).sum().item()
    for r, k in enumerate(('loss_rpn_cls', 'loss_rpn_bbox', 'loss_rpn_iou')):
        assert torch.allclose(losses3[r], sum(out[k]).detach(), rtol=2e-5, atol=1e-6), (k, losses3[r], sum(out[k]))
        assert torch.allclose(per_level[r], torch.stack(out[k]).detach(), rtol=2e-5, atol=1e-6), k
    gy, gs = torch.autograd.grad(losses3.sum(), [y, s2])
    assert torch.allclose(gs, ref_g[15], rtol=2e-4, atol=1e-7), (gs, ref_g[15])
    assert (gy[:, 6 * A:] == 0).all()
    r0 = 0
    for i, (h, w) in enumerate(SIZES):
        n = 2 * h * w
        for lo, hi, ref in ((0, A, ref_g[i]), (A, 5 * A, ref_g[5 + i]), (5 * A, 6 * A, ref_g[10 + i])):
            got = gy[r0:r0 + n, lo:hi].view(2, h, w, hi - lo).permute(0, 3, 1, 2)
            tol = 2e-4 * ref.abs().max().item() + 1e-7
            assert (got - ref).abs().max().item() <= tol, (recipe, i, lo, (got - ref).abs().max().item(), tol)
        r0 += n


@pytest.mark.parametrize('gamma', [0.5, 0.1])
def test_boost_loss_ref_fp32_equals_golden(gamma):
    """fp32 restatement == the reference's values and gradients (fixture g7); tolerances of test_boost_loss_golden"""
    g = load('g7_boost_loss')
    cls = T(g['cls_score']).clone().requires_grad_()
    bb = T(g['bbox_pred']).clone().requires_grad_()
    out3 = R.boost_loss_ref(cls, bb, T(g['labels']), T(g['priors']), None, T(g['bbox_targets']), 4,
                            R.boost_cfg(gamma=gamma, lw_cls=2.0, lw_bbox=2.0), torch.float32)
    gc, gb = torch.autograd.grad(out3[0] + out3[1], [cls, bb])
    assert torch.allclose(out3[0], T(g[f'g{gamma}_loss_cls']), rtol=1e-5)
    assert torch.allclose(out3[1], T(g[f'g{gamma}_loss_bbox']), rtol=1e-5)
    assert torch.allclose(out3[2], T(g[f'g{gamma}_acc'])[0])
    assert torch.allclose(gc, T(g[f'g{gamma}_dcls']), rtol=1e-4, atol=1e-9)
    assert torch.allclose(gb, T(g[f'g{gamma}_dbbox']), rtol=1e-5, atol=1e-9)


# ----------------------------------------------------------------------------- closed forms
def _box(*v):
    return torch.tensor([v], dtype=torch.float64)


def test_iou_log_loss_closed_forms():
    # prediction == gt: IoU 1, loss 0; every max / min ties, so each corner gets half of each of its two paths and the
    # two halves cancel: with a = w h, dL/dx1 = -(1/IoU) (dIoU/dx1) = (1/2)(2 h / a) - h / a = 0
    p = _box(8., 16., 40., 80.).requires_grad_()
    loss = R.iou_log_loss(p, _box(8., 16., 40., 80.))
    assert loss.item() == 0.0
    assert torch.equal(torch.autograd.grad(loss.sum(), p)[0], torch.zeros(1, 4, dtype=torch.float64))
    # only x1 shared, gt inside: ov = a_g = 256, un = a_p = 1024, loss = log un - log ov; the overlap is limited by the
    # gt everywhere except at x1, where the tie passes half of its path to the prediction
    p = _box(0., 0., 32., 32.).requires_grad_()
    q = _box(0., 4., 16., 20.)
    loss = R.iou_log_loss(p, q)
    assert abs(loss.item() - math.log(1024. / 256.)) < 1e-15
    gx1 = torch.autograd.grad(loss.sum(), p)[0][0, 0].item()
    # overlap ov = (16 - max(x1, 0)) * 16: d ov / d x1 = -16 / 2 at the tie; union un = a_p + a_g - ov, d a_p / d x1 = -32
    d_ov, d_un = -8.0, -32.0 + 8.0
    assert abs(gx1 - (-(d_ov / 256.) + d_un / 1024.)) < 1e-15
    # two disjoint unit boxes: IoU 0 floored at 1e-6, weight 0^g floored at 1e-12, no gradient through the floor
    p = _box(0., 0., 1., 1.).requires_grad_()
    q = _box(5., 0., 6., 1.)
    assert R.aligned_iou(p, q).item() == 0.0
    w = (R.aligned_iou(p, q) ** 0.5).clamp(min=R.WEIGHT_FLOOR)
    loss = (R.iou_log_loss(p, q) * w.detach()).sum()
    assert abs(loss.item() - (-math.log(1e-6) * 1e-12)) < 1e-24
    assert torch.equal(torch.autograd.grad(loss, p)[0], torch.zeros(1, 4, dtype=torch.float64))
    # degenerate union: two zero-area boxes, union floored at 1e-6, IoU 0
    assert R.aligned_iou(_box(1., 1., 1., 1.), _box(1., 1., 1., 1.)).item() == 0.0


def test_ciou_closed_forms():
    # identical boxes: IoU = a / (a + eps), rho = 0, v = 0 -> loss = eps / (a + eps)
    b = _box(0.1, -0.2, 1.3, 0.9)
    a = 1.2 * 1.1
    loss, iou, alpha, ci = R.ciou_parts(b.clone(), b, 1e-6)
    assert abs(loss.item() - 1e-6 / (a + 1e-6)) < 1e-15 and alpha.item() == 0.0
    # same centre, same aspect, half the size: IoU = 1/4 (eps aside), rho = 0, v ~ 0 -> loss = 3/4
    loss = R.ciou_loss(_box(-1., -1., 1., 1.), _box(-2., -2., 2., 2.), 0.0)
    assert abs(loss.item() - 0.75) < 1e-15
    # unit squares one apart on x: IoU 0, rho^2 = 1, enclosing box 2 x 1 -> c^2 = 5, loss = 1 + 1/5
    loss = R.ciou_loss(_box(0., 0., 1., 1.), _box(1., 0., 2., 1.), 0.0)
    assert abs(loss.item() - 1.2) < 1e-15
    # aspect term: p 2 x 1 and q 1 x 2 on one centre: IoU = 1/3, v = 4/pi^2 (atan(1/2) - atan 2)^2, alpha = 0 (IoU <= 0.5)
    p, q = _box(-1., -.5, 1., .5), _box(-.5, -1., .5, 1.)
    loss, iou, alpha, ci = R.ciou_parts(p, q, 0.0)
    assert abs(iou.item() - 1 / 3) < 1e-15 and alpha.item() == 0.0 and abs(loss.item() - 2 / 3) < 1e-15
    # ... and above 0.5: p 1 x 1, q 1 x 0.8 on one centre: IoU = 0.8, alpha = v / (0.2 + v), loss = 0.2 + alpha v
    p, q = _box(-.5, -.5, .5, .5), _box(-.5, -.4, .5, .4)
    v = 4 / math.pi ** 2 * (math.atan(1 / 0.8) - math.atan(1.0)) ** 2
    loss, iou, alpha, ci = R.ciou_parts(p, q, 0.0)
    assert abs(alpha.item() - v / (0.2 + v)) < 1e-14 and abs(loss.item() - (0.2 + v * v / (0.2 + v))) < 1e-14
    # a "box" of negative width far away: ci < -1 is clamped, loss 2, no gradient
    p = _box(3., 0., -3., 1.).requires_grad_()
    loss, iou, alpha, ci = R.ciou_parts(p, _box(40., 0., 41., 1.), 1e-6)
    assert ci.item() < -1 and loss.item() == 2.0
    assert torch.equal(torch.autograd.grad(loss.sum(), p)[0], torch.zeros(1, 4, dtype=torch.float64))


def test_focal_closed_form_and_its_backward():
    """inside |x| <= 12 nothing saturates: the closed form equals alpha_t (1 - p_t)^g BCE-with-logits and its analytic
    backward equals autograd of it; far outside, fp32 saturates at -log(FLT_MIN) and stays finite"""
    x = torch.linspace(-12, 12, 49, dtype=torch.float64)
    for is_pos, (gamma, alpha) in itertools.product((True, False), ((2.0, 0.25), (1.5, 0.4), (0.5, 0.75))):
        xa = x.clone().requires_grad_()
        xb = x.clone().requires_grad_()
        m = torch.full_like(x, is_pos, dtype=torch.bool)
        a = R.focal_closed_form(xa, m, gamma, alpha)
        t = m.double()
        p = torch.sigmoid(xb)
        b = torch.nn.functional.binary_cross_entropy_with_logits(xb, t, reduction='none') * \
            (alpha * t + (1 - alpha) * (1 - t)) * ((1 - p) * t + p * (1 - t)) ** gamma
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-300)
        ga, gb = torch.autograd.grad(a.sum(), xa)[0], torch.autograd.grad(b.sum(), xb)[0]
        assert torch.allclose(ga, gb, rtol=1e-9, atol=1e-300), (gamma, alpha, is_pos)
    xs = torch.tensor([30., 60., 100., -30., -60., -100.], dtype=torch.float32, requires_grad=True)
    sat = -math.log(R.FLT_MIN)
    neg = R.focal_closed_form(xs, torch.zeros(6, dtype=torch.bool), 2.0, 0.25)
    assert torch.allclose(neg[:3].detach(), torch.full((3,), 0.75 * sat)) and (neg[3:] == 0).all()
    pos = R.focal_closed_form(xs, torch.ones(6, dtype=torch.bool), 2.0, 0.25)
    assert (pos[:3] == 0).all() and torch.isfinite(pos).all() and pos[5].item() == pytest.approx(0.25 * sat, rel=1e-6)
    g = torch.autograd.grad(pos.sum() + neg.sum(), xs)[0]
    assert torch.isfinite(g).all()


def test_boost_terms_closed_forms():
    # uniform logits: CE = log(C + 1) per row; prior 1 -> weight exactly 0; plain form divides by #{w > 0}
    cls = torch.zeros(4, 5, dtype=torch.float64, requires_grad=True)
    bb = torch.zeros(4, 16, dtype=torch.float64, requires_grad=True)
    labels = torch.tensor([0, 4, 4, 2])
    pri = torch.tensor([0.0, 1.0, 0.75, 0.0], dtype=torch.float64)
    tgt = torch.tensor([[1., -1., 0., 0.05]] * 4, dtype=torch.float64)
    o = R.boost_loss_ref(cls, bb, labels, pri, None, tgt, 4, R.boost_cfg(gamma=0.5, plain=True, beta=0.1), torch.float64)
    assert abs(o[0].item() - math.log(5) * (1 + 0 + 0.5 + 1) / 3) < 1e-15
    # smooth-L1(0.1): |1| and |-1| -> 0.95 each, 0 -> 0, 0.05 -> 0.5 * 0.0025 / 0.1; two foreground rows, over N = 4
    assert abs(o[1].item() - 2 * (0.95 + 0.95 + 0.0125) / 4) < 1e-15
    assert o[2].item() == 25.0                     # all-equal rows: arg-max is class 0, only row 0 has that label
    # norm form: sum L w (sum L / sum w L) / N = sum L / N whatever the weights
    o = R.boost_loss_ref(cls, bb, labels, pri, None, tgt, 4, R.boost_cfg(gamma=0.5, alpha=1.5), torch.float64)
    assert abs(o[0].item() - math.log(5)) < 1e-15
    gb = torch.autograd.grad(o[1], bb)[0]
    assert abs(o[1].item() - 2 * 2.05 / 4) < 1e-15
    assert torch.equal(gb[0, :4], torch.tensor([-.25, .25, 0., -.25], dtype=torch.float64)) and gb[1:3].abs().sum() == 0
    assert gb[0, 4:].abs().sum() == 0 and torch.equal(gb[3, 8:12], gb[0, :4])
    # no foreground row: box term 0 under both normalisations, accuracy counts the first of tied maxima
    lab = torch.full((4,), 4)
    for norm in ('bbox_num', 'mean'):
        o = R.boost_loss_ref(cls, bb, lab, pri, None, tgt, 4, R.boost_cfg(reg_norm=norm), torch.float64)
        assert o[1].item() == 0.0 and o[2].item() == 0.0 and torch.isfinite(o).all()
