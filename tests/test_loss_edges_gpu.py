"""-m gpu: the fused RPN / boosting loss kernels (csrc/train_loss.hip) against the float64 run of tests/loss_ref.py at the
branches the tame inputs of tests/test_train_gpu.py never take: exact max / min ties, disjoint predictions, the dw / dh
clamps, the alpha branch and the clamps of CIoU, every weight exponent, every classification mode, saturated logits,
empty normalisers, block tails, and for the boosting loss odd row counts, both head layouts, both normalisations, the
smooth-L1 knee, exact-0 / exact-1 priors, large logits and arg-max ties across the two 64-lane rounds of an 81-wide row.

Every case is ONE direct `train_ops.rpn_loss` / `train_ops.boost_loss` call plus one backward on a hand-built head
output of a few dozen anchors with a hand-set `gt_inds`; no model, no assigner.

Tolerance rule (no absolute tolerance anywhere).  For every compared tensor
    err32 = |restatement_fp32 - restatement_fp64|        how much fp32 round-off these inputs amplify
    kernel_err = |kernel - restatement_fp64|  <=  K * max(err32) + ULPS fp32 ulps of the reference magnitude
both relative to a magnitude: the element's own |reference| for loss values; for gradients the largest reference
component of the anchor within the tensor (cls, the 4 box deltas and the IoU branch are three tensors, each with its
own err32) or of the RoI row, so that a large gradient elsewhere cannot
mask a small anchor, and for d/dScale of a level the absolute sum of its terms sum |dreg * raw| (the quantity its
round-off scales with: the terms have both signs).  K = 4: expf / logf / powf / atanf of the device are within a few
ulp and the kernel evaluates in another order than torch.  ULPS = 4 is the floor for tensors whose err32 happens to be
(nearly) 0.  max(err32) of every compared tensor must itself stay below a ceiling (1e-4; 5e-2 for the focal gradient of
one logit relative to itself, see tests/loss_ref.py), so that inputs on an ill-conditioned point fail the test instead
of widening its bound.
Where the float64 reference is exactly 0 the kernel must give exactly 0.  Coverage conditions (which branch a case
takes) are asserted from the float64 reference, never from the kernel's output.

Saturated logits (family 7) are the one place where float64 is NOT the target: see the test's docstring.

Observed on the MI355X, worst tensor of each family: kernel_err / max(err32), kernel_err as a fraction of its bound, and
the largest max(err32) among the family's box / IoU-branch / Scale gradient tensors (what those gradients are held to,
times K, plus the floor of 4.8e-7).  A ratio above K = 4 appears only where err32 of that tensor happened to be (nearly)
0 and the ULPS floor carries the bound; no family needs more than K = 4 (every fraction of the bound is below 0.7;
0.25 = the kernel gives the bits of the fp32 restatement).

    family (test)                          kernel_err / max(err32)     kernel_err / bound     err32 of dreg, diou, dscale
    1  exact ties                          3.07  (loss_bbox)           0.25                   6.3e-7
    2  disjoint prediction                 3.56  (loss_bbox)           0.25                   4.8e-7
    3  dw / dh clamps                      104   (loss_bbox, floor)    0.39                   4.9e-7
    3  target-box clamp, CIoU mode         1.09  (dscale)              0.25                   2.5e-6
    4  CIoU alpha branch                   1.52  (dscale)              0.25                   4.0e-6
    5  weight exponent                     2.84  (loss_iou)            0.32                   8.3e-6
    6  classification modes                6.25  (loss_iou, floor)     0.65  (varifocal dcls) 1.2e-5
    7  saturated logits                    9.12  (loss_bbox, floor)    0.51  (diou)           2.8e-6
    8  normalisers                         2.47  (loss_iou)            0.29                   2.3e-6
    9 / 10  block tail, upstream gradient  147   (dscale, floor)       0.25                   1.4e-6
       rows of ignored anchors only        2.10  (dscale)              0.26                   3.9e-6
       boost edges                         165   (out3, floor)         0.37  (dcls, n = 260)  1.1e-7 (dbbox)
       boost all background                1.29                        0.17                   0
       boost one row with weight           3.92  (loss_cls)            0.18                   7.9e-8 (dbbox)
       sigmoid focal kernel (test_ops_gpu) 1.03                        0.25                   -
"""
import math

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import core, train_ops
from tests import loss_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

A, YS, PAD = 9, 64, 7.0
LIMIT = abs(math.log(16 / 1000))
SMALL = ([(3, 4), (2, 3), (1, 2)], [8, 16, 32])          # 216 / 108 / 36 anchors per level: below 256, no multiple of 64
BIG = ([(3, 5), (2, 3)], [8, 16])                        # 270 anchors on level 0: a 14-element tail in a second workgroup
BASE = core.AnchorGenerator(strides=[8, 16, 32], ratios=[0.5, 1.0, 2.0], octave_base_scale=4,
                            scales_per_octave=3).base_anchors
GRID = torch.linspace(-12, 12, 25)                       # fixed logit grid, 0 included
SQUARE = 3                                               # base anchor (ratio 1, scale 4): [-2s, -2s, 2s, 2s], dyadic


_check = R.check_against_fp64           # the tolerance rule of the module docstring, one tensor at a time


def _per_anchor(dy):
    """(rows, ystride) -> (rows, A, 6): each anchor's [cls, 4 reg, iou] gradient"""
    return torch.cat([dy[:, :A, None], dy[:, A:5 * A].reshape(-1, A, 4), dy[:, 5 * A:6 * A, None]], 2)


# ----------------------------------------------------------------------------- RPN cases
class Case:
    """2 images, a hand-built fused head output (rows, 64) with non-zero padding columns, a hand-set gt_inds"""

    def __init__(self, geom, cfg, g3=(1.0, 1.0, 1.0), seed=0):
        self.sizes, self.strides = geom
        self.cfg, self.g3, self.B = cfg, torch.tensor(g3, dtype=torch.float64), 2
        self.L = len(self.sizes)
        self.base = [BASE[l] for l in range(self.L)]
        self.scales = torch.tensor([1.3, 0.7, 1.1][:self.L])
        self.hw = [h * w for h, w in self.sizes]
        self.row0 = [0] + list(np.cumsum([self.B * n for n in self.hw]))
        self.start = [0] + list(np.cumsum([n * A for n in self.hw]))
        rows, n = self.row0[-1], self.row0[-1] * A
        gen = torch.Generator().manual_seed(seed)
        self.y = torch.full((rows, YS), PAD)
        self.y[:, :A] = GRID[(torch.arange(n) * 7) % 25].view(rows, A)
        self.y[:, A:5 * A] = torch.randn(rows, 4 * A, generator=gen) * 0.2
        self.y[:, 5 * A:6 * A] = GRID[(torch.arange(n) * 11 + 3) % 25].view(rows, A) * 0.25
        self.gt_inds = torch.zeros((self.B, self.start[-1]), dtype=torch.int32)
        self.gt_inds.view(-1)[::5] = -1                                   # ignored anchors mixed in
        self.gt_lists = [[], []]
        self.pos = []

    def anchor(self, l, cell, a):
        w = self.sizes[l][1]
        s = float(self.strides[l])
        sh = torch.tensor([(cell % w) * s, (cell // w) * s] * 2, dtype=torch.float32)
        return self.base[l][a] + sh                                       # fp32, as the kernel regenerates it

    def spots(self, n, anchors=tuple(range(A))):
        """n distinct (level, image, cell, a) places spread over the levels, both images and all cells"""
        cand = [(l, b, cell, a) for cell in range(max(self.hw)) for a in anchors for b in range(self.B)
                for l in range(self.L) if cell < self.hw[l]]
        step = next(p for p in (37, 41, 43, 47, 53) if len(cand) % p)       # coprime to len(cand): a permutation
        assert n <= len(cand)
        return [cand[(5 + j * step) % len(cand)] for j in range(n)]

    def add_pos(self, spot, gt, d=None):
        """make `spot` a positive matched to its own gt box; d = the SCALED deltas the loss should see (raw = d / Scale)"""
        l, b, cell, a = spot
        self.gt_lists[b].append([float(v) for v in gt])
        self.gt_inds[b, self.start[l] + cell * A + a] = len(self.gt_lists[b])
        if d is not None:
            raw = (torch.tensor(d, dtype=torch.float64) / self.scales[l].double()).float()
            self.y[self.row0[l] + b * self.hw[l] + cell, A + 4 * a:A + 4 * a + 4] = raw
        self.pos.append(spot)

    def set_cls(self, spot, x):
        l, b, cell, a = spot
        self.y[self.row0[l] + b * self.hw[l] + cell, a] = x

    def cls_in_gt_order(self, new=None):
        """the cls logits as a (B, anchors per image) tensor laid out like gt_inds; `new`: write them back"""
        if new is None:
            return torch.cat([self.y[self.row0[l]:self.row0[l + 1], :A].reshape(self.B, -1) for l in range(self.L)], 1)
        for l in range(self.L):
            self.y[self.row0[l]:self.row0[l + 1], :A] = new[:, self.start[l]:self.start[l + 1]].reshape(-1, A)

    def mark(self, spot, v):
        l, b, cell, a = spot
        self.gt_inds[b, self.start[l] + cell * A + a] = v

    @property
    def gts(self):
        flat = self.gt_lists[0] + self.gt_lists[1]
        return torch.tensor(flat, dtype=torch.float64).float().reshape(-1, 4)

    @property
    def offs(self):
        n0 = len(self.gt_lists[0])
        return [0, n0, n0 + len(self.gt_lists[1])]

    def gt_for_enc(self, spot, enc):
        """the gt box whose encoding against the spot's anchor is `enc` (means 0 / stds 1 scaled by the cfg's)"""
        l, _, cell, a = spot
        an = self.anchor(l, cell, a).double()
        m, s = self.cfg['means'], self.cfg['stds']
        px, py, pw, ph = (an[0] + an[2]) / 2, (an[1] + an[3]) / 2, an[2] - an[0], an[3] - an[1]
        gx, gy = px + pw * (enc[0] * s[0] + m[0]), py + ph * (enc[1] * s[1] + m[1])
        gw, gh = pw * math.exp(enc[2] * s[2] + m[2]), ph * math.exp(enc[3] * s[3] + m[3])
        return [gx - gw / 2, gy - gh / 2, gx + gw / 2, gy + gh / 2]

    # ---- the three runs
    def ref(self, dtype):
        y = self.y.to(dtype).requires_grad_()
        sc = self.scales.to(dtype).requires_grad_()
        args = (self.gt_inds, self.gts, self.offs, self.sizes, self.strides, self.base, A, self.cfg, dtype)
        l3, pl, tot = R.rpn_loss_ref(y, sc, *args)
        gy, gs = torch.autograd.grad((l3 * self.g3.to(dtype)).sum(), [y, sc], allow_unused=True)
        gy = torch.zeros_like(y) if gy is None else gy
        gs = torch.zeros_like(sc) if gs is None else gs
        return dict(l3=l3.detach(), pl=pl.detach(), tot=tot, dy=gy, ds=gs,
                    det=R.rpn_pos_details(y.detach(), sc.detach(), *args))

    def kernel(self):
        c = self.cfg
        meta = train_ops.RPNLossMeta(self.B, self.sizes, self.strides, [b.to(DEV) for b in self.base], A, self.offs,
                                     c['focal_gamma'], c['focal_alpha'], c['pos_weight'], c['iou_gamma'], c['means'],
                                     c['stds'], c['wh_ratio_clip'], c['with_aug'], c['lw_cls'], c['lw_bbox'], c['lw_aug'],
                                     c['lw_iou'], c['cls_mode'], c['reg_mode'])
        y = self.y.to(DEV).requires_grad_()
        sc = self.scales.to(DEV).requires_grad_()
        l3, pl, tot = train_ops.rpn_loss(y, sc, self.gt_inds.to(DEV), self.gts.to(DEV), meta)
        junk = torch.full_like(y, float('nan'))        # the block the allocator hands to the uninitialised dy next
        del junk
        gy, gs = torch.autograd.grad((l3 * self.g3.float().to(DEV)).sum(), [y, sc])
        return dict(l3=l3.detach().cpu(), pl=pl.detach().cpu(), tot=tot.cpu(), dy=gy.cpu(), ds=gs.cpu())

    def cat(self, det, key):
        v = [d[key] for d in det if key in d]
        return torch.cat(v) if v else torch.zeros(0, dtype=torch.float64)


def _compare(tag, case, r64=None, r32=None, cls_vs_fp32=False):
    """one kernel call + backward against the float64 / float32 runs of the restatement; completeness of the outputs
    (family 9) is checked on every case: all finite, padding columns exactly 0, d/dScale per level"""
    r64 = case.ref(torch.float64) if r64 is None else r64
    r32 = case.ref(torch.float32) if r32 is None else r32
    k = case.kernel()
    for name in ('l3', 'pl', 'tot'):
        for r, (g_, a_, b_) in enumerate(zip(k[name].reshape(3 if name != 'tot' else 2, -1),
                                             r64[name].reshape(3 if name != 'tot' else 2, -1),
                                             r32[name].reshape(3 if name != 'tot' else 2, -1))):
            if cls_vs_fp32 and name != 'tot' and r == 0:
                _check(f'{tag} {name}[{r}] vs fp32', g_, b_.double(), b_)
            else:
                focal_sum = name != 'tot' and r == 0 and case.cfg['cls_mode'] == 0
                _check(f'{tag} {name}[{r}]', g_, a_, b_, None, R.CEILING_FOCAL_SUM if focal_sum else R.CEILING)
    dy = k['dy']
    assert torch.isfinite(dy).all() and torch.isfinite(k['ds']).all()
    assert (dy[:, 6 * A:] == 0).all(), 'padding columns of dy'
    pa_k, pa_64, pa_32 = _per_anchor(dy), _per_anchor(r64['dy']), _per_anchor(r32['dy'])
    # the cls, box and IoU-branch gradients are three tensors, each with its own err32: the 1 - p cancellation of the
    # focal term must not set the bound of the box gradients.  Each anchor relative to its largest component of the group
    for nm, lo, hi in (('dcls', 0, 1), ('dreg', 1, 5), ('diou', 5, 6)):
        gk, g64, g32 = pa_k[:, :, lo:hi], pa_64[:, :, lo:hi], pa_32[:, :, lo:hi]
        if nm == 'dcls' and cls_vs_fp32:
            _check(f'{tag} dcls vs fp32', gk, g32.double(), g32)
            continue
        focal = nm == 'dcls' and case.cfg['cls_mode'] == 0
        _check(f'{tag} {nm}', gk, g64, g32, g64.abs().amax(2, keepdim=True),
               R.CEILING_FOCAL_ELEMENT if focal else R.CEILING)
        if focal:       # ... and against the largest cls gradient of the call, where the cancellation does not dominate
            _check(f'{tag} dcls vs max', gk, g64, g32, g64.abs().max().reshape(1, 1, 1))
    smag = torch.stack([(r64['dy'][case.row0[l]:case.row0[l + 1], A:5 * A] * case.y[case.row0[l]:case.row0[l + 1],
                        A:5 * A].double()).abs().sum() / case.scales[l].double().abs() for l in range(case.L)])
    _check(f'{tag} dscale', k['ds'], r64['ds'], r32['ds'], smag)
    return k, r64, r32


def _generic_positives(case, n, seed, anchors=tuple(range(A))):
    """n positives whose gt sits near the anchor (centre shift -0.1 size, size ratio e^0.2, jittered) and whose scaled
    deltas sit near the encoding: well-overlapping decoded boxes, and an encoding that reads as a proper box"""
    gen = torch.Generator().manual_seed(seed)
    for s in case.spots(n, anchors):
        enc = (torch.tensor([-0.1, -0.1, 0.2, 0.2], dtype=torch.float64) +
               (torch.rand(4, generator=gen, dtype=torch.float64) - 0.5) * 0.1)
        u = torch.rand(4, generator=gen, dtype=torch.float64) - 0.5
        d = enc + torch.sign(u) * 0.01 + u * 0.1                            # every coordinate off the encoding's by >= 0.01
        case.add_pos(s, case.gt_for_enc(s, enc.tolist()), d.tolist())


# ---- 1
@pytest.mark.parametrize('variant', ['all', 'x1', 'y2'])
def test_rpn_exact_ties(variant):
    """zero deltas on the dyadic square anchor: the decoded box IS the anchor in fp32 and fp64 alike.  gt == anchor:
    IoU 1, loss 0, all four max / min tie, each corner gets 0.5 of both paths and the IoU gradient cancels exactly;
    gt sharing only x1 / only y2 with it: one tie factor 0.5 in an otherwise generic gradient"""
    case = Case(SMALL, R.rpn_cfg(reg_mode=0, with_aug=True))
    for s in case.spots(4, (SQUARE,)):
        l, _, cell, a = s
        an = case.anchor(l, cell, a).double()
        st = float(case.strides[l])
        gt = {'all': an.tolist(),
              'x1': [an[0], an[1] + st / 2, an[2] - st, an[3] - st / 4],
              'y2': [an[0] + st / 4, an[1] + st / 2, an[2] - st, an[3]]}[variant]
        case.add_pos(s, gt, [0.0, 0.0, 0.0, 0.0])
    r64, r32 = case.ref(torch.float64), case.ref(torch.float32)
    for r in (r64, r32):
        box, gt = case.cat(r['det'], 'box').double(), case.cat(r['det'], 'gt').double()
        tie = box == gt
        want = {'all': [True] * 4, 'x1': [True, False, False, False], 'y2': [False, False, False, True]}[variant]
        assert box.shape[0] == 4 and (tie == torch.tensor(want)).all()
    if variant == 'all':
        assert (case.cat(r64['det'], 'iou_target') == 1).all() and r64['l3'][1].item() == 0
        assert (_per_anchor(r64['dy'])[:, :, 1:5] == 0).all()
    else:
        reg = _per_anchor(r64['dy'])[:, :, 1:5]
        assert (reg.abs().amax(2) > 0).sum() == 4
    _compare(f'ties[{variant}]', case, r64, r32)


# ---- 2
@pytest.mark.parametrize('reg_mode,with_aug', [(0, False), (0, True), (1, False)])
def test_rpn_disjoint_prediction(reg_mode, with_aug):
    """dx / dy so large that the decoded box misses its target: iou_target 0, weight 1e-12, bbox term
    -log(1e-6) * 1e-12 per positive with no IoU gradient (the aug MSE gradient stays), IoU-branch BCE against 0"""
    case = Case(SMALL, R.rpn_cfg(reg_mode=reg_mode, with_aug=with_aug))
    for i, s in enumerate(case.spots(3)):
        enc = [-0.1, -0.1, 0.2, 0.2]
        d = [[5.0, -0.13, 0.23, 0.17], [-0.07, -4.0, 0.1, 0.3], [3.0, 3.0, 0.26, 0.15]][i]   # no coordinate near the encoding's
        case.add_pos(s, case.gt_for_enc(s, enc), d)
    r64 = case.ref(torch.float64)
    assert (case.cat(r64['det'], 'iou_target') == 0).all() and r64['tot'][0] == 3 and r64['tot'][1] == 0
    assert (case.cat(r64['det'], 'weight') == 1e-12).all()
    reg = _per_anchor(r64['dy'])[:, :, 1:5]
    if reg_mode == 0:
        closed = 3 * -math.log(1e-6) * 1e-12
        if not with_aug:
            assert abs(r64['l3'][1].item() - closed) <= 1e-12 * closed and (reg == 0).all()
        else:
            assert r64['l3'][1].item() > closed and (reg.abs().amax(2) > 0).sum() == 3
    k, _, _ = _compare(f'disjoint[{reg_mode},{int(with_aug)}]', case, r64)
    if reg_mode == 0 and not with_aug:
        assert (_per_anchor(k['dy'])[:, :, 1:5] == 0).all()


# ---- 3
@pytest.mark.parametrize('with_aug', [False, True])
def test_rpn_dw_dh_clamps(with_aug):
    """dw / dh just inside, just outside and far outside +-max_ratio, independently: through a clamped component the
    IoU gradient is exactly 0 while the aug MSE gradient is still there"""
    case = Case(BIG, R.rpn_cfg(reg_mode=0, with_aug=with_aug))
    vals = [LIMIT - 0.01, LIMIT + 0.01, 8.0, -(LIMIT - 0.01), -(LIMIT + 0.01), -8.0]
    spots = case.spots(12)
    for i, s in enumerate(spots):
        d = [0.03, -0.02, 0.13, -0.07]
        d[2 + i // 6] = vals[i % 6]
        case.add_pos(s, case.gt_for_enc(s, [0.0, 0.0, 0.1, -0.1]), d)
    r64, r32 = case.ref(torch.float64), case.ref(torch.float32)
    for key in ('dw', 'dh'):
        v64, v32 = case.cat(r64['det'], key), case.cat(r32['det'], key).double()
        assert ((v64.abs() > LIMIT) == (v32.abs() > LIMIT)).all()               # both precisions on the same side
        for sign in (1, -1):
            inside = (sign * v64 > LIMIT - 0.1) & (sign * v64 < LIMIT)
            assert inside.sum() == 1 and (sign * v64 > LIMIT).sum() == 2
    assert (case.cat(r64['det'], 'iou_target') > 1e-6).all()
    reg = torch.stack([_per_anchor(r64['dy'])[case.row0[l] + b * case.hw[l] + cell, a, 1:5] for l, b, cell, a in spots])
    clamped = torch.stack([case.cat(r64['det'], 'dw').abs() > LIMIT, case.cat(r64['det'], 'dh').abs() > LIMIT], 1)
    order = _det_order(case, r64['det'], spots)
    clamped = clamped[order]
    assert (reg.abs().amax(1) > 0).all()
    assert ((reg[:, 2:] == 0) == clamped).all() if not with_aug else (reg[:, 2:] != 0).all()
    _compare(f'clamps[aug={int(with_aug)}]', case, r64, r32)


def _det_order(case, det, spots):
    """index of every spot in the concatenated per-level detail tensors"""
    keys, off = {}, 0
    for l, d in enumerate(det):
        for j, (r, a) in enumerate(zip(d['rows'].tolist(), d['a'].tolist())):
            keys[(l, r, a)] = off + j
        off += len(d['rows'])
    return torch.tensor([keys[(l, b * case.hw[l] + cell, a)] for l, b, cell, a in spots])


def test_rpn_target_box_clamp_in_ciou_mode():
    """reg_mode 1: the loss sees raw deltas, the size clamp applies only to the two decoded boxes of iou_target:
    gt / anchor size ratios beyond 1000 / 16 and below 16 / 1000, predictions on both sides of the clamp"""
    case = Case(SMALL, R.rpn_cfg(reg_mode=1))
    encs = [[0.0, 0.0, math.log(80), 0.1], [0.0, 0.0, 0.1, math.log(80)], [0.0, 0.0, -math.log(80), 0.0],
            [0.0, 0.0, 0.2, -math.log(80)], [0.1, 0.0, math.log(80), math.log(70)]]
    for s, enc in zip(case.spots(5), encs):
        case.add_pos(s, case.gt_for_enc(s, enc), [enc[0] + 0.002, enc[1] - 0.002, enc[2] - 0.4, enc[3] + 0.3])
    r64, r32 = case.ref(torch.float64), case.ref(torch.float32)
    enc = case.cat(r64['det'], 'enc')
    assert ((enc[:, 2] > LIMIT).sum() >= 2 and (enc[:, 3] > LIMIT).sum() >= 2 and (enc[:, 2] < -LIMIT).sum() >= 1 and
            (enc[:, 3] < -LIMIT).sum() >= 1)
    assert (case.cat(r64['det'], 'dw').abs() > LIMIT).sum() >= 1 and (case.cat(r64['det'], 'dw').abs() < LIMIT).sum() >= 1
    assert (case.cat(r64['det'], 'iou_target') > 0.01).all()            # no weight at its floor
    _compare('ciou target clamp', case, r64, r32)


# ---- 4
def test_rpn_ciou_alpha_branch():
    """CIoU on raw deltas with an encoding that reads as a proper box and deltas near it: delta-box IoU > 0.5 (alpha,
    g_v, the aspect gradient live), IoU in (0.45, 0.5] (alpha 0 on the far side), deltas of negative "width" (the w / h /
    cw / ch clamps at 0) and one ci < -1 (the final clamp, no gradient)"""
    case = Case(BIG, R.rpn_cfg(reg_mode=1))
    spots = case.spots(20)
    _generic_positives(case, 10, seed=4)
    base = [-0.1, -0.1, 0.2, 0.2]
    for s, (k_, dl) in zip(spots[10:13], [(2, 0.25), (3, 0.27), (2, 0.29)]):             # IoU ~ 0.3 / (0.3 + dl)
        d = [base[0] + 0.012, base[1] - 0.011, base[2] + 0.013, base[3] - 0.012]       # off every tie by >> fp32 rounding
        d[k_] += dl
        case.add_pos(s, case.gt_for_enc(s, base), d)
    case.add_pos(spots[13], case.gt_for_enc(spots[13], base), [0.2, -0.12, -0.13, 0.25])  # negative width
    case.add_pos(spots[14], case.gt_for_enc(spots[14], base), [-0.12, 0.2, 0.25, -0.13])  # negative height
    q = [0.3, -0.1, -0.2, 0.2]                                                           # the encoding itself inside out on x
    case.add_pos(spots[15], case.gt_for_enc(spots[15], q), [0.55, -0.12, -0.4, 0.25])    # cw clamped, ch not
    q = [0.3, 0.3, -0.2, -0.2]
    case.add_pos(spots[16], case.gt_for_enc(spots[16], q), [0.5, 0.55, -0.4, -0.4])      # cw and ch clamped: c2 = eps
    r64, r32 = case.ref(torch.float64), case.ref(torch.float32)
    iou, alpha, ci = (case.cat(r64['det'], k_) for k_ in ('delta_iou', 'alpha', 'ci'))
    assert (iou > 0.5).sum() >= 8 and ((iou > 0.5) == (alpha > 0)).all() and (alpha > 1e-4).sum() >= 8
    assert ((iou > 0.45) & (iou <= 0.5)).sum() >= 3
    assert (ci < -1).sum() >= 1 and ((ci > -1) & (ci < 1)).sum() >= 15
    dd = torch.cat([case.y[case.row0[l]:case.row0[l + 1], A:5 * A].reshape(-1, A, 4)[d_['rows'], d_['a']].double() *
                    case.scales[l].double() for l, d_ in enumerate(r64['det'])])
    assert ((dd - case.cat(r64['det'], 'enc')).abs() > 1e-3).all()       # no max / min of the loss near a tie
    i32 = case.cat(r32['det'], 'delta_iou').double()
    assert ((i32 > 0.5) == (iou > 0.5)).all() and (case.cat(r32['det'], 'ci').double() < -1).sum() == (ci < -1).sum()
    raw = torch.cat([case.y[case.row0[l]:case.row0[l + 1], A:5 * A].reshape(-1, A, 4)[d['rows'], d['a']]
                     for l, d in enumerate(r64['det'])])
    assert (raw[:, 2] < raw[:, 0]).sum() >= 3 and (raw[:, 3] < raw[:, 1]).sum() >= 2
    _compare('ciou alpha', case, r64, r32)


# ---- 5
@pytest.mark.parametrize('reg_mode', [0, 1])
@pytest.mark.parametrize('iou_gamma', [0.5, 1.0, 2.0, 0.7])
def test_rpn_weight_exponent(iou_gamma, reg_mode):
    """iou_target ** gamma as sqrt, identity, square and (0.7) the general powf path"""
    case = Case(SMALL, R.rpn_cfg(reg_mode=reg_mode, iou_gamma=iou_gamma))
    _generic_positives(case, 8, seed=5)
    r64 = case.ref(torch.float64)
    w, t = case.cat(r64['det'], 'weight'), case.cat(r64['det'], 'iou_target')
    assert (t > 0.3).all() and (t < 1).all() and torch.allclose(w, t ** iou_gamma, rtol=1e-14)
    _compare(f'exponent[{iou_gamma},{reg_mode}]', case, r64)


# ---- 6
@pytest.mark.parametrize('cls_mode,pos_weight', [(0, 0.0), (0, 2.0), (1, 0.0), (2, 0.0)])
def test_rpn_classification_modes(cls_mode, pos_weight):
    """focal (with and without pos_weight) and both varifocal forms on the logit grid [-12, 12] (0 included) over
    positives, negatives and ignored anchors: focal skips ignored anchors (exactly zero loss and gradient), varifocal
    is called without label weights and counts them as negatives"""
    case = Case(SMALL, R.rpn_cfg(cls_mode=cls_mode, pos_weight=pos_weight, focal_alpha=0.25 if cls_mode == 0 else 0.75))
    _generic_positives(case, 25, seed=6)
    cl = case.cls_in_gt_order()
    for sel in (case.gt_inds == -1, case.gt_inds == 0):                   # the whole grid on ignored anchors, on negatives
        cl[sel] = GRID[torch.arange(int(sel.sum())) % 25]
    case.cls_in_gt_order(cl)
    # ... and on positives, in the rotation of the grid that keeps sigmoid(x) clear of the positive's own iou_target:
    # (sigmoid(x) - t) of the varifocal gradient cancels there
    t = case.cat(case.ref(torch.float64)['det'], 'iou_target')[_det_order(case, case.ref(torch.float64)['det'], case.pos)]
    shift = next(k_ for k_ in range(25) if ((torch.sigmoid(GRID.double().roll(k_)) - t).abs() > 0.02).all())
    for i, s in enumerate(case.pos):
        case.set_cls(s, GRID.roll(shift)[i].item())
    r64 = case.ref(torch.float64)
    ign = (case.gt_inds == -1)
    assert ign.sum() > 20 and (case.gt_inds == 0).sum() > 100 and r64['tot'][0] == 25
    dcls64 = torch.cat([r64['dy'][case.row0[l]:case.row0[l + 1], :A].reshape(2, -1) for l in range(case.L)], 1)
    assert (dcls64[ign] == 0).all() if cls_mode == 0 else (dcls64[ign] != 0).all()
    cl = case.cls_in_gt_order()
    for v in GRID.tolist():
        for sel in (ign, case.gt_inds == 0, case.gt_inds > 0):
            assert (cl[sel] == v).any()
    k, _, _ = _compare(f'cls[{cls_mode},{pos_weight}]', case, r64)
    if cls_mode == 0:
        dcls = torch.cat([k['dy'][case.row0[l]:case.row0[l + 1], :A].reshape(2, -1) for l in range(case.L)], 1)
        assert (dcls[ign] == 0).all()
    if pos_weight > 0:
        case0 = Case(SMALL, R.rpn_cfg(cls_mode=0, pos_weight=0.0))
        assert r64['l3'][0] > 1.001 * R.rpn_loss_ref(case.y.double(), case.scales.double(), case.gt_inds, case.gts,
                                                    case.offs, case.sizes, case.strides, case.base, A, case0.cfg,
                                                    torch.float64)[0][0]


# ---- 7
def test_rpn_saturated_logits():
    """Logits of +-30, +-60, +-100 on positives, negatives and ignored anchors (well clear of |x| ~ 16.6, where one ulp
    of sigmoid flips 1 - p between 0 and 2^-24).  Here the true float64 value is NOT the target: the closed form of the
    focal term, log(max(1 - p, FLT_MIN)) with p = sigmoid(x) rounded to fp32, saturates at -log(FLT_MIN) = 87.3 by design
    (it is the native op of the reference), where the mathematical value is |x|.  The classification loss and dcls are
    therefore compared with the FLOAT32 run of the restatement on the CPU, which carries the same saturation: at these
    logits p is exactly 0, exactly 1 or far from both, every factor is exact or one library call, so the bound is the
    ULPS floor alone (K * err32 would be vacuous: err32 is of order 1 here).  Every output must be finite; the box and
    IoU-branch terms of the same call are held to float64 as everywhere else."""
    case = Case(SMALL, R.rpn_cfg(cls_mode=0))
    _generic_positives(case, 12, seed=7)
    sat = [30.0, -30.0, 60.0, -60.0, 100.0, -100.0]
    for i, s in enumerate(case.pos):
        case.set_cls(s, sat[i % 6])
    others = [s for s in case.spots(60) if s not in case.pos]
    for i, s in enumerate(others[:24]):
        case.set_cls(s, sat[i % 6])
        case.mark(s, 0 if i < 12 else -1)
    r64, r32 = case.ref(torch.float64), case.ref(torch.float32)
    assert torch.isfinite(r32['l3']).all() and torch.isfinite(r32['dy']).all()
    assert r32['l3'][0] > 1.05 * r64['l3'][0]                 # the saturation is in play: fp32 is not near float64
    k, _, _ = _compare('saturated', case, r64, r32, cls_vs_fp32=True)
    assert torch.isfinite(k['l3']).all() and torch.isfinite(k['pl']).all() and torch.isfinite(k['dy']).all()


# ---- 8
@pytest.mark.parametrize('variant', ['no_gt', 'no_positive', 'small_iou_sum', 'one_image_empty'])
@pytest.mark.parametrize('reg_mode', [0, 1])
def test_rpn_normalisers(variant, reg_mode):
    """max(num_pos, 1) and max(sum iou_target, 1): no gt at all (the NULL gts pointer), gt without a positive anchor, two
    positives whose iou_target sum stays below 1, one image of the batch without gt"""
    case = Case(SMALL, R.rpn_cfg(reg_mode=reg_mode))
    if variant == 'no_positive':
        case.gt_lists = [[[4., 4., 20., 20.]], [[8., 0., 30., 16.], [0., 0., 8., 8.]]]
    elif variant == 'small_iou_sum':
        for s, d in zip(case.spots(2), ([0.9, -0.13, 0.23, 0.17], [-0.12, 0.8, 0.3, 0.1])):
            case.add_pos(s, case.gt_for_enc(s, [-0.1, -0.1, 0.2, 0.2]), d)
    elif variant == 'one_image_empty':
        spots = [s for s in case.spots(16) if s[1] == 1][:5]
        gen = torch.Generator().manual_seed(8)
        for s in spots:
            d = (torch.tensor([-0.1, -0.1, 0.2, 0.2]) + (torch.rand(4, generator=gen) - 0.5) * 0.1).tolist()
            case.add_pos(s, case.gt_for_enc(s, [-0.1, -0.1, 0.2, 0.2]), d)
    r64 = case.ref(torch.float64)
    if variant in ('no_gt', 'no_positive'):
        assert case.offs[-1] == (0 if variant == 'no_gt' else 3) and r64['tot'].tolist() == [0, 0]
        assert r64['l3'][1] == 0 and r64['l3'][2] == 0 and r64['l3'][0] > 0 and (r64['ds'] == 0).all()
    elif variant == 'small_iou_sum':
        assert r64['tot'][0] == 2 and 0 < r64['tot'][1] < 1 and (case.cat(r64['det'], 'iou_target') > 0.02).all()
    else:
        assert case.offs == [0, 0, 5] and r64['tot'][0] == 5 and r64['tot'][1] > 1
    _compare(f'normalisers[{variant},{reg_mode}]', case, r64)


# ---- 9 + 10
@pytest.mark.parametrize('reg_mode', [0, 1])
def test_rpn_outputs_complete_block_tail_and_upstream_gradient(reg_mode):
    """a level that crosses 256 anchors (block tail, second workgroup) with positives in the tail, a level without any
    positive (d/dScale exactly 0), non-trivial means / stds, non-unit loss weights and the upstream gradient
    (3, 0.5, -2): every element of dy finite, padding columns exactly 0 on every row (checked for every case of this
    module in _compare), d/dScale == sum(dreg * raw) of the reference per level"""
    cfg = R.rpn_cfg(reg_mode=reg_mode, means=(0.01, -0.02, 0.03, 0.04), stds=(0.1, 0.1, 0.2, 0.2), lw_cls=1.5, lw_bbox=2.0,
                    lw_aug=0.5, lw_iou=0.7, iou_gamma=0.7)
    case = Case(BIG, cfg, g3=(3.0, 0.5, -2.0))
    gen = torch.Generator().manual_seed(9)
    spots = [(0, 1, 14, a) for a in (0, SQUARE, 8)] + [(0, 0, 0, 0), (0, 0, 7, 4), (0, 1, 3, 5), (0, 1, 13, 8)]
    assert all((b * 15 + cell) * A + a >= 256 for _, b, cell, a in spots[:3])            # the tail workgroup
    for s in spots:
        enc = (torch.tensor([-1.0, -1.0, 1.0, 1.0], dtype=torch.float64) +
               (torch.rand(4, generator=gen, dtype=torch.float64) - 0.5))
        d = enc + (torch.rand(4, generator=gen, dtype=torch.float64) - 0.5) * 0.8
        case.add_pos(s, case.gt_for_enc(s, enc.tolist()), d.tolist())
    r64 = case.ref(torch.float64)
    assert len(r64['det'][1]['rows']) == 0 and r64['ds'][1] == 0 and r64['ds'][0] != 0
    assert (case.cat(r64['det'], 'iou_target') > 0.2).all()
    k, _, _ = _compare(f'complete[{reg_mode}]', case, r64)
    assert k['ds'][1] == 0 and (k['dy'][:, 6 * A:] == 0).all()


def test_rpn_rows_of_ignored_anchors_only():
    """rows whose nine anchors are all ignored still get their padding columns and their 54 gradients written (zeros)"""
    case = Case(SMALL, R.rpn_cfg(reg_mode=0))
    _generic_positives(case, 6, seed=10)
    free = [(b, lo) for lo in range(0, case.start[-1], A) for b in range(2) if (case.gt_inds[b, lo:lo + A] <= 0).all()]
    for b, lo in free[::7][:4]:
        case.gt_inds[b, lo:lo + A] = -1
    whole = sum(int((case.gt_inds[b, s_:s_ + A] == -1).all()) for b in range(2) for s_ in range(0, case.start[-1], A))
    assert whole >= 2
    k, r64, _ = _compare('ignored rows', case)
    rows = torch.cat([(case.gt_inds[:, case.start[l]:case.start[l + 1]].reshape(2 * case.hw[l], A) == -1).all(1)
                      for l in range(case.L)])
    assert rows.sum() == whole and (k['dy'][rows] == 0).all()


# ----------------------------------------------------------------------------- boosting loss
BETA = float(np.float32(1 / 9))
OPTS = [dict(agnostic=False, reg_norm='bbox_num', plain=False, beta=0.0, gamma=0.5, alpha=0.0, quality=False),
        dict(agnostic=True, reg_norm='mean', plain=True, beta=BETA, gamma=0.3, alpha=1.5, quality=True),
        dict(agnostic=False, reg_norm='mean', plain=True, beta=BETA, gamma=0.5, alpha=1.5, quality=False),
        dict(agnostic=True, reg_norm='bbox_num', plain=False, beta=0.0, gamma=0.3, alpha=0.0, quality=True),
        dict(agnostic=False, reg_norm='bbox_num', plain=True, beta=0.0, gamma=0.5, alpha=0.0, quality=True),
        dict(agnostic=False, reg_norm='mean', plain=False, beta=BETA, gamma=0.3, alpha=1.5, quality=False)]


def _boost_inputs(n, C, seed, agnostic):
    """rows 0..: [fg, prior 0, box differences at +-beta / 0 / just above] [bg, prior 1] [fg, differences just below
    beta / large] [logit 80 on the label] [logit 80 off the label] [all -80 but the label] [arg-max tie low / high]..."""
    gen = torch.Generator().manual_seed(seed)
    nc = C + 1
    cls = torch.randn(n, nc, generator=gen) * 2
    labels = torch.randint(0, nc, (n,), generator=gen)
    labels[2::3] = C
    pri = torch.rand(n, generator=gen) * 0.9 + 0.05
    iou = torch.rand(n, generator=gen)
    bb = torch.randn(n, 4 if agnostic else 4 * C, generator=gen)
    tgt = torch.randn(n, 4, generator=gen)
    hi, lo = (3, 67) if C == 80 else (1, 3)
    up, dn = np.nextafter(np.float32(BETA), np.float32(1)), np.nextafter(np.float32(BETA), np.float32(0))
    knee = [[BETA, -BETA, 0.0, float(up)], [float(dn), 0.5, -0.5 * BETA, -2.0]]
    special = {}
    if n >= 3:
        labels[0], pri[0] = 1, 0.0
        labels[1], pri[1] = C, 1.0
        labels[2] = 0
        for r, kn in ((0, knee[0]), (2, knee[1])):
            tgt[r] = 0.0                                               # the difference is the prediction itself: exact
            c0 = 0 if agnostic else 4 * int(labels[r])
            bb[r, c0:c0 + 4] = torch.tensor(kn)
    if n >= 5:
        cls[3] = torch.randn(nc, generator=gen)
        labels[3] = 2
        cls[3, 2] = 80.0                                               # label on the max
        cls[4] = torch.randn(nc, generator=gen)
        labels[4] = C
        cls[4, 1] = 80.0                                               # label off the max
    if n >= 7:
        cls[5] = -80.0 + torch.randn(nc, generator=gen)
        labels[5] = 0
        cls[5, 0] = 3.0
        cls[6] = torch.randn(nc, generator=gen).clamp(max=2.0)
        cls[6, hi] = cls[6, lo] = 5.0                                  # tie across the two lane rounds (C = 80)
        labels[6] = lo                                                 # the higher index holds the label: counted wrong
        special['tie_wrong'] = 6
    if n >= 260:
        for r, (i_, j_, lab) in {100: (hi, lo, hi), 101: (0, C, C), 102: (0, C, 0), 103: (hi, lo, lo)}.items():
            cls[r] = torch.randn(nc, generator=gen).clamp(max=2.0)
            cls[r, i_] = cls[r, j_] = 6.0
            labels[r] = lab
            assert int(torch.argmax(cls[r])) == min(i_, j_)            # torch counts the first of the tied maxima
        special['ties'] = {100: True, 101: False, 102: True, 103: False}
    return cls, bb, labels, pri, iou, tgt, special


def _boost_compare(tag, cls, bb, labels, pri, iou, tgt, C, o):
    cfg = R.boost_cfg(gamma=o['gamma'], alpha=o['alpha'], iou_gamma=0.7 if o['quality'] else 0.0, lw_cls=2.0, lw_bbox=1.5,
                      reg_norm=o['reg_norm'], agnostic=o['agnostic'], plain=o['plain'], beta=o['beta'])
    io = iou if o['quality'] else None
    ref = {}
    for dt in (torch.float64, torch.float32):
        c1, b1 = cls.to(dt).requires_grad_(), bb.to(dt).requires_grad_()
        o3 = R.boost_loss_ref(c1, b1, labels, pri, io, tgt, C, cfg, dt)
        gc, gb = torch.autograd.grad(3.0 * o3[0] + 0.5 * o3[1], [c1, b1], allow_unused=True)
        ref[dt] = (o3.detach(), gc, torch.zeros_like(b1) if gb is None else gb)
    assert torch.isfinite(ref[torch.float64][0]).all()
    c2, b2 = cls.to(DEV).requires_grad_(), bb.to(DEV).requires_grad_()
    out3 = train_ops.boost_loss(c2, b2, labels.to(DEV), pri.to(DEV), tgt.to(DEV), C, o['gamma'], alpha=o['alpha'],
                                ious=None if io is None else io.to(DEV), iou_gamma=cfg['iou_gamma'], loss_cls_weight=2.0,
                                loss_bbox_weight=1.5, reg_norm=o['reg_norm'], reg_class_agnostic=o['agnostic'],
                                plain_label_weights=o['plain'], smooth_l1_beta=o['beta'])
    junk = torch.full_like(b2, float('nan'))
    del junk
    gc, gb = torch.autograd.grad(3.0 * out3[0] + 0.5 * out3[1], [c2, b2])
    r64, r32 = ref[torch.float64], ref[torch.float32]
    _check(f'{tag} out3', out3, r64[0], r32[0])
    _check(f'{tag} dcls', gc, r64[1], r32[1], r64[1].abs().amax(1, keepdim=True))
    _check(f'{tag} dbbox', gb, r64[2], r32[2], r64[2].abs().amax(1, keepdim=True))
    return out3.detach().cpu(), gc.cpu(), gb.cpu(), r64


@pytest.mark.parametrize('opt', range(len(OPTS)))
@pytest.mark.parametrize('C', [4, 80])
@pytest.mark.parametrize('n', [1, 3, 5, 7, 260])
def test_boost_loss_edges(n, C, opt):
    """row counts around the 4-rows-per-workgroup packing, 5- and 81-wide rows, both head layouts, both normalisations
    of either term, L1 and smooth-L1 with differences at exactly +-beta, 0 and either side, both weight exponents,
    alpha, the quality factor, priors of exactly 0 and 1, logits of magnitude 80 and arg-max ties counted as
    torch.argmax counts them"""
    o = OPTS[opt]
    cls, bb, labels, pri, iou, tgt, special = _boost_inputs(n, C, 100 * n + C + opt, o['agnostic'])
    out3, gc, gb, r64 = _boost_compare(f'boost[{n},{C},{opt}]', cls, bb, labels, pri, iou, tgt, C, o)
    assert out3[2].item() == pytest.approx(100.0 * (cls.argmax(1) == labels).sum().item() / n, rel=1e-6)
    if 'ties' in special:
        for r, hit in special['ties'].items():
            assert (int(torch.argmax(cls[r])) == int(labels[r])) == hit
    if n >= 3:
        assert (gc[1] == 0).all() and (r64[1][1] == 0).all()                  # prior exactly 1: weight exactly 0
    if not o['agnostic']:                                                     # only the label's four columns get a gradient
        keep = torch.zeros(n, 4 * C, dtype=torch.bool)
        for r in range(n):
            if labels[r] < C:
                keep[r, 4 * int(labels[r]):4 * int(labels[r]) + 4] = True
        assert (gb[~keep] == 0).all()
    else:
        assert (gb[labels == C] == 0).all()


@pytest.mark.parametrize('reg_norm', ['bbox_num', 'mean'])
@pytest.mark.parametrize('agnostic', [False, True])
@pytest.mark.parametrize('n,C', [(5, 4), (7, 80)])
def test_boost_loss_all_background(n, C, agnostic, reg_norm):
    """n_pos = 0: loss_bbox exactly 0, dbbox all exact zeros, nothing NaN, under both normalisations"""
    cls, bb, labels, pri, iou, tgt, _ = _boost_inputs(n, C, 7, agnostic)
    labels[:] = C
    o = dict(OPTS[0], agnostic=agnostic, reg_norm=reg_norm, beta=BETA)
    out3, gc, gb, _ = _boost_compare(f'boost bg[{n},{C},{int(agnostic)},{reg_norm}]', cls, bb, labels, pri, iou, tgt, C, o)
    assert out3[1].item() == 0 and (gb == 0).all() and torch.isfinite(out3).all() and torch.isfinite(gc).all()


@pytest.mark.parametrize('plain', [False, True])
def test_boost_loss_one_row_with_weight(plain):
    """all rows but one have prior exactly 1 (weight exactly 0): plain divides by max(#{w > 0}, 1) = 1, not by n"""
    n, C = 7, 4
    cls, bb, labels, pri, iou, tgt, _ = _boost_inputs(n, C, 11, False)
    pri[:] = 1.0
    pri[4] = 0.36
    o = dict(OPTS[0], plain=plain, gamma=0.5)
    out3, gc, gb, r64 = _boost_compare(f'boost one row[{int(plain)}]', cls, bb, labels, pri, iou, tgt, C, o)
    ce4 = 2.0 * torch.nn.functional.cross_entropy(cls[4:5].double(), labels[4:5]).item()
    want = ce4 * 0.8 if plain else 2.0 * torch.nn.functional.cross_entropy(cls.double(), labels, reduction='sum').item() / n
    assert r64[0][0].item() == pytest.approx(want, rel=1e-6)        # (0.36 is not an fp32 number)
    assert (gc[torch.arange(n) != 4] == 0).all() and (gc[4] != 0).all()
