"""GPU tests of the GFL baseline (csrc/gfl_head.hip, GFLHead, GFL).

Against the fixture g30_gfl.npz (tests/golden/make_golden_gfl.py; the reference's fp32 run): labels and kept order exact,
boxes and scores within the 2e-4 of g28's / g29's end-to-end cases (the fixture's reference run is within 5e-5 of its own
float64 run), train losses within rtol 2e-3 / atol 1e-4 as tests/test_atss_gpu.py holds its own.
Against float64 (tests/gfl_ref64.py): bounds stated where used, derived from the fp32 arithmetic of the kernels (eps = 2^-23; an
addition, product or division rounds to eps / 2, expf / logf / powf are counted as 2 eps); none is tuned to what the kernels
give.  Preconditions on the inputs (distances to thresholds and bin edges) are asserted."""
import math
import os
import re

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import build_detector, build_head, ops, train_ops
from brcnn.config import ConfigDict
from tests import atss_ref64 as RA
from tests import gfl_inputs as gi
from tests import gfl_ref64 as R
from tests import util

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G = os.path.join(os.path.dirname(__file__), 'golden', 'g30_gfl.npz')
EPS32 = float(np.finfo(np.float32).eps)
L = len(gi.SIZES)
N_L = [h * w for h, w in gi.SIZES]
STARTS = np.cumsum([0] + N_L)


@pytest.fixture(scope='module')
def gold():
    return {k: v for k, v in np.load(G, allow_pickle=False).items()}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def build(C=4, training=False, **over):
    head = build_head(ConfigDict(gi.head_cfg(C, **over))).train(training)
    with torch.no_grad():
        for s, v in zip(head.scales, gi.SCALES):
            s.scale.fill_(v)
    return head.to(DEV)


def base_table():
    half = [s * gi.OCTAVE / 2 for s in gi.STRIDES]
    return ops.atss_base_anchors([torch.tensor([[-h, -h, h, h]]) for h in half])


def scales_dev():
    return torch.tensor(gi.SCALES, dtype=torch.float32, device=DEV)


def make_rows(cls, raw, reg_max=16, wide=False):
    """per-level (B, c, h, w) RAW outputs as the kernels' (A, R) rows.  Plain: the widths GFLHead.forward_rows leaves (padded
    to 8 columns: 68 -> 72, 32 -> 32, 20 -> 24, zeros).  `wide`: 32 / 96 columns with the class logits at column 3 and the
    box logits at column 5, every other column holding 7.0 -- nothing but the named columns may be read"""
    a0, r0 = R._rows(cls).float(), R._rows(raw).float()
    C, W = a0.shape[1], r0.shape[1]
    assert W == 4 * (reg_max + 1)
    if wide:
        a, r = torch.full((a0.shape[0], 32), 7.0), torch.full((a0.shape[0], 96), 7.0)
        a[:, 3:3 + C], r[:, 5:5 + W] = a0, r0
        offs = (3, 5)
    else:
        a, r = torch.zeros(a0.shape[0], C + (-C % 8)), torch.zeros(a0.shape[0], W + (-W % 8))
        a[:, :C], r[:, :W] = a0, r0
        offs = (0, 0)
    a, r = a.to(DEV).contiguous(), r.to(DEV).contiguous()
    return a, r, ops.GflLayout(a, r, C, reg_max, *offs)


def test_the_library_exports_every_gfl_entry_of_the_header():
    from brcnn import lib
    from brcnn.registry import DETECTORS, HEADS, LOSSES
    header = open(os.path.join(gi.ROOT, 'include', 'brcnn_hip.h')).read()
    declared = sorted(set(re.findall(r'^(?:int|size_t) (brcnn_gfl_\w+)\(', header, re.M)))
    assert declared == ['brcnn_gfl_decode_levels', 'brcnn_gfl_loss_backward', 'brcnn_gfl_loss_finalize',
                        'brcnn_gfl_loss_forward', 'brcnn_gfl_loss_workspace_bytes']
    for name in declared:
        assert name in lib.SIGNATURES and hasattr(lib.load(), name), name
    assert HEADS.get('GFLHead') is not None and DETECTORS.get('GFL') is not None and LOSSES.get('QualityFocalLoss') is not None


# ------------------------------------------------------------------------------------------- test time
def _decode(a, r, layout, inds, metas, rescale, thr, scales=None):
    B = len(metas)
    shp = torch.tensor([m['img_shape'][:2] for m in metas], dtype=torch.float32, device=DEV)
    sf = torch.tensor(np.stack([m['scale_factor'] for m in metas]), dtype=torch.float32, device=DEV) if rescale else None
    out = ops.gfl_decode_levels(inds, a, r, layout, scales_dev() if scales is None else scales, gi.SIZES, gi.STRIDES, base_table(),
                                shp, sf, thr)
    assert out[0].shape[0] == B
    return [t.cpu() for t in out]


DECODE_CASES = [(4, 16, False, False), (1, 7, False, True), (3, 4, True, True), (4, 16, True, True), (3, 7, True, False)]


@pytest.mark.parametrize('C,reg_max,wide,rescale', DECODE_CASES)
def test_candidates_against_float64(C, reg_max, wide, rescale):
    """score, top-k and decode of seeded outputs against the float64 restatement.  Scores: sigmoid is 4 roundings on positive
    values, 4 eps relative.  Boxes: `gfl_ref64.box_bound` per candidate (derived there, to first order in eps), doubled for
    the terms of higher order.  Labels, valid and n_valid exact: no class score lies within 1e-6 of score_thr
    (asserted)."""
    K, thr = 50, 0.05
    cls, raw = gi.head_outputs(60 + C + reg_max, C, reg_max=reg_max)
    metas = gi.metas()
    a, r, layout = make_rows(cls, raw, reg_max, wide)
    ref = R.candidates(cls, raw, gi.SCALES, gi.SIZES, gi.STRIDES, [m['img_shape'] for m in metas],
                       [m['scale_factor'] for m in metas] if rescale else None, reg_max)
    scored = ops.gfl_score(a, layout)
    want_s = torch.cat([x[0].reshape(-1) for x in ref])
    assert scored.shape == want_s.shape and ((scored.cpu().double() - want_s).abs() <= 4 * EPS32 * want_s).all()
    split, r0 = [], 0
    for n in N_L:
        split.append(scored[r0:r0 + 2 * n].view(2, n))
        r0 += 2 * n
    picked = ops.rpn_topk(split, K)
    inds = [p[1] for p in picked]
    boxes, scores, labels, valid, n_valid = _decode(a, r, layout, inds, metas, rescale, thr)
    Tn = sum(i.shape[1] for i in inds)
    assert boxes.shape == (2, Tn * C, 4) and [i.shape[1] for i in inds] == [50, 50, 24, 6, 2]
    worst = 0.0
    for b in range(2):
        wb, ws, we = [], [], []
        for l in range(L):
            idx = inds[l][b].cpu()
            # the picks are the level's K best float64 scores wherever the gap at the boundary exceeds the scores' error
            if N_L[l] > K:
                order = ref[l][0][b].sort(descending=True)[0]
                if order[K - 1] - order[K] > 1e-6:
                    assert set(idx.tolist()) == set(ref[l][0][b].sort(descending=True)[1][:K].tolist()), (b, l)
            wb.append(ref[l][2][b][idx])
            ws.append(ref[l][1][b][idx])
            we.append(ref[l][3][b][idx])
        wb, ws, we = torch.cat(wb), torch.cat(ws), torch.cat(we)
        assert ((ws - thr).abs() > 1e-6).all()
        assert torch.equal(labels[b], torch.arange(C).repeat(Tn))
        assert torch.equal(valid[b], (ws > thr).reshape(-1)) and n_valid[b].item() == int((ws > thr).sum())
        assert ((scores[b].double() - ws.reshape(-1)).abs() <= 4 * EPS32 * ws.reshape(-1)).all()
        err = (boxes[b].double().view(Tn, C, 4) - wb[:, None, :]).abs().amax((1, 2))
        worst = max(worst, float((err / we).max()))
        assert (err <= 2 * we).all(), (b, float(err.max()), float(we.max()))
        assert torch.equal(boxes[b].view(Tn, C, 4)[:, 0], boxes[b].view(Tn, C, 4)[:, C - 1])       # one box per pick
    print('largest box error / its bound', worst, 'bound up to', float(we.max()), 'px')
    assert n_valid.sum().item() > 20


def _one_cell_rows(C=2, reg_max=16):
    """all-zero logits (class logit -9): rows to plant single cells in"""
    cls = [torch.full((2, C, h, w), -9.0) for h, w in gi.SIZES]
    raw = [torch.zeros(2, 4 * (reg_max + 1), h, w) for h, w in gi.SIZES]
    return cls, raw


def test_hand_made_decode_cases():
    n, metas = 17, gi.metas()
    cls, raw = _one_cell_rows()
    # (1) one-hot distributions: 1000 at bins (3, 2, 5, 4) of cell (8, 12) of level 0, centre (96, 64), stride 8, scale 1.0
    for side, k in enumerate((3, 2, 5, 4)):
        raw[0][0, side * n + k, 8, 12] = 1000.0
    cls[0][0, 1, 8, 12] = 2.0
    # (2) logits of +-80 after the scale (0.9 * 88.9 = 80.01) at cell (2, 3) of level 1, centre (48, 32), stride 16
    raw[1][0, :, 2, 3] = torch.tensor([88.9, -88.9] * (2 * n))
    cls[1][0, 0, 2, 3] = 2.0
    # (3) a box clipped at the border: bin 16 on every side at cell (0, 5) of level 2 (centre (160, 0), stride 32, scale 1.1)
    for side in range(4):
        raw[2][0, side * n + 16, 0, 5] = 1000.0
    cls[2][0, 0, 0, 5] = 2.0
    a, r, layout = make_rows(cls, raw)
    inds = [torch.tensor([[8 * 24 + 12], [0]], device=DEV), torch.tensor([[2 * 12 + 3], [0]], device=DEV),
            torch.tensor([[5], [0]], device=DEV), torch.zeros(2, 1, dtype=torch.long, device=DEV),
            torch.zeros(2, 1, dtype=torch.long, device=DEV)]
    boxes, scores, labels, valid, n_valid = _decode(a, r, layout, inds, metas, False, 0.05)
    assert boxes[0, 0].tolist() == boxes[0, 1].tolist() == [96. - 24., 64. - 16., 96. + 40., 64. + 32.]     # exactly k * stride
    assert valid[0].tolist() == [False, True, True, False, True, False, False, False, False, False] and n_valid.tolist() == [3, 0]
    assert torch.isfinite(boxes).all() and torch.isfinite(scores).all()
    # +-80: the softmax puts everything on the even bins, weights equal: expectation (0 + 2 + .. + 16) / 9 = 8 strides of 16
    assert np.allclose(boxes[0, 2].numpy(), [0., 0., 48. + 128., 128.], rtol=0, atol=1e-3)       # (clipped to 128 x 189)
    h, w = metas[0]['img_shape'][:2]
    assert boxes[0, 4].tolist() == [0., 0., float(w), float(h)]                   # 160 -+ 512, 0 -+ 512 clipped to the image
    # (4) a score exactly at score_thr is invalid: the threshold is the kernel's own fp32 score of one candidate
    cls2, raw2 = gi.head_outputs(7, 2)
    a, r, layout = make_rows(cls2, raw2)
    inds = [torch.arange(m, device=DEV).expand(2, m).contiguous() for m in (40, 30, 24, 6, 2)]
    _, s0, _, v0, _ = _decode(a, r, layout, inds, metas, False, 0.0)
    thr = float(s0[0].sort()[0][s0.shape[1] // 2])
    _, s1, _, v1, nv = _decode(a, r, layout, inds, metas, False, thr)
    assert torch.equal(s0, s1) and v0.all() and (s1[0] == thr).sum() >= 1
    assert torch.equal(v1, s1 > thr) and not v1[0][s1[0] == thr].any() and nv.tolist() == [int(x) for x in (s1 > thr).sum(1)]


# ------------------------------------------------------------------------------------------- loss
GT_HAND = [torch.tensor([[40.5, 30.25, 100.75, 90.5],          # image 0: a mid-sized box, level 0
                         [2.5, 1.5, 185.25, 120.75],           # nearly the whole image: sides beyond reg_max from level 0
                         [16., 8., 112., 104.]]),              # whole numbers of level-1 strides from (64, 48)
           torch.tensor([[20.25, 10.5, 90.75, 70.25], [60.5, 40.75, 180.25, 120.5]])]
LABEL_HAND = [torch.tensor([1, 0, 3]), torch.tensor([2, 1])]


def _cell(level, y, x):
    return int(STARTS[level]) + y * gi.SIZES[level][1] + x


def _hand_inds():
    """gt_inds (2, 512) by hand, so that the edges occur by construction (centre = (x * s, y * s)):
      image 0: level 0 cells (6, 8), (7, 9), (8, 10) inside ground truth 0; cell (6, 4), centre (32, 48), LEFT of ground truth 0
      (left distance clamped to 0); cell (1, 1), centre (8, 8), on ground truth 1: right = 22.2, bottom = 14.1 strides (right
      clamped to 15.9); level 1 cell (3, 4), centre (64, 48), on ground truth 2: left = 3, right = 3 strides exactly (right
      bin weight 0), top 2.5, bottom 3.5; level 2 cell (2, 3), centre (96, 64), on ground truth 1; cells 5 and 300 invalid
      image 1: level 0 cells (4, 6), (5, 7) on ground truth 0; level 1 cell (5, 8), centre (128, 80), on ground truth 1; the last
      cell of level 1 invalid
    levels 3 and 4 have no positive."""
    g = torch.zeros(2, gi.ANCHORS, dtype=torch.long)
    for y, x in ((6, 8), (7, 9), (8, 10), (6, 4)):
        g[0, _cell(0, y, x)] = 1
    g[0, _cell(0, 1, 1)] = 2
    g[0, _cell(1, 3, 4)] = 3
    g[0, _cell(2, 2, 3)] = 2
    g[0, 5] = g[0, 300] = -1
    for y, x in ((4, 6), (5, 7)):
        g[1, _cell(0, y, x)] = 1
    g[1, _cell(1, 5, 8)] = 2
    g[1, int(STARTS[2]) - 1] = -1
    return g


def _loss_case(seed, C=4, wide=False, beta=2.0, weights=(1.0, 2.0, 0.25), hand=True, no_gt=False):
    cls, raw = gi.head_outputs(seed, C)
    if hand:
        gt_bboxes, gt_labels, inds64 = GT_HAND, [l.clamp(max=C - 1) for l in LABEL_HAND], list(_hand_inds())
    else:
        gt_bboxes, gt_labels = gi.gts(seed, num_classes=C)
        inds64 = RA.assign(gt_bboxes, gi.SIZES, gi.STRIDES, gi.OCTAVE, gi.TOPK, dtype=torch.float32)
    if no_gt:
        gt_bboxes, gt_labels = [g[:0] for g in gt_bboxes], [l[:0] for l in gt_labels]
        inds64 = [torch.zeros(gi.ANCHORS, dtype=torch.long)] * 2
    a, r, layout = make_rows(cls, raw, 16, wide)
    gts, labels, offs = train_ops.flatten_gts(gt_bboxes, gt_labels)
    gts, labels = gts.to(DEV), labels.to(DEV)
    gt_inds = torch.stack(inds64).to(torch.int32).to(DEV).contiguous()
    meta = train_ops.GflLossMeta(2, gi.SIZES, gi.STRIDES, base_table(), 16, C, offs, beta, 1e-6, *weights)
    return dict(cls=cls, raw=raw, a=a, r=r, layout=layout, gts=gts, labels=labels, gt_inds=gt_inds, meta=meta, beta=beta,
                gt_bboxes=gt_bboxes, gt_labels=gt_labels, inds64=inds64, C=C, weights=weights)


def _ref(c, **kw):
    return R.loss(c['cls'], c['raw'], gi.SCALES, c['inds64'], c['gt_bboxes'], c['gt_labels'], gi.SIZES, gi.STRIDES, gi.OCTAVE,
                  16, c['beta'], 1e-6, c['weights'], **kw)


def _run_loss(c, hook=None):
    a, r = c['a'].clone().requires_grad_(), c['r'].clone().requires_grad_()
    sc = scales_dev().requires_grad_()
    losses, coef, norm2 = train_ops.gfl_loss(a, r, sc, c['gt_inds'], c['gts'], c['labels'], c['layout'], c['meta'], hook)
    losses.sum().backward()
    return losses.detach().cpu(), coef.cpu(), norm2.cpu(), a.grad.cpu(), r.grad.cpu(), sc.grad.cpu()


def _check_loss(c, got, ref):
    """values and gradients against float64 with bounds from the kernels' fp32 arithmetic, as tests/test_atss_gpu.py derives
    its own:
      * a sum of terms: the evaluation error of every term (off the label the bound of gfl_ref64.qfl_background;
        for the label, box and DFL terms twice the first-order error over each rounded intermediate, which
        tests/gfl_ref64.py records), plus the summation -- each partial goes through at most 8 sequential additions in a
        thread, 8 LDS tree levels, and the same again in the one finalize workgroup: <= 40 eps of the sum of the absolute
        terms --, plus 4 eps for the division by the normaliser and the loss weight;
      * a gradient element: four times the first-order error of its expression (twice, doubled once more for the backward
        chain's own roundings), plus 16 eps of the absolute value of each of its two parts (box, DFL) for the coefficients and
        the products."""
    losses, coef, norm2, da, dr, dsc = got
    C, lay, B, n = c['C'], c['layout'].values, 2, 17
    cls_off, reg_off = lay[1], lay[3]
    P = ref['n_pos']
    # the normalisers: the count is exact (an integer below 2^24; one rounding if a rank mean scaled it); the sum of the
    # weights carries 4 eps per sigmoid and n_pos + 16 eps relative for the summation
    assert P > 5 and abs(norm2[0].item() - ref['norm2'][0]) <= EPS32 * ref['norm2'][0]
    s_rel = (P + 16 + 8) * EPS32
    assert abs(norm2[1].item() - ref['norm2'][1]) <= s_rel * ref['norm2'][1]
    N, S = max(ref['norm2'][0], 1.0), max(ref['norm2'][1], 1.0)
    w = c['weights']
    x = R._rows(c['cls']).double().numpy()
    val_bg, der_bg, verr_bg, derr_bg = R.qfl_background(x, c['beta'])
    live = (ref['valid'].numpy()[:, None] > 0) & ~ref['hot'].numpy()
    assert np.abs(val_bg * live - ref['neg_terms'].numpy()).max() <= 1e-12          # (the two float64 forms agree)
    lv, plv = ref['level'].numpy(), ref['pos_level'].numpy()
    for l in range(L):
        rows, sel = lv == l, torch.from_numpy(plv == l)
        neg = float((val_bg * live)[rows].sum())
        hit = float(ref['hit_terms'][sel].sum())
        tol = [w[0] / N * (float((verr_bg * live)[rows].sum()) + 2 * float(ref['hit_value_err'][sel].sum()) + 40 * EPS32 * (neg + hit)),
               w[1] / S * (2 * float(ref['box_value_err'][sel].sum()) + (40 * EPS32 + s_rel) * float(ref['box_terms'][sel].abs().sum())),
               w[2] / S * (2 * float(ref['dfl_value_err'][sel].sum()) + (40 * EPS32 + s_rel) * float(ref['dfl_terms'][sel].abs().sum()))]
        for i in range(3):
            want = float(ref['losses'][i, l])
            print('loss', i, 'level', l, 'got', float(losses[i, l]), 'float64', want, 'bound', tol[i] + 4 * EPS32 * abs(want))
            assert abs(float(losses[i, l]) - want) <= tol[i] + 4 * EPS32 * abs(want), (i, l, float(losses[i, l]), want, tol[i])
    assert np.allclose(coef.numpy(), [w[0] / N, w[1] / S, w[2] / S], rtol=4 * EPS32 + s_rel, atol=0)
    # columns that belong to no head: exactly zero
    assert not da[:, [j for j in range(da.shape[1]) if not cls_off <= j < cls_off + C]].any()
    assert not dr[:, [j for j in range(dr.shape[1]) if not reg_off <= j < reg_off + 4 * n]].any()
    # dcls: off the label, at the label, and the invalid cells
    pos = ref['pos']
    got_c = da[:, cls_off:cls_off + C].double().numpy()
    want_c = R._rows(ref['dcls']).numpy()
    bound_c = w[0] / N * derr_bg * live + 16 * EPS32 * np.abs(want_c) + 1e-30
    hot = ref['hot'].numpy()
    lab = ref['labels'][pos].numpy()
    bound_c[pos.numpy(), lab] = w[0] / N * 4 * ref['dhit_err'].numpy() + 16 * EPS32 * np.abs(want_c[pos.numpy(), lab]) + 1e-30
    assert np.abs(w[0] / N * ref['dhit'].numpy() - want_c[pos.numpy(), lab]).max() <= 1e-12
    print('dcls: largest error', float(np.abs(got_c - want_c).max()), 'largest error / bound', float((np.abs(got_c - want_c) / bound_c).max()))
    assert (np.abs(got_c - want_c) <= bound_c).all(), float((np.abs(got_c - want_c) / bound_c).max())
    assert hot.sum() == P and not got_c[ref['valid'].numpy() == 0].any()              # an invalid cell: exactly zero
    # dreg: zero off the positives, bounded on them
    off = torch.ones(da.shape[0], dtype=torch.bool)
    off[pos] = False
    assert not dr[off].any()
    sc_row = torch.cat([torch.full((B * m,), s, dtype=torch.float64) for m, s in zip(N_L, gi.SCALES)])[pos][:, None, None]
    got_r = dr[pos, reg_off:reg_off + 4 * n].double().view(P, 4, n)
    want_r = R._rows(ref['draw'])[pos].view(P, 4, n)
    k1, k2 = w[1] / S, w[2] / S
    assert (want_r - sc_row * (k1 * ref['dx_box'] + k2 * ref['dx_dfl'])).abs().max() <= 1e-12
    bound_x = 4 * (k1 * ref['dx_box_err'] + k2 * ref['dx_dfl_err']) + \
        (16 * EPS32 + s_rel) * (k1 * ref['dx_box'].abs() + k2 * ref['dx_dfl'].abs())
    bound_r = sc_row * bound_x + 1e-30
    print('dreg: largest error', float((got_r - want_r).abs().max()), 'largest error / bound', float(((got_r - want_r).abs() / bound_r).max()))
    assert ((got_r - want_r).abs() <= bound_r).all(), float(((got_r - want_r).abs() / bound_r).max())
    # dscale_l = sum over the level's positives of d(scaled) * raw: the elements' bounds times |raw|, plus the summation (a
    # thread adds up to 8 rows x 68 elements in sequence, then two trees: <= 8 * 68 + 32 eps of the absolute terms)
    raw_p = R._rows(c['raw']).double()[pos].view(P, 4, n)
    for l in range(L):
        sel = torch.from_numpy(plv == l)
        terms = ((k1 * ref['dx_box'] + k2 * ref['dx_dfl']) * raw_p)[sel]
        bound = float((bound_x * raw_p.abs())[sel].sum()) + (8 * 4 * n + 32) * EPS32 * float(terms.abs().sum())
        print('dscale level', l, 'got', float(dsc[l]), 'float64', float(ref['dscale'][l]), 'bound', bound)
        assert abs(float(dsc[l]) - float(ref['dscale'][l])) <= bound + 1e-30
        if not sel.any():
            assert float(dsc[l]) == 0.0


@pytest.mark.parametrize('C,wide,beta', [(4, False, 2.0), (4, True, 1.5), (1, True, 2.0)])
def test_loss_and_gradients_against_float64(C, wide, beta):
    c = _loss_case(44, C, wide, beta)
    got = _run_loss(c)
    ref = _ref(c)
    # preconditions: no pair of box edges (and no intersection length) within the fp32 error of an edge, 64 eps x the largest
    # coordinate in strides (24), so that every min / max / clamp selects in fp32 what it selects in float64; every target
    # distance is a whole number exactly (both arithmetics agree on it) or further than 1e-4 from one
    assert ref['edge_gap'] > 64 * EPS32 * 24
    frac = (ref['side'] - ref['side'].round()).abs()
    assert ((frac == 0) | (frac > 1e-4)).all()
    # the edges, by construction
    side, t, left = ref['side'], ref['target'], ref['left']
    assert (side > 16).any() and (t == R.clamp_hi(16)).sum() == (side > R.clamp_hi(16)).sum() >= 1     # beyond reg_max
    assert (side < 0).any() and (t[side < 0] == 0).all()                                                # centre outside
    whole = (frac == 0) & (side > 0) & (side < 15)
    assert whole.sum() >= 2 and (t[whole] == left[whole].double()).all()                                # right weight 0
    assert (ref['valid'] == 0).sum() == 3 and set(ref['pos_level'].tolist()) == {0, 1, 2}       # levels 3, 4 empty
    assert ref['n_pos'] == 10
    _check_loss(c, got, ref)
    assert not got[0][1:, 3:].any()                         # a level without positives: box and DFL losses exactly 0
    again = _run_loss(c)
    for x, y in zip(got, again):            # the same bits from run to run
        assert torch.equal(x, y)


def test_loss_against_float64_on_assigned_targets():
    """the assignment's own targets (the fixture's inputs of another seed): more positives per level, contested anchors"""
    c = _loss_case(45, 4, False, hand=False)
    ref = _ref(c)
    frac = (ref['side'] - ref['side'].round()).abs()
    assert ref['edge_gap'] > 64 * EPS32 * 24 and ((frac == 0) | (frac > 1e-4)).all() and ref['n_pos'] > 20
    _check_loss(c, _run_loss(c), ref)


def test_loss_without_positives_is_exactly_zero():
    c = _loss_case(44, 4, True, no_gt=True)
    losses, coef, norm2, da, dr, dsc = _run_loss(c)
    assert norm2.tolist() == [2.0, 0.0]                         # sum over the two images of max(0, 1)
    assert not losses[1].any() and not losses[2].any() and (losses[0] > 0).all()
    assert not dr.any() and not dsc.any()
    assert da[:, 3:7].abs().sum().item() > 0 and not da[:, :3].any() and not da[:, 7:].any()
    assert np.allclose(coef.numpy(), [1.0 / 2.0, 2.0, 0.25], rtol=4 * EPS32)


def test_finalize_with_normalisers_averaged_by_hand():
    """norm2 changed between the sums and the division, as the mean over ranks does: losses and gradients follow the
    float64 run with the same normalisers"""
    c = _loss_case(44, 4, False)

    def hook(n2):
        n2.mul_(torch.tensor([0.75, 1.25], device=n2.device))
    got = list(_run_loss(c, hook))
    plain = _ref(c, grads=False)
    n2 = [plain['norm2'][0] * 0.75, plain['norm2'][1] * 1.25]
    ref = _ref(c, norm2=n2)
    assert ref['norm2'] == n2 and not np.allclose(ref['losses'].numpy(), plain['losses'].numpy(), rtol=0.1)
    _check_loss(c, got, ref)


# ------------------------------------------------------------------------------------------- the fixture
CASES = [(4, 'plain'), (4, 'rescale'), (4, 'empty'), (1, 'plain'), (1, 'rescale')]


def _split_cfg(cfg, thr):
    if thr:
        cfg['test_cfg']['nms'] = dict(cfg['test_cfg']['nms'], split_thr=thr)
    return cfg


def _force_form(monkeypatch, form):
    """'torch': `batched_nms_images_by_level` in its form for more than 16 384 slots"""
    if form == 'torch':
        import functools

        from brcnn import postprocess
        monkeypatch.setattr(postprocess, 'batched_nms_images_by_level',
                            functools.partial(postprocess.batched_nms_images_by_level, fused=False))


def _check_dets(res, gold, C, name, what):
    for b, (det, lab) in enumerate(res):
        want_d, want_l = T(gold[f'bboxes_c{C}_{name}_det{b}']), T(gold[f'bboxes_c{C}_{name}_lab{b}'])
        assert lab.cpu().tolist() == want_l.tolist(), (C, name, what, b)
        assert det.shape == want_d.shape and torch.allclose(det.cpu(), want_d, rtol=0, atol=2e-4), (C, name, what, b)


@pytest.mark.parametrize('form', ['offset', 'fused', 'torch'])
@pytest.mark.parametrize('C,name', CASES)
def test_get_bboxes_golden(gold, monkeypatch, C, name, form):
    """the reference-signature get_bboxes on device tensors against the reference's detections: labels and order exact,
    boxes and scores within 2e-4; on the offset NMS branch and, with split_thr = 100 (132 .. 528 slots per image), on the
    per-class branch in both forms"""
    _force_form(monkeypatch, form)
    seed = int(gold[f'seed_bboxes_c{C}'])
    head = build(C, **_split_cfg(dict(test_cfg=dict(gi.TEST_CFG)), 0 if form == 'offset' else 100)).eval()
    cls, raw = gi.head_outputs(seed, C, empty=(name == 'empty'))
    dv = lambda lst: [t.to(DEV) for t in lst]    # noqa: E731
    res = head.get_bboxes(dv(cls), dv(gi.scaled(raw, gi.SCALES)), gi.metas(), rescale=(name != 'plain'))
    _check_dets(res, gold, C, name, form)
    if name == 'empty':
        assert head.last_n_valid.tolist()[1] == 0 and len(res[1][0]) == 0 and len(res[0][0]) > 0


@pytest.mark.parametrize('C,name', CASES)
def test_get_bboxes_rows_golden(gold, C, name):
    """the fused-row form: RAW rows as the head's own convs leave them, the live scales applied in the kernels"""
    seed = int(gold[f'seed_bboxes_c{C}'])
    head = build(C).eval()
    cls, raw = gi.head_outputs(seed, C, empty=(name == 'empty'))
    a, r, layout = make_rows(cls, raw)
    det, lab, num = head.get_bboxes_rows(a, r, layout, head._scales_tensor(), gi.SIZES, gi.metas(), rescale=(name != 'plain'))
    num = num.tolist()
    _check_dets([(det[b, :num[b]], lab[b, :num[b]]) for b in range(2)], gold, C, name, 'rows')


def test_loss_on_device_tensors_golden(gold):
    """the reference-signature loss on device tensors (assignment + loss kernels behind it) against the reference's values
    at the train iterations' tolerance, and its gradients w.r.t. the scaled box logits"""
    seed = int(gold['seed_loss_c4'])
    head = build(4, True)
    cls, raw = gi.head_outputs(seed, 4)
    gt_bboxes, gt_labels = gi.gts(seed)
    dv = lambda lst: [t.to(DEV).requires_grad_() for t in lst]    # noqa: E731
    dcls, dreg = dv(cls), dv(gi.scaled(raw, gi.SCALES))
    losses = head.loss(dcls, dreg, [g.to(DEV) for g in gt_bboxes], [l.to(DEV) for l in gt_labels], gi.metas())
    assert sorted(losses) == ['loss_bbox', 'loss_cls', 'loss_dfl']
    for k, v in losses.items():
        got = torch.stack(v).detach().cpu()
        assert torch.allclose(got, T(gold[f'loss_c4_{k}']), rtol=2e-3, atol=1e-4), (k, got, gold[f'loss_c4_{k}'])
    sum(sum(v) for v in losses.values()).backward()
    for l in range(L):
        # the fixture's gradient is w.r.t. the RAW logit: d raw = d scaled * scale
        assert torch.allclose(dreg[l].grad.cpu() * gi.SCALES[l], T(gold[f'loss_c4_dreg{l}']), rtol=2e-3, atol=1e-6), l
        assert torch.allclose(dcls[l].grad.cpu(), T(gold[f'loss_c4_dcls{l}']), rtol=2e-3, atol=1e-6), l


def test_loss_on_raw_rows_golden(gold):
    """the train step's form: RAW rows + the scales as a differentiable tensor; dscale against the reference's"""
    seed = int(gold['seed_loss_c4'])
    head = build(4, True)
    cls, raw = gi.head_outputs(seed, 4)
    gt_bboxes, gt_labels = gi.gts(seed)
    a, r, _ = make_rows(cls, raw)
    sc = scales_dev().requires_grad_()
    losses = head.loss_fused(a, r, sc, gi.SIZES, [g.to(DEV) for g in gt_bboxes], [l.to(DEV) for l in gt_labels], gi.metas())
    for k, v in losses.items():
        assert torch.allclose(torch.stack(v).detach().cpu(), T(gold[f'loss_c4_{k}']), rtol=2e-3, atol=1e-4), k
    sum(sum(v) for v in losses.values()).backward()
    assert torch.allclose(sc.grad.cpu(), T(gold['loss_c4_dscale']), rtol=2e-3, atol=1e-6)


def _table(res):
    return np.concatenate([np.concatenate([r, np.full((len(r), 1), c, np.float32)], 1) for c, r in enumerate(res)], 0)


def _model(seed, split_thr=0):
    m = build_detector(ConfigDict(_split_cfg(gi.fixture_model_cfg(), split_thr)))
    m.load_state_dict(gi.fixture_state_dict(m, seed))
    return m.to(DEV)


@pytest.mark.parametrize('form', ['offset', 'fused', 'torch'])
def test_model_end_to_end_golden(gold, monkeypatch, form):
    """`model(return_loss=False)` against the reference's run of the same seeded model: per class the same detections in
    the same order, labels exact, boxes and scores within 2e-4 (g28's / g29's bound; the fixture's reference run is within
    5e-5 of its own float64 run).  `simple_test_device` runs under torch's synchronisation debug mode on 'error': the one
    host read of an inference call is the result copy."""
    _force_form(monkeypatch, form)
    seed = int(gold['seed_e2e'])
    m = _model(seed, 0 if form == 'offset' else 100).eval()
    img, _, _, _ = util.demo_inputs(2, gi.H, gi.W, seed=seed)
    img = img.to(DEV)
    with torch.no_grad():
        res = m(return_loss=False, rescale=True, img=[img], img_metas=[gi.metas()])
        assert len(m.last_n_valid) == 2 and all(n >= sum(len(r) for r in res[b]) > 0 for b, n in enumerate(m.last_n_valid))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            det, lab, nd = m.simple_test_device(img, gi.metas(), rescale=True)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    assert float(gold['e2e_ref_err']) <= 5e-5
    assert nd.tolist() == [sum(len(r) for r in res[b]) for b in range(2)]
    for b in range(2):
        assert len(res[b]) == 4 and all(r.dtype == np.float32 and r.shape[1] == 5 for r in res[b])
        got, ref = _table(res[b]), gold[f'e2e_res{b}']
        assert got.shape == ref.shape and np.array_equal(got[:, 5], ref[:, 5]), (form, b)
        print('image', b, 'largest box / score difference', float(np.abs(got[:, :5] - ref[:, :5]).max()))
        assert np.allclose(got[:, :5], ref[:, :5], rtol=0, atol=2e-4), (form, b, np.abs(got[:, :5] - ref[:, :5]).max())


def _train_batch(seed):
    img, _, _, _ = util.demo_inputs(2, gi.H, gi.W, seed=seed, num_gt=gi.TRAIN_NUM_GT)
    gts, gls = gi.gts(seed)
    return img.to(DEV), [g.to(DEV) for g in gts], [l.to(DEV) for l in gls]


def test_no_host_read_in_the_head_train_step(gold):
    """`bbox_head.forward_train_nhwc` under torch's synchronisation debug mode on 'error': any blocking host read raises.
    The second image's pad_shape is smaller than the batch pad, so the valid-cell table is part of the step"""
    m = _model(int(gold['seed_e2e'])).train()
    img, gts, gls = _train_batch(int(gold['seed_train0']))
    feats = [f.detach() for f in m.extract_feat_nhwc(img)]
    metas = gi.metas(2, pads=[(gi.H, gi.W), (gi.H - 32, gi.W - 64)])
    m.bbox_head.forward_train_nhwc(feats, metas, gts, gls)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        losses = m.bbox_head.forward_train_nhwc(feats, metas, gts, gls)
        total = torch.stack([x for v in losses.values() for x in v]).sum()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert math.isfinite(float(total.detach()))
    ind = m.bbox_head.last_targets[0].cpu()
    assert (ind[0] >= 0).all() and (ind[1] == -1).any() and (ind[1] > 0).any()


def test_two_train_iterations_golden(gold):
    m = _model(int(gold['seed_e2e'])).train()
    for it in range(2):
        img, gts, gls = _train_batch(int(gold[f'seed_train{it}']))
        losses = m(img=img, img_metas=gi.metas(), gt_bboxes=gts, gt_labels=gls)
        assert sorted(losses) == ['loss_bbox', 'loss_cls', 'loss_dfl']
        for k, v in losses.items():
            got = torch.stack(list(v)).detach().cpu().double().reshape(-1)
            ref = T(gold[f'train{it}_{k}']).double().reshape(-1)
            assert torch.allclose(got, ref, rtol=2e-3, atol=1e-4), (it, k, got, ref)
        loss, log_vars = m._parse_losses(losses)
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for n, p in m.bbox_head.named_parameters())
        assert sum(s.scale.grad.abs().item() for s in m.bbox_head.scales) > 0
        assert m.backbone.layer2[0].conv1.weight.grad is not None
        m.zero_grad()


# ------------------------------------------------------------------------------------------- 16-bit modes and the tools
@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
def test_model_16bit_close_to_fp32(gold, dtype):
    """the criterion tests/test_atss_gpu.py::test_model_16bit_close_to_fp32 applies to its 16-bit cases"""
    from brcnn import blocks
    seed = int(gold['seed_e2e'])
    m = _model(seed).eval()
    img, _, _, _ = util.demo_inputs(2, gi.H, gi.W, seed=seed)
    try:
        with torch.no_grad():
            f32 = [f.float() for f in m.extract_feat_nhwc(img.to(DEV))]
            r32 = m.simple_test(img.to(DEV), gi.metas())
            m.set_compute_dtype(dtype)
            f16 = m.extract_feat_nhwc(img.to(DEV))
            assert all(f.dtype == (torch.bfloat16 if dtype == 'bf16' else torch.float16) for f in f16)
            a, r, _ = m.bbox_head.forward_rows(list(f16))
            assert a.dtype == torch.float32 and r.dtype == torch.float32 and r.shape[1] == 72      # fp32 from the head on
            r16 = m.simple_test(img.to(DEV), gi.metas())
    finally:
        blocks.set_compute_dtype('f32')
    for x, y in zip(f16, f32):
        assert (x.float() - y).abs().max().item() / y.abs().max().item() < 0.05
    n32, n16 = sum(len(c) for r in r32 for c in r), sum(len(c) for r in r16 for c in r)
    assert n32 > 0 and abs(n16 - n32) <= 0.2 * n32 + 5, (n16, n32)
    d = np.concatenate([c for r in r32 for c in r]), np.concatenate([c for r in r16 for c in r])
    dist = np.abs(d[0][:, None, :4] - d[1][None, :, :4]).max(-1)
    ds = np.abs(d[0][:, None, 4] - d[1][None, :, 4])
    assert ((dist < 2.0) & (ds < 0.05)).any(1).mean() > 0.7


def test_inference_detector_returns_the_bbox2result_layout():
    from brcnn.apis import inference_detector, init_detector
    model = init_detector(gi.CONFIG, None, device=DEV)
    img = np.random.RandomState(0).randint(0, 255, (120, 160, 3), dtype=np.uint8)
    res = inference_detector(model, img)
    assert isinstance(res, list) and len(res) == 4
    assert all(isinstance(r, np.ndarray) and r.dtype == np.float32 and r.ndim == 2 and r.shape[1] == 5 for r in res)
    both = inference_detector(model, [img, img[:, ::-1].copy()])
    assert len(both) == 2 and all(len(r) == 4 for r in both)


def test_bf16_train_step_is_reproducible_and_fused_sgd_follows(gold):
    from brcnn import blocks
    from brcnn.optim import FusedSGD
    m = _model(int(gold['seed_e2e'])).train()
    img, gts, gls = _train_batch(int(gold['seed_train0']))
    data = dict(img=img, img_metas=gi.metas(), gt_bboxes=gts, gt_labels=gls)
    opt = FusedSGD([p for p in m.parameters() if p.requires_grad], lr=0.01, momentum=0.9, weight_decay=1e-4)
    try:
        m.set_compute_dtype('bf16')
        runs = []
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            out = m.train_step(data, opt)
            out['loss'].backward()
            grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
            runs.append((dict(out['log_vars'].items()), grads))
        assert runs[0][0] == runs[1][0] and 'loss_dfl' in runs[0][0]
        assert runs[0][1].keys() == runs[1][1].keys() and 'bbox_head.gfl_reg.weight' in runs[0][1]
        assert 'bbox_head.scales.4.scale' in runs[0][1]
        assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
        before = m.bbox_head.gfl_cls.weight.detach().clone()
        opt.step()
        torch.cuda.synchronize()
        assert not torch.equal(before, m.bbox_head.gfl_cls.weight.detach())
        assert all(torch.isfinite(p).all() for p in m.parameters())
    finally:
        blocks.set_compute_dtype('f32')


def test_train_and_test_tools_take_the_config(tmp_path):
    """tools/train.py (one epoch on the synthetic 7-image set, checkpoint, validation) and tools/test.py (bbox evaluation,
    result file) with the recipe's model section in the tiny driver config of tests/test_drivers_cpu.py"""
    import importlib.util
    import pickle

    from brcnn import Config
    from tests.test_drivers_cpu import CLASSES, _tiny_cfg

    def tool(name):
        spec = importlib.util.spec_from_file_location(f'brcnn_tool_{name}', os.path.join(gi.ROOT, 'tools', f'{name}.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    cfg = _tiny_cfg(tmp_path, max_epochs=1)
    cfg.model = Config.fromfile(gi.CONFIG).model
    cfg_path = str(tmp_path / 'tiny_gfl.py')
    cfg.dump(cfg_path)
    work = str(tmp_path / 'work_gpu')
    runner = tool('train').main([cfg_path, '--work-dir', work, '--seed', '0', '--allow-random-init'])
    assert runner.epoch == 1 and os.path.exists(os.path.join(work, 'epoch_1.pth'))
    assert all(np.isfinite(v) for row in runner.history for v in row[3].values())
    assert any('loss_dfl' in row[3] and 'loss_bbox' in row[3] for row in runner.history) and len(runner.eval_history) == 1
    out_pkl = str(tmp_path / 'res.pkl')
    metric = tool('test').main([cfg_path, os.path.join(work, 'epoch_1.pth'), '--eval', 'bbox', '--out', out_pkl])
    assert metric == {} or 0.0 <= metric['bbox_mAP'] <= 1.0
    res = pickle.load(open(out_pkl, 'rb'))
    assert len(res) == 7 and len(res[0]) == len(CLASSES) and res[0][0].shape[1] == 5
