"""GPU tests of the ATSS baseline (csrc/atss_head.hip, ATSSAssigner, ATSSHead, ATSS).

Against the fixture g29_atss.npz (tests/golden/make_golden_atss.py; the reference's fp32 run): assignments, labels and kept
order exact, boxes and scores within the 2e-4 of g27's / g28's end-to-end cases (the fixture's reference run is within 5e-5
of its own float64 run), train losses within rtol 2e-3 / atol 1e-4 as tests/test_fcos_gpu.py holds its own.
Against float64 (tests/atss_ref64.py): bounds stated where used, derived from the fp32 arithmetic of the kernels (eps =
2^-23; an addition, product or division rounds to eps / 2, expf / logf / sqrtf are counted as 2 eps); none is tuned to what
the kernels give.  Preconditions on the inputs (rank gaps, distances to thresholds) are asserted."""
import math
import os
import re

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import build_detector, build_head, ops, train_ops
from brcnn.config import ConfigDict
from tests import atss_inputs as ai
from tests import atss_ref64 as R
from tests import dense_loss_ref64 as RD
from tests import util

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G = os.path.join(os.path.dirname(__file__), 'golden', 'g29_atss.npz')
EPS32 = float(np.finfo(np.float32).eps)
L = len(ai.SIZES)
N_L = [h * w for h, w in ai.SIZES]
STARTS = np.cumsum([0] + N_L)


@pytest.fixture(scope='module')
def gold():
    return {k: v for k, v in np.load(G, allow_pickle=False).items()}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def build(C=4, training=False, **over):
    head = build_head(ConfigDict(ai.head_cfg(C, **over))).train(training)
    with torch.no_grad():
        for s, v in zip(head.scales, ai.SCALES):
            s.scale.fill_(v)
    return head.to(DEV)


def base_table():
    half = [s * ai.OCTAVE / 2 for s in ai.STRIDES]
    return ops.atss_base_anchors([torch.tensor([[-h, -h, h, h]]) for h in half])


def test_the_library_exports_every_atss_entry_of_the_header():
    from brcnn import lib
    from brcnn.registry import BBOX_ASSIGNERS, DETECTORS, HEADS
    header = open(os.path.join(ai.ROOT, 'include', 'brcnn_hip.h')).read()
    declared = sorted(set(re.findall(r'^(?:int|size_t) (brcnn_atss_\w+)\(', header, re.M)))
    assert declared == ['brcnn_atss_assign', 'brcnn_atss_decode_levels', 'brcnn_atss_loss_backward', 'brcnn_atss_loss_finalize',
                        'brcnn_atss_loss_forward', 'brcnn_atss_loss_workspace_bytes']
    for name in declared:
        assert name in lib.SIGNATURES and hasattr(lib.load(), name), name
    assert HEADS.get('ATSSHead') is not None and DETECTORS.get('ATSS') is not None and BBOX_ASSIGNERS.get('ATSSAssigner') is not None


# ------------------------------------------------------------------------------------------- assignment
def _valid_hws(pads):
    return None if pads is None else [[[min(math.ceil(p[0] / s), h), min(math.ceil(p[1] / s), w)]
                                       for (h, w), s in zip(ai.SIZES, ai.STRIDES)] for p in pads]


def _assign(gts, pads=None, topk=ai.TOPK, overlaps=False):
    offs = [0]
    for g in gts:
        offs.append(offs[-1] + len(g))
    flat = torch.cat([g.reshape(-1, 4) for g in gts]).float().contiguous().to(DEV)
    v = _valid_hws(pads)
    valid_hw = None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)
    out = train_ops.atss_assign(flat, offs, len(gts), ai.SIZES, ai.STRIDES, base_table(), topk, valid_hw, want_overlaps=overlaps)
    return (out[0].cpu().long(), out[1].cpu()) if overlaps else out.cpu().long()


def _anchor(level, y, x):
    """index of cell (y, x) of `level` among an image's anchors"""
    return int(STARTS[level]) + y * ai.SIZES[level][1] + x


def _restated(gts, pads=None, dtype=torch.float32, topk=ai.TOPK):
    inds, info = R.assign(gts, ai.SIZES, ai.STRIDES, ai.OCTAVE, topk, _valid_hws(pads), dtype, details=True)
    for d in info:
        if d is not None:       # precondition: no candidate within 1e-5 of its IoU threshold or 1e-3 of the side test
            fin = torch.isfinite(d['thr'])[None].expand_as(d['iou'])
            assert ((d['iou'] - d['thr'][None]).abs()[fin] > 1e-5).all() and ((d['side'] - 0.01).abs() > 1e-3).all()
    return torch.stack(inds), info


def test_assign_is_exact_against_the_fixture_and_the_restatement(gold):
    gts, _ = ai.gts(int(gold['seed_assign']))
    got, ov = _assign(gts, overlaps=True)
    for b in range(2):
        assert torch.equal(got[b], T(gold[f'assign_gt_inds{b}'])), (b, (got[b] != T(gold[f'assign_gt_inds{b}'])).nonzero()[:5])
        want = T(gold[f'assign_max_overlaps{b}'])
        assert torch.equal(ov[b] > 0, want > 0) and torch.allclose(ov[b], want, rtol=4 * EPS32, atol=0)
        assert (ov[b][got[b] == 0] == -1e8).all()
    for dtype in (torch.float32, torch.float64):
        want, _ = _restated(gts, dtype=dtype)
        assert torch.equal(got, want), dtype
    assert sum(bool((got[:, STARTS[l]:STARTS[l + 1]] > 0).any()) for l in range(L)) >= 3
    assert torch.equal(_assign(gts), got)                                     # the same bits from run to run


def test_assign_hand_made_cases():
    """each case against the restatement (float32: the reference's own comparisons), then what the case is about"""
    # an image whose pad_shape (60, 100) is smaller than the batch pad: levels 2 / 3 / 4 keep 8 / 2 / 1 valid cells
    pads = [(60, 100), (ai.H, ai.W)]
    small = torch.tensor([[10., 8., 70., 50.], [30., 20., 90., 58.]])
    gts = [small, torch.tensor([[20., 30., 120., 110.]])]
    got = _assign(gts, pads)
    want, info = _restated(gts, pads)
    assert torch.equal(got, want)
    valid = R.valid_mask(ai.SIZES, _valid_hws(pads)[0])
    assert (got[0][~valid] == -1).all() and (got[0][valid] >= 0).all() and (got[1] >= 0).all()
    assert info[0]['cand'].shape[0] == 9 + 9 + 8 + 2 + 1 and valid[info[0]['cand']].all()
    # an image with no ground truth between two that have some
    gts = [small, torch.zeros(0, 4), small + 20]
    got = _assign(gts)
    assert torch.equal(got, _restated(gts)[0]) and not got[1].any() and (got[0] > 0).any() and (got[2] > 0).any()
    # two identical ground truths: every contested anchor goes to the lower index
    gts = [torch.tensor([[40., 24., 120., 104.], [40., 24., 120., 104.]])]
    got = _assign(gts)
    assert torch.equal(got, _restated(gts)[0]) and (got == 1).sum() > 0 and not (got == 2).any()
    # centre (68, 64): on level 0 the 9th rank falls among four equidistant cells (dx = +-12, dy = +-8), the lowest
    # index wins -- the reference leaves this to torch.topk, so the restatement is the only yardstick
    gts = [torch.tensor([[36., 32., 100., 96.]])]
    got = _assign(gts)
    want, info = _restated(gts)
    assert torch.equal(got, want) and float(info[0]['gaps'][0, 0]) == 0.0
    level0 = sorted(int(c) for c in info[0]['cand'][:9, 0])
    tied = [_anchor(0, 7, 7), _anchor(0, 7, 10), _anchor(0, 9, 7), _anchor(0, 9, 10)]
    assert [c for c in level0 if c in tied] == [tied[0]]
    # the same rule where it decides the OUTPUT: a 16 px box centred between four cells, (68, 68), topk = 3: the four nearest
    # anchors tie in distance and in IoU, the three of lowest index are the candidates, and all three come out positive
    gts = [torch.tensor([[60., 60., 76., 76.]])]
    got = _assign(gts, topk=3)
    want, info = _restated(gts, topk=3)
    assert torch.equal(got, want) and float(info[0]['gaps'][0, 0]) == 0.0
    assert (got[0] > 0).nonzero().reshape(-1).tolist() == [_anchor(0, 8, 8), _anchor(0, 8, 9), _anchor(0, 9, 8)]
    # centre on the lattice point (64, 64): the 3 x 3 block is level 0's candidate set, ties inside it, none at its boundary
    gts = [torch.tensor([[40., 40., 88., 88.]])]
    got = _assign(gts)
    want, info = _restated(gts)
    assert torch.equal(got, want) and float(info[0]['gaps'][0, 0]) > 0
    assert sorted(int(c) for c in info[0]['cand'][:9, 0]) == [_anchor(0, y, x) for y in (7, 8, 9) for x in (7, 8, 9)]
    for dtype in (torch.float64,):
        assert torch.equal(got, _restated(gts, dtype=dtype)[0])


def test_assign_refuses_what_it_does_not_serve():
    flat = torch.zeros(1, 4, device=DEV)
    for topk in (0, 17):
        with pytest.raises(ValueError, match='topk'):
            train_ops.atss_assign(flat, [0, 1], 1, ai.SIZES, ai.STRIDES, base_table(), topk)
    with pytest.raises(ValueError, match='images'):
        train_ops.atss_assign(flat, [0] + [1] * 65, 65, ai.SIZES, ai.STRIDES, base_table(), 9)
    with pytest.raises(ValueError, match='one anchor per cell'):
        ops.atss_base_anchors([torch.zeros(3, 4)])


# ------------------------------------------------------------------------------------------- layouts
def _rows(levels):
    return torch.cat([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in levels]).float()


def make_rows(cls, raw, ctr, ctr_in_r=True, wide=False):
    """reference-layout raw head outputs -> the kernels' (A, R) row tensors on the device and their layout.  `wide`: the
    heads are channel slices at non-zero offsets of wider tensors whose other columns hold 7.5 (a kernel that read a wrong
    column would show it)"""
    C = cls[0].shape[1]
    c, r, t = _rows(cls), _rows(raw), _rows(ctr)
    n = c.shape[0]
    if wide:
        cls_off, reg_off = 3, 1
        a = torch.full((n, C + 9), 7.5)
        rr = torch.full((n, 11), 7.5)
        ctr_off = 8 if ctr_in_r else C + 5
    else:
        cls_off = reg_off = 0
        a = torch.full((n, C + (0 if ctr_in_r else 1)), 7.5)
        rr = torch.full((n, 5 if ctr_in_r else 4), 7.5)
        ctr_off = 4 if ctr_in_r else C
    a[:, cls_off:cls_off + C] = c
    rr[:, reg_off:reg_off + 4] = r
    (rr if ctr_in_r else a)[:, ctr_off] = t[:, 0]
    a, rr = a.to(DEV), rr.to(DEV)
    return a, rr, ops.FcosLayout(a, rr, C, cls_off, reg_off, ctr_in_r, ctr_off, False, True)


def scales_dev():
    return torch.tensor(ai.SCALES, dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------------------------------- score + top-k + decode
def _run_candidates(a, r, layout, metas, rescale, nms_pre, thr):
    B = len(metas)
    scored, raw, r0 = ops.fcos_score(a, r, layout), [], 0
    for n in N_L:
        raw.append(scored[r0:r0 + B * n].view(B, n))
        r0 += B * n
    picked = ops.rpn_topk(raw, nms_pre)
    max_shape = torch.tensor([m['img_shape'][:2] for m in metas], dtype=torch.float32, device=DEV)
    sf = torch.tensor(np.stack([m['scale_factor'] for m in metas]), dtype=torch.float32, device=DEV) if rescale else None
    out = ops.atss_decode_levels([p[1] for p in picked], a, r, layout, scales_dev(), ai.SIZES, ai.STRIDES, base_table(),
                                 max_shape, sf, ai.MEANS, ai.STDS, thr)
    return raw, picked, out


def _check_candidates(cls, raw, ctr, C, ctr_in_r, wide, rescale, metas):
    B = len(metas)
    nms_pre, thr = ai.TEST_CFG['nms_pre'], ai.TEST_CFG['score_thr']
    a, r, layout = make_rows(cls, raw, ctr, ctr_in_r, wide)
    scores, picked, (bb, sc, lb, va, nv) = _run_candidates(a, r, layout, metas, rescale, nms_pre, thr)
    ref = R.candidates(cls, raw, ctr, ai.SCALES, ai.SIZES, ai.STRIDES, ai.OCTAVE, ai.MEANS, ai.STDS,
                       [m['img_shape'] for m in metas], [m['scale_factor'] for m in metas] if rescale else None)
    sf = torch.tensor(np.stack([m['scale_factor'] for m in metas]).astype(np.float64)) if rescale else torch.ones(B, 4).double()
    # a sigmoid is exp (2 eps), an addition and a division: 3 eps relative; the product of two, one more rounding: <= 8 eps
    S_TOL = 8 * EPS32
    an_l = R.anchors(ai.SIZES, ai.STRIDES, ai.OCTAVE)
    std = torch.tensor(ai.STDS, dtype=torch.float64)
    boxes, bounds, cscore, cvalid, T_ = [], [], [], [], 0
    for l, (m64, c64, ct64, bx64) in enumerate(ref):
        got = scores[l].cpu().double()
        assert ((got - m64).abs() <= S_TOL * m64).all(), l
        n = N_L[l]
        if n > nms_pre:
            ranked, idx = m64.sort(dim=1, descending=True, stable=True)
            # precondition: neighbouring ranks up to the first one left out differ by more than both values' fp32 error
            gap = (ranked[:, :nms_pre] - ranked[:, 1:nms_pre + 1])
            assert (gap > 2 * S_TOL * ranked[:, :nms_pre]).all(), (l, float(gap.min()))
            idx = idx[:, :nms_pre]
        else:
            idx = torch.arange(n).expand(B, n)
        assert torch.equal(picked[l][1].cpu(), idx), l                  # the picks, exact
        k = idx.shape[1]
        T_ += k
        c_p = torch.gather(c64, 1, idx[..., None].expand(-1, -1, C))
        ct_p = torch.gather(ct64, 1, idx)
        bx_p = torch.gather(bx64, 1, idx[..., None].expand(-1, -1, 4))
        # box bound.  delta = (scale * raw) * std: two roundings, eps |delta|.  Centre gx = px + pw * dxy: the product and the
        # sum round once more each: eps (|gx| + 2 |pw dxy|).  Size gw = pw * exp(clamp(dwh)): the delta's error eps |dwh|
        # becomes relative through exp, exp itself 2 eps, the product eps / 2: eps gw (|dwh| + 3).  A corner gx -+ gw / 2
        # rounds once (eps / 2 of the corner), and so does the division by the scale factor.  The sum, doubled for the
        # second-order terms:
        size = an_l[l][:, 2:] - an_l[l][:, :2]
        ctr_a = (an_l[l][:, :2] + an_l[l][:, 2:]) * 0.5
        dn = raw[l].double().permute(0, 2, 3, 1).reshape(B, n, 4) * ai.SCALES[l] * std
        shift = size[None] * dn[..., :2]
        gw = size[None] * dn[..., 2:].clamp(min=-R.MAX_RATIO, max=R.MAX_RATIO).exp()
        gx = ctr_a[None] + shift
        e_ctr = gx.abs() + 2 * shift.abs()
        e_size = gw * (dn[..., 2:].abs().clamp(max=R.MAX_RATIO) + 3)
        corner = torch.cat([gx - gw / 2, gx + gw / 2], -1).abs()
        bnd = 2 * EPS32 * (torch.cat([e_ctr, e_ctr], -1) + torch.cat([e_size, e_size], -1) / 2 + corner)
        bnd = torch.gather(bnd, 1, idx[..., None].expand(-1, -1, 4)) / sf[:, None, :]
        boxes.append(bx_p[:, :, None, :].expand(B, k, C, 4).reshape(B, k * C, 4))
        bounds.append(bnd[:, :, None, :].expand(B, k, C, 4).reshape(B, k * C, 4))
        cscore.append((c_p * ct_p[..., None]).reshape(B, k * C))
        cvalid.append(c_p.reshape(B, k * C))
    boxes, bounds, cscore, cvalid = (torch.cat(x, 1) for x in (boxes, bounds, cscore, cvalid))
    assert bb.shape == (B, T_ * C, 4) and T_ == sum(min(n, nms_pre) for n in N_L)
    assert torch.equal(lb.cpu(), torch.arange(C).repeat(T_).expand(B, -1))              # (level, pick, class) order
    # precondition: no class sigmoid within its fp32 error of score_thr
    assert ((cvalid - thr).abs() > 4 * EPS32 * thr).all()
    want_valid = cvalid > thr
    assert torch.equal(va.cpu(), want_valid) and nv.cpu().tolist() == want_valid.sum(1).tolist()
    assert ((sc.cpu().double() - cscore).abs() <= S_TOL * cscore).all()
    got = bb.cpu().double()
    assert torch.isfinite(got).all()
    err = (got - boxes).abs()
    print('boxes: largest error', float(err.max()), 'largest error / bound', float((err / bounds).max()))
    assert (err <= bounds).all(), float((err - bounds).max())
    return got, want_valid, sc.cpu(), boxes


@pytest.mark.parametrize('C,ctr_in_r,wide,rescale', [(4, True, False, True), (1, True, True, True), (3, False, True, False)])
def test_score_topk_decode_against_float64(C, ctr_in_r, wide, rescale):
    cls, raw, ctr = ai.head_outputs(11 + C, C, batch=3)
    _, valid, _, _ = _check_candidates(cls, raw, ctr, C, ctr_in_r, wide, rescale, ai.metas(3))
    assert valid.any() and not valid.all()


def test_a_delta_beyond_wh_ratio_clip_is_clamped():
    """scale * raw * std = 1.1 * 40 * 0.2 = 8.8 > |log(16 / 1000)| = 4.135: the decoded size is anchor * 1000 / 16, not anchor *
    e^8.8.  The image border is moved out to 8192 so that the clip to the image leaves the box alone"""
    cls, raw, ctr = ai.head_outputs(5, 4, batch=2)
    for b in range(2):
        raw[2][b, :, 2, 3] = torch.tensor([0., 0., 40., -40.])
        cls[2][b, :, 2, 3] = 6.0                 # certainly picked, first of its level
        ctr[2][b, 0, 2, 3] = 6.0
    metas = [dict(m, img_shape=(8192, 8192, 3)) for m in ai.metas(2)]
    got, _, _, want = _check_candidates(cls, raw, ctr, 4, True, False, False, metas)
    slot = (2 * ai.TEST_CFG['nms_pre'] + 2 * 6 + 3) * 4          # level 2 (24 anchors) passes whole, in index order
    for b in range(2):
        x1, y1, x2, y2 = got[b, slot].tolist()
        # centre (96, 64), 4000 x 1.024: the left edge is clipped at 0
        assert x1 == 0.0 and abs(x2 - (96 + 2000)) < 1e-2 and abs((y2 - y1) - 64 * 16 / 1000) < 1e-4 and abs(y1 + y2 - 128) < 1e-4
        assert x2 < 0.1 * (96 + 32 * math.exp(8.8))                             # (what no clamp would give)


def test_the_score_threshold_is_applied_before_the_centerness_factor():
    """a candidate whose class score passes score_thr = 0.05 but whose class score x centerness does not is VALID, as in
    multiclass_nms(..., score_factors=...); the kept detection carries the product as its score"""
    C = 4
    cls = [torch.full((2, C, h, w), -9.0) for h, w in ai.SIZES]
    raw = [torch.zeros(2, 4, h, w) for h, w in ai.SIZES]
    ctr = [torch.zeros(2, 1, h, w) for h, w in ai.SIZES]
    cls[2][0, 1, 2, 3] = math.log(0.06 / 0.94)          # class sigmoid 0.06 > 0.05
    ctr[2][0, 0, 2, 3] = math.log(0.1 / 0.9)            # centerness 0.1: product 0.006 < 0.05
    head = build(C)
    a, r, layout = make_rows(cls, raw, ctr)
    det, lab, num = head.get_bboxes_rows(a, r, layout, scales_dev(), ai.SIZES, ai.metas(), rescale=False)
    assert num.tolist() == [1, 0] and head.last_n_valid.tolist() == [1, 0]
    assert lab[0, 0].item() == 1 and abs(det[0, 0, 4].item() - 0.006) < 1e-6
    # zero deltas: the box is the anchor of cell (2, 3) of level 2, centre (96, 64), 64 px
    assert np.allclose(det[0, 0, :4].cpu().numpy(), [64., 32., 128., 96.], rtol=0, atol=1e-4)


def test_equal_products_are_ranked_by_index():
    """every anchor of a level with the same logits: all products are one fp32 value, the top-k keeps the lowest indices in
    ascending order (brcnn_rpn_topk's rule)"""
    C = 3
    cls, raw, ctr = ai.head_outputs(9, C)
    cls[0][:] = -2.0
    cls[0][:, 1] = -1.0
    ctr[0][:] = 0.5
    a, r, layout = make_rows(cls, raw, ctr, True, True)
    scores, picked, _ = _run_candidates(a, r, layout, ai.metas(), False, 50, 0.05)
    assert len(torch.unique(scores[0])) == 1
    assert torch.equal(picked[0][1].cpu(), torch.arange(50).expand(2, 50))


# ------------------------------------------------------------------------------------------- loss
LOSS_SEED = {4: 44, 1: 41}


def _loss_case(seed, C, wide, ctr_in_r=True, weights=(1.0, 2.0, 1.0), no_gt=False, clamp=False, invalid=False):
    cls, raw, ctr = ai.head_outputs(seed, C)
    gt_bboxes, gt_labels = ai.gts(seed, num_classes=C)
    if no_gt:
        gt_bboxes, gt_labels = [g[:0] for g in gt_bboxes], [l[:0] for l in gt_labels]
    inds64 = R.assign(gt_bboxes, ai.SIZES, ai.STRIDES, ai.OCTAVE, ai.TOPK, dtype=torch.float32)
    clamped = None
    if clamp:       # the first positive of level 1 predicts a width beyond the clamp: 0.9 * 40 * 0.2 = 7.2 > 4.135
        p = int((inds64[0][STARTS[1]:STARTS[2]] > 0).nonzero()[0])
        raw[1][0, 2, p // ai.SIZES[1][1], p % ai.SIZES[1][1]] = 40.0
        clamped = 2 * N_L[0] + p                                # its row: level 1 starts after both images' level-0 rows
    if invalid:     # a few cells marked invalid by hand (weight 0): a negative, and a positive that stops being one
        for b in range(2):
            inds64[b][5] = -1
            inds64[b][int((inds64[b] > 0).nonzero()[-1])] = -1
    a, r, layout = make_rows(cls, raw, ctr, ctr_in_r, wide)
    gts, labels, offs = train_ops.flatten_gts(gt_bboxes, gt_labels)
    gts, labels = gts.to(DEV), labels.to(DEV)
    gt_inds = torch.stack(inds64).to(torch.int32).to(DEV).contiguous()
    meta = train_ops.AtssLossMeta(2, ai.SIZES, ai.STRIDES, base_table(), C, offs, 2.0, 0.25, 1e-6, *weights, ai.MEANS, ai.STDS)
    return dict(cls=cls, raw=raw, ctr=ctr, a=a, r=r, layout=layout, gts=gts, labels=labels, gt_inds=gt_inds, meta=meta,
                gt_bboxes=gt_bboxes, gt_labels=gt_labels, inds64=inds64, C=C, weights=weights, clamped=clamped, offs=offs)


def _ref(c, **kw):
    return R.loss(c['cls'], c['raw'], c['ctr'], ai.SCALES, c['inds64'], c['gt_bboxes'], c['gt_labels'], ai.SIZES, ai.STRIDES,
                  ai.OCTAVE, ai.MEANS, ai.STDS, weights=c['weights'], **kw)


def _run_loss(c, hook=None):
    a, r = c['a'].clone().requires_grad_(), c['r'].clone().requires_grad_()
    sc = scales_dev().requires_grad_()
    losses, coef, norm2 = train_ops.atss_loss(a, r, sc, c['gt_inds'], c['gts'], c['labels'], c['layout'], c['meta'], hook)
    losses.sum().backward()
    return losses.detach().cpu(), coef.cpu(), norm2.cpu(), a.grad.cpu(), r.grad.cpu(), sc.grad.cpu()


def _check_loss(c, got, ref):
    """values and gradients against float64 with bounds from the kernels' fp32 arithmetic, as tests/test_fcos_gpu.py derives
    its own:
      * a sum of terms: the evaluation error of every term (the focal term's bound of tests/dense_loss_ref64.focal; for
        the box term twice the first-order error over each rounded intermediate, which tests/atss_ref64.py records), plus
        the summation -- each partial goes through at most 8 sequential additions in a thread, 8 LDS tree levels, and the
        same again in the one finalize workgroup: <= 40 eps of the sum of the absolute terms --, plus 4 eps for the
        division by the normaliser and the loss weight;
      * a gradient element: twice the first-order error of its expression (doubled once more for the backward chain's own
        roundings), plus 16 eps of its value for the coefficient and the products."""
    losses, coef, norm2, da, dr, dsc = got
    C, lay, B = c['C'], c['layout'].values, 2
    cls_off, reg_off, ctr_in_r, ctr_off = lay[1], lay[3], lay[4], lay[5]
    # the normalisers: the count is exact (an integer below 2^24; one rounding if a rank mean scaled it), the sum of the
    # centerness targets carries its terms' first-order errors and n_pos + 16 eps relative for the summation
    assert ref['n_pos'] > 5 and abs(norm2[0].item() - ref['norm2'][0]) <= EPS32 * ref['norm2'][0]
    s_rel = (ref['n_pos'] + 16) * EPS32 + 2 * float(ref['ctr_target_err'].sum()) / float(ref['ctr_targets'].sum())
    assert abs(norm2[1].item() - ref['norm2'][1]) <= s_rel * ref['norm2'][1]
    N, S = max(ref['norm2'][0], 1.0), max(ref['norm2'][1], 1.0)
    w = c['weights']
    x = R._rows(c['cls']).double().numpy()
    hit = ref['labels'].numpy()[:, None] == np.arange(C)[None, :]
    t_f, g_f, te_f, ge_f = RD.focal(x, hit, 2.0, 0.25)
    wt = ref['weight'].numpy()[:, None]
    t_f, g_f, te_f, ge_f = t_f * wt, g_f * wt, te_f * wt, ge_f * wt
    lv, plv = ref['level'].numpy(), ref['pos_level'].numpy()
    for l in range(L):
        rows, sel = lv == l, torch.from_numpy(plv == l)
        tol = [w[0] / N * (te_f[rows].sum() + 40 * EPS32 * t_f[rows].sum()),
               w[1] / S * (2 * float(ref['box_value_err'][sel].sum()) + (40 * EPS32 + s_rel) * float(ref['box_terms'][sel].abs().sum())),
               w[2] / N * (2 * float(ref['ctr_value_err'][sel].sum()) + 40 * EPS32 * float(ref['ctr_terms'][sel].sum()))]
        for i in range(3):
            want = float(ref['losses'][i, l])
            print('loss', i, 'level', l, 'got', float(losses[i, l]), 'float64', want, 'bound', tol[i] + 4 * EPS32 * abs(want))
            assert abs(float(losses[i, l]) - want) <= tol[i] + 4 * EPS32 * abs(want), (i, l, float(losses[i, l]), want, tol[i])
    assert np.allclose(coef.numpy(), [w[0] / N, w[1] / S, w[2] / N], rtol=4 * EPS32, atol=0)
    # columns that belong to no head: exactly zero
    a_cols = set(range(cls_off, cls_off + C)) | (set() if ctr_in_r else {ctr_off})
    r_cols = set(range(reg_off, reg_off + 4)) | ({ctr_off} if ctr_in_r else set())
    assert not da[:, [j for j in range(da.shape[1]) if j not in a_cols]].any()
    assert not dr[:, [j for j in range(dr.shape[1]) if j not in r_cols]].any()
    # dcls
    got_c = da[:, cls_off:cls_off + C].double().numpy()
    want_c = w[0] / N * g_f
    assert (np.abs(got_c - want_c) <= w[0] / N * ge_f + 16 * EPS32 * np.abs(want_c) + 1e-30).all()
    assert np.abs(want_c - R._rows(ref['dcls']).numpy()).max() <= 1e-9          # (the two float64 forms agree)
    assert not got_c[ref['weight'].numpy() == 0].any()                          # an invalid cell: exactly zero
    # dctr and dreg: zero off the positives, bounded on them
    pos = ref['pos']
    neg = torch.ones(da.shape[0], dtype=torch.bool)
    neg[pos] = False
    got_t = (dr if ctr_in_r else da)[:, ctr_off].double()
    want_t = R._rows(ref['dctr']).reshape(-1)
    assert not got_t[neg].any() and not dr[neg].any()
    assert ((got_t - want_t)[pos].abs() <= w[2] / N * 2 * ref['dctr_elem_err'] + 16 * EPS32 * want_t[pos].abs()).all()
    sc_row = torch.cat([torch.full((B * n,), s) for n, s in zip(N_L, ai.SCALES)]).double()
    got_r = dr[:, reg_off:reg_off + 4].double()
    want_r = R._rows(ref['draw'])
    e_v = w[1] / S * 4 * ref['dv_err']                                         # error of d loss / d(scale * raw)
    bound_r = sc_row[pos, None] * e_v + (16 * EPS32 + s_rel) * want_r[pos].abs()
    print('dreg: largest error', float((got_r - want_r)[pos].abs().max()), 'its bound', float(bound_r.max()))
    assert ((got_r - want_r)[pos].abs() <= bound_r + 1e-30).all(), float(((got_r - want_r)[pos].abs() - bound_r).max())
    # dscale_l = sum over the level's positives of d(scaled) * raw: the elements' bounds times |raw|, plus the summation
    raw_rows = R._rows(c['raw']).double()
    contrib = (w[1] / S * ref['dv'] * raw_rows[pos]).abs()
    for l in range(L):
        sel = torch.from_numpy(plv == l)
        bound = float((e_v[sel] * raw_rows[pos][sel].abs()).sum() + (40 * EPS32 + s_rel) * contrib[sel].sum())
        want = float(ref['dscale'][l])
        print('dscale', l, 'got', float(dsc[l]), 'float64', want, 'bound', bound)
        assert abs(float(dsc[l]) - want) <= bound + 4 * EPS32 * abs(want), (l, float(dsc[l]), want, bound)


@pytest.mark.parametrize('C,wide,ctr_in_r,invalid', [(4, False, True, False), (1, True, True, True), (4, True, False, False)])
def test_loss_and_gradients_against_float64(C, wide, ctr_in_r, invalid):
    c = _loss_case(LOSS_SEED[C], C, wide, ctr_in_r, weights=(1.0, 1.5, 0.5), clamp=True, invalid=invalid)
    got = _run_loss(c)
    ref = _ref(c)
    # preconditions: no pair of box edges (and no intersection length) within the fp32 error of an edge, 64 eps x the
    # largest coordinate (the clamped box is 16 * 62.5 * ... = 2000 px wide), so that every min / max / clamp selects in
    # fp32 what it selects in float64; no delta within that of the clamp other than the one beyond it
    assert ref['edge_gap'] > 64 * EPS32 * 2400
    dwh = ref['dn'][:, 2:].abs()
    assert ((dwh - R.MAX_RATIO).abs() > 1e-3).all() and (dwh > R.MAX_RATIO).sum() == 1
    _check_loss(c, got, ref)
    # the clamped width: its gradient is exactly 0 (without the clamp it would not be: a wider box has a larger union and
    # hull), the same row's height takes one
    reg_off = c['layout'].values[3]
    row = got[4][c['clamped']]
    assert c['clamped'] in ref['pos'].tolist() and row[reg_off + 2].item() == 0.0 and row[reg_off + 3].item() != 0.0
    again = _run_loss(c)
    for x, y in zip(got, again):            # the same bits from run to run
        assert torch.equal(x, y)


def test_loss_without_positives_is_exactly_zero():
    c = _loss_case(44, 4, True, no_gt=True, weights=(1.0, 2.0, 0.5))
    losses, coef, norm2, da, dr, dsc = _run_loss(c)
    assert norm2.tolist() == [2.0, 0.0]                         # sum over the two images of max(0, 1)
    assert not losses[1].any() and not losses[2].any() and (losses[0] > 0).all()
    assert not dr.any() and not dsc.any()
    assert da[:, 3:7].abs().sum().item() > 0 and not da[:, :3].any() and not da[:, 7:].any()
    assert np.allclose(coef.numpy(), [1.0 / 2.0, 2.0, 0.5 / 2.0], rtol=4 * EPS32)
    # one image of the batch: N = max(0, 1) = 1 and coef3 is the three loss weights
    meta = train_ops.AtssLossMeta(1, ai.SIZES, ai.STRIDES, base_table(), 4, [0, 0], 2.0, 0.25, 1e-6, 1.0, 2.0, 0.5, ai.MEANS, ai.STDS)
    cls, raw, ctr = ai.head_outputs(44, 4, batch=1)
    a, r, layout = make_rows(cls, raw, ctr)
    gi = torch.zeros(1, ai.ANCHORS, dtype=torch.int32, device=DEV)
    empty = torch.zeros(0, 4, device=DEV), torch.zeros(0, dtype=torch.long, device=DEV)
    losses, coef, norm2 = train_ops.atss_loss(a, r, scales_dev(), gi, *empty, layout, meta)
    assert coef.tolist() == [1.0, 2.0, 0.5] and norm2.tolist() == [1.0, 0.0] and not losses[1:].any()


def test_finalize_with_normalisers_averaged_by_hand():
    """norm2 changed between the sums and the division, as the mean over ranks does: losses and gradients follow the
    float64 run with the same normalisers"""
    c = _loss_case(44, 4, False)

    def hook(n2):
        n2.mul_(torch.tensor([0.75, 1.25], device=n2.device))
    got = _run_loss(c, hook)
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


@pytest.mark.parametrize('form', ['offset', 'fused', 'torch'])
@pytest.mark.parametrize('C,name', CASES)
def test_get_bboxes_golden(gold, monkeypatch, C, name, form):
    """the reference-signature get_bboxes on device tensors against the reference's detections: labels and order exact,
    boxes and scores within 2e-4; on the offset NMS branch and, with split_thr = 100 (132 .. 528 slots per image), on the
    per-class branch in both forms"""
    _force_form(monkeypatch, form)
    seed = int(gold[f'seed_bboxes_c{C}'])
    cfg = _split_cfg(ai.head_cfg(C), 0 if form == 'offset' else 100)
    head = build_head(ConfigDict(cfg)).eval()
    with torch.no_grad():
        for s, v in zip(head.scales, ai.SCALES):
            s.scale.fill_(v)
    head = head.to(DEV)
    cls, raw, ctr = ai.head_outputs(seed, C, empty=(name == 'empty'))
    dv = lambda lst: [t.to(DEV) for t in lst]    # noqa: E731
    res = head.get_bboxes(dv(cls), dv(ai.scaled(raw, ai.SCALES)), dv(ctr), ai.metas(), rescale=(name != 'plain'))
    for b, (det, lab) in enumerate(res):
        want_d, want_l = T(gold[f'bboxes_c{C}_{name}_det{b}']), T(gold[f'bboxes_c{C}_{name}_lab{b}'])
        assert lab.cpu().tolist() == want_l.tolist(), (C, name, form, b)
        assert det.shape == want_d.shape and torch.allclose(det.cpu(), want_d, rtol=0, atol=2e-4), (C, name, form, b)
    if name == 'empty':
        assert head.last_n_valid.tolist()[1] == 0 and len(res[1][0]) == 0 and len(res[0][0]) > 0


def test_loss_on_device_tensors_golden(gold):
    """the reference-signature loss on device tensors (assignment + loss kernels behind it) against the reference's values
    at the train iterations' tolerance, and its gradients w.r.t. the scaled deltas"""
    seed = int(gold['seed_loss_c4'])
    head = build(4, True)
    cls, raw, ctr = ai.head_outputs(seed, 4)
    gt_bboxes, gt_labels = ai.gts(seed)
    dv = lambda lst: [t.to(DEV).requires_grad_() for t in lst]    # noqa: E731
    dcls, dreg, dctr = dv(cls), dv(ai.scaled(raw, ai.SCALES)), dv(ctr)
    losses = head.loss(dcls, dreg, dctr, [g.to(DEV) for g in gt_bboxes], [l.to(DEV) for l in gt_labels], ai.metas())
    for k, v in losses.items():
        got = torch.stack(v).detach().cpu()
        assert torch.allclose(got, T(gold[f'loss_c4_{k}']), rtol=2e-3, atol=1e-4), (k, got, gold[f'loss_c4_{k}'])
    sum(sum(v) for v in losses.values()).backward()
    for l in range(L):
        # the fixture's gradient is w.r.t. the RAW delta: d raw = d scaled * scale
        assert torch.allclose(dreg[l].grad.cpu() * ai.SCALES[l], T(gold[f'loss_c4_dreg{l}']), rtol=2e-3, atol=1e-6), l
        assert torch.allclose(dcls[l].grad.cpu(), T(gold[f'loss_c4_dcls{l}']), rtol=2e-3, atol=1e-6), l
        assert torch.allclose(dctr[l].grad.cpu(), T(gold[f'loss_c4_dctr{l}']), rtol=2e-3, atol=1e-6), l


def _table(res):
    return np.concatenate([np.concatenate([r, np.full((len(r), 1), c, np.float32)], 1) for c, r in enumerate(res)], 0)


def _model(seed, split_thr=0):
    m = build_detector(ConfigDict(_split_cfg(ai.fixture_model_cfg(), split_thr)))
    m.load_state_dict(ai.fixture_state_dict(m, seed))
    return m.to(DEV)


@pytest.mark.parametrize('form', ['offset', 'fused', 'torch'])
def test_model_end_to_end_golden(gold, monkeypatch, form):
    """`model(return_loss=False)` against the reference's run of the same seeded model: per class the same detections in
    the same order, labels exact, boxes and scores within 2e-4 (g27's / g28's bound; the fixture's reference run is within
    5e-5 of its own float64 run).  `simple_test_device` runs under torch's synchronisation debug mode on 'error': the one
    host read of an inference call is the result copy."""
    _force_form(monkeypatch, form)
    seed = int(gold['seed_e2e'])
    m = _model(seed, 0 if form == 'offset' else 100).eval()
    img, _, _, _ = util.demo_inputs(2, ai.H, ai.W, seed=seed)
    img = img.to(DEV)
    with torch.no_grad():
        res = m(return_loss=False, rescale=True, img=[img], img_metas=[ai.metas()])
        assert len(m.last_n_valid) == 2 and all(n >= sum(len(r) for r in res[b]) > 0 for b, n in enumerate(m.last_n_valid))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            det, lab, nd = m.simple_test_device(img, ai.metas(), rescale=True)
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
    img, _, _, _ = util.demo_inputs(2, ai.H, ai.W, seed=seed, num_gt=ai.TRAIN_NUM_GT)
    gts, gls = ai.gts(seed)
    return img.to(DEV), [g.to(DEV) for g in gts], [l.to(DEV) for l in gls]


def test_no_host_read_in_the_head_train_step(gold):
    """`bbox_head.forward_train_nhwc` under torch's synchronisation debug mode on 'error': any blocking host read raises.
    The second image's pad_shape is smaller than the batch pad, so the valid-cell table is part of the step"""
    m = _model(int(gold['seed_e2e'])).train()
    img, gts, gls = _train_batch(int(gold['seed_train0']))
    feats = [f.detach() for f in m.extract_feat_nhwc(img)]
    metas = ai.metas(2, pads=[(ai.H, ai.W), (ai.H - 32, ai.W - 64)])
    m.bbox_head.forward_train_nhwc(feats, metas, gts, gls)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        losses = m.bbox_head.forward_train_nhwc(feats, metas, gts, gls)
        total = torch.stack([x for v in losses.values() for x in v]).sum()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert math.isfinite(float(total.detach()))
    gi = m.bbox_head.last_targets[0].cpu()
    assert (gi[0] >= 0).all() and (gi[1] == -1).any() and (gi[1] > 0).any()


def test_two_train_iterations_golden(gold):
    m = _model(int(gold['seed_e2e'])).train()
    for it in range(2):
        img, gts, gls = _train_batch(int(gold[f'seed_train{it}']))
        losses = m(img=img, img_metas=ai.metas(), gt_bboxes=gts, gt_labels=gls)
        assert sorted(losses) == ['loss_bbox', 'loss_centerness', 'loss_cls']
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
    """the criterion tests/test_fcos_gpu.py::test_model_16bit_close_to_fp32 applies to its 16-bit cases"""
    from brcnn import blocks
    seed = int(gold['seed_e2e'])
    m = _model(seed).eval()
    img, _, _, _ = util.demo_inputs(2, ai.H, ai.W, seed=seed)
    try:
        with torch.no_grad():
            f32 = [f.float() for f in m.extract_feat_nhwc(img.to(DEV))]
            r32 = m.simple_test(img.to(DEV), ai.metas())
            m.set_compute_dtype(dtype)
            f16 = m.extract_feat_nhwc(img.to(DEV))
            assert all(f.dtype == (torch.bfloat16 if dtype == 'bf16' else torch.float16) for f in f16)
            r16 = m.simple_test(img.to(DEV), ai.metas())
    finally:
        blocks.set_compute_dtype('f32')
    for a, b in zip(f16, f32):
        assert (a.float() - b).abs().max().item() / b.abs().max().item() < 0.05
    n32, n16 = sum(len(c) for r in r32 for c in r), sum(len(c) for r in r16 for c in r)
    assert n32 > 0 and abs(n16 - n32) <= 0.2 * n32 + 5, (n16, n32)
    d = np.concatenate([c for r in r32 for c in r]), np.concatenate([c for r in r16 for c in r])
    dist = np.abs(d[0][:, None, :4] - d[1][None, :, :4]).max(-1)
    ds = np.abs(d[0][:, None, 4] - d[1][None, :, 4])
    assert ((dist < 2.0) & (ds < 0.05)).any(1).mean() > 0.7


def test_inference_detector_returns_the_bbox2result_layout():
    from brcnn.apis import inference_detector, init_detector
    model = init_detector(ai.CONFIG, None, device=DEV)
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
    data = dict(img=img, img_metas=ai.metas(), gt_bboxes=gts, gt_labels=gls)
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
        assert runs[0][0] == runs[1][0]
        assert runs[0][1].keys() == runs[1][1].keys() and 'bbox_head.atss_centerness.weight' in runs[0][1]
        assert 'bbox_head.scales.4.scale' in runs[0][1]
        assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
        before = m.bbox_head.atss_cls.weight.detach().clone()
        opt.step()
        torch.cuda.synchronize()
        assert not torch.equal(before, m.bbox_head.atss_cls.weight.detach())
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
        spec = importlib.util.spec_from_file_location(f'brcnn_tool_{name}', os.path.join(ai.ROOT, 'tools', f'{name}.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    cfg = _tiny_cfg(tmp_path, max_epochs=1)
    cfg.model = Config.fromfile(ai.CONFIG).model
    cfg_path = str(tmp_path / 'tiny_atss.py')
    cfg.dump(cfg_path)
    work = str(tmp_path / 'work_gpu')
    runner = tool('train').main([cfg_path, '--work-dir', work, '--seed', '0', '--allow-random-init'])
    assert runner.epoch == 1 and os.path.exists(os.path.join(work, 'epoch_1.pth'))
    assert all(np.isfinite(v) for row in runner.history for v in row[3].values())
    assert any('loss_centerness' in row[3] and 'loss_bbox' in row[3] for row in runner.history) and len(runner.eval_history) == 1
    out_pkl = str(tmp_path / 'res.pkl')
    metric = tool('test').main([cfg_path, os.path.join(work, 'epoch_1.pth'), '--eval', 'bbox', '--out', out_pkl])
    assert metric == {} or 0.0 <= metric['bbox_mAP'] <= 1.0
    res = pickle.load(open(out_pkl, 'rb'))
    assert len(res) == 7 and len(res[0]) == len(CLASSES) and res[0][0].shape[1] == 5
