"""GPU tests of the FCOS baseline (csrc/fcos_head.hip, FCOSHead, FCOS).

Against the fixture g28_fcos.npz (tests/golden/make_golden_fcos.py; the reference's fp32 run): labels and kept order exact,
boxes and scores within the 2e-4 of g27's end-to-end cases (the fixture's reference run is within 5e-5 of its own float64
run), train losses within rtol 2e-3 / atol 1e-4 as tests/test_retinanet_gpu.py holds its own.
Against float64 (tests/fcos_ref64.py): bounds stated where used, derived from the fp32 arithmetic of the kernels (eps =
2^-23; an addition, product or division rounds to eps / 2, expf / logf / sqrtf are counted as 2 eps); none is tuned to what
the kernels give.  Preconditions on the inputs (rank gaps, distances to thresholds) are asserted."""
import math
import os

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import build_detector, build_head, ops, train_ops
from brcnn.config import ConfigDict
from tests import dense_loss_ref64 as RD
from tests import fcos_inputs as fi
from tests import fcos_ref64 as R
from tests import util

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G = os.path.join(os.path.dirname(__file__), 'golden', 'g28_fcos.npz')
EPS32 = float(np.finfo(np.float32).eps)
L = len(fi.SIZES)
N_L = [h * w for h, w in fi.SIZES]


@pytest.fixture(scope='module')
def gold():
    return {k: v for k, v in np.load(G, allow_pickle=False).items()}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def build(C=4, training=False, **over):
    head = build_head(ConfigDict(fi.head_cfg(C, **over))).train(training)
    with torch.no_grad():
        for s, v in zip(head.scales, fi.SCALES):
            s.scale.fill_(v)
    return head.to(DEV)


def test_the_library_has_the_fcos_entries():
    from brcnn import lib
    from brcnn.registry import DETECTORS, HEADS, LOSSES
    for name in ('brcnn_fcos_score', 'brcnn_fcos_decode_levels', 'brcnn_fcos_assign', 'brcnn_fcos_loss_workspace_bytes',
                 'brcnn_fcos_loss_forward', 'brcnn_fcos_loss_finalize', 'brcnn_fcos_loss_backward'):
        assert name in lib.SIGNATURES and hasattr(lib.load(), name)
    assert HEADS.get('FCOSHead') is not None and DETECTORS.get('FCOS') is not None and LOSSES.get('GIoULoss') is not None


# ------------------------------------------------------------------------------------------- layouts
def _rows(levels):
    return torch.cat([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in levels]).float()


def make_rows(cls, raw, ctr, ctr_in_r, wide, norm=False, giou=False):
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
    return a, rr, ops.FcosLayout(a, rr, C, cls_off, reg_off, ctr_in_r, ctr_off, norm, giou)


def scales_dev():
    return torch.tensor(fi.SCALES, dtype=torch.float32, device=DEV)


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
    out = ops.fcos_decode_levels([p[1] for p in picked], a, r, layout, scales_dev(), fi.SIZES, fi.STRIDES, max_shape, sf, thr)
    return raw, picked, out


def _check_candidates(cls, raw, ctr, C, norm, ctr_in_r, wide, rescale, B):
    metas = fi.metas(B)
    nms_pre, thr = fi.TEST_CFG['nms_pre'], fi.TEST_CFG['score_thr']
    a, r, layout = make_rows(cls, raw, ctr, ctr_in_r, wide, norm)
    scores, picked, (bb, sc, lb, va, nv) = _run_candidates(a, r, layout, metas, rescale, nms_pre, thr)
    ref = R.candidates(cls, raw, ctr, fi.SCALES, fi.SIZES, fi.STRIDES, norm, [m['img_shape'] for m in metas],
                       [m['scale_factor'] for m in metas] if rescale else None)
    sf = torch.tensor(np.stack([m['scale_factor'] for m in metas]).astype(np.float64)) if rescale else torch.ones(B, 4).double()
    # a sigmoid is exp (2 eps), an addition and a division: 3 eps relative; the product of two, one more rounding: <= 8 eps
    S_TOL = 8 * EPS32
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
        # box bound: v = scale * raw rounds once (|v| eps / 2 in the exponent), exp 2 eps, `* stride` / the edge px -+ d one
        # rounding each on a value of size <= |p| + d, the division by the scale factor one more: all within
        # 2 eps ((|v| + 4) d + |p| + d) / scale_factor
        s = fi.STRIDES[l]
        v = raw[l].double().permute(0, 2, 3, 1).reshape(B, n, 4) * fi.SCALES[l]
        d = v.clamp(min=0) * s if norm else v.exp()
        pmax = float(max(fi.H, fi.W))
        bnd = 2 * EPS32 * ((v.abs() + 4) * d + pmax + d)
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
    fin = torch.isfinite(bounds)
    assert ((got - boxes).abs()[fin] <= bounds[fin]).all(), float(((got - boxes).abs()[fin] - bounds[fin]).max())
    assert torch.equal(got[~fin], boxes[~fin])          # an overflowed distance: exactly the clipped edge
    return got, want_valid, sc.cpu()


@pytest.mark.parametrize('C,norm,ctr_in_r,wide,rescale', [(4, False, False, False, True), (1, True, True, True, True),
                                                         (3, False, True, True, False), (4, True, False, True, False)])
def test_score_topk_decode_against_float64(C, norm, ctr_in_r, wide, rescale):
    cls, raw, ctr = fi.head_outputs(11 + C, C, batch=3, norm_on_bbox=norm)
    _, valid, _ = _check_candidates(cls, raw, ctr, C, norm, ctr_in_r, wide, rescale, 3)
    assert valid.any() and not valid.all()


def test_an_overflowing_distance_gives_the_clipped_whole_image_box():
    """raw = 200: expf overflows to inf, px - inf = -inf -> 0, px + inf -> the image's own width / height; no NaN"""
    cls, raw, ctr = fi.head_outputs(5, 4, batch=3)
    for b in range(3):
        raw[1][b, :, 2, 3] = 200.0
        cls[1][b, :, 2, 3] = 6.0                 # certainly picked
        ctr[1][b, 0, 2, 3] = 6.0
    got, _, _ = _check_candidates(cls, raw, ctr, 4, False, False, False, False, 3)
    metas = fi.metas(3)
    for b in range(3):
        h, w = metas[b]['img_shape'][:2]
        slot = (fi.TEST_CFG['nms_pre'] + 0) * 4      # level 1's first pick: the point with the highest score
        assert got[b, slot].tolist() == [0.0, 0.0, float(w), float(h)]


def test_the_score_threshold_is_applied_before_the_centerness_factor():
    """a candidate whose class score passes score_thr = 0.05 but whose class score x centerness does not is VALID, as in
    multiclass_nms(..., score_factors=...); the kept detection carries the product as its score"""
    C = 4
    cls = [torch.full((2, C, h, w), -9.0) for h, w in fi.SIZES]
    raw = [torch.full((2, 4, h, w), float(np.log(1.5 * s))) for (h, w), s in zip(fi.SIZES, fi.STRIDES)]
    ctr = [torch.zeros(2, 1, h, w) for h, w in fi.SIZES]
    cls[2][0, 1, 2, 3] = math.log(0.06 / 0.94)          # class sigmoid 0.06 > 0.05
    ctr[2][0, 0, 2, 3] = math.log(0.1 / 0.9)            # centerness 0.1: product 0.006 < 0.05
    head = build(C)
    a, r, layout = make_rows(cls, raw, ctr, False, False)
    det, lab, num = head.get_bboxes_rows(a, r, layout, scales_dev(), fi.SIZES, fi.metas(), rescale=False)
    assert num.tolist() == [1, 0] and head.last_n_valid.tolist() == [1, 0]
    assert lab[0, 0].item() == 1 and abs(det[0, 0, 4].item() - 0.006) < 1e-6
    px, py, d = 3 * 32 + 16, 2 * 32 + 16, math.exp(1.1 * math.log(48.0))       # the Scale of level 2 is 1.1
    want = [max(px - d, 0), max(py - d, 0), min(px + d, fi.W - 3), min(py + d, fi.H)]
    assert np.allclose(det[0, 0, :4].cpu().numpy(), want, rtol=0, atol=1e-3)


def test_equal_products_are_ranked_by_index():
    """every point of a level with the same logits: all products are one fp32 value, the top-k keeps the lowest indices in
    ascending order (brcnn_rpn_topk's rule)"""
    C = 3
    cls, raw, ctr = fi.head_outputs(9, C)
    cls[0][:] = -2.0
    cls[0][:, 1] = -1.0
    ctr[0][:] = 0.5
    a, r, layout = make_rows(cls, raw, ctr, False, True)
    scores, picked, _ = _run_candidates(a, r, layout, fi.metas(), False, 50, 0.05)
    assert len(torch.unique(scores[0])) == 1
    assert torch.equal(picked[0][1].cpu(), torch.arange(50).expand(2, 50))


# ------------------------------------------------------------------------------------------- assignment
def _assign(gts, center, radius=1.5):
    offs = [0]
    for g in gts:
        offs.append(offs[-1] + len(g))
    flat = torch.cat([g.reshape(-1, 4) for g in gts]).float().contiguous().to(DEV)
    return train_ops.fcos_assign(flat, offs, len(gts), fi.SIZES, fi.STRIDES, fi.RANGES, center, radius).cpu().long()


def _point(level, y, x):
    """index of cell (y, x) of `level` among an image's points"""
    return sum(N_L[:level]) + y * fi.SIZES[level][1] + x


@pytest.mark.parametrize('center', [False, True])
def test_assign_against_the_restatement(gold, center):
    """gt_inds equal the restated assignment evaluated in float32 (the reference's own comparisons) AND in float64 (no
    decision of these inputs sits on a rounding edge), for: hand-placed edge cases, an image without ground truth, and the
    fixture's demo boxes with the large box (every level populated)"""
    hand = torch.tensor([[4., 0., 12., 12.],         # 0: the level-0 point (4, 4) lies ON its left edge: not inside
                         [8., 8., 28., 20.],         # 1: point (12, 12) has max distance 16 = level 0's upper bound: in
                         [8., 0., 40., 16.],         # 2: level-1 point (24, 8) has max distance 16 = level 1's lower bound: in
                         [100., 40., 140., 80.],     # 3, 4: equal areas (1600) over the level-1 point (120, 56), max
                         [110., 30., 150., 70.]])    #       distances 24 and 30: the lower index wins
    demo, _ = fi.gts(int(gold['seed_targets']))
    gts = [hand, torch.zeros(0, 4)] + demo
    got = _assign(gts, center, fi.RADIUS)
    for dtype in (torch.float32, torch.float64):
        want = torch.stack(R.assign(gts, fi.SIZES, fi.STRIDES, fi.RANGES, center, fi.RADIUS, dtype))
        assert torch.equal(got, want), (center, dtype, (got != want).nonzero()[:5])
    assert (got[1] == -1).all()
    if not center:
        assert got[0, _point(0, 0, 0)].item() == -1               # (4, 4): on the edge of box 0, inside nothing else
        assert got[0, _point(0, 1, 1)].item() == 1                # (12, 12): the inclusive upper bound
        assert got[0, _point(1, 0, 1)].item() == 2                # (24, 8): the inclusive lower bound
        assert got[0, _point(1, 3, 7)].item() == 3                # (120, 56): equal areas, lowest index
        assert (hand[3, 2] - hand[3, 0]) * (hand[3, 3] - hand[3, 1]) == (hand[4, 2] - hand[4, 0]) * (hand[4, 3] - hand[4, 1])
    starts = np.cumsum([0] + N_L)
    assert all((got[2:, starts[l]:starts[l + 1]] >= 0).any() for l in range(L))        # every level populated


def test_center_sampling_changes_the_assignment(gold):
    demo, _ = fi.gts(int(gold['seed_targets']))
    assert not torch.equal(_assign(demo, False), _assign(demo, True, fi.RADIUS))
    assert torch.equal(_assign(demo, False), _assign(demo, True, 1e6))        # a centre box as large as the box itself


# ------------------------------------------------------------------------------------------- loss
def _loss_case(seed, C, variant, wide, weights=(1.0, 1.0, 1.0), no_gt=False):
    over = fi.VARIANTS[variant]
    norm, giou, ctr_in_r = bool(over.get('norm_on_bbox', False)), variant == 'giou', bool(over.get('centerness_on_reg', False))
    cls, raw, ctr = fi.head_outputs(seed, C, norm_on_bbox=norm)
    gt_bboxes, gt_labels = fi.gts(seed, num_classes=C)
    if no_gt:
        gt_bboxes, gt_labels = [g[:0] for g in gt_bboxes], [l[:0] for l in gt_labels]
    a, r, layout = make_rows(cls, raw, ctr, ctr_in_r, wide, norm, giou)
    gts, labels, offs = train_ops.flatten_gts(gt_bboxes, gt_labels)
    gts, labels = gts.to(DEV), labels.to(DEV)
    gt_inds = train_ops.fcos_assign(gts, offs, 2, fi.SIZES, fi.STRIDES, fi.RANGES, over.get('center_sampling', False),
                                    over.get('center_sample_radius', 1.5))
    meta = train_ops.FcosLossMeta(2, fi.SIZES, fi.STRIDES, C, offs, 2.0, 0.25, 1e-6, 1e-6, *weights)
    inds64 = [g for g in gt_inds.cpu().long()]
    return dict(cls=cls, raw=raw, ctr=ctr, a=a, r=r, layout=layout, gts=gts, labels=labels, gt_inds=gt_inds, meta=meta,
                gt_bboxes=gt_bboxes, gt_labels=gt_labels, inds64=inds64, norm=norm, giou=giou, C=C, weights=weights)


def _run_loss(c, hook=None):
    a, r = c['a'].clone().requires_grad_(), c['r'].clone().requires_grad_()
    sc = scales_dev().requires_grad_()
    losses, coef, norm2 = train_ops.fcos_loss(a, r, sc, c['gt_inds'], c['gts'], c['labels'], c['layout'], c['meta'], hook)
    losses.sum().backward()
    return losses.detach().cpu(), coef.cpu(), norm2.cpu(), a.grad.cpu(), r.grad.cpu(), sc.grad.cpu()


def _check_loss(c, got, ref):
    """values and gradients against float64 with bounds from the kernels' fp32 arithmetic:
      * a sum of terms: the evaluation error of every term (the focal term's bound of tests/dense_loss_ref64.focal; for
        the box term twice the first-order error over each rounded intermediate, which tests/fcos_ref64.py records), plus
        the summation -- each
        partial goes through at most 8 sequential additions in a thread, 8 LDS tree levels, and the same again in the one
        finalize workgroup, then one addition per level: <= 40 eps of the sum of the absolute terms --, plus 4 eps for the
        division by the normaliser and the loss weight;
      * a gradient element: twice the first-order error of its expression (the backward chain re-uses the forward
        intermediates, and its partial sums are derivatives w.r.t. them, so their magnitudes are part of that bound;
        doubled once more for the chain's own roundings), plus 16 eps of its value for the coefficient and the products."""
    losses, coef, norm2, da, dr, dsc = got
    C, lay, B = c['C'], c['layout'].values, 2
    cls_off, reg_off, ctr_in_r, ctr_off = lay[1], lay[3], lay[4], lay[5]
    # the normalisers: the count is exact (an integer below 2^24; one rounding if a rank mean scaled it), the sum of the
    # centerness targets (5 eps each) carries n_pos + 16 eps relative -- and so does everything divided by it
    assert ref['n_pos'] > 5 and abs(norm2[0].item() - ref['norm2'][0]) <= EPS32 * ref['norm2'][0]
    s_rel = (ref['n_pos'] + 16) * EPS32
    assert abs(norm2[1].item() - ref['norm2'][1]) <= s_rel * ref['norm2'][1]
    N, S = max(ref['norm2'][0], 1.0), max(ref['norm2'][1], 1e-6)
    w = c['weights']
    # focal term of every (point, class)
    x = R._rows(c['cls']).double().numpy()
    hit = ref['labels'].numpy()[:, None] == np.arange(C)[None, :]
    t_f, g_f, te_f, ge_f = RD.focal(x, hit, 2.0, 0.25)
    tol = [w[0] / N * (te_f.sum() + 40 * EPS32 * t_f.sum()),
           w[1] / S * (2 * float(ref['box_value_err'].sum()) + (40 * EPS32 + s_rel) * ref['abs_terms'][1]),
           w[2] / N * (2 * float(ref['ctr_value_err'].sum()) + 40 * EPS32 * ref['abs_terms'][2])]
    for i in range(3):
        want = float(ref['losses'][i])
        print('loss', i, 'got', float(losses[i]), 'float64', want, 'bound', tol[i] + 4 * EPS32 * abs(want))
        assert abs(float(losses[i]) - want) <= tol[i] + 4 * EPS32 * abs(want), (i, float(losses[i]), want, tol[i])
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
    # dctr and dreg: zero off the positives, bounded on them
    pos = ref['pos']
    neg = torch.ones(da.shape[0], dtype=torch.bool)
    neg[pos] = False
    got_t = (dr if ctr_in_r else da)[:, ctr_off].double()
    want_t = R._rows(ref['dctr']).reshape(-1)
    assert not got_t[neg].any() and not dr[neg].any()
    assert ((got_t - want_t)[pos].abs() <= w[2] / N * 2 * ref['dctr_elem_err'] + 16 * EPS32 * want_t[pos].abs()).all()
    sc_row = torch.cat([torch.full((B * n,), s) for n, s in zip(N_L, fi.SCALES)]).double()
    got_r = dr[:, reg_off:reg_off + 4].double()
    want_r = R._rows(ref['draw'])
    e_v = w[1] / S * 4 * ref['dv_err']                                         # error of d loss / d(scale * raw)
    bound_r = sc_row[pos, None] * e_v + (16 * EPS32 + s_rel) * want_r[pos].abs()
    print('dreg: largest error', float((got_r - want_r)[pos].abs().max()), 'its bound', float(bound_r.max()))
    assert ((got_r - want_r)[pos].abs() <= bound_r + 1e-30).all(), float(((got_r - want_r)[pos].abs() - bound_r).max())
    # dscale_l = sum over the level's positives of d(scaled) * raw: the elements' bounds times |raw|, plus the summation
    raw_rows = R._rows(c['raw']).double()
    contrib = (w[1] / S * ref['dv'] * raw_rows[pos]).abs()
    starts = np.cumsum([0] + [B * n for n in N_L])
    for l in range(L):
        sel = (pos >= starts[l]) & (pos < starts[l + 1])
        bound = float((e_v[sel] * raw_rows[pos][sel].abs()).sum() + (40 * EPS32 + s_rel) * contrib[sel].sum())
        want = float(ref['dscale'][l])
        print('dscale', l, 'got', float(dsc[l]), 'float64', want, 'bound', bound)
        assert abs(float(dsc[l]) - want) <= bound + 4 * EPS32 * abs(want), (l, float(dsc[l]), want, bound)


@pytest.mark.parametrize('variant,C,wide', [('iou', 4, False), ('giou', 4, True), ('iou', 1, True), ('giou', 1, False)])
def test_loss_and_gradients_against_float64(variant, C, wide):
    c = _loss_case(40 + C, C, variant, wide, weights=(1.0, 1.5, 0.5))
    got = _run_loss(c)
    ref = R.loss(c['cls'], c['raw'], c['ctr'], fi.SCALES, c['inds64'], c['gt_bboxes'], c['gt_labels'], fi.SIZES, fi.STRIDES,
                 c['norm'], c['giou'], weights=c['weights'])
    # preconditions: no pair of box edges (and no intersection length) within the fp32 error of an edge, 4 eps x the
    # largest coordinate, so that every min / max / clamp selects in fp32 what it selects in float64; under norm_on_bbox
    # the relu branch runs
    assert ref['edge_gap'] > 64 * EPS32 * (fi.W + 200)
    if c['norm']:
        assert (ref['scaled'] < 0).any()
    _check_loss(c, got, ref)
    again = _run_loss(c)
    for x, y in zip(got, again):            # the same bits from run to run
        assert torch.equal(x, y)


def test_loss_without_positives_is_exactly_zero():
    c = _loss_case(44, 4, 'giou', True, no_gt=True)
    losses, coef, norm2, da, dr, dsc = _run_loss(c)
    assert norm2.tolist() == [0.0, 0.0] and losses[1].item() == 0.0 and losses[2].item() == 0.0 and losses[0].item() > 0
    assert not dr.any() and not dsc.any()
    assert da[:, 3:7].abs().sum().item() > 0 and not da[:, :3].any() and not da[:, 7:].any()
    assert np.allclose(coef.numpy(), [1.0, 1e6, 1.0], rtol=4 * EPS32)


def test_finalize_with_normalisers_averaged_by_hand():
    """norm2 changed between the sums and the division, as the mean over ranks does: losses and gradients follow the
    float64 run with the same normalisers"""
    c = _loss_case(44, 4, 'iou', False)

    def hook(n2):
        n2.mul_(torch.tensor([0.75, 1.25], device=n2.device))
    got = _run_loss(c, hook)
    plain = R.loss(c['cls'], c['raw'], c['ctr'], fi.SCALES, c['inds64'], c['gt_bboxes'], c['gt_labels'], fi.SIZES, fi.STRIDES,
                   grads=False)
    n2 = [plain['norm2'][0] * 0.75, plain['norm2'][1] * 1.25]
    ref = R.loss(c['cls'], c['raw'], c['ctr'], fi.SCALES, c['inds64'], c['gt_bboxes'], c['gt_labels'], fi.SIZES, fi.STRIDES,
                 norm2=n2)
    assert ref['norm2'] == n2 and not np.allclose(ref['losses'].numpy(), plain['losses'].numpy(), rtol=0.1)
    _check_loss(c, got, ref)


# ------------------------------------------------------------------------------------------- the fixture
CASES = [(c, name) for c in fi.CLASS_COUNTS for name in ('plain', 'rescale', 'norm')] + [(4, 'empty')]


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
    norm = name == 'norm'
    cfg = _split_cfg(fi.head_cfg(C, norm_on_bbox=norm), 0 if form == 'offset' else 100)
    head = build_head(ConfigDict(cfg)).eval()
    with torch.no_grad():
        for s, v in zip(head.scales, fi.SCALES):
            s.scale.fill_(v)
    head = head.to(DEV)
    cls, raw, ctr = fi.head_outputs(seed, C, norm_on_bbox=norm, empty=(name == 'empty'))
    dec = fi.decoded(raw, fi.SCALES, norm, False)
    dv = lambda lst: [t.to(DEV) for t in lst]    # noqa: E731
    res = head.get_bboxes(dv(cls), dv(dec), dv(ctr), fi.metas(), rescale=(name != 'plain'))
    for b, (det, lab) in enumerate(res):
        want_d, want_l = T(gold[f'bboxes_c{C}_{name}_det{b}']), T(gold[f'bboxes_c{C}_{name}_lab{b}'])
        assert lab.cpu().tolist() == want_l.tolist(), (C, name, form, b)
        assert det.shape == want_d.shape and torch.allclose(det.cpu(), want_d, rtol=0, atol=2e-4), (C, name, form, b)
    if name == 'empty':
        assert head.last_n_valid.tolist()[1] == 0 and len(res[1][0]) == 0 and len(res[0][0]) > 0


def _table(res):
    return np.concatenate([np.concatenate([r, np.full((len(r), 1), c, np.float32)], 1) for c, r in enumerate(res)], 0)


def _model(seed, split_thr=0):
    m = build_detector(ConfigDict(_split_cfg(fi.fixture_model_cfg(), split_thr)))
    m.load_state_dict(fi.fixture_state_dict(m, seed))
    return m.to(DEV)


@pytest.mark.parametrize('form', ['offset', 'fused', 'torch'])
def test_model_end_to_end_golden(gold, monkeypatch, form):
    """`model(return_loss=False)` against the reference's run of the same seeded model: per class the same detections in
    the same order, labels exact, boxes and scores within 2e-4 (g27's bound; the fixture's reference run is within 5e-5
    of its own float64 run).  `simple_test_device` runs under torch's synchronisation debug mode on 'error': the one host
    read of an inference call is the result copy."""
    _force_form(monkeypatch, form)
    seed = int(gold['seed_e2e'])
    m = _model(seed, 0 if form == 'offset' else 100).eval()
    img, _, _, _ = util.demo_inputs(2, fi.H, fi.W, seed=seed)
    img = img.to(DEV)
    with torch.no_grad():
        res = m(return_loss=False, rescale=True, img=[img], img_metas=[fi.metas()])
        assert len(m.last_n_valid) == 2 and all(n >= sum(len(r) for r in res[b]) > 0 for b, n in enumerate(m.last_n_valid))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            det, lab, nd = m.simple_test_device(img, fi.metas(), rescale=True)
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
    img, _, _, _ = util.demo_inputs(2, fi.H, fi.W, seed=seed, num_gt=fi.TRAIN_NUM_GT)
    gts, gls = fi.gts(seed)
    return img.to(DEV), [g.to(DEV) for g in gts], [l.to(DEV) for l in gls]


def test_no_host_read_in_the_head_train_step(gold):
    """`bbox_head.forward_train_nhwc` under torch's synchronisation debug mode on 'error': any blocking host read raises"""
    m = _model(int(gold['seed_e2e'])).train()
    img, gts, gls = _train_batch(int(gold['seed_train0']))
    feats = [f.detach() for f in m.extract_feat_nhwc(img)]
    m.bbox_head.forward_train_nhwc(feats, fi.metas(), gts, gls)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        losses = m.bbox_head.forward_train_nhwc(feats, fi.metas(), gts, gls)
        total = torch.stack(list(losses.values())).sum()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert math.isfinite(float(total.detach()))


def test_two_train_iterations_golden(gold):
    m = _model(int(gold['seed_e2e'])).train()
    for it in range(2):
        img, gts, gls = _train_batch(int(gold[f'seed_train{it}']))
        losses = m(img=img, img_metas=fi.metas(), gt_bboxes=gts, gt_labels=gls)
        assert sorted(losses) == ['loss_bbox', 'loss_centerness', 'loss_cls']
        for k, v in losses.items():
            got = v.detach().cpu().double().reshape(-1)
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
    """the criterion tests/test_retinanet_gpu.py::test_model_16bit_close_to_fp32 applies to its 16-bit cases"""
    from brcnn import blocks
    seed = int(gold['seed_e2e'])
    m = _model(seed).eval()
    img, _, _, _ = util.demo_inputs(2, fi.H, fi.W, seed=seed)
    try:
        with torch.no_grad():
            f32 = [f.float() for f in m.extract_feat_nhwc(img.to(DEV))]
            r32 = m.simple_test(img.to(DEV), fi.metas())
            m.set_compute_dtype(dtype)
            f16 = m.extract_feat_nhwc(img.to(DEV))
            assert all(f.dtype == (torch.bfloat16 if dtype == 'bf16' else torch.float16) for f in f16)
            r16 = m.simple_test(img.to(DEV), fi.metas())
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
    model = init_detector(fi.CONFIG, None, device=DEV)
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
    data = dict(img=img, img_metas=fi.metas(), gt_bboxes=gts, gt_labels=gls)
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
        assert runs[0][1].keys() == runs[1][1].keys() and 'bbox_head.conv_centerness.weight' in runs[0][1]
        assert 'bbox_head.scales.4.scale' in runs[0][1]
        assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
        before = m.bbox_head.conv_cls.weight.detach().clone()
        opt.step()
        torch.cuda.synchronize()
        assert not torch.equal(before, m.bbox_head.conv_cls.weight.detach())
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
        spec = importlib.util.spec_from_file_location(f'brcnn_tool_{name}', os.path.join(fi.ROOT, 'tools', f'{name}.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    cfg = _tiny_cfg(tmp_path, max_epochs=1)
    cfg.model = Config.fromfile(fi.CONFIG).model
    cfg_path = str(tmp_path / 'tiny_fcos.py')
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
