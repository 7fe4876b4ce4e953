"""GPU tests of the RetinaNet baseline (csrc/dense_head.hip, RetinaHead, SingleStageDetector / RetinaNet).

Against the fixture g27_retinanet.npz (tests/golden/make_golden_retinanet.py; the reference's fp32 run): labels and kept
order exact, boxes and scores within the 2e-4 of the g25 end-to-end cases (the fixture's reference run is within 5e-5 of
its own float64 run), train losses within rtol 2e-3 / atol 1e-4 as tests/test_faster_rcnn_gpu.py holds its own.
Against float64 (written here and in tests/dense_loss_ref64.py): bounds stated where used, derived from the fp32
arithmetic of the kernels; none is tuned to what the kernels give."""
import math
import os

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import build_detector, build_head, ops
from brcnn.config import ConfigDict
from brcnn.core import anchor_inside_flags
from tests import dense_loss_ref64 as R
from tests import retinanet_inputs as ri
from tests import util

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G = os.path.join(os.path.dirname(__file__), 'golden', 'g27_retinanet.npz')
EPS32 = float(np.finfo(np.float32).eps)
A = ri.A


@pytest.fixture(scope='module')
def gold():
    return {k: v for k, v in np.load(G, allow_pickle=False).items()}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_the_library_has_the_dense_head_entries():
    from brcnn import lib
    from brcnn.registry import DETECTORS, HEADS
    for name in ('brcnn_dense_score', 'brcnn_dense_decode_levels', 'brcnn_dense_loss_forward', 'brcnn_dense_loss_finalize',
                 'brcnn_dense_loss_backward', 'brcnn_dense_loss_workspace_bytes'):
        assert name in lib.SIGNATURES and hasattr(lib.load(), name)
    assert HEADS.get('RetinaHead') is not None and DETECTORS.get('RetinaNet') is not None
    assert DETECTORS.get('SingleStageDetector') is not None


# ------------------------------------------------------------------------------------------- score + top-k + decode
def _nhwc(ts, pad=0, off=0):
    """reference-layout (B, ch, h, w) -> NHWC on the device; with `pad` the tensor is `pad` channels wider and the head
    output a channel slice at offset `off` of it (the in-place strided read)"""
    out = []
    for t in ts:
        x = t.permute(0, 2, 3, 1).contiguous()
        if pad:
            wide = torch.full(tuple(x.shape[:3]) + (x.shape[3] + pad,), 7.5)
            wide[..., off:off + x.shape[3]] = x
            out.append(wide.to(DEV)[..., off:off + x.shape[3]])
        else:
            out.append(x.to(DEV))
    return out


def _candidates64(head, cls, reg, metas, C, rescale, nms_pre, thr):
    """float64 restatement of anchor_head.py:640-710 up to multiclass_nms' candidate list: per level the picked anchors
    (descending maximum class sigmoid, ties by ascending index), their decoded boxes fanned out to classes.  Returns per
    level the picks (B, k_l) and overall boxes (B, T*C, 4), their magnitudes, scores (B, T*C), plus the smallest gap
    between two neighbouring ranks among the picks and the rank after them"""
    B = cls[0].shape[0]
    anchors = head.anchor_generator.grid_anchors(ri.SIZES, 'cpu')
    lim = abs(math.log(16 / 1000))
    picks, boxes, mags, scores, gap = [], [], [], [], np.inf
    hi = torch.tensor([[m['img_shape'][1], m['img_shape'][0]] * 2 for m in metas], dtype=torch.float64)
    sf = torch.tensor(np.stack([m['scale_factor'] for m in metas]).astype(np.float64))
    for c_, r_, an in zip(cls, reg, anchors):
        s = c_.double().permute(0, 2, 3, 1).reshape(B, -1, C).sigmoid()
        # the kernels rank the fp32 values: round the float64 sigmoid the way one fp32 evaluation does
        s32 = s.float()
        d = r_.double().permute(0, 2, 3, 1).reshape(B, -1, 4)
        n = s.shape[1]
        if n > nms_pre:
            m = s32.max(-1)[0]
            ranked, idx = m.sort(dim=1, descending=True, stable=True)
            r64 = torch.gather(s.max(-1)[0], 1, idx)
            gap = min(gap, float((r64[:, :nms_pre] - r64[:, 1:nms_pre + 1]).abs().min()))
            idx = idx[:, :nms_pre]
        else:
            idx = torch.arange(n).expand(B, n)
        picks.append(idx)
        s, d = torch.gather(s, 1, idx[..., None].expand(-1, -1, C)), torch.gather(d, 1, idx[..., None].expand(-1, -1, 4))
        an = an.double()[idx]
        px, py = (an[..., 0] + an[..., 2]) * 0.5, (an[..., 1] + an[..., 3]) * 0.5
        pw, ph = an[..., 2] - an[..., 0], an[..., 3] - an[..., 1]
        gw, gh = pw * d[..., 2].clamp(-lim, lim).exp(), ph * d[..., 3].clamp(-lim, lim).exp()
        gx, gy = px + pw * d[..., 0], py + ph * d[..., 1]
        box = torch.stack([gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5], -1)
        mag = torch.stack([gx.abs() + gw, gy.abs() + gh, gx.abs() + gw, gy.abs() + gh], -1)
        box = torch.minimum(box.clamp(min=0), hi[:, None, :])
        if rescale:
            box, mag = box / sf[:, None, :], mag / sf[:, None, :]
        k = idx.shape[1]
        boxes.append(box[:, :, None, :].expand(B, k, C, 4).reshape(B, k * C, 4))
        mags.append(mag[:, :, None, :].expand(B, k, C, 4).reshape(B, k * C, 4))
        scores.append(s.reshape(B, k * C))
    return picks, torch.cat(boxes, 1), torch.cat(mags, 1), torch.cat(scores, 1), gap


def _run_candidates(head, cls_nhwc, reg_nhwc, metas, C, rescale, nms_pre, thr):
    B = cls_nhwc[0].shape[0]
    raw = [ops.dense_score(c, A, C).view(B, -1) for c in cls_nhwc]
    picked = ops.rpn_topk(raw, nms_pre)
    max_shape = torch.tensor([m['img_shape'][:2] for m in metas], dtype=torch.float32, device=DEV)
    sf = torch.tensor(np.stack([m['scale_factor'] for m in metas]), dtype=torch.float32, device=DEV) if rescale else None
    out = ops.dense_decode_levels([p[1] for p in picked], cls_nhwc, reg_nhwc,
                                  [head.anchor_generator.base_anchors[l].to(DEV) for l in range(len(ri.SIZES))], ri.SIZES,
                                  list(head.anchor_generator.strides), C, max_shape, sf, head.bbox_coder.means,
                                  head.bbox_coder.stds, thr)
    return raw, picked, out


@pytest.mark.parametrize('rescale', [False, True])
@pytest.mark.parametrize('C,pad,off', [(4, 0, 0), (1, 0, 0), (3, 0, 0), (4, 7, 3), (1, 5, 0)])
def test_score_topk_decode_against_float64(gold, C, pad, off, rescale):
    """the 64 x 96 pyramid (8x12 .. 1x1, A = 9) at nms_pre = 50: three levels (864 / 216 / 54 anchors) go through the
    select, two (18 / 9) pass through whole, the n_l <= k branch.  Picked indices, labels, valid and n_valid exact; scores within 4 eps32 of the float64 sigmoid (expf to 2 ulp,
    one addition, one division); boxes within 8 eps32 of (|centre| + size), the bound of
    tests/test_faster_rcnn_gpu.py::test_rcnn_decode_plain_against_float64 for the same six operations.
    `pad`: the head tensors are wider than A*C / 4A and read in place.  Image 1 has the smaller img_shape (clip border)
    and its own scale factor."""
    seed, thr, k = int(gold[f'seed_bboxes_c{min(C, 4)}']), 0.05, 50
    head = build_head(ConfigDict(ri.head_cfg(C)))
    cls, reg = ri.head_outputs(seed, C)
    metas = ri.metas()
    picks, box64, mag, s64, gap = _candidates64(head, cls, reg, metas, C, rescale, k, thr)
    # preconditions on the INPUTS: a score (<= 1) is within 4 eps32 of its float64 value, so two ranks further apart than
    # 8 eps32 keep their order and a score further than 4 eps32 from the threshold keeps its side
    assert gap > 8 * EPS32 and float((s64 - thr).abs().min()) > 4 * EPS32
    raw, picked, (bb, sc, lb, va, nv) = _run_candidates(head, _nhwc(cls, pad, off), _nhwc(reg, pad, off), metas, C, rescale, k, thr)
    for l, (h, w) in enumerate(ri.SIZES):
        n = h * w * A
        assert picked[l][1].shape == (2, min(k, n))
        assert torch.equal(picked[l][1].cpu(), picks[l]), l
        m64 = cls[l].double().permute(0, 2, 3, 1).reshape(2, n, C).sigmoid().max(-1)[0]
        assert ((raw[l].cpu().double() - m64).abs() <= 4 * EPS32 * m64).all()
    Tn = sum(p.shape[1] for p in picks)
    assert bb.shape == (2, Tn * C, 4) and Tn == 50 + 50 + 50 + 18 + 9
    assert torch.equal(lb.cpu(), torch.arange(C).repeat(2, Tn))
    assert torch.equal(va.cpu(), s64 > thr)
    assert nv.dtype == torch.int32 and nv.tolist() == (s64 > thr).sum(1).tolist() and min(nv.tolist()) > 0
    assert ((sc.cpu().double() - s64).abs() <= 4 * EPS32 * s64).all()
    assert ((bb.cpu().double() - box64).abs() <= 8 * EPS32 * mag + 1e-30).all()
    # the clip border is the image's own: something of image 1 sits on it
    hw = metas[1]['img_shape']
    edge = torch.tensor([hw[1], hw[0]] * 2, dtype=torch.float64) / (torch.tensor(metas[1]['scale_factor']).double() if rescale else 1.0)
    assert ((box64[1] - edge).abs() < 1e-9).any()


def test_equal_sigmoids_are_ranked_by_index():
    """two logits (20 and 25) whose fp32 sigmoids are both exactly 1.0: `topk` on the sigmoid values cannot tell them
    apart, and the index-ascending tie rule puts anchor 100 before anchor 700 although its logit is smaller; a ranking
    by logit would swap them.  A third anchor ties with them through another class."""
    C, k = 4, 50
    head = build_head(ConfigDict(ri.head_cfg(C)))
    cls, reg = ri.head_outputs(11, C)
    flat = cls[0].permute(0, 2, 3, 1).reshape(2, -1, C)      # (a copy: write back below)
    flat[0, 700, 0], flat[0, 100, 2], flat[0, 400, 3] = 25.0, 20.0, 30.0
    cls[0] = flat.reshape(2, 8, 12, A * C).permute(0, 3, 1, 2).contiguous()
    assert float(torch.tensor(20.0).sigmoid()) == 1.0
    raw, picked, (bb, sc, lb, va, nv) = _run_candidates(head, _nhwc(cls), _nhwc(reg), ri.metas(), C, False, k, 0.05)
    assert picked[0][1][0, :3].tolist() == [100, 400, 700]
    assert picked[0][0][0, :3].tolist() == [1.0, 1.0, 1.0]
    assert sc[0, :3 * C].view(3, C).max(1)[0].tolist() == [1.0, 1.0, 1.0] and lb[0, :3 * C].view(3, C)[0].tolist() == [0, 1, 2, 3]


CASES = [(c, name) for c in ri.CLASS_COUNTS for name in ('plain', 'rescale')] + [(4, 'empty')]


@pytest.mark.parametrize('C,name', CASES)
def test_get_bboxes_golden(gold, C, name):
    """RetinaHead.get_bboxes on the device against the reference's: the same detections in the same order (labels exact),
    boxes and scores within 2e-4; 'empty': nothing of image 1 passes score_thr -- n_valid 0, no detection"""
    seed = int(gold[f'seed_bboxes_c{C}'])
    head = build_head(ConfigDict(ri.head_cfg(C))).to(DEV).eval()
    cls, reg = ri.head_outputs(seed, C, empty=(name == 'empty'))
    res = head.get_bboxes([c.to(DEV) for c in cls], [r.to(DEV) for r in reg], ri.metas(), rescale=(name != 'plain'))
    for b, (det, lab) in enumerate(res):
        want_d, want_l = T(gold[f'bboxes_c{C}_{name}_det{b}']), T(gold[f'bboxes_c{C}_{name}_lab{b}'])
        assert lab.cpu().tolist() == want_l.tolist(), (C, name, b)
        assert det.shape == want_d.shape and torch.allclose(det.cpu(), want_d, rtol=0, atol=2e-4), (C, name, b)
    if name == 'empty':
        assert head.last_n_valid.tolist()[1] == 0 and len(res[1][0]) == 0 and len(res[0][0]) > 0


# ------------------------------------------------------------------------------------------- loss vs float64
LOSS_CASES = {
    # name: (C, loss_bbox, pos_weight, allowed_border, padded)
    'l1_c4': (4, dict(type='L1Loss', loss_weight=1.0), -1, -1, False),
    'smooth_l1_c1': (1, dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=2.0), -1, -1, False),
    'pos_weight': (4, dict(type='L1Loss', loss_weight=1.0), 2.5, -1, False),
    'border': (4, dict(type='L1Loss', loss_weight=1.0), -1, 0, True),
}


def _loss_case(name):
    C, loss_bbox, pos_weight, border, padded = LOSS_CASES[name]
    cfg = ri.head_cfg(C, loss_bbox=loss_bbox)
    cfg['train_cfg'].update(pos_weight=pos_weight, allowed_border=border)
    head = build_head(ConfigDict(cfg)).to(DEV).train()
    cls, reg = ri.head_outputs(31, C, batch=3)
    cls = [c + 3.0 for c in cls]                    # logits around -3: both sides of the focal term carry weight
    # image 0: a 32 x 32 box on a level-0 anchor, an 85 x 57 box for level 1, and a 6 x 5 box of the LAST class that no
    # anchor overlaps by 0.1 -- a low-quality match; image 1: no ground truth (max(n_pos, 1)); image 2: two boxes
    gts = [torch.tensor([[12., 12., 44., 44.], [5., 3., 90., 60.], [50., 20., 56., 25.]]), torch.zeros(0, 4),
           torch.tensor([[30., 8., 70., 50.], [2., 30., 40., 62.]])]
    labels = [torch.tensor([0, C // 2, C - 1]), torch.zeros(0, dtype=torch.long), torch.tensor([C - 1, 0])]
    metas = ri.metas(3)
    if padded:      # the batch is padded beyond image 1's own pad_shape: some of its cells hold no valid anchor
        metas[1] = dict(metas[1], pad_shape=(56, 80, 3), img_shape=(50, 75, 3))
    return head, C, cls, reg, gts, labels, metas


def _host_gt_inds(head, gts, metas):
    """AnchorHead._get_targets_single's assignment on the host: -1 outside the image / invalid / ignore band"""
    sizes = [torch.Size(s) for s in ri.SIZES]
    anchors = torch.cat(head.anchor_generator.grid_anchors(sizes, 'cpu'))
    out = []
    for g, m in zip(gts, metas):
        flags = torch.cat(head.anchor_generator.valid_flags(sizes, m['pad_shape'], 'cpu'))
        inside = anchor_inside_flags(anchors, flags, m['img_shape'][:2], head.train_cfg.allowed_border)
        gi = torch.full((len(anchors),), -1, dtype=torch.long)
        gi[inside] = head.assigner.assign(anchors[inside], g, None, None).gt_inds
        out.append(gi)
    return anchors, torch.stack(out)


@pytest.mark.parametrize('name', list(LOSS_CASES))
def test_dense_loss_against_float64(name):
    """per-level values and both gradients of brcnn_dense_loss_* against tests/dense_loss_ref64.py, on head outputs that
    are WIDER than A*C / 4A (the padded layout of the training convs, garbage in the padding of the inputs).

    Bounds (dense_loss_ref64.dense_loss): a level's sum within (n + 8) eps32 sum|terms| (any fixed summation order) plus
    the summed fp32 evaluation error of its terms (the sigmoid's cancellation in 1 - p, the encoded targets); a
    gradient element within its own evaluation bound; an L1 sign only where |pred - target| exceeds the target's error.
    The padding columns of both gradients are zero, and two runs give the same bits."""
    head, C, cls, reg, gts, labels, metas = _loss_case(name)
    anchors, gt_inds = _host_gt_inds(head, gts, metas)
    offs = [0]
    for g in gts:
        offs.append(offs[-1] + len(g))
    # what the case is about, stated on the targets
    assert (gt_inds == -1).any() and (gt_inds[1] <= 0).all() and (gt_inds[0] == 3).sum() >= 1
    lv = np.concatenate([[0], np.cumsum([h * w * A for h, w in ri.SIZES])])
    per_level_pos = [int((gt_inds[:, lv[l]:lv[l + 1]] > 0).sum()) for l in range(5)]
    assert per_level_pos[0] > 0 and per_level_pos[2:] == [0, 0, 0], per_level_pos       # levels with no positive
    if name == 'border':        # only anchors inside the image count; image 1's padding leaves cells without a valid anchor
        assert (gt_inds == -1).sum() > gt_inds.numel() // 2
        assert not all(head.anchor_generator.valid_flags([torch.Size(s) for s in ri.SIZES], metas[1]['pad_shape'], 'cpu')[0])
    else:
        assert per_level_pos[1] > 0
    cfgb = LOSS_CASES[name]
    x, p, level_sizes = R.flatten_outputs([c.numpy() for c in cls], [r.numpy() for r in reg], C)
    ref = R.dense_loss(x, p, level_sizes, anchors.numpy(), gt_inds.numpy(), torch.cat(gts).numpy(), torch.cat(labels).numpy(),
                       offs, pos_weight=cfgb[2], beta=cfgb[1].get('beta', 0.0), lw_bbox=cfgb[1]['loss_weight'])
    assert ref['num_total_pos'] == int(np.maximum(ref['n_pos'], 1).sum()) and ref['n_pos'][1] == 0

    def rows(ts, width):
        y = torch.cat([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in ts], 0)
        wide = torch.full((y.shape[0], width), 3.25)
        wide[:, :y.shape[1]] = y
        return wide.to(DEV).requires_grad_()

    runs = []
    for _ in range(2):
        yc, yr = rows(cls, 64), rows(reg, 64)
        losses = head.loss_fused(yc, yr, tuple(ri.SIZES), [g.to(DEV) for g in gts], [l.to(DEV) for l in labels], metas)
        assert torch.equal(head.last_targets[0].cpu().long(), gt_inds)
        lc, lb = torch.stack(losses['loss_cls']), torch.stack(losses['loss_bbox'])
        (lc.sum() + lb.sum()).backward()
        runs.append((lc.detach().cpu(), lb.detach().cpu(), yc.grad.cpu(), yr.grad.cpu()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    lc, lb, dyc, dyr = runs[0]
    coef = head.last_targets[1].cpu()
    assert float(coef[2]) == ref['num_total_pos']
    assert (np.abs(lc.double().numpy() - ref['loss_cls']) <= ref['tol_cls']).all(), (lc, ref['loss_cls'], ref['tol_cls'])
    assert (np.abs(lb.double().numpy() - ref['loss_bbox']) <= ref['tol_bbox']).all(), (lb, ref['loss_bbox'], ref['tol_bbox'])
    assert float(lb[4]) == 0.0 and float(lb[0]) > 0
    assert not dyc[:, A * C:].any() and not dyr[:, 4 * A:].any()
    B = 3
    got_c = np.concatenate([dyc[3 * lv[l] // A:3 * lv[l + 1] // A, :A * C].double().numpy().reshape(B, -1, C)
                            for l in range(5)], 1)
    got_r = np.concatenate([dyr[3 * lv[l] // A:3 * lv[l + 1] // A, :4 * A].double().numpy().reshape(B, -1, 4)
                            for l in range(5)], 1)
    assert (np.abs(got_c - ref['dx']) <= ref['dx_err'] + 1e-30).all(), float((np.abs(got_c - ref['dx']) - ref['dx_err']).max())
    ok = ref['dpred_sure']
    assert ok.mean() > 0.99 and (np.abs(got_r - ref['dpred'])[ok] <= ref['dpred_err'][ok] + 1e-30).all()
    assert not got_c[gt_inds.numpy() < 0].any() and not got_r[gt_inds.numpy() <= 0].any()


# ------------------------------------------------------------------------------------------- the model vs the fixture
def _table(res):
    return np.concatenate([np.concatenate([r, np.full((len(r), 1), c, np.float32)], 1) for c, r in enumerate(res)], 0)


def _model(seed):
    m = build_detector(ConfigDict(ri.fixture_model_cfg()))
    m.load_state_dict(ri.fixture_state_dict(m, seed))
    return m.to(DEV)


def test_model_end_to_end_golden(gold):
    """`model(return_loss=False)` against the reference's run of the same seeded model: per class the same number of
    detections in the same order, labels exact, boxes and scores within 2e-4 (the bound of g25's end-to-end cases; the
    fixture's reference run is within 5e-5 of its own float64 run, `e2e_ref_err`)"""
    seed = int(gold['seed_e2e'])
    m = _model(seed).eval()
    img, _, _, _ = util.demo_inputs(2, ri.H, ri.W, seed=seed)
    with torch.no_grad():
        res = m(return_loss=False, rescale=True, img=[img.to(DEV)], img_metas=[ri.metas()])
    assert float(gold['e2e_ref_err']) <= 5e-5
    for b in range(2):
        assert len(res[b]) == 4 and all(r.dtype == np.float32 and r.shape[1] == 5 for r in res[b])
        got, ref = _table(res[b]), gold[f'e2e_res{b}']
        assert got.shape == ref.shape and np.array_equal(got[:, 5], ref[:, 5]), b
        print('image', b, 'largest box / score difference', float(np.abs(got[:, :5] - ref[:, :5]).max()))
        assert np.allclose(got[:, :5], ref[:, :5], rtol=0, atol=2e-4), (b, np.abs(got[:, :5] - ref[:, :5]).max())


def test_one_host_synchronisation_per_inference_call_and_none_in_the_head_train_step(gold):
    """`simple_test_device` (everything before the result copy) and `bbox_head.forward_train_nhwc` run with
    torch's synchronisation debug mode on 'error': any blocking host read inside them raises"""
    seed = int(gold['seed_e2e'])
    m = _model(seed).eval()
    img, _, gts, gls = util.demo_inputs(2, ri.H, ri.W, seed=seed, num_gt=ri.TRAIN_NUM_GT)
    img, gts, gls = img.to(DEV), [g.to(DEV) for g in gts], [l.to(DEV) for l in gls]
    with torch.no_grad():
        m.simple_test_device(img, ri.metas(), rescale=True)            # (first call: constants are uploaded once)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            det, lab, nd = m.simple_test_device(img, ri.metas(), rescale=True)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    assert int(nd.sum()) > 0
    m.train()
    feats = [f.detach() for f in m.extract_feat_nhwc(img)]
    m.bbox_head.forward_train_nhwc(feats, ri.metas(), gts, gls)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        losses = m.bbox_head.forward_train_nhwc(feats, ri.metas(), gts, gls)
        total = torch.stack(losses['loss_cls'] + losses['loss_bbox']).sum()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert math.isfinite(float(total.detach()))


def test_two_train_iterations_golden(gold):
    m = _model(int(gold['seed_e2e'])).train()
    for it in range(2):
        seed = int(gold[f'seed_train{it}'])
        img, _, gts, gls = util.demo_inputs(2, ri.H, ri.W, seed=seed, num_gt=ri.TRAIN_NUM_GT)
        losses = m(img=img.to(DEV), img_metas=ri.metas(), gt_bboxes=[g.to(DEV) for g in gts], gt_labels=[l.to(DEV) for l in gls])
        assert sorted(losses) == ['loss_bbox', 'loss_cls'] and all(len(v) == 5 for v in losses.values())
        for k, v in losses.items():
            got = sum(v).detach().cpu().double().reshape(-1)
            ref = T(gold[f'train{it}_{k}']).double().sum().reshape(-1)
            assert torch.allclose(got, ref, rtol=2e-3, atol=1e-4), (it, k, got, ref)
        loss, log_vars = m._parse_losses(losses)
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for n, p in m.bbox_head.named_parameters())
        assert m.backbone.layer2[0].conv1.weight.grad is not None
        m.zero_grad()


@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
def test_model_16bit_close_to_fp32(gold, dtype):
    """the criterion tests/test_faster_rcnn_gpu.py::test_model_16bit_close_to_fp32 applies to its 16-bit cases"""
    from brcnn import blocks
    seed = int(gold['seed_e2e'])
    m = _model(seed).eval()
    img, _, _, _ = util.demo_inputs(2, ri.H, ri.W, seed=seed)
    try:
        with torch.no_grad():
            f32 = [f.float() for f in m.extract_feat_nhwc(img.to(DEV))]
            r32 = m.simple_test(img.to(DEV), ri.metas())
            m.set_compute_dtype(dtype)
            f16 = m.extract_feat_nhwc(img.to(DEV))
            assert all(f.dtype == (torch.bfloat16 if dtype == 'bf16' else torch.float16) for f in f16)
            r16 = m.simple_test(img.to(DEV), ri.metas())
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
    model = init_detector(ri.CONFIG, None, device=DEV)
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
    seed = int(gold['seed_train0'])
    img, _, gts, gls = util.demo_inputs(2, ri.H, ri.W, seed=seed, num_gt=ri.TRAIN_NUM_GT)
    data = dict(img=img.to(DEV), img_metas=ri.metas(), gt_bboxes=[g.to(DEV) for g in gts], gt_labels=[l.to(DEV) for l in gls])
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
        assert runs[0][1].keys() == runs[1][1].keys() and 'bbox_head.retina_cls.weight' in runs[0][1]
        assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
        before = m.bbox_head.retina_cls.weight.detach().clone()
        opt.step()
        torch.cuda.synchronize()
        assert not torch.equal(before, m.bbox_head.retina_cls.weight.detach())
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
        spec = importlib.util.spec_from_file_location(f'brcnn_tool_{name}', os.path.join(ri.ROOT, 'tools', f'{name}.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    cfg = _tiny_cfg(tmp_path, max_epochs=1)
    cfg.model = Config.fromfile(ri.CONFIG).model
    cfg_path = str(tmp_path / 'tiny_retinanet.py')
    cfg.dump(cfg_path)
    work = str(tmp_path / 'work_gpu')
    runner = tool('train').main([cfg_path, '--work-dir', work, '--seed', '0', '--allow-random-init'])
    assert runner.epoch == 1 and os.path.exists(os.path.join(work, 'epoch_1.pth'))
    assert all(np.isfinite(v) for row in runner.history for v in row[3].values())
    assert any('loss_cls' in row[3] and 'loss_bbox' in row[3] for row in runner.history) and len(runner.eval_history) == 1
    out_pkl = str(tmp_path / 'res.pkl')
    metric = tool('test').main([cfg_path, os.path.join(work, 'epoch_1.pth'), '--eval', 'bbox', '--out', out_pkl])
    assert metric == {} or 0.0 <= metric['bbox_mAP'] <= 1.0
    res = pickle.load(open(out_pkl, 'rb'))
    assert len(res) == 7 and len(res[0]) == len(CLASSES) and res[0][0].shape[1] == 5


# ------------------------------------------------------------------------------------------- the split_thr branch
# At the recipe's shapes (4693 picks x 4 classes = 18 772 slots per image) `get_bboxes_padded` takes mmcv's per-class
# branch: class-major slots through `batched_nms_images_by_level`, in its torch form above 16 384 slots.  The fixture's
# cases reach it with `test_cfg.nms.split_thr` lowered, in both forms.
def _force_form(monkeypatch, form):
    """'fused': the by-level entry as it chooses for <= 16 384 slots and <= 8 classes; 'torch': its form for larger slots"""
    if form == 'torch':
        import functools

        from brcnn import postprocess
        monkeypatch.setattr(postprocess, 'batched_nms_images_by_level',
                            functools.partial(postprocess.batched_nms_images_by_level, fused=False))


def _split_cfg(cfg, thr=100):
    cfg['test_cfg']['nms'] = dict(cfg['test_cfg']['nms'], split_thr=thr)
    return cfg


@pytest.mark.parametrize('form', ['fused', 'torch'])
@pytest.mark.parametrize('C,name', CASES)
def test_get_bboxes_golden_on_the_split_thr_branch(gold, monkeypatch, C, name, form):
    """the cases of test_get_bboxes_golden with split_thr = 100 (177 .. 708 slots per image): the same detections in the
    same order as the reference's, labels exact, boxes and scores within the same 2e-4"""
    _force_form(monkeypatch, form)
    seed = int(gold[f'seed_bboxes_c{C}'])
    head = build_head(ConfigDict(_split_cfg(ri.head_cfg(C)))).to(DEV).eval()
    assert head.test_cfg.nms.split_thr == 100 <= 177 * C
    cls, reg = ri.head_outputs(seed, C, empty=(name == 'empty'))
    res = head.get_bboxes([c.to(DEV) for c in cls], [r.to(DEV) for r in reg], ri.metas(), rescale=(name != 'plain'))
    for b, (det, lab) in enumerate(res):
        want_d, want_l = T(gold[f'bboxes_c{C}_{name}_det{b}']), T(gold[f'bboxes_c{C}_{name}_lab{b}'])
        assert lab.cpu().tolist() == want_l.tolist(), (C, name, form, b)
        assert det.shape == want_d.shape and torch.allclose(det.cpu(), want_d, rtol=0, atol=2e-4), (C, name, form, b)
    if name == 'empty':
        assert head.last_n_valid.tolist()[1] == 0 and len(res[1][0]) == 0 and len(res[0][0]) > 0


@pytest.mark.parametrize('form', ['fused', 'torch'])
def test_model_end_to_end_golden_on_the_split_thr_branch(gold, monkeypatch, form):
    """test_model_end_to_end_golden with split_thr = 100, and `simple_test_device` on that branch under torch's
    synchronisation debug mode on 'error': the one host read of an inference call is the result copy, which also
    brings the per-image candidate counts (`last_n_valid`)"""
    _force_form(monkeypatch, form)
    seed = int(gold['seed_e2e'])
    m = build_detector(ConfigDict(_split_cfg(ri.fixture_model_cfg())))
    m.load_state_dict(ri.fixture_state_dict(m, seed))
    m = m.to(DEV).eval()
    img, _, _, _ = util.demo_inputs(2, ri.H, ri.W, seed=seed)
    img = img.to(DEV)
    with torch.no_grad():
        res = m(return_loss=False, rescale=True, img=[img], img_metas=[ri.metas()])
        assert len(m.last_n_valid) == 2 and all(n >= sum(len(r) for r in res[b]) > 0 for b, n in enumerate(m.last_n_valid))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            det, lab, nd = m.simple_test_device(img, ri.metas(), rescale=True)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    assert nd.tolist() == [sum(len(r) for r in res[b]) for b in range(2)]
    for b in range(2):
        got, ref = _table(res[b]), gold[f'e2e_res{b}']
        assert got.shape == ref.shape and np.array_equal(got[:, 5], ref[:, 5]), (form, b)
        assert np.allclose(got[:, :5], ref[:, :5], rtol=0, atol=2e-4), (form, b, np.abs(got[:, :5] - ref[:, :5]).max())


def test_more_than_16384_slots_take_the_per_class_branch_and_match_the_offset_form():
    """16 classes at nms_pre = 1000 on the small pyramid: 1161 picks x 16 = 18 576 slots per image, above split_thr =
    10 000 and above the fused entries' 16 384 slots and 8 segments -- the size class of the recipe's own inference
    (18 772).  The per-class branch keeps what the offset form (split_thr out of reach) keeps, in the same order, bit for
    bit (both gather the same candidates), and reads nothing back."""
    C = 16
    outs = {}
    cls, reg = ri.head_outputs(41, C)
    cls, reg = [c.to(DEV) for c in cls], [r.to(DEV) for r in reg]
    for thr in (10 ** 9, 10000):
        cfg = ri.head_cfg(C)
        cfg['test_cfg'] = dict(ri.TEST_CFG, nms_pre=1000, max_per_img=100, nms=dict(type='nms', iou_threshold=0.5, split_thr=thr))
        head = build_head(ConfigDict(cfg)).to(DEV).eval()
        f = lambda lst: [t.permute(0, 2, 3, 1).contiguous() for t in lst]    # noqa: E731
        head.get_bboxes_padded(f(cls), f(reg), ri.metas(), rescale=True)       # (first call: constants are uploaded once)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            det, lab, num = head.get_bboxes_padded(f(cls), f(reg), ri.metas(), rescale=True)
        finally:
            torch.cuda.set_sync_debug_mode('default')
        outs[thr] = (det.cpu(), lab.cpu(), num.cpu(), head.last_n_valid.cpu())
    a, b = outs[10 ** 9], outs[10000]
    assert a[0].shape == (2, 100, 5) and a[2].tolist() == [100, 100] and (a[3] > 200).all()
    assert len(set(a[1][0].tolist())) > 4           # several classes among the kept
    assert torch.equal(a[2], b[2]) and torch.equal(a[1], b[1]) and torch.equal(a[0], b[0]) and torch.equal(a[3], b[3])
