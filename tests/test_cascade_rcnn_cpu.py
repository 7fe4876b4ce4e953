"""CPU tests (-m "not gpu") of the Cascade R-CNN baseline: the float64 restatement of the hand-over kernels
(tests/cascade_ref64.py) is pinned to what the reference's refine_bboxes / regress_by_class computed
(tests/golden/g26_cascade_rcnn.npz, made by tests/golden/make_golden_cascade_rcnn.py) before the GPU tests lean on it;
the recipe builds with the reference's parameter names and loads its checkpoints; the refused configurations raise; and
the torch host mirror of CascadeRoIHead (forward_train / simple_test, run on the CPU restatement of the operators,
oracle/cpu_pipeline.py) reproduces the reference's losses and detections."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import Config, build_detector, build_head
from brcnn.config import ConfigDict
from oracle import cpu_pipeline
from tests import cascade_rcnn_inputs as ci
from tests import cascade_ref64 as R
from tests import faster_rcnn_inputs as fi
from tests import util

G = os.path.join(os.path.dirname(__file__), 'golden', 'g26_cascade_rcnn.npz')
EPS32 = R.EPS32


@pytest.fixture(scope='module')
def gold():
    return {k: v for k, v in np.load(G, allow_pickle=False).items()}


@pytest.fixture(scope='module')
def model():
    return build_detector(Config.fromfile(ci.CONFIG).model)


def _table(res):
    return np.concatenate([np.concatenate([r, np.full((len(r), 1), c, np.float32)], 1) for c, r in enumerate(res)], 0)


# ------------------------------------------------------------------------------------------- float64 reference pinned
@pytest.mark.parametrize('tag,agnostic', [('agn', True), ('cls', False)])
def test_float64_reference_agrees_with_the_fixture(gold, tag, agnostic):
    """kept rows and their order exact (the fixture's row counts, and every kept row matching its own float64 box);
    boxes within the fp32 bound 8 * EPS32 * (|centre| + size) of the float64 value, plus the fp32 rounding of the stored
    number"""
    seed = int(gold['seed_refine'])
    rois, labels, cls_score, bbox_pred, flags = ci.refine_rows(seed, agnostic)
    coder = ci.box_head_cfg(0)['bbox_coder']
    means, stds = coder['target_means'], coder['target_stds']
    offs = [0, ci.REFINE_ROWS[0], sum(ci.REFINE_ROWS)]
    max_shape = np.array([m['img_shape'][:2] for m in fi.metas()], dtype=np.float64)
    gt_flags = R.flags_from_pos_is_gt([f.numpy() for f in flags], offs)
    assert gt_flags.sum() == 4 and gt_flags[:4].all()
    out, used = R.refine_train(rois.numpy(), labels.numpy(), gt_flags, offs, cls_score.numpy(), bbox_pred.numpy(), max_shape,
                               means, stds, agnostic, ci.REFINE_C)
    bg = labels.numpy() == ci.REFINE_C
    assert bg.any() and (~bg).any() and np.array_equal(used[~bg], labels.numpy()[~bg])
    assert np.array_equal(used[bg], cls_score[:, :-1].argmax(1).numpy()[bg])
    for b in range(2):
        want = gold[f'refine_{tag}_train{b}'].astype(np.float64)
        boxes, bound = out[b]
        assert boxes.shape == want.shape == (offs[b + 1] - offs[b] - (4 if b == 0 else 0), 4)
        assert (np.abs(boxes - want) <= bound + EPS32 * np.abs(want)).all(), np.abs(boxes - want).max()
    # test time: every row by its arg-max class; rois come in as (n, 5) and leave with their image column
    for b in range(2):
        sl = slice(offs[b], offs[b + 1])
        n = offs[b + 1] - offs[b]
        dets = np.zeros((1, n, 5))
        dets[0, :, :4] = rois.numpy()[sl, 1:]
        got, lab, bound = R.refine_test(dets, np.array([n]), cls_score.numpy()[sl], bbox_pred.numpy()[sl], max_shape[b:b + 1],
                                        means, stds, agnostic)
        want = gold[f'refine_{tag}_test{b}'].astype(np.float64)
        assert want.shape == (n, 5) and (want[:, 0] == b).all()
        assert np.array_equal(lab, cls_score[sl][:, :-1].argmax(1).numpy())
        assert (np.abs(got[0, :, :4] - want[:, 1:]) <= bound[0] + EPS32 * np.abs(want[:, 1:])).all()


def test_float64_reference_tie_rule_and_mean():
    x = np.array([[1., 3., 3., 0., 9.], [2., 2., 2., 1., 0.], [-1., -5., -1., -1., 7.]], dtype=np.float32)
    assert R.argmax_fg(x).tolist() == [1, 0, 0] == torch.tensor(x)[:, :-1].argmax(1).tolist()
    g = torch.Generator().manual_seed(0)
    s = [torch.randn(50, 5, generator=g) * 3 for _ in range(3)]
    want = (s[0] + s[1] + s[2]) / 3.0
    assert np.array_equal(R.mean_logits32([t.numpy() for t in s]), want.numpy())
    assert np.allclose(R.softmax64(want.numpy()), want.double().softmax(1).numpy(), rtol=1e-14, atol=0)


# ------------------------------------------------------------------------------------------- the recipe
def test_config_builds_the_baseline(model):
    from brcnn.dense_heads import RPNHead
    from brcnn.detectors import CascadeRCNN
    from brcnn.necks import FPN
    from brcnn.roi_heads import CascadeRoIHead, Shared2FCBBoxHead
    rh = model.roi_head
    assert type(model) is CascadeRCNN and type(rh) is CascadeRoIHead and type(model.rpn_head) is RPNHead
    assert type(model.neck) is FPN and rh.num_stages == 3 and rh.stage_loss_weights == [1, 0.5, 0.25]
    assert all(type(h) is Shared2FCBBoxHead and h.reg_class_agnostic and h.num_classes == 4 for h in rh.bbox_head)
    assert [list(h.bbox_coder.stds) for h in rh.bbox_head] == [[0.1, 0.1, 0.2, 0.2], [0.05, 0.05, 0.1, 0.1],
                                                               [0.033, 0.033, 0.067, 0.067]]
    assert all(type(h.loss_bbox).__name__ == 'SmoothL1Loss' and h.loss_bbox.beta == 1.0 for h in rh.bbox_head)
    assert [(a.pos_iou_thr, a.neg_iou_thr, a.min_pos_iou, a.match_low_quality) for a in rh.bbox_assigner] == \
        [(t, t, t, False) for t in (0.5, 0.6, 0.7)]
    assert all((s.num, s.pos_fraction, s.add_gt_as_proposals) == (512, 0.25, True) for s in rh.bbox_sampler)
    tp, rp = model.train_cfg.rpn_proposal, model.test_cfg.rpn
    assert (tp.nms_pre, tp.max_per_img, rp.nms_pre, rp.max_per_img) == (2000, 2000, 1000, 1000)
    assert model.test_cfg.rcnn.nms.iou_threshold == 0.5 and model.test_cfg.rcnn.max_per_img == 100
    assert rh.num_classes == 4 and model.rpn_head.device_train_ok() and rh.device_train_ok() and model._device_path_ok()
    full = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
    model.rpn_head._check_proposal_limits(tp, full)
    model.rpn_head._check_proposal_limits(rp, full)
    # the accessor the detector shapes its results by: unchanged for the single-head RoI heads
    std = build_detector(Config.fromfile(fi.CONFIG).model)
    assert std.roi_head.num_classes == std.roi_head.bbox_head.num_classes == 4
    # one extractor / head cfg is shared out over the stages, as the reference does
    one = ci.roi_head_cfg()
    one['bbox_head'] = one['bbox_head'][0]
    assert len(build_head(ConfigDict(one)).bbox_head) == 3


def test_fixture_model_builds_with_the_references_names_and_loads_its_checkpoints(gold):
    m = build_detector(ConfigDict(ci.fixture_model_cfg()))
    sd = m.state_dict()
    want = {str(k): json.loads(str(s)) for k, s in zip(gold['state_keys'], gold['state_shapes'])}
    assert len(want) == len(gold['state_keys']) and {k: list(v.shape) for k, v in sd.items()} == want
    assert 'roi_head.bbox_head.2.shared_fcs.1.weight' in want and 'roi_head.bbox_head.0.fc_reg.bias' in want
    # a reference checkpoint (its keys and shapes) loads strictly, and a round trip gives the same tensors back
    ref_ckpt = {k: torch.full(shape, 0.5) for k, shape in want.items()}
    m.load_state_dict(ref_ckpt, strict=True)
    seeded = ci.fixture_state_dict(m, 3)
    m.load_state_dict(seeded, strict=True)
    m2 = build_detector(ConfigDict(ci.fixture_model_cfg()))
    m2.load_state_dict(copy.deepcopy(m.state_dict()), strict=True)
    assert all(torch.equal(v, m2.state_dict()[k]) and torch.equal(v, seeded[k]) for k, v in m.state_dict().items())


def test_refused_configurations_raise(model):
    cfg = ci.roi_head_cfg
    for key, val in (('mask_head', dict(type='FCNMaskHead')), ('mask_roi_extractor', dict(type='SingleRoIExtractor')),
                     ('shared_head', dict(type='ResLayer'))):
        with pytest.raises(NotImplementedError, match=key):
            build_head(ConfigDict(cfg(), **{key: val}))
    from brcnn.roi_heads import Shared2FCBBoxHead
    try:
        Shared2FCBBoxHead.custom_activation = True
        with pytest.raises(NotImplementedError, match='custom_activation'):
            build_head(ConfigDict(cfg()))
    finally:
        del Shared2FCBBoxHead.custom_activation
    assert Shared2FCBBoxHead.custom_activation is False
    for nms, what in ((dict(type='soft_nms', iou_threshold=0.5), 'soft_nms'),
                      (dict(type='nms', iou_threshold=0.5, class_agnostic=True), 'class_agnostic')):
        c = cfg()
        c['test_cfg']['nms'] = nms
        with pytest.raises(NotImplementedError, match=what):
            build_head(ConfigDict(c))
    coder = dict(type='DeltaXYWHBBoxCoder', target_means=[0., 0., 0., 0.], target_stds=[0.1, 0.1, 0.2, 0.2])
    with pytest.raises(NotImplementedError, match='add_ctr_clamp'):
        build_head(ConfigDict(cfg(bbox_coder=dict(coder, add_ctr_clamp=True))))
    with pytest.raises(NotImplementedError, match='clip_border'):
        build_head(ConfigDict(cfg(bbox_coder=dict(coder, clip_border=False))))
    with pytest.raises(TypeError):
        build_head(ConfigDict(cfg(type='ProbConvFCBBoxHead', num_shared_fcs=2)))
    imgs = [torch.zeros(1, 3, 64, 96), torch.zeros(1, 3, 64, 96)]
    metas = [fi.metas(1), [dict(fi.metas(1)[0], flip=True, flip_direction='horizontal')]]
    assert model.roi_head.supports_tta is False
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        model.aug_test(imgs, metas)
    with pytest.raises(NotImplementedError, match='has no test-time augmentation'):
        model.roi_head.aug_test(None, None, metas)


# ------------------------------------------------------------------------------------------- host mirror vs the fixture
def _assert_dets(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got[:, 5], ref[:, 5]), what
    assert np.allclose(got[:, :5], ref[:, :5], rtol=0, atol=2e-4), (what, np.abs(got[:, :5] - ref[:, :5]).max())


def test_host_mirror_head_level_reproduces_the_reference(gold):
    """section (b): the three stages' losses (the seeded draws come in the reference's order: image by image, positives
    then negatives, stage after stage) and the ensemble's detections"""
    seed = int(gold['seed_head'])
    rh = build_head(ConfigDict(ci.roi_head_cfg()))
    rh.load_state_dict(ci.head_state_dict(rh, seed))
    feats, metas, gts, gls, props = fi.roi_inputs(seed)
    with cpu_pipeline.patched():
        rh.train()
        torch.manual_seed(seed + 100)
        losses = rh.forward_train(feats, metas, props, gts, gls)
        assert sorted(losses) == sorted(f's{i}.{k}' for i in range(3) for k in ('loss_bbox', 'loss_cls', 'acc'))
        for k, v in losses.items():
            want = gold['head_train_' + k].reshape(-1)
            assert np.allclose(v.detach().reshape(-1).numpy(), want, rtol=1e-4, atol=1e-6), (k, v, want)
        sum(v for k, v in losses.items() if 'loss' in k).backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in rh.parameters())
        rh.eval()
        with torch.no_grad():
            res = rh.simple_test(feats, props, metas, rescale=True)
    for b in range(2):
        _assert_dets(_table(res[b]), gold[f'head_res{b}'], ('head', b))


def test_host_mirror_stage_weights_touch_losses_only():
    """only names that contain `loss` are multiplied by the stage weight (cascade_roi_head.py:251-253)"""
    seed = 5
    feats, metas, gts, gls, props = fi.roi_inputs(seed)
    out = []
    for weights in ([1, 0.5, 0.25], [2, 2, 2]):
        c = ci.roi_head_cfg()
        c['stage_loss_weights'] = weights
        rh = build_head(ConfigDict(c))
        rh.load_state_dict(ci.head_state_dict(rh, seed))
        with cpu_pipeline.patched():
            torch.manual_seed(seed)
            out.append(rh.train().forward_train(feats, metas, props, gts, gls))
    for i, (w0, w1) in enumerate(zip([1, 0.5, 0.25], [2, 2, 2])):
        assert torch.equal(out[0][f's{i}.acc'], out[1][f's{i}.acc'])
        for k in ('loss_cls', 'loss_bbox'):
            assert torch.allclose(out[0][f's{i}.{k}'] / w0, out[1][f's{i}.{k}'] / w1, rtol=1e-6, atol=0)


def test_host_mirror_end_to_end_reproduces_the_reference(gold):
    """sections (c) and (d): `model(return_loss=False)` and two train iterations of the small fixture model"""
    torch.set_num_threads(cpu_pipeline.available_cpus())
    seed = int(gold['seed_e2e'])
    with cpu_pipeline.patched():
        m = build_detector(ConfigDict(ci.fixture_model_cfg()))
        m.load_state_dict(ci.fixture_state_dict(m, seed))
        img, _, _, _ = util.demo_inputs(2, fi.H, fi.W, seed=seed)
        m.eval()
        m.roi_head.device_test_path = False         # the host mirror (on CPU tensors the device entries refuse)
        with torch.no_grad():
            res = m(return_loss=False, rescale=True, img=[img], img_metas=[fi.metas()])
        for b in range(2):
            assert len(res[b]) == 4
            _assert_dets(_table(res[b]), gold[f'e2e_res{b}'], ('e2e', b))
        m.train()
        for it in range(2):
            tseed = int(gold[f'seed_train{it}'])
            img, metas, gts, gls = util.demo_inputs(2, fi.H, fi.W, seed=tseed, num_gt=fi.TRAIN_NUM_GT)
            torch.manual_seed(tseed + 100)
            # TwoStageDetector.forward_train's host branch, step by step: the trunk and the RPN outputs are taken without
            # a graph (RPNHead's differentiable tower is a device kernel with no CPU restatement); the losses, the
            # proposals and the cascade are the host path's own, in the order forward_train runs them
            with torch.no_grad():
                x = m.extract_feat(img)
                outs = m.rpn_head(x)
            losses = m.rpn_head.loss(*outs, gts, metas)
            props = m.rpn_head.get_bboxes(*outs, metas, cfg=m.train_cfg.rpn_proposal)
            losses.update(m.roi_head.forward_train(x, metas, props, gts, gls))
            assert sorted(losses) == sorted(['loss_rpn_cls', 'loss_rpn_bbox'] +
                                            [f's{i}.{k}' for i in range(3) for k in ('loss_cls', 'loss_bbox', 'acc')])
            for k, v in losses.items():
                got = (sum(v) if isinstance(v, list) else v).detach().double().reshape(-1)
                want = torch.as_tensor(gold[f'train{it}_{k}']).double().sum().reshape(-1)
                assert torch.allclose(got, want, rtol=1e-4, atol=1e-6), (it, k, got, want)
            loss, log_vars = m._parse_losses(losses)
            assert np.isfinite(log_vars['loss']) and 's2.acc' in log_vars
