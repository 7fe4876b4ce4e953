"""Test-time augmentation, host side (no GPU): the torch helpers of the per-image chain against the fixture of the
imported reference (tests/golden/make_golden_tta.py -> g24_tta.npz), the C ABI of the new entries, and the argument
checks of `forward_test` with more than one aug."""
import os
import re

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import Config, build_detector, core, lib
from oracle import orc
from tests import tta_util, util
from tests.test_host_cpu import CFG, ROOT, T, load

NEW_ENTRIES = ('brcnn_tta_gather_proposals', 'brcnn_tta_map_rois', 'brcnn_rcnn_decode_tta')


@pytest.fixture(scope='module')
def g():
    return load('g24_tta')


@pytest.fixture(scope='module')
def cfg():
    return Config.fromfile(CFG)


def _metas(b):
    return [m[b] for m in tta_util.tta_inputs()[1]]


def test_bbox_mapping_round_trip_all_flips():
    boxes = util.rand_boxes(64, 180., 120., seed=3)
    sf = np.array([1.5, 1.25, 1.5, 1.25], np.float32)
    for direction in ('horizontal', 'vertical', 'diagonal'):
        fwd = core.bbox_mapping(boxes, (150, 270, 3), sf, True, direction)
        assert (fwd[:, 2] >= fwd[:, 0]).all() and (fwd[:, 3] >= fwd[:, 1]).all()
        assert torch.allclose(core.bbox_mapping_back(fwd, (150, 270, 3), sf, True, direction), boxes, atol=1e-4)
        # bbox_flip is its own inverse, on (..., 4k) class-wise boxes too
        wide = torch.cat([fwd, fwd + 1], 1)
        back = core.bbox_flip(core.bbox_flip(wide, (150, 270, 3), direction), (150, 270, 3), direction)
        assert torch.allclose(back, wide, atol=1e-4)
    h = core.bbox_flip(boxes, (120, 180, 3), 'horizontal')
    assert torch.equal(h[:, 0], 180 - boxes[:, 2]) and torch.equal(h[:, 1], boxes[:, 1])
    v = core.bbox_flip(boxes, (120, 180, 3), 'vertical')
    assert torch.equal(v[:, 3], 120 - boxes[:, 1]) and torch.equal(v[:, 0], boxes[:, 0])


def test_merge_aug_proposals_golden(g, cfg):
    """per-aug reference proposals -> the reference's merged proposals: same rows in the same order, same bits"""
    for b in range(2):
        metas = _metas(b)
        props = [T(g[f'props{a}_{b}']) for a in range(len(metas))]
        merged = core.merge_aug_proposals(props, metas, cfg.model.test_cfg.rpn, nms=orc.nms)
        assert torch.equal(merged, T(g[f'merged_{b}'])), b


def test_merge_aug_bboxes_golden(g, cfg):
    """per-aug box-head outputs on the merged proposals -> the reference's merged class boxes and scores.  Boxes and
    the mode-'raw' scores (means of logits) bit for bit; the mode-'fused' scores within rtol 1e-6: `softmax` on the host
    is vectorised differently from one CPU to the next."""
    coder = brcnn.registry.build_bbox_coder(cfg.model.roi_head.bbox_head.bbox_coder)
    for b in range(2):
        metas = _metas(b)
        merged = T(g[f'merged_{b}'])
        boxes_l, raw_l, fused_l = [], [], []
        for a, meta in enumerate(metas):
            rois = core.bbox_mapping(merged[:, :4], meta['img_shape'], meta['scale_factor'], meta['flip'],
                                     meta['flip_direction'] or 'horizontal')
            boxes_l.append(coder.decode(rois, T(g[f'reg{a}_{b}']), max_shape=meta['img_shape']))
            raw_l.append(T(g[f'cls{a}_{b}']))
            fused_l.append((T(g[f'cls{a}_{b}']).softmax(1) * merged[:, 4:5]) ** 0.5)
        one = [[m] for m in metas]
        bboxes, raw = core.merge_aug_bboxes(boxes_l, raw_l, one, cfg.model.test_cfg.rcnn)
        _, fused = core.merge_aug_bboxes(boxes_l, fused_l, one, cfg.model.test_cfg.rcnn)
        assert torch.equal(bboxes, T(g[f'raw_bboxes_{b}'])) and torch.equal(bboxes, T(g[f'fused_bboxes_{b}'])), b
        assert torch.equal(raw, T(g[f'raw_scores_{b}'])), b
        assert torch.allclose(fused, T(g[f'fused_scores_{b}']), rtol=1e-6, atol=0), b
        assert core.merge_aug_bboxes(boxes_l, None, one, None).shape == bboxes.shape


def test_fixture_is_not_fragile(g):
    """what the GPU comparisons lean on: no tied proposal scores, no candidate score within 1e-6 of score_thr"""
    thr = float(g['score_thr'])
    for b in range(2):
        cand = np.concatenate([g[f'props{a}_{b}'][:, 4] for a in range(5)])
        assert len(np.unique(cand)) == len(cand) == 1280
        assert len(np.unique(g[f'merged_{b}'][:, 4])) == len(g[f'merged_{b}']) == 256
        for mode in ('raw', 'fused'):
            assert np.abs(g[f'{mode}_scores_{b}'][:, :-1] - thr).min() > 1e-6
            assert len(g[f'{mode}_det_{b}']) > 20


_C2CT = {'int': lib.c_int, 'float': lib.c_f32, 'double': lib.c_f64}


def test_header_and_binding_agree_on_tta_entries():
    header = open(os.path.join(ROOT, 'include', 'brcnn_hip.h')).read()
    for name in NEW_ENTRIES:
        m = re.search(r'\bint\s+' + name + r'\s*\(([^;]*?)\)\s*;', header, re.S)
        assert m, f'{name} is not declared in include/brcnn_hip.h'
        want = []
        for p in m.group(1).split(','):
            p = ' '.join(p.split())
            want.append(lib.c_ptr if '*' in p else _C2CT[p.replace('const ', '').split(' ')[0]])
        res, args = lib.SIGNATURES[name]
        assert res is lib.c_int and list(args) == want, name
    assert int(re.search(r'#define BRCNN_TTA_MAX_AUGS (\d+)', header).group(1)) == brcnn.ops.TTA_MAX_AUGS
    assert {k: int(re.search(r'#define BRCNN_TTA_' + k.upper() + r' (\d+)', header).group(1))
            for k in brcnn.ops._TTA_MODE} == brcnn.ops._TTA_MODE


def test_geometry_rows():
    _, metas = tta_util.tta_inputs()
    rows = brcnn.ops.tta_geometry_rows(metas)
    assert len(rows) == 10 and all(len(r) == 8 for r in rows)
    assert rows[0] == [120.0, 180.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0]
    assert [r[6] for r in rows[::2]] == [0.0, 1.0, 0.0, 2.0, 3.0]
    assert rows[9][:2] == [78.0, 123.0] and rows[9][2] == float(np.float32(123 / 164))


@pytest.fixture(scope='module')
def model(cfg):
    return build_detector(cfg.model).eval()


def test_forward_test_validates_aug_lists(model):
    """`forward_test` with more than one aug reaches `aug_test` (it raised NotImplementedError before) and refuses bad
    aug lists with a ValueError that names the argument, before any device work"""
    imgs, metas = tta_util.tta_inputs()
    two = lambda: ([t.clone() for t in imgs[:2]], [[dict(m) for m in ms] for ms in metas[:2]])   # noqa: E731
    i2, m2 = two()
    with pytest.raises(ValueError, match='img_metas'):          # aug / meta counts
        model(return_loss=False, img=i2, img_metas=m2 + [m2[0]])
    i2, m2 = two()
    with pytest.raises(ValueError, match=r'imgs\[1\]'):         # batch sizes differ between the augs
        model(return_loss=False, img=[i2[0], i2[1][:1]], img_metas=[m2[0], m2[1][:1]])
    i2, m2 = two()
    with pytest.raises(ValueError, match=r'img_metas\[1\]'):    # metas of an aug do not match its batch
        model(return_loss=False, img=i2, img_metas=[m2[0], m2[1][:1]])
    with pytest.raises(ValueError, match='imgs'):               # more augs than the kernels take
        model(return_loss=False, img=[imgs[0][:1]] * 17, img_metas=[[dict(metas[0][0])] for _ in range(17)])
    i2, m2 = two()
    del m2[1][0]['flip_direction']
    with pytest.raises(ValueError, match=r'img_metas\[1\]\[0\].*flip_direction'):
        model(return_loss=False, img=i2, img_metas=m2)
    i2, m2 = two()
    with pytest.raises(ValueError, match='proposals'):
        model(return_loss=False, img=i2, img_metas=m2, proposals=[None, None])
    i2, m2 = two()
    model.roi_head.test_cfg['tta_scores'] = 'mean'
    try:
        with pytest.raises(ValueError, match='tta_scores'):
            model.roi_head.tta_score_mode()
    finally:
        del model.roi_head.test_cfg['tta_scores']
    assert model.roi_head.tta_score_mode() == 'fused'
