"""-m gpu: test-time augmentation on the device-resident path (csrc/tta.hip, `aug_test_device`) against the fixture of
the imported reference (tests/golden/make_golden_tta.py -> g24_tta.npz: the seeded g10 UTDAC model on five augs,
1.0 / 1.0 + horizontal / 1.5 / 1.5 + vertical / 0.75 + diagonal, of two images of different size in one padded batch,
each image's expectation being the reference's run on it alone with the batch's padded tensors)."""
import copy
import ctypes
import importlib.util
import os
import pickle

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import Config, build_detector, blocks, core, lib, ops
from brcnn.postprocess import batched_nms_images
from tests import tta_util, util
from tests.test_host_cpu import CFG, ROOT, T, load

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
A, B, K, C = 5, 2, 256, 4


def _match_dets(got, ref, box_tol=1e-2, score_tol=1e-3):
    """fraction of reference detections that have a counterpart (same place, same score) -- the measure of the g10
    end-to-end test (tests/test_golden_gpu.py)"""
    if len(ref) == 0:
        return 1.0 if len(got) == 0 else 0.0
    if len(got) == 0:
        return 0.0
    d = np.abs(ref[:, None, :4] - got[None, :, :4]).max(-1)
    s = np.abs(ref[:, None, 4] - got[None, :, 4])
    ok = ((d < box_tol) & (s < score_tol)).any(1)
    return ok.mean()


@pytest.fixture(scope='module')
def g():
    return load('g24_tta')


@pytest.fixture(scope='module')
def inputs():
    return tta_util.tta_inputs()


@pytest.fixture(scope='module')
def model():
    m = build_detector(Config.fromfile(CFG).model)
    m.load_state_dict(util.seeded_state_dict(m, seed=10))
    return m.to(DEV).eval()


def _pad(rows, k):
    """list over images of (n, 5) -> ((B, k, 5) zero padded, (B,) int32) on the device"""
    out = torch.zeros(len(rows), k, 5)
    for b, r in enumerate(rows):
        out[b, :len(r)] = r
    return out.to(DEV), torch.tensor([len(r) for r in rows], dtype=torch.int32, device=DEV)


def _fixture_merged(g):
    return _pad([T(g[f'merged_{b}']) for b in range(B)], K)


def _fixture_head_outputs(g):
    cls = torch.stack([torch.cat([T(g[f'cls{a}_{b}']) for b in range(B)]) for a in range(A)]).to(DEV)
    reg = torch.stack([torch.cat([T(g[f'reg{a}_{b}']) for b in range(B)]) for a in range(A)]).to(DEV)
    return cls, reg


def test_gather_and_merge_golden(g, inputs):
    """brcnn_tta_gather_proposals on the reference's per-aug proposals: candidates bit for bit what `bbox_mapping_back`
    + `torch.cat` give; then the existing prepare / NMS / collect: the reference's merged proposals, same rows, same
    order, same bits.  Aug 2 travels in a wider slot than it fills (num < K)."""
    _, metas = inputs
    widths = [256, 256, 300, 256, 256]
    padded = [_pad([T(g[f'props{a}_{b}']) for b in range(B)], widths[a]) for a in range(A)]
    geom = ops.tta_geometry(metas, padded[0][0])
    cand, boxes, scores, valid = ops.tta_gather_proposals([p for p, _ in padded], [n for _, n in padded], geom)
    assert cand.shape == (B, sum(widths), 5)
    cand, valid = cand.cpu(), valid.cpu()
    assert torch.equal(boxes.cpu(), cand[..., :4]) and torch.equal(scores.cpu(), cand[..., 4])
    for b in range(B):
        ref, col = [], 0
        for a in range(A):
            p, m = T(g[f'props{a}_{b}']), metas[a][b]
            back = core.bbox_mapping_back(p[:, :4], m['img_shape'], m['scale_factor'], m['flip'],
                                          m['flip_direction'] or 'horizontal')
            assert torch.equal(cand[b, col:col + len(p)], torch.cat([back, p[:, 4:]], 1)), (a, b)
            assert valid[b, col:col + len(p)].all() and not valid[b, col + len(p):col + widths[a]].any()
            assert (cand[b, col + len(p):col + widths[a]] == 0).all()
            col += widths[a]
    cfg = Config.fromfile(CFG).model.test_cfg.rpn
    merged, _, num = batched_nms_images(boxes, scores, torch.zeros_like(scores, dtype=torch.long), valid.to(DEV),
                                        cfg.nms.iou_threshold, cfg.max_per_img)
    assert num.tolist() == [K, K]
    for b in range(B):
        assert torch.equal(merged[b].cpu(), T(g[f'merged_{b}'])), b


def test_map_rois_bit_exact(g, inputs):
    """brcnn_tta_map_rois == `bbox_mapping` (all three flip directions are among the augs)"""
    _, metas = inputs
    merged, _ = _fixture_merged(g)
    rois = ops.tta_map_rois(merged, ops.tta_geometry(metas, merged)).cpu()
    assert rois.shape == (A, B * K, 5)
    for a in range(A):
        for b in range(B):
            m = metas[a][b]
            ref = core.bbox_mapping(T(g[f'merged_{b}'])[:, :4], m['img_shape'], m['scale_factor'], m['flip'],
                                    m['flip_direction'] or 'horizontal')
            got = rois[a, b * K:(b + 1) * K]
            assert (got[:, 0] == b).all() and torch.equal(got[:, 1:], ref), (a, b)


@pytest.mark.parametrize('mode', ['fused', 'raw'])
def test_rcnn_decode_tta_golden(g, inputs, mode):
    """brcnn_rcnn_decode_tta on the reference's box-head outputs: merged class boxes and scores within fp32 round-off
    (1e-5 relative, the project's loss-grade bar: device expf and the in-kernel softmax are the only arithmetic that is
    not the reference's), `valid` identical (no fixture score lies within 1e-6 of score_thr: asserted), detections after
    the NMS the reference's, row by row."""
    _, metas = inputs
    cfg = Config.fromfile(CFG).model
    rc, coder = cfg.test_cfg.rcnn, cfg.roi_head.bbox_head.bbox_coder
    merged, num = _fixture_merged(g)
    cls, reg = _fixture_head_outputs(g)
    geom = ops.tta_geometry(metas, merged)
    bb, sc, lb, va = ops.rcnn_decode_tta(cls, reg, merged, num, geom, None, C, rc.score_thr, coder.target_means,
                                         coder.target_stds, mode)
    det, lab, nd = batched_nms_images(bb, sc, lb, va, rc.nms.iou_threshold, rc.max_per_img)
    assert torch.equal(lb.cpu(), torch.arange(C).repeat(B, K))
    for b in range(B):
        ref_b, ref_s = T(g[f'{mode}_bboxes_{b}']), T(g[f'{mode}_scores_{b}'])[:, :C]
        got_b, got_s = bb[b].cpu().view(K, 4 * C), sc[b].cpu().view(K, C)
        print(mode, b, 'max |box err|', (got_b - ref_b).abs().max().item(), 'max |score err|',
              (got_s - ref_s).abs().max().item())
        assert torch.allclose(got_b, ref_b, rtol=1e-5, atol=1e-5), (b, (got_b - ref_b).abs().max())
        assert torch.allclose(got_s, ref_s, rtol=1e-5, atol=1e-5), (b, (got_s - ref_s).abs().max())
        assert ((ref_s - rc.score_thr).abs() > 1e-6).all()
        assert torch.equal(va[b].cpu().view(K, C), ref_s > rc.score_thr), b
        ref_det, ref_lab = T(g[f'{mode}_det_{b}']), T(g[f'{mode}_lab_{b}'])
        n = int(nd[b])
        assert n == len(ref_det) and torch.equal(lab[b, :n].cpu(), ref_lab), b
        assert torch.allclose(det[b, :n].cpu(), ref_det, rtol=1e-5, atol=1e-5), b
    # out_scale: the averaged boxes times aug 0's scale factor (results in the frame of imgs[0])
    sf = torch.tensor([[1.5, 1.25, 1.5, 1.25], [0.75, 2.0, 0.75, 2.0]], device=DEV)
    bb2, sc2, _, va2 = ops.rcnn_decode_tta(cls, reg, merged, num, geom, sf, C, rc.score_thr, coder.target_means,
                                           coder.target_stds, mode)
    assert torch.equal(bb2, bb * sf[:, None, :]) and torch.equal(sc2, sc) and torch.equal(va2, va)


def test_one_aug_equals_simple_test_padded(model):
    """`aug_test_padded` with a single identity aug == `simple_test_padded`, bit for bit -- with an empty image and an
    image that fills a part of its slots only"""
    img, metas, _, _ = util.demo_inputs(2, 128, 192, seed=10)
    for m in metas:
        m['scale_factor'] = np.ones(4, np.float32)
    g_ = torch.Generator().manual_seed(5)
    dets = torch.zeros(2, 64, 5)
    dets[1, :40, :4] = util.rand_boxes(40, 189., 128., seed=6, min_size=4., max_size=120.)
    dets[1, :40, 4] = torch.rand(40, generator=g_)
    dets, num = dets.to(DEV), torch.tensor([0, 40], dtype=torch.int32, device=DEV)
    with torch.no_grad():
        feats = model.extract_feat_nhwc(img.to(DEV))
        for rescale in (True, False):
            ref = model.roi_head.simple_test_padded(feats, dets, num, metas, rescale=rescale)
            got = model.roi_head.aug_test_padded([feats], dets, num, [metas], rescale=rescale)
            assert int(ref[2][0]) == 0 and int(ref[2][1]) > 0
            for r, t in zip(ref, got):
                assert torch.equal(r, t), rescale


def test_decode_tta_one_aug_bits_and_zero_proposals():
    """kernel level, C = 4 and C = 80 (softmax rows of 5 and 81 logits): one identity aug reproduces
    brcnn_rcnn_decode on torch's device softmax bit for bit; rows beyond `num` are never valid"""
    for c, k in ((4, 96), (80, 48)):
        g_ = torch.Generator().manual_seed(c)
        dets = torch.zeros(2, k, 5)
        dets[..., :4] = util.rand_boxes(2 * k, 300., 200., seed=c, min_size=4., max_size=150.).view(2, k, 4)
        dets[..., 4] = torch.rand(2, k, generator=g_)
        cls = (torch.randn(2 * k, c + 1, generator=g_) * 3).to(DEV)
        reg = (torch.randn(2 * k, 4 * c, generator=g_) * 0.3).to(DEV)
        dets, num = dets.to(DEV), torch.tensor([0, k - 7], dtype=torch.int32, device=DEV)
        metas = [[dict(img_shape=(200, 300, 3), scale_factor=np.ones(4, np.float32), flip=False) for _ in range(2)]]
        shape = torch.tensor([[200., 300.]] * 2, device=DEV)
        means, stds = [0.] * 4, [0.1, 0.1, 0.2, 0.2]
        ref = ops.rcnn_decode(cls.softmax(1), reg, dets, num, shape, None, c, 0.05, means, stds)
        got = ops.rcnn_decode_tta(cls[None], reg[None], dets, num, ops.tta_geometry(metas, dets), None, c, 0.05, means,
                                  stds, 'fused')
        for r, t in zip(ref, got):
            assert torch.equal(r, t), c
        assert not got[3][0].any() and not got[3][1].view(k, c)[k - 7:].any() and got[3][1].any()


def test_bad_arguments_are_refused():
    L = lib.load()
    x = torch.zeros(64, device=DEV)
    p, s = x.data_ptr(), lib.raw_stream_handle()
    one = (ctypes.c_void_p * 1)(p)
    k1 = (ctypes.c_int * 1)(4)
    m4 = (ctypes.c_float * 4)(0, 0, 0, 0)
    assert L.brcnn_tta_map_rois(None, p, 1, 1, 4, p, s) == -22
    assert L.brcnn_tta_map_rois(p, p, 17, 1, 4, p, s) == -22
    assert L.brcnn_tta_map_rois(p, p, 0, 1, 4, p, s) == -22
    assert L.brcnn_tta_map_rois(p, p, 1, 0, 4, p, s) == -22
    assert L.brcnn_tta_gather_proposals(one, one, k1, 17, p, 1, p, p, p, p, s) == -22
    assert L.brcnn_tta_gather_proposals(one, one, k1, 1, None, 1, p, p, p, p, s) == -22
    assert L.brcnn_tta_gather_proposals(one, one, (ctypes.c_int * 1)(0), 1, p, 1, p, p, p, p, s) == -22
    assert L.brcnn_tta_gather_proposals((ctypes.c_void_p * 1)(None), one, k1, 1, p, 1, p, p, p, p, s) == -22
    ok = [p, p, p, p, p, None, 1, 1, 2, 1, 0, 0.05, m4, m4, 0.016, p, p, p, p, s]
    for i, bad in ((0, None), (6, 17), (6, 0), (9, 0), (10, 2), (12, None), (14, 0.0), (18, None)):
        args = list(ok)
        args[i] = bad
        assert L.brcnn_rcnn_decode_tta(*args) == -22, i
    with pytest.raises(lib.BrcnnHipError):
        ops.tta_map_rois(torch.zeros(1, 4, 5), torch.zeros(1, 1, 8))       # host tensors
    torch.cuda.synchronize()


def _coco_head(nms):
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'boosting_rcnn', 'boosting_rcnn_r50_fpn_1x_coco.py'))
    rc = brcnn.ConfigDict(dict(score_thr=0.05, nms=nms, max_per_img=100))
    torch.manual_seed(80)
    head = brcnn.build_head(dict(cfg.model.roi_head, train_cfg=None, test_cfg=rc))
    with torch.no_grad():       # (the stock init leaves every class at the same score: spread them)
        head.bbox_head.fc_cls.weight.mul_(20)
        head.bbox_head.fc_reg.weight.mul_(20)
    return head.to(DEV).eval()


@pytest.mark.parametrize('nms', [dict(type='nms', iou_threshold=0.5),
                                 dict(type='soft_nms', iou_threshold=0.5, min_score=0.05)])
def test_coco_head_split_threshold_branches_equal_chain(nms):
    """C = 80, 256 proposals: 20 480 candidates per image, above mmcv's split_thr -- the per-class (soft-)NMS branch of
    `aug_test_padded` against the per-image torch chain `aug_test`, at the g10 end-to-end test's device-vs-chain bar"""
    head = _coco_head(nms)
    g_ = torch.Generator().manual_seed(81)
    sizes = [(32, 48), (16, 24), (8, 12), (4, 6), (2, 3)]
    base = [torch.randn(2, 256, h, w, generator=g_) for h, w in sizes]
    x = [tuple(f.to(DEV) for f in base), tuple(f.flip(3).contiguous().to(DEV) for f in base)]
    shapes = [(128, 189, 3), (120, 192, 3)]
    metas = [[dict(img_shape=shapes[b], scale_factor=np.array([1.2, 1.1, 1.2, 1.1], np.float32), flip=bool(a),
                   flip_direction='horizontal' if a else None) for b in range(2)] for a in range(2)]
    props = []
    for b in range(2):
        bx = util.rand_boxes(256, 189 / 1.2, 120 / 1.1, seed=82 + b, min_size=6., max_size=90.)
        props.append(torch.cat([bx, util.tie_free_scores(256, seed=84 + b)[:, None]], 1).to(DEV))
    merged, num = torch.stack(props), torch.tensor([256, 256], dtype=torch.int32, device=DEV)
    with torch.no_grad():
        feats = [[blocks.to_nhwc(f).contiguous() for f in xa] for xa in x]
        for rescale in (True, False):
            det, lab, nd = head.aug_test_padded(feats, merged, num, metas, rescale=rescale)
            chain = head.aug_test(x, props, metas, rescale=rescale)
            for b in range(2):
                n = int(nd[b])
                got = core.bbox2result(det[b, :n], lab[b, :n], 80)
                assert n > 20
                ref_all, got_all = np.concatenate(chain[b]), np.concatenate(got)
                assert _match_dets(got_all, ref_all) >= 0.95 and _match_dets(ref_all, got_all) >= 0.95, (b, rescale)


def _run(model, inputs, mode, rescale, batch=None):
    imgs, metas = inputs
    if batch is not None:
        imgs, metas = tta_util.single(imgs, metas, batch)
    model.roi_head.test_cfg['tta_scores'] = mode
    try:
        with torch.no_grad():
            return model(return_loss=False, rescale=rescale, img=[t.to(DEV) for t in imgs],
                         img_metas=[[dict(m) for m in ms] for ms in metas])
    finally:
        del model.roi_head.test_cfg['tta_scores']


def test_end_to_end_golden(model, g, inputs):
    """`model(return_loss=False, img=[5 augs], ...)` on the device path, the two-image batch at once: mode 'raw' against
    the reference's own `forward_test` (both `rescale` values), mode 'fused' against the composed expectation; merged
    proposals against the reference's; device path against the per-image chain.  Measures and bars of the g10 test."""
    imgs, metas = inputs
    for rescale in (True, False):
        res = _run(model, inputs, 'raw', rescale)
        assert len(res) == B and len(res[0]) == C
        for b in range(B):
            for c in range(C):
                ref = g[f'ref_res{int(rescale)}_{b}_{c}']
                assert res[b][c].dtype == np.float32 and res[b][c].shape[1] == 5
                assert _match_dets(res[b][c], ref) >= 0.99, (rescale, b, c, len(ref), len(res[b][c]))
                assert _match_dets(ref, res[b][c]) >= 0.99, (rescale, b, c)
    assert sum(len(g[f'ref_res1_{b}_{c}']) for b in range(B) for c in range(C)) > 20
    res = _run(model, inputs, 'fused', True)
    with torch.no_grad():
        dev_imgs = [t.to(DEV) for t in imgs]
        feats = [model.extract_feat_nhwc(t) for t in dev_imgs]
        merged, num, _ = model.rpn_head.aug_test_rpn_padded(feats, metas)
        x = [model.extract_feat(t) for t in dev_imgs]
        pl = model.rpn_head.aug_test_rpn(x, metas)
        res2 = model.roi_head.aug_test(x, pl, metas, rescale=True)
    for b in range(B):
        ref_p = g[f'merged_{b}']
        assert _match_dets(merged[b, :int(num[b])].cpu().numpy(), ref_p, 5e-2, 1e-3) > 0.97
        assert _match_dets(pl[b].cpu().numpy(), ref_p, 5e-2, 1e-3) > 0.97
        det, lab = g[f'fused_det_{b}'], g[f'fused_lab_{b}']
        for c in range(C):
            ref = det[lab == c]
            assert _match_dets(res[b][c], ref) >= 0.99, (b, c, len(ref), len(res[b][c]))
            assert _match_dets(ref, res[b][c]) >= 0.99, (b, c)
            assert _match_dets(res[b][c], res2[b][c]) >= 0.95 and _match_dets(res2[b][c], res[b][c]) >= 0.95
    # an image of the batch gets what it gets alone with the same padded tensors
    for b in range(B):
        alone = _run(model, inputs, 'fused', True, batch=b)
        for c in range(C):
            assert _match_dets(alone[0][c], res[b][c], 1e-3, 1e-5) == 1.0 and len(alone[0][c]) == len(res[b][c])


@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
def test_tta_16bit_close_to_fp32(model, inputs, dtype):
    """the 16-bit conv stack under TTA: runs, and the detection count stays within the share the existing 16-bit
    end-to-end test allows (tests/test_bf16_gpu.py: 20 % + 5)"""
    r32 = _run(model, inputs, 'fused', True)
    try:
        model.set_compute_dtype(dtype)
        r16 = _run(model, inputs, 'fused', True)
    finally:
        blocks.set_compute_dtype('f32')
    n32 = sum(len(c) for r in r32 for c in r)
    n16 = sum(len(c) for r in r16 for c in r)
    assert n32 > 0 and abs(n16 - n32) <= 0.2 * n32 + 5, (n16, n32)
    assert all(np.isfinite(c).all() for r in r16 for c in r)


def test_one_host_synchronisation(model, inputs, monkeypatch):
    """one `forward_test` TTA call: nothing in `aug_test_device` synchronises with the host (torch's sync debug mode
    raises on any), and `aug_test` around it performs exactly one device -> host copy"""
    imgs, metas = inputs
    dev_imgs = [t.to(DEV) for t in imgs]
    _run(model, inputs, 'fused', True)          # warm-up: constant tables, workspaces, weight caches
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with torch.no_grad():
            out = model.aug_test_device(dev_imgs, metas, rescale=True)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert int(out[2].sum()) > 0
    copies = []
    real_cpu, real_tolist, real_item = torch.Tensor.cpu, torch.Tensor.tolist, torch.Tensor.item

    def counted(fn, name):
        def wrapper(self, *a, **k):
            if self.is_cuda:
                copies.append(name)
            return fn(self, *a, **k)
        return wrapper
    monkeypatch.setattr(torch.Tensor, 'cpu', counted(real_cpu, 'cpu'))
    monkeypatch.setattr(torch.Tensor, 'tolist', counted(real_tolist, 'tolist'))
    monkeypatch.setattr(torch.Tensor, 'item', counted(real_item, 'item'))
    with torch.no_grad():
        model(return_loss=False, rescale=True, img=dev_imgs, img_metas=metas)
    assert copies == ['cpu'], copies


def _tool(name):
    spec = importlib.util.spec_from_file_location(f'brcnn_tool_{name}', os.path.join(ROOT, 'tools', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_test_tool_runs_a_flip_and_multiscale_config(tmp_path):
    """tools/test.py on the synthetic dataset of tests/test_drivers_gpu.py with `flip=True` and two `img_scale`s in
    `data.test.pipeline`: four augs per image, batches of two; writes results and an mAP"""
    from brcnn import apis
    from tests.test_drivers_cpu import CLASSES, _tiny_cfg
    cfg = _tiny_cfg(tmp_path, max_epochs=1)
    aug = cfg.data.test.pipeline[1]
    assert aug['type'] == 'MultiScaleFlipAug'
    aug['img_scale'] = [(160, 96), (240, 144)]
    aug['flip'] = True
    cfg.data.val.pipeline = copy.deepcopy(cfg.data.test.pipeline)
    cfg.data.test['samples_per_gpu'] = 2
    cfg_path = str(tmp_path / 'tta_cfg.py')
    cfg.dump(cfg_path)
    m = build_detector(cfg.model)
    m.load_state_dict(util.seeded_state_dict(m, seed=10))
    m.CLASSES = CLASSES
    ckpt = str(tmp_path / 'seeded.pth')
    apis.save_checkpoint(m, ckpt)
    out_pkl = str(tmp_path / 'tta.pkl')
    metric = _tool('test').main([cfg_path, ckpt, '--eval', 'bbox', '--out', out_pkl])
    assert metric == {} or 0.0 <= metric['bbox_mAP'] <= 1.0
    res = pickle.load(open(out_pkl, 'rb'))
    assert len(res) == 7 and len(res[0]) == len(CLASSES) and res[0][0].shape[1] == 5
    assert sum(len(c) for r in res for c in r) > 0
