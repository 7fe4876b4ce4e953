"""not-gpu: the inference API (`init_detector`, `inference_detector`) and the host side of the batched front door
(`pipelines.BatchFrontDoor`): plan parity with the host Compose + collate chain, the pipelines it takes and refuses, the
fallback chain, and the C-ABI surface of the batched kernel."""
import copy
import glob
import os
import re
import warnings

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import Config, apis, lib, ops
from brcnn import pipelines as P
from tests import inference_util as U
from tests.test_host_cpu import CFG, ROOT


def _utdac_pipeline():
    return Config.fromfile(CFG).data.test.pipeline


PLANS = [('utdac', _utdac_pipeline, U.SHAPES), ('tta', U.tta_pipeline, U.SHAPES), ('scale_factor', U.sf_pipeline, U.SHAPES_SF)]


@pytest.mark.parametrize('name,make,shapes', PLANS, ids=[p[0] for p in PLANS])
def test_plan_equals_host_chain(name, make, shapes):
    """per aug: batch shape and img_metas EQUAL to Compose + collate on random images of the same shapes; the job
    table tiles the source block and the destination tensors without gap or overlap"""
    pipe = make()
    assert P.BatchFrontDoor.supported(pipe)
    plan_cfg = P.BatchFrontDoor.parse(pipe)
    door = object.__new__(P.BatchFrontDoor)         # (the constructor allocates nothing, but wants a device name)
    door.__dict__.update(plan_cfg)
    images = U.random_images(shapes, seed=5)
    ref = U.host_chain(pipe, images)
    plan = door.plan_batch([i.shape for i in images])
    A, B = len(ref['img']), len(images)
    assert A == len(door.augs) == {'utdac': 1, 'tta': 6, 'scale_factor': 2}[name]
    assert [tuple(t.shape) for t in ref['img']] == plan.aug_shapes
    U.assert_metas_equal(plan.img_metas, ref['img_metas'])
    if name == 'tta':       # MultiScaleFlipAug's order: scales outside, (no flip), (flip, d)... inside
        assert [(m[0]['flip'], m[0]['flip_direction']) for m in plan.img_metas] == \
            [(False, None), (True, 'horizontal'), (True, 'vertical')] * 2
    # the table
    jobs = plan.jobs
    assert jobs.dtype == ops.PRE_JOB_DTYPE and jobs.dtype.itemsize == 64 and len(jobs) == A * B
    src_cover, blocks = 0, 0
    for b, (h, w) in enumerate(shapes):
        assert plan.src_offsets[b] == src_cover
        src_cover += h * w * 3
    assert src_cover == plan.src_bytes and plan.block_bytes == plan.table_bytes + plan.src_bytes == 64 * A * B + src_cover
    dst_cover = 0
    for a in range(A):
        _, _, PH, PW = plan.aug_shapes[a]
        assert plan.aug_offsets[a] % 4 == 0 and 0 <= plan.aug_offsets[a] - dst_cover < 4
        dst_cover = plan.aug_offsets[a]
        for b, (h, w) in enumerate(shapes):
            j = jobs[a * B + b]
            meta = plan.img_metas[a][b]
            assert (j['src_off'], j['src_h'], j['src_w']) == (plan.src_offsets[b], h, w)
            assert (j['new_h'], j['new_w'], 3) == meta['img_shape'] and (j['pad_h'], j['pad_w']) == (PH, PW)
            assert j['dst_off'] == dst_cover and j['first_block'] == blocks
            assert j['flip'] == {None: 0, 'horizontal': 1, 'vertical': 2}[meta['flip_direction']]
            assert j['scale_x'] == 1.0 / (float(j['new_w']) / float(w)) and j['scale_y'] == 1.0 / (float(j['new_h']) / float(h))
            dst_cover += 3 * PH * PW
            blocks += ops.preprocess_blocks(PH, PW)
    assert dst_cover == plan.dst_elems and blocks == plan.num_blocks


def test_plan_raises_where_the_host_chain_raises():
    door = object.__new__(P.BatchFrontDoor)
    door.__dict__.update(P.BatchFrontDoor.parse(U.pipeline(img_scale=(160, 96), pad=dict(size=(64, 67)))))
    img = U.random_images([(75, 113)])
    with pytest.raises(ValueError):
        U.host_chain(U.pipeline(img_scale=(160, 96), pad=dict(size=(64, 67))), img)     # Pad smaller than the image
    with pytest.raises(ValueError):
        door.plan_batch([i.shape for i in img])
    door.__dict__.update(P.BatchFrontDoor.parse(U.sf_pipeline()))
    with pytest.raises(ValueError):
        door.plan_batch([(1, 1, 3)])            # a one-pixel image under scale_factor=0.5: width 0
    # the fixed Pad that holds every resized image (the kernel's scalar-tail case) plans
    door.__dict__.update(P.BatchFrontDoor.parse(U.tail_pipeline()))
    plan = door.plan_batch([(h, w, 3) for h, w in U.SHAPES])
    assert plan.aug_shapes == [(6, 3, 64, 67)]
    U.assert_metas_equal(plan.img_metas, U.host_chain(U.tail_pipeline(), U.random_images(U.SHAPES))['img_metas'])


def test_supported_pipelines():
    cfgs = sorted(glob.glob(os.path.join(ROOT, 'configs', 'boosting_rcnn', '*.py')))
    assert len(cfgs) == 9
    for c in cfgs:
        assert P.BatchFrontDoor.supported(Config.fromfile(c)), c
    assert P.BatchFrontDoor.supported(U.pipeline(img_scale=(1333, 800), fmt='DefaultFormatBundle', load='LoadImageFromWebcam'))
    crop = U.pipeline(img_scale=(1333, 800))
    crop[1]['transforms'].insert(2, dict(type='RandomCrop', crop_size=(64, 64)))
    assert not P.BatchFrontDoor.supported(crop)
    assert not P.BatchFrontDoor.supported(U.pipeline(img_scale=(1333, 800), pad=dict(size_divisor=32, pad_val=1)))
    no_norm = U.pipeline(img_scale=(1333, 800))
    del no_norm[1]['transforms'][2]
    assert not P.BatchFrontDoor.supported(no_norm)
    assert not P.BatchFrontDoor.supported([dict(type='LoadImageFromFile', to_float32=True)] + U.pipeline(img_scale=(64, 48))[1:])
    assert not P.BatchFrontDoor.supported(U.pipeline(scale_factor=1))       # (Resize asserts a float)
    assert not P.BatchFrontDoor.accepts([np.zeros((4, 4), np.uint8)]) and not P.BatchFrontDoor.accepts([np.zeros((4, 4, 3), np.float32)])
    assert P.BatchFrontDoor.accepts([np.zeros((4, 4, 3), np.uint8), 'x.png'])


class _Stub(torch.nn.Module):
    """records what inference_detector hands to the model"""

    def __init__(self, pipe):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.cfg = Config(dict(data=dict(test=dict(pipeline=pipe))))
        self.calls = []

    def forward(self, img, img_metas, return_loss=True, **kw):
        self.calls.append((img, img_metas, return_loss, kw))
        return [('result', i) for i in range(len(img_metas[0]))]


@pytest.mark.parametrize('make', [U.tta_pipeline, lambda: U.pipeline(img_scale=(160, 96), pad=dict(size_divisor=32, pad_val=1))])
def test_inference_detector_fallback_chain_gives_the_host_pipeline(make, tmp_path):
    pipe = make()
    before = copy.deepcopy(pipe)
    model = _Stub(pipe)
    images = U.random_images([(75, 113), (60, 90), (33, 17)], seed=9)
    out = apis.inference_detector(model, images)
    assert model.last_path == 'compose' and out == [('result', 0), ('result', 1), ('result', 2)]      # (a CPU model: no device door)
    img, metas, return_loss, kw = model.calls[-1]
    assert return_loss is False and kw == dict(rescale=True)
    ref = U.host_chain(pipe, images)
    assert len(img) == len(ref['img']) and all(torch.equal(a, b) for a, b in zip(img, ref['img']))
    U.assert_metas_equal(metas, ref['img_metas'])
    # one image, as an array and as a path: the single result, `filename` in the metas
    assert apis.inference_detector(model, images[0]) == ('result', 0)
    path = str(tmp_path / 'a.npy')
    np.save(path, images[0])
    assert apis.inference_detector(model, path) == ('result', 0)
    assert model.calls[-1][1][0][0]['filename'] == path and model.calls[-2][1][0][0]['filename'] is None
    assert torch.equal(model.calls[-1][0][0], model.calls[-2][0][0])
    assert apis.inference_detector(model, (images[1], images[2])) == [('result', 0), ('result', 1)]
    assert model.cfg.data.test.pipeline == before          # the model's config is left alone
    assert list(apis.inference_stream(model, images, batch_size=2)) == [('result', 0), ('result', 1), ('result', 0)]


def test_init_detector(tmp_path):
    from tests.test_drivers_cpu import CLASSES
    from brcnn.datasets import CocoDataset
    with pytest.raises(TypeError):
        apis.init_detector(dict(model=1))
    model = apis.init_detector(CFG, device='cpu', cfg_options={'model.test_cfg.rcnn.max_per_img': 33})
    assert not model.training and model.cfg.model.test_cfg.rcnn.max_per_img == 33 and model.test_cfg.rcnn.max_per_img == 33
    assert model.cfg.model.train_cfg is None and model.cfg.model.pretrained is None and model.train_cfg is None
    assert not hasattr(model, 'CLASSES') or model.CLASSES is None       # no checkpoint: no class names
    model.CLASSES = CLASSES
    with_meta, bare = str(tmp_path / 'meta.pth'), str(tmp_path / 'bare.pth')
    apis.save_checkpoint(model, with_meta, meta=dict(epoch=1))
    torch.save(dict(state_dict=model.state_dict()), bare)
    cfg = Config.fromfile(CFG)
    assert cfg.model.train_cfg is not None
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        m2 = apis.init_detector(cfg, with_meta, device='cpu')
    assert m2.cfg is cfg and cfg.model.train_cfg is None and tuple(m2.CLASSES) == CLASSES and not m2.training
    k = 'roi_head.bbox_head.fc_cls.weight'
    assert torch.equal(m2.state_dict()[k], model.state_dict()[k])
    with pytest.warns(UserWarning, match='COCO classes'):
        m3 = apis.init_detector(CFG, bare, device='cpu')
    assert m3.CLASSES == CocoDataset.CLASSES and len(m3.CLASSES) == 80
    assert brcnn.init_detector is apis.init_detector and brcnn.inference_detector is apis.inference_detector and \
        brcnn.inference_stream is apis.inference_stream


def test_load_image_from_webcam_fields():
    img = U.random_images([(7, 9)])[0]
    t = P.build_from_cfg(dict(type='LoadImageFromWebcam'), P.PIPELINES)
    r = t(dict(img=img))
    assert r['filename'] is None and r['ori_filename'] is None and r['img'] is img
    assert r['img_shape'] == r['ori_shape'] == (7, 9, 3) and r['img_fields'] == ['img']
    assert P.build_from_cfg(dict(type='LoadImageFromWebcam', to_float32=True), P.PIPELINES)(dict(img=img))['img'].dtype == np.float32


def test_batched_kernel_abi():
    header = open(os.path.join(ROOT, 'include', 'brcnn_hip.h')).read()
    declared = set(re.findall(r'\b(brcnn_[a-z0-9_]+)\s*\(', header))
    for name in ('brcnn_preprocess_u8_batch', 'brcnn_preprocess_u8_batch_blocks'):
        assert name in declared and name in lib.SIGNATURES
    L = lib.load()
    assert hasattr(L, 'brcnn_preprocess_u8_batch')
    # the struct of the header and the numpy row agree field by field
    body = re.search(r'typedef struct brcnn_pre_job \{(.*?)\} brcnn_pre_job;', header, re.S).group(1)
    fields = []
    for typ, names in re.findall(r'(int64_t|double|int32_t)\s+([^;]+);', body):
        fields += [(n.strip(), {'int64_t': '<i8', 'double': '<f8', 'int32_t': '<i4'}[typ]) for n in names.split(',')]
    assert np.dtype(fields) == ops.PRE_JOB_DTYPE and ops.PRE_JOB_DTYPE.itemsize == 64
    assert int(re.search(r'#define BRCNN_PRE_MAX_JOBS (\d+)', header).group(1)) == ops.PRE_MAX_JOBS
    # the host's tile count is the library's (a host function: no device call)
    for ph, pw in [(1, 1), (64, 128), (65, 129), (800, 1344), (64, 67), (1088, 1920)]:
        assert L.brcnn_preprocess_u8_batch_blocks(ph, pw) == ops.preprocess_blocks(ph, pw)
    assert L.brcnn_preprocess_u8_batch_blocks(0, 5) == 0
    # argument errors are answered before any device call
    assert L.brcnn_preprocess_u8_batch(None, 0, None, None, 0, None, 0, None, None, 1, None) == -22
    with pytest.raises(lib.BrcnnHipError):
        ops.preprocess_u8_batch(torch.zeros(12, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8),
                                np.zeros(1, ops.PRE_JOB_DTYPE), torch.zeros(12), [0, 0, 0], [1, 1, 1])
