"""-m gpu: the batched front-door kernel against the C oracle and the per-image kernel (bit exact), and the public
inference API (`inference_detector`, `inference_stream`, tools/infer.py) against the host chain, end to end."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import apis, blocks, build_detector, lib, ops
from brcnn import pipelines as P
from oracle import orc
from tests import inference_util as U
from tests import util
from tests.test_drivers_cpu import CLASSES, _tiny_cfg
from tests.test_drivers_gpu import _tool

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DIRECTION = {0: None, 1: 'horizontal', 2: 'vertical', 3: 'diagonal'}


def _launch_nan_filled(door, images):
    """stage + ONE launch into a destination pre-filled with NaN -> (plan, per-aug tensors)"""
    slot = door.acquire()
    plan = door.stage(slot, images)
    n = plan.block_bytes
    slot.dev[:n].copy_(slot.pinned[:n], non_blocking=True)
    dst = torch.full((plan.dst_elems,), float('nan'), device=DEV)
    ops.preprocess_u8_batch(slot.dev[plan.table_bytes:n], slot.dev, slot.host[:plan.table_bytes].view(ops.PRE_JOB_DTYPE),
                            dst, door.mean, door.std, door.to_rgb)
    torch.cuda.synchronize()
    door.release(slot)
    return plan, [dst[o:o + int(np.prod(s))].view(s).cpu() for o, s in zip(plan.aug_offsets, plan.aug_shapes)]


@pytest.mark.parametrize('to_rgb', [True, False])
@pytest.mark.parametrize('name', ['tta', 'scale_factor', 'tail'])
def test_batched_kernel_bit_exact_vs_oracle_and_per_image_kernel(name, to_rgb):
    """every (aug, image) region of the ONE launch equals the C oracle's image padded to the BATCH shape and the
    per-image kernel's, under torch.equal; the NaN pre-fill proves every element is written"""
    make, shapes = {'tta': (U.tta_pipeline, U.SHAPES), 'scale_factor': (U.sf_pipeline, U.SHAPES_SF),
                    'tail': (U.tail_pipeline, U.SHAPES)}[name]
    pipe = make(norm=dict(U.NORM, to_rgb=to_rgb))
    door = P.BatchFrontDoor(pipe, DEV)
    images = U.random_images(shapes, seed=11)
    plan, outs = _launch_nan_filled(door, images)
    assert len(outs) == {'tta': 6, 'scale_factor': 2, 'tail': 1}[name]
    if name == 'tail':
        assert plan.aug_shapes[0][3] % 4 != 0
    B = len(images)
    for a, out in enumerate(outs):
        assert not torch.isnan(out).any(), (name, a)
        _, _, PH, PW = plan.aug_shapes[a]
        for b, img in enumerate(images):
            j = plan.jobs[a * B + b]
            nw, nh, flip = int(j['new_w']), int(j['new_h']), DIRECTION[int(j['flip'])]
            ref = orc.preprocess_u8(img, nw, nh, PH, PW, flip, U.NORM['mean'], U.NORM['std'], to_rgb)
            assert torch.equal(out[b], ref), (name, a, b, to_rgb)
            one = torch.full((3, PH, PW), float('nan'), device=DEV)
            ops.preprocess_u8(torch.from_numpy(img).to(DEV), one, nw, nh, flip, U.NORM['mean'], U.NORM['std'], to_rgb)
            assert torch.equal(out[b], one.cpu()), (name, a, b, to_rgb)
    # and the public call gives the host chain's tensors and metas
    data = door(images)
    ref = U.host_chain(pipe, images)
    assert all(torch.equal(x.cpu(), y) for x, y in zip(data['img'], ref['img'])) and len(data['img']) == len(ref['img'])
    U.assert_metas_equal(data['img_metas'], ref['img_metas'])


def test_batched_kernel_refuses_bad_arguments_and_queues_nothing():
    door = P.BatchFrontDoor(U.pipeline(img_scale=(64, 48)), DEV)
    images = U.random_images([(33, 17), (20, 40)], seed=1)
    plan = door.plan_batch([i.shape for i in images])
    src = torch.from_numpy(np.concatenate([i.reshape(-1) for i in images])).to(DEV)
    jobs_dev = torch.from_numpy(plan.jobs.view(np.uint8)).to(DEV)
    mean, std = U.NORM['mean'], U.NORM['std']

    def run(jobs=plan.jobs, src=src, jobs_dev=jobs_dev, dst=None, std=std):
        dst = torch.full((plan.dst_elems,), 5.0, device=DEV) if dst is None else dst
        ops.preprocess_u8_batch(src, jobs_dev, jobs, dst, mean, std)
        return dst
    good = run()
    assert not (good == 5.0).any()

    def broken(**fields):
        jobs = plan.jobs.copy()
        for k, v in fields.items():
            jobs[k][1] = v
        return jobs
    cases = [dict(jobs=broken(pad_h=8)), dict(jobs=broken(pad_w=8)),                      # pad smaller than the new size
             dict(jobs=broken(src_off=plan.src_bytes - 10)), dict(jobs=broken(src_off=-3)),     # a row past the source block
             dict(jobs=broken(dst_off=plan.dst_elems - 5)),                                   # ... past the destination
             dict(jobs=broken(flip=4)), dict(jobs=broken(new_w=0)), dict(jobs=broken(first_block=0)),
             dict(jobs=broken(scale_x=0.5)), dict(std=[1., 0., 1.]),
             dict(src=src.cpu()), dict(jobs_dev=jobs_dev.cpu()), dict(dst=torch.zeros(plan.dst_elems))]   # CPU tensors
    for kw in cases:
        dst = kw.get('dst', torch.full((plan.dst_elems,), 5.0, device=DEV))
        with pytest.raises((lib.BrcnnHipError, AssertionError)):
            run(**dict(kw, dst=dst))
        torch.cuda.synchronize()
        assert not dst.is_cuda or bool((dst == 5.0).all()), kw.keys()            # nothing was queued
    with pytest.raises(ValueError):
        P.BatchFrontDoor(U.pipeline(img_scale=(160, 96), pad=dict(size=(64, 67))), DEV)(U.random_images([(75, 113)]))
    with pytest.raises(TypeError):
        door([np.zeros((8, 8), np.uint8)])


# --------------------------------------------------------------------------- the API end to end
TINY_SHAPES = [(75, 113), (60, 90), (96, 160), (120, 80), (33, 47)]
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def _tiny_tta_pipeline():
    return U.pipeline(img_scale=[(160, 96), (128, 80)], flip=True, flip_direction=['horizontal', 'vertical'])


@pytest.fixture(scope='module')
def tiny(tmp_path_factory):
    """config file + checkpoint of the tiny recipe with seeded weights"""
    tmp = tmp_path_factory.mktemp('infer')
    cfg = _tiny_cfg(tmp, max_epochs=1)
    model = build_detector(cfg.model)
    model.load_state_dict(util.seeded_state_dict(model, seed=10))
    model.CLASSES = CLASSES
    ckpt = str(tmp / 'seeded.pth')
    apis.save_checkpoint(model, ckpt, meta=dict(epoch=1))
    cfg_path = str(tmp / 'tiny_cfg.py')
    cfg.dump(cfg_path)
    return cfg_path, ckpt, tmp


def _host_reference(model, pipe, images):
    data = U.host_chain(pipe, images)
    data = dict(img=[t.to(DEV) for t in data['img']], img_metas=data['img_metas'])
    with torch.no_grad():
        return data, model(return_loss=False, rescale=True, img=data['img'], img_metas=copy.deepcopy(data['img_metas']))


def _assert_results_identical(got, ref):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert len(g) == len(r) == len(CLASSES)
        for x, y in zip(g, r):
            assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('tta', [False, True], ids=['plain', 'tta'])
def test_inference_detector_equals_host_chain(tiny, dtype, tta):
    """the batched front door's tensors equal the host chain's bit for bit, so the detections are compared as
    IDENTICAL arrays: same inputs, same kernels, and the device-resident test path has no atomics"""
    cfg_path, ckpt, tmp = tiny
    opts = {'data.test.pipeline': _tiny_tta_pipeline()} if tta else None
    try:
        model = apis.init_detector(cfg_path, ckpt, device=DEV, cfg_options=opts, dtype=dtype)
        assert tuple(model.CLASSES) == CLASSES and not model.training
        pipe = model.cfg.data.test.pipeline
        images = U.random_images(TINY_SHAPES, seed=21)
        # the tensors the model is handed
        door = apis._front_door(model)
        assert door is not None
        data = door(images)
        ref_data, ref = _host_reference(model, pipe, images)
        assert len(data['img']) == (6 if tta else 1)
        assert all(torch.equal(a, b) for a, b in zip(data['img'], ref_data['img']))
        U.assert_metas_equal(data['img_metas'], U.host_chain(pipe, images)['img_metas'])
        print(f'[{dtype} tta={tta}] detections per image:', [sum(len(c) for c in r) for r in ref])
        # B = 5: list and tuple give lists
        for batch in (list(images), tuple(images)):
            got = apis.inference_detector(model, batch)
            assert model.last_path == 'batched' and isinstance(got, list)
            _assert_results_identical(got, ref)
        # B = 1: a bare array and a bare .npy path give the one result
        _, ref1 = _host_reference(model, pipe, images[:1])
        got = apis.inference_detector(model, images[0])
        assert model.last_path == 'batched' and len(got) == len(CLASSES) and isinstance(got[0], np.ndarray)
        _assert_results_identical([got], ref1)
        path = str(tmp / f'one_{dtype}_{tta}.npy')
        np.save(path, images[0])
        got = apis.inference_detector(model, path)
        assert model.last_path == 'batched'
        _assert_results_identical([got], ref1)
        # a pipeline outside the door (pad_val != 0): the Compose chain serves it
        model.cfg.data.test.pipeline[1]['transforms'][3]['pad_val'] = 1
        apis.inference_detector(model, images[:2])
        assert model.last_path == 'compose'
    finally:
        blocks.set_compute_dtype('f32')


@pytest.fixture(scope='module')
def stream_model(tiny):
    cfg_path, ckpt, _ = tiny
    return apis.init_detector(cfg_path, ckpt, device=DEV)


def _stream_images():
    rng = np.random.RandomState(31)
    shapes = [(int(rng.randint(30, 130)), int(rng.randint(30, 170))) for _ in range(19)]
    return U.random_images(shapes, seed=32)


@pytest.mark.parametrize('prefetch', [1, 2])
def test_inference_stream_order_partial_batch_and_block_reuse(stream_model, prefetch):
    model = stream_model
    images = _stream_images()
    ref = []
    for i in range(0, 19, 8):
        ref += apis.inference_detector(model, images[i:i + 8])
    assert len(ref) == 19
    for _ in range(2):                  # the second pass reuses the staging blocks under their fences
        got = list(apis.inference_stream(model, iter(images), batch_size=8, prefetch=prefetch))
        assert model.last_path == 'batched'
        _assert_results_identical(got, ref)
    # leaving early joins the worker and the side stream; the door still works
    gen = apis.inference_stream(model, images, batch_size=4, prefetch=prefetch)
    first = next(gen)
    gen.close()
    assert len(first) == len(CLASSES)          # (another batch composition, another padded shape: liveness only)
    import threading
    assert not any(t.name == 'brcnn-front-door' for t in threading.enumerate())
    _assert_results_identical(apis.inference_detector(model, images[:8]), ref[:8])


def test_inference_stream_worker_error_reaches_the_consumer(stream_model, tmp_path):
    import threading
    model = stream_model
    images = _stream_images()
    ref = apis.inference_detector(model, images[:8])
    items = list(images)
    items[10] = str(tmp_path / 'missing.npy')               # in batch 2
    got = []
    with pytest.raises(FileNotFoundError):
        for r in apis.inference_stream(model, items, batch_size=8, prefetch=2):
            got.append(r)
    _assert_results_identical(got, ref)                     # batch 1 was delivered before the error
    assert not any(t.name == 'brcnn-front-door' for t in threading.enumerate())
    _assert_results_identical(apis.inference_detector(model, images[:8]), ref)


def test_front_door_adds_no_host_synchronisation(stream_model, monkeypatch):
    """front door + `simple_test_device` under torch's sync debug mode (raises on any synchronising call), and the
    device -> host copies of one streamed batch counted: exactly those of the model pass on resident tensors"""
    model = stream_model
    images = _stream_images()[:8]
    door = apis._front_door(model)
    apis.inference_detector(model, images)          # warm-up: staging blocks, constant tables, weight caches
    apis.inference_detector(model, images)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        data = door(images)
        for img, metas in zip(data['img'], data['img_metas']):
            for m in metas:
                m['batch_input_shape'] = tuple(img.shape[-2:])
        with torch.no_grad():
            out = model.simple_test_device(data['img'][0], data['img_metas'][0], rescale=True)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert out[2].numel() == 8
    copies = []
    real = {n: getattr(torch.Tensor, n) for n in ('cpu', 'tolist', 'item')}

    def counted(name):
        def wrapper(self, *a, **k):
            if self.is_cuda:
                copies.append(name)
            return real[name](self, *a, **k)
        return wrapper
    for n in real:
        monkeypatch.setattr(torch.Tensor, n, counted(n))
    resident = door(images)
    torch.cuda.synchronize()
    copies.clear()
    with torch.no_grad():
        model(return_loss=False, rescale=True, **resident)
    per_pass = list(copies)
    assert per_pass, 'the model pass reads its result back'
    copies.clear()
    got = list(apis.inference_stream(model, images * 3, batch_size=8, prefetch=2))
    assert len(got) == 24 and copies == per_pass * 3, (copies, per_pass)


def test_infer_tool_writes_what_inference_detector_returns(tiny, tmp_path):
    cfg_path, ckpt, _ = tiny
    folder = tmp_path / 'frames'
    os.makedirs(folder)
    images = U.random_images(TINY_SHAPES, seed=41)
    files = []
    for i, img in enumerate(images):
        files.append(str(folder / f'f{i}.npy'))
        np.save(files[-1], img)
    out = str(tmp_path / 'res.json')
    infer = _tool('infer')
    infer.main([cfg_path, ckpt, str(folder), '--batch-size', '2', '--score-thr', '0.0', '--out', out])
    records = json.load(open(out))
    model = apis.init_detector(cfg_path, ckpt, device=DEV)
    expect = []
    for i in range(0, 5, 2):
        for f, res in zip(files[i:i + 2], apis.inference_detector(model, files[i:i + 2])):
            expect += infer.to_records(f, res, CLASSES, 0.0)
    assert records == json.loads(json.dumps(expect))
    assert all(set(r) == {'file', 'bbox', 'score', 'category'} and len(r['bbox']) == 4 for r in records)
    assert {r['file'] for r in records} <= set(files) and all(r['category'] in CLASSES for r in records)
