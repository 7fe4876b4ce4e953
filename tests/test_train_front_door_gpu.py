"""-m gpu: the training front door of the multi-scale recipes on the device -- the chain kernel
(`brcnn_preprocess_u8_chain`: resize, crop, resize, flip, normalise, pad in one launch) against the host's
imresize_u8 -> slice -> imresize_u8 -> imflip -> imnormalize -> impad, the fused transform against the host pipeline,
and the loader with the fused pipeline against the host loader.  Every comparison is exact."""
import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import datasets as D
from brcnn import lib, ops
from brcnn import pipelines as P
from tests.front_door_util import MEAN, SHAPES, STD, chain_cfg, real_policies, sample, same, small_policies

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H, V, DG = 'horizontal', 'vertical', 'diagonal'
# (flip of the source, flip of the result)
FLIPS = [(None, None), (None, H), (None, V), (None, DG), (H, None), (V, None), (DG, None), (H, V)]
_IMGS = {}


def _img(shape):
    if shape not in _IMGS:
        a = np.random.RandomState(shape[0]).randint(0, 256, shape + (3,), dtype=np.uint8)
        _IMGS[shape] = (a, torch.from_numpy(a).to(DEV))
    return _IMGS[shape]


def host_chain(img, src_flip, mid, window, new, flip, pad, to_rgb):
    top, left, ch, cw = window
    x = P.imflip(img, src_flip) if src_flip else img
    x = P.imresize_u8(x, (mid[1], mid[0]))[top:top + ch, left:left + cw]
    x = P.imresize_u8(x, (new[1], new[0]))
    x = P.imflip(x, flip) if flip else x
    x = P.impad(P.imnormalize(x, np.array(MEAN, np.float32), np.array(STD, np.float32), to_rgb), pad)
    return torch.from_numpy(np.ascontiguousarray(x.transpose(2, 0, 1)))


# (source, intermediate (H1, W1), window (top, left, ch, cw), result (H2, W2))
GEOMETRY = {
    # stage 1 up: the four corners of the intermediate image and the whole of it; W2 = 45 is no multiple of 4
    'corner_tl': ((37, 53), (50, 70), (0, 0, 20, 30), (33, 45)),
    'corner_tr': ((37, 53), (50, 70), (0, 40, 20, 30), (33, 45)),
    'corner_bl': ((37, 53), (50, 70), (30, 0, 20, 30), (33, 45)),
    'corner_br': ((37, 53), (50, 70), (30, 40, 20, 30), (33, 45)),
    'whole': ((37, 53), (50, 70), (0, 0, 50, 70), (33, 44)),
    'one_wide': ((37, 53), (50, 70), (5, 7, 20, 1), (40, 9)),
    'one_high': ((61, 47), (80, 60), (7, 5, 1, 20), (6, 44)),
    'one_pixel': ((61, 47), (80, 60), (79, 59, 1, 1), (5, 7)),
    # stage 1 down, stage 2 up and down
    'down_up': ((61, 47), (30, 23), (3, 2, 20, 18), (41, 37)),
    'down_down': ((61, 47), (30, 23), (3, 2, 20, 18), (11, 9)),
    'up_down': ((37, 53), (75, 107), (10, 20, 60, 80), (23, 31)),
    # each stage as the identity, and both (a plain crop)
    'identity_1': ((61, 47), (61, 47), (11, 5, 40, 33), (52, 43)),
    'identity_2': ((61, 47), (90, 70), (11, 5, 40, 33), (40, 33)),
    'identity_both': ((37, 53), (37, 53), (3, 4, 30, 41), (30, 41)),
    # more than one workgroup in both directions (tiles of 64 rows x 128 columns)
    'four_tiles': ((37, 53), (90, 200), (5, 10, 80, 180), (70, 150)),
}


@pytest.mark.parametrize('name', sorted(GEOMETRY))
def test_chain_kernel_equals_host_chain(name):
    shape, mid, window, new = GEOMETRY[name]
    img, src = _img(shape)
    for src_flip, flip in FLIPS:
        for extra in (0, 31):                # pad_w = W2 (16-byte stores only where that is a multiple of 4) and W2 + 31
            pad = (new[0] + extra, new[1] + extra)
            for to_rgb in (True, False):
                out = torch.full((3,) + pad, 7.0, device=DEV)
                ops.preprocess_u8_chain(src, out, mid, window, new, flip, MEAN, STD, to_rgb, src_flip_direction=src_flip)
                ref = host_chain(img, src_flip, mid, window, new, flip, pad, to_rgb)
                assert torch.equal(out.cpu(), ref), (name, src_flip, flip, extra, to_rgb)


def test_chain_kernel_as_one_resize_equals_preprocess_u8():
    """whole window + identity second stage: the existing one-resize kernel, bit for bit"""
    img, src = _img((61, 47))
    for new in [(80, 61), (33, 25)]:
        for flip in (None, H, V, DG):
            a, b = torch.empty((3, 96, 64), device=DEV), torch.empty((3, 96, 64), device=DEV)
            ops.preprocess_u8(src, a, new[1], new[0], flip, MEAN, STD, True)
            ops.preprocess_u8_chain(src, b, new, (0, 0) + new, new, flip, MEAN, STD, True)
            assert torch.equal(a, b), (new, flip)


def test_chain_kernel_rejects_bad_arguments_and_launches_nothing():
    img, src = _img((37, 53))
    out = torch.full((3, 40, 48), 7.0, device=DEV)
    good = dict(mid=(50, 70), window=(5, 6, 20, 30), new=(33, 45))
    bad = [dict(window=(31, 6, 20, 30)), dict(window=(5, 41, 20, 30)), dict(window=(-1, 6, 20, 30)),
           dict(window=(5, -1, 20, 30)), dict(window=(5, 6, 0, 30)), dict(window=(5, 6, 20, 0)), dict(mid=(0, 70)),
           dict(mid=(50, 0)), dict(new=(0, 45)), dict(new=(33, 0)), dict(new=(41, 45)), dict(new=(33, 49))]
    for change in bad:
        g = dict(good, **change)
        with pytest.raises(lib.BrcnnHipError, match='invalid argument'):
            ops.preprocess_u8_chain(src, out, g['mid'], g['window'], g['new'], None, MEAN, STD)
    with pytest.raises(lib.BrcnnHipError, match='invalid argument'):
        ops.preprocess_u8_chain(src, out, good['mid'], good['window'], good['new'], None, MEAN, [58.0, 0.0, 57.0])
    # the C entry itself: null pointers, flip codes, an empty source
    import ctypes
    m3, s3 = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)

    def call(src_p=src.data_ptr(), dst_p=out.data_ptr(), sh=37, sw=53, src_flip=0, flip=0, mean=m3, std=s3):
        return lib.load().brcnn_preprocess_u8_chain(src_p, sh, sw, src_flip, 50, 70, 5, 6, 20, 30, dst_p, 33, 45, 40, 48,
                                                    flip, mean, std, 1, None)
    for kw in (dict(src_p=None), dict(dst_p=None), dict(mean=None), dict(std=None), dict(sh=0), dict(sw=0),
               dict(src_flip=4), dict(src_flip=-1), dict(flip=4), dict(flip=-1)):
        assert call(**kw) == -22, kw
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0                       # the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), host_chain(img, None, (50, 70), (5, 6, 20, 30), (33, 45), None, (40, 48), True))


TAIL = [dict(type='DefaultFormatBundle'), dict(type='Collect', keys=['img', 'gt_bboxes', 'gt_labels'])]


def _check_transform(policies, flip_first, shape, seeds, size_divisor=32, direction='horizontal'):
    cfg = chain_cfg(policies, flip_first, size_divisor, direction=direction) + TAIL
    host, dev = P.Compose(cfg), P.Compose(P.fuse_device_pipeline(cfg, DEV, policies=True))
    assert isinstance(dev.transforms[0], P.FusedAugResizeNormalizePad)
    n = 0
    for s in seeds:
        np.random.seed(s)
        a = host(sample(shape, 1000 + s))
        np.random.seed(s)
        b = dev(sample(shape, 1000 + s))
        assert (a is None) == (b is None), (shape, s)
        if a is None:
            continue
        n += 1
        assert b['img'].data.is_cuda and torch.equal(a['img'].data, b['img'].data.cpu()), (shape, s, flip_first)
        assert torch.equal(a['gt_bboxes'].data, b['gt_bboxes'].data) and a['gt_bboxes'].data.dtype == b['gt_bboxes'].data.dtype
        assert torch.equal(a['gt_labels'].data, b['gt_labels'].data)
        assert same(a['img_metas'].data, b['img_metas'].data), (shape, s)
    return n


@pytest.mark.parametrize('flip_first', [True, False])
@pytest.mark.parametrize('allow_negative_crop', [True, False])
def test_fused_transform_equals_host_pipeline(flip_first, allow_negative_crop):
    n = sum(_check_transform(small_policies(allow_negative_crop), flip_first, shape, range(200),
                             direction=['horizontal', 'vertical', 'diagonal']) for shape in SHAPES)
    assert (n == 600) == allow_negative_crop and n > 200      # only a crop that may reject drops samples


def test_fused_transform_equals_host_pipeline_with_the_recipe_policies():
    assert _check_transform(real_policies(), True, (120, 161), range(4), size_divisor=1) == 4


def test_loader_with_the_fused_pipeline_equals_the_host_loader(tmp_path):
    from tests.golden.synth import synthetic_coco
    ann_file, prefix = synthetic_coco(str(tmp_path))
    classes = ('echinus', 'starfish', 'holothurian', 'scallop')
    host_cfg = [dict(type='LoadImageFromFile'), dict(type='LoadAnnotations', with_bbox=True)] + \
        chain_cfg(small_policies(True), True) + TAIL
    batches = []
    for cfg in (host_cfg, P.fuse_device_pipeline(host_cfg, DEV, policies=True)):
        ds = D.build_dataset(dict(type='CocoDataset', ann_file=ann_file, img_prefix=prefix, classes=classes, pipeline=cfg))
        np.random.seed(5)
        loader = D.build_dataloader(ds, 2, 0, dist=False, seed=5)
        it = iter(loader)
        batches.append((type(loader), [next(it), next(it)]))
    assert batches[1][0] is D.MainProcessTail and batches[0][0] is not D.MainProcessTail
    for a, b in zip(batches[0][1], batches[1][1]):
        assert b['img'].is_cuda and b['img'].shape[0] == 2 and torch.equal(a['img'], b['img'].cpu())
        for k in ('gt_bboxes', 'gt_labels'):
            assert len(a[k]) == len(b[k]) == 2 and all(torch.equal(x, y) for x, y in zip(a[k], b[k]))
        assert same(a['img_metas'], b['img_metas'])
