"""Seeded inputs of the test-time-augmentation fixture (tests/golden/g24_tta.npz): the golden generator and the tests
rebuild the same aug images from a seed instead of storing them (4 MB of noise).  Only exact operations: a CPU
generator, integer nearest-neighbour index arithmetic, flips and zero padding -- the same bits on every machine."""
import numpy as np
import torch

# (scale, flip direction or None) of the five augs: 1.0 / 1.0 + horizontal / 1.5 / 1.5 + vertical / 0.75 + diagonal
TTA_AUGS = ((1.0, None), (1.0, 'horizontal'), (1.5, None), (1.5, 'vertical'), (0.75, 'diagonal'))
TTA_SOURCES = ((120, 180), (104, 164))      # source image sizes (h, w): two images of different shape in one batch
_FLIP_DIMS = {'horizontal': (2,), 'vertical': (1,), 'diagonal': (1, 2)}


def tta_inputs(seed=24, sources=TTA_SOURCES, augs=TTA_AUGS, divisor=32):
    """-> (imgs, img_metas): per aug a (B, 3, PH, PW) batch padded to a multiple of `divisor` and its metas"""
    g = torch.Generator().manual_seed(seed)
    srcs = [torch.randn(3, h, w, generator=g) for h, w in sources]
    imgs, img_metas = [], []
    for scale, direction in augs:
        sized, metas = [], []
        for src in srcs:
            H, W = src.shape[1:]
            h, w = int(H * scale + 0.5), int(W * scale + 0.5)
            rows, cols = (torch.arange(h) * H) // h, (torch.arange(w) * W) // w
            im = src[:, rows][:, :, cols]
            if direction is not None:
                im = im.flip(_FLIP_DIMS[direction])
            sized.append(im.contiguous())
            metas.append(dict(img_shape=(h, w, 3), ori_shape=(H, W, 3), filename='<tta>.png',
                              scale_factor=np.array([w / W, h / H, w / W, h / H], dtype=np.float32),
                              flip=direction is not None, flip_direction=direction))
        ph = -(-max(t.shape[1] for t in sized) // divisor) * divisor
        pw = -(-max(t.shape[2] for t in sized) // divisor) * divisor
        batch = torch.zeros(len(sized), 3, ph, pw)
        for b, im in enumerate(sized):
            batch[b, :, :im.shape[1], :im.shape[2]] = im
            metas[b]['pad_shape'] = (ph, pw, 3)
        imgs.append(batch)
        img_metas.append(metas)
    return imgs, img_metas


def single(imgs, img_metas, b):
    """image `b` of the batch alone, with the same padded tensors"""
    return [im[b:b + 1] for im in imgs], [[dict(m[b])] for m in img_metas]
