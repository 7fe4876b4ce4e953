"""The Cascade R-CNN baseline at batch B x 3x800x1344 (seeded synthetic weights): the three hand-over launches alone at
the recipe's shapes (1000 RoIs per image at test time, 512 sampled rows per image in training, 4 classes, class-agnostic
deltas) -- each with the bytes it has to move and the time those take at 8 TB/s of HBM -- beside the aten composition it
replaces (the host mirror's refinement / ensemble run on device tensors), and the train step of the recipe in
BRCNN_DTYPE (default bf16) beside the Faster R-CNN one.  Prints one JSON line per measurement; inference throughput is
tools/bench_recipes.py's (RECIPES=cascade_rcnn,faster_rcnn,1x_utdac)."""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import brcnn  # noqa: E402,F401
from brcnn import build_head, ops, train_ops  # noqa: E402
from brcnn.config import ConfigDict  # noqa: E402
from tests import cascade_rcnn_inputs as ci  # noqa: E402
from tests import util  # noqa: E402
from tools.faster_rcnn_bench import B, HBM, device_ms, train_step  # noqa: E402

C = 4
MEANS, STDS = (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)


def kernels():
    g = torch.Generator().manual_seed(1)
    rh = build_head(ConfigDict(ci.roi_head_cfg())).cuda()
    metas = [dict(img_shape=(800, 1333, 3), scale_factor=[1., 1., 1., 1.]) for _ in range(B)]
    shp = torch.tensor([[800., 1333.]] * B).cuda()
    res = {}
    # ---- test time: K = 1000 proposals per image
    K = 1000
    dets = torch.cat([util.rand_boxes(B * K, seed=3), torch.rand(B * K, 1, generator=g)], 1).view(B, K, 5).cuda()
    numk = torch.full((B,), K, dtype=torch.int32).cuda()
    cls = [(torch.randn(B * K, C + 1, generator=g) * 2).cuda() for _ in range(3)]
    reg = (torch.randn(B * K, 4, generator=g) * 0.5).cuda()
    _, ls = ops.cascade_refine_test(dets, numk, cls[0], reg, shp, C, MEANS, STDS, reg_class_agnostic=True)
    row = (C + 1) * 4
    res['cascade_refine_test'] = (
        device_ms(lambda: ops.cascade_refine_test(dets, numk, cls[1], reg, shp, C, MEANS, STDS, reg_class_agnostic=True,
                                                  logit_sum=ls)),
        B * K * (20 + row + 16 + 20 + 2 * row))                 # dets, logits, deltas in; dets out; logit_sum read + written

    def aten_refine_test():
        # CascadeRoIHead.simple_test's between-stage step on device tensors, per image, and the running sum of the logits
        rois = torch.cat([torch.arange(B, device='cuda', dtype=torch.float32).repeat_interleave(K)[:, None],
                          dets.view(-1, 5)[:, :4]], 1)
        out = []
        for b in range(B):
            sl = slice(b * K, (b + 1) * K)
            out.append(rh.regress_by_class(0, rois[sl], cls[1][sl][:, :-1].argmax(1), reg[sl], metas[b]))
        return torch.cat(out), ls + cls[1]
    res['aten: regress_by_class per image + logit sum'] = (device_ms(aten_refine_test), 0)
    res['cascade_mean_softmax'] = (device_ms(lambda: ops.cascade_mean_softmax(ls, cls[2], 3)), B * K * 3 * row)
    res['aten: (s0 + s1 + s2) / 3 then softmax'] = (device_ms(lambda: ((cls[0] + cls[1] + cls[2]) / 3.0).softmax(-1)), 0)
    # ---- train time: 512 sampled rows per image, a quarter positive, six added ground truths in front
    n = 512
    offs = [b * n for b in range(B + 1)]
    rois = torch.cat([torch.arange(B, dtype=torch.float32).repeat_interleave(n)[:, None], util.rand_boxes(B * n, seed=4)], 1).cuda()
    labels = torch.where(torch.arange(B * n) % n < 128, torch.randint(0, C, (B * n,), generator=g), torch.tensor(C)).cuda()
    flags = (torch.arange(B * n) % n < 6).int().cuda()
    clt = (torch.randn(B * n, C + 1, generator=g) * 2).cuda()
    rgt = (torch.randn(B * n, 4, generator=g) * 0.5).cuda()
    res['cascade_refine_train'] = (
        device_ms(lambda: train_ops.cascade_refine_train(rois, labels, flags, offs, clt, rgt, shp, C, MEANS, STDS,
                                                         reg_class_agnostic=True)),
        B * n * (20 + 8 + 4 + 16 + 20) + 4 * B)                # (an agnostic head's logits are not read)
    pos_is_gts = [flags[b * n:b * n + 128].to(torch.uint8) for b in range(B)]

    def aten_refine_train():
        lab = torch.where(labels == C, clt[:, :-1].argmax(1), labels)
        return rh.refine_bboxes(0, rois, lab, rgt, pos_is_gts, metas)
    res['aten: argmax + refine_bboxes per image'] = (device_ms(aten_refine_train), 0)
    for k, (ms, nbytes) in res.items():
        print(json.dumps(dict(what=k, us=ms * 1e3, bytes=nbytes, hbm_floor_us=nbytes / HBM * 1e6)), flush=True)


if __name__ == '__main__':
    kernels()
    for path in ('configs/cascade_rcnn/cascade_rcnn_r50_fpn_1x_utdac.py', 'configs/faster_rcnn/faster_rcnn_r50_fpn_1x_utdac.py'):
        train_step(path)
