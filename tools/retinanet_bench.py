"""The RetinaNet baseline at batch B x 3x800x1344 (seeded synthetic weights): the new launches alone at the recipe's
shapes (five levels from stride 8, 9 anchors per cell, 4 classes, nms_pre 1000) -- each with the bytes it has to move and
the time those take at 8 TB/s of HBM -- beside the aten composition it replaces (the host mirror's chain run on device
tensors), and the train step of the recipe in BRCNN_DTYPE (default bf16) beside the boosted UTDAC recipe's.
Prints one JSON line per measurement; inference throughput is tools/bench_recipes.py's
(RECIPES=retinanet,faster_rcnn,cascade_rcnn,1x_utdac)."""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import brcnn  # noqa: E402,F401
from brcnn import build_head, core, ops, train_ops  # noqa: E402
from brcnn.config import ConfigDict  # noqa: E402
from brcnn.losses import py_sigmoid_focal_loss  # noqa: E402
from tests import retinanet_inputs as ri  # noqa: E402
from tests import util  # noqa: E402
from tools.faster_rcnn_bench import B, HBM, device_ms, train_step  # noqa: E402

C, A, K = 4, 9, 1000
SIZES = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
WIDE = 64           # columns of the training convs' padded head outputs


def kernels():
    g = torch.Generator().manual_seed(1)
    cfg = ri.head_cfg(C)
    cfg['test_cfg'] = dict(ri.TEST_CFG, nms_pre=K, max_per_img=100)
    head = build_head(ConfigDict(cfg)).cuda()
    L = len(SIZES)
    # (the class maps of all levels are views of ONE (rows, A*C) tensor, as RetinaHead.forward_rows leaves them)
    cls_rows = (torch.randn(B * sum(h * w for h, w in SIZES), A * C, generator=g) * 2 - 4).cuda()
    cls, r0 = [], 0
    for h, w in SIZES:
        cls.append(cls_rows[r0:r0 + B * h * w].view(B, h, w, A * C))
        r0 += B * h * w
    reg = [(torch.randn(B, h, w, 4 * A, generator=g) * 0.3).cuda() for h, w in SIZES]
    bases = [head.anchor_generator.base_anchors[l].cuda() for l in range(L)]
    strides = list(head.anchor_generator.strides)
    anchors = head.anchor_generator.grid_anchors(SIZES, 'cuda')
    shp = torch.tensor([[800., 1333.]] * B).cuda()
    sf = torch.tensor([[1.1, 1.2, 1.1, 1.2]] * B).cuda()
    cells = sum(h * w for h, w in SIZES)
    n = cells * A
    res = {}
    # ---- test time
    res['dense_score (all levels, one launch)'] = (device_ms(lambda: ops.dense_score(cls_rows, A, C)), B * n * (C + 1) * 4)
    res['aten: sigmoid + max over classes'] = (device_ms(lambda: [c.sigmoid().view(B, -1, C).max(-1)[0] for c in cls]), 0)
    raw = [ops.dense_score(c, A, C).view(B, -1) for c in cls]
    picked = ops.rpn_topk(raw, K)
    inds = [p[1] for p in picked]
    T = sum(i.shape[1] for i in inds)
    res['dense_decode_levels'] = (
        device_ms(lambda: ops.dense_decode_levels(inds, cls, reg, bases, SIZES, strides, C, shp, sf, head.bbox_coder.means,
                                                  head.bbox_coder.stds, 0.05)),
        B * T * (8 + 4 * C + 16) + B * T * C * (16 + 4 + 8 + 1) + 4 * B)

    def aten_decode():
        bl, sl = [], []
        for c, r, an, idx in zip(cls, reg, anchors, inds):
            s = torch.gather(c.view(B, -1, C), 1, idx[..., None].expand(-1, -1, C)).sigmoid()
            d = torch.gather(r.view(B, -1, 4), 1, idx[..., None].expand(-1, -1, 4))
            bl.append(core.delta2bbox(an[idx], d, head.bbox_coder.means, head.bbox_coder.stds, max_shape=(800, 1333)))
            sl.append(s)
        boxes, scores = torch.cat(bl, 1) / sf[:, None, :], torch.cat(sl, 1)
        return (boxes[:, :, None, :].expand(B, T, C, 4).reshape(B, T * C, 4), scores.reshape(B, T * C),
                torch.arange(C, device='cuda').repeat(B, T), scores.reshape(B, T * C) > 0.05)
    res['aten: gather + sigmoid + delta2bbox + rescale + class fan-out'] = (device_ms(aten_decode), 0)
    # ---- train time: 120 positives per image, an ignore band of 400 anchors
    rows = B * cells
    ycls = (torch.randn(rows, WIDE, generator=g) * 2 - 4).cuda().requires_grad_()
    yreg = (torch.randn(rows, WIDE, generator=g) * 0.3).cuda().requires_grad_()
    gt_inds = torch.zeros(B, n, dtype=torch.int32)
    for b in range(B):
        p = torch.randperm(n, generator=g)
        gt_inds[b][p[:120]] = torch.randint(1, 7, (120,), generator=g, dtype=torch.int32)
        gt_inds[b][p[120:520]] = -1
    gt_inds = gt_inds.cuda()
    gts = util.rand_boxes(6 * B, img_w=1333., img_h=800., seed=2, min_size=40., max_size=500.).cuda()
    gls = torch.randint(0, C, (6 * B,), generator=g).cuda()
    offs = [6 * b for b in range(B + 1)]
    meta = train_ops.DenseLossMeta(B, SIZES, strides, bases, A, C, offs, 2.0, 0.25, -1, 0.0, (0., 0., 0., 0.), (1., 1., 1., 1.),
                                   1.0, 1.0)
    fwd_bytes = rows * 2 * WIDE * 4 + B * n * 4
    res['dense_loss forward + finalize'] = (
        device_ms(lambda: train_ops.dense_loss(ycls.detach(), yreg.detach(), gt_inds, gts, gls, meta)), fwd_bytes)

    def fwd_bwd():
        ycls.grad = yreg.grad = None
        train_ops.dense_loss(ycls, yreg, gt_inds, gts, gls, meta)[0].sum().backward()
    res['dense_loss forward + finalize + backward'] = (device_ms(fwd_bwd), 2 * fwd_bytes + rows * 2 * WIDE * 4)
    # the aten composition: loss_single of the host mirror per level on device tensors, targets given
    labels = torch.where(gt_inds > 0, gls[(offs[0] + gt_inds.long() - 1).clamp(min=0)], torch.full((), C, device='cuda'))
    weights = (gt_inds >= 0).float()
    tgt = torch.randn(B, n, 4, generator=g).cuda() * (gt_inds > 0)[..., None]
    lv = [0]
    for h, w in SIZES:
        lv.append(lv[-1] + h * w * A)

    def aten_loss(backward):
        ycls.grad = yreg.grad = None
        total, r0 = 0.0, 0
        for l, (h, w) in enumerate(SIZES):
            nr = B * h * w
            x = ycls[r0:r0 + nr, :A * C].reshape(-1, C)
            p = yreg[r0:r0 + nr, :4 * A].reshape(-1, 4)
            r0 += nr
            lab = labels[:, lv[l]:lv[l + 1]].reshape(-1)
            onehot = torch.nn.functional.one_hot(lab, C + 1)[:, :C]
            wl = weights[:, lv[l]:lv[l + 1]].reshape(-1)
            total = total + py_sigmoid_focal_loss(x, onehot, wl, reduction='mean', avg_factor=960.0)
            total = total + ((p - tgt[:, lv[l]:lv[l + 1]].reshape(-1, 4)).abs() * (lab < C)[:, None]).sum() / 960.0
        if backward:
            total.backward()
        return total
    res['aten: focal + L1 per level, targets given, forward'] = (device_ms(lambda: aten_loss(False), n=10, warm=2), 0)
    res['aten: focal + L1 per level, targets given, forward + backward'] = (device_ms(lambda: aten_loss(True), n=10, warm=2), 0)
    for k, (ms, nbytes) in res.items():
        print(json.dumps(dict(what=k, us=ms * 1e3, bytes=nbytes, hbm_floor_us=nbytes / HBM * 1e6)), flush=True)


if __name__ == '__main__':
    kernels()
    for path in ('configs/retinanet/retinanet_r50_fpn_1x_utdac.py', 'configs/boosting_rcnn/boosting_rcnn_r50_pafpn_1x_utdac.py'):
        train_step(path)
