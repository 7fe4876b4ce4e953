"""The GFL baseline at batch B x 3x800x1344 (seeded synthetic weights): the new launches alone at the recipe's shapes (five
levels from stride 8, one anchor of 8 strides per cell -- 22 400 anchors per image --, 4 classes, reg_max 16, nms_pre 1000) --
each with the bytes it has to move and the time those take at 8 TB/s of HBM -- beside the aten composition it replaces (the
host mirror's chain run on device tensors, same process), and the train step of the recipe in BRCNN_DTYPE (default bf16)
beside the boosted UTDAC recipe's.  The assignment is brcnn_atss_assign (tools/atss_bench.py), the ranking score
brcnn_dense_score (tools/retinanet_bench.py).
Prints one JSON line per measurement; inference throughput is tools/bench_recipes.py's."""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import brcnn  # noqa: E402,F401
from brcnn import build_head, ops, train_ops  # noqa: E402
from brcnn.config import ConfigDict  # noqa: E402
from brcnn.dense_heads import distance2bbox  # noqa: E402
from tests import gfl_inputs as gi  # noqa: E402
from tests import util  # noqa: E402
from tools.faster_rcnn_bench import B, HBM, device_ms, train_step  # noqa: E402

C, K, G, N = 4, 1000, 6, 17
SIZES = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
WIDE_A, WIDE_R = 32, 96           # columns of the training convs' padded head outputs (fp32): 4 -> 32, 68 -> 96


def kernels():
    g = torch.Generator().manual_seed(1)
    cfg = gi.head_cfg(C)
    cfg['anchor_generator']['octave_base_scale'] = 8
    cfg['test_cfg'] = dict(gi.TEST_CFG, nms_pre=K, max_per_img=100)
    head = build_head(ConfigDict(cfg)).cuda()
    L = len(SIZES)
    n = sum(h * w for h, w in SIZES)
    rows = B * n
    base = head._base_table()
    # the fused head outputs as GFLHead.forward_rows leaves them: [cls C | pad] (8 columns) and [4 x 17 logits | pad] (72)
    a = (torch.randn(rows, 8, generator=g) * 2 - 4).cuda()
    r = (torch.randn(rows, 72, generator=g) * 2).cuda()
    lay = ops.GflLayout(a, r, C, 16)
    scales = torch.ones(L).cuda()
    shp = torch.tensor([[800., 1333.]] * B).cuda()
    sf = torch.tensor([[1.1, 1.2, 1.1, 1.2]] * B).cuda()
    res = {}
    # ---- test time
    res['dense_score on A in place (the ranking score)'] = (device_ms(lambda: ops.gfl_score(a, lay)), rows * (C + 1) * 4)
    scored, raw, r0 = ops.gfl_score(a, lay), [], 0
    for h, w in SIZES:
        raw.append(scored[r0:r0 + B * h * w].view(B, h * w))
        r0 += B * h * w
    inds = [p[1] for p in ops.rpn_topk(raw, K)]
    T = sum(i.shape[1] for i in inds)
    res['gfl_decode_levels'] = (
        device_ms(lambda: ops.gfl_decode_levels(inds, a, r, lay, scales, SIZES, gi.STRIDES, base, shp, sf, 0.05)),
        B * T * (8 + 4 * (C + 4 * N) + 16) + B * T * C * (16 + 4 + 8 + 1) + 4 * B)
    anchors = head.anchor_generator.grid_anchors(SIZES, 'cuda')
    head.integral.cuda()

    def aten_decode():
        bl, sl, r0 = [], [], 0
        for (h, w), an, idx, st in zip(SIZES, anchors, inds, gi.STRIDES):
            va, vr = a[r0:r0 + B * h * w].view(B, h * w, -1), r[r0:r0 + B * h * w].view(B, h * w, -1)
            r0 += B * h * w
            sl.append(torch.gather(va[..., :C], 1, idx[..., None].expand(-1, -1, C)).sigmoid())
            d = head.integral(torch.gather(vr[..., :4 * N], 1, idx[..., None].expand(-1, -1, 4 * N))).view(B, -1, 4) * st
            box = distance2bbox(head.anchor_center(an[idx]), d)
            bl.append(torch.stack([box[..., 0].clamp(0, 1333), box[..., 1].clamp(0, 800), box[..., 2].clamp(0, 1333),
                                   box[..., 3].clamp(0, 800)], -1))
        boxes, scores = torch.cat(bl, 1) / sf[:, None, :], torch.cat(sl, 1)
        return (boxes[:, :, None, :].expand(B, T, C, 4).reshape(B, T * C, 4), scores.reshape(B, T * C),
                torch.arange(C, device='cuda').repeat(B, T), scores.reshape(B, T * C) > 0.05)
    res['aten: gather + sigmoid + integral + distance2bbox + rescale + class fan-out'] = (device_ms(aten_decode), 0)
    # ---- train time: G ground truths per image
    gt_list = [util.rand_boxes(G, img_w=1333., img_h=800., seed=b, min_size=40., max_size=500.) for b in range(B)]
    gl_list = [torch.randint(0, C, (G,), generator=g) for _ in range(B)]
    gts, gls, offs = train_ops.flatten_gts(gt_list, gl_list)
    gts, gls = gts.cuda(), gls.cuda()
    dev_gt, dev_gl = [t.cuda() for t in gt_list], [t.cuda() for t in gl_list]
    gt_inds = train_ops.atss_assign(gts, offs, B, SIZES, gi.STRIDES, base, gi.TOPK)
    ya = (torch.randn(rows, WIDE_A, generator=g) * 2 - 4).cuda().requires_grad_()
    yr = torch.cat([r.detach().cpu(), torch.zeros(rows, WIDE_R - 72)], 1).cuda().requires_grad_()
    lay_t = ops.GflLayout(ya, yr, C, 16)
    meta = train_ops.GflLossMeta(B, SIZES, gi.STRIDES, base, 16, C, offs, 2.0, 1e-6, 1.0, 2.0, 0.25)
    sc = scales.clone().requires_grad_()
    fwd_bytes = rows * C * 4 + rows * 4 * 3          # the class columns, gt_inds three times (two terms, positive count)
    res['gfl_loss forward + finalize'] = (
        device_ms(lambda: train_ops.gfl_loss(ya.detach(), yr.detach(), scales, gt_inds, gts, gls, lay_t, meta)), fwd_bytes)

    def fwd_bwd():
        ya.grad = yr.grad = sc.grad = None
        train_ops.gfl_loss(ya, yr, sc, gt_inds, gts, gls, lay_t, meta)[0].sum().backward()
    res['gfl_loss forward + finalize + backward'] = (device_ms(fwd_bwd), 2 * fwd_bytes + rows * (WIDE_A + WIDE_R) * 4)
    # the aten composition: the host mirror's loss on device tensors (it reads the positive counts back, as the reference)
    metas = [dict(img_shape=(800, 1333, 3), pad_shape=(800, 1344, 3)) for _ in range(B)]

    def levels(y, c0, c1):
        out, r0 = [], 0
        for (h, w) in SIZES:
            out.append(y[r0:r0 + B * h * w, c0:c1].reshape(B, h, w, c1 - c0).permute(0, 3, 1, 2))
            r0 += B * h * w
        return out

    def host_chain(backward):
        cls, reg = levels(ya, 0, C), levels(yr, 0, 4 * N)
        anchor_list, flags = head.get_anchors(SIZES, metas, device='cuda')
        head._all_valid = None
        an, labels, lw, bt, _, num_pos, _ = head.get_targets(anchor_list, flags, dev_gt, metas, gt_labels_list=dev_gl,
                                                             label_channels=C)
        out = [head.loss_single(*args, num_total_samples=float(max(num_pos, 1)))
               for args in zip(an, cls, reg, labels, lw, bt, gi.STRIDES)]
        avg = sum(o[3] for o in out).clamp(min=1)
        total = sum(o[0] + (o[1] + o[2]) / avg for o in out)
        if backward:
            ya.grad = yr.grad = None
            total.backward()
        return total
    res['aten: targets + QFL + GIoU + DFL, forward'] = (device_ms(lambda: host_chain(False), n=5, warm=1), 0)
    res['aten: targets + QFL + GIoU + DFL, forward + backward'] = (device_ms(lambda: host_chain(True), n=5, warm=1), 0)
    for k, (ms, nbytes) in res.items():
        print(json.dumps(dict(what=k, us=ms * 1e3, bytes=nbytes, hbm_floor_us=nbytes / HBM * 1e6)), flush=True)


if __name__ == '__main__':
    kernels()
    for path in ('configs/gfl/gfl_r50_fpn_1x_utdac.py', 'configs/boosting_rcnn/boosting_rcnn_r50_pafpn_1x_utdac.py'):
        train_step(path)
