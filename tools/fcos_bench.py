"""The FCOS baseline at batch B x 3x800x1344 (seeded synthetic weights): the new launches alone at the recipe's shapes (five
levels from stride 8, 4 classes, nms_pre 1000) -- each with the bytes it has to move and the time those take at 8 TB/s of
HBM -- beside the aten composition it replaces (the host mirror's chain run on device tensors), and the train step of the
recipe in BRCNN_DTYPE (default bf16) beside the boosted UTDAC recipe's.
Prints one JSON line per measurement; inference throughput is tools/bench_recipes.py's."""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import brcnn  # noqa: E402,F401
from brcnn import build_head, ops, train_ops  # noqa: E402
from brcnn.config import ConfigDict  # noqa: E402
from tests import fcos_inputs as fi  # noqa: E402
from tests import util  # noqa: E402
from tools.faster_rcnn_bench import B, HBM, device_ms, train_step  # noqa: E402

C, K = 4, 1000
SIZES = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
RANGES = ((-1, 64), (64, 128), (128, 256), (256, 512), (512, 1e8))
WIDE = 32           # columns of the training convs' padded head outputs (fp32)


def kernels():
    g = torch.Generator().manual_seed(1)
    cfg = fi.head_cfg(C, regress_ranges=RANGES)
    cfg['test_cfg'] = dict(fi.TEST_CFG, nms_pre=K, max_per_img=100)
    head = build_head(ConfigDict(cfg)).cuda()
    L = len(SIZES)
    n = sum(h * w for h, w in SIZES)
    rows = B * n
    # the fused head outputs as FCOSHead.forward_rows leaves them: [cls C | ctr 1 | pad] and [reg 4 | pad]
    a = (torch.randn(rows, 8, generator=g) * 2 - 4).cuda()
    r = torch.cat([torch.randn(B * h * w, 8, generator=g) * 0.5 + float(torch.log(torch.tensor(1.5 * s)))
                   for (h, w), s in zip(SIZES, fi.STRIDES)]).cuda()
    lay = ops.FcosLayout(a, r, C, 0, 0, False, C)
    scales = torch.ones(L).cuda()
    shp = torch.tensor([[800., 1333.]] * B).cuda()
    sf = torch.tensor([[1.1, 1.2, 1.1, 1.2]] * B).cuda()
    res = {}
    # ---- test time
    res['fcos_score (all levels, one launch)'] = (device_ms(lambda: ops.fcos_score(a, r, lay)), rows * (C + 2) * 4)
    res['aten: sigmoid x sigmoid + max over classes'] = (
        device_ms(lambda: (a[:, :C].sigmoid() * a[:, C:C + 1].sigmoid()).max(-1)[0]), 0)
    scored, raw, r0 = ops.fcos_score(a, r, lay), [], 0
    for h, w in SIZES:
        raw.append(scored[r0:r0 + B * h * w].view(B, h * w))
        r0 += B * h * w
    inds = [p[1] for p in ops.rpn_topk(raw, K)]
    T = sum(i.shape[1] for i in inds)
    res['fcos_decode_levels'] = (
        device_ms(lambda: ops.fcos_decode_levels(inds, a, r, lay, scales, SIZES, fi.STRIDES, shp, sf, 0.05)),
        B * T * (8 + 4 * (C + 1) + 16) + B * T * C * (16 + 4 + 8 + 1) + 4 * B)
    pts = head.get_points(SIZES, torch.float32, 'cuda')

    def aten_decode():
        bl, sl, cl, r0 = [], [], [], 0
        for (h, w), p, idx, s in zip(SIZES, pts, inds, fi.STRIDES):
            va, vr = a[r0:r0 + B * h * w].view(B, h * w, -1), r[r0:r0 + B * h * w].view(B, h * w, -1)
            r0 += B * h * w
            sc = torch.gather(va[..., :C], 1, idx[..., None].expand(-1, -1, C)).sigmoid()
            ct = torch.gather(va[..., C], 1, idx).sigmoid()
            d = torch.gather(vr[..., :4], 1, idx[..., None].expand(-1, -1, 4)).exp()
            pp = p[idx]
            bx = torch.stack([pp[..., 0] - d[..., 0], pp[..., 1] - d[..., 1], pp[..., 0] + d[..., 2], pp[..., 1] + d[..., 3]], -1)
            hi = bx.new_tensor([1333., 800., 1333., 800.])
            bx = torch.where(bx < 0, bx.new_zeros(()), bx)
            bl.append(torch.where(bx > hi, hi, bx))
            sl.append(sc)
            cl.append(ct)
        boxes, scores, ctrs = torch.cat(bl, 1) / sf[:, None, :], torch.cat(sl, 1), torch.cat(cl, 1)
        return (boxes[:, :, None, :].expand(B, T, C, 4).reshape(B, T * C, 4), (scores * ctrs[..., None]).reshape(B, T * C),
                torch.arange(C, device='cuda').repeat(B, T), scores.reshape(B, T * C) > 0.05)
    res['aten: gather + sigmoid + exp + distance2bbox + rescale + class fan-out'] = (device_ms(aten_decode), 0)
    # ---- train time: 6 ground truths per image
    gt_list = [util.rand_boxes(6, img_w=1333., img_h=800., seed=b, min_size=40., max_size=500.) for b in range(B)]
    gl_list = [torch.randint(0, C, (6,), generator=g) for _ in range(B)]
    gts, gls, offs = train_ops.flatten_gts(gt_list, gl_list)
    gts, gls = gts.cuda(), gls.cuda()
    res['fcos_assign'] = (device_ms(lambda: train_ops.fcos_assign(gts, offs, B, SIZES, fi.STRIDES, RANGES)),
                          rows * 4 + gts.numel() * 4)
    res['aten: get_targets of the host mirror on device tensors'] = (
        device_ms(lambda: head.get_targets(pts, [t.cuda() for t in gt_list], [t.cuda() for t in gl_list]), n=10, warm=2), 0)
    gt_inds = train_ops.fcos_assign(gts, offs, B, SIZES, fi.STRIDES, RANGES)
    ya = (torch.randn(rows, WIDE, generator=g) * 2 - 4).cuda().requires_grad_()
    yr = torch.cat([r.detach().cpu(), torch.zeros(rows, WIDE - 8)], 1).cuda().requires_grad_()
    lay_t = ops.FcosLayout(ya, yr, C, 0, 0, False, C)
    meta = train_ops.FcosLossMeta(B, SIZES, fi.STRIDES, C, offs, 2.0, 0.25, 1e-6, 1e-6, 1.0, 1.0, 1.0)
    sc = scales.clone().requires_grad_()
    fwd_bytes = rows * (C + 1 + 4) * 4 + rows * 4
    res['fcos_loss forward + finalize'] = (
        device_ms(lambda: train_ops.fcos_loss(ya.detach(), yr.detach(), scales, gt_inds, gts, gls, lay_t, meta)), fwd_bytes)

    def fwd_bwd():
        ya.grad = yr.grad = sc.grad = None
        train_ops.fcos_loss(ya, yr, sc, gt_inds, gts, gls, lay_t, meta)[0].sum().backward()
    res['fcos_loss forward + finalize + backward'] = (device_ms(fwd_bwd), 2 * fwd_bytes + rows * 2 * WIDE * 4)
    # the aten composition: the host mirror's loss on device tensors (it reads the positive count back, as the reference)
    sizes_b = [(B, h, w) for h, w in SIZES]

    def levels(y, c0, c1):
        out, r0 = [], 0
        for (b, h, w) in sizes_b:
            out.append(y[r0:r0 + b * h * w, c0:c1].reshape(b, h, w, c1 - c0).permute(0, 3, 1, 2))
            r0 += b * h * w
        return out

    def aten_loss(backward):
        ya.grad = yr.grad = None
        cls, reg, ctr = levels(ya, 0, C), [t.exp() for t in levels(yr, 0, 4)], levels(ya, C, C + 1)
        f_cls = torch.cat([t.permute(0, 2, 3, 1).reshape(-1, C) for t in cls])
        labels, targets = head.get_targets(pts, [t.cuda() for t in gt_list], [t.cuda() for t in gl_list])
        f_lab, f_t = torch.cat(labels), torch.cat(targets)
        pos = (f_lab < C).nonzero().reshape(-1)
        total = head.loss_cls.loss_weight * brcnn.losses.py_sigmoid_focal_loss(
            f_cls, torch.nn.functional.one_hot(f_lab, C + 1)[:, :C], avg_factor=max(len(pos), 1.0))
        f_box = torch.cat([t.permute(0, 2, 3, 1).reshape(-1, 4) for t in reg])[pos]
        f_ctr = torch.cat([t.permute(0, 2, 3, 1).reshape(-1) for t in ctr])[pos]
        f_pts = torch.cat([p.repeat(B, 1) for p in pts])[pos]
        ct = head.centerness_target(f_t[pos])
        from brcnn.dense_heads import distance2bbox
        total = total + head.loss_bbox(distance2bbox(f_pts, f_box), distance2bbox(f_pts, f_t[pos]), weight=ct,
                                       avg_factor=ct.sum().detach().clamp(min=1e-6))
        total = total + head.loss_centerness(f_ctr, ct, avg_factor=max(len(pos), 1.0))
        if backward:
            total.backward()
        return total
    res['aten: targets + focal + IoU + centerness BCE, forward'] = (device_ms(lambda: aten_loss(False), n=5, warm=1), 0)
    res['aten: targets + focal + IoU + centerness BCE, forward + backward'] = (device_ms(lambda: aten_loss(True), n=5, warm=1), 0)
    for k, (ms, nbytes) in res.items():
        print(json.dumps(dict(what=k, us=ms * 1e3, bytes=nbytes, hbm_floor_us=nbytes / HBM * 1e6)), flush=True)


if __name__ == '__main__':
    kernels()
    for path in ('configs/fcos/fcos_r50_caffe_fpn_gn-head_1x_utdac.py', 'configs/boosting_rcnn/boosting_rcnn_r50_pafpn_1x_utdac.py'):
        train_step(path)
