"""The VFNet baseline at batch B x 3x800x1344 (seeded synthetic weights): the new launches alone at the recipe's shapes (five
levels from stride 8, one point per cell -- 22 400 per image --, 4 classes, 256 channels, nms_pre 1000) -- each with the bytes
it has to move and the time those take at 8 TB/s of HBM -- beside the aten composition it replaces (the host mirror's chain run
on device tensors, same process), the per-level star deformable conv launches (2 x 5 im2col + GEMM in fp32), and the train
step of the recipe in BRCNN_DTYPE (default bf16) beside the boosted UTDAC recipe's.  The assignment is brcnn_atss_assign
(tools/atss_bench.py), the ranking score brcnn_dense_score (tools/retinanet_bench.py).
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
from tests import util  # noqa: E402
from tests import vfnet_inputs as vi  # noqa: E402
from tools.faster_rcnn_bench import B, HBM, device_ms, train_step  # noqa: E402

C, K, G, F = 4, 1000, 6, 256
SIZES = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
WIDE = 32                         # columns of the training convs' padded head outputs (fp32): 4 -> 32


def kernels():
    g = torch.Generator().manual_seed(1)
    cfg = vi.head_cfg(C, in_channels=F, feat_channels=F)
    cfg['anchor_generator']['octave_base_scale'] = 8
    cfg['test_cfg'] = dict(vi.TEST_CFG, nms_pre=K, max_per_img=100)
    head = build_head(ConfigDict(cfg)).cuda()
    L = len(SIZES)
    rows = B * sum(h * w for h, w in SIZES)
    base = head._base_table()
    denoms = [float(d) for d in vi.REG_DENOMS]
    # the fused head outputs as VFNetHead.forward_rows leaves them: [cls C | pad], [4 raw | pad] (8 columns each)
    a = (torch.randn(rows, 8, generator=g) * 2 - 4).cuda()
    r0 = (torch.randn(rows, 8, generator=g) * 0.6 - 1.2).cuda()
    r1 = (torch.randn(rows, 8, generator=g) * 0.3).cuda()
    scales = torch.ones(L).cuda()
    shp = torch.tensor([[800., 1333.]] * B).cuda()
    sf = torch.tensor([[1.1, 1.2, 1.1, 1.2]] * B).cuda()
    res = {}
    # ---- distances and star offsets
    res['vfnet_star_offsets (D0 + 18 offsets per cell)'] = (
        device_ms(lambda: ops.vfnet_star_offsets(r0, scales, B, SIZES, vi.STRIDES, denoms, 0.1)), rows * (16 + 16 + 72))
    d0, off = ops.vfnet_star_offsets(r0, scales, B, SIZES, vi.STRIDES, denoms, 0.1)

    def aten_offsets():
        out, r = [], 0
        for (h, w), s, d in zip(SIZES, vi.STRIDES, denoms):
            n = B * h * w
            p = r0[r:r + n, :4].view(B, h, w, 4).permute(0, 3, 1, 2).exp() * d
            out.append(head.star_dcn_offset(p, 0.1, s))
            r += n
        return out
    res['aten: exp + star_dcn_offset per level'] = (device_ms(aten_offsets), 0)
    # ---- the star deformable convs of one tower: five launches of im2col + GEMM (fp32)
    x = torch.randn(rows, F, generator=g).cuda()
    m, cache = head.vfnet_cls_dconv, head._vf_caches['cls_dconv']
    res['star dconv of one tower, 5 levels (im2col + GEMM + ReLU, fp32)'] = (
        device_ms(lambda: head._star_dconv_rows(x, off, m, cache, B, SIZES)), rows * (F * 4 * 2 + 72 + 9 * F * 4 * 2))
    xb = x.bfloat16()
    cache16 = brcnn.blocks.PackedCache()
    res['star dconv of one tower, 5 levels (16-bit route)'] = (
        device_ms(lambda: head._star_dconv_rows(xb, off, m, cache16, B, SIZES)), rows * (F * 2 * 2 + 72))
    # the same tower, forward + backward in bf16, with the input gradient accumulated in integers (what the head runs:
    # bit-reproducible) and with the fp32 atomics of brcnn_deform_col2im_nhwc_g
    from brcnn.autograd import deform_conv_autograd
    xt = xb.clone().requires_grad_()
    offs_l, q = [], 0
    for h, w in SIZES:
        offs_l.append(off[q:q + B * h * w].view(B, h, w, 18))
        q += B * h * w

    def tower_fwd_bwd(ordered):
        xt.grad = m.weight.grad = None
        ys = [deform_conv_autograd(xl.view(B, h, w, F), ol, m.weight, 1, 1, 1, False, True, True, ordered)
              for xl, ol, (h, w) in zip(torch.split(xt, [B * h * w for h, w in SIZES], 0), offs_l, SIZES)]
        sum(y.float().sum() for y in ys).backward()
    res['star dconv of one tower, forward + backward, bf16, integer dx (ordered)'] = (device_ms(lambda: tower_fwd_bwd(True)), 0)
    res['star dconv of one tower, forward + backward, bf16, fp32-atomic dx'] = (device_ms(lambda: tower_fwd_bwd(False)), 0)
    # ---- test time
    lay = head._layout(a, r1, d0)
    res['dense_score on A in place (the ranking score)'] = (device_ms(lambda: ops.vfnet_score(a, lay)), rows * (C + 1) * 4)
    scored, raw, q = ops.vfnet_score(a, lay), [], 0
    for h, w in SIZES:
        raw.append(scored[q:q + B * h * w].view(B, h * w))
        q += B * h * w
    inds = [p[1] for p in ops.rpn_topk(raw, K)]
    T = sum(i.shape[1] for i in inds)
    res['vfnet_decode_levels'] = (
        device_ms(lambda: ops.vfnet_decode_levels(inds, a, r1, d0, lay, scales, SIZES, vi.STRIDES, base, shp, sf, 0.05)),
        B * T * (8 + 4 * (C + 4 + 4) + 16) + B * T * C * (16 + 4 + 8 + 1) + 4 * B)
    points = head.get_points(SIZES, torch.float32, 'cuda')

    def aten_decode():
        bl, sl, q = [], [], 0
        for (h, w), pts, idx in zip(SIZES, points, inds):
            n = B * h * w
            va, vr, vd = a[q:q + n].view(B, h * w, -1), r1[q:q + n].view(B, h * w, -1), d0[q:q + n].view(B, h * w, 4)
            q += n
            sl.append(torch.gather(va[..., :C], 1, idx[..., None].expand(-1, -1, C)).sigmoid())
            i4 = idx[..., None].expand(-1, -1, 4)
            d = torch.gather(vr[..., :4], 1, i4).exp() * torch.gather(vd, 1, i4)
            box = distance2bbox(pts[idx].reshape(-1, 2), d.reshape(-1, 4)).view(B, -1, 4)
            bl.append(torch.stack([box[..., 0].clamp(0, 1333), box[..., 1].clamp(0, 800), box[..., 2].clamp(0, 1333),
                                   box[..., 3].clamp(0, 800)], -1))
        boxes, scores = torch.cat(bl, 1) / sf[:, None, :], torch.cat(sl, 1)
        return (boxes[:, :, None, :].expand(B, T, C, 4).reshape(B, T * C, 4), scores.reshape(B, T * C),
                torch.arange(C, device='cuda').repeat(B, T), scores.reshape(B, T * C) > 0.05)
    res['aten: gather + sigmoid + exp + distance2bbox + rescale + class fan-out'] = (device_ms(aten_decode), 0)
    # ---- train time: G ground truths per image
    gt_list = [util.rand_boxes(G, img_w=1333., img_h=800., seed=b, min_size=40., max_size=500.) for b in range(B)]
    gl_list = [torch.randint(0, C, (G,), generator=g) for _ in range(B)]
    gts, gls, offs = train_ops.flatten_gts(gt_list, gl_list)
    gts, gls = gts.cuda(), gls.cuda()
    dev_gt, dev_gl = [t.cuda() for t in gt_list], [t.cuda() for t in gl_list]
    gt_inds = train_ops.atss_assign(gts, offs, B, SIZES, vi.STRIDES, base, vi.TOPK)
    ya = (torch.randn(rows, WIDE, generator=g) * 2 - 4).cuda().requires_grad_()
    d1 = ops.vfnet_refine(r1, scales, B, SIZES, d0)
    t0, t1 = d0.clone().requires_grad_(), d1.clone().requires_grad_()
    meta = train_ops.VfnetLossMeta(B, SIZES, vi.STRIDES, base, C, offs, 0.75, 2.0, True, 1e-6, 1.0, 1.5, 2.0)
    fwd_bytes = rows * C * 4 + rows * 4 * 2          # the class columns, gt_inds twice (class term, point terms)
    res['vfnet_loss forward + finalize'] = (
        device_ms(lambda: train_ops.vfnet_loss(ya.detach(), d0, d1, gt_inds, gts, gls, meta)), fwd_bytes)

    def fwd_bwd():
        ya.grad = t0.grad = t1.grad = None
        train_ops.vfnet_loss(ya, t0, t1, gt_inds, gts, gls, meta)[0].sum().backward()
    res['vfnet_loss forward + finalize + backward'] = (device_ms(fwd_bwd), 2 * fwd_bytes + rows * (WIDE + 8) * 4)
    rr0 = r0.clone().requires_grad_()
    sc = scales.clone().requires_grad_()

    def offsets_fwd_bwd():
        rr0.grad = sc.grad = None
        d, offs_l = train_ops.vfnet_star_offsets(rr0, sc, B, SIZES, vi.STRIDES, denoms, 0.1)
        (d.sum() + sum(o.sum() for o in offs_l)).backward()
    res['vfnet_star_offsets forward + backward (with the aten sums that feed it)'] = (device_ms(offsets_fwd_bwd), 0)
    # the aten composition: the host mirror's loss on device tensors (it reads the three normalisers back, as the reference)
    metas = [dict(img_shape=(800, 1333, 3), pad_shape=(800, 1344, 3)) for _ in range(B)]

    def levels(y, c0, c1):
        out, q = [], 0
        for (h, w) in SIZES:
            out.append(y[q:q + B * h * w, c0:c1].reshape(B, h, w, c1 - c0).permute(0, 3, 1, 2))
            q += B * h * w
        return out

    def host_chain(backward):
        cls, p0, p1 = levels(ya, 0, C), levels(t0, 0, 4), levels(t1, 0, 4)
        pts = head.get_points(SIZES, torch.float32, 'cuda')
        labels, _, targets, _ = head.get_targets(cls, pts, dev_gt, dev_gl, metas, None)
        rows_ = lambda lst, n: torch.cat([t.permute(0, 2, 3, 1).reshape(-1, n) for t in lst])        # noqa: E731
        fc, f0, f1 = rows_(cls, C), rows_(p0, 4), rows_(p1, 4)
        fl, ft = torch.cat(labels), torch.cat(targets)
        fp = torch.cat([p.repeat(B, 1) for p in pts])
        pos = ((fl >= 0) & (fl < C)).nonzero().reshape(-1)
        tb = distance2bbox(fp[pos], ft[pos]).detach()
        b0, b1 = distance2bbox(fp[pos], f0[pos]), distance2bbox(fp[pos], f1[pos])
        from brcnn.core import bbox_overlaps
        w0 = bbox_overlaps(b0, tb, is_aligned=True).clamp(min=1e-6).detach()
        w1 = bbox_overlaps(b1, tb, is_aligned=True).clamp(min=1e-6).detach()
        tgt = torch.zeros_like(fc)
        tgt[pos, fl[pos]] = w1
        total = head.loss_cls(fc, tgt, avg_factor=max(float(len(pos)), 1.0)) + \
            head.loss_bbox(b0, tb, weight=w0, avg_factor=w0.sum().clamp(min=1).item()) + \
            head.loss_bbox_refine(b1, tb, weight=w1, avg_factor=w1.sum().clamp(min=1).item())
        if backward:
            ya.grad = t0.grad = t1.grad = None
            total.backward()
        return total
    res['aten: targets + VFL + 2 x GIoU, forward'] = (device_ms(lambda: host_chain(False), n=5, warm=1), 0)
    res['aten: targets + VFL + 2 x GIoU, forward + backward'] = (device_ms(lambda: host_chain(True), n=5, warm=1), 0)
    for k, (ms, nbytes) in res.items():
        print(json.dumps(dict(what=k, us=ms * 1e3, bytes=nbytes, hbm_floor_us=nbytes / HBM * 1e6)), flush=True)


if __name__ == '__main__':
    kernels()
    for path in ('configs/vfnet/vfnet_r50_fpn_1x_utdac.py', 'configs/boosting_rcnn/boosting_rcnn_r50_pafpn_1x_utdac.py'):
        train_step(path)
