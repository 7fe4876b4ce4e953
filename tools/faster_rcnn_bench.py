"""The Faster R-CNN baseline beside the UTDAC boosting recipe at batch B x 3x800x1344 (seeded synthetic weights):
the train step in BRCNN_DTYPE (default bf16), and the new kernels alone at the baseline's shapes -- the sampled RPN loss
forward / backward (five levels from stride 4, 256 anchors drawn per image) and the plain second-stage decode (1000
proposals per image, 4 classes) -- each with the bytes it has to move and the time those take at 8 TB/s of HBM.
Prints one JSON line per measurement; inference throughput is tools/bench_recipes.py's (RECIPES=faster_rcnn,1x_utdac)."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import bench  # noqa: E402
import brcnn  # noqa: E402,F401
from brcnn import Config, build_detector, core, ops, train_ops  # noqa: E402
from tests import util  # noqa: E402

B = int(os.environ.get('B', '8'))
DTYPE = os.environ.get('BRCNN_DTYPE', 'bf16')
HBM = 8e12


def device_ms(fn, n=50, warm=5):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def train_step(path):
    cfg = Config.fromfile(path)
    m = build_detector(cfg.model)
    m.load_state_dict(util.seeded_state_dict(m, seed=0))
    m = m.cuda().train()
    m.set_compute_dtype(DTYPE)
    img, metas = bench.synthetic_batch(B, 'cuda', seed=0)
    g = torch.Generator().manual_seed(0)
    gts = [util.rand_boxes(6, img_w=1333., img_h=800., seed=b, min_size=40., max_size=500.).cuda() for b in range(B)]
    gls = [torch.randint(0, 4, (6,), generator=g).cuda() for _ in range(B)]
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-4, momentum=0.9)

    def step():
        opt.zero_grad(set_to_none=True)
        out = m.train_step(dict(img=img, img_metas=metas, gt_bboxes=gts, gt_labels=gls), opt)
        out['loss'].backward()
        opt.step()
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t, n = time.perf_counter(), 10
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t) / n
    print(json.dumps(dict(what='train_step', recipe=os.path.basename(path), dtype=DTYPE, ms=dt * 1e3, img_per_s=B / dt)),
          flush=True)
    m.set_compute_dtype('f32')


def kernels():
    sizes, strides, A, num, npos, ys = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)], [4, 8, 16, 32, 64], 3, 256, 128, 32
    gen = core.AnchorGenerator(strides=strides, ratios=[0.5, 1.0, 2.0], scales=[8])
    n = sum(h * w for h, w in sizes) * A
    rows = sum(B * h * w for h, w in sizes)
    g = torch.Generator().manual_seed(1)
    y = torch.randn(rows, ys, generator=g).cuda().requires_grad_()
    gt_inds = torch.zeros(B, n, dtype=torch.int32)
    for b in range(B):
        gt_inds[b][torch.randperm(n, generator=g)[:300]] = torch.randint(1, 7, (300,), generator=g, dtype=torch.int32)
    gts = util.rand_boxes(6 * B, img_w=1333., img_h=800., seed=2, min_size=40., max_size=500.).cuda()
    offs = [6 * b for b in range(B + 1)]
    cnt = [(300, n - 300)] * B
    perm, _ = train_ops.draw_sampler_perms(cnt, num, npos, -1)
    total = train_ops.rpn_num_total_samples(cnt, num, npos, -1)
    meta = train_ops.RPNSampledMeta(B, sizes, gen.strides, [t.cuda() for t in gen.base_anchors], A, offs, num, npos, -1,
                                    -1.0, 0.0, (0., 0., 0., 0.), (1., 1., 1., 1.), 1.0, 1.0)
    gi, pd = gt_inds.cuda(), perm.cuda()
    drawn, ws = train_ops.rpn_sampled_draw(gi, pd, meta)
    res = {}
    res['rpn_sampled_draw'] = (device_ms(lambda: train_ops.rpn_sampled_draw(gi, pd, meta)), B * n * 4 * 2)
    with torch.no_grad():
        res['rpn_sampled_loss_forward+finalize'] = (
            device_ms(lambda: train_ops.RPNSampledLossFunction.apply(y.detach(), gi, gts, drawn, ws, meta, total)),
            B * num * (5 * 4 + 4 + 4 + 8))
    loss = train_ops.rpn_sampled_loss(y, gi, gts, drawn, meta, total, workspace=ws)
    gsum = loss.sum()
    res['rpn_sampled_loss_backward'] = (device_ms(lambda: torch.autograd.grad(gsum, y, retain_graph=True)), rows * ys * 4)
    K, C = 1000, 4
    dets = torch.cat([util.rand_boxes(B * K, seed=3), torch.rand(B * K, 1, generator=g)], 1).view(B, K, 5).cuda()
    probs = torch.randn(B * K, C + 1, generator=g).softmax(1).cuda()
    reg = (torch.randn(B * K, 4 * C, generator=g) * 0.5).cuda()
    numk = torch.full((B,), K, dtype=torch.int32).cuda()
    shp = torch.tensor([[800., 1333.]] * B).cuda()
    res['rcnn_decode_plain'] = (
        device_ms(lambda: ops.rcnn_decode_plain(probs, reg, dets, numk, shp, None, C, 0.05, (0., 0., 0., 0.), (.1, .1, .2, .2))),
        B * K * ((C + 1) * 4 + 16 * C + 20 + C * (16 + 4 + 8 + 1)))
    for k, (ms, nbytes) in res.items():
        print(json.dumps(dict(what=k, us=ms * 1e3, bytes=nbytes, hbm_floor_us=nbytes / HBM * 1e6)), flush=True)


if __name__ == '__main__':
    kernels()
    for path in ('configs/faster_rcnn/faster_rcnn_r50_fpn_1x_utdac.py', 'configs/boosting_rcnn/boosting_rcnn_r50_pafpn_1x_utdac.py'):
        train_step(path)
