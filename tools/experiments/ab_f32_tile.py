"""interleaved A/B of the fp32 inference step (batch 8) on ONE box under the persistent-launch hook of the fp32 64 x 64
kernel: python tools/experiments/ab_f32_tile.py [rounds]   (brcnn_conv_set_tile(-5, 0 / 1): plain everywhere / heuristic)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import bench
from brcnn import lib
L = lib.load()
dev = torch.device('cuda', 0)
model, cfg = bench.build_model('boosting_rcnn_r50_pafpn_1x_utdac.py', dev)
model = model.eval()
img, metas = bench.synthetic_batch(8, dev)


def step():
    with torch.no_grad():
        return model(return_loss=False, rescale=True, img=[img], img_metas=[metas])


rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 4
variants = [('plain', 0), ('heuristic', 1)]
for _ in range(5): step()
res = {n: [] for n, _ in variants}
try:
    for rnd in range(rounds):
        for name, mode in variants:
            assert L.brcnn_conv_set_tile(-5, mode) == 0
            for _ in range(3): step()
            torch.cuda.synchronize()
            n0 = L.brcnn_conv_set_tile(-6, 0)
            t0 = time.perf_counter()
            for _ in range(20): step()
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / 20 * 1e3)
            per_step = (L.brcnn_conv_set_tile(-6, 0) - n0) / 20
    lib.handover_status()
finally:
    L.brcnn_conv_set_tile(-5, 1)
for name, v in res.items():
    print(f'{name:12s} ms/step per round: ' + ' '.join(f'{x:6.3f}' for x in v) + f'   mean {sum(v) / len(v):.3f}  spread {max(v) - min(v):.3f}')
print(f'persistent launches per step under the heuristic: {per_step:.0f}')
d = [a - b for a, b in zip(res['plain'], res['heuristic'])]
print('plain - heuristic per round: ' + ' '.join(f'{x:6.3f}' for x in d) + f'   mean {sum(d) / len(d):.3f}')
