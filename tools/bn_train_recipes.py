"""the price of training-mode BatchNorm: the bf16 train step (forward, backward, fused SGD with clipping; batch B x 3x800x1344,
seeded synthetic weights and boxes, the step of bench.py's train leg) of the UTDAC R50 recipe with norm_eval=True (shipped)
and of configs/bn_train (norm_eval=False), run alternately in one process: ROUNDS rounds of STEPS timed steps each after a
warm-up, device time per step from HIP events.  Writes profiles/bn_train_recipes.txt."""
import gc
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import bench  # noqa: E402
import brcnn  # noqa: E402,F401
from brcnn import Config, blocks, build_detector  # noqa: E402
from brcnn.optim import FusedSGD  # noqa: E402
from brcnn.synth import seeded_state_dict  # noqa: E402

B = int(os.environ.get('B', '8'))
ROUNDS, STEPS, WARMUP = int(os.environ.get('ROUNDS', '3')), int(os.environ.get('STEPS', '10')), 3
RECIPES = {'norm_eval=True': 'configs/boosting_rcnn/boosting_rcnn_r50_pafpn_1x_utdac.py',
           'norm_eval=False': 'configs/bn_train/boosting_rcnn_r50_pafpn_1x_utdac_bn_train.py'}


def make_step(path):
    cfg = Config.fromfile(os.path.join(ROOT, path))
    m = build_detector(cfg.model)
    m.load_state_dict(seeded_state_dict(m, seed=0))
    m = m.to('cuda:0').train()
    m.set_compute_dtype('bf16')
    blocks.conv_weights_channels_last(m)
    params = [p for p in m.parameters() if p.requires_grad]
    opt = FusedSGD(params, lr=cfg.optimizer.lr * 1e-3, momentum=cfg.optimizer.momentum, weight_decay=cfg.optimizer.weight_decay)
    opt.register_conv_weights(m, blocks.compute_dtype())
    img, metas = bench.synthetic_batch(B, 'cuda:0', seed=0)
    gtb, gtl = bench.synthetic_gt(B, 'cuda:0', 4, seed=0)
    last = {}

    def step():
        opt.zero_grad(set_to_none=True)
        losses = m(img=img, img_metas=metas, return_loss=True, gt_bboxes=gtb, gt_labels=gtl)
        loss, log_vars = m._parse_losses(losses)
        loss.backward()
        opt.step(max_norm=35)
        last['loss'] = log_vars['loss']
    return step, last


def main():
    assert torch.cuda.is_available(), 'needs the device'
    torch.manual_seed(1234)
    steps = {k: make_step(p) for k, p in RECIPES.items()}
    lines = [f'tools/bn_train_recipes.py: bf16 train step, batch {B} x 3x800x1344, {ROUNDS} alternating rounds of {STEPS} steps '
             f'(device ms per step: median / min / max of the round)']
    med = {k: [] for k in steps}
    gc.collect()
    gc.disable()
    for rnd in range(ROUNDS):
        for k, (step, last) in steps.items():
            for _ in range(WARMUP):
                step()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(STEPS + 1)]
            torch.cuda.synchronize()
            ev[0].record()
            for i in range(STEPS):
                step()
                ev[i + 1].record()
            torch.cuda.synchronize()
            ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(STEPS))
            med[k].append(ms[STEPS // 2])
            lines.append(f'round {rnd}  {k:16s} {ms[STEPS // 2]:8.2f} / {ms[0]:8.2f} / {ms[-1]:8.2f} ms   loss {last["loss"]:.4f}')
            print(lines[-1], flush=True)
    a, b = (sorted(med[k])[ROUNDS // 2] for k in ('norm_eval=True', 'norm_eval=False'))
    lines.append(f'median of the rounds: norm_eval=True {a:.2f} ms, norm_eval=False {b:.2f} ms: training BatchNorm costs '
                 f'{b - a:+.2f} ms per step ({100 * (b - a) / a:+.1f} %)')
    print(lines[-1])
    with open(os.path.join(ROOT, 'profiles', 'bn_train_recipes.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
