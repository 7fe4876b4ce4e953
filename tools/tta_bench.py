"""Times `forward_test` with test-time augmentation on one MI355X: the UTDAC recipe, batch 8, seeded weights, inputs
resident on the device, for A = 1 (plain), 2 (+ horizontal flip) and 4 (two scales x flip) augs.

    python tools/tta_bench.py [--dtype f32|bf16|f16] [--batch 8] [--rounds 10] [--warmup 3] > profiles/tta_bench_f32.txt

Protocol: every variant (the TTA calls, the plain `forward_test` of every single aug, the trunk pass of every aug shape)
is warmed up, then timed once per round with the variants ALTERNATING inside a round, a host clock around a call that
ends synchronised (`forward_test` ends in its device -> host copy; the trunk pass in a stream synchronise); medians over
the rounds, min / max alongside.  Printed per aug count: ms per step, the sum of the A corresponding plain
(`simple_test`) times, their ratio, and the time spent outside the A trunk passes (backbone + neck).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

SCALES = ((800, 1333), (1200, 2000))        # (h, w) of the resized image: img_scale=[(1333, 800), (2000, 1200)]


def aug_batch(batch, scale, flip, device, seed):
    import numpy as np
    import torch
    h, w = SCALES[scale]
    ph, pw = -(-h // 32) * 32, -(-w // 32) * 32
    g = torch.Generator().manual_seed(seed)
    img = torch.zeros(batch, 3, ph, pw)
    img[:, :, :h, :w] = torch.randn(batch, 3, h, w, generator=g)
    if flip:
        img[:, :, :h, :w] = img[:, :, :h, :w].flip(3)
    sf = np.array([w / SCALES[0][1], h / SCALES[0][0]] * 2, dtype=np.float32)
    metas = [dict(img_shape=(h, w, 3), pad_shape=(ph, pw, 3), ori_shape=SCALES[0] + (3,), scale_factor=sf, flip=flip,
                  flip_direction='horizontal' if flip else None) for _ in range(batch)]
    return img.to(device), metas


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', choices=['f32', 'bf16', 'f16'], default='f32')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args(argv)
    import torch
    import brcnn  # noqa: F401
    from brcnn import Config, build_detector
    from brcnn.synth import seeded_state_dict
    if not torch.cuda.is_available():
        raise RuntimeError('tools/tta_bench.py needs a GPU: nothing is measured without one')
    device = torch.device('cuda', 0)
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'boosting_rcnn', 'boosting_rcnn_r50_pafpn_1x_utdac.py'))
    model = build_detector(cfg.model)
    model.load_state_dict(seeded_state_dict(model, seed=0))
    model = model.to(device).eval().freeze_for_inference()
    model.set_compute_dtype(args.dtype)
    # the same source batch at both scales would need a resize; the timing only needs the shapes: one seeded batch per
    # scale, its flip the exact mirror
    augs = [aug_batch(args.batch, s, f, device, seed=s) for s in (0, 1) for f in (False, True)]
    sets = {1: [0], 2: [0, 1], 4: [0, 1, 2, 3]}

    def metas_of(i):
        return [dict(m) for m in augs[i][1]]

    def tta(n):
        def run():
            model(return_loss=False, rescale=True, img=[augs[i][0] for i in sets[n]], img_metas=[metas_of(i) for i in sets[n]])
        return run

    def plain(i):
        def run():
            model(return_loss=False, rescale=True, img=[augs[i][0]], img_metas=[metas_of(i)])
        return run

    def trunk(i):
        def run():
            model.extract_feat_nhwc(augs[i][0])
            torch.cuda.current_stream().synchronize()
        return run

    variants = {f'tta{n}': tta(n) for n in sets}
    variants.update({f'plain{i}': plain(i) for i in range(4)})
    variants.update({f'trunk{i}': trunk(i) for i in (0, 2)})        # (a flip has its scale's shape)
    times = {k: [] for k in variants}
    with torch.no_grad():
        for _ in range(args.warmup):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for k, fn in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                times[k].append(1e3 * (time.perf_counter() - t0))
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f'# tools/tta_bench.py  dtype={args.dtype} batch={args.batch} rounds={args.rounds} warmup={args.warmup}  '
          f'device={torch.cuda.get_device_name(0)}  torch={torch.__version__}')
    print('# ms per call: median [min .. max] over the rounds, variants alternating inside a round')
    for k, v in times.items():
        print(f'{k:8s} {med[k]:9.2f}  [{min(v):9.2f} .. {max(v):9.2f}]')
    print('# augs  tta ms/step  sum of plain  tta / sum   trunk passes  outside the trunk')
    out = {}
    for n, idx in sets.items():
        total = sum(med[f'plain{i}'] for i in idx)
        trunks = sum(med[f'trunk{2 * (i // 2)}'] for i in idx)
        out[n] = dict(tta_ms=med[f'tta{n}'], sum_plain_ms=total, ratio=med[f'tta{n}'] / total, trunk_ms=trunks,
                      outside_trunk_ms=med[f'tta{n}'] - trunks)
        print(f'{n:5d} {med[f"tta{n}"]:12.2f} {total:13.2f} {med[f"tta{n}"] / total:10.4f} {trunks:14.2f} '
              f'{med[f"tta{n}"] - trunks:17.2f}')
    print(json.dumps({'dtype': args.dtype, 'batch': args.batch, 'rounds': args.rounds, 'by_num_augs': out}))
    return out


if __name__ == '__main__':
    main()
