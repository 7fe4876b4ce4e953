"""Times the training front door of the multi-scale recipes, per image and per AutoAugment policy, on one MI355X.

    python tools/train_front_door_bench.py [--reps 20] [--warmup 3] [--commit HASH] [--out profiles/train_front_door_bench.txt]

Sources: synthetic 480 x 640 and 1080 x 1920 uint8 frames with 8 boxes.  Pipeline: the shipped
`boosting_rcnn_r50_pafpn_mstrain_2x_coco` train pipeline from RandomFlip to DefaultFormatBundle, with AutoAugment
holding ONE of its two policies at a time (`resize`: one of 11 short sides; `crop`: resize, random crop, resize).
(host)  `Compose(pipeline)` on one core -- the numpy restatement of OpenCV's resize, flip, normalize, pad, the CHW copy --
        plus the upload of the fp32 tensor; the part before the upload is also given alone, as images / s per core
(fused) `Compose(fuse_device_pipeline(pipeline, policies=True))`: host planning, the upload of the uint8 source and one
        `brcnn_preprocess_u8_chain` launch
Both ends synchronised, host clock, median [min .. max] over --reps samples drawn under the same seeds; the two ways are
compared bit for bit on every sample first.  Every (source, policy) measurement runs in a child process of its own under
a time limit; the first one that fails ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SOURCES = {'480x640': (480, 640), '1080x1920': (1080, 1920)}
POLICIES = {'resize': 0, 'crop': 1}
STEP_TIMEOUT = 240          # seconds per child: ~25 host chains of <= 0.5 s each, the import and the device start-up


def measure(source, policy, reps, warmup):
    """one (source, policy) pair; prints one JSON line"""
    import numpy as np
    import torch
    import brcnn  # noqa: F401
    from brcnn import Config
    from brcnn import pipelines as P
    if not torch.cuda.is_available():
        raise RuntimeError('tools/train_front_door_bench.py needs a GPU: nothing is measured without one')
    torch.set_num_threads(1)
    device = 'cuda:0'
    cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'boosting_rcnn', 'boosting_rcnn_r50_pafpn_mstrain_2x_coco.py'))
    pipe = [dict(c) for c in cfg.data.train.dataset.pipeline]
    types = [c['type'] for c in pipe]
    pipe = pipe[types.index('RandomFlip'):types.index('DefaultFormatBundle') + 1]
    aug = [c for c in pipe if c['type'] == 'AutoAugment'][0]
    aug['policies'] = [aug['policies'][POLICIES[policy]]]
    host, fused = P.Compose(pipe), P.Compose(P.fuse_device_pipeline(pipe, device, policies=True))
    assert isinstance(fused.transforms[0], P.FusedAugResizeNormalizePad)
    h, w = SOURCES[source]
    rng = np.random.RandomState(0)
    img = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
    x, y = np.sort(rng.uniform(0, w, (8, 2)), axis=1), np.sort(rng.uniform(0, h, (8, 2)), axis=1)
    boxes = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(np.float32)

    def fresh():
        return dict(img=img, img_shape=img.shape, ori_shape=img.shape, img_fields=['img'], filename=None,
                    ori_filename=None, gt_bboxes=boxes.copy(), gt_labels=np.zeros(8, np.int64), bbox_fields=['gt_bboxes'])

    def host_way(seed):
        np.random.seed(seed)
        t0 = time.perf_counter()
        r = host(fresh())
        t1 = time.perf_counter()
        t = r['img'].data.to(device)
        torch.cuda.synchronize()
        return t, 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t0)

    def fused_way(seed):
        np.random.seed(seed)
        t0 = time.perf_counter()
        t = fused(fresh())['img'].data
        torch.cuda.synchronize()
        return t, 1e3 * (time.perf_counter() - t0)
    cpu, whole, dev = [], [], []
    for s in range(warmup + reps):
        a, t_cpu, t_whole = host_way(s)
        b, t_dev = fused_way(s)
        assert a.shape == b.shape and torch.equal(a, b), f'the two ways disagree under seed {s}'
        if s >= warmup:
            cpu.append(t_cpu)
            whole.append(t_whole)
            dev.append(t_dev)
    stat = lambda v: [statistics.median(v), min(v), max(v)]                      # noqa: E731
    print(json.dumps(dict(source=source, policy=policy, host_cpu_ms=stat(cpu), host_ms=stat(whole), fused_ms=stat(dev),
                          device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--commit', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--one', nargs=2, metavar=('SOURCE', 'POLICY'), help='measure one pair in this process')
    args = ap.parse_args(argv)
    if args.one:
        return measure(args.one[0], args.one[1], args.reps, args.warmup)
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.run(['git', 'rev-parse', '--short', 'HEAD'], cwd=ROOT, capture_output=True, text=True,
                                    check=True).stdout.strip()
        except Exception:
            commit = 'unknown'
    rows = []
    for source in SOURCES:
        for policy in POLICIES:
            cmd = [sys.executable, os.path.abspath(__file__), '--one', source, policy, '--reps', str(args.reps),
                   '--warmup', str(args.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT)
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f'{source} / {policy}: exit status {r.returncode}; nothing further is run')
            rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(rows[-1], flush=True)
    lines = [f'# tools/train_front_door_bench.py  commit={commit}  reps={args.reps} warmup={args.warmup}  '
             f'device={rows[0]["device"]}  torch={rows[0]["torch"]}',
             '# ms per image, median [min .. max]; host = Compose(RandomFlip .. DefaultFormatBundle) on one core + fp32 upload,',
             '# fused = plan + uint8 upload + one brcnn_preprocess_u8_chain launch; outputs compared bit for bit on every sample',
             '']
    fmt = lambda v: f'{v[0]:9.3f} [{v[1]:9.3f} .. {v[2]:9.3f}]'                  # noqa: E731
    for r in rows:
        lines += [f'## {r["source"]} source, policy `{r["policy"]}`',
                  f'    host chain alone (one core)   {fmt(r["host_cpu_ms"])}   = {1e3 / r["host_cpu_ms"][0]:7.1f} img/s per core',
                  f'    host chain + fp32 upload      {fmt(r["host_ms"])}',
                  f'    fused transform               {fmt(r["fused_ms"])}   = {1e3 / r["fused_ms"][0]:7.1f} img/s per process',
                  f'    host / fused                  {r["host_ms"][0] / r["fused_ms"][0]:9.1f} x', '']
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')
    return rows


if __name__ == '__main__':
    main()
