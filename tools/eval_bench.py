"""Times COCO bbox evaluation, host against device, on seeded synthetic sets shaped like a detector's output (100
detections per image, about 7 ground truths per image, 5 % crowds): 5 000 images x 80 categories and 1 300 x 4.

    python tools/eval_bench.py [--sets 5000x80,1300x4] [--reps 3] [--out profiles/eval_bench.txt]

host    `_det2json + loadRes + COCOeval.evaluate + accumulate` (evaluation.COCOeval, host clock)
cold    DeviceCOCOeval with nothing cached: ground-truth packing and upload, detection packing, upload, the kernels, the
        copy back (host clock, ends synchronised)
warm    the same with the ground-truth table cached, as the eval hook's second epoch sees it (median of --reps)
kernels HIP event pairs around the upload and each of the three stages (from the last warm run)
and whether precision / recall / scores / stats were bit-equal.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def synthetic(n_img, n_cat, seed=0, dets=100, gts=7):
    from brcnn.datasets import COCO
    rng = np.random.RandomState(seed)
    img_ids, cat_ids = list(range(1, n_img + 1)), list(range(1, n_cat + 1))
    anns, results = [], []
    for img in img_ids:
        g = max(1, rng.poisson(gts))
        wh = np.exp(rng.uniform(np.log(8), np.log(300), (g, 2)))
        xy = rng.uniform(0, 500, (g, 2))
        lab = rng.randint(0, n_cat, g)
        crowd = rng.rand(g) < 0.05
        for j in range(g):
            anns.append(dict(id=len(anns) + 1, image_id=img, category_id=cat_ids[lab[j]], iscrowd=int(crowd[j]),
                             bbox=[float(xy[j, 0]), float(xy[j, 1]), float(wh[j, 0]), float(wh[j, 1])],
                             area=float(wh[j, 0] * wh[j, 1])))
        src = rng.randint(0, g, dets)
        near = rng.rand(dets) < 0.6
        bx = np.where(near[:, None], xy[src] + rng.normal(0, 0.1, (dets, 2)) * wh[src], rng.uniform(0, 500, (dets, 2)))
        bw = np.where(near[:, None], wh[src] * np.exp(rng.normal(0, 0.1, (dets, 2))), np.exp(rng.uniform(np.log(8), np.log(300), (dets, 2))))
        bl = np.where(near & (rng.rand(dets) < 0.8), lab[src], rng.randint(0, n_cat, dets))
        rows = np.concatenate([bx, bx + bw, rng.beta(1.2, 2.0, (dets, 1)).round(2)], 1).astype(np.float32)
        none = np.zeros((0, 5), np.float32)
        per = [none] * n_cat
        for c in np.unique(bl):
            per[c] = rows[bl == c]
        results.append(per)
    gt = COCO()
    gt.dataset = dict(images=[dict(id=i, width=800, height=800, file_name=f'{i}.jpg') for i in img_ids],
                      categories=[dict(id=c, name=f'c{c}') for c in cat_ids], annotations=anns)
    gt.createIndex()
    return gt, results, img_ids, cat_ids


class _Shim:
    """`_det2json` of CocoDataset on the synthetic lists"""
    def __init__(self, img_ids, cat_ids):
        self.img_ids, self.cat_ids = img_ids, cat_ids

    def __len__(self):
        return len(self.img_ids)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sets', default='5000x80,1300x4')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import brcnn  # noqa: F401
    from brcnn.datasets import CocoDataset
    from brcnn.evaluation import COCOeval, DeviceCOCOeval
    lines = [f'# tools/eval_bench.py on {torch.cuda.get_device_name(0)}; maxDets (1, 10, 100), 10 IoU thresholds, 4 area ranges']
    torch.zeros(1, device='cuda')
    for spec in args.sets.split(','):
        n_img, n_cat = (int(v) for v in spec.split('x'))
        gt, results, img_ids, cat_ids = synthetic(n_img, n_cat)
        n_det = sum(len(b) for r in results for b in r)
        shim = _Shim(img_ids, cat_ids)
        shim.xyxy2xywh = CocoDataset.xyxy2xywh
        t0 = time.perf_counter()
        dets = CocoDataset._det2json(shim, results)
        t1 = time.perf_counter()
        host = COCOeval(gt, gt.loadRes(dets), 'bbox')
        host.params.imgIds, host.params.catIds = img_ids, cat_ids
        host.evaluate()
        host.accumulate()
        t2 = time.perf_counter()
        host.summarize()

        def device(profile=False):
            torch.cuda.synchronize()
            a = time.perf_counter()
            ev = DeviceCOCOeval(gt, results, img_ids=img_ids, cat_ids=cat_ids, profile=profile)
            ev.params.imgIds, ev.params.catIds = img_ids, cat_ids
            ev.evaluate()
            ev.accumulate()
            b = time.perf_counter()
            ev.summarize()
            return b - a, ev
        cold, ev = device()
        warm = [device()[0] for _ in range(args.reps)]
        _, ev = device(profile=True)
        equal = all(np.array_equal(host.eval[k], ev.eval[k]) for k in ('precision', 'recall', 'scores')) and \
            np.array_equal(host.stats, ev.stats)
        lines += [f'{n_img} images x {n_cat} categories, {n_det} detections, {len(gt.dataset["annotations"])} ground truths: mAP {host.stats[0]:.4f}',
                  f'  host    {t2 - t0:8.3f} s   (_det2json {t1 - t0:.3f} s, loadRes + evaluate + accumulate {t2 - t1:.3f} s)',
                  f'  cold    {cold:8.3f} s   (ground-truth table built and uploaded)',
                  f'  warm    {statistics.median(warm):8.3f} s   (median of {args.reps}; min {min(warm):.3f}, max {max(warm):.3f})',
                  '  kernels ' + ', '.join(f'{k} {v:.3f} ms' for k, v in ev.kernel_ms.items()),
                  f'  bit-equal to the host evaluator: {equal}   host / warm = {(t2 - t0) / statistics.median(warm):.1f}x']
        print('\n'.join(lines[-6:]), flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
