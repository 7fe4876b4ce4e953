#!/usr/bin/env python
"""Run a trained detector on images (the `demo/image_demo.py` use of the reference's `init_detector` +
`inference_detector`, without the visualisation).

    python tools/infer.py CONFIG CHECKPOINT IMAGE_OR_DIR... [--dtype bf16] [--batch-size 8] [--score-thr 0.3] [--out results.json]

Images are streamed through `inference_stream` (batched uint8 front door on a side stream); the detections are written
COCO-style: [{"file", "bbox": [x, y, w, h], "score", "category"}].
"""
import argparse
import json
import os
os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')     # before the HIP runtime starts (see brcnn/__init__.py)
import os.path as osp
import sys

sys.path.insert(0, osp.dirname(osp.dirname(osp.abspath(__file__))))
import torch  # noqa: E402

import brcnn  # noqa: E402,F401
from brcnn.apis import inference_stream, init_detector, limit_host_threads  # noqa: E402
from brcnn.config import DictAction  # noqa: E402

EXTENSIONS = ('.jpg', '.jpeg', '.png', '.bmp', '.npy')


def parse_args(argv=None):
    p = argparse.ArgumentParser(description='detect objects in images')
    p.add_argument('config')
    p.add_argument('checkpoint')
    p.add_argument('inputs', nargs='+', help='image files or directories')
    p.add_argument('--device', default='cuda:0')
    p.add_argument('--dtype', choices=['f32', 'bf16', 'f16'], default='f32', help='arithmetic type of the conv stack')
    p.add_argument('--batch-size', type=int, default=8)
    p.add_argument('--score-thr', type=float, default=0.3)
    p.add_argument('--out', help='output json file (default: print a summary only)')
    p.add_argument('--cfg-options', nargs='+', action=DictAction)
    return p.parse_args(argv)


def collect_files(inputs):
    files = []
    for path in inputs:
        if osp.isdir(path):
            files += [osp.join(path, f) for f in sorted(os.listdir(path)) if f.lower().endswith(EXTENSIONS)]
        else:
            files.append(path)
    return files


def to_records(filename, result, classes, score_thr):
    out = []
    for c, dets in enumerate(result):
        for x1, y1, x2, y2, s in dets.tolist():
            if s >= score_thr:
                out.append(dict(file=filename, bbox=[x1, y1, x2 - x1, y2 - y1], score=s,
                                category=classes[c] if classes is not None else c))
    return out


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError('tools/infer.py needs a GPU: the hot path has no CPU fallback')
    limit_host_threads()
    files = collect_files(args.inputs)
    if not files:
        raise FileNotFoundError(f'no image among {args.inputs}')
    model = init_detector(args.config, args.checkpoint, device=args.device, cfg_options=args.cfg_options, dtype=args.dtype)
    classes = getattr(model, 'CLASSES', None)
    records = []
    for f, result in zip(files, inference_stream(model, files, batch_size=args.batch_size)):
        records += to_records(f, result, classes, args.score_thr)
    print(f'{len(files)} images, {len(records)} detections with score >= {args.score_thr} ({model.last_path} front door)')
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(records, fh)
    return records


if __name__ == '__main__':
    main()
