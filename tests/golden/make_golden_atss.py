"""Generates tests/golden/g29_atss.npz by importing the reference, on the CPU, under the test-only mmcv shim
(tests/golden/_mmcv_shim.py), the way make_golden_fcos.py builds g28: seeded weights and inputs (tests/util.py,
tests/atss_inputs.py), the reference's ATSSAssigner / ATSSHead / ATSS run on them.  The fixture is data (seeds + expected
outputs + the list of the reference model's state-dict keys); no reference source is stored.
Run:  python tests/golden/make_golden_atss.py

The margins are those of make_golden_fcos.py (whose helpers are used): no candidate IoU within 1e-4 of the NMS threshold,
no score gap below 1e-6 at a top-k, score_thr or max_per_img boundary, no score ties; end to end, the fp32 reference within
5e-5 of its own float64 run.  The assignment sections also ask for what the tests lean on, so that the reference's
unspecified choices (torch.topk among equal distances) and rounding edges play no part: positives on at least 3 levels, a
candidate that passes the IoU threshold but fails the centre test, an anchor claimed by two ground truths, no (ground
truth, level) with equal distances at ranks k and k + 1, every candidate's |iou - thr| > 1e-5 and |min side - 0.01| > 1e-3,
no equal IoUs among the claimants of an anchor.  A section whose inputs miss a condition moves on to the next seed; the
seed it settles on is recorded.
"""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_faster_rcnn as F  # noqa: E402  (installs the shim, puts the repository root on the path)
import make_golden_fcos as GF  # noqa: E402

from tests import atss_inputs as ai  # noqa: E402
from tests import atss_ref64 as R  # noqa: E402
from tests import util  # noqa: E402

REF_MARGIN = F.REF_MARGIN
need, cfgdict = F.need, F.cfgdict
check_topk = GF.check_topk


class Spies(GF.Spies):
    """make_golden_fcos.Spies on the ATSS head's multiclass_nms (the same call: threshold on the class score, NMS on class
    score x centerness)"""

    def __enter__(self):
        import mmdet.models.dense_heads.atss_head as AH
        import mmdet.models.dense_heads.fcos_head as FH
        super().__enter__()                                 # FH.multiclass_nms is now the spy
        self.saved.append((AH, 'multiclass_nms', AH.multiclass_nms))
        AH.multiclass_nms = FH.multiclass_nms
        return self


def build(num_classes, training, **over):
    from mmdet.models import build_head
    head = build_head(cfgdict(ai.head_cfg(num_classes, **over)))
    head.train(training)
    with torch.no_grad():
        for s, v in zip(head.scales, ai.SCALES):
            s.scale.fill_(v)
    return head


def check_assignment(gt_bboxes, tag):
    """the conditions of the module docstring, evaluated on the float32 restatement of the assignment"""
    _, info = R.assign(gt_bboxes, ai.SIZES, ai.STRIDES, ai.OCTAVE, ai.TOPK, dtype=torch.float32, details=True)
    inds = R.assign(gt_bboxes, ai.SIZES, ai.STRIDES, ai.OCTAVE, ai.TOPK, dtype=torch.float32)
    starts = np.cumsum([0] + [h * w for h, w in ai.SIZES])
    rejected = two = 0
    for b, d in enumerate(info):
        levels = sum(bool((inds[b][starts[l]:starts[l + 1]] > 0).any()) for l in range(len(ai.SIZES)))
        need(levels >= 3, f'{tag}: image {b} has positives on {levels} levels')
        need(float(d['gaps'].min()) > 0, f'{tag}: equal distances at ranks k and k + 1')
        need(float((d['iou'] - d['thr'][None]).abs().min()) > 1e-5, f'{tag}: a candidate IoU within 1e-5 of its threshold')
        need(float((d['side'] - 0.01).abs().min()) > 1e-3, f'{tag}: a candidate side within 1e-3 of 0.01')
        rejected += int(((d['iou'] >= d['thr'][None]) & ~(d['side'] > 0.01)).sum())
        claims = torch.isfinite(d['claimed'])
        multi = claims.sum(1) >= 2
        two += int(multi.sum())
        for row in d['claimed'][multi]:
            v = row[torch.isfinite(row)]
            need(len(torch.unique(v)) == len(v), f'{tag}: equal IoUs among the claimants of an anchor')
    need(rejected > 0, f'{tag}: no candidate is rejected by the centre test')
    need(two > 0, f'{tag}: no anchor is claimed by two ground truths')


def sec_assign(seed, spies):
    """ATSSAssigner.assign on the head-level anchors, per image: gt_inds and max_overlaps"""
    d = {}
    head = build(4, True)
    gt_bboxes, gt_labels = ai.gts(seed)
    check_assignment(gt_bboxes, 'assign')
    anchors = head.anchor_generator.grid_anchors(ai.SIZES, 'cpu')
    for b in range(2):
        res = head.assigner.assign(torch.cat(anchors), [len(a) for a in anchors], gt_bboxes[b], None, gt_labels[b])
        d[f'assign_gt_inds{b}'], d[f'assign_max_overlaps{b}'], d[f'assign_labels{b}'] = res.gt_inds, res.max_overlaps, res.labels
    return d


def sec_targets(seed, spies):
    """ATSSHead.get_targets: labels, label weights and encoded box targets per level"""
    d = {}
    head = build(4, True)
    gt_bboxes, gt_labels = ai.gts(seed)
    check_assignment(gt_bboxes, 'targets')
    anchor_list, valid_flag_list = head.get_anchors(ai.SIZES, ai.metas(), device='cpu')
    out = head.get_targets(anchor_list, valid_flag_list, gt_bboxes, ai.metas(), gt_labels_list=gt_labels, label_channels=4)
    _, labels, label_weights, bbox_targets, _, num_pos, num_neg = out
    for l in range(len(ai.SIZES)):
        d[f'targets_labels{l}'], d[f'targets_weights{l}'], d[f'targets_box{l}'] = labels[l], label_weights[l], bbox_targets[l]
    d['targets_num'] = np.array([num_pos, num_neg])
    return d


def sec_loss(tag, num_classes, with_grads):
    def run(seed, spies):
        """ATSSHead.loss on the scaled deltas of seeded raw outputs, and (with_grads) the autograd gradients of the summed
        loss w.r.t. the class logits, the RAW deltas, the centerness logits and the per-level scales"""
        d = {}
        head = build(num_classes, True)
        cls, raw, ctr = ai.head_outputs(seed, num_classes, grad=True)
        scales = [torch.tensor(v, requires_grad=True) for v in ai.SCALES]
        gt_bboxes, gt_labels = ai.gts(seed, num_classes=num_classes)
        check_assignment(gt_bboxes, tag)
        losses = head.loss(cls, ai.scaled(raw, scales), ctr, gt_bboxes, gt_labels, ai.metas())
        for k, v in losses.items():
            d[f'{tag}_{k}'] = torch.stack([torch.as_tensor(x) for x in v])
        need(float(d[f'{tag}_loss_bbox'].sum()) > 0, 'no positive anchor')
        if with_grads:
            sum(sum(v) for v in losses.values()).backward()
            for l in range(len(ai.SIZES)):
                d[f'{tag}_dcls{l}'], d[f'{tag}_dreg{l}'], d[f'{tag}_dctr{l}'] = cls[l].grad, raw[l].grad, ctr[l].grad
            d[f'{tag}_dscale'] = torch.stack([s.grad for s in scales])
        return d
    return run


def sec_bboxes(num_classes):
    def run(seed, spies):
        """ATSSHead.get_bboxes, head level, with and without rescale (and, for 4 classes, the image without a class score
        above the threshold)"""
        d, metas = {}, ai.metas()
        cases = [('plain', False, False), ('rescale', True, False)] + ([('empty', True, True)] if num_classes == 4 else [])
        for name, rescale, empty in cases:
            head = build(num_classes, False)
            cls, raw, ctr = ai.head_outputs(seed, num_classes, empty=empty)
            check_topk(cls, ctr, num_classes, ai.TEST_CFG['nms_pre'])
            res = head.get_bboxes(cls, ai.scaled(raw, ai.SCALES), ctr, metas, rescale=rescale)
            for b in range(2):
                d[f'bboxes_c{num_classes}_{name}_det{b}'], d[f'bboxes_c{num_classes}_{name}_lab{b}'] = res[b]
            need(len(res[0][0]) > 0, 'no detections')
            if empty:
                need(len(res[1][0]) == 0, 'the empty case')
        return d
    return run


def sec_model(seed, spies):
    """the detector end to end: simple_test of the seeded model on the seeded demo batch"""
    from mmdet.models import build_detector
    d = {}
    mc = ai.fixture_model_cfg()
    m = build_detector(cfgdict(copy.deepcopy(mc)))
    m.load_state_dict(ai.fixture_state_dict(m, seed))
    img, _, _, _ = util.demo_inputs(2, ai.H, ai.W, seed=seed)
    m.eval()
    sd = m.state_dict()
    d['state_keys'] = np.array(list(sd.keys()))
    d['state_shapes'] = np.array([json.dumps(list(v.shape)) for v in sd.values()])
    with torch.no_grad():
        outs = m.bbox_head(m.extract_feat(img))
        check_topk(outs[0], outs[2], 4, mc['test_cfg']['nms_pre'])
        res = m.simple_test(img, ai.metas(), rescale=True)
        res64 = copy.deepcopy(m).double().simple_test(img.double(), ai.metas(), rescale=True)
    worst = 0.0
    for b in range(2):
        d[f'e2e_res{b}'] = F.dets_table(res[b])
        t64 = F.dets_table(res64[b])
        need(t64.shape == d[f'e2e_res{b}'].shape and np.array_equal(t64[:, 5], d[f'e2e_res{b}'][:, 5]),
             'e2e: the float64 run keeps other detections')
        if len(t64):
            worst = max(worst, float(np.abs(t64[:, :5] - d[f'e2e_res{b}'][:, :5].astype(np.float64)).max()))
    need(worst <= REF_MARGIN, f'e2e: the fp32 reference is {worst:.2e} from its float64 run')
    d['e2e_ref_err'] = worst
    need(all(len(d[f'e2e_res{b}']) > 0 for b in range(2)), 'e2e: an image without detections')
    return d


def sec_train(it, weight_seed):
    def run(seed, spies):
        """one train iteration of the recipe (the e2e section's weights, fresh inputs)"""
        from mmdet.models import build_detector
        m = build_detector(cfgdict(copy.deepcopy(ai.fixture_model_cfg())))
        m.load_state_dict(ai.fixture_state_dict(m, weight_seed()))
        m.train()
        img, _, _, _ = util.demo_inputs(2, ai.H, ai.W, seed=seed, num_gt=ai.TRAIN_NUM_GT)
        tg, tl = ai.gts(seed)
        losses = m.forward_train(img, ai.metas(), tg, tl)
        return {f'train{it}_{k}': torch.stack([torch.as_tensor(x) for x in v]) for k, v in losses.items()}
    return run


def settle(name, fn, first, out):
    """run section `fn` at the first seed from `first` on whose inputs meet the margins; the seed goes into the fixture"""
    for seed in range(first, first + 400):
        try:
            with Spies() as spies:
                d = fn(seed, spies)
        except F.Margin as e:
            print(f'{name}: seed {seed}: {e}; trying the next')
            continue
        out.update(d)
        out[f'seed_{name}'] = seed
        print(f'{name}: seed {seed}')
        return seed
    raise SystemExit(f'{name}: no seed met the margins')


def main():
    out = {}
    settle('assign', sec_assign, 0, out)
    settle('targets', sec_targets, 0, out)
    settle('loss_c4', sec_loss('loss_c4', 4, True), 0, out)
    settle('loss_c1', sec_loss('loss_c1', 1, False), 0, out)
    for c in ai.CLASS_COUNTS:
        settle(f'bboxes_c{c}', sec_bboxes(c), 29, out)
    settle('e2e', sec_model, 29, out)
    for it in range(2):
        settle(f'train{it}', sec_train(it, lambda: out['seed_e2e']), 1000 * (it + 1), out)
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, 'g29_atss.npz')
    np.savez_compressed(path, **out)
    print(f'g29_atss.npz  {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
