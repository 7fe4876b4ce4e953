"""Generates tests/golden/g28_fcos.npz by importing the reference, on the CPU, under the test-only mmcv shim
(tests/golden/_mmcv_shim.py), the way make_golden_retinanet.py builds g27: seeded weights and inputs (tests/util.py,
tests/fcos_inputs.py), the reference's FCOSHead / FCOS run on them.  The fixture is data (seeds + expected outputs + the list
of the reference model's state-dict keys); no reference source is stored.
Run:  python tests/golden/make_golden_fcos.py

The margins are those of make_golden_faster_rcnn.py (whose helpers are used): no candidate IoU within 1e-4 of the NMS
threshold, no score gap below 1e-6 at a top-k, score_thr or max_per_img boundary, no score ties; end to end, the fp32
reference within 5e-5 of its own float64 run.  The target sections also ask for what the tests lean on: every level has a
positive, some point is claimed by two boxes (the area rule decides), center sampling changes the label map, and under
norm_on_bbox some positive's scaled raw distance is negative (the relu branch).  A section whose inputs miss a condition
moves on to the next seed; the seed it settles on is recorded.
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

from tests import fcos_inputs as fi  # noqa: E402
from tests import util  # noqa: E402

SCORE_MARGIN, REF_MARGIN = F.SCORE_MARGIN, F.REF_MARGIN
need, cfgdict = F.need, F.cfgdict


class Spies:
    """margin checks hooked into the reference's own decision point: multiclass_nms as FCOSHead calls it (the threshold is
    on the class score, the NMS runs on class score x centerness)"""

    def __enter__(self):
        import mmdet.models.dense_heads.fcos_head as FH
        self.saved = [(FH, 'multiclass_nms', FH.multiclass_nms)]
        mc_nms = FH.multiclass_nms

        def mc_spy(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1, score_factors=None, **k):
            s = multi_scores[:, :-1]
            need((s.double() - score_thr).abs().min().item() > SCORE_MARGIN, 'score_thr boundary')
            nc = s.shape[1]
            bb = multi_bboxes.view(len(s), -1, 4).expand(len(s), nc, 4)
            lab = torch.arange(nc).view(1, -1).expand_as(s)
            m = s > score_thr
            if m.any():
                F.check_nms(bb[m], (s * score_factors[:, None])[m], lab[m], nms_cfg['iou_threshold'])
            allk = mc_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, -1, score_factors=score_factors, **k)
            F.check_sorted_gap(allk[0][:, 4], max_num, 'max_per_img')
            return mc_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num, score_factors=score_factors, **k)

        FH.multiclass_nms = mc_spy
        return self

    def __exit__(self, *exc):
        for obj, name, val in self.saved:
            setattr(obj, name, val)


def check_topk(cls_scores, centernesses, num_classes, nms_pre):
    """the per-point maximum of class score x centerness of every (level, image): a gap at rank nms_pre, and no two equal
    maxima among the picks"""
    for lvl, ctr in zip(cls_scores, centernesses):
        for b in range(lvl.shape[0]):
            s = lvl[b].detach().permute(1, 2, 0).reshape(-1, num_classes).sigmoid()
            s = (s * ctr[b].detach().reshape(-1, 1).sigmoid()).max(-1)[0]
            F.check_sorted_gap(s, nms_pre, 'top-k')
            if len(s) > nms_pre:
                top = torch.sort(s.double(), descending=True)[0][:nms_pre + 1]
                need((top[:-1] - top[1:]).min().item() > 0, 'two picked points with the same score')


def build(num_classes, training, **over):
    from mmdet.models import build_head
    head = build_head(cfgdict(fi.head_cfg(num_classes, **over)))
    head.train(training)
    with torch.no_grad():
        for s, v in zip(head.scales, fi.SCALES):
            s.scale.fill_(v)
    return head


def sec_bboxes(num_classes):
    def run(seed, spies):
        """FCOSHead.get_bboxes, head level, with and without rescale, both norm_on_bbox settings (and, for 4 classes, the
        image without a class score above the threshold)"""
        d, metas = {}, fi.metas()
        cases = [('plain', False, False, False), ('rescale', True, False, False), ('norm', True, False, True)] + \
            ([('empty', True, True, False)] if num_classes == 4 else [])
        for name, rescale, empty, norm in cases:
            head = build(num_classes, False, norm_on_bbox=norm)
            cls, raw, ctr = fi.head_outputs(seed, num_classes, norm_on_bbox=norm, empty=empty)
            check_topk(cls, ctr, num_classes, fi.TEST_CFG['nms_pre'])
            res = head.get_bboxes(cls, fi.decoded(raw, fi.SCALES, norm, False), ctr, metas, rescale=rescale)
            for b in range(2):
                d[f'bboxes_c{num_classes}_{name}_det{b}'], d[f'bboxes_c{num_classes}_{name}_lab{b}'] = res[b]
            need(len(res[0][0]) > 0, 'no detections')
            if empty:
                need(len(res[1][0]) == 0, 'the empty case')
        return d
    return run


def sec_targets(seed, spies):
    """FCOSHead.get_targets: labels and box targets per level, without and with center sampling"""
    d = {}
    gt_bboxes, gt_labels = fi.gts(seed)
    maps = {}
    for tag, over in (('plain', dict()), ('center', dict(center_sampling=True, center_sample_radius=fi.RADIUS)),
                      ('norm', dict(norm_on_bbox=True))):
        head = build(4, True, **over)
        points = head.get_points(fi.SIZES, torch.float32, 'cpu')
        labels, targets = head.get_targets(points, gt_bboxes, gt_labels)
        maps[tag] = torch.cat(labels)
        for l in range(len(fi.SIZES)):
            d[f'targets_{tag}_labels{l}'], d[f'targets_{tag}_box{l}'] = labels[l], targets[l]
            need(bool((labels[l] < 4).any()), f'{tag}: level {l} has no positive')
    need(not torch.equal(maps['plain'], maps['center']), 'center sampling leaves the label map unchanged')
    # some point lies strictly inside two boxes whose ranges both admit it: the area rule decides
    pts = torch.cat(points)
    rng = torch.cat([p.new_tensor(r)[None].expand_as(p) for p, r in zip(points, fi.RANGES)])
    two = False
    for g in gt_bboxes:
        t = torch.stack([pts[:, 0:1] - g[:, 0], pts[:, 1:2] - g[:, 1], g[:, 2] - pts[:, 0:1], g[:, 3] - pts[:, 1:2]], -1)
        ok = (t.min(-1)[0] > 0) & (t.max(-1)[0] >= rng[:, 0:1]) & (t.max(-1)[0] <= rng[:, 1:2])
        two = two or bool((ok.sum(1) >= 2).any())
    need(two, 'no point is claimed by two boxes')
    return d


def sec_loss(tag, num_classes, variant, with_grads):
    def run(seed, spies):
        """FCOSHead.loss on the decoded distances of seeded raw outputs, and (with_grads) the autograd gradients of the
        summed loss w.r.t. the class logits, the RAW distances, the centerness logits and the per-level scales"""
        d = {}
        over = fi.VARIANTS[variant]
        norm = bool(over.get('norm_on_bbox', False))
        head = build(num_classes, True, **over)
        cls, raw, ctr = fi.head_outputs(seed, num_classes, norm_on_bbox=norm, grad=True)
        scales = [torch.tensor(v, requires_grad=True) for v in fi.SCALES]
        gt_bboxes, gt_labels = fi.gts(seed, num_classes=num_classes)
        losses = head.loss(cls, fi.decoded(raw, scales, norm, True), ctr, gt_bboxes, gt_labels, fi.metas())
        for k, v in losses.items():
            d[f'{tag}_{k}'] = v
        need(float(losses['loss_bbox']) > 0, 'no positive point')
        points = head.get_points(fi.SIZES, torch.float32, 'cpu')
        labels, _ = head.get_targets(points, gt_bboxes, gt_labels)
        need(all(bool((l < num_classes).any()) for l in labels), 'a level without a positive')
        if norm:
            neg = False
            for l, lab in enumerate(labels):
                r = raw[l].detach().permute(0, 2, 3, 1).reshape(-1, 4) * fi.SCALES[l]
                neg = neg or bool((r[lab < num_classes] < 0).any())
            need(neg, 'no positive with a negative scaled raw distance')
        if with_grads:
            sum(losses.values()).backward()
            for l in range(len(fi.SIZES)):
                d[f'{tag}_dcls{l}'], d[f'{tag}_dreg{l}'], d[f'{tag}_dctr{l}'] = cls[l].grad, raw[l].grad, ctr[l].grad
            d[f'{tag}_dscale'] = torch.stack([s.grad for s in scales])
        return d
    return run


def float64_run(m, img):
    """the same detector and input in float64: what the fp32 reference run is an approximation OF"""
    m64 = copy.deepcopy(m).double()
    return m64.simple_test(img.double(), fi.metas(), rescale=True)


def sec_model(seed, spies):
    """the detector end to end: simple_test of the seeded model on the seeded demo batch"""
    from mmdet.models import build_detector
    d = {}
    mc = fi.fixture_model_cfg()
    m = build_detector(cfgdict(copy.deepcopy(mc)))
    m.load_state_dict(fi.fixture_state_dict(m, seed))
    img, _, _, _ = util.demo_inputs(2, fi.H, fi.W, seed=seed)
    m.eval()
    sd = m.state_dict()
    d['state_keys'] = np.array(list(sd.keys()))
    d['state_shapes'] = np.array([json.dumps(list(v.shape)) for v in sd.values()])
    with torch.no_grad():
        outs = m.bbox_head(m.extract_feat(img))
        check_topk(outs[0], outs[2], 4, mc['test_cfg']['nms_pre'])
        res = m.simple_test(img, fi.metas(), rescale=True)
        res64 = float64_run(m, img)
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
        m = build_detector(cfgdict(copy.deepcopy(fi.fixture_model_cfg())))
        m.load_state_dict(fi.fixture_state_dict(m, weight_seed()))
        m.train()
        img, _, _, _ = util.demo_inputs(2, fi.H, fi.W, seed=seed, num_gt=fi.TRAIN_NUM_GT)
        tg, tl = fi.gts(seed)
        losses = m.forward_train(img, fi.metas(), tg, tl)
        return {f'train{it}_{k}': v for k, v in losses.items()}
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
    for c in fi.CLASS_COUNTS:
        settle(f'bboxes_c{c}', sec_bboxes(c), 28, out)
    settle('targets', sec_targets, 28, out)
    for variant in fi.VARIANTS:
        settle(f'loss_{variant}_c4', sec_loss(f'loss_{variant}_c4', 4, variant, True), 28, out)
        settle(f'loss_{variant}_c1', sec_loss(f'loss_{variant}_c1', 1, variant, False), 28, out)
    settle('e2e', sec_model, 28, out)
    for it in range(2):
        settle(f'train{it}', sec_train(it, lambda: out['seed_e2e']), 1000 * (it + 1), out)
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, 'g28_fcos.npz')
    np.savez_compressed(path, **out)
    print(f'g28_fcos.npz  {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
