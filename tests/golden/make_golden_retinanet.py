"""Generates tests/golden/g27_retinanet.npz by importing the reference, on the CPU, under the
test-only mmcv shim (tests/golden/_mmcv_shim.py), the way make_golden_faster_rcnn.py builds g25: seeded weights and inputs
(tests/util.py, tests/retinanet_inputs.py), the reference's RetinaHead / RetinaNet run on them.  The fixture is data (seeds
+ expected outputs + the list of the reference model's state-dict keys); no reference source is stored.
Run:  python tests/golden/make_golden_retinanet.py

The margins are those of make_golden_faster_rcnn.py (whose helpers are used): no candidate IoU within 1e-4 of the NMS or
an assignment threshold, no score gap below 1e-6 at a top-k, score_thr or max_per_img boundary, no score ties; end to
end, the fp32 reference within 5e-5 of its own float64 run.  A section whose inputs miss a margin moves on to the next
seed; the seed it settles on is recorded.
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

from tests import retinanet_inputs as ri  # noqa: E402
from tests import util  # noqa: E402

IOU_MARGIN, SCORE_MARGIN, REF_MARGIN = F.IOU_MARGIN, F.SCORE_MARGIN, F.REF_MARGIN
need, cfgdict = F.need, F.cfgdict


class Spies:
    """margin checks hooked into the reference's own decision points: multiclass_nms as AnchorHead calls it, and the
    assigner's thresholds"""

    def __enter__(self):
        import mmdet.core.bbox.assigners.max_iou_assigner as MA
        import mmdet.models.dense_heads.anchor_head as AH
        self.saved = [(AH, 'multiclass_nms', AH.multiclass_nms),
                      (MA.MaxIoUAssigner, 'assign_wrt_overlaps', MA.MaxIoUAssigner.assign_wrt_overlaps)]
        mc_nms, wrt = AH.multiclass_nms, MA.MaxIoUAssigner.assign_wrt_overlaps

        def mc_spy(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1, *a, **k):
            s = multi_scores[:, :-1]
            need((s.double() - score_thr).abs().min().item() > SCORE_MARGIN, 'score_thr boundary')
            nc = s.shape[1]
            bb = multi_bboxes.view(len(s), -1, 4).expand(len(s), nc, 4)
            lab = torch.arange(nc).view(1, -1).expand_as(s)
            m = s > score_thr
            if m.any():
                F.check_nms(bb[m], s[m], lab[m], nms_cfg['iou_threshold'])
            allk = mc_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, -1, *a, **k)
            F.check_sorted_gap(allk[0][:, 4], max_num, 'max_per_img')
            return mc_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num, *a, **k)

        def wrt_spy(self_, overlaps, gt_labels=None):
            if overlaps.numel():
                for t in (self_.pos_iou_thr, self_.neg_iou_thr, self_.min_pos_iou):
                    if t > 0:
                        need((overlaps.double() - t).abs().min().item() > IOU_MARGIN,
                             f'assignment IoU within {IOU_MARGIN} of {t}')
            return wrt(self_, overlaps, gt_labels)

        AH.multiclass_nms, MA.MaxIoUAssigner.assign_wrt_overlaps = mc_spy, wrt_spy
        return self

    def __exit__(self, *exc):
        for obj, name, val in self.saved:
            setattr(obj, name, val)


def check_topk(cls_scores, num_classes, nms_pre):
    """the per-anchor maximum class score of every (level, image): a gap at rank nms_pre, and no two equal maxima (the
    order of the picks is the order of the candidates)"""
    for lvl in cls_scores:
        for b in range(lvl.shape[0]):
            s = lvl[b].detach().permute(1, 2, 0).reshape(-1, num_classes).sigmoid().max(-1)[0]
            F.check_sorted_gap(s, nms_pre, 'top-k')
            if len(s) > nms_pre:
                top = torch.sort(s.double(), descending=True)[0][:nms_pre + 1]
                need((top[:-1] - top[1:]).min().item() > 0, 'two picked anchors with the same score')


def sec_bboxes(num_classes):
    def run(seed, spies):
        """RetinaHead.get_bboxes, head level, with and without rescale (and, for 4 classes, the image without a score
        above the threshold)"""
        from mmdet.models import build_head
        d, metas = {}, ri.metas()
        head = build_head(cfgdict(ri.head_cfg(num_classes)))
        head.eval()
        cases = [('plain', False, False), ('rescale', True, False)] + ([('empty', True, True)] if num_classes == 4 else [])
        for name, rescale, empty in cases:
            cls, reg = ri.head_outputs(seed, num_classes, empty=empty)
            check_topk(cls, num_classes, ri.TEST_CFG['nms_pre'])
            res = head.get_bboxes(cls, reg, metas, rescale=rescale)
            for b in range(2):
                d[f'bboxes_c{num_classes}_{name}_det{b}'], d[f'bboxes_c{num_classes}_{name}_lab{b}'] = res[b]
            need(len(res[0][0]) > 0, 'no detections')
            if empty:
                need(len(res[1][0]) == 0, 'the empty case')
        return d
    return run


def sec_loss(tag, num_classes, loss_bbox, with_grads):
    def run(seed, spies):
        """RetinaHead.loss with its per-level terms and (with_grads) the autograd gradients of the summed loss"""
        from mmdet.models import build_head
        d = {}
        head = build_head(cfgdict(ri.head_cfg(num_classes, loss_bbox=loss_bbox)))
        head.train()
        cls, reg = ri.head_outputs(seed, num_classes, grad=True)
        gt_bboxes, gt_labels = ri.gts(seed, num_classes=num_classes)
        losses = head.loss(cls, reg, gt_bboxes, gt_labels, ri.metas())
        for k, v in losses.items():
            d[f'{tag}_{k}'] = torch.stack(v)
        need(float(d[f'{tag}_loss_bbox'].sum()) > 0, 'no positive anchor')
        if with_grads:
            sum(losses['loss_cls'] + losses['loss_bbox']).backward()
            for l, (c, r) in enumerate(zip(cls, reg)):
                d[f'{tag}_dcls{l}'], d[f'{tag}_dreg{l}'] = c.grad, r.grad
        return d
    return run


def float64_run(m, img):
    """the same detector and input in float64: what the fp32 reference run is an approximation OF"""
    m64 = copy.deepcopy(m).double()
    return m64.simple_test(img.double(), ri.metas(), rescale=True)


def sec_model(seed, spies):
    """the detector end to end: simple_test of the seeded model on the seeded demo batch"""
    from mmdet.models import build_detector
    d = {}
    mc = ri.fixture_model_cfg()
    m = build_detector(cfgdict(copy.deepcopy(mc)))
    m.load_state_dict(ri.fixture_state_dict(m, seed))
    img, _, _, _ = util.demo_inputs(2, ri.H, ri.W, seed=seed)
    m.eval()
    sd = m.state_dict()
    d['state_keys'] = np.array(list(sd.keys()))
    d['state_shapes'] = np.array([json.dumps(list(v.shape)) for v in sd.values()])
    with torch.no_grad():
        check_topk(m.bbox_head(m.extract_feat(img))[0], 4, mc['test_cfg']['nms_pre'])
        res = m.simple_test(img, ri.metas(), rescale=True)
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
        m = build_detector(cfgdict(copy.deepcopy(ri.fixture_model_cfg())))
        m.load_state_dict(ri.fixture_state_dict(m, weight_seed()))
        m.train()
        img, tm, tg, tl = util.demo_inputs(2, ri.H, ri.W, seed=seed, num_gt=ri.TRAIN_NUM_GT)
        losses = m.forward_train(img, ri.metas(), tg, tl)
        return {f'train{it}_{k}': (torch.stack(v) if isinstance(v, list) else v) for k, v in losses.items()}
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
    for c in ri.CLASS_COUNTS:
        settle(f'bboxes_c{c}', sec_bboxes(c), 27, out)
    settle('loss_l1', sec_loss('loss_l1', 4, dict(type='L1Loss', loss_weight=1.0), True), 27, out)
    settle('loss_sl1', sec_loss('loss_sl1', 1, dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0), False), 27, out)
    settle('e2e', sec_model, 27, out)
    for it in range(2):
        settle(f'train{it}', sec_train(it, lambda: out['seed_e2e']), 1000 * (it + 1), out)
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, 'g27_retinanet.npz')
    np.savez_compressed(path, **out)
    print(f'g27_retinanet.npz  {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
