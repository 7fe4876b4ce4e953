"""Generates tests/golden/g25_faster_rcnn.npz by IMPORTING THE REFERENCE (/root/reference) in the authoring container, on
the CPU, under the test-only mmcv shim (tests/golden/_mmcv_shim.py), the way make_golden.py builds g18_boost_variants:
seeded weights and inputs (tests/util.py, tests/faster_rcnn_inputs.py), the reference's RPNHead / StandardRoIHead /
FasterRCNN run on them.  The fixture is data (seeds + expected outputs); no reference source is stored.
Run:  python tests/golden/make_golden_faster_rcnn.py

Exact comparisons (kept indices, labels, order) only mean something when no decision of the reference sits on a
rounding edge, so the generator asserts margins ON THE INPUTS while it runs and moves on to the next seed when one
fails: no candidate IoU within 1e-4 of an NMS or assignment threshold, no score gap below 1e-6 at a top-k,
score_thr or max_per_img boundary; end to end, the fp32 reference within 5e-5 of its own float64 run.  Every section of the fixture settles on its own seed, which is recorded.
"""
import copy
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import _mmcv_shim  # noqa: E402

_mmcv_shim.install()
from tests import faster_rcnn_inputs as fi  # noqa: E402
from tests import util  # noqa: E402
import brcnn  # noqa: E402,F401

IOU_MARGIN, SCORE_MARGIN = 1e-4, 1e-6
# End to end the tests hold the device to 2e-4 of the reference's fp32 run, which is itself one fp32 evaluation of fifty
# layers: |device - ref32| <= |device - exact| + |ref32 - exact|.  A fixture whose reference run is already 1e-4 off its own
# float64 run would mostly measure the reference's round-off, so an end-to-end section only settles on inputs where the
# reference's boxes and scores are within a quarter of that bound of the float64 run of the same model (same detections,
# same order); three quarters are left to the code under test.
REF_MARGIN = 5e-5


class Margin(Exception):
    pass


def cfgdict(x):
    return _mmcv_shim.ConfigDict.wrap(x)


def need(ok, what):
    if not ok:
        raise Margin(what)


def check_nms(boxes, scores, idxs, thr):
    from mmdet.core.bbox.iou_calculators import bbox_overlaps
    for i in torch.unique(idxs):
        b = boxes[idxs == i]
        if len(b) > 1:
            iou = bbox_overlaps(b.double(), b.double())
            need((iou - thr).abs().min().item() > IOU_MARGIN, f'NMS IoU within {IOU_MARGIN} of {thr}')
    if len(scores) > 1:         # no ties: the order in which the NMS visits (and the result lists) the candidates is defined
        s = torch.sort(scores.double())[0]
        need((s[1:] - s[:-1]).min().item() > SCORE_MARGIN, 'two NMS candidates with the same score')


def check_sorted_gap(scores, k, what):
    """descending `scores`: the k-th and (k+1)-th differ by more than the margin (k = how many are kept)"""
    s = torch.sort(scores.double().reshape(-1), descending=True)[0]
    if 0 < k < len(s):
        need((s[k - 1] - s[k]).item() > SCORE_MARGIN, f'{what}: score gap at rank {k}')


class Spies:
    """margin checks hooked into the reference's own decision points"""

    def __enter__(self):
        import mmdet.core.bbox.assigners.max_iou_assigner as MA
        import mmdet.models.dense_heads.atss_rpn_head as AH
        import mmdet.models.dense_heads.rpn_head as RH
        import mmdet.models.roi_heads.bbox_heads.bbox_head as BH
        self.saved = [(RH, 'batched_nms', RH.batched_nms), (AH, 'batched_nms', AH.batched_nms), (BH, 'multiclass_nms', BH.multiclass_nms),
                      (MA.MaxIoUAssigner, 'assign_wrt_overlaps', MA.MaxIoUAssigner.assign_wrt_overlaps)]
        self.rpn_max_per_img = None
        rpn_nms, mc_nms, wrt = RH.batched_nms, BH.multiclass_nms, MA.MaxIoUAssigner.assign_wrt_overlaps
        spies = self

        def rpn_spy(boxes, scores, idxs, nms_cfg, class_agnostic=False):
            check_nms(boxes, scores, idxs, nms_cfg['iou_threshold'])
            dets, keep = rpn_nms(boxes, scores, idxs, nms_cfg, class_agnostic)
            if spies.rpn_max_per_img:
                check_sorted_gap(dets[:, 4], spies.rpn_max_per_img, 'rpn max_per_img')
            return dets, keep

        def mc_spy(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1, *a, **k):
            s = multi_scores[:, :-1]
            need((s.double() - score_thr).abs().min().item() > SCORE_MARGIN, 'score_thr boundary')
            nc = s.shape[1]
            bb = multi_bboxes.view(len(s), -1, 4).expand(len(s), nc, 4)
            lab = torch.arange(nc).view(1, -1).expand_as(s)
            m = s > score_thr
            if m.any():
                check_nms(bb[m], s[m], lab[m], nms_cfg['iou_threshold'])
            allk = mc_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, -1, *a, **k)
            check_sorted_gap(allk[0][:, 4], max_num, 'rcnn max_per_img')
            return mc_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num, *a, **k)

        def wrt_spy(self_, overlaps, gt_labels=None):
            if overlaps.numel():
                for thr in (self_.pos_iou_thr, self_.neg_iou_thr, self_.min_pos_iou):
                    for t in (thr if isinstance(thr, (tuple, list)) else (thr,)):
                        if t > 0:
                            need((overlaps.double() - t).abs().min().item() > IOU_MARGIN,
                                 f'assignment IoU within {IOU_MARGIN} of {t}')
            return wrt(self_, overlaps, gt_labels)

        RH.batched_nms, BH.multiclass_nms, MA.MaxIoUAssigner.assign_wrt_overlaps = rpn_spy, mc_spy, wrt_spy
        AH.batched_nms = rpn_spy
        return self

    def __exit__(self, *exc):
        for obj, name, val in self.saved:
            setattr(obj, name, val)


def check_topk(cls_scores, nms_pre):
    for lvl in cls_scores:
        for b in range(lvl.shape[0]):
            check_sorted_gap(lvl[b].detach().sigmoid(), nms_pre, 'rpn top-k')


def dets_table(res):
    """per-class result lists of one image -> (n, 6) [x1, y1, x2, y2, score, class], class-major"""
    return np.concatenate([np.concatenate([r, np.full((len(r), 1), c, np.float32)], 1) for c, r in enumerate(res)], 0)


def sec_props(seed, spies):
    """RPNHead.get_bboxes, head level, at the four proposal cfgs"""
    from mmdet.models import build_head
    d, metas = {}, fi.metas()
    head = build_head(cfgdict(fi.rpn_head_cfg()))
    head.eval()
    for name, pc in fi.PROPOSAL_CFGS.items():
        cls, reg = fi.rpn_outputs(seed, empty=(name == 'empty'))
        check_topk(cls, pc['nms_pre'])
        spies.rpn_max_per_img = pc['max_per_img']
        res = head.get_bboxes(cls, reg, metas, cfg=cfgdict(copy.deepcopy(pc)))
        for b in range(2):
            d[f'props_{name}{b}'] = res[b]
    need(len(d['props_empty1']) == 0 and len(d['props_empty0']) > 0, 'the empty case')
    need(0 < len(d['props_minsize0']), 'the min_bbox_size case')
    return d


def sec_rpnloss(seed, spies):
    """RPNHead.loss under a fixed seed, with the drawn indices"""
    from mmdet.models import build_head
    d = {}
    head = build_head(cfgdict(fi.rpn_head_cfg()))
    head.train()
    cls, reg = fi.rpn_outputs(seed, grad=True)
    gt_bboxes, _ = fi.gts(seed)
    drawn = []
    sample = head.sampler.sample

    def sample_spy(assign_result, bboxes, gt, *a, **k):
        r = sample(assign_result, bboxes, gt, *a, **k)
        drawn.append((r.pos_inds.clone(), r.neg_inds.clone()))
        return r
    head.sampler.sample = sample_spy
    torch.manual_seed(seed + 100)
    losses = head.loss(cls, reg, gt_bboxes, fi.metas())
    for k, v in losses.items():
        d[f'rpnloss_{k}'] = torch.stack(v)
    for b, (p, n) in enumerate(drawn):
        d[f'rpnloss_pos{b}'], d[f'rpnloss_neg{b}'] = p, n
    return d


def sec_roi(tag, kind):
    def run(seed, spies):
        """second stage, head level: forward_train losses (seeded sampler) and simple_test detections"""
        from mmdet.models import build_head
        d = {}
        rh = build_head(cfgdict(fi.roi_head_cfg(kind)))
        rh.load_state_dict(util.seeded_state_dict(rh, seed=seed))
        feats, vmetas, vg, vl, props = fi.roi_inputs(seed)
        rh.train()
        torch.manual_seed(seed + 100)
        for k, v in rh.forward_train(feats, vmetas, props, vg, vl).items():
            d[f'{tag}_train_{k}'] = v
        rh.eval()
        with torch.no_grad():
            det, lab = rh.simple_test_bboxes(feats, vmetas, props, rh.test_cfg, rescale=True)
        for b in range(2):
            d[f'{tag}_det{b}'], d[f'{tag}_lab{b}'] = det[b], lab[b]
        return d
    return run


def float64_run(m, img):
    """the same detector and input in float64 (RoIAlign: tests/roi_ref64.py, the reference's operator is fp32 only):
    what the fp32 reference run is an approximation OF"""
    from tests import roi_ref64
    m64 = copy.deepcopy(m).double()
    for layer in m64.roi_head.bbox_roi_extractor.roi_layers:
        layer.forward = (lambda x, rois, l=layer: roi_ref64.roi_align_f64(x.double(), rois, l.output_size[0], l.spatial_scale))
    return m64.simple_test(img.double(), fi.metas(), rescale=True)


def sec_model(tag, mc):
    def run(seed, spies):
        """the detector end to end: simple_test of the seeded model on the seeded demo batch"""
        from mmdet.models import build_detector
        d = {}
        m = build_detector(cfgdict(copy.deepcopy(mc)))
        m.load_state_dict(fi.fixture_state_dict(m, seed))
        img, _, _, _ = util.demo_inputs(2, fi.H, fi.W, seed=seed)
        m.eval()
        if tag == 'e2e':
            sd = m.state_dict()
            d['state_keys'] = np.array(list(sd.keys()))
            d['state_shapes'] = np.array([json.dumps(list(v.shape)) for v in sd.values()])
        with torch.no_grad():
            if type(m.rpn_head).__name__ == 'RPNHead':
                check_topk(m.rpn_head(m.extract_feat(img))[0], mc['test_cfg']['rpn']['nms_pre'])
            else:       # RetinaRPN scores: sqrt(sigmoid(cls) * sigmoid(iou))
                c_, _, i_ = m.rpn_head(m.extract_feat(img))
                for cl, io in zip(c_, i_):
                    for b in range(cl.shape[0]):
                        check_sorted_gap((cl[b].sigmoid() * io[b].sigmoid()).sqrt(), mc['test_cfg']['rpn']['nms_pre'],
                                         'rpn top-k')
            spies.rpn_max_per_img = mc['test_cfg']['rpn']['max_per_img']
            res = m.simple_test(img, fi.metas(), rescale=True)
            res64 = float64_run(m, img)
        worst = 0.0
        for b in range(2):
            d[f'{tag}_res{b}'] = dets_table(res[b])
            t64 = dets_table(res64[b])
            need(t64.shape == d[f'{tag}_res{b}'].shape and np.array_equal(t64[:, 5], d[f'{tag}_res{b}'][:, 5]),
                 f'{tag}: the float64 run keeps other detections')
            if len(t64):
                worst = max(worst, float(np.abs(t64[:, :5] - d[f'{tag}_res{b}'][:, :5].astype(np.float64)).max()))
        need(worst <= REF_MARGIN, f'{tag}: the fp32 reference is {worst:.2e} from its float64 run')
        d[f'{tag}_ref_err'] = worst
        need(sum(len(d[f'{tag}_res{b}']) for b in range(2)) > 0, f'{tag}: no detections')
        return d
    return run


def sec_train(it, weight_seed):
    def run(seed, spies):
        """one train iteration of the recipe (the e2e section's weights, fresh inputs and sampler seed)"""
        from mmdet.models import build_detector
        mc = fi.fixture_model_cfg()
        m = build_detector(cfgdict(copy.deepcopy(mc)))
        m.load_state_dict(fi.fixture_state_dict(m, weight_seed()))
        m.train()
        img, tm, tg, tl = util.demo_inputs(2, fi.H, fi.W, seed=seed, num_gt=fi.TRAIN_NUM_GT)
        with torch.no_grad():
            check_topk(m.rpn_head(m.extract_feat(img))[0], mc['train_cfg']['rpn_proposal']['nms_pre'])
        spies.rpn_max_per_img = mc['train_cfg']['rpn_proposal']['max_per_img']
        torch.manual_seed(seed + 100)
        losses = m.forward_train(img, tm, tg, tl)
        return {f'train{it}_{k}': (torch.stack(v) if isinstance(v, list) else v) for k, v in losses.items()}
    return run


def settle(name, fn, first, out):
    """run section `fn` at the first seed from `first` on whose inputs meet the margins; the seed goes into the fixture"""
    for seed in range(first, first + 400):
        try:
            with Spies() as spies:
                d = fn(seed, spies)
        except Margin as e:
            print(f'{name}: seed {seed}: {e}; trying the next')
            continue
        out.update(d)
        out[f'seed_{name}'] = seed
        print(f'{name}: seed {seed}')
        return seed
    raise SystemExit(f'{name}: no seed met the margins')


def main():
    out = {}
    settle('props', sec_props, 25, out)
    settle('rpnloss', sec_rpnloss, 25, out)
    settle('std', sec_roi('std', 'StandardRoIHead'), 25, out)
    settle('prob', sec_roi('prob', 'ProbRoIHead'), 25, out)
    settle('e2e', sec_model('e2e', fi.fixture_model_cfg()), 25, out)
    settle('atss_std', sec_model('atss_std', fi.cross_model_cfg('atss_std')), 25, out)
    settle('rpn_prob', sec_model('rpn_prob', fi.cross_model_cfg('rpn_prob')), 25, out)
    for it in range(2):
        settle(f'train{it}', sec_train(it, lambda: out['seed_e2e']), 1000 * (it + 1), out)
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, 'g25_faster_rcnn.npz')
    np.savez_compressed(path, **out)
    print(f'g25_faster_rcnn.npz  {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
