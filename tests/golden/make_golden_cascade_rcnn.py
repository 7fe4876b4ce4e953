"""Generates tests/golden/g26_cascade_rcnn.npz by IMPORTING THE REFERENCE (the checkout make_golden_faster_rcnn.py names)
in the authoring container, on the CPU, under the test-only mmcv shim (tests/golden/_mmcv_shim.py), the way
make_golden_faster_rcnn.py builds g25: seeded weights and inputs (tests/util.py, tests/faster_rcnn_inputs.py, tests/cascade_rcnn_inputs.py), the reference's
BBoxHead.refine_bboxes / regress_by_class, CascadeRoIHead and CascadeRCNN run on them.  The fixture is data (seeds +
expected outputs); no reference source is stored.
Run:  python tests/golden/make_golden_cascade_rcnn.py

The discipline is make_golden_faster_rcnn.py's, whose spies and margins are reused as they are: margins are asserted ON
THE INPUTS while a section runs (no candidate IoU within 1e-4 of an NMS threshold or of ANY stage's assignment
threshold -- the assigner spy reads the thresholds off the assigner it is called on --, no score gap below 1e-6 at a
top-k, score_thr or max_per_img boundary; end to end the fp32 reference within 5e-5 of its own float64 run), a seed
whose margins fail is skipped for the next one, and every section's seed is recorded.  One margin is new: wherever the
arg-max of the foreground logits decides which deltas a class-specific head reads, the row's top two foreground logits
differ by more than the score margin.
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
import make_golden_faster_rcnn as G25  # noqa: E402  (installs the shim; its spies, margins and `settle`)

from tests import cascade_rcnn_inputs as ci  # noqa: E402
from tests import faster_rcnn_inputs as fi  # noqa: E402
from tests import util  # noqa: E402

need, cfgdict, settle = G25.need, G25.cfgdict, G25.settle


def check_argmax_gap(cls_score, rows=None):
    """the new margin: top two foreground logits of every (selected) row apart by more than the score margin"""
    fg = cls_score[:, :-1].double()
    if rows is not None:
        fg = fg[rows]
    if fg.shape[0] and fg.shape[1] > 1:
        top = torch.topk(fg, 2, dim=1)[0]
        need((top[:, 0] - top[:, 1]).min().item() > G25.SCORE_MARGIN, 'arg-max: the top two foreground logits of a row tie')


def sec_refine(seed, spies):
    """(a) BBoxHead.refine_bboxes as CascadeRoIHead.forward_train calls it, and regress_by_class as simple_test does,
    on seeded rows, for a class-agnostic and a class-specific head"""
    from mmdet.models import build_head
    d, metas = {}, fi.metas()
    for tag, agnostic in (('agn', True), ('cls', False)):
        head = build_head(cfgdict(ci.box_head_cfg(0, reg_class_agnostic=agnostic)))
        rois, labels, cls_score, bbox_pred, flags = ci.refine_rows(seed, agnostic)
        C = head.num_classes
        if not agnostic:
            check_argmax_gap(cls_score)
        with torch.no_grad():
            roi_labels = torch.where(labels == C, cls_score[:, :-1].argmax(1), labels)
            refined = head.refine_bboxes(rois, roi_labels, bbox_pred, flags, metas)
            for b in range(2):
                m = rois[:, 0] == b
                d[f'refine_{tag}_train{b}'] = refined[b]
                d[f'refine_{tag}_test{b}'] = head.regress_by_class(rois[m], cls_score[m][:, :-1].argmax(1), bbox_pred[m],
                                                                   metas[b])
        need(len(refined[0]) == ci.REFINE_ROWS[0] - 4 and len(refined[1]) == ci.REFINE_ROWS[1], 'refine: rows kept')
        hi = torch.tensor([fi.W - 3.0, float(fi.H)] * 2)
        allb = torch.cat(refined)
        need(bool((allb == 0).any()) and bool((allb == hi).any()), 'refine: no box meets the border')
    return d


def spy_argmax(rh):
    """hook the new margin into the reference's decision points: every stage's regress_by_class sees the labels the
    arg-max chose, so the logits are checked where they are produced (class-specific heads only)"""
    if all(h.reg_class_agnostic for h in rh.bbox_head):
        return
    fwd = rh._bbox_forward

    def spy(stage, x, rois):
        r = fwd(stage, x, rois)
        if not rh.bbox_head[stage].reg_class_agnostic and stage < rh.num_stages - 1:
            check_argmax_gap(r['cls_score'].detach())
        return r
    rh._bbox_forward = spy


def sec_head(seed, spies):
    """(b) the cascade at head level: forward_train losses of the three stages (seeded samplers) and simple_test"""
    from mmdet.models import build_head
    d = {}
    rh = build_head(cfgdict(ci.roi_head_cfg()))
    rh.load_state_dict(ci.head_state_dict(rh, seed))
    spy_argmax(rh)
    feats, vmetas, vg, vl, props = fi.roi_inputs(seed)
    rh.train()
    torch.manual_seed(seed + 100)
    losses = rh.forward_train(feats, vmetas, props, vg, vl)
    need(len(losses) == 3 * ci.NUM_STAGES, 'head: a stage is missing from the losses')
    for k, v in losses.items():
        d[f'head_train_{k}'] = v
    rh.eval()
    with torch.no_grad():
        res = rh.simple_test(feats, props, vmetas, rescale=True)
    for b in range(2):
        d[f'head_res{b}'] = G25.dets_table(res[b])
    need(min(len(d[f'head_res{b}']) for b in range(2)) > 0, 'head: an image without detections')
    return d


def float64_run(m, img):
    """the same detector and input in float64 (RoIAlign: tests/roi_ref64.py): what the fp32 reference run approximates"""
    from tests import roi_ref64
    m64 = copy.deepcopy(m).double()
    for ex in m64.roi_head.bbox_roi_extractor:
        for layer in ex.roi_layers:
            layer.forward = (lambda x, rois, l=layer: roi_ref64.roi_align_f64(x.double(), rois, l.output_size[0], l.spatial_scale))
    return m64.simple_test(img.double(), fi.metas(), rescale=True)


def sec_model(seed, spies):
    """(c) the detector end to end, and (e) its state_dict keys and shapes"""
    from mmdet.models import build_detector
    d = {}
    mc = ci.fixture_model_cfg()
    m = build_detector(cfgdict(copy.deepcopy(mc)))
    m.load_state_dict(ci.fixture_state_dict(m, seed))
    spy_argmax(m.roi_head)
    img, _, _, _ = util.demo_inputs(2, fi.H, fi.W, seed=seed)
    m.eval()
    sd = m.state_dict()
    d['state_keys'] = np.array(list(sd.keys()))
    d['state_shapes'] = np.array([json.dumps(list(v.shape)) for v in sd.values()])
    with torch.no_grad():
        G25.check_topk(m.rpn_head(m.extract_feat(img))[0], mc['test_cfg']['rpn']['nms_pre'])
        spies.rpn_max_per_img = mc['test_cfg']['rpn']['max_per_img']
        res = m.simple_test(img, fi.metas(), rescale=True)
        res64 = float64_run(m, img)
    worst = 0.0
    for b in range(2):
        d[f'e2e_res{b}'] = G25.dets_table(res[b])
        t64 = G25.dets_table(res64[b])
        need(t64.shape == d[f'e2e_res{b}'].shape and np.array_equal(t64[:, 5], d[f'e2e_res{b}'][:, 5]),
             'e2e: the float64 run keeps other detections')
        if len(t64):
            worst = max(worst, float(np.abs(t64[:, :5] - d[f'e2e_res{b}'][:, :5].astype(np.float64)).max()))
    need(worst <= G25.REF_MARGIN, f'e2e: the fp32 reference is {worst:.2e} from its float64 run')
    d['e2e_ref_err'] = worst
    need(sum(len(d[f'e2e_res{b}']) for b in range(2)) > 0, 'e2e: no detections')
    return d


def sec_train(it, weight_seed):
    def run(seed, spies):
        """(d) one train iteration of the recipe (the e2e section's weights, fresh inputs and sampler seed)"""
        from mmdet.models import build_detector
        mc = ci.fixture_model_cfg()
        m = build_detector(cfgdict(copy.deepcopy(mc)))
        m.load_state_dict(ci.fixture_state_dict(m, weight_seed()))
        spy_argmax(m.roi_head)
        m.train()
        img, tm, tg, tl = util.demo_inputs(2, fi.H, fi.W, seed=seed, num_gt=fi.TRAIN_NUM_GT)
        with torch.no_grad():
            G25.check_topk(m.rpn_head(m.extract_feat(img))[0], mc['train_cfg']['rpn_proposal']['nms_pre'])
        spies.rpn_max_per_img = mc['train_cfg']['rpn_proposal']['max_per_img']
        torch.manual_seed(seed + 100)
        losses = m.forward_train(img, tm, tg, tl)
        need(all(f's{i}.loss_cls' in losses for i in range(ci.NUM_STAGES)), 'train: a stage is missing from the losses')
        return {f'train{it}_{k}': (torch.stack(v) if isinstance(v, list) else v) for k, v in losses.items()}
    return run


def main():
    out = {}
    settle('refine', sec_refine, 26, out)
    settle('head', sec_head, 26, out)
    settle('e2e', sec_model, 26, out)
    for it in range(2):
        settle(f'train{it}', sec_train(it, lambda: out['seed_e2e']), 1000 * (it + 1), out)
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, 'g26_cascade_rcnn.npz')
    np.savez_compressed(path, **out)
    print(f'g26_cascade_rcnn.npz  {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
