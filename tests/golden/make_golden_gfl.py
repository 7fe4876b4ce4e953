"""Generates tests/golden/g30_gfl.npz by importing the reference, on the CPU, under the test-only mmcv shim
(tests/golden/_mmcv_shim.py), the way make_golden_atss.py builds g29: seeded weights and inputs (tests/util.py,
tests/gfl_inputs.py), the reference's GFLHead / GFL run on them.  The fixture is data (seeds + expected outputs + the list of
the reference model's state-dict keys); no reference source is stored.
Run:  python tests/golden/make_golden_gfl.py

The margins are those of make_golden_atss.py (whose helpers are used): no candidate IoU within 1e-4 of the NMS threshold, no
score gap below 1e-6 at a top-k, score_thr or max_per_img boundary, no score ties, the assignment conditions of
`make_golden_atss.check_assignment`; end to end, the fp32 reference within 5e-5 of its own float64 run.  One more for the loss
sections: no positive whose target distance (in strides, before the clamp) lies within 1e-4 of an integer, because `floor`
decides the two bins of the Distribution Focal Loss.  A section whose inputs miss a condition moves on to the next seed; the
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
import make_golden_atss as GA  # noqa: E402

from tests import atss_ref64 as RA  # noqa: E402
from tests import gfl_inputs as gi  # noqa: E402
from tests import gfl_ref64 as R  # noqa: E402
from tests import util  # noqa: E402

REF_MARGIN, SCORE_MARGIN = F.REF_MARGIN, F.SCORE_MARGIN
need, cfgdict = F.need, F.cfgdict
check_assignment = GA.check_assignment
BIN_MARGIN = 1e-4


class Spies:
    """margin checks hooked into the reference's own decision point: multiclass_nms as GFLHead calls it (threshold and NMS
    both on the class score)"""

    def __enter__(self):
        import mmdet.models.dense_heads.gfl_head as GH
        self.saved = [(GH, 'multiclass_nms', GH.multiclass_nms)]
        mc_nms = GH.multiclass_nms

        def mc_spy(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num=-1, **k):
            s = multi_scores[:, :-1]
            need((s.double() - score_thr).abs().min().item() > SCORE_MARGIN, 'score_thr boundary')
            nc = s.shape[1]
            bb = multi_bboxes.view(len(s), -1, 4).expand(len(s), nc, 4)
            lab = torch.arange(nc).view(1, -1).expand_as(s)
            m = s > score_thr
            if m.any():
                F.check_nms(bb[m], s[m], lab[m], nms_cfg['iou_threshold'])
            allk = mc_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, -1, **k)
            F.check_sorted_gap(allk[0][:, 4], max_num, 'max_per_img')
            return mc_nms(multi_bboxes, multi_scores, score_thr, nms_cfg, max_num, **k)

        GH.multiclass_nms = mc_spy
        return self

    def __exit__(self, *exc):
        for obj, name, val in self.saved:
            setattr(obj, name, val)


def check_topk(cls_scores, num_classes, nms_pre):
    """make_golden_fcos.check_topk on the class score alone: a centerness logit of 100 is a factor of exactly 1"""
    GF.check_topk(cls_scores, [c.new_full((c.shape[0], 1) + tuple(c.shape[2:]), 100.0) for c in cls_scores], num_classes, nms_pre)


def check_bins(gt_bboxes, tag):
    """no positive's target distance within BIN_MARGIN of an integer"""
    inds = RA.assign(gt_bboxes, gi.SIZES, gi.STRIDES, gi.OCTAVE, gi.TOPK, dtype=torch.float32)
    starts = np.cumsum([0] + [h * w for h, w in gi.SIZES])
    ctrs = R.centers(gi.SIZES, gi.STRIDES, gi.OCTAVE)
    for b, ind in enumerate(inds):
        for l, s in enumerate(gi.STRIDES):
            sel = (ind[starts[l]:starts[l + 1]] > 0).nonzero().reshape(-1)
            if not len(sel):
                continue
            c = ctrs[l][sel] / s
            g = gt_bboxes[b][ind[starts[l]:starts[l + 1]][sel] - 1].double() / s
            side = torch.cat([c - g[:, :2], g[:, 2:] - c], 1)
            need(float((side - side.round()).abs().min()) > BIN_MARGIN, f'{tag}: a target distance within 1e-4 of an integer')


def build(num_classes, training, **over):
    from mmdet.models import build_head
    head = build_head(cfgdict(gi.head_cfg(num_classes, **over)))
    head.train(training)
    with torch.no_grad():
        for s, v in zip(head.scales, gi.SCALES):
            s.scale.fill_(v)
    return head


def sec_targets(seed, spies):
    """GFLHead.get_targets: labels, label weights and box targets (the ground-truth boxes) per level"""
    d = {}
    head = build(4, True)
    gt_bboxes, gt_labels = gi.gts(seed)
    check_assignment(gt_bboxes, 'targets')
    anchor_list, valid_flag_list = head.get_anchors(gi.SIZES, gi.metas(), device='cpu')
    out = head.get_targets(anchor_list, valid_flag_list, gt_bboxes, gi.metas(), gt_labels_list=gt_labels, label_channels=4)
    _, labels, label_weights, bbox_targets, _, num_pos, num_neg = out
    for l in range(len(gi.SIZES)):
        d[f'targets_labels{l}'], d[f'targets_weights{l}'], d[f'targets_box{l}'] = labels[l], label_weights[l], bbox_targets[l]
    d['targets_num'] = np.array([num_pos, num_neg])
    return d


def sec_loss(tag, num_classes, with_grads):
    def run(seed, spies):
        """GFLHead.loss on the scaled box logits of seeded raw outputs, and (with_grads) the autograd gradients of the
        summed loss w.r.t. the class logits, the RAW box logits and the per-level scales"""
        d = {}
        head = build(num_classes, True)
        cls, raw = gi.head_outputs(seed, num_classes, grad=True)
        scales = [torch.tensor(v, requires_grad=True) for v in gi.SCALES]
        gt_bboxes, gt_labels = gi.gts(seed, num_classes=num_classes)
        check_assignment(gt_bboxes, tag)
        check_bins(gt_bboxes, tag)
        losses = head.loss(cls, gi.scaled(raw, scales), gt_bboxes, gt_labels, gi.metas())
        for k, v in losses.items():
            d[f'{tag}_{k}'] = torch.stack([torch.as_tensor(x) for x in v])
        need(float(d[f'{tag}_loss_bbox'].sum()) > 0, 'no positive anchor')
        if with_grads:
            sum(sum(v) for v in losses.values()).backward()
            for l in range(len(gi.SIZES)):
                d[f'{tag}_dcls{l}'], d[f'{tag}_dreg{l}'] = cls[l].grad, raw[l].grad
            d[f'{tag}_dscale'] = torch.stack([s.grad for s in scales])
        return d
    return run


def sec_bboxes(num_classes):
    def run(seed, spies):
        """GFLHead.get_bboxes, head level, with and without rescale (and, for 4 classes, the image without a class score
        above the threshold)"""
        d, metas = {}, gi.metas()
        cases = [('plain', False, False), ('rescale', True, False)] + ([('empty', True, True)] if num_classes == 4 else [])
        for name, rescale, empty in cases:
            head = build(num_classes, False)
            cls, raw = gi.head_outputs(seed, num_classes, empty=empty)
            check_topk(cls, num_classes, gi.TEST_CFG['nms_pre'])
            res = head.get_bboxes(cls, gi.scaled(raw, gi.SCALES), metas, rescale=rescale)
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
    mc = gi.fixture_model_cfg()
    m = build_detector(cfgdict(copy.deepcopy(mc)))
    m.load_state_dict(gi.fixture_state_dict(m, seed))
    img, _, _, _ = util.demo_inputs(2, gi.H, gi.W, seed=seed)
    m.eval()
    sd = m.state_dict()
    d['state_keys'] = np.array(list(sd.keys()))
    d['state_shapes'] = np.array([json.dumps(list(v.shape)) for v in sd.values()])
    with torch.no_grad():
        outs = m.bbox_head(m.extract_feat(img))
        check_topk(outs[0], 4, mc['test_cfg']['nms_pre'])
        res = m.simple_test(img, gi.metas(), rescale=True)
        res64 = copy.deepcopy(m).double().simple_test(img.double(), gi.metas(), rescale=True)
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
        m = build_detector(cfgdict(copy.deepcopy(gi.fixture_model_cfg())))
        m.load_state_dict(gi.fixture_state_dict(m, weight_seed()))
        m.train()
        img, _, _, _ = util.demo_inputs(2, gi.H, gi.W, seed=seed, num_gt=gi.TRAIN_NUM_GT)
        tg, tl = gi.gts(seed)
        losses = m.forward_train(img, gi.metas(), tg, tl)
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
    settle('targets', sec_targets, 0, out)
    settle('loss_c4', sec_loss('loss_c4', 4, True), 0, out)
    settle('loss_c1', sec_loss('loss_c1', 1, False), 0, out)
    for c in gi.CLASS_COUNTS:
        settle(f'bboxes_c{c}', sec_bboxes(c), 30, out)
    settle('e2e', sec_model, 30, out)
    for it in range(2):
        settle(f'train{it}', sec_train(it, lambda: out['seed_e2e']), 1000 * (it + 1), out)
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, 'g30_gfl.npz')
    np.savez_compressed(path, **out)
    print(f'g30_gfl.npz  {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
