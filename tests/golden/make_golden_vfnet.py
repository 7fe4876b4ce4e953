"""Generates tests/golden/g31_vfnet.npz by importing the reference, on the CPU, under the test-only mmcv shim
(tests/golden/_mmcv_shim.py), the way make_golden_gfl.py builds g30: seeded weights and inputs (tests/util.py,
tests/vfnet_inputs.py), the reference's VFNetHead / VFNet run on them.  The fixture is data (seeds + expected outputs + the list
of the reference model's state-dict keys + the resolved recipe as JSON); no reference source is stored.
Run:  python tests/golden/make_golden_vfnet.py

mmcv's compiled DeformConv2d is not available: after the shim is installed, `mmdet.models.dense_heads.vfnet_head.DeformConv2d`
is bound here to a module that keeps mmcv's parameter (`weight`, kaiming-uniform) and evaluates mmcv's sampling rule on torch
ops (tests/vfnet_ref64.deform_conv_v1).

The margins are those of make_golden_atss.py / make_golden_gfl.py (whose helpers are used): no candidate IoU within 1e-4 of
the NMS threshold, no score gap below 1e-6 at a top-k, score_thr or max_per_img boundary, no score ties, the assignment
conditions of `make_golden_atss.check_assignment`; end to end, the fp32 reference within 5e-5 of its own float64 run.  One more
for the section that records a gradient through the star offsets: no star sample coordinate within 1e-3 of an integer, where
the bilinear gradient w.r.t. the offset has a kink (checked in float64).  A section whose inputs miss a condition moves on to
the next seed; the seed it settles on is recorded.
"""
import copy
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_faster_rcnn as F  # noqa: E402  (installs the shim, puts the repository root on the path)
import make_golden_atss as GA  # noqa: E402
import make_golden_gfl as GG  # noqa: E402

from tests import util  # noqa: E402
from tests import vfnet_inputs as vi  # noqa: E402
from tests import vfnet_ref64 as R  # noqa: E402

REF_MARGIN, SCORE_MARGIN = F.REF_MARGIN, F.SCORE_MARGIN
need, cfgdict = F.need, F.cfgdict
check_assignment, check_topk = GA.check_assignment, GG.check_topk
INT_MARGIN = 1e-3
REF_CONFIG = os.path.join(F._mmcv_shim.REFERENCE_ROOT, 'configs', 'vfnet', 'vfnet_r50_fpn_1x_coco.py')


class TorchDeformConv2d(nn.Module):
    """mmcv.ops.DeformConv2d for a 3 x 3, stride 1, padding 1, bias-free conv, on torch ops"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, **kw):
        super().__init__()
        assert kernel_size == 3 and stride == 1 and padding == 1 and not kw
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 3, 3))
        nn.init.kaiming_uniform_(self.weight, nonlinearity='relu')

    def forward(self, x, offset):
        return R.deform_conv_v1(x.permute(0, 2, 3, 1), offset.permute(0, 2, 3, 1), self.weight).permute(0, 3, 1, 2)


def bind_deform_conv():
    import mmdet.models.dense_heads.vfnet_head as VH
    VH.DeformConv2d = TorchDeformConv2d
    return VH


class Spies:
    """margin checks hooked into the reference's own decision point: multiclass_nms as VFNetHead calls it (threshold and NMS
    both on the class score)"""

    def __enter__(self):
        VH = bind_deform_conv()
        self.saved = [(VH, 'multiclass_nms', VH.multiclass_nms)]
        mc_nms = VH.multiclass_nms

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

        VH.multiclass_nms = mc_spy
        return self

    def __exit__(self, *exc):
        for obj, name, val in self.saved:
            setattr(obj, name, val)


def build(num_classes, training, **over):
    from mmdet.models import build_head
    head = build_head(cfgdict(vi.head_cfg(num_classes, **over)))
    head.train(training)
    with torch.no_grad():
        for s, v in zip(head.scales, vi.SCALES):
            s.scale.fill_(v)
        for s, v in zip(head.scales_refine, vi.SCALES_REFINE):
            s.scale.fill_(v)
    return head


def sec_targets(seed, spies):
    """VFNetHead.get_targets: labels and (l, t, r, b) targets per level"""
    d = {}
    head = build(4, True)
    gt_bboxes, gt_labels = vi.gts(seed)
    check_assignment(gt_bboxes, 'targets')
    cls, _, _ = vi.head_outputs(seed)
    pts = head.get_points(vi.SIZES, torch.float32, 'cpu')
    labels, _, targets, _ = head.get_targets(cls, pts, gt_bboxes, gt_labels, vi.metas(), None)
    for l in range(len(vi.SIZES)):
        d[f'targets_labels{l}'], d[f'targets_ltrb{l}'] = labels[l], targets[l]
    return d


def sec_loss(tag, num_classes, with_grads, pads=None):
    def run(seed, spies):
        """VFNetHead.loss on the distances of seeded raw outputs, and (with_grads) the autograd gradients of the summed loss
        w.r.t. the class logits, `bbox_preds` and `bbox_preds_refine`"""
        d = {}
        head = build(num_classes, True)
        cls, raw0, raw1 = vi.head_outputs(seed, num_classes, grad=False)
        d0, d1 = vi.distances(raw0, raw1)
        if with_grads:
            cls, d0, d1 = ([t.detach().requires_grad_() for t in lst] for lst in (cls, d0, d1))
        gt_bboxes, gt_labels = vi.gts(seed, num_classes=num_classes)
        check_assignment(gt_bboxes, tag)
        losses = head.loss(cls, d0, d1, gt_bboxes, gt_labels, vi.metas(pads=pads))
        for k, v in losses.items():
            d[f'{tag}_{k}'] = torch.as_tensor(v).reshape(())
        need(float(d[f'{tag}_loss_bbox']) > 0 and float(d[f'{tag}_loss_bbox_rf']) > 0, 'no positive anchor')
        if with_grads:
            sum(losses.values()).backward()
            for l in range(len(vi.SIZES)):
                d[f'{tag}_dcls{l}'], d[f'{tag}_dd0{l}'], d[f'{tag}_dd1{l}'] = cls[l].grad, d0[l].grad, d1[l].grad
        return d
    return run


def sec_bboxes(num_classes):
    def run(seed, spies):
        """VFNetHead.get_bboxes, head level, with and without rescale (and, for 4 classes, the image without a class score
        above the threshold)"""
        d, metas = {}, vi.metas()
        cases = [('plain', False, False), ('rescale', True, False)] + ([('empty', True, True)] if num_classes == 4 else [])
        for name, rescale, empty in cases:
            head = build(num_classes, False)
            cls, raw0, raw1 = vi.head_outputs(seed, num_classes, empty=empty)
            d0, d1 = vi.distances(raw0, raw1)
            check_topk(cls, num_classes, vi.TEST_CFG['nms_pre'])
            res = head.get_bboxes(cls, d0, d1, metas, rescale=rescale)
            for b in range(2):
                d[f'bboxes_c{num_classes}_{name}_det{b}'], d[f'bboxes_c{num_classes}_{name}_lab{b}'] = res[b]
            need(len(res[0][0]) > 0, 'no detections')
            if empty:
                need(len(res[1][0]) == 0, 'the empty case')
        return d
    return run


def sec_forward(seed, spies):
    """the head's forward on a seeded pyramid with seeded weights: class logits, distances and refined distances through
    the star deformable convs (the forward is continuous in the offsets: no integer margin)"""
    d = {}
    head = build(4, False)
    head.load_state_dict(vi.seeded_head_state(head, seed))
    with torch.no_grad():
        cls, d0, d1 = head(vi.features(seed))
    inside = outside = 0
    for l, (p, s) in enumerate(zip(d0, vi.STRIDES)):
        pts = R.sample_points(head.star_dcn_offset(p.double(), vi.GRADIENT_MUL, s).permute(0, 2, 3, 1))
        h, w = vi.SIZES[l]
        ins = (pts[..., 0] > -1) & (pts[..., 1] > -1) & (pts[..., 0] < h) & (pts[..., 1] < w)
        inside, outside = inside + int(ins.sum()), outside + int((~ins).sum())
    need(inside > 100 and outside > 100, 'forward: star samples inside and outside the maps')
    for l in range(len(vi.SIZES)):
        d[f'fwd_cls{l}'], d[f'fwd_d0{l}'], d[f'fwd_d1{l}'] = cls[l], d0[l], d1[l]
    return d


def sec_forward_grad(seed, spies):
    """level 0 of the same head on ONE small seeded map (`vi.small_feature`), with the gradient of sum(cls) + sum(log
    bbox_preds_refine) w.r.t. the map.  It passes through the offsets, so the integer margin applies -- over the 42 x 12
    distance-dependent coordinates of this map it holds for about one seed in three; over a whole pyramid it never would"""
    d = {}
    head = build(4, False)
    head.load_state_dict(vi.seeded_head_state(head, seed))
    x = vi.small_feature(seed).requires_grad_()
    cls, d0, d1 = head([x])
    off = head.star_dcn_offset(d0[0].detach().double(), vi.GRADIENT_MUL, vi.STRIDES[0]).permute(0, 2, 3, 1)
    need(R.integer_margin(off) > INT_MARGIN, 'forward_grad: a star sample within 1e-3 of an integer')
    (cls[0].sum() + d1[0].log().sum()).backward()
    d['fgrad_cls'], d['fgrad_d0'], d['fgrad_d1'], d['fgrad_dx'] = cls[0], d0[0], d1[0], x.grad
    return d


def sec_model(seed, spies):
    """the detector end to end: simple_test of the seeded model on the seeded demo batch"""
    from mmdet.models import build_detector
    d = {}
    mc = vi.fixture_model_cfg()
    m = build_detector(cfgdict(copy.deepcopy(mc)))
    m.load_state_dict(vi.fixture_state_dict(m, seed))
    img, _, _, _ = util.demo_inputs(2, vi.H, vi.W, seed=seed)
    m.eval()
    sd = m.state_dict()
    d['state_keys'] = np.array(list(sd.keys()))
    d['state_shapes'] = np.array([json.dumps(list(v.shape)) for v in sd.values()])
    with torch.no_grad():
        outs = m.bbox_head(m.extract_feat(img))
        check_topk(outs[0], 4, mc['test_cfg']['nms_pre'])
        res = m.simple_test(img, vi.metas(), rescale=True)
        res64 = copy.deepcopy(m).double().simple_test(img.double(), vi.metas(), rescale=True)
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
        m = build_detector(cfgdict(copy.deepcopy(vi.fixture_model_cfg())))
        m.load_state_dict(vi.fixture_state_dict(m, weight_seed()))
        m.train()
        img, _, _, _ = util.demo_inputs(2, vi.H, vi.W, seed=seed, num_gt=vi.TRAIN_NUM_GT)
        tg, tl = vi.gts(seed)
        losses = m.forward_train(img, vi.metas(), tg, tl)
        return {f'train{it}_{k}': torch.as_tensor(v).reshape(()) for k, v in losses.items()}
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
    from brcnn import Config
    out = {'config_json': json.dumps(Config.fromfile(os.path.normpath(REF_CONFIG)).to_dict(), sort_keys=True)}
    settle('targets', sec_targets, 0, out)
    settle('loss_c4', sec_loss('loss_c4', 4, True), 0, out)
    settle('loss_c1', sec_loss('loss_c1', 1, False), 0, out)
    settle('loss_pad', sec_loss('loss_pad', 4, False, pads=[(128, 192), (96, 160)]), 0, out)
    for c in vi.CLASS_COUNTS:
        settle(f'bboxes_c{c}', sec_bboxes(c), 30, out)
    settle('forward', sec_forward, 0, out)
    settle('forward_grad', sec_forward_grad, 0, out)
    settle('e2e', sec_model, 30, out)
    for it in range(2):
        settle(f'train{it}', sec_train(it, lambda: out['seed_e2e']), 1000 * (it + 1), out)
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    path = os.path.join(HERE, 'g31_vfnet.npz')
    np.savez_compressed(path, **out)
    print(f'g31_vfnet.npz  {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
