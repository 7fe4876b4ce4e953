"""Generates tests/golden/g24_tta.npz by IMPORTING THE REFERENCE in the authoring container, on CPU, under the test-only
mmcv shim (tests/golden/_mmcv_shim.py): test-time augmentation (TwoStageDetector.aug_test) of the seeded g10 UTDAC model
on the five augs of tests/tta_util.py, for each of the batch's two images ALONE with the batch's padded tensors (the
reference's RoI stage reads image 0 only).  Data only; no reference source is stored.
Run:  python tests/golden/make_golden_tta.py

Stored per image b (the aug images are rebuilt from the seed):
  props{a}_{b}            the reference's proposals of aug a, aug frame
  merged_{b}              merge_aug_proposals: original frame
  cls{a}_{b}, reg{a}_{b}  box-head outputs of aug a on the merged proposals mapped into its frame (raw logits)
  raw_*                   mode 'raw' = the reference literally: merged boxes / "scores" (logit means), multiclass_nms,
                          and its own forward_test for both `rescale` values
  fused_*                 mode 'fused': the same chain with sqrt(softmax * prior) per aug (prob_roi_head.py:232-240)
"""
import copy
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
from tests import tta_util, util  # noqa: E402
import brcnn  # noqa: E402,F401
from brcnn.config import Config  # noqa: E402
from oracle import orc  # noqa: E402

REF_CFG = '/root/reference/configs/boosting_rcnn/boosting_rcnn_r50_pafpn_1x_utdac.py'


def main():
    from mmdet.core import bbox2roi, bbox_mapping, merge_aug_bboxes, multiclass_nms
    from mmdet.core.post_processing import merge_augs
    from mmdet.models import build_detector
    # under the shim `from mmcv.ops import nms` inside merge_augs resolved to a placeholder: bind the oracle's
    merge_augs.nms = orc.nms
    cfg = Config.fromfile(REF_CFG)
    m = build_detector(_mmcv_shim.ConfigDict.wrap(copy.deepcopy(cfg.model.to_dict())))
    m.load_state_dict(util.seeded_state_dict(m, seed=10))
    m.eval()
    imgs, img_metas = tta_util.tta_inputs()
    rc = m.roi_head.test_cfg
    d = dict(score_thr=np.float32(rc.score_thr))
    with torch.no_grad():
        for b in range(imgs[0].shape[0]):
            im1, me1 = tta_util.single(imgs, img_metas, b)
            x = m.extract_feats(im1)
            for a, (xa, ma) in enumerate(zip(x, me1)):
                d[f'props{a}_{b}'] = m.rpn_head.simple_test_rpn(xa, ma)[0]
            merged = m.rpn_head.aug_test_rpn(x, me1)[0]
            d[f'merged_{b}'] = merged
            raw_b, raw_s, fus_b, fus_s = [], [], [], []
            for a, (xa, ma) in enumerate(zip(x, me1)):
                meta = ma[0]
                boxes = bbox_mapping(merged[:, :4], meta['img_shape'], meta['scale_factor'], meta['flip'],
                                     meta['flip_direction'])
                rois = bbox2roi([boxes])
                res = m.roi_head._bbox_forward(xa, rois)
                d[f'cls{a}_{b}'], d[f'reg{a}_{b}'] = res['cls_score'], res['bbox_pred']
                fused = (res['cls_score'].softmax(1) * merged[:, -1].reshape(-1, 1)) ** 0.5     # prob_roi_head.py:232-240
                for scores, bl, sl in ((res['cls_score'], raw_b, raw_s), (fused, fus_b, fus_s)):
                    bb, ss = m.roi_head.bbox_head.get_bboxes(rois, scores, res['bbox_pred'], meta['img_shape'],
                                                             meta['scale_factor'], rescale=False, cfg=None)
                    bl.append(bb)
                    sl.append(ss)
            for name, bl, sl in (('raw', raw_b, raw_s), ('fused', fus_b, fus_s)):
                mb, ms = merge_aug_bboxes(bl, sl, me1, rc)
                det, lab = multiclass_nms(mb, ms, rc.score_thr, rc.nms, rc.max_per_img)
                d[f'{name}_bboxes_{b}'], d[f'{name}_scores_{b}'] = mb, ms
                d[f'{name}_det_{b}'], d[f'{name}_lab_{b}'] = det, lab
                cand = ms[:, :-1].reshape(-1)
                print(f'image {b} {name}: {int((cand > rc.score_thr).sum())} candidates above score_thr, {len(det)} '
                      f'detections, closest score to the threshold {float((cand - rc.score_thr).abs().min()):.2e}')
            # the reference's own forward_test (mode raw), both rescale values: per class (k, 5)
            for rescale in (True, False):
                metas = [[dict(mm) for mm in ma] for ma in me1]
                res = m.forward_test([t.clone() for t in im1], metas, rescale=rescale)[0]
                for c, r in enumerate(res):
                    d[f'ref_res{int(rescale)}_{b}_{c}'] = np.asarray(r, dtype=np.float32)
            cand = torch.cat([d[f'props{a}_{b}'] for a in range(len(x))])
            print(f'image {b}: {len(cand)} candidate proposals ({len(torch.unique(cand[:, 4]))} distinct scores), '
                  f'{len(merged)} merged ({len(torch.unique(merged[:, 4]))} distinct scores)')
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in d.items()}
    path = os.path.join(HERE, 'g24_tta.npz')
    np.savez_compressed(path, **out)
    print(f'g24_tta.npz  {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    main()
