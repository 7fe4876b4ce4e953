"""Result sink: COCO bbox mAP without pycocotools.

The reference's `CocoDataset.evaluate` (mmdet/datasets/coco.py:362-560) hands detections to
pycocotools' `COCOeval` (third party, absent here; the published algorithm of
pycocotools/cocoeval.py, bbox branch, is restated): per (image, category) IoU matrix with
crowd handling, greedy matching by descending score at 10 IoU thresholds x 4 area ranges,
precision envelopes sampled at 101 recall points, the 12 summary statistics.
PARITY UNPINNED against pycocotools itself (not installed); pinned by known-answer cases
(tests/test_eval_cpu.py) derived by hand from the algorithm: IoU thresholds, the 101-point envelope,
crowd regions absorbing detections, `ignore` following `iscrowd`, maxDets truncation, area ranges
inclusive at exactly 32^2 and 96^2.
"""
from collections import defaultdict

import numpy as np


class Params:
    def __init__(self):
        self.imgIds, self.catIds = [], []
        self.iouThrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
        self.recThrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
        self.maxDets = [1, 10, 100]
        self.areaRng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
        self.areaRngLbl = ['all', 'small', 'medium', 'large']
        self.useCats = 1


def bbox_iou_xywh(dt, gt, iscrowd):
    """(D,G) IoU of xywh boxes; a crowd ground truth divides by the detection's area"""
    dt = np.asarray(dt, dtype=np.float64).reshape(-1, 4)
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 4)
    if len(dt) == 0 or len(gt) == 0:
        return np.zeros((len(dt), len(gt)))
    da = dt[:, 2] * dt[:, 3]
    ga = gt[:, 2] * gt[:, 3]
    w = np.minimum(dt[:, None, 0] + dt[:, None, 2], gt[None, :, 0] + gt[None, :, 2]) - \
        np.maximum(dt[:, None, 0], gt[None, :, 0])
    h = np.minimum(dt[:, None, 1] + dt[:, None, 3], gt[None, :, 1] + gt[None, :, 3]) - \
        np.maximum(dt[:, None, 1], gt[None, :, 1])
    inter = np.where((w > 0) & (h > 0), w * h, 0.0)
    crowd = np.asarray(iscrowd, dtype=bool)[None, :]
    union = np.where(crowd, da[:, None], da[:, None] + ga[None, :] - inter)
    with np.errstate(divide='ignore', invalid='ignore'):
        out = np.where(inter > 0, inter / union, 0.0)
    return out


class COCOeval:
    def __init__(self, cocoGt, cocoDt, iouType='bbox'):
        assert iouType == 'bbox'
        self.cocoGt, self.cocoDt = cocoGt, cocoDt
        self.params = Params()
        self.params.imgIds = sorted(cocoGt.get_img_ids())
        self.params.catIds = sorted(cocoGt.get_cat_ids())
        self.evalImgs, self.eval, self.stats = [], {}, []

    def _prepare(self):
        p = self.params
        img_set, cat_set = set(p.imgIds), set(p.catIds)
        # useCats == 0 (the 'proposal' metric): every annotation of the images, whatever its category
        gts = [a for i in p.imgIds for a in self.cocoGt.imgToAnns.get(i, []) if not p.useCats or a['category_id'] in cat_set]
        dts = [a for i in p.imgIds for a in self.cocoDt.imgToAnns.get(i, []) if not p.useCats or a['category_id'] in cat_set]
        self._gts, self._dts = defaultdict(list), defaultdict(list)
        for g in gts:
            g['ignore'] = 1 if ('iscrowd' in g and g['iscrowd']) else 0
            self._gts[g['image_id'], g['category_id']].append(g)
        for d in dts:
            if d['image_id'] in img_set:
                self._dts[d['image_id'], d['category_id']].append(d)

    def _of(self, table, imgId, catId):
        """the image's boxes of one category, or (useCats == 0, catId -1) of all categories in category order"""
        if self.params.useCats:
            return table[imgId, catId]
        return [a for c in self.params.catIds for a in table[imgId, c]]

    def computeIoU(self, imgId, catId):
        gt, dt = self._of(self._gts, imgId, catId), self._of(self._dts, imgId, catId)
        if len(gt) == 0 and len(dt) == 0:
            return []
        inds = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in inds][:self.params.maxDets[-1]]
        return bbox_iou_xywh([d['bbox'] for d in dt], [g['bbox'] for g in gt], [int(g['iscrowd']) for g in gt])

    def evaluateImg(self, imgId, catId, aRng, maxDet):
        p = self.params
        gt, dt = self._of(self._gts, imgId, catId), self._of(self._dts, imgId, catId)
        if len(gt) == 0 and len(dt) == 0:
            return None
        ig = [1 if (g['ignore'] or g['area'] < aRng[0] or g['area'] > aRng[1]) else 0 for g in gt]
        gtind = np.argsort(ig, kind='mergesort')
        gt = [gt[i] for i in gtind]
        dtind = np.argsort([-d['score'] for d in dt], kind='mergesort')
        dt = [dt[i] for i in dtind[:maxDet]]
        iscrowd = [int(g['iscrowd']) for g in gt]
        ious = self.ious[imgId, catId]
        ious = ious[:, gtind] if len(ious) > 0 else ious
        T, G, D = len(p.iouThrs), len(gt), len(dt)
        gtm, dtm = np.zeros((T, G)), np.zeros((T, D))
        gtIg = np.array([ig[i] for i in gtind])
        dtIg = np.zeros((T, D))
        if len(ious) != 0:
            for tind, t in enumerate(p.iouThrs):
                for dind, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gind in range(G):
                        if gtm[tind, gind] > 0 and not iscrowd[gind]:
                            continue
                        if m > -1 and gtIg[m] == 0 and gtIg[gind] == 1:
                            break
                        if ious[dind, gind] < iou:
                            continue
                        iou = ious[dind, gind]
                        m = gind
                    if m == -1:
                        continue
                    dtIg[tind, dind] = gtIg[m]
                    dtm[tind, dind] = gt[m]['id']
                    gtm[tind, m] = d['id']
        a = np.array([d['area'] < aRng[0] or d['area'] > aRng[1] for d in dt]).reshape((1, len(dt)))
        dtIg = np.logical_or(dtIg, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return dict(image_id=imgId, category_id=catId, aRng=aRng, maxDet=maxDet,
                    dtIds=[d['id'] for d in dt], gtIds=[g['id'] for g in gt], dtMatches=dtm, gtMatches=gtm,
                    dtScores=[d['score'] for d in dt], gtIgnore=gtIg, dtIgnore=dtIg)

    def evaluate(self):
        p = self.params
        p.imgIds = list(np.unique(p.imgIds))
        if p.useCats:
            p.catIds = list(np.unique(p.catIds))
        p.maxDets = sorted(p.maxDets)
        self._prepare()
        cats = p.catIds if p.useCats else [-1]
        self.ious = {(i, c): self.computeIoU(i, c) for i in p.imgIds for c in cats}
        maxDet = p.maxDets[-1]
        self.evalImgs = [self.evaluateImg(i, c, a, maxDet) for c in cats for a in p.areaRng for i in p.imgIds]

    def accumulate(self):
        p = self.params
        T, R, K, A, M = len(p.iouThrs), len(p.recThrs), len(p.catIds) if p.useCats else 1, len(p.areaRng), len(p.maxDets)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        scores = -np.ones((T, R, K, A, M))
        I0 = len(p.imgIds)
        for k in range(K):
            for a in range(A):
                base = k * A * I0 + a * I0
                E = [e for e in self.evalImgs[base:base + I0] if e is not None]
                if len(E) == 0:
                    continue
                for m, maxDet in enumerate(p.maxDets):
                    dtScores = np.concatenate([e['dtScores'][0:maxDet] for e in E])
                    inds = np.argsort(-dtScores, kind='mergesort')
                    dtScoresSorted = dtScores[inds]
                    dtm = np.concatenate([e['dtMatches'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    dtIg = np.concatenate([e['dtIgnore'][:, 0:maxDet] for e in E], axis=1)[:, inds]
                    gtIg = np.concatenate([e['gtIgnore'] for e in E])
                    npig = np.count_nonzero(gtIg == 0)
                    if npig == 0:
                        continue
                    tps = np.logical_and(dtm, np.logical_not(dtIg))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtIg))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        q, ss = np.zeros((R,)), np.zeros((R,))
                        recall[t, k, a, m] = rc[-1] if nd else 0
                        pr = pr.tolist()
                        for i in range(nd - 1, 0, -1):
                            if pr[i] > pr[i - 1]:
                                pr[i - 1] = pr[i]
                        idx = np.searchsorted(rc, p.recThrs, side='left')
                        for ri, pi in enumerate(idx):
                            if pi >= nd:
                                break
                            q[ri] = pr[pi]
                            ss[ri] = dtScoresSorted[pi]
                        precision[t, :, k, a, m] = q
                        scores[t, :, k, a, m] = ss
        self.eval = dict(params=p, counts=[T, R, K, A, M], precision=precision, recall=recall, scores=scores)

    def _summarize(self, ap=1, iouThr=None, areaRng='all', maxDets=100):
        p = self.params
        aind = [i for i, a in enumerate(p.areaRngLbl) if a == areaRng]
        mind = [i for i, m in enumerate(p.maxDets) if m == maxDets]
        if ap == 1:
            s = self.eval['precision']
            if iouThr is not None:
                s = s[np.where(np.isclose(iouThr, p.iouThrs))[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = self.eval['recall']
            if iouThr is not None:
                s = s[np.where(np.isclose(iouThr, p.iouThrs))[0]]
            s = s[:, :, aind, mind]
        mean_s = -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
        title = 'Average Precision' if ap == 1 else 'Average Recall'
        typ = '(AP)' if ap == 1 else '(AR)'
        iou = f'{p.iouThrs[0]:0.2f}:{p.iouThrs[-1]:0.2f}' if iouThr is None else f'{iouThr:0.2f}'
        line = f' {title:<18} {typ} @[ IoU={iou:<9} | area={areaRng:>6s} | maxDets={maxDets:>3d} ] = {mean_s:0.3f}'
        return mean_s, line

    def summarize(self):
        if not self.eval:
            raise Exception('Please run accumulate() first')
        md = self.params.maxDets
        spec = [(1, None, 'all', md[2]), (1, .5, 'all', md[2]), (1, .75, 'all', md[2]),
                (1, None, 'small', md[2]), (1, None, 'medium', md[2]), (1, None, 'large', md[2]),
                (0, None, 'all', md[0]), (0, None, 'all', md[1]), (0, None, 'all', md[2]),
                (0, None, 'small', md[2]), (0, None, 'medium', md[2]), (0, None, 'large', md[2])]
        stats, lines = np.zeros((12,)), []
        for i, (ap, thr, rng, m) in enumerate(spec):
            stats[i], line = self._summarize(ap, thr, rng, m)
            lines.append(line)
        self.stats = stats
        return '\n'.join(lines)


# ------------------------------------------------------------------------------------------
# PASCAL VOC style mAP (mmdet/core/evaluation/mean_ap.py: average_precision:13-60,
# tpfp_default:159-267, get_cls_results:270-294, eval_map:297-420), as `VOCDataset.evaluate`
# calls it (datasets/voc.py:60-76: iou_thr 0.5, legacy +1 box extents, 11-point AP for VOC2007).
# The reference is importable here, so this part is pinned by a golden fixture (g15).
# ------------------------------------------------------------------------------------------
def bbox_overlaps_np(bboxes1, bboxes2, mode='iou', eps=1e-6, use_legacy_coordinate=False):
    """core/evaluation/bbox_overlaps.py:5-65"""
    assert mode in ('iou', 'iof')
    extra = 1. if use_legacy_coordinate else 0.
    bboxes1 = bboxes1.astype(np.float32)
    bboxes2 = bboxes2.astype(np.float32)
    rows, cols = bboxes1.shape[0], bboxes2.shape[0]
    ious = np.zeros((rows, cols), dtype=np.float32)
    if rows * cols == 0:
        return ious
    exchange = False
    if bboxes1.shape[0] > bboxes2.shape[0]:
        bboxes1, bboxes2 = bboxes2, bboxes1
        ious = np.zeros((cols, rows), dtype=np.float32)
        exchange = True
    area1 = (bboxes1[:, 2] - bboxes1[:, 0] + extra) * (bboxes1[:, 3] - bboxes1[:, 1] + extra)
    area2 = (bboxes2[:, 2] - bboxes2[:, 0] + extra) * (bboxes2[:, 3] - bboxes2[:, 1] + extra)
    for i in range(bboxes1.shape[0]):
        x_start = np.maximum(bboxes1[i, 0], bboxes2[:, 0])
        y_start = np.maximum(bboxes1[i, 1], bboxes2[:, 1])
        x_end = np.minimum(bboxes1[i, 2], bboxes2[:, 2])
        y_end = np.minimum(bboxes1[i, 3], bboxes2[:, 3])
        overlap = np.maximum(x_end - x_start + extra, 0) * np.maximum(y_end - y_start + extra, 0)
        union = area1[i] + area2 - overlap if mode == 'iou' else (area1[i] if not exchange else area2)
        union = np.maximum(union, eps)
        ious[i, :] = overlap / union
    return ious.T if exchange else ious


def average_precision(recalls, precisions, mode='area'):
    no_scale = recalls.ndim == 1
    if no_scale:
        recalls, precisions = recalls[np.newaxis, :], precisions[np.newaxis, :]
    assert recalls.shape == precisions.shape and recalls.ndim == 2
    num_scales = recalls.shape[0]
    ap = np.zeros(num_scales, dtype=np.float32)
    if mode == 'area':
        zeros = np.zeros((num_scales, 1), dtype=recalls.dtype)
        ones = np.ones((num_scales, 1), dtype=recalls.dtype)
        mrec = np.hstack((zeros, recalls, ones))
        mpre = np.hstack((zeros, precisions, zeros))
        for i in range(mpre.shape[1] - 1, 0, -1):
            mpre[:, i - 1] = np.maximum(mpre[:, i - 1], mpre[:, i])
        for i in range(num_scales):
            ind = np.where(mrec[i, 1:] != mrec[i, :-1])[0]
            ap[i] = np.sum((mrec[i, ind + 1] - mrec[i, ind]) * mpre[i, ind + 1])
    elif mode == '11points':
        for i in range(num_scales):
            for thr in np.arange(0, 1 + 1e-3, 0.1):
                precs = precisions[i, recalls[i, :] >= thr]
                ap[i] += precs.max() if precs.size > 0 else 0
        ap /= 11
    else:
        raise ValueError('Unrecognized mode, only "area" and "11points" are supported')
    return ap[0] if no_scale else ap


def tpfp_default(det_bboxes, gt_bboxes, gt_bboxes_ignore=None, iou_thr=0.5, area_ranges=None,
                 use_legacy_coordinate=False):
    extra = 1. if use_legacy_coordinate else 0.
    gt_ignore_inds = np.concatenate((np.zeros(gt_bboxes.shape[0], dtype=bool),
                                     np.ones(gt_bboxes_ignore.shape[0], dtype=bool)))
    gt_bboxes = np.vstack((gt_bboxes, gt_bboxes_ignore))
    num_dets, num_gts = det_bboxes.shape[0], gt_bboxes.shape[0]
    if area_ranges is None:
        area_ranges = [(None, None)]
    tp = np.zeros((len(area_ranges), num_dets), dtype=np.float32)
    fp = np.zeros((len(area_ranges), num_dets), dtype=np.float32)
    if gt_bboxes.shape[0] == 0:
        if area_ranges == [(None, None)]:
            fp[...] = 1
        else:
            det_areas = (det_bboxes[:, 2] - det_bboxes[:, 0] + extra) * (det_bboxes[:, 3] - det_bboxes[:, 1] + extra)
            for i, (lo, hi) in enumerate(area_ranges):
                fp[i, (det_areas >= lo) & (det_areas < hi)] = 1
        return tp, fp
    ious = bbox_overlaps_np(det_bboxes, gt_bboxes, use_legacy_coordinate=use_legacy_coordinate)
    ious_max, ious_argmax = ious.max(axis=1), ious.argmax(axis=1)
    sort_inds = np.argsort(-det_bboxes[:, -1])
    for k, (lo, hi) in enumerate(area_ranges):
        gt_covered = np.zeros(num_gts, dtype=bool)
        if lo is None:
            gt_area_ignore = np.zeros_like(gt_ignore_inds, dtype=bool)
        else:
            gt_areas = (gt_bboxes[:, 2] - gt_bboxes[:, 0] + extra) * (gt_bboxes[:, 3] - gt_bboxes[:, 1] + extra)
            gt_area_ignore = (gt_areas < lo) | (gt_areas >= hi)
        for i in sort_inds:
            if ious_max[i] >= iou_thr:
                m = ious_argmax[i]
                if not (gt_ignore_inds[m] or gt_area_ignore[m]):
                    if not gt_covered[m]:
                        gt_covered[m] = True
                        tp[k, i] = 1
                    else:
                        fp[k, i] = 1
            elif lo is None:
                fp[k, i] = 1
            else:
                b = det_bboxes[i, :4]
                area = (b[2] - b[0] + extra) * (b[3] - b[1] + extra)
                if lo <= area < hi:
                    fp[k, i] = 1
    return tp, fp


def eval_map(det_results, annotations, scale_ranges=None, iou_thr=0.5, dataset=None, logger=None,
             use_legacy_coordinate=False):
    """(mAP, per-class dicts {num_gts, num_dets, recall, precision, ap})"""
    assert len(det_results) == len(annotations)
    extra = 1. if use_legacy_coordinate else 0.
    num_scales = len(scale_ranges) if scale_ranges is not None else 1
    num_classes = len(det_results[0])
    area_ranges = [(r[0] ** 2, r[1] ** 2) for r in scale_ranges] if scale_ranges is not None else None
    eval_results = []
    for c in range(num_classes):
        cls_dets = [img_res[c] for img_res in det_results]
        cls_gts, cls_gts_ignore = [], []
        for ann in annotations:
            cls_gts.append(ann['bboxes'][ann['labels'] == c, :])
            if ann.get('labels_ignore', None) is not None:
                cls_gts_ignore.append(ann['bboxes_ignore'][ann['labels_ignore'] == c, :])
            else:
                cls_gts_ignore.append(np.empty((0, 4), dtype=np.float32))
        tpfp = [tpfp_default(d, g, gi, iou_thr, area_ranges, use_legacy_coordinate)
                for d, g, gi in zip(cls_dets, cls_gts, cls_gts_ignore)]
        tp, fp = tuple(zip(*tpfp))
        num_gts = np.zeros(num_scales, dtype=int)
        for bbox in cls_gts:
            if area_ranges is None:
                num_gts[0] += bbox.shape[0]
            else:
                areas = (bbox[:, 2] - bbox[:, 0] + extra) * (bbox[:, 3] - bbox[:, 1] + extra)
                for k, (lo, hi) in enumerate(area_ranges):
                    num_gts[k] += np.sum((areas >= lo) & (areas < hi))
        cls_dets = np.vstack(cls_dets)
        sort_inds = np.argsort(-cls_dets[:, -1])
        tp = np.cumsum(np.hstack(tp)[:, sort_inds], axis=1)
        fp = np.cumsum(np.hstack(fp)[:, sort_inds], axis=1)
        eps = np.finfo(np.float32).eps
        recalls = tp / np.maximum(num_gts[:, np.newaxis], eps)
        precisions = tp / np.maximum((tp + fp), eps)
        if scale_ranges is None:
            recalls, precisions, n_gt = recalls[0, :], precisions[0, :], num_gts.item()
        else:
            n_gt = num_gts
        ap = average_precision(recalls, precisions, 'area' if dataset != 'voc07' else '11points')
        eval_results.append(dict(num_gts=n_gt, num_dets=cls_dets.shape[0], recall=recalls, precision=precisions, ap=ap))
    if scale_ranges is not None:
        all_ap = np.vstack([r['ap'] for r in eval_results])
        all_gt = np.vstack([r['num_gts'] for r in eval_results])
        mean_ap = [all_ap[all_gt[:, i] > 0, i].mean() if np.any(all_gt[:, i] > 0) else 0.0 for i in range(num_scales)]
    else:
        aps = [r['ap'] for r in eval_results if r['num_gts'] > 0]
        mean_ap = np.array(aps).mean().item() if aps else 0.0
    if logger is not None:
        logger.info(f'mAP@{iou_thr}: {mean_ap}')
    return mean_ap, eval_results



# ------------------------------------------------------------------------------------------
# Proposal recall (mmdet/core/evaluation/recall.py: _recalls:12-44, set_recall_param:47-65, eval_recalls:68-113), the
# 'proposal_fast' metric of CocoDataset.evaluate (datasets/coco.py:311-333,425-434).  The reference is importable here:
# pinned by the golden fixture g22.
# ------------------------------------------------------------------------------------------
def _greedy_gt_ious(ious):
    """the IoU every ground truth ends up with when (gt, proposal) pairs are taken greedily by descending IoU, each
    ground truth and each proposal at most once -- in the order they are taken (rows: ground truths)"""
    ious = np.array(ious, dtype=np.float64)
    g = ious.shape[0]
    out = np.zeros(g)
    if ious.size == 0:
        return out
    for j in range(g):
        # the best remaining proposal of every remaining ground truth, then the best of those (first index on ties)
        best_box = ious.argmax(axis=1)
        best = ious[np.arange(g), best_box]
        gi = int(best.argmax())
        out[j] = best[gi]
        ious[gi, :] = -1
        ious[:, best_box[gi]] = -1
    return out


def eval_recalls(gts, proposals, proposal_nums=None, iou_thrs=0.5, logger=None, use_legacy_coordinate=False):
    """recalls (len(proposal_nums), len(iou_thrs)): the fraction of ground-truth boxes covered at IoU >= thr by the top
    `proposal_num` proposals of their image (descending score when a 5th column carries one), one-to-one greedy matching"""
    assert len(gts) == len(proposals)
    nums = np.array([proposal_nums] if isinstance(proposal_nums, (int, np.integer)) else proposal_nums)
    thrs = np.array([0.5] if iou_thrs is None else
                    ([iou_thrs] if isinstance(iou_thrs, (float, np.floating)) else iou_thrs), dtype=np.float64)
    per_image = []
    for gt, prop in zip(gts, proposals):
        prop = np.asarray(prop)
        if prop.ndim == 2 and prop.shape[1] == 5:
            prop = prop[np.argsort(prop[:, 4])[::-1]]
        keep = min(prop.shape[0], int(nums[-1]))
        if gt is None or len(gt) == 0:
            per_image.append(np.zeros((0, prop.shape[0]), dtype=np.float32))
        else:
            per_image.append(bbox_overlaps_np(np.asarray(gt), prop[:keep, :4], use_legacy_coordinate=use_legacy_coordinate))
    total = sum(m.shape[0] for m in per_image)
    recalls = np.zeros((nums.size, thrs.size))
    for k, n in enumerate(nums):
        covered = np.concatenate([_greedy_gt_ious(m[:, :int(n)]) for m in per_image]) if per_image else np.zeros(0)
        covered = covered.astype(np.float32)            # (the reference collects them in a float32 table)
        for i, t in enumerate(thrs):
            recalls[k, i] = (covered >= t).sum() / float(total) if total else 0.0
    if logger is not None and logger != 'silent' and hasattr(logger, 'info'):
        rows = ['proposals | ' + ' '.join(f'{t:.2f}' for t in thrs)]
        rows += [f'{int(n):9d} | ' + ' '.join(f'{v:.3f}' for v in recalls[k]) for k, n in enumerate(nums)]
        logger.info('\n' + '\n'.join(rows))
    return recalls


# ------------------------------------------------------------------------------------------
# The device back end of COCOeval (csrc/coco_eval.hip: match, order, accumulate).  The host side below is packing only,
# vectorised numpy: one pass over the ground-truth annotations (cached), none over the detections.
# ------------------------------------------------------------------------------------------
MAX_GT_PER_PAIR = 1024      # csrc/coco_eval.hip: CE_MAX_GT
MAX_REC_THRS = 1024         # csrc/coco_eval.hip: CE_MAX_REC


def _eval_ids(img_ids, cat_ids, use_cats):
    """the image / category axes as COCOeval.evaluate fixes them: sorted unique image ids; categories sorted unique, or
    (pooled: useCats == 0) in the order given -- the order `_of` pools a pair's boxes in"""
    img_ids = np.unique(np.asarray(img_ids, dtype=np.int64))
    cats = np.asarray(cat_ids, dtype=np.int64)
    if use_cats:
        cats = np.unique(cats)
    elif len(np.unique(cats)) != len(cats):
        raise ValueError('catIds must not repeat a category')
    return img_ids, cats


def _cat_slots(cats, ids):
    """position of every id of `ids` in `cats` (any order), -1 where absent"""
    ids = np.asarray(ids, dtype=np.int64)
    if len(cats) == 0:
        return np.full(ids.shape, -1, np.int64)
    by = np.argsort(cats, kind='stable')
    at = np.minimum(np.searchsorted(cats[by], ids), len(cats) - 1)
    return np.where(cats[by][at] == ids, by[at], -1)


def pack_ground_truth(cocoGt, img_ids, cat_ids, use_cats=1):
    """The ground truths of (img_ids x cat_ids) as a pair-major table.  pair = category slot * I + image slot (image slot
    alone when categories are pooled); inside a pair the order COCOeval sees: annotation order (pooled: category order
    first).  Returns dict(img_ids, cat_ids, num_cats, box (G, 4) fp64 xywh, area (G,) fp64, flags (G,) uint8 [bit 0
    iscrowd, bit 1 id != 0], ids (G,) int64, off (P + 1,) int32)."""
    img_ids, cats = _eval_ids(img_ids, cat_ids, use_cats)
    slot = {c: n for n, c in enumerate(cats.tolist())}
    rows = [(ii, slot[a['category_id']], a) for ii, i in enumerate(img_ids.tolist())
            for a in cocoGt.imgToAnns.get(i, ()) if a['category_id'] in slot]
    G, I = len(rows), len(img_ids)
    K = len(cats) if use_cats else 1
    ii = np.fromiter((r[0] for r in rows), np.int64, G)
    cs = np.fromiter((r[1] for r in rows), np.int64, G)
    box = np.array([r[2]['bbox'] for r in rows], dtype=np.float64).reshape(G, 4)
    area = np.array([r[2]['area'] for r in rows], dtype=np.float64).reshape(G)
    flags = np.fromiter(((1 if r[2].get('iscrowd', 0) else 0) | (2 if r[2]['id'] else 0) for r in rows), np.uint8, G)
    ids = np.fromiter((r[2]['id'] for r in rows), np.int64, G)
    pair = cs * I + ii if use_cats else ii
    by = np.lexsort((cs, pair))             # stable: annotation order inside (pair, category)
    off = np.zeros(K * I + 1, np.int64)
    np.cumsum(np.bincount(pair, minlength=K * I), out=off[1:])
    return dict(img_ids=img_ids, cat_ids=cats, num_cats=K, use_cats=int(bool(use_cats)), box=np.ascontiguousarray(box[by]),
                area=area[by], flags=flags[by], ids=ids[by], off=off.astype(np.int32))


def pack_detections(results, result_img_ids, label_cat_ids, img_ids, cat_ids, use_cats, max_det):
    """`results` (per image a list of per-class (k, 5) float32 arrays, or one (k, 5) array of proposals = category 1) as
    the pair-major table of the device evaluator: inside a pair by descending score, ties in the order COCOeval's stable
    sort leaves them (pooled: category order, then row; else row), cut to `max_det`.  `img_ids` / `cat_ids` are the axes
    of `_eval_ids`.  No Python object per detection: every step is one numpy call over all of them.
    Returns dict(det (D, 5) float32 xyxy + score, off (P + 1,) int32, src (D,) int64 row in the concatenated results,
    num_results) -- num_results counts the detections before any is dropped."""
    I = len(img_ids)
    K = len(cat_ids) if use_cats else 1
    if len(results) and isinstance(results[0], (list, tuple)):
        L = len(results[0])
        flat = [b for r in results for b in r]
        label_cat_ids = np.asarray(label_cat_ids, dtype=np.int64)
        assert len(label_cat_ids) == L and len(flat) == L * len(results), 'one array per class and image'
    else:
        L, flat, label_cat_ids = 1, list(results), np.array([1], dtype=np.int64)
    counts = np.fromiter(map(len, flat), np.int64, len(flat))
    N = int(counts.sum())
    empty = dict(det=np.zeros((0, 5), np.float32), off=np.zeros(K * I + 1, np.int32), src=np.zeros(0, np.int64), num_results=N)
    if N == 0:
        return empty
    allv = np.concatenate([b for b in flat if len(b)] if N < len(flat) else flat)
    if allv.dtype != np.float32 or allv.ndim != 2 or allv.shape[1] != 5:
        raise TypeError(f'detections must be (k, 5) float32 arrays (got {allv.dtype}, shape {allv.shape})')
    # per slot (image of the results, label): image slot, category slot, whether the evaluation covers it
    res_ids = np.asarray(result_img_ids, dtype=np.int64)
    assert len(res_ids) == len(results), 'one image id per result'
    at = np.minimum(np.searchsorted(img_ids, res_ids), max(I - 1, 0))
    img_slot = np.where(img_ids[at] == res_ids, at, -1) if I else np.full(len(res_ids), -1)
    cat_slot = _cat_slots(np.asarray(cat_ids, dtype=np.int64), label_cat_ids)
    s_img, s_cat = np.repeat(img_slot, L), np.tile(cat_slot, len(results))
    s_ok = (s_img >= 0) & (s_cat >= 0)
    s_pair = s_cat * I + s_img if use_cats else s_img
    ok = np.repeat(s_ok, counts)
    src = np.flatnonzero(ok)
    if len(src) == 0:
        return empty
    pair, cs = np.repeat(s_pair, counts)[src], np.repeat(s_cat, counts)[src]
    neg = -allv[src, 4]
    by = np.lexsort((neg, pair)) if use_cats else np.lexsort((cs, neg, pair))       # (stable)
    n_pair = np.bincount(pair, minlength=K * I)
    start = np.zeros(K * I + 1, np.int64)
    np.cumsum(n_pair, out=start[1:])
    pair = pair[by]
    keep = (np.arange(len(by)) - start[pair]) < max_det
    by = by[keep]
    off = np.zeros(K * I + 1, np.int64)
    np.cumsum(np.minimum(n_pair, max_det), out=off[1:])
    return dict(det=np.ascontiguousarray(allv[src[by]]), off=off.astype(np.int32), src=src[by], num_results=N)


class DeviceCOCOeval(COCOeval):
    """COCOeval with `evaluate` / `accumulate` on the HIP device; `summarize`, `stats`, `eval[...]` are the host class's.
    `results` is what the detectors return (see `pack_detections`); `img_ids[i]` is the image of `results[i]` and
    `cat_ids[l]` the category of label l (defaults: the ground truth's own lists, as CocoDataset uses them).  There are
    no `evalImgs`; `match_records()` gives the same information as flat arrays.  No CPU fallback."""

    def __init__(self, cocoGt, results, img_ids=None, cat_ids=None, device=None, profile=False):
        import torch
        from .lib import BrcnnHipError
        if not torch.cuda.is_available():
            raise BrcnnHipError('DeviceCOCOeval runs on the HIP device only (none is visible); there is no CPU fallback: '
                                "use COCOeval / backend='host'")
        self.cocoGt, self.cocoDt, self.results = cocoGt, None, results
        self.result_img_ids = list(cocoGt.get_img_ids()) if img_ids is None else list(img_ids)
        self.label_cat_ids = list(cocoGt.get_cat_ids()) if cat_ids is None else list(cat_ids)
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.params = Params()
        self.params.imgIds = sorted(cocoGt.get_img_ids())
        self.params.catIds = sorted(cocoGt.get_cat_ids())
        self.evalImgs, self.eval, self.stats = [], {}, []
        self.profile, self.kernel_ms, self._events = profile, {}, []
        self._run = None

    # ---- the cached ground-truth table --------------------------------------------------
    def _ground_truth(self):
        import torch
        p = self.params
        cache = self.cocoGt.__dict__.setdefault('_device_eval_tables', {})
        key = (tuple(int(i) for i in p.imgIds), tuple(int(c) for c in p.catIds), int(bool(p.useCats)), str(self.device))
        if key not in cache:
            host = pack_ground_truth(self.cocoGt, p.imgIds, p.catIds, p.useCats)
            per_pair = np.diff(host['off'])
            if len(per_pair) and per_pair.max() > MAX_GT_PER_PAIR:
                raise ValueError(f'{per_pair.max()} ground truths in one (image, category) pair: the device evaluator '
                                 f'holds at most {MAX_GT_PER_PAIR}')
            f64 = np.concatenate([host['box'].reshape(-1), host['area']])
            dev = dict(f64=torch.from_numpy(f64).to(self.device), flags=torch.from_numpy(host['flags']).to(self.device),
                       off=torch.from_numpy(host['off']).to(self.device))
            cache[key] = dict(host=host, dev=dev, max_gt=int(per_pair.max()) if len(per_pair) else 0)
        return cache[key]

    def _mark(self, name):
        import torch
        if self.profile:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self._events.append((name, e))

    def evaluate(self):
        import torch
        from . import ops
        p = self.params
        p.imgIds = list(np.unique(p.imgIds))
        if p.useCats:
            p.catIds = list(np.unique(p.catIds))
        p.maxDets = sorted(p.maxDets)
        iou = np.ascontiguousarray(p.iouThrs, dtype=np.float64).reshape(-1)
        rec = np.ascontiguousarray(p.recThrs, dtype=np.float64).reshape(-1)
        area = np.ascontiguousarray(p.areaRng, dtype=np.float64).reshape(-1, 2)
        mdets = np.asarray(p.maxDets, dtype=np.int32).reshape(-1)
        T, R, A, M = len(iou), len(rec), len(area), len(mdets)
        if not (1 <= T <= 16 and 1 <= A <= 8 and T * A <= 64 and 1 <= R <= MAX_REC_THRS and M >= 1):
            raise ValueError(f'device evaluator: {T} IoU thresholds (1..16), {A} area ranges (T * A <= 64), {R} recall '
                             f'points (1..{MAX_REC_THRS})')
        if np.any(np.diff(rec) < 0):
            raise ValueError('recThrs must be ascending')
        gt = self._ground_truth()
        host = gt['host']
        I, K = len(host['img_ids']), host['num_cats']
        if I == 0 or (p.useCats and len(host['cat_ids']) == 0):
            raise ValueError('nothing to evaluate: no image or no category')
        dt = pack_detections(self.results, self.result_img_ids, self.label_cat_ids, host['img_ids'], host['cat_ids'],
                             p.useCats, int(mdets[-1]))
        D, G = len(dt['det']), len(host['area'])
        assert dt['off'][-1] == D and np.all(np.diff(dt['off']) >= 0) and host['off'][-1] == G
        # one upload: thresholds, recall points, area ranges | maxDets, detection offsets | detections
        head = np.concatenate([iou, rec, area.reshape(-1)])
        ints = np.concatenate([mdets, dt['off']])
        ints = np.concatenate([ints, np.zeros(len(ints) % 2, np.int32)])
        blob = np.concatenate([head.view(np.uint8), ints.view(np.uint8), dt['det'].reshape(-1).view(np.uint8)])
        with torch.cuda.device(self.device):
            self._events = []
            self._mark('start')
            buf = torch.from_numpy(blob).pin_memory().to(self.device, non_blocking=True)
            nh, ni = head.size * 8, ints.size * 4
            f64, i32 = buf[:nh].view(torch.float64), buf[nh:nh + ni].view(torch.int32)
            det = buf[nh + ni:].view(torch.float32).view(-1, 5)
            d_iou, d_rec, d_area = f64[:T], f64[T:T + R], f64[T + R:]
            d_mdets, d_off = i32[:M], i32[M:M + K * I + 1]
            g = gt['dev']
            self._mark('upload')
            dtm, dtig, gtig, num_gt, rank, key = ops.coco_match(g['f64'][:4 * G], g['f64'][4 * G:], g['flags'], g['off'], det, d_off,
                                                                K, I, d_iou, d_area, gt['max_gt'])
            self._mark('match')
            order = ops.coco_order(key, K)
            self._mark('order')
        self._run = dict(T=T, R=R, K=K, A=A, M=M, I=I, det=det, off=d_off, rec=d_rec, mdets=d_mdets, dtm=dtm, dtig=dtig, gtig=gtig,
                         num_gt=num_gt, rank=rank, order=order, packed=dt, gt=gt, buf=buf)

    def accumulate(self):
        import torch
        from . import ops
        r = self._run
        if r is None:
            raise Exception('Please run evaluate() first')
        T, R, K, A, M = r['T'], r['R'], r['K'], r['A'], r['M']
        with torch.cuda.device(self.device):
            out = torch.empty(2 * T * R * K * A * M + T * K * A * M, dtype=torch.float64, device=self.device)
            ops.coco_accumulate(r['order'], r['off'], r['I'], r['det'], r['rank'], r['dtm'], r['dtig'], r['num_gt'], r['rec'],
                                r['mdets'], T, out)
            self._mark('accumulate')
            host = out.cpu().numpy()            # the one copy back, the one synchronisation
        n5 = T * R * K * A * M
        self.eval = dict(params=self.params, counts=[T, R, K, A, M], precision=host[:n5].reshape(T, R, K, A, M),
                         recall=host[2 * n5:].reshape(T, K, A, M), scores=host[n5:2 * n5].reshape(T, R, K, A, M))
        if self.profile:
            self.kernel_ms = {n: self._events[i - 1][1].elapsed_time(e) for i, (n, e) in enumerate(self._events) if i}

    def match_records(self):
        """what `evalImgs` holds on the host, as flat arrays (pairs are dense: pair = category slot * I + image slot):
        pair_cat / pair_img (slots of every non-empty pair), det_off / gt_off (P + 1,), dt_matched / dt_ignored (D, A)
        uint16 with bit t = IoU threshold t, dt_scores (D,), dt_src (D,) row in the concatenated results, gt_ignored (G,)
        uint8 with bit a = area range a, gt_ids (G,), num_gt (K, A)"""
        r = self._run
        if r is None:
            raise Exception('Please run evaluate() first')
        host, dt = r['gt']['host'], r['packed']
        pairs = np.flatnonzero((np.diff(host['off']) > 0) | (np.diff(dt['off']) > 0))
        return dict(pair_cat=pairs // r['I'], pair_img=pairs % r['I'], det_off=dt['off'], gt_off=host['off'],
                    dt_matched=r['dtm'].cpu().numpy().view(np.uint16), dt_ignored=r['dtig'].cpu().numpy().view(np.uint16),
                    dt_scores=dt['det'][:, 4].copy(), dt_src=dt['src'], gt_ignored=r['gtig'].cpu().numpy(),
                    gt_ids=host['ids'], num_gt=r['num_gt'].cpu().numpy())
