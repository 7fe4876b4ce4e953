"""not-gpu: the host side of the device COCO evaluator (brcnn.evaluation.pack_ground_truth / pack_detections) against the
host COCOeval's own tables, the tie order the device sort has to reproduce, and the `backend` keyword of
CocoDataset.evaluate without a device."""
import json
import sys

import numpy as np
import pytest

import brcnn  # noqa: F401
from brcnn.evaluation import COCOeval, pack_detections, pack_ground_truth
from tests.eval_device_util import assert_not_vacuous, host_eval, make_set, same_dict


def _packed(gt, results, img_ids, cat_ids, use_cats, max_det):
    g = pack_ground_truth(gt, img_ids, cat_ids, use_cats)
    d = pack_detections(results, img_ids, cat_ids, g['img_ids'], g['cat_ids'], use_cats, max_det)
    return g, d


@pytest.mark.parametrize('use_cats,proposals', [(1, False), (0, False), (0, True)])
def test_packing_equals_the_host_tables(use_cats, proposals):
    """pair table, in-pair order, fp64 xywh / area / score / ignore flags: bit for bit what COCOeval._prepare +
    computeIoU see (xyxy2xywh + loadRes values)"""
    gt, results, img_ids, cat_ids = make_set(5, 48, 6, proposals=proposals, max_det=100)
    ev = host_eval(gt, results, img_ids, cat_ids, use_cats=use_cats)
    assert_not_vacuous(ev, img_ids, cat_ids)
    p = ev.params
    g, d = _packed(gt, results, img_ids, cat_ids, use_cats, p.maxDets[-1])
    assert list(g['img_ids']) == list(p.imgIds) and (not use_cats or list(g['cat_ids']) == list(p.catIds))
    I = len(p.imgIds)
    det64 = d['det'].astype(np.float64)
    seen = 0
    for k, c in enumerate(p.catIds if use_cats else [-1]):
        for i, img in enumerate(p.imgIds):
            hg, hd = ev._of(ev._gts, img, c), ev._of(ev._dts, img, c)
            hd = [hd[j] for j in np.argsort([-x['score'] for x in hd], kind='mergesort')][:p.maxDets[-1]]
            pair = k * I + i
            g0, g1, d0, d1 = g['off'][pair], g['off'][pair + 1], d['off'][pair], d['off'][pair + 1]
            assert g1 - g0 == len(hg) and d1 - d0 == len(hd), (k, i)
            seen += len(hd)
            if hg:
                assert np.array_equal(g['box'][g0:g1], np.array([x['bbox'] for x in hg], dtype=np.float64))
                assert np.array_equal(g['area'][g0:g1], np.array([x['area'] for x in hg], dtype=np.float64))
                assert list(g['ids'][g0:g1]) == [x['id'] for x in hg]
                assert list(g['flags'][g0:g1] & 1) == [x['ignore'] for x in hg]
                assert list(g['flags'][g0:g1] >> 1) == [int(bool(x['id'])) for x in hg]
            if hd:
                assert list(d['src'][d0:d1] + 1) == [x['id'] for x in hd], (k, i)        # loadRes ids: row + 1
                x, y = det64[d0:d1, 0], det64[d0:d1, 1]
                w, h = det64[d0:d1, 2] - x, det64[d0:d1, 3] - y         # what the kernel computes from the fp32 rows
                assert np.array_equal(np.stack([x, y, w, h], 1), np.array([v['bbox'] for v in hd]))
                assert np.array_equal(w * h, np.array([v['area'] for v in hd]))
                assert np.array_equal(det64[d0:d1, 4], np.array([v['score'] for v in hd]))
    assert seen == len(d['det']) > 0 and d['num_results'] == sum(len(b) for r in results for b in (r if isinstance(r, list) else [r]))


def test_tie_order_of_the_category_sort():
    """the order the device sort must produce -- a stable sort of the pair-major table by (category, score bits flipped
    for an ascending sort) -- is the host's: np.argsort(-dtScores, kind='mergesort') over the concatenation of the images'
    records in sorted image order, for every maxDet"""
    gt, results, img_ids, cat_ids = make_set(6, 48, 6)
    ev = host_eval(gt, results, img_ids, cat_ids)
    p = ev.params
    g, d = _packed(gt, results, img_ids, cat_ids, 1, p.maxDets[-1])
    I, A = len(p.imgIds), len(p.areaRng)
    pair = np.repeat(np.arange(len(d['off']) - 1), np.diff(d['off']))
    rank = np.arange(len(pair)) - d['off'][pair]
    bits = (d['det'][:, 4] + np.float32(0)).view(np.uint32).astype(np.uint64)
    flip = np.where(bits & 0x80000000, 0xFFFFFFFF, 0x80000000).astype(np.uint64)
    key = ((pair // I).astype(np.uint64) << np.uint64(32)) | ((bits ^ flip) ^ np.uint64(0xFFFFFFFF))
    order = np.argsort(key, kind='stable')
    ties = 0
    for k in range(len(p.catIds)):
        E = [e for e in ev.evalImgs[k * A * I:k * A * I + I] if e is not None]
        mine = order[(pair[order] // I) == k]
        for max_det in p.maxDets:
            sc = np.concatenate([e['dtScores'][:max_det] for e in E]) if E else np.zeros(0)
            ids = np.concatenate([e['dtIds'][:max_det] for e in E]) if E else np.zeros(0)
            by = np.argsort(-sc, kind='mergesort')
            sub = mine[rank[mine] < max_det]
            assert list(d['src'][sub] + 1) == list(ids[by].astype(np.int64)), (k, max_det)
            ties += len(sc) - len(set(sc.tolist()))
    assert ties > 0


def test_packing_creates_no_object_per_detection():
    """a condition, not a timing: packing 5 000 images x 80 classes makes the same, small number of Python-level and
    builtin calls whether the images hold 100 or 200 detections each, and returns arrays"""
    rng = np.random.RandomState(0)
    img_ids, cat_ids = np.arange(5000) * 2 + 1, np.arange(80) + 1

    def results(per_img):
        none, out = np.zeros((0, 5), np.float32), []
        for _ in range(5000):
            per = [none] * 80
            for c in rng.choice(80, 4, replace=False):
                per[c] = rng.rand(per_img // 4, 5).astype(np.float32)
            out.append(per)
        return out

    def calls(res):
        n = [0]

        def prof(frame, event, arg):
            if event in ('call', 'c_call'):
                n[0] += 1
        sys.setprofile(prof)
        try:
            d = pack_detections(res, img_ids, cat_ids, img_ids, cat_ids, 1, 100)
        finally:
            sys.setprofile(None)
        return n[0], d
    n1, d1 = calls(results(100))
    n2, d2 = calls(results(200))
    assert n1 == n2 and n1 < 500, (n1, n2)
    assert all(isinstance(v, np.ndarray) for v in (d1['det'], d1['off'], d1['src']))
    assert len(d1['det']) == 5000 * 100 and d1['det'].dtype == np.float32 and len(d2['det']) == 5000 * 200


def _dataset(tmp_path, seed=7, **kw):
    from brcnn.datasets import CocoDataset
    gt, results, img_ids, cat_ids = make_set(seed, 24, 5, **kw)
    path = tmp_path / 'ann.json'
    path.write_text(json.dumps(gt.dataset))
    ds = CocoDataset(ann_file=str(path), pipeline=[], classes=tuple(f'c{c}' for c in cat_ids), test_mode=True)
    assert ds.cat_ids == cat_ids and ds.img_ids == img_ids
    return ds, results


def test_backend_keyword_without_a_device(tmp_path, monkeypatch):
    import torch
    ds, results = _dataset(tmp_path)
    want = ds.evaluate(results, metric=['bbox', 'proposal'], classwise=True)
    assert same_dict(ds.evaluate(results, metric=['bbox', 'proposal'], classwise=True, backend='host'), want)
    ev = host_eval(ds.coco, results, ds.img_ids, ds.cat_ids, max_dets=(100, 300, 1000))
    assert want['bbox_mAP'] == float(f'{ev.stats[0]:.3f}') and want['bbox_mAP_copypaste'] == ' '.join(f'{v:.3f}' for v in ev.stats[:6])
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ds.evaluate(results, metric='bbox', backend='device')
    with pytest.raises(ValueError):
        ds.evaluate(results, metric='bbox', backend='gpu')
    assert ds.evaluate([np.concatenate(r) for r in results], metric='proposal_fast', backend='device').keys() == {'AR@100', 'AR@300', 'AR@1000'}
