"""Seeded synthetic data sets for the device COCO evaluator's tests (tests/test_eval_device_*.py) and the checks that
make them worth running: every condition `assert_not_vacuous` names is read from the HOST evaluator's own records."""
import numpy as np

from brcnn.datasets import COCO
from brcnn.evaluation import COCOeval


def make_set(seed, n_img, n_cat, gts_per_img=7, dets_per_img=100, dense_every=0, proposals=False, max_det=100):
    """-> (COCO ground truth, results, img_ids in data-set order, cat_ids in label order).  Categories: the last label has
    no ground truth anywhere, the one before it no detection.  Scores are float32 rounded to two decimals."""
    rng = np.random.RandomState(seed)
    img_ids = (rng.permutation(n_img) * 3 + 11).tolist()               # neither sorted nor contiguous
    cat_ids = (rng.permutation(n_cat) * 2 + 1).tolist()                # label l -> cat_ids[l]: odd ids, shuffled
    no_gt, no_dt = n_cat - 1, n_cat - 2
    anns, results = [], []

    def add(img, label, box, crowd=0, area=None):
        anns.append(dict(id=len(anns), image_id=img, category_id=cat_ids[label], bbox=[float(v) for v in box],
                         area=float(box[2] * box[3] if area is None else area), iscrowd=crowd))     # (the first id is 0)

    for n, img in enumerate(img_ids):
        per = [[] for _ in range(n_cat)]
        ng = gts_per_img if not (dense_every and n % dense_every == 0) else 34
        ng = rng.randint(max(1, ng - 3), ng + 4)
        nd = dets_per_img
        if n == 1:
            ng = 0                                                      # detections, no ground truth
        if n == 2:
            nd = 0                                                      # ground truths, no detection
        first = len(anns)
        for _ in range(ng):
            label = int(rng.randint(0, n_cat - 1))                      # (never `no_gt`)
            wh = np.round(np.exp(rng.uniform(np.log(6), np.log(220), 2)) * 4) / 4
            xy = np.round(rng.uniform(0, 400, 2) * 4) / 4
            add(img, label, [xy[0], xy[1], wh[0], wh[1]], crowd=int(rng.rand() < 0.05),
                area=wh[0] * wh[1] * (1.0 if rng.rand() < 0.5 else 0.75))
        if n % 16 == 0 and nd:                                          # by construction, far from the random boxes:
            lab = 0
            add(img, lab, [1000, 0, 2, 1]); add(img, lab, [1000, 50, 4, 1])             # IoU exactly .5 and .75 below
            add(img, lab, [1100, 0, 32, 32]); add(img, lab, [1200, 0, 96, 96])          # areas on the range edges
            add(img, lab, [1400, 0, 200, 200], crowd=1)                                 # a crowd that takes several
            per[lab] += [[1000, 0, 1001, 1, .9], [1000, 50, 1003, 51, .9], [1100, 0, 1132, 32, .8], [1200, 0, 1296, 96, .8],
                         [1410, 10, 1440, 40, .7], [1450, 50, 1480, 80, .7], [1500, 100, 1530, 130, .6]]
        here = anns[first:]
        for _ in range(nd):
            if here and rng.rand() < 0.6:                               # a jittered copy of a ground truth
                g = here[rng.randint(len(here))]
                x, y, w, h = g['bbox']
                j = rng.normal(0, 0.12, 4) * [w, h, w, h]
                box = [x + j[0], y + j[1], x + w + j[2], y + h + j[3]]
                label = cat_ids.index(g['category_id']) if rng.rand() < 0.8 else int(rng.randint(n_cat))
            else:
                wh = np.exp(rng.uniform(np.log(6), np.log(220), 2))
                xy = rng.uniform(0, 400, 2)
                box = [xy[0], xy[1], xy[0] + wh[0], xy[1] + wh[1]]
                label = int(rng.randint(n_cat))
            if label == no_dt:
                label = no_gt
            if box[2] <= box[0] or box[3] <= box[1]:
                continue
            per[label].append(box + [np.round(rng.beta(1.2, 2.0), 2)])
        if n == 3:                                                      # more than maxDets[-1] in one pair
            per[0] += [[5 + i, 5, 60 + i, 70, np.round(0.3 + 0.002 * (i % 50), 2)] for i in range(max_det + 30)]
        per = [np.array(p, dtype=np.float32).reshape(-1, 5) for p in per]
        if proposals:
            allp = np.concatenate(per)
            results.append(allp[rng.permutation(len(allp))])
        else:
            results.append(per)
    gt = COCO()
    gt.dataset = dict(images=[dict(id=i, width=2000, height=500, file_name=f'{i}.npy') for i in img_ids],
                      categories=[dict(id=c, name=f'c{c}') for c in cat_ids], annotations=anns)
    if proposals:       # CocoDataset files proposals under category id 1: keep it among the categories
        assert 1 in cat_ids
    gt.createIndex()
    return gt, results, img_ids, cat_ids


def det_json(results, img_ids, cat_ids):
    """CocoDataset._det2json / _proposal2json"""
    out = []
    for idx, img in enumerate(img_ids):
        per = results[idx] if isinstance(results[idx], list) else None
        for label, b in enumerate(per if per is not None else [results[idx]]):
            for i in range(b.shape[0]):
                v = b[i].tolist()
                out.append(dict(image_id=img, bbox=[v[0], v[1], v[2] - v[0], v[3] - v[1]], score=float(b[i][4]),
                                category_id=cat_ids[label] if per is not None else 1))
    return out


def host_eval(gt, results, img_ids, cat_ids, use_cats=1, max_dets=(1, 10, 100), iou_thrs=None):
    ev = COCOeval(gt, gt.loadRes(det_json(results, img_ids, cat_ids)), 'bbox')
    ev.params.imgIds, ev.params.catIds = list(img_ids), list(cat_ids)
    ev.params.maxDets, ev.params.useCats = list(max_dets), use_cats
    if iou_thrs is not None:
        ev.params.iouThrs = np.asarray(iou_thrs, dtype=np.float64)
    ev.evaluate()
    ev.accumulate()
    ev.summarize()
    return ev


def assert_not_vacuous(ev, img_ids, cat_ids):
    """the generated data really holds the hard cases -- every fact read from the host evaluator's records"""
    p = ev.params
    recs = [e for e in ev.evalImgs if e is not None and e['aRng'] == p.areaRng[0]]
    assert any(len(set(e['dtScores'])) < len(e['dtScores']) for e in recs), 'no pair with tied scores'
    crowd_ids = {g['id'] for gs in ev._gts.values() for g in gs if g['iscrowd']}
    assert any(max((np.count_nonzero(e['dtMatches'][0] == c) for c in crowd_ids & set(e['gtIds'])), default=0) >= 2
               for e in recs), 'no crowd matched by two detections'
    pooled = {}
    for (i, c), ds in ev._dts.items():
        pooled[i if not p.useCats else (i, c)] = pooled.get(i if not p.useCats else (i, c), 0) + len(ds)
    assert max(pooled.values()) > p.maxDets[-1], 'no pair with more detections than maxDets[-1]'
    thr = set(float(t) for t in p.iouThrs)
    assert any(float(v) in thr for m in ev.ious.values() if len(m) for v in np.asarray(m).ravel() if v > 0), \
        'no IoU equal to a threshold'
    for edge in (32.0 ** 2, 96.0 ** 2):
        assert any(g['area'] == edge for gs in ev._gts.values() for g in gs), f'no ground truth of area {edge}'
        assert any(d['area'] == edge for ds in ev._dts.values() for d in ds), f'no detection of area {edge}'
    gi = {i for (i, c), v in ev._gts.items() if v}
    di = {i for (i, c), v in ev._dts.items() if v}
    assert di - gi and gi - di, 'no image with detections only / ground truths only'
    if p.useCats:
        pr = ev.eval['precision']
        assert any((pr[:, :, k] == -1).all() for k in range(pr.shape[2])), 'no category without ground truth'
        assert any((pr[:, :, k, 0, -1] == 0).all() for k in range(pr.shape[2])), 'no category with ground truth and no detection'
    assert any(g['id'] == 0 for gs in ev._gts.values() for g in gs), 'no ground truth with id 0'
    assert list(img_ids) != sorted(img_ids), 'image ids are sorted'
    assert sorted(cat_ids) != list(range(min(cat_ids), min(cat_ids) + len(cat_ids))), 'category ids are contiguous'


def compare_records(ev, dev):
    """the device evaluator's match records against the host's evalImgs, pair by pair: matched / ignored bits of every
    detection, threshold and area range, scores, the ground truths' ignore flags; returns the number of pairs compared"""
    p = ev.params
    rec = dev.match_records()
    I, A = len(p.imgIds), len(p.areaRng)
    cats = p.catIds if p.useCats else [-1]
    n = 0
    for k in range(len(cats)):
        for a in range(A):
            for i in range(I):
                e = ev.evalImgs[(k * A + a) * I + i]
                pair = k * I + i
                d0, d1 = rec['det_off'][pair], rec['det_off'][pair + 1]
                g0, g1 = rec['gt_off'][pair], rec['gt_off'][pair + 1]
                if e is None:
                    assert d0 == d1 and g0 == g1, (k, i)
                    continue
                n += 1
                T = e['dtMatches'].shape[0]
                assert d1 - d0 == len(e['dtIds']) and g1 - g0 == len(e['gtIds']), (k, a, i)
                assert np.array_equal(rec['dt_scores'][d0:d1].astype(np.float64), np.array(e['dtScores'], dtype=np.float64))
                bits = 1 << np.arange(T)
                m = (rec['dt_matched'][d0:d1, a][None, :] & bits[:, None]) != 0
                g = (rec['dt_ignored'][d0:d1, a][None, :] & bits[:, None]) != 0
                assert np.array_equal(m, e['dtMatches'] != 0), ('matched', k, a, i)
                assert np.array_equal(g, e['dtIgnore'].astype(bool)), ('ignored', k, a, i)
                ig = (rec['gt_ignored'][g0:g1] >> a) & 1
                by = np.argsort(ig, kind='mergesort')
                assert np.array_equal(ig[by], e['gtIgnore']) and list(rec['gt_ids'][g0:g1][by]) == e['gtIds'], ('gt', k, a, i)
    return n


def same_dict(a, b):
    """equality of two evaluate() dicts, a nan (a class without ground truth) equal to a nan"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_dict(a[k], b[k]) for k in a)
    if isinstance(a, float) and a != a:
        return isinstance(b, float) and b != b
    return type(a) == type(b) and a == b
