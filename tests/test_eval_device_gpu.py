"""gpu: the device COCO evaluator (brcnn.evaluation.DeviceCOCOeval, csrc/coco_eval.hip) against the host COCOeval run
here on the same inputs.  Bit equality (np.array_equal on fp64 arrays), never a tolerance: every operation involved is a
correctly rounded fp64 operation or a comparison, and every sum an integer count."""
import json

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn.datasets import COCO
from brcnn.evaluation import DeviceCOCOeval
from tests.eval_device_util import assert_not_vacuous, compare_records, host_eval, make_set, same_dict as _eq

pytestmark = pytest.mark.gpu


def _gt(images, anns, cats=(1,), first_id=1):
    c = COCO()
    c.dataset = dict(images=[dict(id=i, width=500, height=500, file_name=f'{i}.npy') for i in images],
                     categories=[dict(id=k, name=f'c{k}') for k in cats],
                     annotations=[dict(id=j + first_id, image_id=a[0], category_id=a[1], bbox=list(a[2]),
                                       area=a[2][2] * a[2][3], iscrowd=a[3] if len(a) > 3 else 0)
                                  for j, a in enumerate(anns)])
    c.createIndex()
    return c


def _results(gt, dets):
    """(image, category, xywh, score) tuples as the detectors' per-image, per-class (k, 5) float32 xyxy arrays"""
    imgs, cats = gt.get_img_ids(), gt.get_cat_ids()
    out = [[[] for _ in cats] for _ in imgs]
    for i, c, (x, y, w, h), s in dets:
        out[imgs.index(i)][cats.index(c)].append([x, y, x + w, y + h, s])
    return [[np.array(b, dtype=np.float32).reshape(-1, 5) for b in per] for per in out]


def _dev(gt, results, img_ids=None, cat_ids=None, use_cats=1, max_dets=(1, 10, 100), iou_thrs=None):
    ev = DeviceCOCOeval(gt, results, img_ids=img_ids, cat_ids=cat_ids)
    if img_ids is not None:
        ev.params.imgIds, ev.params.catIds = list(img_ids), list(cat_ids)
    ev.params.maxDets, ev.params.useCats = list(max_dets), use_cats
    if iou_thrs is not None:
        ev.params.iouThrs = np.asarray(iou_thrs, dtype=np.float64)
    ev.evaluate()
    ev.accumulate()
    ev.summarize()
    return ev


def _run(gt, dets, max_dets=(1, 10, 100)):
    """the device evaluator on a hand-made case; the host evaluator beside it must agree bit for bit"""
    res = _results(gt, dets)
    ev = _dev(gt, res, max_dets=max_dets)
    host = host_eval(gt, res, gt.get_img_ids(), gt.get_cat_ids(), max_dets=max_dets)
    _same(host, ev)
    return ev


def _same(host, dev):
    for name in ('precision', 'recall', 'scores'):
        a, b = host.eval[name], dev.eval[name]
        assert a.shape == b.shape and a.dtype == b.dtype == np.float64, name
        assert np.array_equal(a, b), (name, int(np.count_nonzero(a != b)), a[a != b][:4], b[a != b][:4])
    assert host.eval['counts'] == dev.eval['counts']
    assert np.array_equal(host.stats, dev.stats)


# ---- 1. the hand-derived cases of tests/test_eval_cpu.py, same expected numbers ------------------------------------------
def test_perfect_detections():
    gt = _gt([1, 2], [(1, 1, (10, 10, 50, 50)), (2, 1, (20, 20, 100, 100)), (2, 1, (200, 200, 20, 20))])
    ev = _run(gt, [(1, 1, (10, 10, 50, 50), .9), (2, 1, (20, 20, 100, 100), .8), (2, 1, (200, 200, 20, 20), .7)])
    for i in (0, 1, 2, 3, 4, 5, 8):
        assert ev.stats[i] == pytest.approx(1.0)
    assert ev.stats[6] == pytest.approx(2 / 3)


def test_false_positive_ranked_first_halves_precision():
    gt = _gt([1], [(1, 1, (10, 10, 50, 50))])
    ev = _run(gt, [(1, 1, (300, 300, 50, 50), .95), (1, 1, (10, 10, 50, 50), .9)])
    assert ev.stats[0] == pytest.approx(0.5)
    ev = _run(gt, [(1, 1, (300, 300, 50, 50), .5), (1, 1, (10, 10, 50, 50), .9)])
    assert ev.stats[0] == pytest.approx(1.0)


def test_half_recall_gives_51_of_101_points():
    gt = _gt([1], [(1, 1, (10, 10, 50, 50)), (1, 1, (200, 200, 50, 50))])
    ev = _run(gt, [(1, 1, (10, 10, 50, 50), .9)])
    assert ev.stats[0] == pytest.approx(51 / 101) and ev.stats[8] == pytest.approx(0.5)


def test_iou_thresholds():
    gt = _gt([1], [(1, 1, (10, 10, 50, 50))])
    ev = _run(gt, [(1, 1, (20, 10, 50, 50), .9)])          # IoU 2/3: a hit at .50 .55 .60 .65 only
    assert ev.stats[0] == pytest.approx(4 / 10) and ev.stats[1] == pytest.approx(1.0) and ev.stats[2] == 0.0


def test_crowd_and_area_ranges_and_maxdets():
    gt = _gt([1], [(1, 1, (10, 10, 50, 50)), (1, 1, (200, 200, 100, 100), 1)])
    ev = _run(gt, [(1, 1, (10, 10, 50, 50), .8), (1, 1, (210, 210, 30, 30), .9), (1, 1, (220, 220, 30, 30), .85)])
    assert ev.stats[0] == pytest.approx(1.0)
    gt = _gt([1], [(1, 1, (10, 10, 20, 20))])
    ev = _run(gt, [(1, 1, (10, 10, 20, 20), .9)])
    assert ev.stats[3] == pytest.approx(1.0) and ev.stats[4] == -1 and ev.stats[5] == -1
    gt = _gt([1], [(1, 1, (10, 10, 50, 50))])
    ev = _run(gt, [(1, 1, (300, 300, 50, 50), .95), (1, 1, (10, 10, 50, 50), .9)])
    assert ev.stats[6] == 0.0 and ev.stats[7] == pytest.approx(1.0)
    gt = _gt([1], [(1, 1, (10, 10, 50, 50)), (1, 2, (100, 100, 50, 50))], cats=(1, 2))
    ev = _run(gt, [(1, 1, (10, 10, 50, 50), .9)])
    assert ev.stats[0] == pytest.approx(0.5)


def test_area_range_edges_are_inclusive_on_both_sides():
    gt = _gt([1], [(1, 1, (10, 10, 32, 32))])
    ev = _run(gt, [(1, 1, (10, 10, 32, 32), .9)])
    assert ev.stats[3] == pytest.approx(1.0) and ev.stats[4] == pytest.approx(1.0) and ev.stats[5] == -1
    gt = _gt([1], [(1, 1, (10, 10, 96, 96))])
    ev = _run(gt, [(1, 1, (10, 10, 96, 96), .9)])
    assert ev.stats[3] == -1 and ev.stats[4] == pytest.approx(1.0) and ev.stats[5] == pytest.approx(1.0)
    gt = _gt([1], [(1, 1, (10, 10, 32, 32.03125))])
    ev = _run(gt, [(1, 1, (10, 10, 32, 32.03125), .9)])
    assert ev.stats[3] == -1 and ev.stats[4] == pytest.approx(1.0)
    gt = _gt([1], [(1, 1, (10, 10, 20, 20))])
    ev = _run(gt, [(1, 1, (200, 200, 150, 150), .95), (1, 1, (10, 10, 20, 20), .9)])
    assert ev.stats[3] == pytest.approx(1.0) and ev.stats[0] == pytest.approx(0.5)


def test_maxdets_truncation_and_the_precision_envelope():
    gt = _gt([1], [(1, 1, (10, 10, 50, 50)), (1, 1, (200, 200, 50, 50))])
    dets = [(1, 1, (400, 400, 40, 40), .9), (1, 1, (10, 10, 50, 50), .8), (1, 1, (200, 200, 50, 50), .7)]
    ev = _run(gt, dets, max_dets=(1, 2, 100))
    assert ev.stats[0] == pytest.approx(2 / 3)
    assert ev.stats[6] == 0.0 and ev.stats[7] == pytest.approx(0.5) and ev.stats[8] == pytest.approx(1.0)
    ev2 = _run(gt, dets[::-1], max_dets=(1, 2, 100))
    assert ev2.stats[0] == pytest.approx(2 / 3) and ev2.stats[6] == 0.0


def test_crowd_absorbs_any_number_of_detections():
    gt = _gt([1], [(1, 1, (10, 10, 50, 50)), (1, 1, (200, 200, 200, 200), 1)])
    ev = _run(gt, [(1, 1, (210, 210, 30, 30), .95), (1, 1, (250, 250, 30, 30), .9), (1, 1, (300, 300, 30, 30), .85),
                   (1, 1, (10, 10, 50, 50), .5)])
    assert ev.stats[0] == pytest.approx(1.0) and ev.stats[8] == pytest.approx(1.0)
    ev = _run(gt, [(1, 1, (10, 10, 50, 50), .9), (1, 1, (12, 10, 50, 50), .8)])
    assert ev.stats[0] == pytest.approx(1.0)
    gt = _gt([1], [(1, 1, (200, 200, 200, 200), 1)])
    ev = _run(gt, [(1, 1, (210, 210, 30, 30), .95)])
    assert ev.stats[0] == -1


# ---- 2. / 3. seeded fuzz, not vacuous, bit-equal -------------------------------------------------------------------------
FUZZ = {
    'coco80': dict(seed=11, n_img=300, n_cat=80, use_cats=1, max_dets=(1, 10, 100)),
    'dense4': dict(seed=12, n_img=300, n_cat=4, gts_per_img=9, dense_every=5, use_cats=1, max_dets=(1, 10, 100)),
    'proposals': dict(seed=13, n_img=60, n_cat=5, dets_per_img=400, proposals=True, use_cats=0, max_dets=(100, 300, 1000)),
}


@pytest.mark.parametrize('name', list(FUZZ))
def test_fuzz_bit_equal_to_the_host_evaluator(name):
    kw = dict(FUZZ[name])
    use_cats, max_dets = kw.pop('use_cats'), kw.pop('max_dets')
    gt, results, img_ids, cat_ids = make_set(max_det=max_dets[-1], **kw)
    host = host_eval(gt, results, img_ids, cat_ids, use_cats=use_cats, max_dets=max_dets)
    assert_not_vacuous(host, img_ids, cat_ids)
    dev = _dev(gt, results, img_ids, cat_ids, use_cats=use_cats, max_dets=max_dets)
    assert compare_records(host, dev) > 100
    _same(host, dev)
    # 5. a second run gives the same bits; so does one on a side stream beside a co-running kernel
    again = _dev(gt, results, img_ids, cat_ids, use_cats=use_cats, max_dets=max_dets)
    side = torch.cuda.Stream()
    busy = torch.randn(2048, 2048, device='cuda')
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(8):
        busy = busy @ busy * 1e-3                       # (on the default stream, while the evaluation runs on `side`)
    with torch.cuda.stream(side):
        third = _dev(gt, results, img_ids, cat_ids, use_cats=use_cats, max_dets=max_dets)
    torch.cuda.synchronize()
    for other in (again, third):
        _same(host, other)
        a, b = dev.match_records(), other.match_records()
        assert all(np.array_equal(a[k], b[k]) for k in a)


# ---- 4. the data set's front door ---------------------------------------------------------------------------------------
def test_dataset_evaluate_backend_device(tmp_path):
    from brcnn.datasets import CocoDataset
    gt, results, img_ids, cat_ids = make_set(21, 40, 6)
    path = tmp_path / 'ann.json'
    path.write_text(json.dumps(gt.dataset))
    ds = CocoDataset(ann_file=str(path), pipeline=[], classes=tuple(f'c{c}' for c in cat_ids), test_mode=True)
    want = ds.evaluate(results, metric=['bbox', 'proposal'], classwise=True)
    got = ds.evaluate(results, metric=['bbox', 'proposal'], classwise=True, backend='device', jsonfile_prefix=str(tmp_path / 'r'))
    assert _eq(want, got) and want['bbox_mAP'] > 0 and (tmp_path / 'r.bbox.json').exists()
    tables = ds.coco._device_eval_tables
    kept = {k: v['dev']['f64'] for k, v in tables.items()}
    assert len(kept) == 2                               # one table per category mode
    assert _eq(want, ds.evaluate(results, metric=['bbox', 'proposal'], classwise=True, backend='device'))
    assert all(tables[k]['dev']['f64'] is t for k, t in kept.items()) and len(tables) == 2      # no second upload
    kw = dict(iou_thrs=[0.5, 0.7, 0.9], proposal_nums=(10, 50, 200), metric_items=None)
    assert _eq(ds.evaluate(results, metric=['bbox', 'proposal'], **kw), ds.evaluate(results, metric=['bbox', 'proposal'], backend='device', **kw))
    props = [np.concatenate(r) for r in results]
    assert _eq(ds.evaluate(props, metric='proposal'), ds.evaluate(props, metric='proposal', backend='device'))
    with pytest.raises(KeyError):
        ds.evaluate(props, metric='bbox', backend='device')
    # 6. all results empty: the host path's answer
    empty = [[np.zeros((0, 5), np.float32)] * len(cat_ids) for _ in results]
    assert ds.evaluate(empty, backend='device') == ds.evaluate(empty) == {}


# ---- 6. edge inputs ---------------------------------------------------------------------------------------------------
def test_one_image_one_detection():
    gt = _gt([5], [(5, 3, (10, 10, 50, 50))], cats=(3,), first_id=0)       # (its only ground truth has id 0)
    ev = _run(gt, [(5, 3, (12, 10, 50, 50), .5)])
    assert ev.stats[0] == 0.0                           # matched, but the host tests the stored id's truth value


def test_a_pair_with_1000_detections_and_200_ground_truths():
    rng = np.random.RandomState(3)
    xy = rng.uniform(0, 440, (200, 2)).round(1)
    wh = rng.uniform(8, 60, (200, 2)).round(1)
    gt = _gt([1], [(1, 1, (xy[i, 0], xy[i, 1], wh[i, 0], wh[i, 1]), int(i % 23 == 0)) for i in range(200)])
    pick = rng.randint(0, 200, 1000)
    j = rng.normal(0, 2.0, (1000, 4))
    box = np.concatenate([xy[pick] + j[:, :2], xy[pick] + wh[pick] + j[:, 2:]], 1)
    res = [[np.concatenate([box, rng.rand(1000, 1).round(2)], 1).astype(np.float32)]]
    host = host_eval(gt, res, [1], [1], max_dets=(100, 300, 1000))
    dev = _dev(gt, res, max_dets=(100, 300, 1000))
    assert compare_records(host, dev) == 4
    _same(host, dev)
    assert 0 < host.stats[0] < 1
