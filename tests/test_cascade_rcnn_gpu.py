"""GPU tests of the Cascade R-CNN baseline (CascadeRoIHead / CascadeRCNN on the device path):
  * the hand-over kernels (csrc/cascade.hip) against the float64 restatement tests/cascade_ref64.py, which
    tests/test_cascade_rcnn_cpu.py pins to what the reference's refine_bboxes / regress_by_class computed;
  * brcnn_rcnn_sample_gt against brcnn_rcnn_sample (bit-equal outputs) and the host sampler's pos_is_gt;
  * head and model against tests/golden/g26_cascade_rcnn.npz (made by tests/golden/make_golden_cascade_rcnn.py from the
    imported reference), at the tolerances of tests/test_faster_rcnn_gpu.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import build_detector, build_head, core, lib, ops, train_ops
from brcnn.config import ConfigDict
from tests import cascade_rcnn_inputs as ci
from tests import cascade_ref64 as R
from tests import faster_rcnn_inputs as fi
from tests import util

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G = os.path.join(os.path.dirname(__file__), 'golden', 'g26_cascade_rcnn.npz')
EPS32 = R.EPS32
MEANS = (0., 0., 0., 0.)
STDS = (0.1, 0.1, 0.2, 0.2)
MAX_SHAPE = torch.tensor([[800., 1333.], [750., 1200.], [640., 640.]])
T = torch.as_tensor


@pytest.fixture(scope='module')
def gold():
    return {k: v for k, v in np.load(G, allow_pickle=False).items()}


def d(t):
    return t.to(DEV)


def _within(got, ref64, bound):
    """|got - ref| <= 8 * EPS32 * (|centre| + size) along each coordinate's axis (tests/cascade_ref64.box_bound)"""
    err = np.abs(got.astype(np.float64) - ref64)
    print('largest box error / bound', float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0)
    return bool((err <= bound + 1e-30).all())


# ------------------------------------------------------------------------------------------- test-time refine
def _refine_test_case(C, K, agnostic):
    g = torch.Generator().manual_seed(1000 * C + 10 * K + int(agnostic))
    B = 3
    num = torch.tensor([K, (K + 1) // 2, 0], dtype=torch.int32)
    dets = torch.cat([util.rand_boxes(B * K, seed=K + C), torch.rand(B * K, 1, generator=g)], 1).view(B, K, 5)
    dets[1, int(num[1]):] = 0
    dets[2] = 0
    s0 = torch.randn(B * K, C + 1, generator=g) * 2
    s1 = torch.randn(B * K, C + 1, generator=g) * 2
    reg = torch.randn(B * K, 4 if agnostic else 4 * C, generator=g) * 0.5
    top = float(s0.abs().max()) + 1.0
    # row 0: deltas at both ends of the ratio clip (every class), and the largest logit in the background column
    reg[0].view(-1, 4)[:, 2], reg[0].view(-1, 4)[:, 3] = 60., -60.
    s0[0, C] = top + 3
    if K >= 7:
        if C >= 2:      # row 1: an exact two-way tie of the top foreground logit (the lower index wins)
            s0[1, :C] = -top
            s0[1, [C - 1, C // 2 - 1 if C > 2 else 0]] = top
        if C >= 3:      # row 2: an exact three-way tie
            s0[2, :C] = -top
            s0[2, [1, C // 2, C - 1]] = top
        # rows 3, 4: the decoded box leaves the image on the left / top and on the right / bottom
        dets[0, 3, :4] = torch.tensor([5., 4., 60., 50.])
        reg[3].view(-1, 4)[:] = torch.tensor([-20., -20., 1., 1.])
        dets[0, 4, :4] = torch.tensor([1250., 740., 1330., 799.])
        reg[4].view(-1, 4)[:] = torch.tensor([20., 20., 1., 1.])
    return dets, num, s0, s1, reg


@pytest.mark.parametrize('C', [1, 4, 80])
@pytest.mark.parametrize('K', [1, 7, 300])
@pytest.mark.parametrize('agnostic', [False, True])
def test_cascade_refine_test_against_float64(C, K, agnostic):
    """Validity, zeroed padding and column 4 exact; logit_sum bit-equal to torch's fp32 `s0` and `s0 + s1` on the CPU
    over two successive calls; boxes within 8 * EPS32 * (|centre| + size) of float64, the bound
    test_rcnn_decode_plain_against_float64 derives for the same arithmetic.  The kernel does not emit its labels: for a
    class-specific head they are observable through the deltas it read -- every class has its own random deltas, so a
    wrong label puts the box far outside the bound; on the tie rows and the background row the test also checks that the
    runner-up's box WOULD lie outside.  C = 80 is wider than a wave: the arg-max reduction loops there."""
    dets, num, s0, s1, reg = _refine_test_case(C, K, agnostic)
    B = 3
    ref, lab, bound = R.refine_test(dets.numpy(), num.numpy(), s0.numpy(), reg.numpy(), MAX_SHAPE.numpy(), MEANS, STDS, agnostic)
    assert lab[0] < C and np.array_equal(lab, s0[:, :C].argmax(1).numpy())      # the tie rule is torch's
    if K >= 7 and C >= 2:
        assert lab[1] == (C // 2 - 1 if C > 2 else 0) and (C < 3 or lab[2] == 1)
    out, ls = ops.cascade_refine_test(d(dets), d(num), d(s0), d(reg), d(MAX_SHAPE), C, MEANS, STDS, reg_class_agnostic=agnostic)
    o = out.cpu().numpy()
    valid = (np.arange(K)[None, :] < num.numpy()[:, None])
    assert (o[~valid] == 0).all() and (o[..., 4] == 0).all()
    assert (o[2] == 0).all() and (o[1, int(num[1]):] == 0).all()
    assert _within(o[..., :4], ref[..., :4], bound)
    assert torch.equal(ls.cpu(), s0)
    if K >= 7:
        assert ref[0, 3, 0] == 0 and ref[0, 3, 1] == 0 and ref[0, 4, 2] == 1333. and ref[0, 4, 3] == 800.
        assert o[0, 3, 0] == 0 and o[0, 3, 1] == 0 and o[0, 4, 2] == 1333. and o[0, 4, 3] == 800.
    if not agnostic and C >= 2:
        # a wrong label would show: the runner-up's deltas decode to a box outside the bound
        rows = [0] + ([1] if K >= 7 else []) + ([2] if K >= 7 and C >= 3 else [])
        for r in rows:
            fg = s0[r, :C].clone()
            fg[lab[r]] = -float('inf')
            other = np.array(lab, copy=True)
            other[r] = int(fg.argmax())
            alt = R.delta2bbox(dets.view(-1, 5).numpy()[:, :4], R.gather_deltas(reg.numpy(), other, False), MEANS, STDS,
                               np.repeat(MAX_SHAPE.numpy(), K, axis=0))
            if r != 0:      # (row 0's deltas are the ratio-clip ones for every class: its label is not observable)
                assert (np.abs(alt[r] - o.reshape(-1, 5)[r, :4]) > 16 * bound.reshape(-1, 4)[r]).any()
    # second stage: the refined boxes go back in, the logits arrive as a column block of a wider (fused) tensor
    fused = d(torch.cat([s1, reg, torch.zeros(B * K, 3)], 1))
    cls_v, reg_v = fused[:, :C + 1], fused[:, C + 1:C + 1 + reg.shape[1]]
    assert not cls_v.is_contiguous() and not reg_v.is_contiguous()
    ref2, _, bound2 = R.refine_test(o.astype(np.float64), num.numpy(), s1.numpy(), reg.numpy(), MAX_SHAPE.numpy(), MEANS, STDS,
                                    agnostic)
    out2, ls2 = ops.cascade_refine_test(out, d(num), cls_v, reg_v, d(MAX_SHAPE), C, MEANS, STDS, reg_class_agnostic=agnostic,
                                        logit_sum=ls)
    assert ls2.data_ptr() == ls.data_ptr() and torch.equal(ls2.cpu(), s0 + s1)
    assert _within(out2.cpu().numpy()[..., :4], ref2[..., :4], bound2)
    # two runs, the same bits
    again, ls_again = ops.cascade_refine_test(d(dets), d(num), d(s0), d(reg), d(MAX_SHAPE), C, MEANS, STDS,
                                              reg_class_agnostic=agnostic)
    assert torch.equal(again, out) and torch.equal(ls_again.cpu(), s0)


# ------------------------------------------------------------------------------------------- train-time refine
def _refine_train_case(C, agnostic, pattern, rows=(300, 5, 0), seed=0):
    g = torch.Generator().manual_seed(seed + 100 * C + int(agnostic))
    offs = [0]
    for n in rows:
        offs.append(offs[-1] + n)
    N = offs[-1]
    rois = torch.cat([torch.cat([torch.full((n, 1), float(b)), util.rand_boxes(n, 1200., 640., seed=seed + b, max_size=300.)], 1)
                      for b, n in enumerate(rows) if n] or [torch.zeros(0, 5)])
    labels = torch.randint(0, C + 1, (N,), generator=g)
    labels[0], labels[1] = C, 0                                   # a background and a foreground row for sure
    flags = torch.zeros(N, dtype=torch.int32)
    if pattern == 'front':
        flags[:7] = 1
        flags[offs[1]:offs[1] + 2] = 1
    elif pattern == 'scattered':
        flags[torch.randperm(rows[0], generator=g)[:9]] = 1
        flags[offs[1] + 3] = 1
    elif pattern == 'whole_image':
        flags[offs[1]:offs[2]] = 1
    cls = torch.randn(N, C + 1, generator=g) * 2
    cls[0, C] = 50.                                               # largest logit in the background column
    reg = torch.randn(N, 4 if agnostic else 4 * C, generator=g) * 0.5
    reg[1].view(-1, 4)[:, 2], reg[1].view(-1, 4)[:, 3] = -60., 60.
    return rois, labels, flags, offs, cls, reg


def _check_refine_train(C, agnostic, rois, labels, flags, offs, cls, reg):
    B = len(offs) - 1
    max_shape = MAX_SHAPE[:B].contiguous()
    ref, used = R.refine_train(rois.numpy(), labels.numpy(), flags.numpy(), offs, cls.numpy(), reg.numpy(), max_shape.numpy(),
                               MEANS, STDS, agnostic, C)
    assert (labels == C).any() and (labels < C).any() and (used < C).all()
    args = (d(rois), d(labels), d(flags), offs, d(cls), d(reg), d(max_shape), C, MEANS, STDS)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')          # the refinement reads nothing back
    try:
        props, num = train_ops.cascade_refine_train(*args, reg_class_agnostic=agnostic)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    kout = max(1, max(offs[b + 1] - offs[b] for b in range(B)))
    assert props.shape == (B, kout, 5) and num.dtype == torch.int32
    p, n = props.cpu().numpy(), num.cpu().tolist()
    assert n == [len(r[0]) for r in ref]
    for b in range(B):
        assert _within(p[b, :n[b], :4], ref[b][0], ref[b][1])         # survivors, in their original order
        assert (p[b, n[b]:] == 0).all() and (p[b, :, 4] == 0).all()
    again = train_ops.cascade_refine_train(*args, reg_class_agnostic=agnostic)
    assert torch.equal(again[0], props) and torch.equal(again[1], num)
    return n


@pytest.mark.parametrize('C', [1, 4, 80])
@pytest.mark.parametrize('agnostic', [False, True])
@pytest.mark.parametrize('pattern', ['front', 'scattered', 'whole_image', 'none'])
def test_cascade_refine_train_against_float64(C, agnostic, pattern):
    """num_out, the surviving rows, their order and the zero padding exact (a row out of place would carry another row's
    box: the boxes are random and distinct), boxes within the decode bound; per-image rows [300, 5, 0]; ground-truth
    flags at the front, scattered, on every row of image 1 (num_out = 0 there) and on none; background rows (arg-max
    label) and foreground rows (own label) both occur; one row at both ends of the ratio clip."""
    rois, labels, flags, offs, cls, reg = _refine_train_case(C, agnostic, pattern)
    n = _check_refine_train(C, agnostic, rois, labels, flags, offs, cls, reg)
    assert n == {'front': [293, 3, 0], 'scattered': [291, 4, 0], 'whole_image': [300, 0, 0], 'none': [300, 5, 0]}[pattern]


def test_cascade_refine_train_2048_rows_in_one_image():
    """the sampler's limit: two compaction passes of 1024 rows, flags scattered over both"""
    rois, labels, flags, offs, cls, reg = _refine_train_case(4, False, 'none', rows=(2048, 3), seed=7)
    flags[torch.randperm(2048, generator=torch.Generator().manual_seed(1))[:500]] = 1
    n = _check_refine_train(4, False, rois, labels, flags, offs, cls, reg)
    assert n == [1548, 3]


# ------------------------------------------------------------------------------------------- mean softmax
@pytest.mark.parametrize('C', [1, 4, 80])
def test_cascade_mean_softmax_against_float64(C):
    """The averaged logits are bit-equal to torch's fp32 `(s0 + s1 + s2) / 3.0` on the CPU (adds in stage order, one true
    division).  probs against the float64 softmax of that fp32 mean m, with u = EPS32 / 2 the unit round-off:
      t_i = fl(m_i - max m)          one rounding: the exponent is off by <= |t_i| u, exp(t_i) by the factor e^(|t_i| u)
      e_i = expf(t_i)                2 ulp = 2 EPS32 (the allowance test_rcnn_decode_plain_against_float64 makes for expf)
      S   = sum of C + 1 terms       positive terms, C additions in any order: C u, on top of the terms' own error
      p_i = e_i / S                  one rounding: u
    so |p_i - p64_i| <= p64_i * ((|t_i| + max_j |t_j|) u + 4 EPS32 + (C + 1) u), first order; the test allows 1.25 x that
    for the second-order terms, plus one fp32 denormal step."""
    g = torch.Generator().manual_seed(C)
    rows = 333
    s = [torch.randn(rows, C + 1, generator=g) * 3 for _ in range(3)]
    s[1][0] = 0.0                                      # a row whose mean needs no rounding
    s[2][1, 0] = 40.0                                  # a dominant logit: the others' probabilities are tiny
    want = (s[0] + s[1] + s[2]) / 3.0
    assert np.array_equal(R.mean_logits32([t.numpy() for t in s]), want.numpy())
    fused = d(torch.cat([torch.zeros(rows, 2), s[2]], 1))
    probs, mean = ops.cascade_mean_softmax(d(s[0] + s[1]), fused[:, 2:], 3, want_mean=True)
    assert torch.equal(mean.cpu(), want)
    p64 = R.softmax64(want.numpy())
    t = np.abs(want.numpy().astype(np.float64) - want.numpy().astype(np.float64).max(axis=1, keepdims=True))
    u = EPS32 / 2
    bound = p64 * ((t + t.max(axis=1, keepdims=True)) * u + 4 * EPS32 + (C + 1) * u) * 1.25 + 2.0 ** -149
    err = np.abs(probs.cpu().numpy().astype(np.float64) - p64)
    print('largest softmax error / bound', float((err / bound).max()))
    assert (err <= bound).all()
    assert torch.equal(ops.cascade_mean_softmax(d(s[0] + s[1]), fused[:, 2:], 3), probs)
    # one stage: the plain softmax of the head's logits
    p1 = ops.cascade_mean_softmax(None, d(s[0]), 1)
    b1 = R.softmax64(s[0].numpy())
    t1 = np.abs(s[0].numpy().astype(np.float64) - s[0].numpy().astype(np.float64).max(axis=1, keepdims=True))
    assert (np.abs(p1.cpu().numpy() - b1) <= b1 * ((t1 + t1.max(1, keepdims=True)) * u + 4 * EPS32 + (C + 1) * u) * 1.25
            + 2.0 ** -149).all()


# ------------------------------------------------------------------------------------------- the sampler's gt flags
def test_rcnn_sample_gt_is_rcnn_sample_plus_the_flags():
    """same call, same bits; gt_flags against the host sampler's pos_is_gt on the same draw (the candidate indices below
    the number of added ground truths), over images with many / few / no ground truths"""
    gts, gls, props = [], [], []
    for b, (ng, nrand, jit) in enumerate([(6, 900, 40), (3, 60, 2), (0, 500, 0), (10, 2000, 80)]):
        g = util.rand_boxes(ng, 1333, 800, seed=70 + b, min_size=24, max_size=500) if ng else torch.empty(0, 4)
        gen = torch.Generator().manual_seed(90 + b)
        near = (g.repeat(jit, 1) + torch.randn(ng * jit, 4, generator=gen) * 4) if ng and jit else torch.empty(0, 4)
        bx = torch.cat([near, util.rand_boxes(nrand, 1333, 800, seed=80 + b)], 0)
        bx = torch.cat([torch.min(bx[:, :2], bx[:, 2:]), torch.max(bx[:, :2], bx[:, 2:]) + 1], 1)
        props.append(torch.cat([bx, torch.rand(bx.shape[0], 1, generator=gen)], 1))
        gts.append(g)
        gls.append(torch.randint(0, 4, (ng,), generator=gen))
    B, K, num = len(props), max(len(p) for p in props), 512
    dets = torch.zeros(B, K, 5)
    for b, p in enumerate(props):
        dets[b, :len(p)] = p
    nums = torch.tensor([len(p) for p in props], dtype=torch.int32)
    gflat, lflat, offs = train_ops.flatten_gts([d(g) for g in gts], [d(l) for l in gls])
    gi, cnt = train_ops.assign_max_iou(d(dets), gflat, offs, 0.6, 0.6, 0.6, False, num_boxes=d(nums), want_counts=True)
    counts = [(p_ + offs[b + 1] - offs[b], n_) for b, (p_, n_) in enumerate(cnt.cpu().tolist())]
    torch.manual_seed(5)
    perm, rows = train_ops.draw_sampler_perms(counts, num, num // 4, -1)
    args = (d(dets), d(nums), gi, None, gflat, lflat, offs, d(perm), rows, num, num // 4, -1, 4, MEANS, STDS)
    plain = train_ops.rcnn_sample(*args, want_pos_flags=True)
    flagged = train_ops.rcnn_sample(*args, want_pos_flags=True, want_gt_flags=True)
    assert set(flagged) == set(plain) | {'gt_flags'}
    assert all(torch.equal(plain[k], flagged[k]) for k in plain)
    torch.manual_seed(5)
    want, want_boxes = [], []
    assigner, sampler = core.MaxIoUAssigner(0.6, 0.6, 0.6, match_low_quality=False), core.RandomSampler(num, 0.25)
    for b in range(B):
        sr = sampler.sample(assigner.assign(props[b], gts[b], None, gls[b]), props[b], gts[b], gls[b])
        assert len(sr.pos_inds) + len(sr.neg_inds) == rows[b + 1] - rows[b]
        want += sr.pos_is_gt.tolist() + [0] * len(sr.neg_inds)
        # the candidate indices below the number of added ground truths ARE the ground truths
        assert sr.pos_is_gt.tolist() == (sr.pos_inds < len(gts[b])).int().tolist()
        want_boxes.append(gts[b][sr.pos_inds[sr.pos_inds < len(gts[b])]])
    got = flagged['gt_flags'].cpu()
    assert got.tolist() == want
    per_image = [int(got[rows[b]:rows[b + 1]].sum()) for b in range(B)]
    # image 0 / 3 draw 128 of more positives (some ground truths are not drawn), image 1 keeps all of its own, image 2 has none
    assert per_image[1] == 3 and per_image[2] == 0 and 0 < per_image[0] <= 6 and 0 < per_image[3] <= 10
    assert torch.equal(flagged['rois'].cpu()[got.bool()][:, 1:], torch.cat(want_boxes))


# ------------------------------------------------------------------------------------------- argument errors
def test_entries_refuse_bad_arguments():
    """NULL pointers, C < 1, short row strides, more rows than the limit: BRCNN_EINVAL (-22) before anything is queued"""
    L = lib.load()
    buf = torch.zeros(4096, device=DEV)
    p, m4, s4 = buf.data_ptr(), (ctypes.c_float * 4)(0, 0, 0, 0), (ctypes.c_float * 4)(.1, .1, .2, .2)
    stream = torch.cuda.current_stream().cuda_stream

    def rt(dets=p, num=p, cls=p, cs=5, reg=p, rs=4, ms=p, B=1, K=8, C=4, agn=1, out=p, ls=p, means=m4, clip=0.016):
        return L.brcnn_cascade_refine_test(dets, num, cls, cs, reg, rs, ms, B, K, C, agn, 1, means, s4, clip, out, ls, stream)
    for bad in (dict(dets=None), dict(num=None), dict(cls=None), dict(reg=None), dict(ms=None), dict(out=None), dict(ls=None),
                dict(C=0), dict(cs=4), dict(agn=0, rs=15), dict(B=0), dict(K=0), dict(means=None), dict(clip=0.0)):
        assert rt(**bad) == -22, bad

    def sm(ls=p, cls=p, cs=5, rows=8, C=4, S=3, probs=p):
        return L.brcnn_cascade_mean_softmax(ls, cls, cs, rows, C, S, probs, None, stream)
    for bad in (dict(ls=None), dict(cls=None), dict(probs=None), dict(C=0), dict(S=0), dict(cs=4), dict(rows=-1)):
        assert sm(**bad) == -22, bad
    assert sm(rows=0) == 0

    def tr(rois=p, labels=p, flags=p, offs=(0, 8), B=1, cls=p, cs=5, reg=p, rs=4, ms=p, C=4, agn=1, kout=8, out=p, num=p):
        o = (ctypes.c_int * len(offs))(*offs) if offs is not None else None
        return L.brcnn_cascade_refine_train(rois, labels, flags, o, B, cls, cs, reg, rs, ms, C, agn, m4, s4, 0.016, kout, out,
                                            num, stream)
    for bad in (dict(rois=None), dict(labels=None), dict(flags=None), dict(offs=None), dict(cls=None), dict(reg=None),
                dict(ms=None), dict(out=None), dict(num=None), dict(C=0), dict(cs=4), dict(agn=0, rs=15), dict(B=0),
                dict(B=65, offs=tuple(range(66))), dict(offs=(0, 2049), kout=2049), dict(offs=(0, 8), kout=7),
                dict(offs=(8, 0)), dict(kout=0)):
        assert tr(**bad) == -22, bad
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0            # nothing ran


# ------------------------------------------------------------------------------------------- head and model vs the fixture
def _table(res):
    return np.concatenate([np.concatenate([r, np.full((len(r), 1), c, np.float32)], 1) for c, r in enumerate(res)], 0)


def _assert_dets(got, ref, what):
    """labels and kept order exact, boxes and scores within 2e-4"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got[:, 5], ref[:, 5]), what
    print(what, 'largest box / score difference', float(np.abs(got[:, :5] - ref[:, :5]).max()) if len(ref) else 0.0)
    assert np.allclose(got[:, :5], ref[:, :5], rtol=0, atol=2e-4), (what, np.abs(got[:, :5] - ref[:, :5]).max())


def _assert_losses(losses, gold, prefix):
    for k, v in losses.items():
        got = (sum(v) if isinstance(v, list) else v).detach().cpu().double().reshape(-1)
        ref = T(gold[prefix + k]).double().sum().reshape(-1)
        print(prefix + k, 'difference', float((got - ref).abs().max()), 'of', float(ref.abs().max()))
        assert torch.allclose(got, ref, rtol=2e-3, atol=1e-4), (prefix, k, got, ref)


def _model(seed):
    m = build_detector(ConfigDict(ci.fixture_model_cfg()))
    m.load_state_dict(ci.fixture_state_dict(m, seed))
    return m.to(DEV)


def _head_inputs(seed):
    feats, metas, gts, gls, props = fi.roi_inputs(seed)
    nhwc = [f.to(DEV).permute(0, 2, 3, 1).contiguous() for f in feats]
    K = max(len(p) for p in props)
    dets = torch.zeros(2, K, 5)
    for b, p in enumerate(props):
        dets[b, :len(p)] = p
    num = torch.tensor([len(p) for p in props], dtype=torch.int32)
    return nhwc, metas, gts, gls, d(dets), d(num)


def test_cascade_roi_head_golden(gold):
    """section (b): forward_train_device (three whole-batch samplers with the seeded draws in the reference's order, the
    plain loss kernels, brcnn_cascade_refine_train between the stages) + backward, and simple_test_padded"""
    seed = int(gold['seed_head'])
    rh = build_head(ConfigDict(ci.roi_head_cfg()))
    rh.load_state_dict(ci.head_state_dict(rh, seed))
    rh = rh.to(DEV)
    nhwc, metas, gts, gls, dets, num = _head_inputs(seed)
    rh.train()
    assert rh.device_train_ok()
    torch.manual_seed(seed + 100)
    gt_flat = train_ops.flatten_gts([d(g) for g in gts], [d(l) for l in gls])
    losses, extra = rh.forward_train_device([f.requires_grad_() for f in nhwc], metas, dets, num, gt_flat,
                                            overlap_work=lambda: 'ran')
    assert extra == 'ran' and sorted(losses) == sorted(f's{i}.{k}' for i in range(3) for k in ('loss_cls', 'loss_bbox', 'acc'))
    _assert_losses(losses, gold, 'head_train_')
    # every stage keeps pinned count buffers of its own
    hosts = [rh._stage(i).__dict__['_count_host'] for i in range(3)]
    assert len({id(h) for h in hosts}) == 3 and len({h['counts'].data_ptr() for h in hosts}) == 3
    assert 'gt_flags' in rh.last_samples[0] and 'gt_flags' not in rh.last_samples[2]
    sum(v for k, v in losses.items() if 'loss' in k).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in rh.parameters())
    assert all(f.grad is not None and torch.isfinite(f.grad).all() for f in nhwc[:4])
    rh.eval()
    feats = [f.detach() for f in nhwc]
    with torch.no_grad():
        det, lab, nd = rh.simple_test_padded(feats, dets, num, metas, rescale=True)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')          # no host synchronisation inside the RoI head
        try:
            det2, lab2, nd2 = rh.simple_test_padded(feats, dets, num, metas, rescale=True)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    assert torch.equal(det, det2) and torch.equal(lab, lab2) and torch.equal(nd, nd2)
    for b in range(2):
        n = int(nd[b])
        got = torch.cat([det[b, :n], lab[b, :n, None].to(det.dtype)], 1).cpu().numpy()
        ref = gold[f'head_res{b}']
        # (the fixture lists detections class-major, the device in score order: same sets, same order within a class)
        got = np.concatenate([got[got[:, 5] == c] for c in range(4)], 0)
        _assert_dets(got, ref, ('head', b))


def test_cascade_split_thr_branch_matches_the_plain_one(gold):
    """K * C >= split_thr: mmcv's per-class NMS branch gives the detections of the plain one"""
    seed = int(gold['seed_head'])
    out = []
    for thr in (10000, 1):
        c = ci.roi_head_cfg()
        c['test_cfg']['nms']['split_thr'] = thr
        rh = build_head(ConfigDict(c))
        rh.load_state_dict(ci.head_state_dict(rh, seed))
        rh = rh.to(DEV).eval()
        nhwc, metas, _, _, dets, num = _head_inputs(seed)
        with torch.no_grad():
            det, lab, nd = rh.simple_test_padded(nhwc, dets, num, metas, rescale=True)
        tabs = []
        for b in range(2):
            n = int(nd[b])
            t = torch.cat([det[b, :n], lab[b, :n, None].to(det.dtype)], 1).cpu().numpy()
            tabs.append(np.concatenate([t[t[:, 5] == c_] for c_ in range(4)], 0))
        out.append(tabs)
    for b in range(2):
        assert len(out[0][b]) > 0 and np.array_equal(out[0][b], out[1][b])


def test_model_end_to_end_golden(gold):
    """section (c): `model(return_loss=False)` of the small fixture model against the reference's run of the same seeded
    model: per class the same detections in the same order, labels exact, boxes and scores within 2e-4.  The fixture
    settles only on inputs whose fp32 reference run is within 5e-5 of its own float64 run (`e2e_ref_err`).  Measured on
    the MI355X against this fixture: largest box / score difference 7.6e-5 / 6.1e-5 over the two images, 1.5e-5 at head
    level (printed below, before the assertion)."""
    seed = int(gold['seed_e2e'])
    m = _model(seed).eval()
    img, _, _, _ = util.demo_inputs(2, fi.H, fi.W, seed=seed)
    with torch.no_grad():
        res = m(return_loss=False, rescale=True, img=[d(img)], img_metas=[fi.metas()])
    for b in range(2):
        assert len(res[b]) == 4 and all(r.dtype == np.float32 and r.shape[1] == 5 for r in res[b])
        _assert_dets(_table(res[b]), gold[f'e2e_res{b}'], ('e2e', b))


def test_two_train_iterations_golden(gold):
    """section (d): the seeded draws come in the reference's order (the RPN's, then stage by stage, image by image,
    positives then negatives)"""
    m = _model(int(gold['seed_e2e'])).train()
    for it in range(2):
        seed = int(gold[f'seed_train{it}'])
        img, metas, gts, gls = util.demo_inputs(2, fi.H, fi.W, seed=seed, num_gt=fi.TRAIN_NUM_GT)
        torch.manual_seed(seed + 100)
        losses = m(img=d(img), img_metas=metas, gt_bboxes=[d(g) for g in gts], gt_labels=[d(l) for l in gls])
        assert sorted(losses) == sorted(['loss_rpn_cls', 'loss_rpn_bbox'] +
                                        [f's{i}.{k}' for i in range(3) for k in ('loss_cls', 'loss_bbox', 'acc')])
        _assert_losses(losses, gold, f'train{it}_')
        loss, _ = m._parse_losses(losses)
        loss.backward()
        assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
        assert m.roi_head.bbox_head[2].fc_cls.weight.grad is not None
        m.zero_grad()


@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
def test_model_16bit_close_to_fp32(gold, dtype):
    """the criterion of tests/test_faster_rcnn_gpu.py::test_model_16bit_close_to_fp32 for the cascade recipe"""
    from brcnn import blocks
    seed = int(gold['seed_e2e'])
    m = _model(seed).eval()
    img, _, _, _ = util.demo_inputs(2, fi.H, fi.W, seed=seed)
    try:
        with torch.no_grad():
            f32 = [f.float() for f in m.extract_feat_nhwc(d(img))]
            r32 = m.simple_test(d(img), fi.metas())
            m.set_compute_dtype(dtype)
            f16 = m.extract_feat_nhwc(d(img))
            assert all(f.dtype == (torch.bfloat16 if dtype == 'bf16' else torch.float16) for f in f16)
            r16 = m.simple_test(d(img), fi.metas())
    finally:
        blocks.set_compute_dtype('f32')
    for a, b in zip(f16, f32):
        assert (a.float() - b).abs().max().item() / b.abs().max().item() < 0.05
    n32, n16 = sum(len(c) for r in r32 for c in r), sum(len(c) for r in r16 for c in r)
    assert n32 > 0 and abs(n16 - n32) <= 0.2 * n32 + 5, (n16, n32)
    dd = np.concatenate([c for r in r32 for c in r]), np.concatenate([c for r in r16 for c in r])
    dist = np.abs(dd[0][:, None, :4] - dd[1][None, :, :4]).max(-1)
    ds = np.abs(dd[0][:, None, 4] - dd[1][None, :, 4])
    assert ((dist < 2.0) & (ds < 0.05)).any(1).mean() > 0.7


def test_16bit_train_step_runs(gold):
    from brcnn import blocks
    m = _model(int(gold['seed_e2e'])).train()
    seed = int(gold['seed_train0'])
    img, metas, gts, gls = util.demo_inputs(2, fi.H, fi.W, seed=seed, num_gt=fi.TRAIN_NUM_GT)
    try:
        m.set_compute_dtype('bf16')
        torch.manual_seed(seed + 100)
        losses = m(img=d(img), img_metas=metas, gt_bboxes=[d(g) for g in gts], gt_labels=[d(l) for l in gls])
        loss, log_vars = m._parse_losses(losses)
        loss.backward()
    finally:
        blocks.set_compute_dtype('f32')
    assert np.isfinite(log_vars['loss']) and all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)


def test_inference_detector_returns_the_bbox2result_layout():
    from brcnn.apis import inference_detector, init_detector
    model = init_detector(ci.CONFIG, None, device=DEV)
    img = np.random.RandomState(0).randint(0, 255, (120, 160, 3), dtype=np.uint8)
    res = inference_detector(model, img)
    assert isinstance(res, list) and len(res) == 4
    assert all(isinstance(r, np.ndarray) and r.dtype == np.float32 and r.ndim == 2 and r.shape[1] == 5 for r in res)
    both = inference_detector(model, [img, img[:, ::-1].copy()])
    assert len(both) == 2 and all(len(r) == 4 for r in both)
