"""-m gpu: the Faster R-CNN baseline on the device path.

  * the proposal stage of RPNHead, StandardRoIHead, the recipe end to end, the ablation's two mixes and two train
    iterations against what the imported reference computed (tests/golden/g25_faster_rcnn.npz);
  * the sampled RPN loss kernels (csrc/rpn_sampled.hip) against the float64 reference tests/rpn_sampled_ref64.py, which
    tests/test_faster_rcnn_cpu.py pins to the fixture;
  * brcnn_rcnn_decode_plain against a float64 restatement of softmax -> delta2bbox -> clip -> rescale.

Tolerances.  Against the fixture: the ones tests/test_golden_gpu.py applies to the same kind of data (g5_rpn_get_bboxes:
boxes 2e-4 px, scores 1e-6; g8_g9_test_head: labels exact, detections 2e-4) and the golden train iterations of the
boosting recipes (rtol 2e-3, atol 1e-4).  Against float64: stated where used, from the fp32 summation bound of the number
of terms and the fp32 evaluation error of the terms -- none is tuned to what the kernels return.
"""
import math
import os

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import build_detector, build_head, core, ops, train_ops
from brcnn.config import ConfigDict
from tests import faster_rcnn_inputs as fi
from tests import rpn_sampled_ref64 as R
from tests import util

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G = os.path.join(os.path.dirname(__file__), 'golden', 'g25_faster_rcnn.npz')
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope='module')
def gold():
    return {k: v for k, v in np.load(G, allow_pickle=False).items()}


def T(a):
    return torch.from_numpy(np.asarray(a))


# ------------------------------------------------------------------------------------------- proposals vs the fixture
@pytest.mark.parametrize('name', list(fi.PROPOSAL_CFGS))
def test_rpn_proposals_golden(gold, name):
    """levels 16 x 24 .. 1 x 2 at nms_pre=50: three levels go through the selection, two pass through; 'minsize' drops
    rows by min_bbox_size, in 'empty' nothing of image 1 survives.  Same rows in the same order as the reference (the
    generator asserted that no NMS IoU / score boundary is within rounding reach)"""
    seed = int(gold['seed_props'])
    head = build_head(ConfigDict(fi.rpn_head_cfg())).to(DEV).eval()
    cls, reg = fi.rpn_outputs(seed, empty=(name == 'empty'))
    res = head.get_bboxes([c.to(DEV) for c in cls], [r.to(DEV) for r in reg], fi.metas(),
                          cfg=ConfigDict(fi.PROPOSAL_CFGS[name]))
    for b in range(2):
        ref, got = T(gold[f'props_{name}{b}']), res[b].cpu()
        assert got.shape == ref.shape, (name, b, got.shape, ref.shape)
        assert torch.allclose(got[:, :4], ref[:, :4], rtol=0, atol=2e-4), (name, b)
        assert torch.allclose(got[:, 4], ref[:, 4], rtol=0, atol=1e-6), (name, b)
    if name == 'empty':
        assert res[1].shape == (0, 5) and len(res[0]) > 0
    if name == 'minsize':
        assert not np.array_equal(gold['props_minsize0'], gold['props_train0'])       # the filter removed rows


# ------------------------------------------------------------------------------------------- sampled RPN loss vs float64
SIZES, STRIDES, NA = [(16, 24), (3, 4), (1, 1)], [4, 16, 64], 3       # 1152 + 36 + 3 anchors; the last level is one cell
NUM, NUM_POS, YS = 256, 128, 32


def _case(name):
    """hand-set gt_inds (no assigner), seeded head output; returns everything a sampled-loss call takes"""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    B = 2
    n = sum(h * w for h, w in SIZES) * NA
    gen = core.AnchorGenerator(strides=STRIDES, ratios=[0.5, 1.0, 2.0], scales=[8])
    anchors = torch.cat(gen.grid_anchors(SIZES, 'cpu'))
    gts = [util.rand_boxes(4, img_w=96., img_h=64., seed=3, min_size=6., max_size=60.),
           util.rand_boxes(3, img_w=96., img_h=64., seed=4, min_size=6., max_size=60.)]
    gt_inds = torch.zeros(B, n, dtype=torch.int32)
    n_pos, ignore = [20, 9], 0.1
    kw = dict(pos_weight=-1.0, beta=0.0)
    if name == 'no_gt_image':
        gts[1] = gts[1][:0]
        n_pos = [20, 0]
    elif name == 'many_pos':
        n_pos = [200, 131]                              # more than 128: the positives are subsampled
    elif name == 'few_neg':
        ignore = 0.97                                   # ~35 negatives per image: fewer than the sampler asks for
    elif name == 'zero_pos':
        n_pos = [0, 0]
    elif name == 'pos_weight':
        kw['pos_weight'] = 2.5
    elif name == 'smooth_l1':
        kw['beta'] = 1.0 / 9.0
    for b in range(B):
        gt_inds[b][torch.rand(n, generator=g) < ignore] = -1
        pos = torch.randperm(n, generator=g)[:n_pos[b]]
        if n_pos[b]:
            pos[0] = n - 1                              # the one-cell level takes part
            gt_inds[b][pos] = torch.randint(1, len(gts[b]) + 1, (n_pos[b],), generator=g, dtype=torch.int32)
    rows = sum(B * h * w for h, w in SIZES)
    y = torch.zeros(rows, YS)
    y[:, :NA] = torch.randn(rows, NA, generator=g) * 3
    y[:, NA:5 * NA] = torch.randn(rows, 4 * NA, generator=g) * 0.5
    y[:, 5 * NA:] = 7.0                                 # padding columns: never read, their gradient is zero
    if name == 'smooth_l1':                             # both sides of the knee occur: asserted from the reference below
        y[:, NA:5 * NA] *= 0.3
    offs = [0, len(gts[0]), len(gts[0]) + len(gts[1])]
    return dict(B=B, n=n, gen=gen, anchors=anchors, gts=torch.cat(gts), offs=offs, gt_inds=gt_inds, y=y, **kw)


def _y_to_levels(y, B):
    """fused rows -> per-level (B, A, h, w) / (B, 4A, h, w) arrays, the layout rpn_sampled_ref64 flattens"""
    cls, reg, r0 = [], [], 0
    for h, w in SIZES:
        t = y[r0:r0 + B * h * w].view(B, h, w, -1)
        cls.append(t[..., :NA].permute(0, 3, 1, 2).numpy())
        reg.append(t[..., NA:5 * NA].permute(0, 3, 1, 2).numpy())
        r0 += B * h * w
    return cls, reg


@pytest.mark.parametrize('name', ['plain', 'no_gt_image', 'many_pos', 'few_neg', 'zero_pos', 'pos_weight', 'smooth_l1'])
def test_sampled_rpn_loss_against_float64(name):
    """Loss values: |kernel - float64| <= (n + 8) eps32 sum|terms| (+ the encoded targets' fp32 error for the box term),
    n the number of terms summed (rpn_sampled_ref64.loss_tolerance).  Gradients: the objectness gradient k w (sigmoid - t)
    within 8 eps32 of k w (expf to 2 ulp, one division, one product); the L1 box gradient is +-k EXACTLY unless
    |pred - target| is below the target's own fp32 error; inside the SmoothL1 knee it is k d / beta, held to k (target
    error + 4 eps32 |d|) / beta.  Undrawn anchors and padding columns: exactly 0.  Two runs: the same bits."""
    c = _case(name)
    B, n = c['B'], c['n']
    cnt = [(int((c['gt_inds'][b] > 0).sum()), int((c['gt_inds'][b] == 0).sum())) for b in range(B)]
    torch.manual_seed(5)
    perm, _ = train_ops.draw_sampler_perms(cnt, NUM, NUM_POS, -1)
    total = train_ops.rpn_num_total_samples(cnt, NUM, NUM_POS, -1)
    base = [b.to(DEV) for b in c['gen'].base_anchors]
    meta = train_ops.RPNSampledMeta(B, SIZES, c['gen'].strides, base, NA, c['offs'], NUM, NUM_POS, -1, c['pos_weight'],
                                    c['beta'], (0., 0., 0., 0.), (1., 1., 1., 1.), 1.0, 1.0)
    gi, gts = c['gt_inds'].to(DEV), c['gts'].to(DEV)
    drawn, ws = train_ops.rpn_sampled_draw(gi, perm.to(DEV), meta)
    # the drawing contract, restated on the host: candidates in index order, the host's permutation picks
    want = np.full((B, NUM), -1, np.int64)
    for b, (p_, n_) in enumerate(cnt):
        pos = torch.nonzero(c['gt_inds'][b] > 0).reshape(-1).numpy()
        neg = torch.nonzero(c['gt_inds'][b] == 0).reshape(-1).numpy()
        spos, sneg, eneg = train_ops.sample_counts(p_, n_, NUM, NUM_POS, -1)
        ps = pos[perm[b, :NUM_POS].numpy()] if p_ > NUM_POS else pos
        ns = neg[perm[b, NUM_POS:NUM_POS + eneg].numpy()] if n_ > eneg else neg
        want[b, :spos], want[b, spos:spos + sneg] = ps[:spos], ns[:sneg]
    assert np.array_equal(drawn.cpu().numpy(), want)
    if name == 'many_pos':
        assert all(p_ > NUM_POS for p_, _ in cnt)
    if name == 'few_neg':
        assert all(n_ < NUM - min(p_, NUM_POS) for p_, n_ in cnt)

    runs = []
    for _ in range(2):
        y = c['y'].to(DEV).requires_grad_()
        losses2 = train_ops.rpn_sampled_loss(y, gi, gts, drawn, meta, total)
        (losses2[0] * 1.5 + losses2[1] * 0.5).backward()
        runs.append((losses2.detach().cpu(), y.grad.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    got, dy = runs[0][0].double().numpy(), runs[0][1]

    cls, reg = _y_to_levels(c['y'], B)
    x, p = R.flatten_outputs(cls, reg)
    ref = R.sampled_rpn_loss(x, p, c['anchors'].numpy(), c['gt_inds'].numpy(), c['gts'].numpy(), c['offs'], want, total,
                             pos_weight=c['pos_weight'], beta=c['beta'])
    tol_c, tol_b = R.loss_tolerance(ref)
    assert ref['n_cls'] == sum(int((w_ >= 0).sum()) for w_ in want)
    assert abs(got[0] - ref['loss_cls']) <= tol_c, (got[0], ref['loss_cls'], tol_c)
    assert abs(got[1] - ref['loss_bbox']) <= tol_b, (got[1], ref['loss_bbox'], tol_b)
    if ref['n_bbox'] == 0:
        assert got[1] == 0.0
    # gradients, in the reference's flattened order
    dcls, dreg, r0 = [], [], 0
    for h, w in SIZES:
        t = dy[r0:r0 + B * h * w].view(B, h * w, YS)
        dcls.append(t[..., :NA].reshape(B, -1))
        dreg.append(t[..., NA:5 * NA].reshape(B, -1, 4))
        assert (t[..., 5 * NA:] == 0).all()
        r0 += B * h * w
    dx, dp = torch.cat(dcls, 1).double().numpy(), torch.cat(dreg, 1).double().numpy()
    k = 1.0 / total
    rdx, rdp = 1.5 * ref['dx'], 0.5 * ref['dpred']
    undrawn = np.ones((B, n), bool)
    for b in range(B):
        undrawn[b, want[b][want[b] >= 0]] = False
    assert (dx[undrawn] == 0).all() and (dp[undrawn] == 0).all()
    wmax = max(c['pos_weight'], 1.0)
    assert np.abs(dx - rdx).max() <= 8 * EPS32 * 1.5 * k * wmax
    posrow = ref['terr'].sum(-1) > 0
    if ref['n_bbox'] == 0:
        assert (dp == 0).all()
    else:
        # |pred - target| in float64 from the reference gradient's support
        diff = np.zeros_like(p)
        for b in range(B):
            idx = want[b][want[b] >= 0]
            pi = idx[c['gt_inds'][b].numpy()[idx] > 0]
            t, _ = R.encode(c['anchors'].numpy()[pi].astype(np.float64),
                            c['gts'].numpy().astype(np.float64)[c['offs'][b] + c['gt_inds'][b].numpy()[pi] - 1],
                            (0., 0., 0., 0.), (1., 1., 1., 1.))
            diff[b, pi] = p[b, pi] - t
        ad, terr = np.abs(diff), ref['terr']
        kb = 0.5 * k
        if c['beta'] > 0:
            inside, outside = posrow[..., None] & (ad < c['beta'] - terr), posrow[..., None] & (ad > c['beta'] + terr)
            assert inside.sum() > 10 and outside.sum() > 10
            assert (np.abs(dp - rdp)[inside] <= (kb * (terr + 4 * EPS32 * ad) / c['beta'] + 2 * EPS32 * np.abs(rdp))[inside]).all()
        else:
            outside = posrow[..., None] & (ad > terr)
        # (k = 1 / total rounded once to fp32, the upstream gradient 0.5 a power of two: +-float32(kb) are the exact bits)
        assert (dp[outside] == np.float64(np.float32(kb)) * np.sign(diff)[outside]).all()
        assert (dp[~np.broadcast_to(posrow[..., None], dp.shape)] == 0).all()


def test_sampled_rpn_loss_through_the_head_matches_the_host_path(gold):
    """RPNHead.loss on device tensors (assignment kernel, device compaction, host draw, loss kernels) gives the
    fixture's draw and losses: the same anchors, per-level sums within the fp32 bound of the float64 reference"""
    seed = int(gold['seed_rpnloss'])
    head = build_head(ConfigDict(fi.rpn_head_cfg())).to(DEV).train()
    cls, reg = fi.rpn_outputs(seed)
    gt_bboxes, _ = fi.gts(seed)
    torch.manual_seed(seed + 100)
    losses = head.loss([t.to(DEV).requires_grad_() for t in cls], [t.to(DEV) for t in reg], [g.to(DEV) for g in gt_bboxes],
                       fi.metas())
    gt_inds, drawn, total = head.last_rpn_targets
    drawn = drawn.cpu().numpy()
    for b in range(2):
        pos, neg = gold[f'rpnloss_pos{b}'], gold[f'rpnloss_neg{b}']
        assert total == sum(max(len(gold[f'rpnloss_pos{i}']), 1) + max(len(gold[f'rpnloss_neg{i}']), 1) for i in range(2))
        # the reference sorts its picks (`unique`); the device keeps the draw order: the same sets
        assert sorted(drawn[b, :len(pos)].tolist()) == pos.tolist()
        assert sorted(drawn[b, len(pos):len(pos) + len(neg)].tolist()) == neg.tolist()
    x, p = R.flatten_outputs([c.numpy() for c in cls], [r.numpy() for r in reg])
    anchors = torch.cat(head.anchor_generator.grid_anchors(fi.SIZES, 'cpu')).numpy()
    offs = [0, len(gt_bboxes[0]), len(gt_bboxes[0]) + len(gt_bboxes[1])]
    ref = R.sampled_rpn_loss(x, p, anchors, gt_inds.cpu().numpy(), torch.cat(gt_bboxes).numpy(), offs, drawn, total)
    tol_c, tol_b = R.loss_tolerance(ref)
    assert abs(float(losses['loss_rpn_cls'][0].detach()) - ref['loss_cls']) <= tol_c
    assert abs(float(losses['loss_rpn_bbox'][0].detach()) - ref['loss_bbox']) <= tol_b
    assert abs(ref['loss_cls'] - gold['rpnloss_loss_rpn_cls'].astype(np.float64).sum()) <= tol_c + 8 * EPS32 * ref['loss_cls']


# ------------------------------------------------------------------------------------------- plain second-stage decode
def _decode64(probs, bbox_pred, dets, num, max_shape, sf, C, thr, means, stds, agnostic):
    B, K, _ = dets.shape
    pr = dets[..., :4].double().reshape(B * K, 4)
    d = bbox_pred.double().reshape(B * K, -1, 4)
    d = d.expand(B * K, C, 4) if agnostic else d
    m, s = torch.tensor(means).double(), torch.tensor(stds).double()
    d = d * s + m
    lim = abs(math.log(16 / 1000))
    px, py = ((pr[:, 0] + pr[:, 2]) * 0.5)[:, None], ((pr[:, 1] + pr[:, 3]) * 0.5)[:, None]
    pw, ph = (pr[:, 2] - pr[:, 0])[:, None], (pr[:, 3] - pr[:, 1])[:, None]
    gw, gh = pw * d[..., 2].clamp(-lim, lim).exp(), ph * d[..., 3].clamp(-lim, lim).exp()
    gx, gy = px + pw * d[..., 0], py + ph * d[..., 1]
    box = torch.stack([gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5], -1).view(B, K, C, 4)
    mag = torch.stack([gx.abs() + gw, gy.abs() + gh, gx.abs() + gw, gy.abs() + gh], -1).view(B, K, C, 4)
    hi = max_shape.double()[:, [1, 0, 1, 0]].view(B, 1, 1, 4)
    box = torch.minimum(box.clamp(min=0), hi)
    if sf is not None:
        box, mag = box / sf.double().view(B, 1, 1, 4), mag / sf.double().view(B, 1, 1, 4)
    ok = torch.arange(K)[None, :] < num[:, None]
    valid = (probs.view(B, K, C + 1)[..., :C] > thr) & ok[..., None]
    return box.reshape(B, K * C, 4), mag.reshape(B, K * C, 4), valid.reshape(B, K * C)


@pytest.mark.parametrize('C', [1, 4])
@pytest.mark.parametrize('K', [1, 7, 256])
@pytest.mark.parametrize('agnostic', [False, True])
def test_rcnn_decode_plain_against_float64(C, K, agnostic):
    """scores are the probabilities handed in, bit for bit; valid = (prob > score_thr) & the row is real, exactly (one
    probability is set to score_thr itself, one to the next float above); boxes within 8 eps32 of (|centre| + size):
    six fp32 operations from the proposal to the corner, expf to 2 ulp, the clip and the division by the scale factor
    do not enlarge an error.  The existing fused entry gets the same check beside it, with its sqrt(prob * prior)."""
    g = torch.Generator().manual_seed(100 * C + K + int(agnostic))
    B, thr = 3, 0.05
    dets = torch.cat([util.rand_boxes(B * K, seed=K + C), torch.rand(B * K, 1, generator=g)], 1).view(B, K, 5)
    num = torch.tensor([K, (K + 1) // 2, 0], dtype=torch.int32)              # full, padded rows, none
    dets[1, int(num[1]):] = 0
    dets[2] = 0
    probs = (torch.randn(B * K, C + 1, generator=g) * 2).softmax(1)
    probs[0, 0] = thr
    probs[0, C] = float(np.nextafter(np.float32(thr), np.float32(1)))
    probs[0, 0], probs[0, C] = probs[0, C].clone(), probs[0, 0].clone()      # column 0 just above, the bg column at thr
    if K > 1:
        probs[1, 0] = thr                                                      # exactly thr: not valid
    reg = torch.randn(B * K, 4 if agnostic else 4 * C, generator=g) * 0.5
    reg[0, :4] = torch.tensor([0., 0., 60., -60.])                             # both ends of the ratio clip
    max_shape = torch.tensor([[800., 1333.], [750., 1200.], [640., 640.]])
    sf = torch.tensor([[1.1, 1.2, 1.1, 1.2], [1., 1., 1., 1.], [0.5, 0.5, 0.5, 0.5]])
    means, stds = (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)
    d = lambda t: t.to(DEV)   # noqa: E731
    for scale in (sf, None):
        box64, mag, valid = _decode64(probs, reg, dets, num, max_shape, scale, C, thr, means, stds, agnostic)
        bb, sc, lb, va = ops.rcnn_decode_plain(d(probs), d(reg), d(dets), d(num), d(max_shape), None if scale is None else d(scale),
                                               C, thr, means, stds, reg_class_agnostic=agnostic)
        assert torch.equal(sc.cpu(), probs.view(B, K, C + 1)[..., :C].reshape(B, K * C))
        assert torch.equal(va.cpu(), valid) and bool(valid[0, 0]) and (K == 1 or not bool(valid[0, C]))
        assert not va[2].any() and not va[1].view(K, C)[int(num[1]):].any()
        assert torch.equal(lb.cpu(), torch.arange(C).repeat(B, K))
        assert ((bb.cpu().double() - box64).abs() <= 8 * EPS32 * mag + 1e-30).all()
    if not agnostic:
        box64, mag, _ = _decode64(probs, reg, dets, num, max_shape, sf, C, thr, means, stds, False)
        bb, sc, lb, va = ops.rcnn_decode(d(probs), d(reg), d(dets), d(num), d(max_shape), d(sf), C, thr, means, stds)
        s64 = (probs.double().view(B, K, C + 1)[..., :C] * dets[..., 4:5].double()).sqrt().reshape(B, K * C)
        assert ((sc.cpu().double() - s64).abs() <= 2 * EPS32 * s64).all()      # one product, one sqrt
        assert ((bb.cpu().double() - box64).abs() <= 8 * EPS32 * mag + 1e-30).all()
        ok = (torch.arange(K)[None, :] < num[:, None]).repeat_interleave(C, 1)
        clear = (s64 - thr).abs() > 4 * EPS32
        assert torch.equal(va.cpu()[clear], ((s64 > thr) & ok)[clear])


# ------------------------------------------------------------------------------------------- heads and models vs the fixture
def _table(res):
    return np.concatenate([np.concatenate([r, np.full((len(r), 1), c, np.float32)], 1) for c, r in enumerate(res)], 0)


def _assert_dets(got, ref, what):
    """labels and kept order exact, boxes and scores under the g8_g9_test_head tolerance of tests/test_golden_gpu.py"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(got[:, 5], ref[:, 5]), what
    print(what, 'largest box / score difference', float(np.abs(got[:, :5] - ref[:, :5]).max()) if len(ref) else 0.0)
    assert np.allclose(got[:, :5], ref[:, :5], rtol=0, atol=2e-4), (what, np.abs(got[:, :5] - ref[:, :5]).max())


def _model(cfg, seed, dtype='f32'):
    m = build_detector(ConfigDict(cfg))
    m.load_state_dict(fi.fixture_state_dict(m, seed))
    return m.to(DEV)


@pytest.mark.parametrize('tag,kind', [('std', 'StandardRoIHead'), ('prob', 'ProbRoIHead')])
def test_roi_heads_golden(gold, tag, kind):
    """head level: forward_train (whole-batch device sampler, `_ex` loss kernels) and the device test path of
    StandardRoIHead, and of ProbRoIHead on 5-column proposals, on the seeded pyramid"""
    seed = int(gold[f'seed_{tag}'])
    rh = build_head(ConfigDict(fi.roi_head_cfg(kind)))
    rh.load_state_dict(util.seeded_state_dict(rh, seed=seed))
    rh = rh.to(DEV)
    feats, metas, gts, gls, props = fi.roi_inputs(seed)
    nhwc = [f.to(DEV).permute(0, 2, 3, 1).contiguous() for f in feats]
    K = max(len(p) for p in props)
    dets = torch.zeros(2, K, 5)
    for b, p in enumerate(props):
        dets[b, :len(p)] = p
    num = torch.tensor([len(p) for p in props], dtype=torch.int32)
    rh.train()
    assert rh.device_train_ok()
    torch.manual_seed(seed + 100)
    gt_flat = train_ops.flatten_gts([g.to(DEV) for g in gts], [l.to(DEV) for l in gls])
    losses, _ = rh.forward_train_device([f.requires_grad_() for f in nhwc], metas, dets.to(DEV), num.to(DEV), gt_flat)
    for k in ('loss_cls', 'loss_bbox', 'acc'):
        got, ref = losses[k].detach().cpu().reshape(-1), T(gold[f'{tag}_train_{k}']).reshape(-1)
        assert torch.allclose(got, ref, rtol=2e-3, atol=1e-4), (k, got, ref)
    sum(v for k, v in losses.items() if 'loss' in k).backward()
    rh.eval()
    with torch.no_grad():
        det, lab, nd = rh.simple_test_padded([f.detach() for f in nhwc], dets.to(DEV), num.to(DEV), metas, rescale=True)
    for b in range(2):
        n = int(nd[b])
        assert torch.equal(lab[b, :n].cpu(), T(gold[f'{tag}_lab{b}'])), (tag, b)
        assert torch.allclose(det[b, :n].cpu(), T(gold[f'{tag}_det{b}']), rtol=0, atol=2e-4), (tag, b)


@pytest.mark.parametrize('tag', ['e2e', 'atss_std', 'rpn_prob'])
def test_model_end_to_end_golden(gold, tag):
    """`model(return_loss=False)` of the recipe ('e2e') and of the ablation's two mixes against the reference's run of
    the same seeded model: per class the same number of detections in the same order, labels exact, boxes and scores
    within 2e-4 (the head-level tolerance of g8_g9_test_head, which the issue sets for this end-to-end comparison too).

    The fixture's end-to-end sections settle only on inputs whose fp32 reference run is itself within 5e-5 of the float64
    run of the same model (make_golden_faster_rcnn.py: REF_MARGIN; recorded as `<tag>_ref_err`, 2.0e-5 .. 2.4e-5), so the
    bound measures the device and not the reference's own round-off: with proposal deltas four times larger the
    reference alone sat 1.1e-4 from float64 at the proposal stage, and the device 2.1e-4 .. 3.1e-4 from the reference.
    Measured on the MI355X against this fixture: largest box / score difference 3.6e-5 .. 5.3e-5 over the three cases
    (printed below, before the assertion)."""
    seed = int(gold[f'seed_{tag}'])
    cfg = fi.fixture_model_cfg() if tag == 'e2e' else fi.cross_model_cfg(tag)
    m = _model(cfg, seed).eval()
    img, _, _, _ = util.demo_inputs(2, fi.H, fi.W, seed=seed)
    with torch.no_grad():
        res = m(return_loss=False, rescale=True, img=[img.to(DEV)], img_metas=[fi.metas()])
    for b in range(2):
        assert len(res[b]) == 4 and all(r.dtype == np.float32 and r.shape[1] == 5 for r in res[b])
        _assert_dets(_table(res[b]), gold[f'{tag}_res{b}'], (tag, b))


@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
def test_model_16bit_close_to_fp32(gold, dtype):
    """the criterion of tests/test_bf16_gpu.py::test_detector_bf16_close_to_fp32 (and its f16 twin) for the UTDAC recipe"""
    from brcnn import blocks
    seed = int(gold['seed_e2e'])
    m = _model(fi.fixture_model_cfg(), seed).eval()
    img, _, _, _ = util.demo_inputs(2, fi.H, fi.W, seed=seed)
    try:
        with torch.no_grad():
            f32 = [f.float() for f in m.extract_feat_nhwc(img.to(DEV))]
            r32 = m.simple_test(img.to(DEV), fi.metas())
            m.set_compute_dtype(dtype)
            f16 = m.extract_feat_nhwc(img.to(DEV))
            assert all(f.dtype == (torch.bfloat16 if dtype == 'bf16' else torch.float16) for f in f16)
            r16 = m.simple_test(img.to(DEV), fi.metas())
    finally:
        blocks.set_compute_dtype('f32')
    for a, b in zip(f16, f32):
        assert (a.float() - b).abs().max().item() / b.abs().max().item() < 0.05
    n32, n16 = sum(len(c) for r in r32 for c in r), sum(len(c) for r in r16 for c in r)
    assert n32 > 0 and abs(n16 - n32) <= 0.2 * n32 + 5, (n16, n32)
    d = np.concatenate([c for r in r32 for c in r]), np.concatenate([c for r in r16 for c in r])
    dist = np.abs(d[0][:, None, :4] - d[1][None, :, :4]).max(-1)
    ds = np.abs(d[0][:, None, 4] - d[1][None, :, 4])
    assert ((dist < 2.0) & (ds < 0.05)).any(1).mean() > 0.7


def test_inference_detector_returns_the_bbox2result_layout():
    from brcnn.apis import inference_detector, init_detector
    model = init_detector(fi.CONFIG, None, device=DEV)
    img = np.random.RandomState(0).randint(0, 255, (120, 160, 3), dtype=np.uint8)
    res = inference_detector(model, img)
    assert isinstance(res, list) and len(res) == 4
    assert all(isinstance(r, np.ndarray) and r.dtype == np.float32 and r.ndim == 2 and r.shape[1] == 5 for r in res)
    both = inference_detector(model, [img, img[:, ::-1].copy()])
    assert len(both) == 2 and all(len(r) == 4 for r in both)


# ------------------------------------------------------------------------------------------- train
def test_two_train_iterations_golden(gold):
    m = _model(fi.fixture_model_cfg(), int(gold['seed_e2e'])).train()
    for it in range(2):
        seed = int(gold[f'seed_train{it}'])
        img, metas, gts, gls = util.demo_inputs(2, fi.H, fi.W, seed=seed, num_gt=fi.TRAIN_NUM_GT)
        torch.manual_seed(seed + 100)
        losses = m(img=img.to(DEV), img_metas=metas, gt_bboxes=[g.to(DEV) for g in gts], gt_labels=[l.to(DEV) for l in gls])
        assert sorted(losses) == ['acc', 'loss_bbox', 'loss_cls', 'loss_rpn_bbox', 'loss_rpn_cls']
        for k, v in losses.items():
            got = (sum(v) if isinstance(v, list) else v).detach().cpu().double().reshape(-1)
            ref = T(gold[f'train{it}_{k}']).double().sum().reshape(-1)
            assert torch.allclose(got, ref, rtol=2e-3, atol=1e-4), (it, k, got, ref)
        m.zero_grad()


def test_bf16_train_step_is_reproducible_and_fused_sgd_follows(gold):
    from brcnn import blocks
    from brcnn.optim import FusedSGD
    m = _model(fi.fixture_model_cfg(), int(gold['seed_e2e'])).train()
    seed = int(gold['seed_train0'])
    img, metas, gts, gls = util.demo_inputs(2, fi.H, fi.W, seed=seed, num_gt=fi.TRAIN_NUM_GT)
    data = dict(img=img.to(DEV), img_metas=metas, gt_bboxes=[g.to(DEV) for g in gts], gt_labels=[l.to(DEV) for l in gls])
    opt = FusedSGD([p for p in m.parameters() if p.requires_grad], lr=0.01, momentum=0.9, weight_decay=1e-4)
    try:
        m.set_compute_dtype('bf16')
        runs = []
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            torch.manual_seed(seed + 100)
            out = m.train_step(data, opt)
            out['loss'].backward()
            grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
            runs.append((dict(out['log_vars'].items()), grads))
        assert runs[0][0] == runs[1][0]
        assert runs[0][1].keys() == runs[1][1].keys() and 'rpn_head.rpn_conv.weight' in runs[0][1]
        assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
        before = m.rpn_head.rpn_cls.weight.detach().clone()
        opt.step()
        torch.cuda.synchronize()
        assert not torch.equal(before, m.rpn_head.rpn_cls.weight.detach())
        assert all(torch.isfinite(p).all() for p in m.parameters())
    finally:
        blocks.set_compute_dtype('f32')
