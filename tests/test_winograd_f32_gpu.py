"""-m gpu: the Winograd F(2x2,3x3) form of the fp32 3x3 stride-1 convs (csrc/conv_winograd_f32.hip).

* against float64 at the suite's fp32 bound (route_util), every case proven to have taken the Winograd route by its counter
  (brcnn_conv_set_tile(-12, 0)); the route's own error and the direct kernel's on the same inputs are printed;
* the GroupNorm + ReLU prologue of the input transform: equal BITS to GroupNorm launch -> Winograd conv, both inside the
  float64 bound, and a reference that normalises the PADDED tensor (the halo mistake) outside it;
* the transformed-filter cache follows load_state_dict on a frozen model;
* the frozen model (four Winograd launches per pass) against the non-frozen one (none): fused head outputs and detections;
* what the entry points refuse.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import brcnn  # noqa: F401
from brcnn import Config, build_detector, lib, ops
from tests import route_util, util
from tests.test_host_cpu import CFG

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _match_dets(got, ref, box_tol=1e-2, score_tol=1e-3):
    """fraction of reference detections that have a counterpart (same place, same score): tests/test_golden_gpu.py's"""
    if len(ref) == 0:
        return 1.0 if len(got) == 0 else 0.0
    if len(got) == 0:
        return 0.0
    d = np.abs(ref[:, None, :4] - got[None, :, :4]).max(-1)
    s = np.abs(ref[:, None, 4] - got[None, :, 4])
    return ((d < box_tol) & (s < score_tol)).any(1).mean()


def _close(a, b, tol=2e-4):
    """tests/test_golden_gpu.py's: max |a - b| relative to the magnitude of the reference tensor"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return (a - b).abs().max().item() <= tol * max(b.abs().max().item(), 1e-6)


def _wino_launches():
    return lib.load().brcnn_conv_set_tile(-12, 0)


def _tiles(batch, sizes):
    return sum(batch * ((h + 1) // 2) * ((w + 1) // 2) for h, w in sizes)


def _inputs(batch, sizes, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    rows = sum(batch * h * w for h, w in sizes)
    x = torch.randn(rows, cin, generator=g).to(DEV)
    w = (torch.randn(cout, 3, 3, cin, generator=g) * (1.0 / (3.0 * cin ** 0.5))).to(DEV)
    return x, w


def _segments(t, batch, sizes):
    """(rows, C) -> [(N,H,W,C) per segment]"""
    out, r0 = [], 0
    for h, w in sizes:
        n = batch * h * w
        out.append(t[r0:r0 + n].view(batch, h, w, t.shape[1]))
        r0 += n
    return out


def _ref64(x, w, batch, sizes, scale=None, shift=None, relu=False):
    return torch.cat([route_util.conv_ref64(s, w, scale, shift, None, relu, 1, 1).reshape(-1, w.shape[0])
                      for s in _segments(x, batch, sizes)])


SINGLE = [(2, 7, 11), (1, 13, 21), (2, 1, 5), (1, 2, 2), (1, 5, 1), (2, 8, 12)]
CASES = [(n, [(h, w)], ci, co, False) for (n, h, w) in SINGLE for ci, co in ((32, 64), (256, 256))] + \
        [(2, [(8, 12), (5, 7), (3, 3), (1, 2)], 256, 256, False), (2, [(7, 11)], 256, 256, True)]


@pytest.mark.parametrize('batch,sizes,cin,cout,readout', CASES)
def test_winograd_conv_against_float64(batch, sizes, cin, cout, readout):
    L = lib.load()
    x, w = _inputs(batch, sizes, cin, cout, seed=100 + cin + 7 * len(sizes) + sizes[0][0] * 31 + sizes[0][1])
    scale = shift = None
    if readout:
        g = torch.Generator().manual_seed(5)
        scale = (torch.rand(cout, generator=g) + 0.5).to(DEV)
        shift = torch.randn(cout, generator=g).to(DEV)
    u = ops.winograd_filter(w)
    route_util.clear(L)
    y = ops.conv3x3_winograd_multi(x, u, batch, sizes, scale=scale, shift=shift, relu=readout)
    assert _wino_launches() == 1 and L.brcnn_conv_set_tile(-12, 1) == _tiles(batch, sizes)
    yd, _ = ops.conv2d_nhwc_multi(x, w, batch, sizes, scale, shift, None, readout, 1, 1)
    assert _wino_launches() == 0                     # the direct kernel is another route
    ref = _ref64(x, w, batch, sizes, scale, shift, readout)
    mag = max(1.0, ref.abs().max().item())
    ew, ed = (y.double() - ref).abs().max().item(), (yd.double() - ref).abs().max().item()
    print(f'winograd {batch}x{sizes} {cin}->{cout}: largest error / magnitude: winograd {ew / mag:.3e}, direct {ed / mag:.3e}')
    assert route_util.excess(y, ref, y.dtype) <= 0
    assert torch.isfinite(y).all()


def _gn64(x, gamma, beta, groups, eps, relu, pad):
    """float64 GroupNorm(+ReLU) of one (N,H,W,C) segment; pad = True: the deliberately WRONG form that normalises the
    zero-padded tensor's border too (statistics still from the map itself) -- what a prologue that forgets the halo gives"""
    n, h, w, c = x.shape
    xd = x.double()
    g = xd.reshape(n, h * w, groups, c // groups)
    mean = g.mean((1, 3), keepdim=True)
    var = (g * g).mean((1, 3), keepdim=True) - mean * mean
    rstd = 1.0 / torch.sqrt(var.clamp_min(0) + eps)

    def apply(t):
        hh, ww = t.shape[1:3]
        o = ((t.reshape(n, hh * ww, groups, c // groups) - mean) * rstd).reshape(n, hh, ww, c) * gamma.double() + beta.double()
        return o.relu() if relu else o
    if not pad:
        return apply(xd), 0
    return apply(F.pad(xd, (0, 0, 1, 1, 1, 1))), 1


def test_groupnorm_prologue_bits_and_halo():
    L = lib.load()
    batch, sizes, c, groups, eps = 2, [(7, 11), (4, 6), (1, 3)], 256, 32, 1e-5
    x, w = _inputs(batch, sizes, c, c, seed=77)
    x = x * 1.7 + 0.3
    g = torch.Generator().manual_seed(78)
    gamma = (torch.rand(c, generator=g) + 0.5).to(DEV)
    beta = (torch.rand(c, generator=g) * 0.5 + 0.25).to(DEV)         # > 0 on every channel: relu(beta - ...) != 0 in a wrong halo
    u = ops.winograd_filter(w)
    xn, stats = ops.groupnorm_nhwc_multi(x, gamma, beta, groups, batch, sizes, eps, True, return_stats=True)
    route_util.clear(L)
    y_two = ops.conv3x3_winograd_multi(xn, u, batch, sizes)
    y_one = ops.conv3x3_winograd_multi(x, u, batch, sizes, gn=(stats, gamma, beta, groups, True))
    assert _wino_launches() == 2
    assert torch.equal(y_one, y_two)
    # the statistics-only entry leaves what the full call leaves (up to the order of its double atomics)
    stats2 = ops.groupnorm_stats_multi(x, groups, batch, sizes, eps)
    assert torch.allclose(stats2.view(torch.float32).view(-1, 4)[:, :2], stats.view(torch.float32).view(-1, 4)[:, :2], rtol=1e-6, atol=0)
    good, bad = [], []
    for s in _segments(x, batch, sizes):
        a, _ = _gn64(s, gamma, beta, groups, eps, True, pad=False)
        good.append(route_util.conv_ref64(a, w, None, None, None, False, 1, 1).reshape(-1, c))
        b, p = _gn64(s, gamma, beta, groups, eps, True, pad=True)
        bad.append(route_util.conv_ref64(b, w, None, None, None, False, 1, 0).reshape(-1, c))
    good, bad = torch.cat(good), torch.cat(bad)
    assert good.shape == bad.shape == y_one.shape
    # the GroupNorm statistics and the normalised operand are fp32: their round-off (2^-23 per operation, a handful of
    # operations, on operands of magnitude |xn|max) passes through a K = 9 c sum of products like the accumulation error
    # does, which the suite's 2e-5 rule already budgets for K up to 4608 -- no extra slack
    e_one, e_two = route_util.excess(y_one, good, y_one.dtype), route_util.excess(y_two, good, y_two.dtype)
    e_bad = route_util.excess(y_one, bad, y_one.dtype)
    print(f'prologue: largest error minus bound: fused {e_one:.3e}, two launches {e_two:.3e}, against the padded-norm reference {e_bad:.3e}')
    assert e_one <= 0 and e_two <= 0
    assert e_bad > 0


@pytest.fixture(scope='module')
def models():
    cfg = Config.fromfile(CFG)
    plain = build_detector(cfg.model)
    plain.load_state_dict(util.seeded_state_dict(plain, seed=10))
    frozen = build_detector(cfg.model)
    frozen.load_state_dict(util.seeded_state_dict(frozen, seed=10))
    return plain.to(DEV).eval(), frozen.to(DEV).eval().freeze_for_inference()


@pytest.fixture()
def winograd_on():
    L = lib.load()
    before = L.brcnn_conv_set_tile(-11, 2)
    assert L.brcnn_conv_set_tile(-11, 1) == 0
    yield
    assert L.brcnn_conv_set_tile(-11, before) == 0


def test_frozen_model_matches_the_plain_one(models, winograd_on):
    L = lib.load()
    plain, frozen = models
    img, metas, _, _ = util.demo_inputs(2, 128, 192, seed=10)
    with torch.no_grad():
        feats = plain.extract_feat_nhwc(img.to(DEV))
        route_util.clear(L)
        fp = plain.rpn_head.forward_fused(list(feats))
        assert _wino_launches() == 0
        ff = frozen.rpn_head.forward_fused(list(feats))
        assert _wino_launches() == 4
        for lvl in range(5):
            assert _close(ff[lvl], fp[lvl]), lvl
        rp = plain(return_loss=False, rescale=True, img=[img.to(DEV)], img_metas=[metas])
        assert _wino_launches() == 0
        rf = frozen(return_loss=False, rescale=True, img=[img.to(DEV)], img_metas=[metas])
        assert _wino_launches() == 4
    assert sum(len(d) for im in rp for d in im) > 20
    for b in range(2):
        for c in range(4):
            assert _match_dets(rf[b][c], rp[b][c]) >= 0.99 and _match_dets(rp[b][c], rf[b][c]) >= 0.99, (b, c)
    # the switch off: the frozen model runs the plain launches
    assert L.brcnn_conv_set_tile(-11, 0) == 0
    with torch.no_grad():
        f0 = frozen.rpn_head.forward_fused(list(feats))
    assert _wino_launches() == 0
    for lvl in range(5):
        assert torch.equal(f0[lvl], fp[lvl])


def test_filter_cache_follows_load_state_dict(models, winograd_on):
    L = lib.load()
    plain, frozen = models
    img, _, _, _ = util.demo_inputs(2, 128, 192, seed=10)
    old = {k: v.clone() for k, v in frozen.state_dict().items()}
    try:
        with torch.no_grad():
            feats = plain.extract_feat_nhwc(img.to(DEV))
            before = frozen.rpn_head.forward_fused(list(feats))
            other = util.seeded_state_dict(frozen, seed=11)
            frozen.load_state_dict(other)
            plain.load_state_dict(other)
            route_util.clear(L)
            ff = frozen.rpn_head.forward_fused(list(feats))
            assert _wino_launches() == 4
            fp = plain.rpn_head.forward_fused(list(feats))
        for lvl in range(5):
            assert _close(ff[lvl], fp[lvl]), lvl
        assert not _close(ff[0], before[0])
    finally:
        frozen.load_state_dict(old)
        plain.load_state_dict(old)


def test_entry_points_refuse_other_layers():
    L = lib.load()
    batch, sizes = 1, [(6, 8)]
    x, w = _inputs(batch, sizes, 32, 64, seed=3)
    u = ops.winograd_filter(w)
    ws = ops.winograd_workspace(batch, sizes, 32, DEV)
    y = torch.full((48, 64), 7.0, device=DEV)
    hs, wd = (ctypes.c_int * 1)(6), (ctypes.c_int * 1)(8)

    def call(xp=x, up=u, wsp=ws.data_ptr(), cin=32, k=3, stride=1, pad=1, dt=ops.DT_F32):
        return L.brcnn_conv3x3_winograd_f32_multi(xp.data_ptr(), up.data_ptr(), None, None, None, 0, 0, None, None, 0, y.data_ptr(),
                                                  wsp, ws.numel(), batch, 1, hs, wd, cin, 64, k, k, stride, pad, dt,
                                                  lib.raw_stream_handle())
    route_util.clear(L)
    x24 = torch.randn(48, 24, device=DEV)
    assert call(stride=2) == -22 and call(k=1, pad=0) == -22 and call(xp=x24, cin=24) == -22
    assert call(dt=ops.DT_BF16) == -22 and call(dt=ops.DT_F16) == -22 and call(wsp=None) == -22
    assert L.brcnn_winograd_filter_f32(w.data_ptr(), u.data_ptr(), 64, 24, 3, 3, ops.DT_F32, lib.raw_stream_handle()) == -22
    assert L.brcnn_winograd_filter_f32(w.data_ptr(), u.data_ptr(), 64, 32, 1, 1, ops.DT_F32, lib.raw_stream_handle()) == -22
    assert L.brcnn_winograd_filter_f32(w.data_ptr(), u.data_ptr(), 64, 32, 3, 3, ops.DT_BF16, lib.raw_stream_handle()) == -22
    torch.cuda.synchronize()
    assert _wino_launches() == 0 and bool((y == 7.0).all())
    with pytest.raises(lib.BrcnnHipError):
        ops.conv3x3_winograd_multi(x, u, batch, sizes, stride=2)
    assert call() == 0 and _wino_launches() == 1
