"""-m gpu: the Winograd single-layer route of the frozen fp32 3x3 stride-1 conv + folded-BN / bias layers
(brcnn_conv3x3_winograd_f32_layer, csrc/conv_winograd_f32.hip; blocks.conv_bn_act_nhwc's no-grad tail).

* every GEMM tile (64 x 128, 32 x 128, 64 x 64), forced, against float64 at the suite's fp32 bound (route_util), on maps
  with odd edges, one-pixel rows, fewer tiles than one workgroup and tile counts that are no multiple of 32 or 64; each
  case proven by the route's own counters (launches AND the tile of the launch); all tiles give the bits of the tower's
  entry on the same inputs;
* the result lands in the caller's slice under ops.output_into and nowhere else;
* a frozen Bottleneck and a frozen neck ConvModule against the same modules not frozen, and after load_state_dict;
* what must not take the route: stride 2, a residual, 16-bit compute, grad mode;
* the default rule on the small demo image (nothing wired below its thresholds; the tower keeps its four launches) and the
  whole detector with the route forced.
"""

import pytest
import torch
import torch.nn as nn

import brcnn  # noqa: F401
from brcnn import Config, blocks, build_detector, lib, ops
from brcnn.backbones import Bottleneck
from brcnn.blocks import ConvModule
from tests import route_util, util
from tests.test_host_cpu import CFG
from tests.test_winograd_f32_gpu import _close, _match_dets

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
VARIANTS = (1, 2, 3)        # 64 x 128, 32 x 128, 64 x 64


def _layer_launches(L):
    return L.brcnn_conv_set_tile(-14, 10)


def _last_variant(L):
    return L.brcnn_conv_set_tile(-14, 11)


@pytest.fixture()
def hooks():
    """the Winograd switch on, the route and the GEMM tile at their defaults; every hook put back afterwards"""
    L = lib.load()
    before = (L.brcnn_conv_set_tile(-11, 2), L.brcnn_conv_set_tile(-14, 3), L.brcnn_conv_set_tile(-14, 24))
    assert L.brcnn_conv_set_tile(-11, 1) == 0 and L.brcnn_conv_set_tile(-14, 1) == 0 and L.brcnn_conv_set_tile(-14, 20) == 0
    route_util.clear(L)
    yield L
    assert L.brcnn_conv_set_tile(-11, before[0]) == 0 and L.brcnn_conv_set_tile(-14, before[1]) == 0
    assert L.brcnn_conv_set_tile(-14, 20 + before[2]) == 0


def _inputs(batch, h, w, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, h, w, cin, generator=g).to(DEV)
    wt = (torch.randn(cout, 3, 3, cin, generator=g) * (1.0 / (3.0 * cin ** 0.5))).to(DEV)
    scale = (torch.rand(cout, generator=g) + 0.5).to(DEV)
    shift = torch.randn(cout, generator=g).to(DEV)
    return x, wt, scale, shift


MAPS = [(2, 7, 11), (1, 13, 21), (2, 1, 5), (1, 2, 2), (2, 8, 12)]
CHANNELS = [(32, 64), (128, 128), (256, 256), (512, 512)]


@pytest.mark.parametrize('cin,cout', CHANNELS)
@pytest.mark.parametrize('batch,h,w', MAPS)
def test_every_gemm_tile_against_float64(hooks, batch, h, w, cin, cout):
    L = hooks
    x, wt, scale, shift = _inputs(batch, h, w, cin, cout, seed=500 + cin + 31 * h + w)
    u = ops.winograd_filter(wt)
    tiles = batch * ((h + 1) // 2) * ((w + 1) // 2)
    for readout in (False, True):
        sc, sh = (scale, shift) if readout else (None, None)
        ref = route_util.conv_ref64(x, wt, sc, sh, None, readout, 1, 1)
        tower = ops.conv3x3_winograd_multi(x.view(-1, cin), u, batch, [(h, w)], scale=sc, shift=sh, relu=readout)
        assert L.brcnn_conv_set_tile(-12, 0) == 1 and _layer_launches(L) == 0
        for v in VARIANTS:
            assert L.brcnn_conv_set_tile(-14, 20 + v) == 0
            y = ops.conv3x3_winograd_layer(x, u, sc, sh, readout)
            assert _layer_launches(L) == 1 and _last_variant(L) == v
            assert y.shape == ref.shape and torch.isfinite(y).all()
            e = route_util.excess(y, ref, y.dtype)
            print(f'layer {batch}x{h}x{w} {cin}->{cout} tile {v} readout {readout}: largest error minus bound {e:.3e}')
            assert e <= 0, (v, readout, e)
            # every tile sums an output's K loop in one order: the bits of the tower's entry (64 x 128)
            assert torch.equal(y.view(-1, cout), tower), (v, readout)
        assert L.brcnn_conv_set_tile(-14, 20) == 0
        # the layer entry leaves the tower's counters alone
        assert L.brcnn_conv_set_tile(-12, 0) == 0 and L.brcnn_conv_set_tile(-12, 1) == tiles


@pytest.mark.parametrize('variant', VARIANTS)
def test_output_lands_in_the_callers_slice_only(hooks, variant):
    L = hooks
    batch, h, w, c = 2, 7, 11, 256
    x, wt, scale, shift = _inputs(batch, h, w, c, c, seed=41)
    u = ops.winograd_filter(wt)
    rows = batch * h * w
    buf = torch.full((rows + 2 * 37, c), float('nan'), device=DEV)
    view = buf[37:37 + rows]
    assert L.brcnn_conv_set_tile(-14, 20 + variant) == 0
    with ops.output_into(view):
        y = ops.conv3x3_winograd_layer(x, u, scale, shift, True)
    assert _layer_launches(L) == 1 and _last_variant(L) == variant
    assert y.data_ptr() == view.data_ptr() and tuple(y.shape) == (batch, h, w, c)
    ref = route_util.conv_ref64(x, wt, scale, shift, None, True, 1, 1)
    assert torch.isfinite(view).all() and route_util.excess(view.view(batch, h, w, c), ref, view.dtype) <= 0
    assert torch.isnan(buf[:37]).all() and torch.isnan(buf[37 + rows:]).all()


def _randomise_bn(m, g):
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            mod.weight.data = torch.rand(mod.num_features, generator=g) + 0.5
            mod.bias.data = torch.randn(mod.num_features, generator=g) * 0.1
            mod.running_mean = torch.randn(mod.num_features, generator=g) * 0.1
            mod.running_var = torch.rand(mod.num_features, generator=g) + 0.5
    return m


def _bottleneck(seed, stride=1):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    down = None
    if stride != 1:
        down = nn.Sequential(nn.Conv2d(512, 512, 1, stride=stride, bias=False), nn.BatchNorm2d(512))
    return _randomise_bn(Bottleneck(512, 128, stride=stride, downsample=down), g).to(DEV).eval()


def _neck_conv(seed):
    torch.manual_seed(seed)
    m = ConvModule(256, 256, 3, padding=1, act_cfg=None)
    assert m.conv.bias is not None and m.norm is None
    m.conv.bias.data = torch.randn(256, generator=torch.Generator().manual_seed(seed)) * 0.1
    return m.to(DEV).eval()


def _prepare(m):
    """what TwoStageDetector.prepare_winograd_layers does to a block of the model"""
    if isinstance(m, Bottleneck):
        return blocks.prepare_winograd_layer(m.conv2, m._c[1])
    return blocks.prepare_winograd_layer(m.conv, m._cache)


@pytest.mark.parametrize('kind', ['bottleneck', 'neck'])
def test_frozen_block_matches_the_plain_one_and_follows_load_state_dict(hooks, kind):
    L = hooks
    make, shape = (_bottleneck, (2, 6, 10, 512)) if kind == 'bottleneck' else (_neck_conv, (2, 5, 7, 256))
    plain, frozen, other = make(3), make(3), make(4)
    assert _prepare(frozen)
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    assert L.brcnn_conv_set_tile(-14, 2) == 0                   # route forced: these maps are below the rule's thresholds
    with torch.no_grad():
        yp = plain.forward_nhwc(x)
        assert _layer_launches(L) == 0                          # not frozen: never the Winograd entry
        yf = frozen.forward_nhwc(x)
        assert _layer_launches(L) == 1
        assert _close(yf, yp)
        frozen.load_state_dict(other.state_dict())
        plain.load_state_dict(other.state_dict())
        yf2 = frozen.forward_nhwc(x)
        assert _layer_launches(L) == 1
        yp2 = plain.forward_nhwc(x)
        assert _layer_launches(L) == 0
    assert _close(yf2, yp2) and not _close(yf2, yf)
    # the default rule leaves a map this small on the direct kernels, with today's bits
    assert L.brcnn_conv_set_tile(-14, 1) == 0
    with torch.no_grad():
        yd = frozen.forward_nhwc(x)
    assert _layer_launches(L) == 0 and torch.equal(yd, yp2)


def test_refusals_launch_nothing_and_keep_the_direct_bits(hooks):
    L = hooks
    assert L.brcnn_conv_set_tile(-14, 2) == 0
    g = torch.Generator().manual_seed(21)
    # a stride-2 block: its conv2 has not the form, nothing is prepared
    plain, frozen = _bottleneck(5, stride=2), _bottleneck(5, stride=2)
    assert not _prepare(frozen) and frozen._c[1].wino is None
    x = torch.randn(2, 6, 10, 512, generator=g).to(DEV)
    with torch.no_grad():
        assert torch.equal(frozen.forward_nhwc(x), plain.forward_nhwc(x))
    assert _layer_launches(L) == 0
    # a call with a residual operand
    plain, frozen = _neck_conv(6), _neck_conv(6)
    assert _prepare(frozen)
    x = torch.randn(2, 5, 7, 256, generator=g).to(DEV)
    res = torch.randn(2, 5, 7, 256, generator=g).to(DEV)
    with torch.no_grad():
        assert torch.equal(frozen.forward_nhwc(x, residual=res), plain.forward_nhwc(x, residual=res))
        assert _layer_launches(L) == 0
        frozen.forward_nhwc(x)
        assert _layer_launches(L) == 1                          # (the same module without the residual does take it)
    # grad mode with a trainable weight
    assert frozen.conv.weight.requires_grad
    with torch.enable_grad():
        yf, yp = frozen.forward_nhwc(x), plain.forward_nhwc(x)
    assert yf.requires_grad and torch.equal(yf, yp) and _layer_launches(L) == 0
    # a bf16 model
    plain, frozen = _bottleneck(7), _bottleneck(7)
    before = blocks.compute_dtype()
    try:
        blocks.set_compute_dtype('bf16')
        assert _prepare(frozen)
        xb = torch.randn(2, 6, 10, 512, generator=g).to(DEV).bfloat16()
        with torch.no_grad():
            yf, yp = frozen.forward_nhwc(xb), plain.forward_nhwc(xb)
        assert yf.dtype == torch.bfloat16 and torch.equal(yf, yp) and _layer_launches(L) == 0
    finally:
        blocks.set_compute_dtype(before)
    # the library's switch off: "no Winograd anywhere"
    plain, frozen = _bottleneck(8), _bottleneck(8)
    assert _prepare(frozen)
    x = torch.randn(2, 6, 10, 512, generator=g).to(DEV)
    assert L.brcnn_conv_set_tile(-11, 0) == 0
    with torch.no_grad():
        assert torch.equal(frozen.forward_nhwc(x), plain.forward_nhwc(x))
    assert _layer_launches(L) == 0


@pytest.fixture(scope='module')
def frozen_model():
    cfg = Config.fromfile(CFG)
    m = build_detector(cfg.model)
    m.load_state_dict(util.seeded_state_dict(m, seed=10))
    return m.to(DEV).eval().freeze_for_inference()


def test_default_rule_on_the_demo_image_and_the_forced_detector(hooks, frozen_model):
    L = hooks
    img, metas, _, _ = util.demo_inputs(2, 128, 192, seed=10)
    with torch.no_grad():
        r0 = frozen_model(return_loss=False, rescale=True, img=[img.to(DEV)], img_metas=[metas])
        # at most 192 tiles per map: below every threshold of the measured rule; the tower keeps its four launches
        assert _layer_launches(L) == 0 and L.brcnn_conv_set_tile(-12, 0) == 4
        assert L.brcnn_conv_set_tile(-14, 2) == 0
        r1 = frozen_model(return_loss=False, rescale=True, img=[img.to(DEV)], img_metas=[metas])
        n = _layer_launches(L)
        assert n > 0 and L.brcnn_conv_set_tile(-12, 0) == 4
    print(f'forced detector pass: {n} layer-route launches')
    assert sum(len(d) for im in r0 for d in im) > 20
    for b in range(2):
        for c in range(4):
            assert _match_dets(r1[b][c], r0[b][c]) >= 0.99 and _match_dets(r0[b][c], r1[b][c]) >= 0.99, (b, c)
