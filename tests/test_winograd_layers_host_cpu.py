"""The host side of the Winograd single-layer route that needs no device: the route function (brcnn_winograd_layer_route,
csrc/policy.hip) at both sides of the measured thresholds and on every refusing argument, the GEMM tile rule, and the hook
codes (-14, n) with their counters (csrc/policy.h)."""
import pytest

import brcnn  # noqa: F401
from brcnn import lib, ops

F32, BF16, F16 = ops.DT_F32, ops.DT_BF16, ops.DT_F16


def _route(tiles, cin, cout, k=3, stride=1, pad=1, dil=1, groups=1, dt=F32):
    return lib.load().brcnn_winograd_layer_route(tiles, cin, cout, k, k, stride, pad, dil, groups, dt)


@pytest.fixture()
def defaults():
    """every switch the route reads at its default, whatever ran before; put back afterwards"""
    L = lib.load()
    before = (L.brcnn_conv_set_tile(-11, 2), L.brcnn_conv_set_tile(-14, 3), L.brcnn_conv_set_tile(-14, 24))
    assert L.brcnn_conv_set_tile(-11, 1) == 0 and L.brcnn_conv_set_tile(-14, 1) == 0 and L.brcnn_conv_set_tile(-14, 20) == 0
    yield L
    assert L.brcnn_conv_set_tile(-11, before[0]) == 0 and L.brcnn_conv_set_tile(-14, before[1]) == 0
    assert L.brcnn_conv_set_tile(-14, 20 + before[2]) == 0


# The measured table (profiles/f32_winograd_layers.txt): per channel class the nearest measured losing (or not proven) and
# winning tile counts; the threshold lies midway between them.  (cin, cout, losing tiles, winning tiles, threshold)
THRESHOLDS = [(256, 256, 4200, 6300, 5250), (512, 512, 273, 616, 444)]


@pytest.mark.parametrize('cin,cout,lose,win,at', THRESHOLDS)
def test_measured_rule_at_both_sides_of_its_thresholds(defaults, cin, cout, lose, win, at):
    assert _route(win, cin, cout) == 1 and _route(lose, cin, cout) == 0
    assert _route(at, cin, cout) == 1 and _route(at - 1, cin, cout) == 0
    assert _route(win * 4, cin, cout) == 1 and _route(1, cin, cout) == 0
    # the maps of a 128x192 image (at most 192 tiles) stay on the direct kernels in every class
    for c in (64, 128, 256, 512):
        assert _route(192, c, c) == 0


def test_classes_the_table_leaves_on_the_direct_kernels(defaults):
    # the neck's 25x42 level (256 -> 256, 2 184 tiles) lost; channel pairs that were not measured are not wired
    assert _route(2184, 256, 256) == 0
    assert _route(33600, 64, 64) == 0 and _route(33600, 32, 64) == 0 and _route(33600, 256, 512) == 0 and _route(33600, 1024, 1024) == 0
    # the flagship pass at batch 8: what the table wired
    assert _route(33600, 256, 256) == 1 and _route(8400, 256, 256) == 1 and _route(2184, 512, 512) == 1
    # stage 2 (128 -> 128) won in the table and is left out all the same: with it two detections of the flagship pass whose
    # scores are 4e-7 apart change places (csrc/policy.hip: wino_layer_rule)
    assert _route(33600, 128, 128) == 0 and _route(4200, 128, 128) == 0 and _route(1 << 24, 128, 128) == 0
    # ... and at batch 1 (latency) nothing is wired
    assert _route(4200, 256, 256) == 0 and _route(1050, 256, 256) == 0 and _route(273, 512, 512) == 0


def test_refusing_arguments(defaults):
    L = defaults
    assert L.brcnn_conv_set_tile(-14, 2) == 0                   # "wherever the entry accepts the shape": only the form decides
    assert _route(1, 32, 64) == 1 and _route(192, 512, 512) == 1
    assert _route(100, 256, 256, stride=2) == 0
    assert _route(100, 256, 256, k=1, pad=0) == 0 and _route(100, 256, 256, k=1) == 0
    assert _route(100, 256, 256, pad=0) == 0 and _route(100, 256, 256, dil=2) == 0 and _route(100, 256, 256, groups=32) == 0
    assert _route(100, 24, 64) == 0                             # Cin % 32
    assert _route(100, 32, 32) == 0 and _route(100, 32, 96) == 0      # Cout % 64
    assert _route(100, 256, 256, dt=BF16) == 0 and _route(100, 256, 256, dt=F16) == 0
    assert _route(0, 256, 256) == 0 and _route(-5, 256, 256) == 0 and _route(100, 0, 64) == 0
    assert L.brcnn_conv_set_tile(-14, 0) == 0                   # mode "never"
    assert _route(33600, 256, 256) == 0 and _route(1, 32, 64) == 0
    assert L.brcnn_conv_set_tile(-14, 2) == 0 and L.brcnn_conv_set_tile(-11, 0) == 0       # the library's switch: no Winograd anywhere
    assert _route(33600, 256, 256) == 0
    assert L.brcnn_conv_set_tile(-14, 1) == 0
    assert _route(33600, 256, 256) == 0
    assert L.brcnn_conv_set_tile(-11, 1) == 0
    assert _route(33600, 256, 256) == 1


def test_gemm_tile_rule_and_forcing_hook(defaults):
    L = defaults
    v = L.brcnn_winograd_layer_gemm_variant
    for tiles in (1, 192, 2184, 8400, 33600, 134400):
        for cout in (64, 128, 256, 512):
            assert v(tiles, cout) in (1, 2, 3)
    assert v(33600, 256) == 3 and v(2184, 512) == 3             # 64 x 64 won every row of the table
    for k in (1, 2, 3):
        assert L.brcnn_conv_set_tile(-14, 20 + k) == 0 and L.brcnn_conv_set_tile(-14, 24) == k
        assert v(8400, 256) == k and v(1, 64) == k
    assert L.brcnn_conv_set_tile(-14, 20) == 0 and L.brcnn_conv_set_tile(-14, 24) == 0


def test_hook_codes_get_set_restore(defaults):
    L = defaults
    assert L.brcnn_conv_set_tile(-14, 3) == 1                   # the default: the measured rule
    for mode in (0, 2, 1):
        assert L.brcnn_conv_set_tile(-14, mode) == 0 and L.brcnn_conv_set_tile(-14, 3) == mode
    accepted = {0, 1, 2, 20, 21, 22, 23}
    for nt in list(range(-3, 40)) + [128, 256]:
        if nt in (3, 10, 11, 24):
            continue
        assert L.brcnn_conv_set_tile(-14, nt) == (0 if nt in accepted else -22), nt
        L.brcnn_conv_set_tile(-14, 1), L.brcnn_conv_set_tile(-14, 20)
    assert L.brcnn_conv_set_tile(-14, 3) == 1 and L.brcnn_conv_set_tile(-14, 24) == 0
    # nothing launches without a device: both counters read 0, and (-9, -1) clears them with the others
    assert L.brcnn_conv_set_tile(-14, 10) == 0 and L.brcnn_conv_set_tile(-14, 11) == 0
    assert L.brcnn_conv_set_tile(-9, -1) == 0
    # the route's hook leaves the tower's switch and counters alone
    assert L.brcnn_conv_set_tile(-11, 2) == 1 and L.brcnn_conv_set_tile(-12, 0) == 0
    assert L.brcnn_conv_set_tile(-15, 0) == -22


def test_layer_entry_refuses_without_launching():
    """the entry's argument checks come before any device call"""
    L = lib.load()
    e = L.brcnn_conv3x3_winograd_f32_layer
    assert e(None, None, None, None, 0, None, None, 0, 1, 4, 4, 32, 64, 3, 3, 1, 1, F32, None) == -22
    assert e(8, 8, None, None, 0, 8, 8, 1 << 30, 1, 4, 4, 32, 64, 3, 3, 2, 1, F32, None) == -22         # stride 2
    assert e(8, 8, None, None, 0, 8, 8, 1 << 30, 1, 4, 4, 32, 64, 1, 1, 1, 0, F32, None) == -22         # 1x1
    assert e(8, 8, None, None, 0, 8, 8, 1 << 30, 1, 4, 4, 24, 64, 3, 3, 1, 1, F32, None) == -22         # Cin % 32
    assert e(8, 8, None, None, 0, 8, 8, 1 << 30, 1, 4, 4, 32, 32, 3, 3, 1, 1, F32, None) == -22         # Cout % 64
    assert e(8, 8, None, None, 0, 8, 8, 1 << 30, 1, 4, 4, 32, 64, 3, 3, 1, 1, BF16, None) == -22
    assert e(8, 8, None, None, 0, 8, 8, 1 << 30, 0, 4, 4, 32, 64, 3, 3, 1, 1, F32, None) == -22         # no image
    assert e(8, 8, None, None, 0, 8, 8, 16, 1, 4, 4, 32, 64, 3, 3, 1, 1, F32, None) == -22              # workspace too small
    assert L.brcnn_conv_set_tile(-14, 10) == 0
