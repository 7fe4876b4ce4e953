"""-m gpu: the persistent, balanced launch of the fp32 Winograd GEMM (wino_gemm_kernel<.., true>, csrc/conv_winograd_f32.hip)
against the plain launch of one workgroup per GEMM tile.

Every comparison is torch.equal between the same call under "never" ((-16, 0)) and under "forced" ((-16, 2)); every call
proves through the counters ((-16, 10) launches, (-16, 11) workgroups) which form ran, and "never" must add no persistent
launch.  The workgroup cap hook ((-16, 1000 + n)) makes small maps straddle tiles: the ranges of the launch are those of
sk_table_ranges (csrc/conv_igemm_bf16.hip), `_ranges` below repeats its arithmetic so that each set of caps can state
which kinds of work item it exercises.

A range holds at least one tile's worth of xi planes (the planner refuses anything finer), so a workgroup that holds a
tail and nothing else cannot occur: a tail is shorter than a tile.  The nearest kinds are covered instead: head + tail
with no whole tile between them, and whole tiles + tail with no head (the top range).

The three-stage LDS ring ((-16, 43)) runs the same cases, plain and persistent, against the two-stage plain launch:
torch.equal throughout, the ring of each launch read back from its counter ((-16, 13)).

After every case brcnn_conv_handover_status() is 0.
"""

import pytest
import torch

import brcnn  # noqa: F401
from brcnn import lib, ops
from tests import route_util

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
UNITS = 16
TILE = {1: (64, 128), 2: (32, 128), 3: (64, 64)}        # GEMM tile of a variant: 2x2 output tiles x channels


def _ranges(wg_tiles, slots):
    """per workgroup (first xi of its tail or 0, end xi of its head or 0, whole tiles): sk_table_ranges' cut"""
    q, r = divmod(wg_tiles * UNITS, slots)
    assert q >= UNITS
    out = []
    for w in range(slots):
        sw = q * w + min(w, r)
        ew = sw + q + (1 if w < r else 0)
        tf, te = sw // UNITS, ew // UNITS
        kb, ke = sw - tf * UNITS, ew - te * UNITS
        out.append((kb, ke, te - tf - (1 if kb else 0)))
    return out


def _kinds(wg_tiles, slots):
    return {('H' if ke else '') + ('W' if wh else '') + ('T' if kb else '') for kb, ke, wh in _ranges(wg_tiles, slots)}


def _ends(wg_tiles, slots):
    return {ke for _, ke, _ in _ranges(wg_tiles, slots) if ke}


def _wg_tiles(tiles, cout, variant):
    bm, bn = TILE[variant]
    return ((tiles + bm - 1) // bm) * ((cout + bn - 1) // bn)


@pytest.fixture()
def hooks():
    """the Winograd switches at their defaults, the counters clear; every hook put back, no hand-over lost"""
    L = lib.load()
    before = (L.brcnn_conv_set_tile(-11, 2), L.brcnn_conv_set_tile(-14, 24), L.brcnn_conv_set_tile(-16, 3),
              L.brcnn_conv_set_tile(-16, 24), L.brcnn_conv_set_tile(-16, 39), L.brcnn_conv_set_tile(-16, 999),
              L.brcnn_conv_set_tile(-16, 49))
    assert L.brcnn_conv_set_tile(-11, 1) == 0 and L.brcnn_conv_set_tile(-14, 20) == 0 and L.brcnn_conv_set_tile(-16, 1) == 0
    assert L.brcnn_conv_set_tile(-16, 20) == 0 and L.brcnn_conv_set_tile(-16, 30) == 0 and L.brcnn_conv_set_tile(-16, 1000) == 0
    assert L.brcnn_conv_set_tile(-16, 42) == 0
    assert L.brcnn_conv_handover_status() == 0
    route_util.clear(L)
    yield L
    torch.cuda.synchronize()
    status = L.brcnn_conv_handover_status()
    assert L.brcnn_conv_set_tile(-11, 11) == 0 and L.brcnn_conv_set_tile(-11, before[0]) == 0
    assert L.brcnn_conv_set_tile(-14, 20 + before[1]) == 0 and L.brcnn_conv_set_tile(-16, before[2]) == 0
    assert L.brcnn_conv_set_tile(-16, 20 + before[3]) == 0 and L.brcnn_conv_set_tile(-16, 30 + before[4]) == 0
    assert L.brcnn_conv_set_tile(-16, 1000 + before[5]) == 0 and L.brcnn_conv_set_tile(-16, 40 + before[6]) == 0
    assert status == 0


def _took(L):
    """(persistent launches, workgroups of the last one) since the last look"""
    return L.brcnn_conv_set_tile(-16, 10), L.brcnn_conv_set_tile(-16, 11)


def _plain(L, fn, ring=2):
    assert L.brcnn_conv_set_tile(-16, 0) == 0 and L.brcnn_conv_set_tile(-16, 40 + ring) == 0
    y = fn()
    assert _took(L) == (0, 0) and L.brcnn_conv_set_tile(-16, 13) == ring
    return y


def _forced(L, fn, cap, launches=1, ring=2):
    """`fn` under the forced persistent form with at most `cap` workgroups (0: the hardware's own count)"""
    assert L.brcnn_conv_set_tile(-16, 2) == 0 and L.brcnn_conv_set_tile(-16, 1000 + cap) == 0
    assert L.brcnn_conv_set_tile(-16, 40 + ring) == 0
    y = fn()
    n, wgs = _took(L)
    assert n == launches and (wgs == cap if cap else wgs > 0), (n, wgs, cap)
    assert L.brcnn_conv_set_tile(-16, 13) == ring
    torch.cuda.synchronize()
    assert L.brcnn_conv_handover_status() == 0
    return y


def _layer_inputs(batch, h, w, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, h, w, cin, generator=g).to(DEV)
    wt = (torch.randn(cout, 3, 3, cin, generator=g) * (1.0 / (3.0 * cin ** 0.5))).to(DEV)
    scale = (torch.rand(cout, generator=g) + 0.5).to(DEV)
    shift = torch.randn(cout, generator=g).to(DEV)
    return x, wt, scale, shift


# 2 x 25 x 53: 702 output tiles = 11 row blocks of 64 (the last one ragged: 62), odd width and height.
MAP = (2, 25, 53)
TILES = 2 * 13 * 27
# (variant, cout, caps): per GEMM tile and channel count the workgroup caps, and what their ranges must exercise between
# them -- range ends at xi = 1, 8 and 15; a workgroup holding head + whole tiles + tail; one holding a single whole tile
# (where the tile count allows: 11 tiles on fewer workgroups never leave one alone); head + tail; whole tiles + tail
LAYER_CASES = [
    (3, 64, (8, 10), {8, 15}, {'HWT', 'HT', 'WT', 'HW'}),
    (3, 192, (14, 32), {1, 8, 15}, {'HWT', 'HT', 'WT', 'HW', 'W'}),
    (1, 192, (10, 21), {1, 8, 15}, {'HWT', 'HT', 'WT', 'HW', 'W'}),
    (2, 192, (18, 42), {1, 8, 15}, {'HWT', 'HT', 'WT', 'HW', 'W'}),
]


@pytest.mark.parametrize('variant,cout,caps,ends,kinds', LAYER_CASES)
def test_the_caps_exercise_every_item_kind(variant, cout, caps, ends, kinds):
    """host arithmetic: what the cases below rely on"""
    t = _wg_tiles(TILES, cout, variant)
    got_ends, got_kinds = set(), set()
    for cap in caps:
        got_ends |= _ends(t, cap)
        got_kinds |= _kinds(t, cap)
    assert ends <= got_ends and kinds <= got_kinds, (got_ends, got_kinds)
    if 'W' in kinds:
        assert any((0, 0, 1) in _ranges(t, cap) for cap in caps)       # a workgroup with ONE whole tile and nothing else


# Cin in {32, 96} x Cout in {64, 192} on the 64 x 64 tile, one case each on 64 x 128 and 32 x 128
LAYER_RUNS = [(v, cout, caps, cin) for v, cout, caps, _, _ in LAYER_CASES for cin in ((32, 96) if v == 3 else (96,))]


@pytest.mark.parametrize('variant,cout,caps,cin', LAYER_RUNS)
def test_layer_entry_persistent_equals_plain(hooks, variant, cout, caps, cin):
    L = hooks
    batch, h, w = MAP
    x, wt, scale, shift = _layer_inputs(batch, h, w, cin, cout, seed=900 + cin + cout + variant)
    u = ops.winograd_filter(wt)
    assert L.brcnn_conv_set_tile(-14, 20 + variant) == 0
    for readout in (False, True):
        sc, sh = (scale, shift) if readout else (None, None)
        fn = lambda: ops.conv3x3_winograd_layer(x, u, sc, sh, readout)
        ref = _plain(L, fn)
        assert L.brcnn_conv_set_tile(-14, 11) == variant
        assert torch.equal(_plain(L, fn, ring=3), ref), (variant, cout, cin, readout)
        for ring in (2, 3):
            for cap in caps:
                y = _forced(L, fn, cap, ring=ring)
                assert L.brcnn_conv_set_tile(-14, 11) == variant
                assert torch.equal(y, ref), (variant, cout, cin, cap, readout, ring)


def _tower_inputs(batch, sizes, cin, cout, seed):
    g = torch.Generator().manual_seed(seed)
    rows = sum(batch * h * w for h, w in sizes)
    x = torch.randn(rows, cin, generator=g).to(DEV)
    wt = (torch.randn(cout, 3, 3, cin, generator=g) * (1.0 / (3.0 * cin ** 0.5))).to(DEV)
    gamma = (torch.rand(cin, generator=g) + 0.5).to(DEV)
    beta = (torch.rand(cin, generator=g) * 0.5 + 0.25).to(DEV)
    return x, wt, gamma, beta


# two segments, batch 2: 154 + 48 = 202 output tiles = 4 row blocks of 64.  64 -> 64 is one column tile (4 GEMM tiles: caps
# 2 and 3 cut tiles 1 and 2 at xi 5 and 10 (cap 3) or run two whole tiles each (cap 2)); 64 -> 192 on the 64 x 128 tile has
# two column tiles, so that with two launch pairs ((-11, 12): 128 + 74 tiles, 4 and 4 GEMM tiles) each pair still straddles
@pytest.mark.parametrize('cout,caps', [(64, (2, 3)), (192, (3, 7))])
def test_tower_entry_persistent_equals_plain(hooks, cout, caps):
    L = hooks
    batch, sizes, cin, groups = 2, [(13, 21), (7, 11)], 64, 8
    x, wt, gamma, beta = _tower_inputs(batch, sizes, cin, cout, seed=33 + cout)
    u = ops.winograd_filter(wt)
    stats = ops.groupnorm_stats_multi(x, groups, batch, sizes, 1e-5)
    fn = lambda: ops.conv3x3_winograd_multi(x, u, batch, sizes, gn=(stats, gamma, beta, groups, True))
    ref = _plain(L, fn)
    assert L.brcnn_conv_set_tile(-16, 12) == 1              # the tower's default tile: 64 x 128
    assert torch.equal(_plain(L, fn, ring=3), ref)
    for ring in (2, 3):
        for cap in caps:
            assert torch.equal(_forced(L, fn, cap, ring=ring), ref), (cout, cap, ring)
    # the 64 x 64 tile on the tower entry: the same bits, plain and persistent, either ring
    assert L.brcnn_conv_set_tile(-16, 23) == 0
    assert torch.equal(_plain(L, fn), ref) and L.brcnn_conv_set_tile(-16, 12) == 3
    assert torch.equal(_forced(L, fn, 3), ref) and torch.equal(_forced(L, fn, 3, ring=3), ref)
    assert L.brcnn_conv_set_tile(-16, 20) == 0
    # two launch pairs: each pair plans for itself (its own table, its own epoch of the stream's flags)
    assert L.brcnn_conv_set_tile(-11, 12) == 0
    assert torch.equal(_plain(L, fn), ref)
    pair_cap = 2 if cout == 64 else 3                       # 2 or 4 GEMM tiles per pair
    assert torch.equal(_forced(L, fn, pair_cap, launches=2), ref), cout
    assert torch.equal(_forced(L, fn, pair_cap, launches=2, ring=3), ref) and torch.equal(_plain(L, fn, ring=3), ref), cout
    assert L.brcnn_conv_set_tile(-12, 0) > 0


def test_uncapped_launch_at_the_hardwares_own_count(hooks):
    """no workgroup cap: one workgroup per CU ((-16, 31)) on a launch of 11 x 32 = 352 GEMM tiles"""
    L = hooks
    batch, h, w = MAP
    x, wt, scale, shift = _layer_inputs(batch, h, w, 32, 2048, seed=5)
    u = ops.winograd_filter(wt)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert _wg_tiles(TILES, 2048, 3) >= cus, 'the case needs at least one GEMM tile per CU'
    fn = lambda: ops.conv3x3_winograd_layer(x, u, scale, shift, True)
    ref = _plain(L, fn)
    for ring in (2, 3):
        assert L.brcnn_conv_set_tile(-16, 31) == 0 and L.brcnn_conv_set_tile(-16, 2) == 0 and L.brcnn_conv_set_tile(-16, 40 + ring) == 0
        y = fn()
        assert _took(L) == (1, cus) and L.brcnn_conv_set_tile(-16, 13) == ring
        assert torch.equal(y, ref), ring


def test_fp64_leg_and_bits(hooks):
    L = hooks
    batch, h, w = MAP
    x, wt, scale, shift = _layer_inputs(batch, h, w, 96, 192, seed=17)
    u = ops.winograd_filter(wt)
    fn = lambda: ops.conv3x3_winograd_layer(x, u, scale, shift, True)
    ref64 = route_util.conv_ref64(x, wt, scale, shift, None, True, 1, 1)
    plain = _plain(L, fn)
    for ring in (2, 3):
        y = _forced(L, fn, 32, ring=ring)
        e = route_util.excess(y, ref64, y.dtype)
        print(f'persistent layer 2x25x53 96->192, 32 workgroups, ring {ring}: largest error minus bound {e:.3e}')
        assert e <= 0
        assert torch.equal(y, plain)


def test_fewer_tiles_than_workgroups_takes_the_plain_launch(hooks):
    L = hooks
    batch, h, w = MAP
    x, wt, scale, shift = _layer_inputs(batch, h, w, 32, 64, seed=3)       # 11 GEMM tiles, no cap: one workgroup per CU at least
    u = ops.winograd_filter(wt)
    fn = lambda: ops.conv3x3_winograd_layer(x, u, scale, shift, True)
    ref = _plain(L, fn)
    assert L.brcnn_conv_set_tile(-16, 2) == 0
    y = fn()
    assert _took(L) == (0, 0) and L.brcnn_conv_set_tile(-14, 10) == 2
    assert torch.equal(y, ref)
    # ... and so does a cap above the tile count
    assert L.brcnn_conv_set_tile(-16, 1000 + 12) == 0
    y = fn()
    assert _took(L) == (0, 0) and torch.equal(y, ref)
