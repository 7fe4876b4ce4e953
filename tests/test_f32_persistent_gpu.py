"""-m gpu: the persistent, balanced launch of the fp32 64 x 64 conv kernel (conv_igemm.hip, SK = true;
brcnn_conv_set_tile(-5, 2) forces it) against the plain one-tile-per-workgroup launch of the same call.  The schedule
only moves K tiles between workgroups -- every accumulator keeps its MFMA chain -- so every comparison is torch.equal.

Shapes: small maps with wide outputs (M ~ 2650 rows x 2048+ channels = 1344+ tiles of 64 x 64), so that the tile count
reaches the resident workgroups (at most 5 per CU x 256 CUs = 1280) and tiles x K-tiles is no multiple of them: ranges
straddle tiles, and most workgroups run a K head, a whole tile and a K tail."""
import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import lib as _lib
from brcnn import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _launches(L):
    n = L.brcnn_conv_set_tile(-6, 0)
    assert n >= 0
    return n


def _plain_and_persistent(L, fn):
    """fn() under the plain and under the forced persistent launch; asserts which form each call took"""
    try:
        assert L.brcnn_conv_set_tile(-5, 0) == 0
        n0 = _launches(L)
        ref = fn()
        assert _launches(L) == n0, 'hook 0 must take the plain launch'
        assert L.brcnn_conv_set_tile(-5, 2) == 0
        out = fn()
        assert _launches(L) == n0 + 1, 'the forced call did not take the persistent launch'
    finally:
        L.brcnn_conv_set_tile(-5, 1)
    return ref, out


def _operands(n, h, w, cin, cout, k, stride, pad, has_scale, has_shift, has_res, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, cin, generator=g)
    wt = torch.randn(cout, k, k, cin, generator=g) / np.sqrt(cin * k * k)
    sc = (torch.rand(cout, generator=g) + 0.5) if has_scale else None
    sh = torch.randn(cout, generator=g) if has_shift else None
    ho, wo = ops.conv_out_size(h, w, k, k, stride, pad)
    r = torch.randn(n, ho, wo, cout, generator=g) if has_res else None
    return x, wt, sc, sh, r


def _dev(t):
    return None if t is None else t.to(DEV)


CASES = [
    # N, H, W, Cin, Cout, k, stride, pad, scale, shift, residual, relu       M = 2650 (ragged: 41 row tiles + 26 rows)
    (2, 25, 53, 64, 2048, 1, 1, 0, True, True, True, True),          # nk = 2
    (2, 25, 53, 96, 2048, 1, 1, 0, False, False, False, False),      # nk = 3, bare conv
    (2, 25, 53, 224, 2048, 1, 1, 0, True, False, True, False),       # nk = 7
    (2, 25, 53, 32, 2048, 3, 1, 1, False, True, False, True),        # 3x3, pad 1: nk = 9, the taps inside one chunk
    (2, 50, 105, 32, 2048, 3, 2, 1, True, True, True, True),         # ... stride 2
    (2, 25, 53, 96, 2048, 3, 1, 1, True, True, True, True),          # 3x3 over three channel chunks: nk = 27, K tails start at any (chunk, tap)
    (2, 50, 105, 96, 2048, 3, 2, 1, False, True, False, True),       # ... stride 2
    (2, 25, 53, 96, 2048 + 54, 1, 1, 0, True, True, True, True),     # Cout % 4 != 0: scalar read-out
    (2, 25, 53, 224, 2048 + 52, 1, 1, 0, True, True, True, True),    # Cout % 64 != 0, % 4 == 0: general vector read-out
]


@pytest.mark.parametrize('cfg', CASES)
def test_persistent_launch_is_bit_identical(cfg):
    L = _lib.load()
    n, h, w, cin, cout, k, stride, pad, has_scale, has_shift, has_res, relu = cfg
    x, wt, sc, sh, r = (_dev(t) for t in _operands(n, h, w, cin, cout, k, stride, pad, has_scale, has_shift, has_res, 41))
    ref, out = _plain_and_persistent(L, lambda: ops.conv2d_nhwc(x, wt, sc, sh, r, relu, stride, pad))
    assert torch.equal(out, ref), (out - ref).abs().max().item()


def test_persistent_launch_vs_float64():
    """one case against an fp64 reference at the fp32 conv tolerance of the suite (test_conv2d_nhwc_vs_float64)"""
    import torch.nn.functional as F
    L = _lib.load()
    n, h, w, cin, cout, k, stride, pad = 2, 25, 53, 64, 2048, 1, 1, 0
    x, wt, sc, sh, r = _operands(n, h, w, cin, cout, k, stride, pad, True, True, True, 42)
    y = F.conv2d(x.permute(0, 3, 1, 2).double(), wt.permute(0, 3, 1, 2).double(), None, stride, pad)
    y = (y * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1) + r.permute(0, 3, 1, 2).double()).relu()
    xg, wg, scg, shg, rg = (_dev(t) for t in (x, wt, sc, sh, r))
    ref, out = _plain_and_persistent(L, lambda: ops.conv2d_nhwc(xg, wg, scg, shg, rg, True, stride, pad))
    assert torch.equal(out, ref)
    err = (out.permute(0, 3, 1, 2).cpu().double() - y).abs().max().item()
    assert err < 2e-5 * max(1.0, y.abs().max().item()), err


def test_persistent_launch_general_forms():
    """brcnn_conv_set_tile(-4, 1): the general set-up and read-out under both launches, same bits as the fast forms"""
    L = _lib.load()
    x, wt, sc, sh, r = (_dev(t) for t in _operands(2, 25, 53, 64, 2048, 1, 1, 0, True, True, True, 43))
    fn = lambda: ops.conv2d_nhwc(x, wt, sc, sh, r, True, 1, 0)
    fast = fn()
    try:
        assert L.brcnn_conv_set_tile(-4, 1) == 0
        ref, out = _plain_and_persistent(L, fn)
    finally:
        L.brcnn_conv_set_tile(-4, 0)
    assert torch.equal(ref, fast) and torch.equal(out, fast)


def test_persistent_launch_multi_level():
    """three pyramid levels in one launch; the level boundaries (rows 2460 and 3090) fall inside 64-row tiles"""
    L = _lib.load()
    sizes = [(30, 41), (15, 21), (8, 11)]
    B, cin, cout = 2, 32, 2048
    g = torch.Generator().manual_seed(44)
    xc = torch.cat([torch.randn(B, h, w, cin, generator=g).reshape(-1, cin) for h, w in sizes], 0).to(DEV)
    wt = (torch.randn(cout, 3, 3, cin, generator=g) / 17).to(DEV)
    sh = torch.randn(cout, generator=g).to(DEV)
    rows = sum(B * h * w for h, w in sizes)
    assert rows == 3266 and all(b % 64 for b in (2460, 3090))
    r = torch.randn(rows, cout, generator=g).to(DEV)
    ref, out = _plain_and_persistent(L, lambda: ops.conv2d_nhwc_multi(xc, wt, B, sizes, None, sh, r, True, 1, 1)[0])
    assert torch.equal(out, ref)


def test_excluded_launches_stay_plain():
    """fewer tiles than two workgroups per CU could take (no range of a whole tile's K tiles each: the chain would stay
    serial), a one-K-tile layer and a grouped conv keep the plain launch when forced"""
    L = _lib.load()
    g = torch.Generator().manual_seed(45)
    few = [_dev(t) for t in _operands(2, 16, 20, 64, 2048, 1, 1, 0, True, True, False, 45)]         # 10 x 32 = 320 tiles < 2 x 256
    one_k = [_dev(t) for t in _operands(2, 25, 53, 32, 2048, 1, 1, 0, True, True, False, 46)]       # nk = 1
    xg = torch.randn(2, 25, 53, 2048, generator=g).to(DEV)
    w_tiles, window = ops.pack_grouped_weight(torch.randn(2048, 64, 1, 1, generator=g).to(DEV) / 8, 32)
    calls = [lambda: ops.conv2d_nhwc(few[0], few[1], few[2], few[3], None, True, 1, 0),
             lambda: ops.conv2d_nhwc(one_k[0], one_k[1], one_k[2], one_k[3], None, True, 1, 0),
             lambda: ops.conv2d_nhwc_grouped(xg, w_tiles, window, None, None, None, True, 1, 0)]
    try:
        for i, fn in enumerate(calls):
            assert L.brcnn_conv_set_tile(-5, 0) == 0
            ref = fn()
            assert L.brcnn_conv_set_tile(-5, 2) == 0
            n0 = _launches(L)
            out = fn()
            assert _launches(L) == n0, i
            assert torch.equal(out, ref), i
    finally:
        L.brcnn_conv_set_tile(-5, 1)


def test_heuristic_takes_the_few_tile_class():
    """the default dispatch: launches with fewer tiles than resident workgroups, spread unevenly over the CUs (528 tiles
    on 256 CUs: three K chains on 16 CUs against two), with a long K loop go persistent -- the 2048 -> 256 lateral of the
    8 x 25 x 42 map (64 K tiles, plain 1x1 set-up) and the 3x3 256 -> 256 conv on it (72 K tiles: K tails that start in
    any of the eight channel chunks, at any tap); a short-K layer with many tiles stays plain -- same bits either way"""
    L = _lib.load()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = ((8 * 25 * 42 + 63) // 64) * 4
    in_class = 2 * cus <= tiles < 3 * cus and (tiles + cus - 1) // cus * cus * 5 >= tiles * 6
    lat = [_dev(t) for t in _operands(8, 25, 42, 2048, 256, 1, 1, 0, True, True, False, 48)]
    c33 = [_dev(t) for t in _operands(8, 25, 42, 256, 256, 3, 1, 1, True, True, True, 50)]
    many = [_dev(t) for t in _operands(2, 25, 53, 64, 2048, 1, 1, 0, True, True, False, 49)]
    calls = [lambda: ops.conv2d_nhwc(lat[0], lat[1], lat[2], lat[3], None, True, 1, 0),
             lambda: ops.conv2d_nhwc(c33[0], c33[1], c33[2], c33[3], c33[4], True, 1, 1)]
    try:
        for i, fn in enumerate(calls):
            assert L.brcnn_conv_set_tile(-5, 0) == 0
            ref = fn()
            assert L.brcnn_conv_set_tile(-5, 1) == 0
            n0 = _launches(L)
            out = fn()
            assert _launches(L) == n0 + (1 if in_class else 0), i
            assert torch.equal(out, ref), i
        n0 = _launches(L)
        ops.conv2d_nhwc(many[0], many[1], many[2], many[3], None, True, 1, 0)
        assert _launches(L) == n0
    finally:
        L.brcnn_conv_set_tile(-5, 1)


def test_persistent_launch_repeated_beside_a_second_stream():
    """20 forced launches in a row while a second stream streams memory: every result is the plain one, and no
    hand-over was lost"""
    L = _lib.load()
    x, wt, sc, sh, r = (_dev(t) for t in _operands(2, 25, 53, 224, 2048, 1, 1, 0, True, True, True, 47))
    fn = lambda: ops.conv2d_nhwc(x, wt, sc, sh, r, True, 1, 0)
    side = torch.cuda.Stream()
    a = torch.empty(64 << 20, device=DEV)           # 256 MiB copied back and forth: bandwidth bound
    b = torch.empty_like(a)
    torch.cuda.synchronize()
    try:
        assert L.brcnn_conv_set_tile(-5, 0) == 0
        ref = fn()
        assert L.brcnn_conv_set_tile(-5, 2) == 0
        n0 = _launches(L)
        outs = []
        for i in range(20):
            with torch.cuda.stream(side):
                b.copy_(a)
                a.copy_(b)
            outs.append(fn())
        torch.cuda.synchronize()
        assert _launches(L) == n0 + 20
    finally:
        L.brcnn_conv_set_tile(-5, 1)
    for i, out in enumerate(outs):
        assert torch.equal(out, ref), i
    assert L.brcnn_conv_handover_status() == 0
