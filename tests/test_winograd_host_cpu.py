"""The host side of the Winograd conv (csrc/conv_winograd_f32.hip) that needs no device: the tile table behind the
workspace size, and the policy switch with its two counters (csrc/policy.h)."""
import ctypes

import brcnn  # noqa: F401
from brcnn import lib


def _bytes(batch, sizes, cin):
    L = len(sizes)
    hs = (ctypes.c_int * L)(*[h for h, _ in sizes])
    ws = (ctypes.c_int * L)(*[w for _, w in sizes])
    return lib.load().brcnn_conv3x3_winograd_f32_multi_workspace_bytes(batch, L, hs, ws, cin)


def test_tile_table_counts_half_empty_tiles():
    """tiles per segment = batch * ceil(H / 2) * ceil(W / 2): odd heights and widths give half-empty tiles"""
    cases = [(1, [(2, 2)]), (1, [(1, 1)]), (2, [(1, 5)]), (1, [(5, 1)]), (2, [(7, 11)]), (2, [(8, 12)]), (3, [(13, 21)]),
             (2, [(8, 12), (5, 7), (3, 3), (1, 2)]), (8, [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)])]
    for batch, sizes in cases:
        for cin in (32, 256):
            tiles = sum(batch * -(-h // 2) * -(-w // 2) for h, w in sizes)
            assert _bytes(batch, sizes, cin) == 16 * tiles * cin * 4, (batch, sizes, cin)
    # the tower of the flagship pass: 44 992 tiles
    assert _bytes(8, [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)], 256) == 16 * 44992 * 256 * 4
    # refused geometry: 0
    assert _bytes(0, [(4, 4)], 32) == 0 and _bytes(1, [(0, 4)], 32) == 0 and _bytes(1, [(4, 4)], 0) == 0
    assert _bytes(1, [(4, 4)] * 9, 32) == 0


def test_winograd_switch_and_counters_without_a_gpu():
    L = lib.load()
    before = L.brcnn_conv_set_tile(-11, 2)
    try:
        assert before in (0, 1)
        for v in (0, 1):
            assert L.brcnn_conv_set_tile(-11, v) == 0 and L.brcnn_conv_set_tile(-11, 2) == v
        for n in range(11, 19):
            assert L.brcnn_conv_set_tile(-11, n) == 0
        for bad in (-1, 3, 10, 19):
            assert L.brcnn_conv_set_tile(-11, bad) == -22
        assert L.brcnn_conv_set_tile(-12, 0) == 0 and L.brcnn_conv_set_tile(-12, 1) == 0      # nothing has launched
        assert L.brcnn_conv_set_tile(-12, 2) == -22
    finally:
        L.brcnn_conv_set_tile(-11, 11)
        L.brcnn_conv_set_tile(-11, before)
