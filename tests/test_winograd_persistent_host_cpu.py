"""The host side of the persistent launch of the fp32 Winograd GEMM that needs no device: the hook codes (-16, n) with their
counters (csrc/policy.h, csrc/policy.hip) and the measured rule (brcnn_winograd_persistent_rule) at its measured points, on
both sides of each threshold (profiles/f32_winograd_persistent.txt)."""
import pytest

import brcnn  # noqa: F401
from brcnn import lib

EINVAL = -22


@pytest.fixture()
def hooks():
    L = lib.load()
    before = (L.brcnn_conv_set_tile(-16, 3), L.brcnn_conv_set_tile(-16, 24), L.brcnn_conv_set_tile(-16, 39),
              L.brcnn_conv_set_tile(-16, 999), L.brcnn_conv_set_tile(-16, 49))
    yield L
    assert L.brcnn_conv_set_tile(-16, before[0]) == 0 and L.brcnn_conv_set_tile(-16, 20 + before[1]) == 0
    assert L.brcnn_conv_set_tile(-16, 30 + before[2]) == 0 and L.brcnn_conv_set_tile(-16, 1000 + before[3]) == 0
    assert L.brcnn_conv_set_tile(-16, 40 + before[4]) == 0


def test_defaults(hooks):
    L = hooks
    # the measured rule decides, no caps, the tower's tile by its rule
    assert (L.brcnn_conv_set_tile(-16, 3), L.brcnn_conv_set_tile(-16, 24), L.brcnn_conv_set_tile(-16, 39),
            L.brcnn_conv_set_tile(-16, 999), L.brcnn_conv_set_tile(-16, 49)) == (1, 0, 0, 0, 0)


def test_hook_codes_set_read_back_and_refuse(hooks):
    L = hooks
    for mode in (0, 2, 1):
        assert L.brcnn_conv_set_tile(-16, mode) == 0 and L.brcnn_conv_set_tile(-16, 3) == mode
    for v in (1, 3, 0):
        assert L.brcnn_conv_set_tile(-16, 20 + v) == 0 and L.brcnn_conv_set_tile(-16, 24) == v
    assert L.brcnn_conv_set_tile(-16, 22) == EINVAL and L.brcnn_conv_set_tile(-16, 24) == 0      # 32 x 128 is no tower tile
    for n in (1, 2, 8, 0):
        assert L.brcnn_conv_set_tile(-16, 30 + n) == 0 and L.brcnn_conv_set_tile(-16, 39) == n
    for d in (2, 3, 0):
        assert L.brcnn_conv_set_tile(-16, 40 + d) == 0 and L.brcnn_conv_set_tile(-16, 49) == d
    for n in (1, 32, 2048, 0):
        assert L.brcnn_conv_set_tile(-16, 1000 + n) == 0 and L.brcnn_conv_set_tile(-16, 999) == n
    readers = {3, 10, 11, 12, 13, 24, 39, 49, 999}
    accepted = {0, 1, 2, 20, 21, 23, 40, 42, 43} | set(range(30, 39)) | set(range(1000, 3049))
    for nt in list(range(-3, 60)) + [128, 256, 998, 3049, 4000, 1 << 20]:
        if nt in readers:
            continue
        assert L.brcnn_conv_set_tile(-16, nt) == (0 if nt in accepted else EINVAL), nt
        assert L.brcnn_conv_set_tile(-16, 1) == 0 and L.brcnn_conv_set_tile(-16, 20) == 0
        assert L.brcnn_conv_set_tile(-16, 30) == 0 and L.brcnn_conv_set_tile(-16, 1000) == 0 and L.brcnn_conv_set_tile(-16, 40) == 0
    # the hook leaves its neighbours alone, and -15 stays no code at all
    assert L.brcnn_conv_set_tile(-14, 3) in (0, 1, 2) and L.brcnn_conv_set_tile(-15, 0) == EINVAL
    assert L.brcnn_conv_set_tile(-17, 0) == EINVAL


def test_counters_read_zero_and_clear_with_the_others(hooks):
    L = hooks
    # nothing launches without a device
    assert L.brcnn_conv_set_tile(-9, -1) == 0
    for n in (10, 11, 12, 13):
        assert L.brcnn_conv_set_tile(-16, n) == 0
    assert L.brcnn_conv_set_tile(-16, 14) == EINVAL and L.brcnn_conv_set_tile(-16, 9) == EINVAL
    assert L.brcnn_conv_set_tile(-12, 0) == 0 and L.brcnn_conv_set_tile(-14, 10) == 0


def _rule(wg_tiles, per_cu, cus=256, units=16):
    return lib.load().brcnn_winograd_persistent_rule(wg_tiles, units, cus, per_cu)


# The measured table (profiles/f32_winograd_persistent.txt, 256 CUs): GEMM tiles of each point with the workgroups per CU
# its persistent launch runs, and whether the form won there (gain beyond the spread of the plain rounds)
WON = [(264, 1), (280, 1), (320, 1), (528, 2)]
LOST = [(396, 1), (512, 2), (640, 2), (2100, 4), (1406, 2), (2812, 4)]


def test_rule_at_its_measured_points():
    for t, per_cu in WON:
        assert _rule(t, per_cu) == 1, t
    for t, per_cu in LOST:
        assert _rule(t, per_cu) == 0, t


def test_rule_thresholds_are_the_midpoints():
    # one workgroup per CU: 320 won, 396 lost -> 358
    assert _rule(357, 1) == 1 and _rule(358, 1) == 0 and _rule(256, 1) == 1 and _rule(255, 1) == 0
    # two per CU: 512 lost, 528 won, 640 lost -> 520 .. 583
    assert _rule(519, 2) == 0 and _rule(520, 2) == 1 and _rule(583, 2) == 1 and _rule(584, 2) == 0
    # the same classes on another device are the same tiles per CU
    assert _rule(264 * 2, 1, cus=512) == 1 and _rule(396 * 2, 1, cus=512) == 0 and _rule(528 // 2, 2, cus=128) == 1
    # a per-CU cap on a many-tile launch does not make it a few-tile one
    assert _rule(2100, 1) == 0 and _rule(2100, 2) == 0
    # three and more whole chains per CU were not measured
    assert _rule(800, 3) == 0 and _rule(1056, 4) == 0
    # nothing for degenerate arguments
    assert _rule(0, 2) == 0 and _rule(528, 0) == 0 and _rule(528, 2, cus=0) == 0 and _rule(528, 2, units=8) == 0
