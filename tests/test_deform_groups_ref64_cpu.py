"""tests/deform_groups_ref64.py without a device: the fold of deform groups into the batch against per-group calls of
deform_ref64, v1 against v2 with saturated masks, and the bounds against references with one convention wrong."""
import pytest
import torch

from tests import deform_groups_ref64 as DG
from tests import deform_ref64 as D
from tests import route_util as R


def _inputs(C, G, modulated, seed, **kw):
    s = DG.spec(C, G, modulated, torch.float32, seed, **kw)
    return (s,) + DG.make_inputs(s)


@pytest.mark.parametrize('stride', [1, 2])
def test_g1_modulated_is_deform_ref64_exactly(stride):
    s, x, om, dcol = _inputs(8, 1, True, 11, stride=stride)
    kw = DG.conv_kw(s)
    assert torch.equal(DG.im2col64(x, om, **kw), D.im2col64(x, om, **kw))
    a, b = DG.adjoint64(x, om, dcol, **kw), D.adjoint64(x, om, dcol, **kw)
    for n in ('dx', 'dom', 'S_dx', 'S_om', 'mask_slip'):
        assert torch.equal(getattr(a, n), getattr(b, n)), n
    assert torch.equal(a.cnt, b.cnt.expand_as(a.cnt))


@pytest.mark.parametrize('C,G,Cpad', [(16, 2, 16), (24, 3, 32), (16, 4, 16)])
@pytest.mark.parametrize('modulated', [True, False])
def test_groups_equal_per_group_calls_on_slices(C, G, Cpad, modulated):
    s, x, om, dcol = _inputs(C, G, modulated, 12, Cpad=Cpad)
    cg, T = C // G, 9
    col = DG.im2col64(x, om, G, modulated, channels_padded=Cpad).view(-1, T, Cpad)
    b = DG.adjoint64(x, om, dcol, G, modulated, channels_padded=Cpad)
    assert torch.equal(col[..., C:], torch.zeros_like(col[..., C:]))
    for g in range(G):
        lg = om[..., 2 * T * G + T * g:2 * T * G + T * (g + 1)] if modulated else torch.full(om.shape[:3] + (T,), 100.0)
        om_g = torch.cat([om[..., 2 * T * g:2 * T * (g + 1)], lg], -1)
        x_g = x[..., g * cg:(g + 1) * cg]
        assert torch.equal(col[..., g * cg:(g + 1) * cg].reshape(-1, T * cg), D.im2col64(x_g, om_g))
        d_g = dcol.view(-1, T, Cpad)[..., g * cg:(g + 1) * cg].reshape(-1, T * cg)
        a = D.adjoint64(x_g, om_g, d_g)
        assert torch.equal(b.dx[..., g * cg:(g + 1) * cg], a.dx)
        assert torch.equal(b.dom[..., 2 * T * g:2 * T * (g + 1)], a.dom[..., :2 * T])
        if modulated:
            assert torch.equal(b.dom[..., 2 * T * G + T * g:2 * T * G + T * (g + 1)], a.dom[..., 2 * T:])
    assert b.dom.shape[-1] == DG.om_width(G, modulated)


def test_v1_is_v2_with_saturated_masks_columns_only():
    s, x, om, _ = _inputs(16, 2, False, 13)
    om2 = torch.cat([om, torch.full(om.shape[:3] + (18,), 100.0)], -1)
    assert torch.equal(DG.im2col64(x, om, 2, False), DG.im2col64(x, om2, 2, True))


def test_constants_follow_the_documented_terms():
    assert DG.col_k(True) == D.COL_K and DG.dx_c0(True) == D.DX_C0 and DG.dom_chain(64, True) == D.dom_chain(64)
    assert DG.col_k(False) == D.COL_K - D.SIG and DG.dx_c0(False) == D.DX_C0 - D.SIG
    assert DG.dom_chain(64, False) == D.dom_chain(64) - D.SIG


@pytest.mark.parametrize('mutation,modulated', [('mask_interleave', True), ('group_mod', True), ('group_mod', False),
                                                ('swap', True), ('swap', False)])
def test_bounds_reject_a_reference_with_one_convention_wrong(mutation, modulated):
    s, x, om, dcol = _inputs(16, 2, modulated, 14)
    ref = DG.im2col64(x, om, 2, modulated)
    extra = DG.col_extra(DG.im2col64(x, om, 2, modulated, magnitude=True), modulated)
    bad = DG.im2col64(x, om, 2, modulated, mutation=mutation)
    assert R.excess(ref.float(), ref, torch.float32, extra) <= 0          # the reference rounded to fp32 is inside
    assert R.excess(bad.float(), ref, torch.float32, extra) > 0
    if mutation != 'mask_interleave':
        a, m = DG.adjoint64(x, om, dcol, 2, modulated), DG.adjoint64(x, om, dcol, 2, modulated, mutation=mutation)
        assert R.excess(m.dx.float(), a.dx, torch.float32, DG.dx_extra(a, modulated)) > 0
        assert R.excess(m.dom.float(), a.dom, torch.float32, DG.dom_extra(a, 8, modulated)) > 0
        assert R.excess(a.dom.float(), a.dom, torch.float32, DG.dom_extra(a, 8, modulated)) <= 0


def test_inputs_are_dyadic_and_carry_the_edge_table():
    s, x, om, _ = _inputs(16, 2, True, 15)
    off = om[..., :36]
    near = off.abs() < 1e3
    assert torch.equal((off[near] * 16).round(), off[near] * 16)
    # 2 images x 2 groups x 63 pixels x 9 taps = 2268 slots hold all 324 pairs of the 7 x 9 map
    assert len(D.edge_pairs(s)) == 324
    for lgt in D.MASK_SPECIALS:
        assert (om[..., 36:] == lgt).any()
