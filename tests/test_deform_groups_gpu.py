"""-m gpu: the deformable conv entries with deform groups and the unmodulated form (brcnn_deform_im2col_nhwc_g,
brcnn_deform_col2im_nhwc_g, brcnn_deform_conv_nhwc_g, brcnn_deform_conv_route) against the float64 restatement of
tests/deform_groups_ref64.py, fp32 / bf16 / fp16, v1 and v2.  Inputs are rounded to the dtype first and every offset is
dyadic: no element is excluded from any comparison.

Shapes: the smallest at which the group indexing can go wrong -- C = 16, G = 2 (8 channels per group, the 16-bit minimum);
C = 24 in 32 padded, G = 3 (pad channels outside every group); C = 128 with G = 1 / 2 / 4 -- on 7 x 9 and 5 x 6 maps at
batch 2, stride 1 and 2, with the edge table.  Fused kernel: a group boundary between K steps (C = 128, G = 2), output
channel blocks (cout = 512), stride 2, pixel counts that are no multiple of the 128-row tile (126, 442)."""
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import lib, ops
from brcnn.autograd import deform_conv_autograd
from tests import deform_groups_ref64 as DG
from tests import deform_ref64 as D
from tests import route_util as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EINVAL = -22
f32, bf16, f16 = torch.float32, torch.bfloat16, torch.float16
DT_IDS = {f32: 'f32', bf16: 'bf16', f16: 'f16'}
SHAPES = [(16, 16, 2), (24, 32, 3), (128, 128, 1), (128, 128, 2), (128, 128, 4)]          # C, Cpad, G
MAPS = [(7, 9, 1), (7, 9, 2), (5, 6, 1), (5, 6, 2)]                                       # H, W, stride


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _args(s):
    return (s['N'], s['H'], s['W'], s['C'], 3, 3, s['stride'], s['pad'], 1, s['om_stride'], s['Cpad'])


def _im2col_g(s, x, om, G=None, mod=None):
    Ho, Wo = D.out_size(s['H'], s['W'], 3, 3, s['stride'], s['pad'], 1)
    col = torch.ones(s['N'] * Ho * Wo, 9 * s['Cpad'], dtype=s['dtype'], device=DEV)
    st = lib.load().brcnn_deform_im2col_nhwc_g(x.data_ptr(), om.data_ptr(), col.data_ptr(), *_args(s),
                                               s['G'] if G is None else G, int(s['modulated'] if mod is None else mod),
                                               ops._dt(x), ops._stream())
    assert st == 0, st
    return col


def _col2im_g(s, x, om, dcol):
    dx = torch.zeros(x.shape, dtype=f32, device=DEV)
    dom = torch.full(om.shape, 7.0, dtype=f32, device=DEV)        # every entry of a row must be written
    st = lib.load().brcnn_deform_col2im_nhwc_g(x.data_ptr(), om.data_ptr(), dcol.data_ptr(), dx.data_ptr(), dom.data_ptr(),
                                               *_args(s), s['G'], int(s['modulated']), ops._dt(x), ops._stream())
    assert st == 0, st
    return dx, dom


def _counters():
    L = lib.load()
    return L.brcnn_conv_set_tile(-13, 10), L.brcnn_conv_set_tile(-13, 11)


@pytest.mark.parametrize('hws', MAPS, ids=lambda m: f'{m[0]}x{m[1]}s{m[2]}')
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'C{s[0]}in{s[1]}G{s[2]}')
@pytest.mark.parametrize('modulated', [False, True], ids=['v1', 'v2'])
@pytest.mark.parametrize('dt', [f32, bf16, f16], ids=['f32', 'bf16', 'f16'])
def test_im2col_and_col2im_against_float64(dt, modulated, shape, hws):
    (C, Cpad, G), (H, W, stride) = shape, hws
    s = DG.spec(C, G, modulated, dt, 200 + 7 * SHAPES.index(shape) + MAPS.index(hws), H=H, W=W, stride=stride, Cpad=Cpad)
    x, om, dcol = DG.make_inputs(s, DEV)
    kw = dict(DG.conv_kw(s), channels_padded=Cpad)
    col = _im2col_g(s, x, om)
    ref = DG.im2col64(x, om, G, modulated, **kw)
    mag = DG.im2col64(x, om, G, modulated, magnitude=True, **kw)
    e = R.excess(col, ref, dt, DG.col_extra(mag, modulated))
    print(f'fp64 leg im2col: largest error minus bound {e:.3e}')
    assert bool(torch.isfinite(col.float()).all()) and e <= 0, e
    assert not bool(_bits(col).view(-1, 9, Cpad)[..., C:].any()), 'pad columns are not bit-zero'
    dx, dom = _col2im_g(s, x, om, dcol)
    b = DG.adjoint64(x, om, dcol, G, modulated, **kw)
    e_dx = R.excess(dx, b.dx, f32, DG.dx_extra(b, modulated))
    e_dom = R.excess(dom, b.dom, f32, DG.dom_extra(b, C // G, modulated))
    print(f'fp64 leg col2im: largest error minus bound  dx {e_dx:.3e}  d_om {e_dom:.3e}')
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dom).all())
    assert e_dx <= 0 and e_dom <= 0, (e_dx, e_dom)
    if G > 1:       # the kernel's result is outside the bound of a reference with the group conventions wrong
        wrong = DG.im2col64(x, om, G, modulated, mutation='group_mod', **kw)
        assert R.excess(col, wrong, dt, DG.col_extra(mag, modulated)) > 0
        if modulated:
            wrong = DG.im2col64(x, om, G, modulated, mutation='mask_interleave', **kw)
            assert R.excess(col, wrong, dt, DG.col_extra(mag, modulated)) > 0


# ---- the fused kernel -------------------------------------------------------------------------------------------------------
FUSED = {'c128_g1': (128, 128, 1, 7, 9, 1), 'c128_g2_group_boundary': (128, 128, 2, 7, 9, 1), 'cout512_blocks': (64, 512, 1, 7, 9, 1),
         'c128_cout64_s2': (128, 64, 1, 7, 9, 2), 'c256_g2_m442_four_tiles': (256, 64, 2, 13, 17, 1)}


def _fused_inputs(name, dt, modulated):
    C, cout, G, H, W, stride = FUSED[name]
    s = DG.spec(C, G, modulated, dt, 300 + list(FUSED).index(name), H=H, W=W, stride=stride)
    x, om, _ = DG.make_inputs(s, DEV)
    g = torch.Generator().manual_seed(s['seed'] + 1000)
    w = (torch.randn(cout, 3, 3, C, generator=g) / (9 * C) ** 0.5).to(dt).to(DEV)
    sc, sh = (torch.rand(cout, generator=g) + 0.5).to(DEV), (torch.randn(cout, generator=g) * 0.2).to(DEV)
    return s, x, om, w, sc, sh


@pytest.mark.parametrize('name', list(FUSED))
@pytest.mark.parametrize('modulated', [False, True], ids=['v1', 'v2'])
@pytest.mark.parametrize('dt', [bf16, f16], ids=['bf16', 'f16'])
def test_fused_conv_against_float64(dt, modulated, name):
    """against float64 all the way: the columns' one rounding and the blend's fp32 error, both summed through |w|, on top
    of route_util.bound (the fp32 accumulation and the result's one rounding)"""
    s, x, om, w, sc, sh = _fused_inputs(name, dt, modulated)
    C, cout, G = s['C'], w.shape[0], s['G']
    lib.load().brcnn_conv_set_tile(-9, -1)
    assert ops.deform_conv_route(x, cout, s['stride'], 1, G) == (cout <= 128)      # the default rule: one workgroup column
    for scale, shift, relu in ((None, None, False), (sc, sh, True)):
        y = ops.deform_conv_nhwc(x, om, w, scale, shift, relu, s['stride'], 1, G, modulated)
        ref = DG.deform_conv64(x, om, w, G, modulated, s['stride'], 1)
        mag = DG.im2col64(x, om, G, modulated, stride=s['stride'], pad=1, magnitude=True)
        extra = (R.half_ulp(dt) * 1.001 + DG.col_k(modulated) * DG.U) * \
            (mag @ w.double().abs().view(cout, 9 * C).t()).view(ref.shape)
        if scale is not None:
            ref, extra = (ref * scale.double() + shift.double()).relu(), extra * scale.double()
        assert ref.abs().max().item() > 0.05
        e = R.excess(y, ref, dt, extra)
        print(f'fp64 leg fused {name}: largest error minus bound {e:.3e}')
        assert y.dtype == dt and bool(torch.isfinite(y.float()).all()) and e <= 0, (name, e)
    assert _counters() == (2, 0)


@pytest.mark.parametrize('modulated', [False, True], ids=['v1', 'v2'])
def test_fused_refuses_32_channel_groups_and_the_caller_takes_im2col(modulated):
    s = DG.spec(128, 4, modulated, bf16, 320)
    x, om, _ = DG.make_inputs(s, DEV)
    w = (torch.randn(128, 128, 3, 3, generator=torch.Generator().manual_seed(321)) / 34.0).to(bf16).float().to(DEV)
    L = lib.load()
    y = torch.empty(2, 7, 9, 128, dtype=bf16, device=DEV)
    wp = w.permute(0, 2, 3, 1).to(bf16).contiguous()
    st = L.brcnn_deform_conv_nhwc_g(x.data_ptr(), om.data_ptr(), wp.data_ptr(), None, None, y.data_ptr(), 2, 7, 9, 128, 128,
                                    1, 1, 0, s['om_stride'], 4, int(modulated), ops.DT_BF16, ops._stream())
    assert st == EINVAL
    assert not ops.deform_conv_route(x, 128, 1, 1, 4) and ops.deform_conv_route(x, 128, 1, 1, 2)
    L.brcnn_conv_set_tile(-9, -1)
    with torch.no_grad():
        y = deform_conv_autograd(x, om, w, 1, 1, 4, modulated, route=True)
    assert _counters() == (0, 1)                     # no fused launch, one im2col launch
    ref = DG.deform_conv64(x, om, wp, 4, modulated)
    mag = DG.im2col64(x, om, 4, modulated, magnitude=True)
    extra = (R.half_ulp(bf16) * 1.001 + DG.col_k(modulated) * DG.U) * (mag @ wp.double().abs().view(128, -1).t()).view(ref.shape)
    assert R.excess(y, ref, bf16, extra) <= 0
    # the policy switch sends an accepted shape to im2col + GEMM as well, and back
    try:
        assert L.brcnn_conv_set_tile(-13, 0) == 0 and not ops.deform_conv_route(x, 128, 1, 1, 2)
        s2 = DG.spec(128, 2, modulated, bf16, 322)
        x2, om2, _ = DG.make_inputs(s2, DEV)
        with torch.no_grad():
            y0 = deform_conv_autograd(x2, om2, w, 1, 1, 2, modulated, route=True)
        assert _counters() == (0, 1)
        assert L.brcnn_conv_set_tile(-13, 2) == 0 and L.brcnn_conv_set_tile(-13, 3) == 2
        with torch.no_grad():
            y1 = deform_conv_autograd(x2, om2, w, 1, 1, 2, modulated, route=True)
        assert _counters() == (1, 0)
        ref2 = DG.deform_conv64(x2, om2, wp, 2, modulated)
        tol = R.bound(ref2, bf16).max().item() * 4
        assert (y0.double() - y1.double()).abs().max().item() <= tol
        # the call form without `route` (the Res2Net recipes) never asks the table: fused even where the table says never
        assert L.brcnn_conv_set_tile(-13, 0) == 0
        with torch.no_grad():
            y2 = deform_conv_autograd(x2, om2, w, 1, 1, 2, modulated)
        assert _counters() == (1, 0) and torch.equal(_bits(y2), _bits(y1))
    finally:
        assert L.brcnn_conv_set_tile(-13, 1) == 0


@pytest.mark.parametrize('dt', [bf16, f16], ids=['bf16', 'f16'])
def test_res2net_call_form_keeps_the_fused_kernel_at_cout_256(dt):
    """`deform_conv_autograd(x, om, w, stride, pad)` as Bottle2neck._forward_train calls it, at the stage-4 width where
    the default rule of the table would pick im2col + GEMM: one fused launch, the bits of the original entry point"""
    s = DG.spec(256, 1, True, dt, 325)
    x, om, _ = DG.make_inputs(s, DEV)
    w = (torch.randn(256, 256, 3, 3, generator=torch.Generator().manual_seed(326)) / 48.0).to(dt).float().to(DEV)
    assert not ops.deform_conv_route(x, 256, 1, 1, 1)
    lib.load().brcnn_conv_set_tile(-9, -1)
    with torch.no_grad():
        y = deform_conv_autograd(x, om, w, 1, 1)
    assert _counters() == (1, 0)
    old = ops.deform_conv_nhwc(x, om, w.permute(0, 2, 3, 1).to(dt).contiguous(), None, None, False, 1, 1)
    assert torch.equal(_bits(y), _bits(old))


def test_bad_arguments_are_refused():
    L = lib.load()
    s_ = ops._stream()
    x = torch.zeros(1, 8, 8, 128, dtype=bf16, device=DEV)
    xf = torch.zeros(1, 8, 8, 128, device=DEV)
    om = torch.zeros(1, 8, 8, 27 * 16, device=DEV)
    col = torch.empty(64, 9 * 128, device=DEV)
    dcol = torch.zeros(64, 9 * 128, device=DEV)
    dx = torch.zeros(1, 8, 8, 128, device=DEV)
    w = torch.zeros(128, 3, 3, 128, dtype=bf16, device=DEV)
    y = torch.empty(1, 8, 8, 128, dtype=bf16, device=DEV)
    P = lambda t: t.data_ptr()      # noqa: E731

    def im2col(t, c, cp, G, mod, dt, oms=None):
        oms = (27 if mod else 18) * G if oms is None else oms
        return L.brcnn_deform_im2col_nhwc_g(P(t), P(om), P(col), 1, 8, 8, c, 3, 3, 1, 1, 1, oms, cp, G, mod, dt, s_)

    def col2im(t, c, G, mod, dt, oms=None):
        oms = (27 if mod else 18) * G if oms is None else oms
        return L.brcnn_deform_col2im_nhwc_g(P(t), P(om), P(dcol), P(dx), P(om.clone()), 1, 8, 8, c, 3, 3, 1, 1, 1, oms, c, G,
                                            mod, dt, s_)

    def fused(c, cout, G, mod, oms=None, dt=ops.DT_BF16, stride=1):
        oms = (27 if mod else 18) * G if oms is None else oms
        return L.brcnn_deform_conv_nhwc_g(P(x), P(om), P(w), None, None, P(y), 1, 8, 8, c, cout, stride, 1, 0, oms, G, mod, dt, s_)

    assert im2col(xf, 128, 128, 2, 1, ops.DT_F32) == 0 and im2col(x, 128, 128, 2, 0, ops.DT_BF16) == 0
    assert im2col(xf, 128, 128, 3, 1, ops.DT_F32) == EINVAL                       # C % G
    assert im2col(xf, 24, 24, 3, 1, ops.DT_F32) == 0 and im2col(x, 24, 24, 3, 1, ops.DT_BF16) == 0
    assert im2col(xf, 24, 24, 2, 1, ops.DT_F32) == 0 and im2col(x, 24, 24, 2, 1, ops.DT_BF16) == EINVAL    # 16-bit: 12 per group
    assert im2col(xf, 24, 24, 12, 1, ops.DT_F32) == EINVAL                        # fp32: 2 per group
    assert im2col(xf, 128, 128, 2, 1, ops.DT_F32, 53) == EINVAL and im2col(xf, 128, 128, 2, 0, ops.DT_F32, 35) == EINVAL
    assert im2col(xf, 128, 128, 0, 1, ops.DT_F32) == EINVAL and im2col(xf, 128, 128, 2, 2, ops.DT_F32) == EINVAL
    assert im2col(xf, 128, 128, 2, 1, 7) == EINVAL
    assert col2im(xf, 128, 2, 1, ops.DT_F32) == 0 and col2im(x, 128, 2, 0, ops.DT_BF16) == 0
    assert col2im(xf, 128, 3, 1, ops.DT_F32) == EINVAL and col2im(x, 24, 2, 1, ops.DT_BF16) == EINVAL
    assert col2im(xf, 128, 2, 1, ops.DT_F32, 64) == EINVAL                        # the row is exactly the layout
    assert fused(128, 128, 2, 1) == 0 and fused(128, 128, 1, 0) == 0 and fused(128, 64, 2, 0) == 0
    assert fused(128, 128, 4, 1) == EINVAL and fused(128, 128, 3, 1) == EINVAL    # 32 per group; C % G
    assert fused(128, 96, 1, 1) == EINVAL and fused(128, 0, 1, 1) == EINVAL       # cout % 64
    assert fused(128, 128, 2, 1, 53) == EINVAL and fused(128, 128, 2, 0, 35) == EINVAL
    assert fused(128, 128, 1, 1, dt=ops.DT_F32) == EINVAL and fused(128, 128, 1, 1, stride=3) == EINVAL
    assert L.brcnn_deform_conv_route(1, 8, 8, 128, 128, 1, 1, 4, ops.DT_BF16) == 0
    assert L.brcnn_deform_conv_route(1, 8, 8, 128, 128, 1, 1, 2, ops.DT_F32) == 0
    assert L.brcnn_conv_set_tile(-13, 4) == EINVAL
    torch.cuda.synchronize()


# ---- bit identity with the entries the Res2Net recipes run through ---------------------------------------------------------
@pytest.mark.parametrize('dt', [f32, bf16, f16], ids=['f32', 'bf16', 'f16'])
def test_g1_modulated_equals_the_original_entries_bit_for_bit(dt):
    s = D._spec(64, 2, 7, 9, dt, 330, kind='edge')
    x, om, dcol = D.make_inputs(s, DEV)
    sg = dict(s, G=1, modulated=True)
    L = lib.load()
    a = (s['N'], s['H'], s['W'], s['C'], 3, 3, 1, 1, 1, 27, 64)
    old = torch.ones(2 * 63, 9 * 64, dtype=dt, device=DEV)
    if dt == f32:
        assert L.brcnn_deform_im2col_nhwc(x.data_ptr(), om.data_ptr(), old.data_ptr(), *a, ops._stream()) == 0
    else:
        assert L.brcnn_deform_im2col_nhwc_ex(x.data_ptr(), om.data_ptr(), old.data_ptr(), *a, ops._dt(x), ops._stream()) == 0
    assert torch.equal(_bits(_im2col_g(sg, x, om)), _bits(old))
    dx0, dom0 = torch.zeros(x.shape, device=DEV), torch.full(om.shape, 7.0, device=DEV)
    assert L.brcnn_deform_col2im_nhwc_ex(x.data_ptr(), om.data_ptr(), dcol.data_ptr(), dx0.data_ptr(), dom0.data_ptr(), *a,
                                         ops._dt(x), ops._stream()) == 0
    dx1, dom1 = _col2im_g(sg, x, om, dcol)
    assert torch.equal(_bits(dom1), _bits(dom0))
    b = D.adjoint64(x, om, dcol)
    assert R.excess(dx1, b.dx, f32, D.dx_extra(b)) <= 0 and R.excess(dx0, b.dx, f32, D.dx_extra(b)) <= 0   # (atomics: any order)
    assert ((dx1 - dx0).abs().double() <= 2 * R.bound(b.dx, f32, D.dx_extra(b))).all()


@pytest.mark.parametrize('dt', [bf16, f16], ids=['bf16', 'f16'])
def test_fused_g1_modulated_and_output_blocks_bit_for_bit(dt):
    s, x, om, w, sc, sh = _fused_inputs('cout512_blocks', dt, True)
    L = lib.load()
    y512 = ops.deform_conv_nhwc(x, om, w, sc, sh, True, 1, 1)                       # cout 512: the `_g` entry
    halves = [ops.deform_conv_nhwc(x, om, w[i:i + 256].contiguous(), sc[i:i + 256].contiguous(), sh[i:i + 256].contiguous(),
                                   True, 1, 1) for i in (0, 256)]                   # cout 256: the original entry
    assert torch.equal(_bits(y512), _bits(torch.cat(halves, 3)))
    y_g = torch.empty_like(halves[0])
    w0, sc0, sh0 = w[:256].contiguous(), sc[:256].contiguous(), sh[:256].contiguous()
    st = L.brcnn_deform_conv_nhwc_g(x.data_ptr(), om.data_ptr(), w0.data_ptr(), sc0.data_ptr(), sh0.data_ptr(), y_g.data_ptr(),
                                    2, 7, 9, 64, 256, 1, 1, 1, 27, 1, 1, ops._dt(x), ops._stream())
    assert st == 0 and torch.equal(_bits(y_g), _bits(halves[0]))


@pytest.mark.parametrize('modulated', [False, True], ids=['v1', 'v2'])
@pytest.mark.parametrize('dt', [bf16, f16], ids=['bf16', 'f16'])
def test_fused_a_operand_is_the_grouped_16bit_column_matrix(dt, modulated):
    """an identity weight over the whole K axis (cout = 9 * 128): every output is ONE product with 1, so y is the A operand"""
    s = DG.spec(128, 2, modulated, dt, 340)
    x, om, _ = DG.make_inputs(s, DEV)
    K = 9 * 128
    w = torch.eye(K, dtype=dt, device=DEV).view(K, 3, 3, 128).contiguous()
    y = ops.deform_conv_nhwc(x, om, w, None, None, False, 1, 1, 2, modulated)
    col = _im2col_g(s, x, om)
    assert torch.equal(_bits(y.view(-1, K)), _bits(col))
    assert float(col.float().abs().max()) > 0
