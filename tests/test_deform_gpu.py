"""-m gpu: the modulated deformable conv family (csrc/deform.hip, csrc/deform_common.h, csrc/deform_conv_bf16.hip,
DeformIm2colFunction / DeformConvFunction) and the NHWC average pools against the float64 reference of
tests/deform_ref64.py, fp32 / bf16 / fp16.  The inputs are rounded to the dtype first and every offset is dyadic, so the
kernel's fp32 sample point is the reference's: no element is excluded from any comparison here.  Nothing is compared with
another launch of the same kernel but where a test says so (the fused conv against the GEMM of the im2col kernel's 16-bit
columns, which test_im2col_against_float64 holds to float64 on their own; the staged backward).

The cases of deform_ref64.cases() and what each is there for:
    edge                the 18 x 18 edge table: samples exactly on -1, 0, an interior integer, H - 1, H and 1/16 either side,
                        -1e4 / 1e4 / 3e9; mask logits -100, -20, -0.0, 0, 20, 100
    pile                144 taps into one cell with dcol > 0: many atomics on one dx element, S = the adjoint itself
    s{1,2}_p{0,1,2}*    3 x 3 at stride 1 and 2 with pad 0, 1 and 2, on odd and even maps
    dilation2, k1x1, k5x5, k1x3     dilation != 1, kh / kw != 3 and kh != kw
    om_stride64         offset rows padded to 64 (im2col only: the col2im entries take 27)
    cpad_208_224, cpad_8_24         channels_padded > channels (208 -> 224 is the fp32 padding of the 208-wide splits)
    c4, c8, c224, c260, c512        one lane; one 16-bit vector; the fp32 width of the padded splits; the second pass of
                        col2im's lane loop with a partial wave (260) and a full one (512)
    h1, w1, h2_w2, h1_w1            maps of 1 and 2 rows / columns
    batch3              the image index of a row
WRAP: the grid-stride loop of the im2col kernels past stream_grid's cap of 32768 workgroups.
FUSED: M of 1, 127, 128, 129 and 1350 (11 tiles: the XCD remap with q = 1, r = 3), Cp in {64, 128, 192, 256, 320, 512} with
Cout != Cp, stride 1 / 2, pad 0 / 1 / 2, om_stride 27 / 64, every epilogue branch, the edge table."""
import pytest
import torch
import torch.nn.functional as F

import brcnn  # noqa: F401
from brcnn import lib, ops
from brcnn.autograd import _ints, deform_conv_autograd, deform_im2col_autograd
from tests import deform_ref64 as D
from tests import route_util as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EINVAL = -22
CASES = D.cases()
IM2COL = [n for n, s in CASES.items() if s['im2col']]
COL2IM = [n for n, s in CASES.items() if s['col2im']]
SHARP = ['edge', 's1_p1', 's2_p1_odd', 'k5x5']
f32 = torch.float32
_kept = {}          # ('im2col' | 'col2im', name) -> results of the main legs: no kernel is rerun for the mutation legs


def _bits(t):
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _dims(spec):
    Ho, Wo = D.out_size(spec['H'], spec['W'], spec['kh'], spec['kw'], spec['stride'], spec['pad'], spec['dilation'])
    return spec['N'] * Ho * Wo, spec['kh'] * spec['kw']


def _geom_args(spec):
    return (spec['N'], spec['H'], spec['W'], spec['C'], spec['kh'], spec['kw'], spec['stride'], spec['pad'], spec['dilation'],
            spec['om_stride'], spec['Cpad'])


def _im2col(spec, x, om):
    """the C entry itself (ops.deform_im2col_nhwc takes square kernels only); every element prefilled with 1"""
    M, taps = _dims(spec)
    col = torch.ones(M, taps * spec['Cpad'], dtype=spec['dtype'], device=DEV)
    L = lib.load()
    if spec['dtype'] == f32:
        st = L.brcnn_deform_im2col_nhwc(x.data_ptr(), om.data_ptr(), col.data_ptr(), *_geom_args(spec), ops._stream())
    else:
        st = L.brcnn_deform_im2col_nhwc_ex(x.data_ptr(), om.data_ptr(), col.data_ptr(), *_geom_args(spec), ops._dt(x),
                                           ops._stream())
    assert st == 0, st
    return col


def _col2im(spec, x, om, dcol):
    """dx (zeroed, as the callers do) and d_om (prefilled with 7: every entry of a row must be written)"""
    dx = torch.zeros(x.shape, dtype=f32, device=DEV)
    dom = torch.full(om.shape, 7.0, dtype=f32, device=DEV)
    L = lib.load()
    if spec['dtype'] == f32:
        st = L.brcnn_deform_col2im_nhwc(x.data_ptr(), om.data_ptr(), dcol.data_ptr(), dx.data_ptr(), dom.data_ptr(),
                                        *_geom_args(spec), ops._stream())
    else:
        st = L.brcnn_deform_col2im_nhwc_ex(x.data_ptr(), om.data_ptr(), dcol.data_ptr(), dx.data_ptr(), dom.data_ptr(),
                                           *_geom_args(spec), ops._dt(x), ops._stream())
    assert st == 0, st
    return dx, dom


def _ref_cols(spec, x, om, mutation=0):
    kw = dict(D.conv_kw(spec), channels_padded=spec['Cpad'], mutation=mutation)
    return D.im2col64(x, om, **kw), D.im2col64(x, om, magnitude=True, **kw)


def _inside(spec, om):
    return D.geometry(om.double(), spec['N'], spec['H'], spec['W'], spec['kh'], spec['kw'], spec['stride'], spec['pad'],
                      spec['dilation']).inside


def _check_im2col(name, spec):
    x, om, _ = D.make_inputs(spec, DEV)
    col = _im2col(spec, x, om)
    ref, mag = _ref_cols(spec, x, om)
    e = R.excess(col, ref, spec['dtype'], D.col_extra(mag))
    print(f'fp64 leg im2col {name}: largest error minus bound {e:.3e}')
    assert bool(torch.isfinite(col.float()).all()) and e <= 0, (name, e)
    M, taps = _dims(spec)
    blocks = _bits(col).view(M, taps, spec['Cpad'])
    outside = ~_inside(spec, om).reshape(M, taps)
    assert not bool(blocks[outside].any()), 'a tap outside the domain left a non-zero column block'
    assert not bool(blocks[..., spec['C']:].any()), 'pad columns are not bit-zero'
    return dict(spec=spec, x=x, om=om, col=col)


@pytest.mark.parametrize('name', IM2COL)
def test_im2col_against_float64(name):
    r = _check_im2col(name, CASES[name])
    if name.rsplit('-', 1)[0] in SHARP:
        _kept[('im2col', name)] = r


@pytest.mark.parametrize('name', [f'{n}-{t}' for n in SHARP for t in ('f32', 'bf16', 'f16')])
def test_im2col_refuses_the_mutated_references(name):
    """on the host side of the kernel, from the columns the main leg kept: the offset pair read as (w, h), the mask logit
    read interleaved and the taps transposed are each outside the bound"""
    r = _kept.get(('im2col', name)) or _check_im2col(name, CASES[name])
    spec = r['spec']
    for m in (1, 2, 3):
        wrong, mag = _ref_cols(spec, r['x'], r['om'], mutation=m)
        assert R.excess(r['col'], wrong, spec['dtype'], D.col_extra(mag)) > 0, (name, m)


@pytest.mark.parametrize('name', sorted(D.WRAP))
def test_im2col_grid_stride_wrap(name):
    """more threads than 32768 workgroups hold: the rows past the cap come from the second trip of the loop"""
    spec = D.WRAP[name]
    assert D.im2col_threads(spec) > D.GRID_CAP_THREADS
    _check_im2col(name, spec)


def _check_col2im(name, spec):
    x, om, dcol = D.make_inputs(spec, DEV)
    dx, dom = _col2im(spec, x, om, dcol)
    b = D.adjoint64(x, om, dcol, channels_padded=spec['Cpad'], **D.conv_kw(spec))
    e_dx = R.excess(dx, b.dx, f32, D.dx_extra(b))
    e_dom = R.excess(dom, b.dom, f32, D.dom_extra(b, spec['C']))
    print(f'fp64 leg col2im {name} cnt<={int(b.cnt.max().item())} K={D.dom_chain(spec["C"])}: largest error minus bound  '
          f'dx {e_dx:.3e}  d_om {e_dom:.3e}')
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dom).all())
    assert e_dx <= 0 and e_dom <= 0, (name, e_dx, e_dom)
    taps = spec['kh'] * spec['kw']
    outside = ~b.inside
    for part in (dom[..., 0:2 * taps:2], dom[..., 1:2 * taps:2], dom[..., 2 * taps:3 * taps]):
        assert not bool(part[outside].any()), 'a tap outside the domain has an offset / mask gradient'
    dx2, dom2 = _col2im(spec, x, om, dcol)
    assert torch.equal(_bits(dom), _bits(dom2)), 'd_om is a fixed-order sum'
    assert R.excess(dx2, b.dx, f32, D.dx_extra(b)) <= 0           # (atomics: the order may vary, the bound holds)
    return dict(spec=spec, x=x, om=om, dcol=dcol, dx=dx, dom=dom)


@pytest.mark.parametrize('name', COL2IM)
def test_col2im_against_the_float64_adjoint(name):
    r = _check_col2im(name, CASES[name])
    if name.startswith('edge-'):
        _kept[('col2im', name)] = r


@pytest.mark.parametrize('name', ['edge-f32', 'edge-bf16', 'edge-f16'])
def test_col2im_refuses_the_mutated_references(name):
    """the domain closed at -1 / H, and the cell below an integer coordinate: both move d_om only, and out of the bound"""
    r = _kept.get(('col2im', name)) or _check_col2im(name, CASES[name])
    spec = r['spec']
    for m in (4, 5):
        wrong = D.adjoint64(r['x'], r['om'], r['dcol'], mutation=m, **D.conv_kw(spec))
        assert R.excess(r['dom'], wrong.dom, f32, D.dom_extra(wrong, spec['C'])) > 0, (name, m)
        assert R.excess(r['dx'], wrong.dx, f32, D.dx_extra(wrong)) <= 0


# ---- the fused kernel ----------------------------------------------------------------------------------------------------
def _half_ulp(v, dt):
    """half a unit in the last place of |v| in dt (normal range; fp16 subnormals share the smallest normal's ulp)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(1e-30)))
    if dt == torch.float16:
        e = e.clamp_min(-14)
    return torch.pow(2.0, e - {torch.bfloat16: 7, torch.float16: 10}[dt]) / 2


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('name', list(D.FUSED))
def test_fused_conv_against_the_float64_gemm_of_the_16bit_columns(name, dt):
    spec = D.fused_spec(name, dt)
    x, om, _ = D.make_inputs(spec, DEV)
    w, sc, sh, relu = D.fused_weights(spec, DEV)
    cout, cp = spec['cout'], spec['C']
    y = ops.deform_conv_nhwc(x, om, w, sc, sh, relu, spec['stride'], spec['pad'])
    M, _ = _dims(spec)
    assert y.dtype == dt and y.numel() == M * cout
    if name == 'm1350_11_tiles':
        assert (M + 127) // 128 == 11
    col = _im2col(dict(spec, Cpad=cp), x, om).double()
    w64 = w.double().view(cout, 9 * cp)
    ref = col @ w64.t()
    tol = 1e-5 * (col.abs() @ w64.abs().t())
    if sc is not None:
        ref, tol = ref * sc.double(), tol * sc.double()
    if sh is not None:
        ref = ref + sh.double()
    if relu:
        ref = ref.relu()
    got = y.view(M, cout).double()
    assert ref.abs().max().item() > 0.05            # (a case whose taps all miss the map would check nothing)
    bar = _half_ulp(ref.abs() + tol, dt) + tol
    e = ((got - ref).abs() - bar).max().item()
    print(f'fp64 leg fused {name} {D.SHORT[dt]} M={M}: largest error minus bound {e:.3e}')
    assert bool(torch.isfinite(got).all()) and e <= 0, (name, e)
    # one 16-bit step in one element is refused (the same bar, handed to one_ulp_off as its elementwise term)
    moved = R.one_ulp_off(y.view(M, cout), ref, bar - R.bound(ref, dt))
    assert ((moved.double() - ref).abs() - bar).max().item() > 0
    if spec['epilogue'] == 'none':
        # against float64 all the way: the columns' one rounding (half an ulp of each term) and the blend's fp32 error
        # over the magnitudes, the fp32 accumulation as above, the result's one rounding
        mag = D.im2col64(x, om, stride=spec['stride'], pad=spec['pad'], magnitude=True)
        full = D.im2col64(x, om, stride=spec['stride'], pad=spec['pad']) @ w64.t()
        extra = (R.half_ulp(dt) * 1.001 + D.COL_K * D.U + 1e-5) * (mag @ w64.abs().t())
        e2 = R.excess(y.view(M, cout), full, dt, extra)
        print(f'fp64 leg fused {name} {D.SHORT[dt]} against deform_ref64: largest error minus bound {e2:.3e}')
        assert e2 <= 0, (name, e2)


# ---- the 16-bit backward in stages, then the autograd functions ---------------------------------------------------------
BWD = [(64, 128, 11, 13, 1), (128, 64, 12, 17, 2)]


def _stages(dt, cp, cout, h, w, stride):
    spec = D._spec(cp, 2, h, w, dt, 150 + stride, stride=stride)
    x, om, _ = D.make_inputs(spec, DEV)
    M, _ = _dims(spec)
    g = torch.Generator().manual_seed(151)
    dy = torch.randn(M, cout, generator=g).to(dt).to(DEV)
    weight = (torch.randn(cout, cp, 3, 3, generator=g) / (9 * cp) ** 0.5).to(dt).float().to(DEV)       # parameter layout
    w_p = weight.permute(0, 2, 3, 1).to(dt).contiguous()
    return spec, x, om, dy, weight, w_p, M


def _wgrad(col, dy, M, cout, cp, x):
    dwp = torch.zeros((cout, 1, 1, 9 * cp), dtype=f32, device=DEV)
    one = _ints([1])
    st = lib.load().brcnn_conv2d_wgrad_nhwc_multi(col.data_ptr(), dy.data_ptr(), dwp.data_ptr(), M, 1, one, one, 9 * cp, cout,
                                                  1, 1, 1, 0, ops._dt(x), ops._conv_stream())
    assert st == 0
    return dwp


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('cp,cout,h,w,stride', BWD)
def test_16bit_backward_in_stages_and_through_the_function(dt, cp, cout, h, w, stride):
    spec, x, om, dy, weight, w_p, M = _stages(dt, cp, cout, h, w, stride)
    tag = f'{D.SHORT[dt]} Cp={cp} Cout={cout} s{stride}'
    # stage 1: dcol = dy16 . W16, an fp32 result
    dcol = ops.linear_nhwc(dy, w_p.view(cout, 9 * cp).t().contiguous(), out_f32=True)
    e1 = R.excess(dcol, dy.double() @ w_p.double().view(cout, 9 * cp), f32)
    # stage 2: the 16-bit col2im on that dcol
    dx32, dom = _col2im(spec, x, om, dcol)
    b = D.adjoint64(x, om, dcol, stride=stride)
    e2x, e2o = R.excess(dx32, b.dx, f32, D.dx_extra(b)), R.excess(dom, b.dom, f32, D.dom_extra(b, cp))
    # stage 3: dW from the 16-bit columns, elementwise
    col16 = _im2col(spec, x, om)
    dwp = _wgrad(col16, dy, M, cout, cp, x)
    e3 = R.excess(dwp.view(cout, 9 * cp), dy.double().t() @ col16.double(), f32)
    print(f'fp64 leg dcn backward {tag}: largest error minus bound  dcol {e1:.3e}  dx {e2x:.3e}  d_om {e2o:.3e}  dW {e3:.3e}')
    assert e1 <= 0 and e2x <= 0 and e2o <= 0 and e3 <= 0
    dw_staged = dwp.view(cout, 3, 3, cp).permute(0, 3, 1, 2)
    go = dy.view(spec['N'], -1, om.shape[2], cout)
    for need in ((True, True, True), (True, False, False), (False, True, False), (False, False, True)):
        xg, og, wg = (t.clone().requires_grad_(n) for t, n in zip((x, om, weight), need))
        y = deform_conv_autograd(xg, og, wg, stride, 1)
        y.backward(go)
        for t, n in zip((xg, og, wg), need):
            assert (t.grad is not None) == n, need
        if need[0]:
            assert xg.grad.dtype == dt
            ex = R.excess(xg.grad, b.dx, dt, D.dx_extra(b))
            print(f'fp64 leg DeformConvFunction {tag} needs={need}: dx largest error minus bound {ex:.3e}')
            assert ex <= 0, (need, ex)
        if need[1]:
            assert torch.equal(_bits(og.grad), _bits(dom)), need
        if need[2]:
            assert torch.equal(_bits(wg.grad), _bits(dw_staged)), need


@pytest.mark.parametrize('c,h,w,stride', [(32, 11, 13, 1), (64, 12, 17, 2)])
def test_deform_im2col_function_fp32(c, h, w, stride):
    spec = D._spec(c, 2, h, w, f32, 160 + stride, stride=stride)
    x, om, dcol = D.make_inputs(spec, DEV)
    dx_s, dom_s = _col2im(spec, x, om, dcol)
    b = D.adjoint64(x, om, dcol, stride=stride)
    ref, mag = _ref_cols(spec, x, om)
    for need in ((True, True), (True, False), (False, True)):
        xg, og = x.clone().requires_grad_(need[0]), om.clone().requires_grad_(need[1])
        col = deform_im2col_autograd(xg, og, stride, 1)
        assert R.excess(col.detach(), ref, f32, D.col_extra(mag)) <= 0
        col.backward(dcol)
        assert (xg.grad is not None) == need[0] and (og.grad is not None) == need[1]
        if need[0]:
            ex = R.excess(xg.grad, b.dx, f32, D.dx_extra(b))
            print(f'fp64 leg DeformIm2colFunction C={c} s{stride} needs={need}: dx largest error minus bound {ex:.3e}')
            assert ex <= 0
        if need[1]:
            assert torch.equal(_bits(og.grad), _bits(dom_s))


def test_deform_entries_refuse_maps_smaller_than_the_kernel():
    """a padded map the kernel extent does not fit has no output; C's truncating division used to give it one row at
    stride 2 ((2 - 3) / 2 + 1 = 1), which the entries then wrote"""
    L, s = lib.load(), ops._stream()
    bf = torch.bfloat16
    x = torch.zeros(1, 2, 2, 64, device=DEV)
    xb = x.to(bf)
    om = torch.zeros(64, 27, device=DEV)
    col, colb = torch.full((64, 9 * 64), 3.0, device=DEV), torch.full((64, 9 * 64), 3.0, dtype=bf, device=DEV)
    dcol, dx, dom = torch.zeros(64, 9 * 64, device=DEV), torch.zeros(1, 2, 2, 64, device=DEV), torch.full((64, 27), 3.0, device=DEV)
    w, y = torch.zeros(64, 3, 3, 64, dtype=bf, device=DEV), torch.full((64, 64), 3.0, dtype=bf, device=DEV)
    P = lambda t: t.data_ptr()          # noqa: E731
    for (h, wd) in ((2, 2), (1, 2), (2, 1)):
        g = (1, h, wd, 64, 3, 3, 2, 0, 1, 27, 64)
        assert L.brcnn_deform_im2col_nhwc(P(x), P(om), P(col), *g, s) == EINVAL
        assert L.brcnn_deform_im2col_nhwc_ex(P(xb), P(om), P(colb), *g, ops.DT_BF16, s) == EINVAL
        assert L.brcnn_deform_col2im_nhwc(P(x), P(om), P(dcol), P(dx), P(dom), *g, s) == EINVAL
        assert L.brcnn_deform_col2im_nhwc_ex(P(xb), P(om), P(dcol), P(dx), P(dom), *g, ops.DT_BF16, s) == EINVAL
        assert L.brcnn_deform_conv_nhwc(P(xb), P(om), P(w), None, None, P(y), 1, h, wd, 64, 64, 2, 0, 0, 27, ops.DT_BF16, s) == EINVAL
    torch.cuda.synchronize()
    assert bool((col == 3).all()) and bool((colb == 3).all()) and bool((dom == 3).all()) and bool((y == 3).all())
    # (the smallest map that does fit still runs)
    assert L.brcnn_deform_im2col_nhwc(P(x), P(om), P(col), 1, 2, 2, 64, 3, 3, 2, 1, 1, 27, 64, s) == 0


# ---- the average pools --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', D.DTYPES, ids=list(D.SHORT.values()))
def test_avgpool_every_window_rule_against_float64(dt):
    """k x s x pad x ceil_mode x count_include_pad on maps from 1 x 9 to 9 x 1: the output shape (ceil_mode: the last window
    must start inside the input), the divisor, and maps smaller than the window.  The inputs are multiples of 1/8 below 4
    in magnitude: every window sum is exact in fp32, so the fp32 mean is one division away from float64 (within 4 u of the
    result) and the 16-bit mean is that fp32 mean rounded once, bit for bit.  What torch refuses, the entry refuses
    without a launch"""
    L, s = lib.load(), ops._stream()
    gen = torch.Generator().manual_seed(31)
    worst, refused, ran = 0.0, 0, 0
    for H in range(1, 10):
        W = 10 - H
        x = (torch.randint(-31, 32, (2, H, W, 8), generator=gen).float() / 8).to(dt).to(DEV)
        xn = x.double().permute(0, 3, 1, 2)
        for k in (2, 3):
            for st in (1, 2):
                for pad in (0, 1):
                    for ceil in (False, True):
                        for cip in (False, True):
                            what = (H, W, k, st, pad, ceil, cip)
                            y = torch.full((2, H + 2, W + 2, 8), 5.0, dtype=dt, device=DEV)       # room for any output
                            try:
                                ref = F.avg_pool2d(xn, k, st, pad, ceil_mode=ceil, count_include_pad=cip)
                            except RuntimeError:
                                ref = None
                            rc = L.brcnn_avgpool_nhwc_ex(x.data_ptr(), y.data_ptr(), 2, H, W, 8, k, st, pad, int(ceil),
                                                         int(cip), ops._dt(x), s)
                            if ref is None:
                                refused += 1
                                assert rc == EINVAL, what
                                assert bool((y == 5).all()), what
                                if dt == f32:
                                    assert L.brcnn_avgpool_nhwc(x.data_ptr(), y.data_ptr(), 2, H, W, 8, k, st, pad, int(ceil),
                                                                int(cip), s) == EINVAL, what
                                continue
                            ran += 1
                            assert rc == 0, what
                            ho, wo = ref.shape[2], ref.shape[3]
                            assert (ho, wo) == (ops.avgpool_out_size(H, k, st, pad, ceil), ops.avgpool_out_size(W, k, st, pad, ceil))
                            got = y.view(-1)[:2 * ho * wo * 8].view(2, ho, wo, 8)
                            assert bool((y.view(-1)[2 * ho * wo * 8:] == 5).all()), what         # nothing past the output
                            refn = ref.permute(0, 2, 3, 1)
                            if dt == f32:
                                rel = ((got.double() - refn).abs() / refn.abs().clamp_min(1e-300)).max().item() / D.U
                                worst = max(worst, rel)
                                assert bool((got.double() - refn).abs().le(4 * D.U * refn.abs()).all()), (what, rel)
                            else:
                                assert torch.equal(_bits(got), _bits(refn.float().to(dt))), what
                            assert torch.equal(_bits(ops.avgpool_nhwc(x, k, st, pad, ceil, cip)), _bits(got)), what
    print(f'avgpool {D.SHORT[dt]}: {ran} combinations ran, {refused} refused like torch' +
          (f', largest error {worst:.2f} u of the result' if dt == f32 else ''))
    assert refused > 0 and ran > 200
