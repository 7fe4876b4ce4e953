"""The GroupNorm kernels of csrc/misc.hip against the float64 reference of tests/gn_ref64.py: every route (row-strip:
C % 8 == 0; flat: C % 8 == 4, with and without channel quads that straddle two groups), every chunking rule (rows per
workgroup above 256 past the backward's 64 and the forward's 512 chunks, a second fp32 partial per row lane), maps
smaller than the row lanes, batches of hundreds of 7 x 7 maps, segments in any order, ill-conditioned and constant
groups, zero / negative gamma, all-clipped ReLU -- forward, returned statistics, ReLU mask and backward, fp32 / bf16 /
fp16.  The inputs are rounded to the dtype first: the reference sees the kernel's operands.  Nothing here is compared
with another launch of the same kernels.

y and dx depend on double atomics whose order may vary between launches (the group sums), so they are held to the bound
only; dgamma and dbeta are fixed-order sums and must repeat bit for bit."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import brcnn  # noqa: F401
from brcnn import lib as L
from brcnn import ops
from tests import gn_ref64 as G
from tests import route_util as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = G.cases()
LEGS = [(name, relu) for name, spec in CASES.items() for relu in spec['relus']]
SHARP = ['rows_c256_g32', 'rows_c64_g32', 'flat_c12_g4', 'flat_c252_g36']
_kept = {}          # (name, relu) -> results of the sharpness legs' cases: no kernel is rerun for them


def _stats_pairs(stats, L_, batch, groups):
    """the (mean, rstd) fp32 pairs in the first 8 bytes of every 16-byte entry -> two (L, N, G) float64"""
    v = stats.view(torch.float32).view(-1, 4)
    return v[:, 0].double().view(L_, batch, groups), v[:, 1].double().view(L_, batch, groups)


def _run(name, relu):
    """kernels and reference of one leg; asserts nothing"""
    spec = CASES[name]
    x, dy, gm, bt = G.case_inputs(spec, DEV)
    groups, batch, sizes, eps = spec['G'], spec['batch'], spec['sizes'], spec['eps']
    y, stats = ops.groupnorm_nhwc_multi(x, gm, bt, groups, batch, sizes, eps, relu, return_stats=True)
    dx, dg, db = ops.groupnorm_nhwc_multi_backward(dy, x, stats, gm, bt, groups, batch, sizes, relu)
    f = G.gn_forward64(x, gm, bt, groups, batch, sizes, eps, relu)
    mask = y > 0 if relu else torch.ones_like(y, dtype=torch.bool)
    b = G.gn_backward64(dy, f, gm, mask)            # the mask the FORWARD stored: the backward recomputes it from x
    K = G.param_chain(batch, sizes, spec['dtype'], spec['C'])
    return dict(spec=spec, x=x, dy=dy, gm=gm, bt=bt, y=y, stats=stats, dx=dx, dg=dg, db=db, f=f, b=b, K=K, mask=mask)


@pytest.mark.parametrize('name,relu', LEGS, ids=[f'{n}-{"relu" if r else "plain"}' for n, r in LEGS])
def test_forward_statistics_mask_and_backward_against_float64(name, relu):
    r = _run(name, relu)
    if name.rsplit('-', 1)[0] in SHARP and relu:
        _kept[(name, relu)] = r
    spec, f, b, K, gm, bt = r['spec'], r['f'], r['b'], r['K'], r['gm'], r['bt']
    dt = spec['dtype']
    assert all(bool(torch.isfinite(r[k]).all()) for k in ('y', 'dx', 'dg', 'db'))
    mean, rstd = _stats_pairs(r['stats'], len(spec['sizes']), spec['batch'], spec['G'])
    e = {'y': R.excess(r['y'], f.y, dt, G.y_extra(f, gm, bt)),
         'mean': ((mean - f.mean).abs() - G.mean_bound(f)).max().item(),
         'rstd': ((rstd - f.rstd).abs() - G.rstd_bound(f)).max().item(),
         'dx': R.excess(r['dx'], b.dx, dt, G.dx_extra(f, b, K)),
         'dgamma': R.excess(r['dg'], b.dgamma, torch.float32, G.dgamma_extra(f, b, K)),
         'dbeta': R.excess(r['db'], b.dbeta, torch.float32, G.dbeta_extra(b, K))}
    # how much of the conditioning term the kernel spends (figures only: nothing is sized by them)
    unit = G.U * (f.kappa_e * (f.pre - bt.double()).abs() + f.kappa_e.sqrt() * gm.double().abs())
    cond = ((r['y'].double() - f.y).abs() / unit.clamp_min(1e-300)).max().item() if dt == torch.float32 else float('nan')
    rel = (r['y'].double() - f.y).abs().max().item() / max(1.0, f.y.abs().max().item())
    print(f'fp64 leg gn {name} relu={int(relu)} K={K} kappa<={f.kappa.max().item():.3g}: largest error minus bound  ' +
          '  '.join(f'{k} {v:.3e}' for k, v in e.items()) + f'  | y error / max {rel:.2e}, / conditioning unit {cond:.2f}')
    for k, v in e.items():
        assert v <= 0, (name, relu, k, v)
    if relu:
        band = R.bound(f.pre, dt, G.y_extra(f, gm, bt))
        outside = f.pre.abs() > band
        assert bool(((r['y'] > 0) == (f.pre > 0))[outside].all()), 'ReLU mask differs from float64 outside the band'
        assert 1.0 - outside.double().mean().item() <= G.MASK_BAND_CAP
    kw = spec['kw']
    if kw.get('beta') == -10.0:         # everything clipped: exact zeros, not small numbers
        assert not bool(r['y'].any()) and not bool(r['dx'].any()) and not bool(r['dg'].any()) and not bool(r['db'].any())
    if kw.get('beta') == 10.0:
        assert bool((r['y'] > 0).all())
    for k in kw.get('constant_groups', ()):         # y = beta within the bound was asserted above; spell the case out
        cpg = spec['C'] // spec['G']
        assert (f.pre[:, k * cpg:(k + 1) * cpg] - bt.double()[k * cpg:(k + 1) * cpg]).abs().max().item() <= 1e-9    # (float64)
        assert abs(f.rstd[0, 0, k].item() - spec['eps'] ** -0.5) <= 1e-9 * spec['eps'] ** -0.5


@pytest.mark.parametrize('route', SHARP)
@pytest.mark.parametrize('dtype', ['f32', 'bf16', 'f16'])
def test_the_bounds_refuse_a_moved_result_and_a_wrong_count(route, dtype):
    """on the host, from the results the fp64 leg kept: the kernel's own y and dx moved by twice the bound (fp32) or one
    representable step (16-bit) are refused, and so is a float64 reference computed with D + 1 for D"""
    key = (f'{route}-{dtype}', True)
    r = _kept.get(key) or _run(*key)        # (kept by the leg above when the file runs in order)
    spec, f, b, gm, bt = r['spec'], r['f'], r['b'], r['gm'], r['bt']
    dt = spec['dtype']
    for got, ref, extra in ((r['y'], f.y, G.y_extra(f, gm, bt)), (r['dx'], b.dx, G.dx_extra(f, b, r['K']))):
        moved = R.twice_the_bound_off(got, ref, extra) if dt == torch.float32 else R.one_ulp_off(got, ref, extra)
        assert R.excess(got, ref, dt, extra) <= 0 < R.excess(moved, ref, dt, extra)
    wrong = G.gn_forward64(r['x'], gm, bt, spec['G'], spec['batch'], spec['sizes'], spec['eps'], True, count_slip=1)
    assert R.excess(r['y'], wrong.y, dt, G.y_extra(wrong, gm, bt)) > 0


@pytest.mark.parametrize('name', ['hw1050-f32', 'hw16385-bf16', 'pyramid-f32', 'flat_c36_g9-f16'])
def test_dgamma_and_dbeta_repeat_bit_for_bit(name):
    """fixed-order sums (partials per workgroup, 32 slices, one final pass); dx and y go through double atomics whose
    order may vary and are held to the bound only (the fp64 legs)"""
    spec = CASES[name]
    x, dy, gm, bt = G.case_inputs(spec, DEV)
    a = (spec['G'], spec['batch'], spec['sizes'])
    _, stats = ops.groupnorm_nhwc_multi(x, gm, bt, *a, spec['eps'], True, return_stats=True)
    one = ops.groupnorm_nhwc_multi_backward(dy, x, stats, gm, bt, *a, True)
    two = ops.groupnorm_nhwc_multi_backward(dy, x, stats, gm, bt, *a, True)
    assert torch.equal(one[1], two[1]) and torch.equal(one[2], two[2])


@pytest.mark.parametrize('dtype', G.DTYPES)
@pytest.mark.parametrize('C,groups', [(260, 4), (6, 3), (8, 3)])
def test_unsupported_channel_counts_are_errors_that_write_nothing(C, groups, dtype):
    """more than 256 channels, no whole channel quads, C % G != 0: BRCNN_EINVAL from forward and backward, outputs untouched"""
    lib = L.load()
    rows, hw = 2 * 6, (ctypes.c_int * 1)(6)
    x = torch.randn(rows, C, device=DEV).to(dtype)
    gm, bt = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    y, dx = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    dg, db = torch.full((C,), 7.0, device=DEV), torch.full((C,), 7.0, device=DEV)
    stats = torch.full((2 * groups * 2,), 7.0, dtype=torch.float64, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.float64, device=DEV)
    p = lambda t: t.data_ptr()      # noqa: E731
    st = lib.brcnn_groupnorm_nhwc_multi(p(x), p(gm), p(bt), p(y), p(stats), 2, 1, hw, C, groups, 1e-5, 1, ops._dt(x),
                                        ops._stream())
    assert st == -22
    st = lib.brcnn_groupnorm_nhwc_multi_backward(p(x), p(x), p(stats), p(gm), p(bt), p(dx), p(dg), p(db), p(ws),
                                                 ws.numel() * 8, 2, 1, hw, C, groups, 1, ops._dt(x), ops._stream())
    assert st == -22
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (y, dx, dg, db, stats))
    with pytest.raises(L.BrcnnHipError):
        ops.groupnorm_nhwc_multi(x, gm, bt, groups, 2, ((6, 1),), 1e-5, True)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16, torch.float32])
def test_autograd_function_on_the_flat_route(dtype):
    """GroupNormNHWCFunction with C % 8 == 4: a 16-bit layer of 36 channels used to run its forward and raise in
    backward().  Its gradients are those of the direct calls (dgamma / dbeta bit for bit) and lie within the bound"""
    from brcnn.autograd import GroupNormNHWCFunction
    spec = CASES['flat_c36_g9-' + G._SHORT[dtype]]
    x, dy, gm, bt = G.case_inputs(spec, DEV)
    a = (spec['G'], spec['batch'], spec['sizes'])
    xr, gr, br = x.clone().requires_grad_(True), gm.clone().requires_grad_(True), bt.clone().requires_grad_(True)
    y = GroupNormNHWCFunction.apply(xr, gr, br, *a, spec['eps'], True)
    y.backward(dy)
    y0, stats = ops.groupnorm_nhwc_multi(x, gm, bt, *a, spec['eps'], True, return_stats=True)
    dx0, dg0, db0 = ops.groupnorm_nhwc_multi_backward(dy, x, stats, gm, bt, *a, True)
    assert torch.equal(gr.grad, dg0) and torch.equal(br.grad, db0) and xr.grad.dtype == dtype
    f = G.gn_forward64(x, gm, bt, *a, spec['eps'], True)
    b = G.gn_backward64(dy, f, gm, y > 0)
    K = G.param_chain(spec['batch'], spec['sizes'], dtype, spec['C'])
    assert R.excess(y.detach(), f.y, dtype, G.y_extra(f, gm, bt)) <= 0
    assert R.excess(xr.grad, b.dx, dtype, G.dx_extra(f, b, K)) <= 0


def _conv_module(cin, cout, groups, act):
    from brcnn.blocks import ConvModule
    torch.manual_seed(3)
    m = ConvModule(cin, cout, 1, norm_cfg=dict(type='GN', num_groups=groups, requires_grad=True),
                   act_cfg=dict(type='ReLU') if act else None).to(DEV)
    with torch.no_grad():
        m.norm.weight.copy_(1.0 + 0.25 * torch.randn(cout))
        m.norm.bias.copy_(0.3 * torch.randn(cout))
    return m


@pytest.mark.parametrize('act', [True, False], ids=['relu', 'plain'])
@pytest.mark.parametrize('cout,groups', [(512, 32), (6, 3), (36, 9)])
def test_conv_module_group_norm_in_eval_and_training(cout, groups, act):
    """ConvModule.forward_nhwc with a GroupNorm wider than the kernels' 256 channels, or without whole channel quads
    (both: torch's group norm, in training AND at inference -- the eval route used to raise), and with 36 channels (the
    kernels' flat route), against F.group_norm in float64 on the float64 convolution.  Bound: the suite's conv bound E =
    ACC_TOL max(1, |conv|max) moves xh by at most 2 rstd E (the value and its group's mean), hence y by 2 rstd |gamma| E, on
    top of the suite's own bound on y.  Gradients of gamma / beta (without ReLU: a mask flipped by the conv's round-off
    would move a sum by a whole term): sum |g| 2 rstd E, + ACC_TOL of the sums of magnitudes"""
    m = _conv_module(64, cout, groups, act)
    g = torch.Generator().manual_seed(cout)
    x = torch.randn(2, 9, 7, 64, generator=g).to(DEV)
    dy = torch.randn(2, 9, 7, cout, generator=g).to(DEV)
    conv = F.conv2d(x.double().permute(0, 3, 1, 2), m.conv.weight.detach().double())
    gm, bt = m.norm.weight.detach().double().requires_grad_(True), m.norm.bias.detach().double().requires_grad_(True)
    ref = F.group_norm(conv, groups, gm, bt, m.norm.eps)
    ref = (ref.relu() if act else ref).permute(0, 2, 3, 1)
    E = R.ACC_TOL * max(1.0, conv.abs().max().item())
    var = conv.view(2, groups, -1).var(2, unbiased=False)
    rstd = ((var + m.norm.eps) ** -0.5).max().item()
    extra = 2 * rstd * E * gm.detach().abs()
    m.eval()
    with torch.no_grad():
        y_eval = m.forward_nhwc(x)
    m.train()
    y_train = m.forward_nhwc(x)
    for what, y in (('eval', y_eval), ('training', y_train)):
        e = R.excess(y.detach(), ref.detach(), torch.float32, extra)
        print(f'ConvModule GN C={cout} {what}: largest error minus bound {e:.3e}')
        assert e <= 0, (what, e)
    y_train.backward(dy)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    if not act:
        ref.backward(dy.double())
        xh = ((ref.detach() - bt.detach()) / gm.detach())
        S_beta, S_gamma = dy.double().abs().sum((0, 1, 2)), (dy.double() * xh).abs().sum((0, 1, 2))
        assert R.excess(m.norm.bias.grad, bt.grad, torch.float32, R.ACC_TOL * S_beta) <= 0
        assert R.excess(m.norm.weight.grad, gm.grad, torch.float32, R.ACC_TOL * S_gamma + 2 * rstd * E * S_beta) <= 0


def test_bf16_conv_module_with_36_channel_group_norm_trains_one_step():
    """16-bit activations, C % 8 == 4: forward and backward on the kernels (no torch fall-back: C <= 256, C % 4 == 0), one
    SGD step, finite everywhere"""
    m = _conv_module(64, 36, 9, True)
    opt = torch.optim.SGD(m.parameters(), lr=0.01)
    x = torch.randn(2, 9, 7, 64, device=DEV).to(torch.bfloat16).requires_grad_(True)
    before = m.norm.weight.detach().clone()
    y = m.forward_nhwc(x)
    assert y.dtype == torch.bfloat16 and y.shape == (2, 9, 7, 36)
    y.float().pow(2).sum().backward()
    opt.step()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    assert bool(torch.isfinite(x.grad).all()) and not torch.equal(before, m.norm.weight.detach())
