"""No device: the float64 GroupNorm reference of tests/test_groupnorm_gpu.py (tests/gn_ref64.py) against F.group_norm in
float64 with autograd, the sharpness of every bound it defines, what torch's fp32 group norm itself costs on the conditioning
inputs (the oracle ratios recorded in the module), and the share of every ReLU case inside the mask-agreement band."""
import pytest
import torch
import torch.nn.functional as F

from tests import gn_ref64 as G
from tests import route_util as R


def _nchw(t, batch, hw, C):
    return t.view(batch, hw, C).permute(0, 2, 1).reshape(batch, C, hw, 1)


def _rows(t, batch, hw, C):
    return t.reshape(batch, C, hw).permute(0, 2, 1).reshape(batch * hw, C)


def _torch_group_norm(x, dy, gm, bt, groups, batch, sizes, eps, relu, dtype):
    """F.group_norm per segment in `dtype` with autograd -> y, dx (rows, C), dgamma, dbeta"""
    C = x.shape[1]
    g_, b_ = gm.to(dtype).requires_grad_(True), bt.to(dtype).requires_grad_(True)
    ys, dxs = [], []
    for s, r0, hw in G._segments(batch, sizes):
        xs = _nchw(x[r0:r0 + batch * hw].to(dtype), batch, hw, C).clone().requires_grad_(True)
        y = F.group_norm(xs, groups, g_, b_, eps)
        y = y.relu() if relu else y
        y.backward(_nchw(dy[r0:r0 + batch * hw].to(dtype), batch, hw, C))
        ys.append(_rows(y.detach(), batch, hw, C))
        dxs.append(_rows(xs.grad, batch, hw, C))
    return torch.cat(ys), torch.cat(dxs), g_.grad, b_.grad


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('cpg', [1, 2, 3, 4, 7, 8])
def test_reference_equals_float64_group_norm(cpg, relu):
    """forward and all three gradients, per segment, three segments (one of 1 x 1), one constant group among four"""
    C, groups, batch, sizes = 4 * cpg, 4, 3, ((5, 3), (2, 2), (1, 1))
    x, dy, gm, bt = G.make_case(C, groups, batch, sizes, torch.float32, 5 + cpg, constant_groups=(2,))
    f = G.gn_forward64(x, gm, bt, groups, batch, sizes, 1e-5, relu)
    b = G.gn_backward64(dy, f, gm, f.pre > 0 if relu else torch.ones_like(f.pre, dtype=torch.bool))
    y, dx, dg, db = _torch_group_norm(x, dy, gm, bt, groups, batch, sizes, 1e-5, relu, torch.float64)
    for name, got, want in (('y', f.y, y), ('dx', b.dx, dx), ('dgamma', b.dgamma, dg), ('dbeta', b.dbeta, db)):
        err = (got - want).abs().max().item()
        assert err <= 1e-10 * max(1.0, want.abs().max().item()), (name, err)
    assert f.mean.shape == f.var.shape == f.kappa.shape == (3, batch, groups) and bool(torch.isfinite(f.kappa).all())
    cg = slice(2 * cpg, 3 * cpg)
    assert bool((f.var[:, :, 2] == 0).all()) and bool((f.pre[:, cg] == bt.double()[cg]).all())
    assert abs(f.kappa[0, 0, 2].item() - 1.5 ** 2 / 1e-5) <= 1e-6 * 1.5 ** 2 / 1e-5


def _all_bounds(spec, relu):
    """(name, float64 reference, result dtype, extra) of every quantity the GPU file bounds"""
    x, dy, gm, bt = G.case_inputs(spec)
    f = G.gn_forward64(x, gm, bt, spec['G'], spec['batch'], spec['sizes'], spec['eps'], relu)
    b = G.gn_backward64(dy, f, gm, f.pre > 0 if relu else torch.ones_like(f.pre, dtype=torch.bool))
    K = G.param_chain(spec['batch'], spec['sizes'], spec['dtype'], spec['C'])
    dt = spec['dtype']
    return [('y', f.y, dt, G.y_extra(f, gm, bt)), ('dx', b.dx, dt, G.dx_extra(f, b, K)),
            ('dgamma', b.dgamma, torch.float32, G.dgamma_extra(f, b, K)), ('dbeta', b.dbeta, torch.float32, G.dbeta_extra(b, K))]


SHARP = ['rows_c256_g32', 'rows_c64_g32', 'flat_c12_g4', 'flat_c252_g36']


@pytest.mark.parametrize('route', SHARP + ['kappa_1e2', 'kappa_1e4', 'constant_one'])
def test_every_fp32_bound_refuses_twice_the_bound(route):
    spec = G.cases()[route + '-f32']
    for name, ref, dt, extra in _all_bounds(spec, spec['relus'][-1]):
        got = ref.float()
        assert R.excess(got, ref, torch.float32, extra) <= 0, name
        assert R.excess(R.twice_the_bound_off(got, ref, extra), ref, torch.float32, extra) > 0, name
    x, _, gm, bt = G.case_inputs(spec)
    f = G.gn_forward64(x, gm, bt, spec['G'], spec['batch'], spec['sizes'], spec['eps'], False)
    for name, ref, bnd in (('mean', f.mean, G.mean_bound(f)), ('rstd', f.rstd, G.rstd_bound(f))):
        i = bnd.view(-1).argmax()
        moved = ref.clone()
        moved.view(-1)[i] += 2 * bnd.view(-1)[i]
        assert bool(((moved - ref).abs() <= bnd).sum() == ref.numel() - 1), name


@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('route', SHARP)
def test_every_16_bit_bound_refuses_one_representable_step(route, dtype):
    """y and dx are the 16-bit results; dgamma / dbeta stay fp32 (the fp32 leg above)"""
    spec = G.cases()[f'{route}-{dtype}']
    for name, ref, dt, extra in _all_bounds(spec, True)[:2]:
        got = ref.to(dt)
        assert R.excess(got, ref, dt, extra) <= 0, name
        assert R.excess(R.one_ulp_off(got, ref, extra), ref, dt, extra) > 0, name


def test_wrong_count_reference_is_refused():
    """the classic slip, D + 1 for D: a float64 result computed that way lies outside the fp32 bound on every route shape"""
    for route in SHARP:
        spec = G.cases()[route + '-f32']
        x, _, gm, bt = G.case_inputs(spec)
        a = (x, gm, bt, spec['G'], spec['batch'], spec['sizes'], spec['eps'], False)
        f, wrong = G.gn_forward64(*a), G.gn_forward64(*a, count_slip=1)
        assert R.excess(wrong.y, f.y, torch.float32, G.y_extra(f, gm, bt)) > 0, route


def test_oracle_ratios_recorded_in_the_module_are_reproduced():
    """torch's fp32 F.group_norm (the arithmetic of oracle/cpu_pipeline.py) against the float64 reference on the three
    conditioning cases: it stays below the ceilings gn_ref64 records next to the derived constants, and far below the
    derived bound itself"""
    for i, name in enumerate(('kappa_1-f32', 'kappa_1e2-f32', 'kappa_1e4-f32')):
        spec = G.cases()[name]
        x, dy, gm, bt = G.case_inputs(spec)
        batch, sizes = spec['batch'], spec['sizes']
        f = G.gn_forward64(x, gm, bt, spec['G'], batch, sizes, spec['eps'], False)
        b = G.gn_backward64(dy, f, gm, torch.ones_like(f.pre, dtype=torch.bool))
        K = G.param_chain(batch, sizes, torch.float32, spec['C'])
        y, dx, dg, db = _torch_group_norm(x, dy, gm, bt, spec['G'], batch, sizes, spec['eps'], False, torch.float32)
        err = (y.double() - f.y).abs()
        rel = err.max().item() / max(1.0, f.y.abs().max().item())
        unit = G.U * (f.kappa_e * (f.pre - bt.double()).abs() + f.kappa_e.sqrt() * gm.double().abs())
        cond = (err / unit).max().item()
        r_dx = ((dx.double() - b.dx).abs() / G.dx_extra(f, b, K)).max().item()
        r_dg = ((dg.double() - b.dgamma).abs() / G.dgamma_extra(f, b, K)).max().item()
        r_db = ((db.double() - b.dbeta).abs() / (G.U * b.S_beta)).max().item()
        print(f'{name}: kappa {f.kappa.min().item():.4g} .. {f.kappa.max().item():.4g}  fp32 oracle / float64: y rel {rel:.2e} '
              f'y / conditioning unit {cond:.2f}  dx / dx_extra {r_dx:.3f}  dgamma / dgamma_extra {r_dg:.3f}  '
              f'dbeta / (u S_beta) {r_db:.2f}')
        assert rel <= G.ORACLE_Y_REL[i] and cond <= G.ORACLE_Y_COND[i]
        assert r_dx <= G.ORACLE_DX_OVER_EXTRA and r_dg <= G.ORACLE_DGAMMA_OVER_EXTRA and r_db <= G.ORACLE_DBETA
        assert R.excess(y, f.y, torch.float32, G.y_extra(f, gm, bt)) <= 0
        assert cond < G.K_MEAN          # the derived constants are worst cases: the oracle needs a fraction of them


def test_mask_band_share_of_every_relu_case_stays_under_its_cap():
    """from float64 alone: the elements whose pre-activation lies within the forward bound of 0 -- where the kernel's
    y > 0 may legitimately differ from pre64 > 0 -- are at most MASK_BAND_CAP of each ReLU case of the GPU file"""
    worst = ('', 0.0)
    for name, spec in G.cases().items():
        if True not in spec['relus']:
            continue
        x, _, gm, bt = G.case_inputs(spec)
        f = G.gn_forward64(x, gm, bt, spec['G'], spec['batch'], spec['sizes'], spec['eps'], True)
        share = G.mask_band_share(f, spec['dtype'], gm, bt)
        worst = max(worst, (name, share), key=lambda t: t[1])
        assert share <= G.MASK_BAND_CAP, (name, share)
    print(f'largest share inside the mask band: {worst[1]:.2e} ({worst[0]})')


def test_row_counts_reach_the_chunking_edges():
    """what the GPU file's row counts are chosen for, from the host's two chunking rules: rows per workgroup above 256 past
    the backward's 64 and the forward's 512 chunks, a second fp32 partial per row lane (more than 32 rows per lane and
    chunk) on both statistics variants, maps below the row lanes, both sides of the 128-row strips of the apply kernels"""
    assert G.bwd_chunks(16385) == (64, 257) and G.fwd_chunks(16385)[1] <= 256
    assert G.fwd_chunks(131073)[1] == 257 and G.fwd_chunks(131073)[0] <= 512 and G.bwd_chunks(131073)[1] > 2048
    assert G.fwd_chunks(256)[1] > 32 * G.row_lanes(torch.float32, 8)            # fp32, V = 4: four row lanes
    assert G.fwd_chunks(131073)[1] > 32 * G.row_lanes(torch.bfloat16, 8)        # 16-bit, V = 8: eight row lanes
    assert {1, 3, 7, 128, 129, 256, 257} <= set(G.ROW_COUNTS) and min(G.ROW_COUNTS) < G.row_lanes(torch.float32, 8)
    assert G.param_chain(1, ((131073, 1),), torch.float32, 8) > G.param_chain(2, ((1050, 1),), torch.float32, 8)
