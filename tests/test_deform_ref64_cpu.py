"""tests/deform_ref64.py checked without a device: the float64 reference of the modulated deformable im2col and its
adjoint against oracles that share nothing with its corner logic (an affine field, hand-derived vectors, F.conv2d), the
inputs (dyadic offsets whose fp32 coordinate is exact, the edge table), the mutated references (each distinguishable at
ten times the bound), the pile case and the fp32-restatement figures the module's docstring records."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import deform_ref64 as D
from tests import route_util as R

CASES = D.cases()
f64 = torch.float64


def _affine(H, W, C, gen):
    """x[n, h, w, c] = a_c h + b_c w + c0_c with dyadic coefficients: every float64 blend of it is exact"""
    a, b, c0 = (torch.round(torch.randn(C, generator=gen, dtype=f64) * 8) / 8 for _ in range(3))
    hh, ww = torch.arange(H, dtype=f64).view(H, 1, 1), torch.arange(W, dtype=f64).view(1, W, 1)
    return (a * hh + b * ww + c0).unsqueeze(0), a, b, c0


@pytest.mark.parametrize('kind', ['random', 'edge'])
def test_affine_field_value_and_offset_gradient(kind):
    """bilinear sampling reproduces an affine field: inside [0, H-1] x [0, W-1] the column is s f(h, w) and d off_h is
    s sum_c dcol_c a_c; in the strips -1 < h < 0 and H-1 < h < H (w inside) it is (1 + h) f(0, w) and (H - h) f(H-1, w)"""
    spec = D._spec(4, 1, 6, 7, f64, 7, kind=kind)
    _, om, dcol = D.make_inputs(spec)
    H, W, C = 6, 7, 4
    x, a, b, c0 = _affine(H, W, C, torch.Generator().manual_seed(1))
    dcol = dcol.double()
    col = D.im2col64(x, om).view(-1, 9, C)
    adj = D.adjoint64(x, om, dcol)
    g = D.geometry(om.double(), 1, H, W, 3, 3, 1, 1, 1)
    h, w, s = (t.reshape(-1, 9) for t in (g.h, g.w, g.s))
    f = lambda hh, ww: a * hh.unsqueeze(-1) + b * ww.unsqueeze(-1) + c0          # noqa: E731
    w_in = (w >= 0) & (w <= W - 1)
    inner = (h >= 0) & (h <= H - 1) & w_in
    top, bottom = (h > -1) & (h < 0) & w_in, (h > H - 1) & (h < H) & w_in
    assert int(inner.sum()) > 50 and int(top.sum()) > 3 and int(bottom.sum()) > 3
    scale = col.abs().max().item()
    for where, expect in ((inner, f(h, w)), (top, (1 + h).unsqueeze(-1) * f(torch.zeros_like(h), w)),
                          (bottom, (H - h).unsqueeze(-1) * f(torch.full_like(h, H - 1.0), w))):
        err = ((col - s.unsqueeze(-1) * expect).abs() * where.unsqueeze(-1)).max().item()
        assert err <= 1e-12 * scale, err
    d = dcol.view(-1, 9, C)
    dh, dw = adj.dom[..., 0:18:2].reshape(-1, 9), adj.dom[..., 1:18:2].reshape(-1, 9)
    # (at h = H - 1 exactly the gradient is the one of the cell [H - 1, H], whose upper row is outside the map: -f)
    open_h, open_w = inner & (h < H - 1), inner & (w < W - 1)
    gs = max(dh.abs().max().item(), dw.abs().max().item())
    assert ((dh - s * (d * a).sum(-1)).abs() * open_h).max().item() <= 1e-12 * gs
    assert ((dw - s * (d * b).sum(-1)).abs() * open_w).max().item() <= 1e-12 * gs
    last = inner & (h == H - 1)
    if kind == 'edge':
        assert int(last.sum()) >= 4
    assert ((dh + s * (d * f(h, w)).sum(-1)).abs() * last).max().item() <= 1e-12 * gs
    # outside the open domain: nothing at all
    out = ~g.inside.reshape(-1, 9)
    assert int(out.sum()) > 5 and not bool(col[out].any()) and not bool(dh[out].any()) and not bool(dw[out].any())
    assert not bool(adj.dom[..., 18:27].reshape(-1, 9)[out].any())


# One channel quad on a 3 x 3 map, G[h][w] = 3 h + w + 1 in channel 0 (-G, G^2 and 1 in the others), a 1 x 1 kernel at
# output pixel (0, 0), so the sample point IS the offset pair.  Derived by hand from mmcv 1.4.0
# modulated_deform_conv_cuda_kernel.cuh: the domain test `h_im > -1 && w_im > -1 && h_im < height && w_im < width` of
# modulated_deformable_im2col_gpu_kernel, the corner tests of dmcn_im2col_bilinear (`h_low >= 0 && w_low >= 0`,
# `h_low >= 0 && w_high <= width - 1`, `h_high <= height - 1 && w_low >= 0`, `h_high <= height - 1 && w_high <= width - 1`),
# the offset pair `data_offset_h_ptr = 2 * (i * kernel_w + j)`, `..._w_ptr = 2 * (i * kernel_w + j) + 1`, and
# dmcn_get_coordinate_weight for the gradients (cell [floor(h), floor(h) + 1] also at an integer h).
# (off_h, off_w, value, d value / d h, d value / d w) of channel 0 before the mask
G = [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]]
VECTORS = [
    (0.0, 0.0, 1.0, 3.0, 1.0),                  # exactly at 0: the cell [0, 1] both ways
    (0.5, 0.5, 3.0, 3.0, 1.0),                  # (1 + 2 + 4 + 5) / 4
    (0.25, 1.0, 2.75, 3.0, 1.0),                # the FIRST of the pair is h: .75 G[0][1] + .25 G[1][1]  ((w, h) gives 4.25)
    (1.0, 0.25, 4.25, 3.0, 1.0),
    (1.0, 1.0, 5.0, 3.0, 1.0),                  # an interior integer
    (2.0, 2.0, 9.0, -9.0, -9.0),                # exactly at H - 1: the high corners are outside, the gradient sees -G[2][2]
    (-1.0, 0.0, 0.0, 0.0, 0.0),                 # exactly at -1: outside the open domain, no gradient either
    (0.0, -1.0, 0.0, 0.0, 0.0),
    (3.0, 1.0, 0.0, 0.0, 0.0),                  # exactly at H: outside
    (-0.5, 0.0, 0.5, 1.0, 0.5),                 # only the high-h corners valid: .5 G[0][0]; d/dw = .5 (G[0][1] - G[0][0])
    (-0.5, -0.5, 0.25, 0.5, 0.5),               # only the high-high corner valid
    (2.5, 2.5, 2.25, -4.5, -4.5),               # only the low-low corner valid: .25 G[2][2]
    (2.5, 0.0, 3.5, -7.0, 0.5),                 # only the low-h corners valid: .5 G[2][0]; d/dw = .5 (G[2][1] - G[2][0])
    (-0.9375, 1.0, 0.125, 2.0, 0.0625),         # -1 + 1/16: G[0][1] / 16
    (2.9375, 1.0, 0.5, -8.0, 0.0625),           # H - 1/16: G[2][1] / 16
]


@pytest.mark.parametrize('logit', [0.0, math.log(3.0)])
def test_hand_derived_vectors(logit):
    s = 1.0 / (1.0 + math.exp(-logit))
    g = torch.tensor(G, dtype=f64)
    x = torch.stack([g, -g, g * g, torch.ones_like(g)], -1).unsqueeze(0)          # (1, 3, 3, 4)
    for off_h, off_w, val, dh, dw in VECTORS:
        om = torch.zeros(1, 3, 3, 3, dtype=f64)
        om[0, 0, 0] = torch.tensor([off_h, off_w, logit], dtype=f64)
        col = D.im2col64(x, om, 1, 1, 1, 0, 1)
        assert col.shape == (9, 4)
        assert abs(col[0, 0].item() - s * val) <= 1e-15 and abs(col[0, 1].item() + s * val) <= 1e-15, (off_h, off_w)
        inside = -1 < off_h < 3 and -1 < off_w < 3
        if 0 <= off_h <= 2 and 0 <= off_w <= 2:
            assert abs(col[0, 3].item() - s) <= 1e-15           # the weights of the valid corners sum to 1 on the map
        assert inside or not bool(col[0].any())
        dcol = torch.zeros(9, 4, dtype=f64)
        dcol[0, 0] = 2.0
        adj = D.adjoint64(x, om, dcol, 1, 1, 1, 0, 1)
        got = adj.dom[0, 0, 0].tolist()
        want = [2.0 * s * dh, 2.0 * s * dw, 2.0 * s * (1 - s) * val]
        assert all(abs(a - b) <= 1e-14 for a, b in zip(got, want)), (off_h, off_w, got, want)
        assert not bool(adj.dom[0].reshape(9, 3)[1:].any())
        # dx: the four corner weights times s, on channel 0 only, summing to s x (the valid weights)
        assert not bool(adj.dx[..., 1:].any())
        assert abs((adj.dx[0, :, :, 0] * g).sum().item() - 2.0 * s * val) <= 1e-14


@pytest.mark.parametrize('stride,pad', [(1, 1), (2, 1), (1, 0), (2, 2)])
def test_zero_and_integer_offsets_are_a_convolution(stride, pad):
    gen = torch.Generator().manual_seed(5)
    N, H, W, C, Co = 2, 7, 8, 4, 3
    x = torch.randn(N, H, W, C, generator=gen, dtype=f64)
    w = torch.randn(Co, 3, 3, C, generator=gen, dtype=f64)
    Ho, Wo = D.out_size(H, W, 3, 3, stride, pad, 1)
    xn, wn = x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2)
    for lg, (sh, sw) in ((0.7, (0, 0)), (-1.3, (1, -2)), (0.0, (-3, 2)), (2.0, (0, 9))):
        om = torch.zeros(N, Ho, Wo, 27, dtype=f64)
        om[..., 0:18:2], om[..., 1:18:2], om[..., 18:] = sh, sw, lg
        y = D.deform_conv64(x, om, w, 3, 3, stride, pad).permute(0, 3, 1, 2)
        P = 12
        xp = F.pad(xn, (P, P, P, P))
        xs = xp[:, :, P - pad + sh:P - pad + sh + H + 2 * pad, P - pad + sw:P - pad + sw + W + 2 * pad]
        ref = F.conv2d(xs, wn, None, stride, 0) / (1.0 + math.exp(-lg))
        assert y.shape == ref.shape and (y - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize('name', sorted(CASES) + sorted(D.WRAP) + [f'fused_{n}' for n in D.FUSED])
def test_inputs_make_the_fp32_coordinate_exact(name):
    """every offset a multiple of 2^-4 (the far targets apart), and (float)hb + off without a rounding"""
    spec = CASES.get(name) or D.WRAP.get(name) or D.fused_spec(name[6:], torch.bfloat16)
    if name in D.WRAP:
        spec = dict(spec, H=9, W=9)             # the same generator on a small map
    x, om, dcol = D.make_inputs(spec)
    taps = spec['kh'] * spec['kw']
    off = om[..., :2 * taps]
    near = off.abs() < 1000
    assert bool(torch.isfinite(om).all()) and bool(torch.isfinite(x.float()).all()) and bool(torch.isfinite(dcol).all())
    assert bool(((off * 16) == torch.round(off * 16))[near].all()) and off[near].abs().max().item() <= 48
    hb, wb = D._base(spec)
    for b, o in ((hb, om[..., 0:2 * taps:2]), (wb, om[..., 1:2 * taps:2])):
        assert torch.equal((b.float() + o).double()[o.abs() < 1000], (b + o.double())[o.abs() < 1000])
        far = (b + o.double())[o.abs() >= 1000]
        assert bool(((far < -1000) | (far > 1000)).all())
    if spec['kind'] == 'edge':
        assert D.present_pairs(spec, om) == 324
    assert x.dtype == spec['dtype'] and (name not in D.WRAP or D.im2col_threads(D.WRAP[name]) > D.GRID_CAP_THREADS)


def test_wrap_cases_are_the_smallest_squares_past_the_cap():
    for name, spec in D.WRAP.items():
        assert D.im2col_threads(spec) > D.GRID_CAP_THREADS >= D.im2col_threads(dict(spec, H=spec['H'] - 1, W=spec['W'] - 1))


def _excess10(a, ref, dt, extra):
    return ((a - ref).abs() - 10 * R.bound(ref, dt, extra)).max().item()


@pytest.mark.parametrize('name', sorted(CASES))
def test_mutated_references_differ_by_ten_bounds(name):
    spec = CASES[name]
    x, om, dcol = D.make_inputs(spec)
    kw = D.conv_kw(spec)
    dt = spec['dtype']
    col = D.im2col64(x, om, channels_padded=spec['Cpad'], **kw)
    mag = D.im2col64(x, om, channels_padded=spec['Cpad'], magnitude=True, **kw)
    assert bool((mag >= col.abs() - 1e-12).all())
    muts = [1] if spec['kind'] != 'pile' else []
    if spec['kh'] == spec['kw'] > 1 and spec['kind'] != 'pile':
        muts += [2, 3]
    for m in muts:
        wrong = D.im2col64(x, om, channels_padded=spec['Cpad'], mutation=m, **kw)
        assert _excess10(wrong, col, dt, D.col_extra(mag)) > 0, (name, m)
    if spec['kind'] == 'edge':
        b = D.adjoint64(x, om, dcol, channels_padded=spec['Cpad'], **kw)
        assert bool((b.S_om >= b.dom.abs() - 1e-9).all()) and bool((b.S_dx >= b.dx.abs() - 1e-9).all())
        for m in (4, 5):
            assert (D.im2col64(x, om, mutation=m, **kw) - col).abs().max().item() <= 1e-12        # the columns do not move
            wrong = D.adjoint64(x, om, dcol, mutation=m, sides=False, **kw)
            assert (wrong.dx - b.dx).abs().max().item() <= 1e-12
            assert _excess10(wrong.dom, b.dom, torch.float32, D.dom_extra(b, spec['C'])) > 0, (name, m)
            moved = ((wrong.dom - b.dom).abs() > 1e-12).view(-1, 27)[:, :18]
            g = D.geometry(om.double(), 1, spec['H'], spec['W'], 3, 3, 1, 1, 1)
            h, w = g.h.reshape(-1, 9), g.w.reshape(-1, 9)
            at = ((h == -1) | (w == -1)) if m == 4 else ((h == h.round()) | (w == w.round()))
            assert not bool((moved[:, 0::2] | moved[:, 1::2])[~at].any())                         # only there


@pytest.mark.parametrize('dt', D.DTYPES, ids=list(D.SHORT.values()))
def test_pile_case_every_contribution_counts(dt):
    """144 taps into one cell, dcol > 0: S is the adjoint itself, and the smallest single contribution to any dx element
    exceeds ten times that element's fp32 bound -- a kernel that loses one atomic is refused"""
    spec = CASES[f'pile-{D.SHORT[dt]}']
    x, om, dcol = D.make_inputs(spec)
    b = D.adjoint64(x, om, dcol)
    assert (b.S_dx - b.dx).abs().max().item() <= 1e-12 * b.dx.abs().max().item()
    assert sorted(set(b.cnt.view(-1).tolist())) == [0.0, 144.0]
    bound = R.bound(b.dx, torch.float32, D.dx_extra(b))
    g = D.geometry(om.double(), 1, 4, 4, 3, 3, 1, 1, 1)
    d = dcol.double().view(1, 4, 4, 9, 8)
    worst = float('inf')
    for k in range(4):
        contrib = d * (g.wt[k] * g.s).unsqueeze(-1)                                   # (1, 4, 4, 9, 8), all > 0
        at = bound.view(16, 8)[g.idx[k]]
        worst = min(worst, (contrib / at).min().item())
    print(f'pile {D.SHORT[dt]}: smallest contribution / bound {worst:.1f}')
    assert worst > 10


def test_fp32_restatement_costs_stay_under_the_recorded_ceilings():
    """for the record (the module docstring): the same formulas in torch float32 against float64, as multiples of each
    extra term; nothing the kernels are held to is sized by these"""
    worst = {'col': 0.0, 'dx': 0.0, 'dom': 0.0}
    for name, spec in CASES.items():
        if not spec['col2im']:
            continue
        x, om, dcol = D.make_inputs(spec)
        kw = D.conv_kw(spec)
        cp = spec['Cpad']
        col = D.im2col64(x, om, channels_padded=cp, **kw)
        mag = D.im2col64(x, om, channels_padded=cp, magnitude=True, **kw)
        b = D.adjoint64(x, om, dcol, channels_padded=cp, **kw)
        col32 = D.im2col64(x, om, channels_padded=cp, work=torch.float32, **kw)
        b32 = D.adjoint64(x, om, dcol, channels_padded=cp, sides=False, work=torch.float32, **kw)
        for key, got, ref, extra in (('col', col32, col, D.col_extra(mag)), ('dx', b32.dx, b.dx, D.dx_extra(b)),
                                     ('dom', b32.dom, b.dom, D.dom_extra(b, spec['C']))):
            err = (got.double() - ref).abs()
            worst[key] = max(worst[key], (err / (extra + 1e-30)).max().item())     # (1e-30: sigmoid(-100) is subnormal)
    print('fp32 restatement / extra term: ' + '  '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert worst['col'] <= D.ORACLE_COL and worst['dx'] <= D.ORACLE_DX and worst['dom'] <= D.ORACLE_DOM
