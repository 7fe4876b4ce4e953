"""float64 GroupNorm(+ReLU) over concatenated NHWC segments, its backward in closed form, and the bounds the GPU tests
(tests/test_groupnorm_gpu.py) hold the kernels of csrc/misc.hip to.  Plain torch float64, nothing of the library;
tests/test_gn_ref64_cpu.py checks reference and bounds without a device (F.group_norm only as a cross-check there).

Definitions.  Per (segment, image, group), D = pixels x channels per group elements:
    mean = sum x / D,   var = sum (x - mean)^2 / D  (two passes, biased),   rstd = 1 / sqrt(var + eps)
    kappa = (mean^2 + var) / (var + eps)            <- eps IN the denominator: finite for a constant group
    xh = (x - mean) rstd,  pre = xh gamma + beta,  y = relu(pre) or pre
    g = dy where the mask holds, else 0 (the mask is an ARGUMENT: the GPU tests pass y_kernel > 0)
    dbeta_c = sum g,  dgamma_c = sum g xh;   s1 = sum g gamma, s2 = sum g gamma xh per (segment, image, group)
    dx = rstd (g gamma - s1 / D - xh s2 / D)

Bounds = route_util.bound (half an ulp of the result dtype x |ref| + ACC_TOL max(1, |ref|max)) + a conditioning term
derived from the accumulation scheme the kernels document, u = 2^-24:

  gn_stats_kernel: per lane and channel, sum x and sum x^2 run in fp32 over at most 32 rows, then are folded into
  doubles (everything after -- the row lanes, the channels of a group, the atomics, gn_finalize_kernel -- is double).
    * an fp32 chain of n <= 32 terms errs by <= (n-1) u sum|x| (sum) and <= n u sum x^2 (each square is rounded too), so
          |d sum x| <= 31 u sum|x|,       |d E[x^2]| <= 32 u E[x^2]   (33 below: the double folds, 1 / D)
    * mean:  |d mean| <= 31 u E|x| <= 31 u sqrt(E[x^2]) (Cauchy-Schwarz); its rounding to fp32 adds u |mean|:
          |d mean| <= K_MEAN u sqrt(mean^2 + var),                     K_MEAN = 32
      (counting the rounding alone, K = 1, misses that the fp32 sum moves the mean as well)
    * var = E[x^2] - mean^2 in double from the UNROUNDED mean:  |d var| <= 33 u E[x^2] + 2 |mean| 31 u sqrt(E[x^2])
          <= (33 + 62) u (mean^2 + var),  so  |d var| / (var + eps) <= K_VAR kappa u,     K_VAR = 95
      (the var < 0 clamp only moves a negative value towards the true, non-negative one)
    * rstd = (var + eps)^-1/2, rounded to fp32:   |d rstd| / rstd <= (1 - K_VAR kappa u)^-1/2 - 1 + u  =: rho(kappa)
      -- to first order 47.5 kappa u (the E[x^2] term alone would give 16.5 kappa u: the mean^2 term is the larger one)
  apply: y = (x - mean) rstd gamma + beta in fp32 (4 roundings, inside ACC_TOL), so elementwise
          |d y| <= rho |pre - beta| + K_MEAN sqrt(kappa) u |gamma|      (d mean rstd = K_MEAN u sqrt(kappa))
  backward, same d mean / d rstd to first order:  |d xh| <= mu + |xh| rho,  mu = K_MEAN sqrt(kappa) u
    * gn_bwd_reduce_kernel + gn_bwd_param_kernel + gn_bwd_param_final_kernel sum g and g xh in fp32: a term passes
      through at most K roundings, K = param_chain(): rows per row lane of a chunk + the row lanes combined through LDS
      + rows per lane of a slice of the partials + its 8 LDS lanes + the 32 slices + 3 (xh and the product), so
          |d dbeta| <= K u S_beta,    |d dgamma| <= K u S_gamma + sum |g| (mu + |xh| rho)
      with S_beta = sum |g|, S_gamma = sum |g xh|
    * s1, s2 (the same fp32 chunk sums x gamma, then double atomics, read back as fp32):
          |d s1| <= K u S1,    |d s2| <= K u S2 + mu S1 + rho S2,      S1 = sum |g gamma|, S2 = sum |g gamma xh|
    * dx:  |d dx| <= rho |dx| + rstd / D (|d s1| + (mu + |xh| rho) |s2| + |xh| |d s2|)
                    + 4 u rstd (|g gamma| + (|s1| + |xh| |s2|) / D)     (the fp32 evaluation of the formula)
No constant is fitted to kernel output.

What fp32 costs on the same inputs, measured on the CPU (tests/test_gn_ref64_cpu.py re-measures, prints and asserts
that these stay below the ORACLE_* ceilings): torch's fp32 F.group_norm with autograd -- the arithmetic of
oracle/cpu_pipeline.py -- against this float64 on the cases kappa_1 / kappa_1e2 / kappa_1e4 (mean 0.3 / 10 / 100 at unit
spread, kappa 1.05-1.13 / 92-105 / 9180-10330; C = 32, G = 4, two 7 x 7 maps):
    |y32 - y64| / max(1, |y64|max)                                      7.2e-8 / 7.0e-6 / 4.9e-4      ORACLE_Y_REL
    |y32 - y64| / (u (kappa |pre - beta| + sqrt(kappa) |gamma|))        2.8 / 1.8 / 1.5               ORACLE_Y_COND
        -- the unit of the conditioning term, whose derived constants are K_VAR / 2 = 47.5 and K_MEAN = 32
    |dx32 - dx64| / dx_extra                                            0.032 / 0.038 / 0.030         ORACLE_DX_OVER_EXTRA
    |dgamma32 - dgamma64| / dgamma_extra                                0.006 / 0.006 / 0.006         ORACLE_DGAMMA_OVER_EXTRA
    |dbeta32 - dbeta64| / (u S_beta)  (K = 61 here)                     0.83 / 0.83 / 0.83            ORACLE_DBETA
The derived constants are worst cases of the kernels' scheme (every rounding of a 32-term chain in one direction); random
data spends a few percent of them, on the CPU oracle as above.
"""
import torch

from tests import route_util as R

U = 2.0 ** -24
K_MEAN = 32         # fp32 sum of <= 32 rows (31) + the rounding of the mean to fp32 (1)
K_VAR = 95          # 33 (E[x^2]: 32 rows, each square rounded, + the double folds) + 2 x 31 (mean^2 from the fp32 sum)
GN_PARAM_SLICES = 32
MASK_BAND_CAP = 1e-3

# measured on the CPU, see the docstring: ceilings about twice the measurement (test_gn_ref64_cpu.py prints both)
ORACLE_Y_REL = (2e-7, 2e-5, 1.5e-3)
ORACLE_Y_COND = (6.0, 4.0, 4.0)
ORACLE_DX_OVER_EXTRA = 0.1
ORACLE_DGAMMA_OVER_EXTRA = 0.1
ORACLE_DBETA = 2.0


def rho(kappa):
    """relative error of the kernel's fp32 rstd, see the docstring; kappa elementwise"""
    d = (K_VAR * U * kappa).clamp(max=0.5)
    return (1.0 - d) ** -0.5 - 1.0 + U


def mu(kappa):
    """|d mean| rstd, i.e. the error of xh from the mean alone"""
    return K_MEAN * U * kappa.sqrt()


def bwd_chunks(max_hw):
    """(chunks, rows per chunk) of the backward's row split: at most 64 chunks of at least 256 rows"""
    c = min(64, (max_hw + 255) // 256)
    rpb = (max_hw + c - 1) // c
    return (max_hw + rpb - 1) // rpb, rpb


def fwd_chunks(max_hw):
    """(chunks, rows per chunk) of the forward's: at most 512 chunks"""
    c = min(512, (max_hw + 255) // 256)
    rpb = (max_hw + c - 1) // c
    return (max_hw + rpb - 1) // rpb, rpb


def row_lanes(dtype, channels):
    """row lanes of the statistics / reduce kernels = channels per lane: 8 for 16-bit rows of whole 16-byte vectors"""
    return 8 if dtype != torch.float32 and channels % 8 == 0 else 4


def param_chain(batch, sizes, dtype, channels):
    """K: the most fp32 roundings one term of dgamma / dbeta / s1 / s2 passes through, read off the kernels"""
    max_hw = max(h * w for h, w in sizes)
    chunks, rpb = bwd_chunks(max_hw)
    rl = row_lanes(dtype, channels)
    per = -(-batch * len(sizes) * chunks // GN_PARAM_SLICES)
    return -(-rpb // rl) + rl + -(-per // 8) + 8 + GN_PARAM_SLICES + 3


class Fwd:
    """y, pre, xh (rows, C); mean, var, kappa, rstd (L, N, G); *_e: the same expanded to (rows, C); D_e the count"""


def _segments(batch, sizes):
    r0 = 0
    for s, (h, w) in enumerate(sizes):
        yield s, r0, h * w
        r0 += batch * h * w


def _expand(t, hw, cpg):
    """(N, G) -> (N * hw, G * cpg)"""
    n, g = t.shape
    return t.view(n, 1, g, 1).expand(n, hw, g, cpg).reshape(n * hw, g * cpg)


def gn_forward64(x_cat, gamma, beta, groups, batch, sizes, eps, relu, count_slip=0):
    """`count_slip`: the statistics with D + count_slip for D (one-pass form) -- the wrong reference the sharpness leg
    must see refused; 0 everywhere else"""
    x = x_cat.double()
    rows, C = x.shape
    cpg = C // groups
    assert C % groups == 0 and rows == batch * sum(h * w for h, w in sizes)
    gm, bt = gamma.double(), beta.double()
    f = Fwd()
    means, vars_, exp = [], [], {k: [] for k in ('mean', 'var', 'D')}
    for s, r0, hw in _segments(batch, sizes):
        xs = x[r0:r0 + batch * hw].view(batch, hw, groups, cpg)
        D = hw * cpg
        if count_slip:
            mean = xs.sum((1, 3)) / (D + count_slip)
            var = (xs * xs).sum((1, 3)) / (D + count_slip) - mean * mean
        else:
            mean = xs.mean((1, 3))
            var = ((xs - mean.view(batch, 1, groups, 1)) ** 2).mean((1, 3))
        means.append(mean)
        vars_.append(var)
        exp['mean'].append(_expand(mean, hw, cpg))
        exp['var'].append(_expand(var, hw, cpg))
        exp['D'].append(torch.full((batch * hw, C), float(D), dtype=torch.float64, device=x.device))
    f.mean, f.var = torch.stack(means), torch.stack(vars_)
    f.rstd = (f.var + eps) ** -0.5
    f.kappa = (f.mean ** 2 + f.var) / (f.var + eps)
    f.mean_e, f.var_e, f.D_e = (torch.cat(exp[k]) for k in ('mean', 'var', 'D'))
    f.rstd_e = (f.var_e + eps) ** -0.5
    f.kappa_e = (f.mean_e ** 2 + f.var_e) / (f.var_e + eps)
    f.xh = (x - f.mean_e) * f.rstd_e
    f.pre = f.xh * gm + bt
    f.y = f.pre.relu() if relu else f.pre
    f.groups, f.batch, f.sizes = groups, batch, tuple(sizes)
    return f


class Bwd:
    """dx (rows, C), dgamma, dbeta (C); S_beta, S_gamma (C); s1, s2, S1, S2 (L, N, G) and s2_e, S1_e, S2_e, s1_e (rows, C)"""


def gn_backward64(dy, f, gamma, mask):
    """closed form, as above the reduce kernel; `mask` (rows, C) bool: where the ReLU passed (all True without ReLU)"""
    g = dy.double() * mask.to(torch.float64)
    gm = gamma.double()
    C = g.shape[1]
    cpg = C // f.groups
    b = Bwd()
    b.dbeta, b.dgamma = g.sum(0), (g * f.xh).sum(0)
    b.S_beta, b.S_gamma = g.abs().sum(0), (g * f.xh).abs().sum(0)
    gg = g * gm
    acc = {k: [] for k in ('s1', 's2', 'S1', 'S2')}
    exp = {k: [] for k in acc}
    for s, r0, hw in _segments(f.batch, f.sizes):
        sl = slice(r0, r0 + f.batch * hw)
        v = gg[sl].view(f.batch, hw, f.groups, cpg)
        vx = (gg[sl] * f.xh[sl]).view(f.batch, hw, f.groups, cpg)
        for k, t in (('s1', v.sum((1, 3))), ('s2', vx.sum((1, 3))), ('S1', v.abs().sum((1, 3))), ('S2', vx.abs().sum((1, 3)))):
            acc[k].append(t)
            exp[k].append(_expand(t, hw, cpg))
    b.s1, b.s2, b.S1, b.S2 = (torch.stack(acc[k]) for k in ('s1', 's2', 'S1', 'S2'))
    b.s1_e, b.s2_e, b.S1_e, b.S2_e = (torch.cat(exp[k]) for k in ('s1', 's2', 'S1', 'S2'))
    b.gg = gg
    b.g = g
    b.dx = f.rstd_e * (gg - b.s1_e / f.D_e - f.xh * b.s2_e / f.D_e)
    return b


# ---- the conditioning terms (to be passed as `extra` to route_util.bound / excess / one_ulp_off) ------------------------
def y_extra(f, gamma, beta):
    return rho(f.kappa_e) * (f.pre - beta.double()).abs() + mu(f.kappa_e) * gamma.double().abs()


def mean_bound(f):
    """absolute, (L, N, G): the stats buffer's fp32 mean"""
    return K_MEAN * U * (f.mean ** 2 + f.var).sqrt()


def rstd_bound(f):
    """absolute, (L, N, G): the stats buffer's fp32 rstd"""
    return rho(f.kappa) * f.rstd


def dbeta_extra(b, K):
    return K * U * b.S_beta


def dgamma_extra(f, b, K):
    return K * U * b.S_gamma + (b.g.abs() * (mu(f.kappa_e) + f.xh.abs() * rho(f.kappa_e))).sum(0)


def dx_extra(f, b, K):
    r, m = rho(f.kappa_e), mu(f.kappa_e)
    d_s1 = K * U * b.S1_e
    d_s2 = K * U * b.S2_e + m * b.S1_e + r * b.S2_e
    xa = f.xh.abs()
    return r * b.dx.abs() + f.rstd_e / f.D_e * (d_s1 + (m + xa * r) * b.s2_e.abs() + xa * d_s2) + \
        4 * U * f.rstd_e * (b.gg.abs() + (b.s1_e.abs() + xa * b.s2_e.abs()) / f.D_e)


def mask_band_share(f, dtype, gamma, beta):
    """share of the elements whose float64 pre-activation lies within the forward bound of 0: where y_kernel > 0 may
    differ from pre64 > 0"""
    band = R.bound(f.pre, dtype, y_extra(f, gamma, beta))
    return (f.pre.abs() <= band).double().mean().item()


# ---- inputs, shared by the CPU and the GPU tests ---------------------------------------------------------------------------
def make_case(C, G, batch, sizes, dtype, seed, mean=0.3, spread=1.0, gamma='random', beta='random', constant_groups=(),
              device='cpu'):
    """x (rows, C) ~ N(mean, spread), dy ~ N(0, 1), both rounded to `dtype` (the float64 reference sees the kernel's
    operands); gamma / beta fp32.  gamma: 'random' (1 + 0.5 N, sign as it falls) | 'signed' (zeros and negative entries
    forced in); beta: 'random' (0.3 N) | a number.  `constant_groups`: groups whose x is the constant 1.5 in every
    segment and image"""
    g = torch.Generator().manual_seed(seed)
    rows = batch * sum(h * w for h, w in sizes)
    x = torch.randn(rows, C, generator=g) * spread + mean
    dy = torch.randn(rows, C, generator=g)
    gm = 1.0 + 0.5 * torch.randn(C, generator=g)
    if gamma == 'signed':
        gm[0::3] = 0.0
        gm[1::3] = -gm[1::3].abs() - 0.25
    bt = 0.3 * torch.randn(C, generator=g) if beta == 'random' else torch.full((C,), float(beta))
    cpg = C // G
    for k in constant_groups:
        x[:, k * cpg:(k + 1) * cpg] = 1.5
    return x.to(dtype).to(device), dy.to(dtype).to(device), gm.to(device), bt.to(device)


PYRAMID = ((13, 21), (7, 11), (4, 6), (2, 3), (1, 1))
MAX_LEVELS = 8                  # BRCNN_MAX_LEVELS
ROUTES = {'rows_c256_g32': (256, 32), 'rows_c64_g32': (64, 32), 'rows_c8_g8': (8, 8), 'rows_c8_g1': (8, 1),
          'flat_c4_g1': (4, 1), 'flat_c4_g4': (4, 4), 'flat_c12_g4': (12, 4), 'flat_c36_g9': (36, 9),
          'flat_c252_g36': (252, 36)}
ROUTE_BATCH, ROUTE_SIZES = 2, ((13, 21), (7, 11))
ROW_COUNTS = (1, 3, 7, 49, 128, 129, 256, 257, 273, 1050, 16385, 131073)
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
_SHORT = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16'}


def _spec(C, G, batch, sizes, dtype, seed, relus=(False, True), eps=1e-5, **kw):
    return dict(C=C, G=G, batch=batch, sizes=tuple(sizes), dtype=dtype, seed=seed, relus=relus, eps=eps, kw=kw)


def cases():
    """name -> spec of every fp64 leg of the GPU file; the CPU test holds the float64 mask band of each ReLU one under
    MASK_BAND_CAP.  Shapes: the smallest that reach each route / chunking rule / edge (see the GPU file)"""
    out = {}
    for name, (C, G) in ROUTES.items():
        for dt in DTYPES:
            out[f'{name}-{_SHORT[dt]}'] = _spec(C, G, ROUTE_BATCH, ROUTE_SIZES, dt, 11)
    for hw in ROW_COUNTS:
        for dt in (torch.float32, torch.bfloat16):
            out[f'hw{hw}-{_SHORT[dt]}'] = _spec(8, 2, 2 if hw <= 1050 else 1, ((hw, 1),), dt, 13, relus=(True,))
    for dt in (torch.float32, torch.bfloat16):
        t = _SHORT[dt]
        out[f'n1-{t}'] = _spec(16, 4, 1, ROUTE_SIZES, dt, 17, relus=(True,))
        out[f'box_head_512x7x7-{t}'] = _spec(256, 32, 512, ((7, 7),), dt, 19, relus=(True,))
        out[f'pyramid-{t}'] = _spec(16, 4, 2, PYRAMID, dt, 23, relus=(True,))
        out[f'pyramid_ascending-{t}'] = _spec(16, 4, 2, PYRAMID[::-1], dt, 23, relus=(True,))
        out[f'two_equal-{t}'] = _spec(16, 4, 2, ((7, 11), (7, 11)), dt, 29, relus=(True,))
        out[f'max_levels-{t}'] = _spec(16, 4, 2, tuple((i + 1, 3) for i in range(MAX_LEVELS)), dt, 31, relus=(True,))
    f32 = torch.float32
    st = (32, 4, 2, ((7, 7),), f32, 41)
    out['kappa_1-f32'] = _spec(*st, mean=0.3)
    out['kappa_1e2-f32'] = _spec(*st, mean=10.0)
    out['kappa_1e4-f32'] = _spec(*st, relus=(False,), mean=100.0)     # (its band alone would hold 2 % of the elements)
    out['constant_all-f32'] = _spec(*st, constant_groups=(0, 1, 2, 3))
    out['constant_one-f32'] = _spec(*st, constant_groups=(1,))
    out['constant_one-bf16'] = _spec(32, 4, 2, ((7, 7),), torch.bfloat16, 41, constant_groups=(1,))
    out['eps_1e-3-f32'] = _spec(*st, eps=1e-3)
    out['gamma_signed-f32'] = _spec(*st, gamma='signed')
    out['gamma_signed-flat-bf16'] = _spec(12, 4, 2, ((7, 7),), torch.bfloat16, 43, gamma='signed')
    out['all_clipped-f32'] = _spec(*st, relus=(True,), beta=-10.0)
    out['none_clipped-f32'] = _spec(*st, relus=(True,), beta=10.0)
    return out


def case_inputs(spec, device='cpu'):
    return make_case(spec['C'], spec['G'], spec['batch'], spec['sizes'], spec['dtype'], spec['seed'], device=device,
                     **spec['kw'])
