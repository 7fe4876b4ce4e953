"""float64 training-mode BatchNorm (+residual, +ReLU) over (rows, C) NHWC rows, its running-statistics update and its
backward in closed form, and the bounds the GPU tests (tests/test_bn_train_gpu.py) hold the kernels of csrc/bn_train.hip
to.  Plain torch float64, nothing of the library; tests/test_bn_ref64_cpu.py checks reference and bounds without a device
(F.batch_norm only as a cross-check there).

Definitions, per channel over n = rows values:
    mean = sum z / n,   var = sum (z - mean)^2 / n  (two passes, biased),   rstd = 1 / sqrt(var + eps)
    p = z[0] (the kernels' pivot: row 0 of the tensor),   delta = mean - p
    kappa = (delta^2 + var) / (var + eps)           <- eps IN the denominator: finite for a constant channel
    xh = (z - mean) rstd,  pre = xh gamma + beta (+ res),  y = relu(pre) or pre
    running_mean' = (1 - m) running_mean + m mean,   running_var' = (1 - m) running_var + m var n / (n - 1)
    g = dout where the mask holds, else 0 (the mask is an ARGUMENT: the GPU tests pass y_kernel > 0)
    dbeta = sum g,  dgamma = sum g xh,  dz = gamma rstd (g - dbeta / n - xh dgamma / n),  dres = g

Bounds = route_util.bound (half an ulp of the result dtype x |ref| + ACC_TOL max(1, |ref|max)) + a conditioning term
derived from the accumulation scheme csrc/bn_train.hip documents, u = 2^-24:

  bn_train_stats_kernel: per lane and channel d = fl(z - p) (one rounding), sum d and sum d^2 run in fp32 over chains of
  at most FOLD = 16 rows (`chain()` below: the chain a shape really reaches), then are folded into doubles; everything
  after -- the row lanes, the strips, bn_train_finalize_kernel -- is double.
    * a chain of n terms errs by <= (n - 1) u per term; with d's own rounding      |d S1| <= 16 u sum |z - p|
      and, the square of d (2 u) and the product's rounding (1 u) added,           |d S2| <= 19 u sum (z - p)^2
    * mean = p + S1 / n, rounded to fp32:   E|z - p| <= sqrt(E (z - p)^2) = sqrt(delta^2 + var), so
          |d mean| <= K_SUM u sqrt(delta^2 + var) + u |mean|,                       K_SUM = 16
    * var = S2 / n - (S1 / n)^2 in double:  |d var| <= 19 u (delta^2 + var) + 2 |delta| 16 u sqrt(delta^2 + var)
          <= K_VAR u (delta^2 + var),   K_VAR = 19 + 32 = 51;   the fp32 `batch_var` adds u var
      i.e. |d var| / (var + eps) <= K_VAR kappa u.  kappa is about the PIVOT's distance from the mean, not the mean's
      from zero: p is one value of the channel, delta^2 ~ var and kappa ~ 2 whatever mean^2 / var is (kappa_10 /
      kappa_100 below: mean^2 / var = 1e2 / 1e4, kappa <= 10); an outlier in row 0 costs its own distance, once.
      (the var < 0 clamp only moves a negative value towards the true, non-negative one)
    * rstd = (var + eps)^-1/2 rounded to fp32:   |d rstd| / rstd <= (1 - K_VAR kappa u)^-1/2 - 1 + u  =: rho(kappa)
    * running statistics: formed in double from the unrounded mean / var, rounded once:
          |d running_mean'| <= m K_SUM u sqrt(delta^2 + var) + u |running_mean'|
          |d running_var'|  <= m n / (n - 1) K_VAR u (delta^2 + var) + u |running_var'|
  apply (brcnn_bn_act_forward on scale = fl(gamma rstd), shift = fl(beta - fl(mean scale)), no fused multiply-add):
          |d y| <= (rho + 2 u) |xh gamma| + |gamma| rstd |d mean| (1 + rho)
                   + u (4 |mean gamma rstd| + |beta| + |xh gamma| + |pre| + |y|)
      -- the last line is the price of the two-coefficient form: z scale and shift are each of the size of mean scale.
  backward, same d mean / d rstd to first order:  |d xh| <= mu + |xh| rho,  mu = |d mean| rstd
    * bn_train_bwd_reduce_kernel: sum g in chains of <= 16 (K_DBETA = 16: 15 adds + the rounding to fp32) and
      sum g (z - mean): the difference (1), the product (1), the chain (15), rstd and the rounding to fp32 (1):
          |d dbeta| <= K_DBETA u S_beta,   |d dgamma| <= K_DGAMMA u S_gamma + sum |g| (mu + |xh| rho),   K_DGAMMA = 18
      with S_beta = sum |g|, S_gamma = sum |g xh|
    * bn_train_bwd_write_kernel, dz = gs (g - k1 - xh k2) in fp32 (xh 2, k = sum x fl(1 / n) 2, the product 1, the
      differences 2, gs 1 roundings: 8):
          |d dz| <= (rho + 2 u) |dz| + |gamma| rstd / n (|d dbeta| + (mu + |xh| rho) |dgamma| + |xh| |d dgamma|)
                    + 8 u |gamma| rstd (|g| + (|dbeta| + |xh| |dgamma|) / n)
No constant is fitted to kernel output.

What fp32 costs on the same inputs, measured on the CPU (tests/test_bn_ref64_cpu.py re-measures, prints and asserts that
these stay below the ORACLE_* ceilings): torch's fp32 F.batch_norm(training=True) with autograd against this float64 on
the cases kappa_1 / kappa_10 / kappa_100 (channel mean 0.3 / 10 / 100 at unit spread, mean^2 / var up to 1e4, the pivot's
kappa 1.02-4.93 in all three; 273 rows x 32 channels, ReLU):
    |y32 - y64| / max(1, |y64|max)                                      6.3e-8 / 3.7e-7 / 1.8e-6      ORACLE_Y_REL
    |y32 - y64| / y_extra                                               0.06 / 0.26 / 0.30            ORACLE_Y_OVER_EXTRA
    |var32 - var64| / (u var)                                           2.0 / 1.5 / 2.4               ORACLE_VAR
    |var32 - var64| / (the derived (K_VAR + 1) u (delta^2 + var))       0.026 / 0.028 / 0.036         ORACLE_VAR_OVER_BOUND
    |dz32 - dz64| / dz_extra                                            0.07 / 0.10 / 0.63            ORACLE_DZ_OVER_EXTRA
    |dgamma32 - dgamma64| / dgamma_extra                                0.02 / 0.06 / 0.17            ORACLE_DGAMMA_OVER_EXTRA
    |dbeta32 - dbeta64| / (u S_beta)                                    0.49 / 0.49 / 0.49            ORACLE_DBETA
(torch's CPU kernel keeps its statistics in double: the variance costs it two ulps whatever the mean is; its backward is
fp32 and spends 0.6 of dz_extra at mean 100.)
The derived constants are worst cases of the kernels' scheme (every rounding of a 16-term chain in one direction); random
data spends a fraction of them, and plain fp32 arithmetic on the CPU between 2 % and 60 % -- they are not looser than the
reference arithmetic needs by orders of magnitude.
"""
import torch

from tests import route_util as R

U = 2.0 ** -24
FOLD = 16           # rows per fp32 chain (csrc/bn_train.hip)
K_SUM = 16          # fl(z - p) (1) + a chain of <= 16 adds (15)
K_SQ = 19           # the square of fl(z - p) (2) + its rounding (1) + the chain (15), + 1 for the second-order terms
K_VAR = K_SQ + 2 * K_SUM
K_DBETA = 16
K_DGAMMA = 18
K_DZ = 8
MASK_BAND_CAP = 1e-3

# measured on the CPU, see the docstring: ceilings about twice the measurement (test_bn_ref64_cpu.py prints both)
ORACLE_Y_REL = (1.3e-7, 8e-7, 4e-6)
ORACLE_Y_OVER_EXTRA = 0.6
ORACLE_VAR = (4.0, 3.0, 5.0)
ORACLE_VAR_OVER_BOUND = 0.08
ORACLE_DZ_OVER_EXTRA = 1.3
ORACLE_DGAMMA_OVER_EXTRA = 0.35
ORACLE_DBETA = 1.0


def plan(rows, channels, dtype):
    """(V, CW, RL, chunks, strips, rows per strip) of csrc/bn_train.hip's `plan`"""
    V = 4 if dtype == torch.float32 else 8
    assert channels % V == 0
    cvn = channels // V
    assert cvn & (cvn - 1) == 0
    short = rows < 16384
    cw_max, wg, min_rows = (64, 1024, 32) if short else (256, 512, 64)
    CW = min(cvn, cw_max)
    chunks = cvn // CW
    strips = max(1, wg // chunks)
    rpb = max(-(-rows // strips), min_rows)
    return V, CW, 256 // CW, chunks, -(-rows // rpb), rpb


def chain(rows, channels, dtype):
    """(longest fp32 chain, chains per lane) a shape reaches: whether the fold into doubles happens more than once"""
    _, _, RL, _, _, rpb = plan(rows, channels, dtype)
    per_lane = -(-min(rows, rpb) // RL)
    return min(FOLD, per_lane), -(-per_lane // FOLD)


def rho(kappa):
    """relative error of the kernel's fp32 rstd, see the docstring; kappa elementwise"""
    d = (K_VAR * U * kappa).clamp(max=0.5)
    return (1.0 - d) ** -0.5 - 1.0 + U


def f32(v):
    """a host float as the kernels receive it (float argument), as float64"""
    return float(torch.tensor(float(v), dtype=torch.float32).double())


class Fwd:
    """y, pre, xh (rows, C); mean, var, rstd, delta, kappa, new_rm, new_rv (C)"""


def bn_forward64(z, gamma, beta, eps, relu, res=None, running_mean=None, running_var=None, momentum=0.1,
                 biased_running=False):
    """`biased_running`: the running variance from the BIASED batch variance -- the wrong reference a mutation leg must see
    refused; False everywhere else"""
    x = z.double()
    n = x.shape[0]
    gm, bt = gamma.double(), beta.double()
    f = Fwd()
    f.n, f.eps = n, f32(eps)
    f.mean = x.mean(0)
    f.var = ((x - f.mean) ** 2).mean(0)
    f.rstd = (f.var + f.eps) ** -0.5
    f.delta = f.mean - x[0]
    f.m2 = f.delta ** 2 + f.var
    f.kappa = f.m2 / (f.var + f.eps)
    f.xh = (x - f.mean) * f.rstd
    f.aff = f.xh * gm
    f.pre = f.aff + bt + (res.double() if res is not None else 0.0)
    f.y = f.pre.relu() if relu else f.pre
    f.gamma, f.beta = gm, bt
    if running_mean is not None:
        m = f32(momentum)
        f.m = m
        f.new_rm = (1.0 - m) * running_mean.double() + m * f.mean
        f.new_rv = (1.0 - m) * running_var.double() + m * f.var * (1.0 if biased_running else n / (n - 1.0))
    return f


class Bwd:
    """dz, dres (rows, C), dgamma, dbeta, S_beta, S_gamma (C)"""


def bn_backward64(dout, f, mask, drop_dgamma_term=False):
    """closed form; `mask` (rows, C) bool: where the ReLU passed (all True without ReLU).  `drop_dgamma_term`: dz without
    xh dgamma / n -- the second wrong reference of the mutation legs"""
    g = dout.double() * mask.to(torch.float64)
    b = Bwd()
    b.g = g
    b.dbeta, b.dgamma = g.sum(0), (g * f.xh).sum(0)
    b.S_beta, b.S_gamma = g.abs().sum(0), (g * f.xh).abs().sum(0)
    corr = 0.0 if drop_dgamma_term else f.xh * b.dgamma / f.n
    b.dz = f.gamma * f.rstd * (g - b.dbeta / f.n - corr)
    b.dres = g
    return b


# ---- the bounds ------------------------------------------------------------------------------------------------------------
def mean_err(f):
    """|d mean| before ACC_TOL: absolute, (C)"""
    return K_SUM * U * f.m2.sqrt() + U * f.mean.abs()


def mu(f):
    return mean_err(f) * f.rstd


def mean_bound(f):
    return R.bound(f.mean, torch.float32, mean_err(f))


def var_bound(f):
    return R.bound(f.var, torch.float32, (K_VAR + 1) * U * f.m2)


def rstd_bound(f):
    """no ACC_TOL here: rstd reaches 1 / sqrt(eps), the derived relative bound is the whole of it"""
    return rho(f.kappa) * f.rstd


def running_mean_bound(f):
    return R.bound(f.new_rm, torch.float32, f.m * K_SUM * U * f.m2.sqrt() + U * f.new_rm.abs())


def running_var_bound(f):
    return R.bound(f.new_rv, torch.float32, f.m * f.n / (f.n - 1.0) * K_VAR * U * f.m2 + U * f.new_rv.abs())


def y_extra(f):
    r = rho(f.kappa)
    msc = (f.mean * f.gamma * f.rstd).abs()
    return (r + 2 * U) * f.aff.abs() + f.gamma.abs() * f.rstd * mean_err(f) * (1.0 + r) + \
        U * (4 * msc + f.beta.abs() + f.aff.abs() + f.pre.abs() + f.y.abs())


def dbeta_extra(b):
    return K_DBETA * U * b.S_beta


def dgamma_extra(f, b):
    return K_DGAMMA * U * b.S_gamma + (b.g.abs() * (mu(f) + f.xh.abs() * rho(f.kappa))).sum(0)


def dz_extra(f, b):
    r, m, xa = rho(f.kappa), mu(f), f.xh.abs()
    gs = f.gamma.abs() * f.rstd
    return (r + 2 * U) * b.dz.abs() + \
        gs / f.n * (dbeta_extra(b) + (m + xa * r) * b.dgamma.abs() + xa * dgamma_extra(f, b)) + \
        K_DZ * U * gs * (b.g.abs() + (b.dbeta.abs() + xa * b.dgamma.abs()) / f.n)


def mask_band_share(f, dtype):
    """share of the elements whose float64 pre-activation lies within the forward bound of 0: where y_kernel > 0 may
    differ from pre64 > 0"""
    band = R.bound(f.pre, dtype, y_extra(f))
    return (f.pre.abs() <= band).double().mean().item()


# ---- inputs, shared by the CPU and the GPU tests ---------------------------------------------------------------------------
def make_case(rows, C, dtype, seed, mean=0.3, spread=1.0, residual=False, constant=(), device='cpu'):
    """z (rows, C) ~ N(mean, spread) and dout ~ N(0, 1) (and res ~ N(0, 1)), rounded to `dtype` (the float64 reference sees
    the kernel's operands); gamma = 1 + 0.5 N (sign as it falls), beta = 0.3 N, running_mean = 0.1 N, running_var =
    1 + 0.2 U, all fp32.  `constant`: channels whose z is the constant 1.5"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, C, generator=g) * spread + mean
    dout = torch.randn(rows, C, generator=g)
    res = torch.randn(rows, C, generator=g) if residual else None
    gm = 1.0 + 0.5 * torch.randn(C, generator=g)
    bt = 0.3 * torch.randn(C, generator=g)
    rm = 0.1 * torch.randn(C, generator=g)
    rv = 1.0 + 0.2 * torch.rand(C, generator=g)
    for c in constant:
        z[:, c] = 1.5
    dev = lambda t: None if t is None else t.to(device)       # noqa: E731
    return dict(z=dev(z.to(dtype)), dout=dev(dout.to(dtype)), res=dev(res.to(dtype)) if residual else None, gamma=dev(gm),
                beta=dev(bt), rm=dev(rm), rv=dev(rv))


DTYPES = (torch.float32, torch.bfloat16, torch.float16)
SHORT = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16'}
MIN_C = {torch.float32: 4, torch.bfloat16: 8, torch.float16: 8}
# strip boundaries of `plan` on both sides (one strip up to 32 rows; the short / long rule changes at 16384), GroupNorm's row
# counts kept beside them; 2 rows is the smallest accepted count
ROW_COUNTS = (2, 3, 7, 32, 33, 49, 128, 129, 256, 257, 273, 1050, 16383, 16384, 16385, 131073)
EPS = 1e-5


def _spec(rows, C, dtype, seed, relu, residual, **kw):
    return dict(rows=rows, C=C, dtype=dtype, seed=seed, relu=relu, residual=residual, kw=kw)


def cases():
    """name -> spec of every fp64 leg of the GPU file; the CPU test holds the float64 mask band of each ReLU one under
    MASK_BAND_CAP"""
    out = {}
    for dt in DTYPES:
        t = SHORT[dt]
        for rows in ROW_COUNTS:     # the smallest accepted width: 256 row lanes, one chain each
            out[f'rows{rows}-{t}'] = _spec(rows, MIN_C[dt], dt, 13, True, rows % 2 == 1)
        for relu in (False, True):
            for residual in (False, True):
                out[f'c64-relu{int(relu)}-res{int(residual)}-{t}'] = _spec(273, 64, dt, 17, relu, residual)
        out[f'c2048-{t}'] = _spec(1050, 2048, dt, 19, True, True)           # 8 channel chunks x 64 vectors (fp32), 4 (16-bit)
        out[f'folds-{t}'] = _spec(131073, 64, dt, 23, True, False)          # many partials; fp32: 17 rows per lane, two chains
        if dt != torch.float32:     # 4 row lanes x 64 vectors, 17 rows per lane: two chains in the 16-bit modes too
            out[f'folds_wide-{t}'] = _spec(34817, 512, dt, 41, True, True)
        out[f'kappa_10-{t}'] = _spec(273, 64, dt, 29, True, False, mean=10.0)
        out[f'kappa_100-{t}'] = _spec(273, 64, dt, 31, False, False, mean=100.0)
        out[f'constant-{t}'] = _spec(273, 64, dt, 37, True, True, constant=(0, 5, 63))
    return out


def case_inputs(spec, device='cpu'):
    return make_case(spec['rows'], spec['C'], spec['dtype'], spec['seed'], residual=spec['residual'], device=device,
                     **spec['kw'])
