"""float64 modulated deformable im2col (DCNv2, deform_groups 1) on NHWC maps, its adjoint, the deformable conv on top, and
the bounds the GPU tests (tests/test_deform_gpu.py) hold csrc/deform.hip, csrc/deform_common.h and csrc/deform_conv_bf16.hip
to.  Plain torch float64, nothing of the library; it works on whatever device its inputs live on.
tests/test_deform_ref64_cpu.py checks reference, bounds and inputs without a device.

Definitions (mmcv 1.4.0 modulated_deform_conv_cuda_kernel.cuh: dmcn_im2col_bilinear, dmcn_get_gradient_weight,
dmcn_get_coordinate_weight and the three kernels that call them), per (output pixel m = (n, ho, wo), tap t = i * kw + j):
    off_h, off_w = om[m, 2 t], om[m, 2 t + 1];   s = sigmoid(om[m, 2 taps + t])
    h = ho stride - pad + i dilation + off_h,    w likewise with j
    the tap is inside iff -1 < h < H and -1 < w < W (open on both sides); outside it contributes nothing anywhere
    hl = floor(h), lh = h - hl, hh = 1 - lh (w likewise); the corners (hl, wl), (hl, wl + 1), (hl + 1, wl), (hl + 1, wl + 1)
    carry hh hw, hh lw, lh hw, lh lw; a corner outside [0, H - 1] x [0, W - 1] reads 0
    col[m, t Cpad + c] = s sum_corners weight x[corner, c]           (c < C; the pad channels are zero)
The adjoint is torch autograd through exactly this (floor has no gradient, so at an integer coordinate the gradient is
the one of the cell [h, h + 1], as dmcn_get_coordinate_weight takes it): dx, and d_om with the sigmoid's derivative
included, as the kernel returns it.  adjoint64 also evaluates the same sums over magnitudes: S (the absolute sum of the
terms of every dx element and of every d_om entry) and cnt (the non-zero contributions per dx pixel).

Bounds = route_util.bound (half an ulp of the result dtype x |ref| + ACC_TOL max(1, |ref|max)) + an elementwise term
derived from the arithmetic the kernels document, in units of u = 2^-24 (the relative error of ONE fp32 rounding):

  SIG = 6: the sigmoid 1.f / (1.f + expf(-l)) (deform.hip deform_im2col_nhwc_kernel `const float mask = ...`, the same
    line in deform_col2im_nhwc_kernel and deform_common.h deform_tap_geom): expf within 2 ulp = 4 u (HIP documents 1 ulp),
    which moves s by at most e / (1 + e) < 1 of that; the add u; the division u (-fhip-fp32-correctly-rounded-divide-sqrt).
  WGT = 3: a corner weight: lh = h_im - (float)h_low (u), hh = 1.f - lh (u), the product of two of them (u).
    (On the inputs of this module all three are exact: the budget is the general one.)
  COL_K = WGT + 1 + 3 + SIG + 1 = 14: `(w1 * v1 + w2 * v2 + w3 * v3 + w4 * v4) * mask` (deform_im2col_nhwc_kernel `out.x = `,
    deform_common.h deform_sample8 `s[e] = `): the product weight x corner (1), at most three adds over a term (3), the
    mask (SIG) and the product with it (1):
        |d col| <= COL_K u s sum_corners |weight| |x|                                           col_extra
  DX_C0 = SIG + 1 + 2 (WGT - 1) + 2 = 13: one dx contribution `gx * hh * hw` with `gx = gg[e] * mask` (deform_col2im_nhwc_kernel,
    the four atomicAdd lines): mask (SIG), gg x mask (1), hh and hw (2 each: the kernel multiplies them into gx one after
    the other, 2 more).  cnt such terms meet in one fp32 atomic accumulator in any order: at most cnt - 1 roundings of
    partial sums, each below the absolute sum S of the terms:
        |d dx| <= (cnt + DX_C0) u S                                                             dx_extra
  d_om, K = dom_chain(C) = 4 ceil(C / 256) + 6 + 10 + 13: a term of g_h / g_w / g_m passes through the lane's running
    sum (`for (int c = lane * 4; c < C; c += 256)`, four channels a pass: at most 4 ceil(C / 256) adds), the six
    __shfl_xor levels (6), its own products (`val = hh * hw * a1[e] + ...`: two weight factors at 2 u each, two products,
    three adds, and `gg[e] * val`: 10; the brackets of g_h / g_w need fewer), and the write-out `g_m * mask * (1.f - mask)`
    (mask SIG, the rounding of 1 - mask and two products 3, the other roundings of the line above inside 13):
        |d d_om| <= K u S  +  SIG u s A   at the mask logits                                    dom_extra
    The second term: the kernel forms 1 - s from the ROUNDED s, and |s'(1 - s') - s(1 - s)| = |s' - s| |1 - s - s'|
    <= |s' - s| <= SIG u s whatever 1 - s is (at a logit of 20 the fp32 s is 1 and the kernel's derivative 0, where the
    true one is 2e-9: a relative error of 1 that K u S, which carries the factor 1 - s, cannot hold).  A = sum_c |dcol_c|
    sum_corners |weight| |x|.
  16-bit results (the columns, DeformConvFunction's dx): the one rounding route_util.bound already adds.
No constant is fitted to kernel output.

Inputs (make_inputs, shared by the CPU and the GPU file): every offset is a multiple of 2^-4 of magnitude at most 48
(but for the targets -1e4, 1e4 and 3e9, which are far outside in any arithmetic) on maps of at most a few hundred rows, so
the kernel's `(float)hb + off` is exact in fp32: kernel and reference take the same side of every integer line and of
every edge of the domain by construction, and NO ELEMENT IS EXCLUDED FROM ANY COMPARISON.  x, dcol and dy are rounded to
the dtype first: the reference sees the kernel's operands.  No NaN or Inf inputs.

The edge table: h targets edge_targets(H), w targets edge_targets(W), the full cross product placed one pair per
(pixel, tap) slot in slot order (off = target - hb); the remaining slots carry random dyadic offsets.  Mask logits are
randn * 2 with -100, -20, -0.0, 0, 20, 100 placed in.

Mutated references (`mutation=`): the reference with ONE convention wrong --
  1 the offset pair read as (w, h);  2 the mask logit read interleaved (3 tap + 2) instead of at 2 taps + tap;
  3 the taps transposed, (j, i) for (i, j);  4 the domain closed, [-1, H] x [-1, W] (only d_om at exact -1 changes);
  5 at an integer coordinate the cell below / left, [h - 1, h] (only d_om changes).

What plain fp32 costs on the same inputs, for the record: this restatement evaluated in torch float32 on the CPU
(work=torch.float32: the same formulas, torch's own summation order) against float64, as a multiple of each extra term,
the largest over the col2im cases (tests/test_deform_ref64_cpu.py re-measures, prints and holds them under the ORACLE_*
ceilings, about twice the measurement; nothing the kernels are held to is sized by them):
    |col32 - col64| / col_extra          0.27        ORACLE_COL
    |dx32 - dx64|   / dx_extra           0.24        ORACLE_DX
    |dom32 - dom64| / dom_extra          0.12        ORACLE_DOM
(the ratio is error / (extra + 1e-30): sigmoid(-100) is subnormal in fp32)
"""
import math

import torch

from tests import route_util as R

U = 2.0 ** -24
SIG = 6
WGT = 3
COL_K = WGT + 1 + 3 + SIG + 1
DX_C0 = SIG + 1 + 2 * (WGT - 1) + 2
ORACLE_COL = 0.55
ORACLE_DX = 0.5
ORACLE_DOM = 0.25
MASK_SPECIALS = (-100.0, -20.0, -0.0, 0.0, 20.0, 100.0)
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
SHORT = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16'}


def dom_chain(C):
    """K: the most fp32 roundings one term of a d_om entry passes through, read off deform_col2im_nhwc_kernel"""
    return 4 * -(-C // 256) + 6 + 10 + 13


def out_size(H, W, kh, kw, stride, pad, dilation):
    return (H + 2 * pad - (dilation * (kh - 1) + 1)) // stride + 1, (W + 2 * pad - (dilation * (kw - 1) + 1)) // stride + 1


class Geom:
    """per (n, ho, wo, tap): h, w (sample point), inside, s (sigmoid), and per corner k = 0..3: idx[k] (row of the
    (N H W, C) map, clamped), wt[k] (weight, 0 where the corner is outside), gh[k] / gw[k]: |d weight / d h|, |d .. / d w|"""


def geometry(om, N, H, W, kh, kw, stride, pad, dilation, mutation=0):
    """om (N, Ho, Wo, >= 3 taps) in the working dtype (float64; float32 for the fp32 restatement)"""
    dev, wd = om.device, om.dtype
    taps = kh * kw
    _, Ho, Wo, _ = om.shape
    off_h, off_w = om[..., 0:2 * taps:2], om[..., 1:2 * taps:2]
    logit = om[..., 2 * taps:3 * taps]
    if mutation == 1:
        off_h, off_w = off_w, off_h
    if mutation == 2:
        logit = om[..., 2:3 * taps:3]
    t = torch.arange(taps, device=dev)
    i, j = (t % kh, t // kh) if mutation == 3 else (t // kw, t % kw)
    hb = (torch.arange(Ho, device=dev) * stride - pad).view(1, Ho, 1, 1) + (i * dilation).view(1, 1, 1, taps)
    wb = (torch.arange(Wo, device=dev) * stride - pad).view(1, 1, Wo, 1) + (j * dilation).view(1, 1, 1, taps)
    g = Geom()
    g.h, g.w = hb.to(wd) + off_h, wb.to(wd) + off_w
    if mutation == 4:
        g.inside = (g.h >= -1) & (g.w >= -1) & (g.h <= H) & (g.w <= W)
    else:
        g.inside = (g.h > -1) & (g.w > -1) & (g.h < H) & (g.w < W)
    hl, wl = (torch.ceil(g.h) - 1, torch.ceil(g.w) - 1) if mutation == 5 else (torch.floor(g.h), torch.floor(g.w))
    hl, wl = hl.detach(), wl.detach()
    lh, lw = g.h - hl, g.w - wl
    hh, hw = 1 - lh, 1 - lw
    g.s = torch.sigmoid(logit)
    nb = (torch.arange(N, device=dev) * (H * W)).view(N, 1, 1, 1)
    g.idx, g.wt, g.gh, g.gw, g.ok = [], [], [], [], []
    for hc, wc, wt, gh, gw in ((hl, wl, hh * hw, hw, hh), (hl, wl + 1, hh * lw, lw, hh), (hl + 1, wl, lh * hw, hw, lh),
                               (hl + 1, wl + 1, lh * lw, lw, lh)):
        ok = g.inside & (hc >= 0) & (hc <= H - 1) & (wc >= 0) & (wc <= W - 1)
        g.ok.append(ok)
        g.idx.append(nb + hc.clamp(0, H - 1).long() * W + wc.clamp(0, W - 1).long())
        okf = ok.to(wd)
        g.wt.append(wt * okf)
        g.gh.append(gh.detach().abs() * okf)
        g.gw.append(gw.detach().abs() * okf)
    return g


def _columns(x, g, Cpad, magnitude=False):
    """(M, taps * Cpad) from x (N, H, W, C) in the working dtype"""
    N, H, W, C = x.shape
    xf = x.reshape(N * H * W, C)
    if magnitude:
        xf = xf.abs()
    val = 0
    for k in range(4):
        wt = g.wt[k].abs() if magnitude else g.wt[k]
        val = val + xf[g.idx[k]] * wt.unsqueeze(-1)                  # (N, Ho, Wo, taps, C)
    val = val * g.s.unsqueeze(-1)
    if Cpad > C:
        val = torch.cat([val, val.new_zeros(val.shape[:-1] + (Cpad - C,))], -1)
    n, ho, wo, taps, _ = val.shape
    return val.reshape(n * ho * wo, taps * Cpad)


def im2col64(x, om, kh=3, kw=3, stride=1, pad=1, dilation=1, om_stride=None, channels_padded=None, mutation=0,
             magnitude=False, work=torch.float64):
    """x (N, H, W, C), om (N, Ho, Wo, om_stride) -> columns (M, kh kw Cpad), K order (tap, c), pad channels zero.
    magnitude=True: the same sum over |corner weight| |x| mask (the unit of col_extra)"""
    N, H, W, C = x.shape
    Ho, Wo = out_size(H, W, kh, kw, stride, pad, dilation)
    om_stride = om.shape[-1] if om_stride is None else om_stride
    assert tuple(om.shape) == (N, Ho, Wo, om_stride) and om_stride >= 3 * kh * kw, (om.shape, (N, Ho, Wo, om_stride))
    Cpad = C if channels_padded is None else channels_padded
    g = geometry(om.to(work), N, H, W, kh, kw, stride, pad, dilation, mutation)
    return _columns(x.to(work), g, Cpad, magnitude)


class Adjoint:
    """dx (N, H, W, C), dom (N, Ho, Wo, om_stride; zero past 3 taps) from autograd; S_dx, cnt (N, H, W, 1); S_om and
    mask_slip (s A at the mask logits, 0 elsewhere) shaped like dom; inside (N, Ho, Wo, taps)"""


def adjoint64(x, om, dcol, kh=3, kw=3, stride=1, pad=1, dilation=1, channels_padded=None, mutation=0, sides=True,
              work=torch.float64):
    """the adjoint of im2col64 at (x, om) applied to dcol (M, taps Cpad): torch autograd through the reference"""
    N, H, W, C = x.shape
    taps = kh * kw
    Cpad = C if channels_padded is None else channels_padded
    xr = x.detach().to(work).requires_grad_()
    omr = om.detach().to(work).requires_grad_()
    col = im2col64(xr, omr, kh, kw, stride, pad, dilation, None, Cpad, mutation, work=work)
    dc = dcol.detach().to(work)
    col.backward(dc)
    b = Adjoint()
    b.dx, b.dom = xr.grad, omr.grad
    if not sides:
        return b
    with torch.no_grad():
        g = geometry(omr.detach(), N, H, W, kh, kw, stride, pad, dilation, mutation)
        Ho, Wo = g.h.shape[1], g.h.shape[2]
        d = dc.view(N, Ho, Wo, taps, Cpad)[..., :C].abs()
        xa = xr.detach().reshape(N * H * W, C).abs()
        S_dx = torch.zeros(N * H * W, C, dtype=work, device=x.device)
        cnt = torch.zeros(N * H * W, dtype=work, device=x.device)
        Sh = Sw = A = 0
        for k in range(4):
            w_k = (g.wt[k] * g.s).unsqueeze(-1)
            S_dx.index_add_(0, g.idx[k].reshape(-1), (d * w_k).reshape(-1, C))
            cnt.index_add_(0, g.idx[k].reshape(-1), (g.wt[k] > 0).to(work).reshape(-1))
            dxk = (d * xa[g.idx[k]]).sum(-1)                                     # sum_c |dcol_c| |x_corner,c|
            Sh = Sh + g.gh[k] * dxk
            Sw = Sw + g.gw[k] * dxk
            A = A + g.wt[k] * dxk
        b.S_dx, b.cnt = S_dx.view(N, H, W, C), cnt.view(N, H, W, 1)
        b.S_om, b.mask_slip = torch.zeros_like(b.dom), torch.zeros_like(b.dom)
        b.S_om[..., 0:2 * taps:2] = g.s * Sh
        b.S_om[..., 1:2 * taps:2] = g.s * Sw
        b.S_om[..., 2 * taps:3 * taps] = g.s * (1 - g.s) * A
        b.mask_slip[..., 2 * taps:3 * taps] = g.s * A
        b.inside = g.inside
    return b


def deform_conv64(x, om, w, kh=3, kw=3, stride=1, pad=1, dilation=1, mutation=0):
    """the deformable conv as a float64 GEMM over the reference columns: w (Cout, kh, kw, C) -> (N, Ho, Wo, Cout)"""
    N, H, W, C = x.shape
    Ho, Wo = out_size(H, W, kh, kw, stride, pad, dilation)
    col = im2col64(x, om, kh, kw, stride, pad, dilation, mutation=mutation)
    return (col @ w.double().reshape(w.shape[0], kh * kw * C).t()).view(N, Ho, Wo, w.shape[0])


# ---- the elementwise terms (to be passed as `extra` to route_util.bound / excess / one_ulp_off) ---------------------------
def col_extra(colmag):
    return COL_K * U * colmag


def dx_extra(b):
    return (b.cnt + DX_C0) * U * b.S_dx


def dom_extra(b, C):
    return dom_chain(C) * U * b.S_om + SIG * U * b.mask_slip


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def edge_targets(size):
    """the coordinates at which the open domain, the per-corner validity and the one-sided gradient decide the result"""
    e, mid = 1.0 / 16, float(size // 2 if size > 2 else 0)
    return (-1 - e, -1.0, -1 + e, -0.5, -e, 0.0, e, mid, mid + 0.5, size - 1 - e, size - 1.0, size - 1 + e, size - e,
            float(size), size + e, -1e4, 1e4, 3e9)


def _dyadic(t):
    return (torch.round(t * 16) / 16).clamp(-48, 48)


def _base(spec):
    """hb, wb (Ho, Wo, taps) of every slot"""
    kh, kw = spec['kh'], spec['kw']
    Ho, Wo = out_size(spec['H'], spec['W'], kh, kw, spec['stride'], spec['pad'], spec['dilation'])
    t = torch.arange(kh * kw)
    hb = (torch.arange(Ho) * spec['stride'] - spec['pad']).view(Ho, 1, 1) + (t // kw * spec['dilation']).view(1, 1, -1)
    wb = (torch.arange(Wo) * spec['stride'] - spec['pad']).view(1, Wo, 1) + (t % kw * spec['dilation']).view(1, 1, -1)
    return hb.expand(Ho, Wo, -1).double(), wb.expand(Ho, Wo, -1).double()


def edge_pairs(spec):
    th, tw = edge_targets(spec['H']), edge_targets(spec['W'])
    return [(a, b) for a in th for b in tw]


def make_inputs(spec, device='cpu'):
    """x (N, H, W, C) and dcol (M, taps Cpad; fp32, the pad columns filled too: the kernels must not read them) rounded to
    the dtype, om (N, Ho, Wo, om_stride) fp32.  kind 'random': offsets randn * 2 (one in ten + 30) rounded to 2^-4;
    'edge': the edge table in the first slots of image 0; 'pile': every tap aimed into the cell [1, 2] x [1, 2], dcol > 0"""
    g = torch.Generator().manual_seed(spec['seed'])
    N, H, W, C, kh, kw = (spec[k] for k in ('N', 'H', 'W', 'C', 'kh', 'kw'))
    taps, oms, Cpad, dt = kh * kw, spec['om_stride'], spec['Cpad'], spec['dtype']
    Ho, Wo = out_size(H, W, kh, kw, spec['stride'], spec['pad'], spec['dilation'])
    x = torch.randn(N, H, W, C, generator=g)
    om = torch.randn(N, Ho, Wo, oms, generator=g) * 2.0          # (whatever lies past 3 taps is noise nobody may read)
    off = om[..., :2 * taps]
    off += (torch.rand(off.shape, generator=g) > 0.9).float() * 30
    om[..., :2 * taps] = _dyadic(off)
    dcol = torch.randn(N * Ho * Wo, taps * Cpad, generator=g)
    hb, wb = _base(spec)
    if spec['kind'] == 'edge':
        pairs = edge_pairs(spec)
        assert len(pairs) <= Ho * Wo * taps, 'the edge table does not fit'
        p = torch.tensor(pairs, dtype=torch.float64)
        oh = (p[:, 0] - hb.reshape(-1)[:len(pairs)]).float()
        ow = (p[:, 1] - wb.reshape(-1)[:len(pairs)]).float()
        o0 = om[0, ..., :2 * taps].reshape(-1, 2).clone()
        o0[:len(pairs), 0], o0[:len(pairs), 1] = oh, ow
        om[0, ..., :2 * taps] = o0.view(Ho, Wo, 2 * taps)
    if spec['kind'] == 'pile':
        fr = torch.randint(6, 11, (2, N, Ho, Wo, taps), generator=g).double() / 16      # weights between 6/16 and 10/16
        om[..., 0:2 * taps:2] = (1.0 + fr[0] - hb).float()
        om[..., 1:2 * taps:2] = (1.0 + fr[1] - wb).float()
        om[..., 2 * taps:3 * taps] = torch.rand(N, Ho, Wo, taps, generator=g) - 0.5
        dcol = torch.rand(dcol.shape, generator=g) + 0.5
    else:
        lg = om[..., 2 * taps:3 * taps].reshape(-1).clone()
        for k, v in enumerate(MASK_SPECIALS):
            lg[(7 * k + 3) % lg.numel()] = v
        om[..., 2 * taps:3 * taps] = lg.view(N, Ho, Wo, taps)
    return x.to(dt).to(device), om.to(device), dcol.to(dt).float().to(device)


def present_pairs(spec, om):
    """how many pairs of the edge table occur among the sample points of `om` (float64 of the fp32 offsets)"""
    hb, wb = _base(spec)
    taps = spec['kh'] * spec['kw']
    o = om[0].double().cpu()
    far = lambda v: 3e9 if v > 1e9 else v          # noqa: E731  (3e9 - hb is rounded to fp32: any point past 1e9 is it)
    pts = set(zip(map(far, (hb + o[..., 0:2 * taps:2]).reshape(-1).tolist()),
                  map(far, (wb + o[..., 1:2 * taps:2]).reshape(-1).tolist())))
    return sum((a, b) in pts for a, b in edge_pairs(spec))


def _spec(C, N, H, W, dtype, seed, kh=3, kw=3, stride=1, pad=1, dilation=1, om_stride=None, Cpad=None, kind='random',
          col2im=True):
    oms = 3 * kh * kw if om_stride is None else om_stride
    return dict(C=C, N=N, H=H, W=W, dtype=dtype, seed=seed, kh=kh, kw=kw, stride=stride, pad=pad, dilation=dilation,
                om_stride=oms, Cpad=C if Cpad is None else Cpad, kind=kind,
                im2col=dtype == torch.float32 or C % 8 == 0, col2im=col2im and oms == 3 * kh * kw)


def conv_kw(spec):
    return dict(kh=spec['kh'], kw=spec['kw'], stride=spec['stride'], pad=spec['pad'], dilation=spec['dilation'])


def cases():
    """name -> spec of every fp64 leg of the im2col / col2im tests (spec['im2col'], spec['col2im']: which entry accepts
    it).  Each is the smallest shape that reaches the thing it names; see the GPU file's docstring"""
    out = {}
    for dt in DTYPES:
        t = SHORT[dt]
        out[f'edge-{t}'] = _spec(64, 1, 6, 7, dt, 101, kind='edge')                   # 6 x 7 outputs: 378 slots, 324 pairs
        out[f'pile-{t}'] = _spec(8, 1, 4, 4, dt, 102, kind='pile')                    # 144 taps into one cell
        out[f's1_p1-{t}'] = _spec(8, 2, 7, 9, dt, 103)
        out[f's2_p1_odd-{t}'] = _spec(8, 2, 7, 9, dt, 104, stride=2)
        out[f's2_p1_even-{t}'] = _spec(8, 2, 8, 6, dt, 105, stride=2)
        out[f's1_p0-{t}'] = _spec(8, 2, 7, 9, dt, 106, pad=0)
        out[f's2_p0-{t}'] = _spec(8, 2, 8, 9, dt, 107, stride=2, pad=0)
        out[f's1_p2-{t}'] = _spec(8, 2, 7, 9, dt, 108, pad=2)
        out[f's2_p2-{t}'] = _spec(8, 2, 7, 8, dt, 109, stride=2, pad=2)
        out[f'dilation2-{t}'] = _spec(8, 2, 7, 9, dt, 110, pad=2, dilation=2)
        out[f'k1x1-{t}'] = _spec(8, 2, 5, 6, dt, 111, kh=1, kw=1, pad=0)
        out[f'k5x5-{t}'] = _spec(8, 1, 6, 7, dt, 112, kh=5, kw=5, pad=2)
        out[f'k1x3-{t}'] = _spec(8, 2, 5, 6, dt, 113, kh=1, kw=3, pad=1)
        out[f'om_stride64-{t}'] = _spec(8, 2, 7, 9, dt, 114, om_stride=64)
        out[f'cpad_208_224-{t}'] = _spec(208, 1, 4, 5, dt, 115, Cpad=224)
        out[f'cpad_8_24-{t}'] = _spec(8, 2, 5, 6, dt, 116, Cpad=24)
        out[f'c8-{t}'] = _spec(8, 1, 5, 6, dt, 117)
        out[f'c224-{t}'] = _spec(224, 1, 4, 5, dt, 118)
        out[f'c260-{t}'] = _spec(260, 1, 4, 5, dt, 119)                               # 16-bit: col2im only (C % 8 == 4)
        out[f'c512-{t}'] = _spec(512, 1, 4, 5, dt, 120)
        out[f'h1-{t}'] = _spec(8, 2, 1, 5, dt, 121)
        out[f'w1-{t}'] = _spec(8, 2, 5, 1, dt, 122)
        out[f'h2_w2-{t}'] = _spec(8, 2, 2, 2, dt, 123)
        out[f'h1_w1-{t}'] = _spec(8, 1, 1, 1, dt, 124)
        out[f'batch3-{t}'] = _spec(8, 3, 5, 6, dt, 125)
    out['c4-f32'] = _spec(4, 2, 5, 6, torch.float32, 126)                             # one lane; fp32 only (C % 8 == 4)
    out['c4-bf16'] = _spec(4, 2, 5, 6, torch.bfloat16, 126)                           # col2im only
    return out


# the grid-stride wrap: stream_grid caps the im2col grids at 32768 workgroups of 256 threads (4 fp32 / 8 16-bit channels a
# thread); the smallest square 3 x 3 / stride 1 / pad 1 maps at C = 256 past that
WRAP = {'wrap-f32': _spec(256, 1, 121, 121, torch.float32, 131, col2im=False),
        'wrap-bf16': _spec(256, 1, 171, 171, torch.bfloat16, 132, col2im=False)}
GRID_CAP_THREADS = 32768 * 256


def im2col_threads(spec):
    Ho, Wo = out_size(spec['H'], spec['W'], spec['kh'], spec['kw'], spec['stride'], spec['pad'], spec['dilation'])
    per = 4 if spec['dtype'] == torch.float32 else 8
    return spec['N'] * Ho * Wo * spec['kh'] * spec['kw'] * spec['Cpad'] // per


# the fused kernel: name -> (Cp, Cout, N, H, W, stride, pad, om_stride, epilogue); M = N Ho Wo
FUSED = {
    'm1': (64, 256, 1, 3, 3, 2, 0, 27, 'none'),                 # (a 3 x 3 map: on 1 x 1 nearly every tap falls outside)
    'm127': (128, 64, 1, 1, 127, 1, 1, 64, 'shift'),
    'm128': (256, 128, 1, 1, 128, 1, 1, 27, 'scale_shift'),
    'm129': (192, 64, 1, 1, 129, 1, 1, 64, 'relu'),
    'm1350_11_tiles': (64, 256, 2, 25, 27, 1, 1, 27, 'none'),
    'cp320_s2_p0_odd': (320, 128, 2, 9, 11, 2, 0, 27, 'shift'),
    'cp512_s2_p2_even': (512, 256, 1, 8, 10, 2, 2, 64, 'scale_shift'),
    's2_p1_even': (64, 64, 2, 8, 10, 2, 1, 64, 'relu'),
    's1_p0': (128, 128, 2, 7, 9, 1, 0, 27, 'none'),
    's1_p2': (64, 64, 2, 7, 9, 1, 2, 27, 'none'),
    'edge': (64, 64, 1, 6, 7, 1, 1, 27, 'none'),
}


def fused_spec(name, dtype):
    cp, cout, n, h, w, stride, pad, oms, epi = FUSED[name]
    s = _spec(cp, n, h, w, dtype, 140 + list(FUSED).index(name), stride=stride, pad=pad, om_stride=oms,
              kind='edge' if name == 'edge' else 'random')
    s.update(cout=cout, epilogue=epi)
    return s


def fused_weights(spec, device='cpu'):
    """w (Cout, 3, 3, Cp) rounded to the dtype, scale / shift (Cout) fp32 or None per the epilogue, relu"""
    g = torch.Generator().manual_seed(spec['seed'] + 1000)
    cout, cp = spec['cout'], spec['C']
    w = (torch.randn(cout, 3, 3, cp, generator=g) / math.sqrt(9 * cp)).to(spec['dtype']).to(device)
    sc = (torch.rand(cout, generator=g) + 0.5).to(device)
    sh = (torch.randn(cout, generator=g) * 0.2).to(device)
    epi = spec['epilogue']
    return w, (None if epi in ('none', 'shift') else sc), (None if epi == 'none' else sh), epi == 'relu'
