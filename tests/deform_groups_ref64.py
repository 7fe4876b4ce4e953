"""float64 deformable im2col with deform groups G and the unmodulated form (DCN v1), its adjoint, the conv on top, and the
bounds tests/test_deform_groups_gpu.py and tests/test_resnet_dcn_gpu.py hold the `_g` entry points to.  It extends
tests/deform_ref64.py (which is not edited) and keeps its rules: open domain -1 < h < H, corner rule, the coordinate
gradient of the cell [h, h + 1].

Definitions.  T = kh kw taps, real channels C with C % G == 0, channel c in group c // (C / G); pad channels (c >= C) are
zero and in no group.  The offset row of an output pixel: [2 T g + 2 t] = dy, [2 T g + 2 t + 1] = dx of tap t in group g;
modulated: mask logit at [2 T G + T g + t].  Unmodulated (v1): the SAME sampling with the mask factor identically 1, rows
of 2 T G entries, no sigmoid anywhere.  v1 is defined by this restatement of v2, not by mmcv's v1 source.

How it is computed: a G-group problem on (N, H, W, C) is the G = 1 problem of deform_ref64 on (N G, H, W, C / G) -- the
groups folded into the batch, each with its own 3 T offset row (v1: the logits are +inf, whose sigmoid is exactly 1 and
has derivative 0) -- and unfolded again.  Everything deform_ref64 derives (S, cnt, mask_slip) folds the same way.
tests/test_deform_groups_ref64_cpu.py checks the fold against per-group calls on slices.

Bounds: deform_ref64's documented terms with the per-group channel count in the lane loop (a wave of the col2im kernel
runs over ONE group's channels: dom_chain(C / G)) and, for v1, SIG = 0 in every term that carries the sigmoid budget
(COL_K, DX_C0, the write-out part of dom_chain, the mask slip): the v1 kernels evaluate no sigmoid; their `* mask` is a
product with 1.f, which is exact, but its rounding stays in the budget.  No new constant, nothing fitted to kernel output.

Inputs (make_inputs): deform_ref64's construction per folded image -- offsets multiples of 2^-4 of magnitude <= 48, so
kernel and reference take the same side of every integer line and NO ELEMENT IS EXCLUDED FROM ANY COMPARISON; kind 'edge'
lays the cross product of edge_targets(H) x edge_targets(W) over the (image, group, pixel, tap) slots in order, starting
at pair `seed * 37 % pairs` and wrapping, so maps too small for the whole table (5 x 6, stride 2) carry a different part
of it per case; logits randn * 2 with MASK_SPECIALS placed in.

Mutated references (`mutation=`): 'swap' dy / dx read as (dx, dy); 'mask_interleave' the logit read at [2 T g + T + t];
'group_mod' the channel-to-group map c % G.
"""
import torch

from tests import deform_ref64 as D
from tests import route_util as R

U = D.U


def sig(modulated):
    return D.SIG if modulated else 0


def col_k(modulated):
    return D.WGT + 1 + 3 + sig(modulated) + 1


def dx_c0(modulated):
    return sig(modulated) + 1 + 2 * (D.WGT - 1) + 2


def dom_chain(cg, modulated):
    """deform_ref64.dom_chain over one group's channels; its write-out part carries SIG once"""
    return D.dom_chain(cg) - (D.SIG - sig(modulated))


def om_width(G, modulated, taps=9):
    return (3 if modulated else 2) * taps * G


# ---- fold / unfold --------------------------------------------------------------------------------------------------------
def _fold_x(x, G, group_mod=False):
    N, H, W, C = x.shape
    cg = C // G
    if group_mod:
        return x.reshape(N, H, W, cg, G).permute(0, 4, 1, 2, 3).reshape(N * G, H, W, cg)
    return x.reshape(N, H, W, G, cg).permute(0, 3, 1, 2, 4).reshape(N * G, H, W, cg)


def _unfold_x(xr, N, G, group_mod=False):
    _, H, W, cg = xr.shape
    if group_mod:
        return xr.reshape(N, G, H, W, cg).permute(0, 2, 3, 4, 1).reshape(N, H, W, cg * G)
    return xr.reshape(N, G, H, W, cg).permute(0, 2, 3, 1, 4).reshape(N, H, W, G * cg)


def _fold_om(om, G, modulated, taps, mask_interleave=False):
    N, Ho, Wo, _ = om.shape
    off = om[..., :2 * taps * G].reshape(N, Ho, Wo, G, 2 * taps)
    if not modulated:
        lg = torch.full((N, Ho, Wo, G, taps), float('inf'), dtype=om.dtype, device=om.device)
    elif mask_interleave:
        idx = (2 * taps * torch.arange(G).view(G, 1) + taps + torch.arange(taps).view(1, taps)).to(om.device)
        lg = om[..., idx.reshape(-1)].reshape(N, Ho, Wo, G, taps)
    else:
        lg = om[..., 2 * taps * G:3 * taps * G].reshape(N, Ho, Wo, G, taps)
    return torch.cat([off, lg], -1).permute(0, 3, 1, 2, 4).reshape(N * G, Ho, Wo, 3 * taps)


def _unfold_om(domr, N, G, modulated, taps):
    _, Ho, Wo, _ = domr.shape
    d = domr.reshape(N, G, Ho, Wo, 3 * taps).permute(0, 2, 3, 1, 4)
    parts = [d[..., :2 * taps].reshape(N, Ho, Wo, 2 * taps * G)]
    if modulated:
        parts.append(d[..., 2 * taps:].reshape(N, Ho, Wo, taps * G))
    return torch.cat(parts, -1)


def _fold_col(dcol, N, Ho, Wo, taps, C, Cpad, G, group_mod=False):
    d = dcol.reshape(N, Ho, Wo, taps, Cpad)[..., :C]
    cg = C // G
    if group_mod:
        d = d.reshape(N, Ho, Wo, taps, cg, G).permute(0, 5, 1, 2, 3, 4)
    else:
        d = d.reshape(N, Ho, Wo, taps, G, cg).permute(0, 4, 1, 2, 3, 5)
    return d.reshape(N * G * Ho * Wo, taps * cg)


def _unfold_col(colr, N, Ho, Wo, taps, C, Cpad, G, group_mod=False):
    cg = C // G
    c = colr.reshape(N, G, Ho, Wo, taps, cg)
    c = c.permute(0, 2, 3, 4, 5, 1) if group_mod else c.permute(0, 2, 3, 4, 1, 5)
    c = c.reshape(N, Ho, Wo, taps, C)
    if Cpad > C:
        c = torch.cat([c, c.new_zeros(c.shape[:-1] + (Cpad - C,))], -1)
    return c.reshape(N * Ho * Wo, taps * Cpad)


def _mut(mutation):
    assert mutation in (0, 'swap', 'mask_interleave', 'group_mod'), mutation
    return (1 if mutation == 'swap' else 0), mutation == 'mask_interleave', mutation == 'group_mod'


# ---- the reference ----------------------------------------------------------------------------------------------------------
def im2col64(x, om, G=1, modulated=True, kh=3, kw=3, stride=1, pad=1, dilation=1, channels_padded=None, mutation=0,
             magnitude=False, work=torch.float64):
    """x (N, H, W, C), om (N, Ho, Wo, >= (3 | 2) T G) -> columns (M, T Cpad), K order (tap, c), pad channels zero"""
    N, H, W, C = x.shape
    taps = kh * kw
    assert C % G == 0 and om.shape[-1] >= om_width(G, modulated, taps)
    Cpad = C if channels_padded is None else channels_padded
    m1, inter, gmod = _mut(mutation)
    xr, omr = _fold_x(x.to(work), G, gmod), _fold_om(om.to(work), G, modulated, taps, inter)
    colr = D.im2col64(xr, omr, kh, kw, stride, pad, dilation, mutation=m1, magnitude=magnitude, work=work)
    return _unfold_col(colr, N, omr.shape[1], omr.shape[2], taps, C, Cpad, G, gmod)


class Adjoint:
    """dx, S_dx, cnt (N, H, W, C); dom, S_om, mask_slip (N, Ho, Wo, (3 | 2) T G)"""


def adjoint64(x, om, dcol, G=1, modulated=True, kh=3, kw=3, stride=1, pad=1, dilation=1, channels_padded=None, mutation=0,
              work=torch.float64):
    N, H, W, C = x.shape
    taps = kh * kw
    Cpad = C if channels_padded is None else channels_padded
    m1, inter, gmod = _mut(mutation)
    om = om[..., :om_width(G, modulated, taps)]
    xr, omr = _fold_x(x.to(work), G, gmod), _fold_om(om.to(work), G, modulated, taps, inter)
    assert not inter, 'the adjoint of the interleaved-mask mutation is not needed'
    Ho, Wo = omr.shape[1], omr.shape[2]
    dr = _fold_col(dcol.to(work), N, Ho, Wo, taps, C, Cpad, G, gmod)
    a = D.adjoint64(xr, omr, dr, kh, kw, stride, pad, dilation, mutation=m1, work=work)
    b = Adjoint()
    b.dx, b.S_dx = _unfold_x(a.dx, N, G, gmod), _unfold_x(a.S_dx, N, G, gmod)
    b.cnt = _unfold_x(a.cnt.expand(-1, -1, -1, C // G), N, G, gmod)
    b.dom, b.S_om = _unfold_om(a.dom, N, G, modulated, taps), _unfold_om(a.S_om, N, G, modulated, taps)
    b.mask_slip = _unfold_om(a.mask_slip, N, G, modulated, taps)
    return b


def deform_conv64(x, om, w, G=1, modulated=True, stride=1, pad=1):
    """w (Cout, 3, 3, C) -> (N, Ho, Wo, Cout) float64"""
    N, H, W, C = x.shape
    Ho, Wo = D.out_size(H, W, 3, 3, stride, pad, 1)
    col = im2col64(x, om, G, modulated, stride=stride, pad=pad)
    return (col @ w.double().reshape(w.shape[0], 9 * C).t()).view(N, Ho, Wo, w.shape[0])


class DeformConv64(torch.nn.Module):
    """the deformable conv of a DCN / DCNv2 module as a differentiable float64 composition (conv_offset, then the above)"""

    def __init__(self, mod):
        super().__init__()
        self.w = torch.nn.Parameter(mod.weight.detach().double().clone())
        self.wo = torch.nn.Parameter(mod.conv_offset.weight.detach().double().clone())
        self.bo = torch.nn.Parameter(mod.conv_offset.bias.detach().double().clone())
        self.G, self.modulated, self.stride = mod.deform_groups, mod.modulated, mod.stride

    def forward(self, x_nhwc, om=None):
        """`om`: the offsets to sample at (fp32 values, as the kernels saw them); default: this module's own conv_offset"""
        if om is None:
            om = torch.nn.functional.conv2d(x_nhwc.permute(0, 3, 1, 2), self.wo, self.bo, self.stride, 1).permute(0, 2, 3, 1)
        return deform_conv64(x_nhwc, om, self.w.permute(0, 2, 3, 1), self.G, self.modulated, self.stride, 1)


# ---- the elementwise terms ----------------------------------------------------------------------------------------------------
def col_extra(colmag, modulated):
    return col_k(modulated) * U * colmag


def dx_extra(b, modulated):
    return (b.cnt + dx_c0(modulated)) * U * b.S_dx


def dom_extra(b, cg, modulated):
    return dom_chain(cg, modulated) * U * b.S_om + sig(modulated) * U * b.mask_slip


def conv_extra(x, om, w, G, modulated, stride=1, pad=1, scale=None):
    """the deformable term of a fused / two-launch conv result: the column error summed through |w| (and |scale|)"""
    colmag = im2col64(x, om, G, modulated, stride=stride, pad=pad, magnitude=True)
    N, H, W, C = x.shape
    Ho, Wo = D.out_size(H, W, 3, 3, stride, pad, 1)
    e = (col_extra(colmag, modulated) @ w.double().abs().reshape(w.shape[0], 9 * C).t()).view(N, Ho, Wo, w.shape[0])
    return e * scale.double().abs() if scale is not None else e


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def spec(C, G, modulated, dtype, seed, N=2, H=7, W=9, stride=1, pad=1, Cpad=None, kind='edge', om_stride=None):
    oms = om_width(G, modulated) if om_stride is None else om_stride
    return dict(C=C, G=G, modulated=modulated, dtype=dtype, seed=seed, N=N, H=H, W=W, kh=3, kw=3, stride=stride, pad=pad,
                dilation=1, Cpad=C if Cpad is None else Cpad, kind=kind, om_stride=oms)


def conv_kw(s):
    return dict(stride=s['stride'], pad=s['pad'])


def make_inputs(s, device='cpu'):
    """x (N, H, W, C) and dcol (M, 9 Cpad) fp32 values rounded to the dtype, om (N, Ho, Wo, om_stride) fp32"""
    g = torch.Generator().manual_seed(s['seed'])
    N, H, W, C, G, mod = s['N'], s['H'], s['W'], s['C'], s['G'], s['modulated']
    taps = 9
    Ho, Wo = D.out_size(H, W, 3, 3, s['stride'], s['pad'], 1)
    x = torch.randn(N, H, W, C, generator=g)
    om = torch.randn(N, Ho, Wo, s['om_stride'], generator=g) * 2.0       # (past the layout: noise nobody may read)
    off = om[..., :2 * taps * G].reshape(N, Ho, Wo, G, taps, 2).clone()
    off += (torch.rand(off.shape, generator=g) > 0.9).float() * 30
    off = D._dyadic(off)
    if s['kind'] == 'edge':
        hb, wb = D._base(s)                                              # (Ho, Wo, taps)
        pairs = torch.tensor(D.edge_pairs(s), dtype=torch.float64)
        slots = N * G * Ho * Wo * taps
        k = (torch.arange(min(slots, len(pairs))) + s['seed'] * 37) % len(pairs)
        o = off.permute(0, 3, 1, 2, 4, 5).reshape(slots, 2).clone()      # slot order (image, group, pixel, tap)
        hbf, wbf = hb.reshape(-1).repeat(N * G), wb.reshape(-1).repeat(N * G)
        o[:len(k), 0] = (pairs[k, 0] - hbf[:len(k)]).float()
        o[:len(k), 1] = (pairs[k, 1] - wbf[:len(k)]).float()
        off = o.view(N, G, Ho, Wo, taps, 2).permute(0, 2, 3, 1, 4, 5)
    om[..., :2 * taps * G] = off.reshape(N, Ho, Wo, 2 * taps * G)
    if mod:
        lg = om[..., 2 * taps * G:3 * taps * G].reshape(-1).clone()
        for k, v in enumerate(D.MASK_SPECIALS):
            lg[(7 * k + 3) % lg.numel()] = v
        om[..., 2 * taps * G:3 * taps * G] = lg.view(N, Ho, Wo, taps * G)
    dcol = torch.randn(N * Ho * Wo, taps * s['Cpad'], generator=g)
    return x.to(s['dtype']).to(device), om.contiguous().to(device), dcol.to(s['dtype']).float().to(device)


def bound(ref, dtype, extra=None):
    return R.bound(ref, dtype, extra)
