"""GPU tests of the VFNet baseline (csrc/vfnet_head.hip, VFNetHead, VFNet).

Against the fixture g31_vfnet.npz (tests/golden/make_golden_vfnet.py; the reference's fp32 run): labels and kept order exact,
boxes and scores within the 2e-4 of g29's / g30's end-to-end cases (the fixture's reference run is within 5e-5 of its own
float64 run), losses within rtol 2e-3 / atol 1e-4 as tests/test_gfl_gpu.py holds its own.
Against float64 (tests/vfnet_ref64.py): bounds stated where used, derived from the fp32 arithmetic of the kernels (eps = 2^-23;
an addition, product or division rounds to eps / 2, expf / logf / powf are counted as 2 eps); none is tuned to what the kernels
give.  Two quantities have no short closed form -- the outputs and gradients of the chain raw0 -> offsets -> both star
deformable convs, and the GIoU gradients of the loss, whose errors are cancellations inside bilinear weights and box extents
-- and are held to 4 x the gap between the float32 and the float64 run of the SAME torch restatement on the same inputs,
measured on the CPU inside the test (the factor covers a different but equally valid order of the 9 C terms of a column and
of the terms of a gradient).  Measured gaps of the chain case below (float32 restatement vs float64, largest element): y_reg
2.9e-06, y_cls 1.6e-06 (values up to 5.3), d raw0 1.7e-06 (up to 3.9), d scale 2.2e-06 (of 2.3), d x 1.6e-06 / 1.2e-06 (up
to 5.4), d weight 6.0e-06 / 4.4e-06 (up to 27); of the loss cases: d D0 4.6e-10 .. 7.8e-10 (up to 5e-3), d D1 8.1e-10 ..
1.2e-09 (up to 4e-3)."""
import math
import os
import re

import numpy as np
import pytest
import torch

import brcnn  # noqa: F401
from brcnn import build_detector, build_head, ops, train_ops
from brcnn.config import ConfigDict
from tests import atss_ref64 as RA
from tests import util
from tests import vfnet_inputs as vi
from tests import vfnet_ref64 as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G = os.path.join(os.path.dirname(__file__), 'golden', 'g31_vfnet.npz')
EPS32 = float(np.finfo(np.float32).eps)
L = len(vi.SIZES)
N_L = [h * w for h, w in vi.SIZES]
PADS = [(128, 192), (96, 160)]


@pytest.fixture(scope='module')
def gold():
    return {k: v for k, v in np.load(G, allow_pickle=False).items()}


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def build(C=4, training=False, **over):
    head = build_head(ConfigDict(vi.head_cfg(C, **over))).train(training)
    with torch.no_grad():
        for s, v in zip(head.scales, vi.SCALES):
            s.scale.fill_(v)
        for s, v in zip(head.scales_refine, vi.SCALES_REFINE):
            s.scale.fill_(v)
    return head.to(DEV)


def base_table():
    half = [s * vi.OCTAVE / 2 for s in vi.STRIDES]
    return ops.atss_base_anchors([torch.tensor([[-h, -h, h, h]]) for h in half])


def dev(v):
    return torch.tensor(v, dtype=torch.float32, device=DEV)


def padded(rows, width, off, fill=7.0):
    """(n, c) -> (n, width) with the columns at `off`, every other column holding `fill`: nothing else may be read"""
    out = torch.full((rows.shape[0], width), fill)
    out[:, off:off + rows.shape[1]] = rows
    return out.to(DEV).contiguous()


def test_the_library_exports_every_vfnet_entry_of_the_header():
    from brcnn import lib
    from brcnn.registry import DETECTORS, HEADS, LOSSES
    header = open(os.path.join(vi.ROOT, 'include', 'brcnn_hip.h')).read()
    declared = sorted(set(re.findall(r'^(?:int|size_t) (brcnn_vfnet_\w+)\(', header, re.M)))
    assert declared == ['brcnn_vfnet_decode_levels', 'brcnn_vfnet_loss_backward', 'brcnn_vfnet_loss_finalize',
                        'brcnn_vfnet_loss_forward', 'brcnn_vfnet_loss_workspace_bytes', 'brcnn_vfnet_refine',
                        'brcnn_vfnet_refine_backward', 'brcnn_vfnet_rows_workspace_bytes', 'brcnn_vfnet_star_offsets',
                        'brcnn_vfnet_star_offsets_backward']
    for name in declared:
        assert name in lib.SIGNATURES and hasattr(lib.load(), name), name
    assert HEADS.get('VFNetHead') is not None and DETECTORS.get('VFNet') is not None and LOSSES.get('VarifocalLoss') is not None


# ------------------------------------------------------------------------------------------- distances and star offsets
def test_hand_made_offsets_are_exact():
    """raw = 0, scale = 1, level 0: D0 == 64 exactly (exp(0) = 1), q = (0.9f * 64 + 0.1f * 64) / 8 = 8 (0.9f + 0.1f rounds to
    1); tap 0 gets (-8, -8) - (-1, -1), the centre tap (0, 0), tap 8 (8, 8) - (1, 1): bit for bit"""
    r0 = torch.zeros(2 * 3 * 5, 8, device=DEV)
    d0, off = ops.vfnet_star_offsets(r0, dev([1.0]), 2, [(3, 5)], [8], [64.0], 0.1)
    assert d0.shape == (30, 4) and off.shape == (30, 18)
    assert torch.equal(d0.cpu(), torch.full((30, 4), 64.0))
    want = torch.tensor([-7., -7., -7., 0., -7., 7., 0., -7., 0., 0., 0., 7., 7., -7., 7., 0., 7., 7.])
    assert torch.equal(off.cpu(), want.expand(30, 18))
    # bbox_norm_type='stride': the denominator is the stride; 1 cell per side
    d0, off = ops.vfnet_star_offsets(r0, dev([1.0]), 2, [(3, 5)], [8], [8.0], 0.1)
    assert torch.equal(d0.cpu(), torch.full((30, 4), 8.0)) and torch.equal(off.cpu(), torch.zeros(30, 18))


OFFSET_CASES = [('one level, less than a wave', [(3, 5)], [8], [64.0], 2, 4, 0),
                ('the pyramid', vi.SIZES, vi.STRIDES, [float(d) for d in vi.REG_DENOMS], 2, 4, 0),
                # 3 x 513 = 1539 rows: seven workgroups of 256 threads, the last with three rows
                ('padding columns, ragged tail', vi.SIZES[:4] + [(1, 3)], vi.STRIDES, [float(s) for s in vi.STRIDES], 3, 8, 3)]


@pytest.mark.parametrize('name,sizes,strides,denoms,B,width,off', OFFSET_CASES, ids=[c[0] for c in OFFSET_CASES])
def test_offsets_forward_and_backward_against_float64(name, sizes, strides, denoms, B, width, off):
    """z = scale * raw rounds once (0.5 eps |z| in the argument of exp = that much relative error), expf 2 eps, the product
    with the denominator 0.5: D0 within (0.5 |z| + 2.5) eps.  q = (f0 D + f1 D) / s adds the roundings of f0 and f1, two
    products, a sum and a division, 3 eps; the subtraction of the base offset 0.5 eps of the result: an offset within
    ((0.5 |z| + 5.5) |q| + 0.5 |offset|) eps.  Backward: three-term sums of the offset gradients (1 eps of their absolute
    sum), / s, * f1 (f1's own rounding included: 2 eps), + dD0 (0.5), * D0 (its own error + 0.5), * scale (0.5): d raw within
    (0.5 |z| + 7) eps of the same expression on absolute values; dscale sums B h w products d z * raw (each one more
    rounding) -- eight sequential additions per thread, a tree of 8 levels, up to 256 partials per level added by the same
    scheme: 24 eps of the sum of absolute terms covers the order."""
    g = torch.Generator().manual_seed(11)
    Lc = len(sizes)
    rows = sum(B * h * w for h, w in sizes)
    raw = torch.randn(rows, 4, generator=g) * 0.6 - 0.5
    scales = torch.tensor(vi.SCALES[:Lc])
    dd = torch.randn(rows, 4, generator=g)
    doff = torch.randn(rows, 18, generator=g)
    r0 = padded(raw, width, off).requires_grad_()
    sc = scales.to(DEV).requires_grad_()
    d0, offs = train_ops.vfnet_star_offsets(r0, sc, B, sizes, strides, denoms, vi.GRADIENT_MUL, off)
    assert [tuple(o.shape) for o in offs] == [(B, h, w, 18) for h, w in sizes]
    got_off = torch.cat([o.reshape(-1, 18) for o in offs]).detach().cpu().double()
    # float64
    raw64, sc64 = raw.double().requires_grad_(), scales.double().requires_grad_()
    lvl = torch.cat([torch.full((B * h * w,), l) for l, (h, w) in enumerate(sizes)])
    den, st = torch.tensor(denoms, dtype=torch.float64)[lvl], torch.tensor(strides, dtype=torch.float64)[lvl]
    z = raw64 * sc64[lvl][:, None]
    D = z.exp() * den[:, None]
    o64 = R.star_offsets(D, vi.GRADIENT_MUL, st[:, None])
    zabs = z.detach().abs()
    assert ((d0.detach().cpu().double() - D.detach()).abs() <= (0.5 * zabs + 2.5) * EPS32 * D.detach()).all()
    q = (D.detach() / st[:, None])
    qmax = q.max(1, keepdim=True)[0]
    bound = ((0.5 * zabs.max(1, keepdim=True)[0] + 5.5) * qmax + 0.5 * o64.detach().abs()) * EPS32
    assert ((got_off - o64.detach()).abs() <= bound).all()
    # backward
    r = 0
    total = (d0 * dd.to(DEV)).sum()
    for o, (h, w) in zip(offs, sizes):
        n = B * h * w
        total = total + (o.reshape(n, 18) * doff[r:r + n].to(DEV)).sum()
        r += n
    total.backward()
    ((D * dd.double()).sum() + (o64 * doff.double()).sum()).backward()
    gr = r0.grad.cpu().double()
    assert float(gr[:, :off].abs().max() if off else 0) == 0 and float(gr[:, off + 4:].abs().max() if width > off + 4 else 0) == 0
    o = doff.double().abs()
    mag_sum = torch.stack([o[:, 1] + o[:, 7] + o[:, 13], o[:, 0] + o[:, 2] + o[:, 4], o[:, 5] + o[:, 11] + o[:, 17],
                           o[:, 12] + o[:, 14] + o[:, 16]], 1)
    mag = (dd.double().abs() + vi.GRADIENT_MUL * mag_sum / st[:, None]) * D.detach() * sc64.detach().abs()[lvl][:, None]
    assert ((gr[:, off:off + 4] - raw64.grad).abs() <= (0.5 * zabs + 7) * EPS32 * mag).all()
    terms = (mag / sc64.detach().abs()[lvl][:, None] * raw64.detach().abs())
    for l in range(Lc):
        tol = (0.5 * float(zabs[lvl == l].max()) + 8 + 24) * EPS32 * float(terms[lvl == l].sum())
        assert abs(float(sc.grad[l]) - float(sc64.grad[l])) <= tol, (l, float(sc.grad[l]), float(sc64.grad[l]), tol)


def test_refine_forward_and_backward_against_float64():
    """D1 = exp(scale_refine * raw1) * D0, D0 a constant: the bounds of the offsets test without the offset terms"""
    g = torch.Generator().manual_seed(12)
    B, rows = 2, 2 * vi.ANCHORS
    raw = torch.randn(rows, 4, generator=g) * 0.3
    d0 = torch.rand(rows, 4, generator=g) * 200 + 1
    dd = torch.randn(rows, 4, generator=g)
    r1 = padded(raw, 8, 2).requires_grad_()
    sc = dev(list(vi.SCALES_REFINE)).requires_grad_()
    d0g = d0.to(DEV).requires_grad_()
    d1 = train_ops.vfnet_refine(r1, sc, d0g, B, vi.SIZES, 2)
    (d1 * dd.to(DEV)).sum().backward()
    assert d0g.grad is None                                                     # .detach() in the reference
    lvl = torch.cat([torch.full((B * n,), l) for l, n in enumerate(N_L)])
    raw64, sc64 = raw.double().requires_grad_(), torch.tensor(vi.SCALES_REFINE, dtype=torch.float64).requires_grad_()
    z = raw64 * sc64[lvl][:, None]
    D = z.exp() * d0.double()
    (D * dd.double()).sum().backward()
    zabs = z.detach().abs()
    assert ((d1.detach().cpu().double() - D.detach()).abs() <= (0.5 * zabs + 2.5) * EPS32 * D.detach()).all()
    mag = dd.double().abs() * D.detach() * sc64.detach()[lvl][:, None]
    gr = r1.grad.cpu().double()
    assert ((gr[:, 2:6] - raw64.grad).abs() <= (0.5 * zabs + 4) * EPS32 * mag).all()
    assert float(gr[:, :2].abs().max()) == 0 and float(gr[:, 6:].abs().max()) == 0
    terms = mag / sc64.detach()[lvl][:, None] * raw64.detach().abs()
    for l in range(L):
        tol = (0.5 * float(zabs[lvl == l].max()) + 5 + 24) * EPS32 * float(terms[lvl == l].sum())
        assert abs(float(sc.grad[l]) - float(sc64.grad[l])) <= tol, l


# ------------------------------------------------------------------------------------------- the star deformable convs
CELLS = (0.37, 1.43, 2.71, 4.19, 9.63)      # distances in cells: every star coordinate at least 0.19 from an integer


def chain_inputs():
    """a 6 x 7 map, 2 images, C = 8, level 0 (stride 8, denominator 64); per cell and side a distance drawn from CELLS"""
    g = torch.Generator().manual_seed(21)
    B, h, w, C = 2, 6, 7, 8
    cells = torch.tensor(CELLS)[torch.randint(0, len(CELLS), (B * h * w, 4), generator=g)]
    scale = 1.1
    raw0 = (cells * 8 / 64).log() / scale
    xr, xc = torch.randn(B * h * w, C, generator=g), torch.randn(B * h * w, C, generator=g)
    wr, wc = torch.randn(C, C, 3, 3, generator=g) * 0.3, torch.randn(C, C, 3, 3, generator=g) * 0.3
    gy = [torch.randn(B * h * w, C, generator=g) for _ in range(2)] + [torch.randn(B * h * w, 4, generator=g) * 0.01]
    return dict(B=B, h=h, w=w, C=C, raw0=raw0, scale=scale, xr=xr, xc=xc, wr=wr, wc=wc, gy=gy)


def chain_reference(c, dtype):
    """the torch restatement of the chain in `dtype`: outputs and the gradients of sum(y_reg g0) + sum(y_cls g1) + sum(D0 g2)"""
    B, h, w, C = c['B'], c['h'], c['w'], c['C']
    leaf = lambda t: t.to(dtype).clone().requires_grad_()       # noqa: E731
    raw0, xr, xc, wr, wc = leaf(c['raw0']), leaf(c['xr']), leaf(c['xc']), leaf(c['wr']), leaf(c['wc'])
    sc = torch.tensor([c['scale']], dtype=dtype, requires_grad=True)
    d0, off, yr, yc = R.star_chain([raw0.view(B, h, w, 4)], sc, [xr.view(B, h, w, C)], [xc.view(B, h, w, C)], wr, wc, [8], [64.0],
                                   vi.GRADIENT_MUL)[0]
    g0, g1, g2 = (t.to(dtype) for t in c['gy'])
    (yr.reshape(-1, C) * g0).sum().add((yc.reshape(-1, C) * g1).sum()).add((d0.reshape(-1, 4) * g2).sum()).backward()
    return dict(off=off.detach(), yr=yr.detach().reshape(-1, C), yc=yc.detach().reshape(-1, C), draw0=raw0.grad, dscale=sc.grad,
                dxr=xr.grad, dxc=xc.grad, dwr=wr.grad, dwc=wc.grad)


def test_star_dconv_chain_against_float64():
    """raw0 -> D0, offsets (brcnn_vfnet_star_offsets) -> relu(DCN v1) of both towers on the fp32 route (im2col + GEMM), with
    the gradients w.r.t. raw0, the scale, both inputs and both weights; each held to 4 x the float32-vs-float64 gap of the
    restatement (see the header).  Preconditions: every one of the nine star points lies inside the map for some cell, beyond
    each of the four borders (but within the ring where it is still sampled) for another, and beyond -1 / H or W for a third;
    no coordinate that depends on a distance within 0.1 of an integer (the kink of the bilinear gradient)"""
    c = chain_inputs()
    B, h, w, C = c['B'], c['h'], c['w'], c['C']
    r64, r32 = chain_reference(c, torch.float64), chain_reference(c, torch.float32)
    p = R.sample_points(r64['off'])
    assert R.integer_margin(r64['off']) > 0.1
    y, x = p[..., 0], p[..., 1]
    for t in range(9):
        yt, xt = y[..., t], x[..., t]
        assert ((yt >= 0) & (yt <= h - 1) & (xt >= 0) & (xt <= w - 1)).any(), t
        if t // 3 == 0:
            assert ((yt > -1) & (yt < 0)).any() and (yt < -1).any(), t
        if t // 3 == 2:
            assert ((yt > h - 1) & (yt < h)).any() and (yt > h).any(), t
        if t % 3 == 0:
            assert ((xt > -1) & (xt < 0)).any() and (xt < -1).any(), t
        if t % 3 == 2:
            assert ((xt > w - 1) & (xt < w)).any() and (xt > w).any(), t
    head = build(4, in_channels=C, feat_channels=C, norm_cfg=dict(type='GN', num_groups=2, requires_grad=True))
    with torch.no_grad():
        head.vfnet_reg_refine_dconv.weight.copy_(c['wr'])
        head.vfnet_cls_dconv.weight.copy_(c['wc'])
    sizes = [(h, w)]
    r0 = padded(c['raw0'], 8, 0, 0.0).requires_grad_()
    sc = dev([c['scale']]).requires_grad_()
    xr, xc = c['xr'].to(DEV).requires_grad_(), c['xc'].to(DEV).requires_grad_()
    d0, offs = train_ops.vfnet_star_offsets(r0, sc, B, sizes, [8], [64.0], vi.GRADIENT_MUL)
    yr = head._star_dconv_fused(xr, offs, head.vfnet_reg_refine_dconv, B, sizes)
    yc = head._star_dconv_fused(xc, offs, head.vfnet_cls_dconv, B, sizes)
    g0, g1, g2 = (t.to(DEV) for t in c['gy'])
    ((yr * g0).sum() + (yc * g1).sum() + (d0 * g2).sum()).backward()
    got = dict(yr=yr, yc=yc, draw0=r0.grad[:, :4], dscale=sc.grad, dxr=xr.grad, dxc=xc.grad,
               dwr=head.vfnet_reg_refine_dconv.weight.grad, dwc=head.vfnet_cls_dconv.weight.grad)
    assert float(r0.grad[:, 4:].abs().max()) == 0
    for k, v in got.items():
        gap = float((r32[k].double() - r64[k]).abs().max())
        err = float((v.detach().cpu().double() - r64[k]).abs().max())
        print(f'{k}: float32 restatement vs float64 {gap:.2e}, kernels vs float64 {err:.2e}, largest value '
              f'{float(r64[k].abs().max()):.3g}')
        assert gap > 0 and err <= 4 * gap, (k, err, gap)
    # inference route on the same inputs: the rows form, ReLU in the GEMM's read-out
    with torch.no_grad():
        d0i, off = ops.vfnet_star_offsets(r0.detach(), sc.detach(), B, sizes, [8], [64.0], vi.GRADIENT_MUL)
        yi = head._star_dconv_rows(xr.detach(), off, head.vfnet_reg_refine_dconv, head._vf_caches['refine_dconv'], B, sizes)
    assert torch.equal(d0i, d0.detach()) and torch.equal(off, torch.cat([o.reshape(-1, 18) for o in offs]).detach())
    gap = float((r32['yr'].double() - r64['yr']).abs().max())
    assert float((yi.cpu().double() - r64['yr']).abs().max()) <= 4 * gap


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_ordered_col2im_keeps_its_bits(dtype):
    """the integer-accumulated input gradient of the deformable im2col (brcnn_deform_col2im_nhwc_ordered), on a map whose
    samples pile onto few pixels (offsets of up to 3 cells on a 6 x 7 map, 64 channels): the same bits from run to run; the
    offset gradient is the fp32-atomics entry's bit for bit; dx agrees with that entry's to the order of its additions (16
    eps of the sum of the contributions' magnitudes) plus the grid: m 2^-S per contribution, S = 62 - ceil(log2(6 * 7 * 9 *
    4)) = 51, at most 2 x 42 x 9 x 4 contributions per element; a dcol that is not finite turns dx into NaN"""
    g = torch.Generator().manual_seed(31)
    x = torch.randn(2, 6, 7, 64, generator=g).to(dtype).to(DEV)
    om = (torch.randn(2, 6, 7, 18, generator=g) * 3).to(DEV)
    dcol = torch.randn(2 * 6 * 7, 9 * 64, generator=g).to(DEV)
    dx0, dom0 = ops.deform_col2im_nhwc(x, om, dcol, 1, 1, 1, False)
    dx1, dom1 = ops.deform_col2im_nhwc(x, om, dcol, 1, 1, 1, False, ordered=True)
    dx2, dom2 = ops.deform_col2im_nhwc(x, om, dcol, 1, 1, 1, False, ordered=True)
    assert torch.equal(dx1, dx2) and torch.equal(dom1, dom2) and torch.equal(dom1, dom0)
    mag, _ = ops.deform_col2im_nhwc(x, om, dcol.abs(), 1, 1, 1, False)
    grid = 2 * 6 * 7 * 9 * 4 * float(dcol.abs().max()) * 2.0 ** -51
    assert ((dx1 - dx0).abs() <= 16 * EPS32 * mag + grid).all() and float(dx1.abs().max()) > 0
    bad = dcol.clone()
    bad[:, 70] = float('inf')                # channel 6 of tap 1 of every output pixel: some of those samples lie inside
    dxb, _ = ops.deform_col2im_nhwc(x, om, bad, 1, 1, 1, False, ordered=True)
    assert bool(torch.isnan(dxb).all())
    bad[:, 70] = 3e38                        # finite and huge: nothing saturates, the grid follows the largest dcol
    dxh, _ = ops.deform_col2im_nhwc(x, om, bad, 1, 1, 1, False, ordered=True)
    dxa, _ = ops.deform_col2im_nhwc(x, om, bad, 1, 1, 1, False)
    ok = torch.isfinite(dxa)                 # (a sum of several 3e38 overflows fp32 itself in either entry)
    assert bool(torch.isfinite(dxh[ok]).all()) and float((dxh[ok] - dxa[ok]).abs().max()) <= 16 * EPS32 * 4 * 3e38


def _col2im_float64(om, dcol, B, H, W, C):
    """the float64 input gradient of the DCN v1 im2col by autograd through tests/vfnet_ref64.deform_conv_v1 with a one-hot
    weight (output (tap, c) = column (tap, c)), and the sum of the magnitudes of the contributions of each element"""
    w = torch.zeros(9 * C, C, 3, 3, dtype=torch.float64)
    for t in range(9):
        for c in range(C):
            w[t * C + c, c, t // 3, t % 3] = 1
    out = []
    for d in (dcol.double(), dcol.double().abs()):
        x = torch.zeros(B, H, W, C, dtype=torch.float64, requires_grad=True)
        (R.deform_conv_v1(x, om.double(), w).reshape(-1, 9 * C) * d).sum().backward()
        out.append(x.grad)
    return out


COL2IM_SCALES = [('unit', 0.0, 0.0), ('all at 1e-9', -9.0, -9.0), ('rows over ten decades', -10.0, 0.0)]


@pytest.mark.parametrize('name,lo,hi', COL2IM_SCALES, ids=[c[0] for c in COL2IM_SCALES])
def test_ordered_col2im_against_float64_at_small_gradients(name, lo, hi):
    """fp32 x, dcol rows scaled by 10^u, u uniform in [lo, hi]: gradients of the size a loss divided by the number of
    positives leaves on background cells (1e-9 .. 1e-10), alone and beside rows of size 1 in the same call.  The offsets are
    multiples of 1 / 64, so the sample coordinates, the bilinear fractions and the corner weights (12 bits) are exact in
    fp32 and in the float64 reference alike.  A contribution dcol * weight then rounds once (0.5 eps of itself), the integer
    additions are exact, the conversion of the sum rounds once more (0.5 eps of at most the sum of the magnitudes): each
    element of dx within 1 eps of the sum of the magnitudes of its contributions, plus the grid, m 2^-S per contribution (m =
    max |dcol|, S = 51 on this 6 x 7 map, at most 6 x 7 x 9 x 4 = 1512 contributions of an image per element): 1512 m 2^-51.
    With every row at 1e-9 the grid term is 7e-22 against sums of 1e-9, so the relative precision is fp32's on every
    element (asserted); with rows over ten decades it is 7e-13 of the largest dcol.  The fp32-atomics entry's error is
    printed beside it"""
    g = torch.Generator().manual_seed(33)
    B, H, W, C = 2, 6, 7, 8
    x = torch.randn(B, H, W, C, generator=g).to(DEV)
    om = torch.randint(-192, 193, (B, H, W, 18), generator=g).float() / 64
    scale = 10.0 ** (torch.rand(B * H * W, 1, generator=g) * (hi - lo) + lo)
    dcol = (torch.randn(B * H * W, 9 * C, generator=g) * scale).float()
    ref, mag = _col2im_float64(om, dcol, B, H, W, C)
    dxo, _ = ops.deform_col2im_nhwc(x, om.to(DEV).contiguous(), dcol.to(DEV).contiguous(), 1, 1, 1, False, ordered=True)
    dxa, _ = ops.deform_col2im_nhwc(x, om.to(DEV).contiguous(), dcol.to(DEV).contiguous(), 1, 1, 1, False)
    m = float(dcol.abs().max())
    grid = H * W * 9 * 4 * m * 2.0 ** -51
    err_o, err_a = (dxo.cpu().double() - ref).abs(), (dxa.cpu().double() - ref).abs()
    assert (err_o <= EPS32 * mag + grid).all(), (float((err_o - EPS32 * mag).max()), grid)
    assert float(mag.max()) > 0 and grid <= 1e-12 * m
    if lo == hi:
        assert grid <= 1e-3 * EPS32 * float(mag[mag > 0].min())          # fp32's relative precision on every element
    small = (mag > 0) & (mag < 1e-6 * m)
    print(f'{name}: max |dcol| {m:.3g}, grid term {grid:.3g}, elements below 1e-6 of it: {int(small.sum())}, worst error / (eps mag) '
          f'there: ordered {float((err_o[small] / (EPS32 * mag[small])).max()) if small.any() else 0:.3g}, fp32 atomics '
          f'{float((err_a[small] / (EPS32 * mag[small])).max()) if small.any() else 0:.3g}; everywhere: ordered '
          f'{float((err_o[mag > 0] / (EPS32 * mag[mag > 0])).max()):.3g}, fp32 atomics {float((err_a[mag > 0] / (EPS32 * mag[mag > 0])).max()):.3g}')


# ------------------------------------------------------------------------------------------- test time
DECODE_CASES =[(4, False, False), (1, False, True), (4, True, True), (1, True, False)]


@pytest.mark.parametrize('C,wide,rescale', DECODE_CASES)
def test_candidates_against_float64(C, wide, rescale):
    """every cell of every level is picked, in descending index order.  D1 = exp(z) * D0 within (0.5 |z| + 2.5) eps (see the
    offsets test); a coordinate p -+ d rounds once more (0.5 eps of itself); the clip changes nothing; the division by the
    scale factor divides the error and rounds once: |box - ref| <= ((0.5 |z| + 2.5) d + 0.5 |c|) eps / sf + 0.5 eps |box|.
    The score is a sigmoid: 4 eps.  valid = score > thr is exact away from the threshold (asserted)"""
    seed, thr = 40 + C, 0.05
    cls, raw0, raw1 = vi.head_outputs(seed, C)
    d0l, d1l = vi.distances(raw0, raw1)
    metas = vi.metas()
    a0, r1, d0 = R._rows(cls).float(), R._rows(raw1).float(), R._rows(d0l).float().to(DEV).contiguous()
    a, r = (padded(a0, 16, 3), padded(r1, 8, 2)) if wide else (padded(a0, 8, 0, 0.0), padded(r1, 8, 0, 0.0))
    layout = ops.VfnetLayout(a, r, C, 3 if wide else 0, 2 if wide else 0)
    inds = [torch.arange(n - 1, -1, -1, device=DEV).repeat(2, 1) for n in N_L]
    shp = dev([m['img_shape'][:2] for m in metas])
    sf = dev(np.stack([m['scale_factor'] for m in metas]).tolist()) if rescale else None
    boxes, scores, labels, valid, n_valid = [t.cpu() for t in ops.vfnet_decode_levels(
        inds, a, r, d0, layout, dev(list(vi.SCALES_REFINE)), vi.SIZES, vi.STRIDES, base_table(), shp, sf, thr)]
    # the float64 distances from the same fp32 D0 the kernel reads
    d1_64 = [(x.double() * s).exp() * p.double() for x, s, p in zip(raw1, vi.SCALES_REFINE, d0l)]
    ref = R.candidates(cls, d1_64, vi.SIZES, vi.STRIDES, [m['img_shape'] for m in metas],
                       [m['scale_factor'] for m in metas] if rescale else None)
    t0, nv = 0, [0, 0]
    for l, n in enumerate(N_L):
        order = torch.arange(n - 1, -1, -1)
        sl = slice(t0 * C, (t0 + n) * C)
        for b in range(2):
            gb = boxes[b, sl].view(n, C, 4).double()
            rb = ref[l][2][b][order]
            z = (raw1[l][b].double() * vi.SCALES_REFINE[l]).permute(1, 2, 0).reshape(-1, 4)[order].abs().max(1)[0]
            d = d1_64[l][b].permute(1, 2, 0).reshape(-1, 4)[order].max(1)[0]
            smin = float(min(metas[b]['scale_factor'])) if rescale else 1.0
            # |c| <= |point| + d, a point lies inside the 128 x 192 input
            bound = ((0.5 * z + 2.5) * d + 0.5 * (d + vi.W)) * EPS32 / smin + 0.5 * EPS32 * rb.abs().max(1)[0]
            assert ((gb - rb[:, None]).abs().amax((1, 2)) <= bound).all(), (l, b)
            assert (gb[:, 0:1] == gb).all()                                                  # one box for all classes
            rs = ref[l][1][b][order]
            assert ((scores[b, sl].view(n, C).double() - rs).abs() <= 4 * EPS32).all()
            assert float((rs - thr).abs().min()) > 1e-6
            assert torch.equal(valid[b, sl].view(n, C), rs > thr)
            assert torch.equal(labels[b, sl].view(n, C), torch.arange(C).expand(n, C))
            nv[b] += int((rs > thr).sum())
        t0 += n
    assert n_valid.tolist() == nv and min(nv) > 0


# ------------------------------------------------------------------------------------------- loss
def test_one_positive_loss_by_hand():
    """one level of 2 x 2 cells, stride 8, one image, two classes, every logit 0.  Cell (1, 1) -- the point (8, 8) -- is
    positive for the box (2, 3, 18, 15) of class 1: target (6, 5, 10, 7).  D0 is the target: IoU 1, GIoU loss 0.  D1 = (3, 2,
    5, 4) gives (5, 6, 13, 12) strictly inside the target: IoU = 48 / 192 = 0.25, hull = target, GIoU loss 0.75.  loss_bbox
    = 0; loss_bbox_rf = 2 * (0.25 * 0.75) / max(0.25, 1) = 0.375; the class term: seven elements at 0.75 * 0.5^2 * ln 2 and
    the label at 0.25 * BCE(0, 0.25) = 0.25 ln 2: 1.5625 ln 2 over one positive"""
    sizes, strides = [(2, 2)], [8]
    a = torch.zeros(4, 8, device=DEV).requires_grad_()
    d0 = torch.tensor([[6., 5., 10., 7.]] * 4, device=DEV).requires_grad_()
    d1 = torch.tensor([[3., 2., 5., 4.]] * 4, device=DEV).requires_grad_()
    gt_inds = torch.tensor([[0, 0, 0, 1]], dtype=torch.int32, device=DEV)
    gts, labels = torch.tensor([[2., 3., 18., 15.]], device=DEV), torch.tensor([1], device=DEV)
    base = ops.atss_base_anchors([torch.tensor([[-8., -8., 8., 8.]])])
    meta = train_ops.VfnetLossMeta(1, sizes, strides, base, 2, [0, 1], 0.75, 2.0, True, 1e-6, 1.0, 1.5, 2.0)
    losses, coef, norm3 = train_ops.vfnet_loss(a, d0, d1, gt_inds, gts, labels, meta)
    assert norm3.tolist() == [1.0, 1.0, 0.25] and coef.tolist() == [1.0, 1.5, 2.0]
    ln2 = math.log(2.0)
    assert losses[1].item() == 0.0 and losses[2].item() == 0.375
    assert abs(losses[0].item() - 1.5625 * ln2) <= 16 * EPS32 * 1.5625 * ln2
    losses.sum().backward()
    # d / dx at x = 0: the label 0.25 * (0.5 - 0.25); elsewhere 0.75 * 0.25 * (0.5 + 2 * 0.5 * ln 2)
    want = torch.full((4, 8), 0.75 * 0.25 * (0.5 + ln2))
    want[:, 2:] = 0
    want[3, 1] = 0.0625
    assert torch.allclose(a.grad.cpu(), want, rtol=16 * EPS32, atol=0) and float(a.grad[:, 2:].abs().max()) == 0
    assert float(d0.grad[:3].abs().max()) == 0 and float(d1.grad[:3].abs().max()) == 0
    # box1 strictly inside the target: the loss is 1 - iou, iou = A / 192, A = (l + r)(t + b): dA/dl = 6, dA/dt = 8; times
    # the weight 0.25 and the coefficient 2 / 1
    assert torch.allclose(d1.grad[3].cpu(), -0.5 * torch.tensor([6., 8., 6., 8.]) / 192, rtol=16 * EPS32, atol=0)


def _loss_case(seed, C, gamma, iou_weighted, invalid, wide):
    cls, raw0, raw1 = vi.head_outputs(seed, C)
    d0, d1 = vi.distances(raw0, raw1)
    gt_bboxes, gt_labels = vi.gts(seed, num_classes=C)
    valid = None
    if invalid:
        valid = [[[min(math.ceil(p[0] / s), h), min(math.ceil(p[1] / s), w)] for (h, w), s in zip(vi.SIZES, vi.STRIDES)]
                 for p in PADS]
    inds = RA.assign(gt_bboxes, vi.SIZES, vi.STRIDES, vi.OCTAVE, vi.TOPK, valid_hws=valid, dtype=torch.float32)
    return dict(cls=cls, d0=d0, d1=d1, gts=gt_bboxes, labels=gt_labels, inds=inds, C=C, gamma=gamma, iw=iou_weighted, wide=wide,
                weights=(1.0, 1.5, 2.0), alpha=0.75)


def _run_loss(c, hook=None):
    a0 = R._rows(c['cls']).float()
    off = 3 if c['wide'] else 0
    a = (padded(a0, 16, 3) if c['wide'] else padded(a0, 8, 0, 0.0)).requires_grad_()
    d0, d1 = (R._rows(c[k]).float().to(DEV).contiguous().requires_grad_() for k in ('d0', 'd1'))
    gts, labels, offs = train_ops.flatten_gts([g.to(DEV) for g in c['gts']], [l.to(DEV) for l in c['labels']])
    gt_inds = torch.stack(c['inds']).to(torch.int32).to(DEV).contiguous()
    meta = train_ops.VfnetLossMeta(2, vi.SIZES, vi.STRIDES, base_table(), c['C'], offs, c['alpha'], c['gamma'], c['iw'], 1e-6,
                                   *c['weights'])
    losses, coef, norm3 = train_ops.vfnet_loss(a, d0, d1, gt_inds, gts.to(DEV), labels.to(DEV), meta, off, hook)
    losses.sum().backward()
    return dict(losses=losses.detach().cpu().double(), coef=coef.cpu().double(), norm3=norm3.cpu().double(),
                da=a.grad.cpu().double(), dd0=d0.grad.cpu().double(), dd1=d1.grad.cpu().double(), off=off)


def _box_bounds(b, t):
    """per positive, the fp32 error of the IoU and of the GIoU loss of box b against target t (float64 (P, 4)).  A coordinate
    p -+ d rounds once: 0.5 eps M, M the largest coordinate of the pair.  An extent (a side of either box, of the
    intersection, of the hull) is a difference of two: 1.5 eps M.  A product of two extents u v, both at most E (the longer
    hull side): 1.5 eps M (u + v) + 0.5 eps u v <= 3.5 eps M E =: dA.  union = a1 + a2 - inter: 3 dA + eps U.  iou = inter /
    union with inter <= U: dA / U + (3 dA + eps U) / U + 0.5 eps <= 4 dA / U + 1.5 eps.  (hull - union) / hull with hull >=
    U: (4 dA + 2 eps hull) / hull + 1 eps <= 4 dA / U + 3 eps.  The loss 1 - (iou - that) adds 1.5 eps of values below 2"""
    M = torch.cat([b, t], 1).abs().max(1)[0]
    E = (torch.maximum(b[:, 2:], t[:, 2:]) - torch.minimum(b[:, :2], t[:, :2])).max(1)[0]
    wh = (torch.minimum(b[:, 2:], t[:, 2:]) - torch.maximum(b[:, :2], t[:, :2])).clamp(min=0)
    area = lambda v: (v[:, 2] - v[:, 0]) * (v[:, 3] - v[:, 1])       # noqa: E731
    U = (area(b) + area(t) - wh[:, 0] * wh[:, 1]).clamp(min=1e-6)
    dA = 3.5 * EPS32 * M * E
    return 4 * dA / U + 1.5 * EPS32, 8 * dA / U + 7.5 * EPS32


def _check_loss(c, got, ref, ref32):
    """loss values and dA against derived bounds, dD0 / dD1 against 4 x the float32-vs-float64 gap of the restatement plus
    the normaliser's relative error on the element itself.
    Sums: eight sequential additions per thread, a tree of 8 levels, the partials of a level by the same scheme, five levels:
    40 eps of the sum of absolute terms covers any order.
    Class term off the label, alpha p^gamma softplus(x): the sigmoid carries 4 eps, its power gamma times that + 2, the
    softplus (no cancellation) 5, the two products 1: (4 gamma + 12) eps; at the label q BCE(x, q) with q the clamped IoU of
    the refined box: the IoU's error times |d / dq| <= |BCE| + |x|, and BCE's own arithmetic ((1 - q) x - log sigmoid(x), each
    part within 5 eps of |x| + 1) 8 eps (|x| + 1).
    The derivative off the label alpha p^gamma (p + gamma (1 - p) softplus): (4 gamma + 16) eps of alpha p^gamma (p + gamma
    softplus) (1 - p's error is p's); at the label q (p - q): the IoU's error times (|p - q| + q) + 6 eps.  A coefficient
    lw / max(norm, 1) carries the error of its normaliser + 1 eps; n_pos is exact"""
    P, gm, al = ref['n_pos'], c['gamma'], c['alpha']
    assert P > 5 and float(ref['w_rf'].min()) > 1e-4 and float(ref['w_ini'].min()) > 1e-4       # no IoU at the 1e-6 clamp
    n3 = ref['norm3']
    di0, dg0 = _box_bounds(ref['boxes0'], ref['target_boxes'])
    di1, dg1 = _box_bounds(ref['boxes1'], ref['target_boxes'])
    dS = [0.0, float(di0.sum()) + 40 * EPS32 * n3[1], float(di1.sum()) + 40 * EPS32 * n3[2]]
    assert got['norm3'][0] == P
    for k in (1, 2):
        assert abs(float(got['norm3'][k]) - n3[k]) <= dS[k], k
    N, S = max(n3[0], 1.0), [None, max(n3[1], 1.0), max(n3[2], 1.0)]
    lw = c['weights']
    # class loss
    x = ref['x_hit'].abs()
    hit_err = di1 * (ref['bce_hit'].abs() + x) * (1.0 if c['iw'] else 0.0) + 8 * EPS32 * (x + 1)
    if not c['iw']:
        hit_err = hit_err + di1 * x                                               # BCE(x, q) alone: d / dq = -x
    tol = lw[0] / N * ((4 * gm + 12 + 40) * EPS32 * ref['neg_abs'] + float(hit_err.sum()) + 40 * EPS32 * ref['hit_abs']) + \
        3 * EPS32 * abs(float(ref['losses'][0]))
    assert abs(float(got['losses'][0]) - float(ref['losses'][0])) <= tol, ('loss_cls', got['losses'][0], ref['losses'][0], tol)
    # box losses
    for k, (w, gi, di, dg) in enumerate(((ref['w_ini'], ref['giou0'], di0, dg0), (ref['w_rf'], ref['giou1'], di1, dg1)), 1):
        terms = (w * gi)
        err = float((di * gi.abs() + w * dg + EPS32 * terms.abs()).sum()) + 40 * EPS32 * float(terms.abs().sum())
        val = float(ref['losses'][k])
        tol = lw[k] / S[k] * err + abs(val) * (dS[k] / S[k] + 3 * EPS32)
        assert abs(float(got['losses'][k]) - val) <= tol, (k, got['losses'][k], val, tol)
        assert abs(float(got['coef'][k]) - lw[k] / S[k]) <= lw[k] / S[k] * (dS[k] / S[k] + 2 * EPS32)
    assert float(got['coef'][0]) == np.float32(lw[0]) / np.float32(N)
    # dA
    off, C = got['off'], c['C']
    da = got['da']
    assert float(da[:, :off].abs().max() if off else 0) == 0 and float(da[:, off + C:].abs().max()) == 0
    want = torch.cat([t.permute(0, 2, 3, 1).reshape(-1, C) for t in ref['dcls']])
    p, sp = ref['sigmoid'], ref['softplus']
    bound = (4 * gm + 16 + 2) * EPS32 * lw[0] / N * al * p.pow(gm) * (p + gm * sp)
    q = ref['w_rf']
    ph = p[ref['pos'], ref['labels']]
    hb = lw[0] / N * (di1 * ((ph - q).abs() + q) + 6 * EPS32) if c['iw'] else lw[0] / N * (di1 + 6 * EPS32)
    bound[ref['pos'], ref['labels']] = hb + 2 * EPS32 * want[ref['pos'], ref['labels']].abs()
    assert ((da[:, off:off + C] - want).abs() <= bound).all()
    # dD0 / dD1
    for k, name in ((1, 'dd0'), (2, 'dd1')):
        w64 = torch.cat([t.permute(0, 2, 3, 1).reshape(-1, 4) for t in ref[name]])
        w32 = torch.cat([t.permute(0, 2, 3, 1).reshape(-1, 4) for t in ref32[name]]).double()
        gap = float((w32 - w64).abs().max())
        err = (got[name] - w64).abs()
        # the factor grad * coef * weight of a row carries the error of its normaliser (dS / S, above) and of the sum behind
        # it (40 eps), which one run of the restatement does not sample: that much of the ELEMENT itself on top
        bound = 4 * gap + (40 * EPS32 + dS[k] / S[k]) * w64.abs()
        print(f'{name}: float32 restatement vs float64 {gap:.2e}, kernel vs float64 {float(err.max()):.2e}, largest '
              f'{float(w64.abs().max()):.3g}, normaliser term {40 * EPS32 + dS[k] / S[k]:.2e} of the element')
        assert gap > 0 and (err <= bound).all(), (name, float((err - bound).max()), gap)
        zero = torch.ones(len(w64), dtype=torch.bool)
        zero[ref['pos']] = False
        assert float(got[name][zero].abs().max()) == 0                             # exact zeros off the positives


LOSS_CASES = [(4, 2.0, True), (4, 1.5, True), (1, 2.0, False)]


@pytest.mark.parametrize('invalid', [False, True], ids=['all valid', 'invalid cells'])
@pytest.mark.parametrize('C,gamma,iou_weighted', LOSS_CASES)
def test_loss_and_gradients_against_float64(C, gamma, iou_weighted, invalid):
    c = _loss_case(50 + C, C, gamma, iou_weighted, invalid, wide=(gamma == 1.5))
    kw = dict(alpha=c['alpha'], gamma=gamma, iou_weighted=iou_weighted, weights=c['weights'])
    ref = R.loss(c['cls'], c['d0'], c['d1'], c['inds'], c['gts'], c['labels'], vi.SIZES, vi.STRIDES, **kw)
    ref32 = R.loss(c['cls'], c['d0'], c['d1'], c['inds'], c['gts'], c['labels'], vi.SIZES, vi.STRIDES, dtype=torch.float32, **kw)
    if invalid:
        assert any(bool((i < 0).any()) for i in c['inds'])
    _check_loss(c, _run_loss(c), ref, ref32)


def test_loss_without_positives_is_exactly_zero():
    c = _loss_case(7, 4, 2.0, True, False, False)
    c['gts'], c['labels'] = [torch.zeros(0, 4)] * 2, [torch.zeros(0, dtype=torch.long)] * 2
    c['inds'] = [torch.zeros(vi.ANCHORS, dtype=torch.long)] * 2
    got = _run_loss(c)
    assert got['losses'][1] == 0 and got['losses'][2] == 0 and got['losses'][0] > 0
    assert got['norm3'].tolist() == [0.0, 0.0, 0.0] and got['coef'].tolist() == [1.0, 1.5, 2.0]
    assert float(got['dd0'].abs().max()) == 0 and float(got['dd1'].abs().max()) == 0 and float(got['da'].abs().max()) > 0


def test_finalize_with_normalisers_averaged_by_hand():
    """`norm_hook` stands where the mean over ranks would: each loss scales by max(own, 1) / max(averaged, 1)"""
    c = _loss_case(54, 4, 2.0, True, False, False)
    plain = _run_loss(c)
    new = [plain['norm3'][0].item() * 0.5 + 1, plain['norm3'][1].item() * 2, 0.25]

    def hook(n3):
        n3.copy_(torch.tensor(new, device=n3.device))
    got = _run_loss(c, hook)
    for k in range(3):
        ratio = max(float(plain['norm3'][k]), 1.0) / max(new[k], 1.0)
        assert abs(float(got['losses'][k]) - float(plain['losses'][k]) * ratio) <= 8 * EPS32 * abs(float(got['losses'][k]))


def test_loss_is_bit_reproducible():
    c = _loss_case(54, 4, 2.0, True, True, True)
    x, y = _run_loss(c), _run_loss(c)
    assert all(torch.equal(x[k], y[k]) for k in ('losses', 'coef', 'norm3', 'da', 'dd0', 'dd1'))


# ------------------------------------------------------------------------------------------- the fixture
CASES = [(4, 'plain'), (4, 'rescale'), (4, 'empty'), (1, 'plain'), (1, 'rescale')]


def _split_cfg(cfg, thr):
    if thr:
        cfg['test_cfg']['nms'] = dict(cfg['test_cfg']['nms'], split_thr=thr)
    return cfg


def _force_form(monkeypatch, form):
    """'torch': `batched_nms_images_by_level` in its form for more than 16 384 slots"""
    if form == 'torch':
        import functools

        from brcnn import postprocess
        monkeypatch.setattr(postprocess, 'batched_nms_images_by_level',
                            functools.partial(postprocess.batched_nms_images_by_level, fused=False))


def _check_dets(res, gold, C, name, what):
    for b, (det, lab) in enumerate(res):
        want_d, want_l = T(gold[f'bboxes_c{C}_{name}_det{b}']), T(gold[f'bboxes_c{C}_{name}_lab{b}'])
        assert lab.cpu().tolist() == want_l.tolist(), (C, name, what, b)
        assert det.shape == want_d.shape and torch.allclose(det.cpu(), want_d, rtol=0, atol=2e-4), (C, name, what, b)


@pytest.mark.parametrize('form', ['offset', 'fused', 'torch'])
@pytest.mark.parametrize('C,name', CASES)
def test_get_bboxes_golden(gold, monkeypatch, C, name, form):
    """the reference-signature get_bboxes on device tensors against the reference's detections: labels and order exact,
    boxes and scores within 2e-4; on the offset NMS branch and, with split_thr = 100, on the per-class branch in both forms"""
    _force_form(monkeypatch, form)
    seed = int(gold[f'seed_bboxes_c{C}'])
    head = build(C, **_split_cfg(dict(test_cfg=dict(vi.TEST_CFG)), 0 if form == 'offset' else 100)).eval()
    cls, raw0, raw1 = vi.head_outputs(seed, C, empty=(name == 'empty'))
    d0, d1 = vi.distances(raw0, raw1)
    dv = lambda lst: [t.to(DEV) for t in lst]    # noqa: E731
    res = head.get_bboxes(dv(cls), dv(d0), dv(d1), vi.metas(), rescale=(name != 'plain'))
    _check_dets(res, gold, C, name, form)
    if name == 'empty':
        assert head.last_n_valid.tolist()[1] == 0 and len(res[1][0]) == 0 and len(res[0][0]) > 0


@pytest.mark.parametrize('C,name', CASES)
def test_get_bboxes_rows_golden(gold, C, name):
    """the fused-row form: RAW refinement rows and D0 as the head's own convs and kernels leave them, the live
    scales_refine applied in the decode kernel"""
    seed = int(gold[f'seed_bboxes_c{C}'])
    head = build(C).eval()
    cls, raw0, raw1 = vi.head_outputs(seed, C, empty=(name == 'empty'))
    d0l, _ = vi.distances(raw0, raw1)
    a, r1 = padded(R._rows(cls).float(), 8, 0, 0.0), padded(R._rows(raw1).float(), 8, 0, 0.0)
    d0 = R._rows(d0l).float().to(DEV).contiguous()
    det, lab, num = head.get_bboxes_rows(a, r1, head._layout(a, r1, d0), head._scales_refine_tensor(), vi.SIZES, vi.metas(),
                                         rescale=(name != 'plain'))
    num = num.tolist()
    _check_dets([(det[b, :num[b]], lab[b, :num[b]]) for b in range(2)], gold, C, name, 'rows')


@pytest.mark.parametrize('tag,C,pads', [('loss_c4', 4, None), ('loss_c1', 1, None), ('loss_pad', 4, PADS)])
def test_loss_on_device_tensors_golden(gold, tag, C, pads):
    """the reference-signature loss on device tensors (assignment + loss kernels behind it) against the reference's values
    at the train iterations' tolerance, and its gradients"""
    seed = int(gold[f'seed_{tag}'])
    head = build(C, True)
    cls, raw0, raw1 = vi.head_outputs(seed, C)
    d0, d1 = vi.distances(raw0, raw1)
    gt_bboxes, gt_labels = vi.gts(seed, num_classes=C)
    dv = lambda lst: [t.detach().to(DEV).requires_grad_() for t in lst]    # noqa: E731
    cls, d0, d1 = dv(cls), dv(d0), dv(d1)
    losses = head.loss(cls, d0, d1, [g.to(DEV) for g in gt_bboxes], [l.to(DEV) for l in gt_labels], vi.metas(pads=pads))
    assert sorted(losses) == ['loss_bbox', 'loss_bbox_rf', 'loss_cls']
    for k, v in losses.items():
        assert torch.allclose(v.detach().cpu(), T(gold[f'{tag}_{k}']), rtol=2e-3, atol=1e-4), (k, v, gold[f'{tag}_{k}'])
    sum(losses.values()).backward()
    if tag == 'loss_c4':
        for l in range(L):
            for name, t in (('dcls', cls), ('dd0', d0), ('dd1', d1)):
                g = T(gold[f'{tag}_{name}{l}'])
                assert torch.allclose(t[l].grad.cpu(), g, rtol=2e-3, atol=1e-6), (name, l)


def test_invalid_cells_count_as_negatives(gold):
    """only pad_shape differs between the two calls: loss_cls moves from the fixture's one value to the other"""
    seed = int(gold['seed_loss_c4'])
    assert seed == int(gold['seed_loss_pad'])
    head = build(4, True)
    cls, raw0, raw1 = vi.head_outputs(seed, 4)
    d0, d1 = vi.distances(raw0, raw1)
    gt_bboxes, gt_labels = vi.gts(seed)
    dv = lambda lst: [t.to(DEV) for t in lst]    # noqa: E731
    out = {}
    for tag, pads in (('loss_c4', None), ('loss_pad', PADS)):
        out[tag] = head.loss(dv(cls), dv(d0), dv(d1), dv(gt_bboxes), dv(gt_labels), vi.metas(pads=pads))['loss_cls'].item()
        assert abs(out[tag] - float(gold[f'{tag}_loss_cls'])) <= 2e-3 * float(gold[f'{tag}_loss_cls']) + 1e-4
        if pads:
            assert (head.last_targets[0][1] < 0).any()
    assert abs(out['loss_c4'] - out['loss_pad']) > 1e-3 * out['loss_c4']


def _seeded_head(seed, C=4):
    head = build(C)
    head.load_state_dict(vi.seeded_head_state(head, seed))
    return head.eval()


def test_forward_on_device_golden(gold):
    """the head's forward on the seeded pyramid through the device path (towers, fused heads, star offsets, DCN v1 im2col +
    GEMM) against the reference's fp32 run.  Class logits are O(1) sums of 576 products: held to the 2e-4 the boxes of the
    other sections are held to; the distances are exp() of such a sum times the denominator: 2e-4 relative"""
    seed = int(gold['seed_forward'])
    head = _seeded_head(seed)
    with torch.no_grad():
        cls, d0, d1 = head([f.to(DEV) for f in vi.features(seed)])
    for l in range(L):
        assert torch.allclose(cls[l].cpu(), T(gold[f'fwd_cls{l}']), rtol=0, atol=2e-4), l
        assert torch.allclose(d0[l].cpu(), T(gold[f'fwd_d0{l}']), rtol=2e-4, atol=0), l
        assert torch.allclose(d1[l].cpu(), T(gold[f'fwd_d1{l}']), rtol=2e-4, atol=0), l


def test_forward_gradient_through_the_offsets_golden(gold):
    """the small map of the fixture whose star coordinates keep 1e-3 from the integers: outputs and the gradient w.r.t. the
    map through towers, offsets and both deformable convs, at the tolerance of the train losses"""
    seed = int(gold['seed_forward_grad'])
    head = _seeded_head(seed).train()
    x = vi.small_feature(seed).permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_()         # NHWC, a leaf
    # the device path runs all five levels in one launch per layer; the levels do not mix (GroupNorm statistics are per
    # level and image), so the small map rides as level 0 of a pyramid of seeded fillers
    g = torch.Generator().manual_seed(seed)
    fill = [torch.randn(1, h, w, 64, generator=g).to(DEV) for h, w in ((3, 4), (2, 2), (1, 2), (1, 1))]
    cls, d0, d1 = head.forward_nhwc([x] + fill)
    (cls[0].sum() + d1[0].log().sum()).backward()
    nhwc = lambda k: T(gold[k]).permute(0, 2, 3, 1)        # noqa: E731
    assert torch.allclose(cls[0].detach().cpu(), nhwc('fgrad_cls'), rtol=0, atol=2e-4)
    assert torch.allclose(d1[0].detach().cpu(), nhwc('fgrad_d1'), rtol=2e-4, atol=0)
    g = nhwc('fgrad_dx')
    assert float((x.grad.cpu() - g).abs().max()) <= 2e-3 * float(g.abs().max())


def _table(res):
    return np.concatenate([np.concatenate([r, np.full((len(r), 1), c, np.float32)], 1) for c, r in enumerate(res)], 0)


def _model(seed, split_thr=0):
    m = build_detector(ConfigDict(_split_cfg(vi.fixture_model_cfg(), split_thr)))
    m.load_state_dict(vi.fixture_state_dict(m, seed))
    return m.to(DEV)


@pytest.mark.parametrize('form', ['offset', 'fused', 'torch'])
def test_model_end_to_end_golden(gold, monkeypatch, form):
    """`model(return_loss=False)` against the reference's run of the same seeded model: per class the same detections in
    the same order, labels exact, boxes and scores within 2e-4 (the fixture's reference run is within 5e-5 of its own
    float64 run).  `simple_test_device` runs under torch's synchronisation debug mode on 'error': the one host read of an
    inference call is the result copy."""
    _force_form(monkeypatch, form)
    seed = int(gold['seed_e2e'])
    m = _model(seed, 0 if form == 'offset' else 100).eval()
    img, _, _, _ = util.demo_inputs(2, vi.H, vi.W, seed=seed)
    img = img.to(DEV)
    with torch.no_grad():
        res = m(return_loss=False, rescale=True, img=[img], img_metas=[vi.metas()])
        assert len(m.last_n_valid) == 2 and all(n >= sum(len(r) for r in res[b]) > 0 for b, n in enumerate(m.last_n_valid))
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            det, lab, nd = m.simple_test_device(img, vi.metas(), rescale=True)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    assert float(gold['e2e_ref_err']) <= 5e-5
    assert nd.tolist() == [sum(len(r) for r in res[b]) for b in range(2)]
    for b in range(2):
        assert len(res[b]) == 4 and all(r.dtype == np.float32 and r.shape[1] == 5 for r in res[b])
        got, ref = _table(res[b]), gold[f'e2e_res{b}']
        assert got.shape == ref.shape and np.array_equal(got[:, 5], ref[:, 5]), (form, b)
        print('image', b, 'largest box / score difference', float(np.abs(got[:, :5] - ref[:, :5]).max()))
        assert np.allclose(got[:, :5], ref[:, :5], rtol=0, atol=2e-4), (form, b, np.abs(got[:, :5] - ref[:, :5]).max())


def _train_batch(seed):
    img, _, _, _ = util.demo_inputs(2, vi.H, vi.W, seed=seed, num_gt=vi.TRAIN_NUM_GT)
    gts, gls = vi.gts(seed)
    return img.to(DEV), [g.to(DEV) for g in gts], [l.to(DEV) for l in gls]


def test_no_host_read_in_the_head_train_step(gold):
    """`bbox_head.forward_train_nhwc` under torch's synchronisation debug mode on 'error': any blocking host read raises.
    The second image's pad_shape is smaller than the batch pad, so the valid-cell table is part of the step"""
    m = _model(int(gold['seed_e2e'])).train()
    img, gts, gls = _train_batch(int(gold['seed_train0']))
    feats = [f.detach() for f in m.extract_feat_nhwc(img)]
    metas = vi.metas(2, pads=[(vi.H, vi.W), (vi.H - 32, vi.W - 64)])
    m.bbox_head.forward_train_nhwc(feats, metas, gts, gls)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        losses = m.bbox_head.forward_train_nhwc(feats, metas, gts, gls)
        total = torch.stack(list(losses.values())).sum()
        total.backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert math.isfinite(float(total.detach()))
    ind = m.bbox_head.last_targets[0].cpu()
    assert (ind[0] >= 0).all() and (ind[1] == -1).any() and (ind[1] > 0).any()


def test_two_train_iterations_golden(gold):
    m = _model(int(gold['seed_e2e'])).train()
    for it in range(2):
        img, gts, gls = _train_batch(int(gold[f'seed_train{it}']))
        losses = m(img=img, img_metas=vi.metas(), gt_bboxes=gts, gt_labels=gls)
        assert sorted(losses) == ['loss_bbox', 'loss_bbox_rf', 'loss_cls']
        for k, v in losses.items():
            got, ref = v.detach().cpu().double().reshape(-1), T(gold[f'train{it}_{k}']).double().reshape(-1)
            assert torch.allclose(got, ref, rtol=2e-3, atol=1e-4), (it, k, got, ref)
        loss, log_vars = m._parse_losses(losses)
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for n, p in m.bbox_head.named_parameters())
        assert sum(s.scale.grad.abs().item() for s in m.bbox_head.scales) > 0
        assert sum(s.scale.grad.abs().item() for s in m.bbox_head.scales_refine) > 0
        assert float(m.bbox_head.vfnet_cls_dconv.weight.grad.abs().max()) > 0
        assert m.backbone.layer2[0].conv1.weight.grad is not None
        m.zero_grad()


# ------------------------------------------------------------------------------------------- 16-bit modes and the tools
@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
def test_model_16bit_close_to_fp32(gold, dtype):
    """the criterion tests/test_atss_gpu.py::test_model_16bit_close_to_fp32 applies to its 16-bit cases"""
    from brcnn import blocks
    seed = int(gold['seed_e2e'])
    m = _model(seed).eval()
    img, _, _, _ = util.demo_inputs(2, vi.H, vi.W, seed=seed)
    try:
        with torch.no_grad():
            f32 = [f.float() for f in m.extract_feat_nhwc(img.to(DEV))]
            r32 = m.simple_test(img.to(DEV), vi.metas())
            m.set_compute_dtype(dtype)
            f16 = m.extract_feat_nhwc(img.to(DEV))
            assert all(f.dtype == (torch.bfloat16 if dtype == 'bf16' else torch.float16) for f in f16)
            a, r1, d0, _ = m.bbox_head.forward_rows(list(f16))
            assert a.dtype == torch.float32 and r1.dtype == torch.float32 and d0.dtype == torch.float32    # fp32 from the heads on
            r16 = m.simple_test(img.to(DEV), vi.metas())
    finally:
        blocks.set_compute_dtype('f32')
    for x, y in zip(f16, f32):
        assert (x.float() - y).abs().max().item() / y.abs().max().item() < 0.05
    n32, n16 = sum(len(c) for r in r32 for c in r), sum(len(c) for r in r16 for c in r)
    assert n32 > 0 and abs(n16 - n32) <= 0.2 * n32 + 5, (n16, n32)
    d = np.concatenate([c for r in r32 for c in r]), np.concatenate([c for r in r16 for c in r])
    dist = np.abs(d[0][:, None, :4] - d[1][None, :, :4]).max(-1)
    ds = np.abs(d[0][:, None, 4] - d[1][None, :, 4])
    assert ((dist < 2.0) & (ds < 0.05)).any(1).mean() > 0.7


def test_inference_detector_returns_the_bbox2result_layout():
    from brcnn.apis import inference_detector, init_detector
    model = init_detector(vi.CONFIG, None, device=DEV)
    img = np.random.RandomState(0).randint(0, 255, (120, 160, 3), dtype=np.uint8)
    res = inference_detector(model, img)
    assert isinstance(res, list) and len(res) == 4
    assert all(isinstance(r, np.ndarray) and r.dtype == np.float32 and r.ndim == 2 and r.shape[1] == 5 for r in res)
    both = inference_detector(model, [img, img[:, ::-1].copy()])
    assert len(both) == 2 and all(len(r) == 4 for r in both)


def test_bf16_train_step_is_reproducible_and_fused_sgd_follows(gold):
    from brcnn import blocks
    from brcnn.optim import FusedSGD
    m = _model(int(gold['seed_e2e'])).train()
    img, gts, gls = _train_batch(int(gold['seed_train0']))
    data = dict(img=img, img_metas=vi.metas(), gt_bboxes=gts, gt_labels=gls)
    opt = FusedSGD([p for p in m.parameters() if p.requires_grad], lr=0.01, momentum=0.9, weight_decay=1e-4)
    try:
        m.set_compute_dtype('bf16')
        runs = []
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            out = m.train_step(data, opt)
            out['loss'].backward()
            grads = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
            runs.append((dict(out['log_vars'].items()), grads))
        assert runs[0][0] == runs[1][0] and 'loss_bbox_rf' in runs[0][0]
        assert runs[0][1].keys() == runs[1][1].keys() and 'bbox_head.vfnet_reg.weight' in runs[0][1]
        for k in ('bbox_head.scales.4.scale', 'bbox_head.scales_refine.0.scale', 'bbox_head.vfnet_cls_dconv.weight',
                  'bbox_head.vfnet_reg_refine_dconv.weight'):
            assert k in runs[0][1], k
        assert all(torch.equal(runs[0][1][k], runs[1][1][k]) for k in runs[0][1])
        before = m.bbox_head.vfnet_cls.weight.detach().clone()
        opt.step()
        torch.cuda.synchronize()
        assert not torch.equal(before, m.bbox_head.vfnet_cls.weight.detach())
        assert all(torch.isfinite(p).all() for p in m.parameters())
    finally:
        blocks.set_compute_dtype('f32')


def test_train_and_test_tools_take_the_config(tmp_path):
    """tools/train.py (one epoch on the synthetic 7-image set, checkpoint, validation) and tools/test.py (bbox evaluation,
    result file) with the recipe's model section in the tiny driver config of tests/test_drivers_cpu.py"""
    import importlib.util
    import pickle

    from brcnn import Config
    from tests.test_drivers_cpu import CLASSES, _tiny_cfg

    def tool(name):
        spec = importlib.util.spec_from_file_location(f'brcnn_tool_{name}', os.path.join(vi.ROOT, 'tools', f'{name}.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    cfg = _tiny_cfg(tmp_path, max_epochs=1)
    cfg.model = Config.fromfile(vi.CONFIG).model
    cfg_path = str(tmp_path / 'tiny_vfnet.py')
    cfg.dump(cfg_path)
    work = str(tmp_path / 'work_gpu')
    runner = tool('train').main([cfg_path, '--work-dir', work, '--seed', '0', '--allow-random-init'])
    assert runner.epoch == 1 and os.path.exists(os.path.join(work, 'epoch_1.pth'))
    assert all(np.isfinite(v) for row in runner.history for v in row[3].values())
    assert any('loss_bbox_rf' in row[3] and 'loss_bbox' in row[3] for row in runner.history) and len(runner.eval_history) == 1
    out_pkl = str(tmp_path / 'res.pkl')
    metric = tool('test').main([cfg_path, os.path.join(work, 'epoch_1.pth'), '--eval', 'bbox', '--out', out_pkl])
    assert metric == {} or 0.0 <= metric['bbox_mAP'] <= 1.0
    res = pickle.load(open(out_pkl, 'rb'))
    assert len(res) == 7 and len(res[0]) == len(CLASSES) and res[0][0].shape[1] == 5
