"""-m gpu: ResNet bottlenecks with a deformable conv2 (DCN v1 / DCNv2, deform groups), from one block to the
`dconv_c3-c5` recipe, against a float64 torch composition (conv, eval-BN, the deformable conv of
tests/deform_groups_ref64.py).

One block, inference: every stage is held to float64 ON THE INPUT THAT STAGE SAW (the 16-bit modes round each stage's
output once, and a deformable conv is not Lipschitz in its offsets across an integer line, so the stages are checked one by
one with route_util.bound -- the deformable stage at the fp32 offsets the kernels sampled at, with the deformable term --
and the block's own forward must equal the chain of those stages bit for bit).  Training: gradients against float64
autograd of the whole composition, at the relative tolerances test_deform_conv_backward (tests/test_res2net16_gpu.py)
uses for 16 bits and the suite's ACC_TOL bound for fp32.  conv_offset is non-zero everywhere but in the zero-offset test.
"""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import brcnn  # noqa: F401
from brcnn import Config, blocks, build_detector, lib, ops
from brcnn.backbones import Bottleneck, ResNet
from brcnn.blocks import conv_bn_act_nhwc, to_nhwc
from tests import deform_groups_ref64 as DG
from tests import route_util as R
from tests import util

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
f32, bf16, f16 = torch.float32, torch.bfloat16, torch.float16
MODES = {'f32': f32, 'bf16': bf16, 'f16': f16}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPE = os.path.join(ROOT, 'configs', 'dcn', 'boosting_rcnn_r50_dconv_c3-c5_pafpn_1x_utdac.py')
C3_C5 = (False, True, True, True)


def _seed_module(m, seed, offset_scale=0.1):
    """seeded He-scaled weights, BN statistics / affine away from the identity, conv_offset small but non-zero (offsets
    of a fraction of a pixel to a pixel, as a trained DCN predicts)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in sorted(m.state_dict().items()):
            if k.endswith('num_batches_tracked'):
                continue
            if k.endswith('running_var'):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif k.endswith('running_mean') or k.endswith('.bias'):
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            elif k.endswith('bn3.weight'):      # (a short residual branch: 16 He-scaled blocks must not overflow fp16)
                p.copy_(torch.rand(p.shape, generator=g) * 0.2 + 0.2)
            elif p.dim() == 1:
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            else:
                fan_in = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / fan_in) ** 0.5 * (offset_scale if '.conv_offset.' in k else 1))
    return m


def _block(kind, G, stride, seed=41):
    dcn = None if kind is None else dict(type=kind, deform_groups=G, fallback_on_stride=False)
    down = None
    if stride != 1:
        down = torch.nn.Sequential(torch.nn.Conv2d(256, 256, 1, stride=stride, bias=False), torch.nn.BatchNorm2d(256))
    return _seed_module(Bottleneck(256, 64, stride, down, dcn=dcn), seed).to(DEV).eval()


def _bn64(y, bn):
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    return y * s + (bn.bias.double() - bn.running_mean.double() * s)


def _conv64(x, conv):
    return F.conv2d(x.permute(0, 3, 1, 2), conv.weight.double(), None, conv.stride, conv.padding).permute(0, 2, 3, 1)


def _dcn64(x, blk, om=None):
    c2 = blk.conv2
    if not getattr(blk, 'with_dcn', False):
        return _conv64(x, c2)
    if om is None:
        om = F.conv2d(x.permute(0, 3, 1, 2), c2.conv_offset.weight.double(), c2.conv_offset.bias.double(), c2.stride,
                      1).permute(0, 2, 3, 1)
    return DG.deform_conv64(x, om, c2.weight.double().permute(0, 2, 3, 1), c2.deform_groups, c2.modulated, c2.stride, 1)


def _block64(blk, x, masks=None, stored=None, seen=None):
    """the whole block in float64, differentiable (x (N,H,W,C) float64).  `masks`: the three ReLUs' pass masks, given
    instead of being taken from the float64 pre-activations; `stored`: the 16-bit type every tensor the kernels store
    between two launches is rounded to, with the identity as its derivative (see
    test_block_gradients_against_float64_autograd); `seen`: the kernels' own conv1 and deformable-stage outputs, which then
    stand in for the rounded float64 values of those two tensors (derivative 1 again)"""
    relu = (lambda t, i: t.relu()) if masks is None else (lambda t, i: t * masks[i].to(t.dtype))
    st = (lambda t: t) if stored is None else (lambda t: t + (t.detach().to(stored).double() - t.detach()))
    sub = (lambda t, k: st(t)) if seen is None else (lambda t, k: t + (seen[k].detach().double() - t.detach()))
    o = sub(relu(_bn64(_conv64(x, blk.conv1), blk.bn1), 0), 'o1')
    o = sub(relu(_bn64(st(_dcn64(o, blk)), blk.bn2), 1), 'o2')   # (the raw deformable conv output is stored, then bn2 + ReLU)
    o = _bn64(_conv64(o, blk.conv3), blk.bn3)
    idn = x if blk.downsample is None else st(_bn64(_conv64(x, blk.downsample[0]), blk.downsample[1]))
    return relu(o + idn, 2)


def _x(dt, seed=42):
    return torch.randn(2, 13, 17, 256, generator=torch.Generator().manual_seed(seed)).to(dt).to(DEV)


def _fold(bn):
    s, b = blocks.fold_bn(bn)
    return s.double(), b.double()


CASES = [(k, G, s) for k in ('DCN', 'DCNv2') for G in (1, 2) for s in (1, 2)]
CASE_IDS = [f'{k}-G{G}-s{s}' for k, G, s in CASES]


@pytest.mark.parametrize('kind,G,stride', CASES, ids=CASE_IDS)
@pytest.mark.parametrize('mode', list(MODES))
def test_block_inference_stage_by_stage_against_float64(mode, kind, G, stride):
    dt = MODES[mode]
    blk = _block(kind, G, stride)
    x = _x(dt)
    c2, L = blk.conv2, lib.load()
    try:
        blocks.set_compute_dtype(mode)
        with torch.no_grad():
            o1 = conv_bn_act_nhwc(x, blk.conv1, blk.bn1, blocks.PackedCache(), True)
            L.brcnn_conv_set_tile(-9, -1)
            o2 = blk._dcn_bn_act(o1)
            fused, im2col = L.brcnn_conv_set_tile(-13, 10), L.brcnn_conv_set_tile(-13, 11)
            idn = x if stride == 1 else conv_bn_act_nhwc(x, blk.downsample[0], blk.downsample[1], blocks.PackedCache(), False)
            o3 = conv_bn_act_nhwc(o2, blk.conv3, blk.bn3, blocks.PackedCache(), True, residual=idn)
            y = blk.forward_nhwc(x)
            # the offsets the deformable stage sampled at: the same launch again (fp32 result in every mode)
            # (16 bits: conv_offset padded to 64 output rows, as the block packs it)
            rows = c2.offset_rows
            padr = (-rows) % 64 if dt != f32 else 0
            wo = F.pad(blocks.pack_weight(c2.conv_offset.weight), (0, 0, 0, 0, 0, 0, 0, padr)).to(dt).contiguous()
            bo = F.pad(c2.conv_offset.bias.detach().float(), (0, padr)).contiguous()
            om = ops.conv2d_nhwc(o1, wo, None, bo, None, False, stride, 1, **(dict(out_f32=True) if dt != f32 else {}))
            om, wo = om[..., :rows].contiguous(), wo[:rows]
    finally:
        blocks.set_compute_dtype('f32')
    assert y.dtype == dt and o1.dtype == dt and om.dtype == f32 and om.shape[-1] == c2.offset_rows
    assert torch.equal(y, o3), 'the block is the chain of its stages'
    # which route the deformable stage took: fused in 16 bits where 64 channels per group allow it, else im2col + GEMM
    assert (fused, im2col) == ((1, 0) if dt != f32 and 64 // G >= 64 else (0, 1)), (fused, im2col)
    xd, o1d, o2d = x.double(), o1.double(), o2.double()
    s1, b1 = _fold(blk.bn1)
    w1 = blk.conv1.weight.detach().to(dt).double()          # (the operands the kernels saw: weights rounded to the dtype)
    e1 = R.excess(o1, (F.conv2d(xd.permute(0, 3, 1, 2), w1).permute(0, 2, 3, 1) * s1 + b1).relu(), dt)
    om_ref = F.conv2d(o1d.permute(0, 3, 1, 2), wo.double().permute(0, 3, 1, 2), c2.conv_offset.bias.double(), stride,
                      1).permute(0, 2, 3, 1)
    e_om = R.excess(om, om_ref, f32)
    assert float(om.abs().max()) > 0.05, 'conv_offset is non-zero: the offset path is exercised'
    s2, b2 = _fold(blk.bn2)
    w16 = c2.weight.detach().permute(0, 2, 3, 1).to(dt)
    ref2 = (DG.deform_conv64(o1d, om, w16, G, c2.modulated, stride, 1) * s2 + b2).relu()
    extra = DG.conv_extra(o1d, om, w16, G, c2.modulated, stride, 1, s2)
    if dt != f32:       # the 16-bit columns' own rounding, summed through the weights
        extra = extra * (1 + R.half_ulp(dt) * 1.001 / (DG.col_k(c2.modulated) * DG.U))
    e2 = R.excess(o2, ref2, dt, extra)
    s3, b3 = _fold(blk.bn3)
    w3 = blk.conv3.weight.detach().to(dt).double()
    ref3 = (F.conv2d(o2d.permute(0, 3, 1, 2), w3).permute(0, 2, 3, 1) * s3 + b3 + idn.double()).relu()
    e3 = R.excess(o3, ref3, dt)
    print(f'largest error minus bound: conv1 {e1:.3e}  offsets {e_om:.3e}  deformable {e2:.3e}  conv3 {e3:.3e}')
    assert e1 <= 0 and e_om <= 0 and e2 <= 0 and e3 <= 0, (e1, e_om, e2, e3)
    if dt == f32:
        # and the whole block against the whole float64 composition: four chained stages, each within ACC_TOL of float64
        # on its own input above, each passing the error of the one before through He-scaled weights (gain about 1)
        ref = _block64(blk, xd)
        assert R.excess(y, ref, f32, 4 * R.ACC_TOL * ref.abs().max()) <= 0


def _check_training_forward(blk, dt, G, stride, x, seen, y):
    """the TRAINING forward of the block, each stage held to float64 on the input that stage saw (the gradient reference
    takes conv1's and the deformable stage's outputs over from the kernels, so they are checked here first): the offsets,
    the deformable stage at those offsets, conv3 + bn3 + identity + ReLU.  Bounds as in the inference test, plus one term:
    the training kernels store the raw conv output in the dtype and form the activation from the stored value, so a
    16-bit result carries the rounding of the raw value, half an ulp of it times |bn scale|, besides its own."""
    c2, hu = blk.conv2, R.half_ulp(dt) * 1.001
    rnd = lambda w: w.detach().to(dt).double()          # noqa: E731  (the operands the kernels saw)
    with torch.no_grad():
        o1, o2, om = seen['o1'].detach(), seen['o2'].detach(), seen['om'].detach()
        assert o1.dtype == dt and o2.dtype == dt and om.dtype == f32 and om.shape[-1] == c2.offset_rows
        o1d, o2d, xd = o1.double(), o2.double(), x.double()
        s1, b1 = _fold(blk.bn1)
        raw1 = F.conv2d(xd.permute(0, 3, 1, 2), rnd(blk.conv1.weight)).permute(0, 2, 3, 1)
        e1 = R.excess(o1, (raw1 * s1 + b1).relu(), dt, hu * raw1.abs() * s1.abs())
        om_ref = F.conv2d(o1d.permute(0, 3, 1, 2), rnd(c2.conv_offset.weight), c2.conv_offset.bias.double(), stride,
                          1).permute(0, 2, 3, 1)
        e_om = R.excess(om, om_ref, f32)
        s2, b2 = _fold(blk.bn2)
        w16 = c2.weight.detach().permute(0, 2, 3, 1).to(dt)
        raw2 = DG.deform_conv64(o1d, om, w16, G, c2.modulated, stride, 1)
        extra = DG.conv_extra(o1d, om, w16, G, c2.modulated, stride, 1, s2)
        if dt != f32:
            extra = extra * (1 + R.half_ulp(dt) * 1.001 / (DG.col_k(c2.modulated) * DG.U))
        e2 = R.excess(o2, (raw2 * s2 + b2).relu(), dt, extra + hu * raw2.abs() * s2.abs())
        s3, b3 = _fold(blk.bn3)
        raw3 = F.conv2d(o2d.permute(0, 3, 1, 2), rnd(blk.conv3.weight)).permute(0, 2, 3, 1)
        if blk.downsample is None:
            idn = xd
        else:
            sd, bd = _fold(blk.downsample[1])
            rawd = F.conv2d(xd.permute(0, 3, 1, 2), rnd(blk.downsample[0].weight), None, stride).permute(0, 2, 3, 1)
            idn = (rawd * sd + bd).to(dt).double() if dt != f32 else rawd * sd + bd
        extra3 = hu * raw3.abs() * s3.abs()
        if blk.downsample is not None:
            # the identity branch is a training conv of its own: its stored raw value's rounding through |bn scale|, its
            # result's rounding (the one emulated above may fall on the other side: twice), its fp32 accumulation
            extra3 = extra3 + hu * rawd.abs() * sd.abs() + 2 * hu * idn.abs() + R.ACC_TOL * max(1.0, idn.abs().max().item())
        e3 = R.excess(y.detach(), (raw3 * s3 + b3 + idn).relu(), dt, extra3)
    print(f'training forward, largest error minus bound: conv1 {e1:.3e}  offsets {e_om:.3e}  deformable {e2:.3e}  conv3 {e3:.3e}')
    assert e1 <= 0 and e_om <= 0 and e2 <= 0 and e3 <= 0, (e1, e_om, e2, e3)


GRADS = ('conv2.weight', 'conv2.conv_offset.weight', 'conv2.conv_offset.bias', 'bn1.weight', 'bn1.bias', 'bn2.weight',
         'bn2.bias', 'bn3.weight', 'bn3.bias')


@pytest.mark.parametrize('kind,G,stride', CASES, ids=CASE_IDS)
@pytest.mark.parametrize('mode', list(MODES))
def test_block_gradients_against_float64_autograd(mode, kind, G, stride):
    """x, conv2.weight, conv_offset.{weight,bias} and the BN affine parameters against float64 autograd of the same
    composition.  fp32: the suite's ACC_TOL bound, every gradient.  16 bits: the tolerances of test_deform_conv_backward
    (tests/test_res2net16_gpu.py) -- the data gradient by its largest error relative to the largest magnitude (1e-2 bf16,
    2e-3 fp16), the parameter gradients by cosine > 0.999, as that test holds its weight gradient.
    A ReLU has no gradient at 0, and a 16-bit forward rounds each stage once: a pre-activation within that rounding of 0
    passes in one arithmetic and not in the other, and the identity path hands such an element's whole upstream gradient
    to x (measured with float64's own masks: x off by 0.07 - 0.46 of its largest magnitude in both 16-bit types, at
    cosines of 0.9997 - 0.99997, while fp32 holds ACC_TOL).  Likewise the cell a sample falls into: offsets that differ by
    the 0.4 % of a bf16 rounding put about one tap in two hundred into the neighbouring cell, whose coordinate gradient
    is another one (measured with the masks alone taken over: conv_offset.weight at a cosine of 0.9945).  The gradient
    checked is therefore the one AT THE FORWARD THE KERNELS RAN, as test_deform_conv_backward and tests/deform_ref64.py
    have it ("the reference sees the kernel's operands"): in the 16-bit legs the float64 composition takes the conv
    weights rounded to the dtype (the gradient of a master weight is the gradient at its rounded value), rounds every
    tensor the kernels store between launches once (derivative 1), and takes the three ReLU pass masks from the kernels'
    own stage outputs.  The two tensors the offsets depend on, conv1's output and the deformable stage's, are the kernels'
    own values outright: the training conv rounds its raw output and forms the activation from the rounded value, two
    roundings where the composition has one, which moved the offsets by ~6e-4 pixel in bf16 and left about ten taps per
    case in the neighbouring cell (measured with the rounded float64 values instead: conv_offset.weight at cosines of
    0.998 - 0.9998 in bf16, every other gradient within 0.5 %).  The offsets themselves, the sampling cells and the
    whole backward come from the float64 composition."""
    dt = MODES[mode]
    blk = _block(kind, G, stride)
    ref_blk = copy.deepcopy(blk).double()
    if dt != f32:
        with torch.no_grad():
            for k, p_ in ref_blk.named_parameters():
                if p_.dim() == 4:
                    p_.copy_(p_.to(dt).double())
    x = _x(dt, 43)
    go = torch.randn(2, (13 - 1) // stride + 1, (17 - 1) // stride + 1, 256, generator=torch.Generator().manual_seed(44)).to(dt)
    xg = x.clone().requires_grad_()
    seen, stage = {}, blk._dcn_bn_act

    def spy(t):
        seen['o1'], seen['o2'] = t, stage(t)
        return seen['o2']
    blk._dcn_bn_act = spy
    from brcnn import autograd as A
    conv_autograd = A.conv2d_nhwc_autograd

    def conv_spy(t, weight, *a, **k):
        out = conv_autograd(t, weight, *a, **k)
        if weight is blk.conv2.conv_offset.weight:
            seen['om'] = out
        return out
    A.conv2d_nhwc_autograd = conv_spy
    try:
        blocks.set_compute_dtype(mode)
        y = blk.forward_nhwc(xg)
        assert y.dtype == dt
        y.backward(go.to(DEV))
    finally:
        A.conv2d_nhwc_autograd = conv_autograd
        blocks.set_compute_dtype('f32')
    _check_training_forward(blk, dt, G, stride, x, seen, y)
    masks = None if dt == f32 else [(t.detach() > 0) for t in (seen['o1'], seen['o2'], y)]
    xr = x.double().requires_grad_()
    _block64(ref_blk, xr, masks, None if dt == f32 else dt, None if dt == f32 else seen).backward(go.double().to(DEV))
    got, ref = {'x': xg.grad}, {'x': xr.grad}
    p, pr = dict(blk.named_parameters()), dict(ref_blk.named_parameters())
    for k in GRADS:
        got[k], ref[k] = p[k].grad, pr[k].grad
    tol = {bf16: 1e-2, f16: 2e-3}.get(dt)
    bad = []
    for k in got:
        g, r = got[k].double(), ref[k]
        assert g.shape == r.shape and bool(torch.isfinite(g).all()) and float(r.abs().max()) > 0, k
        rel = (g - r).abs().max().item() / r.abs().max().item()
        a, b = g.flatten(), r.flatten()
        cos = (torch.dot(a, b) / (a.norm() * b.norm())).item()
        print(f'{k}: relative error {rel:.3e}  cosine {cos:.6f}')
        if dt == f32:
            ok = R.excess(got[k], r, f32) <= 0
        elif k == 'x':
            ok = rel < tol
        else:
            ok = cos > 0.999
        if not ok:
            bad.append((k, rel, cos))
    assert not bad, bad


@pytest.mark.parametrize('mode', list(MODES))
def test_zero_offsets_give_the_plain_conv(mode):
    """conv_offset zero: a v1 conv2 stage is the plain conv with the same weight (16 bits: the columns are exactly the plain
    im2col), a v2 one the plain conv with 0.5 of it (sigmoid(0)), each within the GEMM bound of float64"""
    dt = MODES[mode]
    o1 = torch.randn(2, 13, 17, 64, generator=torch.Generator().manual_seed(45)).relu()
    o1 = torch.where(o1 < 2.0 ** -9, torch.zeros(()), o1).to(dt).to(DEV)        # (0.5 x is exact: nothing near the fp16 subnormals)
    for kind, factor in (('DCN', 1.0), ('DCNv2', 0.5)):
        blk = _block(kind, 1, 1)
        with torch.no_grad():
            blk.conv2.conv_offset.weight.zero_()
            blk.conv2.conv_offset.bias.zero_()
            try:
                blocks.set_compute_dtype(mode)
                o2 = blk._dcn_bn_act(o1)
            finally:
                blocks.set_compute_dtype('f32')
            om = torch.zeros(2, 13, 17, blk.conv2.offset_rows, device=DEV)
            col, _ = ops.deform_im2col_nhwc(o1, om, 3, 1, 1, 1, None, 1, kind == 'DCNv2')
        plain = F.unfold(o1.float().permute(0, 3, 1, 2), 3, padding=1).view(2, 64, 9, 13 * 17).permute(0, 3, 2, 1)
        assert torch.equal(col.float().view(2, 13 * 17, 9, 64), plain * factor)
        s2, b2 = _fold(blk.bn2)
        w = blk.conv2.weight.detach().to(dt).double() * factor
        ref = (F.conv2d(o1.double().permute(0, 3, 1, 2), w, None, 1, 1).permute(0, 2, 3, 1) * s2 + b2).relu()
        assert R.excess(o2, ref, dt) <= 0, kind


# ---- the whole backbone ---------------------------------------------------------------------------------------------------
def _backbone(kind='DCN', G=1):
    m = ResNet(depth=50, frozen_stages=1, norm_eval=True, dcn=dict(type=kind, deform_groups=G, fallback_on_stride=False),
               stage_with_dcn=C3_C5)
    return _seed_module(m, 51).to(DEV).eval()


def _backbone64(m, img):
    x = _bn64(F.conv2d(img.double(), m.conv1.weight.double(), None, 2, 3).permute(0, 2, 3, 1), m.bn1).relu()
    x = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    outs = []
    for name in m.res_layers:
        for blk in getattr(m, name):
            x = _block64(blk, x)
        outs.append(x)
    return outs


def test_r50_dconv_c3_c5_backbone():
    """fp32 against the float64 composition at the 1e-4 of the plain backbone's fixture test; bf16 / fp16 against fp32
    with the comparison of test_res2net50_backbone_16bit_close_to_fp32 (0.05 of the stage's largest magnitude)"""
    m = _backbone()
    img = torch.randn(2, 3, 128, 160, generator=torch.Generator().manual_seed(52)).to(DEV)
    with torch.no_grad():
        ref = _backbone64(m, img)
        o32 = m.forward_from_nchw(img)
        o16 = {}
        try:
            for mode in ('bf16', 'f16'):
                blocks.set_compute_dtype(mode)
                o16[mode] = m.forward_from_nchw(img)
        finally:
            blocks.set_compute_dtype('f32')
    assert [tuple(o.shape[1:3]) for o in o32] == [(32, 40), (16, 20), (8, 10), (4, 5)]
    for a, r in zip(o32, ref):
        assert a.dtype == f32
        rel = (a.double() - r).abs().max().item() / r.abs().max().item()
        print(f'fp32 stage against float64: {rel:.3e}')
        assert rel < 1e-4, rel
    for mode, outs in o16.items():
        for a, b in zip(outs, o32):
            assert a.dtype == MODES[mode]
            rel = (a.float() - b).abs().max().item() / b.abs().max().item()
            print(f'{mode} stage against fp32: {rel:.3e}')
            assert rel < 0.05, (mode, rel)


# ---- the recipe -------------------------------------------------------------------------------------------------------------
def _detector(seed=10):
    m = build_detector(Config.fromfile(RECIPE).model)
    sd = util.seeded_state_dict(m, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k in sd:        # small random values in the (zero-initialised) offset branch
        if '.conv_offset.' in k:
            sd[k] = torch.randn(sd[k].shape, generator=g) * (0.1 * (2.0 / max(sd[k][0].numel(), 1)) ** 0.5 if sd[k].dim() > 1 else 0.05)
    m.load_state_dict(sd)
    return m


def _train_step(mode):
    img, metas, gts, gls = util.demo_inputs(2, 128, 160, num_classes=4, seed=10)
    m = _detector().to(DEV).train()
    m.set_compute_dtype(mode)
    torch.manual_seed(77)
    losses = m.forward_train(img.to(DEV), metas, [g_.to(DEV) for g_ in gts], [l.to(DEV) for l in gls])
    loss, log_vars = m._parse_losses(losses)
    loss.backward()
    return dict(log_vars), {k: p.grad.detach().float() for k, p in m.named_parameters() if p.grad is not None}


def test_recipe_inference_and_checkpoint_round_trip(tmp_path):
    m = _detector().to(DEV).eval()
    img, metas, _, _ = util.demo_inputs(2, 128, 160, seed=10)
    with torch.no_grad():
        res = m(img=[img.to(DEV)], img_metas=[metas], return_loss=False)
    assert len(res) == 2 and all(len(r) == 4 for r in res)
    assert all(isinstance(c, np.ndarray) and c.ndim == 2 and c.shape[1] == 5 for r in res for c in r)
    torch.save(dict(state_dict=m.state_dict()), str(tmp_path / 'dcn.pth'))
    m2 = build_detector(Config.fromfile(RECIPE).model)
    sd = torch.load(str(tmp_path / 'dcn.pth'), map_location='cpu', weights_only=False)['state_dict']
    assert any('.conv_offset.' in k for k in sd)
    m2.load_state_dict(sd, strict=True)
    m2 = m2.to(DEV).eval()
    with torch.no_grad():
        res2 = m2(img=[img.to(DEV)], img_metas=[metas], return_loss=False)
    for r, r2 in zip(res, res2):
        for c, c2 in zip(r, r2):
            assert c.shape == c2.shape and np.array_equal(c.view(np.int32), c2.view(np.int32))


def test_recipe_train_step_fp32_and_bf16():
    try:
        lf, gf = _train_step('f32')
        lb, gb = _train_step('bf16')
    finally:
        blocks.set_compute_dtype('f32')
    for lv in (lf, lb):
        assert all(np.isfinite(v) for v in lv.values()), lv
    offs = [k for k in gf if '.conv_offset.' in k]
    assert len(offs) == 2 * (4 + 6 + 3) and not any(k.startswith('backbone.layer1.') for k in gf)
    for grads in (gf, gb):
        for k in offs:
            assert bool(torch.isfinite(grads[k]).all()) and float(grads[k].abs().max()) > 0, k
    for k, tol in (('loss_rpn_cls', 0.05), ('loss_rpn_bbox', 0.05), ('loss_rpn_iou', 0.05), ('loss_bbox', 0.2), ('loss', 0.08)):
        assert abs(lb[k] - lf[k]) <= tol * abs(lf[k]) + 1e-3, (k, lb[k], lf[k])
