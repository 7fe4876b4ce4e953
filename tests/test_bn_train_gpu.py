"""Training-mode BatchNorm on the device (csrc/bn_train.hip, autograd.BnTrainActFunction, the norm_eval=False branch of
blocks.conv_bn_act_nhwc): the kernel entries against tests/bn_ref64.py at its derived bounds, the running statistics,
mutation legs, bit-reproducibility, the version bump the packed-operand caches need, whole Bottlenecks (all BatchNorms
training, one of three, under no_grad, ResNeXt, DCN) against float64 autograd, and the bn_train recipe."""
import copy
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import brcnn  # noqa: F401
from brcnn import Config, backbones, blocks, build_detector, lib, ops
from brcnn.autograd import bn_train_act_autograd
from brcnn.backbones import Bottleneck, BottleneckX
from brcnn.blocks import conv_bn_act_nhwc
from tests import bn_ref64 as B
from tests import deform_groups_ref64 as DG
from tests import route_util as R
from tests import util

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
f32, bf16, f16 = torch.float32, torch.bfloat16, torch.float16
MODES = {'f32': f32, 'bf16': bf16, 'f16': f16}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPE = os.path.join(ROOT, 'configs', 'bn_train', 'boosting_rcnn_r50_pafpn_1x_utdac_bn_train.py')
CASES = B.cases()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return lib.raw_stream_handle()


class Out:
    pass


def _forward(case, relu, momentum=0.1, eps=B.EPS):
    """brcnn_bn_train_stats + brcnn_bn_act_forward on the case's tensors; running statistics updated in clones"""
    L = lib.load()
    z = case['z']
    rows, C = z.shape
    dt = ops._dt(z)
    o = Out()
    o.mean, o.rstd, o.var, o.scale, o.shift = (torch.empty(C, dtype=f32, device=DEV) for _ in range(5))
    o.rm, o.rv = case['rm'].clone(), case['rv'].clone()
    nb = L.brcnn_bn_train_workspace_bytes(rows, C, dt)
    assert nb == B.plan(rows, C, z.dtype)[4] * 2 * C * 8
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    st = L.brcnn_bn_train_stats(_p(z), _p(case['gamma']), _p(case['beta']), eps, momentum, _p(o.rm), _p(o.rv), _p(o.mean),
                                _p(o.rstd), _p(o.var), _p(o.scale), _p(o.shift), _p(ws), nb, rows, C, dt, _stream())
    assert st == 0, st
    o.y = torch.empty_like(z)
    st = L.brcnn_bn_act_forward(_p(z), _p(o.scale), _p(o.shift), _p(case['res']), _p(o.y), rows, C, int(relu), dt, _stream())
    assert st == 0, st
    return o


def _backward(case, o, relu):
    L = lib.load()
    z = case['z']
    rows, C = z.shape
    dt = ops._dt(z)
    o.dz = torch.empty_like(z)
    o.dres = torch.empty_like(z) if case['res'] is not None else None
    o.dgamma, o.dbeta = torch.empty(C, dtype=f32, device=DEV), torch.empty(C, dtype=f32, device=DEV)
    nb = L.brcnn_bn_train_workspace_bytes(rows, C, dt)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    st = L.brcnn_bn_train_backward(_p(case['dout']), _p(o.y) if relu else None, _p(z), _p(case['gamma']), _p(o.mean), _p(o.rstd),
                                   _p(o.dz), _p(o.dres), _p(o.dgamma), _p(o.dbeta), _p(ws), nb, rows, C, int(relu), dt,
                                   _stream())
    assert st == 0, st
    return o


def _ratio(got, ref, bound):
    """largest |got - ref| / bound over ALL elements (<= 1: inside)"""
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    return ((got.double() - ref).abs() / bound).max().item()


# ---- the kernel entries against float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_kernels_against_float64(name):
    spec = CASES[name]
    dt, relu = spec['dtype'], spec['relu']
    case = B.case_inputs(spec, DEV)
    f = B.bn_forward64(case['z'], case['gamma'], case['beta'], B.EPS, relu, case['res'], case['rm'], case['rv'], 0.1)
    if relu:
        share = B.mask_band_share(f, dt)
        assert share <= B.MASK_BAND_CAP, share
    o = _forward(case, relu)
    r = {'mean': _ratio(o.mean, f.mean, B.mean_bound(f)), 'var': _ratio(o.var, f.var, B.var_bound(f)),
         'rstd': _ratio(o.rstd, f.rstd, B.rstd_bound(f)), 'y': _ratio(o.y, f.y, R.bound(f.y, dt, B.y_extra(f))),
         'running_mean': _ratio(o.rm, f.new_rm, B.running_mean_bound(f)),
         'running_var': _ratio(o.rv, f.new_rv, B.running_var_bound(f))}
    mask = o.y > 0 if relu else torch.ones_like(o.y, dtype=torch.bool)
    b = B.bn_backward64(case['dout'], f, mask)
    _backward(case, o, relu)
    r['dbeta'] = _ratio(o.dbeta, b.dbeta, R.bound(b.dbeta, f32, B.dbeta_extra(b)))
    r['dgamma'] = _ratio(o.dgamma, b.dgamma, R.bound(b.dgamma, f32, B.dgamma_extra(f, b)))
    r['dz'] = _ratio(o.dz, b.dz, R.bound(b.dz, dt, B.dz_extra(f, b)))
    if case['res'] is not None:
        assert torch.equal(o.dres, torch.where(mask, case['dout'], torch.zeros_like(case['dout']))), 'dres = dpre, exactly'
    print(name, 'kappa %.2f-%.2f ' % (f.kappa.min().item(), f.kappa.max().item()),
          '  '.join(f'{k} {v:.3f}' for k, v in r.items()), '(error / bound)')
    assert all(v <= 1.0 for v in r.values()), r
    if spec['kw'].get('constant'):
        c = list(spec['kw']['constant'])
        assert bool((o.var[c] == 0).all()) and bool(torch.isfinite(o.rstd[c]).all())
        assert torch.equal(o.rstd[c], torch.full((len(c),), B.f32(B.EPS) ** -0.5, device=DEV).float())


def test_entries_refuse_what_they_do_not_take():
    L = lib.load()
    case = B.make_case(8, 16, f32, 1, device=DEV)
    o = _forward(case, False)
    t = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)

    def stats(rows, C, dt, nb=1 << 16):
        return L.brcnn_bn_train_stats(_p(case['z']), _p(case['gamma']), _p(case['beta']), 1e-5, 0.1, _p(o.rm), _p(o.rv),
                                      _p(o.mean), _p(o.rstd), None, _p(o.scale), _p(o.shift), _p(t), nb, rows, C, dt, _stream())
    before = (o.rm.clone(), o.rv.clone())
    assert stats(8, 16, ops.DT_F32) == 0
    for rows, C, dt in ((1, 16, ops.DT_F32), (0, 16, ops.DT_F32), (8, 12, ops.DT_F32), (8, 6, ops.DT_F32), (8, 4, ops.DT_BF16),
                        (8, 24, ops.DT_BF16), (8, 16, 77), (1 << 58, 16, ops.DT_F32)):
        assert L.brcnn_bn_train_workspace_bytes(rows, C, dt) == 0
        assert stats(rows, C, dt) == -22, (rows, C, dt)
    assert stats(8, 16, ops.DT_F32, nb=8) == -22            # workspace too small
    st = L.brcnn_bn_train_backward(_p(case['dout']), None, _p(case['z']), _p(case['gamma']), _p(o.mean), _p(o.rstd), _p(o.y),
                                   None, _p(o.scale), _p(o.shift), _p(t), 1 << 16, 8, 16, 1, ops.DT_F32, _stream())
    assert st == -22                                        # relu without the saved output
    torch.cuda.synchronize()
    assert not torch.equal(before[0], o.rm) and not torch.equal(before[1], o.rv)        # (only the accepted call ran)


# ---- running statistics through the module path ---------------------------------------------------------------------------
@pytest.mark.parametrize('momentum', [0.1, None])
def test_running_statistics_over_three_calls(momentum):
    bn = torch.nn.BatchNorm2d(64, momentum=momentum).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(1 + 0.3 * torch.randn(64, generator=torch.Generator().manual_seed(1)))
        bn.bias.copy_(0.2 * torch.randn(64, generator=torch.Generator().manual_seed(2)))
    for k in range(1, 4):
        case = B.make_case(2 * 7 * 5, 64, bf16, 60 + k, mean=0.5 * k, device=DEV)
        rm, rv = bn.running_mean.clone(), bn.running_var.clone()
        v0 = (bn.running_mean._version, bn.running_var._version)
        m = 0.1 if momentum is not None else 1.0 / k
        with torch.no_grad():
            y = bn_train_act_autograd(case['z'].view(2, 7, 5, 64), bn, None, True)
        gm, bt = bn.weight.detach(), bn.bias.detach()
        f = B.bn_forward64(case['z'], gm, bt, bn.eps, True, None, rm, rv, m)
        assert int(bn.num_batches_tracked) == k
        assert bn.running_mean._version > v0[0] and bn.running_var._version > v0[1]
        r = (_ratio(bn.running_mean, f.new_rm, B.running_mean_bound(f)), _ratio(bn.running_var, f.new_rv, B.running_var_bound(f)),
             _ratio(y.view(-1, 64), f.y, R.bound(f.y, bf16, B.y_extra(f))))
        assert all(v <= 1.0 for v in r), (k, r)
        # unbiased: the biased form misses by m var / (n - 1), far outside the bound
        w = B.bn_forward64(case['z'], gm, bt, bn.eps, True, None, rm, rv, m, biased_running=True)
        assert _ratio(bn.running_var, w.new_rv, B.running_var_bound(f)) > 20


def test_one_value_per_channel_raises_torchs_error():
    bn = torch.nn.BatchNorm2d(64).to(DEV).train()
    with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
        bn_train_act_autograd(torch.randn(1, 1, 1, 64, device=DEV), bn)
    assert int(bn.num_batches_tracked) == 0 and bool((bn.running_mean == 0).all())


# ---- mutation legs: the bounds can tell a wrong formula from the right one --------------------------------------------------
@pytest.mark.parametrize('mode', list(MODES))
def test_mutated_references_exceed_the_bounds(mode):
    dt = MODES[mode]
    case = B.make_case(257, 64, dt, 71, residual=True, device=DEV)
    f = B.bn_forward64(case['z'], case['gamma'], case['beta'], B.EPS, True, case['res'], case['rm'], case['rv'], 0.1)
    o = _backward(case, _forward(case, True), True)
    mask = o.y > 0
    w = B.bn_forward64(case['z'], case['gamma'], case['beta'], B.EPS, True, case['res'], case['rm'], case['rv'], 0.1,
                       biased_running=True)
    r_right, r_wrong = _ratio(o.rv, f.new_rv, B.running_var_bound(f)), _ratio(o.rv, w.new_rv, B.running_var_bound(w))
    b, wb = B.bn_backward64(case['dout'], f, mask), B.bn_backward64(case['dout'], f, mask, drop_dgamma_term=True)
    d_right = _ratio(o.dz, b.dz, R.bound(b.dz, dt, B.dz_extra(f, b)))
    d_wrong = _ratio(o.dz, wb.dz, R.bound(wb.dz, dt, B.dz_extra(f, wb)))
    print(f'running_var: right {r_right:.3f} biased {r_wrong:.1f};  dz: right {d_right:.3f} without xh dgamma / n {d_wrong:.1f}')
    assert r_right <= 1 and d_right <= 1
    assert r_wrong > 5 and d_wrong > 5


# ---- bit-reproducibility ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_five_calls_give_the_same_bits(mode):
    case = B.make_case(131073, 64, MODES[mode], 23, residual=True, device=DEV)
    first = None
    for _ in range(5):
        o = _backward(case, _forward(case, True), True)
        got = (o.mean, o.rstd, o.var, o.scale, o.shift, o.rm, o.rv, o.dgamma, o.dbeta, o.dz, o.dres)
        if first is None:
            first = got
        else:
            assert all(torch.equal(a, b) for a, b in zip(first, got))


# ---- the version bump ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['f32', 'bf16'])
def test_eval_forward_after_a_train_forward_folds_the_updated_statistics(mode):
    dt = MODES[mode]
    g = torch.Generator().manual_seed(5)
    conv = torch.nn.Conv2d(64, 64, 1, bias=False).to(DEV)
    bn = torch.nn.BatchNorm2d(64).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(64, 64, 1, 1, generator=g) * 0.2)
        bn.running_mean.copy_(torch.randn(64, generator=g))
    cache = blocks.PackedCache()
    x = (torch.randn(2, 9, 11, 64, generator=g) + 1.0).to(dt).to(DEV)
    try:
        blocks.set_compute_dtype(mode)
        with torch.no_grad():
            bn.eval()
            y0 = conv_bn_act_nhwc(x, conv, bn, cache, True)             # fills the cache with the OLD fold
            rm0 = bn.running_mean.clone()
            bn.train()
            conv_bn_act_nhwc(x, conv, bn, cache, True)
            bn.eval()
            y1 = conv_bn_act_nhwc(x, conv, bn, cache, True)
    finally:
        blocks.set_compute_dtype('f32')
    assert not torch.equal(rm0, bn.running_mean) and int(bn.num_batches_tracked) == 1
    raw = F.conv2d(x.double().permute(0, 3, 1, 2), conv.weight.detach().to(dt).double()).permute(0, 2, 3, 1)
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    ref = (raw * s + (bn.bias.double() - bn.running_mean.double() * s)).relu()
    assert R.excess(y1, ref, dt) <= 0
    assert R.excess(y0, ref, dt) > 0, 'the old fold is another function: the test can tell'


# ---- whole blocks against float64 autograd --------------------------------------------------------------------------------
def _seed_module(m, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k, p in sorted(m.state_dict().items()):
            if k.endswith('num_batches_tracked'):
                continue
            if k.endswith('running_var'):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            elif k.endswith('running_mean') or k.endswith('.bias'):
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            elif k.endswith('bn3.weight'):
                p.copy_(torch.rand(p.shape, generator=g) * 0.2 + 0.2)
            elif p.dim() == 1:
                p.copy_(torch.rand(p.shape, generator=g) + 0.5)
            else:
                fan_in = p[0].numel()
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / fan_in) ** 0.5 * (0.1 if '.conv_offset.' in k else 1))
    return m


def _block(kind, stride, seed=41):
    down = None
    if stride != 1:
        down = torch.nn.Sequential(torch.nn.Conv2d(256, 256, 1, stride=stride, bias=False), torch.nn.BatchNorm2d(256))
    if kind == 'x':
        blk = BottleneckX(256, 64, stride, down, groups=32, base_width=4)
    elif kind == 'dcn':
        blk = Bottleneck(256, 64, stride, down, dcn=dict(type='DCN', deform_groups=1, fallback_on_stride=False))
    else:
        blk = Bottleneck(256, 64, stride, down)
    return _seed_module(blk, seed).to(DEV)


def _set_modes(blk, training):
    """`training`: names of the BatchNorms in training mode ('all' = every one, the downsample's included)"""
    blk.eval()
    for name, m in blk.named_modules():
        if isinstance(m, torch.nn.BatchNorm2d) and (training == 'all' or name in training):
            m.train()


def _rnd(w, dt):
    """the operand the kernels saw: the weight rounded to the dtype (the gradient of a master weight is the gradient at its
    rounded value: derivative 1)"""
    return w if dt == f32 else w + (w.detach().to(dt).double() - w.detach())


def _conv64(x, conv, dt):
    w = _rnd(conv.weight, dt)
    return F.conv2d(x.permute(0, 3, 1, 2), w, None, conv.stride, conv.padding, 1, conv.groups).permute(0, 2, 3, 1)


class _Ref64:
    """the block in float64, differentiable, AT THE FORWARD THE KERNELS RAN (tests/test_resnet_dcn_gpu.py has the reasons):
    16-bit legs take the conv weights rounded to the dtype and round every raw conv output the kernels store once
    (derivative 1); every leg takes the ReLU pass masks from the kernels' own stage outputs and the values of conv1's,
    conv2's and the downsample's stage outputs from the kernels outright (derivative 1 again).  A BatchNorm in training mode normalises with the batch statistics of the stored raw conv output,
    differentiably; one in eval mode folds its (untouched) running statistics."""

    def __init__(self, blk, ref_blk, dt, seen, train_flags):
        self.blk, self.ref, self.dt, self.seen, self.train = blk, ref_blk, dt, seen, train_flags

    def st(self, t):
        return t if self.dt == f32 else t + (t.detach().to(self.dt).double() - t.detach())

    def bn(self, z, name):
        bn = dict(self.ref.named_modules())[name]
        if self.train[name]:
            mean = z.mean((0, 1, 2))
            var = ((z - mean) ** 2).mean((0, 1, 2))
            s = bn.weight / torch.sqrt(var + B.f32(bn.eps))
            return z * s + (bn.bias - mean * s), s
        s = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        return z * s + (bn.bias - bn.running_mean * s), s

    def stage(self, x, conv, bn_name, key, res=None, relu=True):
        """conv -> (stored) -> bn (+ res) (+ ReLU by the kernel's mask); with `key` the kernel's own value stands in"""
        raw = _conv64(x, conv, self.dt) if not isinstance(conv, torch.Tensor) else conv
        pre, s = self.bn(self.st(raw), bn_name)
        if res is not None:
            pre = pre + res
        out = pre * (self.seen[key].detach() > 0).double() if relu else pre
        self.last = (raw.detach(), s.detach(), pre.detach().relu() if relu else pre.detach())
        if key != 'y':      # (every stage's reference is held to float64 on the input that stage SAW: _check_forward)
            return out + (self.seen[key].detach().double() - out.detach())
        return self.st(out)

    def forward(self, x, checks):
        r, seen = self.ref, self.seen
        o1 = self.stage(x, r.conv1, 'bn1', 'o1')
        checks.append(('o1', seen['o1'], *self.last))
        if getattr(r, 'with_dcn', False):
            c2 = r.conv2
            om = F.conv2d(o1.permute(0, 3, 1, 2), _rnd(c2.conv_offset.weight, self.dt), c2.conv_offset.bias, c2.stride,
                          1).permute(0, 2, 3, 1)
            raw2 = DG.deform_conv64(o1, om, _rnd(c2.weight, self.dt).permute(0, 2, 3, 1), c2.deform_groups, c2.modulated,
                                    self.blk.conv2_stride, 1)
            o2 = self.stage(o1, raw2, 'bn2', 'o2')
            # (the forward check of this stage takes the kernel's own raw deformable output: the sampling has its own tests)
            pre, s = self.bn(seen['raw2'].detach().double(), 'bn2')
            checks.append(('o2', seen['o2'], seen['raw2'].detach().double(), s.detach(), pre.detach().relu()))
        else:
            o2 = self.stage(o1, r.conv2, 'bn2', 'o2')
            checks.append(('o2', seen['o2'], *self.last))
        if r.downsample is None:
            idn = x
        else:
            idn = self.stage(x, r.downsample[0], 'downsample.1', 'idn', relu=False)
            checks.append(('idn', seen['idn'], *self.last))
        y = self.stage(o2, r.conv3, 'bn3', 'y', res=idn)
        checks.append(('y', seen['y'], *self.last))
        return y


def _run_block(blk, x, go, mode, grad=True):
    """the block's forward (+ backward) with every stage's output recorded: {'o1', 'o2', 'idn', 'y', 'raw2' (DCN)}"""
    seen = {}
    inner, tail = backbones.conv_bn_act_nhwc, backbones.conv_bn_act_tail
    names = {id(blk.conv1): 'o1', id(blk.conv2): 'o2', id(blk.conv3): 'y'}
    if blk.downsample is not None:
        names[id(blk.downsample[0])] = 'idn'

    def spy(x_, conv, *a, **k):
        out = inner(x_, conv, *a, **k)
        seen[names[id(conv)]] = out[0] if isinstance(out, tuple) else out
        return out

    def tail_spy(y_, *a, **k):
        seen['raw2'] = y_
        seen['o2'] = tail(y_, *a, **k)
        return seen['o2']
    backbones.conv_bn_act_nhwc, backbones.conv_bn_act_tail = spy, tail_spy
    try:
        blocks.set_compute_dtype(mode)
        if grad:
            y = blk.forward_nhwc(x)
            y.backward(go)
        else:
            with torch.no_grad():
                y = blk.forward_nhwc(x)
    finally:
        backbones.conv_bn_act_nhwc, backbones.conv_bn_act_tail = inner, tail
        blocks.set_compute_dtype('f32')
    assert y.dtype == MODES[mode]
    return y, seen


def _check_forward(checks, dt):
    """each stage held to float64 on the input that stage saw: the result's own rounding and accumulation slack
    (route_util.bound) + the rounding of the stored raw conv output through |scale| (16 bits: the kernels form the
    activation from the stored value; twice, since the float64 side's rounding may fall on the other side of a tie)"""
    hu = R.half_ulp(dt) * 1.001
    for key, got, raw, s, ref in checks:
        e = R.excess(got.detach(), ref, dt, 2 * hu * raw.abs() * s.abs())
        print(f'training forward {key}: largest error minus bound {e:.3e}')
        assert e <= 0, (key, e)


def _check_block(kind, stride, mode, training, grad=True):
    dt = MODES[mode]
    blk = _block(kind, stride)
    _set_modes(blk, training)
    flags = {n: m.training for n, m in blk.named_modules() if isinstance(m, torch.nn.BatchNorm2d)}
    stats0 = {n: (m.running_mean.clone(), m.running_var.clone()) for n, m in blk.named_modules()
              if isinstance(m, torch.nn.BatchNorm2d)}
    ref_blk = copy.deepcopy(blk).double()
    g = torch.Generator().manual_seed(43)
    x = torch.randn(2, 13, 17, 256, generator=g).to(dt).to(DEV)
    go = torch.randn(2, (13 - 1) // stride + 1, (17 - 1) // stride + 1, 256, generator=g).to(dt).to(DEV)
    xg = x.clone().requires_grad_(grad)
    y, seen = _run_block(blk, xg, go, mode, grad)
    # forward, stage by stage, and the gradient reference at that forward
    checks = []
    xr = x.double().requires_grad_()
    ref = _Ref64(blk, ref_blk, dt, seen, flags)
    yr = ref.forward(xr, checks)
    _check_forward(checks, dt)
    # running statistics: moved where the BatchNorm trains (momentum 0.1, unbiased), untouched elsewhere
    mods = dict(blk.named_modules())
    key_of = {'bn1': 'o1', 'bn2': 'o2', 'bn3': 'y', 'downsample.1': 'idn'}
    raws = {k: raw for k, _, raw, _, _ in checks}
    for n, (rm0, rv0) in stats0.items():
        bn = mods[n]
        if not flags[n]:
            assert torch.equal(bn.running_mean, rm0) and torch.equal(bn.running_var, rv0) and int(bn.num_batches_tracked) == 0
            continue
        assert int(bn.num_batches_tracked) == 1
        z = raws[key_of[n]].reshape(-1, rm0.numel())
        z = z.to(dt) if dt != f32 else z
        f = B.bn_forward64(z, bn.weight.detach(), bn.bias.detach(), bn.eps, False, None, rm0, rv0, 0.1)
        # (the float64 side rounds its own raw conv output: where the kernel's fp32 accumulation falls on the other side of a
        # tie one value of ~n differs by an ulp, m ulp / n of the statistic -- inside ACC_TOL at these sizes)
        rmean = _ratio(bn.running_mean, f.new_rm, B.running_mean_bound(f))
        rvar = _ratio(bn.running_var, f.new_rv, B.running_var_bound(f))
        print(f'{n}: running_mean {rmean:.3f}  running_var {rvar:.3f} (error / bound)')
        assert rmean <= 1 and rvar <= 1, (n, rmean, rvar)
    if not grad:
        assert not y.requires_grad
        return
    yr.backward(go.double())
    got, want = {'x': xg.grad}, {'x': xr.grad}
    p, pr = dict(blk.named_parameters()), dict(ref_blk.named_parameters())
    for k in p:
        if k.startswith('conv2.conv_offset'):
            continue        # (tests/test_resnet_dcn_gpu.py holds the offset branch; its reference needs the kernels' offsets)
        got[k], want[k] = p[k].grad, pr[k].grad
    tol = {bf16: 1e-2, f16: 2e-3}.get(dt)
    bad = []
    for k in got:
        gk, rk = got[k].double(), want[k]
        assert gk.shape == rk.shape and bool(torch.isfinite(gk).all()) and float(rk.abs().max()) > 0, k
        rel = (gk - rk).abs().max().item() / rk.abs().max().item()
        cos = (torch.dot(gk.flatten(), rk.flatten()) / (gk.norm() * rk.norm())).item()
        print(f'{k}: relative error {rel:.3e}  cosine {cos:.6f}')
        if dt == f32:
            ok = R.excess(got[k], rk, f32) <= 0
        elif k == 'x':
            ok = rel < tol
        else:
            ok = cos > 0.999
        if not ok:
            bad.append((k, rel, cos))
    assert not bad, bad


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('mode', list(MODES))
def test_bottleneck_all_batchnorms_training(mode, stride):
    _check_block(None, stride, mode, 'all')


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('mode', list(MODES))
def test_bottleneck_only_bn2_training(mode, stride):
    """the mixed single-consumer case: conv1 (eval) hands out a BnTail, conv2's training BatchNorm does not run it (conv1's
    node does its own backward), and conv3 (eval, `sole_consumer`) finds no tail on conv2's output"""
    _check_block(None, stride, mode, ('bn2',))


@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('mode', list(MODES))
def test_bottleneck_training_batchnorms_under_no_grad(mode, stride):
    _check_block(None, stride, mode, 'all', grad=False)


@pytest.mark.parametrize('mode', list(MODES))
def test_resnext_bottleneck_training(mode):
    _check_block('x', 1, mode, 'all')


@pytest.mark.parametrize('mode', list(MODES))
def test_dcn_bottleneck_training(mode):
    _check_block('dcn', 1, mode, 'all')


def test_stem_and_whole_backbone_in_training_mode():
    """frozen_stages=-1, norm_eval=False: the stem's conv_bn_act_nhwc route (forward_from_nchw steps aside for a training
    bn1) against float64 autograd of bn1's parameters, then the whole backbone under no_grad (a recalibration pass): every
    BatchNorm counts the batch.  (The stem conv's own weight gradient is not part of this: the weight-gradient kernel does
    not take 3 input channels, whatever the BatchNorm mode, so conv1.weight is frozen here.)"""
    from brcnn.backbones import ResNet
    m = _seed_module(ResNet(depth=50, frozen_stages=-1, norm_eval=False), 47).to(DEV).train()
    bns = [b for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]
    assert len(bns) == 53 and all(b.training for b in bns)
    m.conv1.weight.requires_grad_(False)
    g = torch.Generator().manual_seed(48)
    img = torch.randn(2, 3, 64, 96, generator=g).to(DEV)
    go = torch.randn(2, 32, 48, 64, generator=g).to(DEV)
    rm0, rv0 = m.bn1.running_mean.clone(), m.bn1.running_var.clone()
    y = conv_bn_act_nhwc(blocks.to_nhwc(img), m.conv1, m.bn1, m._stem_cache, True)
    y.backward(go)
    ref = copy.deepcopy(m.bn1).double()
    ref.weight.grad = ref.bias.grad = None
    z = F.conv2d(img.double(), m.conv1.weight.double(), None, 2, 3).permute(0, 2, 3, 1)
    mean, var = z.mean((0, 1, 2)), z.var((0, 1, 2), unbiased=False)
    s = ref.weight / torch.sqrt(var + B.f32(m.bn1.eps))
    pre = z * s + (ref.bias - mean * s)
    assert R.excess(y.detach(), pre.detach().relu(), f32) <= 0
    (pre * (y.detach() > 0).double()).backward(go.double())
    assert R.excess(m.bn1.weight.grad, ref.weight.grad, f32) <= 0 and R.excess(m.bn1.bias.grad, ref.bias.grad, f32) <= 0
    f = B.bn_forward64(z.reshape(-1, 64), m.bn1.weight.detach(), m.bn1.bias.detach(), m.bn1.eps, False, None, rm0, rv0, 0.1)
    assert _ratio(m.bn1.running_mean, f.new_rm, B.running_mean_bound(f)) <= 1
    assert _ratio(m.bn1.running_var, f.new_rv, B.running_var_bound(f)) <= 1
    with torch.no_grad():
        outs = m.forward_from_nchw(img)
    assert len(outs) == 4 and all(bool(torch.isfinite(o).all()) for o in outs)
    assert int(m.bn1.num_batches_tracked) == 2 and all(int(b.num_batches_tracked) == 1 for b in bns if b is not m.bn1)


# ---- the recipe -------------------------------------------------------------------------------------------------------------
def _two_steps():
    from brcnn.optim import FusedSGD
    m = build_detector(Config.fromfile(RECIPE).model)
    m.load_state_dict(util.seeded_state_dict(m, seed=10))
    m = m.to(DEV).train()
    m.set_compute_dtype('bf16')
    opt = FusedSGD([p for p in m.parameters() if p.requires_grad], lr=0.002, momentum=0.9, weight_decay=1e-4)
    img, metas, gts, gls = util.demo_inputs(2, 128, 160, num_classes=4, seed=10)
    losses = []
    for step in range(2):
        torch.manual_seed(77 + step)
        opt.zero_grad()
        out = m.forward_train(img.to(DEV), metas, [g_.to(DEV) for g_ in gts], [l.to(DEV) for l in gls])
        loss, log_vars = m._parse_losses(out)
        loss.backward()
        opt.step()
        losses.append(log_vars['loss'])
    torch.cuda.synchronize()
    return m, losses


def test_recipe_two_train_steps_move_the_statistics_and_repeat_bit_for_bit():
    try:
        ref = build_detector(Config.fromfile(RECIPE).model)
        assert ref.backbone.norm_eval is False and ref.backbone.frozen_stages == 1
        sd0 = util.seeded_state_dict(ref, seed=10)
        m, losses = _two_steps()
        assert all(np.isfinite(v) for v in losses), losses
        moved = still = 0
        for name, mod in m.backbone.named_modules():
            if not isinstance(mod, torch.nn.BatchNorm2d):
                continue
            rm0, rv0 = sd0[f'backbone.{name}.running_mean'].to(DEV), sd0[f'backbone.{name}.running_var'].to(DEV)
            if name.startswith(('layer2.', 'layer3.', 'layer4.')):
                assert mod.training, name
                assert int(mod.num_batches_tracked) == int(sd0[f'backbone.{name}.num_batches_tracked']) + 2, name
                assert bool((mod.running_mean != rm0).any()) and bool((mod.running_var != rv0).any()), name
                assert bool(torch.isfinite(mod.running_mean).all()) and bool((mod.running_var > 0).all()), name
                moved += 1
            else:       # the stem and stage 1 are frozen: eval mode, statistics as loaded
                assert not mod.training and int(mod.num_batches_tracked) == int(sd0[f'backbone.{name}.num_batches_tracked'])
                assert torch.equal(mod.running_mean, rm0) and torch.equal(mod.running_var, rv0), name
                still += 1
        assert moved == 3 * (4 + 6 + 3) + 3 and still == 1 + 3 * 3 + 1, (moved, still)
        m2, losses2 = _two_steps()
        assert losses == losses2
        a, b = m.state_dict(), m2.state_dict()
        assert all(torch.equal(a[k], b[k]) for k in a), [k for k in a if not torch.equal(a[k], b[k])][:5]
    finally:
        blocks.set_compute_dtype('f32')
