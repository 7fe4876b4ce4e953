"""Shared by the GPU tests that force a kernel route through a tuning hook:

* the route counters (csrc/policy.h Counters, read and cleared through brcnn_conv_set_tile(-9, n)): which kernel a launch
  really took -- a dispatcher that falls back makes a kernel-against-kernel comparison compare a kernel with itself;
* the float64 reference of the fused convolution, computed on the device from the dtype-representable operands, and the
  two bounds the suite uses against it (fp32: 2e-5 of the largest magnitude; 16-bit: one round-to-nearest-even of the
  result + that accumulation slack).  No shape of the suite needs more: the K loops reach 4608 terms.
"""
import torch
import torch.nn.functional as F

# brcnn_conv_set_tile(-9, n)
CONV_COUNTERS = ('pp_f32', 'pp_f32_rows', 'pp_f32_cols', 'pp_bf16', 'pp128', 'stream', 'sk_chain', 'sk_par', 'sk_wgs',
                 'tile', 'tile_rows', 'tile_cols', 'tile_waves', 'tile_stages', 'wgrad', 'wgrad_tile')
ACC_TOL = 2e-5          # the suite's fp32 accumulation slack, relative to the largest magnitude of the reference


def half_ulp(dtype):
    """largest relative move of one round-to-nearest-even into `dtype` (0 for fp32 results: they are not rounded again)"""
    return {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}[dtype]


def clear(L):
    assert L.brcnn_conv_set_tile(-9, -1) == 0


def take(L):
    """{name: count} of every conv route counter since the last clear / take; clears them"""
    return {name: L.brcnn_conv_set_tile(-9, i) for i, name in enumerate(CONV_COUNTERS)}


def conv_ref64(x, w, scale=None, shift=None, residual=None, relu=False, stride=1, pad=0, absolute=False):
    """float64 of act((x * w) . scale + shift + residual), NHWC x (N,H,W,Cin) and w (Cout,KH,KW,Cin) as the kernels take them;
    absolute = True: the same sum over the magnitudes of the terms of the K loop (|x| * |w|) . |scale|, nothing else"""
    xd, wd = x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2)
    if absolute:
        y = F.conv2d(xd.abs(), wd.abs(), None, stride, pad).permute(0, 2, 3, 1)
        return y * scale.double().abs() if scale is not None else y
    y = F.conv2d(xd, wd, None, stride, pad).permute(0, 2, 3, 1)
    if scale is not None:
        y = y * scale.double()
    if shift is not None:
        y = y + shift.double()
    if residual is not None:
        y = y + residual.double()
    return y.relu() if relu else y


def bound(ref, out_dtype, extra=None):
    """elementwise: half_ulp |ref| 1.001 (the result's one rounding) + ACC_TOL max(1, |ref|max) (+ `extra`, elementwise)"""
    b = half_ulp(out_dtype) * ref.abs() * 1.001 + ACC_TOL * max(1.0, ref.abs().max().item())
    return b if extra is None else b + extra


def excess(y, ref, out_dtype, extra=None):
    """largest |y - ref| - bound over the elements (<= 0: inside)"""
    return ((y.double() - ref).abs() - bound(ref, out_dtype, extra)).max().item()


def check_conv_against_fp64(y, x, w, scale, shift, residual, relu, stride, pad, what=''):
    """asserts the kernel result `y` against float64 at the suite's bound; returns the float64 reference"""
    ref = conv_ref64(x, w, scale, shift, residual, relu, stride, pad)
    e = excess(y, ref, y.dtype)
    print(f'fp64 leg {what}: largest error minus bound {e:.3e}')
    assert e <= 0, (what, e)
    return ref


def twice_the_bound_off(y, ref, extra=None):
    """`y` with its largest element moved by twice the bound: what an fp32 leg must refuse (an fp32 ulp, 6e-8 of the value,
    is below the suite's fp32 bound by construction; there the bit-equality legs notice an ulp)"""
    out = y.clone().contiguous()
    i = out.abs().view(-1).argmax()
    out.view(-1)[i] += 2 * bound(ref, y.dtype, extra).reshape(-1)[i].to(y.dtype)
    return out


def one_ulp_off(y, ref, extra=None):
    """`y` with ONE element moved to the neighbouring representable value of its dtype, away from `ref`: the element where
    that single step leaves the bound by most.  (What the fp64 legs must notice in a 16-bit result; an fp32 ulp, 6e-8 of
    the value, is below the fp32 bound by construction -- there the bit-equality legs notice it.)"""
    it = {4: torch.int32, 2: torch.int16}[y.element_size()]
    yi = y.contiguous().view(it)
    up = y.double() >= ref
    step = torch.where(up == (y > 0), 1, -1).to(it)         # bits + 1 moves away from zero, bits - 1 towards it
    cand = (yi + step).view(y.dtype)
    viol = (cand.double() - ref).abs() - bound(ref, y.dtype, extra)
    viol[(y == 0) | ~torch.isfinite(cand)] = -1.0
    i = viol.view(-1).argmax()
    out = y.clone().contiguous()
    out.view(-1)[i] = cand.view(-1)[i]
    assert int((out != y).sum()) == 1
    return out
