"""the DCNv2 convs of the r2_101 recipes at batch 8 x 800 x 1344 (stages 2 / 3 / 4, the stage-opening stride-2 conv and the
stride-1 one): the fused 16-bit kernel (csrc/deform_conv_bf16.hip) against the 16-bit im2col + GEMM pair and the fp32 pair.
Per variant: time per conv (us), TF/s of the conv's 2 * M * Cout * 9 * Cp flops, and the algorithmic HBM bytes (x, the
27 offset / mask floats per pixel, the weights, the output; the pairs also write and re-read the column matrix).
usage: python tools/deform_bench.py [bf16|f16] [reps]"""
import os
import sys

sys.path.insert(0, os.getcwd())
import torch

import brcnn  # noqa: F401
from brcnn import ops

DT = {'bf16': torch.bfloat16, 'f16': torch.float16}[sys.argv[1] if len(sys.argv) > 1 else 'bf16']
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
N = 8
# (name, H, W of the input map, stride, split width): Res2Net-101 26w x 4s, splits 52 / 104 / 208 channels
SHAPES = [('s2 open  s2', 200, 336, 2, 52), ('s2 block s1', 100, 168, 1, 52), ('s3 open  s2', 100, 168, 2, 104),
          ('s3 block s1', 50, 84, 1, 104), ('s4 open  s2', 50, 84, 2, 208), ('s4 block s1', 25, 42, 1, 208)]


def pad(n, m):
    return (n + m - 1) // m * m


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / REPS * 1e3      # us


def main():
    g = torch.Generator(device='cuda').manual_seed(0)
    print(f'# DCNv2 3x3 convs of r2_101, batch {N}, 800x1344; 16-bit = {DT}; {REPS} timed reps after 3 warm-up')
    print(f'{"conv":12s} {"Cp16":>4s} {"Cp32":>4s} {"M":>7s} | {"fused16 us":>10s} {"TF/s":>5s} {"MB":>6s} | '
          f'{"pair16 us":>9s} {"TF/s":>5s} {"MB":>6s} | {"pair32 us":>9s} {"TF/s":>5s} {"MB":>6s} | fused/pair16')
    for name, h, w, stride, width in SHAPES:
        ho, wo = ops.conv_out_size(h, w, 3, 3, stride, 1)
        m = N * ho * wo
        row = f'{name:12s}'
        cp16, cp32 = pad(width, 64), pad(width, 32)
        row += f' {cp16:4d} {cp32:4d} {m:7d}'
        om = (torch.randn(N, ho, wo, 27, device='cuda', generator=g) * 2).contiguous()
        res = {}
        for tag, cp, dt in (('fused16', cp16, DT), ('pair16', cp16, DT), ('pair32', cp32, torch.float32)):
            x = torch.randn(N, h, w, cp, device='cuda', generator=g).to(dt)
            wt = (torch.randn(cp, 3, 3, cp, device='cuda', generator=g) / (3 * cp ** 0.5)).to(dt)
            sc, sh = torch.ones(cp, device='cuda'), torch.zeros(cp, device='cuda')
            es = 2 if dt != torch.float32 else 4
            base = N * h * w * cp * es + m * 27 * 4 + cp * 9 * cp * es + m * cp * es
            if tag == 'fused16':
                fn = lambda: ops.deform_conv_nhwc(x, om, wt, sc, sh, True, stride, 1)  # noqa: E731
                nbytes = base
            else:
                w2 = wt.view(cp, 1, 1, 9 * cp)

                def fn(x=x, w2=w2, cp=cp):
                    col, _ = ops.deform_im2col_nhwc(x, om, 3, stride, 1, 1)
                    return ops.conv2d_nhwc(col.view(m, 1, 1, 9 * cp), w2, sc, sh, None, True, 1, 0)
                nbytes = base + 2 * m * 9 * cp * es
            us = timed(fn)
            res[tag] = us
            row += f' | {us:10.1f} {2.0 * m * cp * 9 * cp / us / 1e6:5.1f} {nbytes / 1e6:6.1f}'
        row += f' | {res["fused16"] / res["pair16"]:.2f}'
        print(row, flush=True)


if __name__ == '__main__':
    main()
