"""the DCNv2 convs of the r2_101 recipes at batch 8 x 800 x 1344 (stages 2 / 3 / 4, the stage-opening stride-2 conv and the
stride-1 one): the fused 16-bit kernel (csrc/deform_conv_bf16.hip) against the 16-bit im2col + GEMM pair and the fp32 pair.
Per variant: time per conv (us), TF/s of the conv's 2 * M * Cout * 9 * Cp flops, and the algorithmic HBM bytes (x, the
27 offset / mask floats per pixel, the weights, the output; the pairs also write and re-read the column matrix).
usage: python tools/deform_bench.py [bf16|f16] [reps]
       python tools/deform_bench.py [bf16|f16|f32] [reps] resnet
`resnet`: instead, the deformable conv2 of the ResNet-50 dconv_c3-c5 bottlenecks at the same batch (C = cout = 128 on
100 x 168, 256 on 50 x 84, 512 on 25 x 42 at stride 1, and the stride-2 conv of each stage's first block), DCN v1 and
DCNv2 (deform_groups 1): the fused kernel against im2col + GEMM in 16 bits (the route brcnn_deform_conv_route picks is
marked), or with f32 the fp32 im2col + GEMM route alone."""
import os
import sys

sys.path.insert(0, os.getcwd())
import torch

import brcnn  # noqa: F401
from brcnn import ops

DT = {'bf16': torch.bfloat16, 'f16': torch.float16, 'f32': torch.float32}[sys.argv[1] if len(sys.argv) > 1 else 'bf16']
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


# (name, H, W of conv2's input map, stride, planes): ResNet-50 stages c3 / c4 / c5
RESNET_SHAPES = [('c3 first s2', 200, 336, 2, 128), ('c3 block s1', 100, 168, 1, 128), ('c4 first s2', 100, 168, 2, 256),
                 ('c4 block s1', 50, 84, 1, 256), ('c5 first s2', 50, 84, 2, 512), ('c5 block s1', 25, 42, 1, 512)]


def main_resnet():
    g = torch.Generator(device='cuda').manual_seed(0)
    print(f'# deformable conv2 of ResNet-50 dconv_c3-c5, batch {N}, 800x1344; {DT}; {REPS} timed reps after 3 warm-up')
    if DT == torch.float32:
        print(f'{"conv":12s} {"C":>4s} {"M":>7s} | {"v1 im2col+GEMM us":>17s} {"TF/s":>5s} | {"v2 im2col+GEMM us":>17s} {"TF/s":>5s}')
    else:
        print(f'{"conv":12s} {"C":>4s} {"M":>7s} | {"v1 fused us":>11s} {"TF/s":>5s} {"v1 pair us":>10s} {"TF/s":>5s} fused/pair | '
              f'{"v2 fused us":>11s} {"TF/s":>5s} {"v2 pair us":>10s} {"TF/s":>5s} fused/pair | default route')
    for name, h, w, stride, c in RESNET_SHAPES:
        ho, wo = ops.conv_out_size(h, w, 3, 3, stride, 1)
        m = N * ho * wo
        x = torch.randn(N, h, w, c, device='cuda', generator=g).to(DT)
        wt = (torch.randn(c, 3, 3, c, device='cuda', generator=g) / (3 * c ** 0.5)).to(DT)
        sc, sh = torch.ones(c, device='cuda'), torch.zeros(c, device='cuda')
        w2 = wt.view(c, 1, 1, 9 * c)
        row = f'{name:12s} {c:4d} {m:7d}'
        flops = 2.0 * m * c * 9 * c
        for mod in (False, True):
            om = (torch.randn(N, ho, wo, 27 if mod else 18, device='cuda', generator=g) * 2).contiguous()

            def pair(om=om, mod=mod):
                col, _ = ops.deform_im2col_nhwc(x, om, 3, stride, 1, 1, None, 1, mod)
                return ops.conv2d_nhwc(col.view(m, 1, 1, 9 * c), w2, sc, sh, None, True, 1, 0)
            if DT == torch.float32:
                us = timed(pair)
                row += f' | {us:17.1f} {flops / us / 1e6:5.1f}'
                continue
            uf = timed(lambda: ops.deform_conv_nhwc(x, om, wt, sc, sh, True, stride, 1, 1, mod))
            up = timed(pair)
            row += f' | {uf:11.1f} {flops / uf / 1e6:5.1f} {up:10.1f} {flops / up / 1e6:5.1f} {uf / up:10.2f}'
        if DT != torch.float32:
            row += ' | ' + ('fused' if ops.deform_conv_route(x, c, stride, 1, 1) else 'im2col+GEMM')
        print(row, flush=True)


if __name__ == '__main__':
    if len(sys.argv) > 3 and sys.argv[3] == 'resnet':
        main_resnet()
    else:
        assert DT != torch.float32, 'f32 is the `resnet` table only'
        main()
