"""The fp32 64 x 64 conv kernel, plain launch (one workgroup per tile) against the persistent, balanced launch
(brcnn_conv_set_tile(-5, 2)), over the shapes this kernel serves in the fp32 inference pass at batch 8
(profiles/r06_conv_layers.txt).  Per shape: `reps` alternating rounds of `n` launches each; the medians, the spread
(max - min) of the plain rounds, and the verdict -- the persistent form wins where it is faster by more than that spread.
    python tools/f32_tile_persistent_bench.py [reps] [n]  > profiles/f32_tile_persistent.txt"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import brcnn  # noqa: F401
from brcnn import ops, lib

L = lib.load()
PYRAMID = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
SHAPES = [  # name, N, H, W (or level list), Cin, Cout, k, stride, pad, residual
    ('s3 1x1 256->1024 +res', 8, 50, 84, 256, 1024, 1, 1, 0, True),
    ('s2 1x1 128->512 +res', 8, 100, 168, 128, 512, 1, 1, 0, True),
    ('s2 1x1 512->128', 8, 100, 168, 512, 128, 1, 1, 0, False),
    ('s2 1x1 256->128', 8, 200, 336, 256, 128, 1, 1, 0, False),
    ('s1 1x1 256->64', 8, 200, 336, 256, 64, 1, 1, 0, False),
    ('s1 1x1 64->256', 8, 200, 336, 64, 256, 1, 1, 0, False),
    ('s1 1x1 64->64', 8, 200, 336, 64, 64, 1, 1, 0, False),
    ('rpn heads 3x3 256->54 x5 lvl', 8, PYRAMID, None, 256, 54, 3, 1, 1, False),
    ('s4 3x3 512->512', 8, 25, 42, 512, 512, 3, 1, 1, False),
    ('s4 1x1 2048->512', 8, 25, 42, 2048, 512, 1, 1, 0, False),
    ('s4 1x1 512->2048 +res', 8, 25, 42, 512, 2048, 1, 1, 0, True),
    ('s4 1x1 s2 1024->2048', 8, 50, 84, 1024, 2048, 1, 2, 0, False),
    ('neck 3x3 256->256 25x42', 8, 25, 42, 256, 256, 3, 1, 1, False),
    ('neck 1x1 2048->256', 8, 25, 42, 2048, 256, 1, 1, 0, False),
    ('neck 3x3 256->256 13x21', 8, 13, 21, 256, 256, 3, 1, 1, False),
    ('neck 3x3 256->256 7x11', 8, 7, 11, 256, 256, 3, 1, 1, False),
    ('fc 12544->1024', 2048, 1, 1, 12544, 1024, 1, 1, 0, False),
    ('fc 1024->1024', 2048, 1, 1, 1024, 1024, 1, 1, 0, False),
    ('fc 1024->21', 2048, 1, 1, 1024, 21, 1, 1, 0, False),
    ('s2 1x1 s2 256->512', 8, 200, 336, 256, 512, 1, 2, 0, False),
]


def timed(fn, n):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1000.0        # us per launch


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    per_cu = int(os.environ.get('F32_TILE_WGS_PER_CU', '-1'))      # workgroups per CU of the persistent launch (hook -7)
    if per_cu >= 0:
        assert L.brcnn_conv_set_tile(-7, per_cu) == 0
        print(f'# persistent launch: {per_cu} workgroups per CU (0: the occupancy query)')
    print(f'# plain vs persistent 64 x 64 fp32 launch, {reps} alternating rounds of {n} launches, us per launch')
    print(f'# {"shape":30s} {"M":>7s} {"N":>5s} {"K":>6s} {"tiles":>6s} {"nk":>4s} {"wgs":>5s} {"plain":>8s} {"spread":>7s} '
          f'{"persist":>8s} {"spread":>7s} {"gain":>7s}  verdict')
    for name, N, H, W, ci, co, k, st, pd, res in SHAPES:
        g = torch.Generator().manual_seed(1)
        w = (torch.randn(co, k, k, ci, generator=g) * 0.05).cuda()
        sc = (torch.rand(co, generator=g) + 0.5).cuda()
        sh = torch.randn(co, generator=g).cuda()
        if isinstance(H, list):
            sizes = H
            x = torch.randn(sum(N * h * ww for h, ww in sizes), ci, device='cuda')
            M = sum(N * h * ww for h, ww in sizes)
            r = torch.randn(M, co, device='cuda') if res else None
            fn = lambda: ops.conv2d_nhwc_multi(x, w, N, sizes, sc, sh, r, True, st, pd)[0]
        else:
            x = torch.randn(N, H, W, ci, device='cuda')
            ho, wo = ops.conv_out_size(H, W, k, k, st, pd)
            M = N * ho * wo
            r = torch.randn(N, ho, wo, co, device='cuda') if res else None
            fn = lambda: ops.conv2d_nhwc(x, w, sc, sh, r, True, st, pd)
        try:
            L.brcnn_conv_set_tile(-5, 0)
            ref = fn()
            L.brcnn_conv_set_tile(-5, 2)
            before = L.brcnn_conv_set_tile(-6, 0)
            out = fn()
            taken = L.brcnn_conv_set_tile(-6, 0) - before
            wgs = L.brcnn_conv_set_tile(-6, 1) if taken else 0
            assert torch.equal(out, ref), name
            for _ in range(3):
                fn()
            plain, pers = [], []
            for _ in range(reps):
                L.brcnn_conv_set_tile(-5, 0)
                fn()
                plain.append(timed(fn, n))
                if taken:
                    L.brcnn_conv_set_tile(-5, 2)
                    fn()
                    pers.append(timed(fn, n))
        finally:
            L.brcnn_conv_set_tile(-5, 1)
        med = lambda v: sorted(v)[len(v) // 2]
        K = k * k * ci
        tiles = ((M + 63) // 64) * ((co + 63) // 64)
        head = f'{name:32s} {M:7d} {co:5d} {K:6d} {tiles:6d} {K // 32:4d} {wgs:5d} {med(plain):8.1f} {max(plain) - min(plain):7.1f} '
        if not taken:
            print(head + f'{"-":>8s} {"-":>7s} {"-":>7s}  plain only (not this kernel, or fewer tiles than workgroups)')
            continue
        gain = med(plain) - med(pers)
        verdict = 'persistent' if gain > max(plain) - min(plain) else 'plain'
        print(head + f'{med(pers):8.1f} {max(pers) - min(pers):7.1f} {gain:7.1f}  {verdict}')
        del x, w, r, ref, out
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
