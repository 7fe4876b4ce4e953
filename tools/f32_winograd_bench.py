"""The fp32 3x3 stride-1 256 -> 256 layers of the inference pass at batch 8, direct implicit-GEMM conv against the Winograd
F(2x2,3x3) form (csrc/conv_winograd_f32.hip).  Per shape: `reps` alternating rounds of `n` launches each; the medians, the
spread (max - min) of the direct rounds, and the verdict -- Winograd wins where it is faster by more than that spread.
Rows: the RPN tower layer over the five pyramid levels (plain; with the GroupNorm + ReLU prologue against conv + the
GroupNorm apply pass, the statistics launches being common to both; in 1 / 2 / 4 / 8 transform + GEMM launch pairs), and the
neck's output convs per level.
    python tools/f32_winograd_bench.py [reps] [n]  > profiles/f32_winograd.txt"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import brcnn  # noqa: F401
from brcnn import ops, lib

L = lib.load()
PYRAMID = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]


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
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    N, C, G = 8, 256, 32
    print(f'# direct vs Winograd F(2x2,3x3), fp32 3x3 {C}->{C}, batch {N}, {reps} alternating rounds of {n} launches, us per call')
    print(f'# {"shape":44s} {"rows":>7s} {"tiles":>6s} {"direct":>8s} {"spread":>7s} {"winograd":>8s} {"spread":>7s} {"gain":>7s}  verdict')
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(C, 3, 3, C, generator=g) * 0.02).cuda()
    u = ops.winograd_filter(w)
    gamma = (torch.rand(C, generator=g) + 0.5).cuda()
    beta = torch.randn(C, generator=g).cuda()
    rows = [('tower 5 levels', PYRAMID, False, 1), ('tower 5 levels, 2 launch pairs', PYRAMID, False, 2),
            ('tower 5 levels, 4 launch pairs', PYRAMID, False, 4), ('tower 5 levels, 8 launch pairs', PYRAMID, False, 8),
            ('tower 5 levels + GroupNorm/ReLU prologue', PYRAMID, True, 1),
            ('tower 5 levels + prologue, 4 launch pairs', PYRAMID, True, 4)] + \
           [(f'neck {h}x{ww}', [(h, ww)], False, 1) for h, ww in PYRAMID[:3]]
    for name, sizes, prologue, chunks in rows:
        M = sum(N * h * ww for h, ww in sizes)
        tiles = sum(N * ((h + 1) // 2) * ((ww + 1) // 2) for h, ww in sizes)
        x = torch.randn(M, C, device='cuda')
        ws = ops.winograd_workspace(N, sizes, C, 'cuda')
        if prologue:
            _, stats = ops.groupnorm_nhwc_multi(x, gamma, beta, G, N, sizes, 1e-5, True, return_stats=True)
            direct = lambda: ops.conv2d_nhwc_multi(ops.groupnorm_nhwc_multi(x, gamma, beta, G, N, sizes, 1e-5, True), w, N, sizes,
                                                   None, None, None, False, 1, 1)[0]
            # (the direct leg launches the statistics too: time them alone and take them off)
            stat_only = lambda: ops.groupnorm_stats_multi(x, G, N, sizes, 1e-5)
            wino = lambda: ops.conv3x3_winograd_multi(x, u, N, sizes, gn=(stats, gamma, beta, G, True), workspace=ws)
        else:
            stat_only = None
            direct = lambda: ops.conv2d_nhwc_multi(x, w, N, sizes, None, None, None, False, 1, 1)[0]
            wino = lambda: ops.conv3x3_winograd_multi(x, u, N, sizes, workspace=ws)
        assert L.brcnn_conv_set_tile(-11, 10 + chunks) == 0
        try:
            ref, out = direct(), wino()
            err = (out - ref).abs().max().item() / ref.abs().max().item()
            for _ in range(2):
                direct(), wino()
            d, v = [], []
            for _ in range(reps):
                direct()
                t = timed(direct, n)
                if stat_only is not None:
                    t -= timed(stat_only, n)
                d.append(t)
                wino()
                v.append(timed(wino, n))
        finally:
            L.brcnn_conv_set_tile(-11, 11)
        med = lambda q: sorted(q)[len(q) // 2]
        gain = med(d) - med(v)
        verdict = 'winograd' if gain > max(d) - min(d) else 'direct'
        print(f'{name:46s} {M:7d} {tiles:6d} {med(d):8.1f} {max(d) - min(d):7.1f} {med(v):8.1f} {max(v) - min(v):7.1f} {gain:7.1f}  '
              f'{verdict}   (max |difference| / max |direct| {err:.1e})')
        del x, ws
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
