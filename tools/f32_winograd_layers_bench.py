"""The fp32 3x3 stride-1 layers of the inference pass outside the RPN tower (stage-2 / 3 / 4 conv2, the neck's output convs),
today's production launch (ops.conv2d_nhwc: the eight-phase or the persistent 64 x 64 kernel, whichever the dispatcher
picks) against the Winograd single-layer entry with each GEMM tile forced (1 = 64 x 128, 2 = 32 x 128, 3 = 64 x 64;
csrc/conv_winograd_f32.hip), all with the scale / shift / ReLU read-out.  The protocol of tools/f32_winograd_bench.py: `reps`
alternating rounds of `n` launches; medians in us; spread = max - min over the direct rounds; a variant wins where its gain
exceeds that spread.  Batch 8 (the headline) and batch 1 (latency_bs1_ms) of the 100x168 and 50x84 maps.
    python tools/f32_winograd_layers_bench.py [reps] [n]  > profiles/f32_winograd_layers.txt"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import brcnn  # noqa: F401
from brcnn import ops, lib

L = lib.load()
VARIANTS = ((1, '64x128'), (2, '32x128'), (3, '64x64'))
# (name, batch, H, W, channels)
SHAPES = [('neck fpn_convs[0] 100x168', 8, 100, 168, 256), ('stage-2 conv2 100x168', 8, 100, 168, 128),
          ('stage-3 conv2 / neck 50x84', 8, 50, 84, 256), ('stage-4 conv2 25x42', 8, 25, 42, 512), ('neck 25x42', 8, 25, 42, 256),
          ('neck fpn_convs[0] 100x168 bs1', 1, 100, 168, 256), ('stage-2 conv2 100x168 bs1', 1, 100, 168, 128),
          ('stage-3 conv2 / neck 50x84 bs1', 1, 50, 84, 256),
          # the rule's thresholds need a losing point below each winning one: batch 1 of stage 4, and smaller maps per class
          ('stage-4 conv2 25x42 bs1', 1, 25, 42, 512), ('probe 512 ch 13x21', 8, 13, 21, 512), ('probe 512 ch 50x84 bs1', 1, 50, 84, 512),
          ('probe 128 ch 25x42', 8, 25, 42, 128), ('probe 128 ch 50x84 bs1', 1, 50, 84, 128), ('probe 128 ch 50x84 bs2', 2, 50, 84, 128),
          ('probe 256 ch 50x84 bs4', 4, 50, 84, 256), ('probe 256 ch 50x84 bs6', 6, 50, 84, 256)]


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
    print(f'# direct (production dispatch) vs Winograd F(2x2,3x3) per GEMM tile, fp32 3x3 C->C with scale / shift / ReLU, '
          f'{reps} alternating rounds of {n} launches, us per call')
    print(f'# {"shape":34s} {"N":>2s} {"C":>4s} {"tiles":>6s} {"direct":>8s} {"spread":>7s} ' +
          ' '.join(f'{name:>8s} {"gain":>7s}' for _, name in VARIANTS) + '  verdict')
    g = torch.Generator().manual_seed(1)
    med = lambda q: sorted(q)[len(q) // 2]
    for name, N, H, W, C in SHAPES:
        tiles = N * ((H + 1) // 2) * ((W + 1) // 2)
        w = (torch.randn(C, 3, 3, C, generator=g) * (1.0 / (3.0 * C ** 0.5))).cuda()
        scale = (torch.rand(C, generator=g) + 0.5).cuda()
        shift = torch.randn(C, generator=g).cuda()
        x = torch.randn(N, H, W, C, device='cuda')
        u = ops.winograd_filter(w)
        direct = lambda: ops.conv2d_nhwc(x, w, scale, shift, None, True, 1, 1)
        wino = lambda: ops.conv3x3_winograd_layer(x, u, scale, shift, True)
        d, v, err = [], {k: [] for k, _ in VARIANTS}, 0.0
        try:
            ref = direct()
            for k, _ in VARIANTS:
                assert L.brcnn_conv_set_tile(-14, 20 + k) == 0
                out = wino()
                assert L.brcnn_conv_set_tile(-14, 11) == k
                err = max(err, (out - ref).abs().max().item() / ref.abs().max().item())
                wino()
            for _ in range(30):         # clocks up before the first round (the first shape's direct spread was 10 % without)
                direct()
            for _ in range(reps):
                direct()
                d.append(timed(direct, n))
                for k, _ in VARIANTS:
                    L.brcnn_conv_set_tile(-14, 20 + k)
                    wino()
                    v[k].append(timed(wino, n))
        finally:
            L.brcnn_conv_set_tile(-14, 20)
        spread = max(d) - min(d)
        gains = {k: med(d) - med(v[k]) for k, _ in VARIANTS}
        best = max(gains, key=gains.get)
        verdict = f'winograd {dict(VARIANTS)[best]}' if gains[best] > spread else 'direct'
        print(f'{name:36s} {N:2d} {C:4d} {tiles:6d} {med(d):8.1f} {spread:7.1f} ' +
              ' '.join(f'{med(v[k]):8.1f} {gains[k]:7.1f}' for k, _ in VARIANTS) +
              f'  {verdict}   (max |difference| / max |direct| {err:.1e})')
        del x, w, u
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
