"""The fp32 Winograd entries (input transform + GEMM), plain launch of the GEMM (one workgroup per GEMM tile) against the
forced persistent, balanced launch (brcnn_conv_set_tile(-16, 2)) at the occupancy query's workgroups per CU and at two per
CU, each with two and with three LDS stages in the K loop ((-16, 42 / 43)), over the layer classes of the fp32 inference
pass at batch 8 and probes between them, and the five-level RPN tower with its GroupNorm prologue on both of its tiles.
Per shape: 30 warm-up launches, then `reps` alternating rounds of `n` launches per form; the medians, the spread (max - min)
of the rounds, and the verdict -- a form wins where it is faster than the plain two-stage launch by more than the spread of
that launch's rounds.  Every form is checked to give the plain launch's bits first.
    python tools/f32_winograd_persistent_bench.py [reps] [n]  > profiles/f32_winograd_persistent.txt"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import brcnn  # noqa: F401
from brcnn import ops, lib

L = lib.load()
PYRAMID = [(100, 168), (50, 84), (25, 42), (13, 21), (7, 11)]
LAYERS = [  # name, batch, H, W, channels
    ('256 ch  4 200 tiles', 1, 100, 168, 256),
    ('256 ch  6 300 tiles', 6, 50, 84, 256),
    ('256 ch  8 400 tiles', 8, 50, 84, 256),
    ('256 ch 33 600 tiles', 8, 100, 168, 256),
    ('256 ch  5 120 tiles (probe)', 10, 32, 64, 256),
    ('256 ch  8 192 tiles (probe)', 16, 32, 64, 256),
    ('256 ch 10 240 tiles (probe)', 20, 32, 64, 256),
    ('512 ch    616 tiles', 8, 13, 21, 512),
    ('512 ch  1 050 tiles', 1, 50, 84, 512),
    ('512 ch  2 184 tiles', 8, 25, 42, 512),
]
# name, (-16, mode), (-16, 30 + per-CU cap), (-16, 40 + LDS ring stages)
FORMS = [('plain      ring 2', 0, 0, 2), ('plain      ring 3', 0, 0, 3), ('pers/query ring 2', 2, 0, 2), ('pers/query ring 3', 2, 0, 3),
         ('pers/2     ring 2', 2, 2, 2), ('pers/2     ring 3', 2, 2, 3)]


def timed(fn, n):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1000.0        # us per call


def set_form(mode, per_cu, ring):
    assert L.brcnn_conv_set_tile(-16, mode) == 0 and L.brcnn_conv_set_tile(-16, 30 + per_cu) == 0
    assert L.brcnn_conv_set_tile(-16, 40 + ring) == 0


def run(name, fn, tiles, wg_tiles, reps, n):
    try:
        set_form(0, 0, 2)
        ref = fn()
        wgs, forms, seen = {}, [], set()
        for f in FORMS:
            set_form(*f[1:])
            L.brcnn_conv_set_tile(-16, 10)
            out = fn()
            took = L.brcnn_conv_set_tile(-16, 10)
            wgs[f[0]] = L.brcnn_conv_set_tile(-16, 11) if took else 0
            assert torch.equal(out, ref), (name, f[0])
            # a forced form that fell back to the plain launch, or plans the workgroups of one before it, is no form of its own
            key = (wgs[f[0]], f[3])
            if (f[1] == 0 or took) and key not in seen:
                seen.add(key)
                forms.append(f)
        assert L.brcnn_conv_handover_status() == 0
        set_form(0, 0, 2)
        for _ in range(30):
            fn()
        t = {f[0]: [] for f in forms}
        for _ in range(reps):
            for f in forms:
                set_form(*f[1:])
                fn()
                t[f[0]].append(timed(fn, n))
    finally:
        set_form(1, 0, 0)
    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: max(v) - min(v)
    base = t[FORMS[0][0]]
    best = min(t, key=lambda k: med(t[k]))
    verdict = best if med(base) - med(t[best]) > spread(base) else FORMS[0][0]
    for k in t:
        print(f'{name:30s} {tiles:6d} {wg_tiles:6d}  {k:18s} {wgs[k]:5d} {med(t[k]):8.1f} {spread(t[k]):7.1f} {med(base) - med(t[k]):7.1f}'
              + ('  <- verdict' if k == verdict else ''), flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f'# Winograd entry (transform + GEMM), forms of the GEMM launch, {cus} CUs; 30 warm-up launches, {reps} alternating rounds '
          f'of {n} launches, us per call')
    print('# plain: one workgroup per GEMM tile; pers/query: persistent at the occupancy query\'s workgroups per CU (fewer where the '
          'launch has fewer GEMM tiles: floor(tiles / CUs)); pers/2: at most two per CU; ring: LDS stages of the K loop.')
    print('# A form that the schedule sent to the plain launch, or that plans the workgroups of a form above it, is left out.  gain: '
          'against plain ring 2; verdict: the fastest form if its gain exceeds the spread of the plain ring 2 rounds')
    print(f'# {"shape":28s} {"tiles":>6s} {"wgtile":>6s}  {"form":18s} {"wgs":>5s} {"median":>8s} {"spread":>7s} {"gain":>7s}')
    g = torch.Generator().manual_seed(1)
    for name, N, H, W, c in LAYERS:
        x = torch.randn(N, H, W, c, generator=g).cuda()
        u = ops.winograd_filter((torch.randn(c, 3, 3, c, generator=g) * 0.02).cuda())
        sc, sh = (torch.rand(c, generator=g) + 0.5).cuda(), torch.randn(c, generator=g).cuda()
        tiles = N * ((H + 1) // 2) * ((W + 1) // 2)
        v = L.brcnn_winograd_layer_gemm_variant(tiles, c)
        bm, bn = {1: (64, 128), 2: (32, 128), 3: (64, 64)}[v]
        run(name, lambda: ops.conv3x3_winograd_layer(x, u, sc, sh, True), tiles, ((tiles + bm - 1) // bm) * (c // bn), reps, n)
        del x, u
        torch.cuda.empty_cache()
    # the tower: 256 -> 256 over the five levels at batch 8 with the GroupNorm + ReLU prologue
    c, groups, N = 256, 32, 8
    rows = sum(N * h * w for h, w in PYRAMID)
    x = torch.randn(rows, c, generator=g).cuda()
    u = ops.winograd_filter((torch.randn(c, 3, 3, c, generator=g) * 0.02).cuda())
    gamma, beta = (torch.rand(c, generator=g) + 0.5).cuda(), torch.randn(c, generator=g).cuda()
    stats = ops.groupnorm_stats_multi(x, groups, N, PYRAMID, 1e-5)
    tiles = sum(N * ((h + 1) // 2) * ((w + 1) // 2) for h, w in PYRAMID)
    fn = lambda: ops.conv3x3_winograd_multi(x, u, N, PYRAMID, gn=(stats, gamma, beta, groups, True))
    try:
        for v, (bm, bn) in ((1, (64, 128)), (3, (64, 64))):
            assert L.brcnn_conv_set_tile(-16, 20 + v) == 0
            run(f'tower 256 ch, tile {bm} x {bn}', fn, tiles, ((tiles + bm - 1) // bm) * (c // bn), reps, n)
    finally:
        L.brcnn_conv_set_tile(-16, 20)


if __name__ == '__main__':
    main()
