"""microbenchmark of the training-mode BatchNorm entries (csrc/bn_train.hip) on the ResNet-50 stage shapes of a
batch-8 800x1344 train step, with the eval-mode streams of csrc/bn_act.hip on the same shapes beside them in the same
run: time per entry (HIP events around ITERS back-to-back calls, after a warm-up) and the algorithmic bytes of the passes
inside it over that time.  Writes profiles/bn_train_bench_{f32,bf16}.txt.

Passes and their algorithmic bytes (E = rows x C x element size; the per-channel vectors and the partials are not counted):
    stats     brcnn_bn_train_stats      reduce pass reads z (1 E); the finalize launch is latency-sized
    apply     brcnn_bn_act_forward      reads z [+ res], writes out (2 E / 3 E)
    backward  brcnn_bn_train_backward   reduce pass reads dout, out, z (3 E); write pass reads them again and writes
                                        dz [+ dres] (4 E / 5 E): 7 E / 8 E for the entry
    eval fwd  brcnn_bn_eval_act_forward      2 E / 3 E
    eval bwd  brcnn_bn_eval_act_backward_ex  reads dout, z [+ out], writes dz [+ dres]: 3 E / 5 E
The per-kernel split of an entry (reduce / finalize / write) comes from a kernel trace of this script, not from here."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import brcnn  # noqa: E402,F401
from brcnn import lib as L  # noqa: E402
from brcnn.ops import _dt, _ptr  # noqa: E402

DEV = 'cuda:0'
ITERS = int(os.environ.get('BN_BENCH_ITERS', '50'))
# (rows, C, residual): stage outputs of R50 at 8 x 800 x 1344 -- 200x336, 100x168, 50x84, 25x42 maps
SHAPES = [(537600, 256, True), (134400, 128, False), (134400, 512, True), (33600, 256, False), (33600, 1024, True),
          (8400, 512, False), (8400, 2048, True)]


def timed(fn):
    for _ in range(5):
        assert fn() == 0
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / ITERS * 1e3        # us


def run(dtype, out):
    lib = L.load()
    tot = {}
    for rows, c, has_res in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(rows + c)
        z = (torch.randn(rows, c, device=DEV, generator=g) + 0.5).to(dtype)
        res = torch.randn(rows, c, device=DEV, generator=g).to(dtype) if has_res else None
        dout = torch.randn(rows, c, device=DEV, generator=g).to(dtype)
        y, dz = torch.empty_like(z), torch.empty_like(z)
        dres = torch.empty_like(z) if has_res else None
        gm, bt = torch.rand(c, device=DEV) + 0.5, torch.randn(c, device=DEV)
        rm, rv = torch.zeros(c, device=DEV), torch.ones(c, device=DEV)
        st4 = torch.empty(4, c, device=DEV)
        mean, rstd, scale, shift = st4[0], st4[1], st4[2], st4[3]
        dg, db = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        dt = _dt(z)
        nb = lib.brcnn_bn_train_workspace_bytes(rows, c, dt)
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        nbe = lib.brcnn_bn_act_backward_workspace_bytes(rows, c, dt)
        wse = torch.empty(max(nbe, 4), dtype=torch.uint8, device=DEV)
        E = z.numel() * z.element_size()
        r = int(has_res)
        entries = (
            ('stats', 1, lambda: lib.brcnn_bn_train_stats(_ptr(z), _ptr(gm), _ptr(bt), 1e-5, 0.1, _ptr(rm), _ptr(rv), _ptr(mean),
                                                          _ptr(rstd), None, _ptr(scale), _ptr(shift), _ptr(ws), nb, rows, c, dt,
                                                          None)),
            ('apply', 2 + r, lambda: lib.brcnn_bn_act_forward(_ptr(z), _ptr(scale), _ptr(shift), _ptr(res), _ptr(y), rows, c, 1, dt,
                                                              None)),
            ('backward', 7 + r, lambda: lib.brcnn_bn_train_backward(_ptr(dout), _ptr(y), _ptr(z), _ptr(gm), _ptr(mean), _ptr(rstd),
                                                                    _ptr(dz), _ptr(dres), _ptr(dg), _ptr(db), _ptr(ws), nb, rows, c,
                                                                    1, dt, None)),
            ('eval fwd', 2 + r, lambda: lib.brcnn_bn_eval_act_forward(_ptr(z), _ptr(gm), _ptr(bt), _ptr(rm), _ptr(rv), 1e-5,
                                                                      _ptr(res), _ptr(y), rows, c, 1, dt, None)),
            ('eval bwd', 3 + 2 * r, lambda: lib.brcnn_bn_eval_act_backward_ex(_ptr(dout), _ptr(y) if has_res else None, _ptr(z),
                                                                              _ptr(gm), _ptr(bt), _ptr(rm), _ptr(rv), 1e-5,
                                                                              _ptr(dz), _ptr(dres), _ptr(dg), _ptr(db), _ptr(wse),
                                                                              nbe, rows, c, 1, dt, None, 0)),
        )
        for name, streams, fn in entries:
            us = timed(fn)
            tot[name] = tot.get(name, 0.0) + us
            line = (f'rows {rows:7d} C {c:5d} res {r}  {name:9s} {us:9.1f} us  {streams} E = {streams * E / 1e6:8.1f} MB  '
                    f'{streams * E / us / 1e3:7.1f} GB/s')
            print(line, flush=True)
            out.write(line + '\n')
    line = 'sum over the seven shapes, us:  ' + '  '.join(f'{k} {v:.1f}' for k, v in tot.items())
    print(line)
    out.write(line + '\n')


def main():
    assert torch.cuda.is_available(), 'needs the device'
    os.makedirs(os.path.join(ROOT, 'profiles'), exist_ok=True)
    for name, dtype in (('f32', torch.float32), ('bf16', torch.bfloat16)):
        with open(os.path.join(ROOT, 'profiles', f'bn_train_bench_{name}.txt'), 'w') as out:
            out.write(f'tools/bn_train_bench.py, {name}, {ITERS} calls per figure (see the script for what E counts)\n')
            run(dtype, out)


if __name__ == '__main__':
    main()
