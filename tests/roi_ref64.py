"""float64 RoIAlign (avg, aligned=True, adaptive sampling grid) in torch, its adjoint by autograd, and the inputs of the
chunked-gather test (tests/test_ops_gpu.py) with the condition that makes that test sensitive to one lost hit
(tests/test_roi_ref64_cpu.py checks helper and condition without a device).

RoIAlign is separable: a sample is skipped when its y OR its x lies outside, its bilinear weight is wy . wx, so bin
(p, q) of RoI k is  sum_hw Ay[k, p, h] x[c, h, w] Ax[k, q, w] / count  with Ay / Ax the per-axis sums of the sample
weights of bin row p / bin column q.  The per-RoI loop builds Ay and Ax (float64 geometry from the fp32 RoI values);
one einsum per image applies them, and autograd through that einsum is the adjoint.
"""
import math

import torch

SIZES = [(50, 84), (25, 42), (13, 21), (7, 11), (4, 6)]     # the pyramid of a 672 x 400 image
STRIDES = [8, 16, 32, 64, 128]
IMG_W, IMG_H = 672., 400.


def _axis(start, extent, pooled, size):
    """(pooled, size) float64: row p = summed bilinear weights of the samples of bin p along one axis; and the grid count"""
    bin_size = extent / pooled
    grid = int(math.ceil(extent / pooled))
    A = torch.zeros(pooled, size, dtype=torch.float64)
    for p in range(pooled):
        for i in range(grid):
            y = start + p * bin_size + (i + 0.5) * bin_size / grid
            if y < -1.0 or y > size:
                continue
            y = max(y, 0.0)
            lo = int(y)
            if lo >= size - 1:
                lo = hi = size - 1
                y = float(lo)
            else:
                hi = lo + 1
            A[p, lo] += 1.0 - (y - lo)
            A[p, hi] += y - lo
    return A, grid


def roi_align_f64(x, rois, pooled, spatial_scale):
    """x (N, C, H, W) float64 (may require grad), rois (K, 5) [image, x1, y1, x2, y2] -> (K, C, pooled, pooled) float64;
    avg mode, aligned=True, sampling_ratio = 0"""
    N, C, H, W = x.shape
    K = rois.shape[0]
    out = x.new_zeros(K, C, pooled, pooled)
    if K == 0:
        return out
    r = rois.detach().cpu().double()
    Ay = torch.zeros(K, pooled, H, dtype=torch.float64)
    Ax = torch.zeros(K, pooled, W, dtype=torch.float64)
    cnt = torch.ones(K, dtype=torch.float64)
    for k in range(K):
        x1, y1, x2, y2 = (r[k, 1:] * spatial_scale - 0.5).tolist()
        Ay[k], gh = _axis(y1, y2 - y1, pooled, H)
        Ax[k], gw = _axis(x1, x2 - x1, pooled, W)
        cnt[k] = max(gh * gw, 1)
    Ay, Ax, cnt = Ay.to(x.device), Ax.to(x.device), cnt.to(x.device)
    img = r[:, 0].long()
    pieces, order = [], []
    for b in range(N):
        idx = (img == b).nonzero().squeeze(1)
        for j in range(0, idx.numel(), 64):             # (64 RoIs at a time bound the (k, c, h, q) intermediate)
            i = idx[j:j + 64].to(x.device)
            t = torch.einsum('chw,kqw->kchq', x[b], Ax[i])
            pieces.append(torch.einsum('kph,kchq->kcpq', Ay[i], t) / cnt[i].view(-1, 1, 1, 1))
            order.append(i)
    return out.index_add(0, torch.cat(order), torch.cat(pieces))


def map_levels(rois, finest_scale=56, num_levels=5):
    """SingleRoIExtractor.map_roi_levels on the fp32 RoIs"""
    r = rois.detach().cpu().float()
    scale = torch.sqrt((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2]))
    return torch.floor(torch.log2(scale / finest_scale + 1e-6)).clamp(min=0, max=num_levels - 1).long()


def roi_extract_f64(feats_nhwc, rois, pooled=7, strides=STRIDES, finest_scale=56):
    """feats_nhwc: per level (B, H, W, C) float64 -> (K, pooled, pooled, C): every RoI pooled from its own level"""
    lv = map_levels(rois, finest_scale, len(feats_nhwc))
    out = feats_nhwc[0].new_zeros(rois.shape[0], pooled, pooled, feats_nhwc[0].shape[3])
    for l, f in enumerate(feats_nhwc):
        idx = (lv == l).nonzero().squeeze(1)
        if idx.numel():
            y = roi_align_f64(f.permute(0, 3, 1, 2), rois[idx], pooled, 1.0 / strides[l])
            out = out.index_add(0, idx.to(out.device), y.permute(0, 2, 3, 1))
    return out


def roi_extract_adjoint_f64(dy, rois, batch, sizes=SIZES, pooled=7, strides=STRIDES, finest_scale=56, device=None):
    """the gradient of roi_extract_f64 with respect to the pyramid for the output gradient dy (K, pooled, pooled, C):
    per level (B, H, W, C) float64, by autograd"""
    device = device or dy.device
    C = dy.shape[3]
    feats = [torch.zeros(batch, h, w, C, dtype=torch.float64, device=device, requires_grad=True) for h, w in sizes]
    out = roi_extract_f64(feats, rois, pooled, strides, finest_scale)
    grads = torch.autograd.grad(out, feats, dy.to(device).double(), allow_unused=True)
    return [torch.zeros_like(f) if g is None else g for f, g in zip(feats, grads)]       # (a level without RoIs)


# ---- the chunked-gather case -------------------------------------------------------------------------------------------
PILE = {torch.float32: 520, torch.float16: 120, torch.bfloat16: 12}    # RoIs on the piled tile the dtype's rounding still resolves one of
BORDER_0 = [[0, -80., -60., 30., 20.], [0, 650., 380., 720., 460.], [0, 100., 100., 101., 101.], [0, 300., 10., 310., 390.]]
BORDER_2 = [[2, -500., -500., -300., -300.], [2, 0., 0., 672., 400.]]   # hanging over, outside, tiny, huge (the earlier test's)


def _random_rois(n, image, g, lo=4., hi=500.):
    wh = lo + (hi - lo) * torch.rand(n, 2, generator=g) ** 2           # mostly small boxes: the fine levels and few-hit tiles
    xy = torch.rand(n, 2, generator=g) * torch.tensor([IMG_W, IMG_H])
    x1y1 = xy - wh / 2
    return torch.cat([torch.full((n, 1), float(image)), x1y1, x1y1 + wh], 1)


def _pile(n, image, g, x1, y1, x2, y2, jitter):
    j = torch.rand(n, 4, generator=g) * jitter
    box = torch.tensor([x1, y1, x2, y2]) + j * torch.tensor([1., 1., -1., -1.])
    return torch.cat([torch.full((n, 1), float(image)), box], 1)


def gather_case(channels, pile, seed=23):
    """800 RoIs over B = 3 images of 672 x 400, grouped by image, and dY uniform in [0.5, 1.5] (no cancellation: a dropped
    or doubled hit cannot hide in round-off).  Image 0: `pile` near-full-image RoIs first (level 3, the whole 7 x 11 map: both
    of its tiles collect every one of them -- more than the 512 of one collection batch when pile = 520), random RoIs, the
    border cases.  Image 1: none.  Image 2: a pile of 40 on a third of the image (level 2), random RoIs (tiles with a
    handful of hits: the direct path), two border cases.  -> rois (800, 5) fp32, dy (800, 7, 7, C) fp32"""
    g = torch.Generator().manual_seed(seed)
    n0 = 600 - pile - len(BORDER_0)
    rois = torch.cat([_pile(pile, 0, g, 0., 0., IMG_W, IMG_H, 30.), _random_rois(n0, 0, g), torch.tensor(BORDER_0),
                      _pile(40, 2, g, 20., 10., 380., 230., 20.), _random_rois(200 - 40 - len(BORDER_2), 2, g),
                      torch.tensor(BORDER_2)])
    assert rois.shape[0] == 800 and int((rois[:, 0] == 0).sum()) == 600 and int((rois[:, 0] == 1).sum()) == 0
    dy = torch.rand(800, 7, 7, channels, generator=g) + 0.5
    return rois, dy


def probe_rois(rois, pile, seed=29):
    """the RoIs whose loss the test must notice: hit positions 0, 12, 13, 511, 512 and the last of the piled tile (the pile
    comes first in image 0, so its hit positions are its RoI indices), and ten random ones"""
    lv = map_levels(rois)
    piled = ((rois[:, 0] == 0) & (lv == 3)).nonzero().squeeze(1).tolist()
    assert piled[:pile] == list(range(pile))
    want = [p for p in (0, 12, 13, 511, 512) if p < len(piled)] + [len(piled) - 1]
    g = torch.Generator().manual_seed(seed)
    return sorted({piled[p] for p in want} | set(torch.randperm(rois.shape[0], generator=g)[:10].tolist()))


# What fp32 costs on these inputs, per pyramid level: the fp32 C oracle's own  max |oracle - float64| / (2^-24 S)  measured on
# the CPU at the channel counts the GPU test uses (test_roi_ref64_cpu.py re-measures at C = 32 and asserts it stays below).
# C = 32: 7440 / 102 / 24 / 51 / 0 (fp32 pile), 4915 / 114 / 24 / 29 / 0 (fp16 pile), 4915 / 102 / 24 / 19 / 0 (bf16 pile);
# C = 260: 7441 / 101 / 24 / 61 / 0, 5023 / 113 / 24 / 28 / 0, 5023 / 101 / 24 / 22 / 0.  Not summation order: the RoI geometry
# (bin size, sample positions) is fp32 there and float64 here, ~1e-5 px on the fine level's coordinates, which a pixel at the
# rim of a footprint -- S tiny -- sees as a large ratio.  The kernel gets 4 x: other geometry expressions, another summation
# order (per chunk first, then the chunks in order).
K_ORACLE = [7500, 120, 25, 65, 0]
K_KERNEL = [4 * k for k in K_ORACLE]


def gather_bound(k, S, ref, half_ulp):
    """elementwise: k 2^-24 S (fp32 accumulation of terms whose magnitudes sum to S) + half_ulp |ref| 1.001 (the one rounding
    of a 16-bit gradient map, of the fp32 sum rather than of ref: the suite's 1.001; half_ulp = 0 for fp32 maps)"""
    return k * 2.0 ** -24 * S + half_ulp * 1.001 * ref.abs()
