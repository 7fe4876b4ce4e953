"""No device: the float64 RoIAlign helper of the chunked-gather test (tests/roi_ref64.py) against the oracle, the fp32
oracle's own distance from it on that test's inputs (what the kernel's bound is sized by), and the condition on those
inputs that makes the GPU test notice one lost hit."""
import pytest
import torch

import brcnn  # noqa: F401
from oracle import orc
from tests import roi_ref64 as RR
from tests import route_util as R
from tests import util


def test_float64_roi_align_helper_equals_the_oracle():
    """forward: orc.roi_align_f64 (the independent numpy brute force) to 1e-12; adjoint (autograd): the C oracle's fp32
    roi_align_backward to its usual rtol 1e-4 / atol 1e-5 -- RoIs that hang over the border, lie outside, are tiny, huge"""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 13, 21, generator=g).double()
    rois = torch.cat([util.rand_rois(40, 2, 672., 400., seed=8, min_size=4., max_size=900.),
                      torch.tensor([[0, -80., -60., 30., 20.], [1, 650., 380., 720., 460.], [1, -500., -500., -300., -300.],
                                    [0, 100., 100., 101., 101.], [1, 0., 0., 672., 400.], [0, 300., 10., 310., 390.]])])
    want = torch.from_numpy(orc.roi_align_f64(x, rois, 7, 1 / 32., 0, True))
    xr = x.clone().requires_grad_(True)
    got = RR.roi_align_f64(xr, rois, 7, 1 / 32.)
    assert (got.detach() - want).abs().max().item() <= 1e-12
    go = torch.rand(rois.shape[0], 3, 7, 7, generator=g) + 0.5
    got.backward(go.double())
    ref = orc.roi_align_backward(go, rois, x.shape, 7, 1 / 32., 0, True)
    assert torch.allclose(xr.grad.float(), ref, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16])
def test_chunked_gather_inputs_resolve_one_lost_hit(dtype):
    """on the reference alone (C = 32, as the GPU test): (1) the fp32 C oracle stays within K_ORACLE 2^-24 S of the float64 adjoint per level
    -- the measurement the kernel's bound (4 x) is sized by; (2) every probe RoI -- hit positions 0, 12, 13, 511, 512 and the
    last of the piled tile, ten random ones -- moves the reference, when it is removed, by more than 10 x the kernel's
    bound at some pixel of its level: a hit lost at a chunk, batch or direct-path boundary fails the GPU test.  Removing a
    RoI removes its own term (the adjoint is linear), so the move is that RoI's adjoint alone."""
    pile = RR.PILE[dtype]
    rois, dy = RR.gather_case(32, pile)
    lv = RR.map_levels(rois)
    ref = RR.roi_extract_adjoint_f64(dy, rois, 3)          # dY > 0 and every interpolation weight >= 0: S = the adjoint itself
    assert int(((rois[:, 0] == 0) & (lv == 3)).sum()) >= pile and (pile <= 512) == (dtype != torch.float32)
    for l, (h, w) in enumerate(RR.SIZES):
        idx = (lv == l).nonzero().squeeze(1)
        o = orc.roi_align_backward(dy[idx].permute(0, 3, 1, 2).contiguous(), rois[idx], (3, 32, h, w), 7, 1. / RR.STRIDES[l], 0,
                                   True).permute(0, 2, 3, 1).double()
        S = ref[l]
        assert bool((o[S == 0] == 0).all())
        ratio = ((o - S).abs()[S > 0] / (2.0 ** -24 * S[S > 0])).max().item() if bool((S > 0).any()) else 0.0
        print(f'{dtype} level {l}: fp32 oracle / float64 ratio {ratio:.1f} (K_ORACLE {RR.K_ORACLE[l]})')
        assert ratio <= RR.K_ORACLE[l], (l, ratio)
    bounds = [RR.gather_bound(RR.K_KERNEL[l], ref[l], ref[l], R.half_ulp(dtype)) for l in range(5)]
    for k in RR.probe_rois(rois, pile):
        one = RR.roi_extract_adjoint_f64(dy[k:k + 1], rois[k:k + 1], 3)
        l = int(lv[k])
        if not bool((one[l] > 0).any()):
            assert k >= 596 or rois[k, 0] == 2           # only a border case may lie outside its map
            continue
        moved = (one[l] / bounds[l].clamp_min(1e-300))[one[l] > 0].max().item()
        assert moved > 10.0, (k, l, moved)
