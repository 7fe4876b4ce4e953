"""Bit-level record of the dense heads' row kernels (csrc/row_head.h and the four heads on it), to compare two builds of the
library on one device:

    python tools/row_head_bits.py dump OUT.npz [LIBRARY]     every output of the entries below, from seeded inputs
    python tools/row_head_bits.py compare A.npz B.npz        prints `n of n arrays bit-equal`, exit status 1 otherwise

For FCOS, ATSS, GFL and VFNet: *_decode_levels, *_loss_forward (workspace partials and norm), *_loss_finalize (losses, coef3)
and *_loss_backward (every output tensor).  Inputs are those of tests/{fcos,atss,gfl,vfnet}_inputs.py on
  fix4 / fix1 : the fixture pyramid (1024 rows), batch 2, 4 classes and 1 class
  ragged      : batch 1 on levels (41,53) .. (3,4): two point workgroups on level 0, the second with 125 live rows, and a
                partly empty last class workgroup
  noscore     : head_outputs(empty=True), no class score of image 1 reaches the threshold
  nogt        : no ground truth at all
in padded row tensors (random padding columns), FCOS over iou / giou x centerness_on_reg x norm_on_bbox, GFL with reg_max 16
and 1, VFNet with iou_weighted on and off."""
import itertools
import os
import sys

sys.path.insert(0, os.getcwd())
if len(sys.argv) > 3 and sys.argv[1] == 'dump':
    os.environ['BRCNN_LIB_PATH'] = os.path.abspath(sys.argv[3])       # read when brcnn.lib is imported
import numpy as np  # noqa: E402
import torch  # noqa: E402

RAGGED = [(41, 53), (21, 27), (11, 14), (6, 7), (3, 4)]
RAGGED_BOX = (20.3, 30.7, 400.6, 300.1)
# name -> (level sizes or None for the fixture's, batch, classes, head_outputs(empty=), ground truth)
CASES = {'fix4': (None, 2, 4, False, True), 'fix1': (None, 2, 1, False, True), 'ragged': (RAGGED, 1, 4, False, True),
         'noscore': (None, 2, 4, True, True), 'nogt': (None, 2, 4, False, False)}
DEV = 'cuda'


def _rows(levels):
    return torch.cat([t.detach().permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in levels]).float()


def _padded(g, blocks):
    """[pad | block | pad | block ... | pad] with seeded padding columns; returns the tensor and each block's first column"""
    n, cols, offs, c = blocks[0].shape[0], [], [], 0
    for i, b in enumerate(blocks):
        pad = torch.randn(n, 3 - i % 2, generator=g)
        cols += [pad, b]
        offs.append(c + pad.shape[1])
        c += pad.shape[1] + b.shape[1]
    cols.append(torch.randn(n, 2, generator=g))
    return torch.cat(cols, 1).contiguous().to(DEV), offs


class Case:
    """the inputs one head module gives for one case, on the device"""

    def __init__(self, mod, name, **kw):
        from brcnn import ops, train_ops
        from tests import atss_inputs
        sizes, self.B, self.C, empty, with_gt = CASES[name]
        self.sizes = sizes or mod.SIZES
        self.strides = mod.STRIDES
        self.g = torch.Generator().manual_seed(7)
        saved = mod.SIZES
        mod.SIZES = self.sizes                      # head_outputs draws one tensor per entry of the module's SIZES
        try:
            self.outs = mod.head_outputs(31, self.C, batch=self.B, empty=empty, **kw)
        finally:
            mod.SIZES = saved
        if with_gt:
            boxes, labels = mod.gts(5, batch=self.B, num_classes=self.C)
            if sizes:
                boxes = [torch.cat([b, b.new_tensor([RAGGED_BOX])]) for b in boxes]
                labels = [torch.cat([l, l.new_full((1,), self.C - 1)]) for l in labels]
        else:
            boxes, labels = [torch.zeros(0, 4)] * self.B, [torch.zeros(0, dtype=torch.long)] * self.B
        self.gts, self.labels, self.offs = train_ops.flatten_gts([b.to(DEV) for b in boxes], [l.to(DEV) for l in labels])
        self.gts, self.labels = self.gts.to(DEV), self.labels.to(DEV)
        self.scales = torch.tensor(mod.SCALES, device=DEV)
        half = [s * atss_inputs.OCTAVE / 2 for s in self.strides]
        self.base = ops.atss_base_anchors([torch.tensor([[-h, -h, h, h]]) for h in half])
        h, w = self.sizes[0][0] * self.strides[0], self.sizes[0][1] * self.strides[0]
        self.max_shape = torch.tensor([[h - 7., w - 20.], [h - 0., w - 3.]][:self.B], device=DEV)
        self.sf = torch.tensor([[1.1, 1.2, 1.1, 1.2], [0.8, 0.75, 0.8, 0.75]][:self.B], device=DEV)

    def picks(self, score):
        """per level (B, k) int64 cells, the 1000 highest-scoring of each image (every cell of a smaller level)"""
        out, r0 = [], 0
        for h, w in self.sizes:
            s = score[r0:r0 + self.B * h * w].view(self.B, h * w)
            out.append(s.topk(min(1000, h * w), dim=1).indices.contiguous())
            r0 += self.B * h * w
        return out

    def atss_inds(self):
        from brcnn import train_ops
        from tests import atss_inputs
        return train_ops.atss_assign(self.gts, self.offs, self.B, self.sizes, self.strides, self.base, atss_inputs.TOPK)


def _ar_loss(fn, c, a, r, layout, gt_inds, meta):
    """forward partials, finalize and backward of a head on (A, R, scales)"""
    from brcnn import train_ops
    ws, norm = train_ops._centerness_loss_partials(a, r, layout, c.scales, gt_inds, c.gts, c.labels, meta)
    a, r, sc = a.clone().requires_grad_(), r.clone().requires_grad_(), c.scales.clone().requires_grad_()
    losses, coef, norm_b = fn(a, r, sc, gt_inds, c.gts, c.labels, layout, meta)
    wgt = torch.linspace(0.5, 1.5, losses.numel(), device=DEV).view_as(losses)
    (losses * wgt).sum().backward()
    return dict(partials=ws, norm=norm, losses=losses, coef=coef, norm_b=norm_b, da=a.grad, dr=r.grad, dscale=sc.grad)


def _decoded(out):
    return dict(zip(('boxes', 'scores', 'labels', 'valid', 'n_valid'), out))


def fcos(name):
    from brcnn import ops, train_ops
    from tests import fcos_inputs as fi
    res = {}
    for giou, on_reg, norm in itertools.product((False, True), repeat=3):
        c = Case(fi, name, norm_on_bbox=norm)
        cls, raw, ctr = (_rows(t) for t in c.outs)
        a, ao = _padded(c.g, [cls] if on_reg else [cls, ctr])
        r, ro = _padded(c.g, [raw, ctr] if on_reg else [raw])
        layout = ops.FcosLayout(a, r, c.C, ao[0], ro[0], on_reg, ro[1] if on_reg else ao[1], norm, giou)
        inds = c.picks(ops.fcos_score(a, r, layout))
        out = _decoded(ops.fcos_decode_levels(inds, a, r, layout, c.scales, c.sizes, c.strides, c.max_shape, c.sf, 0.05))
        gt_inds = train_ops.fcos_assign(c.gts, c.offs, c.B, c.sizes, c.strides, fi.RANGES)
        meta = train_ops.FcosLossMeta(c.B, c.sizes, c.strides, c.C, c.offs, 2.0, 0.25, 1e-6, 1e-6, 1.0, 1.5, 0.5)
        out.update(_ar_loss(train_ops.fcos_loss, c, a, r, layout, gt_inds, meta))
        res.update({f'giou{int(giou)}_onreg{int(on_reg)}_norm{int(norm)}.{k}': v for k, v in out.items()})
    return res


def atss(name):
    from brcnn import ops, train_ops
    from tests import atss_inputs as ai
    c = Case(ai, name)
    cls, raw, ctr = (_rows(t) for t in c.outs)
    a, ao = _padded(c.g, [cls])
    r, ro = _padded(c.g, [raw, ctr])
    layout = ops.FcosLayout(a, r, c.C, ao[0], ro[0], True, ro[1], False, True)
    inds = c.picks(ops.fcos_score(a, r, layout))
    out = _decoded(ops.atss_decode_levels(inds, a, r, layout, c.scales, c.sizes, c.strides, c.base, c.max_shape, c.sf,
                                          ai.MEANS, ai.STDS, 0.05))
    meta = train_ops.AtssLossMeta(c.B, c.sizes, c.strides, c.base, c.C, c.offs, 2.0, 0.25, 1e-6, 1.0, 2.0, 0.5, ai.MEANS,
                                  ai.STDS)
    out.update(_ar_loss(train_ops.atss_loss, c, a, r, layout, c.atss_inds(), meta))
    return out


def gfl(name):
    from brcnn import ops, train_ops
    from tests import gfl_inputs as gi
    res = {}
    for reg_max in (16, 1):
        c = Case(gi, name, reg_max=reg_max)
        cls, raw = (_rows(t) for t in c.outs)
        a, ao = _padded(c.g, [cls])
        r, ro = _padded(c.g, [raw])
        layout = ops.GflLayout(a, r, c.C, reg_max, ao[0], ro[0])
        inds = c.picks(ops.gfl_score(a, layout))
        out = _decoded(ops.gfl_decode_levels(inds, a, r, layout, c.scales, c.sizes, c.strides, c.base, c.max_shape, c.sf, 0.05))
        meta = train_ops.GflLossMeta(c.B, c.sizes, c.strides, c.base, reg_max, c.C, c.offs, 2.0, 1e-6, 1.0, 2.0, 0.25)
        out.update(_ar_loss(train_ops.gfl_loss, c, a, r, layout, c.atss_inds(), meta))
        res.update({f'regmax{reg_max}.{k}': v for k, v in out.items()})
    return res


def vfnet(name):
    from brcnn import lib, ops, train_ops
    from tests import vfnet_inputs as vi
    res = {}
    for iou_weighted in (True, False):
        c = Case(vi, name)
        cls, raw0, raw1 = (_rows(t) for t in c.outs)
        a, ao = _padded(c.g, [cls])
        r0, o0 = _padded(c.g, [raw0])
        r1, o1 = _padded(c.g, [raw1])
        refine = torch.tensor(vi.SCALES_REFINE, device=DEV)
        d0, off = ops.vfnet_star_offsets(r0, c.scales, c.B, c.sizes, c.strides, vi.REG_DENOMS, vi.GRADIENT_MUL, o0[0])
        d1 = ops.vfnet_refine(r1, refine, c.B, c.sizes, d0, o1[0])
        layout = ops.VfnetLayout(a, r1, c.C, ao[0], o1[0])
        inds = c.picks(ops.vfnet_score(a, layout))
        out = _decoded(ops.vfnet_decode_levels(inds, a, r1, d0, layout, refine, c.sizes, c.strides, c.base, c.max_shape, c.sf,
                                               0.05))
        out.update(d0=d0, offsets=off, d1=d1)
        gt_inds = c.atss_inds()
        meta = train_ops.VfnetLossMeta(c.B, c.sizes, c.strides, c.base, c.C, c.offs, 0.75, 2.0, iou_weighted, 1e-6, 1.0, 1.5, 2.0)
        h = lib.load()
        ws, nb = meta.workspace(h, a.device)
        norm = torch.empty(3, device=DEV)
        st = h.brcnn_vfnet_loss_forward(*train_ops.VfnetLossFunction._args(a, ao[0], d0, d1, gt_inds, c.gts, c.labels, meta),
                                        train_ops._ptr(ws), nb, train_ops._ptr(norm), train_ops._stream())
        lib.check(st, 'brcnn_vfnet_loss_forward')
        ag, g0, g1 = a.clone().requires_grad_(), d0.clone().requires_grad_(), d1.clone().requires_grad_()
        losses, coef, norm_b = train_ops.vfnet_loss(ag, g0, g1, gt_inds, c.gts, c.labels, meta, ao[0])
        (losses * torch.tensor([0.5, 1.0, 1.5], device=DEV)).sum().backward()
        out.update(partials=ws, norm=norm, losses=losses, coef=coef, norm_b=norm_b, da=ag.grad, dd0=g0.grad, dd1=g1.grad)
        res.update({f'iouw{int(iou_weighted)}.{k}': v for k, v in out.items()})
    return res


def dump(path):
    import brcnn  # noqa: F401
    arrays = {}
    for head in (fcos, atss, gfl, vfnet):
        for name in CASES:
            for k, v in head(name).items():
                arrays[f'{head.__name__}.{name}.{k}'] = v.detach().cpu().numpy()
    torch.cuda.synchronize()
    np.savez(path, **arrays)
    print(f'{len(arrays)} arrays -> {path}')


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    keys = sorted(set(a.files) | set(b.files))
    bad = [k for k in keys if k not in a.files or k not in b.files or a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or
           a[k].tobytes() != b[k].tobytes()]
    for k in bad:
        print('differs:', k)
    print(f'{len(keys) - len(bad)} of {len(keys)} arrays bit-equal')
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) >= 3 and sys.argv[1] == 'dump':
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == 'compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
