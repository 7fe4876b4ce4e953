"""RetinaRPN (`ATSSRPNHead`): shared 4-conv GN tower + objectness / box / IoU heads, anchor
target assignment + losses, and the proposal stage.

Mirrors `mmdet/models/dense_heads/atss_rpn_head.py:109-783` on top of
`anchor_head.py:37-268` and `rpn_head.py:16-34` (constructor arguments, parameter names
`rpn_convs.{i}.{conv,gn}`, `rpn_cls/rpn_reg/rpn_iou`, `scales.{i}.scale`, loss definitions,
proposal semantics).  Differences are in execution only:
  * the tower and heads run as NHWC implicit-GEMM convolutions (GroupNorm+ReLU fused kernel;
    the per-level `Scale` folded into the rpn_reg epilogue);
  * `get_bboxes` processes the whole batch at once on the device: fused
    sqrt(sigmoid*sigmoid) scoring, per-level top-k, on-the-fly anchor decode, one segmented
    NMS launch for all images, a single host sync at the end (the reference loops over
    images and levels in Python, atss_rpn_head.py:485,706).
"""
import copy

import torch
import torch.distributed as dist
import torch.nn as nn

from . import ops
from .blocks import (ConvModule, PackedCache, Scale, bias_init_with_prob, pack_weight, to_nhwc)
from .postprocess import batched_nms_images
from .core import (anchor_inside_flags, bbox_overlaps, const_rows, images_to_levels, multi_apply, unmap)
from .registry import (HEADS, build_anchor_generator, build_assigner, build_bbox_coder,
                       build_loss, build_sampler)

EPS = 1e-12


def cat_rows(feats):
    """the pyramid levels as one (rows, C) tensor, level-major: a view when the neck wrote them back to back"""
    from .autograd import cat_rows as _cr
    return _cr(list(feats))


def _nchw_rows(lst):
    """per-level (N,C,h,w) maps -> (rows, C) fp32, level-major rows, the row order of the kernels"""
    return torch.cat([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in lst], 0).float()


def reduce_mean(tensor):
    """mean over ranks (mmdet/core/utils/dist_utils.py:67-73); identity when not distributed"""
    if not (dist.is_available() and dist.is_initialized()):
        return tensor
    tensor = tensor.clone()
    dist.all_reduce(tensor.div_(dist.get_world_size()), op=dist.ReduceOp.SUM)
    return tensor


def valid_cells(anchor_generator, sizes, img_metas, like):
    """AnchorGenerator.valid_flags of a batch as the (B, L, 2) int32 table [valid_h, valid_w] in cells that the assignment
    kernels take, on `like`'s device; None when every cell of every image is valid"""
    import numpy as np
    if all(anchor_generator.all_valid(list(sizes), m['pad_shape']) for m in img_metas):
        return None
    rows = []
    for m in img_metas:
        h, w = m['pad_shape'][:2]
        r = []
        for (fh, fw), st in zip(sizes, anchor_generator.strides):
            r += [min(int(np.ceil(h / st[1])), fh), min(int(np.ceil(w / st[0])), fw)]
        rows.append(r)
    return const_rows(rows, like).to(torch.int32).view(len(img_metas), len(sizes), 2).contiguous()


class AnchorHead(nn.Module):
    """Target assignment shared by anchor-based heads (anchor_head.py:37-268), and what their device paths share: the
    cached anchor tables, the whole-batch MaxIoU assignment and the proposal stage of the two RPN heads."""

    def __init__(self, num_classes, in_channels, feat_channels=256,
                 anchor_generator=dict(type='AnchorGenerator', scales=[8, 16, 32],
                                       ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64]),
                 bbox_coder=dict(type='DeltaXYWHBBoxCoder', clip_border=True,
                                 target_means=(.0, .0, .0, .0), target_stds=(1.0, 1.0, 1.0, 1.0)),
                 reg_decoded_bbox=False,
                 loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                 loss_bbox=dict(type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0),
                 train_cfg=None, test_cfg=None, init_cfg=None):
        super().__init__()
        self.in_channels, self.num_classes, self.feat_channels = in_channels, num_classes, feat_channels
        self.use_sigmoid_cls = loss_cls.get('use_sigmoid', False)
        self.sampling = loss_cls['type'] not in ['FocalLoss', 'GHMC', 'QualityFocalLoss']
        self.cls_out_channels = num_classes if self.use_sigmoid_cls else num_classes + 1
        if self.cls_out_channels <= 0:
            raise ValueError(f'num_classes={num_classes} is too small')
        self.reg_decoded_bbox = reg_decoded_bbox
        self.bbox_coder = build_bbox_coder(bbox_coder)
        self.loss_cls = build_loss(loss_cls)
        self.loss_bbox = build_loss(loss_bbox)
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        if self.train_cfg:
            self.assigner = build_assigner(self.train_cfg.assigner)
            if self.sampling and hasattr(self.train_cfg, 'sampler'):
                sampler_cfg = self.train_cfg.sampler
            else:
                sampler_cfg = dict(type='PseudoSampler')
            self.sampler = build_sampler(sampler_cfg, context=self)
        self.anchor_generator = build_anchor_generator(anchor_generator)
        self.num_anchors = self.anchor_generator.num_base_anchors[0]
        self._init_layers()

    def get_anchors(self, featmap_sizes, img_metas, device='cuda'):
        num_imgs = len(img_metas)
        multi_level_anchors = self.anchor_generator.grid_anchors(featmap_sizes, device)
        anchor_list = [multi_level_anchors for _ in range(num_imgs)]
        valid_flag_list = [self.anchor_generator.valid_flags(featmap_sizes, m['pad_shape'], device)
                           for m in img_metas]
        # remembered for get_targets: images whose flags are all ones by construction
        self._all_valid = [self.anchor_generator.all_valid(featmap_sizes, m['pad_shape']) for m in img_metas]
        return anchor_list, valid_flag_list

    def _get_targets_single(self, flat_anchors, valid_flags, gt_bboxes, gt_bboxes_ignore,
                            gt_labels, img_meta, all_valid=False, label_channels=1, unmap_outputs=True):
        # every anchor valid and no border test: the masked gather / scatter of the reference are
        # identities -- skip them (and the host syncs of `.any()` and boolean indexing)
        identity = bool(all_valid) and self.train_cfg.allowed_border < 0
        if identity:
            anchors = flat_anchors
            unmap_outputs = False
        else:
            inside_flags = anchor_inside_flags(flat_anchors, valid_flags, img_meta['img_shape'][:2],
                                               self.train_cfg.allowed_border)
            if not inside_flags.any():
                return (None,) * 7
            anchors = flat_anchors[inside_flags, :]
        assign_result = self.assigner.assign(anchors, gt_bboxes, gt_bboxes_ignore,
                                             None if self.sampling else gt_labels)
        sampling_result = self.sampler.sample(assign_result, anchors, gt_bboxes)
        num_valid = anchors.shape[0]
        bbox_targets = torch.zeros_like(anchors)
        bbox_weights = torch.zeros_like(anchors)
        labels = anchors.new_full((num_valid,), self.num_classes, dtype=torch.long)
        label_weights = anchors.new_zeros(num_valid, dtype=torch.float)
        pos_inds, neg_inds = sampling_result.pos_inds, sampling_result.neg_inds
        if len(pos_inds) > 0:
            if not self.reg_decoded_bbox:
                pos_bbox_targets = self.bbox_coder.encode(sampling_result.pos_bboxes,
                                                          sampling_result.pos_gt_bboxes)
            else:
                pos_bbox_targets = sampling_result.pos_gt_bboxes
            bbox_targets[pos_inds, :] = pos_bbox_targets
            bbox_weights[pos_inds, :] = 1.0
            if gt_labels is None:
                labels[pos_inds] = 0
            else:
                labels[pos_inds] = gt_labels[sampling_result.pos_assigned_gt_inds]
            label_weights[pos_inds] = 1.0 if self.train_cfg.pos_weight <= 0 \
                else self.train_cfg.pos_weight
        if len(neg_inds) > 0:
            label_weights[neg_inds] = 1.0
        if unmap_outputs:
            n = flat_anchors.size(0)
            labels = unmap(labels, n, inside_flags, fill=self.num_classes)
            label_weights = unmap(label_weights, n, inside_flags)
            bbox_targets = unmap(bbox_targets, n, inside_flags)
            bbox_weights = unmap(bbox_weights, n, inside_flags)
        return (labels, label_weights, bbox_targets, bbox_weights, pos_inds, neg_inds,
                sampling_result)

    def loss_single(self, cls_score, bbox_pred, anchors, labels, label_weights, bbox_targets, bbox_weights,
                    num_total_samples):
        """anchor_head.py:373-421"""
        cls_score = cls_score.permute(0, 2, 3, 1).reshape(-1, self.cls_out_channels)
        loss_cls = self.loss_cls(cls_score, labels.reshape(-1), label_weights.reshape(-1), avg_factor=num_total_samples)
        bbox_pred = bbox_pred.permute(0, 2, 3, 1).reshape(-1, 4)
        if self.reg_decoded_bbox:
            bbox_pred = self.bbox_coder.decode(anchors.reshape(-1, 4), bbox_pred)
        loss_bbox = self.loss_bbox(bbox_pred, bbox_targets.reshape(-1, 4), bbox_weights.reshape(-1, 4),
                                   avg_factor=num_total_samples)
        return loss_cls, loss_bbox

    # ------------------------------------------------------------------ device path: anchor tables + assignment
    def _base_anchors(self, level, device):
        key = (level, str(device))
        if key not in self._base_anchor_cache:
            self._base_anchor_cache[key] = self.anchor_generator.base_anchors[level].to(device)
        return self._base_anchor_cache[key]

    def _anchor_table(self, sizes, device):
        """all levels' grid anchors of ONE image as a cached (n, 4) tensor + the level geometry"""
        key = (tuple(sizes), str(device))
        cache = self.__dict__.setdefault('_anchor_tables', {})
        if key not in cache:
            if len(cache) > 64:
                cache.clear()
            anchors = torch.cat(self.anchor_generator.grid_anchors(list(sizes), device), 0).contiguous()
            starts = [0]
            for (h, w) in sizes:
                starts.append(starts[-1] + h * w * self.num_anchors)
            cache[key] = (anchors, (starts, [w for _, w in sizes], self.num_anchors))
        return cache[key]

    def assign_targets_device(self, sizes, img_metas, gts, gt_offsets, device, want_counts=False):
        """AnchorHead._get_targets_single's assignment for the whole batch on the device: gt_inds
        (B, anchors per image) int32 (-1 ignore / outside, 0 negative, k matched to gt k-1)"""
        from . import train_ops
        anchors, geom = self._anchor_table(sizes, device)
        B = len(img_metas)
        valid_hw = valid_cells(self.anchor_generator, sizes, img_metas, anchors)
        border = self.train_cfg.allowed_border
        img_hw = const_rows([m['img_shape'][:2] for m in img_metas], anchors) if border >= 0 else None
        a = self.assigner
        return train_ops.assign_max_iou(anchors, gts, gt_offsets, a.pos_iou_thr, a.neg_iou_thr, a.min_pos_iou,
                                        a.match_low_quality, batch=B, geom=geom, valid_hw=valid_hw, img_hw=img_hw,
                                        allowed_border=border, want_counts=want_counts)

    # ------------------------------------------------------------------ one anchor per cell + ATSSAssigner (ATSSHead, GFLHead)
    MAX_TOPK = 16        # brcnn_atss_assign

    @classmethod
    def _check_atss_train_cfg(cls, name, tc, feat_channels):
        """what the heads on `brcnn_atss_assign` and the GN towers refuse before they build anything"""
        if tc:
            asg = tc.get('assigner', {})
            if asg.get('type') != 'ATSSAssigner':
                raise NotImplementedError(f"{name}: train_cfg.assigner.type={asg.get('type')!r}; only ATSSAssigner")
            if not 0 < asg.get('topk', 0) <= cls.MAX_TOPK:
                raise ValueError(f"{name}: train_cfg.assigner.topk={asg.get('topk')} outside (0, {cls.MAX_TOPK}]")
            if asg.get('ignore_iof_thr', -1) > 0:
                raise NotImplementedError(f"{name}: train_cfg.assigner.ignore_iof_thr={asg.get('ignore_iof_thr')} > 0 (ignore "
                                          'regions) is not supported')
            if tc.get('pos_weight', -1) > 0:
                raise NotImplementedError(f"{name}: train_cfg.pos_weight={tc.get('pos_weight')} > 0 is not supported")
            if tc.get('allowed_border', -1) >= 0:
                raise NotImplementedError(f"{name}: train_cfg.allowed_border={tc.get('allowed_border')} >= 0 is not supported "
                                          '(inside flags = valid flags)')
        if feat_channels > 256 or feat_channels % 4:
            raise NotImplementedError(f'{name}: feat_channels={feat_channels}; the GroupNorm kernels take up to 256 channels in '
                                      'whole quads')

    def _check_one_square_anchor(self, name):
        if self.num_anchors != 1:
            raise NotImplementedError(
                f'{name}: the anchor_generator gives {self.num_anchors} anchors per cell (several ratios, or scales_per_octave '
                '> 1); only one is supported -- the anchors of a cell share a centre, their distances to a ground truth '
                "tie exactly, and the reference's choice among them is torch.topk's unspecified order")
        if any(s[0] != s[1] for s in self.anchor_generator.strides):
            raise NotImplementedError(f'{name}: anchor_generator.strides={self.anchor_generator.strides}; only square strides')
        if len(self.anchor_generator.strides) > 8:
            raise ValueError(f'{name}: {len(self.anchor_generator.strides)} pyramid levels, at most 8 are supported')

    def _base_table(self):
        """the generator's base anchors as the host array the kernels take (the anchors themselves are never materialised)"""
        if '_base_host' not in self.__dict__:
            self.__dict__['_base_host'] = ops.atss_base_anchors(self.anchor_generator.base_anchors)
        return self.__dict__['_base_host']

    def _assign_atss_device(self, a, sizes, gt_bboxes, gt_labels, img_metas, gt_flat):
        """what the `loss_fused` of the heads on ATSS's assignment starts from: the packed ground truth on the device of `a`
        and brcnn_atss_assign over the valid cells -> (gts, labels, offs, sizes, base, gt_inds)"""
        from . import train_ops
        gts, labels, offs = gt_flat if gt_flat is not None else train_ops.flatten_gts(gt_bboxes, gt_labels)
        gts, labels = gts.to(a.device), labels.to(a.device)
        sizes = [tuple(int(v) for v in s) for s in sizes]
        base = self._base_table()
        gt_inds = train_ops.atss_assign(gts, offs, len(img_metas), sizes, self.strides, base, self.assigner.topk,
                                        valid_cells(self.anchor_generator, sizes, img_metas, a))
        return gts, labels, offs, sizes, base, gt_inds

    def _atss_targets(self, anchor_list, valid_flag_list, gt_bboxes_list, img_metas, gt_bboxes_ignore_list=None,
                      gt_labels_list=None, label_channels=1, unmap_outputs=True, encode=True):
        """`get_targets` of the heads trained on ATSSAssigner (atss_head.py:506-568, gfl_head.py:474-536) on torch ops, the
        host mirror: (anchors, labels, label weights, box targets, box weights) per level with the images stacked, and the
        two sample counts.  `encode`: the box targets are the coder's deltas (ATSSHead) or the ground-truth boxes (GFLHead)"""
        num_imgs = len(img_metas)
        assert len(anchor_list) == len(valid_flag_list) == num_imgs
        num_level_anchors = [a.size(0) for a in anchor_list[0]]
        flat_anchors = [torch.cat(list(a)) for a in anchor_list]
        flat_flags = [torch.cat(list(v)) for v in valid_flag_list]
        ignore = gt_bboxes_ignore_list if gt_bboxes_ignore_list is not None else [None] * num_imgs
        gt_labels_list = gt_labels_list if gt_labels_list is not None else [None] * num_imgs
        res = multi_apply(self._get_target_single, flat_anchors, flat_flags, [num_level_anchors] * num_imgs, gt_bboxes_list,
                          ignore, gt_labels_list, img_metas, label_channels=label_channels, unmap_outputs=unmap_outputs, encode=encode)
        all_anchors, all_labels, all_lw, all_bt, all_bw, pos_list, neg_list = res
        if any(l is None for l in all_labels):
            return None
        num_total_pos = sum(max(p.numel(), 1) for p in pos_list)
        num_total_neg = sum(max(p.numel(), 1) for p in neg_list)
        return tuple(images_to_levels(t, num_level_anchors) for t in (all_anchors, all_labels, all_lw, all_bt, all_bw)) + \
            (num_total_pos, num_total_neg)

    def _get_target_single(self, flat_anchors, valid_flags, num_level_anchors, gt_bboxes, gt_bboxes_ignore, gt_labels,
                           img_meta, label_channels=1, unmap_outputs=True, encode=True):
        """atss_head.py:570-678 / gfl_head.py:538-642"""
        inside_flags = anchor_inside_flags(flat_anchors, valid_flags, img_meta['img_shape'][:2], self.train_cfg.allowed_border)
        if not inside_flags.any():
            return (None,) * 7
        anchors = flat_anchors[inside_flags, :]
        inside_per_level = [int(f.sum()) for f in torch.split(inside_flags, num_level_anchors)]
        assign_result = self.assigner.assign(anchors, inside_per_level, gt_bboxes, gt_bboxes_ignore, gt_labels)
        sampling_result = self.sampler.sample(assign_result, anchors, gt_bboxes)
        n = anchors.shape[0]
        bbox_targets, bbox_weights = torch.zeros_like(anchors), torch.zeros_like(anchors)
        labels = anchors.new_full((n,), self.num_classes, dtype=torch.long)
        label_weights = anchors.new_zeros(n, dtype=torch.float)
        pos_inds, neg_inds = sampling_result.pos_inds, sampling_result.neg_inds
        if len(pos_inds) > 0:
            bbox_targets[pos_inds, :] = self.bbox_coder.encode(sampling_result.pos_bboxes, sampling_result.pos_gt_bboxes) \
                if encode else sampling_result.pos_gt_bboxes
            bbox_weights[pos_inds, :] = 1.0
            labels[pos_inds] = 0 if gt_labels is None else gt_labels[sampling_result.pos_assigned_gt_inds]
            label_weights[pos_inds] = 1.0 if self.train_cfg.pos_weight <= 0 else self.train_cfg.pos_weight
        if len(neg_inds) > 0:
            label_weights[neg_inds] = 1.0
        if unmap_outputs:
            total = flat_anchors.size(0)
            anchors = unmap(anchors, total, inside_flags)
            labels = unmap(labels, total, inside_flags, fill=self.num_classes)
            label_weights = unmap(label_weights, total, inside_flags)
            bbox_targets = unmap(bbox_targets, total, inside_flags)
            bbox_weights = unmap(bbox_weights, total, inside_flags)
        return anchors, labels, label_weights, bbox_targets, bbox_weights, pos_inds, neg_inds

    # ------------------------------------------------------------------ device path: the RPN proposal stage
    def _proposals_padded(self, cls_nhwc, reg_nhwc, iou_nhwc, img_metas, cfg=None, reg_scales=None):
        """Device-resident proposal stage for the whole batch (no host sync).

        Inputs are the NHWC head outputs per level: (B,h,w,A), (B,h,w,4A), (B,h,w,A) (dense or
        channel-slice views of the fused head output; then `reg_scales` carries the per-level
        Scale still to be applied to the raw deltas).
        Returns (dets (B, max_per_img, 5) zero-padded, num (B,) int32)."""
        cfg = copy.deepcopy(self.test_cfg if cfg is None else cfg)
        assert self.use_sigmoid_cls and self.cls_out_channels == 1
        nms_cfg = dict(cfg.nms)
        assert nms_cfg.pop('type', 'nms') == 'nms', 'RPN proposals use greedy NMS'
        B = cls_nhwc[0].shape[0]
        device = cls_nhwc[0].device
        shapes = {tuple(m['img_shape'][:2]) for m in img_metas}
        A = self.num_anchors
        sc_l, pr_l, va_l, id_l = [], [], [], []
        raw = [self._proposal_scores(cls_nhwc[lvl], None if iou_nhwc is None else iou_nhwc[lvl]).view(B, -1)
               for lvl in range(len(cls_nhwc))]
        if 0 < cfg.nms_pre <= 4096:
            # descending, ties by ascending index (the shared tie rule), all levels in one launch
            picked = ops.rpn_topk(raw, cfg.nms_pre)
        else:
            picked = []
            for score in raw:
                n = score.shape[1]
                if cfg.nms_pre > 0 and n > cfg.nms_pre:
                    ranked, rank_inds = score.sort(dim=1, descending=True, stable=True)
                    picked.append((ranked[:, :cfg.nms_pre], rank_inds[:, :cfg.nms_pre].contiguous()))
                else:
                    picked.append((score, torch.arange(n, device=device).expand(B, n).contiguous()))
        dev_scales = isinstance(reg_scales, torch.Tensor)
        if (len(shapes) == 1 or dev_scales) and cfg.min_bbox_size >= 0 and device.type == 'cuda':
            # every level decoded by one launch that also writes the validity and level-id columns of
            # the (B, T) candidate slots; device-resident scales (training) also take the per-image
            # clip border from a device table, so a batch of differently sized images stays one launch
            L = len(cls_nhwc)
            from .core import const_rows
            per_image = const_rows([m['img_shape'][:2] for m in img_metas], raw[0]) if dev_scales and len(shapes) > 1 \
                else None
            props, valid, ids = ops.rpn_decode_levels(
                [picked[l][1] for l in range(L)], [reg_nhwc[l] for l in range(L)],
                [self._base_anchors(l, device) for l in range(L)], [tuple(cls_nhwc[l].shape[1:3]) for l in range(L)],
                list(self.anchor_generator.strides), self.bbox_coder.means, self.bbox_coder.stds, next(iter(shapes)),
                cfg.min_bbox_size, pred_scales=None if reg_scales is None else (reg_scales if dev_scales else list(reg_scales)),
                max_shapes=per_image)
            sc_l = [picked[l][0] for l in range(L)]
            scores = torch.cat(sc_l, 1)
            return self._proposals_from_candidates(props, scores, ids, valid, sc_l, nms_cfg, cfg)
        for lvl in range(len(cls_nhwc)):
            h, w = cls_nhwc[lvl].shape[1:3]
            score, topk_inds = picked[lvl]
            stride = self.anchor_generator.strides[lvl]
            rs = 1.0 if reg_scales is None else reg_scales[lvl]
            if len(shapes) == 1:
                max_shape = next(iter(shapes))
                props, valid = ops.rpn_decode(topk_inds, reg_nhwc[lvl], self._base_anchors(lvl, device),
                                              (h, w), stride, self.bbox_coder.means,
                                              self.bbox_coder.stds, max_shape, cfg.min_bbox_size,
                                              pred_scale=rs)
            else:   # per-image clip border
                pl, vl = [], []
                for b in range(B):
                    p1, v1 = ops.rpn_decode(topk_inds[b:b + 1], reg_nhwc[lvl][b:b + 1],
                                            self._base_anchors(lvl, device), (h, w), stride,
                                            self.bbox_coder.means, self.bbox_coder.stds,
                                            img_metas[b]['img_shape'][:2], cfg.min_bbox_size,
                                            pred_scale=rs)
                    pl.append(p1)
                    vl.append(v1)
                props, valid = torch.cat(pl), torch.cat(vl)
            if cfg.min_bbox_size < 0:
                valid = torch.ones_like(valid)
            sc_l.append(score)
            pr_l.append(props)
            va_l.append(valid.bool())
            id_l.append(torch.full((B, score.shape[1]), lvl, dtype=torch.long, device=device))
        scores = torch.cat(sc_l, 1)            # (B, T)
        props = torch.cat(pr_l, 1)             # (B, T, 4)
        valid = torch.cat(va_l, 1)             # (B, T)  `proposals[valid_mask]` (:750-754)
        ids = torch.cat(id_l, 1)
        return self._proposals_from_candidates(props, scores, ids, valid, sc_l, nms_cfg, cfg)

    @staticmethod
    def _proposals_from_candidates(props, scores, ids, valid, sc_l, nms_cfg, cfg):
        if scores.shape[1] >= nms_cfg.get('split_thr', 10000):
            # mmcv batched_nms switches to its per-id (per-level) loop at >= split_thr candidates
            # (the training proposal cfg: 15 150 per image).  Both of its branches keep the same
            # boxes in the same order (the coordinate offsets already isolate the levels), so the
            # whole batch runs as one segmented launch over (image, level) segments.
            from .postprocess import batched_nms_images_by_level
            return batched_nms_images_by_level(props, scores, ids, valid, [s_.shape[1] for s_ in sc_l],
                                               nms_cfg['iou_threshold'], cfg.max_per_img,
                                               nms_cfg.get('offset', 0))
        dets, _, num = batched_nms_images(props, scores, ids, valid, nms_cfg['iou_threshold'],
                                          cfg.max_per_img, nms_cfg.get('offset', 0))
        return dets, num


@HEADS.register_module()
class ATSSRPNHead(AnchorHead):
    def __init__(self, in_channels, num_classes=1, stacked_convs=4, conv_cfg=None, gamma=1,
                 atss=False, bridge=False, last_conv='norm', aug_reg_loss=None,
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True),
                 loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=0.5),
                 init_cfg=None, num_convs=1, **kwargs):
        assert not atss, 'atss=True (ATSSAssigner targets) is outside the shipped boosting configs'
        assert not bridge and last_conv == 'norm', 'bridge / dcn / aspp variants are out of scope'
        self.stacked_convs, self.conv_cfg, self.norm_cfg = stacked_convs, conv_cfg, norm_cfg
        self.last_conv = last_conv
        super().__init__(num_classes, in_channels, init_cfg=init_cfg, **kwargs)
        self.loss_centerness = build_loss(loss_centerness)
        self.gamma, self.atss, self.bridge = gamma, atss, bridge
        self.with_aug_loss = aug_reg_loss is not None
        if self.with_aug_loss:
            self.aug_loss = build_loss(aug_reg_loss)
        self._head_caches = [PackedCache() for _ in range(8)]
        self._tower_caches = [PackedCache() for _ in range(stacked_convs)]
        self._fused_head_cache = PackedCache()
        # Winograd-transformed tower filters (prepare_winograd: inference with frozen weights, fp32), keyed on the weight
        # like the caches above
        self._wino_caches = [PackedCache() for _ in range(stacked_convs)]
        self._wino_prepared = False
        self._base_anchor_cache = {}
        self.init_weights()

    def _init_layers(self):
        self.rpn_convs = nn.ModuleList()
        for i in range(self.stacked_convs):
            chn = self.in_channels if i == 0 else self.feat_channels
            self.rpn_convs.append(ConvModule(chn, self.feat_channels, 3, stride=1, padding=1,
                                             conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg))
        self.rpn_cls = nn.Conv2d(self.feat_channels, self.num_anchors * self.cls_out_channels, 3,
                                 padding=1)
        self.rpn_reg = nn.Conv2d(self.feat_channels, self.num_anchors * 4, 3, padding=1)
        self.rpn_iou = nn.Conv2d(self.feat_channels, self.num_anchors * 1, 3, padding=1)
        self.scales = nn.ModuleList([Scale(1.0) for _ in self.anchor_generator.strides])

    def init_weights(self):
        """Normal(0, 0.01) convs, rpn_cls bias for prior 0.01 (atss_rpn_head.py:123-131)"""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, 0, 0.01)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.constant_(self.rpn_cls.bias, bias_init_with_prob(0.01))

    # ------------------------------------------------------------------ forward
    def forward_single_nhwc(self, x, level):
        for conv in self.rpn_convs:
            x = conv.forward_nhwc(x)
        scale = self.scales[level].scale
        from .autograd import conv2d_nhwc_autograd, wants_grad
        if wants_grad(x, self.rpn_cls.weight, scale):
            # training: the three heads as one differentiable 54-channel conv
            heads = (self.rpn_cls, self.rpn_reg, self.rpn_iou)
            y = conv2d_nhwc_autograd(x, torch.cat([h.weight for h in heads], 0),
                                     torch.cat([h.bias for h in heads], 0), 1, self.rpn_cls.padding[0], out_f32=True).float()
            a, c = self.num_anchors, self.cls_out_channels
            return (y[..., :a * c], y[..., a * c:a * c + 4 * a] * scale, y[..., a * c + 4 * a:])
        cls = self._head_conv(x, self.rpn_cls, self._head_caches[0], None)
        reg = self._head_conv(x, self.rpn_reg, self._head_caches[1 + level], scale)
        iou = self._head_conv(x, self.rpn_iou, self._head_caches[7], None)
        return cls, reg, iou

    @staticmethod
    def _head_conv(x, conv, cache, scale):
        srcs = [conv.weight, conv.bias] + ([scale] if scale is not None else [])

        def builder():
            from .blocks import pack_weight
            w = pack_weight(conv.weight).to(x.dtype)       # bf16 mode: bf16 operands, fp32 result
            b = conv.bias.detach().float()
            if scale is None:
                return w, None, b.contiguous()
            s = scale.detach().float().expand(conv.out_channels).contiguous()
            return w, s, (b * s).contiguous()   # scale*(conv+b) = conv*s + b*s

        from .autograd import conv2d_nhwc_autograd, wants_grad
        if wants_grad(x, conv.weight, conv.bias, scale):
            y = conv2d_nhwc_autograd(x, conv.weight, conv.bias, 1, conv.padding[0], out_f32=True).float()
            return y * scale if scale is not None else y
        w, s, b = cache.get(srcs, builder)
        # fp32 result in either mode: the proposal stage scores / decodes in fp32
        return ops.conv2d_nhwc(x, w, s, b, None, False, 1, conv.padding[0], out_f32=True)

    def forward_nhwc(self, feats):
        """feats: list of (N,h,w,C) -> 3 lists of (N,h,w,A | 4A | A) NHWC head outputs"""
        from .autograd import wants_grad
        if feats[0].is_cuda and wants_grad(feats[0], self.rpn_cls.weight) and \
                all(isinstance(c.norm, nn.GroupNorm) and c.conv.bias is None and c.conv.groups == 1
                    for c in self.rpn_convs) and self.feat_channels <= 256 and self.feat_channels % 4 == 0:
            return self._forward_train_fused(feats)
        outs = [self.forward_single_nhwc(f, i) for i, f in enumerate(feats)]
        return tuple(map(list, zip(*outs)))

    def _forward_train_fused(self, feats):
        """Training forward with all pyramid levels in one launch per layer: the tower and the
        heads share their weights across levels (atss_rpn_head.py:296-297), so conv forward, data
        gradient and weight gradient of a layer each run once over the concatenated rows, and
        GroupNorm keeps its per-(level, image, group) statistics through the segment table."""
        from .autograd import GroupNormNHWCFunction, conv2d_nhwc_multi_autograd
        B = feats[0].shape[0]
        sizes = tuple(tuple(f.shape[1:3]) for f in feats)
        x = cat_rows(feats)        # (a view when the neck wrote the levels back to back: ops.output_into)
        for conv in self.rpn_convs:
            x = conv2d_nhwc_multi_autograd(x, conv.conv.weight, None, B, sizes, 1, conv.conv.padding[0])
            x = GroupNormNHWCFunction.apply(x, conv.norm.weight, conv.norm.bias, conv.norm.num_groups, B, sizes,
                                            conv.norm.eps, conv.with_activation)
        heads = (self.rpn_cls, self.rpn_reg, self.rpn_iou)
        y = conv2d_nhwc_multi_autograd(x, torch.cat([h.weight for h in heads], 0),
                                       torch.cat([h.bias for h in heads], 0), B, sizes, 1,
                                       self.rpn_cls.padding[0], out_f32=True).float()
        a, c = self.num_anchors, self.cls_out_channels
        cls, reg, iou, r0 = [], [], [], 0
        for lvl, (h, w) in enumerate(sizes):
            n = B * h * w
            t = y[r0:r0 + n].view(B, h, w, y.shape[1])
            cls.append(t[..., :a * c])
            reg.append(t[..., a * c:a * c + 4 * a] * self.scales[lvl].scale)
            iou.append(t[..., a * c + 4 * a:])
            r0 += n
        return cls, reg, iou

    def forward_fused(self, feats):
        """All pyramid levels in ONE launch per layer (the tower and the heads share their
        weights across levels, atss_rpn_head.py:296-297), and the three 3x3 heads as ONE
        54-channel conv (cls 9 | reg 36 | iou 9).  Returns per level a (N,h,w,54) tensor whose
        channel slices are the raw head outputs; the per-level `Scale` of rpn_reg is applied by
        the consumer (`scale(self.rpn_reg(x))` == raw * scale)."""
        B = feats[0].shape[0]
        sizes = [tuple(f.shape[1:3]) for f in feats]
        x = cat_rows(feats)        # (a view when the neck wrote the levels back to back: ops.output_into)
        if self._wino_prepared and x.dtype == torch.float32 and self._winograd_ok() and ops.winograd_enabled():
            x = self._tower_winograd(x, B, sizes)
            return self._fused_heads(x, B, sizes)
        for i, conv in enumerate(self.rpn_convs):
            assert isinstance(conv.norm, nn.GroupNorm) and conv.conv.bias is None
            w = self._tower_caches[i].get([conv.conv.weight],
                                          lambda c=conv: pack_weight(c.conv.weight).to(x.dtype))
            x, _ = ops.conv2d_nhwc_multi(x, w, B, sizes, None, None, None, False, 1, 1)
            x = ops.groupnorm_nhwc_multi(x, conv.norm.weight.detach(), conv.norm.bias.detach(),
                                         conv.norm.num_groups, B, sizes, conv.norm.eps,
                                         conv.with_activation)
        return self._fused_heads(x, B, sizes)

    def prepare_winograd(self):
        """Inference with frozen weights: the tower's four 3x3 convs may run in the Winograd F(2x2,3x3) form (fp32 compute
        only, and only while the library's switch is on: ops.winograd_enabled).  The transformed filters are built here
        when the weights already live on the device, else on the first pass; a later load_state_dict rebuilds them."""
        self._wino_prepared = True
        if self._winograd_ok() and self.rpn_convs[0].conv.weight.is_cuda and ops.winograd_enabled():
            for i, conv in enumerate(self.rpn_convs):
                self._wino_filter(i, conv)
        return self

    def _winograd_ok(self):
        return all(isinstance(c.norm, nn.GroupNorm) and c.conv.bias is None and c.conv.groups == 1 and
                   c.conv.kernel_size == (3, 3) and c.conv.stride == (1, 1) and c.conv.padding == (1, 1) and
                   c.conv.dilation == (1, 1) and c.conv.in_channels % 32 == 0 and c.conv.out_channels % 64 == 0 and
                   c.conv.out_channels <= 256 for c in self.rpn_convs)

    def _wino_filter(self, i, conv):
        return self._wino_caches[i].get([conv.conv.weight], lambda: ops.winograd_filter(pack_weight(conv.conv.weight)))

    def _tower_winograd(self, x, B, sizes):
        """the tower with each layer's GroupNorm + ReLU applied by the NEXT conv's input transform: per layer the Winograd
        conv and the GroupNorm statistics of its raw output; the last layer's GroupNorm runs as the usual pass (the
        54-channel head conv stays direct)"""
        ws = ops.winograd_workspace(B, sizes, max(c.conv.in_channels for c in self.rpn_convs), x.device)    # one for the four layers
        gn, last = None, len(self.rpn_convs) - 1
        for i, conv in enumerate(self.rpn_convs):
            x = ops.conv3x3_winograd_multi(x, self._wino_filter(i, conv), B, sizes, gn=gn, workspace=ws)
            norm = conv.norm
            if i == last:
                return ops.groupnorm_nhwc_multi(x, norm.weight.detach(), norm.bias.detach(), norm.num_groups, B, sizes,
                                                norm.eps, conv.with_activation)
            gn = (ops.groupnorm_stats_multi(x, norm.num_groups, B, sizes, norm.eps), norm.weight.detach(),
                  norm.bias.detach(), norm.num_groups, conv.with_activation)

    def _fused_heads(self, x, B, sizes):
        heads = (self.rpn_cls, self.rpn_reg, self.rpn_iou)

        def builder():
            return (torch.cat([pack_weight(h.weight) for h in heads], 0).to(x.dtype).contiguous(),
                    torch.cat([h.bias.detach().float() for h in heads], 0).contiguous())
        w, b = self._fused_head_cache.get([t for h in heads for t in (h.weight, h.bias)], builder)
        # fp32 result in either mode: the proposal stage scores / decodes in fp32
        y, _ = ops.conv2d_nhwc_multi(x, w, B, sizes, None, b, None, False, 1, 1, out_f32=True)
        outs, r0 = [], 0
        for (h, wd) in sizes:
            n = B * h * wd
            outs.append(y[r0:r0 + n].view(B, h, wd, y.shape[1]))
            r0 += n
        return outs

    def split_fused(self, fused):
        """(cls, reg_raw, iou) channel-slice views of the fused head outputs + per-level scales"""
        a, c = self.num_anchors, self.cls_out_channels
        cls = [f[..., :a * c] for f in fused]
        reg = [f[..., a * c:a * c + 4 * a] for f in fused]
        iou = [f[..., a * c + 4 * a:] for f in fused]
        return cls, reg, iou

    def forward(self, feats, bridge=False):
        """reference signature: list of (N,C,h,w) -> lists of (N,A,h,w), (N,4A,h,w), (N,A,h,w)"""
        cls, reg, iou = self.forward_nhwc([to_nhwc(f) for f in feats])
        v = lambda lst: [t.permute(0, 3, 1, 2) for t in lst]  # noqa: E731
        return v(cls), v(reg), v(iou)

    # ------------------------------------------------------------------ train
    def forward_train(self, x, img_metas, gt_bboxes, gt_labels=None, gt_bboxes_ignore=None,
                      proposal_cfg=None, **kwargs):
        outs = self(x)
        if gt_labels is None:
            loss_inputs = outs + (gt_bboxes, img_metas)
        else:
            loss_inputs = outs + (gt_bboxes, gt_labels, img_metas)
        losses = self.loss(*loss_inputs, gt_bboxes_ignore=gt_bboxes_ignore)
        if proposal_cfg is None:
            return losses
        return losses, self.get_bboxes(*outs, img_metas, cfg=proposal_cfg)

    def get_targets(self, anchor_list, valid_flag_list, gt_bboxes_list, img_metas,
                    gt_bboxes_ignore_list=None, gt_labels_list=None, label_channels=1,
                    unmap_outputs=True):
        num_imgs = len(img_metas)
        assert len(anchor_list) == len(valid_flag_list) == num_imgs
        concat_anchor_list = [torch.cat(a) for a in anchor_list]
        concat_valid_flag_list = [torch.cat(v) for v in valid_flag_list]
        if gt_bboxes_ignore_list is None:
            gt_bboxes_ignore_list = [None] * num_imgs
        if gt_labels_list is None:
            gt_labels_list = [None] * num_imgs
        all_valid = getattr(self, '_all_valid', None)
        if all_valid is None or len(all_valid) != num_imgs:
            all_valid = [False] * num_imgs
        (labels, label_weights, bbox_targets, bbox_weights, _, _, sampling_result) = multi_apply(
            self._get_targets_single, concat_anchor_list, concat_valid_flag_list, gt_bboxes_list,
            gt_bboxes_ignore_list, gt_labels_list, img_metas, all_valid, label_channels=1, unmap_outputs=True)
        self._all_valid = None
        if any(l is None for l in labels):
            return None
        pos_inds = [((0 <= l) & (l < self.num_classes)).nonzero().view(-1) for l in labels]
        gt_inds = [s.pos_assigned_gt_inds for s in sampling_result]
        return (labels, label_weights, bbox_targets, bbox_weights, pos_inds, gt_inds,
                concat_anchor_list, concat_valid_flag_list)

    def loss_single(self, anchors, cls_score, bbox_pred, iou_pred, labels, label_weights,
                    bbox_targets, level_pos_inds=None, num_total_samples=1.0):
        anchors = anchors.reshape(-1, 4)
        cls_score = cls_score.permute(0, 2, 3, 1).reshape(-1, self.cls_out_channels).contiguous()
        bbox_pred = bbox_pred.permute(0, 2, 3, 1).reshape(-1, 4)
        iou_pred = iou_pred.permute(0, 2, 3, 1).reshape(-1)
        bbox_targets = bbox_targets.reshape(-1, 4)
        labels = labels.reshape(-1)
        label_weights = label_weights.reshape(-1)
        pos_inds = level_pos_inds if level_pos_inds is not None else \
            ((labels >= 0) & (labels < self.num_classes)).nonzero().squeeze(1)
        if len(pos_inds) > 0:
            pos_bbox_targets = bbox_targets[pos_inds]
            pos_bbox_pred = bbox_pred[pos_inds]
            pos_anchors = anchors[pos_inds]
            pos_ious = iou_pred[pos_inds]
            if self.reg_decoded_bbox:
                pos_decode_bbox_pred = self.bbox_coder.decode(pos_anchors, pos_bbox_pred)
                pos_encode_bbox_targets = self.bbox_coder.encode(pos_anchors, pos_bbox_targets)
                iou_target = bbox_overlaps(pos_decode_bbox_pred.detach(), pos_bbox_targets,
                                           is_aligned=True)
                if self.with_aug_loss:
                    w_aug = torch.ones_like(pos_bbox_pred) * (iou_target ** self.gamma)[:, None]
                    loss_bbox_aug = self.aug_loss(pos_bbox_pred, pos_encode_bbox_targets,
                                                  w_aug.clamp(min=EPS), avg_factor=1.0)
                bbox_weights = iou_target ** self.gamma
                loss_bbox = self.loss_bbox(pos_decode_bbox_pred, pos_bbox_targets,
                                           weight=bbox_weights.clamp(min=EPS), avg_factor=1.0)
                if self.with_aug_loss:
                    loss_bbox = (loss_bbox + loss_bbox_aug) * 0.5
            else:
                pos_decode_bbox_pred = self.bbox_coder.decode(pos_anchors, pos_bbox_pred)
                pos_decode_bbox_targets = self.bbox_coder.decode(pos_anchors, pos_bbox_targets)
                iou_target = bbox_overlaps(pos_decode_bbox_pred.detach(), pos_decode_bbox_targets,
                                           is_aligned=True)
                bbox_weights = torch.ones_like(pos_bbox_pred) * (iou_target ** self.gamma)[:, None]
                loss_bbox = self.loss_bbox(pos_bbox_pred, pos_bbox_targets,
                                           bbox_weights.clamp(min=EPS), avg_factor=1.0)
            avg_factor = iou_target.sum()
            loss_iou = self.loss_centerness(pos_ious, iou_target, avg_factor=num_total_samples)
        else:
            loss_bbox = bbox_pred.sum() * 0
            loss_iou = iou_pred.sum() * 0
            iou_target = bbox_targets.new_tensor(0.)
            avg_factor = iou_target.sum()
        from .losses import VarifocalLoss
        if isinstance(self.loss_cls, VarifocalLoss):      # atss_rpn_head.py:393-397
            cls_iou_targets = torch.zeros_like(cls_score)
            if len(pos_inds) > 0:
                cls_iou_targets[pos_inds] = iou_target.unsqueeze(-1)
            loss_cls = self.loss_cls(cls_score, cls_iou_targets, avg_factor=num_total_samples)
        else:
            loss_cls = self.loss_cls(cls_score, labels, label_weights, avg_factor=num_total_samples)
        return loss_cls, loss_bbox, loss_iou, avg_factor

    def loss(self, cls_scores, bbox_preds, iou_preds, gt_bboxes, img_metas, gt_bboxes_ignore=None):
        featmap_sizes = [f.size()[-2:] for f in cls_scores]
        assert len(featmap_sizes) == self.anchor_generator.num_levels
        device = cls_scores[0].device
        if device.type == 'cuda' and gt_bboxes_ignore is None and self.device_train_ok():
            # the reference signature on device tensors: repack the per-level NCHW outputs as the fused
            # (rows, 6A) layout (their Scale is already applied: unit scales) and run the HIP kernels
            sizes = tuple(tuple(int(v) for v in s_) for s_ in featmap_sizes)
            rows = [torch.cat([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in (c_, r_, i_)], 1)
                    for c_, r_, i_ in zip(cls_scores, bbox_preds, iou_preds)]
            y = torch.cat(rows, 0).float().contiguous()
            return self.loss_fused(y, sizes, gt_bboxes, img_metas,
                                   scales=torch.ones(len(sizes), dtype=torch.float32, device=device))
        label_channels = self.cls_out_channels if self.use_sigmoid_cls else 1
        num_level_anchors = [int(h) * int(w) * self.num_anchors for h, w in featmap_sizes]

        def build_targets():
            # anchors and flags depend on shapes only; they are created on the stream the targets are
            # built on (a cache miss on another stream would race with the reads below)
            anchor_list, valid_flag_list = self.get_anchors(featmap_sizes, img_metas, device=device)
            targets = self.get_targets(anchor_list, valid_flag_list, gt_bboxes, img_metas,
                                       gt_bboxes_ignore_list=gt_bboxes_ignore, gt_labels_list=None,
                                       label_channels=label_channels)
            if targets is None:
                return None
            (labels_l, label_weights_l, bbox_targets_l, _, pos_inds, _, anchors_l, _) = targets
            lv_labels = images_to_levels(labels_l, num_level_anchors)
            # positives per level, in the flattened (image, anchor) order loss_single uses
            lv_pos = [((l.reshape(-1) >= 0) & (l.reshape(-1) < self.num_classes)).nonzero().squeeze(1)
                      for l in lv_labels]
            return (lv_labels,
                    images_to_levels(label_weights_l, num_level_anchors),
                    images_to_levels(anchors_l, num_level_anchors),
                    images_to_levels(bbox_targets_l, num_level_anchors),
                    lv_pos, sum(p.numel() for p in pos_inds))

        ev = getattr(self, '_inputs_ready', None)
        self._inputs_ready = None
        if ev is not None and device.type == 'cuda':
            # target assignment on the side stream opened before the backbone was queued
            # (detectors.forward_train): its host syncs do not wait for the main stream
            main = torch.cuda.current_stream()
            if getattr(self, '_side_stream', None) is None:
                self._side_stream = torch.cuda.Stream()
            side = self._side_stream
            side.wait_event(ev)
            with torch.cuda.stream(side):
                built = build_targets()
            main.wait_stream(side)
            if built is not None:
                for lst in built[:5]:
                    for t in lst:
                        t.record_stream(main)
        else:
            built = build_targets()
        if built is None:
            return None
        labels_list, label_weights_list, anchor_list, bbox_targets_list, level_pos, num_total_pos = built
        if dist.is_available() and dist.is_initialized():
            # rank mean of the positive count (atss_rpn_head.py:440-444), kept on the device
            num_total_samples = reduce_mean(
                torch.tensor(num_total_pos, dtype=torch.float, device=device)).clamp(min=1.0)
        else:
            num_total_samples = max(float(num_total_pos), 1.0)
        losses_cls, losses_bbox, losses_iou, bbox_avg_factor = multi_apply(
            self.loss_single, anchor_list, cls_scores, bbox_preds, iou_preds, labels_list,
            label_weights_list, bbox_targets_list, level_pos, num_total_samples=num_total_samples)
        bbox_avg_factor = sum(bbox_avg_factor)
        # stays a device scalar: reading it back would stall the host behind the whole forward pass
        bbox_avg_factor = reduce_mean(bbox_avg_factor).clamp(min=1).detach()
        losses_bbox = [x / bbox_avg_factor for x in losses_bbox]
        return dict(loss_rpn_cls=losses_cls, loss_rpn_bbox=losses_bbox, loss_rpn_iou=losses_iou)

    # ------------------------------------------------------------------ device-resident train step
    def _fused_loss_modes(self):
        """(cls_mode, reg_mode) of `brcnn_rpn_loss_*` for this head's loss configuration, or None when the
        kernels do not cover it.  Covered: FocalLoss / VarifocalLoss classification; decoded regression with
        IoULoss('log') [+ MSELoss aug] or raw-delta regression with CIoULoss (reg_decoded_bbox=False)."""
        from .losses import CIoULoss, FocalLoss, IoULoss, MSELoss, VarifocalLoss
        if type(self.loss_cls) is FocalLoss:
            cls_mode = 0
        elif type(self.loss_cls) is VarifocalLoss and self.loss_cls.use_sigmoid:
            cls_mode = 1 if self.loss_cls.iou_weighted else 2
        else:
            return None
        if self.loss_cls.reduction != 'mean' or self.loss_bbox.reduction != 'mean':
            return None
        if self.reg_decoded_bbox:
            if not (type(self.loss_bbox) is IoULoss and self.loss_bbox.mode == 'log'):
                return None
            if self.with_aug_loss and not (type(self.aug_loss) is MSELoss and self.aug_loss.reduction == 'mean'):
                return None
            return cls_mode, 0
        if type(self.loss_bbox) is CIoULoss and self.loss_bbox.eps == 1e-6:
            return cls_mode, 1
        return None

    def device_train_ok(self):
        """the loss / target configurations the fused target / loss kernels cover (all nine recipes):
        focal or varifocal classification, decoded IoU-log regression + MSE aug or CIoU on raw deltas,
        sigmoid-BCE IoU branch, MaxIoU assignment without ignore regions"""
        from .core import MaxIoUAssigner, PseudoSampler
        from .losses import CrossEntropyLoss
        tc = self.train_cfg
        return bool(
            tc is not None and self.use_sigmoid_cls and self.cls_out_channels == 1 and
            self._fused_loss_modes() is not None and
            type(self.loss_centerness) is CrossEntropyLoss and self.loss_centerness.use_sigmoid and
            self.loss_centerness.class_weight is None and self.loss_centerness.reduction == 'mean' and
            type(self.assigner) is MaxIoUAssigner and self.assigner.ignore_iof_thr <= 0 and
            self.assigner.gt_max_assign_all and type(self.sampler) is PseudoSampler and
            not getattr(self.bbox_coder, 'add_ctr_clamp', False))

    def _tower_fusable(self):
        return all(isinstance(c.norm, nn.GroupNorm) and c.conv.bias is None and c.conv.groups == 1
                   for c in self.rpn_convs) and self.feat_channels <= 256 and self.feat_channels % 4 == 0

    def forward_head_fused(self, feats):
        """training forward of tower + heads over all levels (one launch per layer); returns the fused
        head output y (rows, Cpad) fp32 [cls A | reg 4A (raw, before Scale) | iou A | zero padding],
        level-major rows, differentiable"""
        from .autograd import ConvNHWCFunction, GroupNormNHWCFunction, conv2d_nhwc_multi_autograd, fused_head_weights
        B = feats[0].shape[0]
        sizes = tuple(tuple(int(v) for v in f.shape[1:3]) for f in feats)
        x = cat_rows(feats)        # (a view when the neck wrote the levels back to back: ops.output_into)
        for conv in self.rpn_convs:
            x = conv2d_nhwc_multi_autograd(x, conv.conv.weight, None, B, sizes, 1, conv.conv.padding[0])
            x = GroupNormNHWCFunction.apply(x, conv.norm.weight, conv.norm.bias, conv.norm.num_groups, B, sizes,
                                            conv.norm.eps, conv.with_activation)
        heads = (self.rpn_cls, self.rpn_reg, self.rpn_iou)
        # (one differentiable node for cat + pad whose backward hands out views: the fused head's weight-gradient launch
        # leaves the main stream like the others)
        w, b = fused_head_weights(heads, 32 if x.dtype == torch.float32 else 64)
        y = ConvNHWCFunction.apply(x, w, b, B, sizes, 1, self.rpn_cls.padding[0], False, False, True)   # fp32 head output
        return y, sizes

    def loss_fused(self, y, sizes, gt_bboxes, img_metas, gt_flat=None, scales=None):
        """ATSSRPNHead.loss on the fused head output: assignment + every loss term in HIP kernels, no
        host synchronisation.  Each loss comes back as a one-element list holding the sum over the
        pyramid levels (the reference returns the per-level terms and sums them in _parse_losses);
        `self.last_rpn_targets` keeps (gt_inds, per-level losses (3, L), [num_pos, sum iou_target])."""
        from . import train_ops
        device = y.device
        gts, _, offs = gt_flat if gt_flat is not None else train_ops.flatten_gts(gt_bboxes)
        gt_inds = self.assign_targets_device(sizes, img_metas, gts, offs, device)
        tc = self.train_cfg
        meta = train_ops.RPNLossMeta(
            len(img_metas), sizes, self.anchor_generator.strides,
            [self._base_anchors(l, device) for l in range(len(sizes))], self.num_anchors, offs, self.loss_cls.gamma,
            self.loss_cls.alpha, tc.pos_weight, self.gamma, self.bbox_coder.means, self.bbox_coder.stds, 16 / 1000,
            self.with_aug_loss, self.loss_cls.loss_weight, self.loss_bbox.loss_weight,
            self.aug_loss.loss_weight if self.with_aug_loss else 0.0, self.loss_centerness.loss_weight,
            *self._fused_loss_modes())
        if scales is None:
            scales = torch.stack([m.scale.reshape(()) for m in self.scales])
        losses3, per_level, totals = train_ops.rpn_loss(y, scales, gt_inds, gts, meta)
        self.last_rpn_targets = (gt_inds, per_level, totals)
        return dict(loss_rpn_cls=[losses3[0]], loss_rpn_bbox=[losses3[1]], loss_rpn_iou=[losses3[2]])

    def proposals_fused(self, y, sizes, img_metas, cfg):
        """proposal stage straight from the fused head output (no copies: channel-slice views), with
        the live Scale parameters read on the device; returns padded (dets (B,K,5), num (B,))"""
        yd = y.detach()
        B = len(img_metas)
        a, c = self.num_anchors, self.cls_out_channels
        cls, reg, iou, r0 = [], [], [], 0
        for (h, w) in sizes:
            n = B * h * w
            t = yd[r0:r0 + n].view(B, h, w, yd.shape[1])
            cls.append(t[..., :a * c])
            reg.append(t[..., a * c:a * c + 4 * a])
            iou.append(t[..., a * c + 4 * a:a * c + 5 * a])
            r0 += n
        scales = torch.stack([m.scale.detach().reshape(()) for m in self.scales]).float().contiguous()
        return self.get_bboxes_padded(cls, reg, iou, img_metas, cfg=cfg, reg_scales=scales)

    # ------------------------------------------------------------------ proposals
    def _proposal_scores(self, cls, iou):
        return ops.rpn_score(cls, iou)

    def get_bboxes_padded(self, cls_nhwc, reg_nhwc, iou_nhwc, img_metas, cfg=None, reg_scales=None):
        """the device-resident proposal stage (`AnchorHead._proposals_padded`), ranked by sqrt(sigmoid(cls) * sigmoid(iou))"""
        return self._proposals_padded(cls_nhwc, reg_nhwc, iou_nhwc, img_metas, cfg, reg_scales)

    def get_bboxes(self, cls_scores, bbox_preds, iou_preds, img_metas, cfg=None, rescale=False,
                   with_nms=True):
        """reference signature (atss_rpn_head.py:466-503): per-level (N,A,h,w) / (N,4A,h,w) /
        (N,A,h,w) -> list of (k,5) proposals per image."""
        assert with_nms, '``with_nms`` in RPNHead should always True'
        assert len(cls_scores) == len(bbox_preds)
        f = lambda lst: [to_nhwc(t.detach()).contiguous() for t in lst]  # noqa: E731
        dets, num = self.get_bboxes_padded(f(cls_scores), f(bbox_preds), f(iou_preds), img_metas, cfg)
        num = num.tolist()   # the one host sync of the proposal stage
        return [dets[i, :num[i]] for i in range(len(img_metas))]

    def simple_test_rpn(self, x, img_metas):
        cls_scores, bbox_preds, iou_preds = self(x)
        return self.get_bboxes(cls_scores, bbox_preds, iou_preds, img_metas)

    # ------------------------------------------------------------------ test-time augmentation
    def aug_test_rpn(self, feats, img_metas):
        """dense_test_mixins.py:128-160: `feats` per aug the NCHW pyramid, `img_metas` per aug the batch's metas; per aug
        the plain proposal stage, per image the proposals of all augs merged in the original frame
        (core.merge_aug_proposals) -> list over images of (n, 5)"""
        from .core import merge_aug_proposals
        per_aug = [self.simple_test_rpn(x, metas) for x, metas in zip(feats, img_metas)]
        return [merge_aug_proposals([props[b] for props in per_aug], [metas[b] for metas in img_metas], self.test_cfg)
                for b in range(len(img_metas[0]))]

    def aug_test_rpn_padded(self, feats_per_aug, img_metas_per_aug, geom=None, reg_scales=None):
        """`aug_test_rpn` for the whole batch on the device, no host sync: per aug the fused tower and
        `get_bboxes_padded` on its NHWC pyramid, then one launch that maps every aug's proposals back to the original
        image into aug-major candidate slots and ONE segmented NMS (a segment per image, `max_per_img` survivors).
        Returns the merged (dets (B, max_per_img, 5), num (B,) int32) and the geometry table."""
        cfg = self.test_cfg
        nms_cfg = dict(cfg.nms)
        assert nms_cfg.pop('type', 'nms') == 'nms', 'RPN proposals use greedy NMS'
        dets_l, num_l = [], []
        for feats, metas in zip(feats_per_aug, img_metas_per_aug):
            cls, reg, iou = self.split_fused(self.forward_fused(list(feats)))
            if reg_scales is None:      # the live Scale parameters, read on the device
                reg_scales = torch.stack([m.scale.detach().reshape(()) for m in self.scales]).float().contiguous()
            dets, num = self.get_bboxes_padded(cls, reg, iou, metas, reg_scales=reg_scales)
            dets_l.append(dets)
            num_l.append(num)
        if geom is None:
            geom = ops.tta_geometry(img_metas_per_aug, dets_l[0])
        _, boxes, scores, valid = ops.tta_gather_proposals(dets_l, num_l, geom)
        merged, _, num = batched_nms_images(boxes, scores, torch.zeros_like(scores, dtype=torch.long), valid,
                                            nms_cfg['iou_threshold'], cfg.max_per_img, nms_cfg.get('offset', 0))
        return merged, num, geom


# ----------------------------------------------------------------------------- Faster R-CNN baseline
@HEADS.register_module()
class RPNHead(AnchorHead):
    """The plain RPN of the Faster R-CNN baseline (mmdet/models/dense_heads/rpn_head.py:16-249 over
    anchor_head.py:37-497): `rpn_conv` (one 3x3 Conv2d, or `rpn_conv.{i}.conv` for num_convs > 1) + ReLU, then the 1x1
    `rpn_cls` / `rpn_reg`; sigmoid objectness, 256 anchors drawn per image for the loss.  Parameter names and shapes
    are the reference's.  Execution: the 3x3 conv and the two 1x1 heads (as ONE launch, [cls A | reg 4A]) run over
    all pyramid levels at once on the NHWC conv kernels; the proposal stage and the whole-batch assignment are the
    head-agnostic ones of AnchorHead that ATSSRPNHead uses too; the sampled loss has its own kernels (csrc/rpn_sampled.hip)."""

    plain_rpn = True        # (detectors.py: no IoU branch, no per-level Scale, no early RPN backward pass)
    supports_tta = False
    # nms_pre / candidate limits of the device proposal stage (include/brcnn_hip.h: brcnn_rpn_topk, brcnn_nms_prepare_levels)
    MAX_NMS_PRE, MAX_CANDIDATES, MAX_LEVELS = 4096, 16384, 8

    def __init__(self, in_channels, num_classes=1, init_cfg=None, num_convs=1, **kwargs):
        if not kwargs.get('loss_cls', dict(use_sigmoid=True)).get('use_sigmoid', False):
            raise NotImplementedError('RPNHead: loss_cls.use_sigmoid=False (two-channel softmax objectness) is not '
                                      'supported; the device proposal stage and the sampled loss score with a sigmoid')
        self.num_convs = num_convs
        super().__init__(num_classes, in_channels, init_cfg=init_cfg, **kwargs)
        if self.cls_out_channels != 1:
            raise NotImplementedError(f'RPNHead: num_classes={num_classes}; the RPN scores one objectness per anchor')
        self._conv_caches = [PackedCache() for _ in range(max(num_convs, 1))]
        self._fused_head_cache = PackedCache()
        self._base_anchor_cache = {}
        self.init_weights()

    def _init_layers(self):
        if self.num_convs > 1:
            self.rpn_conv = nn.Sequential(*[
                ConvModule(self.in_channels if i == 0 else self.feat_channels, self.feat_channels, 3, padding=1,
                           inplace=False) for i in range(self.num_convs)])
        else:
            self.rpn_conv = nn.Conv2d(self.in_channels, self.feat_channels, 3, padding=1)
        self.rpn_cls = nn.Conv2d(self.feat_channels, self.num_anchors * self.cls_out_channels, 1)
        self.rpn_reg = nn.Conv2d(self.feat_channels, self.num_anchors * 4, 1)

    def init_weights(self):
        """init_cfg=dict(type='Normal', layer='Conv2d', std=0.01) (rpn_head.py:28)"""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, 0, 0.01)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    def _tower_convs(self):
        return [self.rpn_conv] if self.num_convs <= 1 else [m.conv for m in self.rpn_conv]

    # ------------------------------------------------------------------ forward
    def forward_fused(self, feats):
        """inference: list of (B,h,w,C) NHWC maps -> per level a (B,h,w,5A) fp32 tensor [cls A | reg 4A]; every layer
        is one launch over all levels (the weights are shared across them)"""
        B = feats[0].shape[0]
        sizes = [tuple(f.shape[1:3]) for f in feats]
        x = cat_rows(feats)
        for conv, cache in zip(self._tower_convs(), self._conv_caches):
            w, b = cache.get([conv.weight, conv.bias], lambda c=conv: (pack_weight(c.weight).to(x.dtype),
                                                                      c.bias.detach().float().contiguous()))
            x, _ = ops.conv2d_nhwc_multi(x, w, B, sizes, None, b, None, True, 1, 1)      # bias + ReLU in the read-out
        heads = (self.rpn_cls, self.rpn_reg)

        def builder():
            return (torch.cat([pack_weight(h.weight) for h in heads], 0).to(x.dtype).contiguous(),
                    torch.cat([h.bias.detach().float() for h in heads], 0).contiguous())
        w, b = self._fused_head_cache.get([t for h in heads for t in (h.weight, h.bias)], builder)
        y, _ = ops.conv2d_nhwc_multi(x, w, B, sizes, None, b, None, False, 1, 0, out_f32=True)
        outs, r0 = [], 0
        for (h, wd) in sizes:
            n = B * h * wd
            outs.append(y[r0:r0 + n].view(B, h, wd, y.shape[1]))
            r0 += n
        return outs

    def split_fused(self, fused):
        a = self.num_anchors
        return [f[..., :a] for f in fused], [f[..., a:5 * a] for f in fused]

    def forward_head_fused(self, feats):
        """training forward over all levels; returns the fused head output y (rows, Cpad) fp32
        [cls A | reg 4A | zero padding], level-major rows, differentiable"""
        from .autograd import ConvNHWCFunction, conv2d_nhwc_multi_autograd, fused_head_weights
        B = feats[0].shape[0]
        sizes = tuple(tuple(int(v) for v in f.shape[1:3]) for f in feats)
        x = cat_rows(feats)
        mult = 32 if x.dtype == torch.float32 else 64
        for conv in self._tower_convs():
            if conv.out_channels % mult == 0:       # ReLU in the kernel's read-out
                x = ConvNHWCFunction.apply(x, conv.weight, conv.bias, B, sizes, 1, 1, False, True, False)
            else:
                x = conv2d_nhwc_multi_autograd(x, conv.weight, conv.bias, B, sizes, 1, 1).relu()
        w, b = fused_head_weights((self.rpn_cls, self.rpn_reg), mult)
        y = ConvNHWCFunction.apply(x, w, b, B, sizes, 1, 0, False, False, True)
        return y, sizes

    def forward_nhwc(self, feats):
        """list of (B,h,w,C) -> (cls (B,h,w,A), reg (B,h,w,4A)) lists, fp32"""
        from .autograd import wants_grad
        if wants_grad(feats[0], self.rpn_cls.weight, self._tower_convs()[0].weight):
            y, sizes = self.forward_head_fused(list(feats))
            B, fused, r0 = feats[0].shape[0], [], 0
            for (h, w) in sizes:
                fused.append(y[r0:r0 + B * h * w].view(B, h, w, y.shape[1]))
                r0 += B * h * w
        else:
            fused = self.forward_fused(list(feats))
        return self.split_fused(fused)

    def forward(self, feats):
        """reference signature: list of (N,C,h,w) -> lists of (N,A,h,w), (N,4A,h,w)"""
        cls, reg = self.forward_nhwc([to_nhwc(f) for f in feats])
        v = lambda lst: [t.permute(0, 3, 1, 2) for t in lst]  # noqa: E731
        return v(cls), v(reg)

    # ------------------------------------------------------------------ proposals
    def _check_proposal_limits(self, cfg, sizes):
        """the sizes the device proposal stage serves (brcnn_rpn_topk: k <= 4096; brcnn_nms_prepare_levels: <= 8 levels,
        <= 16384 candidates per image); anything beyond is refused, not served some slower way"""
        if not 0 < cfg.nms_pre <= self.MAX_NMS_PRE:
            raise ValueError(f'RPNHead: nms_pre={cfg.nms_pre} outside (0, {self.MAX_NMS_PRE}] (brcnn_rpn_topk)')
        if len(sizes) > self.MAX_LEVELS:
            raise ValueError(f'RPNHead: {len(sizes)} pyramid levels, at most {self.MAX_LEVELS} are supported')
        total = sum(min(cfg.nms_pre, h * w * self.num_anchors) for h, w in sizes)
        if total > self.MAX_CANDIDATES:
            raise ValueError(f'RPNHead: {total} NMS candidates per image, at most {self.MAX_CANDIDATES} are supported '
                             '(brcnn_nms_prepare_levels)')
        if cfg.nms.get('type', 'nms') != 'nms':
            raise ValueError('RPNHead: proposals use greedy NMS')

    def _proposal_scores(self, cls, iou):
        """rpn_head.py:203-205: the sigmoid alone (ATSSRPNHead: sqrt(sigmoid(cls) * sigmoid(iou)))"""
        return cls.float().sigmoid().contiguous()

    def get_bboxes_padded(self, cls_nhwc, reg_nhwc, img_metas, cfg=None, per_image_shapes=False):
        """rpn_head.py:159-249 for the whole batch on the device, no host sync: sigmoid scores, per-level top-k, decode
        (`per_image_shapes`: the clip border from a device table, training batches of differently sized images),
        min_bbox_size filter, level-aware NMS, max_per_img.  Returns (dets (B, max_per_img, 5) zero padded, num (B,))"""
        cfg = self.test_cfg if cfg is None else cfg
        self._check_proposal_limits(cfg, [tuple(c.shape[1:3]) for c in cls_nhwc])
        scales = None
        if per_image_shapes and len({tuple(m['img_shape'][:2]) for m in img_metas}) > 1:
            scales = torch.ones(len(cls_nhwc), dtype=torch.float32, device=cls_nhwc[0].device)
        return self._proposals_padded(cls_nhwc, reg_nhwc, None, img_metas, cfg=cfg, reg_scales=scales)

    def proposals_fused(self, y, sizes, img_metas, cfg):
        """proposal stage straight from the fused training head output (channel-slice views, no copies)"""
        yd = y.detach()
        B, a = len(img_metas), self.num_anchors
        cls, reg, r0 = [], [], 0
        for (h, w) in sizes:
            n = B * h * w
            t = yd[r0:r0 + n].view(B, h, w, yd.shape[1])
            cls.append(t[..., :a])
            reg.append(t[..., a:5 * a])
            r0 += n
        return self.get_bboxes_padded(cls, reg, img_metas, cfg=cfg, per_image_shapes=True)

    def simple_test_padded(self, feats_nhwc, img_metas):
        cls, reg = self.split_fused(self.forward_fused(list(feats_nhwc)))
        return self.get_bboxes_padded(cls, reg, img_metas)

    def get_bboxes(self, cls_scores, bbox_preds, img_metas, cfg=None, rescale=False, with_nms=True):
        """reference signature (rpn_head.py:104-157): per-level (N,A,h,w) / (N,4A,h,w) -> list of (k,5) per image"""
        assert with_nms, '``with_nms`` in RPNHead should always True'
        assert len(cls_scores) == len(bbox_preds)
        f = lambda lst: [to_nhwc(t.detach()).contiguous() for t in lst]  # noqa: E731
        dets, num = self.get_bboxes_padded(f(cls_scores), f(bbox_preds), img_metas, cfg, per_image_shapes=True)
        num = num.tolist()   # the one host sync of the proposal stage
        return [dets[i, :num[i]] for i in range(len(img_metas))]

    def simple_test_rpn(self, x, img_metas):
        cls_scores, bbox_preds = self(x)
        return self.get_bboxes(cls_scores, bbox_preds, img_metas)

    # ------------------------------------------------------------------ train
    def forward_train(self, x, img_metas, gt_bboxes, gt_labels=None, gt_bboxes_ignore=None, proposal_cfg=None, **kwargs):
        outs = self(x)
        losses = self.loss(*outs, gt_bboxes, img_metas, gt_bboxes_ignore=gt_bboxes_ignore)
        if proposal_cfg is None:
            return losses
        return losses, self.get_bboxes(*outs, img_metas, cfg=proposal_cfg)

    def loss(self, cls_scores, bbox_preds, gt_bboxes, img_metas, gt_bboxes_ignore=None):
        """rpn_head.py:70-101 / anchor_head.py:423-497.  Device tensors of a covered configuration go to the HIP
        kernels (`loss_fused`); otherwise the reference's per-image chain in torch (the host path: `self.last_drawn`
        keeps the drawn (pos_inds, neg_inds) per image)."""
        featmap_sizes = [f.size()[-2:] for f in cls_scores]
        assert len(featmap_sizes) == self.anchor_generator.num_levels
        device = cls_scores[0].device
        if device.type == 'cuda' and gt_bboxes_ignore is None and self.device_train_ok():
            sizes = tuple(tuple(int(v) for v in s_) for s_ in featmap_sizes)
            rows = [torch.cat([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in (c_, r_)], 1)
                    for c_, r_ in zip(cls_scores, bbox_preds)]
            return self.loss_fused(torch.cat(rows, 0).float().contiguous(), sizes, gt_bboxes, img_metas)
        num_imgs = len(img_metas)
        anchor_list, valid_flag_list = self.get_anchors(featmap_sizes, img_metas, device=device)
        num_level_anchors = [a.size(0) for a in anchor_list[0]]
        flat_anchors = [torch.cat(a) for a in anchor_list]
        flat_flags = [torch.cat(v) for v in valid_flag_list]
        ignore = gt_bboxes_ignore if gt_bboxes_ignore is not None else [None] * num_imgs
        all_valid = self._all_valid
        self._all_valid = None
        (labels, label_weights, bbox_targets, bbox_weights, pos_inds, neg_inds, _) = multi_apply(
            self._get_targets_single, flat_anchors, flat_flags, gt_bboxes, ignore, [None] * num_imgs, img_metas, all_valid)
        if any(l is None for l in labels):
            return None
        self.last_drawn = list(zip(pos_inds, neg_inds))
        num_total_samples = sum(max(p.numel(), 1) for p in pos_inds) + sum(max(n.numel(), 1) for n in neg_inds)
        losses_cls, losses_bbox = multi_apply(
            self.loss_single, cls_scores, bbox_preds, images_to_levels(flat_anchors, num_level_anchors),
            images_to_levels(labels, num_level_anchors), images_to_levels(label_weights, num_level_anchors),
            images_to_levels(bbox_targets, num_level_anchors), images_to_levels(bbox_weights, num_level_anchors),
            num_total_samples=num_total_samples)
        return dict(loss_rpn_cls=losses_cls, loss_rpn_bbox=losses_bbox)

    # ------------------------------------------------------------------ device-resident train step
    def _tower_fusable(self):
        return True

    def device_train_ok(self):
        """what the sampled-loss kernels cover: sigmoid cross-entropy without class weights, L1 / SmoothL1 on encoded
        deltas, MaxIoU assignment without ignore regions, the RandomSampler without added ground truths"""
        from .core import MaxIoUAssigner, RandomSampler
        from .losses import CrossEntropyLoss, L1Loss, SmoothL1Loss
        tc = self.train_cfg
        return bool(
            tc is not None and type(self.loss_cls) is CrossEntropyLoss and self.loss_cls.use_sigmoid and
            self.loss_cls.class_weight is None and self.loss_cls.reduction == 'mean' and
            type(self.loss_bbox) in (L1Loss, SmoothL1Loss) and self.loss_bbox.reduction == 'mean' and
            not self.reg_decoded_bbox and type(self.assigner) is MaxIoUAssigner and self.assigner.ignore_iof_thr <= 0 and
            self.assigner.gt_max_assign_all and type(self.sampler) is RandomSampler and
            not self.sampler.add_gt_as_proposals and 0 < self.sampler.num <= 2048 and
            not getattr(self.bbox_coder, 'add_ctr_clamp', False))

    def loss_fused(self, y, sizes, gt_bboxes, img_metas, gt_flat=None):
        """RPNHead.loss on the fused head output: whole-batch assignment, then the RandomSampler's draw -- the device
        compacts the candidates, the host reads the (B, 2) counts (this head's one host read) and draws the
        permutations with the reference's calls in the reference's order -- then the sampled loss kernels.
        `self.last_rpn_targets` keeps (gt_inds, drawn (B, num) int32, num_total_samples)."""
        from . import train_ops
        device = y.device
        gts, _, offs = gt_flat if gt_flat is not None else train_ops.flatten_gts(gt_bboxes)
        B, sp = len(img_metas), self.sampler
        gt_inds, counts = self.assign_targets_device(sizes, img_metas, gts, offs, device, want_counts=True)
        num_pos = int(sp.num * sp.pos_fraction)
        cnt = [tuple(c) for c in counts.tolist()]            # the host read: (B, 2) candidate counts
        perm, _ = train_ops.draw_sampler_perms(cnt, sp.num, num_pos, sp.neg_pos_ub)
        total = train_ops.rpn_num_total_samples(cnt, sp.num, num_pos, sp.neg_pos_ub)
        meta = train_ops.RPNSampledMeta(
            B, sizes, self.anchor_generator.strides, [self._base_anchors(l, device) for l in range(len(sizes))],
            self.num_anchors, offs, sp.num, num_pos, sp.neg_pos_ub, self.train_cfg.pos_weight,
            getattr(self.loss_bbox, 'beta', 0.0), self.bbox_coder.means, self.bbox_coder.stds,
            self.loss_cls.loss_weight, self.loss_bbox.loss_weight)
        drawn, ws = train_ops.rpn_sampled_draw(gt_inds, perm.to(device, non_blocking=True), meta)
        losses2 = train_ops.rpn_sampled_loss(y, gt_inds, gts, drawn, meta, total, workspace=ws)
        self.last_rpn_targets = (gt_inds, drawn, total)
        return dict(loss_rpn_cls=[losses2[0]], loss_rpn_bbox=[losses2[1]])


# ----------------------------------------------------------------------------- single-stage detection heads
class DenseDetHead:
    """What RetinaHead, FCOSHead and ATSSHead share beyond their layers (a mixin in front of the nn.Module base): the
    test-cfg and limit checks, the Normal(0.01) / bias_prob initialisation, the class-aware NMS of the device path's
    candidate slots, the `get_bboxes` skeleton (device or host dispatch, the one host sync) with the tail of the host
    mirror, and the reference's simple_test / forward_train drivers.  A head supplies `_get_bboxes_device(outs, img_metas,
    cfg, rescale)` -> padded (dets, labels, num) and the three hooks of `_get_bboxes_host` (RetinaHead, with several
    anchors per cell, keeps a `_get_bboxes_host` of its own)."""

    supports_tta = False
    # nms_pre / level limits of the device path (include/brcnn_hip.h: brcnn_rpn_topk)
    MAX_NMS_PRE, MAX_LEVELS = 4096, 8

    def _init_normal(self, cls_conv):
        """init_cfg=dict(type='Normal', layer='Conv2d', std=0.01, override=dict(name=<the class conv>, bias_prob=0.01))"""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, 0, 0.01)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        nn.init.constant_(cls_conv.bias, bias_init_with_prob(0.01))

    def _check_test_cfg(self, cfg):
        name = type(self).__name__
        nms = cfg.get('nms', dict(type='nms'))
        if nms.get('type', 'nms') != 'nms':
            raise NotImplementedError(f"{name}: test_cfg.nms.type={nms.get('type')!r}; only greedy 'nms' is supported "
                                      '(no soft-NMS)')
        if nms.get('class_agnostic', False):
            raise NotImplementedError(f'{name}: test_cfg.nms.class_agnostic=True is not supported')

    def _check_limits(self, cfg, sizes):
        """the sizes the device path serves (brcnn_rpn_topk: k <= 4096, <= 8 levels); anything beyond is refused"""
        name = type(self).__name__
        if not 0 < cfg.get('nms_pre', -1) <= self.MAX_NMS_PRE:
            raise ValueError(f"{name}: nms_pre={cfg.get('nms_pre', -1)} outside (0, {self.MAX_NMS_PRE}] (brcnn_rpn_topk)")
        self._check_levels(sizes)

    def _check_levels(self, sizes):
        if len(sizes) > self.MAX_LEVELS:
            raise ValueError(f'{type(self).__name__}: {len(sizes)} pyramid levels, at most {self.MAX_LEVELS} are supported')

    def _refuse_ignore(self, gt_bboxes_ignore):
        if gt_bboxes_ignore is not None:
            raise NotImplementedError(f'{type(self).__name__}: gt_bboxes_ignore is not supported on the device path')

    @staticmethod
    def _nms_candidates(bb, sc, lb, va, C, cfg):
        """class-aware NMS + max_per_img of the (level, pick, class) candidate slots of a dense head"""
        B = bb.shape[0]
        nms_cfg = dict(cfg.nms)
        nms_cfg.pop('type', None)
        T = sc.shape[1] // C
        # mmcv's batched_nms changes branch at split_thr by the number of candidates that SURVIVE score_thr (n_valid), which
        # only the device knows here; the branch is chosen by the slot count T * C instead, so no host read is needed.
        # Both branches keep the same boxes in the same order (the coordinate offsets already isolate the classes), with
        # one limit: where the reference takes the offset form and this code the per-class one (or the reverse), the
        # IoUs are computed on un-offset resp. offset fp32 coordinates and can differ in the last ulp -- a pair whose IoU
        # sits within an ulp of iou_threshold may then be decided differently.
        if T * C >= nms_cfg.get('split_thr', 10000):
            # the per-class branch: class-major slots, one segmented NMS launch over (image, class)
            from .postprocess import batched_nms_images_by_level
            cm = lambda t: t.view(B, T, C, *t.shape[2:]).transpose(1, 2).reshape(B, C * T, *t.shape[2:]).contiguous()   # noqa: E731
            return batched_nms_images_by_level(cm(bb), cm(sc), cm(lb), cm(va), [T] * C, nms_cfg['iou_threshold'],
                                               cfg.max_per_img, nms_cfg.get('offset', 0), return_ids=True)
        return batched_nms_images(bb, sc, lb, va, nms_cfg['iou_threshold'], cfg.max_per_img, nms_cfg.get('offset', 0))

    def _get_bboxes(self, outs, img_metas, cfg, rescale, with_nms, batched_nms):
        """`get_bboxes` behind each head's reference signature; `outs`: the per-level lists of the head's outputs.  Device
        tensors take the head's padded device path and are cut to size after its one host sync; CPU tensors take the
        reference's chain on torch ops with the caller's `batched_nms` (this package's NMS is a device kernel)."""
        if not with_nms:
            raise NotImplementedError(f'{type(self).__name__}: with_nms=False is not supported')
        assert all(len(o) == len(outs[0]) for o in outs)
        if outs[0][0].is_cuda:
            det, lab, num = self._get_bboxes_device([[t.detach() for t in o] for o in outs], img_metas, cfg, rescale)
            num = num.tolist()   # the one host sync
            return [(det[i, :num[i]], lab[i, :num[i]]) for i in range(len(img_metas))]
        cfg = self.test_cfg if cfg is None else cfg
        self._check_test_cfg(cfg)
        return self._get_bboxes_host(*outs, img_metas, cfg, rescale, ops.batched_nms if batched_nms is None else batched_nms)

    def _get_bboxes_host(self, *args):
        """the host mirror of `get_bboxes` on torch ops, `args` = (*outs, img_metas, cfg, rescale, batched_nms): per image and
        level the nms_pre best candidates (stable descending sort: ties by ascending index), the head's decode and clip,
        then `_host_nms`.  A head supplies `_priors_host(sizes, outs)` -> per level the anchors or points, `_level_host(l,
        *maps)` -> (box values (n, ..), centerness sigmoid (n,) or None) from the level's (h,w,C) maps after the class map,
        and `_decode_host(priors, d, (h_img, w_img))` -> clipped boxes"""
        *outs, img_metas, cfg, rescale, batched_nms = args
        B, C = outs[0][0].shape[0], self.cls_out_channels
        priors_l = self._priors_host([c.shape[-2:] for c in outs[0]], outs)
        nms_pre = cfg.get('nms_pre', -1)
        out = []
        for b in range(B):
            boxes_l, scores_l, ctr_l = [], [], []
            for l, (priors, cls, *maps) in enumerate(zip(priors_l, *outs)):
                s = cls[b].detach().permute(1, 2, 0).reshape(-1, C).sigmoid()
                d, ct = self._level_host(l, *[m[b].detach().permute(1, 2, 0) for m in maps])
                if 0 < nms_pre < s.shape[0]:
                    rank = s if ct is None else s * ct[:, None]
                    _, idx = rank.max(-1)[0].sort(descending=True, stable=True)   # ties by ascending index
                    idx = idx[:nms_pre]
                    priors, d, s, ct = priors[idx], d[idx], s[idx], (None if ct is None else ct[idx])
                boxes_l.append(self._decode_host(priors, d, img_metas[b]['img_shape'][:2]))
                scores_l.append(s)
                ctr_l.append(ct)
            factor = None if ctr_l[0] is None else torch.cat(ctr_l)
            out.append(self._host_nms(torch.cat(boxes_l), torch.cat(scores_l), factor, img_metas[b], cfg, rescale, batched_nms))
        return out

    def _host_nms(self, boxes, scores, factor, img_meta, cfg, rescale, batched_nms):
        """the tail of the host mirror for one image: rescale, score threshold on the class score (before the optional
        per-box `factor`, bbox_nms.py:48-58), fan-out to classes, class-aware NMS, max_per_img -> (dets (k,5), labels (k,))"""
        C = self.cls_out_channels
        if rescale:
            boxes = boxes / boxes.new_tensor(img_meta['scale_factor'])
        keep = (scores > cfg.score_thr).reshape(-1)
        inds = keep.nonzero(as_tuple=False).reshape(-1)
        labels = torch.arange(C, dtype=torch.long).repeat(scores.shape[0])[inds]
        cb = boxes[:, None].expand(-1, C, 4).reshape(-1, 4)[inds]
        cs = (scores if factor is None else scores * factor[:, None]).reshape(-1)[inds]
        if cb.numel() == 0:
            return torch.cat([cb, cs[:, None]], -1), labels
        dets, kept = batched_nms(cb.contiguous(), cs.contiguous(), labels, dict(cfg.nms))
        if cfg.max_per_img > 0:
            dets, kept = dets[:cfg.max_per_img], kept[:cfg.max_per_img]
        return dets, labels[kept]

    def simple_test(self, feats, img_metas, rescale=False, batched_nms=None):
        """dense_test_mixins.py:17-37: list of (N,C,h,w) -> per image (dets (k,5), labels (k,))"""
        return self.get_bboxes(*self(feats), img_metas, rescale=rescale, batched_nms=batched_nms)

    def aug_test(self, feats, img_metas, rescale=False):
        raise NotImplementedError(f'{type(self).__name__} has no test-time augmentation')

    def forward_train(self, x, img_metas, gt_bboxes, gt_labels=None, gt_bboxes_ignore=None, proposal_cfg=None, **kwargs):
        """base_dense_head.py:48-78"""
        outs = self(x)
        losses = self.loss(*outs, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=gt_bboxes_ignore)
        if proposal_cfg is None:
            return losses
        return losses, self.get_bboxes(*outs, img_metas, cfg=proposal_cfg)


class GNTowerHead(DenseDetHead):
    """What FCOSHead, ATSSHead and GFLHead share on top of DenseDetHead: two towers of `stacked_convs` 3x3 conv + GroupNorm
    + ReLU (`cls_convs`, `reg_convs`), each ending in ONE fused fp32 head conv whose columns `_head_groups()` names, one
    `Scale` per level, and the (A, R) row tensors the kernels of csrc/fcos_head.hip, csrc/atss_head.hip and csrc/gfl_head.hip
    read in place.  A head supplies `_head_groups`, `_cls_conv`, `_split_rows`, `_heads_host`, `_layout`,
    `_rows_from_reference`, `_decode_candidates` and `loss_fused`, and `_score_rows` when it does not rank by the centerness
    product."""

    def _init_towers(self):
        self.cls_convs, self.reg_convs = nn.ModuleList(), nn.ModuleList()
        for i in range(self.stacked_convs):
            chn = self.in_channels if i == 0 else self.feat_channels
            for convs in (self.cls_convs, self.reg_convs):
                convs.append(ConvModule(chn, self.feat_channels, 3, stride=1, padding=1, conv_cfg=self.conv_cfg,
                                        norm_cfg=self.norm_cfg, bias='auto'))
        self._tower_caches = [[PackedCache() for _ in range(self.stacked_convs)] for _ in range(2)]
        self._head_caches = [PackedCache(), PackedCache()]
        self._scale_cache = PackedCache()

    def _check_levels(self, sizes):
        if len(sizes) != len(self.strides):
            raise ValueError(f'{type(self).__name__}: {len(sizes)} pyramid levels for {len(self.strides)} strides')

    def _scales_tensor(self):
        """the per-level Scale parameters as one (L,) fp32 device tensor, for the kernels (inference: cached)"""
        ps = [s.scale for s in self.scales]
        return self._scale_cache.get(ps, lambda: torch.stack([p.detach().float().reshape(()) for p in ps]).contiguous())

    def forward_rows(self, feats):
        """inference: list of (B,h,w,C) NHWC maps -> (A (rows, >= C+1 | C), R (rows, >= 4 | 5)) fp32 in every compute mode,
        level-major rows, zero padding columns, and the level sizes"""
        B = feats[0].shape[0]
        sizes = [tuple(int(v) for v in f.shape[1:3]) for f in feats]
        x0 = cat_rows(feats)
        outs = []
        for convs, caches, heads, hcache in zip((self.cls_convs, self.reg_convs), self._tower_caches, self._head_groups(),
                                                self._head_caches):
            outs.append(self._head_rows(self._tower_rows(x0, convs, caches, B, sizes), heads, hcache, B, sizes))
        return outs[0], outs[1], sizes

    @staticmethod
    def _tower_rows(x, convs, caches, B, sizes):
        """inference: conv + GroupNorm(+ ReLU) layers over the rows of all levels, one launch each per layer"""
        dtype = x.dtype
        for m, cache in zip(convs, caches):
            w = cache.get([m.conv.weight], lambda c=m: pack_weight(c.conv.weight).to(dtype))
            x, _ = ops.conv2d_nhwc_multi(x, w, B, sizes, None, None, None, False, 1, 1)
            x = ops.groupnorm_nhwc_multi(x, m.norm.weight.detach(), m.norm.bias.detach(), m.norm.num_groups, B, sizes,
                                         m.norm.eps, m.with_activation)
        return x

    @staticmethod
    def _head_rows(x, heads, hcache, B, sizes):
        """inference: the 3x3 convs `heads` as ONE conv with an fp32 result, output columns padded to a multiple of 8"""
        dtype = x.dtype

        def builder(hs=heads):
            w = torch.cat([pack_weight(h.weight) for h in hs], 0)
            b = torch.cat([h.bias.detach().float() for h in hs], 0)
            pad = -w.shape[0] % 8
            if pad:
                w = torch.cat([w, w.new_zeros((pad,) + tuple(w.shape[1:]))], 0)
                b = torch.cat([b, b.new_zeros(pad)], 0)
            return w.to(dtype).contiguous(), b.contiguous()
        w, b = hcache.get([t for h in heads for t in (h.weight, h.bias)], builder)
        return ops.conv2d_nhwc_multi(x, w, B, sizes, None, b, None, False, 1, 1, out_f32=True)[0]

    def forward_head_fused(self, feats):
        """training forward over all levels: (A, R) fp32 with zero padding columns, level-major rows, differentiable, and the
        level sizes"""
        B = feats[0].shape[0]
        sizes = tuple(tuple(int(v) for v in f.shape[1:3]) for f in feats)
        x0 = cat_rows(feats)
        outs = []
        for convs, heads in zip((self.cls_convs, self.reg_convs), self._head_groups()):
            outs.append(self._head_fused(self._tower_fused(x0, convs, B, sizes), heads, B, sizes))
        return outs[0], outs[1], sizes

    @staticmethod
    def _tower_fused(x, convs, B, sizes):
        """training: `_tower_rows` on the autograd forms of the same kernels"""
        from .autograd import GroupNormNHWCFunction, conv2d_nhwc_multi_autograd
        for m in convs:
            x = conv2d_nhwc_multi_autograd(x, m.conv.weight, None, B, sizes, 1, 1)
            x = GroupNormNHWCFunction.apply(x, m.norm.weight, m.norm.bias, m.norm.num_groups, B, sizes, m.norm.eps,
                                            m.with_activation)
        return x

    @staticmethod
    def _head_fused(x, heads, B, sizes):
        """training: `_head_rows`, differentiable (fp32 head output)"""
        from .autograd import ConvNHWCFunction, fused_head_weights
        w, b = fused_head_weights(heads, 32 if x.dtype == torch.float32 else 64)
        return ConvNHWCFunction.apply(x, w, b, B, sizes, 1, 1, False, False, True)

    def forward_nhwc(self, feats):
        """list of (B,h,w,C) NHWC maps -> the head's outputs as per-level (B,h,w,.) lists, fp32 (`_split_rows`)"""
        from .autograd import wants_grad
        if not feats[0].is_cuda:
            outs = self.forward([f.permute(0, 3, 1, 2) for f in feats])
            return tuple([t.permute(0, 2, 3, 1) for t in lst] for lst in outs)
        *rows, sizes = self._rows(list(feats), wants_grad(feats[0], self._cls_conv().weight, self.cls_convs[0].conv.weight))
        return self._split_rows(*rows, sizes, feats[0].shape[0])

    def _rows(self, feats, grad):
        """the row tensors `_split_rows` takes, and the level sizes: the training forward when a gradient is wanted"""
        return self.forward_head_fused(feats) if grad else self.forward_rows(feats)

    def forward(self, feats):
        """the reference signature: list of (N,C,h,w) -> the head's outputs as lists of (N,.,h,w).  CPU tensors take the
        host mirror on torch ops: the towers, then the head's `_heads_host(c, r, level)`"""
        if not feats[0].is_cuda:
            outs = [self._heads_host(*self._towers_host(x), l) for l, x in enumerate(feats)]
            return tuple(list(o) for o in zip(*outs))
        outs = self.forward_nhwc([to_nhwc(f) for f in feats])
        return tuple([t.permute(0, 3, 1, 2) for t in lst] for lst in outs)

    def _towers_host(self, x):
        """the host mirror of the two towers on torch ops: one (N,C,h,w) map -> (class tower, box tower) outputs"""
        import torch.nn.functional as F
        outs = []
        for convs in (self.cls_convs, self.reg_convs):
            y = x
            for m in convs:
                y = F.relu(F.group_norm(F.conv2d(y, m.conv.weight, None, padding=1), m.norm.num_groups, m.norm.weight,
                                        m.norm.bias, m.norm.eps))
            outs.append(y)
        return outs

    @staticmethod
    def _level_views(a, r, sizes, B):
        """the (A, R) rows of each level as (B, h, w, columns) views"""
        r0 = 0
        for (h, w) in sizes:
            n = B * h * w
            yield a[r0:r0 + n].view(B, h, w, a.shape[1]), r[r0:r0 + n].view(B, h, w, r.shape[1])
            r0 += n

    def get_bboxes_rows(self, a, r, layout, scales, sizes, img_metas, cfg=None, rescale=False):
        """fcos_head.py:329-471 / atss_head.py:372-504 for the whole batch on the device, no host sync: per-candidate max of
        class sigmoid x centerness sigmoid, per-level top-k, the head's decode (`_decode_candidates`) / clip / rescale with
        the fan-out to classes, score threshold on the class score, class-aware NMS, max_per_img.  Returns (dets (B, K, 5)
        zero padded, labels (B, K), num (B,) int32); `self.last_n_valid` as RetinaHead keeps it."""
        cfg = self.test_cfg if cfg is None else cfg
        self._check_test_cfg(cfg)
        self._check_limits(cfg, sizes)
        B = len(img_metas)
        scored, raw, r0 = self._score_rows(a, r, layout), [], 0
        for (h, w) in sizes:
            raw.append(scored[r0:r0 + B * h * w].view(B, h * w))
            r0 += B * h * w
        picked = ops.rpn_topk(raw, cfg.nms_pre)         # descending, ties by ascending index, all levels in one launch
        max_shape = const_rows([m['img_shape'][:2] for m in img_metas], scored)
        sf = const_rows([list(m['scale_factor']) for m in img_metas], scored) if rescale else None
        bb, sc, lb, va, nv = self._decode_candidates([p[1] for p in picked], a, r, layout, scales, sizes, max_shape, sf, cfg)
        self.last_n_valid = nv
        return self._nms_candidates(bb, sc, lb, va, self.cls_out_channels, cfg)

    def _score_rows(self, a, r, layout):
        """the per-row ranking score of the top-k: the centerness heads' max_c(class sigmoid x centerness sigmoid)"""
        return ops.fcos_score(a, r, layout)

    def simple_test_padded(self, feats_nhwc, img_metas, rescale=False):
        a, r, sizes = self.forward_rows(list(feats_nhwc))
        return self.get_bboxes_rows(a, r, self._layout(a, r), self._scales_tensor(), sizes, img_metas, rescale=rescale)

    def _get_bboxes_device(self, outs, img_metas, cfg, rescale):
        sizes = [tuple(int(v) for v in c.shape[-2:]) for c in outs[0]]
        a, r = self._rows_from_reference(*outs)
        return self.get_bboxes_rows(a, r, self._layout(a, r), a.new_ones(len(sizes)), sizes, img_metas, cfg, rescale)

    def forward_train_nhwc(self, feats_nhwc, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore=None):
        """the device-resident train step of the head: NHWC pyramid -> towers and fused heads over all levels -> the head's
        assignment and loss kernels; no host read"""
        self._refuse_ignore(gt_bboxes_ignore)
        a, r, sizes = self.forward_head_fused(list(feats_nhwc))
        scales = torch.stack([s.scale.float().reshape(()) for s in self.scales])
        return self.loss_fused(a, r, scales, sizes, gt_bboxes, gt_labels, img_metas)

    @staticmethod
    def _norm_hook():
        """`norm_hook` of the loss kernels' two normalisers: their mean over the ranks (the reference's two reduce_mean
        calls as one), None when not distributed"""
        if dist.is_available() and dist.is_initialized():
            return lambda n2: n2.copy_(reduce_mean(n2))
        return None


# ----------------------------------------------------------------------------- RetinaNet baseline
@HEADS.register_module()
class RetinaHead(DenseDetHead, AnchorHead):
    """The head of RetinaNet (mmdet/models/dense_heads/retina_head.py:8-114 over anchor_head.py:37-750): two towers of
    `stacked_convs` 3x3 conv + ReLU (`cls_convs.{i}.conv`, `reg_convs.{i}.conv`), then the 3x3 `retina_cls` (A * C sigmoid
    class logits per cell) and `retina_reg` (4A deltas).  Parameter names and shapes are the reference's.  Execution:
    every layer is one launch over all pyramid levels on the NHWC conv kernels (bias + ReLU in the read-out); scoring,
    top-k, decode + class fan-out and the NMS of the whole batch stay on the device (csrc/dense_head.hip), and so do
    the whole-batch assignment and the focal / L1 loss -- with no sampler there is nothing to draw on the host, and the
    train step reads nothing back inside the head.  CPU tensors take the reference's per-image chain on torch ops (the
    host mirror the CPU tests compare with the fixture)."""

    def __init__(self, num_classes, in_channels, stacked_convs=4, conv_cfg=None, norm_cfg=None,
                 anchor_generator=dict(type='AnchorGenerator', octave_base_scale=4, scales_per_octave=3,
                                       ratios=[0.5, 1.0, 2.0], strides=[8, 16, 32, 64, 128]),
                 init_cfg=None, **kwargs):
        if norm_cfg is not None:
            raise NotImplementedError(f'RetinaHead: norm_cfg={norm_cfg!r}; the towers run conv + bias + ReLU in one launch '
                                      'per layer, a normalisation layer between them is not supported')
        loss_cls = kwargs.get('loss_cls', dict(type='CrossEntropyLoss', use_sigmoid=True))
        loss_bbox = kwargs.get('loss_bbox', dict(type='SmoothL1Loss'))
        if not loss_cls.get('use_sigmoid', False):
            raise NotImplementedError('RetinaHead: loss_cls.use_sigmoid=False (softmax scores with a background column) is '
                                      'not supported; scoring and the focal loss are sigmoid')
        if loss_cls.get('type') != 'FocalLoss':
            raise NotImplementedError(f"RetinaHead: loss_cls.type={loss_cls.get('type')!r}; only FocalLoss is supported")
        if loss_bbox.get('type') not in ('L1Loss', 'SmoothL1Loss'):
            raise NotImplementedError(f"RetinaHead: loss_bbox.type={loss_bbox.get('type')!r}; only L1Loss and SmoothL1Loss "
                                      'on the encoded deltas are supported')
        if kwargs.get('reg_decoded_bbox', False):
            raise NotImplementedError('RetinaHead: reg_decoded_bbox=True (a loss on decoded boxes) is not supported')
        tc = kwargs.get('train_cfg')
        if tc and tc.get('sampler') is not None and tc.get('sampler').get('type') != 'PseudoSampler':
            raise NotImplementedError(f"RetinaHead: train_cfg.sampler.type={tc.get('sampler').get('type')!r}; the focal loss "
                                      'runs over every anchor (PseudoSampler)')
        self.stacked_convs, self.conv_cfg, self.norm_cfg = stacked_convs, conv_cfg, norm_cfg
        super().__init__(num_classes, in_channels, anchor_generator=anchor_generator, init_cfg=init_cfg, **kwargs)
        for loss in (self.loss_cls, self.loss_bbox):
            if loss.reduction != 'mean':
                raise NotImplementedError(f"RetinaHead: {type(loss).__name__}.reduction={loss.reduction!r}; only 'mean'")
        if getattr(self.bbox_coder, 'add_ctr_clamp', False) or not getattr(self.bbox_coder, 'clip_border', True):
            raise NotImplementedError('RetinaHead: bbox_coder needs clip_border=True and add_ctr_clamp=False')
        if self.test_cfg:
            self._check_test_cfg(self.test_cfg)
        self._cls_caches = [PackedCache() for _ in range(stacked_convs)]
        self._reg_caches = [PackedCache() for _ in range(stacked_convs)]
        self._head_caches = [PackedCache(), PackedCache()]
        self._base_anchor_cache = {}
        self.init_weights()

    def _init_layers(self):
        self.relu = nn.ReLU(inplace=True)
        self.cls_convs, self.reg_convs = nn.ModuleList(), nn.ModuleList()
        for i in range(self.stacked_convs):
            chn = self.in_channels if i == 0 else self.feat_channels
            self.cls_convs.append(ConvModule(chn, self.feat_channels, 3, stride=1, padding=1, conv_cfg=self.conv_cfg))
            self.reg_convs.append(ConvModule(chn, self.feat_channels, 3, stride=1, padding=1, conv_cfg=self.conv_cfg))
        self.retina_cls = nn.Conv2d(self.feat_channels, self.num_anchors * self.cls_out_channels, 3, padding=1)
        self.retina_reg = nn.Conv2d(self.feat_channels, self.num_anchors * 4, 3, padding=1)

    def init_weights(self):
        """init_cfg=dict(type='Normal', layer='Conv2d', std=0.01, override=dict(name='retina_cls', bias_prob=0.01))
        (retina_head.py:38-46)"""
        self._init_normal(self.retina_cls)

    # ------------------------------------------------------------------ forward
    def _towers(self):
        return ([m.conv for m in self.cls_convs], self._cls_caches), ([m.conv for m in self.reg_convs], self._reg_caches)

    def forward_rows(self, feats):
        """inference: list of (B,h,w,C) NHWC maps -> (cls (rows, A*C), reg (rows, 4A)) fp32 in every compute mode,
        level-major rows, and the level sizes; each layer of each tower is one launch over all levels (the weights are
        shared across them)"""
        B = feats[0].shape[0]
        sizes = [tuple(f.shape[1:3]) for f in feats]
        x0 = cat_rows(feats)
        outs = []
        for (convs, caches), head, hcache in zip(self._towers(), (self.retina_cls, self.retina_reg), self._head_caches):
            x = x0
            for conv, cache in zip(convs, caches):
                w, b = cache.get([conv.weight, conv.bias], lambda c=conv: (pack_weight(c.weight).to(x0.dtype),
                                                                          c.bias.detach().float().contiguous()))
                x, _ = ops.conv2d_nhwc_multi(x, w, B, sizes, None, b, None, True, 1, 1)      # bias + ReLU in the read-out
            w, b = hcache.get([head.weight, head.bias], lambda h=head: (pack_weight(h.weight).to(x0.dtype),
                                                                       h.bias.detach().float().contiguous()))
            outs.append(ops.conv2d_nhwc_multi(x, w, B, sizes, None, b, None, False, 1, 1, out_f32=True)[0])
        return outs[0], outs[1], sizes

    def forward_fused(self, feats):
        """`forward_rows` as per-level views: (cls (B,h,w,A*C), reg (B,h,w,4A)) lists"""
        yc, yr, sizes = self.forward_rows(feats)
        B = feats[0].shape[0]
        return self._split_rows(yc, B, sizes, yc.shape[1]), self._split_rows(yr, B, sizes, yr.shape[1])

    def forward_head_fused(self, feats):
        """training forward over all levels: (cls (rows, >= A*C), reg (rows, >= 4A)) fp32 with zero padding columns,
        level-major rows, differentiable, and the level sizes"""
        from .autograd import ConvNHWCFunction, conv2d_nhwc_multi_autograd, fused_head_weights
        B = feats[0].shape[0]
        sizes = tuple(tuple(int(v) for v in f.shape[1:3]) for f in feats)
        x0 = cat_rows(feats)
        mult = 32 if x0.dtype == torch.float32 else 64
        outs = []
        for (convs, _), head in zip(self._towers(), (self.retina_cls, self.retina_reg)):
            x = x0
            for conv in convs:
                if conv.out_channels % mult == 0:       # ReLU in the kernel's read-out
                    x = ConvNHWCFunction.apply(x, conv.weight, conv.bias, B, sizes, 1, 1, False, True, False)
                else:
                    x = conv2d_nhwc_multi_autograd(x, conv.weight, conv.bias, B, sizes, 1, 1).relu()
            w, b = fused_head_weights((head,), mult)
            outs.append(ConvNHWCFunction.apply(x, w, b, B, sizes, 1, 1, False, False, True))   # fp32 head output
        return outs[0], outs[1], sizes

    @staticmethod
    def _split_rows(y, B, sizes, width):
        lv, r0 = [], 0
        for (h, w) in sizes:
            n = B * h * w
            lv.append(y[r0:r0 + n].view(B, h, w, y.shape[1])[..., :width])
            r0 += n
        return lv

    def forward_nhwc(self, feats):
        """list of (B,h,w,C) -> (cls (B,h,w,A*C), reg (B,h,w,4A)) lists, fp32"""
        from .autograd import wants_grad
        if not feats[0].is_cuda:
            cls, reg = self.forward([f.permute(0, 3, 1, 2) for f in feats])
            return [c.permute(0, 2, 3, 1) for c in cls], [r.permute(0, 2, 3, 1) for r in reg]
        if wants_grad(feats[0], self.retina_cls.weight, self.cls_convs[0].conv.weight):
            yc, yr, sizes = self.forward_head_fused(list(feats))
            B = feats[0].shape[0]
            return (self._split_rows(yc, B, sizes, self.num_anchors * self.cls_out_channels),
                    self._split_rows(yr, B, sizes, self.num_anchors * 4))
        return self.forward_fused(list(feats))

    def forward(self, feats):
        """reference signature: list of (N,C,h,w) -> lists of (N,A*C,h,w), (N,4A,h,w)"""
        if not feats[0].is_cuda:        # host mirror: retina_head.py:94-114 on torch ops
            import torch.nn.functional as F
            cls, reg = [], []
            for x in feats:
                c = r = x
                for m in self.cls_convs:
                    c = F.relu(F.conv2d(c, m.conv.weight, m.conv.bias, padding=1))
                for m in self.reg_convs:
                    r = F.relu(F.conv2d(r, m.conv.weight, m.conv.bias, padding=1))
                cls.append(F.conv2d(c, self.retina_cls.weight, self.retina_cls.bias, padding=1))
                reg.append(F.conv2d(r, self.retina_reg.weight, self.retina_reg.bias, padding=1))
            return cls, reg
        cls, reg = self.forward_nhwc([to_nhwc(f) for f in feats])
        v = lambda lst: [t.permute(0, 3, 1, 2) for t in lst]  # noqa: E731
        return v(cls), v(reg)

    # ------------------------------------------------------------------ test
    def get_bboxes_padded(self, cls_nhwc, reg_nhwc, img_metas, cfg=None, rescale=False, cls_rows=None):
        """anchor_head.py:507-750 for the whole batch on the device, no host sync: per-anchor max sigmoid, per-level top-k,
        decode / clip / rescale with the fan-out to classes, score threshold, class-aware NMS, max_per_img.  Inputs are the
        NHWC head outputs per level (dense, or channel slices of wider tensors); `cls_rows`: the (rows, A*C) tensor the
        class maps are level-major views of (`forward_rows`), scored by ONE launch instead of one per level.  Returns
        (dets (B, K, 5) zero padded, labels (B, K), num (B,) int32); `self.last_n_valid` keeps, on the device, how many
        candidates of each image passed score_thr -- the count mmcv's split_thr decision looks at, a diagnostic here
        (SingleStageDetector.simple_test copies it out with the results)."""
        cfg = self.test_cfg if cfg is None else cfg
        self._check_test_cfg(cfg)
        sizes = [tuple(c.shape[1:3]) for c in cls_nhwc]
        self._check_limits(cfg, sizes)
        B, device = cls_nhwc[0].shape[0], cls_nhwc[0].device
        A, C = self.num_anchors, self.cls_out_channels
        L = len(cls_nhwc)
        if cls_rows is not None:
            assert cls_rows.dim() == 2 and cls_rows.shape[0] == sum(B * h * w for h, w in sizes)
            scored, raw, r0 = ops.dense_score(cls_rows, A, C), [], 0
            for (h, w) in sizes:
                raw.append(scored[r0:r0 + B * h * w].view(B, h * w * A))
                r0 += B * h * w
        else:
            raw = [ops.dense_score(c, A, C).view(B, -1) for c in cls_nhwc]
        picked = ops.rpn_topk(raw, cfg.nms_pre)         # descending, ties by ascending index, all levels in one launch
        max_shape = const_rows([m['img_shape'][:2] for m in img_metas], raw[0])
        sf = const_rows([list(m['scale_factor']) for m in img_metas], raw[0]) if rescale else None
        bb, sc, lb, va, nv = ops.dense_decode_levels(
            [p[1] for p in picked], list(cls_nhwc), list(reg_nhwc), [self._base_anchors(l, device) for l in range(L)], sizes,
            list(self.anchor_generator.strides), C, max_shape, sf, self.bbox_coder.means, self.bbox_coder.stds, cfg.score_thr)
        self.last_n_valid = nv
        return self._nms_candidates(bb, sc, lb, va, C, cfg)

    def simple_test_padded(self, feats_nhwc, img_metas, rescale=False):
        yc, yr, sizes = self.forward_rows(list(feats_nhwc))
        B = feats_nhwc[0].shape[0]
        return self.get_bboxes_padded(self._split_rows(yc, B, sizes, yc.shape[1]), self._split_rows(yr, B, sizes, yr.shape[1]),
                                      img_metas, rescale=rescale, cls_rows=yc)

    def get_bboxes(self, cls_scores, bbox_preds, img_metas, cfg=None, rescale=False, with_nms=True, batched_nms=None):
        """reference signature (anchor_head.py:507-587): per-level (N,A*C,h,w) / (N,4A,h,w) -> per image (dets (k,5),
        labels (k,)).  Device tensors take `get_bboxes_padded`; CPU tensors the reference's chain on torch ops, with the
        caller's `batched_nms` (this package's NMS is a device kernel)."""
        return self._get_bboxes((cls_scores, bbox_preds), img_metas, cfg, rescale, with_nms, batched_nms)

    def _get_bboxes_device(self, outs, img_metas, cfg, rescale):
        cls, reg = ([to_nhwc(t).float().contiguous() for t in o] for o in outs)
        return self.get_bboxes_padded(cls, reg, img_metas, cfg, rescale)

    def _get_bboxes_host(self, cls_scores, bbox_preds, img_metas, cfg, rescale, batched_nms):
        from .core import delta2bbox
        B, C = cls_scores[0].shape[0], self.cls_out_channels
        anchors_l = self.anchor_generator.grid_anchors([c.shape[-2:] for c in cls_scores], cls_scores[0].device)
        nms_pre = cfg.get('nms_pre', -1)
        out = []
        for b in range(B):
            boxes_l, scores_l = [], []
            for cls, reg, anchors in zip(cls_scores, bbox_preds, anchors_l):
                s = cls[b].detach().permute(1, 2, 0).reshape(-1, C).sigmoid()
                d = reg[b].detach().permute(1, 2, 0).reshape(-1, 4)
                if 0 < nms_pre < s.shape[0]:
                    _, idx = s.max(-1)[0].sort(descending=True, stable=True)      # ties by ascending index, the shared rule
                    idx = idx[:nms_pre]
                    anchors, d, s = anchors[idx], d[idx], s[idx]
                boxes_l.append(delta2bbox(anchors, d, self.bbox_coder.means, self.bbox_coder.stds,
                                          max_shape=tuple(img_metas[b]['img_shape'][:2])))
                scores_l.append(s)
            out.append(self._host_nms(torch.cat(boxes_l), torch.cat(scores_l), None, img_metas[b], cfg, rescale, batched_nms))
        return out

    # ------------------------------------------------------------------ train
    def forward_train_nhwc(self, feats_nhwc, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore=None):
        """the device-resident train step of the head: NHWC pyramid -> towers and heads over all levels -> whole-batch
        assignment and loss kernels; no host read"""
        self._refuse_ignore(gt_bboxes_ignore)
        yc, yr, sizes = self.forward_head_fused(list(feats_nhwc))
        return self.loss_fused(yc, yr, sizes, gt_bboxes, gt_labels, img_metas)

    def loss(self, cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        """anchor_head.py:423-497.  Device tensors go to the HIP kernels (`loss_fused`); CPU tensors take the reference's
        per-image chain in torch (the host mirror)."""
        featmap_sizes = [f.size()[-2:] for f in cls_scores]
        assert len(featmap_sizes) == self.anchor_generator.num_levels
        device = cls_scores[0].device
        if device.type == 'cuda':
            self._refuse_ignore(gt_bboxes_ignore)
            sizes = tuple(tuple(int(v) for v in s_) for s_ in featmap_sizes)
            rows = lambda lst: _nchw_rows(lst).contiguous()   # noqa: E731
            return self.loss_fused(rows(cls_scores), rows(bbox_preds), sizes, gt_bboxes, gt_labels, img_metas)
        num_imgs = len(img_metas)
        anchor_list, valid_flag_list = self.get_anchors(featmap_sizes, img_metas, device=device)
        num_level_anchors = [a.size(0) for a in anchor_list[0]]
        flat_anchors = [torch.cat(a) for a in anchor_list]
        flat_flags = [torch.cat(v) for v in valid_flag_list]
        ignore = gt_bboxes_ignore if gt_bboxes_ignore is not None else [None] * num_imgs
        all_valid = self._all_valid
        self._all_valid = None
        (labels, label_weights, bbox_targets, bbox_weights, pos_inds, neg_inds, _) = multi_apply(
            self._get_targets_single, flat_anchors, flat_flags, gt_bboxes, ignore, gt_labels, img_metas, all_valid)
        if any(l is None for l in labels):
            return None
        num_total_pos = sum(max(p.numel(), 1) for p in pos_inds)            # (no sampling: anchor_head.py:469-470)
        losses_cls, losses_bbox = multi_apply(
            self.loss_single, cls_scores, bbox_preds, images_to_levels(flat_anchors, num_level_anchors),
            images_to_levels(labels, num_level_anchors), images_to_levels(label_weights, num_level_anchors),
            images_to_levels(bbox_targets, num_level_anchors), images_to_levels(bbox_weights, num_level_anchors),
            num_total_samples=num_total_pos)
        return dict(loss_cls=losses_cls, loss_bbox=losses_bbox)

    # ------------------------------------------------------------------ device-resident train step
    def loss_fused(self, ycls, yreg, sizes, gt_bboxes, gt_labels, img_metas, gt_flat=None):
        """AnchorHead.loss on the head outputs of all levels (rows, >= A*C) / (rows, >= 4A): whole-batch assignment, then
        the loss kernels -- targets, the positive count and its reciprocal are formed on the device, nothing is read back.
        Returns the reference's per-level lists; `self.last_targets` keeps (gt_inds, [k_cls, k_bbox, num_total_pos])."""
        from . import train_ops
        from .core import MaxIoUAssigner
        if type(self.assigner) is not MaxIoUAssigner or self.assigner.ignore_iof_thr > 0:
            raise NotImplementedError('RetinaHead: the device path assigns with MaxIoUAssigner without ignore regions')
        device = ycls.device
        gts, labels, offs = gt_flat if gt_flat is not None else train_ops.flatten_gts(gt_bboxes, gt_labels)
        gt_inds = self.assign_targets_device(sizes, img_metas, gts, offs, device)
        L = len(sizes)
        meta = train_ops.DenseLossMeta(
            len(img_metas), sizes, self.anchor_generator.strides, [self._base_anchors(l, device) for l in range(L)],
            self.num_anchors, self.cls_out_channels, offs, self.loss_cls.gamma, self.loss_cls.alpha,
            self.train_cfg.pos_weight, getattr(self.loss_bbox, 'beta', 0.0), self.bbox_coder.means, self.bbox_coder.stds,
            self.loss_cls.loss_weight, self.loss_bbox.loss_weight)
        losses, coef = train_ops.dense_loss(ycls, yreg, gt_inds, gts, labels, meta)
        self.last_targets = (gt_inds, coef)
        return dict(loss_cls=list(losses[0].unbind(0)), loss_bbox=list(losses[1].unbind(0)))


INF = 1e8


def _clamped(box, h, w):
    """(n, 4) corner boxes clamped to an (h, w) image"""
    return torch.stack([box[:, 0].clamp(0, w), box[:, 1].clamp(0, h), box[:, 2].clamp(0, w), box[:, 3].clamp(0, h)], -1)


def distance2bbox(points, distance):
    """core/bbox/transforms.py:118-141 without the clip: (n, 2) points and (n, 4) [l, t, r, b] distances -> corner boxes"""
    return torch.stack([points[..., 0] - distance[..., 0], points[..., 1] - distance[..., 1],
                        points[..., 0] + distance[..., 2], points[..., 1] + distance[..., 3]], -1)


@HEADS.register_module()
class FCOSHead(GNTowerHead, nn.Module):
    """The head of FCOS (mmdet/models/dense_heads/fcos_head.py:18-649 over anchor_free_head.py:16-330): two towers of
    `stacked_convs` 3x3 conv + GroupNorm + ReLU (`cls_convs.{i}.{conv,gn}`, `reg_convs.{i}.{conv,gn}`), then the 3x3
    `conv_cls` (C sigmoid class logits per cell), `conv_reg` (4 distances) and `conv_centerness`, and one `Scale` per
    level (`scales.{l}.scale`).  No anchors: the candidates are the cell centres.  Parameter names and shapes are the
    reference's.  Execution: every tower layer is one conv launch plus one GroupNorm+ReLU launch over all pyramid levels;
    each tower ends in ONE fused fp32 head conv, the centerness riding with the tower it reads ([cls C | ctr 1 | pad] and
    [reg 4 | pad], or [cls C | pad] and [reg 4 | ctr 1 | pad] under `centerness_on_reg`).  The kernels of
    csrc/fcos_head.hip read these two tensors in place and apply the `Scale`, the exp / relu and the test-time `* stride`
    themselves: scoring, top-k, decode + class fan-out and the NMS of the whole batch, and in training the point
    assignment and the focal / centerness-weighted IoU / centerness loss, all on the device -- inference reads the host
    once (when the results leave), the head's train step never.  CPU tensors take the reference's chain on torch ops (the
    host mirror the CPU tests compare with the fixture)."""

    def __init__(self, num_classes, in_channels, feat_channels=256, stacked_convs=4, strides=(4, 8, 16, 32, 64),
                 regress_ranges=((-1, 64), (64, 128), (128, 256), (256, 512), (512, INF)), center_sampling=False,
                 center_sample_radius=1.5, norm_on_bbox=False, centerness_on_reg=False, dcn_on_last_conv=False,
                 conv_bias='auto',
                 loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
                 loss_bbox=dict(type='IoULoss', loss_weight=1.0),
                 loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
                 conv_cfg=None, norm_cfg=dict(type='GN', num_groups=32, requires_grad=True), train_cfg=None, test_cfg=None,
                 init_cfg=None):
        super().__init__()
        name = 'FCOSHead'
        if norm_cfg is None or norm_cfg.get('type') != 'GN':
            raise NotImplementedError(f'{name}: norm_cfg={norm_cfg!r}; the towers run conv + GroupNorm + ReLU, only GN is '
                                      'supported')
        if conv_bias != 'auto':
            raise NotImplementedError(f"{name}: conv_bias={conv_bias!r}; only 'auto' (no tower bias under GN) is supported")
        if dcn_on_last_conv:
            raise NotImplementedError(f'{name}: dcn_on_last_conv=True is not supported')
        if not loss_cls.get('use_sigmoid', False):
            raise NotImplementedError(f'{name}: loss_cls.use_sigmoid=False (softmax scores with a background column) is not '
                                      'supported; scoring and the focal loss are sigmoid')
        if loss_cls.get('type') != 'FocalLoss':
            raise NotImplementedError(f"{name}: loss_cls.type={loss_cls.get('type')!r}; only FocalLoss is supported")
        if loss_bbox.get('type') not in ('IoULoss', 'GIoULoss') or \
                (loss_bbox.get('type') == 'IoULoss' and (loss_bbox.get('linear', False) or loss_bbox.get('mode', 'log') != 'log')):
            raise NotImplementedError(f'{name}: loss_bbox={loss_bbox!r}; only IoULoss(mode=\'log\') and GIoULoss are supported')
        if loss_centerness.get('type') != 'CrossEntropyLoss' or not loss_centerness.get('use_sigmoid', False):
            raise NotImplementedError(f'{name}: loss_centerness={loss_centerness!r}; only the sigmoid CrossEntropyLoss is '
                                      'supported')
        if len(strides) != len(regress_ranges):
            raise ValueError(f'{name}: {len(strides)} strides but {len(regress_ranges)} regress_ranges')
        if len(strides) > self.MAX_LEVELS:
            raise ValueError(f'{name}: {len(strides)} pyramid levels, at most {self.MAX_LEVELS} are supported')
        if feat_channels > 256 or feat_channels % 4:
            raise NotImplementedError(f'{name}: feat_channels={feat_channels}; the GroupNorm kernels take up to 256 channels in '
                                      'whole quads')
        self.num_classes, self.cls_out_channels = num_classes, num_classes
        self.in_channels, self.feat_channels, self.stacked_convs = in_channels, feat_channels, stacked_convs
        self.strides = [int(s) if not isinstance(s, (tuple, list)) else int(s[0]) for s in strides]
        self.regress_ranges = tuple(tuple(r) for r in regress_ranges)
        self.center_sampling, self.center_sample_radius = center_sampling, center_sample_radius
        self.norm_on_bbox, self.centerness_on_reg = norm_on_bbox, centerness_on_reg
        self.conv_cfg, self.norm_cfg = conv_cfg, norm_cfg
        self.loss_cls, self.loss_bbox = build_loss(loss_cls), build_loss(loss_bbox)
        self.loss_centerness = build_loss(loss_centerness)
        for loss in (self.loss_cls, self.loss_bbox, self.loss_centerness):
            if loss.reduction != 'mean':
                raise NotImplementedError(f"{name}: {type(loss).__name__}.reduction={loss.reduction!r}; only 'mean'")
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        if self.test_cfg:
            self._check_test_cfg(self.test_cfg)
        self._init_layers()
        self.init_weights()

    def _init_layers(self):
        self._init_towers()
        self.conv_cls = nn.Conv2d(self.feat_channels, self.cls_out_channels, 3, padding=1)
        self.conv_reg = nn.Conv2d(self.feat_channels, 4, 3, padding=1)
        self.conv_centerness = nn.Conv2d(self.feat_channels, 1, 3, padding=1)
        self.scales = nn.ModuleList([Scale(1.0) for _ in self.strides])

    def init_weights(self):
        """init_cfg=dict(type='Normal', layer='Conv2d', std=0.01, override=dict(name='conv_cls', bias_prob=0.01))
        (fcos_head.py:80-88)"""
        self._init_normal(self.conv_cls)

    # ------------------------------------------------------------------ forward
    def _head_groups(self):
        """the heads each tower ends in, in the column order of its fused output"""
        if self.centerness_on_reg:
            return (self.conv_cls,), (self.conv_reg, self.conv_centerness)
        return (self.conv_cls, self.conv_centerness), (self.conv_reg,)

    def _layout(self, a, r):
        C = self.cls_out_channels
        return ops.FcosLayout(a, r, C, 0, 0, self.centerness_on_reg, 4 if self.centerness_on_reg else C,
                              self.norm_on_bbox, type(self.loss_bbox).__name__ == 'GIoULoss')

    def _cls_conv(self):
        return self.conv_cls

    def _split_rows(self, a, r, sizes, B):
        """(A, R) rows -> the reference's per-level NHWC (cls, bbox_pred AFTER scale / exp | relu [* stride], centerness)"""
        C, co = self.cls_out_channels, (4 if self.centerness_on_reg else self.cls_out_channels)
        cls, reg, ctr = [], [], []
        for l, (va, vr) in enumerate(self._level_views(a, r, sizes, B)):
            d = vr[..., :4] * self.scales[l].scale
            if self.norm_on_bbox:
                d = d.relu()
                d = d if self.training else d * self.strides[l]
            else:
                d = d.exp()
            cls.append(va[..., :C])
            reg.append(d)
            ctr.append((vr if self.centerness_on_reg else va)[..., co:co + 1])
        return cls, reg, ctr

    def _heads_host(self, c, r, l):
        """fcos_head.py:111-161 on the tower outputs of level l: (N,C,h,w) class logits, (N,4,h,w) distances after Scale and
        exp / relu, (N,1,h,w) centerness logits"""
        import torch.nn.functional as F
        cls = F.conv2d(c, self.conv_cls.weight, self.conv_cls.bias, padding=1)
        ctr = F.conv2d(r if self.centerness_on_reg else c, self.conv_centerness.weight, self.conv_centerness.bias, padding=1)
        d = (F.conv2d(r, self.conv_reg.weight, self.conv_reg.bias, padding=1) * self.scales[l].scale).float()
        if self.norm_on_bbox:
            d = F.relu(d)
            d = d if self.training else d * self.strides[l]
        else:
            d = d.exp()
        return cls, d, ctr

    # ------------------------------------------------------------------ test
    def get_points(self, featmap_sizes, dtype, device):
        """per level (h*w, 2) [x, y] cell centres: (x*s + s//2, y*s + s//2) (fcos_head.py:473-483)"""
        pts = []
        for (h, w), s in zip(featmap_sizes, self.strides):
            ys, xs = torch.meshgrid(torch.arange(h, dtype=dtype, device=device), torch.arange(w, dtype=dtype, device=device),
                                    indexing='ij')
            pts.append(torch.stack((xs.reshape(-1) * s, ys.reshape(-1) * s), dim=-1) + s // 2)
        return pts

    def _decode_candidates(self, picked, a, r, layout, scales, sizes, max_shape, sf, cfg):
        return ops.fcos_decode_levels(picked, a, r, layout, scales, sizes, self.strides, max_shape, sf, cfg.score_thr)

    def _rows_from_reference(self, cls_scores, bbox_preds, centernesses, training=False):
        """the reference-signature tensors (decoded distances) as the kernels' (A, R) rows with unit scales: the raw value
        is log(d), or under norm_on_bbox d itself (test time: d / stride, exact for power-of-two strides; a distance
        the relu left at exactly 0 takes no gradient, as through the relu)"""
        if self.norm_on_bbox:
            raw = bbox_preds if training else [d / s for d, s in zip(bbox_preds, self.strides)]
        else:
            raw = [d.log() for d in bbox_preds]
        cls, reg, ctr = _nchw_rows(cls_scores), _nchw_rows(raw), _nchw_rows(centernesses)
        if self.centerness_on_reg:
            return cls.contiguous(), torch.cat([reg, ctr], 1).contiguous()
        return torch.cat([cls, ctr], 1).contiguous(), reg.contiguous()

    def get_bboxes(self, cls_scores, bbox_preds, centernesses, img_metas, cfg=None, rescale=False, with_nms=True,
                   batched_nms=None):
        """reference signature (fcos_head.py:263-327): per-level (N,C,h,w) / (N,4,h,w) / (N,1,h,w) -> per image (dets (k,5),
        labels (k,)).  Device tensors take `get_bboxes_rows`; CPU tensors the reference's chain on torch ops, with the
        caller's `batched_nms` (this package's NMS is a device kernel)."""
        return self._get_bboxes((cls_scores, bbox_preds, centernesses), img_metas, cfg, rescale, with_nms, batched_nms)

    def _priors_host(self, sizes, outs):
        return self.get_points(sizes, outs[1][0].dtype, outs[1][0].device)

    @staticmethod
    def _level_host(l, reg, ctr):
        return reg.reshape(-1, 4), ctr.reshape(-1).sigmoid()

    @staticmethod
    def _decode_host(pts, d, img_hw):
        bx = torch.stack([pts[:, 0] - d[:, 0], pts[:, 1] - d[:, 1], pts[:, 0] + d[:, 2], pts[:, 1] + d[:, 3]], -1)
        hi = bx.new_tensor([img_hw[1], img_hw[0], img_hw[1], img_hw[0]])
        bx = torch.where(bx < 0, bx.new_zeros(()), bx)
        return torch.where(bx > hi, hi, bx)

    # ------------------------------------------------------------------ train
    def loss_fused(self, a, r, scales, sizes, gt_bboxes, gt_labels, img_metas, gt_flat=None):
        """FCOSHead.loss on the fused head outputs of all levels: whole-batch point assignment, then the loss kernels --
        targets and both normalisers are formed on the device (averaged over ranks there when distributed), nothing is
        read back.  `self.last_targets` keeps (gt_inds, coef3, norm2)."""
        from . import train_ops
        gts, labels, offs = gt_flat if gt_flat is not None else train_ops.flatten_gts(gt_bboxes, gt_labels)
        gts, labels = gts.to(a.device), labels.to(a.device)
        B = len(img_metas)
        gt_inds = train_ops.fcos_assign(gts, offs, B, sizes, self.strides, self.regress_ranges, self.center_sampling,
                                        self.center_sample_radius)
        giou = type(self.loss_bbox).__name__ == 'GIoULoss'
        meta = train_ops.FcosLossMeta(B, sizes, self.strides, self.cls_out_channels, offs, self.loss_cls.gamma,
                                      self.loss_cls.alpha, self.loss_bbox.eps if giou else 1e-6, self.loss_bbox.eps,
                                      self.loss_cls.loss_weight, self.loss_bbox.loss_weight, self.loss_centerness.loss_weight)
        losses, coef, norm2 = train_ops.fcos_loss(a, r, scales, gt_inds, gts, labels, self._layout(a, r), meta,
                                                  self._norm_hook())
        self.last_targets = (gt_inds, coef, norm2)
        return dict(loss_cls=losses[0], loss_bbox=losses[1], loss_centerness=losses[2])

    def get_targets(self, points, gt_bboxes_list, gt_labels_list):
        """fcos_head.py:485-628 on torch ops (the host mirror): per level, images concatenated, (labels, bbox_targets)"""
        num_points = [p.size(0) for p in points]
        ranges = torch.cat([p.new_tensor(rr)[None].expand_as(p) for p, rr in zip(points, self.regress_ranges)], 0)
        pts = torch.cat(points, 0)
        radius = torch.cat([p.new_full((p.size(0),), s * self.center_sample_radius) for p, s in zip(points, self.strides)])
        labels_list, targets_list = [], []
        for gt, gl in zip(gt_bboxes_list, gt_labels_list):
            n, G = pts.size(0), gl.size(0)
            if G == 0:
                labels_list.append(gl.new_full((n,), self.num_classes))
                targets_list.append(gt.new_zeros((n, 4)))
                continue
            areas = ((gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]))[None].repeat(n, 1)
            g = gt[None].expand(n, G, 4)
            xs, ys = pts[:, 0:1].expand(n, G), pts[:, 1:2].expand(n, G)
            t = torch.stack((xs - g[..., 0], ys - g[..., 1], g[..., 2] - xs, g[..., 3] - ys), -1)
            if self.center_sampling:
                cx, cy = (g[..., 0] + g[..., 2]) / 2, (g[..., 1] + g[..., 3]) / 2
                rad = radius[:, None].expand(n, G)
                x0, y0, x1, y1 = cx - rad, cy - rad, cx + rad, cy + rad
                c0 = torch.where(x0 > g[..., 0], x0, g[..., 0])
                c1 = torch.where(y0 > g[..., 1], y0, g[..., 1])
                c2 = torch.where(x1 > g[..., 2], g[..., 2], x1)
                c3 = torch.where(y1 > g[..., 3], g[..., 3], y1)
                inside = torch.stack((xs - c0, ys - c1, c2 - xs, c3 - ys), -1).min(-1)[0] > 0
            else:
                inside = t.min(-1)[0] > 0
            far = t.max(-1)[0]
            in_range = (far >= ranges[:, None, 0]) & (far <= ranges[:, None, 1])
            areas[inside == 0] = INF
            areas[in_range == 0] = INF
            min_area, idx = areas.min(dim=1)
            lab = gl[idx]
            lab[min_area == INF] = self.num_classes
            labels_list.append(lab)
            targets_list.append(t[range(n), idx])
        labels_list = [l.split(num_points, 0) for l in labels_list]
        targets_list = [t.split(num_points, 0) for t in targets_list]
        out_l, out_t = [], []
        for i in range(len(points)):
            out_l.append(torch.cat([l[i] for l in labels_list]))
            t = torch.cat([t[i] for t in targets_list])
            out_t.append(t / self.strides[i] if self.norm_on_bbox else t)
        return out_l, out_t

    @staticmethod
    def centerness_target(pos_bbox_targets):
        """fcos_head.py:630-649"""
        lr, tb = pos_bbox_targets[:, [0, 2]], pos_bbox_targets[:, [1, 3]]
        if len(lr) == 0:
            return torch.sqrt(lr[..., 0])
        return torch.sqrt((lr.min(dim=-1)[0] / lr.max(dim=-1)[0]) * (tb.min(dim=-1)[0] / tb.max(dim=-1)[0]))

    def loss(self, cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        """fcos_head.py:164-261.  Device tensors go to the HIP kernels (`loss_fused`, with unit scales on log(d) resp. d);
        CPU tensors take the reference's chain in torch (the host mirror)."""
        assert len(cls_scores) == len(bbox_preds) == len(centernesses)
        featmap_sizes = [tuple(int(v) for v in f.size()[-2:]) for f in cls_scores]
        device = cls_scores[0].device
        if device.type == 'cuda':
            self._refuse_ignore(gt_bboxes_ignore)
            a, r = self._rows_from_reference(cls_scores, bbox_preds, centernesses, True)
            return self.loss_fused(a, r, a.new_ones(len(featmap_sizes)), featmap_sizes, gt_bboxes, gt_labels, img_metas)
        points = self.get_points(featmap_sizes, bbox_preds[0].dtype, device)
        labels, bbox_targets = self.get_targets(points, gt_bboxes, gt_labels)
        num_imgs = cls_scores[0].size(0)
        flat = lambda lst, c: torch.cat([t.permute(0, 2, 3, 1).reshape(-1, c) for t in lst])    # noqa: E731
        f_cls, f_box = flat(cls_scores, self.cls_out_channels), flat(bbox_preds, 4)
        f_ctr = flat(centernesses, 1).reshape(-1)
        f_labels, f_targets = torch.cat(labels), torch.cat(bbox_targets)
        f_points = torch.cat([p.repeat(num_imgs, 1) for p in points])
        pos_inds = ((f_labels >= 0) & (f_labels < self.num_classes)).nonzero().reshape(-1)
        num_pos = max(reduce_mean(torch.tensor(len(pos_inds), dtype=torch.float, device=device)), 1.0)
        loss_cls = self.loss_cls(f_cls, f_labels, avg_factor=num_pos)
        pos_box, pos_ctr, pos_t = f_box[pos_inds], f_ctr[pos_inds], f_targets[pos_inds]
        ctr_t = self.centerness_target(pos_t)
        denorm = max(reduce_mean(ctr_t.sum().detach()), 1e-6)
        if len(pos_inds) > 0:
            pos_pts = f_points[pos_inds]
            loss_bbox = self.loss_bbox(distance2bbox(pos_pts, pos_box), distance2bbox(pos_pts, pos_t), weight=ctr_t,
                                       avg_factor=denorm)
            loss_centerness = self.loss_centerness(pos_ctr, ctr_t, avg_factor=num_pos)
        else:
            loss_bbox, loss_centerness = pos_box.sum(), pos_ctr.sum()
        return dict(loss_cls=loss_cls, loss_bbox=loss_bbox, loss_centerness=loss_centerness)


@HEADS.register_module()
class ATSSHead(GNTowerHead, AnchorHead):
    """The head of ATSS (mmdet/models/dense_heads/atss_head.py:14-686 over anchor_head.py): FCOSHead's two GN towers
    (`cls_convs.{i}.{conv,gn}`, `reg_convs.{i}.{conv,gn}`), then the 3x3 `atss_cls` (C sigmoid class logits), `atss_reg` (4
    deltas of the cell's ONE anchor, through the level's `scales.{l}.scale`) and `atss_centerness` on the box tower.
    Parameter names and shapes are the reference's.  Execution is FCOSHead's with its `centerness_on_reg` grouping -- the
    tower and fused-head code is GNTowerHead's, the base of both heads: A = [cls C | pad], R = [reg 4 | ctr 1 | pad], fp32,
    raw -- and the kernels of csrc/atss_head.hip apply the Scale themselves: scoring (`brcnn_fcos_score`), top-k, anchor decode + class
    fan-out and the NMS of the whole batch; in training the adaptive assignment (`brcnn_atss_assign`: k nearest anchors
    per level, mean + std IoU threshold, centre-inside test, best-IoU resolution) and the focal / centerness-weighted GIoU
    / centerness loss with the targets formed in the kernel.  Inference reads the host once, the head's train step never.
    CPU tensors take the reference's chain on torch ops (the host mirror the CPU tests compare with the fixture)."""

    def __init__(self, num_classes, in_channels, stacked_convs=4, conv_cfg=None,
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True),
                 loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0), init_cfg=None, **kwargs):
        name = 'ATSSHead'
        if norm_cfg is None or norm_cfg.get('type') != 'GN':
            raise NotImplementedError(f'{name}: norm_cfg={norm_cfg!r}; the towers run conv + GroupNorm + ReLU, only GN is '
                                      'supported')
        loss_cls = kwargs.get('loss_cls', dict(type='CrossEntropyLoss', use_sigmoid=True))
        loss_bbox = kwargs.get('loss_bbox', dict(type='SmoothL1Loss'))
        if not loss_cls.get('use_sigmoid', False):
            raise NotImplementedError(f'{name}: loss_cls.use_sigmoid=False (softmax scores with a background column) is not '
                                      'supported; scoring and the focal loss are sigmoid')
        if loss_cls.get('type') != 'FocalLoss':
            raise NotImplementedError(f"{name}: loss_cls.type={loss_cls.get('type')!r}; only FocalLoss is supported")
        if loss_bbox.get('type') != 'GIoULoss':
            raise NotImplementedError(f'{name}: loss_bbox={loss_bbox!r}; only GIoULoss on the decoded boxes is supported')
        if loss_centerness.get('type') != 'CrossEntropyLoss' or not loss_centerness.get('use_sigmoid', False):
            raise NotImplementedError(f'{name}: loss_centerness={loss_centerness!r}; only the sigmoid CrossEntropyLoss is '
                                      'supported')
        if kwargs.get('reg_decoded_bbox', False):
            raise NotImplementedError(f'{name}: reg_decoded_bbox=True is not supported (the head decodes its deltas itself)')
        self._check_atss_train_cfg(name, kwargs.get('train_cfg'), kwargs.get('feat_channels', 256))
        self.stacked_convs, self.conv_cfg, self.norm_cfg = stacked_convs, conv_cfg, norm_cfg
        super().__init__(num_classes, in_channels, init_cfg=init_cfg, **kwargs)
        self._check_one_square_anchor(name)
        self.sampling = False
        self.loss_centerness = build_loss(loss_centerness)
        for loss in (self.loss_cls, self.loss_bbox, self.loss_centerness):
            if loss.reduction != 'mean':
                raise NotImplementedError(f"{name}: {type(loss).__name__}.reduction={loss.reduction!r}; only 'mean'")
        if getattr(self.bbox_coder, 'add_ctr_clamp', False) or not getattr(self.bbox_coder, 'clip_border', True):
            raise NotImplementedError(f'{name}: bbox_coder needs clip_border=True and add_ctr_clamp=False')
        if self.test_cfg:
            self._check_test_cfg(self.test_cfg)
        self.strides = [int(s[0]) for s in self.anchor_generator.strides]
        self.init_weights()

    def _init_layers(self):
        self._init_towers()
        self.atss_cls = nn.Conv2d(self.feat_channels, self.num_anchors * self.cls_out_channels, 3, padding=1)
        self.atss_reg = nn.Conv2d(self.feat_channels, self.num_anchors * 4, 3, padding=1)
        self.atss_centerness = nn.Conv2d(self.feat_channels, self.num_anchors * 1, 3, padding=1)
        self.scales = nn.ModuleList([Scale(1.0) for _ in self.anchor_generator.strides])

    def init_weights(self):
        """init_cfg=dict(type='Normal', layer='Conv2d', std=0.01, override=dict(name='atss_cls', bias_prob=0.01))
        (atss_head.py:35-43)"""
        self._init_normal(self.atss_cls)

    # ------------------------------------------------------------------ forward
    def _head_groups(self):
        """FCOSHead's `centerness_on_reg` grouping: the centerness rides on the box tower's fused head conv"""
        return (self.atss_cls,), (self.atss_reg, self.atss_centerness)

    def _layout(self, a, r):
        return ops.FcosLayout(a, r, self.cls_out_channels, 0, 0, True, 4, False, True)

    def _cls_conv(self):
        return self.atss_cls

    def _split_rows(self, a, r, sizes, B):
        """(A, R) rows -> the reference's per-level NHWC (cls, bbox_pred AFTER the Scale, centerness)"""
        C = self.cls_out_channels
        cls, reg, ctr = [], [], []
        for l, (va, vr) in enumerate(self._level_views(a, r, sizes, B)):
            cls.append(va[..., :C])
            reg.append(vr[..., :4] * self.scales[l].scale)
            ctr.append(vr[..., 4:5])
        return cls, reg, ctr

    def _heads_host(self, c, r, l):
        """atss_head.py:96-141 on the tower outputs of level l: (N,C,h,w) class logits, (N,4,h,w) deltas after the Scale,
        (N,1,h,w) centerness logits"""
        import torch.nn.functional as F
        return (F.conv2d(c, self.atss_cls.weight, self.atss_cls.bias, padding=1),
                (F.conv2d(r, self.atss_reg.weight, self.atss_reg.bias, padding=1) * self.scales[l].scale).float(),
                F.conv2d(r, self.atss_centerness.weight, self.atss_centerness.bias, padding=1))

    # ------------------------------------------------------------------ test
    def _decode_candidates(self, picked, a, r, layout, scales, sizes, max_shape, sf, cfg):
        return ops.atss_decode_levels(picked, a, r, layout, scales, sizes, self.strides, self._base_table(), max_shape, sf,
                                      self.bbox_coder.means, self.bbox_coder.stds, cfg.score_thr)

    @staticmethod
    def _rows_from_reference(cls_scores, bbox_preds, centernesses):
        """the reference-signature tensors (deltas after the Scale) as the kernels' (A, R) rows, to be read with unit scales"""
        return (_nchw_rows(cls_scores).contiguous(),
                torch.cat([_nchw_rows(bbox_preds), _nchw_rows(centernesses)], 1).contiguous())

    def get_bboxes(self, cls_scores, bbox_preds, centernesses, img_metas, cfg=None, rescale=False, with_nms=True,
                   batched_nms=None):
        """reference signature (atss_head.py:312-370): per-level (N,C,h,w) / (N,4,h,w) / (N,1,h,w) -> per image (dets (k,5),
        labels (k,)).  Device tensors take `get_bboxes_rows`; CPU tensors the reference's chain on torch ops, with the
        caller's `batched_nms` (this package's NMS is a device kernel)."""
        return self._get_bboxes((cls_scores, bbox_preds, centernesses), img_metas, cfg, rescale, with_nms, batched_nms)

    def _priors_host(self, sizes, outs):
        return self.anchor_generator.grid_anchors(sizes, outs[0][0].device)

    @staticmethod
    def _level_host(l, reg, ctr):
        return reg.reshape(-1, 4), ctr.reshape(-1).sigmoid()

    def _decode_host(self, anchors, d, img_hw):
        from .core import delta2bbox
        return delta2bbox(anchors, d, self.bbox_coder.means, self.bbox_coder.stds, max_shape=tuple(img_hw))

    # ------------------------------------------------------------------ train
    def loss_fused(self, a, r, scales, sizes, gt_bboxes, gt_labels, img_metas, gt_flat=None):
        """ATSSHead.loss on the fused head outputs of all levels: whole-batch adaptive assignment, then the loss kernels --
        targets and both normalisers are formed on the device (averaged over ranks there when distributed), nothing is
        read back.  Returns the reference's per-level lists; `self.last_targets` keeps (gt_inds, coef3, norm2)."""
        from . import train_ops
        gts, labels, offs, sizes, base, gt_inds = self._assign_atss_device(a, sizes, gt_bboxes, gt_labels, img_metas, gt_flat)
        B = len(img_metas)
        meta = train_ops.AtssLossMeta(B, sizes, self.strides, base, self.cls_out_channels, offs, self.loss_cls.gamma,
                                      self.loss_cls.alpha, self.loss_bbox.eps, self.loss_cls.loss_weight,
                                      self.loss_bbox.loss_weight, self.loss_centerness.loss_weight, self.bbox_coder.means,
                                      self.bbox_coder.stds)
        losses, coef, norm2 = train_ops.atss_loss(a, r, scales, gt_inds, gts, labels, self._layout(a, r), meta,
                                                  self._norm_hook())
        self.last_targets = (gt_inds, coef, norm2)
        return dict(loss_cls=list(losses[0].unbind(0)), loss_bbox=list(losses[1].unbind(0)),
                    loss_centerness=list(losses[2].unbind(0)))

    def get_targets(self, anchor_list, valid_flag_list, gt_bboxes_list, img_metas, gt_bboxes_ignore_list=None,
                    gt_labels_list=None, label_channels=1, unmap_outputs=True):
        """atss_head.py:506-568 on torch ops (the host mirror): (anchors, labels, label weights, box targets, box weights) per
        level with the images stacked, and the two sample counts; the box targets are the encoded deltas"""
        return self._atss_targets(anchor_list, valid_flag_list, gt_bboxes_list, img_metas, gt_bboxes_ignore_list,
                                  gt_labels_list, label_channels, unmap_outputs, encode=True)

    def centerness_target(self, anchors, bbox_targets):
        """atss_head.py:294-310: from the anchor centre to the box the encoded target decodes to"""
        gts = self.bbox_coder.decode(anchors, bbox_targets)
        cx, cy = (anchors[:, 2] + anchors[:, 0]) / 2, (anchors[:, 3] + anchors[:, 1]) / 2
        lr = torch.stack([cx - gts[:, 0], gts[:, 2] - cx], dim=1)
        tb = torch.stack([cy - gts[:, 1], gts[:, 3] - cy], dim=1)
        return torch.sqrt((lr.min(dim=-1)[0] / lr.max(dim=-1)[0]) * (tb.min(dim=-1)[0] / tb.max(dim=-1)[0]))

    def loss_single(self, anchors, cls_score, bbox_pred, centerness, labels, label_weights, bbox_targets, num_total_samples):
        """atss_head.py:143-216"""
        anchors = anchors.reshape(-1, 4)
        cls_score = cls_score.permute(0, 2, 3, 1).reshape(-1, self.cls_out_channels).contiguous()
        bbox_pred = bbox_pred.permute(0, 2, 3, 1).reshape(-1, 4)
        centerness = centerness.permute(0, 2, 3, 1).reshape(-1)
        bbox_targets, labels, label_weights = bbox_targets.reshape(-1, 4), labels.reshape(-1), label_weights.reshape(-1)
        loss_cls = self.loss_cls(cls_score, labels, label_weights, avg_factor=num_total_samples)
        pos_inds = ((labels >= 0) & (labels < self.num_classes)).nonzero().squeeze(1)
        if len(pos_inds) > 0:
            pos_anchors, pos_targets = anchors[pos_inds], bbox_targets[pos_inds]
            ctr_t = self.centerness_target(pos_anchors, pos_targets)
            loss_bbox = self.loss_bbox(self.bbox_coder.decode(pos_anchors, bbox_pred[pos_inds]),
                                       self.bbox_coder.decode(pos_anchors, pos_targets), weight=ctr_t, avg_factor=1.0)
            loss_centerness = self.loss_centerness(centerness[pos_inds], ctr_t, avg_factor=num_total_samples)
        else:
            loss_bbox, loss_centerness = bbox_pred.sum() * 0, centerness.sum() * 0
            ctr_t = bbox_targets.new_tensor(0.)
        return loss_cls, loss_bbox, loss_centerness, ctr_t.sum()

    def loss(self, cls_scores, bbox_preds, centernesses, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        """atss_head.py:218-292.  Device tensors go to the HIP kernels (`loss_fused`, with unit scales on the scaled deltas);
        CPU tensors take the reference's chain in torch (the host mirror)."""
        assert len(cls_scores) == len(bbox_preds) == len(centernesses)
        featmap_sizes = [tuple(int(v) for v in f.size()[-2:]) for f in cls_scores]
        assert len(featmap_sizes) == self.anchor_generator.num_levels
        device = cls_scores[0].device
        if device.type == 'cuda':
            self._refuse_ignore(gt_bboxes_ignore)
            a, r = self._rows_from_reference(cls_scores, bbox_preds, centernesses)
            return self.loss_fused(a, r, a.new_ones(len(featmap_sizes)), featmap_sizes, gt_bboxes, gt_labels, img_metas)
        anchor_list, valid_flag_list = self.get_anchors(featmap_sizes, img_metas, device=device)
        self._all_valid = None
        targets = self.get_targets(anchor_list, valid_flag_list, gt_bboxes, img_metas, gt_bboxes_ignore, gt_labels,
                                   label_channels=self.cls_out_channels)
        if targets is None:
            return None
        anchors, labels, label_weights, bbox_targets, _, num_total_pos, _ = targets
        num_total_samples = max(reduce_mean(torch.tensor(num_total_pos, dtype=torch.float, device=device)).item(), 1.0)
        losses_cls, losses_bbox, losses_ctr, factors = multi_apply(
            self.loss_single, anchors, cls_scores, bbox_preds, centernesses, labels, label_weights, bbox_targets,
            num_total_samples=num_total_samples)
        avg = reduce_mean(sum(factors)).clamp_(min=1).item()
        return dict(loss_cls=losses_cls, loss_bbox=[x / avg for x in losses_bbox], loss_centerness=losses_ctr)


# ----------------------------------------------------------------------------- GFL baseline
class Integral(nn.Module):
    """gfl_head.py:16-49: the expectation sum P(y_i) * y_i over the discrete set {0 .. reg_max} of each box side's softmax
    distribution; `project` is the reference's buffer (checkpoints carry it)"""

    def __init__(self, reg_max=16):
        super().__init__()
        self.reg_max = reg_max
        self.register_buffer('project', torch.linspace(0, self.reg_max, self.reg_max + 1))

    def forward(self, x):
        """(..., 4 * (reg_max + 1)) logits -> (N, 4) distances"""
        import torch.nn.functional as F
        x = F.softmax(x.reshape(-1, self.reg_max + 1), dim=1)
        return F.linear(x, self.project.type_as(x)).reshape(-1, 4)


def bbox2distance(points, bbox, max_dis=None, eps=0.1):
    """core/bbox/transforms.py: (n, 2) points and (n, 4) corner boxes -> (n, 4) [l, t, r, b] distances, clamped to
    [0, max_dis - eps]"""
    d = torch.stack([points[:, 0] - bbox[:, 0], points[:, 1] - bbox[:, 1], bbox[:, 2] - points[:, 0],
                     bbox[:, 3] - points[:, 1]], -1)
    return d if max_dis is None else d.clamp(min=0, max=max_dis - eps)


@HEADS.register_module()
class GFLHead(GNTowerHead, AnchorHead):
    """The head of GFL (mmdet/models/dense_heads/gfl_head.py:52-649 over anchor_head.py): ATSSHead's two GN towers
    (`cls_convs.{i}.{conv,gn}`, `reg_convs.{i}.{conv,gn}`), then the 3x3 `gfl_cls` (C joint class / quality logits) and
    `gfl_reg` (4 * (reg_max + 1) logits: per box side a distribution over the distances 0 .. reg_max strides, through the
    level's `scales.{l}.scale`), and the `integral.project` buffer.  Parameter names and shapes are the reference's.  The
    towers, the fused head convs and the test-time chain are GNTowerHead's: A = [cls C | pad], R = [4 * (reg_max + 1) logits |
    pad], fp32, raw -- the kernels of csrc/gfl_head.hip apply the Scale to the logits themselves.  Test time ranks by the
    class sigmoid alone (`brcnn_dense_score` on A in place), decodes the softmax expectations from the anchor centres with
    the class fan-out (`brcnn_gfl_decode_levels`) and runs the NMS of the whole batch; training uses ATSS's adaptive
    assignment (`brcnn_atss_assign`) and `brcnn_gfl_loss_*`: Quality Focal Loss against the IoU of the predicted box, GIoU
    and Distribution Focal Loss weighted by the anchor's best class score, targets and both normalisers formed in the
    kernels.  Inference reads the host once, the head's train step never.  CPU tensors take the reference's chain on torch
    ops (the host mirror the CPU tests compare with the fixture)."""

    MAX_REG = 16         # brcnn_gfl_*

    def __init__(self, num_classes, in_channels, stacked_convs=4, conv_cfg=None,
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True),
                 loss_dfl=dict(type='DistributionFocalLoss', loss_weight=0.25), reg_max=16, init_cfg=None, **kwargs):
        name = 'GFLHead'
        if norm_cfg is None or norm_cfg.get('type') != 'GN':
            raise NotImplementedError(f'{name}: norm_cfg={norm_cfg!r}; the towers run conv + GroupNorm + ReLU, only GN is '
                                      'supported')
        loss_cls = kwargs.get('loss_cls', dict(type='CrossEntropyLoss', use_sigmoid=True))
        loss_bbox = kwargs.get('loss_bbox', dict(type='SmoothL1Loss'))
        if loss_cls.get('type') != 'QualityFocalLoss' or not loss_cls.get('use_sigmoid', True):
            raise NotImplementedError(f'{name}: loss_cls={loss_cls!r}; only the sigmoid QualityFocalLoss is supported')
        if loss_cls.get('beta', 2.0) < 1:
            raise NotImplementedError(f"{name}: loss_cls.beta={loss_cls.get('beta')} < 1: the derivative of |quality - "
                                      'sigmoid|^beta is unbounded where the two meet')
        if loss_bbox.get('type') != 'GIoULoss':
            raise NotImplementedError(f'{name}: loss_bbox={loss_bbox!r}; only GIoULoss on the decoded boxes is supported')
        if loss_dfl.get('type') != 'DistributionFocalLoss':
            raise NotImplementedError(f'{name}: loss_dfl={loss_dfl!r}; only DistributionFocalLoss is supported')
        if not (isinstance(reg_max, int) and 1 <= reg_max <= self.MAX_REG):
            raise ValueError(f'{name}: reg_max={reg_max} outside [1, {self.MAX_REG}]')
        self._check_atss_train_cfg(name, kwargs.get('train_cfg'), kwargs.get('feat_channels', 256))
        self.stacked_convs, self.conv_cfg, self.norm_cfg, self.reg_max = stacked_convs, conv_cfg, norm_cfg, reg_max
        super().__init__(num_classes, in_channels, init_cfg=init_cfg, **kwargs)
        self._check_one_square_anchor(name)
        self.sampling = False
        self.integral = Integral(self.reg_max)
        self.loss_dfl = build_loss(loss_dfl)
        for loss in (self.loss_cls, self.loss_bbox, self.loss_dfl):
            if loss.reduction != 'mean':
                raise NotImplementedError(f"{name}: {type(loss).__name__}.reduction={loss.reduction!r}; only 'mean'")
        if self.test_cfg:
            self._check_test_cfg(self.test_cfg)
        self.strides = [int(s[0]) for s in self.anchor_generator.strides]
        self.init_weights()

    def _init_layers(self):
        self._init_towers()
        self.gfl_cls = nn.Conv2d(self.feat_channels, self.cls_out_channels, 3, padding=1)
        self.gfl_reg = nn.Conv2d(self.feat_channels, 4 * (self.reg_max + 1), 3, padding=1)
        self.scales = nn.ModuleList([Scale(1.0) for _ in self.anchor_generator.strides])

    def init_weights(self):
        """init_cfg=dict(type='Normal', layer='Conv2d', std=0.01, override=dict(name='gfl_cls', bias_prob=0.01))
        (gfl_head.py:94-102)"""
        self._init_normal(self.gfl_cls)

    # ------------------------------------------------------------------ forward
    def _head_groups(self):
        return (self.gfl_cls,), (self.gfl_reg,)

    def _layout(self, a, r):
        return ops.GflLayout(a, r, self.cls_out_channels, self.reg_max)

    def _score_rows(self, a, r, layout):
        """GFL has no centerness: the top-k ranks by max_c sigmoid(cls_c)"""
        return ops.gfl_score(a, layout)

    def _cls_conv(self):
        return self.gfl_cls

    def _split_rows(self, a, r, sizes, B):
        """(A, R) rows -> the reference's per-level NHWC (cls, bbox_pred (B,h,w,4 * (reg_max + 1)) AFTER the Scale)"""
        C, W = self.cls_out_channels, 4 * (self.reg_max + 1)
        cls, reg = [], []
        for l, (va, vr) in enumerate(self._level_views(a, r, sizes, B)):
            cls.append(va[..., :C])
            reg.append(vr[..., :W] * self.scales[l].scale)
        return cls, reg

    def _heads_host(self, c, r, l):
        """gfl_head.py:154-196 on the tower outputs of level l: (N,C,h,w) class logits and (N,4 * (reg_max + 1),h,w) box
        logits after the Scale"""
        import torch.nn.functional as F
        return (F.conv2d(c, self.gfl_cls.weight, self.gfl_cls.bias, padding=1),
                (F.conv2d(r, self.gfl_reg.weight, self.gfl_reg.bias, padding=1) * self.scales[l].scale).float())

    @staticmethod
    def anchor_center(anchors):
        """gfl_head.py:198-209"""
        return torch.stack([(anchors[..., 2] + anchors[..., 0]) / 2, (anchors[..., 3] + anchors[..., 1]) / 2], dim=-1)

    # ------------------------------------------------------------------ test
    def _decode_candidates(self, picked, a, r, layout, scales, sizes, max_shape, sf, cfg):
        return ops.gfl_decode_levels(picked, a, r, layout, scales, sizes, self.strides, self._base_table(), max_shape, sf,
                                     cfg.score_thr)

    @staticmethod
    def _rows_from_reference(cls_scores, bbox_preds):
        """the reference-signature tensors (box logits after the Scale) as the kernels' (A, R) rows, to be read with unit
        scales"""
        return _nchw_rows(cls_scores).contiguous(), _nchw_rows(bbox_preds).contiguous()

    def get_bboxes(self, cls_scores, bbox_preds, img_metas, cfg=None, rescale=False, with_nms=True, batched_nms=None):
        """reference signature (base_dense_head / gfl_head.py:373-472): per-level (N,C,h,w) / (N,4 * (reg_max + 1),h,w) ->
        per image (dets (k,5), labels (k,)).  Device tensors take `get_bboxes_rows`; CPU tensors the reference's chain on
        torch ops, with the caller's `batched_nms` (this package's NMS is a device kernel)."""
        return self._get_bboxes((cls_scores, bbox_preds), img_metas, cfg, rescale, with_nms, batched_nms)

    def _priors_host(self, sizes, outs):
        return self.anchor_generator.grid_anchors(sizes, outs[0][0].device)

    def _level_host(self, l, reg):
        return self.integral(reg) * self.strides[l], None

    def _decode_host(self, anchors, d, img_hw):
        return _clamped(distance2bbox(self.anchor_center(anchors), d), *img_hw)

    # ------------------------------------------------------------------ train
    def loss_fused(self, a, r, scales, sizes, gt_bboxes, gt_labels, img_metas, gt_flat=None):
        """GFLHead.loss on the fused head outputs of all levels: ATSS's whole-batch adaptive assignment, then the loss
        kernels -- targets, qualities, weights and both normalisers are formed on the device (averaged over ranks there
        when distributed), nothing is read back.  Returns the reference's per-level lists; `self.last_targets` keeps
        (gt_inds, coef3, norm2)."""
        from . import train_ops
        gts, labels, offs, sizes, base, gt_inds = self._assign_atss_device(a, sizes, gt_bboxes, gt_labels, img_metas, gt_flat)
        B = len(img_metas)
        meta = train_ops.GflLossMeta(B, sizes, self.strides, base, self.reg_max, self.cls_out_channels, offs,
                                     self.loss_cls.beta, self.loss_bbox.eps, self.loss_cls.loss_weight,
                                     self.loss_bbox.loss_weight, self.loss_dfl.loss_weight)
        losses, coef, norm2 = train_ops.gfl_loss(a, r, scales, gt_inds, gts, labels, self._layout(a, r), meta,
                                                 self._norm_hook())
        self.last_targets = (gt_inds, coef, norm2)
        return dict(loss_cls=list(losses[0].unbind(0)), loss_bbox=list(losses[1].unbind(0)),
                    loss_dfl=list(losses[2].unbind(0)))

    def get_targets(self, anchor_list, valid_flag_list, gt_bboxes_list, img_metas, gt_bboxes_ignore_list=None,
                    gt_labels_list=None, label_channels=1, unmap_outputs=True):
        """gfl_head.py:474-536 on torch ops (the host mirror): ATSSHead's targets with the ground-truth boxes themselves
        as the box targets"""
        return self._atss_targets(anchor_list, valid_flag_list, gt_bboxes_list, img_metas, gt_bboxes_ignore_list,
                                  gt_labels_list, label_channels, unmap_outputs, encode=False)

    def loss_single(self, anchors, cls_score, bbox_pred, labels, label_weights, bbox_targets, stride, num_total_samples):
        """gfl_head.py:211-297, everything in units of the stride"""
        anchors = anchors.reshape(-1, 4)
        cls_score = cls_score.permute(0, 2, 3, 1).reshape(-1, self.cls_out_channels)
        bbox_pred = bbox_pred.permute(0, 2, 3, 1).reshape(-1, 4 * (self.reg_max + 1))
        bbox_targets, labels, label_weights = bbox_targets.reshape(-1, 4), labels.reshape(-1), label_weights.reshape(-1)
        pos_inds = ((labels >= 0) & (labels < self.num_classes)).nonzero().squeeze(1)
        score = label_weights.new_zeros(labels.shape)
        if len(pos_inds) > 0:
            centers = self.anchor_center(anchors[pos_inds]) / stride
            weight = cls_score.detach().sigmoid().max(dim=1)[0][pos_inds]
            pos_pred = bbox_pred[pos_inds]
            decoded = distance2bbox(centers, self.integral(pos_pred))
            target = bbox_targets[pos_inds] / stride
            score[pos_inds] = bbox_overlaps(decoded.detach(), target, is_aligned=True)
            loss_bbox = self.loss_bbox(decoded, target, weight=weight, avg_factor=1.0)
            loss_dfl = self.loss_dfl(pos_pred.reshape(-1, self.reg_max + 1),
                                     bbox2distance(centers, target, self.reg_max).reshape(-1),
                                     weight=weight[:, None].expand(-1, 4).reshape(-1), avg_factor=4.0)
        else:
            loss_bbox, loss_dfl = bbox_pred.sum() * 0, bbox_pred.sum() * 0
            weight = bbox_pred.new_tensor(0)
        loss_cls = self.loss_cls(cls_score, (labels, score), weight=label_weights, avg_factor=num_total_samples)
        return loss_cls, loss_bbox, loss_dfl, weight.sum()

    def loss(self, cls_scores, bbox_preds, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        """gfl_head.py:299-371.  Device tensors go to the HIP kernels (`loss_fused`, with unit scales on the scaled logits);
        CPU tensors take the reference's chain in torch (the host mirror)."""
        assert len(cls_scores) == len(bbox_preds)
        featmap_sizes = [tuple(int(v) for v in f.size()[-2:]) for f in cls_scores]
        assert len(featmap_sizes) == self.anchor_generator.num_levels
        device = cls_scores[0].device
        if device.type == 'cuda':
            self._refuse_ignore(gt_bboxes_ignore)
            a, r = self._rows_from_reference(cls_scores, bbox_preds)
            return self.loss_fused(a, r, a.new_ones(len(featmap_sizes)), featmap_sizes, gt_bboxes, gt_labels, img_metas)
        anchor_list, valid_flag_list = self.get_anchors(featmap_sizes, img_metas, device=device)
        self._all_valid = None
        targets = self.get_targets(anchor_list, valid_flag_list, gt_bboxes, img_metas, gt_bboxes_ignore, gt_labels,
                                   label_channels=self.cls_out_channels)
        if targets is None:
            return None
        anchors, labels, label_weights, bbox_targets, _, num_total_pos, _ = targets
        num_total_samples = max(reduce_mean(torch.tensor(num_total_pos, dtype=torch.float, device=device)).item(), 1.0)
        losses_cls, losses_bbox, losses_dfl, factors = multi_apply(
            self.loss_single, anchors, cls_scores, bbox_preds, labels, label_weights, bbox_targets, self.strides,
            num_total_samples=num_total_samples)
        avg = reduce_mean(sum(factors)).clamp_(min=1).item()
        return dict(loss_cls=losses_cls, loss_bbox=[x / avg for x in losses_bbox], loss_dfl=[x / avg for x in losses_dfl])


# ----------------------------------------------------------------------------- VFNet baseline
class DeformConv2d(nn.Module):
    """mmcv.ops.DeformConv2d as VFNetHead uses it: 3x3, stride 1, padding 1, one deform group, no bias -- the only parameter
    is `weight`; the offsets are an input"""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels, 3, 3))
        nn.init.kaiming_uniform_(self.weight, nonlinearity='relu')


def deform_conv2d_host(x, offset, weight):
    """the host mirror of the DCN v1 deformable 3x3 conv (stride 1, padding 1, one group) on torch ops, differentiable
    w.r.t. x, offset and weight: x (N, C, H, W), offset (N, 18, H, W) with [2t] = dy, [2t + 1] = dx of tap t, weight (O, C,
    3, 3).  A sample point outside (-1, H) x (-1, W) is zero, a corner outside the map contributes zero (mmcv's rule)"""
    N, C, H, W = x.shape
    ys = torch.arange(H, dtype=x.dtype, device=x.device).view(1, H, 1)
    xs = torch.arange(W, dtype=x.dtype, device=x.device).view(1, 1, W)
    flat = x.reshape(N, C, H * W)
    cols = []
    for t in range(9):
        hy = ys + (t // 3 - 1) + offset[:, 2 * t]
        wx = xs + (t % 3 - 1) + offset[:, 2 * t + 1]
        inside = (hy > -1) & (wx > -1) & (hy < H) & (wx < W)
        h0, w0 = hy.detach().floor(), wx.detach().floor()
        lh, lw = hy - h0, wx - w0
        val = 0
        for hh, ww, wt in ((h0, w0, (1 - lh) * (1 - lw)), (h0, w0 + 1, (1 - lh) * lw), (h0 + 1, w0, lh * (1 - lw)),
                           (h0 + 1, w0 + 1, lh * lw)):
            ok = inside & (hh >= 0) & (hh <= H - 1) & (ww >= 0) & (ww <= W - 1)
            idx = (hh.clamp(0, H - 1) * W + ww.clamp(0, W - 1)).long().view(N, 1, H * W).expand(N, C, H * W)
            val = val + torch.gather(flat, 2, idx).view(N, C, H, W) * torch.where(ok, wt, torch.zeros_like(wt)).unsqueeze(1)
        cols.append(val)
    col = torch.stack(cols, 2)                                                      # (N, C, 9, H, W)
    return torch.einsum('nckhw,ock->nohw', col, weight.reshape(weight.shape[0], C, 9))


@HEADS.register_module()
class VFNetHead(GNTowerHead, AnchorHead):
    """The head of VarifocalNet (mmdet/models/dense_heads/vfnet_head.py:19-792): two GN towers (`cls_convs.{i}.{conv,gn}`,
    `reg_convs.{i}.{conv,gn}`); `vfnet_reg_conv` + `vfnet_reg` give a first box per point, D0 = exp(scales.{l}.scale * raw) *
    reg_denom_l (l, t, r, b) in pixels; the star-shaped deformable convs `vfnet_reg_refine_dconv` (on the box tower's output)
    and `vfnet_cls_dconv` (on the class tower's) sample nine points of that box; `vfnet_reg_refine` gives the refinement
    factor, D1 = exp(scales_refine.{l}.scale * raw1) * D0 with D0 a constant, and `vfnet_cls` the IoU-aware class logits.
    Parameter names and shapes are the reference's.  The towers and the fused fp32 head convs are GNTowerHead's, one launch
    per layer over all levels; `brcnn_vfnet_star_offsets` forms D0 and the 18 offsets of every cell in one launch; the two
    deformable convs run per level on the DCN v1 kernels (fp32: im2col + GEMM, 16-bit: the fused kernel where it takes the
    shape), ReLU in the read-out.  Test time ranks by the class sigmoid (`brcnn_dense_score` on A in place), decodes D1 of the
    picked rows from their points with the class fan-out (`brcnn_vfnet_decode_levels`) and runs the NMS of the whole batch;
    training uses ATSS's adaptive assignment (`brcnn_atss_assign`) and `brcnn_vfnet_loss_*`: Varifocal Loss over every (cell,
    class) -- cells beyond an image's pad_shape count as background, the reference passes no weight --, GIoU on both boxes
    weighted by their own IoU, targets, weights and the three normalisers formed in the kernels.  Inference reads the host
    once, the head's train step never (the reference: three `.item()` calls).  CPU tensors take the reference's chain on
    torch ops (the host mirror the CPU tests compare with the fixture)."""

    INF = 1e8

    def __init__(self, num_classes, in_channels, stacked_convs=4, strides=(4, 8, 16, 32, 64), conv_cfg=None,
                 regress_ranges=((-1, 64), (64, 128), (128, 256), (256, 512), (512, INF)), center_sampling=False,
                 center_sample_radius=1.5, sync_num_pos=True, gradient_mul=0.1, bbox_norm_type='reg_denom',
                 loss_cls_fl=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0), use_vfl=True,
                 loss_cls=dict(type='VarifocalLoss', use_sigmoid=True, alpha=0.75, gamma=2.0, iou_weighted=True,
                               loss_weight=1.0),
                 loss_bbox=dict(type='GIoULoss', loss_weight=1.5), loss_bbox_refine=dict(type='GIoULoss', loss_weight=2.0),
                 norm_cfg=dict(type='GN', num_groups=32, requires_grad=True), use_atss=True, dcn_on_last_conv=False,
                 anchor_generator=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                                       center_offset=0.0, strides=[8, 16, 32, 64, 128]),
                 init_cfg=None, **kwargs):
        name = 'VFNetHead'
        if not use_atss:
            raise NotImplementedError(f'{name}: use_atss=False (FCOS targets) is not supported')
        if not use_vfl:
            raise NotImplementedError(f'{name}: use_vfl=False (focal loss) is not supported')
        if dcn_on_last_conv:
            raise NotImplementedError(f'{name}: dcn_on_last_conv=True is not supported')
        if not sync_num_pos:
            raise NotImplementedError(f'{name}: sync_num_pos=False is not supported: the number of positives is averaged over '
                                      'the ranks and clamped to 1 with the two other normalisers, on the device')
        if norm_cfg is None or norm_cfg.get('type') != 'GN':
            raise NotImplementedError(f'{name}: norm_cfg={norm_cfg!r}; the towers run conv + GroupNorm + ReLU, only GN is '
                                      'supported')
        if loss_cls.get('type') != 'VarifocalLoss' or not loss_cls.get('use_sigmoid', True):
            raise NotImplementedError(f'{name}: loss_cls={loss_cls!r}; only the sigmoid VarifocalLoss is supported')
        if loss_cls.get('gamma', 2.0) < 1:
            raise NotImplementedError(f"{name}: loss_cls.gamma={loss_cls.get('gamma')} < 1: the derivative of sigmoid^gamma "
                                      'is unbounded at 0')
        for key, lb in (('loss_bbox', loss_bbox), ('loss_bbox_refine', loss_bbox_refine)):
            if lb.get('type') != 'GIoULoss':
                raise NotImplementedError(f'{name}: {key}={lb!r}; only GIoULoss on the decoded boxes is supported')
        if bbox_norm_type not in ('reg_denom', 'stride'):
            raise NotImplementedError(f"{name}: bbox_norm_type={bbox_norm_type!r}; 'reg_denom' or 'stride'")
        self._check_atss_train_cfg(name, kwargs.get('train_cfg'), kwargs.get('feat_channels', 256))
        self.stacked_convs, self.conv_cfg, self.norm_cfg = stacked_convs, conv_cfg, norm_cfg
        self.strides = [int(s) for s in strides]
        self.regress_ranges = regress_ranges
        self.reg_denoms = [r[-1] for r in regress_ranges]
        self.reg_denoms[-1] = self.reg_denoms[-2] * 2
        self.center_sampling, self.center_sample_radius, self.sync_num_pos = center_sampling, center_sample_radius, sync_num_pos
        self.gradient_mul, self.bbox_norm_type, self.use_vfl, self.use_atss = gradient_mul, bbox_norm_type, use_vfl, use_atss
        self.dcn_on_last_conv = dcn_on_last_conv
        self.anchor_center_offset = anchor_generator.get('center_offset', 0.5)
        super().__init__(num_classes, in_channels, anchor_generator=anchor_generator, loss_cls=loss_cls, loss_bbox=loss_bbox,
                         init_cfg=init_cfg, **kwargs)
        self._check_one_square_anchor(name)
        if [int(s[0]) for s in self.anchor_generator.strides] != self.strides or len(self.reg_denoms) != len(self.strides):
            raise ValueError(f'{name}: strides={self.strides}, anchor_generator.strides={self.anchor_generator.strides} and '
                             f'{len(self.reg_denoms)} regress_ranges must describe the same levels')
        self.sampling = False
        self.loss_bbox_refine = build_loss(loss_bbox_refine)
        for loss in (self.loss_cls, self.loss_bbox, self.loss_bbox_refine):
            if loss.reduction != 'mean':
                raise NotImplementedError(f"{name}: {type(loss).__name__}.reduction={loss.reduction!r}; only 'mean'")
        if self.test_cfg:
            self._check_test_cfg(self.test_cfg)
        self.init_weights()

    def _init_layers(self):
        self._init_towers()
        C = self.feat_channels
        self.relu = nn.ReLU(inplace=True)
        self.vfnet_reg_conv = ConvModule(C, C, 3, stride=1, padding=1, conv_cfg=self.conv_cfg, norm_cfg=self.norm_cfg,
                                         bias='auto')
        self.vfnet_reg = nn.Conv2d(C, 4, 3, padding=1)
        self.scales = nn.ModuleList([Scale(1.0) for _ in self.strides])
        self.vfnet_reg_refine_dconv = DeformConv2d(C, C)
        self.vfnet_reg_refine = nn.Conv2d(C, 4, 3, padding=1)
        self.scales_refine = nn.ModuleList([Scale(1.0) for _ in self.strides])
        self.vfnet_cls_dconv = DeformConv2d(C, C)
        self.vfnet_cls = nn.Conv2d(C, self.cls_out_channels, 3, padding=1)
        self._vf_caches = {k: PackedCache() for k in ('reg_conv', 'reg', 'refine', 'cls', 'refine_dconv', 'cls_dconv',
                                                      'scales_refine')}

    def init_weights(self):
        """init_cfg=dict(type='Normal', layer='Conv2d', std=0.01, override=dict(name='vfnet_cls', bias_prob=0.01))
        (vfnet_head.py:101-109); the two DeformConv2d are no Conv2d and keep their own initialisation"""
        self._init_normal(self.vfnet_cls)

    # ------------------------------------------------------------------ forward
    def _denoms(self):
        return [float(d) for d in (self.reg_denoms if self.bbox_norm_type == 'reg_denom' else self.strides)]

    def _scales_refine_tensor(self):
        ps = [s.scale for s in self.scales_refine]
        return self._vf_caches['scales_refine'].get(
            ps, lambda: torch.stack([p.detach().float().reshape(()) for p in ps]).contiguous())

    def _check_dcn_channels(self, x):
        mult = 4 if x.dtype == torch.float32 else 8
        if self.feat_channels % mult:
            raise NotImplementedError(f'VFNetHead: feat_channels={self.feat_channels}; the deformable conv kernels take '
                                      f'channels in multiples of {mult} in {x.dtype}')

    def _star_dconv_rows(self, x, off, m, cache, B, sizes):
        """inference: relu(star deformable conv) of the rows of all levels, level by level (DCN v1 kernels)"""
        C = self.feat_channels
        w = cache.get([m.weight], lambda: pack_weight(m.weight).to(x.dtype).contiguous())
        sixteen = x.dtype != torch.float32
        out, r = torch.empty_like(x), 0
        for h, wd in sizes:
            n = B * h * wd
            xl, ol = x[r:r + n].view(B, h, wd, C), off[r:r + n].view(B, h, wd, 18)
            if sixteen and ops.deform_conv_route(xl, C, 1, 1, 1):
                out[r:r + n] = ops.deform_conv_nhwc(xl, ol, w, None, None, True, 1, 1, 1, False).view(n, C)
            else:
                col, _ = ops.deform_im2col_nhwc(xl, ol, 3, 1, 1, 1, None, 1, False)
                out[r:r + n] = ops.linear_nhwc(col, w.view(C, 9 * C), None, True)
            r += n
        return out

    def _star_dconv_fused(self, x, offs, m, B, sizes):
        """training: `_star_dconv_rows` through the autograd forms of the same kernels, the input gradient accumulated in
        integers (`ordered`: a train step carries the same bits from run to run); `offs`: per level (B, h, w, 18)"""
        from .autograd import deform_conv_autograd, deform_im2col_autograd, linear_autograd
        C = self.feat_channels
        outs = []
        for xl, ol, (h, wd) in zip(torch.split(x, [B * h * wd for h, wd in sizes], 0), offs, sizes):
            xl = xl.view(B, h, wd, C)
            if x.dtype != torch.float32:
                outs.append(deform_conv_autograd(xl, ol, m.weight, 1, 1, 1, False, True, True, True).reshape(B * h * wd, C))
            else:
                col = deform_im2col_autograd(xl, ol, 1, 1, 1, False, True)
                outs.append(linear_autograd(col, m.weight.permute(0, 2, 3, 1).reshape(C, 9 * C), None, relu=True))
        return torch.cat(outs, 0)

    def forward_rows(self, feats):
        """inference: list of (B,h,w,C) NHWC maps -> (A (rows, >= C) class logits, R1 (rows, >= 4) raw refinement logits, D0
        (rows, 4) first distances), fp32 in every compute mode, level-major rows, and the level sizes"""
        B = feats[0].shape[0]
        sizes = [tuple(int(v) for v in f.shape[1:3]) for f in feats]
        x0 = cat_rows(feats)
        self._check_dcn_channels(x0)
        c = self._vf_caches
        xc = self._tower_rows(x0, self.cls_convs, self._tower_caches[0], B, sizes)
        xr = self._tower_rows(x0, self.reg_convs, self._tower_caches[1], B, sizes)
        xi = self._tower_rows(xr, [self.vfnet_reg_conv], [c['reg_conv']], B, sizes)
        r0 = self._head_rows(xi, (self.vfnet_reg,), c['reg'], B, sizes)
        d0, off = ops.vfnet_star_offsets(r0, self._scales_tensor(), B, sizes, self.strides, self._denoms(), self.gradient_mul)
        r1 = self._head_rows(self._star_dconv_rows(xr, off, self.vfnet_reg_refine_dconv, c['refine_dconv'], B, sizes),
                             (self.vfnet_reg_refine,), c['refine'], B, sizes)
        a = self._head_rows(self._star_dconv_rows(xc, off, self.vfnet_cls_dconv, c['cls_dconv'], B, sizes),
                            (self.vfnet_cls,), c['cls'], B, sizes)
        return a, r1, d0, sizes

    def forward_head_fused(self, feats):
        """training forward over all levels, differentiable: (A, D0, D1, sizes); A fp32 with zero padding columns, D0 / D1
        (rows, 4) distances in pixels"""
        from . import train_ops
        B = feats[0].shape[0]
        sizes = tuple(tuple(int(v) for v in f.shape[1:3]) for f in feats)
        x0 = cat_rows(feats)
        self._check_dcn_channels(x0)
        xc = self._tower_fused(x0, self.cls_convs, B, sizes)
        xr = self._tower_fused(x0, self.reg_convs, B, sizes)
        r0 = self._head_fused(self._tower_fused(xr, [self.vfnet_reg_conv], B, sizes), (self.vfnet_reg,), B, sizes)
        scales = torch.stack([s.scale.float().reshape(()) for s in self.scales])
        d0, offs = train_ops.vfnet_star_offsets(r0, scales, B, sizes, self.strides, self._denoms(), self.gradient_mul)
        r1 = self._head_fused(self._star_dconv_fused(xr, offs, self.vfnet_reg_refine_dconv, B, sizes),
                              (self.vfnet_reg_refine,), B, sizes)
        a = self._head_fused(self._star_dconv_fused(xc, offs, self.vfnet_cls_dconv, B, sizes), (self.vfnet_cls,), B, sizes)
        scales_refine = torch.stack([s.scale.float().reshape(()) for s in self.scales_refine])
        d1 = train_ops.vfnet_refine(r1, scales_refine, d0, B, sizes)
        return a, d0, d1, sizes

    def _cls_conv(self):
        return self.vfnet_cls

    def _rows(self, feats, grad):
        """(A, D0, D1, sizes): the inference rows end in the refinement kernel"""
        if grad:
            return self.forward_head_fused(feats)
        a, r1, d0, sizes = self.forward_rows(feats)
        return a, d0, ops.vfnet_refine(r1, self._scales_refine_tensor(), feats[0].shape[0], sizes, d0), sizes

    def _split_rows(self, a, d0, d1, sizes, B):
        """(A, D0, D1) rows -> the reference's per-level NHWC (cls (B,h,w,C), bbox_pred (B,h,w,4), bbox_pred_refine)"""
        cls, reg, ref, r = [], [], [], 0
        for h, w in sizes:
            n = B * h * w
            cls.append(a[r:r + n].view(B, h, w, -1)[..., :self.cls_out_channels])
            reg.append(d0[r:r + n].view(B, h, w, 4))
            ref.append(d1[r:r + n].view(B, h, w, 4))
            r += n
        return cls, reg, ref

    def star_dcn_offset(self, bbox_pred, gradient_mul, stride):
        """vfnet_head.py:274-313 on torch ops (the host mirror): (N, 4, H, W) distances -> (N, 18, H, W) offsets"""
        g = ((1 - gradient_mul) * bbox_pred.detach() + gradient_mul * bbox_pred) / stride
        x1, y1, x2, y2 = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
        z = torch.zeros_like(x1)
        ent = [-1.0 * y1, -1.0 * x1, -1.0 * y1, z, -1.0 * y1, x2, z, -1.0 * x1, z, z, z, x2, y2, -1.0 * x1, y2, z, y2, x2]
        base = [float(v) for t in range(9) for v in (t // 3 - 1, t % 3 - 1)]
        return torch.stack(ent, 1) - bbox_pred.new_tensor(base).view(1, 18, 1, 1)

    def _heads_host(self, c, r, l):
        """vfnet_head.py:194-272 on the tower outputs of level l: (N,C,h,w) class logits, (N,4,h,w) distances and (N,4,h,w)
        refined distances"""
        import torch.nn.functional as F
        m = self.vfnet_reg_conv
        ri = F.relu(F.group_norm(F.conv2d(r, m.conv.weight, None, padding=1), m.norm.num_groups, m.norm.weight, m.norm.bias,
                                 m.norm.eps))
        d0 = (F.conv2d(ri, self.vfnet_reg.weight, self.vfnet_reg.bias, padding=1) *
              self.scales[l].scale).float().exp() * self._denoms()[l]
        off = self.star_dcn_offset(d0, self.gradient_mul, self.strides[l]).to(r.dtype)
        r2 = F.relu(deform_conv2d_host(r, off, self.vfnet_reg_refine_dconv.weight))
        d1 = (F.conv2d(r2, self.vfnet_reg_refine.weight, self.vfnet_reg_refine.bias, padding=1) *
              self.scales_refine[l].scale).float().exp() * d0.detach()
        c2 = F.relu(deform_conv2d_host(c, off, self.vfnet_cls_dconv.weight))
        return F.conv2d(c2, self.vfnet_cls.weight, self.vfnet_cls.bias, padding=1), d0, d1

    def get_points(self, featmap_sizes, dtype, device):
        """vfnet_head.py:597-618 with use_atss: (x * s, y * s) + s * center_offset, the centres of the anchors"""
        pts = []
        for (h, w), s in zip(featmap_sizes, self.strides):
            y, x = torch.meshgrid(torch.arange(0, h * s, s, dtype=dtype, device=device),
                                  torch.arange(0, w * s, s, dtype=dtype, device=device), indexing='ij')
            pts.append(torch.stack((x.reshape(-1), y.reshape(-1)), dim=-1) + s * self.anchor_center_offset)
        return pts

    # ------------------------------------------------------------------ test
    def _score_rows(self, a, r, layout):
        return ops.vfnet_score(a, layout)

    def _layout(self, a, r, d0=None):
        lay = ops.VfnetLayout(a, r, self.cls_out_channels)
        lay.d0 = d0
        return lay

    def _decode_candidates(self, picked, a, r, layout, scales, sizes, max_shape, sf, cfg):
        return ops.vfnet_decode_levels(picked, a, r, layout.d0, layout, scales, sizes, self.strides, self._base_table(),
                                       max_shape, sf, cfg.score_thr)

    def simple_test_padded(self, feats_nhwc, img_metas, rescale=False):
        a, r1, d0, sizes = self.forward_rows(list(feats_nhwc))
        return self.get_bboxes_rows(a, r1, self._layout(a, r1, d0), self._scales_refine_tensor(), sizes, img_metas,
                                    rescale=rescale)

    def _get_bboxes_device(self, outs, img_metas, cfg, rescale):
        """the reference-signature tensors on the kernels' rows: the refined distances as D0 under zero refinement logits
        (exp(0) = 1 exactly)"""
        cls_scores, _, refine = outs
        sizes = [tuple(int(v) for v in c.shape[-2:]) for c in cls_scores]
        a, d1 = _nchw_rows(cls_scores).contiguous(), _nchw_rows(refine).contiguous()
        r = torch.zeros_like(d1)
        return self.get_bboxes_rows(a, r, self._layout(a, r, d1), a.new_ones(len(sizes)), sizes, img_metas, cfg, rescale)

    def get_bboxes(self, cls_scores, bbox_preds, bbox_preds_refine, img_metas, cfg=None, rescale=False, with_nms=True,
                   batched_nms=None):
        """reference signature (vfnet_head.py:463-595): per-level (N,C,h,w) / (N,4,h,w) / (N,4,h,w) -> per image (dets (k,5),
        labels (k,)).  Device tensors take `get_bboxes_rows`; CPU tensors the reference's chain on torch ops, with the
        caller's `batched_nms` (this package's NMS is a device kernel)."""
        return self._get_bboxes((cls_scores, bbox_preds, bbox_preds_refine), img_metas, cfg, rescale, with_nms, batched_nms)

    def _priors_host(self, sizes, outs):
        return self.get_points(sizes, outs[1][0].dtype, outs[1][0].device)

    @staticmethod
    def _level_host(l, reg, refine):
        return refine.reshape(-1, 4), None

    @staticmethod
    def _decode_host(points, d, img_hw):
        return _clamped(distance2bbox(points, d), *img_hw)

    # ------------------------------------------------------------------ train
    def forward_train_nhwc(self, feats_nhwc, img_metas, gt_bboxes, gt_labels, gt_bboxes_ignore=None):
        """the device-resident train step of the head; no host read"""
        self._refuse_ignore(gt_bboxes_ignore)
        a, d0, d1, sizes = self.forward_head_fused(list(feats_nhwc))
        return self.loss_fused(a, d0, d1, sizes, gt_bboxes, gt_labels, img_metas)

    def loss_fused(self, a, d0, d1, sizes, gt_bboxes, gt_labels, img_metas, gt_flat=None):
        """VFNetHead.loss on the row tensors of all levels: ATSS's whole-batch adaptive assignment, then the loss kernels --
        targets, IoU weights and the three normalisers are formed on the device (averaged over ranks there when
        distributed), nothing is read back.  `self.last_targets` keeps (gt_inds, coef3, norm3)."""
        from . import train_ops
        gts, labels, offs, sizes, base, gt_inds = self._assign_atss_device(a, sizes, gt_bboxes, gt_labels, img_metas, gt_flat)
        B = len(img_metas)
        meta = train_ops.VfnetLossMeta(B, sizes, self.strides, base, self.cls_out_channels, offs, self.loss_cls.alpha,
                                       self.loss_cls.gamma, self.loss_cls.iou_weighted, self.loss_bbox.eps,
                                       self.loss_cls.loss_weight, self.loss_bbox.loss_weight, self.loss_bbox_refine.loss_weight)
        losses, coef, norm3 = train_ops.vfnet_loss(a, d0, d1, gt_inds, gts, labels, meta, 0, self._norm_hook())
        self.last_targets = (gt_inds, coef, norm3)
        return dict(loss_cls=losses[0], loss_bbox=losses[1], loss_bbox_rf=losses[2])

    def get_targets(self, cls_scores, mlvl_points, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore):
        """vfnet_head.py:620-761 with use_atss, on torch ops (the host mirror): (labels per level, label weights, (l, t, r,
        b) targets per level, box weights)"""
        featmap_sizes = [tuple(int(v) for v in f.size()[-2:]) for f in cls_scores]
        assert len(featmap_sizes) == self.anchor_generator.num_levels
        anchor_list, valid_flag_list = self.get_anchors(featmap_sizes, img_metas, device=cls_scores[0].device)
        self._all_valid = None
        res = self._atss_targets(anchor_list, valid_flag_list, gt_bboxes, img_metas, gt_bboxes_ignore, gt_labels,
                                 self.cls_out_channels, True, encode=False)
        if res is None:
            return None
        _, labels_list, lw_list, bt_list, bw_list, _, _ = res
        num_imgs = len(img_metas)
        targets = [bbox2distance(p.repeat(num_imgs, 1), t.reshape(-1, 4)) for p, t in zip(mlvl_points, bt_list)]
        return ([l.reshape(-1) for l in labels_list], torch.cat([w.reshape(-1) for w in lw_list]), targets,
                torch.cat([w.reshape(-1) for w in bw_list]))

    def loss(self, cls_scores, bbox_preds, bbox_preds_refine, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore=None):
        """vfnet_head.py:315-461.  Device tensors go to the HIP kernels (`loss_fused` on the distances as they are); CPU
        tensors take the reference's chain in torch (the host mirror)."""
        assert len(cls_scores) == len(bbox_preds) == len(bbox_preds_refine)
        featmap_sizes = [tuple(int(v) for v in f.size()[-2:]) for f in cls_scores]
        C = self.cls_out_channels
        rows = lambda lst, n: torch.cat([t.permute(0, 2, 3, 1).reshape(-1, n) for t in lst])        # noqa: E731
        flat_cls, flat_d0, flat_d1 = rows(cls_scores, C), rows(bbox_preds, 4), rows(bbox_preds_refine, 4)
        if cls_scores[0].is_cuda:
            self._refuse_ignore(gt_bboxes_ignore)
            return self.loss_fused(flat_cls.float().contiguous(), flat_d0.float().contiguous(), flat_d1.float().contiguous(),
                                   featmap_sizes, gt_bboxes, gt_labels, img_metas)
        points = self.get_points(featmap_sizes, bbox_preds[0].dtype, bbox_preds[0].device)
        labels, _, bbox_targets, _ = self.get_targets(cls_scores, points, gt_bboxes, gt_labels, img_metas, gt_bboxes_ignore)
        num_imgs = cls_scores[0].size(0)
        flat_labels, flat_targets = torch.cat(labels), torch.cat(bbox_targets)
        flat_points = torch.cat([p.repeat(num_imgs, 1) for p in points])
        pos = ((flat_labels >= 0) & (flat_labels < self.num_classes)).nonzero().reshape(-1)
        num_pos = len(pos)
        num_pos_avg = max(reduce_mean(flat_cls.new_tensor(float(num_pos))).item(), 1.0)
        pos_points = flat_points[pos]
        target_boxes = distance2bbox(pos_points, flat_targets[pos]).detach()
        boxes0, boxes1 = distance2bbox(pos_points, flat_d0[pos]), distance2bbox(pos_points, flat_d1[pos])
        w_ini = bbox_overlaps(boxes0, target_boxes, is_aligned=True).clamp(min=1e-6).detach()
        w_rf = bbox_overlaps(boxes1, target_boxes, is_aligned=True).clamp(min=1e-6).detach()
        avg_ini = reduce_mean(w_ini.sum()).clamp_(min=1).item()
        avg_rf = reduce_mean(w_rf.sum()).clamp_(min=1).item()
        cls_iou_targets = torch.zeros_like(flat_cls)
        if num_pos > 0:
            loss_bbox = self.loss_bbox(boxes0, target_boxes, weight=w_ini, avg_factor=avg_ini)
            loss_bbox_refine = self.loss_bbox_refine(boxes1, target_boxes, weight=w_rf, avg_factor=avg_rf)
            cls_iou_targets[pos, flat_labels[pos]] = w_rf
        else:
            loss_bbox, loss_bbox_refine = flat_d0[pos].sum() * 0, flat_d1[pos].sum() * 0
        loss_cls = self.loss_cls(flat_cls, cls_iou_targets, avg_factor=num_pos_avg)
        return dict(loss_cls=loss_cls, loss_bbox=loss_bbox, loss_bbox_rf=loss_bbox_refine)
