# Faster R-CNN baseline, ResNet-50 + FPN, 1x schedule, UTDAC2020 (4 classes): the model Boosting R-CNN measures itself
# against.  Written as overrides on the boosting recipe -- same data, schedule, runtime and backbone -- so that the two
# differ in exactly what the paper's ablation swaps: the neck (FPN from the stride-4 map, max-pool sixth level), the
# first stage (plain RPN: one 3x3 conv, sigmoid objectness, 256 sampled anchors per image) and the second stage
# (StandardRoIHead: softmax scores, no prior).  Hyper-parameters are the baseline's published ones.
_base_ = ['../boosting_rcnn/boosting_rcnn_r50_pafpn_1x_utdac.py']

_nms07 = dict(type='nms', iou_threshold=0.7)


def _max_iou(pos, neg, min_pos, low_quality):
    return dict(type='MaxIoUAssigner', pos_iou_thr=pos, neg_iou_thr=neg, min_pos_iou=min_pos,
                match_low_quality=low_quality, ignore_iof_thr=-1)


def _random(num, pos_fraction, add_gt):
    return dict(_delete_=True, type='RandomSampler', num=num, pos_fraction=pos_fraction, neg_pos_ub=-1,
                add_gt_as_proposals=add_gt)


model = dict(
    neck=dict(_delete_=True, type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=5),
    rpn_head=dict(
        _delete_=True, type='RPNHead', in_channels=256, feat_channels=256,
        anchor_generator=dict(type='AnchorGenerator', scales=[8], ratios=[0.5, 1.0, 2.0],
                              strides=[4, 8, 16, 32, 64]),
        bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[.0, .0, .0, .0],
                        target_stds=[1.0, 1.0, 1.0, 1.0]),
        loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0),
        loss_bbox=dict(type='L1Loss', loss_weight=1.0)),
    roi_head=dict(
        _delete_=True, type='StandardRoIHead',
        bbox_roi_extractor=dict(type='SingleRoIExtractor',
                                roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0),
                                out_channels=256, featmap_strides=[4, 8, 16, 32]),
        bbox_head=dict(type='Shared2FCBBoxHead', in_channels=256, fc_out_channels=1024, roi_feat_size=7,
                       num_classes=4,
                       bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[0., 0., 0., 0.],
                                       target_stds=[0.1, 0.1, 0.2, 0.2]),
                       reg_class_agnostic=False,
                       loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                       loss_bbox=dict(type='L1Loss', loss_weight=1.0))),
    train_cfg=dict(
        rpn=dict(assigner=_max_iou(0.7, 0.3, 0.3, True), sampler=_random(256, 0.5, False),
                 allowed_border=-1, pos_weight=-1, debug=False),
        rpn_proposal=dict(nms_pre=2000, max_per_img=1000, nms=_nms07, min_bbox_size=0),
        rcnn=dict(assigner=_max_iou(0.5, 0.5, 0.5, False), sampler=_random(512, 0.25, True),
                  pos_weight=-1, debug=False)),
    test_cfg=dict(
        rpn=dict(nms_pre=1000, max_per_img=1000, nms=_nms07, min_bbox_size=0),
        rcnn=dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)))

del _nms07, _max_iou, _random
