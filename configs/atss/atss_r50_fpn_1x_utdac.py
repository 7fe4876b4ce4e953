# ATSS baseline, ResNet-50 + FPN, 1x schedule, UTDAC2020 (4 classes): the anchor-based single-stage detector with
# adaptive training sample selection that the paper compares Boosting R-CNN with.  FPN from the stride-8 map with the two
# extra levels convolved from its own top output, ATSSHead (two 4-conv GN towers, per-level Scale, class / delta /
# centerness branches) over ONE square anchor of 8 strides per cell.  Training picks, per ground truth and level, the 9
# anchors nearest to the box centre and keeps those whose IoU reaches the mean + standard deviation of the candidates' IoUs
# and whose centre lies inside the box; focal loss over every anchor, centerness-weighted GIoU loss (weight 2) and centerness
# BCE over the positives.  Hyper-parameters are the published ones.
_base_ = ['../_base_/datasets/utdac_detection_coco.py', '../_base_/schedules/schedule_1x.py',
          '../_base_/default_runtime.py']

model = dict(
    type='ATSS',
    backbone=dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                  norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, style='pytorch',
                  init_cfg=dict(type='Pretrained', checkpoint='torchvision://resnet50')),
    neck=dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1,
              add_extra_convs='on_output', num_outs=5),
    bbox_head=dict(
        type='ATSSHead', num_classes=4, in_channels=256, stacked_convs=4, feat_channels=256,
        anchor_generator=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                              strides=[8, 16, 32, 64, 128]),
        bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[.0, .0, .0, .0], target_stds=[0.1, 0.1, 0.2, 0.2]),
        loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
        loss_bbox=dict(type='GIoULoss', loss_weight=2.0),
        loss_centerness=dict(type='CrossEntropyLoss', use_sigmoid=True, loss_weight=1.0)),
    train_cfg=dict(assigner=dict(type='ATSSAssigner', topk=9), allowed_border=-1, pos_weight=-1, debug=False),
    test_cfg=dict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.6),
                  max_per_img=100))

optimizer = dict(type='SGD', lr=0.005, momentum=0.9, weight_decay=0.0001)
