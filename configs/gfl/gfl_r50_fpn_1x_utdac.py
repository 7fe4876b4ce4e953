# GFL baseline, ResNet-50 + FPN, 1x schedule, UTDAC2020 (4 classes): ATSS's towers and adaptive assignment with the
# Generalized Focal Loss on top.  GFLHead (two 4-conv GN towers, per-level Scale) over ONE square anchor of 8 strides per
# cell predicts a joint class / localisation-quality score per class and, per box side, a distribution over the distances
# 0 .. 16 strides whose expectation is the side.  Quality Focal Loss supervises the class score with the IoU of the predicted
# box, Distribution Focal Loss (weight 0.25) the two bins around the target distance, GIoU loss (weight 2) the box; the box
# terms are weighted by the anchor's best class score.  Hyper-parameters are the published ones.
_base_ = ['../_base_/datasets/utdac_detection_coco.py', '../_base_/schedules/schedule_1x.py',
          '../_base_/default_runtime.py']

model = dict(
    type='GFL',
    backbone=dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                  norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, style='pytorch',
                  init_cfg=dict(type='Pretrained', checkpoint='torchvision://resnet50')),
    neck=dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1,
              add_extra_convs='on_output', num_outs=5),
    bbox_head=dict(
        type='GFLHead', num_classes=4, in_channels=256, stacked_convs=4, feat_channels=256,
        anchor_generator=dict(type='AnchorGenerator', ratios=[1.0], octave_base_scale=8, scales_per_octave=1,
                              strides=[8, 16, 32, 64, 128]),
        loss_cls=dict(type='QualityFocalLoss', use_sigmoid=True, beta=2.0, loss_weight=1.0),
        loss_dfl=dict(type='DistributionFocalLoss', loss_weight=0.25),
        reg_max=16,
        loss_bbox=dict(type='GIoULoss', loss_weight=2.0)),
    train_cfg=dict(assigner=dict(type='ATSSAssigner', topk=9), allowed_border=-1, pos_weight=-1, debug=False),
    test_cfg=dict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.6),
                  max_per_img=100))

optimizer = dict(type='SGD', lr=0.005, momentum=0.9, weight_decay=0.0001)
