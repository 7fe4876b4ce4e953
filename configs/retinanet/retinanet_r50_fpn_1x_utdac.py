# RetinaNet baseline, ResNet-50 + FPN, 1x schedule, UTDAC2020 (4 classes): the first of the single-stage detectors the
# paper compares Boosting R-CNN with.  FPN from the stride-8 map with the two extra levels convolved from the backbone
# output, RetinaHead (two 4-conv towers without normalisation, 9 anchors per cell, sigmoid class scores), focal loss
# over every anchor without a sampler, L1 on the encoded deltas.  Hyper-parameters are the published ones.
_base_ = ['../_base_/datasets/utdac_detection_coco.py', '../_base_/default_runtime.py',
          '../_base_/schedules/schedule_1x.py']

model = dict(
    type='RetinaNet',
    backbone=dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                  norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, style='pytorch',
                  init_cfg=dict(type='Pretrained', checkpoint='torchvision://resnet50')),
    neck=dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, start_level=1,
              add_extra_convs='on_input', num_outs=5),
    bbox_head=dict(
        type='RetinaHead', num_classes=4, in_channels=256, stacked_convs=4, feat_channels=256,
        anchor_generator=dict(type='AnchorGenerator', octave_base_scale=4, scales_per_octave=3,
                              ratios=[0.5, 1.0, 2.0], strides=[8, 16, 32, 64, 128]),
        bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[.0, .0, .0, .0],
                        target_stds=[1.0, 1.0, 1.0, 1.0]),
        loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=1.0),
        loss_bbox=dict(type='L1Loss', loss_weight=1.0)),
    train_cfg=dict(
        assigner=dict(type='MaxIoUAssigner', pos_iou_thr=0.5, neg_iou_thr=0.4, min_pos_iou=0, ignore_iof_thr=-1),
        allowed_border=-1, pos_weight=-1, debug=False),
    test_cfg=dict(nms_pre=1000, min_bbox_size=0, score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5),
                  max_per_img=100))

optimizer = dict(type='SGD', lr=0.005, momentum=0.9, weight_decay=0.0001)
data = dict(samples_per_gpu=4, workers_per_gpu=8)
