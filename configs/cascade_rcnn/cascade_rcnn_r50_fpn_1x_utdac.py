# Cascade R-CNN baseline, ResNet-50 + FPN, 1x schedule, UTDAC2020 (4 classes): the second two-stage baseline Boosting
# R-CNN measures itself against.  Written as overrides on the Faster R-CNN recipe -- same data, schedule, runtime,
# backbone, neck and RPN head -- so that the two differ in what makes a cascade: three box heads trained at rising IoU
# thresholds (0.5 / 0.6 / 0.7) on each other's regressed boxes, with tightening delta normalisation and class-agnostic
# regression, their losses weighted 1 / 0.5 / 0.25 and their logits averaged at test time.  Hyper-parameters are the
# baseline's published ones (SmoothL1 box losses, RPN anchors inside the image, 2000 training proposals).
_base_ = ['../faster_rcnn/faster_rcnn_r50_fpn_1x_utdac.py']

_nms07 = dict(type='nms', iou_threshold=0.7)


def _head(stds):
    return dict(type='Shared2FCBBoxHead', in_channels=256, fc_out_channels=1024, roi_feat_size=7, num_classes=4,
                bbox_coder=dict(type='DeltaXYWHBBoxCoder', target_means=[0., 0., 0., 0.], target_stds=stds),
                reg_class_agnostic=True,
                loss_cls=dict(type='CrossEntropyLoss', use_sigmoid=False, loss_weight=1.0),
                loss_bbox=dict(type='SmoothL1Loss', beta=1.0, loss_weight=1.0))


def _stage(iou):
    return dict(assigner=dict(type='MaxIoUAssigner', pos_iou_thr=iou, neg_iou_thr=iou, min_pos_iou=iou,
                              match_low_quality=False, ignore_iof_thr=-1),
                sampler=dict(type='RandomSampler', num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True),
                pos_weight=-1, debug=False)


model = dict(
    type='CascadeRCNN',
    rpn_head=dict(loss_bbox=dict(_delete_=True, type='SmoothL1Loss', beta=1.0 / 9.0, loss_weight=1.0)),
    roi_head=dict(
        _delete_=True, type='CascadeRoIHead', num_stages=3, stage_loss_weights=[1, 0.5, 0.25],
        bbox_roi_extractor=dict(type='SingleRoIExtractor',
                                roi_layer=dict(type='RoIAlign', output_size=7, sampling_ratio=0),
                                out_channels=256, featmap_strides=[4, 8, 16, 32]),
        bbox_head=[_head([0.1, 0.1, 0.2, 0.2]), _head([0.05, 0.05, 0.1, 0.1]), _head([0.033, 0.033, 0.067, 0.067])]),
    train_cfg=dict(
        rpn=dict(allowed_border=0),
        rpn_proposal=dict(nms_pre=2000, max_per_img=2000, nms=_nms07, min_bbox_size=0),
        rcnn=[_stage(0.5), _stage(0.6), _stage(0.7)]),
    test_cfg=dict(
        rpn=dict(nms_pre=1000, max_per_img=1000, nms=_nms07, min_bbox_size=0),
        rcnn=dict(score_thr=0.05, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100)))

del _nms07, _head, _stage
