# Boosting R-CNN, ResNet-50 + PAFPN, 1x schedule, UTDAC2020, with deformable convs (DCN v1, mmcv DeformConv2dPack) as the
# 3x3 conv of every bottleneck in stages c3-c5 (mmdetection's `dconv_c3-c5` naming).
_base_ = '../boosting_rcnn/boosting_rcnn_r50_pafpn_1x_utdac.py'

model = dict(
    backbone=dict(dcn=dict(type='DCN', deform_groups=1, fallback_on_stride=False),
                  stage_with_dcn=(False, True, True, True)))
