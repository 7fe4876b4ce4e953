# Boosting R-CNN, ResNet-50 + PAFPN, 1x schedule, UTDAC2020, with the backbone's BatchNorm layers in training mode
# (norm_eval=False): stages 2-4 normalise with batch statistics and update their running statistics -- fine-tuning the
# statistics on underwater data, which is far from ImageNet's.  frozen_stages=1 of the base recipe stays: the stem and
# stage 1 keep their weights and their running statistics.
_base_ = '../boosting_rcnn/boosting_rcnn_r50_pafpn_1x_utdac.py'

model = dict(backbone=dict(norm_eval=False))
