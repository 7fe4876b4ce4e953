"""ResNet with DCN / DCNv2 bottlenecks (mmdetection's `dconv_c3-c5`), construction side: parameter names and shapes as
mmcv's DeformConv2dPack / ModulatedDeformConv2dPack, zero-initialised offset branch, strides, freezing, the recipe, and a
plain-ResNet checkpoint under a DCN backbone.  No device."""
import os

import pytest
import torch

import brcnn  # noqa: F401
from brcnn import Config, build_detector
from brcnn.backbones import DCN, DCNv2, ResNet, ResNeXt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPE = os.path.join(ROOT, 'configs', 'dcn', 'boosting_rcnn_r50_dconv_c3-c5_pafpn_1x_utdac.py')
V1 = dict(type='DCN', deform_groups=1, fallback_on_stride=False)
C3_C5 = (False, True, True, True)


def _r50(dcn=V1, **kw):
    return ResNet(depth=50, dcn=dcn, stage_with_dcn=C3_C5, **kw)


def test_r50_dconv_c3_c5_parameter_layout():
    m = _r50()
    sd = m.state_dict()
    assert not any('conv_offset' in k for k in sd if k.startswith('layer1.'))
    assert all(isinstance(b.conv2, torch.nn.Conv2d) for b in m.layer1)
    for li, nb, p in ((2, 4, 128), (3, 6, 256), (4, 3, 512)):
        for b in range(nb):
            pre = f'layer{li}.{b}.conv2.'
            assert tuple(sd[pre + 'weight'].shape) == (p, p, 3, 3)
            assert tuple(sd[pre + 'conv_offset.weight'].shape) == (18, p, 3, 3)
            assert tuple(sd[pre + 'conv_offset.bias'].shape) == (18,)
            assert pre + 'bias' not in sd
            blk = getattr(m, f'layer{li}')[b]
            assert type(blk.conv2) is DCN and blk.with_dcn
            assert float(sd[pre + 'conv_offset.weight'].abs().max()) == 0 and float(sd[pre + 'conv_offset.bias'].abs().max()) == 0
            assert float(sd[pre + 'weight'].abs().max()) > 0
            s = 2 if b == 0 else 1
            assert blk.conv2.stride == s and blk.conv2.conv_offset.stride == (s, s)
            assert blk.conv2.conv_offset.padding == (1, 1) and blk.conv2.conv_offset.dilation == (1, 1)
    # the key set is the plain net's plus the offset branches
    plain = set(ResNet(depth=50).state_dict())
    assert plain < set(sd) and all('.conv_offset.' in k for k in set(sd) - plain)


def test_dcnv2_deform_groups_rows():
    m = _r50(dict(type='DCNv2', deform_groups=4, fallback_on_stride=False))
    c = m.layer3[1].conv2
    assert type(c) is DCNv2 and c.deform_groups == 4 and c.modulated
    assert tuple(c.conv_offset.weight.shape) == (108, 256, 3, 3) and tuple(c.conv_offset.bias.shape) == (108,)
    assert tuple(_r50(dict(type='DCN', deform_groups=2)).layer2[0].conv2.conv_offset.weight.shape) == (36, 128, 3, 3)


def test_init_weights_rezeroes_conv_offset():
    m = _r50()
    for p in m.parameters():
        torch.nn.init.normal_(p)
    m.init_weights()
    for k, v in m.state_dict().items():
        if '.conv_offset.' in k:
            assert float(v.abs().max()) == 0, k
    assert float(m.layer2[0].conv1.weight.detach().abs().max()) > 0


def test_frozen_stages_and_norm_eval_as_the_plain_net():
    m = _r50(frozen_stages=2, norm_eval=True).train()
    assert not m.layer2.training and m.layer3.training
    assert not any(p.requires_grad for p in m.layer2.parameters())          # the offset branch of a frozen stage too
    assert all(p.requires_grad for p in m.layer3[0].conv2.parameters())
    assert all(not b.training for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d))
    m2 = _r50(frozen_stages=-1, norm_eval=False).train()
    assert m2.layer4[0].bn2.training and all(p.requires_grad for p in m2.parameters())


def test_refusals():
    with pytest.raises(NotImplementedError, match='fallback_on_stride'):
        _r50(dict(type='DCN', deform_groups=1, fallback_on_stride=True))
    with pytest.raises(AssertionError):
        ResNet(depth=50, dcn=V1, stage_with_dcn=(False, True, True))
    with pytest.raises(KeyError):
        _r50(dict(type='DCNv3'))
    with pytest.raises(NotImplementedError, match='ResNeXt'):
        ResNeXt(depth=50, groups=32, base_width=4, dcn=V1, stage_with_dcn=C3_C5)
    with pytest.raises(AssertionError):
        DCN(64, 64, groups=2)


def test_recipe_loads_and_builds():
    cfg = Config.fromfile(RECIPE)
    b = cfg.model.backbone
    assert dict(b.dcn) == V1 and tuple(b.stage_with_dcn) == C3_C5 and b.depth == 50
    base = Config.fromfile(os.path.join(ROOT, 'configs', 'boosting_rcnn', 'boosting_rcnn_r50_pafpn_1x_utdac.py'))
    assert cfg.model.roi_head == base.model.roi_head and cfg.data == base.data and cfg.optimizer == base.optimizer
    m = build_detector(cfg.model)
    assert type(m.backbone.layer4[2].conv2) is DCN and isinstance(m.backbone.layer1[0].conv2, torch.nn.Conv2d)


def test_plain_resnet_checkpoint_under_a_dcn_backbone(tmp_path, monkeypatch):
    from brcnn.blocks import load_pretrained
    src = ResNet(depth=50)
    sd = {k: torch.randn_like(v) if v.is_floating_point() else v for k, v in src.state_dict().items()}
    sd['fc.weight'], sd['fc.bias'] = torch.zeros(1000, 2048), torch.zeros(1000)       # as in a torchvision file
    torch.save(sd, str(tmp_path / 'resnet50.pth'))
    monkeypatch.delenv('BRCNN_ALLOW_RANDOM_INIT', raising=False)
    m = _r50()
    assert load_pretrained(m, dict(type='Pretrained', checkpoint=str(tmp_path / 'resnet50.pth')))
    got = m.state_dict()
    for k, v in got.items():
        if '.conv_offset.' in k:
            assert float(v.abs().max()) == 0, k
        else:
            assert torch.equal(v, sd[k]), k
