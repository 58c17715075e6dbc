"""The BIT family of the reference's registry (/root/reference/models/networks.py:171-182) over the HIP engine.

So far its CNN baseline: ``ResNet`` (networks.py:223-304; ``define_G("base_resnet18")``, :172-173), the class ``BASE_Transformer``
subclasses.  The transformer part (tokenizer, encoder / decoder between ``conv_pred`` and the differencing) is the follow-up and
will live here too.

Same constructor arguments, ``forward(x1, x2) -> logits`` contract and ``state_dict`` keys / order / shapes as the reference class,
so checkpoints interchange both ways.  The sub-modules are parameter holders only -- they are never called; forward and backward
are single calls into libstcd_hip.so (both dates batched through the shared trunk, per-date BatchNorm statistics).  No CPU
fallback.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn as nn

from .modules import HipChangeDetector
from .segcd import _ENCODERS, _PLANES, _URL_ROOT, _BasicBlock

_STRIDES = (1, 2, 1, 1)      # replace_stride_with_dilation=[False, True, True] on BasicBlock, which keeps dilation 1 (models/resnet.py:47-48)


class _ResNetHolder(nn.Module):
    """torchvision-style ResNet holders as ``models.resnet18 / resnet34(replace_stride_with_dilation=[False, True, True])`` builds
    them (models/resnet.py:127-190): layer3 / layer4 at stride 1 (their first blocks keep a 1x1 stride-1 down-sample, the width
    changes), ``avgpool`` and the unused ``fc`` included."""

    def __init__(self, name):
        super().__init__()
        _, layers, _ = _ENCODERS[name]
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        inpl = 64
        for li, (nb, pl, st) in enumerate(zip(layers, _PLANES, _STRIDES)):
            blocks = []
            for b in range(nb):
                stride = st if b == 0 else 1
                down = None
                if b == 0 and (stride != 1 or inpl != pl):               # ResNet._make_layer (models/resnet.py:165-187)
                    down = nn.Sequential(nn.Conv2d(inpl, pl, kernel_size=1, stride=stride, bias=False), nn.BatchNorm2d(pl))
                blocks.append(_BasicBlock(inpl, pl, stride, down))
                inpl = pl
            setattr(self, f"layer{li + 1}", nn.Sequential(*blocks))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512, 1000)
        for m in self.modules():                      # models/resnet.py:157-163
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)


class ResNet(HipChangeDetector):
    """``ResNet(input_nc, output_nc, resnet_stages_num=5, backbone='resnet18', output_sigmoid=False, if_upsample_2x=True)
    .forward(x1, x2)`` -> logits ``[B, output_nc, H, W]``: a ResNet trunk at 1/8 resolution on each date (shared weights, per-date
    BatchNorm statistics), nearest x2, ``conv_pred`` (3x3, -> 32), ``|x1 - x2|``, bilinear x4, ``classifier`` (networks.py:267-304).

    Supported: ``backbone`` resnet18 / resnet34, ``resnet_stages_num`` 4 (the trunk stops after layer3, BIT's configuration) or 5,
    ``if_upsample_2x=True``, ``input_nc == 3`` (the reference ignores the argument: its ``conv1`` always takes 3 channels),
    ``output_nc`` 1 or 2; anything else raises NotImplementedError (resnet50's Bottleneck really dilates its 3x3 convolutions).
    H and W must be multiples of 32.

    Deviations from the reference, both deliberate:

    * ``backbone_weights`` replaces the hard-wired ``pretrained=True`` (there may be no network to fetch a checkpoint from):
      None -- the backbone's own random init (models/resnet.py:157-163); a path -- that ResNet's ``state_dict`` file;
      "imagenet" -- served through torch.hub, i.e. from the hub cache when there is no network.
    * The parameters no output depends on (``resnet.fc.*``, and ``resnet.layer4.*`` with 4 stages) receive an exactly ZERO
      gradient, where the reference leaves ``grad is None``.  Optimizers skip a None gradient but not a zero one, so weight decay
      acts on these tensors here; nothing the network computes changes."""

    ARCH = "base_resnet18_s5"
    OUT_MAPS = 1

    def __init__(self, input_nc: int = 3, output_nc: int = 2, resnet_stages_num: int = 5, backbone: str = "resnet18",
                 output_sigmoid: bool = False, if_upsample_2x: bool = True, backbone_weights: Optional[str] = None,
                 dtype: Optional[str] = None):
        if (backbone not in ("resnet18", "resnet34") or resnet_stages_num not in (4, 5) or if_upsample_2x is not True
                or input_nc != 3 or output_nc not in (1, 2)):
            raise NotImplementedError("ResNet (base_resnet18) on the HIP engine: backbone resnet18 / resnet34, resnet_stages_num 4 or 5, "
                                      "if_upsample_2x=True, input_nc 3, output_nc 1 or 2")
        self.ARCH = "base_{}_s{}".format(backbone, resnet_stages_num)
        super().__init__(3, output_nc, dtype)
        self.resnet = _ResNetHolder(backbone)
        self.relu = nn.ReLU()
        self.upsamplex2 = nn.Upsample(scale_factor=2)
        self.upsamplex4 = nn.Upsample(scale_factor=4, mode="bilinear")
        # TwoLayerConv2d (models/help_funcs.py): conv3x3 without bias, BatchNorm2d, ReLU, conv3x3 with bias
        self.classifier = nn.Sequential(nn.Conv2d(32, 32, kernel_size=3, padding=1, bias=False), nn.BatchNorm2d(32), nn.ReLU(),
                                        nn.Conv2d(32, output_nc, kernel_size=3, padding=1))
        self.resnet_stages_num = resnet_stages_num
        self.if_upsample_2x = if_upsample_2x
        self.conv_pred = nn.Conv2d(512 if resnet_stages_num == 5 else 256, 32, kernel_size=3, padding=1)
        self.output_sigmoid = output_sigmoid
        self.sigmoid = nn.Sigmoid()
        self._backbone = backbone
        self._ctor = dict(input_nc=3, output_nc=output_nc, resnet_stages_num=resnet_stages_num, backbone=backbone,
                          output_sigmoid=output_sigmoid, if_upsample_2x=True)
        if backbone_weights is not None:
            self._load_backbone(backbone_weights)
        self._check_layout()

    def _load_backbone(self, weights: str):
        if os.path.exists(weights):
            sd = torch.load(weights, map_location="cpu")
        elif weights == "imagenet":
            sd = torch.hub.load_state_dict_from_url(_URL_ROOT + _ENCODERS[self._backbone][2], map_location="cpu")
        else:
            raise KeyError("Wrong pretrained weights `{}` for backbone `{}`. Available options are: "
                           "['imagenet', <path to a state_dict file>]".format(weights, self._backbone))
        self.resnet.load_state_dict(sd)

    def __deepcopy__(self, memo):
        new = type(self)(dtype=self._engine.dtype, **self._ctor)
        new.load_state_dict({k: v.detach().clone() for k, v in self.state_dict().items()})
        new.train(self.training)
        if self._flat_params is not None:
            new.to(self._flat_params.device)
        return new

    def _wrap_output(self, out, B):
        return torch.sigmoid(out) if self.output_sigmoid else out
