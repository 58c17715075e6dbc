"""The BIT family of the reference's registry (/root/reference/models/networks.py:171-182) over the HIP engine.

``ResNet`` (networks.py:223-304; ``define_G("base_resnet18")``, :172-173) is its CNN baseline; ``BASE_Transformer``
(networks.py:307-441; ``base_transformer_pos_s4*``, :174-182) subclasses it and puts the token path -- semantic tokenizer, token
encoder, cross-attention decoder -- between ``conv_pred`` and the differencing.

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
        self.ARCH = self._arch_name(backbone, resnet_stages_num)
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
        self._add_holders()
        if backbone_weights is not None:
            self._load_backbone(backbone_weights)
        self._check_layout()

    def _arch_name(self, backbone, stages):
        return "base_{}_s{}".format(backbone, stages)

    def _add_holders(self):
        """Holders a subclass registers after ``conv_pred`` (before the layout check)."""

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


# ---- parameter holders of the token path, named and nested like models/help_funcs.py (never called)
class Residual(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn


class Residual2(Residual):
    pass


class PreNorm(nn.Module):
    def __init__(self, dim, fn):
        super().__init__()
        self.norm = nn.LayerNorm(dim)
        self.fn = fn


class PreNorm2(PreNorm):
    """One LayerNorm applied to the pixels AND to the memory tokens (help_funcs.py:43-49): its gradients have two sources."""


class FeedForward(nn.Module):
    def __init__(self, dim, hidden_dim, dropout=0.):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(dim, hidden_dim), nn.GELU(), nn.Dropout(dropout), nn.Linear(hidden_dim, dim), nn.Dropout(dropout))


class Attention(nn.Module):
    def __init__(self, dim, heads=8, dim_head=64, dropout=0.):
        super().__init__()
        self.heads, self.scale = heads, dim ** -0.5
        self.to_qkv = nn.Linear(dim, dim_head * heads * 3, bias=False)
        self.to_out = nn.Sequential(nn.Linear(dim_head * heads, dim), nn.Dropout(dropout))


class Cross_Attention(nn.Module):
    def __init__(self, dim, heads=8, dim_head=64, dropout=0., softmax=True):
        super().__init__()
        self.heads, self.scale, self.softmax = heads, dim ** -0.5, softmax
        self.to_q = nn.Linear(dim, dim_head * heads, bias=False)
        self.to_k = nn.Linear(dim, dim_head * heads, bias=False)
        self.to_v = nn.Linear(dim, dim_head * heads, bias=False)
        self.to_out = nn.Sequential(nn.Linear(dim_head * heads, dim), nn.Dropout(dropout))


class Transformer(nn.Module):
    def __init__(self, dim, depth, heads, dim_head, mlp_dim, dropout):
        super().__init__()
        self.layers = nn.ModuleList([nn.ModuleList([Residual(PreNorm(dim, Attention(dim, heads=heads, dim_head=dim_head, dropout=dropout))),
                                                    Residual(PreNorm(dim, FeedForward(dim, mlp_dim, dropout=dropout)))])
                                     for _ in range(depth)])


class TransformerDecoder(nn.Module):
    def __init__(self, dim, depth, heads, dim_head, mlp_dim, dropout, softmax=True):
        super().__init__()
        self.layers = nn.ModuleList([nn.ModuleList([Residual2(PreNorm2(dim, Cross_Attention(dim, heads=heads, dim_head=dim_head, dropout=dropout,
                                                                                            softmax=softmax))),
                                                    Residual(PreNorm(dim, FeedForward(dim, mlp_dim, dropout=dropout)))])
                                     for _ in range(depth)])


_BIT_ARCH = {(1, 64): "bit_s4_dd1_dh64", (8, 64): "bit_s4_dd8_dh64", (8, 8): "bit_s4_dd8_dh8"}


class BASE_Transformer(ResNet):
    """``BASE_Transformer(input_nc, output_nc, with_pos, resnet_stages_num=5, token_len=4, ..., dec_depth=1, decoder_dim_head=64,
    ...).forward(x1, x2)`` -> ``[logits]`` (a one-element list, as the reference): ``ResNet``'s trunk up to ``conv_pred`` on each
    date, then per date 4 semantic tokens (``conv_a`` 1x1 without bias, softmax over the positions of an image), one token-encoder
    layer over the 8 tokens of the pair (``+ pos_embedding``), the cross-attention decoder over every pixel with that date's 4
    encoded tokens as memory (``dec_depth`` layers), and ``ResNet``'s tail: ``|x1 - x2|``, bilinear x4, ``classifier``.  Both
    attentions scale by ``dim ** -0.5 = 32 ** -0.5``.  On the device the decoder never forms the ``[pixels, heads * dim_head]``
    queries: the projections are folded against the 4 memory tokens per image (stcd_amd/csrc/kernels_bit.hip).

    Supported -- the three configurations the reference registers (networks.py:174-182): ``backbone='resnet18'``,
    ``resnet_stages_num=4``, ``token_len=4``, ``with_pos='learned'``, ``enc_depth=1``, ``dim_head=64``, and (``dec_depth``,
    ``decoder_dim_head``) in {(1, 64), (8, 64), (8, 8)}; ``tokenizer``, ``token_trans``, ``with_decoder``, ``decoder_softmax`` and
    ``if_upsample_2x`` True, ``with_decoder_pos`` None.  Anything else raises NotImplementedError.  ``output_sigmoid``,
    ``backbone_weights`` and ``dtype`` as ``ResNet`` has them; ``state_dict`` keys / order / shapes are the reference's
    (``pos_embedding`` first)."""

    RETURNS_LIST = True

    def __init__(self, input_nc: int = 3, output_nc: int = 2, with_pos: Optional[str] = "learned", resnet_stages_num: int = 5,
                 token_len: int = 4, token_trans: bool = True, enc_depth: int = 1, dec_depth: int = 1, dim_head: int = 64,
                 decoder_dim_head: int = 64, tokenizer: bool = True, if_upsample_2x: bool = True, pool_mode: str = "max", pool_size: int = 2,
                 backbone: str = "resnet18", decoder_softmax: bool = True, with_decoder_pos: Optional[str] = None, with_decoder: bool = True,
                 output_sigmoid: bool = False, backbone_weights: Optional[str] = None, dtype: Optional[str] = None):
        if (tokenizer is not True or token_trans is not True or with_decoder is not True or decoder_softmax is not True
                or with_decoder_pos is not None or with_pos != "learned" or if_upsample_2x is not True or backbone != "resnet18"
                or resnet_stages_num != 4 or token_len != 4 or enc_depth != 1 or dim_head != 64
                or (dec_depth, decoder_dim_head) not in _BIT_ARCH or input_nc != 3 or output_nc not in (1, 2)):
            raise NotImplementedError("BASE_Transformer on the HIP engine: backbone resnet18, resnet_stages_num 4, token_len 4, with_pos 'learned', "
                                      "enc_depth 1, dim_head 64, (dec_depth, decoder_dim_head) in (1, 64) / (8, 64) / (8, 8), tokenizer / token_trans / "
                                      "with_decoder / decoder_softmax / if_upsample_2x True, with_decoder_pos None, input_nc 3, output_nc 1 or 2")
        self._bit = (dec_depth, decoder_dim_head)
        super().__init__(3, output_nc, resnet_stages_num=4, backbone="resnet18", output_sigmoid=output_sigmoid, if_upsample_2x=True,
                         backbone_weights=backbone_weights, dtype=dtype)
        self._ctor = dict(input_nc=3, output_nc=output_nc, with_pos="learned", resnet_stages_num=4, token_len=4, enc_depth=1,
                          dec_depth=dec_depth, dim_head=64, decoder_dim_head=decoder_dim_head, output_sigmoid=output_sigmoid)

    def _arch_name(self, backbone, stages):
        return _BIT_ARCH[self._bit]

    def _add_holders(self):      # registration order of BASE_Transformer.__init__ (networks.py:324-357)
        dec_depth, decoder_dim_head = self._bit
        self.token_len = 4
        self.conv_a = nn.Conv2d(32, 4, kernel_size=1, padding=0, bias=False)
        self.tokenizer, self.token_trans, self.with_decoder = True, True, True
        self.with_pos, self.with_decoder_pos = "learned", None
        self.pos_embedding = nn.Parameter(torch.randn(1, 8, 32))
        self.enc_depth, self.dec_depth, self.dim_head, self.decoder_dim_head = 1, dec_depth, 64, decoder_dim_head
        self.transformer = Transformer(dim=32, depth=1, heads=8, dim_head=64, mlp_dim=64, dropout=0)
        self.transformer_decoder = TransformerDecoder(dim=32, depth=dec_depth, heads=8, dim_head=decoder_dim_head, mlp_dim=64, dropout=0,
                                                      softmax=True)

    def _wrap_output(self, out, B):
        return [torch.sigmoid(out) if self.output_sigmoid else out]
