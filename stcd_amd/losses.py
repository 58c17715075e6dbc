"""Loss functions of the path, same names and argument meaning as the reference
(/root/reference/models/losses.py:6-21 ``cross_entropy``, :24-34 ``cd_loss``, :38-59 ``get_alpha``, :70-160 ``FocalLoss``,
:170-242 ``mIoULoss`` / ``mmIoULoss``; /root/reference/train_pse_cd.py:436-462 ``Dice`` / ``BCE_DICE``), computed by the
fused HIP kernels of libstcd_hip.so (forward value and gradient in one pass; the autograd node only scales by the incoming
gradient)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from ._lib import StcdError

_scratch = {}


def _scratch_for(device):
    s = _scratch.get(device)
    if s is None:
        s = torch.empty(_lib.lib().stcd_loss_scratch_bytes(), dtype=torch.uint8, device=device)
        _scratch[device] = s
    return s


def _p(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(t, what):
    if not t.is_cuda:
        raise StcdError(f"{what}: the HIP loss kernels need tensors on the GPU; there is no CPU fallback")


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, ignore_index):
        B, Cn = logits.shape[:2]
        hw = logits.numel() // (B * Cn)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        need_grad = logits.requires_grad
        dl = torch.empty_like(logits) if need_grad else None
        with torch.cuda.device(logits.device):
            _lib.check(_lib.lib().stcd_loss_ce(_p(logits), _p(target), B, Cn, hw, ignore_index, _p(loss),
                                               _p(dl) if need_grad else None, _p(_scratch_for(logits.device)), _stream()))
        ctx.dl = dl
        return loss

    @staticmethod
    def backward(ctx, g):
        return ctx.dl * g, None, None


def cross_entropy(input, target, weight=None, reduction="mean", ignore_index=255):
    """logSoftmax_with_loss: input N*C*H*W, target N*1*H*W or N*H*W (any numeric dtype)."""
    if weight is not None or reduction != "mean":
        raise NotImplementedError("only the reference's call form (weight=None, reduction='mean') is implemented")
    _need_cuda(input, "cross_entropy")
    target = target.long()
    if target.dim() == 4:
        target = torch.squeeze(target, dim=1)
    if input.shape[-1] != target.shape[-1]:
        input = F.interpolate(input, size=target.shape[1:], mode="bilinear", align_corners=True)
    return _CrossEntropyFn.apply(input.contiguous().float(), target.contiguous(), int(ignore_index))


class _BceDiceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target, from_logits):
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        need_grad = x.requires_grad
        dx = torch.empty_like(x) if need_grad else None
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().stcd_loss_bce_dice(_p(x), _p(target), x.numel(), int(from_logits), _p(loss),
                                                     _p(dx) if need_grad else None, _p(_scratch_for(x.device)), _stream()))
        ctx.dx = dx
        return loss

    @staticmethod
    def backward(ctx, g):
        return ctx.dx * g, None, None


def cd_loss(input, target):
    """BCE(mean) + Dice(smooth=1) on PROBABILITIES, as the reference calls it."""
    _need_cuda(input, "cd_loss")
    return _BceDiceFn.apply(input.contiguous().float(), target.contiguous().float(), False)


def bce_dice_with_logits(logits, target):
    """cd_loss(sigmoid(logits), target) with the sigmoid fused into the kernel (train_pse_cd.py:227-228)."""
    _need_cuda(logits, "bce_dice_with_logits")
    return _BceDiceFn.apply(logits.contiguous().float(), target.contiguous().float(), True)


class _ContrastiveFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, cd_label, pse_label):
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        need_grad = pred.requires_grad
        dp = torch.empty_like(pred) if need_grad else None
        with torch.cuda.device(pred.device):
            _lib.check(_lib.lib().stcd_loss_contrastive(_p(pred), _p(cd_label), _p(pse_label), cd_label.numel(), _p(loss),
                                                        _p(dp) if need_grad else None, _p(_scratch_for(pred.device)), _stream()))
        ctx.dp = dp
        return loss

    @staticmethod
    def backward(ctx, g):
        return ctx.dp * g, None, None


def contrastive_loss(pred, cd_label, pse_label, img_name=None):
    """/root/reference/train_stcd.py:334-385, same arguments (``img_name`` only fed the reference's commented-out
    visualisation): ``pred`` = change PROBABILITIES of cat(real pairs, pseudo pairs) along the batch axis, the labels of
    the two halves [b,1,H,W]; masked MSE between the halves where the labels agree plus masked MSE against the inverted
    real prediction where they differ.  One fused HIP pass for value and gradient (both halves receive gradient)."""
    _need_cuda(pred, "contrastive_loss")
    b = cd_label.shape[0]
    if pred.shape[0] != 2 * b or cd_label.shape != pse_label.shape or pred[:b].shape != cd_label.shape:
        raise StcdError(f"contrastive_loss: pred {tuple(pred.shape)} must hold 2 x the label batch {tuple(cd_label.shape)}")
    return _ContrastiveFn.apply(pred.contiguous().float(), cd_label.contiguous().long(), pse_label.contiguous().long())


class Dice(nn.Module):
    """train_pse_cd.py:436-447: 1 - (2*sum(p*t) + 1) / (sum(p) + sum(t) + 1) on probabilities."""

    def forward(self, pred, target):
        _need_cuda(pred, "Dice")
        return _BceDiceFn.apply(pred.contiguous().float(), target.contiguous().float(), 2)


class BCE_DICE(nn.Module):
    """train_pse_cd.py:451-462: forward(pmask = sigmoid output, rmask = {0,1} target)."""

    def forward(self, pmask, rmask):
        return cd_loss(pmask, rmask)


# ------------------------------------------------------------------ focal / mIoU / min-max IoU (reference models/losses.py:38-242)
def get_alpha(supervised_loader):
    """Pixel count per class over the loader's labels ``batch['L']``: a list of length max label + 1, with 255 (the ignore
    label) counted as class 0, as the reference computes it -- but without writing 0 into the batch as the reference does."""
    counts = torch.zeros(0, dtype=torch.int64)
    for batch in supervised_loader:
        lab = torch.as_tensor(batch["L"]).detach().reshape(-1).cpu().long()
        lab = torch.where(lab == 255, torch.zeros_like(lab), lab)
        if lab.numel() and int(lab.min()) < 0:
            raise ValueError("get_alpha: negative label %d" % int(lab.min()))
        c = torch.bincount(lab)
        if c.numel() > counts.numel():
            c[:counts.numel()] += counts
            counts = c
        else:
            counts[:c.numel()] += c
    return [int(v) for v in counts]


def softmax_helper(x):
    """Softmax over the class axis (dim 1).  ``FocalLoss(apply_nonlin=softmax_helper)`` recognises this function and fuses the
    softmax into its kernel."""
    return torch.softmax(x, 1)


def _target_long(target, npix, what):
    t = target.detach()
    if t.numel() != npix:
        raise StcdError(f"{what}: target {tuple(target.shape)} does not hold one label per pixel ({npix})")
    return t.reshape(-1).long().contiguous()


class _FocalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target, alpha, gamma, smooth, flags):
        B, Cn = x.shape[:2]
        hw = x.numel() // (B * Cn)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        need_grad = x.requires_grad
        dx = torch.empty_like(x) if need_grad else None
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().stcd_loss_focal(_p(x), _p(target), B, Cn, hw, _p(alpha), float(gamma), float(smooth), int(flags),
                                                  _p(loss), _p(dx) if need_grad else None, _p(_scratch_for(x.device)), _stream()))
        ctx.dx = dx
        return loss

    @staticmethod
    def backward(ctx, g):
        return ctx.dx * g, None, None, None, None, None


class FocalLoss(nn.Module):
    """Focal loss with label smoothing (reference models/losses.py:70-160), same constructor and ``forward(logit, target)``.
    Per pixel: k = one-hot(label) clamped to [smooth/(C-1), 1-smooth], pt = sum_c k_c p_c + smooth,
    loss = -alpha[label] (1-pt)^gamma log(pt), averaged over the pixels (summed when ``size_average=False``).
    ``apply_nonlin``: ``softmax_helper`` -- the softmax runs inside the kernel; ``None`` -- ``logit`` holds probabilities;
    any other callable is applied in torch first.  ``alpha``: None -> ones; a list / ndarray of class counts -> the inverse
    class frequency sum(a)/a (a zero count raises here, the reference would produce inf); a float -> 1-alpha for every
    class and alpha at ``balance_index``.  Label 225 counts as class 0 as in the reference; any other label outside [0, C)
    gives a NaN loss (the reference raises in ``scatter_``).  2 <= C <= 16."""

    def __init__(self, apply_nonlin=None, alpha=None, gamma=1, balance_index=0, smooth=1e-5, size_average=True):
        super().__init__()
        self.apply_nonlin = apply_nonlin
        self.alpha = alpha
        self.gamma = gamma
        self.balance_index = balance_index
        self.smooth = smooth
        self.size_average = size_average
        if self.smooth is not None and (self.smooth < 0 or self.smooth > 1.0):
            raise ValueError("smooth value should be in [0,1]")
        self._alpha_dev = {}

    def _alpha_vector(self, num_class, device):
        a = self.alpha
        if a is None:
            key = None
        elif isinstance(a, (list, np.ndarray)):
            key = ("counts", tuple(np.asarray(a, np.float64).ravel().tolist()))
        elif isinstance(a, float):
            key = ("float", float(a), int(self.balance_index))
        else:
            raise TypeError("Not support alpha type")
        ck = (str(device), num_class, key)
        vec = self._alpha_dev.get(ck)
        if vec is None:
            if key is None:
                host = np.ones(num_class, np.float64)
            elif key[0] == "counts":
                host = np.asarray(key[1], np.float64)
                if host.size != num_class:
                    raise ValueError(f"FocalLoss: alpha holds {host.size} entries for {num_class} classes")
                if (host == 0).any():
                    raise ValueError("FocalLoss: a class count of zero in alpha (its inverse frequency is infinite)")
                host = 1.0 / (host / host.sum())
            else:
                host = np.full(num_class, 1.0 - key[1])
                host[key[2]] = key[1]
            vec = torch.tensor(host, dtype=torch.float32).to(device)
            self._alpha_dev = {ck: vec}
        return vec

    def forward(self, logit, target):
        _need_cuda(logit, "FocalLoss")
        fused = self.apply_nonlin is softmax_helper
        if self.apply_nonlin is not None and not fused:
            logit = self.apply_nonlin(logit)
        x = logit.contiguous().float()
        B, Cn = x.shape[:2]
        if not 2 <= Cn <= 16:
            raise StcdError(f"FocalLoss: {Cn} classes; the kernel supports 2 to 16")
        npix = x.numel() // Cn
        t = _target_long(target.to(x.device), npix, "FocalLoss")
        flags = (1 if fused else 0) | (0 if self.size_average else 2)
        return _FocalFn.apply(x, t, self._alpha_vector(Cn, x.device), float(self.gamma), float(self.smooth or 0.0), flags)


class _IoUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, weight, mode):
        B, Cn = logits.shape[:2]
        hw = logits.numel() // (B * Cn)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        need_grad = logits.requires_grad
        dl = torch.empty_like(logits) if need_grad else None
        l = _lib.lib()
        scratch = torch.empty(l.stcd_loss_iou_scratch_bytes(B, Cn, hw), dtype=torch.uint8, device=logits.device)
        with torch.cuda.device(logits.device):
            _lib.check(l.stcd_loss_iou(_p(logits), _p(target), B, Cn, hw, _p(weight) if weight is not None else None, int(mode),
                                       _p(loss), _p(dl) if need_grad else None, _p(scratch), _stream()))
        ctx.dl = dl
        return loss

    @staticmethod
    def backward(ctx, g):
        return ctx.dl * g, None, None, None


def _iou_loss(inputs, target, n_classes, weight, mode, what):
    _need_cuda(inputs, what)
    x = inputs.contiguous().float()
    if x.dim() < 3 or x.shape[1] != n_classes:
        raise StcdError(f"{what}: input {tuple(inputs.shape)} must be N x {n_classes} x H x W")
    if not 2 <= n_classes <= 16:
        raise StcdError(f"{what}: {n_classes} classes; the kernel supports 2 to 16")
    t = _target_long(target.to(x.device), x.numel() // n_classes, what)
    return _IoUFn.apply(x, t, weight, mode)


class mIoULoss(nn.Module):
    """Weighted mean-IoU loss (reference models/losses.py:170-206), same constructor and ``forward(inputs, target)``:
    p = softmax(inputs), t = one-hot(target); per (sample, class) iou = sum p t / (sum (p + t - p t) + 1e-8);
    loss = -mean(weight_c iou).  ``weight=None`` means ones (the reference fails in ``forward`` on ``None * inter``).
    A label outside [0, n_classes) gives a NaN loss.  ``size_average`` is accepted and unused, as in the reference."""

    def __init__(self, weight=None, size_average=True, n_classes=2):
        super().__init__()
        self.classes = n_classes
        self.weights = weight
        self._w_dev = None

    def _weight_vector(self, device):
        w = self.weights
        if w is None:
            return None
        if self._w_dev is None or self._w_dev[0] is not w or self._w_dev[1].device != device:
            v = torch.as_tensor(w).detach().reshape(-1).to(device=device, dtype=torch.float32).contiguous()
            if v.numel() != self.classes:
                raise StcdError(f"mIoULoss: weight holds {v.numel()} entries for {self.classes} classes")
            self._w_dev = (w, v)
        return self._w_dev[1]

    def forward(self, inputs, target, is_target_variable=False):
        return _iou_loss(inputs, target, self.classes, self._weight_vector(inputs.device), 0, "mIoULoss")


class mmIoULoss(nn.Module):
    """Min-max IoU loss (reference models/losses.py:208-242): loss = -min(iou) - mean(iou) over (sample, class), iou as in
    ``mIoULoss``; the gradient of the min is split evenly among tied entries (torch's ``min()`` backward)."""

    def __init__(self, n_classes=2):
        super().__init__()
        self.classes = n_classes

    def forward(self, inputs, target, is_target_variable=False):
        return _iou_loss(inputs, target, self.classes, None, 1, "mmIoULoss")
