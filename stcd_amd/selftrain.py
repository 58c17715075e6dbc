"""The self-training round between two trainings: reliability split and pseudo-labels, on the device.

In the reference this is /root/reference/train_stcd.py:96-204.  K saved checkpoints predict every training pair; the IoU of the
change class between each earlier checkpoint's mask and the last checkpoint's mask is averaged into a per-pair reliability; the
upper half of the sorted pairs goes to ``list/reliable_ids.txt``, the rest to ``list/unreliable_ids.txt`` (:96-135).  Then the
model predicts every pair of such a list, the mask times 255 is saved under ``pseudo_label/`` and the scores of the change class
against the true labels are printed (:137-204).  The reference does both with batch size 1 and, per pair and checkpoint, a
sigmoid, a compare, an ``.int()``, a ``.cpu()`` and a host ``bincount``; here one launch of ``stcd_selftrain_score`` per batch
(include/stcd_hip.h) takes the raw outputs of all checkpoints and leaves the mask and integer counts on the device, and the
drivers copy back once per ``flush`` batches.

``scene_round`` is the same round over one pair of whole scenes instead of pre-cut crops: every checkpoint goes through
``scene.predict_scene`` (``gate="seg"``: ``scene.predict_scene_heads`` and its gated mask, train_stcd.py:170-176),
``stcd_scene_cell_agree`` counts the agreement per cell of the scene, ``stcd_mask_close`` is the 5 x 5 closing of the pseudo-label
(train_stcd.py:186-188), and ``export_cells`` writes the tile set and the two lists.  ``refine_round`` cleans a round's pseudo-label
at object level (``objects.filter_objects``: small blobs cleared, small holes filled) and scores it again.

``reliability``, ``split_reliable``, ``write_lists`` and ``cell_grid`` are host-only and need no GPU.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Iterable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import StcdError
from .metrics import scores_from_cm
from .scene import MAX_MODELS, _change_logits, _device_of, _evaluating, _label_tensor, _model_list, _ptr, predict_scene


class BatchScore(NamedTuple):
    mask: torch.Tensor                  # uint8 [B,H,W] on the device: the LAST model's prediction, mask_value where change
    agree: Optional[torch.Tensor]       # int64 [B,K-1,2,2] on the device, agree[b, i, last, pred_i]; None for one model
    cm: Optional[torch.Tensor]          # int64 [4] on the device, cm[2 * label + pred_last] (label given)


class Selection(NamedTuple):
    reliable: List[str]
    unreliable: List[str]
    names: List[str]                    # every pair, in processing order
    reliability: np.ndarray             # float64 [N], aligned with names
    agree: np.ndarray                   # int64 [N,K-1,2,2]


def score_batch(models, x1: torch.Tensor, x2: torch.Tensor, label: Optional[torch.Tensor] = None, threshold: float = 0.0,
                mask_value: int = 1, cm: Optional[torch.Tensor] = None) -> BatchScore:
    """Every model of ``models`` (1..8 modules on one GPU: engine families, ``SegCD``, ``ChangeFormerV6`` or any torch module that
    maps two ``[B,3,H,W]`` fp32 batches to ``[B,1|2,H,W]`` logits, or to a list / tuple whose last element is that) predicts the
    batch in ``eval()`` mode under ``torch.no_grad()`` and ``frozen_weights``; the previous modes are restored on exit.  One launch
    then turns the K raw outputs into the last model's mask, the agreement of every earlier model with it and, with a ``label``
    (uint8 ``[B,H,W]``, >= 1 is change, 255 is ignored), the confusion matrix of the last model.  One-class models predict change
    where the raw output is above ``threshold`` (0 is the reference's ``sigmoid > 0.5``), two-class models where class 1 wins.
    A ``cm`` passed in (int64 ``[4]`` on the device) is accumulated into.  Everything stays on the device; nothing synchronises."""
    models = _model_list(models)
    dev = _device_of(models, "the self-training round")
    for name, x in (("x1", x1), ("x2", x2)):
        if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 4:
            raise StcdError(f"{name} must be an fp32 [B,C,H,W] tensor")
        if x.device != dev:
            raise StcdError(f"{name} is on {x.device}, the models on {dev}")
    if x1.shape != x2.shape or x1.shape[0] < 1:
        raise StcdError(f"x1 and x2 must share one shape with B >= 1: {tuple(x1.shape)} and {tuple(x2.shape)}")
    B, H, W = int(x1.shape[0]), int(x1.shape[2]), int(x1.shape[3])
    if label is not None:
        if not torch.is_tensor(label) or label.dtype != torch.uint8 or tuple(label.shape) != (B, H, W):
            raise StcdError(f"label must be uint8 [{B},{H},{W}]")
        if label.device != dev:
            raise StcdError(f"label is on {label.device}, the models on {dev}")
    if cm is not None:
        if label is None:
            raise StcdError("cm needs a label")
        if not torch.is_tensor(cm) or cm.dtype != torch.int64 or cm.numel() != 4 or cm.device != dev or not cm.is_contiguous():
            raise StcdError(f"cm must be a contiguous int64 tensor of 4 elements on {dev}")
    if not 1 <= int(mask_value) <= 255:
        raise StcdError(f"mask_value must be in [1, 255], got {mask_value}")
    # everything is checked: from here on the device works
    K = len(models)
    with torch.cuda.device(dev), _evaluating(models):
        outs = []
        for m in models:
            lg = _change_logits(m(x1, x2))
            if not torch.is_tensor(lg) or lg.dim() != 4 or lg.shape[0] != B or lg.shape[1] not in (1, 2) or tuple(lg.shape[2:]) != (H, W):
                got = tuple(lg.shape) if torch.is_tensor(lg) else type(lg).__name__
                raise StcdError(f"a model returned {got} for {B} pairs of {H} x {W}: expected [{B},1|2,{H},{W}]")
            if outs and lg.shape[1] != outs[0].shape[1]:
                raise StcdError("the models differ in their number of classes")
            outs.append(lg.float().contiguous())
        classes = int(outs[0].shape[1])
        lab = None if label is None else label.contiguous()
        mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
        agree = torch.zeros((B, K - 1, 2, 2), dtype=torch.int64, device=dev) if K > 1 else None
        if lab is not None and cm is None:
            cm = torch.zeros(4, dtype=torch.int64, device=dev)
        ptrs = (C.c_void_p * K)(*[o.data_ptr() for o in outs])
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.lib().stcd_selftrain_score(ptrs, K, B, classes, H * W, C.c_float(threshold), _ptr(lab), int(mask_value), _ptr(mask),
                                                   _ptr(agree), _ptr(cm), stream))
    return BatchScore(mask, agree, cm)


# ------------------------------------------------------------------------------------------------ host side: reliability and split
def _agree_array(agree) -> np.ndarray:
    a = np.asarray(agree)
    if a.ndim == 3 and a.shape[-1] == 4:
        a = a.reshape(a.shape[0], a.shape[1], 2, 2)
    if a.ndim != 4 or a.shape[2:] != (2, 2) or not np.issubdtype(a.dtype, np.integer):
        raise StcdError(f"agree must be an integer array [N,K-1,2,2], got {a.dtype} {a.shape}")
    if a.shape[1] < 1:
        raise StcdError("reliability needs at least two models (one earlier checkpoint to compare with the last)")
    return a.astype(np.int64)


def reliability(agree, cumulative: bool = False) -> np.ndarray:
    """float64 ``[N]`` from ``agree`` int64 ``[N,K-1,2,2]`` (``agree[n, i, last, pred_i]``), numpy only.

    ``cumulative=False``: per pair the mean over the K-1 earlier models of ``IoU_1 = a11 / (a11 + a10 + a01)`` of that pair's own
    matrix; an empty union (neither mask holds change) is full agreement, 1.0.  This is the rule of ST++ that the reference's loop
    evidently means, and the library's own specification where the two part.

    ``cumulative=True``: the reference's literal arithmetic.  Its metric object is created once before the loop and never reset
    (train_stcd.py:106; ``addBatch`` only adds), so the IoU it appends at :122 is that of the matrix accumulated over every earlier
    pair and checkpoint in processing order: prefix sums of ``agree``.  0 / 0 is NaN, as there."""
    a = _agree_array(agree)
    N, E = a.shape[:2]
    if cumulative:
        a = np.cumsum(a.reshape(N * E, 2, 2), axis=0).reshape(N, E, 2, 2)
    inter = a[:, :, 1, 1].astype(np.float64)
    union = (a[:, :, 1, 1] + a[:, :, 1, 0] + a[:, :, 0, 1]).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / union
    if not cumulative:
        iou = np.where(union == 0, 1.0, iou)
    total = iou[:, 0].copy()
    for i in range(1, E):                                       # the reference's sum(mIOU): left to right
        total = total + iou[:, i]
    return total / E


def split_reliable(names: Sequence[str], rel) -> Tuple[List[str], List[str]]:
    """Descending reliability, ties in input order (Python's stable ``sort(reverse=True)``, train_stcd.py:127), NaN last in input
    order (own rule: the reference's order is undefined there); the first ``len // 2`` are reliable (:130-134)."""
    names = list(names)
    rel = np.asarray(rel, dtype=np.float64).ravel()
    if rel.shape[0] != len(names):
        raise StcdError(f"{len(names)} names for {rel.shape[0]} reliabilities")
    finite = [i for i in range(len(names)) if not np.isnan(rel[i])]
    finite.sort(key=lambda i: rel[i], reverse=True)
    order = finite + [i for i in range(len(names)) if np.isnan(rel[i])]
    ranked = [names[i] for i in order]
    half = len(ranked) // 2
    return ranked[:half], ranked[half:]


def write_lists(list_dir: str, reliable: Sequence[str], unreliable: Sequence[str]) -> None:
    """``reliable_ids.txt`` and ``unreliable_ids.txt`` under ``list_dir``, one name and a newline per line (train_stcd.py:128-135)."""
    os.makedirs(list_dir, exist_ok=True)
    for fname, ids in (("reliable_ids.txt", reliable), ("unreliable_ids.txt", unreliable)):
        with open(os.path.join(list_dir, fname), "w") as f:
            for name in ids:
                f.write(name + "\n")


# ------------------------------------------------------------------------------------------------ drivers
def _check_names(names, batch: int, seen: set) -> List[str]:
    names = [names] if isinstance(names, str) else list(names)
    if len(names) != batch:
        raise StcdError(f"{len(names)} names for a batch of {batch} pairs")
    for n in names:
        if not isinstance(n, str) or not n:
            raise StcdError(f"a pair's name must be a non-empty string, got {n!r}")
        if n in seen:
            raise StcdError(f"the name {n!r} comes twice")
        seen.add(n)
    return names


def _batch_size(x1) -> int:
    if not torch.is_tensor(x1) or x1.dim() != 4:
        raise StcdError("x1 must be an fp32 [B,C,H,W] tensor")
    return int(x1.shape[0])


def _to_host(parts: List[torch.Tensor]) -> List[np.ndarray]:
    """One copy for tensors of one shape (the usual case), one each otherwise; the only place a driver waits for the device."""
    if not parts:
        return []
    if all(p.shape[1:] == parts[0].shape[1:] for p in parts):
        return [torch.cat(parts).cpu().numpy()]
    return [p.cpu().numpy() for p in parts]


def select_reliable(models, batches: Iterable, list_dir: Optional[str] = None, cumulative: bool = False, threshold: float = 0.0,
                    flush: int = 64) -> Selection:
    """The reliability split of train_stcd.py:96-135 over ``batches``, an iterable of ``(x1, x2, label_or_None, names)`` of any batch
    size (the label is not used).  Every batch is enqueued without a host sync; the agreement counts wait in device buffers and come
    back once per ``flush`` batches.  With ``list_dir`` the two lists are written there."""
    models = _model_list(models)
    if len(models) < 2:
        raise StcdError("the reliability split compares earlier checkpoints with the last: at least two models")
    if int(flush) < 1:
        raise StcdError(f"flush must be >= 1, got {flush}")
    names: List[str] = []
    seen: set = set()
    pending: List[torch.Tensor] = []
    done: List[np.ndarray] = []
    with _evaluating(models):
        for x1, x2, _label, batch_names in batches:
            names += _check_names(batch_names, _batch_size(x1), seen)
            pending.append(score_batch(models, x1, x2, threshold=threshold).agree)
            if len(pending) >= flush:
                done += _to_host(pending)
                pending = []
        done += _to_host(pending)
    K = len(models)
    agree = np.concatenate(done).reshape(-1, K - 1, 2, 2) if done else np.zeros((0, K - 1, 2, 2), np.int64)
    rel = reliability(agree, cumulative) if len(names) else np.zeros(0, np.float64)
    reliable, unreliable = split_reliable(names, rel)
    if list_dir is not None:
        write_lists(list_dir, reliable, unreliable)
    return Selection(reliable, unreliable, names, rel, agree)


def generate_pseudo_labels(model, batches: Iterable, out_dir: Optional[str], threshold: float = 0.0, write: bool = True,
                           flush: int = 64) -> Optional[dict]:
    """The pseudo-label writer of train_stcd.py:137-204 over ``batches`` (as ``select_reliable``): ``model`` predicts every pair, the
    mask times 255 is saved as a mode-``L`` PNG under the pair's own name in ``out_dir`` (``write=False``: scores only), and when
    the batches carry labels the ``scores_from_cm`` of the confusion matrix over all pairs are returned (else None).  The masks
    wait on the device and come back once per ``flush`` batches; the confusion matrix comes back once, at the end."""
    models = _model_list([model])
    if int(flush) < 1:
        raise StcdError(f"flush must be >= 1, got {flush}")
    if write:
        if out_dir is None:
            raise StcdError("out_dir is needed to write the masks")
        from PIL import Image
        os.makedirs(out_dir, exist_ok=True)
    seen: set = set()
    pending: List[torch.Tensor] = []
    pending_names: List[str] = []
    cm = None
    labelled: Optional[bool] = None

    def drain():
        nonlocal pending, pending_names
        at = 0
        for block in _to_host(pending):
            for m in block:                                     # uint8 [H,W]: Pillow's mode L
                Image.fromarray(m).save(os.path.join(out_dir, pending_names[at]), format="PNG")
                at += 1
        pending, pending_names = [], []

    with _evaluating(models):
        for x1, x2, label, batch_names in batches:
            batch_names = _check_names(batch_names, _batch_size(x1), seen)
            if labelled is None:
                labelled = label is not None
            elif labelled != (label is not None):
                raise StcdError("either every batch carries a label or none does")
            res = score_batch(models, x1, x2, label=label, threshold=threshold, mask_value=255, cm=cm)
            cm = res.cm
            if write:
                pending.append(res.mask)
                pending_names += batch_names
                if len(pending) >= flush:
                    drain()
        if write:
            drain()
    if cm is None:
        return None
    return scores_from_cm(cm.cpu().numpy().reshape(2, 2))


# ------------------------------------------------------------------------------------------------ the round on whole scenes
class SceneRound(NamedTuple):
    masks: List[torch.Tensor]           # K uint8 [H,W] on the device: predict_scene's mask of every checkpoint, 1 is change
    pseudo: torch.Tensor                # uint8 [H,W] on the device: the last checkpoint's mask, 0 / 255, closed if close_radius > 0
    agree: Optional[np.ndarray]         # int64 [cells_y,cells_x,K-1,2,2], agree[cy, cx, i, last, pred_i]; None for one model
    reliability: np.ndarray             # float64 [cells_y,cells_x]; all ones for one model
    cell_cm: Optional[np.ndarray]       # int64 [cells_y,cells_x,2,2], cm[cy, cx, label, pseudo] (label given)
    cm: Optional[np.ndarray]            # int64 [2,2]: the sum of cell_cm
    scores: Optional[dict]              # metrics.scores_from_cm(cm)
    names: List[str]                    # f"{stem}_{cy:04d}_{cx:04d}.png" of every cell, row-major
    full: np.ndarray                    # bool [cells_y,cells_x]: the cell is a whole cell x cell square
    reliable: List[str]                 # split_reliable over the full cells only
    unreliable: List[str]
    cell: int                           # the cell edge the grid was cut with
    seg_a: Optional[torch.Tensor] = None    # gate="seg": the last checkpoint's building mask of scene A, uint8 [H,W], else None
    seg_b: Optional[torch.Tensor] = None    # ... of scene B


def cell_grid(height: int, width: int, cell: int) -> Tuple[int, int]:
    """``(cells_y, cells_x) = (ceil(height / cell), ceil(width / cell))``: non-overlapping squares, the last ones cut off at the border."""
    height, width, cell = int(height), int(width), int(cell)
    if height < 0 or width < 0 or cell < 1:
        raise StcdError(f"cell_grid: bad sizes {height} x {width}, cell {cell}")
    return -(-height // cell), -(-width // cell)


def _check_mask(t, name: str, shape=None, dev=None) -> None:
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != 2 or not t.is_cuda or not t.is_contiguous():
        raise StcdError(f"{name} must be a contiguous uint8 [H,W] tensor on the GPU")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise StcdError(f"{name} is {tuple(t.shape)}, expected {tuple(shape)}")
    if dev is not None and t.device != dev:
        raise StcdError(f"{name} is on {t.device}, expected {dev}")


def scene_cell_agree(masks: Sequence[torch.Tensor], cell: int, label: Optional[torch.Tensor] = None, agree: Optional[torch.Tensor] = None,
                     cm: Optional[torch.Tensor] = None) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """One ``stcd_scene_cell_agree`` launch over K (1..8) contiguous uint8 ``[H,W]`` masks on one GPU (non-zero is change; the last
    plays the label): ``(agree, cm)`` on the device, ``agree`` int64 ``[cells_y,cells_x,K-1,2,2]`` (None for one mask) and, with a
    ``label`` (uint8 ``[H,W]``, >= 1 is change, 255 is ignored), ``cm`` int64 ``[cells_y,cells_x,2,2]`` of the last mask.  Buffers
    passed in are added to.  Nothing synchronises."""
    masks = list(masks)
    if not 1 <= len(masks) <= MAX_MODELS:
        raise StcdError(f"between 1 and {MAX_MODELS} masks, got {len(masks)}")
    _check_mask(masks[0], "masks[0]")
    dev, (H, W) = masks[0].device, masks[0].shape
    for k, m in enumerate(masks[1:], 1):
        _check_mask(m, f"masks[{k}]", (H, W), dev)
    cells_y, cells_x = cell_grid(H, W, cell)
    K = len(masks)
    if label is not None:
        _check_mask(label, "label", (H, W), dev)
    elif K == 1:
        raise StcdError("one mask and no label: nothing to compute")
    for name, buf, want, on in (("agree", agree, (cells_y, cells_x, K - 1, 2, 2), K > 1), ("cm", cm, (cells_y, cells_x, 2, 2), label is not None)):
        if buf is None:
            continue
        if not on:
            raise StcdError(f"{name} was passed but there is nothing to count into it")
        if not torch.is_tensor(buf) or buf.dtype != torch.int64 or tuple(buf.shape) != want or buf.device != dev or not buf.is_contiguous():
            raise StcdError(f"{name} must be a contiguous int64 {list(want)} tensor on {dev}")
    with torch.cuda.device(dev):
        if agree is None and K > 1:
            agree = torch.zeros((cells_y, cells_x, K - 1, 2, 2), dtype=torch.int64, device=dev)
        if cm is None and label is not None:
            cm = torch.zeros((cells_y, cells_x, 2, 2), dtype=torch.int64, device=dev)
        ptrs = (C.c_void_p * K)(*[m.data_ptr() for m in masks])
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.lib().stcd_scene_cell_agree(ptrs, K, int(H), int(W), int(cell), cells_x, cells_y, _ptr(label), _ptr(agree), _ptr(cm), stream))
    return agree, cm


def mask_close(mask: torch.Tensor, radius: int = 2, mask_value: int = 255) -> torch.Tensor:
    """One ``stcd_mask_close`` launch: the binary closing of a contiguous uint8 ``[H,W]`` mask on the GPU (non-zero is set) with the
    ``(2 * radius + 1)``-square, ``radius`` in 1..4, as a new tensor holding ``mask_value`` where set.  ``radius=2`` is the
    reference's ``cv2.morphologyEx(img, cv2.MORPH_CLOSE, np.ones((5, 5)))`` (train_stcd.py:186-188)."""
    _check_mask(mask, "mask")
    if not 1 <= int(radius) <= 4:
        raise StcdError(f"radius must be in [1, 4], got {radius}")
    if not 1 <= int(mask_value) <= 255:
        raise StcdError(f"mask_value must be in [1, 255], got {mask_value}")
    H, W = mask.shape
    with torch.cuda.device(mask.device):
        out = torch.empty_like(mask)
        if H and W:                                             # an empty mask has one address for both: nothing to close
            stream = C.c_void_p(torch.cuda.current_stream(mask.device).cuda_stream)
            _lib.check(_lib.lib().stcd_mask_close(_ptr(mask), int(H), int(W), int(radius), int(mask_value), _ptr(out), stream))
    return out


def scene_round(models, scene_a, scene_b, cell: int = 256, tile: int = 256, stride: Optional[int] = None, batch: int = 16,
                window: str = "flat", tta=None, threshold: float = 0.0, close_radius: int = 0, label=None, cumulative: bool = False,
                stem: str = "scene", gate: Optional[str] = None) -> SceneRound:
    """The round of train_stcd.py:96-204 over one pair of whole uint8 ``[H,W,3]`` scenes instead of pre-cut crops.

    Each of the K ``models`` (1..8 modules on one GPU, earlier checkpoints first) goes through ``scene.predict_scene`` alone, in the
    given order, with ``tile``, ``stride``, ``batch``, ``window``, ``tta`` and ``threshold`` as given: ``masks[k]`` is bit-equal to
    ``predict_scene(models[k], ...).mask``.  One ``stcd_scene_cell_agree`` launch then counts, per ``cell`` x ``cell`` square of the
    scene, the agreement of every earlier checkpoint with the last; ``reliability(agree, cumulative)`` runs over the cells in
    row-major order.  ``pseudo`` is the last checkpoint's mask as 0 / 255, closed by ``stcd_mask_close`` if ``close_radius`` > 0
    (2 is the reference's 5 x 5 closing).  With a ``label`` (uint8 ``[H,W]``, >= 1 is change, 255 is ignored) a second launch gives
    the confusion matrix of ``pseudo`` per cell; ``cm`` is their sum and ``scores`` its ``scores_from_cm``.

    ``gate="seg"`` applies the decision-level gate the reference sketches at train_stcd.py:170-176,
    ``min(|pred_B - pred_A|, change_prediction)``: every checkpoint (``SegCD`` / ``FFCTLCD``, three maps per forward) goes through
    ``scene.predict_scene_heads`` instead and ``masks[k]`` is its ``gated = change & (seg_a != seg_b)``; agreement, closing and
    scores then run on those masks as above, and ``seg_a`` / ``seg_b`` hold the last checkpoint's building masks.  ``gate=None``
    is the round without the gate; any other value is an error.

    Cells at the right and bottom edge that are no whole square are scored and reported (``full`` is False there) but never
    listed: ``reliable`` / ``unreliable`` are ``split_reliable`` over the full cells.  The counts come back in one copy.  Every
    argument error is raised before the first launch."""
    from . import scene as _scene

    if gate is not None and gate != "seg":
        raise StcdError(f"unknown gate {gate!r} (None or 'seg')")
    models = _model_list(models)
    dev = _device_of(models)
    a, b = _scene._scene_tensor(scene_a, "scene_a"), _scene._scene_tensor(scene_b, "scene_b")
    if a.shape != b.shape:
        raise StcdError(f"the scenes differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
    H, W = int(a.shape[0]), int(a.shape[1])
    if H < 1 or W < 1:
        raise StcdError(f"an empty scene: {H} x {W}")
    _scene.plan_tiles(H, W, tile, stride)
    _scene.window_table(tile, window)
    _scene.parse_tta(tta)
    if int(batch) < 1:
        raise StcdError(f"batch must be >= 1, got {batch}")
    cells_y, cells_x = cell_grid(H, W, cell)
    cell = int(cell)
    if not 0 <= int(close_radius) <= 4:
        raise StcdError(f"close_radius must be in [0, 4] (0: no closing), got {close_radius}")
    if not isinstance(stem, str) or not stem:
        raise StcdError(f"stem must be a non-empty string, got {stem!r}")
    lab = _label_tensor(label, "label", H, W)
    # everything is checked: from here on the device works
    a, b = a.to(dev).contiguous(), b.to(dev).contiguous()       # once, not once per checkpoint
    lab = None if lab is None else lab.to(dev).contiguous()
    K = len(models)
    seg_a = seg_b = None
    if gate == "seg":
        heads = [_scene.predict_scene_heads(m, a, b, tile=tile, stride=stride, batch=batch, window=window, threshold=threshold, tta=tta)
                 for m in models]
        masks, seg_a, seg_b = [h.gated for h in heads], heads[-1].seg_a, heads[-1].seg_b
    else:
        masks = [predict_scene(m, a, b, tile=tile, stride=stride, batch=batch, window=window, threshold=threshold, tta=tta).mask for m in models]
    agree_dev = scene_cell_agree(masks, cell)[0] if K > 1 else None
    pseudo = mask_close(masks[-1], int(close_radius), 255) if int(close_radius) > 0 else masks[-1] * 255
    cm_dev = scene_cell_agree([pseudo], cell, label=lab)[1] if lab is not None else None
    # the only wait for the device: the counts
    agree = None if agree_dev is None else agree_dev.cpu().numpy().reshape(cells_y, cells_x, K - 1, 2, 2)
    cell_cm = None if cm_dev is None else cm_dev.cpu().numpy().reshape(cells_y, cells_x, 2, 2)
    n = cells_y * cells_x
    rel = reliability(agree.reshape(n, K - 1, 2, 2), cumulative) if K > 1 else np.ones(n, np.float64)
    names = [f"{stem}_{cy:04d}_{cx:04d}.png" for cy in range(cells_y) for cx in range(cells_x)]
    full = np.zeros((cells_y, cells_x), bool)
    full[:H // cell, :W // cell] = True
    listed = [int(i) for i in np.flatnonzero(full)]
    reliable, unreliable = split_reliable([names[i] for i in listed], rel[listed])
    cm = None if cell_cm is None else cell_cm.sum(axis=(0, 1))
    return SceneRound(masks, pseudo, agree, rel.reshape(cells_y, cells_x), cell_cm, cm, None if cm is None else scores_from_cm(cm), names, full,
                      reliable, unreliable, cell, seg_a, seg_b)


def export_cells(round: SceneRound, scene_a, scene_b, root: str, label=None) -> None:
    """The full cells of a ``scene_round`` as the tile set the reference's ``CD_Dataset`` reads (data/dataset.py:169-212, :337-344):
    ``A/<name>`` and ``B/<name>`` (RGB PNG) cut from the uint8 ``[H,W,3]`` scenes, ``pseudo_label/<name>`` (mode L, 0 / 255) from
    ``round.pseudo``, ``label/<name>`` (mode L) when a ``label`` (uint8 ``[H,W]``) is given, and ``list/reliable_ids.txt`` /
    ``list/unreliable_ids.txt``.  A crop is a slice of the tensor where it lives (GPU or CPU) and one copy to the host; the PNG
    encoding is host work.  Partial edge cells are not written."""
    from PIL import Image

    from .scene import _scene_tensor
    a, b = _scene_tensor(scene_a, "scene_a"), _scene_tensor(scene_b, "scene_b")
    H, W = (int(v) for v in round.pseudo.shape)
    if tuple(a.shape) != (H, W, 3) or tuple(b.shape) != (H, W, 3):
        raise StcdError(f"the scenes must be [{H},{W},3] as the round's pseudo-label: {tuple(a.shape)} and {tuple(b.shape)}")
    lab = _label_tensor(label, "label", H, W)
    cell = int(round.cell)
    cells_y, cells_x = cell_grid(H, W, cell)
    if tuple(round.full.shape) != (cells_y, cells_x) or len(round.names) != cells_y * cells_x:
        raise StcdError("the round's cell grid does not fit its pseudo-label")
    layers = [("A", a), ("B", b), ("pseudo_label", round.pseudo)] + ([("label", lab)] if lab is not None else [])
    for sub, _ in layers:
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for cy in range(cells_y):
        for cx in range(cells_x):
            if not round.full[cy, cx]:
                continue
            name = round.names[cy * cells_x + cx]
            for sub, src in layers:
                crop = src[cy * cell:(cy + 1) * cell, cx * cell:(cx + 1) * cell].contiguous().cpu().numpy()
                Image.fromarray(crop).save(os.path.join(root, sub, name), format="PNG")
    write_lists(os.path.join(root, "list"), round.reliable, round.unreliable)


def refine_round(round: SceneRound, min_area: int = 0, max_hole: int = 0, connectivity: int = 8, label=None) -> SceneRound:
    """A ``scene_round`` result with its pseudo-label cleaned at object level: ``pseudo`` becomes
    ``objects.filter_objects(round.pseudo, min_area, max_hole, connectivity, 255)`` (set objects below ``min_area`` pixels are
    cleared, then holes of at most ``max_hole`` pixels off the scene border are filled).  With a ``label`` (uint8 ``[H,W]``, >= 1 is
    change, 255 is ignored) ``cell_cm``, ``cm`` and ``scores`` are counted again from the new pseudo-label by one
    ``stcd_scene_cell_agree`` launch and one copy; without one they are None.  Every other field is carried over, so
    ``export_cells`` works on the result unchanged.  Every argument error is raised before the first launch."""
    from . import objects as _objects

    if not isinstance(round, SceneRound):
        raise StcdError(f"refine_round takes a SceneRound, got {type(round).__name__}")
    _check_mask(round.pseudo, "round.pseudo")
    H, W = (int(v) for v in round.pseudo.shape)
    cells_y, cells_x = cell_grid(H, W, round.cell)
    _objects._check_connectivity(connectivity)
    if int(max_hole) < 0:
        raise StcdError(f"max_hole must be >= 0, got {max_hole}")
    lab = _label_tensor(label, "label", H, W)
    # everything is checked: from here on the device works
    dev = round.pseudo.device
    lab = None if lab is None else lab.to(dev).contiguous()
    pseudo = _objects.filter_objects(round.pseudo, min_area=min_area, max_hole=max_hole, connectivity=connectivity, mask_value=255)
    cell_cm = cm = scores = None
    if lab is not None:
        cell_cm = scene_cell_agree([pseudo], round.cell, label=lab)[1].cpu().numpy().reshape(cells_y, cells_x, 2, 2)
        cm = cell_cm.sum(axis=(0, 1))
        scores = scores_from_cm(cm)
    return round._replace(pseudo=pseudo, cell_cm=cell_cm, cm=cm, scores=scores)
