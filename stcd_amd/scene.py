"""Whole-scene inference: tile two co-registered uint8 scenes, predict, and stitch one change mask -- on the device.

The reference cuts its scenes into 256-pixel crops offline (/root/reference/split.py:17-46), normalises them on the host
(data/dataset.py:499-500) and scores the crops one by one (models/trainer.py:197-203, train_pse_cd.py:361-368); it never
puts a scene back together.  ``predict_scene`` does the whole round on the GPU around the eval forward:
``stcd_scene_gather`` (uint8 HWC scene -> normalised fp32 NCHW tile batch, mirror reflection past the edges),
``model(x1, x2)``, ``stcd_scene_stitch`` (window-weighted sums per scene pixel, no float atomics: bit-reproducible and
independent of the batch split) and ``stcd_scene_finalize`` (mask, optional probability, optional confusion matrix);
see include/stcd_hip.h.  The overlap blend is this library's own specification: the reference has none.

Test-time augmentation over the eight symmetries of the square and checkpoint ensembles are further links of the same chain:
``stcd_scene_gather_d4`` writes a flipped / transposed view of the tiles directly and ``stcd_scene_stitch_d4`` reads the
network's output for that view back through the inverse, so no tile or logit is permuted on the host.

``plan_tiles``, ``window_table`` and ``parse_tta`` are host-only and need no GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._lib import StcdError
from .metrics import scores_from_cm
from .pseudo import MEAN, STD


class TilePlan(NamedTuple):
    tiles_y: int
    tiles_x: int
    n: int
    tile: int
    stride: int


class SceneResult(NamedTuple):
    mask: torch.Tensor                  # uint8 [H,W] on the model's device: 1 is change
    prob: Optional[torch.Tensor]        # fp32 [H,W] (return_prob=True): softmax class 1 / sigmoid of the blended logits
    cm: Optional[np.ndarray]            # int64 [2,2], cm[label, pred] over the non-ignored pixels (label given)
    scores: Optional[dict]              # metrics.scores_from_cm(cm)


def plan_tiles(height: int, width: int, tile: int = 256, stride: Optional[int] = None) -> TilePlan:
    """The regular tile grid of a ``height x width`` scene: ``tiles = max(0, ceil((L - tile) / stride)) + 1`` per axis, tile k at
    origin ``((k // tiles_x) * stride, (k % tiles_x) * stride)``.  The last tiles may reach past the scene."""
    stride = tile if stride is None else stride
    height, width, tile, stride = int(height), int(width), int(tile), int(stride)
    if height < 1 or width < 1 or tile < 1:
        raise StcdError(f"plan_tiles: bad sizes {height} x {width}, tile {tile}")
    if not 1 <= stride <= tile:
        raise StcdError(f"plan_tiles: stride {stride} must be in [1, tile = {tile}] (a larger stride leaves pixels uncovered)")
    ty = max(0, -(-(height - tile) // stride)) + 1
    tx = max(0, -(-(width - tile) // stride)) + 1
    return TilePlan(ty, tx, ty * tx, tile, stride)


def window_table(tile: int, kind: str = "flat") -> np.ndarray:
    """fp32 [tile] per-axis blend weights; a tile pixel weighs ``window[ty] * window[tx]``.  ``hann`` is sampled at the pixel
    centres, so it is strictly positive and every scene pixel ends with ``wsum > 0``."""
    tile = int(tile)
    if tile < 1:
        raise StcdError(f"window_table: bad tile {tile}")
    if kind == "flat":
        return np.ones(tile, np.float32)
    if kind == "hann":
        i = np.arange(tile, dtype=np.float64)
        return (0.5 - 0.5 * np.cos(2.0 * np.pi * (i + 0.5) / tile)).astype(np.float32)
    raise StcdError(f"window_table: unknown window {kind!r} (flat or hann)")


MAX_MODELS = 8                          # STCD_SELFTRAIN_MAX_MODELS of include/stcd_hip.h: an ensemble is at most one self-training round
TTA_VIEWS = {"flip": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}


def parse_tta(tta) -> tuple:
    """The D4 element codes of a ``tta`` argument, in the order they are run: bit 0 mirrors columns, bit 1 mirrors rows, bit 2
    transposes (applied last).  ``None``: ``(0,)``; ``"flip"``: ``(0,1,2,3)``; ``"d4"``: ``(0..7)``; or a non-empty sequence of
    distinct ints in 0..7, kept in the given order."""
    if tta is None:
        return (0,)
    if isinstance(tta, str):
        if tta not in TTA_VIEWS:
            raise StcdError(f"unknown tta {tta!r} (None, 'flip', 'd4' or a sequence of D4 codes in 0..7)")
        return TTA_VIEWS[tta]
    try:
        views = list(tta)
    except TypeError:
        raise StcdError(f"tta must be None, 'flip', 'd4' or a sequence of D4 codes in 0..7, got {tta!r}") from None
    if not views:
        raise StcdError("tta: the view list is empty")
    for d in views:
        if isinstance(d, bool) or not isinstance(d, (int, np.integer)) or not 0 <= int(d) <= 7:
            raise StcdError(f"tta: a view must be an int in 0..7, got {d!r}")
    views = tuple(int(d) for d in views)
    if len(set(views)) != len(views):
        raise StcdError(f"tta: a view is repeated in {views}")
    return views


def _model_list(model) -> list:
    """One module or a non-empty list / tuple of at most MAX_MODELS modules, all on one GPU."""
    models = list(model) if isinstance(model, (list, tuple)) else [model]
    if not 1 <= len(models) <= MAX_MODELS:
        raise StcdError(f"between 1 and {MAX_MODELS} models, got {len(models)}")
    devs = []
    for m in models:
        if not isinstance(m, torch.nn.Module):
            raise StcdError(f"a model must be a torch.nn.Module, got {type(m).__name__}")
        prm = next(iter(m.parameters()), None)
        devs.append(None if prm is None else prm.device)
    if any(d != devs[0] for d in devs):
        raise StcdError(f"the models are on different devices: {[str(d) for d in devs]}")
    if devs[0] is None or devs[0].type != "cuda":
        raise StcdError("predict_scene runs on the GPU: move the model there first (no CPU fallback)")
    return models


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _scene_tensor(scene, name: str) -> torch.Tensor:
    """Checks only: the tensor stays where it is."""
    if isinstance(scene, np.ndarray):
        if scene.dtype != np.uint8:
            raise StcdError(f"{name} must be uint8, got {scene.dtype}")
        scene = torch.from_numpy(np.ascontiguousarray(scene))
    if not torch.is_tensor(scene):
        raise StcdError(f"{name} must be a torch tensor or a numpy array")
    if scene.dtype != torch.uint8:
        raise StcdError(f"{name} must be uint8, got {scene.dtype}")
    if scene.dim() != 3 or scene.shape[-1] != 3:
        raise StcdError(f"{name} must be uint8 [H,W,3], got {tuple(scene.shape)}")
    return scene


def _change_logits(out):
    """The change logits as CDTrainer takes them: the last element of a list / tuple (ChangeFormer's five maps, SegCD's three)."""
    return out[-1] if isinstance(out, (list, tuple)) else out


def predict_scene(model, scene_a, scene_b, tile: int = 256, stride: Optional[int] = None, batch: int = 16, window: str = "flat",
                  label=None, return_prob: bool = False, threshold: float = 0.0, mean: Sequence[float] = MEAN,
                  std: Sequence[float] = STD, tta=None) -> SceneResult:
    """Run ``model`` over two co-registered uint8 ``[H,W,3]`` scenes (torch tensors or numpy arrays) and return one mask.

    The tiles of ``plan_tiles(H, W, tile, stride)`` go through ``model.eval()`` in ascending order, ``batch`` at a time (the last
    batch may be short), under ``torch.no_grad()`` and ``frozen_weights(model)``; the model's previous mode is restored on exit.
    ``model`` is any module on a GPU that maps two ``[n,3,tile,tile]`` fp32 batches to ``[n,1|2,tile,tile]`` logits (or a list /
    tuple whose last element is that).  ``window``: ``flat`` or ``hann`` (``window_table``).  ``label``: optional uint8 ``[H,W]``
    (>= 1 is change, 255 is ignored) -> ``cm`` and ``scores``.  ``threshold`` applies to one-class models, on the blended raw
    output (0 is "sigmoid > 0.5").

    ``tta`` (``parse_tta``): ``None`` is the single upright view, ``"flip"`` the views ``(0,1,2,3)``, ``"d4"`` all eight
    symmetries of the square, or a sequence of distinct D4 codes.  Each view of the tiles is written by the gather, predicted, and
    read back through the inverse by the stitch.  ``model`` may also be a non-empty list or tuple of at most 8 modules (an
    ensemble of checkpoints) on one device that return the same number of classes.  Order: models outermost in the given order,
    then views in the given order, then tile batches ascending.  All of it goes into one ``acc`` / ``wsum`` pair, so the result
    is the ``wsum``-weighted mean of the logits over models, views and overlapping tiles.  The bits depend on that order and on
    nothing else: they are the same on every run and independent of ``batch``.  Every argument error is raised before the first
    launch."""
    from .modules import frozen_weights

    views = parse_tta(tta)
    models = _model_list(model)
    dev = next(iter(models[0].parameters())).device
    a, b = _scene_tensor(scene_a, "scene_a"), _scene_tensor(scene_b, "scene_b")
    if a.shape != b.shape:
        raise StcdError(f"the scenes differ in shape: {tuple(a.shape)} and {tuple(b.shape)}")
    H, W = int(a.shape[0]), int(a.shape[1])
    plan = plan_tiles(H, W, tile, stride)
    if int(batch) < 1:
        raise StcdError(f"batch must be >= 1, got {batch}")
    batch = min(int(batch), plan.n)
    win = window_table(plan.tile, window)
    lab = None
    if label is not None:
        lab = torch.from_numpy(np.ascontiguousarray(label)) if isinstance(label, np.ndarray) else label
        if not torch.is_tensor(lab) or lab.dtype != torch.uint8 or tuple(lab.shape) != (H, W):
            raise StcdError(f"label must be uint8 [{H},{W}]")
    if len(mean) != 3 or len(std) != 3 or min(std) <= 0:
        raise StcdError("mean and std hold three values, std positive")
    # everything is checked: from here on the device works
    a, b = a.to(dev).contiguous(), b.to(dev).contiguous()
    lab = None if lab is None else lab.to(dev).contiguous()
    win = None if window == "flat" else torch.from_numpy(win).to(dev)         # NULL window: all ones

    l = _lib.lib()
    T, S = plan.tile, plan.stride
    m3, s3 = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
    was_training = [m.training for m in models]
    try:
        with torch.cuda.device(dev), torch.no_grad():
            stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            x1 = torch.empty((batch, 3, T, T), dtype=torch.float32, device=dev)       # reused by every batch
            x2 = torch.empty_like(x1)
            acc = wsum = None
            classes = 0
            for m in models:
                m.eval()
                with frozen_weights(m):
                    for d4 in views:
                        for first in range(0, plan.n, batch):
                            n = min(batch, plan.n - first)
                            _lib.check(l.stcd_scene_gather_d4(_ptr(a), _ptr(b), H, W, T, S, plan.tiles_x, first, n, m3, s3, _ptr(x1), _ptr(x2),
                                                              d4, stream))
                            logits = _change_logits(m(x1[:n], x2[:n]))
                            if logits.dim() != 4 or logits.shape[0] != n or logits.shape[1] not in (1, 2) or tuple(logits.shape[2:]) != (T, T):
                                raise StcdError(f"the model returned {tuple(logits.shape)} for {n} tiles of {T} x {T}: expected [{n},1|2,{T},{T}]")
                            if acc is None:
                                classes = int(logits.shape[1])
                                acc = torch.zeros((classes, H, W), dtype=torch.float32, device=dev)
                                wsum = torch.zeros((H, W), dtype=torch.float32, device=dev)
                            elif logits.shape[1] != classes:
                                raise StcdError("the number of classes changed between batches, views or models")
                            logits = logits.float().contiguous()
                            _lib.check(l.stcd_scene_stitch_d4(_ptr(logits), classes, H, W, T, S, plan.tiles_x, plan.tiles_y, first, n,
                                                              _ptr(win), _ptr(acc), _ptr(wsum), d4, stream))
            mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
            prob = torch.empty((H, W), dtype=torch.float32, device=dev) if return_prob else None
            cm = torch.zeros(4, dtype=torch.int64, device=dev) if lab is not None else None
            _lib.check(l.stcd_scene_finalize(_ptr(acc), _ptr(wsum), classes, H, W, C.c_float(threshold), _ptr(lab), _ptr(mask), _ptr(prob),
                                             _ptr(cm), stream))
    finally:
        for m, was in zip(models, was_training):
            m.train(was)
    cm_host = cm.cpu().numpy().reshape(2, 2) if cm is not None else None
    return SceneResult(mask, prob, cm_host, scores_from_cm(cm_host) if cm_host is not None else None)
