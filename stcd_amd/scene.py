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

``predict_scene_heads`` keeps all three maps of ``SegCD`` / ``FFCTLCD`` (``stcd_scene_stitch_heads_d4``, ``stcd_scene_finalize_seg``: the
two building masks, the change mask and the decision-level gate of train_stcd.py:170-176), and ``predict_scene_seg`` runs a
one-input network such as ``UnetSeg`` over one scene (``stcd_scene_gather_one_d4``).

The three entry points share one checker (``_check_args``) and one tile loop (``_stitched``), which always gathers through a
``_d4`` entry (view 0 is the upright one) and stitches through ``stcd_scene_stitch_heads_d4`` with one head or three: the
single-head entries of the header are that kernel with one head, so the bits are theirs.

``plan_tiles``, ``window_table`` and ``parse_tta`` are host-only and need no GPU.
"""
from __future__ import annotations

import contextlib
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
    """A module is one model, anything else is iterated: 1..MAX_MODELS modules.  Where they are is ``_device_of``'s to check."""
    if isinstance(model, torch.nn.Module):
        models = [model]
    else:
        try:
            models = list(model)
        except TypeError:
            raise StcdError(f"a model must be a torch.nn.Module, got {type(model).__name__}") from None
    if not 1 <= len(models) <= MAX_MODELS:
        raise StcdError(f"between 1 and {MAX_MODELS} models, got {len(models)}")
    for m in models:
        if not isinstance(m, torch.nn.Module):
            raise StcdError(f"a model must be a torch.nn.Module, got {type(m).__name__}")
    return models


def _device_of(models, who: str = "predict_scene") -> torch.device:
    """The one GPU that every model's parameters are on; ``who`` is the caller the no-CPU-fallback error names."""
    devs = []
    for m in models:
        prm = next(iter(m.parameters()), None)
        devs.append(None if prm is None else prm.device)
    if any(d != devs[0] for d in devs):
        raise StcdError(f"the models are on different devices: {[str(d) for d in devs]}")
    if devs[0] is None or devs[0].type != "cuda":
        raise StcdError(f"{who} runs on the GPU: move the model there first (no CPU fallback)")
    return devs[0]


@contextlib.contextmanager
def _evaluating(models):
    """eval(), no_grad and frozen_weights for every model; the previous modes come back on exit, also on error."""
    from .modules import frozen_weights
    was = [m.training for m in models]
    try:
        with contextlib.ExitStack() as stack:
            stack.enter_context(torch.no_grad())
            for m in models:
                m.eval()
                stack.enter_context(frozen_weights(m))
            yield
    finally:
        for m, w in zip(models, was):
            m.train(w)


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


def _label_tensor(label, name: str, H: int, W: int) -> Optional[torch.Tensor]:
    """Checks only, as ``_scene_tensor``: None stays None."""
    if label is None:
        return None
    lab = torch.from_numpy(np.ascontiguousarray(label)) if isinstance(label, np.ndarray) else label
    if not torch.is_tensor(lab) or lab.dtype != torch.uint8 or tuple(lab.shape) != (H, W):
        raise StcdError(f"{name} must be uint8 [{H},{W}]")
    return lab


def _tile_args(H: int, W: int, tile, stride, batch, window, mean, std):
    """The checks of the grid, the batch, the window and the normalisation: ``(plan, batch, window table)``."""
    plan = plan_tiles(H, W, tile, stride)
    if int(batch) < 1:
        raise StcdError(f"batch must be >= 1, got {batch}")
    win = window_table(plan.tile, window)
    if len(mean) != 3 or len(std) != 3 or min(std) <= 0:
        raise StcdError("mean and std hold three values, std positive")
    return plan, min(int(batch), plan.n), win


def _check_map(t, n: int, T: int, what: str) -> None:
    if not torch.is_tensor(t) or t.dim() != 4 or t.shape[0] != n or t.shape[1] not in (1, 2) or tuple(t.shape[2:]) != (T, T):
        got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
        raise StcdError(f"the model returned {what}{got} for {n} tiles of {T} x {T}: expected [{n},1|2,{T},{T}]")


def _change_logits(out):
    """The change logits as CDTrainer takes them: the last element of a list / tuple (ChangeFormer's five maps, SegCD's three)."""
    return out[-1] if isinstance(out, (list, tuple)) else out


class _SceneArgs(NamedTuple):
    """The checked arguments of one run; nothing in it is on the device yet."""
    views: tuple
    scenes: list                        # one or two uint8 [H,W,3] tensors
    H: int
    W: int
    plan: TilePlan
    batch: int
    win: Optional[np.ndarray]           # None: the flat window, NULL to the stitch
    labels: list                        # uint8 [H,W] tensors or None, in the order they were given
    models: list
    dev: torch.device
    mean: Sequence[float]
    std: Sequence[float]


def _check_args(model, scenes, labels, tile, stride, batch, window, mean, std, tta) -> _SceneArgs:
    """Every argument check of the three entry points, in one order: ``tta``, the scenes, the tile grid, the labels, the models and,
    last, their device, so that every other error shows without a GPU.  ``scenes`` and ``labels`` are ``(value, name)`` pairs."""
    views = parse_tta(tta)
    scenes = [_scene_tensor(t, name) for t, name in scenes]
    if any(t.shape != scenes[0].shape for t in scenes):
        raise StcdError(f"the scenes differ in shape: {' and '.join(str(tuple(t.shape)) for t in scenes)}")
    H, W = int(scenes[0].shape[0]), int(scenes[0].shape[1])
    plan, batch, win = _tile_args(H, W, tile, stride, batch, window, mean, std)
    labels = [_label_tensor(t, name, H, W) for t, name in labels]
    models = _model_list(model)
    return _SceneArgs(views, scenes, H, W, plan, batch, None if window == "flat" else win, labels, models, _device_of(models), mean, std)


def _on(t: Optional[torch.Tensor], dev) -> Optional[torch.Tensor]:
    return None if t is None else t.to(dev).contiguous()


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _stitched(args: _SceneArgs, n_heads: int, maps_of):
    """The tile loop of every entry point: models outermost in the given order, then views, then the batches of tiles ascending;
    each batch is gathered (one scene or two), predicted and stitched into one ``acc [n_heads*classes,H,W]`` / ``wsum [H,W]`` pair.
    ``maps_of`` turns what a forward returned into its ``n_heads`` maps, or raises.  Returns ``(acc, wsum, classes)``."""
    l = _lib.lib()
    dev, plan, H, W = args.dev, args.plan, args.H, args.W
    T, S = plan.tile, plan.stride
    scenes = [_on(t, dev) for t in args.scenes]
    win = None if args.win is None else torch.from_numpy(args.win).to(dev)
    m3, s3 = (C.c_float * 3)(*args.mean), (C.c_float * 3)(*args.std)
    acc = wsum = None
    classes = 0
    with torch.cuda.device(dev), _evaluating(args.models):
        stream = _stream(dev)
        xs = [torch.empty((args.batch, 3, T, T), dtype=torch.float32, device=dev) for _ in scenes]     # reused by every batch
        for m in args.models:
            for d4 in args.views:
                for first in range(0, plan.n, args.batch):
                    n = min(args.batch, plan.n - first)
                    if len(scenes) == 2:
                        _lib.check(l.stcd_scene_gather_d4(_ptr(scenes[0]), _ptr(scenes[1]), H, W, T, S, plan.tiles_x, first, n, m3, s3,
                                                          _ptr(xs[0]), _ptr(xs[1]), d4, stream))
                    else:
                        _lib.check(l.stcd_scene_gather_one_d4(_ptr(scenes[0]), H, W, T, S, plan.tiles_x, first, n, m3, s3, _ptr(xs[0]), d4,
                                                              stream))
                    maps = maps_of(m(*[x[:n] for x in xs]))
                    for h, t in enumerate(maps):
                        _check_map(t, n, T, f"map {h} as " if n_heads > 1 else "")
                    if len({tuple(t.shape) for t in maps}) != 1:                              # only predict_scene_heads has several
                        raise StcdError(f"the three maps differ in shape: {[tuple(t.shape) for t in maps]}")
                    if acc is None:
                        classes = int(maps[0].shape[1])
                        acc = torch.zeros((n_heads * classes, H, W), dtype=torch.float32, device=dev)
                        wsum = torch.zeros((H, W), dtype=torch.float32, device=dev)
                    elif maps[0].shape[1] != classes:
                        raise StcdError("the number of classes changed between batches, views or models")
                    maps = [t.float().contiguous() for t in maps]
                    ptrs = (C.c_void_p * n_heads)(*[t.data_ptr() for t in maps])
                    _lib.check(l.stcd_scene_stitch_heads_d4(ptrs, n_heads, classes, H, W, T, S, plan.tiles_x, plan.tiles_y, first, n,
                                                            _ptr(win), _ptr(acc), _ptr(wsum), d4, stream))
    return acc, wsum, classes


def _scene_result(args: _SceneArgs, acc, wsum, classes: int, threshold: float, return_prob: bool) -> SceneResult:
    """``stcd_scene_finalize`` over one stitched map: the result of ``predict_scene`` and of ``predict_scene_seg``."""
    dev, H, W = args.dev, args.H, args.W
    lab = _on(args.labels[0], dev)
    with torch.cuda.device(dev):
        mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
        prob = torch.empty((H, W), dtype=torch.float32, device=dev) if return_prob else None
        cm = torch.zeros(4, dtype=torch.int64, device=dev) if lab is not None else None
        _lib.check(_lib.lib().stcd_scene_finalize(_ptr(acc), _ptr(wsum), classes, H, W, C.c_float(threshold), _ptr(lab), _ptr(mask),
                                                  _ptr(prob), _ptr(cm), _stream(dev)))
    cm_host = cm.cpu().numpy().reshape(2, 2) if cm is not None else None
    return SceneResult(mask, prob, cm_host, scores_from_cm(cm_host) if cm_host is not None else None)


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
    launch, the device's last, so that the others show without a GPU."""
    args = _check_args(model, ((scene_a, "scene_a"), (scene_b, "scene_b")), ((label, "label"),), tile, stride, batch, window, mean, std, tta)
    acc, wsum, classes = _stitched(args, 1, lambda out: [_change_logits(out)])
    return _scene_result(args, acc, wsum, classes, threshold, return_prob)


# ------------------------------------------------------------------------------------------------ one scene, and SegCD's three maps
class SceneHeads(NamedTuple):
    seg_a: torch.Tensor                 # uint8 [H,W] on the model's device: 1 is a building in scene A (SegCD's mask_t1)
    seg_b: torch.Tensor                 # ... in scene B (mask_t2)
    change: torch.Tensor                # uint8 [H,W]: predict_scene's mask
    gated: torch.Tensor                 # uint8 [H,W]: change & (seg_a != seg_b), the gate of train_stcd.py:170-176
    prob: Optional[torch.Tensor]        # fp32 [3,H,W] (return_prob=True): seg_a, seg_b, change
    cm: dict                            # int64 [2,2] under "seg_a", "seg_b", "change", "gated" where the label was given
    scores: dict                        # the same keys through metrics.scores_from_cm


HEAD_KEYS = ("seg_a", "seg_b", "change", "gated")


def predict_scene_seg(model, scene, tile: int = 256, stride: Optional[int] = None, batch: int = 16, window: str = "flat", label=None,
                      return_prob: bool = False, threshold: float = 0.0, mean: Sequence[float] = MEAN, std: Sequence[float] = STD,
                      tta=None) -> SceneResult:
    """``predict_scene`` for a one-input network: ``model`` is ``UnetSeg`` (the network train_sup.py:303 pre-trains) or any module on
    a GPU that maps one ``[n,3,tile,tile]`` fp32 batch to ``[n,1|2,tile,tile]`` logits, or a list / tuple of at most 8 of them;
    ``scene`` is one uint8 ``[H,W,3]`` scene.  ``stcd_scene_gather_one_d4`` writes the tiles, the rest is ``predict_scene``'s
    pipeline and contract to the letter: eval mode and ``frozen_weights`` with the previous modes restored on exit, models outermost,
    then views, then tile batches into one ``acc`` / ``wsum`` pair, ``label`` uint8 ``[H,W]`` (>= 1 is set, 255 is ignored), every
    argument error raised before the first launch, no CPU fallback."""
    args = _check_args(model, ((scene, "scene"),), ((label, "label"),), tile, stride, batch, window, mean, std, tta)
    acc, wsum, classes = _stitched(args, 1, lambda out: [out])
    return _scene_result(args, acc, wsum, classes, threshold, return_prob)


def _three_maps(out):
    if not isinstance(out, (list, tuple)) or len(out) != 3:
        got = f"a {type(out).__name__} of {len(out)}" if isinstance(out, (list, tuple)) else (
            f"one tensor {tuple(out.shape)}" if torch.is_tensor(out) else f"a {type(out).__name__}")
        raise StcdError(f"predict_scene_heads needs the three maps (mask_t1, mask_t2, change) of SegCD / FFCTLCD: the model returned {got}")
    return out


def predict_scene_heads(model, scene_a, scene_b, tile: int = 256, stride: Optional[int] = None, batch: int = 16, window: str = "flat",
                        label=None, label_a=None, label_b=None, threshold: float = 0.0, seg_threshold: float = 0.0,
                        return_prob: bool = False, mean: Sequence[float] = MEAN, std: Sequence[float] = STD, tta=None) -> SceneHeads:
    """``predict_scene`` that keeps all three maps of ``SegCD`` / ``FFCTLCD``, ``(mask_t1, mask_t2, change)``
    (decoders/unet/model.py:316-332): every forward must return a tuple or list of exactly three equally shaped
    ``[n,1|2,tile,tile]`` maps; anything else (a bare tensor, BIT's one-element list, ChangeFormer's five) is a ``StcdError``
    naming what came back.  One ``stcd_scene_stitch_heads_d4`` launch per batch adds the three maps into one
    ``acc [3*classes,H,W]`` over one ``wsum``, and one ``stcd_scene_finalize_seg`` turns them into ``seg_a``, ``seg_b``, ``change``
    and ``gated = change & (seg_a != seg_b)``, the decision-level gate of train_stcd.py:170-176.  ``threshold`` applies to the
    change map and ``seg_threshold`` to the two building maps of one-class models.  ``label`` (change), ``label_a`` and
    ``label_b`` (buildings per date) are independent optional uint8 ``[H,W]`` maps (>= 1 is set, 255 is ignored): ``cm`` and
    ``scores`` hold ``"change"`` and ``"gated"`` with ``label``, ``"seg_a"`` with ``label_a``, ``"seg_b"`` with ``label_b``.

    Everything else is ``predict_scene``'s contract (modes, order of models, views and batches, errors before the first launch, no
    CPU fallback), and ``change`` is bit-equal to ``predict_scene(...).mask`` for the same arguments."""
    args = _check_args(model, ((scene_a, "scene_a"), (scene_b, "scene_b")), ((label_a, "label_a"), (label_b, "label_b"), (label, "label")),
                       tile, stride, batch, window, mean, std, tta)
    acc, wsum, classes = _stitched(args, 3, _three_maps)
    dev, H, W = args.dev, args.H, args.W
    labs = [_on(t, dev) for t in args.labels]
    with torch.cuda.device(dev):
        masks = torch.empty((4, H, W), dtype=torch.uint8, device=dev)
        prob = torch.empty((3, H, W), dtype=torch.float32, device=dev) if return_prob else None
        cm = torch.zeros((4, 4), dtype=torch.int64, device=dev) if any(t is not None for t in labs) else None
        _lib.check(_lib.lib().stcd_scene_finalize_seg(_ptr(acc), _ptr(wsum), classes, H, W, C.c_float(seg_threshold), C.c_float(threshold),
                                                      _ptr(labs[0]), _ptr(labs[1]), _ptr(labs[2]), _ptr(masks[0]), _ptr(masks[1]),
                                                      _ptr(masks[2]), _ptr(masks[3]), _ptr(prob), _ptr(cm), _stream(dev)))
    cms = {}
    if cm is not None:
        cm_host = cm.cpu().numpy().reshape(4, 2, 2)
        cms = {key: cm_host[row] for row, key in enumerate(HEAD_KEYS) if labs[min(row, 2)] is not None}
    return SceneHeads(masks[0], masks[1], masks[2], masks[3], prob, cms, {key: scores_from_cm(v) for key, v in cms.items()})
