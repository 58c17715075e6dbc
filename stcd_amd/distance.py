"""Distances on the device: the exact squared Euclidean distance transform of a mask, disc buffers of any radius and boundary scores.

No counterpart in the reference: what ``scipy.ndimage.distance_transform_edt``, ``binary_dilation`` / ``binary_erosion`` with a disc
and a boundary F1 / Hausdorff distance give on the host, behind ``stcd_edt``, ``stcd_mask_buffer`` and ``stcd_boundary_match``
(include/stcd_hip.h; the kernels are stcd_amd/csrc/kernels_edt.hip).  Every function takes contiguous uint8 ``[H,W]`` tensors on the
GPU with ``1 <= H, W <= 16384``, raises ``StcdError`` and has no CPU fallback.  All outputs are integers: tests/edt_spec.py states
them in numpy and the tests ask for equality.

A pixel is set iff its byte is non-zero; pixel (i, j) is a lattice point and ``d2`` the squared distance to the nearest seed inside
the frame, ``NO_SEED`` where the frame holds none.  A transform is four launches whatever the data (three for the column pass, one
row pass whose epilogue writes the plane, the threshold or the match counts).

``nearest_seed`` is the same transform keeping WHICH seed is nearest (the feature transform, ``stcd_edt_nearest``) and
``expand_labels`` Voronoi growth of a label plane read off it (``stcd_edt_gather``); tests/nearest_spec.py states both, ties included:
the smallest column wins, then the smallest row.  ``objects.split_objects`` builds the split of touching objects on them."""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import StcdError
from .selftrain import _check_mask

NO_SEED = 2 ** 30          # d2 where the frame holds no seed; above the largest real value, 2 * 16383**2
DIM_MAX = 16384
MAX_TOLERANCES = 8
COL_CHUNK = 64             # rows per chunk of the column pass (EDT_COL_CHUNK of kernels_edt.hip): where the carried seed rows cross
COL_BLOCK_COLS = 1024      # columns per block of the column pass (EDT_THREADS lanes of EDT_LANE_COLS columns) and per epilogue step of the row pass
ROW_THREADS = 256          # midpoints the row pass deals per step (EDT_THREADS)
ROW_LANE_MAX = 64          # the longest argmin range a lane scans alone (EDT_ROW_LANE_MAX); a wavefront takes longer ones

_SEEDS = {"unset": 0, "set": 1, "boundary": 2}
_OPS = ("dilate", "erode", "close", "open")
_SCRATCH = {}              # (device, bytes) -> scratch tensor: one allocation per scene size, not per call


class BoundaryScores(NamedTuple):
    n_pred: int                         # boundary pixels of the prediction
    n_label: int                        # boundary pixels of the label
    within_pred: Tuple[int, ...]        # per tolerance: those of the prediction within it of the label's boundary
    within_label: Tuple[int, ...]       # per tolerance: those of the label within it of the prediction's boundary
    precision: Tuple[float, ...]        # within_pred / n_pred, 0.0 for no boundary pixel
    recall: Tuple[float, ...]           # within_label / n_label, 0.0 for no boundary pixel
    f1: Tuple[float, ...]
    hausdorff2: int                     # the squared Hausdorff distance of the two boundaries; NO_SEED if exactly one is empty
    counts: torch.Tensor                # int64 [2, 2 + T] on the device: (n, max_d2, within[t]) per side


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check_frame(mask, name="mask"):
    _check_mask(mask, name)
    H, W = (int(v) for v in mask.shape)
    if not (1 <= H <= DIM_MAX and 1 <= W <= DIM_MAX):
        raise StcdError(f"{name} must be [H,W] with 1 <= H, W <= {DIM_MAX}, got {(H, W)}")
    return H, W


def _scratch_for(device, height: int, width: int) -> torch.Tensor:
    nbytes = int(_lib.lib().stcd_edt_scratch_bytes(int(height), int(width)))
    key = (str(device), nbytes)
    t = _SCRATCH.get(key)
    if t is None:
        t = _SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return t


def buffer_q(radius) -> int:
    """The integer the kernels compare with: ``floor(radius**2)``, clamped to ``NO_SEED - 1`` so that "no seed" is within no radius
    (1, 1.5, 2, 7.3 give 1, 2, 4, 53)."""
    try:
        r = float(radius)
    except (TypeError, ValueError):
        raise StcdError(f"radius must be a number >= 0, got {radius!r}") from None
    if not r >= 0.0:
        raise StcdError(f"radius must be >= 0, got {radius!r}")
    v = r * r
    return NO_SEED - 1 if v >= NO_SEED - 1 else int(math.floor(v))


def squared_distance(mask: torch.Tensor, to: str = "unset", ignore: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int32 ``[H,W]`` on the device: the squared distance of every pixel to the nearest seed of ``mask`` inside the frame, exact
    (include/stcd_hip.h, ``stcd_edt``; tests/edt_spec.py is the specification and the device equals it to the bit).  ``to="unset"``
    measures to the nearest zero pixel (``scipy.ndimage.distance_transform_edt(mask)**2``), ``"set"`` to the nearest object pixel,
    ``"boundary"`` to the nearest boundary pixel: a set pixel that is not void with a 4-neighbour inside the frame that is unset and
    not void, ``ignore`` (uint8 ``[H,W]``, with ``to="boundary"`` only) marking void pixels by byte 255.  ``NO_SEED`` everywhere
    when there is no seed.  Nothing synchronises."""
    H, W = _check_frame(mask)
    if to not in _SEEDS:
        raise StcdError(f"to must be 'unset', 'set' or 'boundary', got {to!r}")
    dev = mask.device
    if ignore is not None:
        if to != "boundary":
            raise StcdError("an ignore plane is read with to='boundary' alone")
        _check_mask(ignore, "ignore", (H, W), dev)
    with torch.cuda.device(dev):
        d2 = torch.empty((H, W), dtype=torch.int32, device=dev)
        scratch = _scratch_for(dev, H, W)
        _lib.check(_lib.lib().stcd_edt(_ptr(mask), _ptr(ignore), H, W, _SEEDS[to], _ptr(d2), _ptr(scratch), scratch.numel(), _stream(dev)))
    return d2


def buffer_mask(mask: torch.Tensor, radius, op: str = "dilate", mask_value: int = 255) -> torch.Tensor:
    """A new uint8 mask holding ``mask_value`` where set: ``mask`` dilated, eroded, closed (dilate, then erode) or opened (erode,
    then dilate) by the disc of ``radius`` pixels, any real ``radius >= 0``, as a threshold on the exact distance transform at
    ``buffer_q(radius)`` (include/stcd_hip.h, ``stcd_mask_buffer``): dilation sets a pixel within ``radius`` of a set pixel, erosion
    keeps a pixel farther than ``radius`` from every unset pixel of the frame and does not eat in from the frame edge
    (``scipy.ndimage.binary_dilation`` with the disc, ``binary_erosion(border_value=1)``).  The cost does not depend on the
    radius; radius 0 returns the mask as 0 / ``mask_value``.  Nothing synchronises."""
    H, W = _check_frame(mask)
    q = buffer_q(radius)
    if op not in _OPS:
        raise StcdError(f"op must be one of {_OPS}, got {op!r}")
    if isinstance(mask_value, bool) or not isinstance(mask_value, int) or not 1 <= mask_value <= 255:
        raise StcdError(f"mask_value must be an integer in [1, 255], got {mask_value!r}")
    dev = mask.device
    steps = {"dilate": (1,), "erode": (0,), "close": (1, 0), "open": (0, 1)}[op]       # seeds per half: 1 (set) dilates, 0 (unset) erodes
    with torch.cuda.device(dev):
        scratch = _scratch_for(dev, H, W)
        src = mask
        for seeds in steps:
            out = torch.empty((H, W), dtype=torch.uint8, device=dev)
            _lib.check(_lib.lib().stcd_mask_buffer(_ptr(src), H, W, seeds, q, 1 - seeds, mask_value, _ptr(out), _ptr(scratch), scratch.numel(),
                                                   _stream(dev)))
            src = out
    return out


def _nearest_scratch_for(device, height: int, width: int) -> torch.Tensor:
    nbytes = int(_lib.lib().stcd_edt_nearest_scratch_bytes(int(height), int(width)))
    key = (str(device), nbytes)                                 # the size is stcd_edt's: one buffer serves both
    t = _SCRATCH.get(key)
    if t is None:
        t = _SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return t


def nearest_seed(mask: torch.Tensor, to: str = "set", ignore: Optional[torch.Tensor] = None, return_distance: bool = False):
    """int32 ``[H,W]`` on the device: for every pixel the linear index ``y * W + x`` of the nearest seed of ``mask`` inside the
    frame, the feature transform (``scipy.ndimage.distance_transform_edt(return_indices=True)`` as one plane; include/stcd_hip.h,
    ``stcd_edt_nearest``; tests/nearest_spec.py is the specification and the device equals it to the bit).  Seeds, ``to`` and
    ``ignore`` are ``squared_distance``'s.  Among seeds at the same distance the one in the smallest column wins, then the one in the
    smallest row; a seed's nearest seed is itself; -1 everywhere when there is no seed.  ``index // W`` and ``index % W`` are the
    seed's row and column.  With ``return_distance=True`` the result is ``(index, d2)``, ``d2`` being ``squared_distance``'s plane
    to the bit, out of the same four launches.  Nothing synchronises."""
    H, W = _check_frame(mask)
    if to not in _SEEDS:
        raise StcdError(f"to must be 'unset', 'set' or 'boundary', got {to!r}")
    dev = mask.device
    if ignore is not None:
        if to != "boundary":
            raise StcdError("an ignore plane is read with to='boundary' alone")
        _check_mask(ignore, "ignore", (H, W), dev)
    with torch.cuda.device(dev):
        index = torch.empty((H, W), dtype=torch.int32, device=dev)
        d2 = torch.empty((H, W), dtype=torch.int32, device=dev) if return_distance else None
        scratch = _nearest_scratch_for(dev, H, W)
        _lib.check(_lib.lib().stcd_edt_nearest(_ptr(mask), _ptr(ignore), H, W, _SEEDS[to], _ptr(d2), _ptr(index), _ptr(scratch), scratch.numel(),
                                               _stream(dev)))
    return (index, d2) if return_distance else index


def expand_labels(labels, distance) -> torch.Tensor:
    """A new int32 ``[H,W]`` label plane on the device: every label of ``labels`` (a ``Components`` of ``objects.label_components``,
    or a contiguous int32 ``[H,W]`` tensor on the GPU, 0 the background) grown by ``distance`` pixels without running into another
    label, ``skimage.segmentation.expand_labels``: a background pixel within ``distance`` (``buffer_q(distance)`` in squared
    distance) of a labelled pixel takes the label of the nearest one, under ``nearest_seed``'s tie rule; the other pixels keep what
    they hold (include/stcd_hip.h, ``stcd_edt_gather``).  Distance 0 returns a copy of the labels.  One elementwise pass forms the
    seed bytes, then one transform whose epilogue gathers; nothing synchronises."""
    plane = getattr(labels, "labels", labels)
    if not torch.is_tensor(plane) or plane.dtype != torch.int32 or plane.dim() != 2 or not plane.is_cuda or not plane.is_contiguous():
        raise StcdError("labels must be a Components or a contiguous int32 [H,W] tensor on the GPU")
    H, W = (int(v) for v in plane.shape)
    if not (1 <= H <= DIM_MAX and 1 <= W <= DIM_MAX):
        raise StcdError(f"labels must be [H,W] with 1 <= H, W <= {DIM_MAX}, got {(H, W)}")
    q = buffer_q(distance)
    dev = plane.device
    with torch.cuda.device(dev):
        seeds = (plane != 0).to(torch.uint8)
        out = torch.empty((H, W), dtype=torch.int32, device=dev)
        scratch = _nearest_scratch_for(dev, H, W)
        _lib.check(_lib.lib().stcd_edt_gather(_ptr(seeds), H, W, _SEEDS["set"], q, _ptr(plane), _ptr(out), _ptr(scratch), scratch.numel(),
                                              _stream(dev)))
    return out


def scores_from_counts(counts: np.ndarray):
    """``(precision, recall, f1, hausdorff2)`` from the integer ``counts`` ``[2, 2 + T]``, on the host: tuples per tolerance, an
    empty denominator gives 0.0 as in ``objects.score_tables``."""
    counts = np.asarray(counts, np.int64)
    n0, n1 = int(counts[0, 0]), int(counts[1, 0])
    precision = tuple(int(w) / n0 if n0 else 0.0 for w in counts[0, 2:])
    recall = tuple(int(w) / n1 if n1 else 0.0 for w in counts[1, 2:])
    f1 = tuple(2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(precision, recall))
    return precision, recall, f1, max(int(counts[0, 1]), int(counts[1, 1]))


def boundary_scores(pred: torch.Tensor, label: torch.Tensor, tolerances: Sequence[float] = (2.0,), check: bool = True) -> BoundaryScores:
    """Boundary precision, recall and F1 of ``pred`` against ``label`` at up to 8 ``tolerances`` in pixels, and the squared
    Hausdorff distance of the two boundaries (include/stcd_hip.h, ``stcd_boundary_match``).  The label's byte 255 is void for both
    masks: a void pixel is no boundary pixel and makes none.  A boundary pixel of the prediction counts towards the precision at
    tolerance t if a boundary pixel of the label lies within ``floor(t**2)`` in squared distance, and the reverse for the recall.
    Two transforms on the device, then one host read, of ``counts``.  ``check=False`` synchronises nothing: ``counts`` stays on the
    device, the integer fields are -1 and the float fields NaN; ``scores_from_counts(s.counts.cpu().numpy())`` gives them later."""
    H, W = _check_frame(pred, "pred")
    dev = pred.device
    _check_mask(label, "label", (H, W), dev)
    try:
        qs = [buffer_q(t) for t in tolerances]
    except TypeError:
        raise StcdError(f"tolerances must be a sequence of numbers >= 0, got {tolerances!r}") from None
    if len(qs) > MAX_TOLERANCES:
        raise StcdError(f"at most {MAX_TOLERANCES} tolerances, got {len(qs)}")
    T = len(qs)
    with torch.cuda.device(dev):
        counts = torch.empty((2, 2 + T), dtype=torch.int64, device=dev)
        scratch = _scratch_for(dev, H, W)
        _lib.check(_lib.lib().stcd_boundary_match(_ptr(pred), _ptr(label), H, W, (C.c_int32 * max(T, 1))(*qs), T, _ptr(counts), _ptr(scratch),
                                                  scratch.numel(), _stream(dev)))
        if not check:
            nan = (float("nan"),) * T
            return BoundaryScores(-1, -1, (-1,) * T, (-1,) * T, nan, nan, nan, -1, counts)
        c = counts.cpu().numpy()
    precision, recall, f1, h2 = scores_from_counts(c)
    return BoundaryScores(int(c[0, 0]), int(c[1, 0]), tuple(int(v) for v in c[0, 2:]), tuple(int(v) for v in c[1, 2:]), precision, recall, f1, h2,
                          counts)
