"""Change objects on the device: connected components of a mask, their table, the area / hole filter and object-level scores.

No counterpart in the reference: the pseudo-label cleaning of ``selftrain.mask_close`` (train_stcd.py:186-188) and the scoring of
``metrics.scores_from_cm`` one level up, from pixels to objects.  Every function takes a contiguous uint8 ``[H,W]`` tensor on the
GPU (the checks of ``selftrain._check_mask``), raises ``StcdError`` and has no CPU fallback; the kernels are
stcd_amd/csrc/kernels_objects.hip behind ``stcd_objects_label``, ``stcd_objects_table`` and ``stcd_mask_filter_objects``
(include/stcd_hip.h).  All outputs are integers: tests/objects_spec.py states them in numpy and the tests ask for equality.

``object_rings`` goes on from numbered objects to vector data: the boundary rings of every object with their holes, on the device
(stcd_amd/csrc/kernels_rings.hip behind ``stcd_rings_count`` and ``stcd_rings_write``; tests/rings_spec.py is the specification),
``simplify_rings`` thins them with Douglas-Peucker, still on the device (stcd_amd/csrc/kernels_simplify.hip behind
``stcd_rings_simplify_count`` and ``stcd_rings_simplify_write``; tests/simplify_spec.py is the specification),
``simplify_rings_safe`` does the same and then restores vertices until no two edges conflict and no object has jumped into another's
polygon, and ``ring_conflicts`` says which edges of any ring set conflict (stcd_amd/csrc/kernels_topo.hip behind
``stcd_rings_conflicts`` and ``stcd_rings_safe_begin`` / ``_round`` / ``_write``; tests/topology_spec.py is the specification), and
``rings_to_geojson`` writes either as polygons on the host.  ``convex_hulls`` and ``oriented_boxes`` give every ring its convex hull and
its minimum-area rectangle, on the device (stcd_amd/csrc/kernels_hull.hip behind ``stcd_rings_hull_count``, ``stcd_rings_hull_write`` and
``stcd_rings_boxes``; tests/hull_spec.py is the specification); ``box_shape`` and ``boxes_to_geojson`` read them on the host.  ``rasterize_rings`` goes the other way, from rings to a mask on the
device (stcd_amd/csrc/kernels_raster.hip behind ``stcd_rings_raster``; tests/raster_spec.py is the specification), with the
confusion counts against an overlay in the same pass, and ``geojson_to_rings`` reads polygons back on the host.

``split_objects`` comes before all of that where one component holds several buildings: the distance-transform split, on the device
(``distance.buffer_mask``, ``label_components`` and ``distance.nearest_seed``, then one pass of stcd_amd/csrc/kernels_split.hip behind
``stcd_objects_split_cut``; tests/nearest_spec.py is the specification).
"""
from __future__ import annotations

import ctypes as C
import json
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import StcdError
from .selftrain import _check_mask

TILE = 64               # the tile pass labels TILE x TILE pixels per block (OBJ_TILE of kernels_objects.hip): where the seams lie
SIMPLIFY_WAVE_MAX = 64     # the longest ring one wavefront simplifies (SM_WAVE_MAX of kernels_simplify.hip); a block takes longer ones
SIMPLIFY_LDS_MAX = 2048     # the longest ring whose state the block keeps in LDS (SM_LDS_MAX); above it the state is in global memory
HULL_WAVE_MAX = 64     # the longest ring one wavefront hulls (HL_WAVE_MAX of kernels_hull.hip); a block takes longer ones
HULL_LDS_MAX = 2048     # the longest ring whose hull state the block keeps in LDS (HL_LDS_MAX); above it the state is in global memory
BOX_WAVE_MAX = 64     # the longest hull one wavefront boxes (BX_WAVE_MAX of kernels_hull.hip); the block takes longer ones
BOX_LDS_MAX = 1024     # the longest hull the block holds in LDS (BX_LDS_MAX); above it the vertices are read from global memory
RASTER_SPAN_MAX = 32     # the longest clipped row span of an edge one lane rasterizes alone (RS_SPAN_MAX of kernels_raster.hip); a wavefront strides over longer ones
RASTER_ROW_CHUNK = 1024     # columns of a row a wavefront scans per step with a carried sum (RS_ROW_CHUNK)
TOPO_TILE = 256     # the edges of one grid cell staged in LDS at a time (TP_TILE of kernels_topo.hip); a fuller cell loops over tile pairs
TOPO_CELL = 16     # the default side, in pixels, of the grid cells candidate pairs come from (TP_CELL_DEFAULT)
TOPO_CELLS = (0, 8, 16, 32, 64, 128, 256)     # what ``cell`` may be; 0 stands for TOPO_CELL

_SCRATCH = {}         # (device, bytes) -> scratch tensor: one allocation per scene size, not per call


class Components(NamedTuple):
    labels: torch.Tensor                # int32 [H,W] on the device: 0 background, 1..count in raster order of the first pixel
    count: int


class ObjectTable(NamedTuple):
    area: torch.Tensor                  # int64 [n] on the device
    bbox: torch.Tensor                  # int32 [n,4] on the device: (y0, x0, y1, x1), inclusive
    overlap: Optional[torch.Tensor]     # int64 [n,2] on the device: (pixels not ignored by the overlay, those where it is set)


class Rings(NamedTuple):
    vertices: torch.Tensor              # int32 [V,2] on the device: (y, x) lattice corners, ring after ring, the first not repeated
    offsets: torch.Tensor               # int64 [count+1] on the device: ring r is vertices[offsets[r]:offsets[r + 1]]
    object: torch.Tensor                # int32 [count] on the device: the label of the ring's object
    area2: torch.Tensor                 # int64 [count] on the device: twice the signed area, > 0 outer ring, < 0 hole
    count: int


class RingConflicts(NamedTuple):
    flags: torch.Tensor                 # uint8 [V] on the device: 1 where the edge that starts at this vertex conflicts with another edge
    count: object                       # the number of flagged edges: an int, or an int64 tensor on the device (check=False)


class SafeRings(NamedTuple):
    rings: Rings
    rounds: int                         # rounds that restored something
    restored: int                       # vertices kept beyond plain Douglas-Peucker's
    conflicts: int                      # conflicting edges of ``rings``: 0 for conflict-free input without a round cap


class OrientedBoxes(NamedTuple):
    edge: torch.Tensor                  # int32 [count] on the device: the hull edge the box stands on, -1 for a hull of fewer than 3 vertices
    origin: torch.Tensor                # int32 [count,2] on the device: the edge's first vertex (y, x)
    dir: torch.Tensor                   # int32 [count,2] on the device: the edge vector e = (ey, ex)
    extent: torch.Tensor                # int64 [count,3] on the device: (dmin, dmax, Z), in units of |e| (tests/hull_spec.py, rule 8)
    count: int


class Raster(NamedTuple):
    mask: torch.Tensor                  # uint8 [H,W] on the device
    cm: Optional[torch.Tensor]          # int64 [2,2] on the device, cm[label, pred], None without an overlay


class SplitObjects(NamedTuple):
    mask: torch.Tensor                  # uint8 [H,W] on the device: the mask with its cut pixels cleared
    owner: torch.Tensor                 # int32 [H,W] on the device: the core (1..n_cores) a set pixel belongs to, 0 for unset pixels and orphans
    n_cores: int
    cut_pixels: object                  # an int, or an int64 scalar tensor on the device (check=False)
    orphan_pixels: object               # set pixels with owner 0, likewise


class ObjectScores(NamedTuple):
    n_pred: int                         # predicted objects with at least one counted pixel
    n_label: int                        # labelled objects with at least one counted pixel
    tp_pred: int                        # predicted objects matched by the label
    tp_label: int                       # labelled objects found by the prediction
    precision: float                    # tp_pred / n_pred, 0.0 for no object
    recall: float                       # tp_label / n_label, 0.0 for no object
    f1: float
    pred_table: ObjectTable
    label_table: ObjectTable


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _scratch_for(device, height: int, width: int) -> torch.Tensor:
    nbytes = int(_lib.lib().stcd_objects_scratch_bytes(int(height), int(width)))
    key = (str(device), nbytes)
    t = _SCRATCH.get(key)
    if t is None:
        t = _SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return t


def _check_shape(H: int, W: int) -> None:
    if H * W >= 2 ** 31:
        raise StcdError(f"a scene of {H} x {W} has 2^31 pixels or more: the labels are int32")


def _check_connectivity(connectivity) -> int:
    if connectivity not in (4, 8):
        raise StcdError(f"connectivity must be 4 or 8, got {connectivity!r}")
    return int(connectivity)


def _raise_if_status(status: int, what: str) -> None:
    if status:
        raise StcdError(f"{what}: a find / union loop reached its iteration cap (status {status}); this is a bug in the kernels, not a property of the mask")


def label_components(mask: torch.Tensor, connectivity: int = 8, invert: bool = False) -> Components:
    """The connected components of the non-zero (``invert``: the zero) pixels of ``mask``: int32 labels on the device, 0 for the
    background and 1..count in raster order of each component's first pixel (``scipy.ndimage.label`` with the cross structure for
    4, the full 3 x 3 structure for 8).  Reads back the count and the status word: one copy of 8 bytes."""
    _check_mask(mask, "mask")
    connectivity = _check_connectivity(connectivity)
    H, W = (int(v) for v in mask.shape)
    _check_shape(H, W)
    dev = mask.device
    with torch.cuda.device(dev):
        labels = torch.empty((H, W), dtype=torch.int32, device=dev)
        if H == 0 or W == 0:
            return Components(labels, 0)
        scratch = _scratch_for(dev, H, W)
        tail = scratch[-8:]                                     # the count, then the status word
        _lib.check(_lib.lib().stcd_objects_label(_ptr(mask), H, W, connectivity, 1 if invert else 0, _ptr(labels), _ptr(tail), _ptr(scratch),
                                                 scratch.numel(), _stream(dev)))
        count, status = (int(v) for v in tail.cpu().numpy().view(np.int32))
    _raise_if_status(status, "label_components")
    return Components(labels, count)


def object_table(components: Components, overlay: Optional[torch.Tensor] = None) -> ObjectTable:
    """Area, bounding box and, with an ``overlay`` (uint8 ``[H,W]``, >= 1 is set, 255 is ignored), the overlap counts of every
    component, on the device.  Nothing synchronises."""
    labels, n = components.labels, int(components.count)
    if not torch.is_tensor(labels) or labels.dtype != torch.int32 or labels.dim() != 2 or not labels.is_cuda or not labels.is_contiguous():
        raise StcdError("components.labels must be a contiguous int32 [H,W] tensor on the GPU")
    H, W = (int(v) for v in labels.shape)
    _check_shape(H, W)
    if not 0 <= n <= H * W:
        raise StcdError(f"components.count must be in [0, {H * W}], got {n}")
    dev = labels.device
    if overlay is not None:
        _check_mask(overlay, "overlay", (H, W), dev)
    with torch.cuda.device(dev):
        area = torch.zeros(n, dtype=torch.int64, device=dev)
        bbox = torch.zeros((n, 4), dtype=torch.int32, device=dev)
        overlap = None if overlay is None else torch.zeros((n, 2), dtype=torch.int64, device=dev)
        if n and H and W:
            _lib.check(_lib.lib().stcd_objects_table(_ptr(labels), H, W, n, _ptr(overlay), _ptr(area), _ptr(bbox), _ptr(overlap), _stream(dev)))
    return ObjectTable(area, bbox, overlap)


def filter_objects(mask: torch.Tensor, min_area: int = 0, max_hole: int = 0, connectivity: int = 8, mask_value: int = 255,
                   check: bool = True) -> torch.Tensor:
    """One ``stcd_mask_filter_objects`` call: a new mask holding ``mask_value`` where set.  Step 1 clears every component of
    non-zero pixels with fewer than ``min_area`` pixels (``min_area <= 1``: none); step 2, on that result, sets every component of
    unset pixels (complementary connectivity) of at most ``max_hole`` pixels that touches no scene border (``max_hole == 0``:
    none).  ``check=True`` reads the 4-byte status word afterwards and raises if it is set; ``check=False`` synchronises nothing."""
    _check_mask(mask, "mask")
    connectivity = _check_connectivity(connectivity)
    min_area, max_hole = int(min_area), int(max_hole)
    if max_hole < 0:
        raise StcdError(f"max_hole must be >= 0, got {max_hole}")
    if not 1 <= int(mask_value) <= 255:
        raise StcdError(f"mask_value must be in [1, 255], got {mask_value}")
    H, W = (int(v) for v in mask.shape)
    _check_shape(H, W)
    dev = mask.device
    with torch.cuda.device(dev):
        out = torch.empty_like(mask)
        if H == 0 or W == 0:                                    # an empty mask has one address for both: nothing to filter
            return out
        scratch = _scratch_for(dev, H, W)
        _lib.check(_lib.lib().stcd_mask_filter_objects(_ptr(mask), H, W, connectivity, min(min_area, 2 ** 62), min(max_hole, 2 ** 62),
                                                       int(mask_value), _ptr(out), _ptr(scratch), scratch.numel(), _stream(dev)))
        if check:
            _raise_if_status(int(scratch[-4:].cpu().numpy().view(np.int32)[0]), "filter_objects")
    return out


def split_objects(mask: torch.Tensor, radius, min_core_area: int = 0, connectivity: int = 8, mask_value: int = 255,
                  check: bool = True) -> SplitObjects:
    """The distance-transform split of objects that touch: ``mask`` with a cut of one to two pixels where two buildings that one
    connected component merges meet, on the device (include/stcd_hip.h, ``stcd_objects_split_cut``; tests/nearest_spec.py is the
    specification and the device equals it to the bit).

    1. The cores are ``distance.buffer_mask(mask, radius, "erode")``, the pixels farther than ``radius`` from every unset pixel;
       with ``min_core_area > 0`` cores of fewer pixels are dropped (``filter_objects(core, min_area=min_core_area)``).
    2. The cores and the mask are labelled (``label_components``, ``connectivity``): ``Lc`` with ``n_cores``, and ``L0``.
    3. ``index = distance.nearest_seed(core, "set")``.
    4. The owner of a set pixel ``p`` is ``Lc[index[p]]`` if ``L0[index[p]] == L0[p]``, else 0: an orphan, whose nearest core
       lies in another component or whose component has no core.  Unset pixels have owner 0.
    5. A set pixel with a non-zero owner is cut if its right, down-left, down or down-right neighbour has another non-zero owner.
       Orphans never cut and are never cut: a thin arm of one building that reaches towards another's core stays attached.

    Returns ``SplitObjects(mask, owner, n_cores, cut_pixels, orphan_pixels)``: ``mask`` holds ``mask_value`` where a set pixel
    was not cut.  Of two 8-adjacent pixels with different owners the earlier in raster order is cut, so a component of it (4- or
    8-connected) holds two owners only where orphan pixels join them, and ``label_components``, ``object_rings``,
    ``oriented_boxes`` and ``match_objects`` see one object per core.  Limits: a cut costs area; a single building with a neck
    narrower than ``2 * radius`` is split (``min_core_area`` is the guard); an orphan region that touches two owners keeps them
    joined.  With ``n_cores == 0`` the transform is skipped and ``mask`` is the input as 0 / ``mask_value``, every set pixel an
    orphan.

    Two host reads, the 8 bytes each of the two ``label_components`` calls (count and status word); ``check=True`` adds one, of
    the two counts (16 bytes).  With ``check=False`` ``cut_pixels`` and ``orphan_pixels`` are int64 scalar tensors on the device."""
    from . import distance                                      # distance does not import this module
    H, W = distance._check_frame(mask)
    connectivity = _check_connectivity(connectivity)
    min_core_area = int(min_core_area)
    if min_core_area < 0:
        raise StcdError(f"min_core_area must be >= 0, got {min_core_area}")
    if isinstance(mask_value, bool) or not isinstance(mask_value, int) or not 1 <= mask_value <= 255:
        raise StcdError(f"mask_value must be an integer in [1, 255], got {mask_value!r}")
    dev = mask.device
    with torch.cuda.device(dev):
        core = distance.buffer_mask(mask, radius, "erode")
        if min_core_area > 1:
            core = filter_objects(core, min_area=min_core_area, connectivity=connectivity, check=False)
        cores = label_components(core, connectivity)
        whole = label_components(mask, connectivity)
        if cores.count:
            index = distance.nearest_seed(core, "set")
        else:
            index = torch.full((H, W), -1, dtype=torch.int32, device=dev)
        out = torch.empty((H, W), dtype=torch.uint8, device=dev)
        owner = torch.empty((H, W), dtype=torch.int32, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().stcd_objects_split_cut(_ptr(mask), _ptr(whole.labels), _ptr(cores.labels), _ptr(index), H, W, mask_value, _ptr(out),
                                                     _ptr(owner), _ptr(counts), _stream(dev)))
        if not check:
            return SplitObjects(out, owner, cores.count, counts[0], counts[1])
        cut, orphan = (int(v) for v in counts.cpu().numpy())
    return SplitObjects(out, owner, cores.count, cut, orphan)


def _check_components(components):
    labels, n = components.labels, int(components.count)
    if not torch.is_tensor(labels) or labels.dtype != torch.int32 or labels.dim() != 2 or not labels.is_cuda or not labels.is_contiguous():
        raise StcdError("components.labels must be a contiguous int32 [H,W] tensor on the GPU")
    H, W = (int(v) for v in labels.shape)
    _check_shape(H, W)
    if not 0 <= n <= H * W:
        raise StcdError(f"components.count must be in [0, {H * W}], got {n}")
    return labels, n, H, W


def _ring_scratch_for(device, height: int, width: int, max_corners: int) -> torch.Tensor:
    nbytes = int(_lib.lib().stcd_rings_scratch_bytes(int(height), int(width), int(max_corners)))
    key = (str(device), "rings", nbytes)
    t = _SCRATCH.get(key)
    if t is None:
        t = _SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return t


def object_rings(components: Components, connectivity: int = 8, max_corners: Optional[int] = None) -> Rings:
    """The boundary rings of every object of ``components`` (``label_components``' result, or any int32 label image with its
    largest label as ``count``), on the device: for each object its outer ring (``area2 > 0``) and one ring per hole
    (``area2 < 0``), as corner vertices ``(y, x)`` on the pixel lattice, in raster order of each ring's first vertex (include/stcd_hip.h,
    ``stcd_rings_count`` / ``stcd_rings_write``; tests/rings_spec.py is the specification).  ``connectivity`` decides where two
    diagonal pixels of one object meet: 8 joins them into one ring, 4 keeps them apart; use the connectivity the labels were made
    with (with 4 on labels made with 8 an object can have several outer rings).

    One host read, of ring count, vertex count and status (24 bytes), between the two phases.  ``max_corners`` is the capacity of
    the per-corner scratch, which has to be sized before the vertex count is known: by default a quarter of the pixel count plus
    4096; if the scene has more corners the count phase is repeated once with the exact number (a second host read)."""
    labels, n, H, W = _check_components(components)
    connectivity = _check_connectivity(connectivity)
    dev = labels.device
    bound = 4 * (H + 1) * (W + 1)
    if max_corners is None:
        max_corners = H * W // 4 + 4096
    max_corners = int(max_corners)
    if max_corners < 0:
        raise StcdError(f"max_corners must be >= 0, got {max_corners}")
    max_corners = min(max_corners, bound, 2 ** 31 - 1)
    with torch.cuda.device(dev):
        if n == 0 or H == 0 or W == 0:
            return Rings(torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                         torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), 0)
        counts = torch.empty(3, dtype=torch.int64, device=dev)
        for attempt in range(2):
            scratch = _ring_scratch_for(dev, H, W, max_corners)
            _lib.check(_lib.lib().stcd_rings_count(_ptr(labels), H, W, connectivity, max_corners, _ptr(counts), _ptr(scratch), scratch.numel(),
                                                   _stream(dev)))
            R, V, status = (int(v) for v in counts.cpu().numpy())
            if not status & 4 or attempt == 1:
                break
            if V >= 2 ** 31:
                raise StcdError(f"object_rings: the scene has {V} ring vertices: corner ids are int32")
            max_corners = V
        if status:
            raise StcdError(f"object_rings: the count phase reports status {status} (bit 1 / 2: an iteration cap or an impossible link, "
                            "bit 4: the corner capacity); this is a bug in the kernels, not a property of the labels")
        vertices = torch.empty((V, 2), dtype=torch.int32, device=dev)
        offsets = torch.empty(R + 1, dtype=torch.int64, device=dev)
        obj = torch.empty(R, dtype=torch.int32, device=dev)
        area2 = torch.empty(R, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().stcd_rings_write(_ptr(labels), H, W, connectivity, max_corners, R, V, _ptr(vertices), _ptr(offsets), _ptr(obj),
                                               _ptr(area2), _ptr(scratch), scratch.numel(), _stream(dev)))
    return Rings(vertices, offsets, obj, area2, R)


def simplify_q(tolerance) -> int:
    """The integer the kernels compare with: ``floor(4 * tolerance**2)``, clamped to ``2**31 - 1`` (1.0, 1.5, 2.0 give 4, 9, 16)."""
    t = float(tolerance)
    if not t >= 0.0:
        raise StcdError(f"tolerance must be >= 0, got {tolerance!r}")
    v = 4.0 * t * t
    return 2 ** 31 - 1 if v >= 2 ** 31 - 1 else int(math.floor(v))


def _check_rings(rings):
    vertices, offsets, obj, area2, R = rings.vertices, rings.offsets, rings.object, rings.area2, int(rings.count)
    for t, dtype, name in ((vertices, torch.int32, "vertices"), (offsets, torch.int64, "offsets"), (obj, torch.int32, "object"), (area2, torch.int64, "area2")):
        if not torch.is_tensor(t) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or t.device != vertices.device:
            raise StcdError(f"rings.{name} must be a contiguous {str(dtype).split('.')[-1]} tensor on the GPU, all four on one device")
    if vertices.dim() != 2 or vertices.shape[1] != 2 or R < 0 or tuple(offsets.shape) != (R + 1,) or tuple(obj.shape) != (R,) or tuple(area2.shape) != (R,):
        raise StcdError("rings: vertices must be [V,2], offsets [count+1], object and area2 [count]")
    if vertices.shape[0] >= 2 ** 31 or R >= 2 ** 31:
        raise StcdError("rings: 2^31 vertices or rings and more are not supported")
    return vertices, offsets, obj, R, int(vertices.shape[0])


def simplify_rings(rings: Rings, tolerance: float = 1.5) -> Rings:
    """Douglas-Peucker over every ring of ``rings`` (``object_rings``' result, or any ``Rings`` with int32 ``(y, x)`` vertices in
    ``[0, 16384]``), on the device: a new ``Rings`` with the same ``count``, ``object`` and ring order, every ring a subsequence of
    its input in travel order with the first vertex still first, ``area2`` recomputed from the vertices that remain.  The rule set
    is integer arithmetic on ``simplify_q(tolerance)`` (include/stcd_hip.h, ``stcd_rings_simplify_count`` /
    ``stcd_rings_simplify_write``; tests/simplify_spec.py is the specification and the device equals it to the bit): two anchors per
    ring, the largest distance from the segment first with the lowest index on ties, a triangle at the least, and a ring whose
    simplified area is 0 or has changed its sign is returned whole, so that a hole stays a hole and an outer ring an outer ring.
    ``tolerance`` is in pixels; 0 returns the rings of ``object_rings`` bit for bit.

    Douglas-Peucker does not protect topology: a simplified hole may touch or cross its exterior, and the polygons of two objects
    may overlap by up to the tolerance.  ``simplify_rings_safe`` repairs that, and ``ring_conflicts`` reports it.  Orthogonalising
    building outlines is out of scope.

    One host read, of the new vertex count and a status word (16 bytes), between the two phases."""
    q = simplify_q(tolerance)
    vertices, offsets, obj, R, V = _check_rings(rings)
    dev = vertices.device
    with torch.cuda.device(dev):
        if R == 0:
            return Rings(torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                         torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), 0)
        nbytes = int(_lib.lib().stcd_rings_simplify_scratch_bytes(R, V))
        key = (str(dev), "simplify", nbytes)
        scratch = _SCRATCH.get(key)
        if scratch is None:
            scratch = _SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().stcd_rings_simplify_count(_ptr(vertices), _ptr(offsets), R, V, q, _ptr(counts), _ptr(scratch), scratch.numel(),
                                                        _stream(dev)))
        n_out, status = (int(v) for v in counts.cpu().numpy())
        if status:
            raise StcdError(f"simplify_rings: the count phase reports status {status} (bit 1: a coordinate outside [0, 16384], bit 4: offsets that "
                            "do not ascend from 0 to the vertex count; bit 2: a ring reached its round cap, which is a bug in the kernels, "
                            "not a property of the rings)")
        out_vertices = torch.empty((n_out, 2), dtype=torch.int32, device=dev)
        out_offsets = torch.empty(R + 1, dtype=torch.int64, device=dev)
        out_area2 = torch.empty(R, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().stcd_rings_simplify_write(_ptr(vertices), _ptr(offsets), R, V, q, n_out, _ptr(out_vertices), _ptr(out_offsets),
                                                        _ptr(out_area2), _ptr(scratch), scratch.numel(), _stream(dev)))
    return Rings(out_vertices, out_offsets, obj.clone(), out_area2, R)


_TOPO_STATUS = ("bit 1: a coordinate outside [0, 16384], bit 4: offsets that do not ascend from 0 to the vertex count; bit 2: a ring reached "
                "its round cap, bit 8: a vertex count that is not the device's own, bit 16: the grid's entry capacity, all three bugs in "
                "the kernels or the wrapper, not properties of the rings")


def _check_cell(cell) -> int:
    if cell not in TOPO_CELLS:
        raise StcdError(f"cell must be 0 or one of {TOPO_CELLS[1:]}, got {cell!r}")
    return int(cell)


def _topo_buffers(dev, R: int, V: int, cell: int):
    nbytes = int(_lib.lib().stcd_rings_topo_scratch_bytes(R, V, cell))
    key = (str(dev), "topo", nbytes)
    scratch = _SCRATCH.get(key)
    if scratch is None:
        scratch = _SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return scratch


def _topo_entries(dev, n: int) -> torch.Tensor:
    """The (cell, edge) entries of the grid: a buffer of its own, so that it can grow while the scratch buffer holds a state."""
    key = (str(dev), "topo_entries")
    t = _SCRATCH.get(key)
    if t is None or t.numel() < n:
        t = _SCRATCH[key] = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    return t


def ring_conflicts(rings: Rings, cell: int = 0, check: bool = True) -> RingConflicts:
    """Which edges of ``rings`` (any ``Rings`` with int32 ``(y, x)`` vertices in ``[0, 16384]``: traced, simplified, hulls, foreign)
    conflict with another edge, of the same ring or of another, on the device: ``flags`` is uint8 ``[V]``, 1 where the edge from
    vertex ``k`` of its ring to vertex ``k + 1`` (the last one back to the first) does, ``count`` their number (include/stcd_hip.h,
    ``stcd_rings_conflicts``; tests/topology_spec.py is the specification and the device equals it to the bit).  Proper crossings, a
    vertex inside another edge, collinear overlaps and spikes conflict; two edges that meet at a vertex of both do not, so the rings
    of ``object_rings`` have none.  Known limit: a crossing exactly through a vertex that both rings share is not seen.

    Candidate pairs come from a uniform grid of ``cell`` x ``cell`` pixels (a power of two from 8 to 256, 0 for the default of
    ``TOPO_CELL``); the result does not depend on it.  ``check=True`` reads the counts afterwards (one copy of 64 bytes), repeats the
    call once with the exact capacity if the grid held more entries than the default allows, and raises ``StcdError`` on a status;
    ``count`` is an int.  ``check=False`` reads nothing back: ``count`` is an int64 tensor on the device, -1 where a status was set
    (the flags are then not valid)."""
    cell = _check_cell(cell)
    vertices, offsets, obj, R, V = _check_rings(rings)
    dev = vertices.device
    with torch.cuda.device(dev):
        flags = torch.zeros(V, dtype=torch.uint8, device=dev)
        if R == 0 or V == 0:
            return RingConflicts(flags, 0 if check else torch.zeros((), dtype=torch.int64, device=dev))
        scratch = _topo_buffers(dev, R, V, cell)
        counts = torch.empty(8, dtype=torch.int64, device=dev)
        cap = 4 * V + 4096
        for attempt in range(2):
            entries = _topo_entries(dev, cap)
            _lib.check(_lib.lib().stcd_rings_conflicts(_ptr(vertices), _ptr(offsets), R, V, cell, _ptr(flags), _ptr(counts), _ptr(entries), cap,
                                                       _ptr(scratch), scratch.numel(), _stream(dev)))
            if not check:
                return RingConflicts(flags, counts[4])
            c = [int(v) for v in counts.cpu().numpy()]
            if c[0] != 16 or attempt == 1:
                break
            cap = c[2]
        if c[0]:
            raise StcdError(f"ring_conflicts: status {c[0]} ({_TOPO_STATUS})")
    return RingConflicts(flags, c[4])


def simplify_rings_safe(rings: Rings, tolerance: float = 1.5, max_rounds: Optional[int] = None, cell: int = 0) -> SafeRings:
    """``simplify_rings`` with its topology repaired, on the device: ``SafeRings(rings, rounds, restored, conflicts)``.  Round 0 is
    ``simplify_rings`` itself.  Then, round by round, every current edge that conflicts with another one (``ring_conflicts``' rule) or
    whose pocket is hit -- the closed polygon of the vertices it dropped holds the first vertex of another ring, on its boundary or
    inside -- gets back the dropped vertex Douglas-Peucker would split at next; a ring whose kept area then is 0 or has changed its
    sign gets back all of them; the loop ends with the round that restores nothing (include/stcd_hip.h, ``stcd_rings_safe_begin`` /
    ``_round`` / ``_write``; tests/topology_spec.py is the specification and the device equals it to the bit).  On conflict-free input
    (every ``object_rings`` result) the result has no conflicting edge, and every ring winds round every other ring's first vertex as
    often, mod 2, as in the input: no hole leaves its exterior and no object ends up inside another's polygon.  Where plain
    Douglas-Peucker has no flagged edge the result equals ``simplify_rings`` bit for bit, after round 0 and one detection pass.

    ``rings`` is a ``Rings`` (same count, object and ring order, every ring a subsequence of its input with the first vertex still
    first, ``area2`` recomputed); ``rounds`` counts the rounds that restored something, ``restored`` the vertices kept beyond plain
    Douglas-Peucker's, ``conflicts`` the conflicting edges of the result: 0 unless the input conflicts already (foreign rings: the loop
    still ends) or ``max_rounds`` was reached, after which one more detection pass is made and what stands is returned.  ``cell`` is
    the grid cell of ``ring_conflicts``; the result does not depend on it.  Tolerance 0 returns the input.  Known limit: a crossing
    exactly through a vertex that both rings share is not seen.

    One host read of 64 bytes after round 0 and one per round: the status, the number of restored vertices, which decides whether
    another round follows and sizes it, and the grid's entry count, which sizes its buffer.  Nothing else is copied to the host."""
    q = simplify_q(tolerance)
    cell = _check_cell(cell)
    if max_rounds is not None:
        max_rounds = int(max_rounds)
        if max_rounds < 0:
            raise StcdError(f"max_rounds must be >= 0 or None, got {max_rounds}")
    vertices, offsets, obj, R, V = _check_rings(rings)
    dev = vertices.device
    L = _lib.lib()
    with torch.cuda.device(dev):
        if R == 0 or V == 0:
            return SafeRings(Rings(vertices.clone(), offsets.clone(), obj.clone(), rings.area2.clone(), R), 0, 0, 0)
        if q == 0:
            return SafeRings(Rings(vertices.clone(), offsets.clone(), obj.clone(), rings.area2.clone(), R), 0, 0,
                             ring_conflicts(rings, cell).count)
        scratch = _topo_buffers(dev, R, V, cell)
        counts = torch.empty(8, dtype=torch.int64, device=dev)

        def read(what):
            c = [int(v) for v in counts.cpu().numpy()]
            if c[0] & ~16:
                raise StcdError(f"simplify_rings_safe: {what} reports status {c[0]} ({_TOPO_STATUS})")
            return c

        _lib.check(L.stcd_rings_safe_begin(_ptr(vertices), _ptr(offsets), R, V, q, cell, _ptr(counts), _ptr(scratch), scratch.numel(), _stream(dev)))
        E0 = E = read("round 0")[1]
        cap = 4 * E + 4096
        rounds = 0
        while True:
            restore = max_rounds is None or rounds < max_rounds
            for attempt in range(2):
                entries = _topo_entries(dev, cap)
                _lib.check(L.stcd_rings_safe_round(_ptr(vertices), _ptr(offsets), R, V, cell, E, 1 if restore else 0, _ptr(counts), _ptr(entries), cap,
                                                   _ptr(scratch), scratch.numel(), _stream(dev)))
                c = read(f"round {rounds + 1}")
                if not c[0]:
                    break
                if attempt == 1:
                    raise StcdError(f"simplify_rings_safe: round {rounds + 1} reports status {c[0]} ({_TOPO_STATUS})")
                cap = c[2]                                      # the grid held more entries than the buffer: nothing was restored
            conflicts = c[4]
            if not restore or c[3] == 0:
                break
            E += c[3]
            cap = max(cap, c[2] + 4 * c[3] + 4096)
            rounds += 1
            if rounds > V:
                raise StcdError("simplify_rings_safe: more rounds than vertices; this is a bug in the kernels, not a property of the rings")
        out_vertices = torch.empty((E, 2), dtype=torch.int32, device=dev)
        out_offsets = torch.empty(R + 1, dtype=torch.int64, device=dev)
        out_area2 = torch.empty(R, dtype=torch.int64, device=dev)
        _lib.check(L.stcd_rings_safe_write(_ptr(vertices), _ptr(offsets), R, V, cell, E, _ptr(out_vertices), _ptr(out_offsets), _ptr(out_area2),
                                           _ptr(counts), _ptr(scratch), scratch.numel(), _stream(dev)))
    return SafeRings(Rings(out_vertices, out_offsets, obj.clone(), out_area2, R), rounds, E - E0, conflicts)


def convex_hulls(rings: Rings) -> Rings:
    """The convex hull of every ring of ``rings`` (``object_rings``' result, or any ``Rings`` with int32 ``(y, x)`` vertices in
    ``[0, 16384]``), on the device: a new ``Rings`` with the same ``count``, ``object`` and ring order, every ring the subsequence
    of its input, in input order, of the strict extreme points of the hull of its point set (a vertex collinear with its hull
    neighbours is dropped, a repeated coordinate counts at its lowest index), ``area2`` recomputed from the vertices that remain
    (include/stcd_hip.h, ``stcd_rings_hull_count`` / ``stcd_rings_hull_write``; tests/hull_spec.py is the specification and the
    device equals it to the bit).  For a ring that does not cross itself, every ring of ``object_rings`` among them, the result is
    a strictly convex polygon travelled in the input's direction: a hole's hull keeps ``area2 < 0``, and ``|area2|`` does not
    shrink.  A ring of 0, 1 or 2 distinct points, or all on one line, gives 0, 1 or 2 vertices and ``area2`` 0.  ``rings_to_geojson``,
    ``rasterize_rings`` and ``oriented_boxes`` take the result unchanged.

    A ring that crosses itself (a foreign ring of ``geojson_to_rings``, possibly a ring of ``simplify_rings``, never one of
    ``simplify_rings_safe`` on traced rings) or repeats a hull
    vertex still gives a subsequence that holds its leftmost and rightmost vertex, but which others it holds is unspecified and it
    need not be a convex polygon in travel order: take the hull of the traced rings first, which costs nothing extra.

    One host read, of the hull vertex count and a status word (16 bytes), between the two phases."""
    vertices, offsets, obj, R, V = _check_rings(rings)
    dev = vertices.device
    with torch.cuda.device(dev):
        if R == 0:
            return Rings(torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
                         torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), 0)
        nbytes = int(_lib.lib().stcd_rings_hull_scratch_bytes(R, V))
        key = (str(dev), "hull", nbytes)
        scratch = _SCRATCH.get(key)
        if scratch is None:
            scratch = _SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().stcd_rings_hull_count(_ptr(vertices), _ptr(offsets), R, V, _ptr(counts), _ptr(scratch), scratch.numel(), _stream(dev)))
        n_out, status = (int(v) for v in counts.cpu().numpy())
        if status:
            raise StcdError(f"convex_hulls: the count phase reports status {status} (bit 1: a coordinate outside [0, 16384], bit 4: offsets that "
                            "do not ascend from 0 to the vertex count; bit 2: a ring reached its round cap, which is a bug in the kernels, "
                            "not a property of the rings)")
        out_vertices = torch.empty((n_out, 2), dtype=torch.int32, device=dev)
        out_offsets = torch.empty(R + 1, dtype=torch.int64, device=dev)
        out_area2 = torch.empty(R, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().stcd_rings_hull_write(_ptr(vertices), _ptr(offsets), R, V, n_out, _ptr(out_vertices), _ptr(out_offsets),
                                                    _ptr(out_area2), _ptr(scratch), scratch.numel(), _stream(dev)))
    return Rings(out_vertices, out_offsets, obj.clone(), out_area2, R)


def oriented_boxes(hulls: Rings, check: bool = True) -> OrientedBoxes:
    """The minimum-area rectangle of every ring of ``hulls`` (``convex_hulls``' result), on the device, one launch: the rectangle
    stands on a hull edge, and for every edge the exact integer extents of the hull along and across it are compared as fractions
    in 128 bits, the lowest edge index winning ties (include/stcd_hip.h, ``stcd_rings_boxes``; tests/hull_spec.py is the
    specification and the device equals it to the bit).  Per ring: ``edge``, ``origin`` (that edge's first vertex), ``dir`` (the edge
    vector ``e``) and ``extent = (dmin, dmax, Z)``; ``box_shape`` turns them into corners, width, height and angle on the host.  A
    hull of fewer than 3 vertices gets edge -1 and zeros.  The rules ask for no convexity, so any ``Rings`` is taken, but only a
    convex ring's rectangle is its minimum-area one.

    ``check=True`` reads the 4-byte status word afterwards and raises ``StcdError`` naming the bit (1: a coordinate outside
    ``[0, 16384]``, 4: offsets that do not ascend from 0 to the vertex count); ``check=False`` synchronises nothing."""
    vertices, offsets, obj, R, V = _check_rings(hulls)
    dev = vertices.device
    with torch.cuda.device(dev):
        edge = torch.empty(R, dtype=torch.int32, device=dev)
        origin = torch.empty((R, 2), dtype=torch.int32, device=dev)
        direction = torch.empty((R, 2), dtype=torch.int32, device=dev)
        extent = torch.empty((R, 3), dtype=torch.int64, device=dev)
        if R == 0:
            return OrientedBoxes(edge, origin, direction, extent, 0)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().stcd_rings_boxes(_ptr(vertices), _ptr(offsets), R, V, _ptr(edge), _ptr(origin), _ptr(direction), _ptr(extent),
                                               _ptr(status), _stream(dev)))
        if check:
            st = int(status.cpu().numpy()[0])
            if st:
                raise StcdError(f"oriented_boxes: status {st} (bit 1: a coordinate outside [0, 16384], bit 4: offsets that do not ascend "
                                "from 0 to the vertex count); the boxes are not valid")
    return OrientedBoxes(edge, origin, direction, extent, R)


def _host_array(x, dtype):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype)


def rings_to_geojson(rings, path=None, transform=None, properties: Optional[ObjectTable] = None) -> dict:
    """A GeoJSON ``FeatureCollection`` (a dict; written to ``path`` if given) with one ``Polygon`` per object of ``rings``
    (``object_rings``' result, or the same five fields as numpy arrays or CPU tensors): the outer ring first, then the object's
    holes in stored order, every ring closed by repeating its first vertex, coordinates as ``[x, y]``.  Host side.

    ``transform=(a, b, c, d, e, f)`` maps lattice coordinates to ``x' = a x + b y + c``, ``y' = d x + e y + f``, the usual affine
    geotransform.  In output coordinates read with y pointing up, the stored travel order is RFC 7946's: exterior rings
    counter-clockwise (positive signed area), holes clockwise.  A transform that mirrors (``a e - b d < 0``: the north-up case,
    ``e < 0``) would turn every ring round, so its rings are listed in reverse travel order, the first vertex staying first: the
    exterior is counter-clockwise with and without a transform.  ``properties``, an ``ObjectTable`` of the same
    components, adds ``area``, ``bbox`` and, where present, ``overlap`` to each feature's ``label``.  An object with more than one
    outer ring raises ``StcdError``: that happens only when the labels were made with connectivity 8 and the rings with 4.
    The rings are written as they come: exact pixel outlines from ``object_rings``, thinned ones from ``simplify_rings``
    (Douglas-Peucker on the device), whose result this takes unchanged."""
    vertices = _host_array(rings.vertices, np.int64).reshape(-1, 2)
    offsets = _host_array(rings.offsets, np.int64).reshape(-1)
    obj = _host_array(rings.object, np.int64).reshape(-1)
    area2 = _host_array(rings.area2, np.int64).reshape(-1)
    R = int(rings.count)
    if offsets.shape[0] != R + 1 or obj.shape[0] != R or area2.shape[0] != R or (R and int(offsets[-1]) != vertices.shape[0]):
        raise StcdError("rings_to_geojson: the fields of `rings` do not fit together")
    mirrored = False
    if transform is not None:
        a, b, c, d, e, f = (float(v) for v in transform)
        mirrored = a * e - b * d < 0
    table = None
    if properties is not None:
        table = (_host_array(properties.area, np.int64), _host_array(properties.bbox, np.int64),
                 None if properties.overlap is None else _host_array(properties.overlap, np.int64))
    polygons = {}                                               # label -> [outer ring or None, holes], in order of first appearance
    for r in range(R):
        ring = vertices[offsets[r]:offsets[r + 1]]
        ys, xs = ring[:, 0].tolist(), ring[:, 1].tolist()
        if transform is None:
            coords = [[x, y] for x, y in zip(xs, ys)]
        else:
            coords = [[a * x + b * y + c, d * x + e * y + f] for x, y in zip(xs, ys)]
        if mirrored:
            coords = coords[:1] + coords[:0:-1]
        coords.append(list(coords[0]))
        entry = polygons.setdefault(int(obj[r]), [None, []])
        if area2[r] > 0:
            if entry[0] is not None:
                raise StcdError(f"rings_to_geojson: object {int(obj[r])} has more than one outer ring: the labels and the rings' connectivity disagree")
            entry[0] = coords
        else:
            entry[1].append(coords)
    features = []
    for label in sorted(polygons):
        outer, holes = polygons[label]
        if outer is None:
            raise StcdError(f"rings_to_geojson: object {label} has holes and no outer ring")
        props = {"label": label}
        if table is not None:
            if not 1 <= label <= table[0].shape[0]:
                raise StcdError(f"rings_to_geojson: `properties` has no row for object {label}")
            props["area"] = int(table[0][label - 1])
            props["bbox"] = [int(v) for v in table[1][label - 1]]
            if table[2] is not None:
                props["overlap"] = [int(v) for v in table[2][label - 1]]
        features.append({"type": "Feature", "properties": props, "geometry": {"type": "Polygon", "coordinates": [outer] + holes}})
    collection = {"type": "FeatureCollection", "features": features}
    if path is not None:
        with open(path, "w") as fh:
            json.dump(collection, fh)
    return collection


def box_shape(boxes, rings=None, hulls=None) -> dict:
    """What ``oriented_boxes``' integer columns say, as float64 numpy arrays, on the host (``boxes``: an ``OrientedBoxes``, or the same
    five fields as numpy arrays or CPU tensors).  With ``e = (ey, ex)`` the box's edge vector, ``L = |e|^2`` and ``(dmin, dmax, Z)``
    its extent: ``corners`` ``[R,4,2]`` as ``(y, x)``, ``origin + (d / L) e + (z / L) (ex, -ey)`` for ``(d, z)`` = ``(dmin, 0)``,
    ``(dmax, 0)``, ``(dmax, Z)``, ``(dmin, Z)``; ``width = (dmax - dmin) / sqrt(L)`` along the edge and ``height = |Z| / sqrt(L)``
    across it; ``angle = atan2(ey, ex)`` folded into ``[0, pi)`` (the fold is made on the integers, so an edge along x gives 0.0);
    ``area = (dmax - dmin) |Z| / L``.  With ``rings`` (the rings the hulls were made from, same count): ``rectangularity =
    |area2| / (2 area)``; with ``rings`` and ``hulls``: ``solidity = |area2| / |hull area2|``.  A ring with edge -1 gets NaN in
    every column."""
    R = int(boxes.count)
    edge = _host_array(boxes.edge, np.int64).reshape(-1)
    origin = _host_array(boxes.origin, np.int64).reshape(-1, 2)
    e = _host_array(boxes.dir, np.int64).reshape(-1, 2)
    extent = _host_array(boxes.extent, np.int64).reshape(-1, 3)
    if edge.shape[0] != R or origin.shape[0] != R or e.shape[0] != R or extent.shape[0] != R:
        raise StcdError("box_shape: the fields of `boxes` do not fit together")
    none = edge < 0
    L = np.where(none, 1, e[:, 0] ** 2 + e[:, 1] ** 2).astype(np.float64)
    dmin, dmax, Z = (extent[:, k].astype(np.float64) for k in range(3))
    o, ef = origin.astype(np.float64), e.astype(np.float64)
    nf = np.stack([ef[:, 1], -ef[:, 0]], axis=1)
    corners = np.stack([o + (d / L)[:, None] * ef + (z / L)[:, None] * nf
                        for d, z in ((dmin, np.zeros(R)), (dmax, np.zeros(R)), (dmax, Z), (dmin, Z))], axis=1)
    flip = (e[:, 0] < 0) | ((e[:, 0] == 0) & (e[:, 1] < 0))
    up = np.where(flip[:, None], -e, e).astype(np.float64)
    out = {"corners": corners, "width": (dmax - dmin) / np.sqrt(L), "height": np.abs(Z) / np.sqrt(L), "angle": np.arctan2(up[:, 0], up[:, 1]),
           "area": ((extent[:, 1] - extent[:, 0]) * np.abs(extent[:, 2])).astype(np.float64) / L}
    if hulls is not None and rings is None:
        raise StcdError("box_shape: solidity needs `rings` as well as `hulls`")
    if rings is not None:
        area2 = np.abs(_host_array(rings.area2, np.int64).reshape(-1)).astype(np.float64)
        if area2.shape[0] != R:
            raise StcdError("box_shape: `rings` and `boxes` differ in count")
        with np.errstate(divide="ignore", invalid="ignore"):
            out["rectangularity"] = area2 / (2.0 * out["area"])
            if hulls is not None:
                hull2 = np.abs(_host_array(hulls.area2, np.int64).reshape(-1)).astype(np.float64)
                if hull2.shape[0] != R:
                    raise StcdError("box_shape: `hulls` and `boxes` differ in count")
                out["solidity"] = area2 / hull2
    for v in out.values():
        v[none] = np.nan
    return out


def boxes_to_geojson(boxes, rings, path=None, transform=None, properties: Optional[dict] = None) -> dict:
    """A GeoJSON ``FeatureCollection`` (a dict; written to ``path`` if given) with one rectangle ``Polygon`` per object: the box of
    its outer ring (``rings.area2 > 0``; holes give no box).  ``boxes`` are ``oriented_boxes``' of the hulls of ``rings``, ring for
    ring.  Host side.  ``transform``, the ``[x, y]`` order and the ring closure are ``rings_to_geojson``'s; the exterior is
    counter-clockwise with and without a mirroring transform, decided by the signed area of the four transformed corners (a
    clockwise rectangle is listed in reverse, its first corner staying first).  Each feature's properties hold ``label`` and
    every per-ring column of ``properties``, a ``box_shape`` result for the same boxes (by default ``box_shape(boxes, rings)``:
    ``angle``, ``width``, ``height``, ``area`` and ``rectangularity``; pass ``box_shape(boxes, rings, hulls)`` for ``solidity`` too).
    An object with more than one outer ring, or an outer ring without a box (edge -1), raises ``StcdError``."""
    R = int(boxes.count)
    obj = _host_array(rings.object, np.int64).reshape(-1)
    area2 = _host_array(rings.area2, np.int64).reshape(-1)
    edge = _host_array(boxes.edge, np.int64).reshape(-1)
    if int(rings.count) != R or obj.shape[0] != R or area2.shape[0] != R or edge.shape[0] != R:
        raise StcdError("boxes_to_geojson: `boxes` and `rings` differ in count")
    shape = box_shape(boxes, rings) if properties is None else properties
    corners = np.asarray(shape["corners"], np.float64).reshape(-1, 4, 2)
    if corners.shape[0] != R:
        raise StcdError("boxes_to_geojson: `properties` is not the box_shape of these boxes")
    if transform is not None:
        a, b, c, d, e, f = (float(v) for v in transform)
    features = {}
    for r in range(R):
        if area2[r] <= 0:
            continue
        label = int(obj[r])
        if label in features:
            raise StcdError(f"boxes_to_geojson: object {label} has more than one outer ring: the labels and the rings' connectivity disagree")
        if edge[r] < 0:
            raise StcdError(f"boxes_to_geojson: the outer ring of object {label} has no box")
        coords = [[float(x), float(y)] if transform is None else [a * float(x) + b * float(y) + c, d * float(x) + e * float(y) + f]
                  for y, x in corners[r].tolist()]
        if sum(p[0] * q[1] - q[0] * p[1] for p, q in zip(coords, coords[1:] + coords[:1])) < 0:
            coords = coords[:1] + coords[:0:-1]
        coords.append(list(coords[0]))
        props = {"label": label}
        for name, column in shape.items():
            if name != "corners":
                props[name] = float(column[r])
        features[label] = {"type": "Feature", "properties": props, "geometry": {"type": "Polygon", "coordinates": [coords]}}
    collection = {"type": "FeatureCollection", "features": [features[label] for label in sorted(features)]}
    if path is not None:
        with open(path, "w") as fh:
            json.dump(collection, fh)
    return collection


_RASTER_RULES = {"positive": 0, "evenodd": 1}


def rasterize_rings(rings: Rings, shape, rule: str = "positive", mask_value: int = 255, overlay: Optional[torch.Tensor] = None,
                    check: bool = True) -> Raster:
    """The rings of ``rings`` (``object_rings``' or ``simplify_rings``' result, or any ``Rings`` on the GPU with int32 ``(y, x)``
    vertices in ``[0, 16384]``, ``geojson_to_rings``' among them) back to pixels: a new uint8 mask of ``shape = (H, W)``,
    ``1 <= H, W <= 16384``, holding ``mask_value`` where set, on the device.  Pixel ``(i, j)`` is sampled at its centre; the rule is
    exact integer arithmetic (include/stcd_hip.h, ``stcd_rings_raster``; tests/raster_spec.py is the specification and the device
    equals it to the bit): every edge adds its sign to a delta plane at the first column whose centre is not left of it, a row's
    running sum is the winding number ``w``, and a pixel is set where ``w > 0`` (``rule="positive"``: the union of overlapping
    polygons, holes subtract) or where ``w`` is odd (``rule="evenodd"``: for foreign rings whose orientation means nothing).  Parts
    of a ring beyond the frame are clipped exactly; ``rasterize_rings(object_rings(c), c.labels.shape).mask`` is ``(c.labels > 0) * 255``.
    ``rings.object`` and ``rings.area2`` are not read.

    With an ``overlay`` (uint8 ``[H,W]`` on the same device, >= 1 is set, 255 is ignored) the same pass counts ``cm`` int64
    ``[2,2]``, ``cm[overlay, raster]``, freshly zeroed per call: ``metrics.scores_from_cm(r.cm.cpu().numpy())`` scores the polygons
    against the overlay, and ``cm[0, 1] + cm[1, 0]`` is the number of pixels that differ.  A mask that marks its objects with 255
    is all "ignored" as an overlay: pass ``(mask != 0).to(torch.uint8)``.

    ``check=True`` reads the 4-byte status word afterwards and raises ``StcdError`` naming the bit (1: a coordinate outside
    ``[0, 16384]``, 4: offsets that do not ascend from 0 to the vertex count); ``check=False`` synchronises nothing."""
    vertices, offsets, obj, R, V = _check_rings(rings)
    try:
        H, W = (int(v) for v in shape)
    except (TypeError, ValueError):
        raise StcdError(f"shape must be (height, width), got {shape!r}") from None
    if not (1 <= H <= 16384 and 1 <= W <= 16384):
        raise StcdError(f"shape must lie in [1, 16384] x [1, 16384], got {(H, W)}")
    if rule not in _RASTER_RULES:
        raise StcdError(f"rule must be 'positive' or 'evenodd', got {rule!r}")
    if not 1 <= int(mask_value) <= 255:
        raise StcdError(f"mask_value must be in [1, 255], got {mask_value}")
    dev = vertices.device
    if overlay is not None:
        _check_mask(overlay, "overlay", (H, W), dev)
    with torch.cuda.device(dev):
        mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
        cm = None if overlay is None else torch.zeros((2, 2), dtype=torch.int64, device=dev)
        nbytes = int(_lib.lib().stcd_rings_raster_scratch_bytes(H, W))
        key = (str(dev), "raster", nbytes)
        scratch = _SCRATCH.get(key)
        if scratch is None:
            scratch = _SCRATCH[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(_lib.lib().stcd_rings_raster(_ptr(vertices), _ptr(offsets), R, V, H, W, _RASTER_RULES[rule], int(mask_value), _ptr(overlay),
                                                _ptr(cm), _ptr(mask), _ptr(scratch), scratch.numel(), _stream(dev)))
        if check:
            status = int(scratch[:4].cpu().numpy().view(np.int32)[0])
            if status:
                raise StcdError(f"rasterize_rings: status {status} (bit 1: a coordinate outside [0, 16384], bit 4: offsets that do not ascend "
                                "from 0 to the vertex count); the mask is not valid")
    return Raster(mask, cm)


def _geojson_polygons(doc):
    """``[(properties or None, [polygon, ...])]``, one entry per feature, a polygon being its list of rings."""
    kind = doc.get("type") if isinstance(doc, dict) else None
    if kind == "FeatureCollection":
        features = doc.get("features")
        if not isinstance(features, list):
            raise StcdError("geojson_to_rings: a FeatureCollection needs a list of features")
    elif kind == "Feature":
        features = [doc]
    elif kind in ("Polygon", "MultiPolygon"):
        features = [{"type": "Feature", "properties": None, "geometry": doc}]
    else:
        raise StcdError(f"geojson_to_rings: expected a FeatureCollection, Feature, Polygon or MultiPolygon, got type {kind!r}")
    out = []
    for k, feat in enumerate(features):
        geom = feat.get("geometry") if isinstance(feat, dict) and feat.get("type") == "Feature" else None
        kind = geom.get("type") if isinstance(geom, dict) else None
        if kind == "Polygon":
            polys = [geom.get("coordinates")]
        elif kind == "MultiPolygon":
            polys = geom.get("coordinates")
        else:
            raise StcdError(f"geojson_to_rings: feature {k} holds {kind!r}: only Polygon and MultiPolygon are read (lines and points are out of scope)")
        if not isinstance(polys, list) or not all(isinstance(p, list) for p in polys):
            raise StcdError(f"geojson_to_rings: feature {k} has no coordinate lists")
        out.append((feat.get("properties"), polys))
    return out


def geojson_to_rings(doc_or_path, transform=None, device=None) -> Rings:
    """The host-side inverse of ``rings_to_geojson``: a GeoJSON ``FeatureCollection``, ``Feature``, ``Polygon`` or ``MultiPolygon``
    (a dict, or the path of a file) as a ``Rings``, ready for ``rasterize_rings``.  ``device=None`` returns CPU tensors (which
    ``rings_to_geojson`` accepts), otherwise the tensors are put on ``device``.

    Each ring loses its repeated closing vertex; every coordinate ``[x', y']`` goes back through the inverse of ``transform``
    (the six numbers ``(a, b, c, d, e, f)`` of ``rings_to_geojson``: ``x' = a x + b y + c``, ``y' = d x + e y + f``; singular is an
    error) and is rounded to the pixel lattice as ``floor(v + 1/2)``.  ROUNDING MOVES A FOREIGN VERTEX BY UP TO HALF A PIXEL in x
    and in y; sub-pixel vertices are out of scope, as are lines and points.  The first ring of a polygon becomes an outer ring and
    the others holes: ``area2`` is recomputed with the project's formula (the sum of ``x_t y_h - x_h y_t``, > 0 for an outer
    ring) and a ring whose sign disagrees with its role is reversed with its first vertex kept first, which is exactly what
    undoes ``rings_to_geojson``'s reversal under a north-up transform.  Rings whose rounded ``area2`` is 0 are dropped; a
    coordinate that lands outside ``[0, 16384]`` (or is not finite) raises ``StcdError``.  Rings come in document order: per
    feature, per polygon, the outer ring and then its holes.  ``object`` is the feature's ``properties["label"]`` when every
    feature has a positive integer one, else the feature's index plus 1; the polygons of a ``MultiPolygon`` share it."""
    doc = doc_or_path
    if not isinstance(doc, dict):
        with open(doc_or_path) as fh:
            doc = json.load(fh)
    inv = None
    if transform is not None:
        try:
            a, b, c, d, e, f = (float(v) for v in transform)
        except (TypeError, ValueError):
            raise StcdError(f"geojson_to_rings: transform must be six numbers (a, b, c, d, e, f), got {transform!r}") from None
        det = a * e - b * d
        if not (math.isfinite(det) and det != 0.0 and all(math.isfinite(v) for v in (c, f))):
            raise StcdError(f"geojson_to_rings: the transform {tuple(transform)} is singular")
        inv = (a, b, c, d, e, f, det)
    features = _geojson_polygons(doc)
    labels = []
    for props, _ in features:
        lab = props.get("label") if isinstance(props, dict) else None
        labels.append(lab if isinstance(lab, int) and not isinstance(lab, bool) and 0 < lab < 2 ** 31 else None)
    if any(lab is None for lab in labels):
        labels = list(range(1, len(features) + 1))
    verts, offs, objs, area2 = [], [0], [], []
    for k, (_, polys) in enumerate(features):
        for poly in polys:
            for role, coords in enumerate(poly):
                try:
                    pts = [(float(p[0]), float(p[1])) for p in coords]
                except (TypeError, ValueError, IndexError):
                    raise StcdError(f"geojson_to_rings: feature {k} has a ring that is not a list of [x, y] positions") from None
                if len(pts) > 1 and pts[-1] == pts[0]:
                    pts.pop()
                ring = []
                for x, y in pts:
                    if inv is not None:
                        a, b, c, d, e, f, det = inv
                        x, y = (e * (x - c) - b * (y - f)) / det, (a * (y - f) - d * (x - c)) / det
                    if not (math.isfinite(x) and math.isfinite(y)):
                        raise StcdError(f"geojson_to_rings: feature {k} has a coordinate that is not finite")
                    yi, xi = math.floor(y + 0.5), math.floor(x + 0.5)
                    if not (0 <= yi <= 16384 and 0 <= xi <= 16384):
                        raise StcdError(f"geojson_to_rings: feature {k} has a vertex at (y, x) = ({yi}, {xi}), outside [0, 16384]")
                    ring.append((yi, xi))
                a2 = sum(xt * yh - xh * yt for (yt, xt), (yh, xh) in zip(ring, ring[1:] + ring[:1]))
                if a2 == 0:
                    continue
                if (a2 > 0) != (role == 0):
                    ring, a2 = ring[:1] + ring[:0:-1], -a2
                verts.extend(ring)
                offs.append(len(verts))
                objs.append(labels[k])
                area2.append(a2)
    out = Rings(torch.from_numpy(np.asarray(verts, np.int32).reshape(-1, 2)), torch.from_numpy(np.asarray(offs, np.int64)),
                torch.from_numpy(np.asarray(objs, np.int32)), torch.from_numpy(np.asarray(area2, np.int64)), len(objs))
    if device is not None:
        out = Rings(*(t.to(device) for t in out[:4]), out.count)
    return out


def score_tables(pred_overlap: np.ndarray, label_overlap: np.ndarray, min_overlap: float = 0.5):
    """``(n_pred, n_label, tp_pred, tp_label, precision, recall, f1)`` from the two integer overlap tables ``[n,2]``, on the host: an
    object with no counted pixel is dropped, an object is matched if ``overlap[1] >= min_overlap * overlap[0]``."""
    out = []
    for ov in (pred_overlap, label_overlap):
        ov = np.asarray(ov, np.int64).reshape(-1, 2)
        ov = ov[ov[:, 0] > 0]
        out.append((int(ov.shape[0]), int(np.count_nonzero(ov[:, 1] >= float(min_overlap) * ov[:, 0]))))
    (n_pred, tp_pred), (n_label, tp_label) = out
    precision = tp_pred / n_pred if n_pred else 0.0
    recall = tp_label / n_label if n_label else 0.0
    f1 = 2 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    return n_pred, n_label, tp_pred, tp_label, precision, recall, f1


def match_objects(pred: torch.Tensor, label: torch.Tensor, connectivity: int = 8, min_overlap: float = 0.5) -> ObjectScores:
    """Object-level scores of a predicted mask against a label (uint8 ``[H,W]``, >= 1 is an object pixel, 255 is ignored).  The
    components of ``pred`` are tabled with the label as overlay, the components of the label's object pixels with ``pred`` (as
    0 / 1: a prediction ignores no pixel, whatever byte marks it) as overlay; every decision is then made on the host from the two integer tables (``score_tables``)."""
    _check_mask(pred, "pred")
    _check_mask(label, "label", tuple(pred.shape), pred.device)
    if not 0.0 < float(min_overlap) <= 1.0:
        raise StcdError(f"min_overlap must be in (0, 1], got {min_overlap}")
    with torch.cuda.device(pred.device):
        objects = torch.where(label == 255, torch.zeros_like(label), label)
        pred_table = object_table(label_components(pred, connectivity), overlay=label)
        label_table = object_table(label_components(objects, connectivity), overlay=(pred != 0).to(torch.uint8))
        scores = score_tables(pred_table.overlap.cpu().numpy(), label_table.overlap.cpu().numpy(), min_overlap)
    return ObjectScores(*scores, pred_table, label_table)
