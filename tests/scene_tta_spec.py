"""numpy restatement of the D4 views of the whole-scene kernels (include/stcd_hip.h: stcd_scene_gather_d4 / stcd_scene_stitch_d4)
and of predict_scene's ``tta`` argument, built on tests/scene_spec.py.  Like that module it states the library's own
specification (the reference has no scene tiler and no test-time augmentation); it lives beside the tests.

D4 element code d in 0..7: bit 0 mirrors columns, bit 1 mirrors rows, bit 2 transposes, the transpose applied last."""
import numpy as np

from tests import scene_spec as SP

VIEWS = tuple(range(8))


def d4_apply(x, d):
    """View d of [..., T, T]: Xd[..., i, j] = X[..., p, q] (slicing form)."""
    f = x[..., ::-1, :] if d & 2 else x
    f = f[..., ::-1] if d & 1 else f
    return f.swapaxes(-1, -2) if d & 4 else f


def d4_invert(y, d):
    """The upright array of which y is view d."""
    f = y.swapaxes(-1, -2) if d & 4 else y
    f = f[..., ::-1] if d & 1 else f
    return f[..., ::-1, :] if d & 2 else f


def d4_apply_index(x, d):
    """d4_apply by the index formulas: (a,b) = (j,i) if d & 4 else (i,j); p = T-1-a if d & 2 else a; q = T-1-b if d & 1 else b."""
    T = x.shape[-1]
    i, j = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    a, b = (j, i) if d & 4 else (i, j)
    p = T - 1 - a if d & 2 else a
    q = T - 1 - b if d & 1 else b
    return x[..., p, q]


def d4_invert_index(y, d):
    """d4_invert by the index formulas: upright (p,q) reads Ld[i,j] with a = T-1-p if d & 2 else p, b = T-1-q if d & 1 else q,
    (i,j) = (b,a) if d & 4 else (a,b)."""
    T = y.shape[-1]
    p, q = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    a = T - 1 - p if d & 2 else p
    b = T - 1 - q if d & 1 else q
    i, j = (b, a) if d & 4 else (a, b)
    return y[..., i, j]


def gather_d4(scene, tile, stride, tiles_x, first_tile, n_tiles, mean, std, d):
    """View d of the tiles scene_spec.gather writes."""
    return np.ascontiguousarray(d4_apply(SP.gather(scene, tile, stride, tiles_x, first_tile, n_tiles, mean, std), d))


def stitch_d4(logits_d, height, width, tile, stride, tiles_x, tiles_y, first_tile, window, acc, wsum, d):
    """logits_d are the outputs for view d of the tiles: un-transform, then scene_spec.stitch (weights in upright coordinates)."""
    return SP.stitch(np.ascontiguousarray(d4_invert(logits_d, d)), height, width, tile, stride, tiles_x, tiles_y, first_tile, window, acc, wsum)


# predict_scene's tta argument -> the views it runs, in order
TTA_EXPECTED = [
    (None, (0,)),
    ("flip", (0, 1, 2, 3)),
    ("d4", (0, 1, 2, 3, 4, 5, 6, 7)),
    ([0], (0,)),
    ((5, 0, 3), (5, 0, 3)),
    ([7, 6, 5, 4, 3, 2, 1, 0], (7, 6, 5, 4, 3, 2, 1, 0)),
    (np.array([4, 1]), (4, 1)),
]
TTA_ERRORS = ["D4", "rot90", "", [], (), [0, 0], [1, 2, 1], [8], [-1], [0, 1.5], ["d4"], [True], 3]

# One wrong argument each for predict_scene / predict_scene_seg / predict_scene_heads on 8 x 8 scenes with tile=8, and the word
# its error must hold.  "scene" and "label" stand for each scene and each label argument of the entry point in turn.
BAD_CALLS = [
    (dict(scene=np.zeros((8, 8), np.uint8)), r"\[H,W,3\]"),
    (dict(label=np.zeros((8, 7), np.uint8)), "must be uint8"),
    (dict(label=np.zeros((8, 8), np.int64)), "must be uint8"),
    (dict(stride=9), "stride"),
    (dict(window="hamming"), "window"),
    (dict(batch=0), "batch"),
    (dict(mean=(0.5, 0.5)), "mean"),
    (dict(tta="rot90"), "tta"),
]


def check_argument_errors(fn, model, meta_model, scene_names, label_names):
    """Every BAD_CALLS entry through ``fn`` with ``model``, a module on the CPU: the error names the wrong argument, not the
    device, although the device is wrong too.  Then a valid call ends at the device, and ``[model, meta_model]`` at the two devices."""
    import pytest

    from stcd_amd._lib import StcdError

    def call(models, **kw):
        return fn(models, **{**{name: np.zeros((8, 8, 3), np.uint8) for name in scene_names}, "tile": 8, **kw})

    for kw, word in BAD_CALLS:
        if "scene" in kw:
            cases = [({name: kw["scene"]}, word) for name in scene_names]
        elif "label" in kw:
            cases = [({name: kw["label"]}, name + " " + word) for name in label_names]
        else:
            cases = [(kw, word)]
        for case, want in cases:
            with pytest.raises(StcdError, match=want) as e:
                call(model, **case)
            assert "GPU" not in str(e.value), (case, str(e.value))
    with pytest.raises(StcdError, match="GPU"):
        call(model)
    with pytest.raises(StcdError, match="different devices"):
        call([model, meta_model])
