"""The self-training round on whole scenes, the part that needs no GPU: the two C-ABI entries exist and refuse bad arguments before
any HIP call, the specification of tests/scene_round_spec.py (plain loops) equals scipy's closing with OpenCV's border rule and
tests/selftrain_spec.py's counts, scene_round's host logic (names, full cells, the split over full cells only, one model) holds with
predict_scene and the two launches replaced by the specification, and export_cells writes what CD_Dataset reads."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from stcd_amd import _lib
from stcd_amd import selftrain as ST
from stcd_amd.metrics import scores_from_cm
from tests import scene_round_spec as RS
from tests import selftrain_spec as SP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_declared_bound_and_exported():
    hdr = open(os.path.join(REPO, "include", "stcd_hip.h")).read()
    declared = set(re.findall(r"\b(stcd_[a-z0-9_]+)\s*\(", hdr))
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("stcd_scene_cell_agree", "stcd_mask_close"):
        assert name in declared and name in _lib.EXPORTS and hasattr(raw, name)
    assert "train_stcd.py:118-125" in hdr and "train_stcd.py:186-188" in hdr     # what they replace
    assert _lib.lib().stcd_abi_version() == 2                                   # additions only


# ------------------------------------------------------------------------------------------------ the C entries' argument checks
def _agree_call(masks="ok", n_models=2, height=10, width=12, cell=4, cells_x=3, cells_y=3, label=False, agree="auto", cm=False):
    """Calls the entry with HOST buffers: every case here is refused (or has nothing to launch) before any HIP call."""
    bufs = [np.zeros(256, np.uint8) for _ in range(9)]
    keep = [np.zeros(256, np.uint8), np.zeros(9 * 8 * 4, np.int64), np.zeros(9 * 4, np.int64)]
    ptrs = (C.c_void_p * 9)(*[b.ctypes.data for b in bufs])
    if masks == "hole":
        ptrs[1] = None
    vp = lambda on, a: C.c_void_p(a.ctypes.data) if on else None
    if agree == "auto":
        agree = n_models != 1
    rc = _lib.lib().stcd_scene_cell_agree(None if masks is None else ptrs, n_models, height, width, cell, cells_x, cells_y, vp(label, keep[0]),
                                          vp(agree, keep[1]), vp(cm, keep[2]), None)
    return rc, _lib.lib().stcd_last_error().decode()


@pytest.mark.parametrize("kw", [dict(masks=None), dict(masks="hole"), dict(n_models=0), dict(n_models=9), dict(n_models=-1), dict(cells_x=4), dict(cells_x=2),
                                dict(cells_y=2), dict(cells_y=4), dict(cell=0), dict(cell=-4), dict(label=True), dict(cm=True), dict(n_models=1),
                                dict(n_models=1, agree=True, label=True, cm=True), dict(agree=False), dict(height=-1), dict(width=-1)])
def test_cell_agree_refuses_bad_arguments_before_any_hip_call(kw):
    rc, err = _agree_call(**kw)
    assert rc != 0, kw
    assert err.startswith("stcd_scene_cell_agree: "), err


@pytest.mark.parametrize("kw", [dict(height=0, cells_y=0), dict(width=0, cells_x=0), dict(height=0, cells_y=0, n_models=1, label=True, cm=True),
                                dict(height=0, width=0, cells_x=0, cells_y=0, n_models=8)])
def test_cell_agree_launches_nothing_for_an_empty_scene(kw):
    rc, err = _agree_call(**kw)
    assert rc == 0, err


def _close_call(height=8, width=8, radius=2, mask_value=255, inp=0, out=64, null=None):
    buf = np.zeros(256, np.uint8)
    base = buf.ctypes.data
    a = None if null == "in" else C.c_void_p(base + inp)
    b = None if null == "out" else C.c_void_p(base + out)
    rc = _lib.lib().stcd_mask_close(a, height, width, radius, mask_value, b, None)
    return rc, _lib.lib().stcd_last_error().decode()


@pytest.mark.parametrize("kw", [dict(radius=0), dict(radius=5), dict(radius=-1), dict(mask_value=0), dict(mask_value=256), dict(out=0), dict(out=63),
                                dict(out=1), dict(inp=63, out=0), dict(inp=100, out=37), dict(null="in"), dict(null="out"), dict(height=-1), dict(width=-1)])
def test_mask_close_refuses_bad_arguments_before_any_hip_call(kw):
    rc, err = _close_call(**kw)
    assert rc != 0, kw
    assert err.startswith("stcd_mask_close: "), err


def test_mask_close_launches_nothing_for_an_empty_mask():
    for kw in (dict(height=0), dict(width=0)):
        rc, err = _close_call(**kw)
        assert rc == 0, err


# ------------------------------------------------------------------------------------------------ the specification of the closing
def _random_masks():
    rng = np.random.default_rng(5)
    shapes = [(1, 1), (1, 9), (7, 1), (3, 3), (5, 30), (17, 12), (33, 47)]
    for n, (h, w) in enumerate(shapes * 2):
        for radius in (1, 2, 3, 4):
            dens = (0.02, 0.3, 0.7)[(n + radius) % 3]
            yield (rng.random((h, w)) < dens).astype(np.uint8) * np.uint8((1, 7, 255)[n % 3]), radius


def test_spec_closing_is_scipys_with_the_opencv_border_rule():
    ndi = pytest.importorskip("scipy.ndimage")
    for m, radius in _random_masks():
        k = np.ones((2 * radius + 1, 2 * radius + 1), bool)
        want = ndi.binary_erosion(ndi.binary_dilation(m != 0, k, border_value=0), k, border_value=1)
        np.testing.assert_array_equal(RS.close(m, radius), want.astype(np.uint8))


def test_spec_closing_is_the_max_pool_composition_and_its_fast_form():
    import torch.nn.functional as F
    for m, radius in _random_masks():
        k = 2 * radius + 1
        x = torch.from_numpy((m != 0).astype(np.float32))[None, None]
        want = -F.max_pool2d(-F.max_pool2d(x, k, 1, radius), k, 1, radius)          # max_pool2d pads with -inf: outside never contributes
        np.testing.assert_array_equal(RS.close(m, radius, 255), want[0, 0].numpy().astype(np.uint8) * 255)
        np.testing.assert_array_equal(RS.close_fast(m, radius, 255), RS.close(m, radius, 255))


def test_spec_closing_is_extensive_and_idempotent():
    for m, radius in _random_masks():
        once = RS.close(m, radius)
        assert set(np.unique(once)) <= {0, 1}
        assert (once >= (m != 0)).all()                                            # extensive: nothing set is lost
        np.testing.assert_array_equal(RS.close(once, radius), once)                # idempotent


def test_spec_closing_structured_cases():
    for radius in (1, 2, 3, 4):
        for shape in ((1, 1), (4, 9), (12, 12)):
            np.testing.assert_array_equal(RS.close(np.zeros(shape, np.uint8), radius, 255), np.zeros(shape, np.uint8))
            np.testing.assert_array_equal(RS.close(np.full(shape, 3, np.uint8), radius, 255), np.full(shape, 255, np.uint8))
        corner = np.zeros((9, 11), np.uint8)
        corner[0, 0] = 1
        np.testing.assert_array_equal(RS.close(corner, radius), corner)             # a single pixel at (0,0) stays alone
    for a, b, bridged in ((15, 20, True), (15, 21, False)):
        m = np.zeros((9, 40), np.uint8)
        m[4, a] = m[4, b] = 1
        got = RS.close(m, 2)
        want = m.copy()
        if bridged:
            want[4, a:b + 1] = 1                                                    # a gap of 4 <= 2 r: filled; of 5: not
        np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------------------------------------ the specification of the counts
@pytest.mark.parametrize("H,W,cell", [(1, 1, 1), (5, 7, 4), (33, 47, 16), (64, 64, 64), (40, 24, 8)])
def test_spec_counts_sum_to_the_whole_scene_and_to_the_cells_pixels(H, W, cell):
    rng = np.random.default_rng(H * W + cell)
    K = 3
    masks = [rng.choice(np.array([0, 1, 7, 255], np.uint8), size=(H, W)) for _ in range(K)]
    label = rng.choice(np.array([0, 1, 7, 255], np.uint8), size=(H, W))
    agree, cm = RS.cell_agree(masks, cell, label)
    cells_y, cells_x = RS.grid(H, W, cell)
    assert agree.shape == (cells_y * cells_x, K - 1, 4) and cm.shape == (cells_y * cells_x, 4)
    logits = [np.where(m.reshape(1, 1, -1) != 0, 1.0, -1.0).astype(np.float32) for m in masks]
    _, whole_agree, whole_cm = SP.score(logits, 0.0, label.reshape(1, -1))
    np.testing.assert_array_equal(agree.sum(0), whole_agree[0])
    np.testing.assert_array_equal(cm.sum(0), whole_cm)
    pixels = RS.cell_pixels(H, W, cell)
    assert pixels.sum() == H * W
    np.testing.assert_array_equal(agree.sum(-1), np.repeat(pixels[:, None], K - 1, 1))       # each cell's four counts: its real pixels
    assert (cm.sum(-1) <= pixels).all() and cm.sum() == (label != 255).sum()
    assert RS.cell_agree(masks[-1:], cell)[0] is None and RS.cell_agree(masks[-1:], cell, label)[1].sum() == (label != 255).sum()
    assert RS.full_cells(H, W, cell).sum() == (H // cell) * (W // cell)
    np.testing.assert_array_equal(pixels.reshape(cells_y, cells_x) == cell * cell, RS.full_cells(H, W, cell))


# ------------------------------------------------------------------------------------------------ scene_round's host logic
class FakeDevice:
    """Stands in for the device on the host: predict_scene returns the model's own prepared mask, the two launches are the
    specification's loops.  Counts what was launched."""

    def __init__(self, monkeypatch, masks_by_model):
        self.predicts, self.agrees, self.closes = [], 0, 0
        self.masks_by_model = masks_by_model
        monkeypatch.setattr(ST, "_device_of", lambda models: torch.device("cpu"))
        monkeypatch.setattr(ST, "predict_scene", self.predict_scene)
        monkeypatch.setattr(ST, "scene_cell_agree", self.scene_cell_agree)
        monkeypatch.setattr(ST, "mask_close", self.mask_close)

    def predict_scene(self, model, a, b, **kw):
        from stcd_amd.scene import SceneResult
        self.predicts.append((model, kw))
        return SceneResult(torch.from_numpy(self.masks_by_model[model].copy()), None, None, None)

    def scene_cell_agree(self, masks, cell, label=None, agree=None, cm=None):
        self.agrees += 1
        H, W = masks[0].shape
        cy, cx = RS.grid(H, W, cell)
        a, c = RS.cell_agree([m.numpy() for m in masks], cell, None if label is None else label.numpy())
        return (None if a is None else torch.from_numpy(a).reshape(cy, cx, len(masks) - 1, 2, 2), None if c is None else torch.from_numpy(c).reshape(cy, cx, 2, 2))

    def mask_close(self, mask, radius=2, mask_value=255):
        self.closes += 1
        return torch.from_numpy(RS.close(mask.numpy(), radius, mask_value))


def _scene_case(H, W, K, seed):
    rng = np.random.default_rng(seed)
    a = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    b = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    base = rng.random((H, W)) < 0.3
    base[:H // 3] = False                                                          # cells where no checkpoint sees change
    models = [torch.nn.Identity() for _ in range(K)]
    masks = {m: (base ^ (rng.random((H, W)) < 0.05 * (K - k))).astype(np.uint8) for k, m in enumerate(models)}
    for m in masks.values():
        m[:H // 3] = 0
    label = rng.choice(np.array([0, 1, 7, 255], np.uint8), size=(H, W), p=[0.6, 0.25, 0.05, 0.1])
    return a, b, models, masks, label


@pytest.mark.parametrize("cumulative", [False, True])
@pytest.mark.parametrize("close_radius", [0, 2])
def test_scene_round_host_logic(monkeypatch, cumulative, close_radius):
    H, W, cell, K = 44, 59, 8, 3
    a, b, models, masks, label = _scene_case(H, W, K, seed=3)
    models[0].train()
    models[1].eval()
    fake = FakeDevice(monkeypatch, masks)
    r = ST.scene_round(models, a, b, cell=cell, tile=16, stride=8, batch=4, window="hann", tta="flip", threshold=0.25, close_radius=close_radius,
                       label=label, cumulative=cumulative, stem="whu")
    # every checkpoint alone, in the given order, with the caller's arguments
    assert [p[0] for p in fake.predicts] == models
    assert all(p[1] == dict(tile=16, stride=8, batch=4, window="hann", threshold=0.25, tta="flip") for p in fake.predicts)
    assert fake.agrees == 2 and fake.closes == (1 if close_radius else 0)
    cells_y, cells_x = RS.grid(H, W, cell)
    assert (cells_y, cells_x) == (6, 8) and r.cell == cell
    ms = [masks[m] for m in models]
    for got, want in zip(r.masks, ms):
        np.testing.assert_array_equal(got.numpy(), want)
    want_pseudo = RS.close(ms[-1], close_radius, 255) if close_radius else ms[-1] * 255
    np.testing.assert_array_equal(r.pseudo.numpy(), want_pseudo)
    assert r.pseudo.dtype == torch.uint8 and set(np.unique(r.pseudo.numpy())) <= {0, 255}
    want_agree, _ = RS.cell_agree(ms, cell)
    _, want_cm = RS.cell_agree([want_pseudo], cell, label)
    assert r.agree.shape == (cells_y, cells_x, K - 1, 2, 2) and r.agree.dtype == np.int64
    np.testing.assert_array_equal(r.agree.reshape(-1, K - 1, 4), want_agree)
    np.testing.assert_array_equal(r.cell_cm.reshape(-1, 4), want_cm)
    np.testing.assert_array_equal(r.cm, want_cm.sum(0).reshape(2, 2))
    want_scores = scores_from_cm(want_cm.sum(0).reshape(2, 2))
    assert r.scores.keys() == want_scores.keys()
    for k in want_scores:
        np.testing.assert_array_equal(r.scores[k], want_scores[k])
    want_rel = SP.reliability_cumulative(want_agree) if cumulative else SP.reliability_per_pair(want_agree)
    assert r.reliability.shape == (cells_y, cells_x) and r.reliability.dtype == np.float64
    np.testing.assert_allclose(r.reliability.ravel(), want_rel, rtol=1e-12, equal_nan=True)
    # names, full cells, and the lists over the full cells only
    assert r.names == RS.cell_names(H, W, cell, "whu") and r.names[0] == "whu_0000_0000.png" and r.names[-1] == "whu_0005_0007.png"
    np.testing.assert_array_equal(r.full, RS.full_cells(H, W, cell))
    assert r.full.dtype == bool and r.full.sum() == 5 * 7 and not r.full[-1].any() and not r.full[:, -1].any()
    listed = [i for i in range(cells_y * cells_x) if r.full.ravel()[i]]
    partial = {r.names[i] for i in range(cells_y * cells_x) if not r.full.ravel()[i]}
    assert (r.reliable, r.unreliable) == SP.split([r.names[i] for i in listed], want_rel[listed])
    assert (r.reliable, r.unreliable) == ST.split_reliable([r.names[i] for i in listed], r.reliability.ravel()[listed])
    assert not partial & set(r.reliable + r.unreliable) and len(partial) == 13                 # partial cells are never listed
    assert sorted(r.reliable + r.unreliable) == sorted(r.names[i] for i in listed) and len(r.reliable) == len(listed) // 2
    assert [m.training for m in models] == [True, False, True]


def test_scene_round_with_one_model_and_without_a_label(monkeypatch):
    H, W, cell = 20, 33, 10
    a, b, models, masks, label = _scene_case(H, W, 1, seed=4)
    fake = FakeDevice(monkeypatch, masks)
    r = ST.scene_round(models[0], a, b, cell=cell, tile=16)
    assert fake.agrees == 0 and fake.closes == 0 and len(fake.predicts) == 1
    assert r.agree is None and r.cell_cm is None and r.cm is None and r.scores is None
    np.testing.assert_array_equal(r.reliability, np.ones((2, 4)))
    np.testing.assert_array_equal(r.pseudo.numpy(), masks[models[0]] * 255)
    full_names = [f"scene_{cy:04d}_{cx:04d}.png" for cy in range(2) for cx in range(3)]
    assert (r.reliable, r.unreliable) == (full_names[:3], full_names[3:])                      # ties keep the input order
    r = ST.scene_round(models, a, b, cell=cell, tile=16, label=label, close_radius=1)
    assert fake.agrees == 1 and fake.closes == 1 and r.agree is None
    np.testing.assert_array_equal(r.cell_cm.reshape(-1, 4), RS.cell_agree([RS.close(masks[models[0]], 1, 255)], cell, label)[1])
    r = ST.scene_round(models, a, b, cell=64, tile=16)                                          # no full cell: nothing listed
    assert r.full.shape == (1, 1) and not r.full.any() and r.reliable == [] and r.unreliable == [] and r.names == ["scene_0000_0000.png"]


def test_scene_round_raises_every_argument_error_before_the_first_launch(monkeypatch):
    H, W = 20, 24
    a, b, models, masks, label = _scene_case(H, W, 2, seed=5)
    fake = FakeDevice(monkeypatch, masks)
    ok = dict(cell=8, tile=16)
    for args, kw in (((models, a, b), dict(ok, cell=0)), ((models, a, b), dict(ok, close_radius=5)), ((models, a, b), dict(ok, close_radius=-1)),
                     ((models, a, b), dict(ok, stride=17)), ((models, a, b), dict(ok, tile=0)), ((models, a, b), dict(ok, batch=0)),
                     ((models, a, b), dict(ok, window="box")), ((models, a, b), dict(ok, tta="rot")), ((models, a, b), dict(ok, stem="")),
                     ((models, a, b), dict(ok, label=label[:, :5])), ((models, a, b), dict(ok, label=label.astype(np.int64))),
                     ((models, a, b[:10]), ok), ((models, a[..., 0], b[..., 0]), ok), ((models, a.float(), b.float()), ok),
                     (([], a, b), ok), ((models * 5, a, b), ok), (([lambda x, y: x], a, b), ok)):
        with pytest.raises(_lib.StcdError):
            ST.scene_round(*args, **kw)
    assert fake.predicts == [] and fake.agrees == 0 and fake.closes == 0
    monkeypatch.undo()
    with pytest.raises(_lib.StcdError):                                                         # modules on the CPU: no fallback
        ST.scene_round(models, a, b, **ok)
    for bad in (torch.zeros(4, 4, dtype=torch.uint8), torch.zeros(4, 4)):                       # the wrappers take GPU tensors only
        with pytest.raises(_lib.StcdError):
            ST.scene_cell_agree([bad, bad], 2)
        with pytest.raises(_lib.StcdError):
            ST.mask_close(bad, 2)


# ------------------------------------------------------------------------------------------------ export_cells
@pytest.mark.parametrize("with_label", [False, True])
def test_export_cells_writes_what_the_dataset_reads(monkeypatch, tmp_path, with_label):
    from PIL import Image
    H, W, cell = 37, 50, 16
    a, b, models, masks, label = _scene_case(H, W, 3, seed=6)
    FakeDevice(monkeypatch, masks)
    r = ST.scene_round(models, a, b, cell=cell, tile=16, close_radius=2, stem="s")
    root = str(tmp_path / "train")
    ST.export_cells(r, a, b.numpy(), root, label=label if with_label else None)
    full = [(cy, cx) for cy in range(2) for cx in range(3)]
    names = [f"s_{cy:04d}_{cx:04d}.png" for cy, cx in full]
    subs = ["A", "B", "pseudo_label"] + (["label"] if with_label else [])
    assert sorted(os.listdir(root)) == sorted(subs + ["list"])
    for sub in subs:
        assert sorted(os.listdir(os.path.join(root, sub))) == names                             # the 2 x 3 full cells, no partial one
    pseudo = r.pseudo.numpy()
    for (cy, cx), name in zip(full, names):
        win = (slice(cy * cell, (cy + 1) * cell), slice(cx * cell, (cx + 1) * cell))
        for sub, src in (("A", a.numpy()), ("B", b.numpy())):
            im = Image.open(os.path.join(root, sub, name))
            assert im.mode == "RGB" and im.format == "PNG" and im.size == (cell, cell)
            np.testing.assert_array_equal(np.asarray(im), src[win])
            np.testing.assert_array_equal(np.uint8(np.asarray(im.convert("RGB"), dtype=float)), src[win])          # data/dataset.py:196-199
        im = Image.open(os.path.join(root, "pseudo_label", name))
        assert im.mode == "L" and im.format == "PNG"
        np.testing.assert_array_equal(np.asarray(im), pseudo[win])
        assert set(np.unique(np.asarray(im))) <= {0, 255}
        got = np.asarray(im.convert("RGB"), dtype=np.int32)[:, :, 0]                            # data/dataset.py:206-209
        np.testing.assert_array_equal(got >= 1, pseudo[win] != 0)
        if with_label:
            im = Image.open(os.path.join(root, "label", name))
            assert im.mode == "L"
            np.testing.assert_array_equal(np.asarray(im), label[win])
    with open(os.path.join(root, "list", "reliable_ids.txt"), "r") as f:                        # data/dataset.py:176-183
        assert f.read().splitlines() == r.reliable
    with open(os.path.join(root, "list", "unreliable_ids.txt"), "r") as f:
        assert f.read().splitlines() == r.unreliable
    assert sorted(r.reliable + r.unreliable) == names and len(r.reliable) == 3
    with pytest.raises(_lib.StcdError):
        ST.export_cells(r, a[:10], b[:10], root)
    with pytest.raises(_lib.StcdError):
        ST.export_cells(r, a, b, root, label=label[:5])
