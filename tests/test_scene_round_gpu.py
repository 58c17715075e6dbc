"""The self-training round on whole scenes on the GPU: stcd_scene_cell_agree and stcd_mask_close through the C ABI against
tests/scene_round_spec.py, and scene_round end to end against predict_scene and the specification.  Every output is an integer or a
byte: equality throughout, no tolerance."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from stcd_amd import _lib, synth
from stcd_amd import selftrain as ST
from stcd_amd.metrics import scores_from_cm
from stcd_amd.scene import predict_scene
from tests import scene_round_spec as RS
from tests import selftrain_spec as SP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VALUES = np.array([0, 1, 7, 255], np.uint8)
# the issue's shapes, then two the 16-byte path needs: a partial bottom row of cells, and cells of several row segments (also the
# scalar path's: 257 x 130 with cell 256)
AGREE_SHAPES = [(1, 1, 1), (5, 7, 4), (33, 47, 16), (64, 64, 64), (100, 259, 32), (257, 130, 256), (100, 160, 32), (300, 512, 256)]
CLOSE_SHAPES = [(1, 1), (1, 40), (3, 3), (5, 300), (63, 65), (64, 64), (130, 257), (200, 520)]    # the tile is 48 x 240: up to 5 x 3 tiles


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def to_device(x, misaligned):
    """uint8 array -> contiguous device tensor; `misaligned`: a view one byte past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(x))
    if not misaligned:
        d = t.to(DEV)
        assert d.data_ptr() % 16 == 0
        return d
    buf = torch.empty(x.size + 1, dtype=torch.uint8, device=DEV)
    view = buf[1:].view(x.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    return view


def gpu_cell_agree(masks, cell, label, agree, cm):
    K = len(masks)
    H, W = masks[0].shape
    cells_y, cells_x = RS.grid(H, W, cell)
    ptrs = (C.c_void_p * K)(*[m.data_ptr() for m in masks])
    _lib.check(_lib.lib().stcd_scene_cell_agree(ptrs, K, H, W, cell, cells_x, cells_y, _p(label), _p(agree), _p(cm), _stream()))


def gpu_close(inp, radius, mask_value, out):
    H, W = inp.shape
    _lib.check(_lib.lib().stcd_mask_close(_p(inp), H, W, radius, mask_value, _p(out), _stream()))


# ------------------------------------------------------------------ 1. stcd_scene_cell_agree against the spec
@pytest.mark.parametrize("K", [1, 2, 3, 8])
@pytest.mark.parametrize("H,W,cell", AGREE_SHAPES)
def test_cell_agree_matches_spec(H, W, cell, K):
    rng = np.random.default_rng(1000 * K + H + W + cell)
    cells = int(np.prod(RS.grid(H, W, cell)))
    pixels = RS.cell_pixels(H, W, cell)
    for with_label, misaligned in itertools.product((False, True), (False, True)):
        if K == 1 and not with_label:
            continue                                                                          # nothing to compute: refused (CPU test)
        masks = [rng.choice(VALUES, size=(H, W), p=[0.55, 0.2, 0.15, 0.1]) for _ in range(K)]
        lab = rng.choice(VALUES, size=(H, W), p=[0.5, 0.3, 0.1, 0.1]) if with_label else None
        dm = [to_device(m, misaligned) for m in masks]
        dlab = None if lab is None else to_device(lab, misaligned)
        agree = torch.full((cells, K - 1, 4), 1000, dtype=torch.int64, device=DEV) if K > 1 else None       # sentinels: the counts are ADDED
        cm = torch.full((cells, 4), 5, dtype=torch.int64, device=DEV) if with_label else None
        gpu_cell_agree(dm, cell, dlab, agree, cm)
        want_agree, want_cm = RS.cell_agree(masks, cell, lab)
        tag = f"H {H} W {W} cell {cell} K {K} label {with_label} misaligned {misaligned}"
        if K > 1:
            np.testing.assert_array_equal(agree.cpu().numpy(), 1000 + want_agree, err_msg=tag)
            np.testing.assert_array_equal(want_agree.sum(-1), np.repeat(pixels[:, None], K - 1, 1))
        if with_label:
            np.testing.assert_array_equal(cm.cpu().numpy(), 5 + want_cm, err_msg=tag)
        gpu_cell_agree(dm, cell, dlab, agree, cm)                                             # a second call doubles the increments
        if K > 1:
            np.testing.assert_array_equal(agree.cpu().numpy(), 1000 + 2 * want_agree, err_msg=tag)
        if with_label:
            np.testing.assert_array_equal(cm.cpu().numpy(), 5 + 2 * want_cm, err_msg=tag)


def test_cell_agree_one_mask_misaligned_alone_takes_the_scalar_path():
    """16-byte loads need EVERY pointer aligned: one mask, or the label alone, one byte off."""
    H, W, cell, K = 64, 96, 32, 3
    rng = np.random.default_rng(9)
    masks = [rng.choice(VALUES, size=(H, W)) for _ in range(K)]
    lab = rng.choice(VALUES, size=(H, W))
    want_agree, want_cm = RS.cell_agree(masks, cell, lab)
    for off in range(K + 1):
        dm = [to_device(m, k == off) for k, m in enumerate(masks)]
        dlab = to_device(lab, off == K)
        agree = torch.zeros((6, K - 1, 4), dtype=torch.int64, device=DEV)
        cm = torch.zeros((6, 4), dtype=torch.int64, device=DEV)
        gpu_cell_agree(dm, cell, dlab, agree, cm)
        np.testing.assert_array_equal(agree.cpu().numpy(), want_agree)
        np.testing.assert_array_equal(cm.cpu().numpy(), want_cm)


def test_cell_agree_more_cells_than_blocks():
    """76 800 cells of 2 x 2 pixels: more work items than the launch has blocks (65 536), so blocks walk on to further cells."""
    H, W, cell = 512, 600, 2
    rng = np.random.default_rng(11)
    masks = [rng.choice(VALUES, size=(H, W)) for _ in range(2)]
    lab = rng.choice(VALUES, size=(H, W))
    want_agree, want_cm = RS.cell_agree(masks, cell, lab)
    assert want_agree.shape[0] == 76800
    agree, cm = ST.scene_cell_agree([to_device(m, False) for m in masks], cell, label=to_device(lab, False))
    np.testing.assert_array_equal(agree.cpu().numpy().reshape(-1, 1, 4), want_agree)
    np.testing.assert_array_equal(cm.cpu().numpy().reshape(-1, 4), want_cm)


def test_cell_agree_wrapper_returns_the_spec_and_adds_into_buffers():
    H, W, cell, K = 70, 90, 32, 3
    rng = np.random.default_rng(10)
    masks = [rng.choice(VALUES, size=(H, W)) for _ in range(K)]
    lab = rng.choice(VALUES, size=(H, W))
    want_agree, want_cm = RS.cell_agree(masks, cell, lab)
    dm, dlab = [to_device(m, False) for m in masks], to_device(lab, False)
    agree, cm = ST.scene_cell_agree(dm, cell, label=dlab)
    assert agree.shape == (3, 3, K - 1, 2, 2) and cm.shape == (3, 3, 2, 2) and agree.dtype == cm.dtype == torch.int64
    np.testing.assert_array_equal(agree.cpu().numpy().reshape(-1, K - 1, 4), want_agree)
    np.testing.assert_array_equal(cm.cpu().numpy().reshape(-1, 4), want_cm)
    again = ST.scene_cell_agree(dm, cell, label=dlab, agree=agree, cm=cm)
    assert again[0] is agree and again[1] is cm
    np.testing.assert_array_equal(agree.cpu().numpy().reshape(-1, K - 1, 4), 2 * want_agree)
    only = ST.scene_cell_agree(dm, cell)
    assert only[1] is None
    np.testing.assert_array_equal(only[0].cpu().numpy().reshape(-1, K - 1, 4), want_agree)
    for args, kw in (((dm, 0), {}), ((dm[:1], cell), {}), ((dm, cell), dict(label=dlab[:5])), ((dm, cell), dict(cm=cm)),
                     ((dm, cell), dict(agree=agree[:2])), (([dm[0], dm[1][:, :5].contiguous()], cell), {}), ((dm * 3, cell), {})):
        with pytest.raises(_lib.StcdError):
            ST.scene_cell_agree(*args, **kw)


# ------------------------------------------------------------------ 2. stcd_mask_close against the spec
@pytest.mark.parametrize("radius", [1, 2, 3, 4])
@pytest.mark.parametrize("H,W", CLOSE_SHAPES)
def test_mask_close_matches_spec(H, W, radius):
    rng = np.random.default_rng(100 * radius + H + W)
    for n, (density, misaligned) in enumerate(itertools.product((0.02, 0.3, 0.7), (False, True))):
        mask_value = (1, 255)[(n + radius) % 2]
        m = (rng.random((H, W)) < density).astype(np.uint8) * rng.choice(VALUES[1:], size=(H, W))
        din = to_device(m, misaligned)
        out = to_device(np.full((H, W), 7, np.uint8), misaligned)                            # a sentinel: an unwritten byte shows
        gpu_close(din, radius, mask_value, out)
        want = RS.close_fast(m, radius, mask_value)
        if H * W <= 4096:
            np.testing.assert_array_equal(want, RS.close(m, radius, mask_value))             # the loops themselves where they are quick
        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"H {H} W {W} radius {radius} density {density} misaligned {misaligned}")
        np.testing.assert_array_equal(din.cpu().numpy(), m)                                  # the input is left alone


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
def test_mask_close_structured_cases(radius):
    def run(m, mask_value=1):
        out = torch.full(m.shape, 7, dtype=torch.uint8, device=DEV)
        gpu_close(to_device(m, False), radius, mask_value, out)
        return out.cpu().numpy()

    for shape in ((1, 1), (4, 9), (60, 250), (100, 500)):
        np.testing.assert_array_equal(run(np.zeros(shape, np.uint8), 255), np.zeros(shape, np.uint8))
        np.testing.assert_array_equal(run(np.full(shape, 3, np.uint8), 255), np.full(shape, 255, np.uint8))
    for shape in ((9, 11), (100, 500)):                                                      # a single pixel in each corner stays alone
        for y, x in ((0, 0), (0, shape[1] - 1), (shape[0] - 1, 0), (shape[0] - 1, shape[1] - 1)):
            m = np.zeros(shape, np.uint8)
            m[y, x] = 1
            np.testing.assert_array_equal(run(m), m)
    # two pixels of one row, and of one column, 2 r + 1 apart are bridged and 2 r + 2 apart are not; also across the tile
    # borders at column 240 and row 48
    for base in (15, 236, 44):
        for gap, bridged in ((2 * radius + 1, True), (2 * radius + 2, False)):
            m = np.zeros((21, 300), np.uint8)                                                # 10 > 2 r rows to either border: the row stays a row
            m[10, base] = m[10, base + gap] = 1
            want = m.copy()
            if bridged:
                want[10, base:base + gap + 1] = 1
            np.testing.assert_array_equal(RS.close_fast(m, radius), want)
            np.testing.assert_array_equal(run(m), want)
            np.testing.assert_array_equal(run(np.ascontiguousarray(m.T)), want.T)
    m = np.zeros((9, 40), np.uint8)                                                          # the CPU test's case, at its radius
    m[4, 15] = m[4, 20] = 1
    np.testing.assert_array_equal(run(m), RS.close(m, radius))


def test_mask_close_wrapper_is_extensive_idempotent_and_the_max_pool_composition():
    import torch.nn.functional as F
    rng = np.random.default_rng(12)
    m = (rng.random((150, 333)) < 0.1).astype(np.uint8)
    d = to_device(m, False)
    for radius in (1, 2, 3, 4):
        once = ST.mask_close(d, radius, 255)
        assert once.shape == d.shape and once.dtype == torch.uint8 and once.data_ptr() != d.data_ptr()
        np.testing.assert_array_equal(once.cpu().numpy(), RS.close_fast(m, radius, 255))
        assert bool(((once != 0) >= (d != 0)).all())
        assert torch.equal(ST.mask_close(once, radius, 255), once)
        k = 2 * radius + 1
        x = d[None, None].float()
        pooled = -F.max_pool2d(-F.max_pool2d(x, k, 1, radius), k, 1, radius)
        assert torch.equal(once, (pooled[0, 0] * 255).to(torch.uint8))
    for kw in (dict(radius=0), dict(radius=5), dict(mask_value=0), dict(mask_value=256)):
        with pytest.raises(_lib.StcdError):
            ST.mask_close(d, **kw)


# ------------------------------------------------------------------ 3. scene_round end to end
class _Plain(torch.nn.Module):
    """Not an engine module: nothing in the round depends on the engine."""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(6, 1, 3, padding=1)
        self.bn = torch.nn.BatchNorm2d(1)

    def forward(self, x1, x2):
        return self.bn(self.conv(torch.cat([x1, x2], 1)))


def _models(name):
    out = []
    for i in range(3):
        torch.manual_seed(700 + i)
        if name == "diff":
            from stcd_amd.modules import SiamUnet_diff
            m = SiamUnet_diff(3, 1, dtype="fp32")
        else:
            m = _Plain()
        out.append(m.to(DEV))
    return out


@pytest.fixture(scope="module")
def scene():
    H, W = 96, 80
    a, b, lab = synth.make_pairs_u8(1, H, W, seed=21)
    lab = lab[0].copy()
    lab[:3, :] = 255                                                                          # an ignored band
    lab[40:50, 10:20] = 7
    return a[0], b[0], lab


@pytest.mark.parametrize("name,tta", [("diff", None), ("diff", "flip"), ("plain", None)])
def test_scene_round_is_predict_scene_and_the_spec(scene, name, tta):
    a, b, lab = scene
    H, W, cell = 96, 80, 32
    models = _models(name)
    models[0].train()
    models[1].eval()
    models[2].train()
    kw = dict(tile=32, stride=16, window="hann", tta=tta)
    want_masks = [predict_scene(m, a, b, batch=16, **kw).mask for m in models]
    ms = [m.cpu().numpy() for m in want_masks]
    assert any(0 < int(m.sum()) < m.size for m in ms)                                         # the checkpoints see something
    want_agree, _ = RS.cell_agree(ms, cell)
    rounds = {}
    for close_radius, batch in ((0, 16), (2, 16), (2, 1)):
        r = ST.scene_round(models, a, b, cell=cell, batch=batch, close_radius=close_radius, label=lab, stem="t", **kw)
        rounds[close_radius, batch] = r
        assert len(r.masks) == 3
        for got, want in zip(r.masks, want_masks):
            assert got.dtype == torch.uint8 and got.device == want.device and torch.equal(got, want)      # byte-equal to predict_scene
        want_pseudo = RS.close_fast(ms[-1], close_radius, 255) if close_radius else ms[-1] * 255
        np.testing.assert_array_equal(r.pseudo.cpu().numpy(), want_pseudo)
        _, want_cm = RS.cell_agree([want_pseudo], cell, lab)
        assert r.agree.shape == (3, 3, 2, 2, 2) and r.cell_cm.shape == (3, 3, 2, 2)
        np.testing.assert_array_equal(r.agree.reshape(-1, 2, 4), want_agree)
        np.testing.assert_array_equal(r.cell_cm.reshape(-1, 4), want_cm)
        np.testing.assert_array_equal(r.cm.ravel(), want_cm.sum(0))
        want_scores = scores_from_cm(want_cm.sum(0).reshape(2, 2))
        for k in want_scores:
            np.testing.assert_array_equal(r.scores[k], want_scores[k])
        want_rel = SP.reliability_per_pair(want_agree)
        np.testing.assert_allclose(r.reliability.ravel(), want_rel, rtol=1e-12)
        np.testing.assert_array_equal(r.full, RS.full_cells(H, W, cell))
        listed = [i for i in range(9) if r.full.ravel()[i]]
        assert len(listed) == 6 and r.names == RS.cell_names(H, W, cell, "t")
        assert (r.reliable, r.unreliable) == SP.split([r.names[i] for i in listed], want_rel[listed])
        assert [m.training for m in models] == [True, False, True]                            # modes restored
    one, sixteen = rounds[2, 1], rounds[2, 16]                                                # the same for batch 1 and 16
    assert torch.equal(one.pseudo, sixteen.pseudo) and all(torch.equal(x, y) for x, y in zip(one.masks, sixteen.masks))
    np.testing.assert_array_equal(one.agree, sixteen.agree)
    np.testing.assert_array_equal(one.cell_cm, sixteen.cell_cm)
    assert (one.reliable, one.unreliable) == (sixteen.reliable, sixteen.unreliable)
    assert torch.equal(rounds[0, 16].pseudo, rounds[0, 16].masks[-1] * 255)


def test_scene_round_one_model_cumulative_and_export(scene, tmp_path):
    from PIL import Image
    a, b, lab = scene
    models = _models("plain")
    r = ST.scene_round(models[-1], a, b, cell=32, tile=32, close_radius=1)
    assert r.agree is None and r.cm is None and (r.reliability == 1.0).all() and len(r.reliable) == 3
    r = ST.scene_round(models, a, b, cell=32, tile=32, stride=16, cumulative=True, close_radius=2)
    ms = [m.cpu().numpy() for m in r.masks]
    want = SP.reliability_cumulative(RS.cell_agree(ms, 32)[0])
    np.testing.assert_allclose(r.reliability.ravel(), want, rtol=1e-12, equal_nan=True)
    root = str(tmp_path / "train")
    ST.export_cells(r, torch.from_numpy(a).to(DEV), b, root, label=lab)                       # device crops and host crops alike
    pseudo = r.pseudo.cpu().numpy()
    for cy in range(3):
        for cx in range(2):
            win = (slice(cy * 32, cy * 32 + 32), slice(cx * 32, cx * 32 + 32))
            name = f"scene_{cy:04d}_{cx:04d}.png"
            np.testing.assert_array_equal(np.asarray(Image.open(f"{root}/A/{name}")), a[win])
            np.testing.assert_array_equal(np.asarray(Image.open(f"{root}/B/{name}")), b[win])
            np.testing.assert_array_equal(np.asarray(Image.open(f"{root}/pseudo_label/{name}")), pseudo[win])
            np.testing.assert_array_equal(np.asarray(Image.open(f"{root}/label/{name}")), lab[win])
    assert open(f"{root}/list/reliable_ids.txt").read().splitlines() == r.reliable and len(r.reliable) == 3
    with pytest.raises(_lib.StcdError):
        ST.scene_round(models, a, b, cell=0)
    with pytest.raises(_lib.StcdError):
        ST.scene_round([m.cpu() for m in _models("plain")], a, b)
