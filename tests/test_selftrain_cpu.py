"""The self-training round, the part that needs no GPU: the C-ABI entry exists and refuses bad arguments before any HIP call, the two
reliability rules equal the fixture recorded from the reference's own metric class (tests/golden/make_selftrain_golden.py) and the
plain loops of tests/selftrain_spec.py, the split reproduces the reference's order and halves, the list files read back as
CD_Dataset reads them, and the drivers' host logic (flush, name checks, batch-size independence) holds with a fake score_batch."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from stcd_amd import _lib
from stcd_amd import selftrain as ST
from stcd_amd.metrics import scores_from_cm
from tests import selftrain_spec as SP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("a", "b")


def agree_of(masks):
    """uint8 [K,N,h,w] -> int64 [N,K-1,2,2], agree[n, i, last, pred_i], by the spec's bincount."""
    K, N = masks.shape[:2]
    logits = [np.where(masks[k].reshape(N, 1, -1) > 0, 1.0, -1.0).astype(np.float32) for k in range(K)]
    return SP.score(logits)[1].reshape(N, K - 1, 2, 2)


@pytest.fixture(scope="module")
def fx(golden):
    return golden("selftrain_metric.npz")


def test_entry_is_declared_bound_and_exported():
    hdr = open(os.path.join(REPO, "include", "stcd_hip.h")).read()
    assert "stcd_selftrain_score" in set(re.findall(r"\b(stcd_[a-z0-9_]+)\s*\(", hdr))
    assert "train_stcd.py:111-125" in hdr and ":155-177" in hdr                # what it replaces
    assert "stcd_selftrain_score" in _lib.EXPORTS
    assert hasattr(C.CDLL(_lib.LIB_PATH), "stcd_selftrain_score")
    assert _lib.lib().stcd_abi_version() == 2                                 # additions only


@pytest.mark.parametrize("case", CASES)
def test_cumulative_rule_is_the_references_arithmetic(fx, case):
    agree = agree_of(fx[f"{case}/masks"])
    want = fx[f"{case}/cumulative"]
    got = ST.reliability(agree, cumulative=True)
    assert got.dtype == np.float64 and got.shape == want.shape
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))              # NaN in the same places
    assert np.isnan(want).sum() == (1 if case == "b" else 0)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)
    np.testing.assert_allclose(SP.reliability_cumulative(agree), want, rtol=1e-12, atol=0, equal_nan=True)
    np.testing.assert_array_equal(ST.reliability(agree.reshape(len(agree), -1, 4), cumulative=True), got)     # the kernel's [N,K-1,4] too


@pytest.mark.parametrize("case", CASES)
def test_default_rule_is_the_fresh_metric_with_empty_unions_at_one(fx, case):
    agree = agree_of(fx[f"{case}/masks"])
    fresh = fx[f"{case}/fresh"]                                               # [N,K-1], NaN where the union is empty
    assert np.isnan(fresh).all(axis=1).sum() >= 3
    filled = np.where(np.isnan(fresh), 1.0, fresh)
    want = filled[:, 0].copy()
    for i in range(1, filled.shape[1]):
        want = want + filled[:, i]
    want = want / filled.shape[1]
    got = ST.reliability(agree)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert np.isfinite(got).all() and (got[np.isnan(fresh).all(axis=1)] == 1.0).all()
    np.testing.assert_allclose(SP.reliability_per_pair(agree), want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", CASES)
def test_split_reproduces_the_references_order_and_halves(fx, case):
    rel = fx[f"{case}/cumulative"]
    N = len(rel)
    assert N % 2 == (0 if case == "a" else 1)                                 # N even and odd
    names = [f"pair_{i:03d}.png" for i in range(N)]
    want = [int(i) for i in fx[f"{case}/order"]] + [i for i in range(N) if math.isnan(rel[i])]      # NaN last
    assert sorted(want) == list(range(N))
    reliable, unreliable = ST.split_reliable(names, rel)
    assert reliable + unreliable == [names[i] for i in want]
    assert len(reliable) == N // 2 and len(unreliable) == N - N // 2          # :130-134
    assert (reliable, unreliable) == SP.split(names, rel)
    if case == "b":
        assert unreliable[-1] == names[0]                                     # the pair whose cumulative matrix is still empty


@pytest.mark.parametrize("case", CASES)
def test_split_keeps_ties_in_input_order(fx, case):
    agree = agree_of(fx[f"{case}/masks"])
    rel = ST.reliability(agree)
    names = [f"n{i}" for i in range(len(rel))]
    ones = [names[i] for i in range(len(rel)) if rel[i] == 1.0]
    assert len(ones) >= 4                                                     # three empty pairs and one of identical masks
    reliable, unreliable = ST.split_reliable(names, rel)
    assert (reliable + unreliable)[:len(ones)] == ones
    assert (reliable, unreliable) == SP.split(names, rel)


def test_split_edge_cases():
    assert ST.split_reliable([], []) == ([], [])
    assert ST.split_reliable(["x"], [0.5]) == ([], ["x"])
    nan = float("nan")
    assert ST.split_reliable(list("abcde"), [nan, 0.2, nan, 0.9, 0.2]) == (["d", "b"], ["e", "a", "c"])
    with pytest.raises(_lib.StcdError):
        ST.split_reliable(["a", "b"], [1.0])
    with pytest.raises(_lib.StcdError):
        ST.reliability(np.zeros((3, 0, 2, 2), np.int64))                      # one model: nothing to agree with
    with pytest.raises(_lib.StcdError):
        ST.reliability(np.zeros((3, 2, 2, 2), np.float32))


def test_lists_read_back_as_the_dataset_reads_them(tmp_path):
    reliable, unreliable = ["train_1.png", "train_7.png"], ["train_3.png", "a b.png", "train_2.png"]
    d = str(tmp_path / "list")
    ST.write_lists(d, reliable, unreliable)
    with open(os.path.join(d, "reliable_ids.txt"), "r") as f:                 # data/dataset.py:176-179
        assert f.read().splitlines() == reliable
    with open(os.path.join(d, "unreliable_ids.txt"), "r") as f:
        assert f.read().splitlines() == unreliable
    assert open(os.path.join(d, "unreliable_ids.txt")).read().endswith("train_2.png\n")
    ST.write_lists(d, [], reliable)                                           # a second round overwrites
    assert open(os.path.join(d, "reliable_ids.txt")).read() == ""


# ------------------------------------------------------------------------------------------------ the C entry's argument checks
def _call(logits="ok", n_models=2, batch=2, classes=1, hw=16, mask_value=1, label=False, mask=True, agree="auto", cm=False):
    """Calls the entry with HOST buffers: every case here is refused (or has nothing to launch) before any HIP call."""
    bufs = [np.zeros(64, np.float32) for _ in range(8)]
    keep = [np.zeros(64, np.uint8), np.zeros(64, np.uint8), np.zeros(64, np.int64), np.zeros(4, np.int64)]
    ptrs = (C.c_void_p * 8)(*[b.ctypes.data for b in bufs])
    if logits == "hole":
        ptrs[1] = None
    vp = lambda on, a: C.c_void_p(a.ctypes.data) if on else None
    if agree == "auto":
        agree = n_models != 1
    rc = _lib.lib().stcd_selftrain_score(None if logits is None else ptrs, n_models, batch, classes, hw, C.c_float(0.0), vp(label, keep[0]),
                                         mask_value, vp(mask, keep[1]), vp(agree, keep[2]), vp(cm, keep[3]), None)
    return rc, _lib.lib().stcd_last_error().decode()


@pytest.mark.parametrize("kw", [dict(logits=None), dict(logits="hole"), dict(n_models=0), dict(n_models=9), dict(n_models=-1), dict(classes=0),
                                dict(classes=3), dict(mask_value=0), dict(mask_value=256), dict(mask=False), dict(agree=False),
                                dict(n_models=1, agree=True), dict(label=True), dict(cm=True), dict(batch=-1), dict(hw=-1)])
def test_entry_refuses_bad_arguments_before_any_hip_call(kw):
    rc, err = _call(**kw)
    assert rc != 0, kw
    assert err.startswith("stcd_selftrain_score: "), err


@pytest.mark.parametrize("kw", [dict(batch=0), dict(hw=0), dict(batch=0, n_models=1), dict(hw=0, label=True, cm=True), dict(batch=0, n_models=8, classes=2)])
def test_entry_launches_nothing_for_an_empty_batch(kw):
    rc, err = _call(**kw)
    assert rc == 0, err


def test_score_batch_refuses_cpu_modules_and_bad_model_lists():
    from stcd_amd.modules import SiamUnet_diff
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(_lib.StcdError):
        ST.score_batch([SiamUnet_diff(3, 1)], x, x)
    with pytest.raises(_lib.StcdError):
        ST.score_batch([torch.nn.Conv2d(3, 1, 1)] * 2, x, x)
    with pytest.raises(_lib.StcdError):
        ST.score_batch([], x, x)
    with pytest.raises(_lib.StcdError):
        ST.score_batch([torch.nn.Conv2d(3, 1, 1)] * 9, x, x)
    with pytest.raises(_lib.StcdError):
        ST.score_batch([lambda a, b: a], x, x)


# ------------------------------------------------------------------------------------------------ the drivers' host logic
class FakeScore:
    """Stands in for score_batch on the host: the first K channels of x1 ARE the K models' one-class logits; x2 is ignored."""

    def __init__(self):
        self.calls = 0

    def __call__(self, models, x1, x2, label=None, threshold=0.0, mask_value=1, cm=None):
        self.calls += 1
        (B, _, H, W), K = x1.shape, len(models)
        logits = [x1[:, k].reshape(B, 1, H * W).numpy() for k in range(K)]
        mask, agree, c = SP.score(logits, threshold, None if label is None else label.reshape(B, -1).numpy(), mask_value)
        if c is not None:
            c = torch.from_numpy(c) + (0 if cm is None else cm)
        return ST.BatchScore(torch.from_numpy(mask).reshape(B, H, W), None if agree is None else torch.from_numpy(agree).reshape(B, K - 1, 2, 2), c)


def fake_pairs(n, k, h, w, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, k, h, w)).astype(np.float32)
    x[::5] = -1.0                                                             # pairs without change in any model
    lab = rng.choice(np.array([0, 1, 7, 255], np.uint8), size=(n, h, w), p=[0.6, 0.25, 0.05, 0.1])
    return torch.from_numpy(x), torch.from_numpy(lab), [f"p{i:02d}.png" for i in range(n)]


def batches_of(x, lab, names, bs, with_label=True):
    for s in range(0, len(names), bs):
        yield x[s:s + bs], x[s:s + bs], lab[s:s + bs] if with_label else None, tuple(names[s:s + bs])


@pytest.fixture
def fake(monkeypatch):
    f = FakeScore()
    monkeypatch.setattr(ST, "score_batch", f)
    copies = []
    real = ST._to_host
    monkeypatch.setattr(ST, "_to_host", lambda parts: (copies.append(len(parts)) if parts else None, real(parts))[1])
    f.copies = copies
    return f


def test_select_reliable_does_not_depend_on_batch_size_or_flush(fake, tmp_path):
    K, N = 3, 23
    x, lab, names = fake_pairs(N, K, 6, 5, seed=1)
    models = [torch.nn.Identity() for _ in range(K)]
    models[1].train()
    models[0].eval()
    want_agree = SP.score([x[:, k].reshape(N, 1, -1).numpy() for k in range(K)])[1].reshape(N, K - 1, 2, 2)
    for cumulative in (False, True):
        for bs, flush in ((1, 64), (7, 1), (16, 2), (1, 4), (23, 64)):
            fake.copies.clear()
            d = str(tmp_path / f"list_{int(cumulative)}_{bs}_{flush}")
            sel = ST.select_reliable(models, batches_of(x, lab, names, bs), list_dir=d, cumulative=cumulative, flush=flush)
            nb = -(-N // bs)
            assert fake.copies == [flush] * (nb // flush) + ([nb % flush] if nb % flush else [])      # one copy per `flush` batches
            assert sel.names == names
            np.testing.assert_array_equal(sel.agree, want_agree)
            want_rel = SP.reliability_cumulative(want_agree) if cumulative else SP.reliability_per_pair(want_agree)
            np.testing.assert_allclose(sel.reliability, want_rel, rtol=1e-12, equal_nan=True)
            assert (sel.reliable, sel.unreliable) == SP.split(names, want_rel)
            assert sorted(sel.reliable + sel.unreliable) == sorted(names) and len(sel.reliable) == N // 2
            assert open(os.path.join(d, "reliable_ids.txt")).read().splitlines() == sel.reliable
            assert open(os.path.join(d, "unreliable_ids.txt")).read().splitlines() == sel.unreliable
    assert [m.training for m in models] == [False, True, True]                # modes restored


def test_generate_pseudo_labels_writes_masks_and_scores(fake, tmp_path):
    from PIL import Image
    N = 11
    x, lab, names = fake_pairs(N, 1, 6, 5, seed=2)
    model = torch.nn.Identity()
    mask, _, cm = SP.score([x.reshape(N, 1, -1).numpy()], 0.0, lab.reshape(N, -1).numpy(), 255)
    want = scores_from_cm(cm.reshape(2, 2))
    for bs, flush in ((1, 64), (4, 1), (16, 2)):
        out = str(tmp_path / f"pseudo_{bs}_{flush}")
        fake.copies.clear()
        got = ST.generate_pseudo_labels(model, batches_of(x, lab, names, bs), out, flush=flush)
        assert sum(fake.copies) == -(-N // bs)
        assert sorted(os.listdir(out)) == sorted(names)
        for i, n in enumerate(names):
            im = Image.open(os.path.join(out, n))
            assert im.mode == "L" and im.format == "PNG"
            np.testing.assert_array_equal(np.asarray(im), mask[i].reshape(6, 5))
            assert set(np.unique(np.asarray(im))) <= {0, 255}
        assert got.keys() == want.keys()
        for k in want:
            np.testing.assert_array_equal(got[k], want[k])
    assert ST.generate_pseudo_labels(model, batches_of(x, lab, names, 4, with_label=False), None, write=False) is None
    only_scores = ST.generate_pseudo_labels(model, batches_of(x, lab, names, 4), None, write=False)
    np.testing.assert_array_equal(only_scores["iou"], want["iou"])
    assert model.training


def test_drivers_check_names_before_anything_is_enqueued(fake, tmp_path):
    x, lab, names = fake_pairs(4, 2, 4, 4, seed=3)
    models = [torch.nn.Identity(), torch.nn.Identity()]
    for bad in ([(x, x, None, names[:3])], [(x, x, None, ["a", "b", "a", "c"])], [(x, x, None, ["a", "b", 3, "c"])], [(x, x, None, ["a", "", "b", "c"])],
                [(x[:2], x[:2], None, names[:2]), (x[2:], x[2:], None, names[1:3])]):          # the last: a name of an earlier batch
        before = fake.calls
        with pytest.raises(_lib.StcdError):
            ST.select_reliable(models, bad)
        assert fake.calls - before == len(bad) - 1
        before = fake.calls
        with pytest.raises(_lib.StcdError):
            ST.generate_pseudo_labels(models[0], bad, str(tmp_path / "x"))
        assert fake.calls - before == len(bad) - 1
    with pytest.raises(_lib.StcdError):
        ST.select_reliable(models[:1], [(x, x, None, names)])                 # one model: nothing to compare
    with pytest.raises(_lib.StcdError):
        ST.select_reliable(models, [(x, x, None, names)], flush=0)
    with pytest.raises(_lib.StcdError):
        ST.generate_pseudo_labels(models[0], [(x[:2], x[:2], lab[:2], names[:2]), (x[2:], x[2:], None, names[2:])], None, write=False)
    with pytest.raises(_lib.StcdError):
        ST.generate_pseudo_labels(models[0], [(x, x, None, names)], None)     # write without a directory
    sel = ST.select_reliable(models, [])
    assert sel.names == [] and sel.reliable == [] and sel.unreliable == [] and sel.agree.shape == (0, 1, 2, 2)
