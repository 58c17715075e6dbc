"""The self-training round on the GPU: stcd_selftrain_score through the C ABI against tests/selftrain_spec.py, score_batch over
engine families, SegCD and a plain torch module, and the two drivers end to end.  Every output is an integer or a byte: equality
throughout, no tolerance."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

from stcd_amd import _lib, synth
from stcd_amd import selftrain as ST
from stcd_amd.metrics import scores_from_cm
from tests import selftrain_spec as SP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HWS = (1, 63, 20 * 12, 256 * 256)
BATCHES = (1, 3, 16)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def make_logits(rng, batch, classes, hw):
    """Multiples of 0.5 in [-2, 2]: exact ties between the classes and values exactly on the thresholds 0 and 0.5 are common;
    +-inf and NaN are sprinkled in (also inf against inf of the same sign: a tie)."""
    x = (rng.integers(-4, 5, size=(batch, classes, hw)) * 0.5).astype(np.float32)
    special = rng.random(x.shape)
    x[special < 0.02] = np.inf
    x[(special >= 0.02) & (special < 0.04)] = -np.inf
    x[(special >= 0.04) & (special < 0.06)] = np.nan
    return x


def to_device(x, misaligned):
    """fp32 array -> device tensor; `misaligned`: a one-float offset view of a larger buffer, 4 bytes past a 16-byte boundary."""
    t = torch.from_numpy(x)
    if not misaligned:
        return t.to(DEV)
    buf = torch.empty(x.size + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].view(x.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def gpu_score(dev_logits, threshold, label, mask_value, mask, agree, cm):
    K = len(dev_logits)
    batch, classes, hw = dev_logits[0].shape
    ptrs = (C.c_void_p * K)(*[t.data_ptr() for t in dev_logits])
    _lib.check(_lib.lib().stcd_selftrain_score(ptrs, K, batch, classes, hw, C.c_float(threshold), _p(label), mask_value, _p(mask), _p(agree),
                                               _p(cm), _stream()))


# ------------------------------------------------------------------ 1. the entry against the spec
@pytest.mark.parametrize("K", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("classes", [1, 2])
def test_entry_matches_spec(classes, K):
    rng = np.random.default_rng(100 * classes + K)
    for n, (batch, hw, misaligned) in enumerate(itertools.product(BATCHES, HWS, (False, True))):
        threshold = (0.0, 0.5)[(n // 2 + n // 8) % 2]
        mask_value = (1, 255)[(n // 4 + n) % 2]
        with_label = n % 3 != 2
        logits = [make_logits(rng, batch, classes, hw) for _ in range(K)]
        lab = rng.choice(np.array([0, 1, 7, 255], np.uint8), size=(batch, hw), p=[0.5, 0.3, 0.1, 0.1]) if with_label else None
        dl = [to_device(x, misaligned) for x in logits]
        dlab = None if lab is None else torch.from_numpy(lab).to(DEV)
        mask = torch.full((batch, hw), 7, dtype=torch.uint8, device=DEV)                      # sentinels: an unwritten byte shows,
        agree = torch.full((batch, K - 1, 4), 1000, dtype=torch.int64, device=DEV) if K > 1 else None     # and the counts are ADDED
        cm = torch.full((4,), 5, dtype=torch.int64, device=DEV) if with_label else None
        gpu_score(dl, threshold, dlab, mask_value, mask, agree, cm)
        want_mask, want_agree, want_cm = SP.score(logits, threshold, lab, mask_value)
        tag = f"classes {classes} K {K} batch {batch} hw {hw} misaligned {misaligned} threshold {threshold} mask_value {mask_value}"
        np.testing.assert_array_equal(mask.cpu().numpy(), want_mask, err_msg=tag)
        assert set(np.unique(want_mask)) <= {0, mask_value}
        if K > 1:
            np.testing.assert_array_equal(agree.cpu().numpy(), 1000 + want_agree, err_msg=tag)
            assert (want_agree.sum(-1) == hw).all()
        if with_label:
            np.testing.assert_array_equal(cm.cpu().numpy(), 5 + want_cm, err_msg=tag)
            gpu_score(dl, threshold, dlab, mask_value, mask, agree, cm)                      # cm accumulates over two calls
            np.testing.assert_array_equal(cm.cpu().numpy(), 5 + 2 * want_cm, err_msg=tag)
            assert want_cm.sum() == (lab != 255).sum()


def test_entry_special_values_one_by_one():
    """Each rule on its own, four pixels per line (the vector path) and three (the scalar path)."""
    inf, nan = np.inf, np.nan
    for hw in (4, 3):
        one = np.array([0.0, 0.5, nan, inf, -inf, 0.75, -0.0, -0.75][:2 * hw], np.float32).reshape(2, 1, hw)
        for threshold, rule in ((0.0, lambda v: v > 0), (0.5, lambda v: v > 0.5)):
            mask = torch.full((2, hw), 7, dtype=torch.uint8, device=DEV)
            gpu_score([torch.from_numpy(one).to(DEV)], threshold, None, 1, mask, None, None)
            with np.errstate(invalid="ignore"):
                np.testing.assert_array_equal(mask.cpu().numpy(), rule(one[:, 0]).astype(np.uint8))
        c0 = np.array([1.0, inf, nan, 0.0, -inf, 2.0, inf, -1.0][:2 * hw], np.float32)
        c1 = np.array([1.0, inf, 1.0, nan, -inf, 2.5, 1.0, inf][:2 * hw], np.float32)
        want = np.array([0, 0, 0, 0, 0, 1, 0, 1][:2 * hw], np.uint8).reshape(2, hw)             # ties, NaN on either side: class 0
        two = np.stack([c0.reshape(2, hw), c1.reshape(2, hw)], 1)
        mask = torch.full((2, hw), 7, dtype=torch.uint8, device=DEV)
        gpu_score([torch.from_numpy(np.ascontiguousarray(two)).to(DEV)], 0.0, None, 255, mask, None, None)
        np.testing.assert_array_equal(mask.cpu().numpy(), want * 255)


# ------------------------------------------------------------------ 2. pure function of the inputs
@pytest.mark.parametrize("classes,K,hw", [(1, 3, 256 * 256), (2, 8, 63), (2, 2, 256 * 256), (1, 5, 20 * 12)])
def test_entry_is_reproducible_and_independent_of_the_batch_split(classes, K, hw):
    rng = np.random.default_rng(7 * K + classes)
    B = 16
    logits = [make_logits(rng, B, classes, hw) for _ in range(K)]
    lab = torch.from_numpy(rng.choice(np.array([0, 1, 7, 255], np.uint8), size=(B, hw))).to(DEV)
    dl = [torch.from_numpy(x).to(DEV) for x in logits]

    def run(parts):
        mask = torch.full((B, hw), 7, dtype=torch.uint8, device=DEV)
        agree = torch.zeros((B, K - 1, 4), dtype=torch.int64, device=DEV)
        cm = torch.zeros(4, dtype=torch.int64, device=DEV)
        for s, e in parts:
            gpu_score([t[s:e] for t in dl], 0.0, lab[s:e], 1, mask[s:e], agree[s:e], cm)
        return mask.cpu().numpy().tobytes(), agree.cpu().numpy().tobytes(), cm.cpu().numpy().tobytes()

    whole = run([(0, B)])
    assert run([(0, B)]) == whole                                                             # the same call twice: the same bytes
    assert run([(b, b + 1) for b in range(B)]) == whole                                       # sixteen batches of 1
    assert run([(0, 5), (5, 6), (6, 16)]) == whole


# ------------------------------------------------------------------ 3. score_batch end to end
class _Plain(torch.nn.Module):
    """Not an engine module: nothing in the kernel depends on the engine."""

    def __init__(self, classes=1):
        super().__init__()
        self.conv = torch.nn.Conv2d(6, classes, 3, padding=1)
        self.bn = torch.nn.BatchNorm2d(classes)

    def forward(self, x1, x2):
        return self.bn(self.conv(torch.cat([x1, x2], 1)))


def _models(name, k=3):
    out = []
    for i in range(k):
        torch.manual_seed(500 + i)
        if name == "diff":
            from stcd_amd.modules import SiamUnet_diff
            m = SiamUnet_diff(3, 1, dtype="fp32")
        elif name == "conc":
            from stcd_amd.modules import SiamUnet_conc
            m = SiamUnet_conc(3, 2, dtype="fp32")
        elif name == "segcd":
            from stcd_amd.segcd import SegCD
            m = SegCD()
        else:
            m = _Plain()
        out.append(m.to(DEV))
    return out


def _eval_logits(model, x1, x2):
    """The model's own eval-mode change logits, fp32 [B,classes,hw] on the host."""
    was = model.training
    model.eval()
    with torch.no_grad():
        out = model(x1, x2)
    model.train(was)
    out = out[-1] if isinstance(out, (list, tuple)) else out
    return out.float().reshape(out.shape[0], out.shape[1], -1).cpu().numpy()


def _pairs(n, size, seed):
    a, b, lab = synth.make_pairs_u8(n, size, size, seed)
    lab = lab.copy()
    lab[:, :2] = 255                                                                          # an ignored band
    return (torch.from_numpy(synth.normalize_nchw(a)).to(DEV), torch.from_numpy(synth.normalize_nchw(b)).to(DEV), torch.from_numpy(lab).to(DEV))


@pytest.mark.parametrize("name", ["diff", "conc", "segcd", "plain"])
def test_score_batch_equals_the_spec_on_the_models_own_logits(name):
    size = 64 if name == "segcd" else 32
    models = _models(name)
    models[0].train()
    models[1].eval()
    models[2].train()
    x1, x2, lab = _pairs(5, size, seed=31)
    logits = [_eval_logits(m, x1, x2) for m in models]
    assert not np.array_equal(logits[0], logits[2])                                           # differently seeded
    want_mask, want_agree, want_cm = SP.score(logits, 0.0, lab.reshape(5, -1).cpu().numpy(), 1)
    res = ST.score_batch(models, x1, x2, label=lab)
    assert res.mask.shape == (5, size, size) and res.mask.dtype == torch.uint8 and res.mask.device == x1.device
    assert res.agree.shape == (5, 2, 2, 2) and res.agree.dtype == torch.int64 and res.cm.shape == (4,)
    np.testing.assert_array_equal(res.mask.reshape(5, -1).cpu().numpy(), want_mask)
    np.testing.assert_array_equal(res.agree.reshape(5, 2, 4).cpu().numpy(), want_agree)
    np.testing.assert_array_equal(res.cm.cpu().numpy(), want_cm)
    assert [m.training for m in models] == [True, False, True]                                # modes restored
    again = ST.score_batch(models, x1, x2, label=lab, mask_value=255, cm=res.cm)             # a cm passed in is accumulated into
    assert again.cm is res.cm
    np.testing.assert_array_equal(res.cm.cpu().numpy(), 2 * want_cm)
    np.testing.assert_array_equal(again.mask.reshape(5, -1).cpu().numpy(), want_mask * 255)
    single = ST.score_batch(models[-1:], x1, x2)                                              # one model: a mask, nothing else
    assert single.agree is None and single.cm is None
    np.testing.assert_array_equal(single.mask.reshape(5, -1).cpu().numpy(), want_mask)
    if name == "diff":                                                                        # one class: the threshold is on the raw output
        t = ST.score_batch(models, x1, x2, threshold=0.5)
        np.testing.assert_array_equal(t.mask.reshape(5, -1).cpu().numpy(), SP.score(logits, 0.5)[0])


def test_score_batch_restores_modes_on_error_and_checks_before_any_launch():
    models = _models("plain", 2)
    models[0].train()
    models[1].eval()
    x1, x2, lab = _pairs(2, 32, seed=32)

    class Bad(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def forward(self, a, b):
            return a                                                                          # [B,3,H,W]: not change logits

    bad = Bad().to(DEV).train()
    with pytest.raises(_lib.StcdError):
        ST.score_batch([models[0], bad], x1, x2)
    assert models[0].training and bad.training and not models[1].training
    cpu = _Plain()
    for args, kw in (((models, x1.cpu(), x2), {}), ((models, x1, x2[:1]), {}), ((models, x1.double(), x2.double()), {}), ((models, x1[0], x2[0]), {}),
                     ((models, x1, x2), dict(label=lab.long())), ((models, x1, x2), dict(label=lab[:1])), ((models, x1, x2), dict(label=lab.cpu())),
                     ((models, x1, x2), dict(cm=torch.zeros(4, dtype=torch.int64, device=DEV))),
                     ((models, x1, x2), dict(label=lab, cm=torch.zeros(4, dtype=torch.int32, device=DEV))),
                     ((models, x1, x2), dict(mask_value=0)), ((models, x1, x2), dict(mask_value=256)),
                     (([models[0], cpu], x1, x2), {}), (([cpu], x1.cpu(), x2.cpu()), {}), (([], x1, x2), {}), ((models * 5, x1, x2), {})):
        with pytest.raises(_lib.StcdError):
            ST.score_batch(*args, **kw)
    assert models[0].training and not models[1].training


# ------------------------------------------------------------------ 4. the drivers
def _batches(x1, x2, lab, names, bs):
    for s in range(0, len(names), bs):
        yield x1[s:s + bs], x2[s:s + bs], None if lab is None else lab[s:s + bs], names[s:s + bs]


@pytest.mark.parametrize("name", ["diff", "plain"])
def test_round_on_40_pairs_does_not_depend_on_batch_size_or_flush(name, tmp_path):
    from PIL import Image
    N, size = 40, 32
    models = _models(name)
    x1, x2, lab = _pairs(N, size, seed=33)
    names = [f"pair_{i:02d}.png" for i in range(N)]
    # the spec on the models' own eval logits, one pair at a time (the reference's batch size)
    logits = [np.concatenate([_eval_logits(m, x1[i:i + 1], x2[i:i + 1]) for i in range(N)]) for m in models]
    want_mask, want_agree, _ = SP.score(logits, 0.0, None, 255)
    want_agree = want_agree.reshape(N, 2, 2, 2)
    for cumulative in (False, True):
        want_rel = SP.reliability_cumulative(want_agree) if cumulative else SP.reliability_per_pair(want_agree)
        want_split = SP.split(names, want_rel)
        for bs, flush in ((1, 64), (7, 2), (16, 1), (16, 64)):
            d = str(tmp_path / f"{int(cumulative)}_{bs}_{flush}")
            sel = ST.select_reliable(models, _batches(x1, x2, lab, names, bs), list_dir=os.path.join(d, "list"), cumulative=cumulative, flush=flush)
            np.testing.assert_array_equal(sel.agree, want_agree)
            np.testing.assert_allclose(sel.reliability, want_rel, rtol=1e-12, equal_nan=True)
            assert (sel.reliable, sel.unreliable) == want_split
            assert sorted(sel.reliable + sel.unreliable) == names and not set(sel.reliable) & set(sel.unreliable)     # a partition
            assert len(sel.reliable) == N // 2
            with open(os.path.join(d, "list", "unreliable_ids.txt")) as f:
                listed = f.read().splitlines()
            assert listed == sel.unreliable
            # pseudo-labels of the unreliable half with the last checkpoint, as the reference's recipe goes on
            idx = torch.tensor([names.index(n) for n in listed], device=DEV)
            out = os.path.join(d, "pseudo_label")
            scores = ST.generate_pseudo_labels(models[-1], _batches(x1[idx], x2[idx], lab[idx], listed, bs), out, flush=flush)
            assert sorted(os.listdir(out)) == sorted(listed)
            for n in listed:
                im = Image.open(os.path.join(out, n))
                assert im.mode == "L"
                np.testing.assert_array_equal(np.asarray(im), want_mask[names.index(n)].reshape(size, size))
            ii = idx.cpu().numpy()
            want_cm = SP.score([logits[-1][ii]], 0.0, lab[idx].reshape(len(ii), -1).cpu().numpy(), 255)[2]
            want_scores = scores_from_cm(want_cm.reshape(2, 2))
            assert scores.keys() == want_scores.keys()
            for k in want_scores:
                np.testing.assert_array_equal(scores[k], want_scores[k])
    assert ST.generate_pseudo_labels(models[-1], _batches(x1, x2, None, names, 16), None, write=False) is None


def test_drivers_refuse_cpu_modules_and_wrong_devices(tmp_path):
    x1, x2, lab = _pairs(2, 32, seed=34)
    names = ["a.png", "b.png"]
    with pytest.raises(_lib.StcdError):
        ST.select_reliable([_Plain(), _Plain()], [(x1, x2, None, names)])
    with pytest.raises(_lib.StcdError):
        ST.generate_pseudo_labels(_Plain(), [(x1, x2, lab, names)], str(tmp_path / "p"))
    models = _models("plain", 2)
    with pytest.raises(_lib.StcdError):
        ST.select_reliable(models, [(x1.cpu(), x2.cpu(), None, names)])
    with pytest.raises(_lib.StcdError):
        ST.generate_pseudo_labels(models[0], [(x1, x2, lab.cpu(), names)], str(tmp_path / "q"))
    assert not os.path.exists(str(tmp_path / "q")) or os.listdir(str(tmp_path / "q")) == []
