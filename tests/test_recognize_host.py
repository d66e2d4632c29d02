"""CPU tests of the greedy recognition's surface (hctr_recognize*, ``hctr_model.recognize``, ``ctc_codec.recognize``,
``Recognition``): the float64 yardstick tests/recognize_ref.py on hand-written collapse cases, against the oracle codec's
greedy decode and against torch's float64 ctc_loss; the host-side result object; argument validation; the C ABI symbols.
The device results are checked by tests/test_gpu_recognize.py."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import codec_cases
import recognize_ref as ref
from conftest import PKG, ROOT
from oracle import ctc_ref


@pytest.fixture(scope="module")
def ctc():
    return importlib.import_module(PKG + ".ctc")


def _spans(r, b=0):
    n = int(r["lengths"][b])
    return [(int(r["labels"][b, j]), int(r["starts"][b, j]), int(r["ends"][b, j])) for j in range(n)]


@pytest.mark.parametrize("name,k1,spans", ref.HAND_CASES, ids=[c[0] for c in ref.HAND_CASES])
def test_ref_hand_written_cases(name, k1, spans):
    rng = np.random.RandomState(len(k1))
    z = ref.hand_logits(rng, k1)
    r = ref.recognize_ref(z)
    assert r["k1"][0].tolist() == k1
    assert _spans(r) == spans
    lp = z[:, 0].astype(np.float64) - ref.lse64(z[:, 0])[:, None]
    for j, (label, s, e) in enumerate(spans):
        assert abs(r["logps"][0, j] - lp[s:e, label].sum()) < 1e-12
        peak = s + int(np.argmax(lp[s:e, label]))
        assert r["alt_labels"][0, j] == r["k2"][0, peak] != label
        assert abs(r["alt_logps"][0, j] - lp[peak, r["k2"][0, peak]]) < 1e-12
        assert r["alt_logps"][0, j] <= lp[peak, label]
    assert abs(r["path_logp"][0] - lp[np.arange(len(k1)), k1].sum()) < 1e-12
    if ref.HAND_C - 1 not in k1:                           # the greedy path is an alignment of its text unless a column
        assert r["path_logp"][0] <= -r["text_nll"][0] + 1e-12      # decodes to C-1, which the collapse drops like a blank
    if not spans:                                          # an empty text has one alignment: all blanks
        want = -lp[:, 0].sum()
        assert abs(r["text_nll"][0] - want) < 1e-12
        if all(k == 0 for k in k1):
            assert abs(r["text_nll"][0] + r["path_logp"][0]) < 1e-12
    assert (r["labels"][0, len(spans):] == 0).all() and (r["logps"][0, len(spans):] == 0).all()


def test_ref_straddle_cases():
    for W, k1, spans in ref.STRADDLE_CASES:
        r = ref.recognize_ref(ref.hand_logits(np.random.RandomState(W), k1))
        assert _spans(r) == spans, W


def test_ref_top2_order():
    nan, inf = np.nan, np.inf
    assert ref.top2(np.zeros(5, np.float32)) == (0, 1)
    assert ref.top2(np.array([1, 3, 3, 2], np.float32)) == (1, 2)
    assert ref.top2(np.array([1, 3, 0, 2, 2], np.float32)) == (1, 3)
    assert ref.top2(np.array([1, nan, 7, nan], np.float32)) == (1, 3)
    assert ref.top2(np.array([1, 7, nan, 7], np.float32)) == (2, 1)
    assert ref.top2(np.full(4, -inf, np.float32)) == (0, 1)
    assert ref.top2(np.array([-inf, -inf, 2, -inf], np.float32)) == (2, 0)
    assert ref.top2(np.array([2, -inf, -inf], np.float32)) == (0, 1)


@pytest.mark.parametrize("case", [c for c in codec_cases.CODEC_CASES if c[4] <= 300], ids=lambda c: c[0])
def test_ref_labels_equal_the_oracle_codec(case):
    name, seed, W, B, C, style = case
    logits = codec_cases.gen_logits(seed, W, B, C, style)
    chars = codec_cases.vocab(C)
    codec = ctc_ref.CtcCodecRef(chars)
    r = ref.recognize_ref(logits)
    got = ["".join(codec.characters[i] for i in r["labels"][b, :r["lengths"][b]]) for b in range(B)]
    assert got == codec.decode(logits)
    assert (r["lengths"] > 0).any()
    for b in range(B):                                     # spans: ordered, disjoint, inside the line
        sp = _spans(r, b)
        assert all(0 <= s < e <= W for _, s, e in sp)
        assert all(sp[j][2] <= sp[j + 1][1] for j in range(len(sp) - 1))


def test_ref_text_nll_equals_torch_float64():
    rng = np.random.RandomState(3)
    W, B, C = 40, 4, 9
    logits = rng.standard_normal((W, B, C)).astype(np.float32)                  # flat: texts of ~30 labels, with repeats
    logits[:, 1] = ref.planted(rng, W, C, [3, 3, 4, 1, 1, 1, 7])[0]
    logits[:, 2, 0] += 20                                                        # an empty text
    r = ref.recognize_ref(logits)
    assert r["lengths"][2] == 0 and r["lengths"][1] == 7 and r["lengths"][0] > 7
    tl = torch.from_numpy(r["lengths"].astype(np.int64))
    tg = torch.from_numpy(np.concatenate([r["labels"][b, :r["lengths"][b]] for b in range(B)]).astype(np.int64))
    want = torch.nn.functional.ctc_loss(torch.from_numpy(logits).double().log_softmax(2), tg,
                                        torch.full((B,), W, dtype=torch.int64), tl, blank=0, reduction="none").numpy()
    np.testing.assert_allclose(r["text_nll"], want, rtol=1e-12, atol=1e-12)
    clean = ~(r["k1"] == C - 1).any(axis=1)                # lines whose greedy path is an alignment of their text
    assert clean[1] and clean[2] and (r["path_logp"] <= -r["text_nll"] + 1e-12)[clean].all()


def test_recognition_object(ctc, pkg):
    labels = np.array([[4, 4, 0], [7, 0, 0], [0, 0, 0]], np.int32)
    lengths = np.array([2, 1, 0], np.int32)
    starts = np.array([[0, 2, 0], [1, 0, 0], [0, 0, 0]], np.int32)
    ends = np.array([[1, 3, 0], [3, 0, 0], [0, 0, 0]], np.int32)
    logps = np.log(np.array([[0.5, 0.25, 1], [0.25 * 0.25, 1, 1], [1, 1, 1]], np.float32))
    alts = np.array([[2, 0, 0], [1, 0, 0], [0, 0, 0]], np.int32)
    alt_logps = np.log(np.array([[0.25, 0.5, 1], [0.125, 1, 1], [1, 1, 1]], np.float32))
    r = ctc.Recognition(labels, lengths, starts, ends, logps, alts, alt_logps,
                        np.log(np.array([0.1, 0.2, 0.5], np.float32)), -np.log(np.array([0.2, 0.25, 0.5], np.float32)))
    assert len(r) == 3 and pkg.Recognition is ctc.Recognition
    lines = list(r.lines())
    assert [[(c, s, e, a) for c, s, e, _, a, _ in ln] for ln in lines] == [[(4, 0, 1, 2), (4, 2, 3, 0)], [(7, 1, 3, 1)], []]
    np.testing.assert_allclose([p for ln in lines for _, _, _, p, _, _ in ln], [0.5, 0.25, 0.25], rtol=1e-6)
    np.testing.assert_allclose([p for ln in lines for _, _, _, _, _, p in ln], [0.25, 0.5, 0.125], rtol=1e-6)
    np.testing.assert_allclose(r.text_posterior, [0.2, 0.25, 0.5], rtol=1e-6)
    assert r.text_posterior.dtype == np.float64
    assert [v.tolist() for v in r.label_lists()] == [[4, 4], [7], []]
    np.testing.assert_allclose(np.exp(r.path_logp), [0.1, 0.2, 0.5], rtol=1e-6)
    assert r.labels is labels and r.lengths is lengths


def test_argument_validation(ctc, pkg):
    """what the Python entry points refuse before any device work"""
    chars = codec_cases.vocab(12)
    cd = pkg.ctc_codec(chars)
    with pytest.raises(ValueError):
        cd.recognize(np.zeros((5, 2), np.float32))                       # not [W, B, C]
    with pytest.raises(ValueError):
        cd.recognize(np.zeros((5, 2, 11), np.float32))                   # the codec has 12 classes
    with pytest.raises(ValueError):
        cd.recognize(np.zeros((0, 2, 12), np.float32))                   # no steps
    with pytest.raises(ValueError):
        ctc.recognize_logits(None, np.zeros((4, 1, 1), np.float32), 0)   # one class
    with pytest.raises(ValueError):
        ctc.recognize_logits(None, np.zeros((4, 3), np.float32), 0)
    empty = ctc.recognize_logits(None, np.zeros((4, 0, 7), np.float32), 0)      # B = 0: no call is made
    assert len(empty) == 0 and empty.labels.shape == (0, 4) and list(empty.lines()) == []
    m = pkg.hctr_model(12)
    with pytest.raises(RuntimeError):
        m.recognize(np.zeros((1, 1, 128, 32), np.float32))               # not on a GPU
    for bad in (np.zeros((1, 128, 32), np.float32), np.zeros((1, 1, 64, 32), np.float32), np.zeros((1, 64, 32), np.uint8)):
        with pytest.raises(ValueError):
            pkg.hctr_model._img_args(bad)
    with pytest.raises(ValueError):
        pkg.hctr_model._widths([3, 4], 3)


def test_recognize_symbols_exported_declared_and_bound(pkg):
    lib = pkg.load_library()
    with open(os.path.join(ROOT, "include", "hctr_hip.h")) as f:
        header = f.read()
    _lib = importlib.import_module(PKG + "._lib")
    for name, nargs in (("hctr_recognize", 16), ("hctr_recognize_logits", 15)):
        assert hasattr(lib, name)
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl and decl.group(1).count(",") + 1 == nargs, name
        sig = [s for s in _lib.SIGNATURES if s[0] == name]
        assert len(sig) == 1 and len(sig[0][2]) == nargs, sig
        assert len(getattr(lib, name).argtypes) == nargs
    assert hasattr(pkg.hctr_model, "recognize") and hasattr(pkg.ctc_codec, "recognize")
