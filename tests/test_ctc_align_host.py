"""CPU tests of the forced alignment's surface (hctr_ctc_align*, ``CTCAligner``, ``hctr_model.align``): the float64
yardstick tests/ctc_align_ref.py on planted paths and on the tie table, the host-side result object and target
normalisation, and the C ABI symbols. The device results are checked by tests/test_gpu_ctc_align.py."""
import importlib
import os
import re

import numpy as np
import pytest

import ctc_align_ref as ref
from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def ctc():
    return importlib.import_module(PKG + ".ctc")


@pytest.mark.parametrize("T,C,L", [(40, 11, 0), (40, 11, 1), (150, 50, 30), (150, 50, 75), (600, 7358, 290),
                                   (1100, 64, 1030)])
def test_helper_recovers_planted_paths(T, C, L):
    """noise N(0, 1) plus 12 on the planted class: the float64 Viterbi returns the planted path exactly, the float32
    one agrees, and the score is the planted path's"""
    rng = np.random.RandomState(T + L)
    tg = ref.random_target(rng, C, L, repeat=0.05 if L > 1000 else 0.3)
    logits, states = ref.planted(rng, T, C, tg)
    r64 = ref.viterbi(logits, tg, np.float64)
    r32 = ref.viterbi(logits, tg, np.float32)
    np.testing.assert_array_equal(r64["states"], states)
    np.testing.assert_array_equal(r32["states"], states)
    st, en = ref.spans_of_states(states, L)
    np.testing.assert_array_equal(r64["starts"], st)
    np.testing.assert_array_equal(r64["ends"], en)
    want = ref.path_score64(r64["lp64"], r64["path"])
    assert abs(float(r64["score"]) - want) <= 1e-9 * abs(want) + 1e-9
    assert abs(float(r32["score"]) - want) <= 1e-5 * abs(want) + 1e-3
    np.testing.assert_array_equal(ref.collapse(r64["path"]), tg)
    assert abs(float(r64["logps"].sum()) + float(r64["lp64"][r64["path"] == 0, 0].sum()) - want) <= 1e-9 * abs(want) + 1e-9


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_helper_reproduces_the_tie_table(dtype):
    for T, tg, path in ref.TIE_TABLE:
        r = ref.viterbi(np.zeros((T, 13), np.float32), tg, dtype)
        assert r["path"].tolist() == path, (T, tg)
        assert abs(float(r["score"]) + T * np.log(13.0)) < 1e-4


def test_helper_infeasible_and_forced_lines():
    z = np.random.RandomState(0).standard_normal((3, 5)).astype(np.float32)
    r = ref.viterbi(z, [2, 2], np.float32)                 # needs 3 steps: label, blank, label
    assert r["path"].tolist() == [2, 0, 2] and r["starts"].tolist() == [0, 2] and r["ends"].tolist() == [1, 3]
    r = ref.viterbi(z[:2], [2, 2], np.float32)
    assert np.isneginf(r["score"]) and (r["path"] == -1).all() and (r["starts"] == -1).all()
    assert np.isneginf(r["logps"]).all()
    assert not ref.feasible([2, 2], 2) and ref.feasible([2, 2], 3) and ref.feasible([], 1)


def test_alignment_object_and_normalisation(ctc):
    tg, tl = ctc.normalize_targets(np.array([[4, 4, 0], [7, 0, 0], [0, 0, 0]]), [2, 1, 0], 3)
    assert tg.tolist() == [4, 4, 7] and tl.tolist() == [2, 1, 0] and tg.dtype == np.int32
    tg1, tl1 = ctc.normalize_targets([4, 4, 7], [2, 1, 0], 3)
    assert tg1.tolist() == tg.tolist() and tl1.tolist() == tl.tolist()
    paths = np.array([[4, 0, 4, 4, -1], [0, 7, 7, 7, 0], [0, 0, 0, 0, 0]], np.int32)
    lp = np.log(np.array([0.5, 0.25 * 0.25, 0.125], np.float32))
    a = ctc.CTCAlignment(paths, np.zeros(3, np.float32), np.array([0, 2, 1], np.int32), np.array([1, 4, 4], np.int32),
                         lp, tg, tl)
    assert a.offsets.tolist() == [0, 2, 3, 3] and len(a) == 3
    lines = list(a.lines())
    assert [[(c, s, e) for c, s, e, _ in ln] for ln in lines] == [[(4, 0, 1), (4, 2, 4)], [(7, 1, 4)], []]
    np.testing.assert_allclose([p for ln in lines for _, _, _, p in ln], [0.5, 0.25, 0.5], rtol=1e-6)
    # a line without an alignment: spans -1, confidence 0
    b = ctc.CTCAlignment(np.full((1, 2), -1, np.int32), np.array([-np.inf], np.float32), np.array([-1], np.int32),
                         np.array([-1], np.int32), np.array([-np.inf], np.float32), np.array([3], np.int32), [1])
    assert list(b.lines()) == [[(3, -1, -1, 0.0)]]
    with pytest.raises(NotImplementedError):
        ctc.CTCAligner(blank=1)
    with pytest.raises(ValueError):
        ctc.CTCAligner().to("cpu")


def test_align_symbols_exported_declared_and_bound(pkg):
    lib = pkg.load_library()
    with open(os.path.join(ROOT, "include", "hctr_hip.h")) as f:
        header = f.read()
    _lib = importlib.import_module(PKG + "._lib")
    for name, nargs in (("hctr_ctc_align", 15), ("hctr_ctc_align_logits", 14)):
        assert hasattr(lib, name)
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl and decl.group(1).count(",") + 1 == nargs, name
        sig = [s for s in _lib.SIGNATURES if s[0] == name]
        assert len(sig) == 1 and len(sig[0][2]) == nargs, sig
        assert len(getattr(lib, name).argtypes) == nargs
    assert pkg.CTCAligner is importlib.import_module(PKG + ".ctc").CTCAligner
    assert hasattr(pkg.hctr_model, "align")
