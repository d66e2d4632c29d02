"""CPU tests of the evaluation's surface (hctr_edit_distance / hctr_evaluate*, ``hctr_model.evaluate``,
``ctc_codec.evaluate``, ``Evaluation``): the numpy yardstick tests/edit_ref.py against the oracle's two-row loop, the
contract's known answers, identities and map consistency; the lane-skewed schedule the kernel runs, emulated; the
host-side result object; the C ABI symbols. The device results are checked by tests/test_gpu_evaluate.py."""
import importlib
import importlib.util
import os
import re
import time

import numpy as np
import pytest

import edit_ref as ref
from conftest import PKG, ROOT
from oracle import ctc_ref


@pytest.fixture(scope="module")
def ctc():
    return importlib.import_module(PKG + ".ctc")


def _codes(s):
    return [ord(ch) for ch in s]


def _pairs(n, seed, alphabets=(2, 5, 7000), max_len=40):
    rng = np.random.RandomState(seed)
    for k in range(n):
        A = alphabets[k % len(alphabets)]
        yield rng.randint(0, A, rng.randint(0, max_len)), rng.randint(0, A, rng.randint(0, max_len))


def test_ref_against_the_oracle_loop():
    for r, h in _pairs(300, 1):
        assert ref.align(r, h)[0] == ctc_ref.edit_distance(h.tolist(), r.tolist()) == int(ref.table(r, h)[-1, -1])


def test_known_answers():
    e, c, rm, hm = ref.align(_codes("kitten"), _codes("sitting"))
    assert (e, c.tolist(), hm.tolist(), rm.tolist()) == (3, [4, 2, 0, 1], [0, 1, 2, 3, 4, 5, -1], [0, 1, 2, 3, 4, 5])
    e, c, rm, hm = ref.align(_codes("ab"), _codes("ba"))       # the tie rule: two substitutions, not delete + insert
    assert (e, c.tolist(), rm.tolist(), hm.tolist()) == (2, [0, 2, 0, 0], [0, 1], [0, 1])
    e, c, rm, hm = ref.align([], [5, 6, 7])
    assert (e, c.tolist(), rm.tolist(), hm.tolist()) == (3, [0, 0, 0, 3], [], [-1, -1, -1])
    e, c, rm, hm = ref.align([5, 6], [])
    assert (e, c.tolist(), rm.tolist(), hm.tolist()) == (2, [0, 0, 2, 0], [-1, -1], [])
    assert ref.align([], [])[0] == 0


def test_identities_and_map_consistency():
    for r, h in _pairs(300, 2):
        e, (hits, S, D, I), rm, hm = ref.align(r, h)
        assert hits + S + D == len(r) and hits + S + I == len(h) and S + D + I == e
        at = np.flatnonzero(rm >= 0)
        assert (hm[rm[at]] == at).all() and (rm[hm[hm >= 0]] == np.flatnonzero(hm >= 0)).all()      # inverse maps
        assert (np.diff(rm[at]) > 0).all() and (np.diff(hm[hm >= 0]) > 0).all()                     # increasing
        assert int((r[at] == h[rm[at]]).sum()) == hits and len(at) == hits + S
        assert int((rm < 0).sum()) == D and int((hm < 0).sum()) == I


def test_the_skewed_schedule_is_the_row_recursion():
    """the kernel's schedule (rows per lane NS, a step per anti-diagonal of lanes), emulated lane by lane"""
    for NS in (1, 2, 4):
        for r, h in _pairs(100, 3 + NS, max_len=30):
            assert ref.skewed(r, h, NS) == ref.align(r, h)[0], (NS, r, h)


def test_ref_is_quick_at_the_limit():
    rng = np.random.RandomState(4)
    r, h = rng.randint(0, 50, 2047), rng.randint(0, 50, 2047)
    t0 = time.perf_counter()
    e, c, rm, hm = ref.align(r, h)
    dt = time.perf_counter() - t0
    print("2047 x 2047 in %.3f s" % dt)
    assert c[1] + c[2] + c[3] == e and dt < 1.0


def test_batch_layout():
    hyp = np.array([[1, 2, 3, 9], [4, 4, 9, 9]], np.int32)
    out = ref.batch(hyp, [3, 2], [1, 3, 4, 5, 4], [2, 3])
    assert out["edits"].tolist() == [1, 1] and out["counts"].tolist() == [[2, 0, 0, 1], [2, 0, 1, 0]]
    assert out["ref_map"].tolist() == [0, 2, 0, -1, 1] and out["hyp_map"].tolist() == [[0, -1, 1, 0], [0, 2, 0, 0]]


def _evaluation(ctc, hyps, refs):
    lab, n = ctc.pad_sequences(hyps)
    tl = np.array([len(r) for r in refs], np.int32)
    tg = np.concatenate([np.asarray(_codes(r) if isinstance(r, str) else r, np.int32) for r in refs] + [np.zeros(0, np.int32)])
    out = ref.batch(lab, n, tg, tl)
    return ctc.Evaluation(out["edits"], out["counts"], out["ref_map"], out["hyp_map"], lab, n, tg.astype(np.int32), tl)


def test_evaluation_rates_and_confusions(ctc):
    ev = _evaluation(ctc, ["sitting", "ba", "", "abc"], ["kitten", "ab", "xy", "abc"])
    assert len(ev) == 4 and ev.edits.tolist() == [3, 2, 2, 0]
    assert ev.total_chars == 13 and ev.total_edits == 7 and ev.totals == (7, 4, 2, 1)
    assert ev.cer == 7 / 13 and ev.cr == (13 - 2 - 4) / 13 and ev.ar == (13 - 2 - 4 - 1) / 13
    o = ord
    assert ev.confusions() == {(o("k"), o("s")): 1, (o("e"), o("i")): 1, (o("a"), o("b")): 1, (o("b"), o("a")): 1}
    lines = list(ev.lines())
    assert lines[0][0] == (o("k"), o("s"), 0, 0) and lines[0][-1] == (None, o("g"), -1, 6) and len(lines[0]) == 7
    assert lines[2] == [(o("x"), None, 0, -1), (o("y"), None, 1, -1)] and len(lines[3]) == 3
    # test.py's figure for the same pairs
    spec = importlib.util.spec_from_file_location("hctr_test_cli", os.path.join(ROOT, "test.py"))
    test_py = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(test_py)
    pairs = list(zip(["sitting", "ba", "", "abc"], ["kitten", "ab", "xy", "abc"]))
    assert ev.cer == sum(test_py.edit_distance(p, t) for p, t in pairs) / sum(len(t) for _, t in pairs)
    empty = _evaluation(ctc, [], [])
    assert len(empty) == 0 and np.isnan(empty.cer)
    only = ctc.Evaluation(ev.edits, None, None, None, None, ev.lengths, ev.targets, ev.target_lengths)
    assert only.cer == ev.cer
    with pytest.raises(ValueError):
        only.cr
    with pytest.raises(ValueError):
        only.confusions()


def test_pad_sequences_and_argument_checks(ctc):
    lab, n = ctc.pad_sequences(["ab", "", [7, -3, 2 ** 31 - 1]])
    assert lab.tolist() == [[97, 98, 0], [0, 0, 0], [7, -3, 2 ** 31 - 1]] and n.tolist() == [2, 0, 3]
    assert ctc.pad_sequences([])[0].shape == (0, 1)
    with pytest.raises(ValueError):
        ctc.edit_distance_sequences(None, ["a"], ["a", "b"])
    with pytest.raises(ValueError):
        ctc.edit_distance_labels(None, np.zeros((2, 3), np.int32), [1], [1], [1])


def test_evaluate_symbols_exported_declared_and_bound(pkg):
    lib = pkg.load_library()
    with open(os.path.join(ROOT, "include", "hctr_hip.h")) as f:
        header = f.read()
    _lib = importlib.import_module(PKG + "._lib")
    for name, nargs in (("hctr_edit_distance", 11), ("hctr_evaluate", 15), ("hctr_evaluate_logits", 14)):
        assert hasattr(lib, name)
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert decl and decl.group(1).count(",") + 1 == nargs, name
        sig = [s for s in _lib.SIGNATURES if s[0] == name]
        assert len(sig) == 1 and len(sig[0][2]) == nargs, sig
    assert hasattr(pkg.hctr_model, "evaluate") and hasattr(pkg.ctc_codec, "evaluate")
    assert callable(pkg.edit_distance) and pkg.Evaluation is importlib.import_module(PKG + ".ctc").Evaluation
