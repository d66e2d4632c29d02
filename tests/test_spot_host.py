"""CPU tests of keyword spotting's surface (hctr_spot*): the float64 yardstick tests/spot_ref.py against enumeration of
all paths, the L = 1 closed form, the automaton tables the library exports (``hctr_spot_automaton``, host only) against
the yardstick's, argument errors, and the host-side result object. The device results are checked by
tests/test_gpu_spot.py."""
import ctypes
import importlib

import numpy as np
import pytest

import spot_ref as ref
from conftest import PKG

FIXED = [[1, 1], [1, 2, 1], [1, 1, 2]]      # aa, aba, aab


def _tiny_cases():
    """>= 50 cases with C <= 4, T <= 7, L <= 3: the fixed queries at several T, one that cannot fit, random ones"""
    rng = np.random.RandomState(7)
    cases = []
    for q in FIXED:
        for T in (3, 5, 6):
            cases.append((3, T, q))
    cases.append((3, 3, [1, 1, 1]))          # L + repeats = 5 > T = 3
    cases.append((4, 2, [2, 2]))             # 3 > 2
    while len(cases) < 56:
        C = int(rng.randint(2, 5))
        T = int(rng.randint(1, 8 if C < 4 else 7))
        L = int(rng.randint(1, 4))
        cases.append((C, T, [int(v) for v in rng.randint(1, C, size=L)]))
    return cases


@pytest.mark.parametrize("i,case", list(enumerate(_tiny_cases())))
def test_oracle_equals_brute_force(i, case):
    C, T, q = case
    lp = ref.log_softmax(np.random.RandomState(100 + i).randn(T, C) * 2.0)
    got, want = ref.contain_logp(lp, q), ref.brute_contain(lp, q)
    seg, bseg = ref.best_segment(lp, q), ref.brute_segment(lp, q)
    rep = sum(q[j] == q[j - 1] for j in range(1, len(q)))
    if len(q) + rep > T:
        assert got == -np.inf and want == -np.inf
        assert seg == (-np.inf, -1, -1) and bseg == (-np.inf, -1, -1)
        return
    assert abs(got - want) <= 1e-12 * abs(want) + 1e-12, (got, want)
    assert abs(seg[0] - bseg[0]) <= 1e-12 * abs(bseg[0]) + 1e-12 and seg[1:] == bseg[1:], (seg, bseg)
    assert got >= seg[0] - 1e-12
    assert abs(ref.segment_score(lp, q, seg[1], seg[2]) - seg[0]) <= 1e-12


def test_unfit_cases_present():
    assert sum(len(q) + sum(q[j] == q[j - 1] for j in range(1, len(q))) > T for _, T, q in _tiny_cases()) >= 2
    assert all(any(q == f for _, _, q in _tiny_cases()) for f in FIXED)


def test_closed_form_of_one_character():
    rng = np.random.RandomState(3)
    lp = ref.log_softmax(rng.randn(40, 9) * 3.0)
    for c in (1, 5, 8):
        want = np.log1p(-np.exp(np.log1p(-np.exp(lp[:, c])).sum()))
        assert abs(ref.contain_logp(lp, [c]) - want) <= 1e-12 * abs(want)
        s, t0, t1 = ref.best_segment(lp, [c])
        assert (s, t0, t1) == (lp[:, c].max(), int(lp[:, c].argmax()), int(lp[:, c].argmax()) + 1)
    assert ref.contain_logp(lp[:0], [1]) == -np.inf and ref.best_segment(lp[:0], [1]) == (-np.inf, -1, -1)


def test_tie_rule_on_equal_columns():
    """all columns equal: every segment of a length scores the same; the shortest wins, at the earliest end"""
    lp = ref.log_softmax(np.zeros((9, 5)))
    for q, n in (([1], 1), ([1, 2], 2), ([1, 1], 3), ([1, 2, 1], 3), ([2, 2, 2], 5)):
        s, t0, t1 = ref.best_segment(lp, q)
        assert (t0, t1) == (0, n) and abs(s + n * np.log(5)) < 1e-12


# ---- the library's tables (host only: no GPU, no context) ----
@pytest.fixture(scope="module")
def lib():
    return importlib.import_module(PKG + "._lib")


def _lib_automaton(lib, q):
    q = np.ascontiguousarray(q, np.int32)
    L = int(q.size)
    cap = 2080
    classes, delta = np.full(32, -1, np.int32), np.full(32 * 32, -1, np.int32)
    ptr, src, slot = np.full(2 * 32 + 1, -1, np.int32), np.full(cap, -1, np.int32), np.full(cap, -1, np.int32)
    mask = np.zeros(64, np.uint64)
    nq, ns, ne = ctypes.c_int32(-1), ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = lib.load().hctr_spot_automaton(lib.ptr(q), L, lib.ptr(classes), ctypes.byref(nq), lib.ptr(delta), ctypes.byref(ns),
                                        lib.ptr(ptr), lib.ptr(src), lib.ptr(slot), cap, ctypes.byref(ne), lib.ptr(mask))
    if rc:
        return rc
    n, S, E = nq.value, ns.value, ne.value
    return dict(classes=classes[:n].tolist(), delta=delta[:L * n].reshape(L, n).tolist(), num_states=S,
                in_ptr=ptr[:S + 1].tolist(), in_src=src[:E].tolist(), in_slot=slot[:E].tolist(),
                fall_mask=[int(v) for v in mask[:S]])


def _queries():
    rng = np.random.RandomState(11)
    return {"a": [7], "aa": [7, 7], "abab": [3, 9, 3, 9], "aabaa": [4, 4, 6, 4, 4],
            "random32": rng.randint(1, 12, size=32).tolist(), "distinct32": list(range(40, 8, -1)),
            "equal32": [5] * 32}


@pytest.mark.parametrize("name", sorted(_queries()))
def test_library_automaton_equals_oracle(lib, name):
    q = _queries()[name]
    got, want = _lib_automaton(lib, q), ref.automaton(q)
    assert got == want
    assert got["num_states"] == 2 * len(q) and len(got["in_src"]) <= 2080
    assert got["in_ptr"][1] == 0                      # Z is fed by the fall masks, not by edges
    # every (state, slot) pair of a live state goes somewhere exactly once: an edge or the fall mask
    nq, S = len(got["classes"]), got["num_states"]
    out = {}
    for s in range(S):
        for e in range(got["in_ptr"][s], got["in_ptr"][s + 1]):
            out.setdefault(got["in_src"][e], []).append(got["in_slot"][e])
    for s in range(S - 1):
        slots = sorted(out.get(s, []) + [b for b in range(nq + 3) if got["fall_mask"][s] >> b & 1])
        assert slots == list(range(nq + 2)), (s, slots)
    assert out[S - 1] == [nq + 2] and got["fall_mask"][S - 1] == 0


@pytest.mark.parametrize("name", ["aa", "abab", "aabaa", "random32"])
def test_library_tables_drive_the_recursion(lib, name):
    """the kernel's recursion restated over the exported tables - in-edges for every state but Z, Z from the fall
    masks, rest = max(0, 1 - the seen probabilities) from float32 emissions - gives the oracle's posterior"""
    q = _queries()[name]
    a = _lib_automaton(lib, q)
    rng = np.random.RandomState(len(q))
    T, C = 3 * len(q) + 5, 14
    z = rng.randn(T, C)
    path = [c for ch in q for c in (ch, ch, 0)]
    z[np.arange(len(path)) + 2, path] += 9.0
    lp = ref.log_softmax(z)
    nq, S = len(a["classes"]), a["num_states"]
    st = np.zeros(S)
    st[0] = 1.0
    for t in range(T):
        p = np.exp(lp[t, [0] + a["classes"]].astype(np.float32).astype(np.float64))
        p = np.concatenate([p, [max(0.0, 1.0 - p.sum()), 1.0]])
        new = np.zeros(S)
        new[0] = sum(st[s] * sum(p[b] for b in range(nq + 2) if a["fall_mask"][s] >> b & 1) for s in range(S))
        for s in range(1, S):
            new[s] = sum(st[a["in_src"][e]] * p[a["in_slot"][e]] for e in range(a["in_ptr"][s], a["in_ptr"][s + 1]))
        st = new
        assert abs(st.sum() - 1.0) < 1e-5
    want = ref.contain_logp(lp, q)
    assert want > -5.0 and abs(np.log(st[S - 1]) - want) <= 1e-5 * abs(want) + 1e-5


def test_known_delta(lib):
    a = _lib_automaton(lib, [3, 9, 3, 9])             # abab over classes (a=3, b=9)
    assert a["classes"] == [3, 9]
    assert a["delta"] == [[1, 0], [1, 2], [3, 0], [1, 4]]
    a = _lib_automaton(lib, [4, 4, 6, 4, 4])          # aabaa
    assert a["delta"] == [[1, 0], [2, 0], [2, 3], [4, 0], [5, 0]]


def test_automaton_bad_arguments(lib):
    assert _lib_automaton(lib, [1] * 33) == lib.ERR_ARG
    assert _lib_automaton(lib, [1, 0, 2]) == lib.ERR_ARG
    assert _lib_automaton(lib, [1, -4]) == lib.ERR_ARG
    L = lib.load()
    q = np.array([1, 2], np.int32)
    assert L.hctr_spot_automaton(lib.ptr(q), 0, None, None, None, None, None, None, None, 0, None, None) == lib.ERR_ARG
    assert L.hctr_spot_automaton(None, 2, None, None, None, None, None, None, None, 0, None, None) == lib.ERR_ARG
    src = np.zeros(2, np.int32)
    assert L.hctr_spot_automaton(lib.ptr(q), 2, None, None, None, None, None, lib.ptr(src), None, 2, None, None) == lib.ERR_ARG
    assert b"edge_cap" in L.hctr_last_error(None)
    ne = ctypes.c_int32(-1)
    assert L.hctr_spot_automaton(lib.ptr(q), 2, None, None, None, None, None, None, None, 0, ctypes.byref(ne), None) == 0
    assert ne.value == len(ref.automaton([1, 2])["in_src"])


def test_chunk_cap_is_readable(lib, monkeypatch):
    L = lib.load()
    monkeypatch.delenv("HCTR_SPOT_CLASSES", raising=False)
    assert L.hctr_spot_chunk_classes(64, 2000) == (256 << 20) // (4 * 64 * 2000)
    assert L.hctr_spot_chunk_classes(1, 16) == 1024 and L.hctr_spot_chunk_classes(100000, 2000) == 64
    monkeypatch.setenv("HCTR_SPOT_CLASSES", "4")
    assert L.hctr_spot_chunk_classes(64, 2000) == 4


# ---- the Python surface that needs no device ----
def test_spotting_result_object():
    ctc = importlib.import_module(PKG + ".ctc")
    logp = np.log(np.array([[0.9, 0.2], [0.6, 1.0]], np.float32))
    r = ctc.Spotting(logp, logp - 1, np.array([[3, -1], [0, 7]], np.int32), np.array([[5, -1], [2, 9]], np.int32))
    assert len(r) == 2 and r.probs().shape == (2, 2) and abs(float(r.probs()[0, 0]) - 0.9) < 1e-6
    hits = r.hits(0.5)
    assert [(h[0], h[1]) for h in hits] == [(0, 0), (1, 0), (1, 1)]
    assert hits[0][3:] == (3, 5) and abs(hits[2][2] - 1.0) < 1e-6
    assert [len(x) for x in r.lines()] == [2, 2] and list(r.lines())[0][1][2:] == (-1, -1)


def test_normalize_queries():
    ctc = importlib.import_module(PKG + ".ctc")
    flat, ql = ctc.normalize_queries([[1, 2], [3], np.array([4, 4, 4])])
    assert flat.dtype == np.int32 and flat.tolist() == [1, 2, 3, 4, 4, 4] and ql.tolist() == [2, 1, 3]
    with pytest.raises(ValueError):
        ctc.normalize_queries([])
    with pytest.raises(ValueError):
        ctc.normalize_queries([[1], []])
    with pytest.raises(ValueError):
        ctc.normalize_queries([list(range(1, 34))])


def test_codec_rejects_characters_outside_the_vocabulary():
    codec = importlib.import_module(PKG + ".codec")
    c = codec.ctc_codec(["a", "b", "c"])
    flat, ql = c.encode_queries(["ab", "c"])
    assert ql.tolist() == [2, 1] and flat.tolist() == c.encode(["ab", "c"])[0].tolist()
    with pytest.raises(ValueError):
        c.encode_queries(["az"])
    with pytest.raises(ValueError):
        c.encode_queries([""])
