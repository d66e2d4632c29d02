"""CPU tests of the set form of a pattern (``hctr_pat_build_sets``, ``Pattern.from_sets``, ``Pattern.compile(sets=)``):
the float64 yardstick of the block recursion (tests/pattern_set_ref.py) against the explicit form's yardstick
(tests/pattern_ref.py) on the expanded automaton, the compiler's set arcs against ``re.fullmatch``, the state counts of
both forms, the builder's errors and limits, and which form ``compile`` chooses at the full vocabulary. The device
results are checked by tests/test_gpu_pattern_set.py."""
import importlib
import itertools
import re

import numpy as np
import pytest

import pattern_ref
import pattern_set_ref as ref
from test_pattern_host import ALPHABET, EXPRESSIONS, SPELLINGS

SIX = "abcdef"                                   # the 6-label alphabet of the yardstick cases


@pytest.fixture(scope="module")
def ctc(pkg):
    return importlib.import_module(pkg.__name__ + ".ctc")


@pytest.fixture(scope="module")
def codec4(pkg):
    return pkg.ctc_codec(ALPHABET)


@pytest.fixture(scope="module")
def codec6(pkg):
    return pkg.ctc_codec(SIX)


@pytest.fixture(scope="module")
def codec_full(pkg):
    cd = pkg.ctc_codec("".join(chr(0x4E00 + i) for i in range(7356)))
    assert len(cd.characters) == 7358 and "年" in cd.dict
    return cd


def dfa(pat):
    return pat.arcs, pat.sets, pat.finals, pat.num_states


@pytest.mark.parametrize("expr", [".", ".{2,4}", ".*a.*", "[^ab]+a{2}", "(.a)*"])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
def test_yardstick_equals_the_explicit_yardstick_on_expanded_arcs(expr, T, ctc, codec6):
    pat = ctc.Pattern.compile(expr, codec6, sets=True)
    assert pat.kind == 1
    C = len(SIX) + 2
    rng = np.random.RandomState(900 + T)
    want_t = pattern_ref.tables(pat.expanded_arcs(), pat.finals, pat.num_states)
    got_t = ref.tables(*dfa(pat))
    assert got_t["S"] == len(want_t["state_label"]) and got_t["state_label"].tolist() == want_t["state_label"].tolist()
    assert got_t["start"].tolist() == want_t["start"].tolist()
    feasible = 0
    for scale in (1.0, 4.0, 0.0):                                     # 0: every score ties, the tie rule alone decides
        lp = pattern_ref.log_softmax(rng.randn(T, C) * scale)
        want, got = pattern_ref.recurse(lp, want_t), ref.recurse(lp, got_t)
        if want[2] is None:
            assert got[0] == -np.inf and got[1] == -np.inf and got[2] is None
            continue
        feasible += 1
        assert abs(got[0] - want[0]) <= 1e-12 and abs(got[1] - want[1]) <= 1e-12, (expr, T, got[:2], want[:2])
        assert got[2] == want[2], (expr, T, scale)
    # infeasible lengths: two characters on one column; "xaa" needs a blank between the two a
    assert (feasible == 0) == ((expr, T) in ((".{2,4}", 1), ("[^ab]+a{2}", 1), ("[^ab]+a{2}", 2), ("[^ab]+a{2}", 3)))


def test_cases_include_infeasible_lengths_and_a_final_start(ctc, codec6):
    lp = pattern_ref.log_softmax(np.zeros((1, 8)))
    assert ref.recurse(lp, ref.tables(*dfa(ctc.Pattern.compile(".{2,4}", codec6, sets=True))))[2] is None
    t = ref.tables(*dfa(ctc.Pattern.compile("(.a)*", codec6, sets=True)))
    assert 0 in t["finals"] and ref.recurse(lp, t)[2] == [0]


def all_strings(n=6):
    return ["".join(s) for k in range(n + 1) for s in itertools.product(ALPHABET, repeat=k)]


@pytest.mark.parametrize("expr", EXPRESSIONS + [e for pair in SPELLINGS for e in pair])
def test_set_compiler_accepts_what_re_fullmatch_accepts(expr, ctc, codec4):
    pat = ctc.Pattern.compile(expr, codec4, sets=True)
    assert pat.kind == 1
    d = {}
    for p, k, q in pat.arcs:
        for c in pat.sets[k]:
            assert (int(p), int(c)) not in d
            d[(int(p), int(c))] = int(q)
    fin = set(int(f) for f in pat.finals)
    want = re.compile(expr)
    for s in all_strings():
        q = 0
        for ch in s:
            q = d.get((q, codec4.dict[ch]), -1)
            if q < 0:
                break
        assert (q in fin) == (want.fullmatch(s) is not None), (expr, s)
    assert all(1 <= c <= len(ALPHABET) for v in pat.sets for c in v)          # <unknown> is never matched
    # the same automaton as the explicit form's, and the same counts
    ex = ctc.Pattern.compile(expr, codec4, sets=False)
    assert ex.kind == 0 and pat.expanded_arcs().tobytes() == ex.arcs.tobytes() == ex.expanded_arcs().tobytes()
    a, b = pat.info(), ex.info()
    assert (a["dfa_states"], a["states"], a["classes"]) == (b["dfa_states"], b["states"], b["classes"])
    assert ctc.Pattern.compile(expr, codec4).kind == 0                       # the default keeps the explicit form


def test_info_and_tables_of_the_set_form(ctc, codec6):
    pat = ctc.Pattern.compile(".*a.*", codec6, sets=True)
    t = ref.tables(*dfa(pat))
    i = pat.info()
    deg = np.bincount(t["arc_state"], minlength=t["S"])
    assert i == {"dfa_states": 2, "states": t["S"], "edges": len(t["arc_state"]), "classes": 6, "max_in_degree": int(deg.max())}
    assert i["states"] == 2 + 5 + 6 and i["edges"] == 5 + 1 + 6 and i["max_in_degree"] == 2
    with pytest.raises(ValueError, match="no edge list"):
        pat.tables()


def test_pruning_and_parallel_arcs(ctc):
    # two arcs between one pair of states, an unreachable state 2 and a dead end 3
    sets = [[1, 2], [4], [3], [5]]
    arcs = [(0, 0, 1), (0, 1, 1), (1, 2, 1), (2, 0, 1), (0, 3, 3), (3, 3, 3)]
    pat = ctc.Pattern.from_sets(arcs, sets, [1], 4, 6)
    ex = ctc.Pattern(pat.expanded_arcs(), [1], 4, 6)
    assert pat.info()["dfa_states"] == 2 == ex.info()["dfa_states"] and pat.info()["states"] == ex.info()["states"] == 6
    lp = pattern_ref.log_softmax(np.random.RandomState(905).randn(7, 6))
    want = pattern_ref.recurse(lp, pattern_ref.tables(pat.expanded_arcs(), [1], 4))
    got = ref.recurse(lp, ref.tables(arcs, sets, [1], 4))
    assert abs(got[0] - want[0]) <= 1e-12 and abs(got[1] - want[1]) <= 1e-12 and got[2] == want[2]


def test_builder_errors(ctc):
    def message(arcs, sets, finals, nq, C):
        with pytest.raises(ValueError) as e:
            ctc.Pattern.from_sets(arcs, sets, finals, nq, C)
        return str(e.value)

    ok, one = [(0, 0, 1)], [[1, 2]]
    msgs = [message(ok, [[]], [1], 2, 6), message(ok, [[0, 1]], [1], 2, 6), message(ok, [[1, 6]], [1], 2, 6),
            message(ok, [[2, 1]], [1], 2, 6), message(ok, [[1, 1]], [1], 2, 6),
            message([(0, 0, 1), (0, 1, 0)], [[1, 2], [2, 3]], [1], 2, 6), message(ok, one, [], 2, 6),
            message([(0, 0, 2)], one, [1], 2, 6), message([(0, 1, 1)], one, [1], 2, 6), message(ok, one, [1], 0, 6),
            message(ok, one, [2], 2, 6)]
    words = ("set 0 is empty", "label 0", "label 6", "not ascending", "not ascending", "overlap on label 2", "empty",
             "outside [0,1]", "names set 1", "num_states >= 1", "finals[0]=2")
    for m, word in zip(msgs, words):
        assert word in m and "hctr_pat_build_sets" in m, (word, m)
    assert len(set(msgs)) == len(msgs)
    # the limits, each naming its figure
    full = [list(range(1, 7357))]
    m = message([(i, 0, i + 1) for i in range(9)], full, [9], 10, 7358)
    assert "65535" in m and "HCTR_PATSET_MAX_STATES" in m
    m = message([(i, 0, i + 1) for i in range(4100)], [[1]], [4100], 4101, 6)
    assert "4096" in m and "HCTR_PATSET_MAX_DFA_STATES" in m and "4101 DFA states" in m
    # 1200 states, each entered from 40 states on its own 40 labels: 49 200 CTC states, 1 920 000 in-arcs
    n = 1200
    sets = [list(range(1 + 40 * j, 41 + 40 * j)) for j in range(40)]
    m = message([(p, q % 40, q) for p in range(n) for q in ((p + 1 + j) % n for j in range(40))], sets, [0], n, 1602)
    assert "HCTR_PATSET_MAX_INARCS is 1048576" in m, m


def test_full_vocabulary_builds_as_sets(ctc, codec_full):
    for expr, dfa_states, states in ((".{2,4}", 5, 5 + 4 * 7356), (".*年.*", 2, 2 + 7355 + 7356)):
        pat = ctc.Pattern.compile(expr, codec_full)                          # sets=None: the explicit build is refused
        assert pat.kind == 1
        i = pat.info()
        assert (i["dfa_states"], i["states"], i["classes"]) == (dfa_states, states, 7356), (expr, i)
        with pytest.raises(ValueError, match="HCTR_PAT_MAX_STATES is 8192"):
            ctc.Pattern.compile(expr, codec_full, sets=False)
    assert ctc.Pattern.compile(".*年.*", codec_full).info()["edges"] == 7355 + 2 + 7355
    assert ctc.Pattern.compile(".", codec_full).kind == 0              # within the explicit limits: unchanged
    for sets in (None, True):
        with pytest.raises(ValueError, match="65535"):
            ctc.Pattern.compile(".{9}", codec_full, sets=sets)
