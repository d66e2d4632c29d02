"""CPU tests of pattern-constrained recognition's host side (hctr_pat_*, ``Pattern``): the regular-expression compiler
against ``re.fullmatch``, the float64 yardstick tests/pattern_ref.py against enumeration of all paths and against the
family's other yardsticks (torch's float64 ctc_loss, tests/lexicon_ref.py, tests/spot_ref.py), the tables the library
exports (``hctr_pat_tables``, host only) against the yardstick's, and the builder's errors. The device results are
checked by tests/test_gpu_pattern.py."""
import importlib
import itertools
import re

import numpy as np
import pytest
import torch

import lexicon_ref
import pattern_ref as ref
import spot_ref

ALPHABET = "ab12"
EXPRESSIONS = [
    "ab", "a|b", "(a|b)+1?", "a*", "(ab)*", "a{2,4}", "a{3}", "a{2,}", r"\d{2}", r"[ab]\d", "[^a]+",
    "(a(b|1)){1,2}2?",                  # nested groups
    "(a?b)?12",                         # an optional prefix
    ".{0,3}", "a.b", "[a-b]+[1-2]", "((a|b)(1|2))*a", "(a|ab)(1|b1)",
    "(a|b)*ab(a|b)*",                   # a cycle around a literal
    r"\d+(a\d+)?", r"[^\d]{1,2}", "(?:a|b){2}1*", "a{,2}b", "(a|b|1|2)*", r"(1|2){2}(a|b)?\d",
]
SPELLINGS = [("a+b+", "aa*bb*"), (r"\d{2}", "(1|2)[12]"), ("(a|b)*", "(a*b*)*"), ("(ab|a1)2?", "a(b|1)(2|)")]


@pytest.fixture(scope="module")
def ctc(pkg):
    return importlib.import_module(pkg.__name__ + ".ctc")


@pytest.fixture(scope="module")
def codec(pkg):
    return pkg.ctc_codec(ALPHABET)


def all_strings(n=6):
    return ["".join(s) for k in range(n + 1) for s in itertools.product(ALPHABET, repeat=k)]


def same_tables(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in set(a) | set(b) if k != "nQ")


@pytest.mark.parametrize("expr", EXPRESSIONS + [e for pair in SPELLINGS for e in pair])
def test_compiler_accepts_what_re_fullmatch_accepts(expr, ctc, codec):
    pat = ctc.Pattern.compile(expr, codec)
    d = {(int(p), int(c)): int(q) for p, c, q in pat.arcs}
    fin = set(int(f) for f in pat.finals)
    want = re.compile(expr)
    n_acc = 0
    for s in all_strings():
        q = 0
        for ch in s:
            q = d.get((q, codec.dict[ch]), -1)
            if q < 0:
                break
        got = q in fin
        assert got == (want.fullmatch(s) is not None), (expr, s)
        n_acc += got
    assert n_acc > 0
    assert all(1 <= c <= len(ALPHABET) for _, c, _ in pat.arcs)          # <unknown> is never matched


def test_expressions_cover_the_cases():
    assert len(EXPRESSIONS) >= 20
    assert any(re.fullmatch(e, "") for e in EXPRESSIONS) and any("[^" in e for e in EXPRESSIONS)
    assert any("{1,2}" in e or "{2,4}" in e for e in EXPRESSIONS) and any("((" in e for e in EXPRESSIONS)


@pytest.mark.parametrize("e1,e2", SPELLINGS)
def test_two_spellings_of_one_language_give_identical_tables(e1, e2, ctc, codec):
    p1, p2 = ctc.Pattern.compile(e1, codec), ctc.Pattern.compile(e2, codec)
    assert p1.arcs.tobytes() == p2.arcs.tobytes() and p1.finals.tobytes() == p2.finals.tobytes()
    assert p1.info() == p2.info() and same_tables(p1.tables(), p2.tables())


def test_sizes_of_digit_chains(ctc, pkg):
    cd = pkg.ctc_codec("0123456789")
    for n, states, edges in ((8, 89, 879), (18, 199, 2089)):
        i = ctc.Pattern.compile(r"\d{%d}" % n, cd).info()
        assert (i["dfa_states"], i["states"], i["edges"], i["classes"], i["max_in_degree"]) == (n + 1, states, edges, 10, 11)


def test_compiler_errors(ctc, codec):
    for expr, word in (("ax", "vocabulary"), ("(ab", "missing"), ("ab)", "unbalanced"), ("a**", "quantifier"),
                       ("*a", "unexpected"), (r"\w", "escape"), ("a{3,2}", "n < m"), ("[b-a]", "range")):
        with pytest.raises(ValueError, match=word):
            ctc.Pattern.compile(expr, codec)
    with pytest.raises(ValueError, match="empty"):
        ctc.Pattern.compile("a[^ab12]", codec)


# ---- the yardstick against enumeration of all C^T paths ----
TINY = [
    # (arcs, finals, num_states): (a|b)+c?, a literal with a doubled label, a chain of three of {1, 2}, (12)*, a|ab|abc
    ([(0, 1, 1), (0, 2, 1), (1, 1, 1), (1, 2, 1), (1, 3, 2)], [1, 2], 3),
    ref.literal([1, 1, 2]),
    ([(i, c, i + 1) for i in range(3) for c in (1, 2)], [3], 4),
    ([(0, 1, 1), (1, 2, 0)], [0], 2),
    ref.trie([[1], [1, 2], [1, 2, 3]]),
]


@pytest.mark.parametrize("i", range(len(TINY)))
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
def test_reference_equals_enumeration(i, T):
    arcs, finals, nq = TINY[i]
    lp = ref.log_softmax(np.random.RandomState(700 + 10 * i + T).randn(T, 4) * 2.0)
    logp, best, path = ref.recurse(lp, ref.tables(arcs, finals, nq))
    want_logp, want_best, want_paths = ref.enumerate_paths(lp, arcs, finals)
    if want_best == -np.inf:
        assert logp == -np.inf and best == -np.inf and path is None
        return
    assert abs(logp - want_logp) <= 1e-12 and abs(best - want_best) <= 1e-12
    assert len(want_paths) == 1 and path == want_paths[0]


def test_tiny_cases_include_infeasible_lengths():
    lp = ref.log_softmax(np.zeros((2, 4)))
    assert ref.recurse(lp, ref.tables(*TINY[1]))[0] == -np.inf and ref.recurse(lp, ref.tables(*TINY[2]))[0] == -np.inf
    assert ref.recurse(lp[:1], ref.tables(*TINY[3]))[0] > -np.inf          # the start state is final: all blanks


# ---- relations to the family's other yardsticks ----
def test_literal_pattern_equals_torch_ctc_loss():
    rng = np.random.RandomState(710)
    C, T = 9, 40
    lp = ref.log_softmax(rng.randn(T, C) * 2.0)
    for text in ([3], [1, 1, 2, 2, 2, 5], list(rng.randint(1, C, size=20)), [4] * 21):
        logp = ref.recurse(lp, ref.tables(*ref.literal(text)))[0]
        nll = torch.nn.functional.ctc_loss(torch.from_numpy(lp)[:, None, :], torch.tensor([text]), torch.tensor([T]),
                                           torch.tensor([len(text)]), blank=0, reduction="none").item()
        if np.isinf(nll):
            assert logp == -np.inf and text == [4] * 21
        else:
            assert abs(logp + nll) <= 1e-10


def test_union_of_literals_equals_the_lexicon_yardstick():
    rng = np.random.RandomState(711)
    C, T = 7, 30
    es = sorted(set(tuple(int(v) for v in rng.randint(1, C, size=rng.randint(1, 6))) for _ in range(60)))
    z = rng.randn(T, 1, C) * 2.0
    want = lexicon_ref.logsumexp(lexicon_ref.scores(z, es)[0])
    got = ref.run(z, *ref.trie(es))[0][0]
    assert abs(got - want) <= 1e-10


def test_pattern_of_every_text_has_probability_one():
    rng = np.random.RandomState(712)
    C = 5
    arcs = [(0, c, 0) for c in range(1, C)]
    for T in (1, 2, 17):
        logp = ref.run(rng.randn(T, 1, C) * 3.0, arcs, [0], 1)[0][0]
        assert abs(logp) <= 1e-12


def test_contains_pattern_equals_the_spotting_yardstick():
    rng = np.random.RandomState(713)
    C, T = 6, 24
    lp = ref.log_softmax(rng.randn(T, C) * 2.0)
    for q in ([2], [1, 2], [3, 3], [1, 2, 1, 3], [2, 2, 2]):
        got = ref.recurse(lp, ref.tables(*ref.contains(q, C)))[0]
        assert abs(got - spot_ref.contain_logp(lp, q)) <= 1e-10, q


# ---- the exported tables ----
def dfa_with_dead_ends():
    """(a|b)+c? over C = 6 with an unreachable state 3, a dead end 4 (reachable, cannot finish) and arcs among them"""
    return ([(0, 1, 1), (0, 2, 1), (1, 1, 1), (1, 2, 1), (1, 3, 5), (3, 1, 1), (3, 2, 3), (0, 4, 4), (4, 4, 4), (1, 5, 4)],
            [1, 5], 6)


@pytest.mark.parametrize("dfa", [dfa_with_dead_ends(), ref.trie([[1, 2, 3], [1, 2], [4, 4, 1], [2]]), ref.contains([1, 2, 1], 6),
                                 ([(0, c, 0) for c in range(1, 6)], [0], 1)])
def test_exported_tables_equal_the_reference_builder(dfa, ctc):
    arcs, finals, nq = dfa
    pat = ctc.Pattern(arcs, finals, nq, 6)
    want, got, info = ref.tables(arcs, finals, nq), pat.tables(), pat.info()
    assert same_tables(want, got)
    deg = np.diff(got["in_ptr"])
    assert info == {"dfa_states": want["nQ"], "states": len(got["state_label"]), "edges": len(got["in_src"]),
                    "classes": len(got["classes"]), "max_in_degree": int(deg.max())}
    assert (deg >= 1).all() and all(np.all(np.diff(got["in_src"][a:b].astype(int)) > 0)
                                    for a, b in zip(got["in_ptr"][:-1], got["in_ptr"][1:]))
    lp = ref.log_softmax(np.random.RandomState(720).randn(9, 6) * 2.0)
    a, b = ref.recurse(lp, got), ref.recurse(lp, want)
    assert a == b and a[2] is not None


def test_pruning_keeps_the_relative_order(ctc):
    arcs, finals, nq = dfa_with_dead_ends()
    assert ctc.Pattern(arcs, finals, nq, 6).info()["dfa_states"] == 3           # states 0, 1, 5 survive
    assert ref.prune(arcs, finals, nq) == ([(0, 1, 1), (0, 2, 1), (1, 1, 1), (1, 2, 1), (1, 3, 2)], [1, 2], 3)


def test_builder_errors(ctc, pkg):
    lib = pkg.load_library()

    def message(arcs, finals, nq, C):
        with pytest.raises(Exception) as e:
            ctc.Pattern(arcs, finals, nq, C)
        return str(e.value)

    ok = [(0, 1, 1)]
    msgs = [message(ok + [(0, 1, 0)], [1], 2, 6), message([(0, 0, 1)], [1], 2, 6), message([(0, 6, 1)], [1], 2, 6),
            message([(0, 1, 2)], [1], 2, 6), message(ok, [], 2, 6), message(ok, [1], 0, 6),
            message([(i, 1 + i % 5, i + 1) for i in range(8200)], [8200], 8201, 6),
            message([(0, c, 1) for c in range(1, 601)] + [(1, c, 2) for c in range(1, 601)], [2], 3, 700)]
    for m, word in zip(msgs, ("deterministic", "label 0", "label 6", "outside [0,1]", "empty", "num_states >= 1",
                              "HCTR_PAT_MAX_STATES is 8192", "262144 edges")):
        assert word in m, (word, m)
    assert len(set(msgs)) == len(msgs)
    assert "16401 CTC states" in msgs[6]
    assert lib is not None
    # within the limits: one full-vocabulary wildcard
    i = ctc.Pattern([(0, c, 1) for c in range(1, 7358)], [1], 2, 7359).info()
    assert (i["states"], i["edges"], i["max_in_degree"]) == (7359, 22073, 7358)
