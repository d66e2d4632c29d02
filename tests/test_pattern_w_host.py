"""CPU tests of weighted patterns' host side (hctr_pat_build_weighted, hctr_pat_weights, hctr_pat_text_weight,
``Pattern(weights=)``, ``Pattern.compile(label_weights=)``, ``Pattern.bigram``): the float64 yardstick
tests/pattern_w_ref.py against enumeration of all paths with weights and against the family's other yardsticks, the
tables and weights the library exports against the yardstick's, text weights, the bigram's sizes and the builder's
errors. The device results are checked by tests/test_gpu_pattern_w.py."""
import importlib
import itertools

import numpy as np
import pytest
import torch

import lexicon_ref
import pattern_ref
import pattern_w_ref as ref

ALPHABET = "ab12"


@pytest.fixture(scope="module")
def ctc(pkg):
    return importlib.import_module(pkg.__name__ + ".ctc")


@pytest.fixture(scope="module")
def codec(pkg):
    return pkg.ctc_codec(ALPHABET)


def same_tables(a, b):
    keys = ("state_label", "state_slot", "in_ptr", "in_src", "classes", "accept", "start")
    return all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in keys)


def same_weights(a, b):
    return all(a[k].dtype == np.float32 and b[k].dtype == np.float32 and a[k].tobytes() == b[k].tobytes()
               for k in ("in_w", "accept_w", "start_w"))


def rand_w(seed, n, scale=3.0):
    return (np.random.RandomState(seed).randn(n) * scale).astype(np.float32)


# ---- the yardstick against enumeration of all C^T paths ----
def tiny():
    """(arcs, finals, num_states, weights, final_weights)"""
    out = []
    # (a|b)+c?: eps_(1,1) and eps_(1,2) are each fed by arcs from states 0 and 1 with different weights
    arcs = [(0, 1, 1), (0, 2, 1), (1, 1, 1), (1, 2, 1), (1, 3, 2)]
    out.append((arcs, [1, 2], 3, rand_w(1, 5), rand_w(2, 2)))
    # a literal with a doubled label
    a, f, n = pattern_ref.literal([1, 1, 2])
    out.append((a, f, n, rand_w(3, 3), rand_w(4, 1)))
    # a chain of three of {1, 2}
    arcs = [(i, c, i + 1) for i in range(3) for c in (1, 2)]
    out.append((arcs, [3], 4, rand_w(5, 6), None))
    # (12)*: the start state is final, and a cycle
    out.append(([(0, 1, 1), (1, 2, 0)], [0], 2, rand_w(6, 2), rand_w(7, 1)))
    # a|ab|abc with priors as final weights, no arc weights
    a, f, n = pattern_ref.trie([[1], [1, 2], [1, 2, 3]])
    out.append((a, f, n, None, np.log(np.array([0.2, 0.5, 0.3])).astype(np.float32)))
    # two DFA states p = 0 and p = 2 reach state 1 on label 1 with weights +4 and -4: one shared eps_(1,1)
    arcs = [(0, 1, 1), (0, 2, 2), (2, 1, 1), (1, 3, 1), (2, 3, 2)]
    out.append((arcs, [1], 3, np.array([4, 0.5, -4, 1, -1], np.float32), np.array([0.25], np.float32)))
    return out


TINY = tiny()


@pytest.mark.parametrize("i", range(len(TINY)))
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
def test_reference_equals_enumeration(i, T):
    arcs, finals, nq, w, fw = TINY[i]
    lp = ref.log_softmax(np.random.RandomState(900 + 10 * i + T).randn(T, 4) * 2.0)
    t = ref.tables(arcs, finals, nq, w, fw)
    logp, best, path = ref.recurse(lp, t)
    want_logp, want_best, want_paths = ref.enumerate_paths(lp, t)
    if want_best == -np.inf:
        assert logp == -np.inf and best == -np.inf and path is None
        return
    assert abs(logp - want_logp) <= 1e-12 and abs(best - want_best) <= 1e-12
    assert path in want_paths
    assert best <= logp + 1e-12


def test_tiny_cases_cover_what_they_should():
    assert len(TINY) >= 5
    lp = ref.log_softmax(np.zeros((2, 4)))
    assert ref.recurse(lp, ref.tables(*TINY[1]))[0] == -np.inf and ref.recurse(lp, ref.tables(*TINY[2]))[0] == -np.inf
    assert 0 in TINY[3][1] and ref.recurse(lp[:1], ref.tables(*TINY[3]))[0] > -np.inf      # start-final, and a cycle
    t = ref.tables(*TINY[5])                                   # a shared eps state fed by arcs of different weights
    s = int(np.flatnonzero(t["state_label"] == 1)[0])
    w = t["in_w"][t["in_ptr"][s]:t["in_ptr"][s + 1]]
    assert 4.0 in w and -4.0 in w and 0.0 in w
    assert ref.recurse(ref.log_softmax(np.zeros((3, 4))), t)[0] > 0          # logp is no probability


# ---- the exported tables and weights ----
def dfa_with_dead_ends():
    """(a|b)+c? over C = 6 with an unreachable state 3, a dead end 4 (reachable, cannot finish) and arcs among them"""
    return ([(0, 1, 1), (0, 2, 1), (1, 1, 1), (1, 2, 1), (1, 3, 5), (3, 1, 1), (3, 2, 3), (0, 4, 4), (4, 4, 4), (1, 5, 4)],
            [1, 5, 4], 6)


def export_cases():
    out = [TINY[i][:3] for i in (0, 3, 5)]
    out += [dfa_with_dead_ends(), pattern_ref.trie([[1, 2, 3], [1, 2], [4, 4, 1], [2]]), pattern_ref.contains([1, 2, 1], 6),
            ([(0, c, 0) for c in range(1, 6)], [0], 1)]
    return out


@pytest.mark.parametrize("i", range(len(export_cases())))
def test_exported_tables_and_weights_equal_the_reference_builder(i, ctc):
    arcs, finals, nq = export_cases()[i]
    w, fw = rand_w(40 + i, len(arcs)), rand_w(60 + i, len(finals))
    pat = ctc.Pattern(arcs, finals, nq, 6, weights=w, final_weights=fw)
    plain = ctc.Pattern(arcs, finals, nq, 6)
    assert (pat.kind, plain.kind) == (2, 0) and pat.weighted and not plain.weighted
    assert same_tables(pat.tables(), plain.tables()) and pat.info() == plain.info()
    want = ref.tables(arcs, finals, nq, w, fw)
    got = dict(pat.tables(), **pat.weights())
    assert same_tables(want, got) and same_weights(want, got)
    assert len(got["in_w"]) == len(got["in_src"]) and len(got["accept_w"]) == len(got["accept"])
    # self edges and the in-edges of beta states weigh nothing
    for s in range(len(got["state_label"])):
        for j in range(got["in_ptr"][s], got["in_ptr"][s + 1]):
            if got["in_src"][j] == s or got["state_label"][s] == 0:
                assert got["in_w"][j] == 0
    lp = ref.log_softmax(np.random.RandomState(920 + i).randn(9, 6) * 2.0)
    got["arc_w"], got["final_w"] = want["arc_w"], want["final_w"]
    a, b = ref.recurse(lp, got), ref.recurse(lp, want)
    assert a == b and a[2] is not None
    # the object's own walk over its pruned arcs
    rng = np.random.RandomState(940 + i)
    for _ in range(200):
        text = rng.randint(1, 6, size=rng.randint(0, 6)).tolist()
        assert pat.text_weight(text) == ref.text_weight(want, text)
    assert pat.text_weight(a[2] and ref.collapse(a[2])) > -np.inf


def test_null_weights_mean_zeros_and_one_side_may_be_given(ctc):
    arcs, finals, nq = TINY[0][:3]
    w = rand_w(70, len(arcs))
    only_arcs = ctc.Pattern(arcs, finals, nq, 6, weights=w)
    assert only_arcs.kind == 2 and not only_arcs.weights()["accept_w"].any() and only_arcs.weights()["in_w"].any()
    only_fin = ctc.Pattern(arcs, finals, nq, 6, final_weights=[1.5, -2.5])
    assert only_fin.kind == 2 and not only_fin.weights()["in_w"].any() and not only_fin.weights()["start_w"].any()
    assert sorted(set(only_fin.weights()["accept_w"].tolist())) == [-2.5, 1.5]
    # a final state listed twice with one weight is no conflict
    ctc.Pattern(arcs, [1, 2, 1], nq, 6, final_weights=[0.5, 1.0, 0.5])


# ---- equalities on the yardstick ----
def test_zero_weights_give_the_unweighted_yardstick():
    rng = np.random.RandomState(950)
    for arcs, finals, nq, _, _ in TINY:
        lp = ref.log_softmax(rng.randn(7, 4) * 2.0)
        a, b = ref.recurse(lp, ref.tables(arcs, finals, nq)), pattern_ref.recurse(lp, pattern_ref.tables(arcs, finals, nq))
        assert abs(a[0] - b[0]) <= 1e-12 and abs(a[1] - b[1]) <= 1e-12 and a[2] == b[2]


def test_literal_with_constant_arc_weight_is_the_loss_plus_n_beta():
    rng = np.random.RandomState(951)
    C, T, beta = 9, 40, np.float32(0.7)
    lp = ref.log_softmax(rng.randn(T, C) * 2.0)
    for text in ([3], [1, 1, 2, 2, 2, 5], list(rng.randint(1, C, size=20))):
        arcs, finals, nq = pattern_ref.literal(text)
        logp = ref.recurse(lp, ref.tables(arcs, finals, nq, np.full(len(arcs), beta)))[0]
        nll = torch.nn.functional.ctc_loss(torch.from_numpy(lp)[:, None, :], torch.tensor([text]), torch.tensor([T]),
                                           torch.tensor([len(text)]), blank=0, reduction="none").item()
        assert abs(logp - (-nll + len(text) * float(beta))) <= 1e-12


def test_union_of_literals_with_priors_equals_the_lexicon_yardstick():
    rng = np.random.RandomState(952)
    C, T = 7, 30
    es = sorted(set(tuple(int(v) for v in rng.randint(1, C, size=rng.randint(1, 6))) for _ in range(60)))
    prior = np.log(rng.dirichlet(np.ones(len(es)))).astype(np.float32)
    arcs, finals, nq = pattern_ref.trie(es)
    node = {}                                                  # entry -> its final state in the trie
    d = {(p, c): q for p, c, q in arcs}
    for e in es:
        v = 0
        for c in e:
            v = d[(v, c)]
        node[e] = v
    fw = np.array([prior[[node[e] for e in es].index(f)] for f in finals], np.float32)
    t = ref.tables(arcs, finals, nq, None, fw)
    # planted: the line reads one entry clearly, so the best path's entry is the top-ranked one
    z = rng.randn(T, 1, C) * 0.5
    target = es[17]
    for k, c in enumerate(target):
        z[2 + 4 * k:4 + 4 * k, 0, c] += 9.0
    blank = np.ones(T, bool)
    for k in range(len(target)):
        blank[2 + 4 * k:4 + 4 * k] = False
    z[blank, 0, 0] += 9.0
    sc = lexicon_ref.scores(z, es)[0]
    top, _, total, _ = lexicon_ref.rank(sc, prior, 1)
    logp, _, path = ref.run(z, t)[0]
    assert abs(logp - total) <= 1e-12
    assert tuple(ref.collapse(path)) == es[int(top[0])] == target


def test_bigram_with_zero_weights_is_the_plus_of_its_labels(ctc, codec):
    big = ctc.Pattern.bigram([1, 2, 3, 4], np.zeros((4, 4)), num_classes=6)
    rex = ctc.Pattern.compile("[ab12]+", codec)
    assert big.kind == 2 and rex.kind == 0
    rng = np.random.RandomState(953)
    lp = ref.log_softmax(rng.randn(8, 6) * 2.0)
    a = ref.recurse(lp, ref.tables(big.arcs, big.finals, big.num_states))
    b = pattern_ref.recurse(lp, pattern_ref.tables(rex.arcs, rex.finals, rex.num_states))
    assert abs(a[0] - b[0]) <= 1e-12 and abs(a[1] - b[1]) <= 1e-12 and a[2] == b[2]
    assert not any(big.weights()[k].any() for k in ("in_w", "accept_w", "start_w"))


def test_bigram_places_its_weights(ctc):
    rng = np.random.RandomState(954)
    n, labels = 3, [4, 2, 5]
    tr, ini, fin = rng.randn(n, n).astype(np.float32), rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    tr[1, 2] = -np.inf                                         # no "5 after 2"
    pat = ctc.Pattern.bigram(labels, tr, ini, fin, num_classes=7)
    assert pat.text_weight([2, 4, 5]) == float(ini[1]) + float(tr[1, 0]) + float(tr[0, 2]) + float(fin[2])
    assert pat.text_weight([4]) == float(ini[0]) + float(fin[0])
    assert pat.text_weight([2, 5]) == -np.inf and pat.text_weight([]) == -np.inf and pat.text_weight([1]) == -np.inf
    with pytest.raises(ValueError, match="distinct"):
        ctc.Pattern.bigram([1, 1], np.zeros((2, 2)), num_classes=6)
    with pytest.raises(ValueError, match=r"\[n, n\]"):
        ctc.Pattern.bigram([1, 2], np.zeros((2, 3)), num_classes=6)


# ---- Pattern.compile(label_weights=) ----
SPELLINGS = [("a+b+", "aa*bb*"), (r"\d{2}", "(1|2)[12]"), ("(a|b)*", "(a*b*)*"), ("(ab|a1)2?", "a(b|1)(2|)")]


@pytest.mark.parametrize("e1,e2", SPELLINGS)
def test_two_spellings_give_identical_tables_and_weights(e1, e2, ctc, codec):
    lw = {"a": 0.5, "b": -1.25, "1": 2.0}
    p1, p2 = ctc.Pattern.compile(e1, codec, label_weights=lw), ctc.Pattern.compile(e2, codec, label_weights=lw)
    assert p1.kind == 2 and same_tables(p1.tables(), p2.tables()) and same_weights(p1.weights(), p2.weights())
    assert same_tables(p1.tables(), ctc.Pattern.compile(e1, codec).tables())


@pytest.mark.parametrize("how", ["scalar", "dict", "array"])
def test_text_weight_is_the_sum_of_label_weights(how, ctc, codec):
    C = len(codec.characters)
    lw = {"scalar": 0.75, "dict": {"a": 0.5, "2": -1.5}, "array": rand_w(960, C)}[how]
    per = (np.full(C, 0.75, np.float32) if how == "scalar" else lw if how == "array" else
           np.array([{"a": 0.5, "2": -1.5}.get(ch, 0.0) for ch in codec.characters], np.float32))
    import re
    for expr in ("(a|b)+1?", r"[ab]\d", "(a|b)*ab(a|b)*", ".{0,3}"):
        pat = ctc.Pattern.compile(expr, codec, label_weights=lw)
        want = re.compile(expr)
        n_in = 0
        for k in range(7):
            for s in itertools.product(ALPHABET, repeat=k):
                lab = [codec.dict[ch] for ch in s]
                w = pat.text_weight(lab)
                if want.fullmatch("".join(s)):
                    n_in += 1
                    assert w == float(np.sum([np.float64(per[c]) for c in lab]) if lab else 0.0), (expr, s)
                else:
                    assert w == -np.inf, (expr, s)
        assert n_in > 0


def test_compile_with_weights_is_always_the_explicit_form(ctc, codec, pkg):
    with pytest.raises(ValueError, match="set form"):
        ctc.Pattern.compile("a+", codec, sets=True, label_weights=1.0)
    with pytest.raises(ValueError, match="not a character"):
        ctc.Pattern.compile("a+", codec, label_weights={"x": 1.0})
    with pytest.raises(ValueError, match="entries"):
        ctc.Pattern.compile("a+", codec, label_weights=[1.0, 2.0])
    big = pkg.ctc_codec("".join(chr(0x4E00 + i) for i in range(600)))
    assert ctc.Pattern.compile("..", big).kind == 1                      # unweighted: the set form takes over
    with pytest.raises(ValueError, match=r"hctr_pat_build_weighted: .*HCTR_PAT_MAX_EDGES"):
        ctc.Pattern.compile("..", big, label_weights=0.5)
    assert ctc.Pattern.compile("a+", codec, label_weights=None).kind == 0


# ---- the bigram's sizes ----
def test_bigram_sizes_and_the_edge_limit(ctc):
    for n in (10, 100, 361):
        i = ctc.Pattern.bigram(np.arange(1, n + 1), np.zeros((n, n)), num_classes=n + 2).info()
        assert (i["states"], i["edges"]) == (2 * n + 1, 2 * n * n + 3 * n + 1)
        assert i["edges"] <= pattern_ref.MAX_EDGES
    assert 2 * 10 * 10 + 31 == 231 and 2 * 100 * 100 + 301 == 20301
    with pytest.raises(ValueError, match=r"hctr_pat_build_weighted: .*262144 edges"):
        ctc.Pattern.bigram(np.arange(1, 363), np.zeros((362, 362)), num_classes=400)


# ---- errors ----
def test_builder_errors(ctc):
    def message(arcs, finals, nq, C, w=None, fw=None):
        with pytest.raises(ValueError) as e:
            ctc.Pattern(arcs, finals, nq, C, weights=[0.0] * len(arcs) if w is None else w,
                        final_weights=[0.0] * len(finals) if fw is None else fw)
        assert ": hctr_pat_build_weighted: " in str(e.value) and "hctr_pat_build:" not in str(e.value), str(e.value)
        return str(e.value)

    ok = [(0, 1, 1)]
    msgs = [message(ok, [1], 2, 6, w=[np.nan]), message(ok, [1], 2, 6, w=[np.inf]), message(ok, [1], 2, 6, w=[-np.inf]),
            message(ok, [1], 2, 6, fw=[np.nan]), message(ok, [1], 2, 6, fw=[np.inf]), message(ok, [1], 2, 6, fw=[-np.inf]),
            message(ok, [1, 1], 2, 6, fw=[0.5, 0.25])]
    for m, word in zip(msgs, ("arcs_weight[0] is nan", "arcs_weight[0] is +inf", "arcs_weight[0] is -inf",
                              "final_weight[0] is nan", "final_weight[0] is +inf", "final_weight[0] is -inf",
                              "listed twice with different weights")):
        assert word in m, (word, m)
    # the inherited errors under the new prefix
    inherited = [message(ok + [(0, 1, 0)], [1], 2, 6), message([(0, 0, 1)], [1], 2, 6), message([(0, 6, 1)], [1], 2, 6),
                 message([(0, 1, 2)], [1], 2, 6), message(ok, [], 2, 6), message(ok, [1], 0, 6),
                 message(ok, [2], 2, 6), message(ok, [1], 2, 1),
                 message([(i, 1 + i % 5, i + 1) for i in range(8200)], [8200], 8201, 6),
                 message([(0, c, 1) for c in range(1, 601)] + [(1, c, 2) for c in range(1, 601)], [2], 3, 700)]
    for m, word in zip(inherited, ("deterministic", "label 0", "label 6", "outside [0,1]", "empty", "num_states >= 1",
                                   "finals[0]=2", "C >= 2", "HCTR_PAT_MAX_STATES is 8192", "262144 edges")):
        assert word in m, (word, m)
    assert len(set(msgs + inherited)) == len(msgs) + len(inherited)
    with pytest.raises(ValueError, match="2 weights for 1 arcs"):
        ctc.Pattern(ok, [1], 2, 6, weights=[1.0, 2.0])
    with pytest.raises(ValueError, match="final weights"):
        ctc.Pattern(ok, [1], 2, 6, final_weights=[1.0, 2.0])
    with pytest.raises(ValueError, match="set form"):
        ctc.Pattern([(0, 0, 1)], [1], 2, 6, sets=[[1, 2]], weights=[1.0])


def test_weights_and_text_weight_refuse_unweighted_patterns(ctc, codec):
    plain = ctc.Pattern([(0, 1, 1)], [1], 2, 6)
    sets = ctc.Pattern.compile("a+", codec, sets=True)
    assert (plain.kind, sets.kind) == (0, 1)
    for pat in (plain, sets):
        with pytest.raises(ValueError, match="hctr_pat_weights: the pattern has no weights"):
            pat.weights()
        with pytest.raises(ValueError, match="hctr_pat_text_weight: the pattern has no weights"):
            pat.text_weight([1])
