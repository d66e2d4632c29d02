"""CPU tests of word-sequence recognition's surface: the float64 yardstick tests/words_ref.py against a brute force
over all paths and all segmentations, the word tables the library exports (``hctr_lex_word_tables``, host only) against
the yardstick's, a float32 recursion over the exported tables against the yardstick, and the argument errors that need no
GPU. The device results are checked by tests/test_gpu_words.py."""
import ctypes
import importlib

import numpy as np
import pytest

import words_ref as ref

RTOL, ATOL = 1e-5, 1e-3                      # float32 recursion vs float64 on the same logits (the loss tests' rule)
NINF = -np.inf

# (name, C, entries, priors, bonus, masked classes)
TINY = [
    ("prefixes", 3, [[1], [1, 2], [1, 2, 2]], None, 0.0, ()),
    ("prefixes, priors, penalty", 3, [[1], [1, 2], [1, 2, 2]], [-0.3, -1.0, 0.4], -0.7, ()),
    ("same label across the boundary", 3, [[1], [1, 2], [2, 1]], None, 0.0, ()),
    ("same label across the boundary, bonus", 3, [[1], [1, 2], [2, 1]], [0.0, -0.5, -0.2], 1.5, ()),
    ("ambiguous segmentations", 4, [[1, 2], [3], [1], [2, 3]], None, 0.0, ()),
    ("ambiguous, priors decide", 4, [[1, 2], [3], [1], [2, 3]], [-0.1, -0.2, -1.0, -2.0], 0.25, ()),
    ("duplicates with different priors", 4, [[1, 2], [3], [1, 2], [3], [3, 3]], [-2.0, -0.5, -1.0, -0.25, -3.0], 0.0, ()),
    ("a masked class", 4, [[1, 2], [3], [1], [2, 3]], None, 0.0, (2,)),
    ("masked blank", 3, [[1], [2, 2], [1, 2]], None, -0.1, (0,)),
    ("too short for any word", 3, [[1, 1, 2], [2, 2, 1, 1]], None, 0.0, ()),
    ("one doubled word", 3, [[1, 1]], None, 0.3, ()),
]


def _logits(rng, T, C, masked):
    z = rng.randn(T, C) * 2.0
    z[:, list(masked)] = NINF
    return z


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("case", TINY, ids=[c[0] for c in TINY])
def test_reference_equals_brute_force(case, T):
    name, C, entries, priors, bonus, masked = case
    rng = np.random.RandomState(1000 + 7 * T + len(name))
    for _ in range(3):
        z = _logits(rng, T, C, masked)
        lp = ref.log_softmax(z)
        tab = ref.word_tables(entries, priors, bonus)
        score, words, starts, _ = ref.decode(ref.emissions(z, tab["classes"]), tab)
        want = ref.brute_force(lp, entries, priors, bonus)
        if want == NINF:
            assert score == NINF and words == [] and starts == []
            continue
        assert abs(score - want) <= 1e-9 * max(1.0, abs(want)), (name, T, score, want)
        assert len(words) >= 1 and starts == sorted(set(starts)) and 0 <= starts[0] and starts[-1] < T
        wt = [float(tab["weight"][ref.build_trie(entries)[2][w]]) for w in words]
        seg = ref.segmentation_score(lp, [entries[w] for w in words], wt, starts, T)
        assert abs(seg - want) <= 1e-9 * max(1.0, abs(want)), (name, T, seg, want)


def test_tiny_cases_cover_the_edges():
    rng = np.random.RandomState(5)
    short = [c for c in TINY if c[0] == "too short for any word"][0]
    for T in (1, 2, 3):
        assert ref.brute_force(ref.log_softmax(_logits(rng, T, 3, ())), short[2]) == NINF
    assert ref.brute_force(ref.log_softmax(_logits(rng, 4, 3, ())), short[2]) > NINF
    # the boundary rule matters: with the blank masked, "1" + "1" needs a blank that cannot be emitted
    z = _logits(rng, 2, 3, (0, 2))
    assert ref.words(z[:, None, :], [[1]])[0][1] == [0]           # one word over both columns, not two
    # a wrong boundary or a wrong word can only lose
    z = _logits(rng, 6, 4, ())
    lp = ref.log_softmax(z)
    es = [[1, 2], [3], [1], [2, 3]]
    score, words, starts = ref.words(z[:, None, :], es)[0]
    for alt in ([0, 1], [2, 3], [2, 0], [1]):
        for st in itertools_starts(len(alt), 6):
            assert ref.segmentation_score(lp, [es[w] for w in alt], [0.0] * len(alt), st, 6) <= score + 1e-12


def itertools_starts(n, T):
    import itertools
    return [list(s) for s in itertools.combinations(range(T), n)]


@pytest.fixture(scope="module")
def ctc(pkg):
    return importlib.import_module(pkg.__name__ + ".ctc")


def random_entries(rng, C, n, lo=1, hi=4):
    return [[int(v) for v in rng.randint(1, C, size=rng.randint(lo, hi + 1))] for _ in range(n)]


def test_exported_tables_equal_the_python_builder(ctc):
    rng = np.random.RandomState(61)
    es = random_entries(rng, 60, 400) + [[7], [7, 7], [7, 7, 7], [7], [5, 6], [5, 6]]
    pr = rng.randn(len(es)).astype(np.float32)
    pr[-1] = pr[-2]                                              # an exact tie: the lower index wins
    for priors, bonus in ((None, 0.0), (pr, 0.0), (pr, -1.25), (None, 0.3)):
        lex = ctc.Lexicon(es, num_classes=60, priors=priors)
        got, want = ctc.lex_word_tables(lex, bonus), ref.word_tables(es, priors, bonus)
        assert lex.info()["nodes"] == len(want["node"])
        for k in ("node", "slot", "entry", "classes"):
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        assert got["weight"].tobytes() == want["weight"].tobytes()
        assert got["entry"][ref.build_trie(es)[2][-1]] == len(es) - 2
        t = lex.tables()
        np.testing.assert_array_equal(got["node"][1:] & ref.PARENT_MASK, t["parent"][1:])
        np.testing.assert_array_equal(got["classes"][got["slot"]], t["label"])


def test_float32_recursion_over_the_exported_tables(ctc):
    rng = np.random.RandomState(62)
    C, W = 60, 90
    es = random_entries(rng, C, 300)
    pr = (rng.randn(len(es)) * 0.5).astype(np.float32)
    lex = ctc.Lexicon(es, num_classes=C, priors=pr)
    tab = ctc.lex_word_tables(lex, -0.5)
    z = (rng.randn(W, C) * 3.0).astype(np.float32)
    want, ww, ws, _ = ref.decode(ref.emissions(z, tab["classes"]), ref.word_tables(es, pr, -0.5))
    got, gw, gs, _ = ref.decode(ref.emissions(z, tab["classes"], np.float32), tab, np.float32)
    print("float32 %.6f float64 %.6f |d| %.2e rule %.2e" % (got, want, abs(got - want), RTOL * abs(want) + ATOL))
    assert np.isfinite(want) and abs(got - want) <= RTOL * abs(want) + ATOL
    lp = ref.log_softmax(z)
    seg = ref.segmentation_score(lp, [es[w] for w in gw], [float(tab["weight"][lex.tables()["entry_node"][w]]) for w in gw],
                                 gs, W)
    assert seg <= want + 1e-9 and abs(seg - want) <= RTOL * abs(want) + ATOL


def test_argument_errors_without_a_gpu(pkg, ctc):
    lib = pkg.load_library()
    lex = ctc.Lexicon([[1, 2], [3]], num_classes=6)
    for bad in (np.inf, -np.inf, np.nan):
        with pytest.raises(Exception) as e:
            ctc.lex_word_tables(lex, bad)
        assert "word_bonus" in str(e.value)
    assert lib.hctr_lex_word_tables(None, 0.0, None, None, None, None, None, None, None) == -1
    with pytest.raises(ValueError):
        ctc.lex_word_tables("no lexicon")
    with pytest.raises(ValueError):
        ctc._words_outputs(lex, 2, 10, 0)
    with pytest.raises(ValueError):
        ctc._words_outputs(lex, 2, 10, 11)
    assert ctc._words_outputs(lex, 2, 10, None)[0] == 10


def test_trie_over_the_node_limit_is_refused(pkg, ctc):
    rng = np.random.RandomState(63)
    es = random_entries(rng, 300, 40000, lo=3, hi=3)
    lex = ctc.Lexicon(es, num_classes=300)
    nodes = lex.info()["nodes"]
    assert nodes > ref.MAX_NODES
    with pytest.raises(Exception) as e:
        ctc.lex_word_tables(lex, 0.0)
    assert str(nodes) in str(e.value) and str(ref.MAX_NODES) in str(e.value)
    ok = ctc.Lexicon(es[:20000], num_classes=300)
    assert ref.LDS_NODES < ok.info()["nodes"] <= ref.MAX_NODES and len(ctc.lex_word_tables(ok)["node"]) == ok.info()["nodes"]


def test_result_object(pkg, synth, ctc):
    codec = pkg.ctc_codec(synth.characters())
    chars = codec.labels_to_text([np.array([5, 6]), np.array([9])])
    lex = ctc.Lexicon(chars, codec=codec)
    res = ctc.WordsResult(np.array([-1.0, NINF], np.float32), np.array([3, 0], np.int32),
                          np.array([[1, 0], [-1, -1]], np.int32), np.array([[2, 5], [-1, -1]], np.int32),
                          np.array([[9, 5, 6, 9, 0, 0, 0, 0, 0, 0], [0] * 10], np.int32), np.array([4, 0], np.int32),
                          np.array([np.log(4.0), np.inf], np.float32), np.array([9, 10], np.int32))
    assert list(res.lines(lex)) == [[(1, chars[1], 2, 5), (0, chars[0], 5, None)], []]
    np.testing.assert_allclose(res.posterior(), [0.25, 0.0], rtol=1e-6)
    assert res.texts(codec) == [chars[1] + chars[0] + chars[1], ""]
