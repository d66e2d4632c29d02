"""CPU tests of lexicon recognition's surface (hctr_lex_*): the float64 yardstick tests/lexicon_ref.py against
enumeration of all paths and against torch's float64 ctc_loss, the trie and the unit tables the library exports
(``hctr_lex_tables``, host only) against the yardstick's, the partition's invariants, the recursion driven with the
exported unit tables, and the builder's errors. The device results are checked by tests/test_gpu_lexicon.py."""
import ctypes

import numpy as np
import pytest
import torch

import lexicon_ref as ref

TINY = [
    # (C, T, entries): doubled characters, entries that are prefixes of each other, one that cannot fit
    (3, 5, [[1], [1, 1], [1, 1, 1], [1, 2], [2, 1], [1, 2, 1], [2]]),
    (3, 6, [[1, 1], [1, 1, 2], [2, 2, 1], [1, 2, 2], [2], [2, 1, 2, 1], [1, 1, 1, 1]]),
    (4, 4, [[3], [3, 3], [1, 2, 3], [1, 2], [3, 2, 1], [2, 2, 2], [1, 3]]),
    (4, 1, [[1], [2], [1, 1], [3, 1]]),
    (2, 6, [[1], [1, 1], [1, 1, 1], [1, 1, 1, 1]]),
    (4, 5, [[1, 2, 3, 1], [1, 2, 3], [1, 2], [1], [2, 3, 3], [2, 3], [1, 2, 3, 1]]),
]


@pytest.mark.parametrize("i,case", list(enumerate(TINY)))
def test_reference_equals_enumeration(i, case):
    C, T, entries = case
    z = np.random.RandomState(300 + i).randn(T, 1, C) * 2.0
    got = ref.scores(z, entries)[0]
    want = ref.enumerate_scores(ref.log_softmax(z[:, 0]), entries)
    unfit = np.array([not ref.fits(e, T) for e in entries])
    np.testing.assert_array_equal(np.isneginf(got), unfit)
    np.testing.assert_array_equal(np.isneginf(want), unfit)
    np.testing.assert_allclose(got[~unfit], want[~unfit], rtol=1e-12, atol=1e-12)


def test_tiny_cases_cover_the_edges():
    assert any(not ref.fits(e, T) for _, T, es in TINY for e in es)
    assert any(a == b for _, _, es in TINY for e in es for a, b in zip(e, e[1:]))
    assert any(e1 != e2 and e1 == e2[:len(e1)] for _, _, es in TINY for e1 in es for e2 in es)


def make_entries(rng, C, n, lo=1, hi=9):
    return [[int(v) for v in rng.randint(1, C, size=rng.randint(lo, hi + 1))] for _ in range(n)]


def lexicon_300(C=60):
    """about 300 entries: random ones, prefixes and extensions, doubled characters, a 64-label entry, duplicates, one
    first label with more than 128 nodes under it and under one of its children"""
    rng = np.random.RandomState(41)
    es = make_entries(rng, C, 140)
    es += [e[:k] for e in es[:30] for k in (1, 2) if k < len(e)]
    es += [e + [int(rng.randint(1, C))] for e in es[:30]]
    es += [[7], [7, 7], [7, 7, 7], [int(v) for v in rng.randint(1, C, size=64)], es[3], es[50]]
    es += [[11, 12] + [int(v) for v in rng.randint(1, C, size=rng.randint(1, 7))] for _ in range(70)]
    return es


def test_reference_equals_torch_ctc_loss():
    C, W = 60, 160
    rng = np.random.RandomState(42)
    es = lexicon_300(C)
    assert 280 <= len(es) <= 340
    z = rng.randn(W, 2, C) * 2.0
    il = np.array([W, 40], np.int32)
    got = ref.scores(z, es, il)
    lp = torch.from_numpy(ref.log_softmax(z))
    for b in range(2):
        T = int(il[b])
        tl = torch.tensor([len(e) for e in es])
        tg = torch.tensor([c for e in es for c in e])
        nll = torch.nn.functional.ctc_loss(lp[:T, b:b + 1].expand(T, len(es), C).contiguous(), tg,
                                           torch.full((len(es),), T, dtype=torch.long), tl, blank=0,
                                           reduction="none").numpy()
        unfit = np.array([not ref.fits(e, T) for e in es])
        np.testing.assert_array_equal(np.isneginf(got[b]), unfit)
        np.testing.assert_array_equal(np.isposinf(nll), unfit)
        np.testing.assert_allclose(got[b][~unfit], -nll[~unfit], rtol=1e-12, atol=1e-10)
    assert np.isneginf(got[1]).any() and np.isfinite(got[0]).all()


@pytest.fixture(scope="module")
def ctc(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".ctc")


@pytest.fixture(scope="module", params=[128, 0])
def built(request, ctc):
    es = lexicon_300()
    lex = ctc.Lexicon(es, num_classes=60, unit_nodes=request.param)
    return es, lex, lex.tables(), (request.param or ref.DEFAULT_UNIT)


def test_global_trie_equals_python_trie(built):
    es, lex, t, _ = built
    parent, label, entry_node = ref.build_trie(es)
    info = lex.info()
    assert info["nodes"] == len(parent) and info["entries"] == len(es) == len(lex)
    assert info["max_len"] == 64 and info["classes"] == len({c for e in es for c in e})
    np.testing.assert_array_equal(t["parent"], parent)
    np.testing.assert_array_equal(t["label"], label)
    np.testing.assert_array_equal(t["entry_node"], entry_node)
    dup = [k for k, e in enumerate(es) if es.index(e) != k]
    assert dup and all(t["entry_node"][k] == t["entry_node"][es.index(es[k])] for k in dup)


def test_partition_invariants(built):
    es, lex, t, cap = built
    parent, label, _ = ref.build_trie(es)
    uo, units = t["unit_off"], lex.info()["units"]
    assert units == len(uo) - 1 and (units > 1) == (cap == 128)
    owners = np.zeros(len(parent), np.int64)
    for u in range(units):
        nodes = t["unit_node"][uo[u]:uo[u + 1]]
        word = t["unit_word"][uo[u]:uo[u + 1]]
        owned = t["unit_owned"][uo[u]:uo[u + 1]]
        assert 2 <= len(nodes) <= cap and nodes[0] == 0 and owned[0] == 0
        assert len(set(nodes.tolist())) == len(nodes)
        lp = word & ref.PARENT_MASK
        for i in range(1, len(nodes)):
            assert lp[i] < i                                   # parents before children
            assert nodes[lp[i]] == parent[nodes[i]]            # closed under parent, through copies
            assert bool(word[i] & ref.FIRST) == (parent[nodes[i]] == 0)
            assert bool(word[i] & ref.SKIP) == (parent[nodes[i]] != 0 and label[parent[nodes[i]]] != label[nodes[i]])
        np.add.at(owners, nodes[owned == 1], 1)
        cls = t["unit_class"][t["class_off"][u]:t["class_off"][u + 1]]
        assert cls[0] == 0 and (np.diff(cls) > 0).all()
        np.testing.assert_array_equal(cls[t["unit_kidx"][uo[u]:uo[u + 1]]], label[nodes])
        # a copy is an ancestor of an owned node of the unit
        anc = set()
        for g in nodes[owned == 1]:
            p = parent[g]
            while p > 0:
                anc.add(int(p))
                p = parent[p]
        assert set(nodes[owned == 0].tolist()) - {0} <= anc
    assert owners[0] == 0 and (owners[1:] == 1).all()          # every non-root node is owned exactly once
    # the entries that end on each owned local node
    ep, el = t["entry_ptr"], t["entry_list"]
    assert ep[0] == 0 and ep[-1] == len(es) and sorted(el.tolist()) == list(range(len(es)))
    for i in np.nonzero(np.diff(ep))[0]:
        assert t["unit_owned"][i] == 1
        ends = el[ep[i]:ep[i + 1]]
        assert (np.diff(ends) > 0).all() and (t["entry_node"][ends] == t["unit_node"][i]).all()


def test_partition_equals_python_partition(built):
    es, lex, t, cap = built
    parent, label, _ = ref.build_trie(es)
    want = ref.partition(parent, label, cap)
    uo = t["unit_off"]
    assert len(want) == len(uo) - 1
    for u, (nodes, owned) in enumerate(want):
        np.testing.assert_array_equal(t["unit_node"][uo[u]:uo[u + 1]], nodes)
        np.testing.assert_array_equal(t["unit_owned"][uo[u]:uo[u + 1]], owned)


def test_split_of_large_subtrees():
    """unit_nodes = 128 with more than 128 nodes under one first label and under one depth-2 node: both are split"""
    es = lexicon_300()
    parent, label, _ = ref.build_trie(es)
    size = np.ones(len(parent), np.int64)
    for v in range(len(parent) - 1, 0, -1):
        size[parent[v]] += size[v]
    big = [v for v in range(1, len(parent)) if size[v] > 128]
    assert any(parent[v] == 0 for v in big) and any(parent[v] != 0 and parent[parent[v]] == 0 for v in big)


def test_recursion_over_the_exported_units_reproduces_the_reference(built):
    es, lex, t, _ = built
    rng = np.random.RandomState(43)
    W, C = 90, 60
    z = rng.randn(W, 1, C) * 2.0
    want = ref.scores(z, es)[0]
    lp = ref.log_softmax(z[:, 0])
    got = np.full(len(es), np.nan)
    uo, ep, el = t["unit_off"], t["entry_ptr"], t["entry_list"]
    for u in range(len(uo) - 1):
        sl = slice(uo[u], uo[u + 1])
        cls = t["unit_class"][t["class_off"][u]:t["class_off"][u + 1]]
        local_parent = (t["unit_word"][sl] & ref.PARENT_MASK).astype(np.int64)
        a_n, a_b = ref.forward(lp, local_parent, cls[t["unit_kidx"][sl]].astype(np.int64))
        sc = np.logaddexp(a_b, a_n)
        for i in range(uo[u], uo[u + 1]):
            got[el[ep[i]:ep[i + 1]]] = sc[i - uo[u]]
    np.testing.assert_array_equal(got, want)                   # the same float64 operations: exactly equal


def test_ranking_reference():
    sc = np.array([-3.0, -1.0, -np.inf, -1.0, -2.0])
    top, tr, tot, cnt = ref.rank(sc, None, 4)
    assert top.tolist() == [1, 3, 4, 0] and cnt == 4 and abs(tot - np.log(np.exp(sc).sum())) < 1e-12
    top, tr, tot, cnt = ref.rank(sc, np.array([0.0, -5.0, 0.0, 0.0, 1.0]), 5)
    assert top.tolist() == [3, 4, 0, 1, -1] and cnt == 4 and tr[4] == -np.inf
    assert ref.rank(np.full(3, -np.inf), None, 2)[2:] == (-np.inf, 0)


def test_builder_errors(pkg, ctc):
    lib = pkg.load_library()
    vp = ctypes.c_void_p

    def build(entries, lengths, N, C, prior=None, unit_nodes=0):
        e, ln = np.array(entries, np.int32), np.array(lengths, np.int32)
        pr = None if prior is None else np.array(prior, np.float32)
        h = vp()
        rc = lib.hctr_lex_build(e.ctypes.data_as(vp), ln.ctypes.data_as(vp), N, C,
                                None if pr is None else pr.ctypes.data_as(vp), unit_nodes, ctypes.byref(h))
        if rc == 0:
            lib.hctr_lex_free(h)
        else:
            assert not h.value
        return rc, lib.hctr_last_error(None)

    assert build([1, 2, 3], [2, 1], 2, 6)[0] == 0
    rc, msg = build([1, 6], [2], 1, 6)
    assert rc == -1 and b"outside [1,5]" in msg
    assert build([0], [1], 1, 6)[0] == -1
    rc, msg = build([1] * 65, [65], 1, 6)
    assert rc == -1 and b"outside [1,64]" in msg
    assert build([1], [0], 1, 6)[0] == -1
    rc, msg = build([1], [1], 0, 6)
    assert rc == -1 and b"N" in msg
    for bad in (np.inf, -np.inf, np.nan):
        rc, msg = build([1, 2], [1, 1], 2, 6, prior=[0.0, bad])
        assert rc == -1 and b"log_prior[1]" in msg
    assert build([1], [1], 1, 6, unit_nodes=127)[0] == -1
    assert build([1], [1], 1, 6, unit_nodes=128)[0] == 0
    assert build([1] * 64, [64], 1, 6, unit_nodes=128)[0] == 0
    for exc_args in (dict(entries=[[1, 9]], num_classes=6), dict(entries=[[]], num_classes=6),
                     dict(entries=[], num_classes=6), dict(entries=[[1]], num_classes=6, priors=[0.0, 1.0]),
                     dict(entries=[[1]], num_classes=6, priors=[np.nan]), dict(entries=[[1]], num_classes=6, unit_nodes=5)):
        with pytest.raises(ValueError):
            ctc.Lexicon(**exc_args)


def test_strings_through_a_codec(pkg, synth, ctc):
    codec = pkg.ctc_codec(synth.characters())
    chars = codec.labels_to_text([np.array([5, 6, 7]), np.array([5, 6]), np.array([9])])
    lex = ctc.Lexicon(chars, codec=codec, priors=[0.0, -1.0, -2.0])
    assert [e.tolist() for e in lex.labels] == [[5, 6, 7], [5, 6], [9]] and lex.entry(1) == chars[1]
    assert lex.info() == {"entries": 3, "nodes": 5, "units": 1, "classes": 4, "max_len": 3}
    with pytest.raises(ValueError):
        ctc.Lexicon([chars[0], "\x00\x01"], codec=codec)
    res = ctc.LexiconResult(lex, np.array([[1, 0, -1]], np.int32), np.array([[-1.0, -2.0, -np.inf]], np.float32),
                            np.array([[-2.0, -2.0, -np.inf]]), np.array([-2.0 + np.log(2.0)]), np.array([2], np.int32))
    np.testing.assert_allclose(res.posteriors(), [[0.5, 0.5, 0.0]])
    assert res.best() == [chars[1]] and [r[0] for r in next(res.lines())] == [1, 0]
