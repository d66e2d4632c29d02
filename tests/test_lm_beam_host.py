"""Host tests (no GPU) of the flat n-gram table behind the device LM search (C ABI hctr_lm_build / hctr_lm_word_logp,
csrc/lm_flat.h) and of its yardstick tests/lm_beam_ref.py.

  * hctr_lm_word_logp - the routine the device search runs, compiled for the host - is BIT-EQUAL to the string-keyed
    scorer of csrc/ngram_lm.cpp (hctr_ngram_word_logp, one term of hctr_ngram_score) for every word, OOV included, after
    contexts of every length 0 .. order drawn from the vocabulary plus <s> (and the OOV id), for models of order 1, 2, 3,
    5 and 6 and a model without <unk>; a model of order 7 is refused with HCTR_ERR_ARG and a message;
  * the yardstick's 1-best is hctr_beam_search(builtin_lm = 3)'s text on the same lists, and its memoised LM evaluation
    is bit-equal to re-scoring whole sentences with ArpaRef.
"""
import ctypes
import importlib

import numpy as np
import pytest

import lm_beam_ref as lr
import nbest_ref as nr
from oracle.ctc_ref import ArpaRef

ERR_ARG = -1
vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def lib(pkg):
    return pkg.load_library()


@pytest.fixture(scope="module")
def codec_mod(pkg):
    return importlib.import_module(pkg.__name__ + ".codec")


def _bits(x):
    return np.asarray(x, np.float64).tobytes()


@pytest.mark.parametrize("order,unk", [(1, True), (2, True), (3, True), (5, True), (6, True), (3, False)])
def test_flat_table_is_bit_equal_to_the_string_keyed_scorer(lib, codec_mod, tmp_path, order, unk):
    n_chars, C = 9, 14                                     # classes 10 .. 12 are out of vocabulary
    path = str(tmp_path / "m.arpa")
    total = lr.write_arpa(path, order, n_chars, seed=3, unk=unk)
    lm = codec_mod.ArpaLM(path)
    assert lm.order == order
    chars = ["<blank>"] + list(lr.chars_of(C)) + ["<unknown>"]
    words = lm.label_words(chars)
    assert (words[n_chars + 1:] == lm.word_id("<unk>")).all() and (lm.word_id("<unk>") >= 0) == unk
    flat = lm.flat(chars)
    assert flat.value == lm.flat(chars).value              # built once
    assert lib.hctr_lm_order(flat) == order
    vocab = sorted(set(int(w) for w in words if w >= 0) | {lm.word_id("<s>"), lm.word_id("</s>")})
    pool = np.array(vocab + [-1], np.int32)                # a context may hold the OOV id too
    rng = np.random.RandomState(order)
    got, want, hits = [], [], 0
    for nctx in range(0, order + 1):
        for _ in range(1 if nctx == 0 else 60):
            ctx = pool[rng.randint(0, len(pool), nctx)].astype(np.int32)
            if nctx and rng.rand() < 0.3:
                ctx[0] = lm.word_id("<s>")
            cp = ctx.ctypes.data_as(vp) if nctx else None
            for w in list(vocab) + [-1]:
                got.append(lib.hctr_lm_word_logp(flat, cp, nctx, w))
                want.append(lib.hctr_ngram_word_logp(lm._h, cp, nctx, w))
    got, want = np.array(got), np.array(want)
    assert not np.isnan(want).any()
    assert _bits(got) == _bits(want), np.flatnonzero(got != want)[:10]
    if not unk:
        assert (want == -100.0).any()                      # the OOV word of a model without <unk>
    assert len(set(np.round(want, 6))) > min(total, 50) // 2     # the walk ended at many different n-grams
    # a sentence scored term by term through the flat table is hctr_ngram_score's own sum
    sent = [lr.chars_of(C)[i] for i in (0, 3, 11, 2, 2, 7, 10, 1)]
    ids, s = [lm.word_id("<s>")], 0.0
    for ch in sent:
        a = np.array(ids, np.int32)
        w = lm.word_id(ch)
        s += lib.hctr_lm_word_logp(flat, a.ctypes.data_as(vp), len(ids), w)
        ids.append(w if w >= 0 else lm.word_id("<unk>"))
    assert _bits(s) == _bits(lm.score(" ".join(sent), bos=True, eos=False))
    assert _bits(s) == _bits(ArpaRef(path).score(" ".join(sent), eos=False))


def test_build_errors(lib, codec_mod, tmp_path):
    path = str(tmp_path / "m7.arpa")
    lr.write_arpa(path, 7, 6, seed=1)
    lm = codec_mod.ArpaLM(path)
    assert lm.order == 7
    words = np.zeros(8, np.int32)
    h = vp()
    assert lib.hctr_lm_build(lm._h, words.ctypes.data_as(vp), 8, ctypes.byref(h)) == ERR_ARG and not h.value
    assert b"6" in lib.hctr_ngram_last_error()
    with pytest.raises(ValueError):
        lm.flat(["<blank>"] + list(lr.chars_of(8)) + ["<unknown>"])
    path3 = str(tmp_path / "m3.arpa")
    lr.write_arpa(path3, 3, 6, seed=1)
    lm3 = codec_mod.ArpaLM(path3)
    assert lib.hctr_lm_build(None, words.ctypes.data_as(vp), 8, ctypes.byref(h)) == ERR_ARG
    assert lib.hctr_lm_build(lm3._h, None, 8, ctypes.byref(h)) == ERR_ARG
    assert lib.hctr_lm_build(lm3._h, words.ctypes.data_as(vp), 8, None) == ERR_ARG
    bad = words.copy()
    bad[3] = 10 ** 6
    assert lib.hctr_lm_build(lm3._h, bad.ctypes.data_as(vp), 8, ctypes.byref(h)) == ERR_ARG and not h.value
    assert lib.hctr_lm_build(lm3._h, words.ctypes.data_as(vp), 8, ctypes.byref(h)) == 0 and h.value
    assert lib.hctr_lm_order(h) == 3 and lib.hctr_lm_order(None) == 0
    assert np.isnan(lib.hctr_lm_word_logp(None, None, 0, 0))
    lib.hctr_lm_free(h)
    lib.hctr_lm_free(None)


def _lists(seed, T, B, C, k):
    rng = np.random.RandomState(seed)
    return nr.topk_lists(nr.planted_lines(rng, T, B, C, density=0.35, boost=6.0), k)


def test_memoised_yardstick_equals_the_plain_one(tmp_path):
    path = str(tmp_path / "m.arpa")
    lr.write_arpa(path, 3, 8, seed=2)
    T, B, C, k = 14, 2, 12, 6
    idx, lp = _lists(11, T, B, C, k)
    arpa = ArpaRef(path)
    fast = lr.search(lr.make_codec(C, k, arpa, 2, 5.8), idx, lp, 6, 6)
    plain = lr.search(lr.make_codec(C, k, arpa, 2, 5.8, memo=False), idx, lp, 6, 6)
    assert (fast["count"] > 0).all()
    for f in ("labels", "lengths", "logp", "score", "lm", "count", "ends"):
        assert fast[f].tobytes() == plain[f].tobytes(), f
    assert fast["gap"] == plain["gap"]


@pytest.mark.parametrize("order,unk,pen,bonus", [(3, True, 2.0, 5.8), (5, True, 0.8, 4.8), (3, False, 2.0, 5.8)])
def test_yardstick_one_best_is_the_host_search(lib, pkg, codec_mod, tmp_path, order, unk, pen, bonus):
    path = str(tmp_path / "m.arpa")
    lr.write_arpa(path, order, 14, seed=5, unk=unk)
    T, B, C, k, beam = 40, 4, 18, 10, 10
    idx, lp = _lists(20 + order, T, B, C, k)
    idx[30:, 0, 0], idx[30:, 0, 1] = 0, idx[30:, 0, 0].copy() + (idx[30:, 0, 0] == 0)      # line 0 ends early
    ref = lr.search(lr.make_codec(C, k, path, pen, bonus), idx, lp, beam, 1)
    assert ref["ends"][0] < T and (ref["count"] == 1).all()
    lm = codec_mod.ArpaLM(path)
    chars = ["<blank>"] + list(lr.chars_of(C)) + ["<unknown>"]
    words = lm.label_words(chars)
    lb = importlib.import_module(pkg.__name__ + "._lib")
    P = lb.BeamParams()
    P.skip_search, P.beam_size, P.search_depth, P.lm_panelty, P.len_bonus = 0, beam, k, pen, bonus
    P.builtin_lm, P.num_threads, P.ngram, P.label_words = 3, 1, lm._h, words.ctypes.data
    labels, lengths, status = np.zeros((B, T), np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    blank = np.zeros((T, B), np.float32)
    rc = lib.hctr_beam_search(ctypes.byref(P), T, B, C, k, idx.ctypes.data_as(vp), lp.ctypes.data_as(vp),
                              blank.ctypes.data_as(vp), None, None, None, None, labels.ctypes.data_as(vp),
                              lengths.ctypes.data_as(vp), status.ctypes.data_as(vp))
    assert rc == 0
    for b in range(B):
        assert labels[b, :lengths[b]].tolist() == ref["labels"][b, 0, :ref["lengths"][b, 0]].tolist(), b
        assert lengths[b] > 0
