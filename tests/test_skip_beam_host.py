"""Host tests (no GPU) of tests/skip_beam_ref.py, the yardstick of the device skip search (hctr_nbest_skip*):
  * its 1-best is the REAL reference's ``skip_zero`` string of tests/golden/codec_cases.json for every CODEC_CASES entry
    (run without the device's cap of 32 candidates, which mixed_wide exceeds); flat_c7358, where the reference raises
    IndexError, reports status 2;
  * its 1-best is ``oracle.ctc_ref.CtcCodecRef.beam_skip``'s text and ``hctr_beam_search(skip_search = 1, builtin_lm =
    3)``'s on lines with an n-gram model;
  * its memoised LM evaluation is bit-equal to re-scoring whole sentences with ArpaRef.
"""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest

import codec_cases
import lm_beam_ref as lr
import skip_beam_ref as sr
import skip_cases as sc
from oracle.ctc_ref import ArpaRef, CtcCodecRef

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
vp = ctypes.c_void_p

# (T, B, C, LM order, characters in the model, <unk>, lm_panelty, len_bonus, beam, seed)
LM_CASES = [
    (48, 3, 18, 3, 14, True, 2.0, 5.8, 10, 1),
    (40, 2, 40, 5, 30, True, 0.8, 4.8, 10, 2),
    (40, 2, 18, 3, 14, False, 2.0, 5.8, 10, 3),
]


def test_one_best_is_the_real_reference(tmp_path):
    with open(os.path.join(GOLDEN, "codec_cases.json"), encoding="utf-8") as f:
        gold = json.load(f)
    tag, _, _, pen, bonus, beam, _ = next(s for s in codec_cases.BEAM_SETTINGS if s[0] == "skip_zero")
    for name, seed, W, B, C, style in codec_cases.CODEC_CASES:
        chars = codec_cases.vocab(C)
        lists = sr.lists_of_logp(sc.logp_of(codec_cases.gen_logits(seed, W, B, C, style)))
        got = sr.search(sr.make_codec(C, None, pen, bonus), *lists, beam, 1, cap=None)
        want = gold[name][tag]
        if want == "IndexError":
            assert name == "flat_c7358" and got["status"].tolist() == [sr.EMPTIED] and got["count"].tolist() == [0]
            continue
        assert (got["status"] == sr.OK).all() and (got["count"] == 1).all(), name
        texts = ["".join(chars[c - 1] for c in got["labels"][b, 0, :got["lengths"][b, 0]]) for b in range(B)]
        assert texts == want, name
        if name in ("peaky_small", "peaky_wide", "single_col"):
            assert (got["ranked"] == 0).all(), name
        if name == "flat_small":
            assert (got["ranked"] == got["ends"]).all()
    # with the device's cap both lines of mixed_wide overflow
    name, seed, W, B, C, style = next(c for c in codec_cases.CODEC_CASES if c[0] == "mixed_wide")
    lists = sr.lists_of_logp(sc.logp_of(codec_cases.gen_logits(seed, W, B, C, style)))
    got = sr.search(sr.make_codec(C, None, pen, bonus), *lists, beam, 1)
    assert got["status"].tolist() == [sr.OVERFLOW] * B and (got["count"] == 0).all()


def _lm_case(tmp_path, spec):
    T, B, C, order, n_chars, unk, pen, bonus, beam, seed = spec
    path = str(tmp_path / ("skip%d.arpa" % seed))
    lr.write_arpa(path, order, n_chars, seed=seed, unk=unk)
    z = sc.mixed_lines(50 + seed, T, B, C)
    sc.quiet_tail(z, 0, T - 9)
    return path, sc.logp_of(z)


@pytest.mark.parametrize("spec", LM_CASES)
def test_one_best_is_the_oracle_and_the_host_search(pkg, tmp_path, spec):
    T, B, C, order, n_chars, unk, pen, bonus, beam, seed = spec
    path, logp = _lm_case(tmp_path, spec)
    top1, blank, off, ci, cl = sr.lists_of_logp(logp)
    got = sr.search(sr.make_codec(C, path, pen, bonus), top1, blank, off, ci, cl, beam, 1)
    assert (got["status"] == sr.OK).all() and (got["ranked"] > 0).all() and (got["ranked"] < got["ends"]).all()
    assert got["ends"][0] < T - 4
    mine = [got["labels"][b, 0, :got["lengths"][b, 0]].tolist() for b in range(B)]
    # the oracle's own skip search on the full log-prob rows
    oc = CtcCodecRef(lr.chars_of(C))
    oc.ngram, oc.use_tfm_pred, oc.beam_size, oc.lm_panelty, oc.len_bonus = ArpaRef(path), False, beam, pen, bonus
    oc.search_depth = 1
    assert [[ord(ch) - lr.BASE for ch in s] for s in oc.beam_skip(logp)] == mine
    # the host search of the library
    codec_mod = importlib.import_module(pkg.__name__ + ".codec")
    lb = importlib.import_module(pkg.__name__ + "._lib")
    lib = pkg.load_library()
    lm = codec_mod.ArpaLM(path)
    words = lm.label_words(["<blank>"] + list(lr.chars_of(C)) + ["<unknown>"])
    P = lb.BeamParams()
    P.skip_search, P.beam_size, P.search_depth, P.lm_panelty, P.len_bonus = 1, beam, 1, pen, bonus
    P.builtin_lm, P.num_threads, P.ngram, P.label_words = 3, 1, lm._h, words.ctypes.data
    labels, lengths, status = np.zeros((B, T), np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    tl = np.ascontiguousarray(np.take_along_axis(logp, top1[:, :, None].astype(np.int64), axis=2))
    rc = lib.hctr_beam_search(ctypes.byref(P), T, B, C, 1, top1.ctypes.data_as(vp), tl.ctypes.data_as(vp),
                              blank.ctypes.data_as(vp), off.ctypes.data_as(vp), ci.ctypes.data_as(vp),
                              cl.ctypes.data_as(vp), None, labels.ctypes.data_as(vp), lengths.ctypes.data_as(vp),
                              status.ctypes.data_as(vp))
    assert rc == 0 and (status == 0).all()
    assert [labels[b, :lengths[b]].tolist() for b in range(B)] == mine


def test_memoised_yardstick_equals_the_plain_one(tmp_path):
    spec = (30, 2, 12, 3, 8, True, 2.0, 5.8, 6, 4)
    T, B, C, order, n_chars, unk, pen, bonus, beam, seed = spec
    path, logp = _lm_case(tmp_path, spec)
    lists = sr.lists_of_logp(logp)
    arpa = ArpaRef(path)
    fast = sr.search(sr.make_codec(C, arpa, pen, bonus), *lists, beam, beam)
    plain = sr.search(sr.make_codec(C, arpa, pen, bonus, memo=False), *lists, beam, beam)
    assert (fast["count"] > 0).all() and (fast["ranked"] > 0).all()
    for f in ("labels", "lengths", "logp", "score", "lm", "count", "status", "ranked", "ends", "dup_steps"):
        assert fast[f].tobytes() == plain[f].tobytes(), f
    assert fast["gap"] == plain["gap"]


def test_crafted_lines_do_what_they_are_for():
    """the duplicate line starts ranked steps from a list with a text twice; the branch line takes all four in-place
    branches on a list of several hypotheses"""
    codec = sr.make_codec(6, None, 2.0, 5.8)
    for seed in range(6):
        got = sr.search(codec, *sr.lists_of_logp(sc.logp_of(sc.duplicate_line(seed))), 4, 4)
        assert got["dup_steps"][0] >= 1 and got["status"][0] == sr.OK, seed
    got = sr.search(codec, *sr.lists_of_logp(sc.logp_of(sc.branch_line())), 8, 8)
    assert {(br, True) for br in (1, 2, 3, 4)} <= got["branches"]
