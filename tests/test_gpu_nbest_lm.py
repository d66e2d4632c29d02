"""GPU tests (-m gpu) of the device prefix beam search with an n-gram model (C ABI hctr_nbest_lm_topk /
hctr_nbest_lm_logits / hctr_nbest_lm, ``hctr_model.nbest(lm=)``, ``ctc_codec.nbest(lm=)``).

The yardstick is tests/lm_beam_ref.py: ``oracle.ctc_ref.CtcCodecRef.step`` with ``ArpaRef`` and the codec's own greedy
line, suffixes and end step (tests/test_lm_beam_host.py checks the yardstick and the flat table on the host). What must
hold, through hctr_nbest_lm_topk on identical float32 lists:
  * counts, lengths, labels and the n-gram score ``lm`` EXACTLY: ``lm`` is a sum of float32 values widened to double,
    added in the same order on both sides;
  * logp and score within 1e-14 * T * max(1, |want|), the figure tests/test_gpu_nbest.py uses for the device's log1p /
    exp; each case first asserts, on the yardstick alone, that its smallest nonzero gap between adjacent totals is at
    least 100x that tolerance (seeds were picked on the CPU so that it is);
  * a line with an empty greedy text returns nothing and disturbs no other line; lm_panelty = 0 is the plain search over
    the end steps; the 1-best is hctr_beam_search(builtin_lm = 3)'s text; the three entry points agree byte for byte, also
    through the stored-logits front end in a fresh process; two models alternate on one context; the new argument errors;
    no LM call changes what the other entry points return.
"""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import lm_beam_ref as lr
import nbest_lm_child as shared
import nbest_ref as nr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
vp = ctypes.c_void_p
PLAIN = ("labels", "lengths", "logps", "scores", "counts")


@pytest.fixture(scope="module")
def ctc(pkg):
    return importlib.import_module(pkg.__name__ + ".ctc")


@pytest.fixture(scope="module")
def codec_mod(pkg):
    return importlib.import_module(pkg.__name__ + ".codec")


@pytest.fixture(scope="module")
def ctx(pkg):
    al = pkg.CTCAligner().cuda(0)
    yield al._context()                       # a weightless context: the list and logits entries need no weights
    del al


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("nbest_lm")


def _tol(T, want):
    return 1e-14 * T * np.maximum(1.0, np.abs(want))


# (name, T, B, C, k, beam, nbest, LM order, characters in the model, <unk>, lm_panelty, len_bonus, seed): the smallest
# shapes at which each part can go wrong - one step; the reference's defaults with ragged input_lengths, OOV labels and a
# line whose text ends more than 4 columns before its L_b; k = C (so <unknown> is in every row) on the widest instance;
# the middle instance with a 5-gram model; the longest context the table holds; the -100 path of a model without <unk>;
# the workload's class count, where almost every label is OOV
CASES = [
    ("one step, unigram model", 2, 1, 5, 2, 2, 2, 1, 3, True, 2.0, 5.8, 0),
    ("defaults, ragged, OOV", 63, 3, 18, 10, 10, 10, 3, 14, True, 2.0, 5.8, 1),
    ("k = C, widest instance", 40, 1, 12, 12, 32, 32, 2, 8, True, 0.8, 4.8, 2),
    ("middle instance", 65, 3, 40, 12, 16, 16, 5, 30, True, 2.0, 5.8, 3),
    ("longest context", 33, 1, 40, 10, 10, 1, 6, 30, True, 2.0, 5.8, 4),
    ("model without <unk>", 33, 2, 18, 10, 10, 10, 3, 14, False, 2.0, 5.8, 5),
    ("workload classes", 130, 2, 7375, 10, 10, 10, 3, 14, True, 2.0, 5.8, 6),
]
_DONE = {}


def _spec(name):
    return next(c for c in CASES if c[0] == name)


def arpa_of(work, name):
    _, _, _, _, _, _, _, order, n_chars, unk, _, _, seed = _spec(name)
    path = os.path.join(str(work), "case%d.arpa" % seed)
    if not os.path.exists(path):
        lr.write_arpa(path, order, n_chars, seed=seed, unk=unk)
    return path


def lists_of(name):
    _, T, B, C, k, _, _, _, n_chars, _, _, _, seed = _spec(name)
    rng = np.random.RandomState(2000 + seed)
    z = nr.planted_lines(rng, T, B, C, density=0.35, boost=6.0)
    if C > 1000:                               # keep some planted classes inside the model's few characters
        cls = z.argmax(axis=2)
        for b in range(B):
            for t in range(0, T, 3):
                if cls[t, b] not in (0, C - 1):
                    z[t, b, 1 + (cls[t, b] % n_chars)] += np.float32(7.0)
    il = None if B == 1 else np.maximum(1, T - np.arange(B) * max(1, T // 7)).astype(np.int32)
    if name == "defaults, ragged, OOV":        # line 0: nothing but blanks after column 40, so end_0 < L_0 = 63
        z[41:, 0, 1:] -= np.float32(20.0)
        z[41:, 0, 0] += np.float32(9.0)
    idx, lp = nr.topk_lists(z, k)
    return idx, lp, il


def case(work, name):
    """(idx, lp, input_lengths, yardstick results) of a case, computed once"""
    if name not in _DONE:
        _, T, B, C, k, beam, nbest, _, _, _, pen, bonus, _ = _spec(name)
        idx, lp, il = lists_of(name)
        codec = lr.make_codec(C, k, arpa_of(work, name), pen, bonus)
        _DONE[name] = (idx, lp, il, lr.search(codec, idx, lp, beam, nbest, il))
    return _DONE[name]


def flat_of(codec_mod, work, name, keep={}):
    if name not in keep:
        C = _spec(name)[3]
        lm = codec_mod.ArpaLM(arpa_of(work, name))
        keep[name] = (lm, lm.flat(["<blank>"] + list(lr.chars_of(C)) + ["<unknown>"]))
    return keep[name]


def run(ctc, codec_mod, ctx, work, name, **over):
    _, T, B, C, k, beam, nbest, _, _, _, pen, bonus, _ = _spec(name)
    idx, lp, il, _ = case(work, name)
    kw = dict(n=nbest, beam=beam, len_bonus=bonus, input_lengths=il, lm=flat_of(codec_mod, work, name)[1], lm_panelty=pen)
    kw.update(over)
    return ctc.nbest_topk(ctx, idx, lp, C, **kw)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_against_yardstick(ctc, codec_mod, ctx, work, name):
    _, T, B, C, k, beam, nbest, order, _, _, pen, bonus, _ = _spec(name)
    idx, lp, il, want = case(work, name)
    fin = np.isfinite(want["score"])
    worst = float(_tol(T, np.concatenate([want["logp"][fin], want["score"][fin]])).max())
    print("%s: smallest nonzero gap between adjacent totals %.3e, tolerance at most %.3e, end steps %s"
          % (name, want["gap"], worst, want["ends"].tolist()))
    assert want["gap"] >= 100 * worst, "the yardstick's own ranking is not settled at this seed"
    assert (want["count"] > 0).all()
    if name == "defaults, ragged, OOV":
        assert want["ends"][0] < il[0] - 4
    got = run(ctc, codec_mod, ctx, work, name)
    np.testing.assert_array_equal(got.counts, want["count"])
    np.testing.assert_array_equal(got.lengths, want["lengths"])
    np.testing.assert_array_equal(got.labels, want["labels"])
    assert got.lm_scores.tobytes() == want["lm"].tobytes(), (got.lm_scores, want["lm"])
    for g, w, what in ((got.logps, want["logp"], "logp"), (got.scores, want["score"], "score")):
        np.testing.assert_array_equal(g[~fin], w[~fin], err_msg=what)
        err = np.abs(g[fin] - w[fin])
        print("%s %s: max |d| %.3e over %d figures" % (name, what, err.max() if err.size else 0.0, err.size))
        assert (err <= _tol(T, w[fin])).all(), (name, what, g, w)


def test_empty_greedy_line(ctc, codec_mod, ctx, work):
    """line 1's top-1 class is the blank or <unknown> in every column: count 0 there (the host search reports
    HCTR_ERR_EMPTY_LINE), the call returns, and lines 0 and 2 equal their single-line results"""
    name = "defaults, ragged, OOV"
    _, T, B, C, k, beam, nbest, _, _, _, pen, bonus, _ = _spec(name)
    idx, lp, il, _ = case(work, name)
    idx, lp = idx.copy(), lp.copy()
    for t in range(T):
        c = 0 if t % 5 else C - 1
        j = int(np.flatnonzero(idx[t, 1] == c)[0]) if (idx[t, 1] == c).any() else k - 1
        idx[t, 1, j] = idx[t, 1, 0]
        idx[t, 1, 0] = c
    lp[:, 1, :] = -np.sort(-lp[:, 1, :], axis=1)
    flat = flat_of(codec_mod, work, name)[1]
    kw = dict(n=nbest, beam=beam, len_bonus=bonus, lm=flat, lm_panelty=pen)
    got = ctc.nbest_topk(ctx, idx, lp, C, input_lengths=il, **kw)
    assert got.counts[1] == 0 and (got.lengths[1] == 0).all() and (got.labels[1] == 0).all()
    assert (got.logps[1] == -np.inf).all() and (got.scores[1] == -np.inf).all() and (got.lm_scores[1] == -np.inf).all()
    for b in (0, 2):
        one = ctc.nbest_topk(ctx, idx[:, b:b + 1], lp[:, b:b + 1], C, input_lengths=il[b:b + 1], **kw)
        assert one.counts[0] > 0
        for f in shared.FIELDS:
            assert getattr(got, f)[b].tobytes() == getattr(one, f)[0].tobytes(), (b, f)


@pytest.mark.parametrize("name", ["defaults, ragged, OOV", "middle instance"])
def test_zero_penalty_is_the_plain_search(ctc, codec_mod, ctx, work, name):
    """lm_panelty = 0: the texts, logp bytes and counts of hctr_nbest_topk over input_lengths = the end steps"""
    _, T, B, C, k, beam, nbest, _, _, _, pen, bonus, _ = _spec(name)
    idx, lp, il, want = case(work, name)
    got = run(ctc, codec_mod, ctx, work, name, lm_panelty=0.0)
    plain = ctc.nbest_topk(ctx, idx, lp, C, n=nbest, beam=beam, len_bonus=bonus, input_lengths=want["ends"])
    for f in ("labels", "lengths", "logps", "counts"):
        assert getattr(got, f).tobytes() == getattr(plain, f).tobytes(), f
    assert np.isfinite(got.lm_scores[:, 0]).all()


@pytest.mark.parametrize("name", ["defaults, ragged, OOV", "model without <unk>"])
def test_one_best_is_the_host_search(pkg, ctc, codec_mod, ctx, work, name):
    _, T, B, C, k, beam, nbest, _, _, _, pen, bonus, _ = _spec(name)
    idx, lp, il, _ = case(work, name)
    got = run(ctc, codec_mod, ctx, work, name, n=1)
    lm, _ = flat_of(codec_mod, work, name)
    words = lm.label_words(["<blank>"] + list(lr.chars_of(C)) + ["<unknown>"])
    lb = importlib.import_module(pkg.__name__ + "._lib")
    lib = pkg.load_library()
    for b in range(B):                                     # the host search takes no input_lengths: line by line
        L = int(il[b])
        i1, l1 = np.ascontiguousarray(idx[:L, b:b + 1]), np.ascontiguousarray(lp[:L, b:b + 1])
        P = lb.BeamParams()
        P.skip_search, P.beam_size, P.search_depth, P.lm_panelty, P.len_bonus = 0, beam, k, pen, bonus
        P.builtin_lm, P.num_threads, P.ngram, P.label_words = 3, 1, lm._h, words.ctypes.data
        labels, lengths, status = np.zeros((1, L), np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
        blank = np.zeros((L, 1), np.float32)
        rc = lib.hctr_beam_search(ctypes.byref(P), L, 1, C, k, i1.ctypes.data_as(vp), l1.ctypes.data_as(vp),
                                  blank.ctypes.data_as(vp), None, None, None, None, labels.ctypes.data_as(vp),
                                  lengths.ctypes.data_as(vp), status.ctypes.data_as(vp))
        assert rc == 0 and lengths[0] > 0
        assert got.labels[b, 0, :got.lengths[b, 0]].tolist() == labels[0, :lengths[0]].tolist(), b


def test_entries_agree(pkg, work):
    shared.check_logits_entry(pkg, work)
    shared.check_images(pkg, work)


def test_entries_agree_through_stored_logits(work):
    env = dict(os.environ, HCTR_FUSE_BEAM="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "nbest_lm_child.py"), str(work)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_two_models_alternate_on_one_context(ctc, codec_mod, ctx, work):
    """the context keeps the device copy of the model used last, recognised by its serial number"""
    name = "defaults, ragged, OOV"
    _, T, B, C, k, beam, nbest, _, _, _, pen, bonus, _ = _spec(name)
    idx, lp, il, want = case(work, name)
    chars = ["<blank>"] + list(lr.chars_of(C)) + ["<unknown>"]
    path_b = os.path.join(str(work), "other.arpa")
    lr.write_arpa(path_b, 2, 16, seed=77)
    lm_a, lm_b = codec_mod.ArpaLM(arpa_of(work, name)), codec_mod.ArpaLM(path_b)
    kw = dict(n=nbest, beam=beam, len_bonus=bonus, input_lengths=il, lm_panelty=pen)
    a1 = ctc.nbest_topk(ctx, idx, lp, C, lm=lm_a.flat(chars), **kw)
    b1 = ctc.nbest_topk(ctx, idx, lp, C, lm=lm_b.flat(chars), **kw)
    a2 = ctc.nbest_topk(ctx, idx, lp, C, lm=lm_a.flat(chars), **kw)
    b2 = ctc.nbest_topk(ctx, idx, lp, C, lm=lm_b.flat(chars), **kw)
    assert a1.lm_scores.tobytes() == want["lm"].tobytes()
    assert a1.lm_scores.tobytes() != b1.lm_scores.tobytes() and a1.scores.tobytes() != b1.scores.tobytes()
    shared.same(a1, a2, "model A again")
    shared.same(b1, b2, "model B again")
    # a second object built from model A has another serial number and gives A's results
    lib, h = codec_mod._lib.load(), vp()
    words = lm_a.label_words(chars)
    assert lib.hctr_lm_build(lm_a._h, words.ctypes.data_as(vp), C, ctypes.byref(h)) == 0
    try:
        shared.same(a1, ctc.nbest_topk(ctx, idx, lp, C, lm=h, **kw), "model A rebuilt")
    finally:
        lib.hctr_lm_free(h)


def test_argument_errors(pkg, codec_mod, ctx, work):
    lib = pkg.load_library()
    name = "one step, unigram model"
    _, T, B, C, k, beam, nbest, _, _, _, pen, bonus, _ = _spec(name)
    idx, lp, _, _ = case(work, name)
    flat = flat_of(codec_mod, work, name)[1]
    other = flat_of(codec_mod, work, "defaults, ragged, OOV")[1]            # built for C = 18
    outs = [np.zeros((B, nbest, T), np.int32), np.zeros((B, nbest), np.int32)]

    def call(lm=flat, pen=pen, bonus=bonus, beam=beam, nbest=nbest, k=k, idx=idx):
        return lib.hctr_nbest_lm_topk(ctx, lm, None if idx is None else idx.ctypes.data_as(vp), lp.ctypes.data_as(vp), T, B,
                                      C, k, beam, nbest, ctypes.c_double(pen), ctypes.c_double(bonus), None,
                                      outs[0].ctypes.data_as(vp), outs[1].ctypes.data_as(vp), None, None, None, None)

    assert call() == 0
    for kw in (dict(lm=None), dict(pen=float("nan")), dict(lm=other), dict(bonus=float("nan")), dict(beam=33),
               dict(nbest=0), dict(k=C + 1), dict(idx=None)):
        assert call(**kw) == ERR_ARG, kw
        assert lib.hctr_last_error(ctx), kw
    z = np.zeros((T, B, C), np.float32)
    assert lib.hctr_nbest_lm_logits(ctx, None, z.ctypes.data_as(vp), 0, T, B, C, k, beam, nbest, ctypes.c_double(pen),
                                    ctypes.c_double(bonus), None, None, None, None, None, None, None) == ERR_ARG
    assert b"lm" in lib.hctr_last_error(ctx)
    assert lib.hctr_nbest_lm_logits(ctx, other, z.ctypes.data_as(vp), 0, T, B, C, k, beam, nbest, ctypes.c_double(pen),
                                    ctypes.c_double(bonus), None, None, None, None, None, None, None) == ERR_ARG
    assert b"18" in lib.hctr_last_error(ctx)
    assert call() == 0                                     # the context is still usable
    assert lib.hctr_nbest_lm_topk(ctx, flat, None, None, T, 0, C, k, beam, nbest, ctypes.c_double(pen),
                                  ctypes.c_double(bonus), None, None, None, None, None, None, None) == 0      # a no-op


def test_no_side_effects(pkg, synth, ctc, codec_mod, work):
    """greedy and zero-LM nbest results of a context, and the guard figures of auto precision, are what they were after
    LM-scored calls on it"""
    C = synth.DEFAULT_VOCAB + 2
    m = pkg.hctr_model(C, precision="auto").cuda(0)
    m.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    cd = pkg.ctc_codec(synth.characters())
    imgs = synth.make_font_lines(3, 96, 31)
    rng = np.random.RandomState(12)
    logits = rng.standard_normal((90, 3, 40)).astype(np.float32)

    def others():
        g = m.greedy(imgs)
        guard = m.last_guard()
        nb = m.nbest(imgs)
        nl = ctc.nbest_logits(m._ctx, logits, 0, n=4, beam=8, depth=8, len_bonus=5.8)
        return g, guard, [getattr(r, f) for r in (nb, nl) for f in PLAIN]

    g0, guard0, arrays0 = others()
    path = os.path.join(str(work), "side.arpa")
    lr.write_arpa(path, 3, list(synth.characters())[:40], seed=9)
    lm = codec_mod.ArpaLM(path)
    res = m.nbest(imgs, lm=lm, codec=cd, len_bonus=5.8)
    assert res.lm_scores is not None
    small = pkg.ctc_codec(lr.chars_of(40))
    ctc.nbest_logits(m._ctx, logits, 0, n=4, beam=8, depth=8, len_bonus=5.8, lm=lm.flat(small.characters))
    g1, guard1, arrays1 = others()
    for x, y in zip(g0, g1):
        np.testing.assert_array_equal(x, y)
    for i, (x, y) in enumerate(zip(arrays0, arrays1)):
        assert x.tobytes() == y.tobytes(), i
    assert guard0["lines"] == guard1["lines"] and guard0["flagged"] == guard1["flagged"]
    for f in ("flags", "min_margin", "scale"):
        np.testing.assert_array_equal(guard0[f], guard1[f])
