"""GPU tests (-m gpu) of the device prefix beam search (C ABI hctr_nbest_topk / hctr_nbest_logits / hctr_nbest,
``hctr_model.nbest``, ``ctc_codec.nbest``): the N best texts of a line with their log-probabilities.

The yardstick is tests/nbest_ref.py: ``oracle.ctc_ref.CtcCodecRef.step`` with a zero LM, driven over the caller's number
of steps (tests/test_nbest_host.py checks the yardstick itself). What must hold:
  * through hctr_nbest_topk, on identical float32 lists: labels, lengths and counts exact, logp and score within
    1e-14 * T * max(1, |want|) - both sides are float64 sums and logaddexps of the same inputs, a few ulp per step. A
    reordering would need two totals closer than that, so each case first asserts, on the oracle alone, that its smallest
    nonzero gap between adjacent totals is at least 100x the tolerance;
  * exact ties are decided by first touch, and a prefix re-derived as an extension is one entry at the earlier place;
  * the degenerate counts, -inf log-probs and NaN rows follow the contract;
  * logp is a lower bound of the text's -CTC loss, with equality when the search cannot cut;
  * the logits entry equals the list entry on hctr_beam_frontend's lists, the image entry equals the list entry on
    hctr_beam_frontend's output of the same images and mode (the fused front end included), bit for bit and across
    internal passes; host-pointer, device-pointer and repeated calls are bit-identical; every output may be NULL;
  * with the reference's end step and len_bonus 5.8 the 1-best is hctr_beam_search's text (zero LM);
  * argument errors are HCTR_ERR_ARG with a message, and no N-best call changes what the other entry points return.
"""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import nbest_ref as nr
from oracle import ctc_ref

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-3                      # engine figure vs float64 on the same logits (tests/test_gpu_ctc.py's)
FIELDS = ("labels", "lengths", "logps", "scores", "counts")
ERR_ARG = -1


@pytest.fixture(scope="module")
def ctc(pkg):
    return importlib.import_module(pkg.__name__ + ".ctc")


@pytest.fixture(scope="module")
def model_mod(pkg):
    return importlib.import_module(pkg.__name__ + ".model")


@pytest.fixture(scope="module")
def aligner(pkg):
    return pkg.CTCAligner().cuda(0)


@pytest.fixture(scope="module")
def ctx(aligner):
    return aligner._context()                 # a weightless context: the list and logits entries need no weights


@pytest.fixture(scope="module")
def m_trained(pkg, synth):
    C = synth.DEFAULT_VOCAB + 2
    m = pkg.hctr_model(C, precision="auto").cuda(0)
    m.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    return m


def _same(a, b, what):
    for k in FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s: %s differs" % (what, k)


def _tol(T, want):
    return 1e-14 * T * np.maximum(1.0, np.abs(want))


# (name, T, B, C, k, beam, nbest, len_bonus, style, seed): T at and around one wave's 64, beam and k at the ends and
# inside of the three instances (<= 10/10, <= 16/16, <= 32/32), nbest 1 and beam, ragged input_lengths for B > 1,
# k = C cases have <unknown> (C-1) in every row
CASES = [
    ("one step", 1, 1, 5, 1, 1, 1, 0.0, "flat", 0),
    ("two steps", 2, 3, 7, 2, 2, 2, 5.8, "flat", 1),
    ("10/10 ragged", 63, 3, 40, 10, 10, 10, 5.8, "planted", 2),
    ("k = C, beam 32", 64, 5, 12, 12, 32, 1, 0.0, "flat", 3),
    ("k = C, all 32 back", 65, 1, 12, 12, 32, 32, 5.8, "planted", 4),
    ("32/32", 130, 1, 300, 32, 32, 1, 0.0, "flat", 5),
    ("workload classes", 130, 3, 7375, 10, 10, 10, 5.8, "planted", 6),
    ("narrow rows, wide beam", 64, 3, 40, 2, 10, 10, 0.0, "planted", 7),
    ("wide rows, beam 2", 65, 3, 40, 10, 2, 1, 5.8, "flat", 8),
    ("k 32, beam 1", 63, 1, 300, 32, 1, 1, 0.0, "planted", 9),
    ("middle instance", 65, 5, 40, 12, 16, 16, 5.8, "flat", 10),
]
_ORACLE = {}


def _case(name):
    """(idx, lp, input_lengths, oracle results) of a case, computed once"""
    if name not in _ORACLE:
        _, T, B, C, k, beam, nbest, bonus, style, seed = next(c for c in CASES if c[0] == name)
        rng = np.random.RandomState(1000 + seed)
        z = (rng.standard_normal((T, B, C)).astype(np.float32) * 2 if style == "flat"
             else nr.planted_lines(rng, T, B, C, density=0.35, boost=6.0))
        idx, lp = nr.topk_lists(z, k)
        il = None if B == 1 else np.maximum(1, T - np.arange(B) * max(1, T // 7)).astype(np.int32)
        _ORACLE[name] = (idx, lp, il, nr.search(idx, lp, C, beam, nbest, bonus, il))
    return _ORACLE[name]


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_against_restatement(ctc, ctx, name):
    _, T, B, C, k, beam, nbest, bonus, _, _ = next(c for c in CASES if c[0] == name)
    idx, lp, il, (labels, lengths, logp, score, count, gap, _) = _case(name)
    fin = np.isfinite(score)
    worst = float(_tol(T, np.concatenate([logp[fin], score[fin]])).max())
    print("%s: smallest nonzero gap between adjacent totals %.3e, tolerance at most %.3e" % (name, gap, worst))
    assert gap >= 100 * worst, "the oracle's own ranking is not settled at this seed"
    got = ctc.nbest_topk(ctx, idx, lp, C, n=nbest, beam=beam, len_bonus=bonus, input_lengths=il)
    np.testing.assert_array_equal(got.counts, count)
    np.testing.assert_array_equal(got.lengths, lengths)
    np.testing.assert_array_equal(got.labels, labels)
    for g, w, what in ((got.logps, logp, "logp"), (got.scores, score, "score")):
        np.testing.assert_array_equal(g[~fin], w[~fin], err_msg=what)
        err = np.abs(g[fin] - w[fin])
        print("%s %s: max |d| %.3e over %d figures" % (name, what, err.max() if err.size else 0.0, err.size))
        assert (err <= _tol(T, w[fin])).all(), (name, what, g, w)
    assert (count > 0).all()


def _lists(rows, k):
    """[T, 1, k] lists from [(classes, log-probs), ...]"""
    idx = np.array([r[0] for r in rows], np.int32).reshape(len(rows), 1, k)
    lp = np.array([r[1] for r in rows], np.float32).reshape(len(rows), 1, k)
    return idx, lp


def _texts(res, b=0):
    return [v.tolist() for v in res.label_lists()[b]]


def test_exact_ties_follow_first_touch(ctc, ctx):
    """two classes with equal float32 log-probs in consecutive steps, beam 3: every cut falls inside a tie"""
    C = 6
    row = ([1, 2, 0], [-1.0, -1.0, -2.0])
    idx, lp = _lists([row, row, row], 3)
    for steps, want in ((1, [[1], [2], []]), (2, [[1], [2], [1, 2]])):
        il = np.array([steps], np.int32)
        got = ctc.nbest_topk(ctx, idx, lp, C, n=3, beam=3, input_lengths=il)
        labels, lengths, logp, score, count, _, _ = nr.search(idx, lp, C, 3, 3, 0.0, il)
        assert _texts(got) == want and got.counts[0] == 3
        np.testing.assert_array_equal(got.labels, labels)
        np.testing.assert_array_equal(got.lengths, lengths)
        assert np.abs(got.scores - score).max() <= 1e-14 * steps * 4
    assert got.scores[0, 0] == got.scores[0, 1]                    # "1" and "2": the same arithmetic, the same bits
    got = ctc.nbest_topk(ctx, idx, lp, C, n=3, beam=3)
    labels, lengths = nr.search(idx, lp, C, 3, 3)[:2]
    np.testing.assert_array_equal(got.labels, labels)
    np.testing.assert_array_equal(got.lengths, lengths)


def test_rederived_prefix_is_one_entry_at_the_earlier_place(ctc, ctx):
    """After two steps the list is ["", "1"], both at -2. Step 3 (classes 1 and 2 at -1): "" + 1 re-derives "1" before
    hypothesis "1" is reached, so the merged entry stands where the extension stood: the entries are "" (-inf), "1", "2",
    "11", "12", all at -3, and beam 3 keeps "1", "2", "11". At the prefix's own place it would be "2", "1", "11"."""
    C = 6
    idx, lp = _lists([([1, 0], [-1.0, -1.0]), ([0, 5], [-1.0, -3.0]), ([1, 2], [-1.0, -1.0])], 2)
    two = ctc.nbest_topk(ctx, idx, lp, C, n=3, beam=3, input_lengths=np.array([2], np.int32))
    assert _texts(two) == [[], [1]] and two.counts[0] == 2 and two.logps[0].tolist()[:2] == [-2.0, -2.0]
    got = ctc.nbest_topk(ctx, idx, lp, C, n=3, beam=3)
    assert _texts(got) == [[1], [2], [1, 1]]
    assert got.logps[0].tolist() == [-3.0, -3.0, -3.0]              # "1": one entry, -inf (+) (-2 + -1), not two
    labels, lengths, logp = nr.search(idx, lp, C, 3, 3)[:3]
    np.testing.assert_array_equal(got.labels, labels)
    np.testing.assert_array_equal(got.logps, logp)
    five = ctc.nbest_topk(ctx, idx, lp, C, n=5, beam=5)
    assert _texts(five) == [[1], [2], [1, 1], [1, 2], []] and five.logps[0, 4] == -np.inf and five.counts[0] == 5
    # summed mass: the same step with hypothesis "1" holding non-blank mass too
    idx, lp = _lists([([1, 0], [-1.0, -1.5]), ([1, 0], [-1.0, -1.5])], 2)
    got = ctc.nbest_topk(ctx, idx, lp, C, n=3, beam=3)
    want = nr.search(idx, lp, C, 3, 3)
    np.testing.assert_array_equal(got.labels, want[0])
    one = _texts(got).index([1])
    mass = np.logaddexp(np.logaddexp(-1.0 + -1.0, -1.5 + -1.0), -1.0 + -1.5)      # repeat, from "", blank after "1"
    assert abs(got.logps[0, one] - mass) <= 1e-14 * 2 * abs(mass)


def test_degenerate_counts(ctc, ctx):
    C = 5
    # k = 1 and a step whose only class is <unknown>: nothing is left
    idx, lp = _lists([([1], [-0.5]), ([4], [-0.25]), ([2], [-0.125])], 1)
    got = ctc.nbest_topk(ctx, idx, lp, C, n=2, beam=2)
    assert got.counts.tolist() == [0] and (got.lengths == 0).all() and (got.labels == 0).all()
    assert (got.logps == -np.inf).all() and (got.scores == -np.inf).all()
    # k = 1, blank only: the empty text with the sum of the blank log-probs
    idx, lp = _lists([([0], [-0.3]), ([0], [-0.7]), ([0], [-0.11])], 1)
    got = ctc.nbest_topk(ctx, idx, lp, C, n=2, beam=2, len_bonus=5.8)
    want = (np.float64(np.float32(-0.3)) + np.float64(np.float32(-0.7))) + np.float64(np.float32(-0.11))
    assert got.counts.tolist() == [1] and got.lengths[0].tolist() == [0, 0]
    assert got.logps[0].tolist() == [want, -np.inf] and got.scores[0].tolist() == [want, -np.inf]
    # a -inf log-prob in a list: its extension is an entry with total -inf, last but kept while there is room
    idx, lp = _lists([([1, 0, 2], [-0.5, -1.0, -np.inf]), ([2, 1, 0], [-0.5, -1.0, -np.inf])], 3)
    got = ctc.nbest_topk(ctx, idx, lp, C, n=8, beam=8)
    labels, lengths, logp, score, count, _, _ = nr.search(idx, lp, C, 8, 8)
    np.testing.assert_array_equal(got.counts, count)
    np.testing.assert_array_equal(got.labels, labels)
    np.testing.assert_array_equal(got.lengths, lengths)
    fin = np.isfinite(logp)
    np.testing.assert_array_equal(got.logps[~fin], logp[~fin])
    assert (~fin[0, :count[0]]).any() and not np.isnan(got.logps).any()
    assert np.abs(got.logps[fin] - logp[fin]).max() <= 1e-14 * 2 * 4


def test_nan_row_leaves_other_lines_alone(ctc, ctx):
    name = "10/10 ragged"
    _, T, B, C, k, beam, nbest, bonus, _, _ = next(c for c in CASES if c[0] == name)
    idx, lp, il, _ = _case(name)
    clean = ctc.nbest_topk(ctx, idx, lp, C, n=nbest, beam=beam, len_bonus=bonus, input_lengths=il)
    bad = lp.copy()
    bad[7, 1, :] = np.nan
    bad[20, 1, 3] = np.nan
    got = ctc.nbest_topk(ctx, idx, bad, C, n=nbest, beam=beam, len_bonus=bonus, input_lengths=il)
    for b in (0, 2):
        for f in FIELDS:
            assert getattr(got, f)[b].tobytes() == getattr(clean, f)[b].tobytes(), (b, f)
    assert 0 <= got.counts[1] <= nbest and (got.lengths[1] >= 0).all() and (got.lengths[1] <= T).all()


def _losses(ctc, ctx, logits, res, il):
    """float64 [B, n]: -hctr_ctc_loss_logits of every returned hypothesis (n calls of B lines), NaN for unused slots"""
    B, n = res.lengths.shape
    out = np.full((B, n), np.nan)
    for i in range(n):
        tl = np.where(i < res.counts, res.lengths[:, i], 0).astype(np.int32)
        tg = np.concatenate([res.labels[b, i, :tl[b]] for b in range(B)] + [np.zeros(0, np.int32)]).astype(np.int32)
        nll = ctc.loss_logits(ctx, logits, 0, tg, tl, il)
        out[:, i] = np.where(i < res.counts, -nll.astype(np.float64), np.nan)
    return out


def test_logp_is_a_lower_bound_of_the_text_posterior(ctc, ctx):
    rng = np.random.RandomState(21)
    W, B, C = 48, 3, 30
    logits = nr.planted_lines(rng, W, B, C, density=0.35, boost=4.0)
    il = np.array([W, W - 9, 17], np.int32)
    res = ctc.nbest_logits(ctx, logits, 0, n=6, beam=6, depth=6, len_bonus=0.0, input_lengths=il)
    assert (res.counts == 6).all()
    post = _losses(ctc, ctx, logits, res, il)
    fin = np.isfinite(post)
    assert (res.logps[~fin] == -np.inf).all() and fin[:, 0].all()
    d = res.logps[fin] - post[fin]
    print("logp - (-nll): largest %.3e, smallest %.3e over %d texts" % (d.max(), d.min(), d.size))
    assert (d <= RTOL * np.abs(post[fin]) + ATOL).all(), (res.logps, post)
    p = res.posteriors()
    assert np.allclose(p.sum(axis=1), 1.0) and (p[:, 0] >= p[:, 1]).all()


@pytest.mark.parametrize("T", [1, 3, 4])
def test_uncut_search_equals_the_loss(ctc, ctx, T):
    """k = C = 4, two usable labels, T <= 4, beam 32: the search cannot cut, logp IS -nll of the text"""
    rng = np.random.RandomState(30 + T)
    C, B = 4, 3
    logits = rng.standard_normal((T, B, C)).astype(np.float32) * 2
    res = ctc.nbest_logits(ctx, logits, 0, n=32, beam=32, depth=C)
    assert (res.counts == sum(2 ** n for n in range(T + 1))).all()
    post = _losses(ctc, ctx, logits, res, None)
    used = ~np.isnan(post)
    inf = used & np.isinf(post)
    assert (res.logps[inf] == -np.inf).all()                        # texts without an alignment (a repeat needs a blank)
    ok = used & ~inf
    err = np.abs(res.logps[ok] - post[ok])
    print("T=%d: max |logp + nll| %.3e over %d texts, %d without an alignment" % (T, err.max(), ok.sum(), inf.sum()))
    assert (err <= RTOL * np.abs(post[ok]) + ATOL).all()


def test_logits_entry_equals_list_entry(pkg, ctc, model_mod, ctx):
    """hctr_nbest_logits == hctr_nbest_topk on hctr_beam_frontend's lists of the same logits, bit for bit; host pointer,
    device pointer and repeated calls agree; every output may be NULL"""
    rng = np.random.RandomState(5)
    W, B, C, k, beam, n = 70, 3, 50, 10, 10, 4
    logits = nr.planted_lines(rng, W, B, C, density=0.3, boost=3.0)
    il = np.array([W, 33, 64], np.int32)
    fe = model_mod.beam_frontend_call(ctx, None, 1, 0, None, logits, 0, B, W, C, k, False)
    lists = ctc.nbest_topk(ctx, fe["topk_idx"], fe["topk_logp"], C, n=n, beam=beam, len_bonus=5.8, input_lengths=il)
    host = ctc.nbest_logits(ctx, logits, 0, n=n, beam=beam, depth=k, len_bonus=5.8, input_lengths=il)
    _same(lists, host, "logits entry")
    assert (host.counts == n).all() and host.lengths[:, 0].min() > 0
    dev_t = torch.from_numpy(logits).cuda(0)
    torch.cuda.synchronize()
    _same(host, ctc.nbest_logits(ctx, dev_t, 1, n=n, beam=beam, depth=k, len_bonus=5.8, input_lengths=il), "device pointer")
    ctc.nbest_logits(ctx, rng.standard_normal((9, 1, 5)).astype(np.float32), 0, n=1, beam=32, depth=5)     # another layout
    _same(host, ctc.nbest_logits(ctx, logits, 0, n=n, beam=beam, depth=k, len_bonus=5.8, input_lengths=il), "repeated call")
    lib = pkg.load_library()
    vp = ctypes.c_void_p
    full = [getattr(host, f) for f in FIELDS]

    def call(kind, outs):
        ptrs = [None if a is None else a.ctypes.data_as(vp) for a in outs]
        tail = [k, beam, n, ctypes.c_double(5.8), il.ctypes.data_as(vp)] + ptrs
        if kind == "logits":
            return lib.hctr_nbest_logits(ctx, vp(dev_t.data_ptr()), 1, W, B, C, *tail)
        return lib.hctr_nbest_topk(ctx, fe["topk_idx"].ctypes.data_as(vp), fe["topk_logp"].ctypes.data_as(vp), W, B, C, *tail)

    for kind in ("logits", "topk"):
        assert call(kind, [None] * 5) == 0
        for i, f in enumerate(FIELDS):                     # every output alone (labels with lengths)
            outs = [None] * 5
            outs[i] = np.full(full[i].shape, 77, full[i].dtype)
            if f == "labels":
                outs[1] = np.full(full[1].shape, 77, full[1].dtype)
            assert call(kind, outs) == 0, (kind, f)
            assert outs[i].tobytes() == full[i].tobytes(), (kind, f)


def _images(synth, W=160):
    return synth.make_font_lines(3, W, 40 + W), np.array([W, W - 29, W - 50], np.int32)


def test_images(pkg, synth, ctc, m_trained):
    """hctr_nbest(images) == hctr_nbest_topk on hctr_beam_frontend's output for the same images and mode, bit for bit
    (the front end both use: fused head epilogues at this k; its log-probs need not equal row_topk's to the last bit,
    which is why the lists and not the stored logits are the cross-check), also with the batch split into internal
    passes; auto takes every line in f16x3 and leaves the guard figures alone; no top-k copy is part of the call"""
    C = synth.DEFAULT_VOCAB + 2
    imgs, widths = _images(synth)
    W = imgs.shape[-1]
    il = np.array([W, W - 20, W - 45], np.int32)
    kw = dict(n=5, beam=10, depth=10, len_bonus=5.8, widths=widths, input_lengths=il)
    by_mode = {}
    try:
        for mode in ("f16", "f16x3"):
            m_trained.set_precision(mode)
            res = m_trained.nbest(imgs, **kw)
            fe = m_trained.beam_frontend(imgs, 10, widths=widths)
            lists = ctc.nbest_topk(m_trained._ctx, fe["topk_idx"], fe["topk_logp"], C, n=5, beam=10, len_bonus=5.8,
                                   input_lengths=il)
            _same(res, lists, mode + " lists of the front end")
            assert (res.counts == 5).all() and res.lengths[:, 0].min() > 0
            for inp in (torch.from_numpy(imgs), torch.from_numpy(imgs).cuda(0)):
                _same(res, m_trained.nbest(inp, **kw), mode + " torch input")
            by_mode[mode] = res
            m_trained.set_profiling(True)
            m_trained.nbest(imgs, **kw)
            names = [nm for nm, _ in m_trained.last_profile()]
            m_trained.set_profiling(False)
            assert names[-2:] == ["prefix_beam", "prefix_backtrace"], names
    finally:
        m_trained.set_precision("auto")
        m_trained.set_profiling(False)
    m_trained.greedy(imgs, widths=widths)
    guard0 = m_trained.last_guard()
    auto = m_trained.nbest(imgs, **kw)
    guard1 = m_trained.last_guard()
    _same(by_mode["f16x3"], auto, "auto")
    assert guard0["lines"] == guard1["lines"] and guard0["flagged"] == guard1["flagged"]
    for f in ("flags", "min_margin", "scale"):
        np.testing.assert_array_equal(guard0[f], guard1[f])
    os.environ["HCTR_MAX_COLS"] = "600"                    # f16x3 passes of 200 columns: one line each
    try:
        small = pkg.hctr_model(C, precision="auto").cuda(0)
    finally:
        del os.environ["HCTR_MAX_COLS"]
    small.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    assert small.lines_per_pass(3, W, f16x3=True) < 3
    _same(auto, small.nbest(imgs, **kw), "split passes")


def test_one_best_is_the_host_search(pkg, ctc):
    """planted-peak lines, input_lengths = the reference's end step, len_bonus 5.8, 10/10: the 1-best equals
    hctr_beam_search(builtin_lm = 1) on the same front-end output, for every line"""
    rng = np.random.RandomState(8)
    W, B, C = 120, 6, 200
    logits = nr.planted_lines(rng, W, B, C, density=0.3, boost=5.0)
    logits[100:, 0, 1:] -= 20.0                            # a line whose text ends early: end step < W
    logits[100:, 0, 0] += 9.0
    chars = "".join(chr(nr.BASE + c) for c in range(1, C - 1))
    cd = pkg.ctc_codec(chars).cuda(0)
    cd.set_beam_search(ngram_path="zero", use_tfm_pred=False, len_bonus=5.8, beam_size=10, search_depth=10)
    fe = importlib.import_module(pkg.__name__ + ".model").beam_frontend_call(cd._context(), None, 1, 0, None, logits, 0,
                                                                           B, W, C, 10, False)
    want = cd.decode_frontend(fe)
    ref = ctc_ref.CtcCodecRef(chars)
    ends = []
    for b in range(B):
        top_line = ref._top_line(fe["topk_idx"][:, b, 0])
        assert top_line
        ends.append(ref._end_step(top_line, W))
    assert min(ends) < W
    got = ctc.nbest_topk(cd._context(), fe["topk_idx"], fe["topk_logp"], C, n=1, beam=10, len_bonus=5.8,
                         input_lengths=np.array(ends, np.int32))
    assert cd.labels_to_text([line[0] for line in got.label_lists()]) == want and all(want)
    res = cd.nbest(logits, n=3, beam=10, depth=10, len_bonus=5.8, input_lengths=ends)
    assert [t[0] for t in res.texts] == want and isinstance(res, pkg.NBest)
    assert cd.decode(logits) == want                       # decode is not rerouted


def test_argument_errors(pkg, ctx):
    lib = pkg.load_library()
    vp = ctypes.c_void_p
    W, B, C, k = 6, 2, 9, 3
    rng = np.random.RandomState(2)
    idx, lp = nr.topk_lists(rng.standard_normal((W, B, C)).astype(np.float32), k)
    labels, lengths = np.zeros((B, 2, W), np.int32), np.zeros((B, 2), np.int32)

    def call(idx=idx, lp=lp, W=W, B=B, C=C, k=k, beam=4, nbest=2, bonus=0.0, il=None, labels=labels, lengths=lengths):
        p = [None if a is None else a.ctypes.data_as(vp) for a in (idx, lp, il, labels, lengths)]
        return lib.hctr_nbest_topk(ctx, p[0], p[1], W, B, C, k, beam, nbest, ctypes.c_double(bonus), p[2], p[3], p[4],
                                   None, None, None)

    assert call() == 0
    dup = idx.copy()
    dup[3, 1, 2] = dup[3, 1, 0]
    big = idx.copy()
    big[0, 0, 1] = C
    bad = [dict(beam=33, nbest=2), dict(nbest=0), dict(nbest=5), dict(k=0), dict(k=C + 1), dict(C=1), dict(W=0),
           dict(idx=None), dict(lp=None), dict(lengths=None), dict(il=np.array([W, 0], np.int32)),
           dict(il=np.array([W + 1, 1], np.int32)), dict(bonus=float("nan")), dict(idx=dup), dict(idx=big)]
    for kw in bad:
        assert call(**kw) == ERR_ARG, kw
        assert lib.hctr_last_error(ctx), kw
    z = np.zeros((W, B, 40), np.float32)
    assert lib.hctr_nbest_logits(ctx, z.ctypes.data_as(vp), 0, W, B, 40, 33, 33, 1, ctypes.c_double(0.0), None, None, None,
                                 None, None, None) == ERR_ARG
    assert b"32" in lib.hctr_last_error(ctx)
    assert call(B=0, idx=None, lp=None) == 0               # a no-op
    assert call() == 0                                     # the context is still usable


def test_no_side_effects(pkg, synth, ctc, m_trained):
    rng = np.random.RandomState(12)
    W, B, C = 90, 3, 40
    logits = rng.standard_normal((W, B, C)).astype(np.float32)
    tl = np.array([7, 0, 25], np.int32)
    targets = rng.randint(1, C - 1, int(tl.sum())).astype(np.int32)
    imgs = synth.make_font_lines(3, 96, 31)
    ctx = m_trained._ctx

    def others():
        g = m_trained.greedy(imgs)
        guard = m_trained.last_guard()
        nll = ctc.loss_logits(ctx, logits, 0, targets, tl, None)
        nll2, grad = ctc.loss_grad_logits(ctx, logits, 0, targets, tl, None, None)
        al = ctc.align_logits(ctx, logits, 0, targets, tl, None)
        rec = ctc.recognize_logits(ctx, logits, 0)
        ev = ctc.evaluate_logits(ctx, logits, 0, targets, tl)
        fe = m_trained.beam_frontend(imgs, 10)
        return g, guard, (nll, nll2, grad, al.paths, al.scores, al.logps, rec.labels, rec.logps, rec.text_nll, ev.edits,
                          ev.counts, fe["topk_idx"], fe["topk_logp"], fe["blank_logp"])

    g0, guard0, arrays0 = others()
    ctc.nbest_logits(ctx, rng.standard_normal((200, 2, 300)).astype(np.float32), 0, n=32, beam=32, depth=32)
    res = m_trained.nbest(imgs)
    assert np.isfinite(res.logps[:, 0]).all()
    g1, guard1, arrays1 = others()
    for x, y in zip(g0, g1):
        np.testing.assert_array_equal(x, y)
    for i, (x, y) in enumerate(zip(arrays0, arrays1)):
        assert x.tobytes() == y.tobytes(), i
    assert guard0["lines"] == guard1["lines"] and guard0["flagged"] == guard1["flagged"]
    for f in ("flags", "min_margin", "scale"):
        np.testing.assert_array_equal(guard0[f], guard1[f])
