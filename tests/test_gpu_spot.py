"""GPU tests (-m gpu) of keyword spotting (C ABI hctr_spot / hctr_spot_logits, ``KeywordSpotter``, ``hctr_model.spot``,
``ctc_codec.spot``): per (line, query) the posterior probability that the line's text contains the query, and the best
tight segment that reads it.

The reference project has no counterpart; the yardstick is tests/spot_ref.py, a float64 restatement of the definitions
in include/hctr_hip.h that tests/test_spot_host.py checks against enumeration of all paths. What must hold:
  * on planted lines (unit noise plus 12 on a planted path; T < W, T = 1 and T = 0 among them) contain_logp and seg_logp
    are within the loss tests' 1e-5 relative + 1e-3 of float64 on the same logits, and the spans are EQUAL;
  * on flat random logits, where near-ties may resolve differently in float32, the reported segment is a valid one whose
    float64 score is the reported one and the float64 optimum, both within the rule;
  * all-zero logits tie everything exactly, so the documented tie rule alone decides the spans;
  * contain_logp >= seg_logp and contain_logp >= -nll of the loss with the query as target, on the device's own figures;
  * a pair's bits do not depend on the other queries, their order, the chunking, host or device pointers, repetition;
  * the image path equals spotting the engine's own f16x3 logits, bit for bit, across internal passes;
  * a result below float64's floor is -inf, never NaN and never a large number;
  * no spot call changes what the loss, the alignment or greedy decoding compute.
"""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import spot_ref as ref

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-3                      # engine score vs float64 on the same logits (tests/test_gpu_ctc.py's)
FLOOR = -600.0                               # every asserted log P of the oracle stays above it, bar the floor case
FIELDS = ("logp", "seg_logp", "starts", "ends")


def _tol(want):
    return RTOL * np.abs(want) + ATOL


def _check_scores(got, want, what):
    """got within the rule of want where want is finite, -inf exactly where want is"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert not np.isnan(got).any(), what
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isneginf(got), ~fin, err_msg="%s: -inf pattern" % what)
    err = np.abs(got[fin] - want[fin])
    print("%s: %d finite, max |d| %.3e (largest |want| %.1f), worst excess over the rule %.3e"
          % (what, int(fin.sum()), float(err.max()) if err.size else 0.0, float(np.abs(want[fin]).max()) if err.size else 0.0,
             float((err - _tol(want[fin])).max()) if err.size else 0.0))
    assert (err <= _tol(want[fin])).all(), what


def _same_bits(a, b, what, cols=None):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if cols is not None:
            x = x[:, cols]
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), (what, f)


@pytest.fixture(scope="module")
def ctc(pkg):
    return importlib.import_module(pkg.__name__ + ".ctc")


@pytest.fixture(scope="module")
def spotter(pkg):
    return pkg.KeywordSpotter().cuda(0)


@pytest.fixture(scope="module")
def m_trained(pkg, synth):
    C = synth.DEFAULT_VOCAB + 2
    m = pkg.hctr_model(C, precision="auto").cuda(0)
    m.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    return m


def plant(rng, W, C, text, T=None, margin=12.0, lead=2):
    """unit noise [W][C] plus `margin` on a path that reads `text` in columns [0, T): `lead` blanks, then per character
    a run of two columns and one blank"""
    T = W if T is None else T
    z = rng.standard_normal((W, C))
    path = [0] * lead + [c for ch in text for c in (ch, ch, 0)]
    path = (path + [0] * T)[:T]
    assert T < lead + 3 * len(text) or ref.collapse(path) == list(text)
    z[np.arange(T), path] += margin
    return z.astype(np.float32)


# ---- the planted case, shared (with its float64 results) by several tests ----
C0, W0 = 60, 160
Q32 = [21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 21, 23, 25, 27, 29, 31, 33, 35, 22, 24, 26, 28, 30, 32, 34, 36]
A32 = [41, 42, 43, 44, 45, 46, 47, 48, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 49, 50, 51, 52, 41, 43, 45, 47, 49, 51, 53, 54]
TEXTS = [[5, 6, 5, 6, 5, 7, 7, 8] + Q32,                  # ababa, a doubled character, the 32-long query (and its 31 prefix)
         [9, 10, 11, 12, 9, 10, 11] + Q32[1:],             # a keyword twice; the 31-long suffix of Q32, not all of it
         [5],
         [6, 7]]
LENGTHS = [W0, 130, 1, 0]
LEADS = [2, 2, 0, 0]
READS = [TEXTS[0], TEXTS[1], [5], []]                     # what the columns that count hold


def planted_queries():
    rng = np.random.RandomState(21)
    qs = [[5], [59], [12], [5, 6], [6, 5], [57, 58], [7, 7], [5, 6, 5], [6, 5, 6], [7, 7, 8], [7, 7, 7], [9, 10, 11],
          [11, 12, 9], [5, 6, 5, 6, 5], [6, 5, 7, 7, 8], [14, 14, 15, 14, 14], [10, 11, 12, 9, 10], Q32, Q32[:31], Q32[1:],
          A32, A32[1:], [5, 6], Q32]                       # the last two: duplicates
    while len(qs) < 40:
        qs.append([int(v) for v in rng.randint(1, C0, size=rng.randint(2, 6))])
    return qs


@pytest.fixture(scope="module")
def planted_case(spotter):
    rng = np.random.RandomState(20)
    logits = np.stack([plant(rng, W0, C0, t, T, lead=n) for t, T, n in zip(TEXTS, LENGTHS, LEADS)], axis=1)      # [W][B][C]
    il = np.array(LENGTHS, np.int32)
    qs = planted_queries()
    want = ref.spot(logits, qs, il)
    got = spotter(logits, qs, il)
    return logits, il, qs, want, got


def test_planted_lines(planted_case):
    logits, il, qs, (contain, seg, st, en), got = planted_case
    assert sorted({len(q) for q in qs} & {1, 2, 3, 5, 31, 32}) == [1, 2, 3, 5, 31, 32]
    assert (contain[np.isfinite(contain)] > FLOOR).all() and (seg[np.isfinite(seg)] > FLOOR).all()
    present = contain > np.log(0.5)                       # what the planted texts hold, and nothing else
    for b, text in enumerate(READS):
        for k, q in enumerate(qs):
            assert bool(present[b, k]) == ref._contains(list(text), list(q)), (b, q)
    assert present[0, qs.index(Q32)] and not present[1, qs.index(Q32)] and present[1, qs.index(Q32[1:])]
    assert np.isneginf(contain[3]).all() and (st[3] == -1).all()          # T = 0
    assert np.isfinite(contain[2, 0]) and np.isneginf(contain[2, 3])      # T = 1: one character fits, two do not
    _check_scores(got.logp, contain, "contain_logp")
    _check_scores(got.seg_logp, seg, "seg_logp")
    np.testing.assert_array_equal(got.starts, st)
    np.testing.assert_array_equal(got.ends, en)
    # 'aba' in 'ababa' (runs at columns 2-3, 5-6, 8-9, 11-12, 14-15): one of the two occurrences, tight
    k = qs.index([5, 6, 5])
    assert (got.starts[0, k], got.ends[0, k]) in ((3, 9), (9, 15))


def test_invariants_on_the_device(planted_case, spotter, ctc):
    """contain >= seg and contain >= -nll(q as the target), from the engine's own entries"""
    logits, il, qs, _, got = planted_case
    ctx = spotter._context()
    live = il >= 1
    x = np.ascontiguousarray(logits[:, live])
    slack = lambda v: RTOL * np.abs(v) + ATOL
    fin = np.isfinite(got.seg_logp)
    assert (got.logp[fin] >= got.seg_logp[fin] - slack(got.seg_logp[fin])).all()
    assert np.isfinite(got.logp[fin]).all()
    for k, q in enumerate(qs):
        n = int(live.sum())
        nll = ctc.loss_logits(ctx, x, 0, np.tile(np.array(q, np.int32), n), np.full(n, len(q), np.int32), il[live])
        lo = -nll.astype(np.float64)
        ok = np.isfinite(lo)
        assert (got.logp[live, k][ok] >= lo[ok] - slack(lo[ok])).all(), (q, got.logp[live, k], lo)


def test_line_planted_with_exactly_the_query(spotter, ctc):
    """then containing q and reading exactly q are nearly the same event: the float64 gap is small, and the device
    figures reproduce it"""
    rng = np.random.RandomState(5)
    q, W = [3, 4, 4, 9, 3], 40
    logits = plant(rng, W, C0, q)[:, None, :]
    lp = torch.from_numpy(ref.log_softmax(logits))
    nll64 = float(torch.nn.functional.ctc_loss(lp, torch.tensor([q]), torch.tensor([W]), torch.tensor([len(q)]),
                                               blank=0, reduction="none")[0])
    c64 = ref.contain_logp(lp[:, 0].numpy(), q)
    assert 0.0 <= c64 + nll64 < 0.1, (c64, nll64)
    got = spotter(logits, [q])
    nll = ctc.loss_logits(spotter._context(), logits, 0, np.array(q, np.int32), np.array([len(q)], np.int32), None)
    _check_scores(got.logp, [[c64]], "contain of the exact line")
    gap = float(got.logp[0, 0]) + float(nll[0])
    print("contain %.6f, -nll %.6f, gap %.6f (float64 %.6f)" % (got.logp[0, 0], -nll[0], gap, c64 + nll64))
    slack = _tol(c64) + _tol(nll64)
    assert -slack <= gap <= c64 + nll64 + slack


def test_flat_random_logits(spotter):
    rng = np.random.RandomState(8)
    W, B = 80, 3
    logits = rng.standard_normal((W, B, C0)).astype(np.float32)
    il = np.array([W, 57, 80], np.int32)
    qs = [[4], [4, 4], [7, 9], [1, 2, 1], [3, 3, 3], [5, 9, 5, 9, 5], Q32[:31], Q32]
    qs += [[int(v) for v in rng.randint(1, C0, size=n)] for n in (2, 3, 5, 5)]
    contain, seg, _, _ = ref.spot(logits, qs, il)
    assert (contain > FLOOR).all() and (seg > FLOOR).all()
    got = spotter(logits, qs, il)
    _check_scores(got.logp, contain, "flat contain_logp")
    _check_scores(got.seg_logp, seg, "flat seg_logp (vs the float64 optimum)")
    for b in range(B):
        lp = ref.log_softmax(logits[:il[b], b])
        for k, q in enumerate(qs):
            s, e = int(got.starts[b, k]), int(got.ends[b, k])
            assert 0 <= s < e <= il[b], (b, q, s, e)
            own = ref.segment_score(lp, q, s, e)           # -inf if the window admits no segment path
            assert np.isfinite(own), (b, q, s, e)
            assert abs(own - float(got.seg_logp[b, k])) <= _tol(own), (b, q, own, got.seg_logp[b, k])
            assert abs(own - seg[b, k]) <= _tol(seg[b, k]), (b, q, own, seg[b, k])


def test_tie_rule(spotter):
    """all-zero logits: every path of a length has the same float32 score, the documented rule alone decides"""
    W, C = 12, 5
    logits = np.zeros((W, 2, C), np.float32)
    il = np.array([W, 4], np.int32)
    qs = [[1], [1, 2], [1, 1], [1, 2, 1], [2, 2, 2], [3, 3, 4, 4]]
    contain, seg, st, en = ref.spot(logits, qs, il)
    got = spotter(logits, qs, il)
    need = [1, 2, 3, 3, 5, 6]                              # L + repeats: the shortest segment, at the earliest end
    for k, n in enumerate(need):
        for b in range(2):
            fits = n <= il[b]
            assert (st[b, k], en[b, k]) == ((0, n) if fits else (-1, -1))
    np.testing.assert_array_equal(got.starts, st)
    np.testing.assert_array_equal(got.ends, en)
    _check_scores(got.seg_logp, seg, "tie seg_logp")
    _check_scores(got.logp, contain, "tie contain_logp")


def test_bit_identity(planted_case, spotter, pkg):
    logits, il, qs, _, base = planted_case
    _same_bits(base, spotter(logits, qs, il), "repeated call")
    rev = spotter(logits, qs[::-1], il)
    _same_bits(base, rev, "reversed queries", cols=list(range(len(qs)))[::-1])
    for k in (0, 3, 7, 13, 17, 18, 20, 22, 30):
        _same_bits(base, spotter(logits, [qs[k]], il), "query %d alone" % k, cols=[k])
    dev = spotter(torch.from_numpy(logits).cuda(0), qs, torch.from_numpy(il))
    _same_bits(base, dev, "device pointer")
    lib = pkg.load_library()
    os.environ["HCTR_SPOT_CLASSES"] = "4"
    try:
        assert lib.hctr_spot_chunk_classes(4, W0) == 4
        small = spotter(logits, qs, il)
    finally:
        del os.environ["HCTR_SPOT_CLASSES"]
    assert lib.hctr_spot_chunk_classes(4, W0) > 60
    _same_bits(base, small, "chunks of 4 classes")


def test_floor(spotter):
    """margin 40 and an absent 32-long query: the probability is below float64's range. The result is -inf or the
    oracle's, never NaN, never above the floor; the other pairs of the call keep the rule"""
    rng = np.random.RandomState(9)
    W = 120
    logits = plant(rng, W, C0, [5, 6, 5, 6, 5, 7, 7, 8], margin=40.0)[:, None, :]
    qs = [A32, [5, 6, 5], [7, 7]]
    contain, seg, st, en = ref.spot(logits, qs)
    assert not contain[0, 0] > 2 * FLOOR and contain[0, 1] > -1.0 and contain[0, 2] > -1.0
    got = spotter(logits, qs)
    v = float(got.logp[0, 0])
    print("floor case: engine %r, float64 %r" % (v, contain[0, 0]))
    assert not np.isnan(v) and v <= FLOOR
    assert np.isneginf(v) or (np.isfinite(contain[0, 0]) and abs(v - contain[0, 0]) <= _tol(contain[0, 0]))
    _check_scores(got.logp[:, 1:], contain[:, 1:], "floor case, present queries")
    _check_scores(got.seg_logp[:, 1:], seg[:, 1:], "floor case, present segments")
    # at this margin both occurrences of 'aba' score 0 to float32's last bit, so the span is checked as on flat logits
    lp = ref.log_softmax(logits[:, 0])
    for k in (1, 2):
        own = ref.segment_score(lp, qs[k], int(got.starts[0, k]), int(got.ends[0, k]))
        assert np.isfinite(own) and abs(own - seg[0, k]) <= _tol(seg[0, k]), (qs[k], own, seg[0, k])
    assert not np.isnan(got.seg_logp).any()


def test_workload_shape(spotter):
    """the flagship's logits shape: C = 7358, W = 2000"""
    rng = np.random.RandomState(10)
    C, W, B = 7358, 2000, 2
    text0 = [int(v) for v in rng.randint(1, C, size=400)]
    text1 = [int(v) for v in rng.randint(1, C, size=300)]
    logits = np.stack([plant(rng, W, C, text0), plant(rng, W, C, text1, T=1500)], axis=1)
    il = np.array([W, 1500], np.int32)
    qs = [text0[100:103], text1[200:202], text0[397:400], [text0[5]], text1[10:15], [7000, 7001], text0[50:52] + [6999],
          text0[300:304]]
    contain, seg, st, en = ref.spot(logits, qs, il)
    assert (contain > FLOOR).all() and (seg > FLOOR).all()
    got = spotter(torch.from_numpy(logits).cuda(0), qs, il)
    _check_scores(got.logp, contain, "workload contain_logp")
    _check_scores(got.seg_logp, seg, "workload seg_logp")
    np.testing.assert_array_equal(got.starts, st)
    np.testing.assert_array_equal(got.ends, en)


def test_argument_errors(spotter, pkg):
    lib, ctx = pkg.load_library(), spotter._context()
    vp = ctypes.c_void_p
    W, B, C = 8, 2, 6
    x = np.zeros((W, B, C), np.float32)
    out = np.zeros((B, 1), np.float32)                     # (the one call that succeeds with Q = 2 gets its own)

    def call(q, ql, Q, il=None, logits=x, out=out):
        q, ql = np.array(q, np.int32), np.array(ql, np.int32)
        return lib.hctr_spot_logits(ctx, None if logits is None else logits.ctypes.data_as(vp), 0, W, B, C,
                                    q.ctypes.data_as(vp), ql.ctypes.data_as(vp), Q,
                                    None if il is None else np.array(il, np.int32).ctypes.data_as(vp),
                                    out.ctypes.data_as(vp), None, None, None)

    assert call([1, 2, 3], [2, 1], 2, out=np.zeros((B, 2), np.float32)) == 0
    assert call([1, 2, 3], [2, 1], 0) == -1 and b"Q" in lib.hctr_last_error(ctx)
    assert call([1, 2, 3], [3, 0], 2) == -1
    assert call([1] * 33, [33], 1) == -1
    assert call([1, 6], [2], 1) == -1 and b"outside [1,5]" in lib.hctr_last_error(ctx)
    assert call([0], [1], 1) == -1
    assert call([1], [1], 1, il=[8, 9]) == -1
    assert call([1], [1], 1, il=[-1, 3]) == -1
    assert call([1], [1], 1, logits=None) == -1
    assert call([1], [1], 1, il=[0, 8]) == 0               # the context is still usable; T = 0 is a line like any other
    assert np.isneginf(out[0, 0]) and np.isfinite(out[1, 0])
    with pytest.raises(ValueError):
        spotter(x, [[1], list(range(1, 34))])
    with pytest.raises(ValueError):
        spotter(x, [[9]])
    empty = spotter(np.zeros((W, 0, C), np.float32), [[1]])
    assert empty.logp.shape == (0, 1) and empty.hits() == []


def test_no_side_effects(pkg, ctc, synth, m_trained):
    rng = np.random.RandomState(12)
    W, B, C = 90, 3, 40
    logits = rng.standard_normal((W, B, C)).astype(np.float32)
    targets = rng.randint(1, C, size=32).astype(np.int32)
    tl = np.array([7, 0, 25], np.int32)
    imgs = synth.make_font_lines(3, 96, 31)
    ctx = m_trained._ctx

    def others():
        g = m_trained.greedy(imgs)
        nll = ctc.loss_logits(ctx, logits, 0, targets, tl, None)
        al = ctc.align_logits(ctx, logits, 0, targets, tl, None)
        return g, nll, al

    g0, nll0, al0 = others()
    guard0 = m_trained.last_guard()
    ctc.spot_logits(ctx, logits, 0, [[1, 2], Q32, [3]], None)             # another scratch layout in between
    sp = m_trained.spot(imgs, [list(g0[0][:2]) if len(g0[0]) >= 2 else [1], [5]])
    guard1 = m_trained.last_guard()
    assert guard0["lines"] == guard1["lines"] and guard0["flagged"] == guard1["flagged"]
    assert not np.isnan(sp.logp).any()
    g1, nll1, al1 = others()
    for x, y in zip(g0, g1):
        np.testing.assert_array_equal(x, y)
    assert nll0.tobytes() == nll1.tobytes()
    for k in ("paths", "starts", "ends", "logps", "scores"):
        assert getattr(al0, k).tobytes() == getattr(al1, k).tobytes(), k


def test_image_path_equals_logits_path(pkg, synth, m_trained):
    """hctr_spot(images) == hctr_spot_logits(hctr_forward_logits(images) in f16x3), also with the batch split into
    internal passes (a second context with a small pass size); a line's own greedy text is found in it"""
    C, W = synth.DEFAULT_VOCAB + 2, 160
    imgs = synth.make_font_lines(3, W, 40 + W)
    widths = np.array([W, W - 29, W - 50], np.int32)
    labels = m_trained.greedy(imgs, widths=widths)
    assert all(len(v) >= 1 for v in labels)                 # (a line of this width reads two or three characters)
    qs = [[int(c) for c in labels[0][:2]], [int(c) for c in labels[1][-2:]], [int(c) for c in labels[2][:1]],
          [int(labels[0][0])], [C - 2, C - 3], [int(c) for c in labels[2][:32]]]
    fused = m_trained.spot(imgs, qs, widths=widths)
    m_trained.set_precision("f16x3")
    try:
        logits = m_trained(torch.from_numpy(imgs).cuda(0), widths=widths)
    finally:
        m_trained.set_precision("auto")
    unfused = pkg.KeywordSpotter().attach(m_trained)(logits, qs)
    os.environ["HCTR_MAX_COLS"] = "600"                    # f16x3 passes of 200 columns: one or two lines each
    try:
        small = pkg.hctr_model(C, precision="auto").cuda(0)
    finally:
        del os.environ["HCTR_MAX_COLS"]
    small.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    assert small.lines_per_pass(3, W, f16x3=True) < 3
    split = small.spot(imgs, qs, widths=widths)
    _same_bits(fused, unfused, "logits path")
    _same_bits(fused, split, "split passes")
    for b, k in ((0, 0), (1, 1), (2, 2), (0, 3), (2, 5)):        # a piece of the line's own text beats an absent pair
        assert fused.logp[b, k] > fused.logp[b, 4] and 0 <= fused.starts[b, k] < fused.ends[b, k] <= W, (b, k)
    assert len(fused.hits(0.0)) == 3 * len(qs) and not np.isnan(fused.logp).any()
    # strings through a codec: the same queries, and a character outside the vocabulary is refused
    codec = pkg.ctc_codec(synth.characters()).attach(m_trained)
    texts = codec.labels_to_text([np.array(q) for q in qs[:4]])
    by_text = m_trained.spot(imgs, texts, widths=widths, codec=codec)
    for f in FIELDS:
        assert getattr(by_text, f).tobytes() == np.ascontiguousarray(getattr(fused, f)[:, :4]).tobytes(), f
    by_codec = codec.spot(logits, texts)
    for f in FIELDS:
        assert getattr(by_codec, f).tobytes() == np.ascontiguousarray(getattr(fused, f)[:, :4]).tobytes(), f
    with pytest.raises(ValueError):
        codec.spot(logits, ["\u0001"])
