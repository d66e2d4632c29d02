"""GPU tests (-m gpu) of lexicon recognition (C ABI hctr_lexicon / hctr_lexicon_logits, ``LexiconRecognizer``,
``hctr_model.lexicon``, ``ctc_codec.lexicon``): the exact log p(entry | line) of every entry of a closed list by one
CTC forward pass over the lexicon's trie, the n best entries with ranks, and the lexicon's total mass.

The reference project has no counterpart; the yardstick is tests/lexicon_ref.py, a float64 restatement of the
definitions in include/hctr_hip.h that tests/test_lexicon_host.py checks against enumeration of all paths and against
torch's float64 ctc_loss. What must hold:
  * on planted lines (unit noise plus 12 on a planted path; T = 160, 130, 5, 1) the scores are within the loss tests'
    1e-5 relative + 1e-3 of float64 on the same logits with the same -inf pattern, the top-1 is the planted text, an
    exact duplicate ties bit for bit and comes second, top_entry is the stable ordering of the device's own ranks and
    log_total is the float64 logsumexp of those ranks to 2 * 5e-9 * max(1, |log_total|) (float64 summation of <= 2^20
    positive terms errs by at most N * 2^-53 = 1.2e-10 relative, plus a few ulps of exp / log, on either side);
  * every score has the bits of -nll of hctr_ctc_loss_logits with the entry as the line's target;
  * a pair's bits do not depend on unit_nodes, the class chunking, the entry order, the other entries, host or device
    pointers, repetition; priors shift ranks, order and log_total as defined and leave the scores' bits alone;
  * all-zero logits tie exactly, so the tie rule alone decides;
  * the image path equals the logits path on the engine's own f16x3 logits, bit for bit, across internal passes;
  * no lexicon call changes what the loss, the alignment, spotting or greedy decoding compute.
No entry of <= 64 labels can miss a 160-column line (64 + 63 repeats = 127), so the entry that needs 127 columns fits
the first two lines only; the -inf pattern is exercised on the lines of 5 and 1 columns.
"""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import lexicon_ref as ref

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-3                      # engine score vs float64 on the same logits (tests/test_gpu_ctc.py's)
FIELDS = ("entries", "logp", "rank", "log_total", "count", "scores")


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
          % (what, int(fin.sum()), float(err.max()), float(np.abs(want[fin]).max()), float((err - _tol(want[fin])).max())))
    assert (err <= _tol(want[fin])).all(), what


def _check_ranking(res, priors, what):
    """top_entry / top_rank / count / log_total against the device's own scores: rank = (double)score + (double)prior,
    the stable descending order, -inf left out; log_total within 2e of numpy's float64 logsumexp of those ranks"""
    n = res.entries.shape[1]
    for b in range(len(res)):
        top, tr, tot, cnt = ref.rank(res.scores[b], None if priors is None else np.asarray(priors, np.float32), n)
        np.testing.assert_array_equal(res.entries[b], top, err_msg="%s line %d" % (what, b))
        assert res.count[b] == cnt
        assert res.rank[b].tobytes() == tr.tobytes(), (what, b)
        live = top >= 0
        assert res.logp[b][live].tobytes() == res.scores[b][top[live]].tobytes() and np.isneginf(res.logp[b][~live]).all()
        if cnt == 0:
            assert res.log_total[b] == -np.inf
        else:
            e = 5e-9 * max(1.0, abs(tot))
            print("%s line %d: log_total %.12f, numpy %.12f, |d| %.2e (2e = %.2e)"
                  % (what, b, res.log_total[b], tot, abs(res.log_total[b] - tot), 2 * e))
            assert abs(res.log_total[b] - tot) <= 2 * e, (what, b)


def _same_bits(a, b, what, fields=FIELDS):
    for f in fields:
        assert np.ascontiguousarray(getattr(a, f)).tobytes() == np.ascontiguousarray(getattr(b, f)).tobytes(), (what, f)


@pytest.fixture(scope="module")
def ctc(pkg):
    return importlib.import_module(pkg.__name__ + ".ctc")


@pytest.fixture(scope="module")
def recognizer(pkg):
    return pkg.LexiconRecognizer().cuda(0)


@pytest.fixture(scope="module")
def m_trained(pkg, synth):
    C = synth.DEFAULT_VOCAB + 2
    m = pkg.hctr_model(C, precision="auto").cuda(0)
    m.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    return m


def plant(rng, W, C, text, T=None, margin=12.0, lead=2):
    """unit noise [W][C] plus `margin` on a path that reads `text` in columns [0, T): `lead` blanks, then per character
    a run of two columns and one blank (tests/test_gpu_spot.py's)"""
    T = W if T is None else T
    z = rng.standard_normal((W, C))
    path = [0] * lead + [c for ch in text for c in (ch, ch, 0)]
    path = (path + [0] * T)[:T]
    assert ref.collapse(path) == list(text)
    z[np.arange(T), path] += margin
    return z.astype(np.float32)


# ---- the planted case, shared (with its float64 results) by several tests ----
C0, W0, N_TOP = 60, 160, 6
TEXTS = [[5, 6, 5, 6, 5, 7, 7, 8, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 21, 23, 25, 27, 29, 31],
         [9, 10, 11, 12, 9, 10, 11, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36],
         [5],
         [6]]
LENGTHS = [W0, 130, 5, 1]
LEADS = [2, 2, 2, 0]
LONG64 = [1 + (7 * i) % 59 for i in range(64)]
SAME64 = [44] * 64                                           # needs 127 columns


def planted_entries():
    rng = np.random.RandomState(51)
    es = [list(t) for t in TEXTS]
    for t in TEXTS[:2]:
        es += [t[:k] for k in (1, 2, 3, len(t) // 2, len(t) - 1)]
        es += [t + [40], t + [t[-1]]]
    es += [[7], [7, 7], [7, 7, 7], LONG64, SAME64]
    es += [[11, 12] + [int(v) for v in rng.randint(1, C0, size=rng.randint(1, 7))] for _ in range(70)]
    while len(es) < 299:
        es.append([int(v) for v in rng.randint(1, C0, size=rng.randint(1, 10))])
    es.append(list(TEXTS[0]))                                # an exact duplicate of a planted text, at the highest index
    return es


@pytest.fixture(scope="module")
def planted_case(recognizer, ctc):
    rng = np.random.RandomState(50)
    logits = np.stack([plant(rng, W0, C0, t, T, lead=n) for t, T, n in zip(TEXTS, LENGTHS, LEADS)], axis=1)      # [W][B][C]
    il = np.array(LENGTHS, np.int32)
    es = planted_entries()
    want = ref.scores(logits, es, il)
    lex = ctc.Lexicon(es, num_classes=C0)
    got = recognizer(logits, lex, n=N_TOP, input_lengths=il, scores=True)
    return logits, il, es, want, lex, got


def test_planted_lines(planted_case):
    logits, il, es, want, lex, got = planted_case
    assert len(es) == 300 and lex.info()["units"] == 1
    unfit = np.array([[not ref.fits(e, T) for e in es] for T in LENGTHS])
    np.testing.assert_array_equal(np.isneginf(want), unfit)
    assert not unfit[0].any() and not unfit[1].any() and unfit[2].any() and unfit[3].sum() > 250
    _check_scores(got.scores, want, "planted scores")
    _check_ranking(got, None, "planted")
    dup = len(es) - 1
    for b in range(4):
        order = np.argsort(-want[b], kind="stable")
        first = [e for e in order if es[e] != es[order[0]]][0]
        gap = want[b][order[0]] - want[b][first]
        print("line %d: top-1 %r, float64 gap to the runner-up %.2f nats" % (b, es[order[0]][:8], gap))
        assert es[order[0]] == TEXTS[b] and gap > 1.0         # (float32 errs by <= 3.4e-4)
        assert es[got.entries[b, 0]] == TEXTS[b] and got.best()[b] == TEXTS[b]
    assert got.entries[0, 0] == 0 and got.entries[0, 1] == dup          # the duplicate ties bit for bit and comes second
    assert got.scores[:, 0].tobytes() == got.scores[:, dup].tobytes()
    assert got.count.tolist() == [N_TOP, N_TOP, N_TOP, min(N_TOP, int((~unfit[3]).sum()))]
    post = got.posteriors()
    assert post[1, 0] > 0.9 and post[0, 0] == post[0, 1] and 0.45 < post[0, 0] <= 0.5


def test_bit_equality_with_the_loss(planted_case, recognizer, ctc):
    logits, il, es, _, _, got = planted_case
    ctx = recognizer._context()
    N = len(es)
    tg = np.array([c for e in es for c in e], np.int32)
    tl = np.array([len(e) for e in es], np.int32)
    for b in range(4):
        x = np.ascontiguousarray(np.repeat(logits[:, b:b + 1], N, axis=1))
        nll = ctc.loss_logits(ctx, x, 0, tg, tl, np.full(N, il[b], np.int32))
        assert np.asarray(-nll, np.float32).tobytes() == got.scores[b].tobytes(), b
        assert np.isposinf(nll).sum() == np.isneginf(got.scores[b]).sum()


def test_bit_identity(planted_case, recognizer, ctc, pkg):
    logits, il, es, _, lex, base = planted_case
    call = lambda x, l, le=il: recognizer(x, l, n=N_TOP, input_lengths=le, scores=True)
    _same_bits(base, call(logits, lex), "repeated call")
    _same_bits(base, call(torch.from_numpy(logits).cuda(0), lex, torch.from_numpy(il)), "device pointer")
    small = ctc.Lexicon(es, num_classes=C0, unit_nodes=128)
    assert small.info()["units"] > 3
    _same_bits(base, call(logits, small), "unit_nodes = 128")
    lib = pkg.load_library()
    os.environ["HCTR_LEX_CLASSES"] = "4"
    try:
        assert lib.hctr_lexicon_chunk_classes(4, W0) == 4
        _same_bits(base, call(logits, small), "chunks of 4 classes, units of 128 nodes")
        _same_bits(base, call(logits, lex), "chunks of 4 classes")
    finally:
        del os.environ["HCTR_LEX_CLASSES"]
    assert lib.hctr_lexicon_chunk_classes(4, W0) > 60
    perm = np.random.RandomState(52).permutation(len(es))
    shuffled = call(logits, ctc.Lexicon([es[k] for k in perm], num_classes=C0, unit_nodes=128))
    assert shuffled.scores.tobytes() == np.ascontiguousarray(base.scores[:, perm]).tobytes()
    assert shuffled.log_total.shape == base.log_total.shape
    sub = [0, 3, 17, 40, 41, 42, 150, 299]
    part = call(logits, ctc.Lexicon([es[k] for k in sub], num_classes=C0))
    assert part.scores.tobytes() == np.ascontiguousarray(base.scores[:, sub]).tobytes()
    alone = call(logits, ctc.Lexicon([es[120]], num_classes=C0))
    assert alone.scores.tobytes() == np.ascontiguousarray(base.scores[:, [120]]).tobytes()


def test_priors(planted_case, recognizer, ctc):
    logits, il, es, _, _, base = planted_case
    rng = np.random.RandomState(53)
    pr = (rng.standard_normal(len(es)) * 3.0).astype(np.float32)
    pr[0] = -30.0                                              # the planted text of line 0 loses to its duplicate
    got = recognizer(logits, ctc.Lexicon(es, num_classes=C0, priors=pr), n=N_TOP, input_lengths=il, scores=True)
    assert got.scores.tobytes() == base.scores.tobytes()
    _check_ranking(got, pr, "priors")
    assert got.entries[0, 0] == len(es) - 1 and 0 not in got.entries[0, :2].tolist()
    assert not np.array_equal(got.entries, base.entries) and not np.array_equal(got.log_total, base.log_total)


def test_flat_random_logits(recognizer, ctc):
    rng = np.random.RandomState(54)
    W, B = 80, 3
    logits = rng.standard_normal((W, B, C0)).astype(np.float32)
    il = np.array([W, 57, 9], np.int32)
    es = planted_entries()
    want = ref.scores(logits, es, il)
    got = recognizer(logits, ctc.Lexicon(es, num_classes=C0, unit_nodes=128), n=32, input_lengths=il, scores=True)
    _check_scores(got.scores, want, "flat scores")
    _check_ranking(got, None, "flat")
    assert np.isneginf(want[0]).any() and (got.count == 32).all()


def test_tie_rule(recognizer, ctc):
    """all-zero logits: every entry of one length and repeat count has the same float32 score, the rule alone decides"""
    W, C = 12, 5
    logits = np.zeros((W, 2, C), np.float32)
    il = np.array([W, 3], np.int32)
    es = [[3], [1, 2], [4], [1], [2, 2], [2, 1], [1, 1], [2], [4, 3], [1, 2, 3], [3, 2, 1], [1, 1, 1], [4, 4, 4, 4, 4, 4, 4]]
    got = recognizer(logits, ctc.Lexicon(es, num_classes=C), n=32, input_lengths=il, scores=True)
    _check_scores(got.scores, ref.scores(logits, es, il), "tie scores")
    _check_ranking(got, None, "tie")
    kind = lambda e: (len(e), sum(a == b for a, b in zip(e, e[1:])))
    for b in range(2):
        for i, a in enumerate(es):
            for j, c in enumerate(es):
                if kind(a) == kind(c):
                    assert got.scores[b, i].tobytes() == got.scores[b, j].tobytes(), (a, c)
        top = [int(e) for e in got.entries[b] if e >= 0]
        for x, y in zip(top, top[1:]):                         # equal scores: the lower index first
            assert got.scores[b, x] > got.scores[b, y] or (got.scores[b, x] == got.scores[b, y] and x < y)
    fit = [sum(ref.fits(e, T) for e in es) for T in il]
    assert fit == [12, 11] and got.count.tolist() == fit
    assert (got.entries[1, 11:] == -1).all() and np.isneginf(got.rank[1, 11:]).all() and np.isneginf(got.logp[1, 11:]).all()
    singles = [e for e in got.entries[0].tolist() if len(es[e]) == 1]
    assert singles == [0, 2, 3, 7]


def test_image_path_equals_logits_path(pkg, synth, m_trained, ctc):
    """hctr_lexicon(images) == hctr_lexicon_logits(hctr_forward_logits(images) in f16x3), also with the batch split into
    internal passes (a second context with a small pass size); a line's own greedy text wins"""
    C, W = synth.DEFAULT_VOCAB + 2, 160
    imgs = synth.make_font_lines(3, W, 40 + W)
    widths = np.array([W, W - 29, W - 50], np.int32)
    labels = m_trained.greedy(imgs, widths=widths)
    assert all(len(v) >= 1 for v in labels)
    rng = np.random.RandomState(55)
    es = [[int(c) for c in v] for v in labels] + [[int(c) for c in labels[0][:1]], [C - 2, C - 3]]
    es += [[int(v) for v in rng.randint(1, C, size=rng.randint(1, 6))] for _ in range(200)]
    lex = ctc.Lexicon(es, num_classes=C, unit_nodes=128)
    fused = m_trained.lexicon(imgs, lex, n=4, widths=widths, scores=True)
    m_trained.set_precision("f16x3")
    try:
        logits = m_trained(torch.from_numpy(imgs).cuda(0), widths=widths)
    finally:
        m_trained.set_precision("auto")
    unfused = pkg.LexiconRecognizer().attach(m_trained)(logits, lex, n=4, scores=True)
    os.environ["HCTR_MAX_COLS"] = "600"                    # f16x3 passes of 200 columns: one or two lines each
    try:
        small = pkg.hctr_model(C, precision="auto").cuda(0)
    finally:
        del os.environ["HCTR_MAX_COLS"]
    small.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    assert small.lines_per_pass(3, W, f16x3=True) < 3
    split = small.lexicon(imgs, lex, n=4, widths=widths, scores=True)
    _same_bits(fused, unfused, "logits path")
    _same_bits(fused, split, "split passes")
    assert not np.isnan(fused.scores).any() and np.isfinite(fused.log_total).all()
    for b in range(3):
        assert es[fused.entries[b, 0]] == es[b], b
    # strings through a codec
    codec = pkg.ctc_codec(synth.characters()).attach(m_trained)
    texts = codec.labels_to_text([np.array(e) for e in es[:5]])
    by_text = ctc.Lexicon(texts, codec=codec)
    best, res = codec.lexicon(logits, by_text, n=2, scores=True)
    assert res.scores.tobytes() == np.ascontiguousarray(fused.scores[:, :5]).tobytes()
    assert best == texts[:3] and res.best() == texts[:3]
    assert [r[0][1] for r in res.lines()] == texts[:3]


def test_workload_shape(recognizer, ctc):
    """the flagship's logits shape: C = 7358, W = 2000; 5000 entries of 2-6 labels, half of them cut from the lines"""
    rng = np.random.RandomState(56)
    C, W, B, N = 7358, 2000, 2, 5000
    texts = [[int(v) for v in rng.randint(1, C, size=400)], [int(v) for v in rng.randint(1, C, size=300)]]
    logits = np.stack([plant(rng, W, C, texts[0]), plant(rng, W, C, texts[1], T=1500)], axis=1)
    il = np.array([W, 1500], np.int32)
    es = []
    for k in range(N // 2):
        t = texts[k % 2]
        at, n = int(rng.randint(0, len(t) - 6)), int(rng.randint(2, 7))
        es.append(t[at:at + n])
    es += [[int(v) for v in rng.randint(1, C, size=rng.randint(2, 7))] for _ in range(N - len(es))]
    lex = ctc.Lexicon(es, num_classes=C)
    info = lex.info()
    print("workload lexicon:", info)
    assert 10000 <= info["nodes"] <= 20000 and info["units"] >= 3
    want = ref.scores(logits, es, il)
    got = recognizer(torch.from_numpy(logits).cuda(0), lex, n=5, input_lengths=il, scores=True)
    _check_scores(got.scores, want, "workload scores")
    _check_ranking(got, None, "workload")


def test_argument_errors(recognizer, ctc, pkg):
    lib, ctx = pkg.load_library(), recognizer._context()
    vp = ctypes.c_void_p
    W, B, C = 8, 2, 6
    x = np.zeros((W, B, C), np.float32)
    lex, other = ctc.Lexicon([[1, 2], [3]], num_classes=C), ctc.Lexicon([[1]], num_classes=C + 1)
    top = np.zeros((B, 2), np.int32)

    def call(lx, n=2, il=None, logits=x):
        return lib.hctr_lexicon_logits(ctx, None if lx is None else lx._h, None if logits is None else logits.ctypes.data_as(vp),
                                       0, W, B, C, None if il is None else np.array(il, np.int32).ctypes.data_as(vp), n,
                                       top.ctypes.data_as(vp), None, None, None, None, None)

    assert call(lex) == 0 and top.tolist() == [[0, 1], [0, 1]]         # (more paths read two characters than one)
    assert call(None) == -1 and b"lex" in lib.hctr_last_error(ctx)
    assert call(other) == -1 and b"classes" in lib.hctr_last_error(ctx)
    assert call(lex, n=0) == -1 and call(lex, n=33) == -1 and b"outside [1,32]" in lib.hctr_last_error(ctx)
    assert call(lex, il=[0, 8]) == -1 and call(lex, il=[8, 9]) == -1
    assert call(lex, logits=None) == -1
    for kw in (dict(n=0), dict(n=33), dict(input_lengths=[0, 8]), dict(input_lengths=[8, 9]), dict(input_lengths=[8])):
        with pytest.raises(ValueError):
            recognizer(x, lex, **kw)
    with pytest.raises(ValueError):
        recognizer(x, other)
    with pytest.raises(ValueError):
        recognizer(x, "not a lexicon")
    empty = recognizer(np.zeros((W, 0, C), np.float32), lex, n=3, scores=True)
    assert empty.entries.shape == (0, 3) and empty.scores.shape == (0, 2) and empty.best() == []
    ok = recognizer(x, lex, n=3, input_lengths=[1, 8], scores=True)      # the context is still usable
    assert ok.count.tolist() == [1, 2] and ok.entries[0].tolist() == [1, -1, -1] and np.isneginf(ok.scores[0, 0])


def test_no_side_effects(pkg, ctc, synth, m_trained):
    rng = np.random.RandomState(57)
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
        sp = ctc.spot_logits(ctx, logits, 0, [[1, 2], [3]], None)
        return g, nll, al, sp

    g0, nll0, al0, sp0 = others()
    guard0 = m_trained.last_guard()
    es = [[int(v) for v in rng.randint(1, C, size=rng.randint(1, 8))] for _ in range(50)]
    ctc.lexicon_logits(ctx, logits, 0, ctc.Lexicon(es, num_classes=C), 5, None, True)     # another scratch layout in between
    big = ctc.Lexicon([list(g0[0][:2]) if len(g0[0]) >= 2 else [1], [5]], num_classes=synth.DEFAULT_VOCAB + 2)
    res = m_trained.lexicon(imgs, big, n=2)
    guard1 = m_trained.last_guard()
    assert guard0["lines"] == guard1["lines"] and guard0["flagged"] == guard1["flagged"]
    assert not np.isnan(res.logp).any() and res.scores is None
    g1, nll1, al1, sp1 = others()
    for x, y in zip(g0, g1):
        np.testing.assert_array_equal(x, y)
    assert nll0.tobytes() == nll1.tobytes()
    for k in ("paths", "starts", "ends", "logps", "scores"):
        assert getattr(al0, k).tobytes() == getattr(al1, k).tobytes(), k
    for k in ("logp", "seg_logp", "starts", "ends"):
        assert getattr(sp0, k).tobytes() == getattr(sp1, k).tobytes(), k
