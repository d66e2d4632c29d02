"""GPU tests (-m gpu) of word-sequence recognition (C ABI hctr_words / hctr_words_logits, ``WordRecognizer``,
``hctr_model.words``, ``ctc_codec.words``): the best segmentation of a line into entries of a lexicon by token passing
over the looped trie.

The reference project has no counterpart; the yardstick is tests/words_ref.py, a float64 restatement of the definition
in include/hctr_hip.h that tests/test_words_host.py checks against a brute force over all paths and segmentations.
What must hold:
  * ``score`` is within the loss tests' 1e-5 relative + 1e-3 of the yardstick on the same logits, -inf where it is;
  * the segmentation: equal-score segmentations are structural (``ab`` + ``c`` against ``a`` + ``bc`` under zero
    priors), so the words are compared with the yardstick's only on planted lines whose spellings make the optimum
    unique; everywhere the sandwich holds: the float64 score of the returned words with the returned starts (blanks
    before the first start, every word first emitted at its start, plus the weights) can never exceed the optimum and
    must reach it within the same rule, so a wrong word or boundary fails;
  * ``labels`` is the concatenation of the returned entries, ``count`` their number, ``text_nll`` has the bits of
    hctr_ctc_loss_logits on that text;
  * every output's bits do not depend on the storage form (LDS or scratch), host or device pointers, repetition, the
    grouping of lines, the other lines of the batch or the internal passes of the image path; the score's bits do not
    depend on the order of the entries;
  * masked and non-finite logits do what include/hctr_hip.h says; no words call changes what other calls compute.
Shapes: C = 12 and 60, lines of 160, 40, 5, 2 and 1 columns; tries below 1024, 2048 and 4096 nodes (one, two and four
nodes per thread of the LDS form) and one of 6 - 8 thousand (C = 200, the scratch form).
"""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import pattern_ref
import words_ref as ref

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-3                      # engine score vs float64 on the same logits (tests/test_gpu_ctc.py's)
FIELDS = ("score", "count", "words", "starts", "labels", "lengths", "text_nll")
W0 = 160
LENGTHS = [W0, 40, 5, 2, 1]
CHARS = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUV"       # labels 1..58


def _tol(want):
    return RTOL * np.abs(want) + ATOL


def _same_bits(a, b, what, fields=FIELDS):
    for f in fields:
        assert np.ascontiguousarray(getattr(a, f)).tobytes() == np.ascontiguousarray(getattr(b, f)).tobytes(), (what, f)


@pytest.fixture(scope="module")
def ctc(pkg):
    return importlib.import_module(pkg.__name__ + ".ctc")


@pytest.fixture(scope="module")
def recognizer(pkg):
    return pkg.WordRecognizer().cuda(0)


@pytest.fixture(scope="module")
def m_trained(pkg, synth):
    C = synth.DEFAULT_VOCAB + 2
    m = pkg.hctr_model(C, precision="auto").cuda(0)
    m.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    return m


def plant(rng, W, C, text, T=None, margin=12.0, lead=2):
    """unit noise [W][C] plus `margin` on a path that reads `text` in columns [0, T): `lead` blanks, then per character
    a run of two columns and one blank (tests/test_gpu_lexicon.py's)"""
    T = W if T is None else T
    z = rng.standard_normal((W, C))
    path = [0] * lead + [c for ch in text for c in (ch, ch, 0)]
    path = (path + [0] * T)[:T]
    z[np.arange(T), path] += margin
    return z.astype(np.float32)


def weight(pr, bonus, e):
    p = 0.0 if pr is None else np.float64(np.float32(pr[e]))
    return float(np.float32(p + np.float64(np.float32(bonus))))


def check(res, logits, il, es, pr, bonus, want, what):
    """every line of res against the yardstick's (score, words, starts) in `want`: the score rule, the -inf pattern,
    labels / count / lengths against the returned words, and the sandwich"""
    assert not np.isnan(res.score).any(), what
    for b in range(len(res)):
        T, w = int(il[b]), want[b][0]
        n = int(res.count[b])
        words, starts = res.words[b, :n].tolist(), res.starts[b, :n].tolist()
        assert (res.words[b, n:] == -1).all() and (res.starts[b, n:] == -1).all()
        if w == -np.inf:
            assert n == 0 and res.score[b] == -np.inf and res.lengths[b] == 0 and res.text_nll[b] == np.inf, (what, b)
            continue
        err = abs(float(res.score[b]) - w)
        lp = ref.log_softmax(logits[:T, b])
        seg = ref.segmentation_score(lp, [es[e] for e in words], [weight(pr, bonus, e) for e in words], starts, T)
        print("%s line %d (T=%d): score %.5f yardstick %.5f |d| %.2e, sandwich %.5f gap %.2e, rule %.2e, %d words"
              % (what, b, T, res.score[b], w, err, seg, w - seg, _tol(w), n))
        assert err <= _tol(w), (what, b)
        assert n >= 1 and all(0 <= e < len(es) for e in words) and starts == sorted(set(starts)) and starts[0] >= 0 \
            and starts[-1] < T, (what, b)
        text = [c for e in words for c in es[e]]
        assert res.lengths[b] == len(text) and res.labels[b, :len(text)].tolist() == text, (what, b)
        assert (res.labels[b, len(text):] == 0).all()
        assert seg <= w + 1e-9 * max(1.0, abs(w)), (what, b)            # (a fault of the test's, were it to fail)
        assert w - seg <= _tol(w), (what, b)


def text_nll_bits(ctc, ctx, res, logits, il, what):
    have = res.count > 0
    tl = np.where(have, res.lengths, 0).astype(np.int32)
    tg = np.concatenate([res.labels[b, :tl[b]] for b in range(len(res))]).astype(np.int32)
    nll = ctc.loss_logits(ctx, logits, 0, tg, tl, il)
    assert have.any() and res.text_nll[have].tobytes() == nll[have].tobytes(), what
    assert np.isposinf(res.text_nll[~have]).all(), what
    assert (res.posterior()[~have] == 0).all() and (res.posterior()[have] > 0).all()


def random_entries(rng, C, n, lo=1, hi=4):
    return [[int(v) for v in rng.randint(1, C, size=rng.randint(lo, hi + 1))] for _ in range(n)]


def grown(seed, C, lo, hi, step):
    """random entries of 1 - 4 labels whose trie has between lo and hi nodes"""
    rng = np.random.RandomState(seed)
    es = []
    while True:
        es += random_entries(rng, C, step)
        nn = len(ref.build_trie(es)[0])
        if nn >= lo:
            assert nn < hi, nn
            return es


# name -> (C, entries, priors, word_bonus)
def lexica():
    rng = np.random.RandomState(900)
    out = {
        "prefixes": (12, [[1], [1, 2], [1, 2, 2]], [-0.3, -1.0, 0.4], -0.7),
        "boundary": (12, [[1], [1, 2], [2, 1], [3, 3]], None, 0.0),
        "ambiguous": (12, [[1, 2], [3], [1], [2, 3]], None, 0.0),
        "duplicates": (12, [[1, 2], [3], [1, 2], [3], [3, 3]], [-2.0, -0.5, -1.0, -0.25, -3.0], 0.5),
        "short": (12, [[1, 1, 2], [2, 2, 1, 1]], None, 0.25),              # no word fits fewer than four columns
        "masked": (12, [[1, 2], [3], [1], [2, 3]], None, 0.0),             # masks that remove every segmentation
        "npt1": (60, grown(901, 60, 600, 1024, 50), None, -1.0),
        "npt2": (60, grown(902, 60, 1100, 2048, 50), "random", 0.0),
        "npt4": (60, grown(903, 60, 2200, 4096, 100), "random", -0.5),
        "scratch": (200, grown(904, 200, 6000, 8000, 200), "random", -0.25),
    }
    for k, (C, es, pr, bonus) in out.items():
        if isinstance(pr, str):
            out[k] = (C, es, (rng.randn(len(es)) * 0.5).astype(np.float32), bonus)
    return out


LEXICA = lexica()


def batch(seed, C, es):
    """five lines of 160, 40, 5, 2 and 1 columns: a planted sequence of entries, plain noise, and short planted words"""
    rng = np.random.RandomState(seed)
    one = [e for e in es if len(e) == 1][0]
    seq = [c for k in rng.randint(0, len(es), size=12) for c in es[k]][:50]
    lines = [plant(rng, W0, C, seq), (rng.standard_normal((W0, C)) * 3.0).astype(np.float32),
             plant(rng, W0, C, es[0][:1], T=5, lead=1), plant(rng, W0, C, one, T=2, lead=0),
             plant(rng, W0, C, one, T=1, lead=0)]
    return np.stack(lines, axis=1), np.array(LENGTHS, np.int32)


def batch_short(seed, C, es):
    """lines of 160, 40, 3, 2 and 1 columns: the last three are too short for any word (score -inf, count 0)"""
    rng = np.random.RandomState(seed)
    lines = [plant(rng, W0, C, es[0] + es[1] + es[0]), (rng.standard_normal((W0, C)) * 3.0).astype(np.float32),
             plant(rng, W0, C, [1], T=3, lead=0), plant(rng, W0, C, [2], T=2, lead=0), plant(rng, W0, C, [1], T=1, lead=0)]
    return np.stack(lines, axis=1), np.array([W0, 40, 3, 2, 1], np.int32)


def batch_masked(seed, C, es):
    """batch()'s lines with masked (-inf) classes: every label of the lexicon on the line of 40 columns, all but label
    2 (no entry is it alone) on the line of 5 - no segmentation is left on either -, the blank on the line of 160 and
    class 3 on the line of 2, which keep theirs"""
    logits, il = batch(seed, C, es)
    logits[:, 1, 1:4] = -np.inf
    logits[:, 2, [1, 3]] = -np.inf
    logits[:, 0, 0] = -np.inf
    logits[:, 3, 3] = -np.inf
    return logits, il


BATCHES = {"short": batch_short, "masked": batch_masked}
NO_WORDS = {"short": [2, 3, 4], "masked": [1, 2]}            # the lines without a segmentation


@pytest.fixture(scope="module")
def cases(recognizer, ctc):
    out = {}
    for k, (name, (C, es, pr, bonus)) in enumerate(LEXICA.items()):
        logits, il = BATCHES.get(name, batch)(910 + k, C, es)
        lex = ctc.Lexicon(es, num_classes=C, priors=pr)
        out[name] = dict(C=C, es=es, pr=pr, bonus=bonus, logits=logits, il=il, lex=lex, nodes=lex.info()["nodes"],
                         want=ref.words(logits, es, pr, bonus, il), got=recognizer(logits, lex, bonus, input_lengths=il))
    return out


def test_cases_cover_the_forms(cases):
    nodes = {k: c["nodes"] for k, c in cases.items()}
    print(nodes)
    assert nodes["npt1"] <= 1024 < nodes["npt2"] <= 2048 < nodes["npt4"] <= ref.LDS_NODES
    assert 6000 <= nodes["scratch"] <= 8000


@pytest.mark.parametrize("name", list(LEXICA))
def test_against_the_yardstick(name, cases, recognizer, ctc):
    c = cases[name]
    check(c["got"], c["logits"], c["il"], c["es"], c["pr"], c["bonus"], c["want"], name)
    none = np.array([w[0] == -np.inf for w in c["want"]])          # (check() holds the engine to the same pattern)
    assert np.flatnonzero(none).tolist() == NO_WORDS.get(name, [])  # elsewhere a one-label word fits every line
    assert ((c["got"].count == 0) == none).all() and (c["got"].score[none] == -np.inf).all()
    text_nll_bits(ctc, recognizer._context(), c["got"], c["logits"], c["il"], name)


@pytest.mark.parametrize("name", list(LEXICA))
def test_bit_identity(name, cases, recognizer):
    c = cases[name]
    logits, il, lex, bonus, base = c["logits"], c["il"], c["lex"], c["bonus"], c["got"]
    call = lambda x, le=il: recognizer(x, lex, bonus, input_lengths=le)
    _same_bits(base, call(logits), name + ": repeated call")
    _same_bits(base, call(torch.from_numpy(logits).cuda(0), torch.from_numpy(il)), name + ": device pointer")
    for var, what in (("HCTR_WORDS_LDS", "0"), ("HCTR_WORDS_LINES", "2")):
        os.environ[var] = what
        try:
            _same_bits(base, call(logits), "%s: %s=%s" % (name, var, what))
        finally:
            del os.environ[var]
    for b in (0, 1, 3):
        alone = call(np.ascontiguousarray(logits[:, b:b + 1]), il[b:b + 1])
        for f in FIELDS:
            assert getattr(alone, f)[0].tobytes() == getattr(base, f)[b].tobytes(), (name, b, f)


def test_planted_words_with_a_unique_optimum(recognizer, ctc):
    """spellings over disjoint labels: one segmentation per text, and a planted margin of 12 per column"""
    C = 12
    es = [[1, 2, 3], [4, 5], [6, 7, 8, 9], [10], [11, 11]]
    rng = np.random.RandomState(920)
    seqs = [[0, 1, 3, 2, 4, 0, 3], [2, 2, 1], [4], [3]]
    T = [W0, 40, 5, 1]
    logits = np.stack([plant(rng, W0, C, [c for w in s for c in es[w]], T=t, lead=l)
                       for s, t, l in zip(seqs, T, (2, 2, 0, 0))], axis=1)
    il = np.array(T, np.int32)
    lex = ctc.Lexicon(es, num_classes=C)
    want = ref.words(logits, es, None, -0.5, il)
    got = recognizer(logits, lex, -0.5, input_lengths=il)
    check(got, logits, il, es, None, -0.5, want, "unique")
    for b, s in enumerate(seqs):
        assert want[b][1] == s                                    # (the plant decides, in float64)
        assert got.words[b, :got.count[b]].tolist() == s and got.starts[b, :got.count[b]].tolist() == want[b][2], b
    spans = list(got.lines(lex))
    assert [w[0] for w in spans[0]] == seqs[0] and spans[0][-1][3] == W0 and spans[0][0][2] == 2
    assert all(a[3] == b[2] for a, b in zip(spans[0], spans[0][1:])) and spans[3] == [(3, [10], 0, 1)]
    # fewer places than words: the first words and the true count
    few = recognizer(logits, lex, -0.5, max_words=3, input_lengths=il)
    assert few.words.shape == (4, 3) and few.count.tolist() == got.count.tolist() == [7, 3, 1, 1]
    assert few.words.tobytes() == np.ascontiguousarray(got.words[:, :3]).tobytes()
    assert few.starts.tobytes() == np.ascontiguousarray(got.starts[:, :3]).tobytes()
    _same_bits(few, got, "max_words", ("score", "count", "labels", "lengths", "text_nll"))
    assert list(few.lines(lex))[0][-1][3] is None


def test_against_the_pattern_of_the_same_language(pkg, recognizer, ctc):
    """(w1|w2|...)+ as a Pattern: the same best path, found by the DFA's Viterbi"""
    codec = pkg.ctc_codec(CHARS)
    C = len(codec.characters)
    texts = ["ab", "cd", "efg", "h", "ba"]
    lex = ctc.Lexicon(texts, codec=codec)
    pat = ctc.Pattern.compile("(" + "|".join(texts) + ")+", codec)
    rng = np.random.RandomState(930)
    planted = ["abhefgcd", "baab", "h", "h"]
    T = [W0, 40, 5, 1]
    lines = [plant(rng, W0, C, [codec.dict[ch] for ch in t], T=n, lead=l) for t, n, l in zip(planted, T, (2, 1, 1, 0))]
    lines.append((rng.standard_normal((W0, C)) * 3.0).astype(np.float32))
    logits, il = np.stack(lines, axis=1), np.array(T + [40], np.int32)
    got = recognizer(logits, lex, 0.0, input_lengths=il)
    ctx = recognizer._context()
    want = ctc.pattern_logits(ctx, logits, 0, pat, il)
    err = np.abs(got.score.astype(np.float64) - want.best_logp)
    print("words against the pattern: score", got.score, "best_logp", want.best_logp, "max |d| %.2e" % err.max())
    assert np.isfinite(want.best_logp).all() and (err <= _tol(want.best_logp.astype(np.float64))).all()
    assert got.texts(codec)[:4] == planted == want.texts(codec)[:4]
    assert [w[1] for w in next(got.lines(lex))] == ["ab", "h", "efg", "cd"]


def test_score_bits_under_a_permutation_of_the_entries(cases, recognizer, ctc):
    for name in ("ambiguous", "npt2", "scratch"):
        c = cases[name]
        perm = np.random.RandomState(940).permutation(len(c["es"]))
        es = [c["es"][k] for k in perm]
        pr = None if c["pr"] is None else c["pr"][perm]
        got = recognizer(c["logits"], ctc.Lexicon(es, num_classes=c["C"], priors=pr), c["bonus"], input_lengths=c["il"])
        assert got.score.tobytes() == c["got"].score.tobytes(), name
        check(got, c["logits"], c["il"], es, pr, c["bonus"], c["want"], name + " permuted")


def test_masked_and_non_finite_logits(recognizer, ctc):
    C = 12
    es = [[1, 2], [3, 4], [5]]
    lex = ctc.Lexicon(es, num_classes=C)
    rng = np.random.RandomState(950)
    logits = np.stack([plant(rng, 40, C, [1, 2, 5, 3, 4]) for _ in range(4)], axis=1)
    clean = recognizer(logits, lex)
    assert all(clean.words[b, :clean.count[b]].tolist() == [0, 2, 1] for b in range(4))
    # a masked class that removes every path of the best first word: the runner-up, as float64 has it
    masked = logits.copy()
    masked[:, 1, 2] = -np.inf
    got = recognizer(masked, lex)
    want = ref.words(masked, es)
    check(got, masked, np.full(4, 40), es, None, 0.0, want, "masked")
    assert 0 not in got.words[1, :got.count[1]].tolist() and got.words[1, :got.count[1]].tolist() == want[1][1]
    for b in (0, 2, 3):
        for f in FIELDS:
            assert getattr(got, f)[b].tobytes() == getattr(clean, f)[b].tobytes(), (b, f)
    # a NaN, a +inf and a row of nothing but -inf zero their own line only
    for what, put in (("NaN", lambda z: z.__setitem__((7, 2, 9), np.nan)), ("+inf", lambda z: z.__setitem__((7, 2, 3), np.inf)),
                      ("NaN on a lexicon class", lambda z: z.__setitem__((39, 2, 1), np.nan)),
                      ("all -inf", lambda z: z.__setitem__((0, 2), -np.inf))):
        bad = logits.copy()
        put(bad)
        got = recognizer(bad, lex)
        assert got.count[2] == 0 and got.score[2] == -np.inf and got.text_nll[2] == np.inf and got.lengths[2] == 0, what
        assert (got.words[2] == -1).all() and (got.starts[2] == -1).all() and (got.labels[2] == 0).all(), what
        for b in (0, 1, 3):
            for f in FIELDS:
                assert getattr(got, f)[b].tobytes() == getattr(clean, f)[b].tobytes(), (what, b, f)
    # the bad row beyond the line's length does not count
    bad = logits.copy()
    bad[30, 2] = np.nan
    il = np.array([40, 40, 30, 40], np.int32)
    got, ok = recognizer(bad, lex, input_lengths=il), recognizer(logits, lex, input_lengths=il)
    _same_bits(got, ok, "a NaN row beyond the length")


def test_argument_errors(recognizer, ctc, pkg):
    lib, ctx = pkg.load_library(), recognizer._context()
    vp = ctypes.c_void_p
    W, B, C = 8, 2, 6
    x = np.zeros((W, B, C), np.float32)
    lex, other = ctc.Lexicon([[1, 2], [3]], num_classes=C), ctc.Lexicon([[1]], num_classes=C + 1)
    score = np.zeros(B, np.float32)

    def call(lx, il=None, logits=x, bonus=0.0, mw=W):
        return lib.hctr_words_logits(ctx, None if lx is None else lx._h, None if logits is None else logits.ctypes.data_as(vp),
                                     0, W, B, C, None if il is None else np.array(il, np.int32).ctypes.data_as(vp),
                                     bonus, mw, score.ctypes.data_as(vp), *([None] * 6))

    assert call(lex) == 0 and np.isfinite(score).all()
    assert call(None) == -1 and b"lex" in lib.hctr_last_error(ctx)
    assert call(other) == -1 and b"classes" in lib.hctr_last_error(ctx)
    assert call(lex, il=[0, 8]) == -1 and call(lex, il=[8, 9]) == -1 and b"outside [1,8]" in lib.hctr_last_error(ctx)
    assert call(lex, logits=None) == -1
    for bad in (np.nan, np.inf, -np.inf):
        assert call(lex, bonus=bad) == -1 and b"word_bonus" in lib.hctr_last_error(ctx)
    assert call(lex, mw=0) == -1 and call(lex, mw=W + 1) == -1 and b"max_words" in lib.hctr_last_error(ctx)
    for kw in (dict(input_lengths=[0, 8]), dict(input_lengths=[8, 9]), dict(input_lengths=[8]), dict(max_words=0),
               dict(max_words=W + 1)):
        with pytest.raises(ValueError):
            recognizer(x, lex, **kw)
    with pytest.raises(ValueError):
        recognizer(x, other)
    with pytest.raises(ValueError):
        recognizer(x, "not a lexicon")
    empty = recognizer(np.zeros((W, 0, C), np.float32), lex)
    assert empty.score.shape == (0,) and empty.words.shape == (0, W) and empty.label_lists() == []
    ok = recognizer(x, lex, input_lengths=[1, 8])                # the context is still usable
    assert ok.count[0] == 1 and ok.words[0, 0] == 1 and ok.count[1] >= 1


def test_trie_over_the_node_limit_is_refused_by_the_host_check(recognizer, ctc, pkg):
    lib, ctx = pkg.load_library(), recognizer._context()
    rng = np.random.RandomState(63)
    C = 300
    lex = ctc.Lexicon(random_entries(rng, C, 40000, lo=3, hi=3), num_classes=C)
    nodes = lex.info()["nodes"]
    assert nodes > ref.MAX_NODES
    # nothing is read of the logits and nothing is launched: the tables are refused first
    rc = lib.hctr_words_logits(ctx, lex._h, ctypes.c_void_p(64), 0, 8, 1, C, None, 0.0, 1, *([None] * 7))
    msg = lib.hctr_last_error(ctx)
    assert rc == -1 and str(nodes).encode() in msg and str(ref.MAX_NODES).encode() in msg


def test_image_path_equals_logits_path(pkg, synth, m_trained, ctc):
    """hctr_words(images) == hctr_words_logits(hctr_forward_logits(images) in f16x3), also with the batch split into
    internal passes (a second context with a small pass size)"""
    C, W = synth.DEFAULT_VOCAB + 2, 160
    imgs = synth.make_font_lines(3, W, 40 + W)
    widths = np.array([W, W - 29, W - 50], np.int32)
    labels = m_trained.greedy(imgs, widths=widths)
    assert all(len(v) >= 2 for v in labels)
    rng = np.random.RandomState(960)
    es = [[int(c) for c in v[:len(v) // 2]] for v in labels] + [[int(c) for c in v[len(v) // 2:]] for v in labels]
    es += random_entries(rng, C, 200, hi=5)
    lex = ctc.Lexicon(es, num_classes=C)
    fused = m_trained.words(imgs, lex, -1.0, widths=widths)
    m_trained.set_precision("f16x3")
    try:
        logits = m_trained(torch.from_numpy(imgs).cuda(0), widths=widths)
    finally:
        m_trained.set_precision("auto")
    unfused = pkg.WordRecognizer().attach(m_trained)(logits, lex, -1.0)
    os.environ["HCTR_MAX_COLS"] = "600"                    # f16x3 passes of 200 columns: one or two lines each
    try:
        small = pkg.hctr_model(C, precision="auto").cuda(0)
    finally:
        del os.environ["HCTR_MAX_COLS"]
    small.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    assert small.lines_per_pass(3, W, f16x3=True) < 3
    split = small.words(imgs, lex, -1.0, widths=widths)
    _same_bits(fused, unfused, "logits path")
    _same_bits(fused, split, "split passes")
    assert np.isfinite(fused.score).all() and np.isfinite(fused.text_nll).all()
    for b in range(3):
        assert fused.label_lists()[b].tolist() == [int(c) for c in labels[b]], b
    codec = pkg.ctc_codec(synth.characters()).attach(m_trained)
    word_lists, res = codec.words(logits, lex, -1.0)
    _same_bits(fused, res, "through the codec")
    assert [sum(len(w) for w in line) for line in word_lists] == [len(v) for v in labels]


def test_workload_shape(recognizer, ctc):
    """the flagship's logits shape, C = 7358, W = 2000, 4 lines, about 3000 entries cut from the lines' texts: the score
    rule, the sandwich and finiteness. The texts are random label sequences planted on the lines (margin 12), which
    are then the lines' greedy texts by construction; no model is loaded to produce them."""
    rng = np.random.RandomState(970)
    C, W = 7358, 2000
    texts = [[int(v) for v in rng.randint(1, C, size=n)] for n in (300, 200, 320, 100)]
    T = [W, 1500, W, 700]
    es = []
    for t in texts:
        k = 0
        while k < len(t):                                        # one segmentation of the text, then random cuts
            n = rng.randint(1, 5)
            es.append(t[k:k + n])
            k += n
        for _ in range(650):
            k, n = rng.randint(0, len(t)), rng.randint(1, 5)
            es.append(t[k:k + n])
    pr = (rng.randn(len(es)) * 0.5).astype(np.float32)
    lex = ctc.Lexicon(es, num_classes=C, priors=pr)
    print(lex.info())
    logits = np.stack([plant(rng, W, C, t, n) for t, n in zip(texts, T)], axis=1)
    il = np.array(T, np.int32)
    got = recognizer(torch.from_numpy(logits).cuda(0), lex, -0.5, input_lengths=il)
    want = ref.words(logits, es, pr, -0.5, il)
    check(got, logits, il, es, pr, -0.5, want, "workload")
    assert np.isfinite(got.score).all() and np.isfinite(got.text_nll).all() and (got.count > 20).all()


def test_no_side_effects(pkg, ctc, synth, m_trained):
    rng = np.random.RandomState(980)
    W, B, C = 90, 3, 40
    logits = rng.standard_normal((W, B, C)).astype(np.float32)
    targets = rng.randint(1, C, size=32).astype(np.int32)
    tl = np.array([7, 0, 25], np.int32)
    imgs = synth.make_font_lines(3, 96, 31)
    ctx = m_trained._ctx
    es = random_entries(rng, C, 50, hi=7)
    lex = ctc.Lexicon(es, num_classes=C)
    pat = ctc.Pattern(*pattern_ref.trie(es), C)

    def others():
        g = m_trained.greedy(imgs)
        nll = ctc.loss_logits(ctx, logits, 0, targets, tl, None)
        al = ctc.align_logits(ctx, logits, 0, targets, tl, None)
        lx = ctc.lexicon_logits(ctx, logits, 0, lex, 5, None, True)
        pt = ctc.pattern_logits(ctx, logits, 0, pat)
        return g, nll, al, lx, pt

    g0, nll0, al0, lx0, pt0 = others()
    guard0 = m_trained.last_guard()
    w0 = ctc.words_logits(ctx, logits, 0, lex, -0.5)
    os.environ["HCTR_WORDS_LDS"] = "0"
    try:
        w1 = ctc.words_logits(ctx, logits, 0, lex, 0.25)         # another bonus: other tables, another scratch layout
    finally:
        del os.environ["HCTR_WORDS_LDS"]
    big = ctc.Lexicon([[int(c) for c in g0[0][:2]] if len(g0[0]) >= 2 else [1], [5]], num_classes=synth.DEFAULT_VOCAB + 2)
    res = m_trained.words(imgs, big)
    guard1 = m_trained.last_guard()
    assert guard0["lines"] == guard1["lines"] and guard0["flagged"] == guard1["flagged"]
    assert not np.isnan(res.score).any() and (w0.count >= 1).all() and (w1.count >= 1).all()
    # the other bonus on the same lexicon is another set of tables: each call against its own yardstick
    for w, bonus in ((w0, -0.5), (w1, 0.25)):
        check(w, logits, np.full(B, W), es, None, bonus, ref.words(logits, es, None, bonus), "bonus %g" % bonus)
    assert (np.abs(w0.score - w1.score) > 0.5).all()              # (at least one word each: the scores differ by 0.75 a word)
    g1, nll1, al1, lx1, pt1 = others()
    for x, y in zip(g0, g1):
        np.testing.assert_array_equal(x, y)
    assert nll0.tobytes() == nll1.tobytes()
    for k in ("paths", "starts", "ends", "logps", "scores"):
        assert getattr(al0, k).tobytes() == getattr(al1, k).tobytes(), k
    for k in ("entries", "logp", "rank", "log_total", "count", "scores"):
        assert getattr(lx0, k).tobytes() == getattr(lx1, k).tobytes(), k
    for k in pt0.FIELDS:
        assert getattr(pt0, k).tobytes() == getattr(pt1, k).tobytes(), k
    _same_bits(w0, ctc.words_logits(ctx, logits, 0, lex, -0.5), "words after the others")


def test_cli_decode_method_words(tmp_path, pkg, synth, state_dict):
    """test.py -dm words --lexicon FILE: with zero priors and no bonus the best segmentation reads the f16x3 greedy text
    whenever the lexicon can spell it, and the CLI prints its words separated by /"""
    import ast
    import subprocess
    import sys
    from PIL import Image
    from conftest import ROOT
    folder = tmp_path / "lines"
    folder.mkdir()
    widths = [120, 97]
    imgs = [synth.make_line_images(1, w, 710 + i)[0] for i, w in enumerate(widths)]
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(folder / ("%06d.png" % i))
    cd = pkg.ctc_codec(synth.characters())
    m = pkg.hctr_model(synth.DEFAULT_VOCAB + 2, precision="f16x3").cuda(0)
    m.load_state_dict(state_dict)
    batch = np.zeros((2, 128, max(widths)), np.uint8)
    for j in range(2):
        batch[j, :, :widths[j]] = imgs[j]
    want = cd.labels_to_text(m.greedy(batch, widths=np.array(widths, np.int32)))
    assert all(len(t) >= 2 and "/" not in t for t in want)
    with open(tmp_path / "words.txt", "w", encoding="utf-8") as f:
        for t in want:
            for k in range(0, len(t), 3):
                f.write(t[k:k + 3] + "\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "test.py"), "-m", "hctr", "-f", "synthetic", "-b", "2", "-i",
                        str(folder), "-dm", "words", "--lexicon", str(tmp_path / "words.txt"), "--precision", "auto"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    got = []
    for line in r.stdout.splitlines():
        if line.startswith("predicted results: "):
            got += ast.literal_eval(line[len("predicted results: "):])
    print(got)
    assert [g.replace("/", "") for g in got] == want and all("/" in g for g in got if len(g) > 4)
