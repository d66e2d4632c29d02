"""GPU tests (-m gpu) of the set form of pattern-constrained recognition (``hctr_pat_build_sets`` patterns through
hctr_pattern_logits): arcs that carry label sets, the recursion in block form (pattern_set_kernel).

The yardstick is tests/pattern_set_ref.py (float64, exclusion by prefix and suffix log-sums), which
tests/test_pattern_set_host.py checks against tests/pattern_ref.py. What must hold:
  * logp within the family's 1e-5 * |x| + 1e-3 of the float64 yardstick with the same -inf pattern; best_logp <= logp <= 0;
  * every Viterbi output (best_logp, path, labels, lengths, spans, char_logp, text_nll) has the bits of the explicit form
    of the same language on the same logits - planted, flat random and all-zero logits (the tie rule alone), no tolerance;
  * a line's bits do not depend on LDS or scratch storage of the step buffers (HCTR_PATSET_LDS=0), the grouping of lines,
    host or device pointers, repetition, the other lines, the spelling, or whether the Viterbi outputs are asked for;
  * `.*` without <unknown> has probability 1, `.*q.*` is spotting's containment posterior, text_nll has the loss's bits;
  * masked and non-finite logits behave as include/hctr_hip.h states for hctr_pattern_logits;
  * at the full vocabulary (C = 7358) `.{2,3}` and `.*年.*` build only as sets and agree with the yardstick and spotting;
  * no set call changes what the other entry points compute.
The cases cover one thread per state (S <= 1024) and several (S = 1181, 2361), one block and 41 blocks.
"""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import pattern_ref
import pattern_set_ref as ref

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-3                      # engine score vs float64 on the same logits (tests/test_gpu_ctc.py's)
C0, W0 = 60, 160
CHARS = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUV"       # labels 1..58; 1..10 are the digits
LENGTHS = [W0, 130, 5, 1]
VITERBI = ("best_logp", "path", "labels", "lengths", "starts", "ends", "logps", "text_nll")


def _tol(want):
    return RTOL * np.abs(want) + ATOL


def _check_scores(got, want, what, factor=1.0):
    """got within the rule of want where want is finite, -inf exactly where want is"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert not np.isnan(got).any(), what
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isneginf(got), ~fin, err_msg="%s: -inf pattern" % what)
    if fin.any():
        err = np.abs(got[fin] - want[fin])
        k = int(np.argmax(err))
        print("%s: %d finite, max |d| %.3e at |x| %.1f, worst excess over the rule %.3e"
              % (what, int(fin.sum()), float(err[k]), float(np.abs(want[fin][k])), float((err - factor * _tol(want[fin])).max())))
        assert (err <= factor * _tol(want[fin])).all(), what


def _same_bits(a, b, what, fields=None):
    for f in fields or a.FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), (what, f)


@pytest.fixture(scope="module")
def ctc(pkg):
    return importlib.import_module(pkg.__name__ + ".ctc")


@pytest.fixture(scope="module")
def recognizer(pkg):
    return pkg.PatternRecognizer().cuda(0)


@pytest.fixture(scope="module")
def codec(pkg):
    cd = pkg.ctc_codec(CHARS)
    assert len(cd.characters) == C0
    return cd


def plant(rng, W, C, text, T=None, margin=12.0, lead=2):
    """unit noise [W][C] plus `margin` on a path that reads `text` in columns [0, T): `lead` blanks, then per character
    a run of two columns and one blank (tests/test_gpu_pattern.py's)"""
    T = W if T is None else T
    z = rng.standard_normal((W, C))
    path = [0] * lead + [c for ch in text for c in (ch, ch, 0)]
    path = (path + [0] * T)[:T]
    assert pattern_ref.collapse(path) == list(text)
    z[np.arange(T), path] += margin
    return z.astype(np.float32)


def sets_dfa(pat):
    return pat.arcs, pat.sets, pat.finals, pat.num_states


# name, expression (None: built from sets below), the text planted on the lines of 160, 130, 5 and 1 columns, the blanks
# that lead each line
CASES = [
    ("any1", r".", ["k", "Q", "g", "4"], [2, 2, 2, 0]),
    ("any2to4", r".{2,4}", ["k7Q", "ab", "g3", "4"], [2, 2, 0, 0]),                      # infeasible at T = 1
    ("contains7", r".*7.*", ["abc7de7", "7", "7", "7"], [2, 2, 2, 0]),
    ("negated", r"[^0-9]+\d{2}", ["hello42", "x07", "a1", "4"], [2, 2, 0, 0]),           # infeasible at T = 1
    ("wild_digits", r".\d{3}", ["k123", "Q900", "g3", "4"], [2, 2, 0, 0]),
    ("loop58", None, ["anytextatall0123", "", "g3", "4"], [2, 2, 0, 0]),                 # a 58-label set looping on a final state
    ("six", r".{6}", ["abcdef", "012345", "g", "4"], [2, 2, 2, 0]),                      # infeasible at T = 5 and 1
    ("any20", r".{20}", ["abcdefghij0123456789", "ABCDEFGHIJabcdefghij", "g", "4"], [2, 2, 2, 0]),       # S = 1181
    ("any2to40", r".{2,40}", ["abcdefghij0123456789ABCDEFGHIJ", "k7", "g3", "4"], [2, 2, 0, 0]),        # S = 2361
]


def build_pair(ctc, codec, expr):
    """(the set form, the explicit form) of one language"""
    if expr is None:
        every = list(range(1, 59))
        return (ctc.Pattern.from_sets([(0, 0, 0)], [every], [0], 1, C0), ctc.Pattern([(0, c, 0) for c in every], [0], 1, C0))
    return ctc.Pattern.compile(expr, codec, sets=True), ctc.Pattern.compile(expr, codec, sets=False)


@pytest.fixture(scope="module")
def cases(recognizer, ctc, codec):
    out = {}
    for k, (name, expr, texts, leads) in enumerate(CASES):
        rng = np.random.RandomState(1800 + k)
        labels = [[codec.dict[ch] for ch in t] for t in texts]
        planted = np.stack([plant(rng, W0, C0, t, T, lead=n) for t, T, n in zip(labels, LENGTHS, leads)], axis=1)
        flat = rng.standard_normal((W0, 4, C0)).astype(np.float32)
        il = np.array(LENGTHS, np.int32)
        pat, explicit = build_pair(ctc, codec, expr)
        c = dict(expr=expr, texts=texts, labels=labels, il=il, pat=pat, explicit=explicit, logits={}, got={}, want={}, ex={})
        for kind, z in (("planted", planted), ("flat", flat)):
            c["logits"][kind] = z
            c["got"][kind] = recognizer(z, pat, input_lengths=il)
            c["ex"][kind] = recognizer(z, explicit, input_lengths=il)
            c["want"][kind] = ref.run(z, *sets_dfa(pat), input_lengths=il)
        out[name] = c
    return out


def test_cases_cover_the_kernel(cases):
    info = {k: v["pat"].info() for k, v in cases.items()}
    print(info)
    assert all(v["pat"].kind == 1 and v["explicit"].kind == 0 for v in cases.values())
    for k, v in cases.items():
        a, b = info[k], v["explicit"].info()
        assert (a["dfa_states"], a["states"], a["classes"]) == (b["dfa_states"], b["states"], b["classes"]), k
    assert info["any1"]["states"] == 60 and info["loop58"]["dfa_states"] == 1 and info["loop58"]["states"] == 59
    assert info["any20"]["states"] == 1181 and info["any2to40"]["states"] == 2361 and info["any2to40"]["dfa_states"] == 41
    assert info["contains7"]["max_in_degree"] == 2
    for name, lines in (("six", (2, 3)), ("any2to4", (3,)), ("negated", (3,)), ("wild_digits", (3,))):
        for b in lines:
            assert cases[name]["want"]["planted"][b][2] is None, (name, b)
    assert all(c["want"]["planted"][0][2] is not None for c in cases.values())


def test_scores_against_float64(cases):
    worst = (0.0, 0.0)
    for name, c in cases.items():
        for kind in ("planted", "flat"):
            got, want = c["got"][kind], c["want"][kind]
            _check_scores(got.logp, [w[0] for w in want], "%s %s logp" % (name, kind))
            _check_scores(got.best_logp, [w[1] for w in want], "%s %s best_logp" % (name, kind))
            fin = np.isfinite(got.logp)
            assert (got.best_logp[fin] <= got.logp[fin]).all() and (got.logp <= 0).all(), name
            w = np.array([x[0] for x in want])
            if fin.any():
                err = np.abs(got.logp[fin].astype(np.float64) - w[fin])
                k = int(np.argmax(err))
                worst = max(worst, (float(err[k]), float(abs(w[fin][k]))))
            for b, x in enumerate(want):
                if x[2] is None:
                    assert got.lengths[b] == 0 and (got.path[b] == -1).all() and np.isposinf(got.text_nll[b]), (name, b)
                else:
                    T = LENGTHS[b]
                    assert got.path[b, :T].tolist() == x[2] and (got.path[b, T:] == -1).all(), (name, kind, b)
    print("largest |logp - float64| %.3e at |x| = %.1f" % worst)


def test_viterbi_outputs_have_the_explicit_forms_bits(cases, recognizer):
    for name, c in cases.items():
        for kind in ("planted", "flat"):
            _same_bits(c["got"][kind], c["ex"][kind], "%s %s" % (name, kind), VITERBI)
            # the sums of the two forms differ in their order alone
            _check_scores(c["got"][kind].logp, c["ex"][kind].logp.astype(np.float64), "%s %s logp against the explicit form"
                          % (name, kind), factor=2.0)
        # all-zero logits: every score ties, the tie rule alone decides
        z = np.zeros((24, 3, C0), np.float32)
        il = np.array([24, 7, 2], np.int32)
        got, ex = recognizer(z, c["pat"], input_lengths=il), recognizer(z, c["explicit"], input_lengths=il)
        _same_bits(got, ex, name + " ties", VITERBI)
        want = ref.run(z, *sets_dfa(c["pat"]), input_lengths=il)
        for b, w in enumerate(want):
            if w[2] is None:
                assert np.isneginf(got.best_logp[b]) and got.lengths[b] == 0
            else:
                assert got.path[b, :il[b]].tolist() == w[2], (name, b)


def test_planted_text_is_decoded(cases, codec):
    for name, c in cases.items():
        texts = c["got"]["planted"].texts(codec)
        for b, w in enumerate(c["want"]["planted"]):
            if w[2] is not None and pattern_ref.collapse(w[2]) == c["labels"][b]:
                assert texts[b] == c["texts"][b], (name, b)
        assert texts[0] == c["texts"][0], name
        post = c["got"]["planted"].posterior()
        assert ((post >= 0) & (post <= np.exp(2 * ATOL + 1e-3))).all(), name


def test_bit_identity(cases, recognizer, ctc, codec):
    for name, c in cases.items():
        logits, il, pat, base = c["logits"]["planted"], c["il"], c["pat"], c["got"]["planted"]
        call = lambda x, p=pat, le=il, **kw: recognizer(x, p, input_lengths=le, **kw)
        _same_bits(base, call(logits), name + ": repeated call")
        _same_bits(base, call(torch.from_numpy(logits).cuda(0), le=torch.from_numpy(il)), name + ": device pointer")
        os.environ["HCTR_PATSET_LDS"] = "0"
        try:
            _same_bits(base, call(logits), name + ": step buffers in scratch")
            only = call(logits, full=False)
            assert only.logp.tobytes() == base.logp.tobytes(), name + ": forward-only, scratch"
            os.environ["HCTR_PAT_LINES"] = "1"
            _same_bits(base, call(logits), name + ": scratch, groups of one line")
        finally:
            del os.environ["HCTR_PATSET_LDS"]
            os.environ.pop("HCTR_PAT_LINES", None)
        os.environ["HCTR_PAT_LINES"] = "1"
        try:
            _same_bits(base, call(logits), name + ": groups of one line")
        finally:
            del os.environ["HCTR_PAT_LINES"]
        for b in (1, 2):
            alone = call(np.ascontiguousarray(logits[:, b:b + 1]), le=il[b:b + 1])
            for f in base.FIELDS:
                assert getattr(alone, f)[0].tobytes() == getattr(base, f)[b].tobytes(), (name, b, f)
        only = call(logits, full=False)
        assert only.logp.tobytes() == base.logp.tobytes() and only.path is None, name
    # two spellings of one language
    c = cases["negated"]
    other = ctc.Pattern.compile(r"[a-zA-V][^0123456789]*(0|1|2|3|4|5|6|7|8|9)[0-9]", codec, sets=True)
    assert other.kind == 1
    _same_bits(c["got"]["planted"], recognizer(c["logits"]["planted"], other, input_lengths=c["il"]), "two spellings")


def test_identities(cases, recognizer, ctc, codec):
    ctx = recognizer._context()
    rng = np.random.RandomState(1850)
    # every text without <unknown>: probability 1
    z = rng.standard_normal((W0, 3, C0)).astype(np.float32) * 2
    z[:, :, C0 - 1] = -np.inf
    il = np.array([W0, 77, 1], np.int32)
    every = recognizer(z, cases["loop58"]["pat"], input_lengths=il, full=False)
    print("logp of every text:", every.logp)
    assert (np.abs(every.logp) <= 1e-3).all()
    # containment against spotting: `.` never matches <unknown>, so on logits that mask it
    c = cases["contains7"]
    two = ctc.Pattern.compile(r".*ab.*", codec, sets=True)
    for kind in ("planted", "flat"):
        zz = c["logits"][kind].copy()
        zz[:, :, C0 - 1] = -np.inf
        sp = ctc.spot_logits(ctx, zz, 0, [[codec.dict["7"]], [codec.dict["a"], codec.dict["b"]]], c["il"])
        _check_scores(recognizer(zz, c["pat"], input_lengths=c["il"], full=False).logp, sp.logp[:, 0],
                      "contains 7, %s, against spotting" % kind, factor=2.0)
        _check_scores(recognizer(zz, two, input_lengths=c["il"], full=False).logp, sp.logp[:, 1],
                      "contains ab, %s, against spotting" % kind, factor=2.0)
    # text_nll has the loss's bits
    for name, c in cases.items():
        for kind in ("planted", "flat"):
            got = c["got"][kind]
            nll = ctc.loss_logits(ctx, c["logits"][kind], 0, np.concatenate(got.label_lists()).astype(np.int32), got.lengths, c["il"])
            have = np.isfinite(got.best_logp)
            assert have.any() and got.text_nll[have].tobytes() == nll[have].tobytes(), (name, kind)
            assert np.isposinf(got.text_nll[~have]).all()
            assert (-got.text_nll[have] <= got.logp[have] + 2 * _tol(got.logp[have])).all()


def test_masked_and_non_finite_logits(cases, recognizer):
    for name in ("any2to4", "contains7", "negated", "any20"):
        c = cases[name]
        il, pat = c["il"], c["pat"]
        base = c["got"]["flat"]
        # masked classes: the digit 7 and the blank of some columns have probability 0; the defined result, no NaN
        z = c["logits"]["flat"].copy()
        z[:, :, 8] = -np.inf
        z[10:20, 0, 0] = -np.inf
        got, ex = recognizer(z, pat, input_lengths=il), recognizer(z, c["explicit"], input_lengths=il)
        want = ref.run(z, *sets_dfa(pat), input_lengths=il)
        _check_scores(got.logp, [w[0] for w in want], name + " masked logp")
        _check_scores(got.best_logp, [w[1] for w in want], name + " masked best_logp")
        _same_bits(got, ex, name + " masked", VITERBI)
        for b, w in enumerate(want):
            if w[2] is not None:
                assert 8 not in got.path[b].tolist() and got.path[b, :il[b]].tolist() == w[2], (name, b)
        if name == "contains7":
            assert np.isneginf(got.logp).all() and (got.lengths == 0).all() and np.isposinf(got.text_nll).all()
        # a non-finite row on line 1: nothing on that line, the other lines' bits untouched
        for row, value in ((0, np.nan), (64, np.inf), (129, np.nan), (30, -np.inf)):
            z = c["logits"]["flat"].copy()
            if value == -np.inf:
                z[row, 1, :] = value
            else:
                z[row, 1, 3] = value
            got = recognizer(z, pat, input_lengths=il)
            assert np.isneginf(got.logp[1]) and np.isneginf(got.best_logp[1]) and got.lengths[1] == 0, (name, row)
            assert (got.path[1] == -1).all() and np.isposinf(got.text_nll[1]) and not got.labels[1].any(), (name, row)
            for f in base.FIELDS:
                for b in (0, 2, 3):
                    assert getattr(got, f)[b].tobytes() == getattr(base, f)[b].tobytes(), (name, row, f, b)
        z = c["logits"]["flat"].copy()
        z[140, 1, :] = np.nan                                                 # beyond the line's 130 columns: never read
        _same_bits(base, recognizer(z, pat, input_lengths=il), name + ": a row beyond T")


def test_full_vocabulary(recognizer, ctc, pkg):
    """C = 7358, W = 200, 3 lines: patterns that build only as sets, their step buffers too large for LDS"""
    C, W = 7358, 200
    cd = pkg.ctc_codec("".join(chr(0x4E00 + i) for i in range(C - 2)))
    year = cd.dict["年"]
    rng = np.random.RandomState(1860)
    texts = [[100, 200, 300], [7, year, 9, 9, 10], [5000, 6000]]
    T = [W, 150, 40]
    logits = np.stack([plant(rng, W, C, t, n) for t, n in zip(texts, T)], axis=1)
    logits[:, :, C - 1] = -np.inf                  # `.` never matches <unknown>: masked, containment is spotting's
    il = np.array(T, np.int32)
    dev = torch.from_numpy(logits).cuda(0)
    ctx = recognizer._context()
    for expr, hits in ((".{2,3}", [0, 2]), (".*年.*", [1])):
        with pytest.raises(ValueError, match="HCTR_PAT_MAX_STATES"):
            ctc.Pattern.compile(expr, cd, sets=False)
        pat = ctc.Pattern.compile(expr, cd)
        assert pat.kind == 1
        print(expr, pat.info())
        want = ref.run(logits, *sets_dfa(pat), input_lengths=il)
        got = recognizer(dev, pat, input_lengths=il)
        _check_scores(got.logp, [w[0] for w in want], "full vocabulary %s logp" % expr)
        _check_scores(got.best_logp, [w[1] for w in want], "full vocabulary %s best_logp" % expr)
        for b in hits:
            assert got.label_lists()[b].tolist() == texts[b] and got.path[b, :T[b]].tolist() == want[b][2], (expr, b)
        only = recognizer(dev, pat, input_lengths=il, full=False)
        assert only.logp.tobytes() == got.logp.tobytes()
        _same_bits(got, recognizer(logits, pat, input_lengths=il), expr + ": host pointer")
        if "年" in expr:
            sp = ctc.spot_logits(ctx, logits, 0, [np.array([year], np.int32)], il)
            _check_scores(got.logp, sp.logp[:, 0], "full vocabulary containment against spotting", factor=2.0)
            assert got.logp[1] > -0.05 and got.logp[0] < -3


def test_argument_errors_and_no_side_effects(cases, recognizer, ctc, codec, pkg):
    lib, ctx = pkg.load_library(), recognizer._context()
    vp = ctypes.c_void_p
    rng = np.random.RandomState(1870)
    W, B, C = 90, 3, 40
    logits = rng.standard_normal((W, B, C)).astype(np.float32)
    targets = rng.randint(1, C, size=32).astype(np.int32)
    tl = np.array([7, 0, 25], np.int32)
    es = [[int(v) for v in rng.randint(1, C, size=rng.randint(1, 8))] for _ in range(50)]
    lex = ctc.Lexicon(es, num_classes=C)
    explicit = ctc.Pattern(*pattern_ref.trie(es), C)

    def others():
        nll = ctc.loss_logits(ctx, logits, 0, targets, tl, None)
        al = ctc.align_logits(ctx, logits, 0, targets, tl, None)
        sp = ctc.spot_logits(ctx, logits, 0, [[1, 2], [3]], None)
        lx = ctc.lexicon_logits(ctx, logits, 0, lex, 5, None, True)
        pt = ctc.pattern_logits(ctx, logits, 0, explicit)
        rc = ctc.recognize_logits(ctx, logits, 0)
        return [nll.tobytes()] + [getattr(al, k).tobytes() for k in ("paths", "starts", "ends", "logps", "scores")] + \
            [getattr(sp, k).tobytes() for k in ("logp", "seg_logp", "starts", "ends")] + \
            [getattr(lx, k).tobytes() for k in ("entries", "logp", "rank", "log_total", "count", "scores")] + \
            [getattr(pt, k).tobytes() for k in pt.FIELDS] + \
            [getattr(rc, k).tobytes() for k in ("labels", "lengths", "starts", "ends", "logps", "path_logp", "text_nll")]

    before = others()
    sets = [list(range(1, C - 1))]
    pat = ctc.Pattern.from_sets([(0, 0, 1), (1, 0, 1)], sets, [1], 2, C)
    other = ctc.Pattern.from_sets([(0, 0, 1)], sets, [1], 2, C + 1)
    logp = np.zeros(B, np.float32)

    def call(p, il=None, z=logits):
        return lib.hctr_pattern_logits(ctx, None if p is None else p._h, None if z is None else z.ctypes.data_as(vp),
                                       0, W, B, C, None if il is None else np.array(il, np.int32).ctypes.data_as(vp),
                                       logp.ctypes.data_as(vp), *([None] * 8))

    assert call(pat) == 0 and np.isfinite(logp).all()
    assert call(other) == -1 and b"classes" in lib.hctr_last_error(ctx)
    assert call(pat, il=[0, 8, 8]) == -1 and call(pat, il=[8, 91, 8]) == -1 and b"outside [1,90]" in lib.hctr_last_error(ctx)
    assert call(pat, z=None) == -1
    assert lib.hctr_pat_kind(pat._h) == 1 and lib.hctr_pat_kind(explicit._h) == 0 and lib.hctr_pat_kind(None) == -1
    with pytest.raises(ValueError):
        recognizer(logits, other)
    empty = recognizer(np.zeros((W, 0, C), np.float32), pat)
    assert empty.logp.shape == (0,) and empty.path.shape == (0, W)
    os.environ["HCTR_PATSET_LDS"] = "0"
    try:
        res = recognizer(logits, pat, input_lengths=[1, 90, 45])             # another scratch layout, and usable after errors
    finally:
        del os.environ["HCTR_PATSET_LDS"]
    assert np.isfinite(res.logp).all() and res.lengths[0] == 1
    recognizer(cases["any2to40"]["logits"]["flat"], cases["any2to40"]["pat"])
    assert others() == before
