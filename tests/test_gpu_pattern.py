"""GPU tests (-m gpu) of pattern-constrained recognition (C ABI hctr_pattern / hctr_pattern_logits,
``PatternRecognizer``, ``hctr_model.pattern``, ``ctc_codec.pattern``): the exact log-probability that a line's text
matches a pattern (a DFA over labels) and the best matching reading with spans, by the CTC sum and max recursions over
the automaton.

The reference project has no counterpart; the yardstick is tests/pattern_ref.py, a float64 restatement of the
definitions in include/hctr_hip.h that tests/test_pattern_host.py checks against enumeration of all paths and against
the family's other yardsticks. What must hold:
  * on planted lines (unit noise plus 12 on a planted path; T = 160, 130, 5, 1) logp and best_logp are within the loss
    tests' 1e-5 relative + 1e-3 of float64 on the same logits with the same -inf pattern, the planted text is decoded
    and the path is the yardstick's;
  * every path is valid: its collapse is the decoded text, the pattern's expression accepts it, its float64 score is
    within the rule of best_logp, the spans are its runs and char_logp the float32 sums over them;
  * on flat random logits the path is an accepted one whose float64 score is within the rule of the optimum; on all-zero
    logits every score ties exactly and the tie rule alone decides the path;
  * best_logp <= logp <= 0;
  * the device's own relations: a literal pattern against the loss, a union of literals against the lexicon's total, a
    "contains" pattern against spotting, text_nll against the loss on the decoded labels (bit for bit);
  * every NPT instance of the kernel (S up to about 6000) on trie-shaped automata against the lexicon;
  * a pair's bits do not depend on the grouping of lines, host or device pointers, repetition, the other lines, the
    spelling of the expression, or whether the Viterbi outputs are asked for;
  * the image path equals the logits path on the engine's own f16x3 logits, bit for bit, across internal passes;
  * no pattern call changes what the loss, the alignment, spotting, the lexicon or greedy decoding compute.
"""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

import pattern_ref as ref

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-3                      # engine score vs float64 on the same logits (tests/test_gpu_ctc.py's)
C0, W0 = 60, 160
CHARS = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUV"       # labels 1..58; 1..10 are the digits
LENGTHS = [W0, 130, 5, 1]


def _tol(want):
    return RTOL * np.abs(want) + ATOL


def _check_scores(got, want, what):
    """got within the rule of want where want is finite, -inf exactly where want is"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert not np.isnan(got).any(), what
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isneginf(got), ~fin, err_msg="%s: -inf pattern" % what)
    if fin.any():
        err = np.abs(got[fin] - want[fin])
        print("%s: %d finite, max |d| %.3e (largest |want| %.1f), worst excess over the rule %.3e"
              % (what, int(fin.sum()), float(err.max()), float(np.abs(want[fin]).max()), float((err - _tol(want[fin])).max())))
        assert (err <= _tol(want[fin])).all(), what


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
    assert ref.collapse(path) == list(text)
    z[np.arange(T), path] += margin
    return z.astype(np.float32)


def dfa(pat):
    return pat.arcs, pat.finals, pat.num_states


# ---- the planted cases, shared (with their float64 results) by several tests: name, expression, the text planted on
# the lines of 160, 130, 5 and 1 columns, the blanks that lead each line ----
CASES = [
    ("digits", r"\d{8}", ["20261020", "13579246", "5", "6"], [2, 2, 2, 0]),              # infeasible at T = 5 and 1
    ("alternation", r"(abc|de\d+)(xy)?|[gh]", ["de2026xy", "abcxy", "g", "h"], [2, 2, 2, 0]),
    ("cycle", r"(ab\d)+", ["ab1ab2ab3ab4ab5", "ab7", "7", "a"], [2, 2, 2, 0]),
    ("set58", r".\d", ["k7", "Q0", "g3", "4"], [2, 2, 0, 0]),
    ("start_final", r"(\d\d)*", ["2026102013", "", "", ""], [2, 2, 2, 0]),
]


@pytest.fixture(scope="module")
def cases(recognizer, ctc, codec):
    out = {}
    for k, (name, expr, texts, leads) in enumerate(CASES):
        rng = np.random.RandomState(800 + k)
        labels = [[codec.dict[ch] for ch in t] for t in texts]
        logits = np.stack([plant(rng, W0, C0, t, T, lead=n) for t, T, n in zip(labels, LENGTHS, leads)], axis=1)
        il = np.array(LENGTHS, np.int32)
        pat = ctc.Pattern.compile(expr, codec)
        out[name] = dict(expr=expr, texts=texts, labels=labels, logits=logits, il=il, pat=pat,
                         want=ref.run(logits, *dfa(pat), input_lengths=il), got=recognizer(logits, pat, input_lengths=il))
    return out


def test_cases_cover_the_patterns(cases):
    info = {k: v["pat"].info() for k, v in cases.items()}
    print(info)
    assert info["set58"]["max_in_degree"] >= 58 and info["digits"]["states"] == 89
    assert 0 in cases["start_final"]["pat"].tables()["accept"]
    want = cases["digits"]["want"]
    assert want[2][2] is None and want[3][2] is None and want[0][2] is not None       # infeasible at T = 5 and T = 1
    assert cases["cycle"]["want"][3][2] is None and cases["set58"]["want"][3][2] is None


def test_scores_against_float64(cases):
    for name, c in cases.items():
        got, want = c["got"], c["want"]
        _check_scores(got.logp, [w[0] for w in want], name + " logp")
        _check_scores(got.best_logp, [w[1] for w in want], name + " best_logp")
        for b, w in enumerate(want):
            if w[2] is None:
                assert got.lengths[b] == 0 and (got.path[b] == -1).all() and np.isposinf(got.text_nll[b]), (name, b)
                assert not got.labels[b].any() and not got.starts[b].any() and not got.ends[b].any()
        fin = np.isfinite(got.logp)
        assert (got.best_logp[fin] <= got.logp[fin]).all() and (got.logp <= 0).all(), name


def test_planted_text_is_decoded(cases, codec):
    for name, c in cases.items():
        texts = c["got"].texts(codec)
        for b, (t, w) in enumerate(zip(c["texts"], c["want"])):
            if re.fullmatch(c["expr"], t) and w[2] is not None:
                assert texts[b] == t, (name, b)
                T = LENGTHS[b]
                assert c["got"].path[b, :T].tolist() == w[2] and (c["got"].path[b, T:] == -1).all(), (name, b)
        post = c["got"].posterior()
        assert ((post >= 0) & (post <= np.exp(2 * ATOL + 1e-3))).all(), name    # (two float32 figures, each within the rule)
    assert cases["digits"]["got"].posterior()[0] > 0.9


def _check_paths(res, logits, il, expr, codec, what):
    """every line's path is an accepted path: collapse, acceptance, score, spans, char_logp"""
    for b in range(len(res)):
        T = int(il[b])
        if np.isneginf(res.best_logp[b]):
            continue
        lp = ref.log_softmax(logits[:T, b])
        path = res.path[b, :T].tolist()
        assert min(path) >= 0 and (res.path[b, T:] == -1).all()
        n = int(res.lengths[b])
        labels, st, en, sums = ref.spans(path, lp)
        assert labels == ref.collapse(path) == res.labels[b, :n].tolist(), (what, b)
        assert re.fullmatch(expr, "".join(codec.characters[c] for c in labels)), (what, b)
        score = float(sum(lp[k, c] for k, c in enumerate(path)))
        assert abs(score - float(res.best_logp[b])) <= _tol(score), (what, b)
        assert st == res.starts[b, :n].tolist() and en == res.ends[b, :n].tolist(), (what, b)
        got = res.logps[b, :n].astype(np.float64)
        run = np.array(en) - np.array(st)
        assert (np.abs(got - np.array(sums, np.float64)) <= 2e-7 * run * (np.abs(got) + 20.0)).all(), (what, b)
        assert not res.labels[b, n:].any() and not res.starts[b, n:].any() and not res.ends[b, n:].any()
        assert not res.logps[b, n:].any()


def test_paths_are_valid(cases, codec, recognizer, ctc):
    ctx = recognizer._context()
    for name, c in cases.items():
        _check_paths(c["got"], c["logits"], c["il"], c["expr"], codec, name)
        # the forced alignment of the decoded text is the same path: its spans and float32 sums, bit for bit
        got = c["got"]
        al = ctc.align_logits(ctx, c["logits"], 0, np.concatenate(got.label_lists()), got.lengths, c["il"])
        o = 0
        for b in range(4):
            n = int(got.lengths[b])
            if re.fullmatch(c["expr"], c["texts"][b]) and n:
                assert al.starts[o:o + n].tolist() == got.starts[b, :n].tolist(), (name, b)
                assert al.logps[o:o + n].tobytes() == got.logps[b, :n].tobytes(), (name, b)
            o += n


def test_flat_random_logits(recognizer, ctc, codec):
    rng = np.random.RandomState(810)
    W, B = 80, 3
    logits = rng.standard_normal((W, B, C0)).astype(np.float32)
    il = np.array([W, 57, 9], np.int32)
    for _, expr, _, _ in CASES:
        pat = ctc.Pattern.compile(expr, codec)
        got, want = recognizer(logits, pat, input_lengths=il), ref.run(logits, *dfa(pat), input_lengths=il)
        _check_scores(got.logp, [w[0] for w in want], "flat %s logp" % expr)
        _check_scores(got.best_logp, [w[1] for w in want], "flat %s best_logp" % expr)     # the optimum, by value
        _check_paths(got, logits, il, expr, codec, "flat " + expr)


def test_tie_rule(recognizer, ctc, codec):
    """all-zero logits: every path has the same score, the rule alone decides the path"""
    W = 12
    logits = np.zeros((W, 3, C0), np.float32)
    il = np.array([W, 7, 2], np.int32)
    for _, expr, _, _ in CASES:
        pat = ctc.Pattern.compile(expr, codec)
        got, want = recognizer(logits, pat, input_lengths=il), ref.run(logits, *dfa(pat), input_lengths=il)
        for b, w in enumerate(want):
            T = int(il[b])
            if w[2] is None:
                assert np.isneginf(got.best_logp[b]) and got.lengths[b] == 0
            else:
                assert got.path[b, :T].tolist() == w[2], (expr, b)
                assert abs(got.best_logp[b] + T * np.log(C0)) <= 1e-3


def test_relations_on_the_device(cases, recognizer, ctc, pkg):
    ctx = recognizer._context()
    c = cases["digits"]
    logits, il = c["logits"], c["il"]
    # a literal pattern against the loss
    text = c["labels"][0]
    lit = recognizer(logits, ctc.Pattern(*ref.literal(text), C0), input_lengths=il)
    nll = ctc.loss_logits(ctx, logits, 0, np.array(text * 4, np.int32), np.full(4, len(text), np.int32), il)
    _check_scores(lit.logp, -nll.astype(np.float64), "literal against the loss")
    assert np.isneginf(lit.logp[2:]).all() and lit.label_lists()[0].tolist() == text
    # a union of 300 literals against the lexicon's total
    rng = np.random.RandomState(811)
    es = set(tuple(t) for t in c["labels"])
    while len(es) < 300:
        es.add(tuple(int(v) for v in rng.randint(1, C0, size=rng.randint(1, 10))))
    es = [list(e) for e in sorted(es)]
    lex = ctc.lexicon_logits(ctx, logits, 0, ctc.Lexicon(es, num_classes=C0), 1, il, False)
    uni = recognizer(logits, ctc.Pattern(*ref.trie(es), C0), input_lengths=il)
    _check_scores(uni.logp, lex.log_total, "union against the lexicon's total")
    for b in range(4):
        assert lex.entries[b, 0] < 0 or es[lex.entries[b, 0]] == uni.label_lists()[b].tolist(), b
    # "contains q" against spotting
    q = text[2:5]
    sp = ctc.spot_logits(ctx, logits, 0, [np.array(q, np.int32)], il)
    has = recognizer(logits, ctc.Pattern(*ref.contains(q, C0), C0), input_lengths=il, full=False)
    _check_scores(has.logp, sp.logp[:, 0], "contains against spotting")
    assert has.logp[0] > -0.01 and has.best_logp is None


def test_text_nll_has_the_bits_of_the_loss(cases, recognizer, ctc):
    ctx = recognizer._context()
    for name, c in cases.items():
        got = c["got"]
        nll = ctc.loss_logits(ctx, c["logits"], 0, np.concatenate(got.label_lists()).astype(np.int32), got.lengths, c["il"])
        have = np.isfinite(got.best_logp)
        assert have.any() and got.text_nll[have].tobytes() == nll[have].tobytes(), name
        assert np.isposinf(got.text_nll[~have]).all()
        assert (-got.text_nll[have] <= got.logp[have] + 2 * _tol(got.logp[have])).all()     # the text's mass is part of the pattern's


@pytest.mark.parametrize("nodes", [600, 1500, 3000])
def test_every_instance_on_tries(nodes, recognizer, ctc):
    """S of about 1 200, 3 000 and 6 000 CTC states: two, four and eight states per thread"""
    rng = np.random.RandomState(820 + nodes)
    texts = [[5, 6, 5, 7, 7, 8], [9, 10, 11]]
    es = set(tuple(t) for t in texts)
    while True:
        es.update(tuple(int(v) for v in rng.randint(1, C0, size=rng.randint(2, 7))) for _ in range(nodes // 50))
        arcs, finals, nq = ref.trie(sorted(es))
        if nq >= nodes:
            break
    es = [list(e) for e in sorted(es)]
    pat = ctc.Pattern(arcs, finals, nq, C0)
    info = pat.info()
    print("trie of %d nodes:" % nq, info)
    assert 1.8 * nodes <= info["states"] <= 2.2 * nodes
    logits = np.stack([plant(rng, W0, C0, texts[0]), plant(rng, W0, C0, texts[1], T=40)], axis=1)
    il = np.array([W0, 40], np.int32)
    got = recognizer(logits, pat, input_lengths=il)
    want = ref.run(logits, arcs, finals, nq, input_lengths=il)
    _check_scores(got.logp, [w[0] for w in want], "trie logp")
    _check_scores(got.best_logp, [w[1] for w in want], "trie best_logp")
    lex = ctc.lexicon_logits(recognizer._context(), logits, 0, ctc.Lexicon(es, num_classes=C0), 1, il, False)
    _check_scores(got.logp, lex.log_total, "trie against the lexicon's total")
    for b in range(2):
        assert got.label_lists()[b].tolist() == texts[b] == es[lex.entries[b, 0]], b
        assert got.path[b, :il[b]].tolist() == want[b][2], b
    only = recognizer(logits, pat, input_lengths=il, full=False)
    assert only.logp.tobytes() == got.logp.tobytes()


def test_bit_identity(cases, recognizer, ctc, codec, pkg):
    lib = pkg.load_library()
    for name, c in cases.items():
        logits, il, pat, base = c["logits"], c["il"], c["pat"], c["got"]
        call = lambda x, p=pat, le=il, **kw: recognizer(x, p, input_lengths=le, **kw)
        _same_bits(base, call(logits), name + ": repeated call")
        _same_bits(base, call(torch.from_numpy(logits).cuda(0), le=torch.from_numpy(il)), name + ": device pointer")
        i = pat.info()
        assert lib.hctr_pattern_group_lines(i["states"], i["classes"] + 1, W0) >= 4
        os.environ["HCTR_PAT_LINES"] = "1"
        try:
            assert lib.hctr_pattern_group_lines(i["states"], i["classes"] + 1, W0) == 1
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
    c = cases["digits"]
    _same_bits(c["got"], recognizer(c["logits"], ctc.Pattern.compile("[0-9]{4}[0123456789]{2}(0|1|2|3|4|5|6|7|8|9){2}", codec),
                                    input_lengths=c["il"]), "two spellings")
    assert lib.hctr_pattern_group_lines(7359, 7358, 2000) == 24


def test_image_path_equals_logits_path(pkg, synth, m_trained, ctc):
    """hctr_pattern(images) == hctr_pattern_logits(hctr_forward_logits(images) in f16x3), also with the batch split into
    internal passes (a second context with a small pass size); a line's own greedy text wins"""
    C, W = synth.DEFAULT_VOCAB + 2, 160
    imgs = synth.make_font_lines(3, W, 40 + W)
    widths = np.array([W, W - 29, W - 50], np.int32)
    labels = m_trained.greedy(imgs, widths=widths)
    assert all(len(v) >= 1 for v in labels)
    rng = np.random.RandomState(830)
    es = [[int(c) for c in v] for v in labels] + [[int(c) for c in labels[0][:1]], [C - 2, C - 3]]
    es += [[int(v) for v in rng.randint(1, C, size=rng.randint(1, 6))] for _ in range(200)]
    pat = ctc.Pattern(*ref.trie(es), C)
    fused = m_trained.pattern(imgs, pat, widths=widths)
    m_trained.set_precision("f16x3")
    try:
        logits = m_trained(torch.from_numpy(imgs).cuda(0), widths=widths)
    finally:
        m_trained.set_precision("auto")
    unfused = pkg.PatternRecognizer().attach(m_trained)(logits, pat)
    os.environ["HCTR_MAX_COLS"] = "600"                    # f16x3 passes of 200 columns: one or two lines each
    try:
        small = pkg.hctr_model(C, precision="auto").cuda(0)
    finally:
        del os.environ["HCTR_MAX_COLS"]
    small.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    assert small.lines_per_pass(3, W, f16x3=True) < 3
    split = small.pattern(imgs, pat, widths=widths)
    _same_bits(fused, unfused, "logits path")
    _same_bits(fused, split, "split passes")
    assert np.isfinite(fused.logp).all() and np.isfinite(fused.text_nll).all()
    for b in range(3):
        assert fused.label_lists()[b].tolist() == es[b], b
    only = m_trained.pattern(imgs, pat, widths=widths, full=False)
    assert only.logp.tobytes() == fused.logp.tobytes()
    # an expression through a codec
    codec = pkg.ctc_codec(synth.characters()).attach(m_trained)
    texts = codec.labels_to_text([np.array(e) for e in es[:3]])
    by_expr = ctc.Pattern.compile("|".join(texts) + "|.", codec)
    best, res = codec.pattern(logits, by_expr)
    assert best == texts and res.texts(codec) == texts and [len(r) for r in res.lines()] == [len(t) for t in texts]


def test_workload_shape(recognizer, ctc):
    """the flagship's logits shape: C = 7358, W = 2000, 4 lines; an 18-digit and a date-shaped pattern (labels 1..10 the
    digits, 11 / 12 / 13 the year, month and day signs)"""
    rng = np.random.RandomState(840)
    C, W = 7358, 2000
    digit = list(range(1, 11))

    id18 = ([(i, c, i + 1) for i in range(18) for c in digit], [18], 19)
    # \d{4} Y \d{1,2} M \d{1,2} D
    a = [(i, c, i + 1) for i in range(4) for c in digit] + [(4, 11, 5)]
    a += [(5, c, 6) for c in digit] + [(6, c, 7) for c in digit] + [(6, 12, 8), (7, 12, 8)]
    a += [(8, c, 9) for c in digit] + [(9, c, 10) for c in digit] + [(9, 13, 11), (10, 13, 11)]
    date = (a, [11], 12)
    texts = [[1 + (7 * i) % 10 for i in range(18)], [3, 1, 3, 7, 11, 2, 1, 12, 3, 1, 13],
             [int(v) for v in rng.randint(1, C, size=300)], [4, 5, 6, 7, 11, 9, 12, 8, 13]]
    T = [W, 1500, W, 700]
    logits = np.stack([plant(rng, W, C, t, n) for t, n in zip(texts, T)], axis=1)
    il = np.array(T, np.int32)
    dev = torch.from_numpy(logits).cuda(0)
    lps = [ref.log_softmax(logits[:n, b]) for b, n in enumerate(T)]
    for name, d, hits in (("id18", id18, [0]), ("date", date, [1, 3])):
        pat = ctc.Pattern(*d, C)
        print(name, pat.info())
        tab = ref.tables(*d)
        want = [ref.recurse(lp, tab) for lp in lps]
        got = recognizer(dev, pat, input_lengths=il)
        for f, k in (("logp", 0), ("best_logp", 1)):
            w = np.array([x[k] for x in want])
            err = np.abs(getattr(got, f).astype(np.float64) - w)
            print("workload %s %s: largest |d| %.3e, largest |x| %.1f" % (name, f, err.max(), np.abs(w).max()))
            _check_scores(getattr(got, f), w, "workload %s %s" % (name, f))
        for b in hits:
            assert got.label_lists()[b].tolist() == texts[b] and got.path[b, :T[b]].tolist() == want[b][2], (name, b)
        assert got.posterior()[hits[0]] > 0.9


def test_argument_errors(recognizer, ctc, pkg):
    lib, ctx = pkg.load_library(), recognizer._context()
    vp = ctypes.c_void_p
    W, B, C = 8, 2, 6
    x = np.zeros((W, B, C), np.float32)
    pat, other = ctc.Pattern(*ref.literal([1, 2]), C), ctc.Pattern(*ref.literal([1]), C + 1)
    logp = np.zeros(B, np.float32)

    def call(p, il=None, logits=x):
        return lib.hctr_pattern_logits(ctx, None if p is None else p._h, None if logits is None else logits.ctypes.data_as(vp),
                                       0, W, B, C, None if il is None else np.array(il, np.int32).ctypes.data_as(vp),
                                       logp.ctypes.data_as(vp), *([None] * 8))

    assert call(pat) == 0 and np.isfinite(logp).all()
    assert call(None) == -1 and b"pat" in lib.hctr_last_error(ctx)
    assert call(other) == -1 and b"classes" in lib.hctr_last_error(ctx)
    assert call(pat, il=[0, 8]) == -1 and call(pat, il=[8, 9]) == -1 and b"outside [1,8]" in lib.hctr_last_error(ctx)
    assert call(pat, logits=None) == -1
    for kw in (dict(input_lengths=[0, 8]), dict(input_lengths=[8, 9]), dict(input_lengths=[8])):
        with pytest.raises(ValueError):
            recognizer(x, pat, **kw)
    with pytest.raises(ValueError):
        recognizer(x, other)
    with pytest.raises(ValueError):
        recognizer(x, "not a pattern")
    empty = recognizer(np.zeros((W, 0, C), np.float32), pat)
    assert empty.logp.shape == (0,) and empty.path.shape == (0, W) and empty.label_lists() == []
    ok = recognizer(x, pat, input_lengths=[1, 8])          # the context is still usable
    assert np.isneginf(ok.logp[0]) and ok.lengths.tolist() == [0, 2] and ok.label_lists()[1].tolist() == [1, 2]


def test_no_side_effects(pkg, ctc, synth, m_trained):
    rng = np.random.RandomState(850)
    W, B, C = 90, 3, 40
    logits = rng.standard_normal((W, B, C)).astype(np.float32)
    targets = rng.randint(1, C, size=32).astype(np.int32)
    tl = np.array([7, 0, 25], np.int32)
    imgs = synth.make_font_lines(3, 96, 31)
    ctx = m_trained._ctx
    es = [[int(v) for v in rng.randint(1, C, size=rng.randint(1, 8))] for _ in range(50)]
    lex = ctc.Lexicon(es, num_classes=C)

    def others():
        g = m_trained.greedy(imgs)
        nll = ctc.loss_logits(ctx, logits, 0, targets, tl, None)
        al = ctc.align_logits(ctx, logits, 0, targets, tl, None)
        sp = ctc.spot_logits(ctx, logits, 0, [[1, 2], [3]], None)
        lx = ctc.lexicon_logits(ctx, logits, 0, lex, 5, None, True)
        return g, nll, al, sp, lx

    g0, nll0, al0, sp0, lx0 = others()
    guard0 = m_trained.last_guard()
    ctc.pattern_logits(ctx, logits, 0, ctc.Pattern(*ref.trie(es), C))          # another scratch layout in between
    big = ctc.Pattern(*ref.trie([list(g0[0][:2]) if len(g0[0]) >= 2 else [1], [5]]), synth.DEFAULT_VOCAB + 2)
    res = m_trained.pattern(imgs, big)
    guard1 = m_trained.last_guard()
    assert guard0["lines"] == guard1["lines"] and guard0["flagged"] == guard1["flagged"]
    assert not np.isnan(res.logp).any()
    g1, nll1, al1, sp1, lx1 = others()
    for x, y in zip(g0, g1):
        np.testing.assert_array_equal(x, y)
    assert nll0.tobytes() == nll1.tobytes()
    for k in ("paths", "starts", "ends", "logps", "scores"):
        assert getattr(al0, k).tobytes() == getattr(al1, k).tobytes(), k
    for k in ("logp", "seg_logp", "starts", "ends"):
        assert getattr(sp0, k).tobytes() == getattr(sp1, k).tobytes(), k
    for k in ("entries", "logp", "rank", "log_total", "count", "scores"):
        assert getattr(lx0, k).tobytes() == getattr(lx1, k).tobytes(), k
