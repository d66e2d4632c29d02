"""GPU tests (-m gpu) of weighted patterns (hctr_pat_build_weighted through hctr_pattern / hctr_pattern_logits,
``Pattern(weights=)``, ``Pattern.compile(label_weights=)``, ``Pattern.bigram``): logp = log sum over the pattern's texts
of p(text | line) * exp(w(text)) and the best reading under path log-probability + w(text).

The yardstick is tests/pattern_w_ref.py, a float64 restatement of the header's definitions that
tests/test_pattern_w_host.py checks against enumeration of all paths. What must hold:
  * weights that outvote the emissions flip the decoded text, and the kind-0 pattern of the same automaton still decodes
    what the emissions favour;
  * logp and best_logp within the family's 1e-5 relative + 1e-3 of float64 with an equal -inf pattern, the path equal to
    the yardstick's on planted lines, every path valid (its collapse accepted, its float64 score plus its text's weight
    equal to best_logp by the rule), text_nll with the bits of the loss, ``PatternResult.weights`` = ``text_weight``;
  * all-zero weights give every output of the kind-0 pattern, bit for bit;
  * every instance that the cases mean to reach (states per thread, edges and weights in LDS or through L2) is the one
    the pure selection function names;
  * bit identity under the grouping of lines, host / device pointers, repetition, the other lines, forward-only;
  * the image path equals the logits path; the contract for masked and non-finite logits holds as for kind 0;
  * patterns with equal tables and different weights are told apart by the context's cache, and no weighted call
    changes what the other entry points compute.
"""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import lexicon_ref
import masked_cases as mc
import pattern_ref
import pattern_w_ref as ref

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-3                      # engine score vs float64 on the same logits: the family's rule
C0, W0 = 60, 160
CHARS = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUV"       # labels 1..58; 1..10 are the digits
LENGTHS = [W0, 130, 5, 1]
WORST = {}                                   # what -> (largest |d|, |x| there), printed by the last test


def _tol(want):
    return RTOL * np.abs(want) + ATOL


def _check_scores(got, want, what):
    """got within the rule of want where want is finite, -inf exactly where want is"""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert not np.isnan(got).any(), what
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isneginf(got), ~fin, err_msg="%s: -inf pattern" % what)
    if fin.any():
        err = np.abs(got[fin] - want[fin])
        k = int(np.argmax(err))
        print("%s: %d finite, max |d| %.3e at |x| = %.1f, worst excess over the rule %.3e"
              % (what, int(fin.sum()), float(err[k]), float(np.abs(want[fin][k])), float((err - _tol(want[fin])).max())))
        key = what.split(":")[0]
        if err[k] >= WORST.get(key, (-1.0, 0.0))[0]:
            WORST[key] = (float(err[k]), float(np.abs(want[fin][k])))
        assert (err <= _tol(want[fin])).all(), what


FIELDS = ("logp", "best_logp", "path", "labels", "lengths", "starts", "ends", "logps", "text_nll", "weights")


def _same_bits(a, b, what, fields=FIELDS):
    for f in fields:
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
    a run of two columns and one blank (tests/test_gpu_pattern.py's)"""
    T = W if T is None else T
    z = rng.standard_normal((W, C))
    path = [0] * lead + [c for ch in text for c in (ch, ch, 0)]
    path = (path + [0] * T)[:T]
    assert ref.collapse(path) == list(text)
    z[np.arange(T), path] += margin
    return z.astype(np.float32)


def tab(pat):
    """the yardstick's weighted tables of a Pattern (from the arcs and weights it was given)"""
    return ref.tables(pat.arcs, pat.finals, pat.num_states, pat.weights_given, pat.final_weights_given)


def reaches(pat, npt, edges_lds, weights_lds, full=True):
    """the instance the case means to reach, by the pure selection function"""
    assert pat.kind == 2 and pat.instance(full) == (npt, edges_lds, weights_lds), (pat.info(), pat.instance(full))


def check_against(res, want, t, pat, logits, il, what, paths=True):
    """scores by the rule, the -inf pattern, the path, path validity, the texts' weights"""
    _check_scores(res.logp, [w[0] for w in want], what + ": logp")
    _check_scores(res.best_logp, [w[1] for w in want], what + ": best_logp")
    for b, w in enumerate(want):
        T = int(il[b])
        if w[2] is None:
            assert res.lengths[b] == 0 and (res.path[b] == -1).all() and np.isposinf(res.text_nll[b]), (what, b)
            assert np.isnan(res.weights[b]), (what, b)
            continue
        path = res.path[b, :T].tolist()
        if paths:
            assert path == w[2], (what, b)
        assert min(path) >= 0 and (res.path[b, T:] == -1).all()
        n = int(res.lengths[b])
        labels, st, en, _ = ref.spans(path, np.zeros((T, logits.shape[2])))
        assert labels == res.labels[b, :n].tolist() and st == res.starts[b, :n].tolist() and en == res.ends[b, :n].tolist()
        tw = ref.text_weight(t, labels)
        assert tw > -np.inf and res.weights[b] == tw == pat.text_weight(labels), (what, b)       # the collapse is in L
        lp = ref.log_softmax(logits[:T, b])
        score = float(sum(lp[k, c] for k, c in enumerate(path))) + tw
        assert abs(score - float(res.best_logp[b])) <= _tol(score), (what, b)
        assert res.best_logp[b] <= res.logp[b] + _tol(res.logp[b]), (what, b)


# ---- 1. the decision flips ----
def test_weights_flip_the_decision(recognizer, ctc, codec):
    """ab1 and ab2 share a prefix; the emissions favour ab1 by 2 nats (1 on each of its two columns), the weights favour
    ab2 by 5. Instance: NPT 1, edges and weights in LDS."""
    rng = np.random.RandomState(1000)
    ab1 = [codec.dict[ch] for ch in "ab1"]
    one, two = codec.dict["1"], codec.dict["2"]
    z = plant(rng, W0, C0, ab1)
    cols = np.flatnonzero(np.argmax(z, axis=1) == one)
    assert len(cols) == 2
    z[cols, two] = z[cols, one] - 1.0
    logits = z[:, None, :]
    heavy = ctc.Pattern.compile("ab(1|2)", codec, label_weights={"2": 5.0})
    plain = ctc.Pattern.compile("ab(1|2)", codec)
    reaches(heavy, 1, True, True)
    assert plain.kind == 0 and heavy.tables()["in_src"].tobytes() == plain.tables()["in_src"].tobytes()
    got, base = recognizer(logits, heavy), recognizer(logits, plain)
    assert got.texts(codec) == ["ab2"] and base.texts(codec) == ["ab1"]
    t = tab(heavy)
    want = ref.run(logits, t)
    check_against(got, want, t, heavy, logits, [W0], "flip")
    assert ref.collapse(want[0][2]) == [codec.dict[ch] for ch in "ab2"]
    assert got.weights[0] == 5.0 and base.weights[0] == 0.0
    assert abs((got.best_logp[0] - base.best_logp[0]) - 3.0) <= 2e-3          # +5 of weight, -2 of emissions
    # the posterior under the weights: ab2's share of exp(-nll + w) over both texts
    assert abs(got.posterior()[0] - 1 / (1 + np.exp(-3.0))) <= 0.01


# ---- 2. weighted cases against the yardstick, shared by several tests ----
CASES = [
    ("digits", r"\d{8}", ["20261020", "13579246", "5", "6"], [2, 2, 2, 0]),              # infeasible at T = 5 and 1
    ("alternation", r"(abc|de\d+)(xy)?|[gh]", ["de2026xy", "abcxy", "g", "h"], [2, 2, 2, 0]),
    ("cycle", r"(ab\d)+", ["ab1ab2ab3ab4ab5", "ab7", "7", "a"], [2, 2, 2, 0]),
    ("start_final", r"(\d\d)*", ["2026102013", "", "", ""], [2, 2, 2, 0]),
]


def weighted_case_pattern(ctc, codec, k, name, expr):
    rng = np.random.RandomState(1100 + k)
    if name == "cycle":                                        # per-label weights
        return ctc.Pattern.compile(expr, codec, label_weights=rng.uniform(-10, 10, C0).astype(np.float32))
    p = ctc.Pattern.compile(expr, codec)                       # per-arc and per-final weights within +-10
    return ctc.Pattern(p.arcs, p.finals, p.num_states, C0, weights=rng.uniform(-10, 10, len(p.arcs)),
                       final_weights=rng.uniform(-10, 10, len(p.finals)))


@pytest.fixture(scope="module")
def cases(recognizer, ctc, codec):
    out = {}
    for k, (name, expr, texts, leads) in enumerate(CASES):
        rng = np.random.RandomState(1010 + k)
        labels = [[codec.dict[ch] for ch in t] for t in texts]
        logits = np.stack([plant(rng, W0, C0, t, T, lead=n) for t, T, n in zip(labels, LENGTHS, leads)], axis=1)
        il = np.array(LENGTHS, np.int32)
        pat = weighted_case_pattern(ctc, codec, k, name, expr)
        t = tab(pat)
        out[name] = dict(expr=expr, logits=logits, il=il, pat=pat, tab=t, want=ref.run(logits, t, il),
                         got=recognizer(logits, pat, input_lengths=il))
    return out


def test_cases_against_float64(cases, recognizer, ctc):
    ctx = recognizer._context()
    for name, c in cases.items():
        reaches(c["pat"], 1, True, True)                       # S <= 1024, a few thousand edges: everything in LDS
        reaches(c["pat"], 1, True, True, full=False)
        got = c["got"]
        check_against(got, c["want"], c["tab"], c["pat"], c["logits"], c["il"], "cases " + name)
        have = np.isfinite(got.best_logp)
        nll = ctc.loss_logits(ctx, c["logits"], 0, np.concatenate(got.label_lists()).astype(np.int32), got.lengths, c["il"])
        assert have.any() and got.text_nll[have].tobytes() == nll[have].tobytes(), name
        assert np.isposinf(got.text_nll[~have]).all()
    assert cases["digits"]["want"][2][2] is None and cases["digits"]["want"][3][2] is None
    assert 0 in cases["start_final"]["pat"].tables()["accept"]
    assert (np.abs(np.concatenate([c["pat"].weights()["in_w"] for c in cases.values()])) <= 10).all()


# ---- 3. zero weights ----
def test_zero_weights_give_the_kind0_bits(cases, recognizer, ctc):
    for name, c in cases.items():
        p = c["pat"]
        zero = ctc.Pattern(p.arcs, p.finals, p.num_states, C0, weights=np.zeros(len(p.arcs)))
        plain = ctc.Pattern(p.arcs, p.finals, p.num_states, C0)
        assert (zero.kind, plain.kind) == (2, 0)
        a, b = recognizer(c["logits"], zero, input_lengths=c["il"]), recognizer(c["logits"], plain, input_lengths=c["il"])
        for f in FIELDS[:-1]:                                  # every output of the device call
            np.testing.assert_array_equal(getattr(a, f), getattr(b, f), err_msg="%s %s" % (name, f))
        have = np.isfinite(a.best_logp)
        assert not a.weights[have].any() and np.isnan(a.weights[~have]).all() and not b.weights.any()
        a1 = recognizer(c["logits"], zero, input_lengths=c["il"], full=False)
        b1 = recognizer(c["logits"], plain, input_lengths=c["il"], full=False)
        np.testing.assert_array_equal(a1.logp, b1.logp)
        np.testing.assert_array_equal(a1.logp, a.logp)
        assert a1.path is None and a1.weights is None


# ---- 4. tries with log priors as final weights: NPT = 2, 4, 8 ----
@pytest.mark.parametrize("nodes,npt,weights_lds", [(600, 2, True), (1500, 4, True), (3000, 8, False)])
def test_tries_with_priors(nodes, npt, weights_lds, recognizer, ctc):
    """tries of 630, 1511 and 3103 nodes (tests/test_gpu_pattern.py's): S = 1259, 3021, 6205. The edge lists fit in LDS;
    the largest's weights (6 bytes an edge with the list, 92 KB beside 99 KB of states) are read through L2 in the full
    call and staged in the forward-only one."""
    rng = np.random.RandomState(820 + nodes)
    texts = [[5, 6, 5, 7, 7, 8], [9, 10, 11]]
    es = set(tuple(t) for t in texts)
    while True:
        es.update(tuple(int(v) for v in rng.randint(1, C0, size=rng.randint(2, 7))) for _ in range(nodes // 50))
        arcs, finals, nq = pattern_ref.trie(sorted(es))
        if nq >= nodes:
            break
    es = [list(e) for e in sorted(es)]
    assert nq == {600: 630, 1500: 1511, 3000: 3103}[nodes]
    prior = np.log(np.random.RandomState(nodes).dirichlet(np.ones(len(es)))).astype(np.float32)
    d = {(p, c): q for p, c, q in arcs}
    at = {}
    for i, e in enumerate(es):
        v = 0
        for c in e:
            v = d[(v, c)]
        at[v] = i
    pat = ctc.Pattern(arcs, finals, nq, C0, final_weights=[prior[at[f]] for f in finals])
    reaches(pat, npt, True, weights_lds)
    reaches(pat, npt, True, True, full=False)
    logits = np.stack([plant(rng, W0, C0, texts[0]), plant(rng, W0, C0, texts[1], T=40)], axis=1)
    il = np.array([W0, 40], np.int32)
    got = recognizer(logits, pat, input_lengths=il)
    t = tab(pat)
    want = ref.run(logits, t, il)
    check_against(got, want, t, pat, logits, il, "trie %d" % nq)
    lex = ctc.lexicon_logits(recognizer._context(), logits, 0, ctc.Lexicon(es, num_classes=C0, priors=prior), 1, il, True)
    total = [lexicon_ref.logsumexp(lex.scores[b].astype(np.float64) + prior.astype(np.float64)) for b in range(2)]
    _check_scores(got.logp, total, "trie %d: logp against the lexicon's scores + priors" % nq)
    for b in range(2):
        assert got.label_lists()[b].tolist() == texts[b] == es[lex.entries[b, 0]], b
    only = recognizer(logits, pat, input_lengths=il, full=False)
    assert only.logp.tobytes() == got.logp.tobytes()


# ---- 5. bigrams ----
def test_bigram_of_ten_labels(recognizer, ctc):
    rng = np.random.RandomState(1200)
    n = 10
    pat = ctc.Pattern.bigram(np.arange(1, n + 1), rng.randn(n, n) * 2, rng.randn(n) * 2, rng.randn(n) * 2, num_classes=C0)
    assert pat.info()["states"] == 21 and pat.info()["edges"] == 231
    reaches(pat, 1, True, True)
    texts = [[2, 1, 2, 6, 1, 10, 2, 3], [4, 5, 5, 4], [7], [9]]
    logits = np.stack([plant(rng, W0, C0, t, T, lead=n) for t, T, n in zip(texts, LENGTHS, [2, 2, 2, 0])], axis=1)
    il = np.array(LENGTHS, np.int32)
    t = tab(pat)
    check_against(recognizer(logits, pat, input_lengths=il), ref.run(logits, t, il), t, pat, logits, il, "bigram 10")


def test_bigram_at_the_edge_limit(recognizer, ctc):
    """n = 361 on C = 400: 261 726 edges, S = 723; edges and weights through L2"""
    rng = np.random.RandomState(1201)
    n, C, W = 361, 400, 32
    pat = ctc.Pattern.bigram(np.arange(1, n + 1), rng.randn(n, n) * 2, rng.randn(n) * 2, rng.randn(n) * 2, num_classes=C)
    assert pat.info()["states"] == 723 and pat.info()["edges"] == 2 * n * n + 3 * n + 1 <= pattern_ref.MAX_EDGES
    reaches(pat, 1, False, False)
    reaches(pat, 1, False, False, full=False)
    texts = [[17, 360, 5, 5, 212, 90, 1, 361], [300, 2, 300]]
    il = np.array([W, 21], np.int32)
    logits = np.stack([plant(rng, W, C, t, T) for t, T in zip(texts, il)], axis=1)
    # the yardstick's recursion over the exported tables and weights (tests/test_pattern_w_host.py holds them to the
    # yardstick's own builder, which takes seconds at this size); nothing is pruned, so the arcs keep their numbers
    assert pat.info()["dfa_states"] == pat.num_states
    t = dict(pat.tables(), **pat.weights())
    t["arc_w"] = {(int(p), int(c)): (int(q), w) for (p, c, q), w in zip(pat.arcs, pat.weights_given)}
    t["final_w"] = {int(f): w for f, w in zip(pat.finals, pat.final_weights_given)}
    got = recognizer(logits, pat, input_lengths=il)
    check_against(got, ref.run(logits, t, il), t, pat, logits, il, "bigram 361")
    assert recognizer(logits, pat, input_lengths=il, full=False).logp.tobytes() == got.logp.tobytes()


# ---- 6. the flagship's logits shape ----
def test_workload_shape_with_a_character_bonus(recognizer, ctc):
    rng = np.random.RandomState(1300)
    C, W = 7358, 2000
    digit = list(range(1, 11))
    arcs = [(i, c, i + 1) for i in range(18) for c in digit]
    pat = ctc.Pattern(arcs, [18], 19, C, weights=np.full(len(arcs), 1.0))
    reaches(pat, 1, True, True)
    texts = [[1 + (7 * i) % 10 for i in range(18)], [3, 1, 3, 7, 11, 2, 1, 12, 3, 1, 13],
             [int(v) for v in rng.randint(1, C, size=300)], [1 + (3 * i) % 10 for i in range(18)]]
    T = [W, 1500, W, 700]
    logits = np.stack([plant(rng, W, C, t, n) for t, n in zip(texts, T)], axis=1)
    il = np.array(T, np.int32)
    t = tab(pat)
    want = ref.run(logits, t, il)
    got = recognizer(torch.from_numpy(logits).cuda(0), pat, input_lengths=il)
    check_against(got, want, t, pat, logits, il, "workload", paths=False)
    for b in (0, 3):                                           # the planted lines
        assert got.label_lists()[b].tolist() == texts[b] and got.weights[b] == 18.0
        assert got.path[b, :T[b]].tolist() == want[b][2]


# ---- 7. bit identity ----
def test_bit_identity(cases, recognizer, pkg):
    lib = pkg.load_library()
    for name, c in cases.items():
        logits, il, pat, base = c["logits"], c["il"], c["pat"], c["got"]
        call = lambda x, le=il, **kw: recognizer(x, pat, input_lengths=le, **kw)
        _same_bits(base, call(logits), name + ": repeated call")
        _same_bits(base, call(torch.from_numpy(logits).cuda(0), le=torch.from_numpy(il)), name + ": device pointer")
        i = pat.info()
        assert lib.hctr_pattern_group_lines(i["states"], i["classes"] + 1, W0) >= 4
        os.environ["HCTR_PAT_LINES"] = "1"
        try:
            _same_bits(base, call(logits), name + ": groups of one line")
        finally:
            del os.environ["HCTR_PAT_LINES"]
        for b in (1, 2):
            alone = call(np.ascontiguousarray(logits[:, b:b + 1]), le=il[b:b + 1])
            for f in FIELDS:
                assert getattr(alone, f)[0].tobytes() == getattr(base, f)[b].tobytes(), (name, b, f)
        only = call(logits, full=False)
        assert only.logp.tobytes() == base.logp.tobytes() and only.path is None, name


# ---- 8. the image path ----
def test_image_path_equals_logits_path(pkg, synth, m_trained, ctc):
    """hctr_pattern(images) == hctr_pattern_logits(the engine's f16x3 logits), also with the batch split into internal
    passes; priors as final weights make a line's own greedy text lose to its one-character prefix where they say so"""
    C, W = synth.DEFAULT_VOCAB + 2, 160
    imgs = synth.make_font_lines(3, W, 40 + W)
    widths = np.array([W, W - 29, W - 50], np.int32)
    labels = m_trained.greedy(imgs, widths=widths)
    assert all(len(v) >= 2 for v in labels)
    rng = np.random.RandomState(1400)
    es = sorted(set([tuple(int(c) for c in v) for v in labels] + [(int(labels[0][0]),), (C - 2, C - 3)] +
                    [tuple(int(v) for v in rng.randint(1, C, size=rng.randint(1, 6))) for _ in range(200)]))
    arcs, finals, nq = pattern_ref.trie(es)
    pat = ctc.Pattern(arcs, finals, nq, C, weights=rng.uniform(-3, 3, len(arcs)), final_weights=rng.uniform(-3, 3, len(finals)))
    reaches(pat, 2 if pat.info()["states"] > 1024 else 1, True, True)          # about a thousand states, 3 edges each
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
    _same_bits(fused, unfused, "logits path")
    _same_bits(fused, small.pattern(imgs, pat, widths=widths), "split passes")
    assert np.isfinite(fused.logp).all() and np.isfinite(fused.text_nll).all() and np.isfinite(fused.weights).all()
    t = tab(pat)
    z = logits.cpu().numpy() if hasattr(logits, "cpu") else np.asarray(logits)
    check_against(fused, ref.run(z, t), t, pat, z, [z.shape[0]] * 3, "image path", paths=False)
    assert m_trained.pattern(imgs, pat, widths=widths, full=False).logp.tobytes() == fused.logp.tobytes()


# ---- 9. masked and non-finite logits ----
def masked_patterns(ctc, case):
    out = {}
    for k, (name, (arcs, finals, nq)) in enumerate(sorted(mc.patterns(case).items())):
        rng = np.random.RandomState(1500 + k)
        out[name] = ctc.Pattern(arcs, finals, nq, mc.C, weights=rng.uniform(-4, 4, len(arcs)),
                                final_weights=rng.uniform(-4, 4, len(finals)))
    return out


@pytest.mark.parametrize("name", ["vocab", "columns", "single", "infeasible", "single5", "infeasible5"])
def test_masked_logits(name, recognizer, ctc):
    c, _ = mc.get(name)
    logits, il = c["logits"], c["il"]
    none = 0
    for pname, pat in masked_patterns(ctc, c).items():
        reaches(pat, 1, True, True)
        t = tab(pat)
        want = ref.run(logits, t, il)
        got = recognizer(logits, pat, input_lengths=il)
        check_against(got, want, t, pat, logits, il, "masked %s %s" % (name, pname))
        none += sum(w[2] is None for w in want)
        dev = recognizer(torch.from_numpy(logits).cuda(0), pat, input_lengths=il)
        _same_bits(got, dev, "masked %s %s: device pointer" % (name, pname))
    assert none >= 1 or name != "vocab"                        # the literal through a masked class has no path there


@pytest.mark.parametrize("kind", mc.POISON_KINDS)
def test_non_finite_rows(kind, recognizer, ctc):
    """a NaN, a +inf or a row of nothing but -inf on line 1: HCTR_OK, the other lines' bits untouched, no finite score on
    the bad line, its integers in range; in a row >= T nothing is read"""
    clean_case, _ = mc.get("poison_clean")
    c, _ = mc.get("poison_" + kind)
    late = kind.startswith("late_")
    T = int(c["il"][1])
    for pname, pat in masked_patterns(ctc, clean_case).items():
        clean = recognizer(clean_case["logits"], pat, input_lengths=clean_case["il"])
        bad = recognizer(c["logits"], pat, input_lengths=c["il"])
        for f in FIELDS:
            for b in (0, 2) + ((1,) if late else ()):
                assert np.ascontiguousarray(getattr(bad, f)[b]).tobytes() == np.ascontiguousarray(getattr(clean, f)[b]).tobytes(), \
                    (kind, pname, f, b)
        if not late:
            for f in ("logp", "best_logp", "text_nll", "weights"):
                assert not np.isfinite(np.float64(getattr(bad, f)[1])), (kind, pname, f)
            assert -1 <= bad.path[1].min() and bad.path[1].max() <= mc.C - 1
            assert 0 <= bad.labels[1].min() and bad.labels[1].max() <= mc.C - 1 and 0 <= bad.lengths[1] <= T
            assert 0 <= bad.starts[1].min() and bad.ends[1].max() <= T
        _same_bits(clean, recognizer(clean_case["logits"], pat, input_lengths=clean_case["il"]), "usable after " + kind)


# ---- 10. caching ----
def test_caching_and_side_effects(pkg, ctc, codec, synth, m_trained):
    rng = np.random.RandomState(1600)
    W, B, C = 90, 3, 40
    logits = rng.standard_normal((W, B, C)).astype(np.float32)
    targets = rng.randint(1, C, size=32).astype(np.int32)
    tl = np.array([7, 0, 25], np.int32)
    imgs = synth.make_font_lines(3, 96, 31)
    ctx = m_trained._ctx
    es = [[int(v) for v in rng.randint(1, C, size=rng.randint(1, 8))] for _ in range(50)]
    lex = ctc.Lexicon(es, num_classes=C)
    arcs, finals, nq = pattern_ref.trie(es)
    plain = ctc.Pattern(arcs, finals, nq, C)
    cd40 = pkg.ctc_codec(CHARS[:C - 2])
    sets = ctc.Pattern.compile(".{1,3}", cd40, sets=True)
    assert (plain.kind, sets.kind) == (0, 1)

    def others():
        g = m_trained.greedy(imgs)
        nll = ctc.loss_logits(ctx, logits, 0, targets, tl, None)
        lx = ctc.lexicon_logits(ctx, logits, 0, lex, 5, None, True)
        p0 = ctc.pattern_logits(ctx, logits, 0, plain)
        p1 = ctc.pattern_logits(ctx, logits, 0, sets)
        return g, nll, lx, p0, p1

    g0, nll0, lx0, p00, p10 = others()
    # two weighted patterns with equal tables and different weights, alternated
    w1, w2 = rng.uniform(-5, 5, len(arcs)), rng.uniform(-5, 5, len(arcs))
    pa = ctc.Pattern(arcs, finals, nq, C, weights=w1)
    pb = ctc.Pattern(arcs, finals, nq, C, weights=w2, final_weights=rng.uniform(-5, 5, len(finals)))
    assert all(pa.tables()[k].tobytes() == pb.tables()[k].tobytes() for k in pa.tables())
    ta, tb = tab(pa), tab(pb)
    wa, wb = ref.run(logits, ta), ref.run(logits, tb)
    first = {}
    for rnd in range(2):
        for key, pat, t, want in (("a", pa, ta, wa), ("b", pb, tb, wb)):
            got = ctc.pattern_logits(ctx, logits, 0, pat)
            check_against(got, want, t, pat, logits, [W] * B, "alternated " + key, paths=False)
            if key in first:
                _same_bits(first[key], got, "alternated " + key)
            first[key] = got
    assert first["a"].logp.tobytes() != first["b"].logp.tobytes()
    m_trained.pattern(imgs, ctc.Pattern([(0, 5, 1)], [1], 2, synth.DEFAULT_VOCAB + 2, weights=[2.0]))
    g1, nll1, lx1, p01, p11 = others()
    for x, y in zip(g0, g1):
        np.testing.assert_array_equal(x, y)
    assert nll0.tobytes() == nll1.tobytes()
    for k in ("entries", "logp", "rank", "log_total", "count", "scores"):
        assert getattr(lx0, k).tobytes() == getattr(lx1, k).tobytes(), k
    _same_bits(p00, p01, "kind 0 after weighted calls")
    _same_bits(p10, p11, "set form after weighted calls")


# ---- 11. argument errors ----
def test_argument_errors(recognizer, ctc, codec, pkg):
    lib, ctx = pkg.load_library(), recognizer._context()
    vp = ctypes.c_void_p
    W, B, C = 8, 2, 6
    x = np.zeros((W, B, C), np.float32)
    pat = ctc.Pattern(*pattern_ref.literal([1, 2]), C, weights=[0.5, -0.5])
    other = ctc.Pattern(*pattern_ref.literal([1]), C + 1, weights=[1.0])
    logp = np.zeros(B, np.float32)

    def call(p, il=None, logits=x):
        return lib.hctr_pattern_logits(ctx, None if p is None else p._h, None if logits is None else logits.ctypes.data_as(vp),
                                       0, W, B, C, None if il is None else np.array(il, np.int32).ctypes.data_as(vp),
                                       logp.ctypes.data_as(vp), *([None] * 8))

    assert call(pat) == 0 and np.isfinite(logp).all()
    assert call(other) == -1 and b"classes" in lib.hctr_last_error(ctx)
    assert call(pat, il=[0, 8]) == -1 and call(pat, il=[8, 9]) == -1 and b"outside [1,8]" in lib.hctr_last_error(ctx)
    assert call(pat, logits=None) == -1
    with pytest.raises(ValueError):
        recognizer(x, pat, input_lengths=[8])
    with pytest.raises(ValueError):
        recognizer(x, other)
    with pytest.raises(ValueError, match="set form"):
        ctc.Pattern.compile("a+", codec, sets=True, label_weights=1.0)
    empty = recognizer(np.zeros((W, 0, C), np.float32), pat)
    assert empty.logp.shape == (0,) and empty.weights.shape == (0,)
    ok = recognizer(x, pat, input_lengths=[1, 8])          # the context is still usable
    assert np.isneginf(ok.logp[0]) and np.isnan(ok.weights[0]) and ok.weights[1] == 0.0
    assert ok.label_lists()[1].tolist() == [1, 2]
    assert lib.hctr_pattern_instance(0, 0, 1, 1) == -1 and lib.hctr_pattern_instance(100, 300000, 1, 1) == -1


def test_report_largest_differences():
    """(last) the largest |engine - float64| seen per group of cases, for DESIGN.md"""
    for k, (d, x) in sorted(WORST.items()):
        print("largest |d| %-40s %.3e at |x| = %.1f (the rule allows %.3e)" % (k, d, x, _tol(x)))
