"""GPU tests (-m gpu) of the CTC entry points on masked (-inf) and non-finite logits: loss, gradient, forced alignment,
spotting, lexicon, pattern and greedy recognition on the cases of tests/masked_cases.py, whose float64 oracles
tests/test_masked_host.py checks against each other, torch and enumeration. The contract is in include/hctr_hip.h
("masked and non-finite logits") and DESIGN.md.

What must hold:
  * every score is within the family's rule, 1e-5 * |want| + 1e-3, of float64 on the same logits; -inf exactly where the
    oracle has it and NaN nowhere; paths, spans, segments, rankings and decoded labels are the oracle's;
  * a line whose every path has probability 0 gets the outputs of a line that fails the length test, entry by entry;
  * the gradient: on unmasked entries test_gpu_ctc_grad.py's rule, |w| * max(4 * e32, 2e-5), against torch's float64
    CPU gradient with the log-probs as the leaf (e32 from its float32 run); exactly 0 at a masked entry and on lines
    without an alignment; rows sum to 0 within C * 2e-5 * |w|; through ``CTCLoss`` under all three reductions;
  * the relations that tie the family together hold bit for bit under masks (lexicon score / pattern text_nll /
    recognition text_nll against the loss), the inequalities hold, a host pointer and a device tensor give the same bits;
  * the ladder: every instance of the recursion (one state per lane, two, two waves) hands a -inf on; a line's bits do
    not depend on the batch it is in;
  * a non-finite row (NaN, +inf, nothing but -inf): HCTR_OK, the other lines' bits untouched, no finite score on the
    bad line, every integer output in range, the context usable afterwards; a bad row at t >= T is never read.
"""
import importlib

import numpy as np
import pytest
import torch

import lexicon_ref
import masked_cases as mc
import pattern_ref
import recognize_ref

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-3                            # engine score vs float64 on the same logits (tests/test_gpu_ctc.py's)
FACTOR, FLOOR = 4.0, 2e-5                          # the gradient's rule (tests/test_gpu_ctc_grad.py's)
NAMES = ["vocab", "columns", "single", "infeasible", "ladder"]
WORST = {}                                         # entry -> (largest |got - want|, |want| there), printed by the tests


def _tol(want):
    return RTOL * np.abs(want) + ATOL


def _check_scores(got, want, what, key=None):
    """got within the rule of want where want is finite, -inf exactly where want is (test_gpu_pattern.py's)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got).any(), what
    fin = np.isfinite(want)
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want), err_msg="%s: -inf pattern" % what)
    np.testing.assert_array_equal(np.isposinf(got), np.isposinf(want), err_msg="%s: +inf pattern" % what)
    if fin.any():
        err = np.abs(got[fin] - want[fin])
        k = int(np.argmax(err))
        print("%s: %d finite, %d infinite, max |d| %.3e at want %.2f, worst excess over the rule %.3e"
              % (what, int(fin.sum()), int((~fin).sum()), float(err[k]), float(want[fin][k]),
                 float((err - _tol(want[fin])).max())))
        if key and err[k] >= WORST.get(key, (0.0, 0.0))[0]:
            WORST[key] = (float(err[k]), float(want[fin][k]))
        assert (err <= _tol(want[fin])).all(), what


@pytest.fixture(scope="module")
def ctc(pkg):
    return importlib.import_module(pkg.__name__ + ".ctc")


@pytest.fixture(scope="module")
def crit(pkg):
    return pkg.CTCLoss(reduction="none", zero_infinity=True).cuda(0)


@pytest.fixture(scope="module")
def ctx(crit):
    return crit._context()


_TABLES = {}


def _tables(ctc, name):
    """(Lexicon, {pattern name: Pattern}) of a case, built once"""
    if name not in _TABLES:
        c, _ = mc.get(name)
        _TABLES[name] = (ctc.Lexicon(mc.entries(c), num_classes=mc.C),
                         {k: ctc.Pattern(*d, mc.C) for k, d in mc.patterns(c).items()})
    return _TABLES[name]


def run_all(ctc, ctx, c, tables=None, logits=None, il=None, grad=True, rec=True):
    """every entry point on one case -> {output name: (array, layout)}; layout "B" = a line per leading index, "WBC",
    or "flat" (per target position, in the order of the targets). ``tables``: the case's (Lexicon, patterns), None for
    loss, gradient and alignment alone. ``logits``: a device tensor in place of the case's host array."""
    z = c["logits"] if logits is None else logits
    on_dev = int(logits is not None)
    il = c["il"] if il is None else il
    out = {"nll": (ctc.loss_logits(ctx, z, on_dev, c["targets"], c["tl"], il), "B")}
    if grad:
        nll, g = ctc.loss_grad_logits(ctx, z, on_dev, c["targets"], c["tl"], il, None)
        out["grad.nll"] = (nll, "B")
        out["grad"] = (g.cpu().numpy() if on_dev else g, "WBC")
    al = ctc.align_logits(ctx, z, on_dev, c["targets"], c["tl"], il)
    out.update({"align.paths": (al.paths, "B"), "align.scores": (al.scores, "B"), "align.starts": (al.starts, "flat"),
                "align.ends": (al.ends, "flat"), "align.logps": (al.logps, "flat")})
    if tables is not None:
        lex, pats = tables
        sp = ctc.spot_logits(ctx, z, on_dev, mc.queries(c), il)
        out.update({"spot." + k: (getattr(sp, k), "B") for k in ("logp", "seg_logp", "starts", "ends")})
        lx = ctc.lexicon_logits(ctx, z, on_dev, lex, len(lex), il, True)
        out.update({"lex." + k: (getattr(lx, k), "B") for k in ("entries", "logp", "rank", "log_total", "count", "scores")})
        for name, p in pats.items():
            r = ctc.pattern_logits(ctx, z, on_dev, p, il)
            out.update({"pat.%s.%s" % (name, f): (getattr(r, f), "B") for f in r.FIELDS})
    if rec:
        r = ctc.recognize_logits(ctx, z, on_dev)
        out.update({"rec." + k: (getattr(r, k), "B") for k in ("labels", "lengths", "starts", "ends", "logps", "alt_labels",
                                                               "alt_logps", "path_logp", "text_nll")})
    return out


def _line(res, key, b, c):
    a, layout = res[key]
    if layout == "B":
        return np.ascontiguousarray(a[b])
    if layout == "WBC":
        return np.ascontiguousarray(a[:, b])
    off = np.concatenate([[0], np.cumsum(c["tl"])])
    return np.ascontiguousarray(a[off[b]:off[b + 1]])


_RESULTS = {}


@pytest.fixture(scope="module")
def results(ctc, ctx):
    def get(name):
        if name not in _RESULTS:
            c, _ = mc.get(name)
            _RESULTS[name] = run_all(ctc, ctx, c, None if name == "ladder" else _tables(ctc, name))
        return _RESULTS[name]
    return get


def _pad(path, Wc):
    return list(path) + [-1] * (Wc - len(path))


def check_scores_against_float64(name, r):
    """the scores, paths, spans, rankings and decoded labels of `r`, a ``run_all`` result of the case `name`, against the
    case's float64 oracle (also what tests/test_gpu_history.py holds its first-call results to)"""
    c, o = mc.get(name)
    Wc, B, _ = c["logits"].shape
    _check_scores(r["nll"][0], o["nll"], name + " loss", "loss")
    assert r["grad.nll"][0].tobytes() == r["nll"][0].tobytes()
    _check_scores(r["align.scores"][0], [a["score"] for a in o["align"]], name + " alignment score", "alignment score")
    _check_scores(r["align.logps"][0], np.concatenate([a["logps"] for a in o["align"]]), name + " span_logp", "span_logp")
    for b, a in enumerate(o["align"]):
        assert r["align.paths"][0][b].tolist() == _pad(a["path"], Wc), "%s line %d: alignment path" % (name, b)
        assert _line(r, "align.starts", b, c).tolist() == a["starts"].tolist(), (name, b)
        assert _line(r, "align.ends", b, c).tolist() == a["ends"].tolist(), (name, b)
    if name == "ladder":
        return
    contain, seg, st, en = o["spot"]
    _check_scores(r["spot.logp"][0], contain, name + " containment", "containment")
    _check_scores(r["spot.seg_logp"][0], seg, name + " segment", "segment")
    np.testing.assert_array_equal(r["spot.starts"][0], st, err_msg=name + " seg_start")
    np.testing.assert_array_equal(r["spot.ends"][0], en, err_msg=name + " seg_end")
    _check_scores(r["lex.scores"][0], o["lex"], name + " lexicon scores", "lexicon score")
    n = len(o["entries"])
    for b in range(B):
        top, tr, total, count = lexicon_ref.rank(o["lex"][b], None, n)
        assert r["lex.entries"][0][b].tolist() == top.tolist(), "%s line %d: ranking" % (name, b)
        assert int(r["lex.count"][0][b]) == count == int(np.isfinite(o["lex"][b]).sum())
        _check_scores(r["lex.logp"][0][b], tr, "%s line %d lexicon top logp" % (name, b), "lexicon score")
        _check_scores(r["lex.log_total"][0][b], total, "%s line %d lexicon log_total" % (name, b), "lexicon log_total")
    for pname, want in o["pat"].items():
        key = "pat.%s." % pname
        _check_scores(r[key + "logp"][0], [w[0] for w in want], "%s pattern %s logp" % (name, pname), "pattern logp")
        _check_scores(r[key + "best_logp"][0], [w[1] for w in want], "%s pattern %s best_logp" % (name, pname),
                      "pattern best_logp")
        for b, w in enumerate(want):
            path = r[key + "path"][0][b]
            if w[2] is None:
                assert (path == -1).all() and r[key + "lengths"][0][b] == 0 and np.isposinf(r[key + "text_nll"][0][b])
                continue
            assert path.tolist() == _pad(w[2], Wc), "%s pattern %s line %d: path" % (name, pname, b)
            labels, st, en, _ = pattern_ref.spans(w[2], np.zeros((len(w[2]), mc.C)))
            L = int(r[key + "lengths"][0][b])
            assert r[key + "labels"][0][b, :L].tolist() == labels and r[key + "starts"][0][b, :L].tolist() == st
            assert r[key + "ends"][0][b, :L].tolist() == en
    want = recognize_ref.recognize_ref(c["logits"])
    np.testing.assert_array_equal(r["rec.lengths"][0], want["lengths"])
    for k in ("labels", "starts", "ends", "alt_labels"):
        np.testing.assert_array_equal(r["rec." + k][0], want[k], err_msg="%s recognition %s" % (name, k))
    _check_scores(r["rec.path_logp"][0], want["path_logp"], name + " recognition path_logp", "recognition path_logp")
    _check_scores(r["rec.text_nll"][0], want["text_nll"], name + " recognition text_nll", "recognition text_nll")
    _check_scores(r["rec.logps"][0], want["logps"], name + " recognition logps", "recognition char logp")
    _check_scores(r["rec.alt_logps"][0], want["alt_logps"], name + " recognition alt_logps", "recognition alt logp")
    if name == "single":
        for b, rows in enumerate(c["single_rows"]):
            for t in rows:
                k = c["paths"][b][t]
                assert r["align.paths"][0][b, t] == k, (b, t)
                assert b != 0 or r["pat.literal.path"][0][0, t] == k, t      # (the literal is line 0's text)
        lp = np.float64(r["rec.alt_logps"][0])
        assert np.isneginf(lp).any(), "no runner-up of a single-class row was reported"
    print("largest errors so far:", {k: "%.3e at %.2f" % v for k, v in sorted(WORST.items())})


@pytest.mark.parametrize("name", NAMES)
def test_scores_against_float64(name, results):
    check_scores_against_float64(name, results(name))


def test_no_alignment_outputs(results):
    """entry by entry: a line whose every path has probability 0 gets what a line that fails the length test gets"""
    for name in ("vocab", "infeasible"):
        c, o = mc.get(name)
        r = results(name)
        Wc = c["logits"].shape[0]
        assert c["no_path"] and all(len(c["lines"][b]) + 1 <= c["il"][b] for b in c["no_path"])
        for b in c["no_path"]:
            what = "%s line %d" % (name, b)
            L = len(c["lines"][b])
            assert np.isposinf(r["nll"][0][b]) and np.isposinf(r["grad.nll"][0][b]), what
            assert not _line(r, "grad", b, c).any(), what + ": gradient rows"
            assert np.isneginf(r["align.scores"][0][b]), what + ": alignment score"
            assert r["align.paths"][0][b].tolist() == [-1] * Wc, what + ": alignment path"
            assert _line(r, "align.starts", b, c).tolist() == [-1] * L == _line(r, "align.ends", b, c).tolist(), what
            assert np.isneginf(_line(r, "align.logps", b, c)).all() and L > 0, what
        # spotting, the lexicon and the pattern: (line, query / entry / pattern) pairs without a path
        pairs = [(b, 4) for b in range(len(c["lines"]))] if name == "vocab" else [(0, 0)]
        for b, k in pairs:
            assert np.isneginf(o["spot"][0][b, k]), "the case no longer has the pair"
            got = [r["spot." + f][0][b, k] for f in ("logp", "seg_logp", "starts", "ends")]
            assert np.isneginf(got[0]) and np.isneginf(got[1]) and got[2] == -1 and got[3] == -1, (name, b, k, got)
        dead = np.isneginf(o["lex"])
        assert dead.any() and np.isneginf(r["lex.scores"][0][dead]).all()
        for b in range(len(c["lines"])):
            listed = r["lex.entries"][0][b]
            listed = set(listed[listed >= 0].tolist())
            assert listed == set(np.flatnonzero(~dead[b]).tolist()), "%s line %d: -inf entries are left out" % (name, b)
        pname = "masked_literal" if name == "vocab" else "literal"
        for b, w in enumerate(o["pat"][pname]):
            if w[2] is not None:
                continue
            key = "pat.%s." % pname
            assert np.isneginf(r[key + "logp"][0][b]) and np.isneginf(r[key + "best_logp"][0][b]), (name, b)
            assert (r[key + "path"][0][b] == -1).all() and r[key + "lengths"][0][b] == 0
            assert np.isposinf(r[key + "text_nll"][0][b])
        assert any(w[2] is None for w in o["pat"][pname])


def _check_grad(got, c, g64, g32, w, what):
    """the module docstring's gradient rule, line by line"""
    Wc, B, Cc = c["logits"].shape
    got = np.asarray(got, np.float64)
    assert not np.isnan(got).any(), what
    for b in range(B):
        T = int(c["il"][b])
        assert not got[T:, b].any(), (what, b)
        if b in c["no_path"]:
            assert not got[:, b].any(), "%s line %d: no alignment, yet a gradient" % (what, b)
            continue
        m = c["mask"][:T, b]
        assert (got[:T, b][m] == 0).all(), "%s line %d: a masked entry's gradient is not exactly 0" % (what, b)
        e32 = float(np.abs((g32[:T, b] - g64[:T, b])[~m]).max())
        err = float(np.abs((got[:T, b] - w[b] * g64[:T, b])[~m]).max())
        lim = abs(w[b]) * max(FACTOR * e32, FLOOR)
        rows = float(np.abs(got[:T, b].sum(axis=1)).max())
        print("%s line %d: err %.3e, e32 %.3e, limit %.3e, largest |row sum| %.3e, weight %g" % (what, b, err, e32, lim, rows, w[b]))
        if w[b] == 1.0 and err >= WORST.get("gradient", (0.0, 0.0))[0]:
            WORST["gradient"] = (err, e32)
        assert err <= lim, (what, b, err, e32, lim)
        assert rows <= Cc * 2e-5 * abs(w[b]), (what, b, rows)


@pytest.mark.parametrize("name", NAMES)
def test_gradient(name, results, crit):
    c, o = mc.get(name)
    r = results(name)
    g64, g32 = mc.torch_grads(c)
    B = len(c["lines"])
    _check_grad(r["grad"][0], c, g64, g32, np.ones(B), name + " C entry")
    if name == "columns":                                     # the blank is masked on column 1 of every line
        assert c["mask"][1, :, 0].all() and not r["grad"][0][1, :, 0].any()
    weights = {"none": np.ones(B), "sum": np.ones(B), "mean": 1.0 / (B * np.maximum(c["tl"], 1.0))}
    try:
        for red, w in weights.items():
            crit.reduction = red
            x = torch.from_numpy(c["logits"]).cuda(0).requires_grad_()
            loss = crit(x, c["targets"], c["il"], c["tl"])
            (loss.sum() if red == "none" else loss).backward()
            _check_grad(x.grad.cpu().numpy(), c, g64, g32, w, "%s CTCLoss(%s).backward()" % (name, red))
    finally:
        crit.reduction = "none"
    print("largest gradient error at weight 1 so far: %.3e (e32 %.3e)" % WORST["gradient"])


@pytest.mark.parametrize("name", ["vocab", "columns", "single", "infeasible"])
def test_relations_under_masks(name, results, ctc, ctx):
    c, o = mc.get(name)
    r = results(name)
    Wc, B, _ = c["logits"].shape
    z, il = c["logits"], c["il"]
    # a lexicon score has the bits of -nll of the loss with the entry as every line's target
    for e, entry in enumerate(o["entries"]):
        nll = ctc.loss_logits(ctx, z, 0, np.array(entry * B, np.int32), np.full(B, len(entry), np.int32), il)
        assert (-nll).tobytes() == np.ascontiguousarray(r["lex.scores"][0][:, e]).tobytes(), (name, entry)
    # text_nll of every pattern and of the recognition has the bits of the loss on the decoded labels
    for pname in o["pat"]:
        key = "pat.%s." % pname
        lengths, labels = r[key + "lengths"][0], r[key + "labels"][0]
        flat = np.concatenate([labels[b, :lengths[b]] for b in range(B)]).astype(np.int32)
        nll = ctc.loss_logits(ctx, z, 0, flat, lengths, il)
        have = np.isfinite(r[key + "best_logp"][0])
        assert r[key + "text_nll"][0][have].tobytes() == nll[have].tobytes(), (name, pname)
        assert np.isposinf(r[key + "text_nll"][0][~have]).all()
        lp, best = np.float64(r[key + "logp"][0]), np.float64(r[key + "best_logp"][0])
        assert (best <= lp).all() and (lp <= 0).all(), (name, pname)
        assert (-np.float64(nll[have]) <= lp[have] + 2 * _tol(lp[have])).all()
    lengths, labels = r["rec.lengths"][0], r["rec.labels"][0]
    flat = np.concatenate([labels[b, :lengths[b]] for b in range(B)]).astype(np.int32)
    assert r["rec.text_nll"][0].tobytes() == ctc.loss_logits(ctx, z, 0, flat, lengths, None).tobytes(), name
    # a literal pattern against the loss, a union of literals against the lexicon's total, by the rule
    text = [t for t in c["lines"] if t][0]
    nll = ctc.loss_logits(ctx, z, 0, np.array(text * B, np.int32), np.full(B, len(text), np.int32), il)
    _check_scores(r["pat.literal.logp"][0], -np.float64(nll), name + " literal pattern against the loss")
    _check_scores(r["pat.union.logp"][0], r["lex.log_total"][0], name + " union against the lexicon's total")
    # containment holds the segment and the line's own text
    contain, seg = np.float64(r["spot.logp"][0]), np.float64(r["spot.seg_logp"][0])
    assert (contain >= seg).all() and (contain <= 0).all(), name
    for b, t in enumerate(c["lines"]):
        for k, q in enumerate(o["queries"]):
            if any(t[i:i + len(q)] == q for i in range(len(t))):
                assert contain[b, k] >= -np.float64(r["nll"][0][b]) - 2 * ATOL, (name, b, k)
    # the same bits from a device tensor
    dev = run_all(ctc, ctx, c, _tables(ctc, name), logits=torch.from_numpy(z).cuda(0))
    for key in r:
        assert np.ascontiguousarray(dev[key][0]).tobytes() == np.ascontiguousarray(r[key][0]).tobytes(), (name, key)


def test_ladder_alone_equals_batched(results, ctc, ctx):
    c, o = mc.get("ladder")
    r = results("ladder")
    assert [2 * len(t) + 1 for t in c["lines"]] == [11, 81, 141]
    off = np.concatenate([[0], np.cumsum(c["tl"])])
    for b in range(3):
        one = dict(c, logits=np.ascontiguousarray(c["logits"][:, b:b + 1]), targets=c["targets"][off[b]:off[b + 1]],
                   tl=c["tl"][b:b + 1], il=c["il"][b:b + 1])
        alone = run_all(ctc, ctx, one, rec=False)
        for key in alone:
            assert _line(alone, key, 0, one).tobytes() == _line(r, key, b, c).tobytes(), "ladder line %d: %s" % (b, key)
        _check_scores(alone["nll"][0], o["nll"][b:b + 1], "ladder line %d alone: loss" % b)
        assert np.isfinite(alone["align.scores"][0]).all()


FLOATS_NOT_FINITE = ["nll", "grad.nll", "align.scores", "spot.logp", "lex.logp", "lex.rank", "lex.log_total", "lex.scores",
                     "rec.path_logp", "rec.text_nll"]


@pytest.mark.parametrize("kind", mc.POISON_KINDS)
def test_poison(kind, ctc, ctx):
    """every call returns HCTR_OK (``_lib.check`` raises otherwise)"""
    clean_case, _ = mc.get("poison_clean")
    c, _ = mc.get("poison_" + kind)
    tables = _tables(ctc, "poison_clean")
    if "poison_clean" not in _RESULTS:
        _RESULTS["poison_clean"] = run_all(ctc, ctx, clean_case, tables)
    clean = _RESULTS["poison_clean"]
    bad = run_all(ctc, ctx, c, tables)
    late = kind.startswith("late_")
    T, t_bad, Cc, Wc = int(c["il"][1]), c["bad_t"], mc.C, c["logits"].shape[0]
    for key in clean:
        for b in (0, 2):
            assert _line(bad, key, b, c).tobytes() == _line(clean, key, b, c).tobytes(), "%s: line %d %s moved" % (kind, b, key)
        if late and not key.startswith("rec."):                # (recognition reads all W columns: it has no lengths)
            assert _line(bad, key, 1, c).tobytes() == _line(clean, key, 1, c).tobytes(), "%s: row %d >= T was read: %s" % (kind, t_bad, key)
    line = {key: _line(bad, key, 1, c) for key in bad}
    names = FLOATS_NOT_FINITE if not late else ["rec.path_logp", "rec.text_nll"]
    names = names + ([] if late else [k for k in bad if k.startswith("pat.") and k.split(".")[2] in ("logp", "best_logp", "text_nll")])
    for key in names:
        assert not np.isfinite(np.asarray(line[key], np.float64)).any(), "%s: a finite %s on the bad line: %s" % (kind, key, line[key])
    print("%s, the bad line: " % kind + ", ".join("%s %s" % (k, np.unique(np.asarray(line[k], np.float64))) for k in names))
    if not late:
        # the gradient: zeros where the loss is +inf; where it is NaN, NaN in the bad row and at the line's own classes
        g = line["grad"]
        if np.isposinf(line["nll"]):
            assert not g.any(), kind
        else:
            own = sorted(set([0] + c["lines"][1]))
            assert np.isnan(g[t_bad]).all() and np.isnan(g[:T][:, own]).all() and not g[T:].any(), kind
        # the segment: the best among those that end before the bad row, bit for bit a call that stops there, or none
        short = ctc.spot_logits(ctx, c["logits"], 0, mc.queries(c), np.array([c["il"][0], t_bad, c["il"][2]], np.int32))
        for f in ("seg_logp", "starts", "ends"):
            assert line["spot." + f].tobytes() == np.ascontiguousarray(getattr(short, f)[1]).tobytes(), (kind, f)
        # a span that holds the bad row has no finite log-probability
        for j, (s, e) in enumerate(zip(line["align.starts"], line["align.ends"])):
            if s <= t_bad < e:
                assert not np.isfinite(line["align.logps"][j]), (kind, j)
    # every integer output of the bad line is in range
    N = len(tables[0])
    ranges = {"align.paths": (-1, Cc - 1), "align.starts": (-1, T), "align.ends": (-1, T), "spot.starts": (-1, T),
              "spot.ends": (-1, T), "lex.entries": (-1, N - 1), "lex.count": (0, N), "rec.labels": (0, Cc - 1),
              "rec.lengths": (0, Wc), "rec.starts": (0, Wc), "rec.ends": (0, Wc), "rec.alt_labels": (0, Cc - 1)}
    for key in bad:
        if key.startswith("pat."):
            f = key.split(".")[2]
            if f in ("path",):
                ranges[key] = (-1, Cc - 1)
            elif f in ("labels",):
                ranges[key] = (0, Cc - 1)
            elif f in ("lengths", "starts", "ends"):
                ranges[key] = (0, T)
    for key, (lo, hi) in ranges.items():
        v = line[key]
        assert v.dtype == np.int32 and v.size and lo <= v.min() and v.max() <= hi, (kind, key, v.min(), v.max())
    # the context is usable: the clean call again, the same bits
    again = run_all(ctc, ctx, clean_case, tables)
    for key in clean:
        assert np.ascontiguousarray(again[key][0]).tobytes() == np.ascontiguousarray(clean[key][0]).tobytes(), (kind, key)
