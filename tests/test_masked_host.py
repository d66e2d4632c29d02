"""Host tests (no GPU) of the masked-logits cases of tests/masked_cases.py: before the engine is measured against the
float64 yardsticks on logits that hold -inf, the yardsticks are checked against each other, against torch and against
enumeration of all paths on the same inputs, and the gradient oracle is shown to be usable there.

  * loss: recognize_ref.ctc_nll64 == torch's float64 ctc_loss on log_softmax64(z), +inf on the same lines;
  * a literal pattern's logp, a lexicon entry's score == -nll of that text; containment >= the segment and >= -nll;
  * W = 5: every path of 12^5 visited: the `infeasible` lines have none, the `single` lines' best path is the yardstick's;
  * ctc_align_ref.viterbi returns -1 paths exactly on the lines whose loss is +inf, and a finite best path never visits a
    masked cell;
  * the gradient oracle is torch's CPU ctc_loss with the LOG-PROBS as the leaf (differentiating through log_softmax
    gives NaN everywhere once a logit is -inf): its NaNs lie exactly on the masked entries of lines that have an
    alignment, lines without one get zeros, the float64 rows sum to 0 over the unmasked entries;
  * preconditions that give the GPU tests' tolerances their meaning: every finite score is above -200, a `columns` line's
    best path differs from the planted one, every line meant to have an alignment has a finite loss.
"""
import numpy as np
import pytest

import ctc_align_ref as align_ref
import masked_cases as mc
import pattern_ref
import recognize_ref
import spot_ref

NAMES = ["vocab", "columns", "single", "infeasible", "ladder", "single5", "infeasible5"]
TOL = 1e-9                                         # float64 against float64, |x| < 200


def _same(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert not np.isnan(a).any() and not np.isnan(b).any(), what
    np.testing.assert_array_equal(np.isinf(a), np.isinf(b), err_msg=what)
    np.testing.assert_array_equal(a[np.isinf(a)], b[np.isinf(b)], err_msg=what)
    fin = np.isfinite(a)
    assert (np.abs(a[fin] - b[fin]) <= TOL * (1 + np.abs(b[fin]))).all(), (what, a, b)


def _lp(c, b):
    return align_ref.log_softmax64(c["logits"][:int(c["il"][b]), b])


@pytest.mark.parametrize("name", NAMES)
def test_yardsticks_agree(name):
    c, o = mc.get(name)
    B = len(c["lines"])
    _same(o["nll"], mc.torch_nll64(c), name + ": ctc_nll64 against torch")
    assert np.flatnonzero(np.isposinf(o["nll"])).tolist() == c["no_path"], (name, o["nll"])
    if "lex" not in o:                                        # (the ladder: loss, gradient and alignment only)
        return
    text = [t for t in c["lines"] if t][0]
    for pname, t in (("literal", text), ("masked_literal", [text[0], 9, text[-1]])):
        want = [-recognize_ref.ctc_nll64(_lp(c, b), t) for b in range(B)]
        _same([w[0] for w in o["pat"][pname]], want, "%s: %s pattern against the loss" % (name, pname))
    for b in range(B):
        want = [-recognize_ref.ctc_nll64(_lp(c, b), e) for e in o["entries"]]
        _same(o["lex"][b], want, "%s line %d: lexicon against the loss" % (name, b))
        _same(o["pat"]["union"][b][0], pattern_ref.logsumexp(o["lex"][b]), "%s line %d: union against the lexicon" % (name, b))
    contain, seg, st, en = o["spot"]
    assert not np.isnan(contain).any() and not np.isnan(seg).any()
    assert (contain >= seg - TOL).all() and (contain <= TOL).all(), name
    for b, t in enumerate(c["lines"]):
        for k, q in enumerate(o["queries"]):
            if spot_ref._contains(t, q):
                assert contain[b, k] >= -o["nll"][b] - TOL, (name, b, k)
            if np.isfinite(seg[b, k]):
                lp = _lp(c, b)
                assert abs(spot_ref.segment_score(lp, q, st[b, k], en[b, k]) - seg[b, k]) <= TOL * (1 + abs(seg[b, k]))
            else:
                assert (st[b, k], en[b, k]) == (-1, -1)
    for pname, per_line in o["pat"].items():
        for b, (logp, best, path) in enumerate(per_line):
            assert best <= logp + TOL and logp <= TOL, (name, pname, b)
            assert (path is None) == np.isneginf(best), (name, pname, b)
    # the best reading of "one or more live labels" on a line that has an alignment scores at least the forced alignment
    for b, a in enumerate(o["align"]):
        if c["lines"][b] and np.isfinite(a["score"]) and all(v in mc.LIVE for v in c["lines"][b]):
            assert o["pat"]["live_plus"][b][1] >= a["score"] - TOL, (name, b)


@pytest.mark.parametrize("name", NAMES)
def test_viterbi_on_masked_logits(name):
    c, o = mc.get(name)
    moved = 0
    for b, a in enumerate(o["align"]):
        T, L = int(c["il"][b]), len(c["lines"][b])
        if np.isposinf(o["nll"][b]):
            assert a["states"] is None and np.isneginf(a["score"]) and (a["path"] == -1).all(), (name, b)
            assert (a["starts"] == -1).all() and (a["ends"] == -1).all() and np.isneginf(a["logps"]).all()
            continue
        assert np.isfinite(a["score"]) and a["score"] <= -o["nll"][b] + TOL, (name, b)
        path = a["path"]
        assert align_ref.collapse(path).tolist() == c["lines"][b], (name, b)
        assert not c["mask"][np.arange(T), b, path].any(), "%s line %d: the best path visits a masked cell" % (name, b)
        assert abs(align_ref.path_score64(a["lp64"], path) - a["score"]) <= TOL * (1 + abs(a["score"]))
        assert (a["starts"] >= 0).all() and (a["ends"] > a["starts"]).all() and len(a["starts"]) == L
        moved += path.tolist() != c["paths"][b]
    if name == "columns":
        assert moved >= 1, "no best path of `columns` had to leave the planted one"
    if name.startswith("single"):
        for b, rows in enumerate(c["single_rows"]):
            lp = o["align"][b]["lp64"]
            for t in rows:
                k = c["paths"][b][t]
                assert lp[t, k] == 0.0 and np.isneginf(np.delete(lp[t], k)).all() and o["align"][b]["path"][t] == k


@pytest.mark.parametrize("name", ["single5", "infeasible5"])
def test_every_path_at_five_columns(name):
    c, o = mc.get(name)
    paths = mc.flat_paths(5)
    assert paths.shape == (mc.C ** 5, 5)
    text = mc.collapse_all(paths)
    for b, t in enumerate(c["lines"]):
        lp = _lp(c, b)
        score = lp[np.arange(5), paths].sum(axis=1)
        hit = (text == np.array(t + [0] * (5 - len(t)))).all(axis=1)
        assert hit.sum() > 0                                  # L + repeats <= T: the length test admits the line
        total = pattern_ref.logsumexp(score[hit])
        _same(-o["nll"][b], total, "%s line %d: the loss against every path" % (name, b))
        a = o["align"][b]
        if b in c["no_path"]:
            assert np.isneginf(score[hit]).all() and a["states"] is None, (name, b)
            continue
        best = score[hit].max()
        winners = paths[hit][score[hit] == best]
        assert abs(best - a["score"]) <= TOL * (1 + abs(best)) and len(winners) == 1, (name, b)
        assert winners[0].tolist() == a["path"].tolist(), (name, b)
    if name == "infeasible5":
        assert c["no_path"] == [0, 1] and c["lines"][0] == [1, 1] and c["mask"][1:4, 0, 0].all()


@pytest.mark.parametrize("name", NAMES)
def test_gradient_oracle(name):
    c, o = mc.get(name)
    g64, g32 = mc.torch_grads(c)
    Wc, B, _ = c["logits"].shape
    worst = 0.0
    for b in range(B):
        T = int(c["il"][b])
        assert not g64[T:, b].any() and not g32[T:, b].any(), (name, b)
        if b in c["no_path"]:
            assert not g64[:, b].any() and not g32[:, b].any(), "%s line %d: no alignment, zero_infinity" % (name, b)
            continue
        m = c["mask"][:T, b]
        np.testing.assert_array_equal(np.isnan(g64[:T, b]), m, err_msg="%s line %d float64" % (name, b))
        np.testing.assert_array_equal(np.isnan(g32[:T, b]), m, err_msg="%s line %d float32" % (name, b))
        rows = np.where(m, 0.0, g64[:T, b]).sum(axis=1)
        worst = max(worst, float(np.abs(rows).max()))
        e32 = float(np.abs(np.where(m, 0.0, g32[:T, b] - g64[:T, b])).max())
        assert e32 < 1e-3, (name, b, e32)
    print("%s: largest |row sum| of the float64 gradient over the unmasked entries %.2e" % (name, worst))
    assert worst <= 1e-11, (name, worst)                    # float64 rounding of <= 12 terms of magnitude <= 1


@pytest.mark.parametrize("name", NAMES)
def test_scores_are_in_the_tolerances_range(name):
    c, o = mc.get(name)
    vals = [-o["nll"], [a["score"] for a in o["align"]], np.concatenate([a["logps"] for a in o["align"]])]
    if "lex" in o:
        vals += [o["spot"][0], o["spot"][1], o["lex"]]
    for per_line in o.get("pat", {}).values():
        vals += [[w[0] for w in per_line], [w[1] for w in per_line]]
    v = np.concatenate([np.asarray(x, np.float64).reshape(-1) for x in vals])
    assert not np.isnan(v).any() and not np.isposinf(v).any()
    fin = v[np.isfinite(v)]
    print("%s: %d finite scores, the lowest %.1f; %d are -inf" % (name, fin.size, fin.min(), int(np.isneginf(v).sum())))
    assert fin.min() > -200 and fin.max() <= TOL
    if name in ("vocab", "infeasible", "infeasible5"):
        assert np.isneginf(v).any()


def test_poison_cases_differ_in_one_row_only():
    clean, _ = mc.get("poison_clean")
    for kind in mc.POISON_KINDS:
        c, _ = mc.get("poison_" + kind)
        diff = np.argwhere(c["logits"].view(np.uint32) != clean["logits"].view(np.uint32))
        assert len(diff) and set(diff[:, 0]) == {c["bad_t"]} and set(diff[:, 1]) == {1}, kind
        assert (c["bad_t"] >= c["il"][1]) == kind.startswith("late_")
        row = c["logits"][c["bad_t"], 1].astype(np.float64)
        assert np.isnan(recognize_ref.lse64(row)), kind        # the definition of a non-finite row
