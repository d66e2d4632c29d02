"""Float64 oracle and checker of the beam front end (log-softmax, top-k, blank log-prob, p > 0.001 candidate lists),
plus a numpy emulation of the kernels' float32 arithmetic with switchable defects. Pure numpy, no GPU.

The oracle
----------
``reference(logits)`` is the log-softmax of the float32 inputs, taken as given, in float64: ``d = x - rowmax``,
``L = ln sum exp(d)``, ``lp = d - L``. A ``-inf`` input gives ``-inf``; every row needs one finite entry; NaN and
``+inf`` are outside the contract.

The tolerance
-------------
``tol = 2^-22 * max(1, |d| + |L|)`` per element. The kernels (csrc/kernels.hip ``row_topk_kernel``; the fused path
shares the arithmetic) compute ``lp = (x - max) - logf((float)sum)`` with ``sum`` the float64 sum of ``expf(x - max)``:

* ``x - max`` rounds to float32: at most 2^-24 |d| (exact when both are within a factor of two);
* each ``expf`` term is off by about an ulp (2^-23 relative) plus e^d * 2^-24 |d| from the rounded argument; the
  terms that matter have |d| of order one, so the sum is off by a few 2^-23 relative, ``(float)sum`` adds 2^-24, and
  the logarithm turns a relative error of the sum into the same absolute error of ``L``: a few 2^-23;
* ``logf`` is off by about an ulp of |L|: 2^-23 |L|;
* the last subtraction rounds to float32: 2^-24 (|d| + |L|).

Together about 2^-23 (|d| + |L|) with a floor of a few 2^-23 where |d| + |L| is small; the bound doubles the first
and covers the second with the ``max(1, .)``. The emulation below stays within 0.72 of it on C from 2 to 12288 and
logit scales from 0.01 to 1000.

What ``check_frontend`` asserts is listed in its docstring.
"""
import numpy as np

LN_THRESH = float(np.log(0.001))          # the candidate threshold, float64 like the engine's std::log(0.001)
EPS = 2.0 ** -22


def _split(logits_wbc):
    x = np.asarray(logits_wbc)
    assert x.dtype == np.float32 and x.ndim == 3, "logits are float32 [W,B,C]"
    assert not np.isnan(x).any() and not np.isposinf(x).any(), "NaN / +inf logits are outside the contract"
    x64 = x.astype(np.float64)
    mx = x64.max(axis=2, keepdims=True)
    assert np.isfinite(mx).all(), "every row needs a finite entry"
    d = x64 - mx
    L = np.log(np.exp(d).sum(axis=2, keepdims=True))
    return d, L


def reference(logits_wbc):
    """float64 log-softmax [W,B,C] of float32 logits."""
    d, L = _split(logits_wbc)
    return d - L


def tolerance(logits_wbc):
    """[W,B,C] float64: 2^-22 * max(1, |d| + |L|); 0 where the reference is -inf (the device must give -inf there)."""
    d, L = _split(logits_wbc)
    with np.errstate(invalid="ignore"):
        tol = EPS * np.maximum(1.0, np.abs(d) + np.abs(L))
    tol[np.isneginf(d)] = 0.0
    return tol


def _ranking(lp_row):
    """Classes by (lp64 descending, class ascending)."""
    return np.lexsort((np.arange(lp_row.size), -lp_row))


def _settled(lp_row, tol_row, order, k):
    """settled[j], j < k: ranks j and j+1 differ by more than the sum of their tolerances. The last one compares rank
    k-1 with rank k (the first class left out); with k == C there is no such class and the boundary is settled."""
    C = lp_row.size
    n = min(k + 1, C)
    v, t = lp_row[order[:n]], tol_row[order[:n]]
    with np.errstate(invalid="ignore"):
        gap = v[:-1] - v[1:]                      # -inf minus -inf is NaN: compares False, unsettled
        s = gap > t[:-1] + t[1:]
    if n == k:
        s = np.append(s, True)
    return s


def ambiguity(logits_wbc, k, want_candidates):
    """Share of rows with an unsettled top-k position or a class within ``tol`` of the candidate threshold: where the
    oracle cannot say what the device must return. From the oracle alone."""
    lp, tol = reference(logits_wbc), tolerance(logits_wbc)
    W, B, C = lp.shape
    bad = 0
    for t in range(W):
        for b in range(B):
            row, tl = lp[t, b], tol[t, b]
            amb = not _settled(row, tl, _ranking(row), k).all()
            if want_candidates and not amb:
                amb = bool((np.abs(row - LN_THRESH) <= tl).any())
            bad += int(amb)
    return bad / float(W * B)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def check_frontend(fe, logits_wbc, k, want_candidates, stats=None):
    """Assert that the front-end dict ``fe`` (keys of ``model.beam_frontend_call``) is a correct front end of the
    float32 ``logits_wbc`` [W,B,C]. Returns ``ambiguity(logits_wbc, k, want_candidates)``. ``stats``, if a dict, gets
    ``worst`` = the largest ``err / tol`` over every compared value.

    Values: topk_logp, blank_logp and cand_logp within ``tol`` of the float64 log-prob of their class, exactly -inf
    where that is -inf.
    Self-consistency (bit-exact): top-k classes distinct and in [0, C); topk_logp non-increasing; equal device
    log-probs in ascending class order; a class in both the top-k and the candidate list has the same bits in both;
    class 0 in the top-k equals blank_logp; cand_off starts at 0, never decreases and ends at the number of entries;
    classes of a candidate slice strictly ascending; a class is listed exactly when its own float32 log-prob, as a
    double, exceeds ln 0.001 (checked on every listed class and every top-k class).
    Order: with the oracle's ranking (lp64 descending, class ascending), a settled position holds the oracle's class
    and a maximal run of unsettled positions holds the oracle's set of classes; a run that reaches past rank k holds
    classes of the oracle's run continued to its first settled gap. Classes with bit-equal inputs come lowest first:
    a listed class never has an unlisted lower class with the same input bits.
    Candidates: lp64 > ln 0.001 + tol must be listed, lp64 < ln 0.001 - tol must not be."""
    x = np.asarray(logits_wbc)
    W, B, C = x.shape
    lp, tol = reference(x), tolerance(x)
    assert (fe["W"], fe["B"], fe["C"], fe["k"]) == (W, B, C, k)
    ti, tv, bl = np.asarray(fe["topk_idx"]), np.asarray(fe["topk_logp"]), np.asarray(fe["blank_logp"])
    assert ti.shape == (W, B, k) and tv.shape == (W, B, k) and bl.shape == (W, B)
    assert tv.dtype == np.float32 and bl.dtype == np.float32 and ti.dtype == np.int32
    assert ((ti >= 0) & (ti < C)).all(), "top-k class out of range"
    worst = [0.0]

    def values(got, cls, where):
        """got: float32 device values of classes cls of row `where`."""
        want, tl = lp[where][cls], tol[where][cls]
        ninf = np.isneginf(want)
        assert np.isneginf(got[ninf]).all(), ("expected -inf", where)
        g = got[~ninf].astype(np.float64)
        err = np.abs(g - want[~ninf])
        ok = err <= tl[~ninf]                        # (a NaN compares False)
        assert ok.all(), ("log-prob off", where, cls[~ninf][~ok][:4], g[~ok][:4], want[~ninf][~ok][:4],
                          float(np.nanmax(err / tl[~ninf])) if (~ok).any() else 0.0)
        if err.size:
            worst[0] = max(worst[0], float((err / tl[~ninf]).max()))

    if want_candidates:
        off, ci, cl = np.asarray(fe["cand_off"]), np.asarray(fe["cand_idx"]), np.asarray(fe["cand_logp"])
        assert off.shape == (W * B + 1,) and off[0] == 0 and (np.diff(off) >= 0).all(), "cand_off"
        ncand = int(off[-1])
        assert ci.shape == (max(1, ncand),) and cl.shape == ci.shape, "cand_off[-1] is the number of entries"
        assert cl.dtype == np.float32

    unsettled_rows = 0
    for t in range(W):
        for b in range(B):
            where = (t, b)
            row, tl, xr = lp[t, b], tol[t, b], x[t, b]
            idx, val = ti[t, b].astype(np.int64), tv[t, b]
            assert len(set(idx.tolist())) == k, ("top-k classes repeat", where, idx)
            values(val, idx, where)
            values(bl[t, b].reshape(1), np.zeros(1, np.int64), where)
            with np.errstate(invalid="ignore"):
                assert not (np.diff(val.astype(np.float64)) > 0).any() and not np.isnan(val).any(), \
                    ("topk_logp rises", where, val)
            same = val[1:] == val[:-1]
            assert (idx[1:][same] > idx[:-1][same]).all(), ("equal log-probs not in ascending class order", where, idx, val)
            z = np.flatnonzero(idx == 0)
            if z.size:
                assert _bits(val[z])[0] == _bits(bl[t, b].reshape(1))[0], ("class 0 in the top-k differs from blank_logp", where)
            # order against the oracle
            order = _ranking(row)
            st = _settled(row, tl, order, k)
            if st.all():
                assert np.array_equal(idx, order[:k]), ("top-k order", where, idx, order[:k])
            else:
                unsettled_rows += 1
                j = 0
                while j < k:
                    if st[j] and (j == 0 or st[j - 1]):
                        assert idx[j] == order[j], ("settled position", where, j, idx, order[:k])
                        j += 1
                        continue
                    # a run starts at j (position j-1 settled or j == 0) and ends at the first settled position e
                    e = j
                    while e < k and not st[e]:
                        e += 1
                    if e < k:                          # closed run: positions j..e
                        assert set(idx[j:e + 1].tolist()) == set(order[j:e + 1].tolist()), \
                            ("unsettled run holds other classes", where, j, e, idx, order[:k])
                        j = e + 1
                    else:                              # reaches past rank k: continue the oracle's run to its end
                        full = _settled(row, tl, order, C)
                        e2 = k
                        while e2 < C and not full[e2]:
                            e2 += 1
                        assert set(idx[j:k].tolist()) <= set(order[j:min(e2 + 1, C)].tolist()), \
                            ("run at the k-th place holds other classes", where, j, idx, order[:e2 + 1])
                        j = k
            # bit-equal inputs: the lowest classes first, so no unlisted lower class shares a listed class's input
            xb = _bits(xr)
            listed = np.zeros(C, bool)
            listed[idx] = True
            eq = (xb[None, :] == xb[idx][:, None]) & (np.arange(C)[None, :] < idx[:, None]) & ~listed[None, :]
            assert not eq.any(), ("a lower class with the same input is left out", where, idx[eq.any(axis=1)])
            if not want_candidates:
                continue
            r = t * B + b
            cc, cv = ci[off[r]:off[r + 1]].astype(np.int64), cl[off[r]:off[r + 1]]
            assert ((cc >= 0) & (cc < C)).all() and (np.diff(cc) > 0).all(), ("candidate classes not ascending", where, cc[:8])
            values(cv, cc, where)
            assert (cv.astype(np.float64) > LN_THRESH).all(), ("listed candidate not above ln 0.001", where)
            inlist = np.zeros(C, bool)
            inlist[cc] = True
            pos = np.full(C, -1, np.int64)
            pos[cc] = np.arange(cc.size)
            both = inlist[idx]
            assert np.array_equal(_bits(val[both]), _bits(cv[pos[idx[both]]])), ("top-k and candidate bits differ", where)
            above = val.astype(np.float64) > LN_THRESH
            assert np.array_equal(above, both), ("a top-k class is listed iff its own log-prob exceeds ln 0.001", where,
                                                 idx[above != both], val[above != both])
            must, mustnot = row > LN_THRESH + tl, row < LN_THRESH - tl
            assert inlist[must].all(), ("candidate missing", where, np.flatnonzero(must & ~inlist)[:8])
            assert not inlist[mustnot].any(), ("class below the threshold listed", where, np.flatnonzero(mustnot & inlist)[:8])
    if stats is not None:
        stats["worst"] = max(stats.get("worst", 0.0), worst[0])
        stats["unsettled_rows"] = unsettled_rows
    return ambiguity(x, k, want_candidates)


def check_full_logp(full, fe, logits_wbc, want_candidates, stats=None):
    """The whole log-softmax tensor (``log_softmax_rows_kernel``) against the oracle with the same tolerance, and
    bit-equal to ``fe``'s top-k and candidate values for the classes those list."""
    x = np.asarray(logits_wbc)
    W, B, C = x.shape
    lp, tol = reference(x), tolerance(x)
    full = np.asarray(full)
    assert full.shape == x.shape and full.dtype == np.float32
    ninf = np.isneginf(lp)
    assert np.isneginf(full[ninf]).all()
    err = np.abs(full[~ninf].astype(np.float64) - lp[~ninf])
    assert (err <= tol[~ninf]).all(), float(np.nanmax(err / tol[~ninf]))
    if stats is not None:
        stats["worst"] = max(stats.get("worst", 0.0), float((err / tol[~ninf]).max()))
    assert np.array_equal(_bits(np.take_along_axis(full, fe["topk_idx"].astype(np.int64), axis=2)), _bits(fe["topk_logp"]))
    assert np.array_equal(_bits(full[:, :, 0]), _bits(fe["blank_logp"]))
    if want_candidates:
        off = fe["cand_off"]
        flat = full.reshape(W * B, C)
        for r in range(W * B):
            cc = fe["cand_idx"][off[r]:off[r + 1]].astype(np.int64)
            assert np.array_equal(_bits(flat[r, cc]), _bits(fe["cand_logp"][off[r]:off[r + 1]])), r


# ---------------------------------------------------------------------------------------------------------------------
# The kernels' arithmetic in numpy: float32 steps, the exponentials summed in float64. ``defect`` plants one mistake.
# ---------------------------------------------------------------------------------------------------------------------
DEFECTS = ("tie_high", "thresh_ge_f32", "thresh_002", "rows_bw", "skip_last", "no_max", "logs_added", "prev_row",
           "blank_from_1", "cand_desc", "sum_trunc")


def emulate(logits_wbc, k, want_candidates, defect=None):
    assert defect is None or defect in DEFECTS
    x = np.ascontiguousarray(logits_wbc, dtype=np.float32)
    W, B, C = x.shape
    R = W * B
    rows = x.reshape(R, C)
    n = C - 1 if defect == "skip_last" else C
    with np.errstate(all="ignore"):
        if defect == "no_max":
            d = rows
            s = np.exp(rows[:, :n]).astype(np.float32).sum(axis=1, dtype=np.float32).astype(np.float64)
        else:
            mx = rows[:, :n].max(axis=1, keepdims=True)
            d = rows - mx                                                     # float32
            e = np.exp(d[:, :n])                                              # float32
            if defect == "sum_trunc":
                s = e[:, :C & ~255].sum(axis=1, dtype=np.float32).astype(np.float64)
            else:
                s = e.astype(np.float64).sum(axis=1)
        logs = np.log(s.astype(np.float32))[:, None]                          # float32
        lp = (d + logs if defect == "logs_added" else d - logs).astype(np.float32)
    sel = np.roll(lp, 1, axis=0) if defect == "prev_row" else lp
    cls = np.arange(n)
    ti = np.empty((R, k), np.int32)
    for r in range(R):
        v = sel[r, :n].astype(np.float64)
        v = np.where(np.isnan(v), -np.inf, v)
        order = np.lexsort((-cls if defect == "tie_high" else cls, -v))[:k]
        if order.size < k:
            order = np.concatenate([order, np.zeros(k - order.size, np.int64)])
        ti[r] = order
    tv = np.take_along_axis(sel, ti.astype(np.int64), axis=1)
    bl = lp[:, 1 if defect == "blank_from_1" else 0].copy()
    fe = {"W": W, "B": B, "C": C, "k": k, "cand_off": None, "cand_idx": None, "cand_logp": None}
    if want_candidates:
        if defect == "thresh_ge_f32":
            keep = lp[:, :n] >= np.float32(LN_THRESH)
        elif defect == "thresh_002":
            keep = lp[:, :n].astype(np.float64) > np.log(0.002)
        else:
            keep = lp[:, :n].astype(np.float64) > LN_THRESH
        off, ci, cl = [0], [], []
        for r in range(R):
            c = np.flatnonzero(keep[r])
            if defect == "cand_desc":
                c = c[::-1]
            ci.append(c)
            cl.append(lp[r, c])
            off.append(off[-1] + c.size)
        ci, cl = np.concatenate(ci).astype(np.int32), np.concatenate(cl).astype(np.float32)
        fe["cand_off"] = np.array(off, np.int64)
        fe["cand_idx"] = ci if ci.size else np.zeros(1, np.int32)
        fe["cand_logp"] = cl if cl.size else np.zeros(1, np.float32)
    if defect == "rows_bw":                      # rows written at b*W + t instead of t*B + b
        dst = (np.arange(R) % B) * W + np.arange(R) // B
        ti2, tv2, bl2 = np.empty_like(ti), np.empty_like(tv), np.empty_like(bl)
        ti2[dst], tv2[dst], bl2[dst] = ti, tv, bl
        ti, tv, bl = ti2, tv2, bl2
    fe["topk_idx"], fe["topk_logp"], fe["blank_logp"] = ti.reshape(W, B, k), tv.reshape(W, B, k), bl.reshape(W, B)
    return fe


# ---------------------------------------------------------------------------------------------------------------------
# The case list of the stored-logits path: shared by the CPU self-test and the GPU test.
# ---------------------------------------------------------------------------------------------------------------------
class Case(object):
    def __init__(self, style, W, B, C, k, seed):
        self.style, self.W, self.B, self.C, self.k, self.seed = style, W, B, C, k, seed
        # cases built to contain exact ties (equal values, or several -inf) are exempt from the ambiguity cap
        self.ties = style in ("q025", "equal", "onehot", "infblock", "thr999", "thr1000", "thr1001")
        self.name = "%s-w%db%d-c%d-k%d" % (style, W, B, C, k)

    def logits(self):
        return make_logits(self.style, self.W, self.B, self.C, self.seed)


AMBIGUITY_CAP = 0.05
INF_EDGE = 20             # "infblock": classes [INF_EDGE, C - INF_EDGE) are -inf, 2 * INF_EDGE stay finite
THR_GAP = 60.0            # threshold rows: the classes outside the common value lie this far below it


def make_logits(style, W, B, C, seed):
    """float32 [W,B,C] logits of one style (see the issue list in tests/test_gpu_frontend.py)."""
    rng = np.random.RandomState(seed)
    g = rng.standard_normal((W, B, C))
    if style == "g3":
        x = g * 3
    elif style == "g30":
        x = g * 30
    elif style == "g30off":
        x = g * 30 + 1e4
    elif style == "g1000":
        x = g * 1000
    elif style in ("peaky", "flat"):
        import codec_cases
        x = codec_cases.gen_logits(seed, W, B, C, style)
    elif style == "q025":                     # multiples of 0.25: many exact ties, also at the k-th place
        x = np.round(g * 1.5 * 4) / 4
    elif style == "equal":
        x = np.full((W, B, C), 0.75)
    elif style == "onehot":
        x = np.full((W, B, C), -np.inf)
        for r in range(W * B):
            x[r // B, r % B, (7 * r + 1) % C] = rng.standard_normal() * 5
    elif style == "infblock":
        x = g * 3
        x[:, :, INF_EDGE:C - INF_EDGE] = -np.inf
    elif style in ("thr999", "thr1000", "thr1001"):
        n = int(style[3:])
        x = np.full((W, B, C), 3.5 - THR_GAP)
        for r in range(W * B):
            x[r // B, r % B, rng.permutation(C)[:n]] = 3.5
    else:
        raise ValueError(style)
    return np.ascontiguousarray(x, dtype=np.float32)


def stored_cases():
    """A covering subset of C x (W,B) x k x style: every C in {2, 3, 63, 64, 65, 255, 256, 257, 1000, 7358, 12288},
    every k in {1, 2, min(C,10), C for C <= 65, 33 and 64 for C >= 256}, every shape, (5,3) with the largest C.
    Styles whose values crowd stay at a k the oracle can settle: below the one strong class of a "peaky" row lie C
    uniform values 2/C apart on average, a few hundred tolerances at C = 7358, so one row in three would have an
    unsettled place among its first ten (k = 1 there); the 2^-10 input grid of "g30off" makes exact ties among the
    first 64 of 256 classes likely enough to cross the cap on 15 rows (k = 2 and 33 there, and 64 on a single row)."""
    T = [("g3", 1, 1, 2, 1), ("g3", 5, 3, 2, 2), ("g30", 17, 2, 3, 3), ("g3", 5, 3, 3, 1),
         ("g3", 5, 3, 63, 10), ("g30", 17, 2, 63, 63), ("g3", 17, 2, 64, 64), ("g30off", 5, 3, 64, 2),
         ("g3", 17, 2, 65, 65), ("g1000", 5, 3, 65, 10),
         ("g3", 5, 3, 255, 10), ("g30", 17, 2, 255, 1),
         ("g3", 17, 2, 256, 33), ("g30", 17, 2, 256, 64),
         ("g3", 5, 3, 257, 64), ("g1000", 17, 2, 257, 33),
         ("g3", 17, 2, 1000, 10), ("g30", 5, 3, 1000, 33), ("g30", 1, 1, 1000, 64),
         ("g30", 5, 3, 7358, 10), ("g3", 17, 2, 7358, 33), ("g30off", 1, 1, 7358, 64), ("g1000", 5, 3, 7358, 2),
         ("g3", 5, 3, 12288, 10), ("g30", 5, 3, 12288, 64), ("g1000", 1, 1, 12288, 1), ("g30off", 17, 2, 12288, 33),
         ("peaky", 17, 2, 300, 10), ("flat", 17, 2, 300, 10), ("peaky", 5, 3, 7358, 1), ("flat", 5, 3, 65, 65),
         ("q025", 5, 3, 257, 10), ("q025", 17, 2, 7358, 33), ("q025", 5, 3, 64, 64), ("q025", 5, 3, 12288, 2),
         ("equal", 5, 3, 1000, 10), ("equal", 1, 1, 12288, 64), ("equal", 5, 3, 3, 3),
         ("onehot", 5, 3, 65, 1), ("onehot", 17, 2, 257, 10), ("onehot", 5, 3, 12288, 33),
         ("infblock", 17, 2, 65, 65), ("infblock", 5, 3, 1000, 64), ("infblock", 5, 3, 12288, 33),
         ("thr999", 5, 3, 7358, 10), ("thr1001", 5, 3, 7358, 10), ("thr999", 5, 3, 1100, 10),
         ("thr1001", 5, 3, 1100, 10), ("thr1000", 5, 3, 1100, 10)]
    return [Case(s, w, b, c, k, 1000 + i) for i, (s, w, b, c, k) in enumerate(T)]


def check_case_expectations(case, fe, logits):
    """What a style promises beyond the general rules."""
    off = fe["cand_off"]
    W, B, C, k = case.W, case.B, case.C, case.k
    if case.style == "onehot":
        hot = np.argmax(logits, axis=2)
        assert np.array_equal(fe["topk_idx"][:, :, 0], hot) and (fe["topk_logp"][:, :, 0] == 0).all()
        assert np.isneginf(fe["topk_logp"][:, :, 1:]).all()
        for t in range(W):
            for b in range(B):
                rest = [c for c in range(min(C, k + 1)) if c != hot[t, b]][:k - 1]
                assert fe["topk_idx"][t, b, 1:].tolist() == rest, (t, b)
        assert np.array_equal(np.diff(off), np.ones(W * B)) and np.array_equal(fe["cand_idx"].reshape(W, B), hot)
    elif case.style == "equal":
        assert (fe["topk_idx"] == np.arange(k)).all()
        assert _bits(fe["topk_logp"]).min() == _bits(fe["topk_logp"]).max() == _bits(fe["blank_logp"]).min()
    elif case.style == "thr999":
        assert (np.diff(off) == 999).all()
        assert np.array_equal(fe["cand_idx"].reshape(W * B, 999), np.sort(np.argsort(-logits.reshape(W * B, C), axis=1,
                                                                                     kind="stable")[:, :999], axis=1))
    elif case.style == "thr1001":
        assert int(off[-1]) == 0
