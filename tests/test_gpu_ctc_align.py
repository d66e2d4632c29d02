"""GPU tests (-m gpu) of the CTC forced alignment (C ABI hctr_ctc_align / hctr_ctc_align_logits, ``hctr_model.align``,
``CTCAligner``): the best path of a known transcription, which gives each character's pixel span and confidence.

The reference project has no counterpart; the yardstick is tests/ctc_align_ref.py, a numpy restatement of the definition
in include/hctr_hip.h. What must hold:
  * planted paths (noise plus 12 on the planted class) and forced lines come back exactly, across every instance of the
    recursion's launch ladder, with the float64 score of the path to the loss tests' 1e-5 relative + 1e-3;
  * all-zero logits tie every path exactly in float32, so the documented tie rule alone decides the result;
  * on flat random logits, where near-ties may resolve differently in float32, the path is a valid alignment whose
    float64 score is within float32 rounding of the float64 optimum, and score <= -nll;
  * the image path equals aligning the engine's own f16x3 logits, bit for bit, across internal passes;
  * no align call changes what the loss, its gradient or greedy decoding compute.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import ctc_align_ref as ref

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-3                      # engine score vs float64 on the same logits (tests/test_gpu_ctc.py's)


def _close(got, want, what):
    err = abs(float(got) - float(want))
    print("%s: score %.6f vs float64 %.6f (|d| %.2e)" % (what, float(got), float(want), err))
    assert err <= RTOL * abs(float(want)) + ATOL, (what, got, want)


@pytest.fixture(scope="module")
def aligner(pkg):
    return pkg.CTCAligner().cuda(0)


@pytest.fixture(scope="module")
def m_trained(pkg, synth):
    C = synth.DEFAULT_VOCAB + 2
    m = pkg.hctr_model(C, precision="auto").cuda(0)
    m.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    return m


def _check_line(a, b, off, L, T, W, want_states, ext_classes, what):
    """line b of alignment a equals the state sequence want_states"""
    np.testing.assert_array_equal(a.paths[b, :T], ext_classes[want_states], err_msg="%s path" % what)
    assert (a.paths[b, T:] == -1).all(), what
    st, en = ref.spans_of_states(want_states, L)
    np.testing.assert_array_equal(a.starts[off:off + L], st, err_msg="%s starts" % what)
    np.testing.assert_array_equal(a.ends[off:off + L], en, err_msg="%s ends" % what)


def _ext(tg):
    e = np.zeros(2 * len(tg) + 1, np.int32)
    e[1::2] = tg
    return e


def _spans_consistent(a, b, off, tg, T):
    """the spans of line b are the runs of its labels in the path, in order, parted by blanks only"""
    p = a.paths[b, :T]
    pos = 0
    for j, c in enumerate(tg):
        s, e = int(a.starts[off + j]), int(a.ends[off + j])
        assert pos <= s < e <= T, (b, j, s, e)
        assert (p[pos:s] == 0).all() and (p[s:e] == c).all(), (b, j)
        if j and tg[j - 1] == c:
            assert s > pos, (b, j)                      # a blank parts equal neighbours
        pos = e
    assert (p[pos:] == 0).all(), b


def _planted_batch(rng, W, C, Ls, Ts, repeats):
    B = len(Ls)
    logits = rng.standard_normal((W, B, C)).astype(np.float32)
    tgs, sts = [], []
    for b in range(B):
        tg = ref.random_target(rng, C, Ls[b], repeats[b])
        z, states = ref.planted(rng, Ts[b], C, tg)
        logits[:Ts[b], b] = z
        tgs.append(tg)
        sts.append(states)
    return logits, tgs, sts


def _run_planted(aligner, rng, W, C, Ls, Ts, repeats):
    logits, tgs, sts = _planted_batch(rng, W, C, Ls, Ts, repeats)
    tl = np.array(Ls, np.int32)
    targets = np.concatenate(tgs).astype(np.int32)
    a = aligner(logits, targets, np.array(Ts, np.int32), tl)
    off = 0
    for b, L in enumerate(Ls):
        what = "planted W=%d C=%d L=%d T=%d" % (W, C, L, Ts[b])
        _check_line(a, b, off, L, Ts[b], W, sts[b], _ext(tgs[b]), what)
        lp64 = ref.log_softmax64(logits[:Ts[b], b])
        _close(a.scores[b], ref.path_score64(lp64, _ext(tgs[b])[sts[b]]), what)
        for j in range(L):                                 # span_logp: the label's log-probabilities over its span
            s, e = a.starts[off + j], a.ends[off + j]
            want = lp64[s:e, tgs[b][j]].sum()
            assert abs(a.logps[off + j] - want) <= RTOL * abs(want) + ATOL, (what, j)
        off += L
    return a


def test_planted_paths_every_ladder_instance(aligner):
    """S = 2L + 1 = 41 .. 2201 reaches every bucket of the launch ladder (<= 64, 128, 256, 512, 1024, 2048, 4096) as the
    batch's largest; each bucket also runs alone, since a batch launches the instance of its longest target"""
    W, C = 1200, 64
    Ls = [20, 50, 100, 200, 400, 900, 1100]
    Ts = [1000, W, W, 1111, W, W, W]
    reps = [0.3, 0.3, 0.3, 0.3, 0.3, 0.1, 0.04]
    rng = np.random.RandomState(5)
    a = _run_planted(aligner, rng, W, C, Ls, Ts, reps)
    assert (a.paths[0, 1000:] == -1).all() and (a.paths[3, 1111:] == -1).all()
    for n in range(1, 7):                                   # the shorter ladders: the first n lines on their own
        _run_planted(aligner, np.random.RandomState(50 + n), W, C, Ls[:n], Ts[:n], reps[:n])


def test_planted_paths_real_row_width(aligner):
    _run_planted(aligner, np.random.RandomState(6), 300, 7358, [40, 0, 120], [300, 300, 257], [0.3, 0.3, 0.3])


def test_forced_lines(aligner, pkg):
    """T = L + repeats has one alignment; L = 0 is all blanks; one step short of the limit has none"""
    C, W = 13, 24
    rng = np.random.RandomState(7)
    logits = rng.standard_normal((W, 5, C)).astype(np.float32)
    lines = [[5, 5, 6, 6, 6, 7, 1, 2, 3], [], [4], [4, 4], [4, 4]]
    il = np.array([12, W, 1, 3, 2], np.int32)               # 9 + 3 repeats = 12; L = 1 at T = 1; 2 + 1 = 3; 3 > 2
    tl = np.array([len(v) for v in lines], np.int32)
    a = aligner(logits, np.array(sum(lines, []), np.int32), il, tl)
    assert a.paths[0, :12].tolist() == [5, 0, 5, 6, 0, 6, 0, 6, 7, 1, 2, 3] and (a.paths[0, 12:] == -1).all()
    assert a.starts[:9].tolist() == [0, 2, 3, 5, 7, 8, 9, 10, 11] and a.ends[:9].tolist() == [1, 3, 4, 6, 8, 9, 10, 11, 12]
    lp = ref.log_softmax64(logits.transpose(1, 0, 2))
    _close(a.scores[0], ref.path_score64(lp[0, :12], a.paths[0, :12]), "limit")
    assert (a.paths[1] == 0).all()
    _close(a.scores[1], lp[1, :, 0].sum(), "L=0")
    assert a.paths[2, 0] == 4 and (a.paths[2, 1:] == -1).all() and (a.starts[9], a.ends[9]) == (0, 1)
    _close(a.scores[2], lp[2, 0, 4], "L=1, T=1")
    assert a.paths[3, :3].tolist() == [4, 0, 4] and a.starts[10:12].tolist() == [0, 2]
    # one step short: no alignment
    assert np.isneginf(a.scores[4]) and (a.paths[4] == -1).all()
    assert (a.starts[12:] == -1).all() and (a.ends[12:] == -1).all() and np.isneginf(a.logps[12:]).all()
    assert np.isfinite(a.scores[:4]).all() and np.isfinite(a.logps[:12]).all()
    # (an L = 1 line sits at its limit with T = 1, line 2; input_lengths < 1 is an argument error, so the shortest
    # line one step short of its limit is the repeated pair of line 4)
    nll = pkg.CTCLoss(reduction="none").cuda(0)(logits, np.array(sum(lines, []), np.int32), il, tl)
    assert np.isposinf(nll[4]) and np.isfinite(nll[:4]).all()


def test_tie_rule(aligner):
    """all-zero logits: every path ties exactly in float32 (sums of one value in one order), so the rule decides"""
    C = 13
    for T, tg, path in ref.TIE_TABLE:
        a = aligner(np.zeros((T, 1, C), np.float32), np.array(tg, np.int32), None, np.array([len(tg)], np.int32))
        assert a.paths[0].tolist() == path, (T, tg, a.paths[0])
    rng = np.random.RandomState(8)
    W = 700
    Ls = [0, 1, 7, 40, 150, 300]
    tgs = [ref.random_target(rng, C, L, 0.4) for L in Ls]
    il = np.array([W, 33, W, 200, W, 699], np.int32)
    a = aligner(np.zeros((W, len(Ls), C), np.float32), np.concatenate(tgs).astype(np.int32), il, np.array(Ls, np.int32))
    off = 0
    for b, L in enumerate(Ls):
        r = ref.viterbi(np.zeros((il[b], C), np.float32), tgs[b], np.float32)
        _check_line(a, b, off, L, il[b], W, r["states"], _ext(tgs[b]), "tie L=%d" % L)
        assert abs(a.scores[b] - r["score"]) <= 1e-6 * abs(r["score"])
        off += L


def _edge_targets(C, W, rng):
    """the loss tests' edge lines scaled to W: L = 0; L = 1; adjacent repeats; exactly at the feasibility limit with a
    short input; one step short of it (infeasible); a long target at L + repeats = W; a long random target"""
    def rnd(n):
        return list(rng.randint(1, C, n))
    rep = []
    for v in rnd(20):
        rep += [v] * int(rng.randint(1, 4))
    lim = [5, 5, 6, 6, 6, 7] + rnd(10)
    lim[6] = 8 if lim[6] == 7 else lim[6]
    for j in range(7, 16):                                 # exactly 3 repeats: needs 19 steps
        while lim[j] == lim[j - 1]:
            lim[j] = int(rng.randint(1, C))
    inf = [9, 9, 9] + [10, 11] * 7 + [12]                  # 18 labels, 2 repeats: needs 20 > 19
    longt, cost = [], 0
    while cost < W:
        if longt and W - cost >= 2 and rng.rand() < 0.4:
            longt.append(longt[-1])
            cost += 2
        else:
            v = int(rng.randint(1, C))
            while longt and v == longt[-1]:
                v = int(rng.randint(1, C))
            longt.append(v)
            cost += 1
    lines = [[], rnd(1), rep, lim, inf, longt, rnd(W // 6)]
    il = [W, W - 7, W, 19, 19, W, W // 2]
    return lines, np.array(il, np.int32)


@pytest.mark.parametrize("C,W", [(50, 300), (7358, 150)])
def test_flat_random_logits(aligner, pkg, C, W):
    rng = np.random.RandomState(C)
    lines, il = _edge_targets(C, W, rng)
    B = len(lines)
    tl = np.array([len(v) for v in lines], np.int32)
    targets = np.array(sum(lines, []), np.int32)
    logits = rng.standard_normal((W, B, C)).astype(np.float32)
    a = aligner(logits, targets, il, tl)
    nll = pkg.CTCLoss(reduction="none").cuda(0)(logits, targets, il, tl)
    assert np.isneginf(a.scores[4]) and (a.paths[4] == -1).all() and np.isposinf(nll[4])
    off, differ, n = 0, 0, 0
    for b in range(B):
        T, tg = int(il[b]), np.array(lines[b], np.int32)
        if b != 4:
            assert ref.feasible(tg, T)
            r = ref.viterbi(logits[:T, b], tg, np.float64)
            p = a.paths[b, :T]
            assert (a.paths[b, T:] == -1).all()
            np.testing.assert_array_equal(ref.collapse(p), tg)
            _spans_consistent(a, b, off, tg, T)
            opt = float(r["score"])
            mine = ref.path_score64(r["lp64"], p)
            bound = 4 * T * 2.0 ** -24 * abs(opt)
            print("C=%d line %d (T=%d, L=%d): optimum %.6f, path %.6f, score %.6f, bound %.2e, -nll %.6f" % (
                C, b, T, len(tg), opt, mine, float(a.scores[b]), bound, -float(nll[b])))
            assert mine >= opt - bound, (b, mine, opt, bound)
            assert abs(float(a.scores[b]) - mine) <= bound, (b, float(a.scores[b]), mine, bound)
            assert float(a.scores[b]) <= -float(nll[b]) + ATOL, (b, a.scores[b], nll[b])
            differ += int(not np.array_equal(p, r["path"]))
            n += 1
        off += len(tg)
    print("C=%d: %d of %d lines differ from the float64 path" % (C, differ, n))


def test_host_device_and_log_prob_input(aligner):
    rng = np.random.RandomState(10)
    W, B, C = 120, 4, 30
    Ls = [10, 0, 33, 5]
    tgs = [ref.random_target(rng, C, L) for L in Ls]
    logits = (rng.standard_normal((W, B, C)) * 3).astype(np.float32)
    targets, tl = np.concatenate(tgs).astype(np.int32), np.array(Ls, np.int32)
    il = np.array([W, 50, W, 99], np.int32)
    host = aligner(logits, targets, il, tl)
    dev_t = torch.from_numpy(logits).cuda(0)
    dev = aligner(dev_t, torch.from_numpy(targets), torch.from_numpy(il), torch.from_numpy(tl))
    for k in ("paths", "scores", "starts", "ends", "logps", "offsets"):
        np.testing.assert_array_equal(getattr(host, k), getattr(dev, k), err_msg=k)
    lp = aligner(dev_t.log_softmax(2), targets, il, tl)
    np.testing.assert_array_equal(lp.paths, host.paths)
    np.testing.assert_array_equal(lp.starts, host.starts)
    np.testing.assert_allclose(lp.scores, host.scores, rtol=RTOL, atol=ATOL)
    padded = np.zeros((B, max(Ls)), np.int64)
    for b, v in enumerate(tgs):
        padded[b, :len(v)] = v
    np.testing.assert_array_equal(aligner(logits, padded, il, tl).paths, host.paths)
    confs = [c for ln in host.lines() for _, _, _, c in ln]
    assert len(confs) == sum(Ls) and all(0.0 < c <= 1.0 for c in confs)


def test_argument_errors(aligner, pkg):
    C, W = 9, 16
    logits = np.zeros((W, 2, C), np.float32)
    tl = np.array([2, 1], np.int32)
    for bad in ([0, 1, 2], [1, C, 2], [1, -3, 2]):
        with pytest.raises(ValueError):
            aligner(logits, np.array(bad, np.int32), None, tl)
    for il in ([0, W], [W + 1, 5]):
        with pytest.raises(ValueError):
            aligner(logits, np.array([1, 2, 3], np.int32), np.array(il, np.int32), tl)
    lib = pkg.load_library()
    ctx = aligner._context()
    vp = ctypes.c_void_p

    def p(x):
        return x.ctypes.data_as(vp)

    # L > 2047 on a feasible line
    Wl = 2100
    big = np.zeros((Wl, 1, 3), np.float32)
    tg = np.tile(np.array([1, 2], np.int32), 1024)
    rc = lib.hctr_ctc_align_logits(ctx, p(big), 0, Wl, 1, 3, p(tg), p(np.array([2048], np.int32)), None, None, None, None,
                                   None, None)
    err_arg = -1                                           # HCTR_ERR_ARG
    assert rc == err_arg
    tg3 = np.array([0, 1, 2], np.int32)
    assert lib.hctr_ctc_align_logits(ctx, p(logits), 0, W, 2, C, p(tg3), p(tl), None, None, None, None, None,
                                     None) == err_arg
    bad_il = np.array([0, W], np.int32)
    ok3 = np.array([1, 2, 3], np.int32)
    assert lib.hctr_ctc_align_logits(ctx, p(logits), 0, W, 2, C, p(ok3), p(tl), p(bad_il), None, None, None, None,
                                     None) == err_arg
    # every output pointer may be NULL, alone or together; B == 0 is a no-op
    assert lib.hctr_ctc_align_logits(ctx, p(logits), 0, W, 2, C, p(ok3), p(tl), None, None, None, None, None, None) == 0
    score = np.full(2, np.nan, np.float32)
    assert lib.hctr_ctc_align_logits(ctx, p(logits), 0, W, 2, C, p(ok3), p(tl), None, None, None, None, None,
                                     p(score)) == 0
    np.testing.assert_allclose(score, -W * np.log(C), rtol=1e-5)
    path = np.full((2, W), 77, np.int32)
    assert lib.hctr_ctc_align_logits(ctx, p(logits), 0, W, 2, C, p(ok3), p(tl), None, p(path), None, None, None,
                                     None) == 0
    assert path[0].tolist() == [1, 2] + [0] * (W - 2) and path[1].tolist() == [3] + [0] * (W - 1)
    assert lib.hctr_ctc_align_logits(ctx, None, 0, W, 0, C, None, None, None, None, None, None, None, None) == 0
    empty = aligner(np.zeros((W, 0, C), np.float32), np.zeros(0, np.int32), None, np.zeros(0, np.int32))
    assert empty.paths.shape == (0, W) and empty.scores.shape == (0,) and list(empty.lines()) == []


def test_no_side_effects(pkg, synth, m_trained):
    ctc = __import__("importlib").import_module(pkg.__name__ + ".ctc")
    rng = np.random.RandomState(12)
    W, B, C = 90, 3, 40
    logits = rng.standard_normal((W, B, C)).astype(np.float32)
    tgs = [ref.random_target(rng, C, L) for L in (7, 0, 25)]
    targets, tl = np.concatenate(tgs).astype(np.int32), np.array([7, 0, 25], np.int32)
    imgs = synth.make_font_lines(3, 96, 31)
    ctx = m_trained._ctx

    def others():
        g = m_trained.greedy(imgs)
        guard = m_trained.last_guard()
        nll = ctc.loss_logits(ctx, logits, 0, targets, tl, None)
        nll2, grad = ctc.loss_grad_logits(ctx, logits, 0, targets, tl, None, None)
        return g, guard, nll, nll2, grad

    g0, guard0, nll0, nll20, grad0 = others()
    big = [ref.random_target(rng, C, L) for L in (80, 3, 40)]             # another scratch layout in between
    ctc.align_logits(ctx, logits, 0, np.concatenate(big).astype(np.int32), np.array([80, 3, 40], np.int32), None)
    al = m_trained.align(imgs, np.concatenate(g0).astype(np.int32), np.array([len(v) for v in g0], np.int32))
    after = m_trained.last_guard()
    assert guard0["lines"] == after["lines"] and guard0["flagged"] == after["flagged"]
    for k in ("flags", "min_margin", "scale"):
        np.testing.assert_array_equal(guard0[k], after[k])
    assert np.isfinite(al.scores).all()
    g1, guard1, nll1, nll21, grad1 = others()
    for x, y in zip(g0, g1):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(nll0, nll1)
    np.testing.assert_array_equal(nll20, nll21)
    np.testing.assert_array_equal(grad0, grad1)
    for k in ("flags", "min_margin", "scale"):
        np.testing.assert_array_equal(guard0[k], guard1[k])


def _image_case(pkg, synth, m, W):
    imgs = synth.make_font_lines(3, W, 40 + W)
    widths = np.array([W, W - 29, W - 50], np.int32)
    labels = m.greedy(imgs, widths=widths)
    tl = np.array([len(v) for v in labels], np.int32)
    targets = np.concatenate(labels).astype(np.int32) if tl.sum() else np.zeros(0, np.int32)
    return imgs, widths, labels, targets, tl


@pytest.mark.parametrize("W", [96, 160])
def test_image_path_equals_logits_path(pkg, synth, m_trained, W):
    """hctr_ctc_align(images) == hctr_ctc_align_logits(hctr_forward_logits(images) in f16x3), also with the batch split
    into internal passes (a second context with a small pass size); every path collapses to the greedy text"""
    C = synth.DEFAULT_VOCAB + 2
    imgs, widths, labels, targets, tl = _image_case(pkg, synth, m_trained, W)
    assert tl.sum() > 0
    fused = m_trained.align(imgs, targets, tl, widths=widths)
    m_trained.set_precision("f16x3")
    try:
        logits = m_trained(torch.from_numpy(imgs).cuda(0), widths=widths)
    finally:
        m_trained.set_precision("auto")
    unfused = pkg.CTCAligner().attach(m_trained)(logits, targets, None, tl)
    os.environ["HCTR_MAX_COLS"] = "600"                    # f16x3 passes of 200 columns: one or two lines each
    try:
        small = pkg.hctr_model(C, precision="auto").cuda(0)
    finally:
        del os.environ["HCTR_MAX_COLS"]
    small.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    assert small.lines_per_pass(3, W, f16x3=True) < 3
    split = small.align(imgs, targets, tl, widths=widths)
    for got, what in ((unfused, "logits path"), (split, "split passes")):
        for k in ("paths", "starts", "ends", "logps"):
            np.testing.assert_array_equal(getattr(fused, k), getattr(got, k), err_msg="%s %s" % (what, k))
        assert fused.scores.tobytes() == got.scores.tobytes(), (what, fused.scores, got.scores)
    for b in range(3):
        np.testing.assert_array_equal(ref.collapse(fused.paths[b]), labels[b])
    assert (fused.paths >= 0).all()                        # input_lengths None: the pad columns count


def test_python_surface(pkg, synth, m_trained):
    W = 96
    imgs, widths, labels, targets, tl = _image_case(pkg, synth, m_trained, W)
    want = m_trained.align(imgs, targets, tl, widths=widths)
    padded = np.zeros((3, max(1, int(tl.max()))), np.int64)
    for b, v in enumerate(labels):
        padded[b, :len(v)] = v
    il = np.full(3, W, np.int32)
    for inp in (imgs, torch.from_numpy(imgs), torch.from_numpy(imgs).cuda(0)):
        for tg in (targets, padded, torch.from_numpy(padded)):
            got = m_trained.align(inp, tg, tl, input_lengths=il, widths=widths)
            for k in ("paths", "scores", "starts", "ends", "logps", "offsets"):
                np.testing.assert_array_equal(getattr(want, k), getattr(got, k), err_msg=k)
    m_trained.set_precision("f16x3")
    try:
        logits = m_trained(imgs, widths=widths)                                  # numpy [W, B, C]
    finally:
        m_trained.set_precision("auto")
    al = pkg.CTCAligner().attach(m_trained)
    lib, ctx = pkg.load_library(), m_trained._ctx
    vp = ctypes.c_void_p
    path = np.empty((3, W), np.int32)
    st, en = np.empty(int(tl.sum()), np.int32), np.empty(int(tl.sum()), np.int32)
    lg, sc = np.empty(int(tl.sum()), np.float32), np.empty(3, np.float32)
    assert lib.hctr_ctc_align_logits(ctx, logits.ctypes.data_as(vp), 0, W, 3, logits.shape[2], targets.ctypes.data_as(vp),
                                     tl.ctypes.data_as(vp), None, path.ctypes.data_as(vp), st.ctypes.data_as(vp),
                                     en.ctypes.data_as(vp), lg.ctypes.data_as(vp), sc.ctypes.data_as(vp)) == 0
    for inp in (logits, torch.from_numpy(logits), torch.from_numpy(logits).cuda(0)):
        for tg in (targets, padded):
            got = al(inp, tg, None, tl)
            np.testing.assert_array_equal(got.paths, path)
            np.testing.assert_array_equal(got.starts, st)
            np.testing.assert_array_equal(got.ends, en)
            np.testing.assert_array_equal(got.logps, lg)
            np.testing.assert_array_equal(got.scores, sc)
    np.testing.assert_array_equal(want.paths, path)
    confs = [c for ln in want.lines() for _, _, _, c in ln]
    assert len(confs) == int(tl.sum()) and all(0.0 < c <= 1.0 for c in confs), confs
    assert [[c for c, _, _, _ in ln] for ln in want.lines()] == [list(v) for v in labels]
