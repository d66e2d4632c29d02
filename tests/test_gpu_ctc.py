"""GPU tests (-m gpu) of the CTC loss (C ABI hctr_ctc_loss / hctr_ctc_loss_logits, ``hctr_model.ctc_loss``, ``CTCLoss``):
the criterion of the reference's evaluation stack, ``CTCLoss(zero_infinity=True)`` over ``preds.log_softmax(2)``
(main.py:205,379-409), forward only.

What must hold:
  * on caller logits the engine equals torch's CPU ctc_loss in float64 to 1e-5 relative + 1e-3, infeasible lines are
    exactly +inf, and log-probs score like the raw logits;
  * the fused image path equals scoring the engine's own logits, in f16 and f16x3, across internal passes;
  * against the REAL reference's losses (tests/golden/ctc_lines.json) within the proven bound
    |dNLL| <= 2 * sum_t max_c |dz_t,c| with the logit tolerances the parity suite asserts;
  * invariants without an oracle, mode 2 = mode 1 bit for bit, and no CTC call changes what other paths compute.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

LOGIT_RTOL, LOGIT_ATOL = 0.01, 0.05          # f16 logits vs the fp32 reference (tests/test_gpu_parity.py)
X3_RTOL = 2e-4                               # f16x3 logits vs the fp32 reference (tests/test_gpu_parity.py)
RTOL, ATOL = 1e-5, 1e-3                      # engine loss vs torch float64 on the same logits


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert (np.isinf(got) == np.isinf(want)).all(), (what, got, want)
    fin = np.isfinite(want)
    err = np.abs(got[fin] - want[fin])
    lim = RTOL * np.abs(want[fin]) + ATOL
    assert (err <= lim).all(), (what, float((err / lim).max()), got, want)
    return float(err.max()) if err.size else 0.0


def _torch64(logits, targets, tl, il):
    W, B, _ = logits.shape
    lp = torch.from_numpy(np.asarray(logits)).double().log_softmax(2)
    il = torch.full((B,), W, dtype=torch.long) if il is None else torch.as_tensor(np.asarray(il), dtype=torch.long)
    return torch.nn.functional.ctc_loss(lp, torch.as_tensor(np.asarray(targets), dtype=torch.long),
                                        il, torch.as_tensor(np.asarray(tl), dtype=torch.long),
                                        reduction="none", zero_infinity=False).numpy()


@pytest.fixture(scope="module")
def m_random(pkg, synth, state_dict):
    m = pkg.hctr_model(synth.DEFAULT_VOCAB + 2, precision="auto").cuda(0)
    m.load_state_dict(state_dict)
    return m


@pytest.fixture(scope="module")
def m_trained(pkg, synth):
    C = synth.DEFAULT_VOCAB + 2
    m = pkg.hctr_model(C, precision="auto").cuda(0)
    m.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    return m


def _edge_targets(C, W, rng):
    """lines: L = 0; L = 1; adjacent repeats; exactly at the feasibility limit (L + repeats = T) with a short input;
    one step short of it (infeasible); a long target (2L + 1 > 2048 states: the largest recursion instance) at
    L + repeats = W; a long random target"""
    def rnd(n):
        return list(rng.randint(1, C, n))
    rep = []
    for v in rnd(20):
        rep += [v] * int(rng.randint(1, 4))
    lim = [5, 5, 6, 6, 6, 7] + rnd(10)                     # 16 labels, 3 repeats: needs 19 steps
    inf = [9, 9, 9] + rnd(15)                              # 18 labels, 2 repeats: needs 20 > 19
    longt, cost = [], 0
    while cost < W:
        if longt and W - cost >= 2 and rng.rand() < 0.4:
            longt.append(longt[-1])                        # a repeat costs two steps (a blank between)
            cost += 2
        else:
            v = int(rng.randint(1, C))
            while longt and v == longt[-1]:
                v = int(rng.randint(1, C))
            longt.append(v)
            cost += 1
    assert 2 * len(longt) + 1 > 2048
    lines = [[], rnd(1), rep, lim, inf, longt, rnd(300)]
    il = [W, W - 7, W, 19, 19, W, W // 2]
    tl = np.array([len(t) for t in lines], np.int32)
    return np.array(sum(lines, []), np.int32), tl, np.array(il, np.int32)


@pytest.mark.parametrize("scale", [3.0, 30.0])
def test_logits_entry_matches_torch_float64(pkg, synth, scale):
    C, W = synth.DEFAULT_VOCAB + 2, 2000
    rng = np.random.RandomState(int(scale))
    targets, tl, il = _edge_targets(C, W, rng)
    B = len(tl)
    logits = (rng.standard_normal((W, B, C)) * scale).astype(np.float32)
    want = _torch64(logits, targets, tl, il)
    assert np.isinf(want[4]) and np.isfinite(np.delete(want, 4)).all()
    crit = pkg.CTCLoss(reduction="none").cuda(0)
    got_host = crit(logits, targets, il, tl)
    err = _close(got_host, want, "host logits")
    assert np.isinf(got_host[4]) and got_host[4] > 0
    dev = torch.from_numpy(logits).cuda(0)
    got_dev = crit(dev, torch.from_numpy(targets), torch.from_numpy(il), torch.from_numpy(tl))
    assert got_dev.is_cuda
    np.testing.assert_array_equal(got_dev.cpu().numpy(), got_host)
    got_lp = crit(dev.log_softmax(2), targets, il, tl)
    _close(got_lp.cpu().numpy(), want, "log-prob input")
    # input_lengths None = W for every line (main.py's preds_sizes)
    want_w = _torch64(logits, targets, tl, None)
    _close(crit(logits, targets, None, tl), want_w, "input_lengths=None")
    print("scale %g: max |dNLL| %.2e, NLL up to %.3g" % (scale, err, float(want[np.isfinite(want)].max())))


def test_logits_entry_small_shapes(pkg):
    """tiny C and T, every line at its own length, B = 1, and a weightless context (ctc_codec's kind)"""
    rng = np.random.RandomState(4)
    crit = pkg.CTCLoss(reduction="none").cuda(0)
    for (W, B, C) in [(1, 1, 2), (2, 3, 3), (7, 5, 4), (64, 9, 5), (129, 4, 50)]:
        logits = (rng.standard_normal((W, B, C)) * 5).astype(np.float32)
        tl = rng.randint(0, min(W, 6) + 1, B).astype(np.int32)
        targets = rng.randint(1, C, int(tl.sum())).astype(np.int32)
        il = rng.randint(1, W + 1, B).astype(np.int32)
        _close(crit(logits, targets, il, tl), _torch64(logits, targets, tl, il), (W, B, C))


def _font_batch(synth, n, W, seed):
    imgs, truth = synth.make_font_lines(n, W, seed, with_truth=True)
    return imgs, [synth.font_truth_text(b, W) for b in truth]


@pytest.mark.parametrize("precision", ["f16", "f16x3"])
def test_fused_equals_unfused(pkg, synth, m_random, precision):
    """hctr_ctc_loss(images) == hctr_ctc_loss_logits(hctr_forward_logits(images)): unequal widths, 64 x 2000 (one pass in
    f16, four in f16x3) with each line's greedy text as targets plus some random strings"""
    C, W = synth.DEFAULT_VOCAB + 2, 2000
    m_random.set_precision(precision)
    try:
        rng = np.random.RandomState(9)
        imgs = torch.from_numpy(synth.make_line_images(64, W, seed=13)).cuda(0)
        widths = rng.randint(600, W + 1, 64).astype(np.int32)
        widths[0] = W
        labels = m_random.greedy(imgs, widths=widths)
        for b in range(0, 64, 8):
            labels[b] = rng.randint(1, C, int(rng.randint(0, 200))).astype(np.int32)
        tl = np.array([len(v) for v in labels], np.int32)
        targets = np.concatenate(labels).astype(np.int32)
        fused = m_random.ctc_loss(imgs, targets, tl, widths=widths, reduction="none", zero_infinity=False)
        logits = m_random(imgs, widths=widths)
        crit = pkg.CTCLoss(reduction="none").attach(m_random)
        unfused = crit(logits, targets, None, tl)
        err = _close(fused.cpu().numpy(), unfused.cpu().numpy(), precision)
        print("%s: fused vs unfused max |dNLL| %.2e" % (precision, err))
    finally:
        m_random.set_precision("auto")


def test_fused_two_passes_b80(pkg, synth, m_trained):
    """80 lines of 2000 columns run in two internal f16 passes; input_lengths mixed"""
    C, W = synth.DEFAULT_VOCAB + 2, 2000
    m_trained.set_precision("f16")
    try:
        assert m_trained.lines_per_pass(80, W) < 80
        imgs, texts = _font_batch(synth, 80, W, 17)
        cd = pkg.ctc_codec(synth.characters())
        targets, tl = cd.encode(texts)
        il = np.random.RandomState(2).randint(W // 2, W + 1, 80).astype(np.int32)
        il[:40] = W
        fused = m_trained.ctc_loss(imgs, targets, tl, input_lengths=il, reduction="none", zero_infinity=False)
        logits = m_trained(torch.from_numpy(imgs).cuda(0))
        unfused = pkg.CTCLoss(reduction="none").attach(m_trained)(logits, targets, il, tl).cpu().numpy()
        _close(fused, unfused, "B=80")
    finally:
        m_trained.set_precision("auto")


def _golden():
    with open(os.path.join(GOLDEN, "ctc_lines.json"), encoding="utf-8") as f:
        return json.load(f)


@pytest.mark.parametrize("precision", ["f16", "f16x3"])
def test_against_the_real_reference(pkg, synth, m_random, m_trained, precision):
    """per-line NLL of the reference's own logits (fixture, float64) within 2 * T * (logit tolerance): the proven bound
    |dNLL| <= 2 * sum_t max_c |dz_t,c|; the 'mean' of main.py's criterion within the same bound"""
    g = _golden()
    cd = pkg.ctc_codec(synth.characters())
    report = []
    for rec in g["batches"]:
        m = m_random if rec["checkpoint"] == "random" else m_trained
        m.set_precision(precision)
        try:
            n, W = len(rec["widths"]), rec["W"]
            if rec["generator"] == "lines":
                imgs = synth.make_line_images(n, W, rec["seed"])
            else:
                imgs = synth.make_font_lines(n, W, rec["seed"], with_truth=True)[0]
            widths = np.array(rec["widths"], np.int32)
            targets, tl = cd.encode(rec["texts"])
            got = m.ctc_loss(imgs, targets, tl, widths=widths, reduction="none", zero_infinity=False)
            mean = m.ctc_loss(imgs, targets, tl, widths=widths)                  # main.py: mean, zero_infinity
        finally:
            m.set_precision("auto")
        want = np.array(rec["nll_fp64"], np.float64)
        scale = np.array(rec["line_logit_scale"], np.float64)
        tol = X3_RTOL * scale if precision == "f16x3" else LOGIT_RTOL * scale + LOGIT_ATOL
        bound = 2.0 * W * tol
        inf = np.isinf(want)
        assert (np.isinf(got) == inf).all(), (rec["name"], got, want)
        dev = np.abs(got[~inf] - want[~inf])
        assert (dev <= bound[~inf]).all(), (rec["name"], dev, bound)
        fin_l = np.maximum(np.array(tl, np.float64), 1.0)
        mean_bound = float(np.sum(np.where(inf, 0.0, bound) / fin_l) / n)
        assert abs(float(mean) - rec["mean_zero_infinity"]) <= mean_bound + 1e-5 * abs(rec["mean_zero_infinity"]), (
            rec["name"], float(mean), rec["mean_zero_infinity"])
        report.append("%s: |dNLL| %s (bound %s), mean %.5f vs %.5f" % (
            rec["name"], np.array2string(dev, precision=4), np.array2string(bound[~inf], precision=1), float(mean),
            rec["mean_zero_infinity"]))
    print("%s: %s" % (precision, "; ".join(report)))


def test_invariants_on_font_lines(pkg, synth, m_trained):
    """trained-like checkpoint: NLL(truth) is small where the greedy text is the truth; one substituted character
    raises it; NLL(greedy text) <= -sum_t max_c log p_t(c) (the best path is one alignment of the greedy text)"""
    C, W = synth.DEFAULT_VOCAB + 2, 320
    m_trained.set_precision("f16")
    try:
        imgs, texts = _font_batch(synth, 16, W, 23)
        cd = pkg.ctc_codec(synth.characters())
        greedy = m_trained.greedy(imgs)
        gtext = cd.labels_to_text(greedy)
        ok = [b for b in range(16) if gtext[b] == texts[b] and texts[b]]
        assert len(ok) >= 4, (gtext, texts)
        targets, tl = cd.encode([texts[b] for b in ok])
        sub = imgs[ok]
        nll = m_trained.ctc_loss(sub, targets, tl, reduction="none", zero_infinity=False)
        assert (nll < 1.0).all(), nll
        bad = targets.copy()
        off = np.concatenate([[0], np.cumsum(tl)[:-1]])
        bad[off] = bad[off] % (C - 2) + 1                     # first character of every line -> another known class
        assert (bad[off] != targets[off]).all()
        nll_bad = m_trained.ctc_loss(sub, bad, tl, reduction="none", zero_infinity=False)
        assert (nll_bad > nll + 1.0).all(), (nll, nll_bad)
        # greedy text of every line: bounded by the best path's cost
        fe = m_trained.beam_frontend(imgs, 1)
        best = -fe["topk_logp"][:, :, 0].astype(np.float64).sum(axis=0)
        clean = [b for b in range(16) if (fe["topk_idx"][:, b, 0] != C - 1).all()]
        gl = np.array([len(greedy[b]) for b in clean], np.int32)
        gt = np.concatenate([greedy[b] for b in clean]).astype(np.int32)
        nll_g = m_trained.ctc_loss(imgs[clean], gt, gl, reduction="none", zero_infinity=False)
        assert (nll_g <= best[clean] + 1e-5 * np.abs(best[clean]) + 1e-3).all(), (nll_g, best[clean])
    finally:
        m_trained.set_precision("auto")


def test_auto_mode_is_f16x3_and_keeps_the_guard(pkg, synth, m_random):
    imgs = synth.make_line_images(6, 480, seed=3)
    widths = np.array([480, 400, 320, 480, 96, 200], np.int32)
    m_random.set_precision("auto")
    labels = m_random.greedy(imgs, widths=widths)
    guard = m_random.last_guard()
    tl = np.array([len(v) for v in labels], np.int32)
    targets = np.concatenate(labels).astype(np.int32)
    auto = m_random.ctc_loss(imgs, targets, tl, widths=widths, reduction="none")
    after = m_random.last_guard()
    assert guard["lines"] == after["lines"] == 6 and guard["flagged"] == after["flagged"]
    for k in ("flags", "min_margin", "scale"):
        np.testing.assert_array_equal(guard[k], after[k])
    m_random.set_precision("f16x3")
    try:
        x3 = m_random.ctc_loss(imgs, targets, tl, widths=widths, reduction="none")
    finally:
        m_random.set_precision("auto")
    np.testing.assert_array_equal(auto, x3)


def test_existing_paths_unchanged_after_a_ctc_call(pkg, synth, state_dict):
    C = synth.DEFAULT_VOCAB + 2
    imgs = synth.make_line_images(4, 640, seed=8)

    def run(m):
        return m.greedy(imgs), m.beam_frontend(imgs, 5, want_candidates=True)

    fresh = pkg.hctr_model(C).cuda(0)
    fresh.load_state_dict(state_dict)
    want_g, want_fe = run(fresh)
    del fresh
    m = pkg.hctr_model(C).cuda(0)
    m.load_state_dict(state_dict)
    targets = np.concatenate(want_g).astype(np.int32)
    tl = np.array([len(v) for v in want_g], np.int32)
    m.ctc_loss(imgs, targets, tl)
    got_g, got_fe = run(m)
    for a, b in zip(want_g, got_g):
        np.testing.assert_array_equal(a, b)
    for k in ("topk_idx", "topk_logp", "blank_logp", "cand_off", "cand_idx", "cand_logp"):
        np.testing.assert_array_equal(want_fe[k], got_fe[k], err_msg=k)


def test_reductions_and_criterion_on_engine_logits(pkg, synth, m_random):
    """reduction / zero_infinity against torch.nn.CTCLoss (CPU, fp32) on the engine's own logits; the criterion on numpy
    and torch input; the image path's reductions"""
    W = 300
    imgs = synth.make_line_images(4, W, seed=19)
    m_random.set_precision("f16")
    try:
        logits = m_random(imgs)                                  # numpy [W, B, C]
        labels = m_random.greedy(imgs)
        texts = [list(v) for v in labels]
        texts[1] = [5] * 200                                     # infeasible at T = 300 (200 + 199 > 300)
        texts[2] = []
        tl = np.array([len(v) for v in texts], np.int32)
        targets = np.array(sum(texts, []), np.int32)
        il = np.full(4, W, np.int32)
        lp = torch.from_numpy(logits).log_softmax(2)
        for red in ("none", "sum", "mean"):
            for zi in (False, True):
                want = torch.nn.CTCLoss(reduction=red, zero_infinity=zi)(lp, torch.from_numpy(targets).long(),
                                                                         torch.from_numpy(il).long(),
                                                                         torch.from_numpy(tl).long()).numpy()
                crit = pkg.CTCLoss(reduction=red, zero_infinity=zi).attach(m_random)
                got_np = crit(logits, targets, il, tl)
                assert isinstance(got_np, (np.ndarray, np.floating))
                got_t = crit(torch.from_numpy(logits).cuda(0), torch.from_numpy(targets), torch.from_numpy(il),
                             torch.from_numpy(tl))
                assert isinstance(got_t, torch.Tensor) and got_t.is_cuda
                np.testing.assert_array_equal(np.asarray(got_np), got_t.cpu().numpy())
                np.testing.assert_allclose(got_np, want, rtol=2e-5, atol=1e-3, err_msg="%s %s" % (red, zi))
                img = m_random.ctc_loss(imgs, targets, tl, reduction=red, zero_infinity=zi)
                np.testing.assert_allclose(img, got_np, rtol=2e-5, atol=1e-3, err_msg="image %s %s" % (red, zi))
        padded = np.zeros((4, int(tl.max())), np.int64)
        for b, v in enumerate(texts):
            padded[b, :len(v)] = v
        np.testing.assert_array_equal(m_random.ctc_loss(imgs, padded, tl, reduction="none"),
                                      m_random.ctc_loss(imgs, targets, tl, reduction="none"))
        tt = m_random.ctc_loss(torch.from_numpy(imgs).cuda(0), targets, tl)
        assert isinstance(tt, torch.Tensor) and tt.is_cuda
    finally:
        m_random.set_precision("auto")


def test_error_codes(pkg, synth, m_random):
    C, W = synth.DEFAULT_VOCAB + 2, 64
    imgs = synth.make_line_images(2, W, seed=1)
    logits = np.zeros((W, 2, C), np.float32)
    crit = pkg.CTCLoss(reduction="none").cuda(0)
    tl = np.array([2, 1], np.int32)
    for bad in ([0, 1, 2], [1, C, 2], [1, -3, 2]):               # ids outside [1, C-1]
        with pytest.raises(ValueError):
            crit(logits, np.array(bad, np.int32), None, tl)
        with pytest.raises(ValueError):
            m_random.ctc_loss(imgs, np.array(bad, np.int32), tl)
    with pytest.raises(ValueError):                             # length sum mismatch
        crit(logits, np.array([1, 2], np.int32), None, tl)
    for il in ([0, W], [W + 1, 5]):                             # input_lengths outside [1, W]
        with pytest.raises(ValueError):
            crit(logits, np.array([1, 2, C - 1], np.int32), np.array(il, np.int32), tl)
        with pytest.raises(ValueError):
            m_random.ctc_loss(imgs, np.array([1, 2, 3], np.int32), tl, input_lengths=np.array(il, np.int32))
    # the unknown id C-1 is a valid target
    assert np.isfinite(crit(logits, np.array([1, 2, C - 1], np.int32), None, tl)).all()
    # B = 0 is a no-op, at the C ABI with NULL pointers too
    lib = pkg.load_library()
    assert lib.hctr_ctc_loss_logits(crit._context(), None, 0, W, 0, C, None, None, None, None) == 0
    x = np.zeros((1, 128, W), np.uint8)
    assert lib.hctr_ctc_loss(m_random._ctx, x.ctypes.data_as(ctypes.c_void_p), 0, 0, None, 0, W, None, None, None,
                             None) == 0
    assert crit(np.zeros((W, 0, C), np.float32), np.zeros(0, np.int32), None, np.zeros(0, np.int32)).shape == (0,)
