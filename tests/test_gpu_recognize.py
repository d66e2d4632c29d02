"""GPU tests (-m gpu) of the greedy recognition (C ABI hctr_recognize / hctr_recognize_logits, ``hctr_model.recognize``,
``ctc_codec.recognize``): the decoded text with per-character spans, confidences and runners-up, the greedy path's
log-probability and the posterior of the text.

The reference project has no counterpart; the yardstick is tests/recognize_ref.py, a float64 numpy restatement of the
contract in include/hctr_hip.h. What must hold:
  * planted greedy paths (noise, +12 on the planted class, +6 on a planted runner-up) come back exactly - labels, spans
    and runners-up - with every float figure within the family's 1e-5 relative + 1e-3 of float64, the forced alignment
    of the decoded text returns the same spans, and path_logp <= -text_nll;
  * the collapse's edge cases, runs that straddle a 64-column chunk, exact ties and NaN rows follow the contract;
  * on flat random logits the labels are the greedy decode's and text_nll is the loss's, bit for bit;
  * host-pointer, device-pointer and repeated calls are bit-identical, and every output may be NULL;
  * the image path equals recognising the engine's own logits of the same mode, bit for bit, across internal passes;
  * no recognise call changes what greedy decoding, the loss, its gradient or the alignment compute.
"""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

import codec_cases
import recognize_ref as ref
from oracle import ctc_ref

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-5, 1e-3                      # engine figure vs float64 on the same logits (tests/test_gpu_ctc.py's)
FIELDS = ("labels", "lengths", "starts", "ends", "logps", "alt_labels", "alt_logps", "path_logp", "text_nll")
ERR_ARG = -1


@pytest.fixture(scope="module")
def ctc(pkg):
    return importlib.import_module(pkg.__name__ + ".ctc")


@pytest.fixture(scope="module")
def aligner(pkg):
    return pkg.CTCAligner().cuda(0)


@pytest.fixture(scope="module")
def ctx(aligner):
    return aligner._context()                 # a weightless context: the logits entry needs no weights


@pytest.fixture(scope="module")
def m_trained(pkg, synth):
    C = synth.DEFAULT_VOCAB + 2
    m = pkg.hctr_model(C, precision="auto").cuda(0)
    m.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    return m


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg="%s: NaN pattern" % what)
    inf = np.isinf(want)
    np.testing.assert_array_equal(got[inf], want[inf], err_msg="%s: infinities" % what)
    ok = ~np.isnan(want) & ~inf
    err = np.abs(got[ok] - want[ok])
    print("%s: max |d| %.3e over %d figures (largest |want| %.3f)" % (
        what, err.max() if err.size else 0.0, err.size, np.abs(want[ok]).max() if err.size else 0.0))
    assert (err <= RTOL * np.abs(want[ok]) + ATOL).all(), (what, got, want)


def _valid(a, lengths):
    """the valid entries of a [B, W] per-character array, line after line"""
    return np.concatenate([a[b, :int(n)] for b, n in enumerate(lengths)]) if len(lengths) else a[:0, 0]


def _same(a, b, what):
    for k in FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s: %s differs" % (what, k)


def _check_ref(rec, r, what, lp64=None):
    """rec (engine) against recognize_ref's dict r: the integers exact, the floats within tolerance; the runner-up is
    the float64 one, or - where float32 moves the peak among columns tied to rounding - that of another column of the
    span whose lp1 is within the tolerance of the span's largest"""
    np.testing.assert_array_equal(rec.lengths, r["lengths"], err_msg=what)
    for k in ("labels", "starts", "ends"):
        np.testing.assert_array_equal(getattr(rec, k), r[k], err_msg="%s %s" % (what, k))
    n = r["lengths"]
    assert all((getattr(rec, k)[b, n[b]:] == 0).all() for k in FIELDS[:7] if k != "lengths" for b in range(len(n)))
    _close(_valid(rec.logps, n), _valid(r["logps"], n), what + " char_logp")
    _close(rec.path_logp, r["path_logp"], what + " path_logp")
    _close(rec.text_nll, r["text_nll"], what + " text_nll")
    moved, got, want = 0, [], []
    for b in range(len(n)):
        for j in range(n[b]):
            if np.isnan(r["logps"][b, j]):
                assert np.isnan(rec.alt_logps[b, j]), (what, b, j)
                continue
            got.append(rec.alt_logps[b, j])
            want.append(r["alt_logps"][b, j])
            if rec.alt_labels[b, j] != r["alt_labels"][b, j]:
                assert lp64 is not None, (what, b, j)
                s, e, c = r["starts"][b, j], r["ends"][b, j], r["labels"][b, j]
                run = lp64[s:e, b, c]
                near = [t for t in range(s, e) if run[t - s] >= run.max() - ATOL and r["k2"][b, t] == rec.alt_labels[b, j]]
                assert near, (what, b, j)
                want[-1] = lp64[near[0], b, rec.alt_labels[b, j]]
                moved += 1
    _close(got, want, what + " alt_logp")
    print("%s: %d runners-up taken at another near-tied peak column" % (what, moved))


def _lp64(logits):
    return logits.astype(np.float64) - ref.lse64(logits)[..., None]


def _random_labels(rng, C, L, repeat=0.3):
    out = []
    for _ in range(L):
        out.append(out[-1] if out and rng.rand() < repeat else int(rng.randint(1, C - 1)))
    return out


# (W, B, C): C = 2051 is no multiple of 4 and just past one 8 x 256 sweep of the row pass; 7358 is the workload's
@pytest.mark.parametrize("W,B,C", [(96, 4, 37), (64, 3, 2051), (32, 2, 7358)])
def test_planted_paths(ctc, ctx, aligner, W, B, C):
    rng = np.random.RandomState(W + C)
    logits = np.empty((W, B, C), np.float32)
    texts, paths, alts = [], [], []
    for b in range(B):
        lab = _random_labels(rng, C, [W // 3, 0, W // 5, 1][b])
        logits[:, b], path, alt = ref.planted(rng, W, C, lab)
        texts.append(lab), paths.append(path), alts.append(alt)
    rec = ctc.recognize_logits(ctx, logits, 0)
    r = ref.recognize_ref(logits)
    lp = _lp64(logits)
    for b in range(B):                                     # the planted truth, exactly
        n = int(rec.lengths[b])
        assert rec.labels[b, :n].tolist() == texts[b], b
        np.testing.assert_array_equal(r["k1"][b], paths[b])
        np.testing.assert_array_equal(r["k2"][b], alts[b])
        for j in range(n):
            s, e, c = rec.starts[b, j], rec.ends[b, j], rec.labels[b, j]
            assert (paths[b][s:e] == c).all() and (s == 0 or paths[b][s - 1] != c) and (e == W or paths[b][e] != c)
            peak = s + int(np.argmax(lp[s:e, b, c]))
            assert rec.alt_labels[b, j] == alts[b][peak], (b, j)
    _check_ref(rec, r, "planted (%d, %d, %d)" % (W, B, C))
    np.testing.assert_array_equal(rec.alt_labels, r["alt_labels"])
    assert (rec.path_logp <= -rec.text_nll + ATOL).all(), (rec.path_logp, rec.text_nll)
    # the forced alignment of the decoded text is the greedy path
    tg = np.concatenate(rec.label_lists()).astype(np.int32)
    al = aligner(logits, tg, None, rec.lengths)
    np.testing.assert_array_equal(al.starts, _valid(rec.starts, rec.lengths))
    np.testing.assert_array_equal(al.ends, _valid(rec.ends, rec.lengths))
    _close(al.logps, _valid(rec.logps, rec.lengths).astype(np.float64), "aligner span_logp")
    confs = [(conf, ap) for ln in rec.lines() for _, _, _, conf, _, ap in ln]
    assert len(confs) == int(rec.lengths.sum()) and all(0.5 < c <= 1.0 and 0.0 < a < 0.5 for c, a in confs)
    assert ((rec.text_posterior > 0.0) & (rec.text_posterior <= 1.0 + 1e-6)).all()


def _spans(rec, b=0):
    return [(int(rec.labels[b, j]), int(rec.starts[b, j]), int(rec.ends[b, j])) for j in range(int(rec.lengths[b]))]


def test_collapse_edge_cases(ctc, ctx):
    """the host test's hand-written cases on the device, and runs that straddle columns 63/64 and 127/128"""
    cases = [(name, k1, spans) for name, k1, spans in ref.HAND_CASES]
    cases += [("W = %d straddle" % W, k1, spans) for W, k1, spans in ref.STRADDLE_CASES]
    for name, k1, spans in cases:
        z = ref.hand_logits(np.random.RandomState(len(k1)), k1)
        rec = ctc.recognize_logits(ctx, z, 0)
        assert _spans(rec) == spans, name
        _check_ref(rec, ref.recognize_ref(z), name)
        if name == "all blank":
            _close(rec.text_nll, -rec.path_logp.astype(np.float64), "all blank: text_nll == -path_logp")


def test_ties(ctc, ctx):
    W, C = 10, 37
    z = np.zeros((W, 3, C), np.float32)
    z[4, 1, 3] = 1.0                                       # line 1: one character, every other class tied
    z[7, 1, 5] = z[7, 1, 9] = 2.0                          # two classes exactly tied: the lower index is the label
    z[2, 2, 1] = z[2, 2, 3] = 2.0                          # line 2: the winner is class 1, tied with class 3
    z[4, 2, 1] = 1.0                                       # class 1 alone: the others tie, class 0 first
    z[6, 2, :] = -np.inf                                   # one finite class: the runner-up is the first -inf,
    z[6, 2, 4] = 0.0                                       # which the row kernel's last thread has to supply
    z[8, 2, :] = -np.inf
    z[8, 2, 1] = z[8, 2, 0] = 0.5                          # two finite classes, tied, class 0 (the blank) among them
    rec = ctc.recognize_logits(ctx, z, 0)
    assert rec.lengths.tolist() == [0, 2, 3]               # all-zero rows: argmax 0, an empty text
    assert _spans(rec, 2) == [(1, 2, 3), (1, 4, 5), (4, 6, 7)]             # column 8 goes to the blank: first maximum
    assert rec.alt_labels[2, :3].tolist() == [3, 0, 0]
    assert rec.alt_logps[2, 0] == rec.logps[2, 0] and rec.logps[2, 2] == 0.0 and np.isneginf(rec.alt_logps[2, 2])
    assert np.isfinite(rec.path_logp).all() and np.isfinite(rec.text_nll).all()
    np.testing.assert_allclose(rec.path_logp[0], -W * np.log(C), rtol=1e-6)      # lp = -log C in every column
    np.testing.assert_allclose(rec.text_nll[0], W * np.log(C), rtol=1e-6)
    assert _spans(rec, 1) == [(3, 4, 5), (5, 7, 8)]
    # k2 = the first index of the largest among the others: class 0 under a lone winner, the tied partner under a tie
    # (had class 0 won, as in an all-zero row, it would be class 1 - a column without a character, which no output shows)
    assert rec.alt_labels[1, :2].tolist() == [0, 9]
    np.testing.assert_allclose(rec.alt_logps[1, 0], -np.log(C - 1 + np.e), rtol=1e-6)
    assert rec.alt_logps[1, 1] == rec.logps[1, 1]
    _check_ref(rec, ref.recognize_ref(z), "ties")
    z0 = np.zeros((3, 1, C), np.float32)
    z0[1, 0, 0] = 1.0                                      # class 0 wins: the runner-up is class 1
    assert ref.recognize_ref(z0)["k2"][0].tolist() == [1, 1, 1]


def test_nan_rows(pkg, ctc, ctx):
    """tests/golden/codec_cases.json's peaky_small logits with the NaN / inf rows of the parity suite's
    test_nan_logits_follow_numpy_argmax planted in them (the golden file itself stores no NaN)"""
    name, seed, W, B, C, style = codec_cases.CODEC_CASES[0]
    logits = codec_cases.gen_logits(seed, W, B, C, style)
    logits[3, 0, 4] = np.nan
    logits[3, 0, 6] = np.nan                               # two NaNs in a row: the first wins
    logits[7, 1, 0] = np.nan                               # NaN on the blank
    logits[9, 0, :] = -np.inf                              # all -inf: index 0
    logits[10, 1, 2] = np.inf
    # a three-column run of class 5 whose last column is NaN in class 5 itself and whose peak is a clean column: the
    # character's sum is NaN, so its alt_logp must be NaN although the peak's own lp2 is a number
    logits[19:24, 2, :] = 0.0
    logits[19, 2, 0] = logits[23, 2, 0] = 9.0
    logits[20, 2, 5], logits[21, 2, 5], logits[22, 2, 5] = 8.0, 11.0, np.nan
    cd = pkg.ctc_codec(codec_cases.vocab(C)).cuda(0)
    texts, rec = cd.recognize(logits)
    assert texts == cd.decode(logits) == ctc_ref.CtcCodecRef(codec_cases.vocab(C)).decode(logits)
    lab, n = np.empty((B, W), np.int32), np.empty(B, np.int32)
    vp = ctypes.c_void_p
    assert pkg.load_library().hctr_decode_greedy_logits(ctx, logits.ctypes.data_as(vp), 0, W, B, C, lab.ctypes.data_as(vp),
                                                        n.ctypes.data_as(vp)) == 0
    np.testing.assert_array_equal(rec.lengths, n)
    np.testing.assert_array_equal(_valid(rec.labels, n), _valid(lab, n))
    r = ref.recognize_ref(logits)
    assert np.isnan(r["path_logp"]).tolist() == [True, True, True] and np.isnan(r["text_nll"]).tolist() == [True, True, True]
    j = [j for j in range(n[2]) if (rec.labels[2, j], rec.starts[2, j], rec.ends[2, j]) == (5, 20, 23)]
    assert len(j) == 1 and np.isnan(rec.logps[2, j[0]]) and np.isnan(rec.alt_logps[2, j[0]])
    assert np.isfinite(_valid(rec.logps, n)).sum() > 10                  # the other characters keep their figures
    assert np.isnan(_valid(r["logps"], n)).sum() >= 2 and not np.isnan(_valid(r["logps"], n)).all()
    _check_ref(rec, r, "NaN rows")                         # NaN exactly where float64 has it; alt_label there is free


def test_flat_random_logits(pkg, ctc, ctx):
    W, B, C = 131, 5, 7358
    rng = np.random.RandomState(131)
    logits = rng.standard_normal((W, B, C)).astype(np.float32)
    logits[:, 3, 0] += 5.0                                 # a line of fewer characters
    rec = ctc.recognize_logits(ctx, logits, 0)
    lab, n = np.empty((B, W), np.int32), np.empty(B, np.int32)
    vp = ctypes.c_void_p
    assert pkg.load_library().hctr_decode_greedy_logits(ctx, logits.ctypes.data_as(vp), 0, W, B, C, lab.ctypes.data_as(vp),
                                                        n.ctypes.data_as(vp)) == 0
    np.testing.assert_array_equal(rec.lengths, n)
    np.testing.assert_array_equal(_valid(rec.labels, n), _valid(lab, n))
    assert n[3] < 100 < n[0]
    nll = ctc.loss_logits(ctx, logits, 0, _valid(rec.labels, n), n, None)
    assert nll.tobytes() == rec.text_nll.tobytes(), (nll, rec.text_nll)
    _check_ref(rec, ref.recognize_ref(logits), "flat random", _lp64(logits))


def _call(lib, ctx, logits_ptr, on_dev, W, B, C, outs):
    vp = ctypes.c_void_p
    return lib.hctr_recognize_logits(ctx, logits_ptr, on_dev, W, B, C,
                                     *[None if a is None else a.ctypes.data_as(vp) for a in outs])


def test_determinism_and_null_outputs(pkg, ctc, ctx):
    rng = np.random.RandomState(17)
    W, B, C = 70, 3, 50
    logits = (rng.standard_normal((W, B, C)) * 3).astype(np.float32)
    host = ctc.recognize_logits(ctx, logits, 0)
    dev_t = torch.from_numpy(logits).cuda(0)
    torch.cuda.synchronize()
    _same(host, ctc.recognize_logits(ctx, dev_t, 1), "device pointer")
    ctc.recognize_logits(ctx, rng.standard_normal((9, 1, 5)).astype(np.float32), 0)         # another layout in between
    _same(host, ctc.recognize_logits(ctx, logits, 0), "repeated call")
    lib = pkg.load_library()
    vp = ctypes.c_void_p
    full = [getattr(host, k) for k in FIELDS]
    assert _call(lib, ctx, logits.ctypes.data_as(vp), 0, W, B, C, [None] * 9) == 0
    for i, k in enumerate(FIELDS):                         # every output alone
        outs = [None] * 9
        outs[i] = np.full(full[i].shape, 77, full[i].dtype)
        assert _call(lib, ctx, vp(dev_t.data_ptr()), 1, W, B, C, outs) == 0, k
        assert outs[i].tobytes() == full[i].tobytes(), k
    # errors leave the context usable; B == 0 is a no-op
    outs = [np.zeros_like(a) for a in full]
    assert _call(lib, ctx, None, 0, W, B, C, outs) == ERR_ARG
    assert _call(lib, ctx, logits.ctypes.data_as(vp), 0, W, B, 1, outs) == ERR_ARG
    assert _call(lib, ctx, logits.ctypes.data_as(vp), 0, 0, B, C, outs) == ERR_ARG
    assert _call(lib, ctx, None, 0, W, 0, C, [None] * 9) == 0
    _same(host, ctc.recognize_logits(ctx, logits, 0), "after errors")


def test_text_beyond_the_label_limit_gets_nan(ctc, ctx):
    """2100 kept columns exceed the loss's 2047 labels: that line's text_nll is NaN, nothing else changes"""
    W, C = 2100, 4
    z = np.zeros((W, 2, C), np.float32)
    z[np.arange(W), 0, 1 + (np.arange(W) & 1)] = 8.0       # 1 2 1 2 ...: every column a character
    z[:, 1, 0] = 8.0
    z[5:9, 1, 2] = 16.0
    rec = ctc.recognize_logits(ctx, z, 0)
    assert rec.lengths.tolist() == [W, 1] and _spans(rec, 1) == [(2, 5, 9)]
    assert np.isnan(rec.text_nll[0]) and np.isfinite(rec.text_nll[1]) and np.isfinite(rec.path_logp).all()
    alone = ctc.loss_logits(ctx, np.ascontiguousarray(z[:, 1:2]), 0, np.array([2], np.int32), np.array([1], np.int32), None)
    assert alone.tobytes() == rec.text_nll[1:].tobytes()
    assert (rec.ends[0] - rec.starts[0] == 1).all()


def _images(synth, W=160):
    return synth.make_font_lines(3, W, 40 + W), np.array([W, W - 29, W - 50], np.int32)


def test_images(pkg, synth, ctc, m_trained):
    """hctr_recognize(images) == hctr_recognize_logits(hctr_forward_logits(images)) of the same mode, bit for bit, also
    with the batch split into internal passes; the labels are hctr_greedy's; auto takes every line in f16x3"""
    C = synth.DEFAULT_VOCAB + 2
    imgs, widths = _images(synth)
    W = imgs.shape[-1]
    by_mode = {}
    try:
        for mode in ("f16", "f16x3"):
            m_trained.set_precision(mode)
            rec = m_trained.recognize(imgs, widths=widths)
            greedy = m_trained.greedy(imgs, widths=widths)
            assert sum(len(v) for v in greedy) > 0
            for a, b in zip(rec.label_lists(), greedy):
                np.testing.assert_array_equal(a, b, err_msg=mode)
            logits = m_trained(torch.from_numpy(imgs).cuda(0), widths=widths)
            torch.cuda.synchronize()
            _same(rec, ctc.recognize_logits(m_trained._ctx, logits, 1), mode + " logits path")
            for inp in (torch.from_numpy(imgs), torch.from_numpy(imgs).cuda(0)):
                _same(rec, m_trained.recognize(inp, widths=widths), mode + " torch input")
            by_mode[mode] = rec
    finally:
        m_trained.set_precision("auto")
    m_trained.greedy(imgs, widths=widths)
    guard0 = m_trained.last_guard()
    auto = m_trained.recognize(imgs, widths=widths)
    guard1 = m_trained.last_guard()
    _same(by_mode["f16x3"], auto, "auto")
    assert guard0["lines"] == guard1["lines"] and guard0["flagged"] == guard1["flagged"]
    for k in ("flags", "min_margin", "scale"):
        np.testing.assert_array_equal(guard0[k], guard1[k])
    os.environ["HCTR_MAX_COLS"] = "600"                    # f16x3 passes of 200 columns: one line each
    try:
        small = pkg.hctr_model(C, precision="auto").cuda(0)
    finally:
        del os.environ["HCTR_MAX_COLS"]
    small.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    assert small.lines_per_pass(3, W, f16x3=True) < 3
    _same(auto, small.recognize(imgs, widths=widths), "split passes")
    confs = [c for ln in auto.lines() for _, _, _, c, _, _ in ln]
    assert confs and all(0.0 < c <= 1.0 for c in confs)


def test_no_side_effects(pkg, synth, ctc, m_trained):
    rng = np.random.RandomState(12)
    W, B, C = 90, 3, 40
    logits = rng.standard_normal((W, B, C)).astype(np.float32)
    tl = np.array([7, 0, 25], np.int32)
    targets = np.concatenate([_random_labels(rng, C, L) for L in tl] + [[]]).astype(np.int32)
    imgs = synth.make_font_lines(3, 96, 31)
    ctx = m_trained._ctx

    def others():
        g = m_trained.greedy(imgs)
        guard = m_trained.last_guard()
        nll = ctc.loss_logits(ctx, logits, 0, targets, tl, None)
        nll2, grad = ctc.loss_grad_logits(ctx, logits, 0, targets, tl, None, None)
        al = ctc.align_logits(ctx, logits, 0, targets, tl, None)
        return g, guard, nll, nll2, grad, al

    g0, guard0, nll0, nll20, grad0, al0 = others()
    ctc.recognize_logits(ctx, rng.standard_normal((200, 2, 300)).astype(np.float32), 0)       # another scratch layout
    rec = m_trained.recognize(imgs)
    assert np.isfinite(rec.path_logp).all()
    g1, guard1, nll1, nll21, grad1, al1 = others()
    for x, y in zip(g0, g1):
        np.testing.assert_array_equal(x, y)
    for x, y in ((nll0, nll1), (nll20, nll21), (grad0, grad1)):
        assert x.tobytes() == y.tobytes()
    for k in ("paths", "scores", "starts", "ends", "logps"):
        assert getattr(al0, k).tobytes() == getattr(al1, k).tobytes(), k
    assert guard0["lines"] == guard1["lines"] and guard0["flagged"] == guard1["flagged"]
    for k in ("flags", "min_margin", "scale"):
        np.testing.assert_array_equal(guard0[k], guard1[k])


def test_codec_surface(pkg, ctc):
    name, seed, W, B, C, style = codec_cases.CODEC_CASES[3]
    logits = codec_cases.gen_logits(seed, W, B, C, style)
    cd = pkg.ctc_codec(codec_cases.vocab(C)).cuda(0)
    texts, rec = cd.recognize(logits)
    assert texts == cd.decode(logits) and isinstance(rec, pkg.Recognition)
    dev = torch.from_numpy(logits).cuda(0)
    texts2, rec2 = cd.recognize(dev)
    assert texts2 == texts
    _same(rec, rec2, "CUDA tensor")
    cd.set_beam_search(ngram_path="zero", use_tfm_pred=False)      # recognize stays greedy whatever decode is set to
    assert cd.recognize(logits)[0] == texts
