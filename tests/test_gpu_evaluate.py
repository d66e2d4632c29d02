"""GPU tests (-m gpu) of the evaluation (C ABI hctr_edit_distance / hctr_evaluate / hctr_evaluate_logits,
``hctr_model.evaluate``, ``ctc_codec.evaluate``, ``hctr_amd.edit_distance``): the edit distance of decoded text against
its transcription with the error counts and the character alignment.

The reference's figure is editdistance.eval per line (test.py:275); the yardstick here is tests/edit_ref.py, the numpy
restatement of the contract in include/hctr_hip.h. Everything is integer: every comparison is ==, no tolerances.
What must hold:
  * at every rung of the sweep's instance ladder (read from csrc/kernels.hip), at its last reference length and one
    beyond, at L = 0, 1 and 2047, with hypotheses shorter, equal, longer, empty and of the full stride, in batches that
    mix long and short lines, over a tie-rich alphabet of 2 and one of 7000: edits, counts and both maps;
  * lines whose hand-over across a wave boundary carries the decisive value at every step;
  * the distance-only instance and every subset of NULL outputs give the same figures;
  * arbitrary int32 symbols; argument errors leave the context usable; repeated calls agree bit for bit;
  * hctr_evaluate_logits and hctr_evaluate decode exactly as the greedy entries do, in all three modes, across internal
    passes and through the guarded re-run, and change nothing the other entries compute.
"""
import ctypes
import importlib
import importlib.util
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import edit_ref
import recognize_ref
from conftest import PKG, ROOT
from oracle import ctc_ref

pytestmark = pytest.mark.gpu

ERR_ARG = -1
LIMIT = 2047
OUTS = ("edits", "counts", "ref_map", "hyp_map")


def ladder():
    """[(NS, NW)] as csrc/kernels.hip declares it"""
    with open(os.path.join(ROOT, PKG, "csrc", "kernels.hip")) as f:
        line = re.search(r"#define HCTR_EDIT_LADDER\(X\)(.*)", f.read()).group(1)
    rungs = [(int(a), int(b)) for a, b in re.findall(r"X\((\d+),\s*(\d+)\)", line)]
    assert rungs and 64 * rungs[-1][0] * rungs[-1][1] > LIMIT
    return rungs


RUNGS = ladder()
ROWS = [64 * ns * nw for ns, nw in RUNGS]


@pytest.fixture(scope="module")
def ctc(pkg):
    return importlib.import_module(pkg.__name__ + ".ctc")


@pytest.fixture(scope="module")
def ctx(pkg):
    bound = pkg.CTCAligner().cuda(0)
    yield bound._context()                      # a weightless context: the entry needs no weights
    del bound


@pytest.fixture(scope="module")
def m_trained(pkg, synth):
    C = synth.DEFAULT_VOCAB + 2
    m = pkg.hctr_model(C, precision="auto").cuda(0)
    m.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    return m


def _noisy(rng, ref, H, A):
    """a hypothesis of length H: the reference with random substitutions, cut or extended"""
    h = np.array(ref[:H], np.int64)
    flip = rng.rand(h.size) < 0.2
    h[flip] = rng.randint(0, A, int(flip.sum()))
    return np.concatenate([h, rng.randint(0, A, H - h.size)])


def _batch(pairs):
    """(hyp [B, stride], hyp_lengths, ref, ref_lengths) of [(ref, hyp)]; the stride is the longest hypothesis"""
    n = np.array([len(h) for _, h in pairs], np.int32)
    hyp = np.zeros((len(pairs), max(1, int(n.max()))), np.int32)
    for b, (_, h) in enumerate(pairs):
        hyp[b, :n[b]] = h
    tl = np.array([len(r) for r, _ in pairs], np.int32)
    ref = np.concatenate([np.asarray(r, np.int32) for r, _ in pairs] + [np.zeros(0, np.int32)]).astype(np.int32)
    return hyp, n, ref, tl


def _same(ev, want, what):
    for k in OUTS:
        np.testing.assert_array_equal(getattr(ev, k), want[k], err_msg="%s: %s" % (what, k))


def _check(ctc, ctx, pairs, what):
    hyp, n, ref, tl = _batch(pairs)
    ev = ctc.edit_distance_labels(ctx, hyp, n, ref, tl)
    _same(ev, edit_ref.batch(hyp, n, ref, tl), what)
    only = ctc.edit_distance_labels(ctx, hyp, n, ref, tl, maps=False)
    np.testing.assert_array_equal(only.edits, ev.edits, err_msg=what + ": distance-only")
    return ev


# the longest reference of a batch picks the rung: each rung's last length and one beyond it, and the range's ends
EDGES = sorted({0, 1, LIMIT} | {min(r, LIMIT) for r in ROWS} | {r + 1 for r in ROWS if r + 1 <= LIMIT})


@pytest.mark.parametrize("A", [2, 7000])
@pytest.mark.parametrize("Lmax", EDGES)
def test_every_rung(ctc, ctx, Lmax, A):
    rng = np.random.RandomState(Lmax * 3 + A)
    long_ref = rng.randint(0, A, Lmax)
    pairs = [(long_ref, _noisy(rng, long_ref, Lmax, A)),                   # H == L
             (long_ref, _noisy(rng, long_ref, Lmax // 2, A)),              # shorter
             (long_ref, _noisy(rng, long_ref, Lmax + 37, A)),              # longer: H == hyp_stride
             (long_ref, rng.randint(0, A, Lmax)),                          # unrelated
             (long_ref, []),                                               # H == 0
             ([], rng.randint(0, A, 4)),                                   # lines far below the rung
             (rng.randint(0, A, 3), rng.randint(0, A, 5)),
             (rng.randint(0, A, 5), []),
             (rng.randint(0, A, min(Lmax, 70)), rng.randint(0, A, 9))]
    ev = _check(ctc, ctx, pairs, "Lmax %d, alphabet %d" % (Lmax, A))
    assert ev.hyp_map.shape[1] == Lmax + 37 and ev.lengths[2] == Lmax + 37
    c = ev.counts
    np.testing.assert_array_equal(c[:, 0] + c[:, 1] + c[:, 2], ev.target_lengths)
    np.testing.assert_array_equal(c[:, 0] + c[:, 1] + c[:, 3], ev.lengths)
    np.testing.assert_array_equal(c[:, 1] + c[:, 2] + c[:, 3], ev.edits)


@pytest.mark.parametrize("ns,nw", [r for r in RUNGS if r[1] > 1][::2] + [RUNGS[-1]])
def test_wave_boundary(ctc, ctx, ns, nw):
    """all-equal against all-different: every cell's value comes down the diagonal or across the boundary"""
    rows = 64 * ns * nw
    pin = min(rows, LIMIT)                                                 # a line that pins the rung
    lengths = [64 * ns * w + d for w in (1, 2) for d in (-1, 0, 1) if 64 * ns * w + d <= pin]
    pairs = []
    for L in lengths + [pin]:
        same, diff = np.full(L, 7), np.arange(100, 100 + L + 1)
        pairs += [(same, diff[:L]), (diff[:L], same), (same, diff[:L + 1]), (diff[:L], same[:L - 1])]
    ev = _check(ctc, ctx, pairs, "rung %d x %d" % (ns, nw))
    assert (ev.counts[:, 0] == 0).all() and (ev.edits == np.maximum(ev.target_lengths, ev.lengths)).all()
    half = np.arange(pin) % 2                                              # equal runs against alternating symbols
    _check(ctc, ctx, [(half, np.zeros(pin, np.int64)), (np.zeros(pin, np.int64), half), (half, half[1:])],
           "rung %d x %d, two symbols" % (ns, nw))


def _raw(lib, ctx, hyp, n, stride, ref, tl, B, outs):
    vp = ctypes.c_void_p
    p = lambda a: None if a is None else a.ctypes.data_as(vp)
    return lib.hctr_edit_distance(ctx, p(hyp), p(n), stride, p(ref), p(tl), B, *[p(a) for a in outs])


def _mixed_case(seed=5, A=4):
    rng = np.random.RandomState(seed)
    pairs = []
    for L, H in ((150, 140), (0, 3), (64, 64), (65, 90), (3, 0), (0, 0), (1, 1), (129, 31)):
        r = rng.randint(0, A, L)
        pairs.append((r, _noisy(rng, r, H, A)))
    return _batch(pairs)


def test_every_subset_of_null_outputs(pkg, ctx):
    hyp, n, ref, tl = _mixed_case()
    B, stride = hyp.shape
    want = edit_ref.batch(hyp, n, ref, tl)
    lib = pkg.load_library()
    for mask in itertools.product((False, True), repeat=4):
        outs = [np.full(want[k].shape, 77, np.int32) if on else None for k, on in zip(OUTS, mask)]
        assert _raw(lib, ctx, hyp, n, stride, ref, tl, B, outs) == 0, mask
        for k, a in zip(OUTS, outs):
            if a is not None:
                np.testing.assert_array_equal(a, want[k], err_msg="%s with %s" % (k, mask))


def test_symbols(ctc, ctx):
    big = np.array([-2 ** 31, 2 ** 31 - 1, -1, 0, 1, 2 ** 30, -2 ** 30, 65536, -65536], np.int64)
    rng = np.random.RandomState(9)
    r = big[rng.randint(0, big.size, 200)]
    h = _noisy(rng, r, 180, 5)                                             # 0..4 replace a fifth: 2, 3, 4 equal no reference symbol
    h2 = np.where(rng.rand(200) < 0.3, 12345, r)                           # a symbol the reference never holds
    ev = _check(ctc, ctx, [(r, h), (r, h2), (big, big[::-1]), (big, big)], "int32 symbols")
    assert ev.edits[3] == 0 and ev.counts[3].tolist() == [9, 0, 0, 0] and ev.edits[1] == int((h2 != r).sum())


def test_errors_leave_the_context_usable(pkg, ctx):
    hyp, n, ref, tl = _mixed_case()
    B, stride = hyp.shape
    want = edit_ref.batch(hyp, n, ref, tl)
    lib = pkg.load_library()

    def good():
        outs = [np.full(want[k].shape, 77, np.int32) for k in OUTS]
        assert _raw(lib, ctx, hyp, n, stride, ref, tl, B, outs) == 0
        for k, a in zip(OUTS, outs):
            np.testing.assert_array_equal(a, want[k], err_msg=k)

    good()
    e = np.zeros(B, np.int32)
    long_tl = tl.copy()
    long_tl[2] = LIMIT + 1
    long_ref = np.zeros(int(long_tl.sum()), np.int32)
    assert _raw(lib, ctx, hyp, n, stride, long_ref, long_tl, B, [e, None, None, None]) == ERR_ARG
    assert b"ref_lengths[2]" in lib.hctr_last_error(ctx)
    good()
    bad_n = n.copy()
    bad_n[4] = stride + 1
    assert _raw(lib, ctx, hyp, bad_n, stride, ref, tl, B, [e, None, None, None]) == ERR_ARG
    assert b"hyp_lengths[4]" in lib.hctr_last_error(ctx)
    good()
    neg = tl.copy()
    neg[0] = -1
    assert _raw(lib, ctx, hyp, n, stride, ref, neg, B, [e, None, None, None]) == ERR_ARG
    assert _raw(lib, ctx, None, n, stride, ref, tl, B, [e, None, None, None]) == ERR_ARG
    good()
    assert _raw(lib, ctx, None, None, stride, None, None, 0, [None] * 4) == 0          # B == 0: a no-op
    good()
    # exactly at the limit
    r = np.arange(LIMIT, dtype=np.int32)
    one = np.zeros(1, np.int32)
    assert _raw(lib, ctx, r[None, :].copy(), np.array([LIMIT], np.int32), LIMIT, r, np.array([LIMIT], np.int32), 1,
                [one, None, None, None]) == 0 and one[0] == 0


def test_determinism(ctc, ctx):
    hyp, n, ref, tl = _mixed_case(seed=6)
    a = ctc.edit_distance_labels(ctx, hyp, n, ref, tl)
    b = ctc.edit_distance_labels(ctx, hyp, n, ref, tl)
    rng = np.random.RandomState(1)
    big = rng.randint(0, 3, 1500)
    ctc.edit_distance_labels(ctx, *_batch([(big, _noisy(rng, big, 1400, 3))] * 3))        # the scratch grows
    c = ctc.edit_distance_labels(ctx, hyp, n, ref, tl)
    for k in OUTS:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes() == getattr(c, k).tobytes(), k
    _same(a, edit_ref.batch(hyp, n, ref, tl), "determinism")


def _random_labels(rng, C, L, repeat=0.3):
    out = []
    for _ in range(L):
        out.append(out[-1] if out and rng.rand() < repeat else int(rng.randint(1, C - 1)))
    return out


@pytest.mark.parametrize("W,B,C", [(96, 4, 37), (64, 3, 2051)])
def test_evaluate_logits(pkg, ctc, ctx, W, B, C):
    """planted greedy paths, as test_gpu_recognize.test_planted_paths builds them; line 1 decodes to the empty text and
    line 0 has an empty target"""
    rng = np.random.RandomState(W + C)
    logits = np.empty((W, B, C), np.float32)
    texts = []
    for b in range(B):
        lab = _random_labels(rng, C, [W // 3, 0, W // 5, 1][b])
        logits[:, b] = recognize_ref.planted(rng, W, C, lab)[0]
        texts.append(lab)
    truths = [[]] + [[int(v) for v in _noisy(rng, np.array(t + [1, 2]), len(t) + 1, C - 2) + 1] for t in texts[1:]]
    tl = np.array([len(t) for t in truths], np.int32)
    tg = np.array([v for t in truths for v in t], np.int32)
    lab, n = np.empty((B, W), np.int32), np.empty(B, np.int32)
    vp = ctypes.c_void_p
    assert pkg.load_library().hctr_decode_greedy_logits(ctx, logits.ctypes.data_as(vp), 0, W, B, C, lab.ctypes.data_as(vp),
                                                        n.ctypes.data_as(vp)) == 0
    assert n.tolist() == [len(t) for t in texts] and n[1] == 0
    for on_dev, z in ((0, logits), (1, torch.from_numpy(logits).cuda(0))):
        torch.cuda.synchronize()
        ev = ctc.evaluate_logits(ctx, z, on_dev, tg, tl)
        np.testing.assert_array_equal(ev.lengths, n)
        for b in range(B):
            np.testing.assert_array_equal(ev.labels[b, :n[b]], lab[b, :n[b]])
        _same(ev, edit_ref.batch(ev.labels, n, tg, tl), "evaluate_logits (%d, %d, %d)" % (W, B, C))
        only = ctc.evaluate_logits(ctx, z, on_dev, tg, tl, maps=False)
        np.testing.assert_array_equal(only.edits, ev.edits)
    assert ev.edits[0] == n[0] and ev.edits[1] == tl[1]
    with pytest.raises(ValueError):                                        # hctr_ctc_loss_logits' check of the ids
        ctc.evaluate_logits(ctx, logits, 0, np.where(tg == tg[0], C, tg), tl)
    with pytest.raises(ValueError):
        ctc.evaluate_logits(ctx, logits, 0, np.where(tg == tg[0], 0, tg), tl)
    _same(ctc.evaluate_logits(ctx, logits, 0, tg, tl), edit_ref.batch(ev.labels, n, tg, tl), "after errors")


def image_case(synth, W=320):
    """a handful of font lines of unequal widths and their own texts with a few characters altered"""
    widths = np.array([W, W - 29, W - 50, W, W - 72], np.int32)
    imgs, boxes = synth.make_font_lines(len(widths), W, 40 + W, with_truth=True)
    chars = synth.characters()
    truths = [synth.font_truth_text(bx, int(w)) for bx, w in zip(boxes, widths)]
    assert all(len(t) >= 2 for t in truths)
    truths[0] = truths[0][:1] + chars[17] + truths[0][2:]                  # a substitution
    truths[1] = truths[1][:1] + truths[1][2:]                              # the decode has one more: an insertion
    truths[2] = truths[2][:1] + chars[4000] + truths[2][1:]                # the truth has one more: a deletion
    truths[4] = ""                                                         # an empty truth
    return imgs, widths, truths


def _evaluate_like_greedy(m, codec, imgs, widths, truths, what):
    tg, tl = codec.encode(truths)
    greedy = m.greedy(imgs, widths=widths)
    g1 = m.last_guard()
    m.greedy(imgs[:2], widths=widths[:2])                                  # the guard figures of another batch in between
    ev = m.evaluate(imgs, tg, tl, widths=widths)
    g2 = m.last_guard()
    assert sum(len(v) for v in greedy) > 0
    np.testing.assert_array_equal(ev.lengths, [len(v) for v in greedy], err_msg=what)
    for b, v in enumerate(greedy):
        np.testing.assert_array_equal(ev.labels[b, :len(v)], v, err_msg=what)
    _same(ev, edit_ref.batch(ev.labels, ev.lengths, tg, tl), what)
    only = m.evaluate(imgs, tg, tl, widths=widths, maps=False)
    np.testing.assert_array_equal(only.edits, ev.edits, err_msg=what)
    assert only.counts is None and ev.cer == only.cer
    assert (g1["lines"], g1["flagged"]) == (g2["lines"], g2["flagged"]), what       # hctr_last_guard: as after greedy
    for k in ("flags", "min_margin", "scale"):
        np.testing.assert_array_equal(g1[k], g2[k], err_msg=what)
    return ev, g2


def test_images(pkg, synth, m_trained):
    imgs, widths, truths = image_case(synth)
    codec = pkg.ctc_codec(synth.characters())
    try:
        for mode in ("f16", "f16x3", "auto"):
            m_trained.set_precision(mode)
            ev, _ = _evaluate_like_greedy(m_trained, codec, imgs, widths, truths, mode)
            for inp in (torch.from_numpy(imgs), torch.from_numpy(imgs).cuda(0)):
                _same(m_trained.evaluate(inp, ev.targets, ev.target_lengths, widths=widths),
                      {k: getattr(ev, k) for k in OUTS}, mode + " torch input")
    finally:
        m_trained.set_precision("auto")
    hits, S, D, I = ev.totals
    assert S > 0 and D > 0 and I > 0 and hits > 0, ev.totals
    assert ev.edits[4] == ev.lengths[4] and ev.cr == (ev.total_chars - D - S) / ev.total_chars
    assert len(list(ev.lines())) == 5 and sum(ev.confusions().values()) == S


def test_images_guarded_rerun(pkg, synth, m_trained):
    """a guard setting that flags the least certain line only: its results come from the f16x3 re-run"""
    imgs, widths, truths = image_case(synth)
    codec = pkg.ctc_codec(synth.characters())
    m_trained.greedy(imgs, widths=widths)
    mg = np.sort(m_trained.last_guard()["min_margin"].astype(np.float64))
    try:
        m_trained.set_guard(rel=0.0, abs=(mg[0] + mg[1]) / 4 if mg[1] > mg[0] else mg[0])
        _, g = _evaluate_like_greedy(m_trained, codec, imgs, widths, truths, "guarded")
        assert 1 <= int(g["flags"].sum()) < len(widths) or mg[1] == mg[0]
        m_trained.set_guard(rel=0.0, abs=1e9)                              # every line runs again
        _, g = _evaluate_like_greedy(m_trained, codec, imgs, widths, truths, "all flagged")
        assert int(g["flags"].sum()) == len(widths)
    finally:
        m_trained.set_guard()


def test_images_in_several_passes(pkg, synth, m_trained, tmp_path):
    imgs, widths, truths = image_case(synth)
    tg, tl = pkg.ctc_codec(synth.characters()).encode(truths)
    ev = m_trained.evaluate(imgs, tg, tl, widths=widths)
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, HCTR_MAX_COLS="700")                            # two lines of 320 columns per f16 pass
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "evaluate_child.py"), out], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(out)
    assert int(got["passes"]) >= 3
    for k in OUTS + ("lengths",):
        np.testing.assert_array_equal(got[k], getattr(ev, k), err_msg=k)
    for b, n in enumerate(ev.lengths):
        np.testing.assert_array_equal(got["labels"][b, :n], ev.labels[b, :n])


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
        nll = ctc.loss_logits(ctx, logits, 0, targets, tl, None)
        al = ctc.align_logits(ctx, logits, 0, targets, tl, None)
        rec = m_trained.recognize(imgs)
        return g, nll, al, rec

    g0, nll0, al0, rec0 = others()
    big = rng.randint(0, 3, 700)
    ctc.edit_distance_labels(ctx, *_batch([(big, big[::-1])]))            # another scratch layout
    ev = m_trained.evaluate(imgs, targets[:7], np.array([3, 0, 4], np.int32))
    assert len(ev) == 3
    g1, nll1, al1, rec1 = others()
    for x, y in zip(g0, g1):
        np.testing.assert_array_equal(x, y)
    assert nll0.tobytes() == nll1.tobytes()
    for k in ("paths", "scores", "starts", "ends", "logps"):
        assert getattr(al0, k).tobytes() == getattr(al1, k).tobytes(), k
    for k in ("labels", "lengths", "starts", "ends", "logps", "alt_labels", "alt_logps", "path_logp", "text_nll"):
        assert getattr(rec0, k).tobytes() == getattr(rec1, k).tobytes(), k


def _host_loop_cer(pairs):
    spec = importlib.util.spec_from_file_location("hctr_test_cli", os.path.join(ROOT, "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return sum(cli.edit_distance(p, t) for p, t in pairs) / sum(len(t) for _, t in pairs)


def test_python_surface(pkg, synth, ctc):
    import codec_cases
    name, seed, W, B, C, style = codec_cases.CODEC_CASES[3]
    logits = codec_cases.gen_logits(seed, W, B, C, style)
    vocab = codec_cases.vocab(C)
    cd = pkg.ctc_codec(vocab).cuda(0)
    decoded = cd.decode(logits)
    truths = [t[:2] + vocab[5] + t[3:] + vocab[1] if b % 2 else t[1:] for b, t in enumerate(decoded)]
    texts, ev = cd.evaluate(logits, truths)
    assert texts == decoded and isinstance(ev, pkg.Evaluation) and len(ev) == B
    want = [ctc_ref.edit_distance(p, t) for p, t in zip(decoded, truths)]
    assert ev.edits.tolist() == want and sum(want) > 0                      # no duplicate characters: label space == strings
    assert ev.cer == _host_loop_cer(list(zip(decoded, truths)))
    texts2, ev2 = cd.evaluate(torch.from_numpy(logits).cuda(0), truths)
    assert texts2 == texts and all(getattr(ev, k).tobytes() == getattr(ev2, k).tobytes() for k in OUTS)
    # strings from any decoder, with characters outside the vocabulary
    hyps = [t + "é\U0001f600" if b == 0 else t for b, t in enumerate(decoded)] + ["", "abc"]
    refs = ["è" + t for t in truths] + ["xyz", ""]
    texts3, ev3 = cd.evaluate(hyps, refs)
    want3 = [ctc_ref.edit_distance(p, t) for p, t in zip(hyps, refs)]
    assert texts3 == hyps and ev3.edits.tolist() == want3
    assert ev3.cer == _host_loop_cer(list(zip(hyps, refs)))
    assert ev3.totals[1] + ev3.totals[2] + ev3.totals[3] == sum(want3)
    d = pkg.edit_distance(hyps, refs)
    assert d.dtype == np.int32 and d.tolist() == want3
    assert pkg.edit_distance([[1, 2, 3], []], [[1, 3], [4]]).tolist() == [1, 1]
    assert pkg.edit_distance([], []).shape == (0,)
