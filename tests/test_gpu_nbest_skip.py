"""GPU tests (-m gpu) of the device skip search (C ABI hctr_nbest_skip_lists / hctr_nbest_skip_logits / hctr_nbest_skip,
``hctr_model.nbest(skip_search=True)``, ``ctc_codec.nbest(skip_search=True)``).

The yardstick is tests/skip_beam_ref.py, which goes the reference's own way (tests/test_skip_beam_host.py checks it against
the real reference's strings, the oracle and the host search). Through hctr_nbest_skip_lists on identical float32 lists:
  * count, status, ranked, lengths and labels EXACTLY; lm_score exactly on lines where no fold occurred;
  * lm_score, logp and score within 1e-14 * T * max(1, |want|), the figure of tests/test_gpu_nbest.py; each case first
    asserts, on the yardstick alone, that its smallest nonzero gap between adjacent totals is at least 100x that.
"""
import ctypes
import importlib
import json
import os

import numpy as np
import pytest

import codec_cases
import lm_beam_ref as lr
import skip_beam_ref as sr
import skip_cases as sc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERR_ARG = -1
vp = ctypes.c_void_p
FIELDS = ("labels", "lengths", "logps", "scores", "counts", "lm_scores", "status", "ranked")


@pytest.fixture(scope="module")
def ctc(pkg):
    return importlib.import_module(pkg.__name__ + ".ctc")


@pytest.fixture(scope="module")
def codec_mod(pkg):
    return importlib.import_module(pkg.__name__ + ".codec")


@pytest.fixture(scope="module")
def ctx(pkg):
    al = pkg.CTCAligner().cuda(0)
    yield al._context()                       # a weightless context: the list and logits entries need no weights
    del al


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("nbest_skip")


def _tol(T, want):
    return 1e-14 * T * np.maximum(1.0, np.abs(want))


def same(a, b, what):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s: %s differs" % (what, f)


def compare(name, T, got, want):
    """the contract's comparison of a device result with the yardstick's"""
    fin = np.isfinite(want["score"])
    both = np.concatenate([want["logp"][fin], want["score"][fin]])
    worst = float(_tol(T, both).max()) if both.size else 1e-14 * T
    print("%s: smallest nonzero gap %.3e, tolerance at most %.3e, ends %s, ranked %s, status %s, duplicate steps %s"
          % (name, want["gap"], worst, want["ends"].tolist(), want["ranked"].tolist(), want["status"].tolist(),
             want["dup_steps"].tolist()))
    assert want["gap"] >= 100 * worst, "the yardstick's own ranking is not settled at this seed"
    np.testing.assert_array_equal(got.counts, want["count"])
    np.testing.assert_array_equal(got.status, want["status"])
    np.testing.assert_array_equal(got.ranked, want["ranked"])
    np.testing.assert_array_equal(got.lengths, want["lengths"])
    np.testing.assert_array_equal(got.labels, want["labels"])
    for b in np.flatnonzero(want["dup_steps"] == 0):
        assert got.lm_scores[b].tobytes() == want["lm"][b].tobytes(), (name, b, got.lm_scores[b], want["lm"][b])
    for g, w, what in ((got.lm_scores, want["lm"], "lm_score"), (got.logps, want["logp"], "logp"),
                       (got.scores, want["score"], "score")):
        np.testing.assert_array_equal(g[~fin], w[~fin], err_msg=what)
        err = np.abs(g[fin] - w[fin])
        print("%s %s: max |d| %.3e over %d figures" % (name, what, err.max() if err.size else 0.0, err.size))
        assert (err <= _tol(T, w[fin])).all(), (name, what, g, w)


# ---- 1. the goldens of the real reference at its skip_zero setting -------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in codec_cases.CODEC_CASES])
def test_goldens(ctc, ctx, name):
    with open(os.path.join(GOLDEN, "codec_cases.json"), encoding="utf-8") as f:
        gold = json.load(f)[name]["skip_zero"]
    _, seed, W, B, C, style = next(c for c in codec_cases.CODEC_CASES if c[0] == name)
    _, _, _, pen, bonus, beam, _ = next(s for s in codec_cases.BEAM_SETTINGS if s[0] == "skip_zero")
    lists = sr.lists_of_logp(sc.logp_of(codec_cases.gen_logits(seed, W, B, C, style)))
    want = sr.search(sr.make_codec(C, None, pen, bonus), *lists, beam, beam)
    got = ctc.nbest_skip_lists(ctx, *lists, C, n=beam, beam=beam, len_bonus=bonus, lm=None, lm_panelty=pen)
    compare(name, W, got, want)
    rows = np.diff(lists[2])
    if name in ("peaky_small", "peaky_wide", "single_col"):
        assert (got.ranked == 0).all() and (got.status == 0).all()
    elif name == "flat_small":
        assert (got.ranked == want["ends"]).all() and rows.max() == 12 and want["gap"] >= 1.5e-4
    elif name == "mixed_small":
        assert (got.ranked > 0).all() and (got.ranked < want["ends"]).all() and rows.max() == 16 and want["gap"] >= 2.2e-4
    elif name == "flat_c7358":
        assert gold == "IndexError" and got.status.tolist() == [2] and got.counts.tolist() == [0]
    elif name == "mixed_wide":
        assert rows.max() == 300 and got.status.tolist() == [3, 3] and (got.counts == 0).all()
    if isinstance(gold, list) and (got.status == 0).all():
        chars = codec_cases.vocab(C)
        assert ["".join(chars[c - 1] for c in got.labels[b, 0, :got.lengths[b, 0]]) for b in range(B)] == gold
        assert (got.lm_scores[got.lengths > 0] == 0).all() and (got.lm_scores[:, 0] == 0).all()


# ---- 2. duplicates --------------------------------------------------------------------------------------------------
def _arpa(work, order, n_chars, seed, unk=True):
    path = os.path.join(str(work), "o%d_n%d_s%d_%d.arpa" % (order, n_chars, seed, unk))
    if not os.path.exists(path):
        lr.write_arpa(path, order, n_chars, seed=seed, unk=unk)
    return path


def _flat(codec_mod, path, C, keep={}):
    if (path, C) not in keep:
        lm = codec_mod.ArpaLM(path)
        keep[(path, C)] = (lm, lm.flat(["<blank>"] + list(lr.chars_of(C)) + ["<unknown>"]))
    return keep[(path, C)][1]


@pytest.mark.parametrize("with_lm", [False, True])
def test_duplicates_are_folded(ctc, codec_mod, ctx, work, with_lm):
    T, C, beam = 24, 6, 4
    path = _arpa(work, 3, 4, 8) if with_lm else None
    flat = _flat(codec_mod, path, C) if with_lm else None
    twice = []
    for seed in range(6):
        lists = sr.lists_of_logp(sc.logp_of(sc.duplicate_line(seed, T, C)))
        want = sr.search(sr.make_codec(C, path, 2.0, 5.8), *lists, beam, beam)
        assert want["dup_steps"][0] >= 1 and want["status"][0] == 0
        got = ctc.nbest_skip_lists(ctx, *lists, C, n=beam, beam=beam, len_bonus=5.8, lm=flat, lm_panelty=2.0)
        compare("duplicates, seed %d%s" % (seed, ", 3-gram" if with_lm else ""), T, got, want)
        texts = [tuple(x) for x in got.label_lists()[0]]
        twice.append(len(set(texts)) < len(texts))
    assert any(twice), "no line returned a text twice in its N-best"


# ---- 3. the in-place branches ---------------------------------------------------------------------------------------
def test_inplace_branches(ctc, ctx):
    T, C, beam = 12, 6, 8
    lists = sr.lists_of_logp(sc.logp_of(sc.branch_line(T, C)))
    want = sr.search(sr.make_codec(C, None, 2.0, 5.8), *lists, beam, beam)
    assert {(br, True) for br in (1, 2, 3, 4)} <= want["branches"]
    assert float(lists[1][3, 0]) < sr.THRESH                  # branch 4 read a blank that is no candidate
    compare("branches", T, ctc.nbest_skip_lists(ctx, *lists, C, n=beam, beam=beam, len_bonus=5.8), want)


# ---- 4. n-gram models -----------------------------------------------------------------------------------------------
# (name, T, B, C, beam, LM order, characters in the model, <unk>, lm_panelty, len_bonus, seed)
LM_CASES = [
    ("defaults, ragged, OOV", 63, 3, 18, 10, 3, 14, True, 2.0, 5.8, 1),
    ("middle instance, 5-gram", 65, 3, 40, 16, 5, 30, True, 2.0, 5.8, 2),
    ("widest instance, longest context", 40, 2, 40, 32, 6, 30, True, 0.8, 4.8, 3),
    ("model without <unk>", 33, 2, 18, 10, 3, 14, False, 2.0, 5.8, 4),
    ("workload classes", 130, 2, 7375, 10, 3, 14, True, 2.0, 5.8, 5),
]
_DONE = {}


def lm_case(work, name):
    if name not in _DONE:
        _, T, B, C, beam, order, n_chars, unk, pen, bonus, seed = next(c for c in LM_CASES if c[0] == name)
        z = sc.mixed_lines(300 + seed, T, B, C)
        if C > 1000:                              # keep the lines inside the model's few characters now and then
            for b in range(B):
                for t in range(0, T, 3):
                    sc.certain(z, t, b, 1 + (t * 7 + b) % n_chars)
        il = np.maximum(1, T - np.arange(B) * max(1, T // 7)).astype(np.int32)
        if name == "defaults, ragged, OOV":
            sc.quiet_tail(z, 0, 41)               # line 0: nothing but blanks after column 40, so end_0 < L_0 - 4
        lists = sr.lists_of_logp(sc.logp_of(z))
        path = _arpa(work, order, n_chars, seed, unk)
        want = sr.search(sr.make_codec(C, path, pen, bonus), *lists, beam, beam, il)
        _DONE[name] = (z, lists, il, path, want)
    return _DONE[name]


@pytest.mark.parametrize("name", [c[0] for c in LM_CASES])
def test_ngram_models(ctc, codec_mod, ctx, work, name):
    _, T, B, C, beam, order, n_chars, unk, pen, bonus, seed = next(c for c in LM_CASES if c[0] == name)
    z, lists, il, path, want = lm_case(work, name)
    assert (want["status"] == 0).all() and (want["ranked"] > 0).all() and (want["ranked"] < want["ends"]).all()
    if name == "defaults, ragged, OOV":
        assert want["ends"][0] < il[0] - 4
    got = ctc.nbest_skip_lists(ctx, *lists, C, n=beam, beam=beam, len_bonus=bonus, input_lengths=il,
                               lm=_flat(codec_mod, path, C), lm_panelty=pen)
    compare(name, T, got, want)


# ---- 5. the cap -----------------------------------------------------------------------------------------------------
def test_cap(ctc, codec_mod, ctx, work):
    T, B, C, beam = 20, 3, 40, 10
    rng = np.random.RandomState(9)
    z = sc.mixed_lines(77, T, B, C)
    z[6, 1, :] = sc.FLOOR
    sc.offer(z, 6, 1, list(range(2, 34)), rng)                # 32 candidates: searched
    path = _arpa(work, 3, 30, 11)
    flat = _flat(codec_mod, path, C)
    kw = dict(n=beam, beam=beam, len_bonus=5.8, lm=flat, lm_panelty=2.0)
    lists = sr.lists_of_logp(sc.logp_of(z))
    assert np.diff(lists[2]).max() == 32
    want = sr.search(sr.make_codec(C, path, 2.0, 5.8), *lists, beam, beam)
    assert (want["status"] == 0).all() and want["ends"][1] > 6
    ok = ctc.nbest_skip_lists(ctx, *lists, C, **kw)
    compare("32 candidates", T, ok, want)
    z[6, 1, 34] = z[6, 1, 33]                                 # 33 in line 1's row
    lists = sr.lists_of_logp(sc.logp_of(z))
    assert np.diff(lists[2]).max() == 33
    over = ctc.nbest_skip_lists(ctx, *lists, C, **kw)
    assert over.status.tolist() == [0, 3, 0] and over.counts[1] == 0 and over.ranked[1] == ok.ranked[1]
    assert (over.lengths[1] == 0).all() and (over.labels[1] == 0).all() and (over.logps[1] == -np.inf).all()
    for b in (0, 2):
        for f in FIELDS:
            assert getattr(over, f)[b].tobytes() == getattr(ok, f)[b].tobytes(), (b, f)


# ---- 6. plumbing ----------------------------------------------------------------------------------------------------
def test_entries_agree_on_logits(pkg, ctc, codec_mod, work):
    import torch
    model_mod = importlib.import_module(pkg.__name__ + ".model")
    name = "defaults, ragged, OOV"
    _, T, B, C, beam, order, n_chars, unk, pen, bonus, seed = next(c for c in LM_CASES if c[0] == name)
    z, _, il, path, _ = lm_case(work, name)
    cd = pkg.ctc_codec(lr.chars_of(C)).cuda(0)
    lm = codec_mod.ArpaLM(path)
    flat = lm.flat(cd.characters)
    ctx = cd._context()
    fe = model_mod.beam_frontend_call(ctx, None, 1, 0, None, z, 0, B, T, C, 1, True)
    for use in (flat, None):
        kw = dict(n=beam, beam=beam, len_bonus=bonus, input_lengths=il, lm=use, lm_panelty=pen)
        lists = ctc.nbest_skip_lists(ctx, fe["topk_idx"][:, :, 0], fe["blank_logp"], fe["cand_off"], fe["cand_idx"],
                                     fe["cand_logp"], C, **kw)
        host = ctc.nbest_skip_logits(ctx, z, 0, **kw)
        same(lists, host, "logits entry")
        assert (host.status == 0).all() and (host.counts > 0).all() and (host.ranked > 0).all()
        dev_t = torch.from_numpy(z).cuda(0)
        torch.cuda.synchronize()
        same(host, ctc.nbest_skip_logits(ctx, dev_t, 1, **kw), "device pointer")
        same(host, ctc.nbest_skip_logits(ctx, z, 0, **kw), "repeated call")
        same(lists, ctc.nbest_skip_lists(ctx, fe["topk_idx"][:, :, 0], fe["blank_logp"], fe["cand_off"], fe["cand_idx"],
                                         fe["cand_logp"], C, **kw), "repeated lists call")
        res = cd.nbest(z, n=beam, beam=beam, len_bonus=bonus, input_lengths=il, lm=lm if use else None, lm_panelty=pen,
                       skip_search=True)
        same(host, res, "ctc_codec.nbest")
        assert [len(t) for t in res.texts] == res.counts.tolist()
    plain = cd.nbest(z, n=4, beam=beam)
    assert plain.status is None and plain.ranked is None


def test_image_entry_agrees(pkg, synth, ctc, codec_mod, work):
    C = synth.DEFAULT_VOCAB + 2
    m = pkg.hctr_model(C, precision="f16").cuda(0)
    m.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    cd = pkg.ctc_codec(synth.characters())
    W = 160
    imgs, boxes = synth.make_font_lines(3, W, 40 + W, with_truth=True)
    truths = [synth.font_truth_text(bx, W) for bx in boxes]
    widths = np.array([W, W - 29, W - 50], np.int32)
    il = np.array([W, W - 20, W - 45], np.int32)
    seen = sorted(set("".join(truths)))
    path = os.path.join(str(work), "images.arpa")
    lr.write_arpa(path, 3, seen[:max(4, len(seen) - 3)], seed=6)
    lm = codec_mod.ArpaLM(path)
    flat = lm.flat(cd.characters)
    fe = m.beam_frontend(imgs, 1, widths=widths, want_candidates=True)
    before = ctc.nbest_topk(m._ctx, fe["topk_idx"], fe["topk_logp"], C, n=1, beam=10, len_bonus=5.8, input_lengths=il,
                            lm=flat, lm_panelty=2.0)
    for use in (lm, None):
        kw = dict(n=5, beam=10, len_bonus=5.8, input_lengths=il, lm_panelty=2.0)
        res = m.nbest(imgs, widths=widths, lm=use, codec=cd, skip_search=True, **kw)
        lists = ctc.nbest_skip_lists(m._ctx, fe["topk_idx"][:, :, 0], fe["blank_logp"], fe["cand_off"], fe["cand_idx"],
                                     fe["cand_logp"], C, lm=flat if use else None, **kw)
        same(res, lists, "lists of the front end")
        print("image entry: status %s ranked %s counts %s" % (res.status.tolist(), res.ranked.tolist(), res.counts.tolist()))
        assert (res.status == 0).all() and (res.counts > 0).all() and res.lengths[:, 0].min() > 0
        assert len(res.texts) == 3 and all(isinstance(t, str) for line in res.texts for t in line)
    # the LM upload is shared: the full search returns what it returned before the skip calls
    after = ctc.nbest_topk(m._ctx, fe["topk_idx"], fe["topk_logp"], C, n=1, beam=10, len_bonus=5.8, input_lengths=il,
                           lm=flat, lm_panelty=2.0)
    for f in ("labels", "lengths", "logps", "scores", "counts", "lm_scores"):
        assert getattr(before, f).tobytes() == getattr(after, f).tobytes(), f
    m.set_profiling(True)
    m.nbest(imgs, widths=widths, lm=lm, codec=cd, skip_search=True, n=5, beam=10, len_bonus=5.8, input_lengths=il)
    names = [nm for nm, _ in m.last_profile()]
    m.set_profiling(False)
    assert names[-4:] == ["skip_candidates", "beam_lm_prepass", "prefix_beam_skip", "prefix_backtrace"], names
    with pytest.raises(ValueError):
        m.nbest(imgs, lm=lm, skip_search=True)                # a language model needs the codec


def test_auto_precision_runs_f16x3_and_leaves_the_guard_alone(pkg, synth):
    """mode 2: every line of the image entry runs in f16x3, and the guard figures of the last guarded call stay"""
    C = synth.DEFAULT_VOCAB + 2
    sd = synth.make_state_dict(C, seed=0, head="trained")
    imgs = synth.make_font_lines(3, 96, 31)
    m = pkg.hctr_model(C, precision="auto").cuda(0)
    m.load_state_dict(sd)
    g0 = m.greedy(imgs)
    guard0 = m.last_guard()
    res = m.nbest(imgs, n=3, beam=10, len_bonus=5.8, skip_search=True)
    guard1 = m.last_guard()
    assert guard0["lines"] == guard1["lines"] and guard0["flagged"] == guard1["flagged"]
    for f in ("flags", "min_margin", "scale"):
        np.testing.assert_array_equal(guard0[f], guard1[f])
    for x, y in zip(g0, m.greedy(imgs)):
        np.testing.assert_array_equal(x, y)
    m.set_precision("f16x3")
    same(res, m.nbest(imgs, n=3, beam=10, len_bonus=5.8, skip_search=True), "f16x3")
    assert (res.status == 0).all() and (res.counts > 0).all() and (res.lm_scores[:, 0] == 0).all()


def test_argument_errors(pkg, codec_mod, ctx, work):
    lib = pkg.load_library()
    T, B, C, beam = 12, 1, 6, 4
    top1, blank, off, ci, cl = sr.lists_of_logp(sc.logp_of(sc.branch_line(T, C)))
    flat6 = _flat(codec_mod, _arpa(work, 3, 4, 8), C)
    other = _flat(codec_mod, _arpa(work, 3, 14, 1), 18)
    outs = [np.zeros((B, beam, T), np.int32), np.zeros((B, beam), np.int32)]
    st, rk = np.zeros(B, np.int32), np.zeros(B, np.int32)

    def call(lm=None, pen=2.0, bonus=5.8, beam=beam, nbest=beam, top1=top1, off=off, ci=ci, il=None, B=B):
        return lib.hctr_nbest_skip_lists(ctx, lm, None if top1 is None else top1.ctypes.data_as(vp), blank.ctypes.data_as(vp),
                                         off.ctypes.data_as(vp), ci.ctypes.data_as(vp), cl.ctypes.data_as(vp), T, B, C, beam,
                                         nbest, ctypes.c_double(pen), ctypes.c_double(bonus),
                                         None if il is None else il.ctypes.data_as(vp), outs[0].ctypes.data_as(vp),
                                         outs[1].ctypes.data_as(vp), None, None, None, None, st.ctypes.data_as(vp),
                                         rk.ctypes.data_as(vp))

    assert call() == 0 and st[0] == 0
    assert call(lm=flat6) == 0
    assert call(pen=float("nan")) == 0                        # lm == NULL: lm_panelty is unused
    down = off.copy()
    down[3] = down[2] - 1
    wide, swapped, bad1 = ci.copy(), ci.copy(), top1.copy()
    wide[0] = C
    swapped[0], swapped[1] = ci[1], ci[0]                     # row 0 offers {0, 1, 2}: no longer ascending
    bad1[2, 0] = -1
    for kw in (dict(lm=flat6, pen=float("nan")), dict(lm=other), dict(bonus=float("nan")), dict(beam=33), dict(nbest=0),
               dict(nbest=beam + 1), dict(top1=None), dict(off=down), dict(ci=wide), dict(ci=swapped), dict(top1=bad1),
               dict(il=np.array([T + 1], np.int32))):
        assert call(**kw) == ERR_ARG, kw
        assert lib.hctr_last_error(ctx), kw
    z = np.zeros((T, B, C), np.float32)
    assert lib.hctr_nbest_skip_logits(ctx, other, z.ctypes.data_as(vp), 0, T, B, C, beam, beam, ctypes.c_double(2.0),
                                      ctypes.c_double(5.8), None, None, None, None, None, None, None, None, None) == ERR_ARG
    assert b"18" in lib.hctr_last_error(ctx)
    assert lib.hctr_nbest_skip_logits(ctx, None, None, 0, T, B, C, beam, beam, ctypes.c_double(2.0), ctypes.c_double(5.8),
                                      None, None, None, None, None, None, None, None, None) == ERR_ARG
    assert call() == 0                                        # the context is still usable
    assert call(B=0) == 0                                     # a no-op
    # all-zero logits: every class is a candidate of every row and the greedy text is empty
    assert lib.hctr_nbest_skip_logits(ctx, None, z.ctypes.data_as(vp), 0, T, B, C, beam, beam, ctypes.c_double(2.0),
                                      ctypes.c_double(5.8), None, None, None, None, None, None, None, st.ctypes.data_as(vp),
                                      rk.ctypes.data_as(vp)) == 0
    assert st[0] == 1 and rk[0] == 0
