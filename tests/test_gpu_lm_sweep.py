"""GPU tests (-m gpu) of the LM weight sweep (C ABI hctr_lm_sweep_topk / hctr_lm_sweep_logits / hctr_lm_sweep,
``hctr_model.lm_sweep``, ``ctc_codec.lm_sweep``, ``LMSweepTotals``).

The yardstick is tests/lm_sweep_ref.py: per pair tests/lm_beam_ref.py's search with nbest = 1 and tests/edit_ref.py's
distance (tests/test_lm_sweep_host.py checks that the fixture is not vacuous). What must hold:
  * on the fixture the integer outputs (edits, hyp_lengths, empty, labels) EXACTLY, logp / score / lm_score within
    1e-14 * T * max(1, |want|), the figure tests/test_gpu_nbest_lm.py uses for the device's log1p / exp;
  * for every pair, every output bit for bit what hctr_nbest_lm_topk(nbest = 1) + hctr_edit_distance return - on the
    fixture and on the (16, 16) instance of the search;
  * chunk 0, 1, 2 and G, and a repeated call, give the same bytes; G = 1 is the single-pair entry;
  * the line with an empty greedy text: empty = 1, edits = L_b under every pair, the other lines unaffected;
  * the three entry points agree byte for byte, the image entry in two internal passes in a fresh process;
  * every argument error, after each of which the context serves a correct call; no effect on hctr_last_guard;
  * the Python layer over two batches equals per-pair ``nbest(lm=, n=1)`` + ``codec.evaluate`` totals.
"""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import lm_beam_ref as lr
import lm_sweep_ref as sr
import nbest_ref as nr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
vp = ctypes.c_void_p
FIELDS = ("edits", "hyp_lengths", "empty", "labels", "logps", "scores", "lm_scores")


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
    return tmp_path_factory.mktemp("lm_sweep")


def chars_of(C):
    return ["<blank>"] + list(lr.chars_of(C)) + ["<unknown>"]


@pytest.fixture(scope="module")
def fix(codec_mod, work):
    """the fixture, its yardstick and its flat model (the ArpaLM is kept: it owns the flat handle)"""
    idx, lp, il, tg, tl, path, grid, want = sr.fixture(work)
    lm = codec_mod.ArpaLM(path)
    return dict(idx=idx, lp=lp, il=il, tg=tg, tl=tl, grid=grid, want=want, lm=lm, flat=lm.flat(chars_of(sr.C)), C=sr.C,
                beam=sr.BEAM)


@pytest.fixture(scope="module")
def wide(codec_mod, work):
    """the (16, 16) instance: beam 12 over k = 12 of C = 20 classes, W = 24, B = 2, four pairs"""
    C, k, W, B = 20, 12, 24, 2
    path = sr.write_arpa(work, "wide.arpa", order=3, n_chars=15, seed=12)
    idx, lp, il, tg, tl = sr.make_lists(5, W=W, B=B, C=C, k=k, input_lengths=(24, 19), empty_line=None)
    lm = codec_mod.ArpaLM(path)
    return dict(idx=idx, lp=lp, il=il, tg=tg, tl=tl, grid=[(0.0, 0.0), (2.0, 5.8), (0.8, -1.0), (4.0, 2.0)], lm=lm,
                flat=lm.flat(chars_of(C)), C=C, beam=12)


def sweep(ctc, ctx, f, grid=None, **kw):
    return ctc.lm_sweep_topk(ctx, f["idx"], f["lp"], f["C"], f["tg"], f["tl"], f["flat"], pairs=grid or f["grid"],
                             beam=f["beam"], input_lengths=f["il"], texts=True, **kw)


def same(a, b, what):
    for k in FIELDS:
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s: %s differs" % (what, k)


def single_pair(ctc, ctx, f, a, b):
    """the parent's way to one pair's figures: hctr_nbest_lm_topk(nbest = 1), then hctr_edit_distance on its labels"""
    nb = ctc.nbest_topk(ctx, f["idx"], f["lp"], f["C"], n=1, beam=f["beam"], len_bonus=b, input_lengths=f["il"], lm=f["flat"],
                        lm_panelty=a)
    ev = ctc.edit_distance_labels(ctx, nb.labels[:, 0], nb.lengths[:, 0], f["tg"], f["tl"], maps=False)
    return nb, ev


def test_fixture_against_yardstick(ctc, ctx, fix):
    want = fix["want"]
    assert all(sr.properties(want)) and sr.settled(want)
    got = sweep(ctc, ctx, fix)
    np.testing.assert_array_equal(got.empty, want["empty"])
    np.testing.assert_array_equal(got.hyp_lengths, want["hyp_lengths"])
    np.testing.assert_array_equal(got.labels, want["labels"])
    np.testing.assert_array_equal(got.edits, want["edits"])
    np.testing.assert_array_equal(got.ref_lengths, fix["tl"])
    assert got.total_edits.tolist() == want["edits"].sum(axis=1).tolist()
    live = want["empty"] == 0
    for g, w, what in ((got.logps, want["logp"], "logp"), (got.scores, want["score"], "score"),
                       (got.lm_scores, want["lm"], "lm_score")):
        assert (g[:, ~live] == -np.inf).all(), what
        err = np.abs(g[:, live] - w[:, live])
        print("%s: max |d| %.3e over %d figures" % (what, err.max(), err.size))
        assert (err <= sr.tol(sr.W, w[:, live])).all(), (what, g, w)


@pytest.mark.parametrize("which", ["fixture", "wide"])
def test_agrees_with_the_single_pair_entries(ctc, ctx, fix, wide, which):
    f = fix if which == "fixture" else wide
    got = sweep(ctc, ctx, f)
    texts = set()
    for g, (a, b) in enumerate(f["grid"]):
        nb, ev = single_pair(ctc, ctx, f, a, b)
        for mine, theirs, what in ((got.labels[g], nb.labels[:, 0], "labels"), (got.hyp_lengths[g], nb.lengths[:, 0], "lengths"),
                                   (got.logps[g], nb.logps[:, 0], "logp"), (got.scores[g], nb.scores[:, 0], "score"),
                                   (got.lm_scores[g], nb.lm_scores[:, 0], "lm_score"), (got.edits[g], ev.edits, "edits")):
            assert mine.dtype == theirs.dtype and mine.tobytes() == np.ascontiguousarray(theirs).tobytes(), (which, g, what)
        np.testing.assert_array_equal(got.empty, (nb.counts == 0).astype(np.uint8))
        texts.add(got.labels[g].tobytes())
    assert len(texts) > 1, "every pair read the same texts: the case compares nothing"


def test_chunking_and_repeats(ctc, ctx, fix):
    G = len(fix["grid"])
    first = sweep(ctc, ctx, fix)
    for chunk in (0, 1, 2, G):
        same(first, sweep(ctc, ctx, fix, chunk=chunk), "chunk %d" % chunk)
    same(first, sweep(ctc, ctx, fix), "a second call")
    assert ctc.lm_sweep_chunk(sr.B, sr.W, sr.BEAM, G) == G               # this fixture: one launch when left to the engine
    assert ctc.lm_sweep_chunk(64, 2000, 10, 250) == 128                  # the workload: 8192 / 64 lines


def test_one_pair_is_the_single_pair_entry(ctc, ctx, fix):
    a, b = fix["grid"][3]
    got = sweep(ctc, ctx, fix, grid=[(a, b)])
    nb, ev = single_pair(ctc, ctx, fix, a, b)
    assert got.edits.shape == (1, sr.B)
    assert got.labels[0].tobytes() == np.ascontiguousarray(nb.labels[:, 0]).tobytes()
    assert got.scores[0].tobytes() == np.ascontiguousarray(nb.scores[:, 0]).tobytes()
    assert got.logps[0].tobytes() == np.ascontiguousarray(nb.logps[:, 0]).tobytes()
    assert got.lm_scores[0].tobytes() == np.ascontiguousarray(nb.lm_scores[:, 0]).tobytes()
    assert got.edits[0].tobytes() == ev.edits.tobytes()
    same(got, sweep(ctc, ctx, fix, grid=[(a, b)], chunk=1), "chunk 1 of 1")


def test_empty_greedy_line(ctc, ctx, fix):
    """line 2's top-1 class is the blank in every column: empty = 1 and edits = L_b under every pair; the other lines
    are what they are without it"""
    e = sr.EMPTY_LINE
    got = sweep(ctc, ctx, fix)
    assert got.empty.tolist() == [int(b == e) for b in range(sr.B)]
    assert (got.edits[:, e] == fix["tl"][e]).all() and (got.hyp_lengths[:, e] == 0).all() and (got.labels[:, e] == 0).all()
    keep = [b for b in range(sr.B) if b != e]
    off = np.concatenate([[0], np.cumsum(fix["tl"])])
    rest = dict(fix, idx=np.ascontiguousarray(fix["idx"][:, keep]), lp=np.ascontiguousarray(fix["lp"][:, keep]),
                il=fix["il"][keep], tl=fix["tl"][keep],
                tg=np.concatenate([fix["tg"][off[b]:off[b + 1]] for b in keep]))
    alone = sweep(ctc, ctx, rest)
    assert not alone.empty.any()
    for k in FIELDS:
        if k != "empty":
            assert np.ascontiguousarray(getattr(got, k)[:, keep]).tobytes() == getattr(alone, k).tobytes(), k


def test_logits_entry(pkg, ctc, ctx, fix):
    """hctr_lm_sweep_logits on random logits == hctr_lm_sweep_topk on hctr_log_softmax + top-k lists of them"""
    import torch
    W, B, C, k = 40, 3, sr.C, sr.K
    rng = np.random.RandomState(21)
    logits = nr.planted_lines(rng, W, B, C, density=0.4, boost=2.5)
    il = np.array([40, 31, 22], np.int32)
    tl = np.array([6, 4, 5], np.int32)
    tg = rng.randint(1, C - 1, size=int(tl.sum())).astype(np.int32)
    full = np.zeros((W, B, C), np.float32)
    assert pkg.load_library().hctr_log_softmax(ctx, logits.ctypes.data_as(vp), 0, W, B, C, full.ctypes.data_as(vp)) == 0
    order = np.lexsort((np.broadcast_to(np.arange(C), full.shape), -full), axis=2)[:, :, :k]      # log-prob descending, index ascending
    idx, lp = order.astype(np.int32), np.take_along_axis(full, order, axis=2)
    kw = dict(pairs=fix["grid"], beam=sr.BEAM, input_lengths=il, texts=True)
    lists = ctc.lm_sweep_topk(ctx, idx, lp, C, tg, tl, fix["flat"], **kw)
    host = ctc.lm_sweep_logits(ctx, logits, 0, tg, tl, fix["flat"], depth=k, **kw)
    same(lists, host, "logits entry")
    assert host.hyp_lengths.max() > 0 and len(set(host.labels[g].tobytes() for g in range(len(host)))) > 1
    dev = torch.from_numpy(logits).cuda(0)
    torch.cuda.synchronize()
    same(host, ctc.lm_sweep_logits(ctx, dev, 1, tg, tl, fix["flat"], depth=k, **kw), "device pointer")
    same(host, ctc.lm_sweep_logits(ctx, logits, 0, tg, tl, fix["flat"], depth=k, chunk=1, **kw), "chunk 1")


def test_image_entry_in_two_passes(work):
    env = dict(os.environ, HCTR_MAX_COLS="600")             # f16x3 passes of 200 columns: two lines of width 96, then one
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lm_sweep_child.py"), str(work)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_argument_errors(pkg, ctc, codec_mod, ctx, fix, wide):
    lib = pkg.load_library()
    idx, lp, il, tg, tl = fix["idx"], fix["lp"], fix["il"], fix["tg"], fix["tl"]
    G = len(fix["grid"])
    al = np.array([a for a, _ in fix["grid"]])
    be = np.array([b for _, b in fix["grid"]])
    edits = np.zeros((G, sr.B), np.int32)
    P = lambda a: None if a is None else a.ctypes.data_as(vp)
    good = dict(lm=fix["flat"], idx=idx, k=sr.K, beam=sr.BEAM, al=al, be=be, G=G, chunk=0, il=il, tg=tg, tl=tl)

    def call(**over):
        a = dict(good, **over)
        edits[:] = -1
        return lib.hctr_lm_sweep_topk(ctx, a["lm"], P(a["idx"]), P(lp), sr.W, sr.B, sr.C, a["k"], a["beam"], P(a["al"]),
                                      P(a["be"]), a["G"], a["chunk"], P(a["il"]), P(a["tg"]), P(a["tl"]), P(edits), None, None,
                                      None, None, None, None)

    def nan_at(arr, g):
        out = arr.copy()
        out[g] = np.nan
        return out

    long_tl = tl.copy()
    long_tl[1] = 2048
    long_tg = np.ones((int(long_tl.sum()),), np.int32)
    bad_idx = idx.copy()
    bad_idx[3, 1, 2] = bad_idx[3, 1, 0]                                  # a class twice in a row
    assert call() == 0
    np.testing.assert_array_equal(edits, fix["want"]["edits"])
    cases = [
        (dict(lm=None), b"lm"), (dict(lm=wide["flat"]), b"20"),          # everything hctr_nbest_lm_topk rejects ...
        (dict(beam=33), b"beam"), (dict(beam=0), b"beam"), (dict(k=sr.C + 1), b"k="), (dict(k=0), b"k="),
        (dict(idx=None), b"NULL"), (dict(idx=bad_idx), b"repeated"),
        (dict(il=np.array([40, 41, 17, 40], np.int32)), b"input_lengths[1]"),
        (dict(tl=None), b"ref_lengths"), (dict(tg=None), b"ref is NULL"),          # ... and hctr_evaluate_logits
        (dict(tg=np.zeros_like(tg)), b"target id 0"),
        (dict(tg=np.where(np.arange(tg.size) == 4, sr.C, tg).astype(np.int32)), b"target id 12"),
        (dict(tl=np.array([18, -1, 3, 25], np.int32)), b"ref_lengths[1]"),
        (dict(tl=long_tl, tg=long_tg), b"2047"),                         # a transcription longer than 2047
        (dict(G=0), b"G"), (dict(G=-3), b"G"), (dict(al=None), b"NULL"), (dict(be=None), b"NULL"),
        (dict(al=nan_at(al, 4)), b"pair 4"), (dict(be=nan_at(be, 2)), b"pair 2"),
        (dict(chunk=-1), b"chunk"), (dict(chunk=G + 1), b"chunk"),
    ]
    for over, word in cases:
        assert call(**over) == ERR_ARG, over
        msg = lib.hctr_last_error(ctx)
        assert msg and word in msg, (over, msg)
        assert call() == 0, over                                         # the context still serves a correct call
        np.testing.assert_array_equal(edits, fix["want"]["edits"])
    z = np.zeros((sr.W, sr.B, sr.C), np.float32)
    assert lib.hctr_lm_sweep_logits(ctx, fix["flat"], P(z), 0, sr.W, sr.B, sr.C, sr.K, sr.BEAM, P(al), P(be), G, G + 1, None,
                                    P(tg), P(tl), None, None, None, None, None, None, None) == ERR_ARG
    assert b"chunk" in lib.hctr_last_error(ctx)
    assert lib.hctr_lm_sweep_logits(ctx, None, P(z), 0, sr.W, sr.B, sr.C, sr.K, sr.BEAM, P(al), P(be), G, 0, None, P(tg), P(tl),
                                    None, None, None, None, None, None, None) == ERR_ARG
    # B == 0 is a no-op
    assert lib.hctr_lm_sweep_topk(ctx, fix["flat"], None, None, sr.W, 0, sr.C, sr.K, sr.BEAM, P(al), P(be), G, 0, None, None,
                                  None, None, None, None, None, None, None, None) == 0
    # every output may be NULL
    assert lib.hctr_lm_sweep_topk(ctx, fix["flat"], P(idx), P(lp), sr.W, sr.B, sr.C, sr.K, sr.BEAM, P(al), P(be), G, 0, P(il),
                                  P(tg), P(tl), None, None, None, None, None, None, None) == 0


def test_python_layer_over_two_batches(pkg, synth, ctc, codec_mod, work):
    """model.lm_sweep and codec.lm_sweep through LMSweepTotals == per-pair nbest(lm=, n=1) + codec.evaluate totals, the
    answer == a plain loop; the sweep leaves the guard figures of "auto" precision alone"""
    C = synth.DEFAULT_VOCAB + 2
    m = pkg.hctr_model(C, precision="auto").cuda(0)
    m.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    cd = pkg.ctc_codec(synth.characters()).attach(m)
    W = 128
    batches = []
    for seed in (51, 52):
        imgs, boxes = synth.make_font_lines(2, W, seed, with_truth=True)
        batches.append((imgs, [synth.font_truth_text(bx, W) for bx in boxes]))
    seen = sorted(set("".join(t for _, ts in batches for t in ts)))
    path = os.path.join(str(work), "python_layer.arpa")
    lr.write_arpa(path, 3, seen[:max(4, len(seen) - 2)], seed=10)
    lm = codec_mod.ArpaLM(path)
    alphas, betas = (0.0, 2.0), (-2.0, 1.0, 5.8)
    grid = sr.pairs(alphas, betas)
    m.greedy(batches[0][0])
    guard0, guard1 = m.last_guard(), None
    totals, totals_logits = ctc.LMSweepTotals(), ctc.LMSweepTotals()
    want_edits, want_logits, nchars = np.zeros((len(grid),), np.int64), np.zeros((len(grid),), np.int64), 0
    for imgs, truths in batches:
        s = m.lm_sweep(imgs, truths, lm=lm, codec=cd, alphas=alphas, betas=betas, texts=True)
        assert s.pairs == grid
        totals.update(s)
        if guard1 is None:
            guard1 = m.last_guard()                                      # right after the sweep: the forward below sets its own
        m.set_precision("f16x3")                                         # what "auto" runs every line of the sweep in
        try:
            logits = m(imgs)
            for g, (a, b) in enumerate(grid):
                nb = m.nbest(imgs, n=1, lm=lm, lm_panelty=a, len_bonus=b, codec=cd)
                one = [t[0] if t else "" for t in nb.texts]
                assert s.texts[g] == one, (g, s.texts[g], one)
                want_edits[g] += cd.evaluate(one, truths, maps=False)[1].total_edits
        finally:
            m.set_precision("auto")
        nchars += sum(len(t) for t in truths)
        totals_logits.update(cd.lm_sweep(logits, truths, lm, alphas, betas))
        for g, (a, b) in enumerate(grid):                                # the stored-logits front end, against itself
            one = [t[0] if t else "" for t in cd.nbest(logits, n=1, lm=lm, lm_panelty=a, len_bonus=b).texts]
            want_logits[g] += cd.evaluate(one, truths, maps=False)[1].total_edits
    assert guard0["lines"] == guard1["lines"] and guard0["flagged"] == guard1["flagged"]
    for f in ("flags", "min_margin", "scale"):
        np.testing.assert_array_equal(guard0[f], guard1[f])
    assert totals.nchars == nchars and totals.total_edits.tolist() == want_edits.tolist()
    assert totals_logits.nchars == nchars and totals_logits.total_edits.tolist() == want_logits.tolist()
    best, best_cer = (0, 0), 1.0
    for pair, e in zip(grid, want_edits.tolist()):
        if e / nchars < best_cer:
            best, best_cer = pair, e / nchars
    assert totals.best() == (best, best_cer)
    assert totals.report()[-1] == "min params:{}, min cer: {}".format(best, best_cer)
