"""GPU tests (-m gpu): a call on an engine context does not depend on the calls that ran on the context before it.

The context keeps device state between calls - the grow-only CTC scratch that every scoring family re-carves with its own
layout, the trunk arena's sticky parts, the pinned staging buffer, the last front end's candidate lists, the last guard
figures, and one cached device copy each of the last LM, lexicon and pattern ("A call does not depend
on the calls before it"). Every family's own module tests it on a context of its own, where a freshly allocated block is
typically zero; here the probes of tests/history_cases.py run after other calls. Every comparison is byte equality of
every returned array in full, the entries beyond lengths, counts and T included; the only tolerances are the families'
existing rules in the check of the first-call results against the existing oracles.

  * base: each probe as the first call on a new context, checked against its oracle (a result that is history-independent
    but wrong must not pass);
  * dirty: on one context the big dirtier (larger than every probe in every carved dimension, three non-finite lines, so
    that emissions, alpha / beta rows, log-sum-exps, gradient scratch, the words call's step buffers and exit records
    hold NaN and inf; int32 extremes in the edit tables; the widest search), then the probe - for every probe, host and
    device pointers, and under the layout switches HCTR_SPOT_CLASSES=4, HCTR_LEX_CLASSES=4, HCTR_PAT_LINES=1,
    HCTR_PATSET_LDS=0, HCTR_WORDS_LDS=0 and HCTR_WORDS_LINES=1; the words probe also right after each of the big
    dirtier's two words calls, whose records and step buffers then lie where it carves its own;
  * grow: on one context the small dirtier (B = 1, W = 2, C = 3), then the probes in ascending order of (estimated)
    scratch need, so that the block grows under them; each probe also right after the small dirtier on a context of its
    own; and the wide recognition probe from blocks of known size, where the call grows the block between its two
    layouts and ``ctc_reserve(keep)`` moves the kept log-sum-exps;
  * mixed: on one context all probes in order, in reverse order, and each twice in a row;
  * the fills include/hctr_hip.h documents beyond the valid part of an output, asserted on the dirty results;
  * the cached tables: two lexicons and two patterns alternating, a pattern freed and another built, one object on two
    contexts; one lexicon through the exact-lexicon and the words call in turn (three device copies under one serial),
    under two bonuses, two lexicons through the words call, a lexicon freed and another built, and patterns of kind 0,
    2, 1, 2 (forward only), 0 in a row on the dirty context, the kind-0 and kind-2 ones with equal tables;
  * the image entries of two models: the second runs the first's calls reversed, each after a call of another family at
    another shape and once after the big dirtier, and returns the first's bytes, guard figures included.
"""
import contextlib
import importlib
import os

import numpy as np
import pytest
import torch

import history_cases as hc
import lexicon_ref
import lm_beam_ref as lr
import lm_sweep_ref as swr
import masked_cases as mc
import nbest_ref as nr
import skip_beam_ref as skr
import test_gpu_masked as tm
import test_gpu_nbest_skip as tskip
import test_gpu_pattern_set as tps
import test_gpu_pattern_w as tpw
import test_gpu_words as tw

pytestmark = pytest.mark.gpu

PAT_NAMES = ("literal", "masked_literal", "union", "live_plus")
PATW_PROBES = ["pattern_w.union", "pattern_w.live_plus", "pattern.union.fwd", "pattern_w.union.fwd"]
SWITCHES = [("HCTR_SPOT_CLASSES", "4", ["spot"]), ("HCTR_LEX_CLASSES", "4", ["lexicon"]),
            ("HCTR_PAT_LINES", "1", ["pattern." + p for p in PAT_NAMES] + ["pattern_set"] + PATW_PROBES),
            ("HCTR_PATSET_LDS", "0", ["pattern_set"]), ("HCTR_WORDS_LDS", "0", ["words"]),
            ("HCTR_WORDS_LINES", "1", ["words"])]
BOTH = {"HCTR_PATSET_LDS": ("HCTR_PAT_LINES", "pattern_set"), "HCTR_WORDS_LDS": ("HCTR_WORDS_LINES", "words")}
NBEST_FIELDS = ("labels", "lengths", "logps", "scores", "counts")
REC_FIELDS = ("labels", "lengths", "starts", "ends", "logps", "alt_labels", "alt_logps", "path_logp", "text_nll")


@contextlib.contextmanager
def switch(name, value):
    """an engine switch that is read at every call, set around one"""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


class Env(object):
    """what the probes and dirtiers are called with: the cases, their host-built tables (Lexicon, Pattern, flat LM) and
    device copies of the probes' logits"""

    def __init__(self, pkg, work):
        self.pkg = pkg
        self.ctc = ctc = importlib.import_module(pkg.__name__ + ".ctc")
        self.model_mod = importlib.import_module(pkg.__name__ + ".model")
        codec_mod = importlib.import_module(pkg.__name__ + ".codec")
        self.v, self.vo = hc.vocab()
        self.lex, self.pats = tm._tables(ctc, "vocab")
        self.ps = hc.patset()
        self.ps_pat = ctc.Pattern.from_sets(self.ps["arcs"], self.ps["sets"], self.ps["finals"], self.ps["num_states"], self.ps["C"])
        assert self.ps_pat.kind == 1 and all(p.kind == 0 for p in self.pats.values())
        self.wd, self.pw = hc.words(), hc.pattern_w()
        self.wlex = ctc.Lexicon(self.wd["entries"], num_classes=mc.C, priors=self.wd["priors"])
        self.wpats = {k: ctc.Pattern(p["arcs"], p["finals"], p["states"], mc.C, weights=p["weights"],
                                     final_weights=p["final_weights"]) for k, p in self.pw.items()}
        assert all(p.kind == 2 for p in self.wpats.values())
        for k, p in self.wpats.items():                       # equal tables: only the weights tell kind 2 from kind 0
            assert all(p.tables()[t].tobytes() == self.pats[k].tables()[t].tobytes() for t in p.tables()), k
        self.ed, self.nb, self.wide = hc.edit(), hc.nbest(), hc.recognize_wide()
        self.arpa = hc.arpa(work)
        self.lm = codec_mod.ArpaLM(self.arpa)                        # (kept: it owns the flat handle)
        self.flat = self.lm.flat(hc.chars(self.nb["C"]))
        self.dev = {k: torch.from_numpy(z).cuda(0) for k, z in (("vocab", self.v["logits"]), ("patset", self.ps["logits"]),
                                                                 ("nbest", self.nb["logits"]), ("wide", self.wide["logits"]))}
        torch.cuda.synchronize()
        self.dirt = {}
        for kind, d in (("big", hc.big()), ("small", hc.small())):
            C = d["logits"].shape[2]
            self.dirt[kind] = dict(case=d, lex=ctc.Lexicon(d["entries"], num_classes=C),
                                   pats=[ctc.Pattern(*p, C) for p in d["patterns"].values()],
                                   set_pat=ctc.Pattern.from_sets(*d["set_pattern"], C),
                                   words_lex=ctc.Lexicon(d["words_entries"], num_classes=C) if d["words_entries"] else None,
                                   wpats=[ctc.Pattern(*p, C, weights=d["pattern_weights"][k][0],
                                                      final_weights=d["pattern_weights"][k][1])
                                          for k, p in d["patterns"].items()])
        big = self.dirt["big"]
        assert big["words_lex"].info()["nodes"] > ctc.WORDS_LDS_NODES >= big["lex"].info()["nodes"]
        assert all(p.kind == 2 for kind in self.dirt for p in self.dirt[kind]["wpats"])
        self._bound = []

    def new_ctx(self):
        """a new weightless context (kept alive for the module)"""
        b = self.pkg.CTCAligner().cuda(0)
        self._bound.append(b)
        return b._context()


@pytest.fixture(scope="module")
def E(pkg, tmp_path_factory):
    return Env(pkg, tmp_path_factory.mktemp("history"))


def run_probe(E, ctx, name, dev=False):
    """one probe on `ctx` -> {output name: numpy array}, the names of tests/test_gpu_masked.py's run_all where it has them"""
    ctc, on = E.ctc, int(dev)
    if name == "edit":
        ev = ctc.edit_distance_sequences(ctx, E.ed["hyps"], E.ed["refs"], True)
        return {"edit." + k: getattr(ev, k) for k in ("edits", "counts", "ref_map", "hyp_map")}
    if name == "recognize_wide":
        r = ctc.recognize_logits(ctx, E.dev["wide"] if dev else E.wide["logits"], on)
        return {"wide." + k: getattr(r, k) for k in REC_FIELDS}
    if name == "pattern_set":
        z = E.dev["patset"] if dev else E.ps["logits"]
        r = ctc.pattern_logits(ctx, z, on, E.ps_pat, E.ps["il"])
        return {"ps." + f: getattr(r, f) for f in r.FIELDS}
    if name in ("nbest_logits", "nbest_topk", "nbest_lm", "skip_zero", "skip_lm", "lm_sweep"):
        nb = E.nb
        z = E.dev["nbest"] if dev else nb["logits"]
        kw = dict(n=nb["n"], beam=nb["beam"], len_bonus=nb["bonus"], input_lengths=nb["il"])
        if name == "lm_sweep":
            s = ctc.lm_sweep_logits(ctx, z, on, nb["tg"], nb["tl"], E.flat, pairs=nb["grid"], beam=nb["beam"], depth=nb["k"],
                                    input_lengths=nb["il"], texts=True)
            return {"sweep." + k: getattr(s, k) for k in ("edits", "hyp_lengths", "empty", "labels", "logps", "scores", "lm_scores")}
        if name == "nbest_topk":
            r, fields = ctc.nbest_topk(ctx, nb["idx"], nb["lp"], nb["C"], **kw), NBEST_FIELDS
        elif name == "nbest_logits":
            r, fields = ctc.nbest_logits(ctx, z, on, depth=nb["k"], **kw), NBEST_FIELDS
        elif name == "nbest_lm":
            r = ctc.nbest_logits(ctx, z, on, depth=nb["k"], lm=E.flat, lm_panelty=nb["pen"], **kw)
            fields = NBEST_FIELDS + ("lm_scores",)
        else:
            r = ctc.nbest_skip_logits(ctx, z, on, lm=E.flat if name == "skip_lm" else None, lm_panelty=nb["pen"], **kw)
            fields = tskip.FIELDS
        return {"%s.%s" % (name, f): getattr(r, f) for f in fields}
    c = E.v
    z = E.dev["vocab"] if dev else c["logits"]
    tg, tl, il = c["targets"], c["tl"], c["il"]
    if name == "loss":
        return {"nll": ctc.loss_logits(ctx, z, on, tg, tl, il)}
    if name == "grad":
        nll, g = ctc.loss_grad_logits(ctx, z, on, tg, tl, il, None)
        return {"grad.nll": nll, "grad": g.cpu().numpy() if dev else g}
    if name == "align":
        al = ctc.align_logits(ctx, z, on, tg, tl, il)
        return {"align." + k: getattr(al, k) for k in ("paths", "scores", "starts", "ends", "logps")}
    if name == "spot":
        sp = ctc.spot_logits(ctx, z, on, mc.queries(c), il)
        return {"spot." + k: getattr(sp, k) for k in ("logp", "seg_logp", "starts", "ends")}
    if name == "lexicon":
        lx = ctc.lexicon_logits(ctx, z, on, E.lex, len(E.lex), il, True)
        return {"lex." + k: getattr(lx, k) for k in ("entries", "logp", "rank", "log_total", "count", "scores")}
    if name == "words":
        r = ctc.words_logits(ctx, z, on, E.wlex, E.wd["bonus"], None, il)
        return {"words." + f: getattr(r, f) for f in tw.FIELDS}
    if name.endswith(".fwd"):                                 # the forward-only instance: logp alone
        kind, pname, _ = name.split(".")
        r = ctc.pattern_logits(ctx, z, on, (E.wpats if kind == "pattern_w" else E.pats)[pname], il, full=False)
        assert r.best_logp is None and r.path is None
        return {name + ".logp": r.logp}
    if name.startswith("pattern_w."):
        pname = name.split(".")[1]
        r = ctc.pattern_logits(ctx, z, on, E.wpats[pname], il)
        return {"patw.%s.%s" % (pname, f): getattr(r, f) for f in tpw.FIELDS}       # (weights: the host's, of the texts)
    if name.startswith("pattern."):
        pname = name.split(".")[1]
        r = ctc.pattern_logits(ctx, z, on, E.pats[pname], il)
        return {"pat.%s.%s" % (pname, f): getattr(r, f) for f in r.FIELDS}
    if name == "recognize":
        r = ctc.recognize_logits(ctx, z, on)
        return {"rec." + k: getattr(r, k) for k in REC_FIELDS}
    assert name == "evaluate", name
    ev = ctc.evaluate_logits(ctx, z, on, tg, tl, True)
    return {"ev." + k: getattr(ev, k) for k in ("labels", "lengths", "edits", "counts", "ref_map", "hyp_map")}


def run_dirtier_words(E, ctx, kind, which=("scratch", "lds")):
    """the dirtier's words calls: the big one's lexicon of more than 4096 trie nodes (the scratch form: step buffers of
    2 * nodes * 16 bytes a line in the block, three lines of them non-finite), then its small lexicon (the LDS form's
    exit records); the small one's one entry at W = 2. HCTR_OK, and what the contract says of the non-finite lines."""
    ctc, d = E.ctc, E.dirt[kind]
    c = d["case"]
    for form in which:
        lex = d["words_lex"] if form == "scratch" else d["lex"]
        if lex is None:
            continue
        r = ctc.words_logits(ctx, c["logits"], 0, lex, c["words_bonus"], None, c["il"])
        bad = sorted(hc.BIG_BAD) if kind == "big" else []
        assert (r.count[bad] == 0).all() and np.isneginf(r.score[bad]).all() and np.isposinf(r.text_nll[bad]).all(), form
        assert (np.delete(r.count, bad) >= 1).all() and np.isfinite(np.delete(r.score, bad)).all(), form


def run_dirtier(E, ctx, kind):
    """the big or the small dirtier: every call returns HCTR_OK (``_lib.check`` raises otherwise)"""
    ctc, d = E.ctc, E.dirt[kind]
    c = d["case"]
    z, tg, tl, il = c["logits"], c["targets"], c["tl"], c["il"]
    ctc.loss_grad_logits(ctx, z, 0, tg, tl, il, None)
    ctc.align_logits(ctx, z, 0, tg, tl, il)
    ctc.spot_logits(ctx, z, 0, c["queries"], il)
    ctc.lexicon_logits(ctx, z, 0, d["lex"], min(len(d["lex"]), ctc.LEX_MAX_TOP), il, True)
    run_dirtier_words(E, ctx, kind)
    for p in d["pats"] + [d["set_pat"]]:
        ctc.pattern_logits(ctx, z, 0, p, il)
    for p in d["wpats"]:
        ctc.pattern_logits(ctx, z, 0, p, il)
        if kind == "big":
            ctc.pattern_logits(ctx, z, 0, p, il, full=False)
    ctc.recognize_logits(ctx, z, 0)
    ctc.evaluate_logits(ctx, z, 0, tg, tl, True)
    ctc.edit_distance_sequences(ctx, c["edit"][0], c["edit"][1], True)
    ctc.nbest_logits(ctx, c["clean"], 0, len_bonus=5.8, input_lengths=il, **c["search"])


def same(got, want, what):
    assert list(got) == list(want), what
    for k in want:
        x, y = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert x.dtype == y.dtype and x.shape == y.shape, (what, k, x.dtype, y.dtype, x.shape, y.shape)
        if x.tobytes() != y.tobytes():
            bad = np.flatnonzero(x.reshape(-1).view(np.uint8) != y.reshape(-1).view(np.uint8)) // x.dtype.itemsize
            at = np.unravel_index(int(bad[0]), x.shape) if x.ndim else ()
            raise AssertionError("%s: %s differs in %d entries, first at %s: %r, base %r"
                                 % (what, k, len(set(bad.tolist())), at, x[at], y[at]))


_BASE, _DIRTY = {}, {}


@pytest.fixture(scope="module")
def base(E):
    """name -> the probe's result as the first call on a new context"""
    def get(name):
        if name not in _BASE:
            _BASE[name] = run_probe(E, E.new_ctx(), name)
        return _BASE[name]
    return get


@pytest.fixture(scope="module")
def dirty_ctx(E):
    return E.new_ctx()


@pytest.fixture(scope="module")
def dirty(E, dirty_ctx):
    """name -> the probe's result right after the big dirtier, all on one context"""
    def get(name):
        if name not in _DIRTY:
            run_dirtier(E, dirty_ctx, "big")
            _DIRTY[name] = run_probe(E, dirty_ctx, name)
        return _DIRTY[name]
    return get


# ---- 1. the first call against the existing oracles -----------------------------------------------------------------
def test_base_of_the_masked_family_against_float64(E, base):
    """tests/test_gpu_masked.py's own checks, run on the first-call results of the `vocab` probes"""
    merged = {}
    for name in ["loss", "grad", "align", "spot", "lexicon", "recognize"] + ["pattern." + p for p in PAT_NAMES]:
        for k, v in base(name).items():                       # (run_all's layouts)
            merged[k] = (v, "WBC" if k == "grad" else "flat" if k in ("align.starts", "align.ends", "align.logps") else "B")
    tm.check_scores_against_float64("vocab", merged)
    g64, g32 = mc.torch_grads(E.v)
    tm._check_grad(merged["grad"][0], E.v, g64, g32, np.ones(5), "vocab, first call")


def test_base_of_the_set_form_against_float64(E, base):
    r, want = base("pattern_set"), E.ps["want"]
    tps._check_scores(r["ps.logp"], [w[0] for w in want], "set form logp")
    tps._check_scores(r["ps.best_logp"], [w[1] for w in want], "set form best_logp")
    for b, w in enumerate(want):
        T = int(E.ps["il"][b])
        assert r["ps.path"][b, :T].tolist() == w[2] and r["ps.lengths"][b] == len(E.ps["labels"][b]), b
        assert r["ps.labels"][b, :r["ps.lengths"][b]].tolist() == E.ps["labels"][b], b


def test_base_of_the_words_probe_against_float64(E, base):
    """tests/test_gpu_words.py's ``check``: the score within 1e-5 relative + 1e-3 of words_ref's, the -inf pattern, the
    fills, labels / count / lengths against the returned words, and the sandwich on the returned segmentation"""
    r, c = base("words"), E.v
    res = E.ctc.WordsResult(*[r["words." + f] for f in tw.FIELDS], input_lengths=c["il"])
    tw.check(res, c["logits"], c["il"], E.wd["entries"], E.wd["priors"], E.wd["bonus"], E.wd["want"], "words probe")
    want = np.array([w[0] for w in E.wd["want"]])
    print("words probe: largest |score - float64| %.3e" % np.abs(res.score - want).max())
    assert (res.count >= 1).all() and res.count.max() >= 2 and len(set(res.count.tolist())) >= 2
    tw.text_nll_bits(E.ctc, E.new_ctx(), res, c["logits"], c["il"], "words probe")


def test_base_of_the_weighted_patterns_against_float64(E, base):
    """tests/test_gpu_pattern_w.py's ``check_against``: logp and best_logp within 1e-5 relative + 1e-3 of pattern_w_ref's
    with an equal -inf pattern, the path, spans and the text's weight equal; the forward-only instances' logp by the
    same rule, and with the bits of the full call's"""
    c = E.v
    for pname, p in E.pw.items():
        r = base("pattern_w." + pname)
        res = E.ctc.PatternResult(*[r["patw.%s.%s" % (pname, f)] for f in tpw.FIELDS])
        tpw.check_against(res, p["want"], p["tab"], E.wpats[pname], c["logits"], c["il"], "pattern_w." + pname)
        for k, f in ((0, "logp"), (1, "best_logp")):
            want = np.array([w[k] for w in p["want"]])
            print("pattern_w.%s: largest |%s - float64| %.3e" % (pname, f, np.abs(getattr(res, f) - want).max()))
        plain = base("pattern." + pname)
        texts = [res.labels[b, :res.lengths[b]].tolist() for b in range(len(res))]
        other = [plain["pat.%s.labels" % pname][b, :plain["pat.%s.lengths" % pname][b]].tolist() for b in range(len(res))]
        assert texts != other, pname                           # the weights decide a line: the kind-0 tables cannot pass
    for name, want, full in (("pattern.union.fwd", [w[0] for w in E.vo["pat"]["union"]], base("pattern.union")["pat.union.logp"]),
                             ("pattern_w.union.fwd", [w[0] for w in E.pw["union"]["want"]],
                              base("pattern_w.union")["patw.union.logp"])):
        got = base(name)[name + ".logp"]
        tpw._check_scores(got, want, name)
        print("%s: largest |logp - float64| %.3e" % (name, np.abs(got - np.array(want)).max()))
        assert got.tobytes() == full.tobytes(), name
    assert base("pattern.union.fwd")["pattern.union.fwd.logp"].tobytes() != base("pattern_w.union.fwd")["pattern_w.union.fwd.logp"].tobytes()


def test_base_of_the_wide_recognition(E, base):
    """tests/test_gpu_masked.py's rule for recognition: integers exactly, scores within 1e-5 * |want| + 1e-3"""
    r, want = base("recognize_wide"), E.wide["want"]
    for k in ("lengths", "labels", "starts", "ends", "alt_labels"):
        np.testing.assert_array_equal(r["wide." + k], want[k], err_msg=k)
    for k in ("path_logp", "text_nll", "logps", "alt_logps"):
        tm._check_scores(r["wide." + k], want[k], "wide recognition " + k)
    assert [r["wide.labels"][b, :n].tolist() for b, n in enumerate(r["wide.lengths"])] == E.wide["texts"]


def test_base_of_the_edit_family(E, base):
    r = base("edit")
    for k, want in E.ed["want"].items():
        np.testing.assert_array_equal(r["edit." + k], want, err_msg=k)
    r, want = base("evaluate"), hc.evaluate_want()
    np.testing.assert_array_equal(r["ev.lengths"], want["lengths"])
    for b, n in enumerate(want["lengths"]):
        assert r["ev.labels"][b, :n].tolist() == want["labels"][b, :n].tolist(), b
    for k in ("edits", "counts", "ref_map", "hyp_map"):
        np.testing.assert_array_equal(r["ev." + k], want[k], err_msg=k)


def _tol(T, want):
    return 1e-14 * T * np.maximum(1.0, np.abs(want))


def _check_search(name, T, r, labels, lengths, logp, score, count, gap, lm=None):
    """tests/test_gpu_nbest.py's and test_gpu_nbest_lm.py's rule: integers and the n-gram score exactly, logp and score
    within 1e-14 * T * max(1, |want|), on a yardstick whose own ranking is settled"""
    fin = np.isfinite(score)
    worst = float(_tol(T, np.concatenate([logp[fin], score[fin]])).max())
    assert gap >= 100 * worst, "the yardstick's own ranking is not settled"
    np.testing.assert_array_equal(r[name + ".counts"], count)
    np.testing.assert_array_equal(r[name + ".lengths"], lengths)
    np.testing.assert_array_equal(r[name + ".labels"], labels)
    if lm is not None:
        assert r[name + ".lm_scores"].tobytes() == lm.tobytes()
    for g, w, what in ((r[name + ".logps"], logp, "logp"), (r[name + ".scores"], score, "score")):
        np.testing.assert_array_equal(g[~fin], w[~fin], err_msg=what)
        err = np.abs(g[fin] - w[fin])
        print("%s %s: max |d| %.3e over %d figures" % (name, what, err.max() if err.size else 0.0, err.size))
        assert (err <= _tol(T, w[fin])).all(), (name, what)


def test_base_of_the_searches_against_their_yardsticks(E, base):
    """the list entry on the numpy lists; the logits entries on the engine's own front-end lists of the same logits
    (taken on another context), which is what they are specified to search"""
    nb = E.nb
    T, B, C, k, beam, n, pen, bonus, il = (nb[x] for x in ("T", "B", "C", "k", "beam", "n", "pen", "bonus", "il"))
    ctx = E.new_ctx()
    fe = E.model_mod.beam_frontend_call(ctx, None, 1, 0, None, nb["logits"], 0, B, T, C, k, False)
    fs = E.model_mod.beam_frontend_call(ctx, None, 1, 0, None, nb["logits"], 0, B, T, C, 1, True)
    skip_lists = (fs["topk_idx"][:, :, 0], fs["blank_logp"], fs["cand_off"], fs["cand_idx"], fs["cand_logp"])
    _check_search("nbest_topk", T, base("nbest_topk"), *nr.search(nb["idx"], nb["lp"], C, beam, n, bonus, il)[:6])
    _check_search("nbest_logits", T, base("nbest_logits"), *nr.search(fe["topk_idx"], fe["topk_logp"], C, beam, n, bonus, il)[:6])
    w = lr.search(lr.make_codec(C, k, E.arpa, pen, bonus), fe["topk_idx"], fe["topk_logp"], beam, n, il)
    _check_search("nbest_lm", T, base("nbest_lm"), w["labels"], w["lengths"], w["logp"], w["score"], w["count"], w["gap"], w["lm"])
    for name, path in (("skip_zero", None), ("skip_lm", E.arpa)):
        want = skr.search(skr.make_codec(C, path, pen, bonus), *skip_lists, beam, n, il)
        r = base(name)
        tskip.compare(name, T, E.ctc.NBest(*[r["%s.%s" % (name, f)] for f in tskip.FIELDS[:5]],
                                           **{f: r["%s.%s" % (name, f)] for f in tskip.FIELDS[5:]}), want)
        assert (want["status"] == 0).all() and (want["count"] > 0).all()
    want = swr.yardstick(fe["topk_idx"], fe["topk_logp"], il, nb["tg"], nb["tl"], E.arpa, nb["grid"], C=C, k=k, beam=beam)
    assert all(swr.properties(want)) and swr.settled(want, T)
    r = base("lm_sweep")
    for key, wk in (("empty", "empty"), ("hyp_lengths", "hyp_lengths"), ("labels", "labels"), ("edits", "edits")):
        np.testing.assert_array_equal(r["sweep." + key], want[wk], err_msg=key)
    for key, wk in (("logps", "logp"), ("scores", "score"), ("lm_scores", "lm")):
        assert (np.abs(r["sweep." + key] - want[wk]) <= swr.tol(T, want[wk])).all(), key


# ---- 2. after the big dirtier ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", hc.PROBES)
def test_after_the_big_dirtier(name, base, dirty):
    same(dirty(name), base(name), name + " after the big dirtier")


@pytest.mark.parametrize("name", hc.LOGITS_PROBES)
def test_device_pointer_after_the_big_dirtier(name, E, base, dirty_ctx):
    run_dirtier(E, dirty_ctx, "big")
    same(run_probe(E, dirty_ctx, name, dev=True), base(name), name + ", device pointer, after the big dirtier")


@pytest.mark.parametrize("var,value,names", SWITCHES, ids=[s[0] for s in SWITCHES])
def test_layout_switches_after_the_big_dirtier(var, value, names, E, base, dirty_ctx):
    """the chunked and alternate layouts carve the scratch their own way; the results are those without the switch"""
    for name in names:
        run_dirtier(E, dirty_ctx, "big")
        with switch(var, value):
            got = run_probe(E, dirty_ctx, name)
        same(got, base(name), "%s under %s=%s after the big dirtier" % (name, var, value))
    if var in BOTH:                                           # both at once: scratch step buffers in groups of one line
        lines, name = BOTH[var]
        run_dirtier(E, dirty_ctx, "big")
        with switch(var, value), switch(lines, "1"):
            got = run_probe(E, dirty_ctx, name)
        same(got, base(name), name + " under both switches")


@pytest.mark.parametrize("form", ["scratch", "lds"])
def test_words_right_after_the_big_words_calls(form, E, base, dirty_ctx):
    """nothing in between: the probe carves its emissions, records and (in the scratch form) step buffers from the bytes
    a words call of eight lines, three of them non-finite, just left - the large trie's scratch-form buffers and
    records, or the LDS form's records of 160 columns, which the walk back must never follow"""
    for switches in ((), (("HCTR_WORDS_LDS", "0"),), (("HCTR_WORDS_LDS", "0"), ("HCTR_WORDS_LINES", "1"))):
        run_dirtier(E, dirty_ctx, "big")
        run_dirtier_words(E, dirty_ctx, "big", which=(form,))
        with contextlib.ExitStack() as stack:
            for var, value in switches:
                stack.enter_context(switch(var, value))
            got = run_probe(E, dirty_ctx, "words")
        same(got, base("words"), "words after the big %s-form words call, %s" % (form, dict(switches)))


# ---- 3. the grow path -----------------------------------------------------------------------------------------------
def test_after_the_small_dirtier_in_ascending_order(E, base):
    """a context that has run only the small dirtier holds a small block: every probe that needs more than the calls
    before it grows it (the order is by estimated need; the sizes are not read back from the engine)"""
    ctx = E.new_ctx()
    run_dirtier(E, ctx, "small")
    for name in hc.PROBES:
        same(run_probe(E, ctx, name), base(name), name + " after the small dirtier")


@pytest.mark.parametrize("name", hc.PROBES)
def test_first_call_after_the_small_dirtier(name, E, base):
    """the same with nothing in between, on a context per probe: the probe's own growth from the small dirtier's block"""
    ctx = E.new_ctx()
    run_dirtier(E, ctx, "small")
    same(run_probe(E, ctx, name), base(name), name + " right after the small dirtier")


def test_recognition_moves_its_kept_log_sum_exps(E, base):
    """``ctc_reserve(keep)``: the wide probe's second request exceeds its first (tests/test_history_host.py asserts the
    numbers), so the block grows in mid-call and the log-sum-exps move - from a block that recognition of the small
    case alone sized (3328 bytes, by the same formula), and from one a larger recognition sized, where the first request
    fits and only the move allocates"""
    first, second, kept = hc.recognize_needs(E.wide["want"]["labels"], E.wide["want"]["lengths"], hc.WIDE_W)
    assert second > first > kept
    ctx = E.new_ctx()
    E.ctc.recognize_logits(ctx, hc.small()["logits"], 0)
    same(run_probe(E, ctx, "recognize_wide"), base("recognize_wide"), "after the small recognition")
    same(run_probe(E, ctx, "recognize_wide"), base("recognize_wide"), "again, the block large enough")
    ctx = E.new_ctx()
    same(run_probe(E, ctx, "recognize"), base("recognize"), "the vocab recognition")       # 12544 bytes: first <= it < second
    same(run_probe(E, ctx, "recognize_wide"), base("recognize_wide"), "after the vocab recognition")


# ---- 4. every family after every other ------------------------------------------------------------------------------
def test_mixed_order_on_one_context(E, base):
    ctx = E.new_ctx()
    for rnd, order in (("in order", hc.PROBES), ("reversed", hc.PROBES[::-1]), ("twice", [p for p in hc.PROBES for _ in (0, 1)])):
        for name in order:
            same(run_probe(E, ctx, name), base(name), "%s, %s" % (name, rnd))


# ---- 5. the documented fills, on the results that followed the big dirtier -------------------------------------------
def _beyond(a, lengths):
    """the entries a[b, lengths[b]:] of every line, flat"""
    return np.concatenate([np.asarray(a[b, int(n):]).reshape(-1) for b, n in enumerate(lengths)])


def test_documented_fills(E, dirty):
    c = E.v
    for name, key in (("recognize", "rec."), ("recognize_wide", "wide.")):
        r = dirty(name)
        for k in ("labels", "starts", "ends", "logps", "alt_labels", "alt_logps"):
            assert not _beyond(r[key + k], r[key + "lengths"]).any(), "%s %s beyond lengths" % (name, k)
    for name, il in [("pat.%s." % p, c["il"]) for p in PAT_NAMES] + [("ps.", E.ps["il"])]:
        r = dirty("pattern_set" if name == "ps." else "pattern." + name.split(".")[1])
        for k in ("labels", "starts", "ends", "logps"):
            assert not _beyond(r[name + k], r[name + "lengths"]).any(), name + k
        feasible = np.isfinite(r[name + "best_logp"])
        assert (_beyond(r[name + "path"], np.where(feasible, il, 0)) == -1).all(), name + "path"
    r = dirty("align")
    assert (_beyond(r["align.paths"], np.where(np.isfinite(r["align.scores"]), c["il"], 0)) == -1).all()
    assert not _beyond(dirty("edit")["edit.hyp_map"], E.ed["n"]).any()
    r = dirty("evaluate")
    assert not _beyond(r["ev.hyp_map"], r["ev.lengths"]).any() and not _beyond(r["ev.labels"], r["ev.lengths"]).any()
    for name in ("nbest_logits", "nbest_topk", "nbest_lm", "skip_zero", "skip_lm"):
        r = dirty(name)
        labels, lengths, counts = r[name + ".labels"], r[name + ".lengths"], r[name + ".counts"]
        B, n, W = labels.shape
        assert not _beyond(labels.reshape(B * n, W), lengths.reshape(-1)).any(), name
        assert not _beyond(lengths, counts).any(), name
        for k in ("logps", "scores") + (("lm_scores",) if name + ".lm_scores" in r else ()):
            assert np.isneginf(_beyond(r["%s.%s" % (name, k)], counts)).all(), (name, k)
    r = dirty("lm_sweep")
    G, B, W = r["sweep.labels"].shape
    assert not _beyond(r["sweep.labels"].reshape(G * B, W), r["sweep.hyp_lengths"].reshape(-1)).any()
    r = dirty("lexicon")
    assert (r["lex.count"] < r["lex.entries"].shape[1]).any(), "no line leaves a place unused"
    assert (_beyond(r["lex.entries"], r["lex.count"]) == -1).all()
    assert np.isneginf(_beyond(r["lex.logp"], r["lex.count"])).all() and np.isneginf(_beyond(r["lex.rank"], r["lex.count"])).all()
    _words_fills(dirty("words"), "the words probe", some=True)
    for pname in E.pw:
        _weighted_fills(dirty("pattern_w." + pname), "patw.%s." % pname, c["il"], some=True)


def _words_fills(r, what, some=False, none=False):
    """words / starts are -1 beyond count, labels 0 beyond lengths; a line without a segmentation has score -inf, count
    and lengths 0, text_nll +inf. ``some`` / ``none``: there are lines with / without a segmentation, and unused places"""
    count, lengths = r["words.count"], r["words.lengths"]
    have = count > 0
    assert (_beyond(r["words.words"], count) == -1).all() and (_beyond(r["words.starts"], count) == -1).all(), what
    assert not _beyond(r["words.labels"], lengths).any(), what
    assert np.isneginf(r["words.score"][~have]).all() and np.isposinf(r["words.text_nll"][~have]).all(), what
    assert not lengths[~have].any() and np.isfinite(r["words.score"][have]).all() and (lengths[have] > 0).all(), what
    if some:
        assert have.any() and (count[have] < r["words.words"].shape[1]).any() and (lengths[have] < r["words.labels"].shape[1]).any()
        assert all((r["words.words"][b, :n] >= 0).all() and (r["words.starts"][b, :n] >= 0).all() for b, n in enumerate(count))
    if none:
        assert (~have).any(), what


def _weighted_fills(r, key, il, some=False, none=False):
    """the pattern family's fills (labels, starts, ends, logps 0 beyond lengths; path -1 beyond the line's length, and
    everywhere on an infeasible line), and the texts' weights: NaN exactly on the infeasible lines"""
    for k in ("labels", "starts", "ends", "logps"):
        assert not _beyond(r[key + k], r[key + "lengths"]).any(), key + k
    feasible = np.isfinite(r[key + "best_logp"])
    assert (_beyond(r[key + "path"], np.where(feasible, il, 0)) == -1).all(), key + "path"
    assert (np.isnan(r[key + "weights"]) == ~feasible).all() and np.isfinite(r[key + "weights"][feasible]).all(), key + "weights"
    assert not r[key + "lengths"][~feasible].any() and np.isposinf(r[key + "text_nll"][~feasible]).all(), key
    if some:
        assert feasible.any() and (r[key + "lengths"][feasible] < r[key + "labels"].shape[1]).any(), key
        assert (np.asarray(il)[feasible] < r[key + "path"].shape[1]).any(), key + ": no feasible line leaves path places unused"
    if none:
        assert (~feasible).any(), key


def test_documented_fills_of_lines_without_a_reading(E, dirty_ctx):
    """the `vocab` probes of the words and the weighted pattern calls read every line, so their own results cannot show
    the fills of a line that has no reading. At the same shape, after the big dirtier: the words call on the three
    entries of the probe's lexicon that need the masked class 9 (no line has a segmentation), and `vocab`'s literal
    through class 9 as a weighted pattern (no line has a path)."""
    c = E.v
    es = [e for e in E.wd["entries"] if 9 in e]
    assert len(es) >= 2
    lex = E.ctc.Lexicon(es, num_classes=mc.C, priors=np.arange(len(es), dtype=np.float32))
    run_dirtier(E, dirty_ctx, "big")
    r = E.ctc.words_logits(dirty_ctx, c["logits"], 0, lex, E.wd["bonus"], None, c["il"])
    r = {"words." + f: getattr(r, f) for f in tw.FIELDS}
    _words_fills(r, "entries through a masked class", none=True)
    assert not r["words.count"].any() and (r["words.words"] == -1).all() and not r["words.labels"].any()
    arcs, finals, ns = mc.patterns(c)["masked_literal"]
    pat = E.ctc.Pattern(arcs, finals, ns, mc.C, weights=np.full(len(arcs), 1.5), final_weights=[-0.5] * len(finals))
    assert pat.kind == 2
    run_dirtier(E, dirty_ctx, "big")
    r = E.ctc.pattern_logits(dirty_ctx, c["logits"], 0, pat, c["il"])
    r = {"patw." + f: getattr(r, f) for f in tpw.FIELDS}
    _weighted_fills(r, "patw.", c["il"], none=True)
    assert np.isnan(r["patw.weights"]).all() and (r["patw.path"] == -1).all() and np.isneginf(r["patw.logp"]).all()


# ---- 6. the cached tables ---------------------------------------------------------------------------------------------
def _lexicon(E, ctx, lex):
    c = E.v
    lx = E.ctc.lexicon_logits(ctx, c["logits"], 0, lex, min(len(lex), E.ctc.LEX_MAX_TOP), c["il"], True)
    return {"lex." + k: getattr(lx, k) for k in ("entries", "logp", "rank", "log_total", "count", "scores")}


def _second_lexicon(E):
    """some 400 entries over the vocabulary's live labels in units of 128 nodes: several units, where `vocab`'s has one"""
    rng = np.random.RandomState(9950)
    es = [[int(v) for v in rng.randint(1, 8, size=rng.randint(1, 7))] for _ in range(400)]
    lex = E.ctc.Lexicon(es, num_classes=mc.C, unit_nodes=128)
    assert lex.info()["units"] > E.lex.info()["units"] == 1
    return lex, es


def test_two_lexicons_alternate(E, base):
    ctx = E.new_ctx()
    other, es = _second_lexicon(E)
    a1 = _lexicon(E, ctx, E.lex)
    b1 = _lexicon(E, ctx, other)
    same(_lexicon(E, ctx, E.lex), a1, "lexicon A after B")
    same(_lexicon(E, ctx, other), b1, "lexicon B after A")
    same(a1, base("lexicon"), "lexicon A")
    same(_lexicon(E, E.new_ctx(), other), b1, "lexicon B as a first call")
    want = lexicon_ref.scores(E.v["logits"], es, E.v["il"])
    tm._check_scores(b1["lex.scores"], want, "lexicon B against float64")


def _words(E, ctx, lex, bonus=None):
    c = E.v
    r = E.ctc.words_logits(ctx, c["logits"], 0, lex, E.wd["bonus"] if bonus is None else bonus, None, c["il"])
    return {"words." + f: getattr(r, f) for f in tw.FIELDS}


def test_one_lexicon_through_the_exact_and_the_words_call(E, base):
    """the exact-lexicon call's device copy, the words call's host tables and its device copy all go by the one serial
    of the object: neither call takes the other's tables for its own"""
    ctx = E.new_ctx()
    first = {}
    for rnd in range(2):
        for key, call in (("lexicon", _lexicon), ("words", _words)):
            got = call(E, ctx, E.wlex)
            same(got, first.setdefault(key, got), "%s, round %d" % (key, rnd))
    same(first["words"], base("words"), "words after the exact-lexicon call")
    same(_lexicon(E, E.new_ctx(), E.wlex), first["lexicon"], "the exact-lexicon call as a first call")


def test_one_lexicon_under_two_bonuses(E, base):
    """the word tables hold prior + bonus: another bonus on the same lexicon is another set of tables, on the host and on
    the device"""
    ctx = E.new_ctx()
    first = {}
    for rnd in range(2):
        for bonus in (E.wd["bonus"], 1.25):
            got = _words(E, ctx, E.wlex, bonus)
            same(got, first.setdefault(bonus, got), "bonus %g, round %d" % (bonus, rnd))
    a, b = first[E.wd["bonus"]], first[1.25]
    same(a, base("words"), "the probe's bonus")
    assert (a["words.count"] >= 1).all() and (b["words.count"] >= 1).all()       # so 1.75 a word parts the scores
    assert (b["words.score"] > a["words.score"] + 1.0).all()
    same(_words(E, E.new_ctx(), E.wlex, 1.25), b, "the other bonus as a first call")


def test_two_lexicons_alternate_through_the_words_call(E, base):
    ctx = E.new_ctx()
    other, es = _second_lexicon(E)
    assert other.info()["nodes"] > E.wlex.info()["nodes"]
    a1 = _words(E, ctx, E.wlex)
    b1 = _words(E, ctx, other)
    same(_words(E, ctx, E.wlex), a1, "words of lexicon A after B")
    same(_words(E, ctx, other), b1, "words of lexicon B after A")
    same(a1, base("words"), "words of lexicon A")
    same(_words(E, E.new_ctx(), other), b1, "words of lexicon B as a first call")
    c = E.v
    res = E.ctc.WordsResult(*[b1["words." + f] for f in tw.FIELDS], input_lengths=c["il"])
    tw.check(res, c["logits"], c["il"], es, None, E.wd["bonus"], tw.ref.words(c["logits"], es, None, E.wd["bonus"], c["il"]),
             "words of lexicon B against float64")


def test_lexicon_freed_and_another_built(E, base):
    """the device copy and the host tables are recognised by serial number: a lexicon built where a freed one lay is
    another lexicon"""
    c = E.v
    lists = {"probe": (E.wd["entries"], E.wd["priors"]), "heads": ([e[:2] for e in E.wd["entries"] if 9 not in e], None)}
    fresh = {}
    for key, (es, pr) in lists.items():
        fresh[key] = _words(E, E.new_ctx(), E.ctc.Lexicon(es, num_classes=mc.C, priors=pr))
    same(fresh["probe"], base("words"), "the probe's list")
    assert fresh["heads"]["words.score"].tobytes() != fresh["probe"]["words.score"].tobytes()
    ctx = E.new_ctx()
    for rnd, key in enumerate(("probe", "heads", "probe", "heads")):
        lex = E.ctc.Lexicon(lists[key][0], num_classes=mc.C, priors=lists[key][1])
        same(_words(E, ctx, lex), fresh[key], "%s built anew (%d)" % (key, rnd))
        del lex


def test_pattern_kinds_in_a_row_on_the_dirty_context(E, base, dirty_ctx):
    """kind 0, 2, 1, 2 (forward only), 0 on one context after the big dirtier: the three kinds share one device block and
    one serial, the weighted block is the explicit one's plus the weights, and the kind-0 and kind-2 patterns here
    have equal tables"""
    run_dirtier(E, dirty_ctx, "big")
    for step, name in enumerate(("pattern.union", "pattern_w.union", "pattern_set", "pattern_w.union.fwd", "pattern.union")):
        same(run_probe(E, dirty_ctx, name), base(name), "%s, step %d of the kinds in a row" % (name, step))


def test_two_pattern_forms_alternate(E, base):
    ctx = E.new_ctx()
    for rnd in range(2):
        same(run_probe(E, ctx, "pattern.union"), base("pattern.union"), "explicit form, round %d" % rnd)
        same(run_probe(E, ctx, "pattern_set"), base("pattern_set"), "set form, round %d" % rnd)
    same(run_probe(E, ctx, "pattern.union"), base("pattern.union"), "explicit form after the set form")


def test_pattern_freed_and_another_built(E, base):
    """the device copy is recognised by serial number: a pattern built where a freed one lay is another pattern"""
    ctx = E.new_ctx()
    c, defs = E.v, mc.patterns(E.v)
    fields = E.ctc.PatternResult.FIELDS
    for rnd, pname in enumerate(("literal", "masked_literal", "literal", "live_plus")):
        p = E.ctc.Pattern(*defs[pname], mc.C)
        r = E.ctc.pattern_logits(ctx, c["logits"], 0, p, c["il"])
        same({"pat.%s.%s" % (pname, f): getattr(r, f) for f in fields}, base("pattern." + pname), "%s built anew (%d)" % (pname, rnd))
        del p, r


def test_one_table_on_two_contexts(E, base):
    a, b = E.new_ctx(), E.new_ctx()
    for rnd in range(2):
        for ctx in (a, b):
            same(run_probe(E, ctx, "lexicon"), base("lexicon"), "lexicon, round %d" % rnd)
            same(run_probe(E, ctx, "pattern.union"), base("pattern.union"), "pattern, round %d" % rnd)
            same(run_probe(E, ctx, "pattern_set"), base("pattern_set"), "set form, round %d" % rnd)
            same(run_probe(E, ctx, "nbest_lm"), base("nbest_lm"), "LM, round %d" % rnd)
            same(run_probe(E, ctx, "words"), base("words"), "words, round %d" % rnd)
            same(run_probe(E, ctx, "pattern_w.union"), base("pattern_w.union"), "weighted pattern, round %d" % rnd)


# ---- 7. the image entries of two models -------------------------------------------------------------------------------
SHAPES = [(3, 96), (1, 33), (5, 17)]
IMAGE_CALLS = ["greedy", "forward", "beam_frontend", "nbest", "ctc_loss", "recognize", "evaluate", "pattern", "words",
               "pattern_w"]
AUTO_GUARDED = ("greedy", "forward", "beam_frontend", "evaluate")     # the calls after which the guard figures are compared


@pytest.fixture(scope="module")
def models(pkg, synth):
    C = synth.DEFAULT_VOCAB + 2
    sd = synth.make_state_dict(C, seed=0, head="trained")
    out = []
    for _ in range(2):
        m = pkg.hctr_model(C, precision="auto").cuda(0)
        m.load_state_dict(sd)
        out.append(m)
    return out


def _font_pattern(E, synth, weighted=False):
    """one or more of the font's labels, at the model's vocabulary; ``weighted``: the same arcs with seeded weights in
    [-2, 2] (kind 2)"""
    labels = sorted(synth.font_label(k) for k in range(synth.FONT_CLASSES))
    arcs = [(0, c, 1) for c in labels] + [(1, c, 1) for c in labels]
    if not weighted:
        return E.ctc.Pattern(arcs, [1], 2, synth.DEFAULT_VOCAB + 2)
    rng = np.random.RandomState(9980)
    return E.ctc.Pattern(arcs, [1], 2, synth.DEFAULT_VOCAB + 2, weights=rng.uniform(-2, 2, len(arcs)), final_weights=[0.5])


def _font_lexicon(E, synth):
    """every font label alone and every ordered pair of two different ones, with seeded priors"""
    labels = sorted(synth.font_label(k) for k in range(synth.FONT_CLASSES))
    es = [[a] for a in labels] + [[a, b] for a in labels for b in labels if a != b]
    pr = (np.random.RandomState(9981).randn(len(es)) * 0.5).astype(np.float32)
    return E.ctc.Lexicon(es, num_classes=synth.DEFAULT_VOCAB + 2, priors=pr)


def _image_call(m, what, imgs, targets, pat):
    """one image entry -> ({name: array}, the guard figures after it); ``pat``: the plain and the weighted font pattern
    and the font lexicon"""
    tg, tl = targets
    if what == "greedy":
        g = m.greedy(imgs)
        out = {"greedy.lengths": np.array([len(x) for x in g], np.int32), "greedy.labels": np.concatenate(g + [np.zeros(0, np.int32)])}
    elif what == "forward":
        out = {"logits": m(imgs)}
    elif what == "beam_frontend":
        fe = m.beam_frontend(imgs, 10)
        out = {"fe." + k: fe[k] for k in ("topk_idx", "topk_logp", "blank_logp")}
    elif what == "nbest":
        r = m.nbest(imgs)
        out = {"nbest." + f: getattr(r, f) for f in NBEST_FIELDS}
    elif what == "ctc_loss":
        out = {"nll": np.asarray(m.ctc_loss(imgs, tg, tl, reduction="none", zero_infinity=False))}
    elif what == "recognize":
        r = m.recognize(imgs)
        out = {"rec." + k: getattr(r, k) for k in ("labels", "lengths", "starts", "ends", "logps", "alt_labels", "alt_logps",
                                                   "path_logp", "text_nll")}
    elif what == "evaluate":
        ev = m.evaluate(imgs, tg, tl)
        out = {"ev." + k: getattr(ev, k) for k in ("labels", "lengths", "edits", "counts", "ref_map", "hyp_map")}
    elif what == "words":
        r = m.words(imgs, pat["lex"], -0.5)
        out = {"words." + f: getattr(r, f) for f in tw.FIELDS}
    elif what == "pattern_w":
        r = m.pattern(imgs, pat["weighted"])
        out = {"patw." + f: getattr(r, f) for f in tpw.FIELDS}
    else:
        assert what == "pattern"
        r = m.pattern(imgs, pat["plain"])
        out = {"pat." + f: getattr(r, f) for f in r.FIELDS}
    g = m.last_guard()
    out.update({"guard.lines": np.int64(g["lines"]), "guard.flagged": np.int64(g["flagged"]), "guard.flags": g["flags"],
                "guard.min_margin": g["min_margin"], "guard.scale": g["scale"]})
    return out


def test_image_entries_of_two_models(E, synth, models):
    """model 2 runs model 1's calls reversed, each after a call of another family at another shape, and once after the
    big caller-logits dirtier on its context: the same bytes, the guard figures after every call included (the scoring
    entries leave them as they were, so they are those of the call before, which differs between the two orders: they
    are compared after the calls that set them)"""
    m1, m2 = models
    pat = {"plain": _font_pattern(E, synth), "weighted": _font_pattern(E, synth, weighted=True), "lex": _font_lexicon(E, synth)}
    assert (pat["plain"].kind, pat["weighted"].kind) == (0, 2)
    imgs = {sh: synth.make_font_lines(sh[0], sh[1], 90 + i) for i, sh in enumerate(SHAPES)}
    targets = {}
    for sh in SHAPES:                                         # each line's transcription: model 1's own greedy text
        g = m1.greedy(imgs[sh])
        targets[sh] = (np.concatenate(g + [np.zeros(0, np.int32)]).astype(np.int32), np.array([len(x) for x in g], np.int32))
    assert targets[SHAPES[0]][1].min() > 0, "the font lines of the widest shape decode to nothing"
    calls = [(what, sh) for sh in SHAPES for what in IMAGE_CALLS]
    first = {}
    for what, sh in calls:
        first[(what, sh)] = _image_call(m1, what, imgs[sh], targets[sh], pat)
    assert first[("forward", SHAPES[0])]["guard.lines"] == SHAPES[0][0]
    for i, (what, sh) in enumerate(calls[::-1]):
        if i == len(calls) // 2:
            run_dirtier(E, m2._ctx, "big")
        other = IMAGE_CALLS[(IMAGE_CALLS.index(what) + 3) % len(IMAGE_CALLS)]
        osh = SHAPES[(SHAPES.index(sh) + 1) % len(SHAPES)]
        before = _image_call(m2, other, imgs[osh], targets[osh], pat)
        got, want = _image_call(m2, what, imgs[sh], targets[sh], pat), first[(what, sh)]
        if what not in AUTO_GUARDED:                          # the figures are left as the call before left them
            same({k: v for k, v in got.items() if k.startswith("guard.")}, {k: v for k, v in before.items() if k.startswith("guard.")},
                 "guard figures across %s at %s" % (what, sh))
            got = {k: v for k, v in got.items() if not k.startswith("guard.")}
            want = {k: v for k, v in want.items() if not k.startswith("guard.")}
        same(got, want, "%s at %s, model 2" % (what, sh))
