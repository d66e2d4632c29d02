"""Shared inputs of tests/test_history_host.py and tests/test_gpu_history.py: does a call on an engine context depend on
the calls that ran on the context before it? Plain numpy builders, so the host and the GPU tests see the same bits.

Probes: one small case per scoring family, each taken from a case module that already has a float64 (or integer) oracle;
this file adds no oracle of its own.
  * tests/masked_cases.py's ``vocab`` (W = 40, B = 5, C = 12, ragged input lengths, an L = 0 line, masked classes): loss,
    gradient, alignment, spotting, lexicon (all scores), its four patterns, recognition, and ``evaluate_logits``;
  * recognition once more on lines of 20 and 6 distinct labels (W = 48, B = 3, C = 30, recognize_ref.planted): the one
    shape here at which the call outgrows the scratch between its two layouts and moves the log-sum-exps it keeps;
  * the set form of a pattern: ``any1`` (the full-vocabulary wildcard ``.``), the smallest case of
    tests/test_gpu_pattern_set.py, on lines planted by that module's ``plant`` - at W = 48 instead of its 160, so that the
    big dirtier below is wider than every probe - against tests/pattern_set_ref.py;
  * ``edit_distance_sequences`` on a ragged batch with an empty hypothesis and an empty reference (tests/edit_ref.py);
  * the "defaults, ragged, OOV" row of tests/test_gpu_nbest_lm.py's CASES (T = 63, B = 3, C = 18): the logits that module's
    ``lists_of`` builds its lists from, for nbest_logits, nbest_topk, nbest_logits(lm=), nbest_skip_logits (zero LM and
    model) and lm_sweep_logits over a 2 x 2 grid, against tests/nbest_ref.py, lm_beam_ref.py, skip_beam_ref.py and
    lm_sweep_ref.py;
  * word-sequence recognition on `vocab` with its lexicon entries (two need the masked class 9), seeded priors and a word
    bonus of -0.5, against tests/words_ref.py: a trie of 27 nodes, the one-node-per-thread LDS instance;
  * `vocab`'s ``union`` and ``live_plus`` patterns as weighted (kind 2) patterns with seeded arc and final weights in
    [-2, 2], against tests/pattern_w_ref.py, and the forward-only (``full=False``, logp alone) instances of the plain and
    the weighted ``union``.

Dirtiers: legal calls that leave hostile bytes in the context's scratch and are larger (``big``), then smaller
(``small``), than every probe in every dimension a scratch layout is carved by. ``big`` holds three non-finite lines
(masked_cases.POISON_KINDS' inputs: one NaN, one +inf, one row of nothing but -inf), whose contract is HCTR_OK. Its words
calls run a lexicon of more than 4096 trie nodes (the scratch form, which sizes step buffers in the block) and then its
small one (the LDS form's records); its ``literal`` and ``union`` patterns run once more with weights, with and without
the Viterbi outputs.
``dims`` states the dimensions; tests/test_history_host.py asserts the ordering numerically.
"""
import functools
import os

import numpy as np

import edit_ref
import lm_beam_ref as lr
import masked_cases as mc
import nbest_ref as nr
import pattern_ref
import pattern_set_ref
import pattern_w_ref
import recognize_ref
import words_ref

NBEST_NAME = "defaults, ragged, OOV"
SWEEP_ALPHAS, SWEEP_BETAS = (0.0, 2.0), (-1.5, 5.8)
PATSET_W, PATSET_LENGTHS = 48, [48, 33, 5, 1]
BIG_W, BIG_B, BIG_C = 160, 8, 64
BIG_BAD = {1: "nan", 4: "posinf", 6: "row_neginf"}         # line -> the kind of its non-finite row (row BAD_T)
BAD_T, BAD_C = 7, 3
WORDS_BONUS, WORDS_PRIOR_SEED = -0.5, 9960
PATW_SEEDS = {"union": 9972, "live_plus": 9973}            # of the probes' arc and final weights, uniform in [-2, 2]
BIG_WORDS_BONUS, BIG_WORDS_NODES = 0.75, (4200, 6000)      # the big dirtier's word bonus; its large trie's nodes lie between
EDIT_SYMBOLS = (0x7FC00000, -1, 2 ** 31 - 1, -2 ** 31)     # a float NaN's bits, all ones, INT32_MAX, INT32_MIN

# the probes in ascending order of the CTC scratch they need: what the `grow` history runs them in. The figures are
# estimates by hand from the "Device scratch" formulas of include/hctr_hip.h at the probes' shapes (bytes, rounded; every
# array is rounded up to 256 bytes, which they ignore); only recognition's are computed (`recognize_needs`)
PROBES = ["edit",                   # 4 * (H + L) per line and the backpointers of five short lines: 3 KB
          "evaluate",               # 2 * 4 * W*B (argmax, labels) + the edit stage: 5 KB
          "loss",                   # 4 * B*W*D emissions (D <= 6) + 8 * B*W: 7 KB
          "spot",                   # emissions of the queries' 8 classes + 16 * B*Q: 7 KB
          "align",                  # emissions + backpointers + 4 * B*W + 12 * sum L: 8 KB
          "pattern.union.fwd",      # forward only: 4 * B*W*D emissions at D = 9 and the class tables, no backpointers: 8 KB
          "pattern_w.union.fwd",
          "recognize",              # 8 * B*W + 40 * B*W: 10 KB
          "grad",                   # the loss's + 4 * sum T (2L + 1) alpha rows: 13 KB
          "recognize_wide",         # 9.3 KB, then 13.8 KB for the text's emissions (`recognize_needs`, exact)
          "pattern.literal",        # 4 * W*D + 2 * W*S per line, S = 11 .. 53, + 20 * B*W: 15 KB .. 34 KB
          "pattern.masked_literal", "pattern.live_plus", "pattern_w.live_plus",
          "words",                  # 4 * B*W*D emissions at D = 9 + 32 * B*W records + 12 * B*W words, starts, labels: 17 KB
          "pattern.union", "pattern_w.union",
          "lexicon",                # emissions + the trie's 2 * 30 states per line and step + B*N scores: 30 KB
          "nbest_topk",             # 8 * T*B*k lists + 8 * T*B*beam history: 30 KB
          "nbest_logits",           # + the rows of the front end, 4 * T*B*C: 45 KB
          "nbest_lm", "skip_zero", "skip_lm",
          "pattern_set",            # 4 * W*D emissions + 2 * W*S backpointers at D = S = 60, four lines: 70 KB
          "lm_sweep"]               # the search's history once per pair, G = 4: 100 KB
LOGITS_PROBES = [p for p in PROBES if p not in ("edit", "nbest_topk")]      # the ones that take on_dev


def _seq_dims(seqs):
    seqs = [list(map(int, s)) for s in seqs]
    return dict(longest=max(len(s) for s in seqs), total=sum(len(s) for s in seqs),
                distinct=len(set(c for s in seqs for c in s)))


def _arc_dims(arcs):
    arcs = np.asarray(arcs).reshape(-1, 3)
    return dict(total=int(arcs.shape[0]), distinct=len(set(arcs[:, 1].tolist())))


def _shape(z):
    W, B, C = z.shape
    return dict(W=W, B=B, C=C)


# ---- the probes ------------------------------------------------------------------------------------------------------
def vocab():
    """(case, oracle) of masked_cases' `vocab`"""
    return mc.get("vocab")


def _ctc():
    """the package's ctc module (host side: building a Lexicon needs no GPU)"""
    import importlib
    from conftest import PKG
    return importlib.import_module(PKG + ".ctc")


@functools.lru_cache(maxsize=None)
def words():
    """the words probe: dict(entries, priors float32, bonus, want) - masked_cases.entries(vocab), seeded priors, and
    words_ref.words' (score, words, starts) per line"""
    c, _ = vocab()
    es = mc.entries(c)
    pr = (np.random.RandomState(WORDS_PRIOR_SEED).randn(len(es)) * 0.5).astype(np.float32)
    return dict(entries=es, priors=pr, bonus=WORDS_BONUS, want=words_ref.words(c["logits"], es, pr, WORDS_BONUS, c["il"]))


def _weights(seed, arcs, finals):
    rng = np.random.RandomState(seed)
    return rng.uniform(-2, 2, len(arcs)).astype(np.float32), rng.uniform(-2, 2, len(finals)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pattern_w():
    """the weighted probes: name -> dict(arcs, finals, states, weights, final_weights, tab, want) - `vocab`'s ``union`` and
    ``live_plus`` automata with seeded float32 weights, pattern_w_ref's tables of them and its (logp, best_logp, path) per
    line"""
    c, _ = vocab()
    out = {}
    for name, seed in PATW_SEEDS.items():
        arcs, finals, ns = mc.patterns(c)[name]
        w, fw = _weights(seed, arcs, finals)
        tab = pattern_w_ref.tables(arcs, finals, ns, w, fw)
        out[name] = dict(arcs=arcs, finals=finals, states=ns, weights=w, final_weights=fw, tab=tab,
                         want=pattern_w_ref.run(c["logits"], tab, c["il"]))
    return out


@functools.lru_cache(maxsize=None)
def patset():
    """the set-form probe: dict(logits [48, 4, 60], il, labels, arcs, sets, finals, num_states, want) - `any1` of
    tests/test_gpu_pattern_set.py (one state, one arc that carries every real label: what ``Pattern.compile(".", codec,
    sets=True)`` builds), its texts and leading blanks, planted by that module's ``plant`` with its seed"""
    import test_gpu_pattern_set as tps
    k = 0
    name, expr, texts, leads = tps.CASES[k]
    assert (name, expr) == ("any1", r".") and tps.C0 == 60
    rng = np.random.RandomState(1800 + k)
    labels = [[1 + tps.CHARS.index(ch) for ch in t] for t in texts]
    z = np.stack([tps.plant(rng, PATSET_W, tps.C0, t, T, lead=n) for t, T, n in zip(labels, PATSET_LENGTHS, leads)], axis=1)
    il = np.array(PATSET_LENGTHS, np.int32)
    arcs, sets, finals, ns = [(0, 0, 1)], [list(range(1, len(tps.CHARS) + 1))], [1], 2
    want = pattern_set_ref.run(z, arcs, sets, finals, ns, input_lengths=il)
    return dict(logits=z, il=il, labels=labels, arcs=arcs, sets=sets, finals=finals, num_states=ns, want=want, C=tps.C0)


WIDE_W, WIDE_C = 48, 30


@functools.lru_cache(maxsize=None)
def recognize_wide():
    """dict(logits [48, 3, 30], texts, want): recognition whose decoded text has 20 distinct classes on one line, planted
    by recognize_ref.planted. The emissions of such a text need more scratch than the row figures and spans did, so the
    second ``ctc_reserve`` of the call grows the block and moves the kept log-sum-exps (`recognize_needs`); the `vocab`
    probe, with at most 7 distinct classes a line, never gets there. Line 2 decodes to nothing."""
    rng = np.random.RandomState(9600)
    texts = [(rng.permutation(20) + 1).tolist(), [3, 3, 7, 21, 22, 28], []]
    z = np.stack([recognize_ref.planted(rng, WIDE_W, WIDE_C, t)[0] for t in texts], axis=1)
    return dict(logits=np.ascontiguousarray(z), texts=texts, want=recognize_ref.recognize_ref(z))


def _align256(n):
    return (int(n) + 255) // 256 * 256


def recognize_needs(labels, lengths, W):
    """(first, second, kept): the bytes csrc/engine.cpp's rec_pass asks ``ctc_reserve`` for - the log-sum-exps, ten
    per-column arrays and two per-line ones; then the log-sum-exps (the `kept` bytes, moved when the block grows), the
    loss's tables, nll and the emissions of the decoded text, D = the most distinct classes of a line, blank included"""
    n = len(lengths)
    col_b, line_b, lse_b = _align256(n * W * 4), _align256(n * 4), _align256(n * W * 8)
    D = max(1 + len(set(int(c) for c in labels[b][:int(lengths[b])])) for b in range(n))
    tab_b = _align256(4 * (4 * n + n * D + int(np.sum(lengths))))
    return lse_b + 10 * col_b + 2 * line_b, lse_b + tab_b + line_b + n * W * D * 4, lse_b


@functools.lru_cache(maxsize=None)
def edit():
    """dict(hyps, refs, hyp [B, stride], n, tg, tl, want): a ragged batch with an empty hypothesis, an empty reference
    and a line that has neither"""
    rng = np.random.RandomState(9700)
    long_ref = rng.randint(1, 9, 40)
    long_hyp = long_ref[:35].copy()
    flip = rng.rand(35) < 0.2
    long_hyp[flip] = rng.randint(1, 9, int(flip.sum()))
    pairs = [([1, 2, 3, 4, 5], [1, 3, 4, 5, 6, 7]), ([], [4, 4]), ([3, 1, 2], []), ([], []), (long_ref.tolist(), long_hyp.tolist())]
    refs, hyps = [p[0] for p in pairs], [p[1] for p in pairs]
    n = np.array([len(h) for h in hyps], np.int32)
    hyp = np.zeros((len(hyps), max(1, int(n.max()))), np.int32)
    for b, h in enumerate(hyps):
        hyp[b, :len(h)] = h
    tl = np.array([len(r) for r in refs], np.int32)
    tg = np.array([c for r in refs for c in r], np.int32)
    return dict(hyps=hyps, refs=refs, hyp=hyp, n=n, tg=tg, tl=tl, want=edit_ref.batch(hyp, n, tg, tl))


@functools.lru_cache(maxsize=None)
def evaluate_want():
    """what evaluate_logits returns on `vocab` with its own targets: the greedy decode (recognize_ref) and edit_ref's
    figures on it"""
    c, _ = vocab()
    g = recognize_ref.recognize_ref(c["logits"])
    labels, lengths = np.asarray(g["labels"], np.int32), np.asarray(g["lengths"], np.int32)
    return dict(labels=labels, lengths=lengths, **edit_ref.batch(labels, lengths, c["targets"], c["tl"]))


@functools.lru_cache(maxsize=None)
def nbest():
    """dict of the N-best probes: spec fields, the logits z [63, 3, 18] tests/test_gpu_nbest_lm.py's ``lists_of`` builds
    for its "defaults, ragged, OOV" row (tests/test_history_host.py holds this copy to that function's lists), il, the
    numpy lists (idx, lp) and, for the sweep, transcriptions made as tests/lm_sweep_ref.py's ``make_lists`` makes them"""
    import test_gpu_nbest_lm as tnl
    _, T, B, C, k, beam, n, order, n_chars, unk, pen, bonus, seed = tnl._spec(NBEST_NAME)
    rng = np.random.RandomState(2000 + seed)
    z = nr.planted_lines(rng, T, B, C, density=0.35, boost=6.0)
    il = np.maximum(1, T - np.arange(B) * max(1, T // 7)).astype(np.int32)
    z[41:, 0, 1:] -= np.float32(20.0)
    z[41:, 0, 0] += np.float32(9.0)
    idx, lp = nr.topk_lists(z, k)
    refs = []
    for b in range(B):
        top, text, prev = z[:il[b], b].argmax(axis=1), [], -1
        for c in top:
            if c != 0 and c != C - 1 and c != prev:
                text.append(int(c))
            prev = c
        refs.append([1 + (c % (C - 2)) if i % 5 == 4 else c for i, c in enumerate(text)][:-1])
    return dict(T=T, B=B, C=C, k=k, beam=beam, n=n, order=order, n_chars=n_chars, unk=unk, pen=pen, bonus=bonus, seed=seed,
                logits=z, il=il, idx=idx, lp=lp, tl=np.array([len(r) for r in refs], np.int32),
                tg=np.array([c for r in refs for c in r], np.int32),
                grid=[(float(a), float(b)) for a in SWEEP_ALPHAS for b in SWEEP_BETAS])


def arpa(work):
    """the probe's n-gram model, written once into the scratch directory `work`"""
    nb = nbest()
    path = os.path.join(str(work), "history_case%d.arpa" % nb["seed"])
    if not os.path.exists(path):
        lr.write_arpa(path, nb["order"], nb["n_chars"], seed=nb["seed"], unk=nb["unk"])
    return path


def chars(C):
    return ["<blank>"] + list(lr.chars_of(C)) + ["<unknown>"]


@functools.lru_cache(maxsize=None)
def probe_dims():
    """name -> the dimensions the probe's scratch is carved by (only those that apply to it)"""
    c, o = vocab()
    v = _shape(c["logits"])
    ps, ed, nb = patset(), edit(), nbest()
    pats = mc.patterns(c)
    out = {}
    for name in ("loss", "grad", "align", "evaluate"):
        out[name] = dict(v, **_seq_dims(c["lines"]))
    out["recognize"] = dict(v)
    out["recognize_wide"] = dict(_shape(recognize_wide()["logits"]), **_seq_dims(recognize_wide()["texts"][:2]))
    out["spot"] = dict(v, count=len(o["queries"]), **_seq_dims(o["queries"]))
    out["lexicon"] = dict(v, count=len(o["entries"]), **_seq_dims(o["entries"]))
    for pname, (arcs, finals, ns) in pats.items():
        out["pattern." + pname] = dict(v, states=int(ns), **_arc_dims(arcs))
    for name in ("pattern_w.union", "pattern_w.live_plus", "pattern.union.fwd", "pattern_w.union.fwd"):
        out[name] = dict(out["pattern." + name.split(".")[1]])
    wd = words()
    lex = _ctc().Lexicon(wd["entries"], num_classes=mc.C, priors=wd["priors"])
    out["words"] = dict(v, count=len(wd["entries"]), nodes=int(lex.info()["nodes"]), **_seq_dims(wd["entries"]))
    out["pattern_set"] = dict(_shape(ps["logits"]), states=ps["num_states"],
                              **_arc_dims(pattern_set_ref.expand(ps["arcs"], ps["sets"])))
    out["edit"] = dict(B=len(ed["refs"]), stride=int(ed["hyp"].shape[1]), **_seq_dims(ed["refs"]))
    search = dict(_shape(nb["logits"]), beam=nb["beam"], depth=nb["k"], n=nb["n"])
    for name in ("nbest_logits", "nbest_topk", "nbest_lm"):
        out[name] = dict(search)
    for name in ("skip_zero", "skip_lm"):
        out[name] = dict(_shape(nb["logits"]), beam=nb["beam"], n=nb["n"])
    out["lm_sweep"] = dict(_shape(nb["logits"]), beam=nb["beam"], depth=nb["k"], longest=int(nb["tl"].max()),
                           total=int(nb["tl"].sum()))
    assert sorted(out) == sorted(PROBES)
    return out


# ---- the dirtiers ----------------------------------------------------------------------------------------------------
def _edit_batch(pairs):
    return [p[1] for p in pairs], [p[0] for p in pairs]


@functools.lru_cache(maxsize=None)
def big():
    """dict: logits [160, 8, 64] with the three bad lines, clean (the same without them), il, lines / targets / tl,
    queries, entries, patterns name -> (arcs, finals, states), pattern_weights name -> (arc weights, final weights),
    set_pattern (arcs, sets, finals, states), edit (hyps, refs), search dict(n, beam, depth), words_entries (random
    entries of 1 - 4 of the 63 live labels, as tests/test_gpu_words.py's ``grown`` makes them, whose trie has more than
    4096 nodes: the scratch form) and words_bonus. Texts as masked_cases.ladder() makes its L = 70 line, over 63 live labels; line 0
    holds every one of them"""
    rng = np.random.RandomState(9800)
    live = list(range(1, BIG_C))
    lens = (70, 5, 40, 70, 12, 0, 33, 64)
    il = [160, 153, 160, 160, 120, 160, 110, 160]
    lines = []
    for b, L in enumerate(lens):
        t = (rng.permutation(BIG_C - 1) + 1).tolist() if b == 0 else []
        while len(t) < L:
            t.append(t[-1] if t and rng.rand() < 0.2 else int(rng.choice(live)))
        lines.append(t[:L])
    paths = [mc.planted_path(t, T, run=1 if len(t) > 40 else 2) for t, T in zip(lines, il)]
    clean = np.stack([mc.plant(rng, BIG_W, T, p, classes=BIG_C) for p, T in zip(paths, il)], axis=1)
    z = clean.copy()
    for b, kind in BIG_BAD.items():
        assert BAD_T < il[b]
        if kind == "nan":
            z[BAD_T, b, BAD_C] = np.nan
        elif kind == "posinf":
            z[BAD_T, b, BAD_C] = np.inf
        else:
            z[BAD_T, b, :] = -np.inf
    case = mc._case("history_big", lines, il, paths, z)
    texts = [t for t in lines if t]
    queries = [list(range(1, 33)), list(range(32, 64)), lines[0][:32], lines[3][10:42], lines[2][:20], [5], lines[7][:32],
               [63, 1], lines[0][38:70]]
    entries = [list(range(1, 64))]
    for t in texts:
        for e in (t[:64], t[:33], t[:6], t[:1], t[:5] + [t[-1] % 63 + 1], t[-9:]):
            if e and e not in entries:
                entries.append(list(e))
    every = list(range(1, BIG_C))
    syms = np.array(EDIT_SYMBOLS, np.int64)
    ref = syms[rng.randint(0, 4, 300)]

    def noisy(H):
        h = np.concatenate([ref[:H], syms[rng.randint(0, 4, max(0, H - 300))]])
        flip = rng.rand(H) < 0.25
        h[flip] = syms[rng.randint(0, 4, int(flip.sum()))]
        return h.tolist()

    pairs = [(ref.tolist(), noisy(280)), (ref.tolist(), noisy(310)), ([], noisy(5)), (ref[:7].tolist(), []),
             (ref[:150].tolist(), noisy(150)), (ref.tolist(), noisy(300))]
    hyps, refs = _edit_batch(pairs)
    patterns = {"literal": pattern_ref.literal(lines[0]), "union": pattern_ref.trie(entries)}
    wrng, words_entries = np.random.RandomState(9801), []
    while len(words_ref.build_trie(words_entries or [[1]])[0]) < BIG_WORDS_NODES[0]:
        words_entries += [[int(v) for v in wrng.randint(1, BIG_C, size=wrng.randint(1, 5))] for _ in range(200)]
    case.update(clean=clean, queries=queries, entries=entries, patterns=patterns,
                pattern_weights={k: _weights(9810 + i, p[0], p[1]) for i, (k, p) in enumerate(patterns.items())},
                set_pattern=([(0, 0, 1), (1, 0, 1)], [every], [1], 2), edit=(hyps, refs), search=dict(n=32, beam=32, depth=32),
                words_entries=words_entries, words_bonus=BIG_WORDS_BONUS)
    return case


@functools.lru_cache(maxsize=None)
def small():
    """the same families at B = 1, W = 2, C = 3, masked_cases.single(5)'s way: row 0 keeps one live class. `clean` is the
    same without the mask. One query, one entry (the lexicon of its words call too: a trie of two nodes), one-state
    patterns that loop on label 1, once more with a weight."""
    rng = np.random.RandomState(9900)
    lines, il = [[1]], [2]
    paths = [mc.planted_path(lines[0], 2, lead=0, run=1)]
    clean = np.stack([mc.plant(rng, 2, 2, paths[0], classes=3)], axis=1)
    z = clean.copy()
    z[0, 0, :1] = -np.inf
    z[0, 0, 2:] = -np.inf
    case = mc._case("history_small", lines, il, paths, z)
    case.update(clean=clean, queries=[[1]], entries=[[1]], patterns={"loop": ([(0, 1, 0)], [0], 1)},
                pattern_weights={"loop": (np.array([-1.5], np.float32), np.array([0.5], np.float32))},
                set_pattern=([(0, 0, 0)], [[1]], [0], 1), edit=([[1]], [[2]]), search=dict(n=1, beam=2, depth=2),
                words_entries=None, words_bonus=0.25)
    return case


def dirtier_dims(d, worst):
    """every dimension of a dirtier's calls, the largest (worst = max, the big dirtier) or smallest (min) over them"""
    hyps, refs = d["edit"]
    lexica = [d["entries"]] + ([d["words_entries"]] if d["words_entries"] else [])      # of the words calls
    seqs = [d["lines"], d["queries"], refs] + lexica
    arcs = [a for a, _, _ in d["patterns"].values()] + [pattern_set_ref.expand(d["set_pattern"][0], d["set_pattern"][1])]
    states = [ns for _, _, ns in d["patterns"].values()] + [d["set_pattern"][3]]
    out = dict(_shape(d["logits"]))
    for key in ("longest", "total", "distinct"):
        out[key] = worst([_seq_dims([s for s in ss if len(s)] or [[]])[key] for ss in seqs])
    out["total"] = worst([out["total"]] + [_arc_dims(a)["total"] for a in arcs])
    out["distinct"] = worst([out["distinct"]] + [_arc_dims(a)["distinct"] for a in arcs])
    out["count"] = worst([len(d["queries"])] + [len(es) for es in lexica])
    out["nodes"] = worst([len(words_ref.build_trie(es)[0]) for es in lexica])
    out["states"] = worst(states)
    out["B"] = worst([out["B"], len(refs)])
    out["stride"] = max(len(h) for h in hyps)
    out.update(d["search"])
    return out
