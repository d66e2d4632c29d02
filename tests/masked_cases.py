"""Shared inputs of tests/test_masked_host.py and tests/test_gpu_masked.py: logits in which classes are masked out with
-inf (the usual way to restrict a CTC model: digits only, one script only, no blank inside a forced region) and logits
with a non-finite row (a NaN, a +inf, nothing but -inf), for every ``*_logits`` entry point of the CTC family. Plain
numpy builders, so the host and the GPU tests see the same bits, and the float64 oracles of each case, computed once.

Logits are unit-normal noise times 3 plus a boost of 8 on a planted alignment, float32, C = 12 classes (0 = blank),
W = 40 columns unless a case says otherwise, with mixed input lengths.
"""
import functools

import numpy as np

import ctc_align_ref as align_ref
import lexicon_ref
import pattern_ref
import recognize_ref
import spot_ref

C, W = 12, 40
NOISE, BOOST = 3.0, 8.0
LIVE = list(range(1, 8))                           # the labels the `vocab` mask leaves; 8..11 are masked
POISON_T, POISON_C, POISON_LATE = 7, 3, 35         # the bad row of the `poison` cases; the row past line 1's length


def planted_path(text, T, lead=2, run=None):
    """the class per column of: `lead` blanks, then per label a run of `run` columns (an int, or one per label; two
    where they fit by default) and one blank, blanks to T"""
    L = len(text)
    if run is None:
        run = max(1, min(2, (T - lead) // max(L, 1) - 1))
    runs = [run] * L if np.isscalar(run) else list(run)
    path = [0] * lead + [c for ch, n in zip(text, runs) for c in [int(ch)] * n + [0]]
    assert len(path) <= T + 1, "the planted path does not fit"
    path = (path + [0] * T)[:T]
    assert align_ref.collapse(path).tolist() == [int(c) for c in text]
    return path


def plant(rng, Wc, T, path, classes=C):
    """[Wc][classes] float32: noise in every column, the boost on path[t] for t < T"""
    z = NOISE * rng.standard_normal((Wc, classes))
    z[np.arange(T), np.asarray(path[:T])] += BOOST
    return z.astype(np.float32)


def _case(name, lines, il, paths, logits, **more):
    """lines: the targets, a list of label lists; paths: the planted class per column of every line"""
    logits = np.ascontiguousarray(logits, np.float32)
    out = dict(name=name, logits=logits, il=np.asarray(il, np.int32), lines=[list(map(int, t)) for t in lines],
               paths=paths, targets=np.array([c for t in lines for c in t], np.int32),
               tl=np.array([len(t) for t in lines], np.int32), mask=np.isneginf(logits), no_path=[])
    out.update(more)
    return out


def _build(name, seed, lines, il, Wc=W, lead=2, run=None, runs=None):
    rng = np.random.RandomState(seed)
    paths = [planted_path(t, int(T), lead, run if runs is None else runs[b]) for b, (t, T) in enumerate(zip(lines, il))]
    logits = np.stack([plant(rng, Wc, int(T), p) for p, T in zip(paths, il)], axis=1)
    return _case(name, lines, il, paths, logits)


def vocab():
    """classes 8..11 masked in every column; a repeat, an L = 0 line, and a fifth line whose target holds class 9"""
    c = _build("vocab", 9100, [[1, 2, 3, 4, 5], [3, 3, 6, 7], [], [7, 1, 2], [2, 9, 4]], [W, W - 7, W, W - 14, W])
    c["logits"][:, :, 8:] = -np.inf
    c["mask"] = np.isneginf(c["logits"])
    c["no_path"] = [4]
    return c


def columns():
    """a target class masked on the first 6 of the 8 columns its planted run had (the other labels' runs have 2), the
    blank masked on column 1: every line keeps an alignment, and its best path has to move. The texts are near misses
    of each other, so that a line's text is not hopeless on the other lines."""
    lines, at = [[1, 2, 3, 4], [1, 2, 3], [1, 2, 7, 4]], [1, 0, 3]      # `at`: the masked target position of each line
    runs = [[8 if j == k else 2 for j in range(len(t))] for t, k in zip(lines, at)]
    c = _build("columns", 9200, lines, [W, W - 7, W], runs=runs)
    for b, j in enumerate(at):
        start = 2 + 3 * j
        assert c["paths"][b][start:start + 8] == [c["lines"][b][j]] * 8
        c["logits"][start:start + 6, b, c["lines"][b][j]] = -np.inf
        assert c["paths"][b][1] == 0
        c["logits"][1, b, 0] = -np.inf
    c["mask"] = np.isneginf(c["logits"])
    return c


def single(Wc=W):
    """rows that keep one live class only (its log-probability is 0 exactly), on cells of the planted path: the best
    path goes through them, and the runner-up of such a row is a -inf class. Five rows per line at W = 40, two at 5."""
    if Wc >= 40:
        c = _build("single", 9300, [[1, 2, 3], [4, 4, 5]], [Wc, Wc - 7], Wc=Wc, run=5)
        rows = [[2, 5, 7, 10, 39], [3, 7, 8, 12, 30]]         # label and blank cells; (1, 7) is the blank between the 4s
    else:
        c = _build("single%d" % Wc, 9300 + Wc, [[1, 2], [4, 4]], [Wc, Wc], Wc=Wc, lead=0, run=1)
        rows = [[0, 2], [1, 2]]
    for b, ts in enumerate(rows):
        for t in ts:
            keep = c["paths"][b][t]
            c["logits"][t, b, :keep] = -np.inf
            c["logits"][t, b, keep + 1:] = -np.inf
    c["mask"] = np.isneginf(c["logits"])
    c["single_rows"] = rows
    return c


def infeasible(Wc=W):
    """L + repeats <= T for every line, yet: line 0 ([1, 1], the blank masked on every interior column) and line 1
    ([2, 3], class 3 masked everywhere) have no path; line 2 is an ordinary line"""
    il = [12, Wc - 7, Wc] if Wc >= 40 else [Wc] * 3        # (line 0 short: all its interior columns must be labels)
    c = _build("infeasible%d" % Wc, 9400 + Wc, [[1, 1], [2, 3], [4, 5]], il, Wc=Wc, lead=0 if Wc < 40 else 2,
               run=None if Wc >= 40 else 1)
    c["logits"][1:il[0] - 1, 0, 0] = -np.inf
    c["logits"][:, 1, 3] = -np.inf
    c["mask"] = np.isneginf(c["logits"])
    c["no_path"] = [0, 1]
    return c


def ladder():
    """the vocab mask at L = 5, 40, 70 (S = 11, 81, 141) over W = 160: the one-state-per-lane instance, the two-state
    one, and the two-wave one, where a -inf crosses the wave boundary through LDS"""
    rng = np.random.RandomState(9500)
    lines = []
    for L in (5, 40, 70):
        t = []
        for _ in range(L):
            t.append(t[-1] if t and rng.rand() < 0.2 else int(rng.choice(LIVE)))
        lines.append(t)
    il = [160, 153, 160]
    paths = []
    for t, T in zip(lines, il):                               # a blank after every label, so repeats are parted
        paths.append(planted_path(t, T, run=1 if len(t) > 40 else 2))
    logits = np.stack([plant(rng, 160, T, p) for p, T in zip(paths, il)], axis=1)
    logits[:, :, 8:] = -np.inf
    return _case("ladder", lines, il, paths, logits)


POISON_KINDS = ("nan", "posinf", "row_neginf", "late_nan", "late_posinf", "late_row_neginf")


def poison(kind):
    """the first three lines of `vocab` with line 1 (T = 33) given one NaN at (7, 3), one +inf there, or a row 7 of
    nothing but -inf; `late_*`: the same at row 35 >= T, which no entry point may read"""
    v = vocab()
    z = np.ascontiguousarray(v["logits"][:, :3])
    t = POISON_LATE if kind.startswith("late_") else POISON_T
    what = kind.replace("late_", "")
    if what == "nan":
        z[t, 1, POISON_C] = np.nan
    elif what == "posinf":
        z[t, 1, POISON_C] = np.inf
    else:
        assert what == "row_neginf"
        z[t, 1, :] = -np.inf
    c = _case("poison_" + kind, v["lines"][:3], v["il"][:3], v["paths"][:3], z)
    c["bad_t"] = t
    return c


def clean_of_poison():
    v = vocab()
    return _case("poison_clean", v["lines"][:3], v["il"][:3], v["paths"][:3], v["logits"][:, :3])


# ---- what is asked of a case besides its own targets ----
def queries(case):
    """spotting queries of 2 to 4 labels: parts of the planted texts, a near miss, one that needs class 9"""
    texts = [t for t in case["lines"] if len(t) >= 2]
    a, b = texts[0], texts[-1]
    miss = [a[0], a[1] % 7 + 1] if a[1] % 7 + 1 != a[0] else [a[0], (a[1] + 1) % 7 + 1]
    return [a[:2], a[-4:], b[:3], miss, [a[0], 9]]


def entries(case):
    """about a dozen lexicon entries that share prefixes: the planted texts, their prefixes, near misses, one with a
    masked class"""
    out = []
    for t in case["lines"]:
        if not t:
            continue
        if len(t) > 6:                                        # (the ladder's long targets: their heads)
            t = t[:6]
        for e in (t, t[:-1], t[:1], t + [t[-1] % 7 + 1], t[:-1] + [t[-1] % 7 + 1]):
            if e and e not in out:
                out.append(list(e))
    for e in ([2, 9], [9], [1, 2, 9, 4]):
        if e not in out:
            out.append(e)
    return out


def patterns(case):
    """name -> (arcs, finals, states): a literal, a literal through a masked class, a union of literals, and one or more
    of the live labels (the `\\d+` of a vocabulary whose digits are 1..7)"""
    text = [t for t in case["lines"] if t][0]
    plus = [(0, c, 1) for c in LIVE] + [(1, c, 1) for c in LIVE]
    return {"literal": pattern_ref.literal(text), "masked_literal": pattern_ref.literal([text[0], 9, text[-1]]),
            "union": pattern_ref.trie(entries(case)), "live_plus": (plus, [1], 2)}


# ---- float64 oracles, once per case ----
def nll64(case):
    out = []
    for b, t in enumerate(case["lines"]):
        T = int(case["il"][b])
        out.append(recognize_ref.ctc_nll64(align_ref.log_softmax64(case["logits"][:T, b]), t))
    return np.array(out)


def torch_nll64(case):
    import torch
    lp = torch.from_numpy(align_ref.log_softmax64(case["logits"]))
    return torch.nn.functional.ctc_loss(lp, torch.from_numpy(case["targets"].astype(np.int64)),
                                        torch.from_numpy(case["il"].astype(np.int64)),
                                        torch.from_numpy(case["tl"].astype(np.int64)), reduction="none").numpy()


def torch_grads(case):
    """(g64, g32): torch's CPU gradient of sum_b nll_b with the LOG-PROBS as the leaf (float64, and the same
    log-probs rounded to float32), zero_infinity on. It is exp(lp) - gamma, the engine's definition, wherever lp is
    finite; torch leaves NaN at the masked entries of a line that has an alignment."""
    import torch
    out = []
    for dt in (torch.float64, torch.float32):
        lp = torch.from_numpy(align_ref.log_softmax64(case["logits"])).to(dt).requires_grad_()
        nll = torch.nn.functional.ctc_loss(lp, torch.from_numpy(case["targets"].astype(np.int64)),
                                           torch.from_numpy(case["il"].astype(np.int64)),
                                           torch.from_numpy(case["tl"].astype(np.int64)), reduction="none",
                                           zero_infinity=True)
        nll.sum().backward()
        out.append(lp.grad.numpy().astype(np.float64))
    return out[0], out[1]


def viterbi64(case):
    return [align_ref.viterbi(case["logits"][:int(case["il"][b]), b], t) for b, t in enumerate(case["lines"])]


def oracle(case):
    """dict: nll [B]; align (ctc_align_ref.viterbi per line); spot (contain, seg, starts, ends [B][Q]); lex [B][N];
    pat name -> per line (logp, best_logp, path or None). The `ladder` has the first two only."""
    out = dict(nll=nll64(case), align=viterbi64(case))
    if case["name"] == "ladder":                              # loss, gradient and alignment only: a short text is hopeless
        return out                                            # on a line of 70 planted labels
    q, es = queries(case), entries(case)
    out.update(queries=q, entries=es, spot=spot_ref.spot(case["logits"], q, case["il"]),
               lex=lexicon_ref.scores(case["logits"], es, case["il"]), pat={})
    for name, d in patterns(case).items():
        out["pat"][name] = pattern_ref.run(case["logits"], *d, input_lengths=case["il"])
    return out


CASES = {"vocab": vocab, "columns": columns, "single": single, "infeasible": infeasible, "ladder": ladder}


@functools.lru_cache(maxsize=None)
def get(name):
    """(case, oracle) of a named case, built once per process; treat both as read-only"""
    if name in CASES:
        c = CASES[name]()
    elif name == "single5":
        c = single(5)
    elif name == "infeasible5":
        c = infeasible(5)
    elif name == "poison_clean":
        c = clean_of_poison()
    else:
        c = poison(name[len("poison_"):])
    return c, (oracle(c) if not name.startswith("poison_") or name == "poison_clean" else None)


def flat_paths(T, classes=C):
    """every path of classes^T as an int array [classes^T][T] (tiny T only)"""
    return np.stack(np.meshgrid(*[np.arange(classes)] * T, indexing="ij"), axis=-1).reshape(-1, T)


def collapse_all(paths):
    """the collapse of every row of `paths`, left-justified and zero-padded, [N][T]"""
    prev = np.concatenate([np.zeros((len(paths), 1), paths.dtype), paths[:, :-1]], axis=1)
    keep = (paths != 0) & (paths != prev)
    pos = np.cumsum(keep, axis=1) - 1
    out = np.zeros_like(paths)
    r, c = np.nonzero(keep)
    out[r, pos[r, c]] = paths[r, c]
    return out
