"""Fixture and yardstick of the LM weight sweep (include/hctr_hip.h, hctr_lm_sweep*), shared by
tests/test_lm_sweep_host.py and tests/test_gpu_lm_sweep.py.

The yardstick is existing test code only: per pair ``lm_beam_ref.make_codec(C, k, arpa, a, b)`` +
``lm_beam_ref.search(..., nbest=1)``, then ``edit_ref.table`` on the 1-best against the line's transcription.

The fixture: C = 12 classes, k = 5, W = 40 columns, B = 4 lines of 40, 33, 17 and 40 columns, an order-3 model over 9 of
the 10 characters (one is OOV), lists from a seed with a weak planted text so that the language model decides between
close hypotheses, line 2 with the blank on top of every column (its greedy text is empty), and a 3 x 2 grid that holds
lm_panelty = 0 and a negative len_bonus. SEED was chosen on the CPU, by the yardstick alone, as the first for which
``properties`` holds: two pairs disagree on some line's text, two pairs disagree on the total distance, and the smallest
nonzero gap between adjacent totals of every pair is at least 100 times the tolerance of the device's float64 sums.
"""
import os

import numpy as np

import edit_ref
import lm_beam_ref as lr
import nbest_ref as nr
from oracle.ctc_ref import ArpaRef

C, K, W, B, BEAM, ORDER, N_CHARS = 12, 5, 40, 4, 10, 3, 9
INPUT_LENGTHS = (40, 33, 17, 40)
EMPTY_LINE = 2
ALPHAS = (0.0, 1.0, 2.5)
BETAS = (-1.5, 3.0)
SEED = 0


def pairs(alphas=ALPHAS, betas=BETAS):
    """alpha-major, as the reference's loops run"""
    return [(float(a), float(b)) for a in alphas for b in betas]


def tol(T, want):
    """tests/test_gpu_nbest_lm.py's bound for logp and score: the device's log1p / exp over T steps"""
    return 1e-14 * T * np.maximum(1.0, np.abs(want))


def write_arpa(work, name="sweep.arpa", order=ORDER, n_chars=N_CHARS, seed=11):
    path = os.path.join(str(work), name)
    if not os.path.exists(path):
        lr.write_arpa(path, order, n_chars, seed=seed)
    return path


def make_lists(seed, W=W, B=B, C=C, k=K, input_lengths=INPUT_LENGTHS, empty_line=EMPTY_LINE, boost=2.2):
    """(idx int32 [W, B, k], lp float32 [W, B, k], input_lengths int32 [B], targets int32 [sum L], target_lengths int32
    [B]): the transcription of a line is its planted text with every fifth character replaced and the last one dropped,
    so no pair reads it exactly; the empty line's is three characters."""
    rng = np.random.RandomState(3000 + seed)
    z = nr.planted_lines(rng, W, B, C, density=0.4, boost=boost)
    if empty_line is not None:
        z[:, empty_line, 0] += np.float32(30.0)
    idx, lp = nr.topk_lists(z, k)
    il = np.asarray(input_lengths, np.int32)
    refs = []
    for b in range(B):
        if b == empty_line:
            refs.append([1, 2, 3])
            continue
        top, text, prev = z[:il[b], b].argmax(axis=1), [], -1
        for c in top:
            if c != 0 and c != C - 1 and c != prev:
                text.append(int(c))
            prev = c
        text = [1 + (c % (C - 2)) if i % 5 == 4 else c for i, c in enumerate(text)][:-1]
        refs.append(text)
    tl = np.array([len(r) for r in refs], np.int32)
    tg = np.array([c for r in refs for c in r], np.int32)
    return idx, lp, il, tg, tl


def yardstick(idx, lp, il, tg, tl, arpa_path, grid, C=C, k=K, beam=BEAM):
    """per pair of ``grid`` the 1-best by lm_beam_ref and its distance by edit_ref: dict of labels int32 [G, B, W],
    hyp_lengths, edits int32 [G, B], logp, score, lm float64 [G, B], empty uint8 [B], gap (the smallest over the pairs)"""
    Wn, Bn, _ = idx.shape
    G = len(grid)
    arpa = ArpaRef(arpa_path)
    off = np.concatenate([[0], np.cumsum(tl)])
    out = dict(labels=np.zeros((G, Bn, Wn), np.int32), hyp_lengths=np.zeros((G, Bn), np.int32),
               edits=np.zeros((G, Bn), np.int32), logp=np.zeros((G, Bn)), score=np.zeros((G, Bn)), lm=np.zeros((G, Bn)),
               empty=np.zeros((Bn,), np.uint8), gap=float("inf"))
    for g, (a, b) in enumerate(grid):
        r = lr.search(lr.make_codec(C, k, arpa, a, b), idx, lp, beam, 1, il)
        out["labels"][g], out["hyp_lengths"][g] = r["labels"][:, 0], r["lengths"][:, 0]
        out["logp"][g], out["score"][g], out["lm"][g] = r["logp"][:, 0], r["score"][:, 0], r["lm"][:, 0]
        out["empty"] = (r["ends"] == 0).astype(np.uint8)
        out["gap"] = min(out["gap"], r["gap"])
        for ln in range(Bn):
            hyp = r["labels"][ln, 0, :r["lengths"][ln, 0]]
            out["edits"][g, ln] = edit_ref.table(tg[off[ln]:off[ln + 1]], hyp)[-1, -1]
    return out


def properties(want):
    """(two pairs differ in some line's text, two pairs differ in total edits)"""
    G = want["labels"].shape[0]
    texts = any((want["labels"][g] != want["labels"][0]).any() for g in range(1, G))
    totals = len(set(want["edits"].astype(np.int64).sum(axis=1).tolist())) > 1
    return texts, totals


def settled(want, T=W):
    fin = np.isfinite(want["score"])
    worst = float(tol(T, np.concatenate([want["logp"][fin], want["score"][fin]])).max())
    return want["gap"] >= 100 * worst


_DONE = {}


def fixture(work):
    """(idx, lp, il, tg, tl, arpa path, grid, yardstick) of the fixture, computed once per scratch directory"""
    key = str(work)
    if key not in _DONE:
        path = write_arpa(work)
        idx, lp, il, tg, tl = make_lists(SEED)
        grid = pairs()
        _DONE[key] = (idx, lp, il, tg, tl, path, grid, yardstick(idx, lp, il, tg, tl, path, grid))
    return _DONE[key]
