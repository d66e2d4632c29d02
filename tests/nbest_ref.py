"""Float64 restatement of the device prefix beam search (include/hctr_hip.h, hctr_nbest*), the yardstick of
tests/test_gpu_nbest.py and tests/test_nbest_host.py.

It invents nothing: every step is ``oracle.ctc_ref.CtcCodecRef.step`` - the restatement of the reference's
__context_beam_search__ that the goldens pin - with ``ngram = ZeroLM()``, ``use_tfm_pred = False`` and no suffix, fed
``{class: float32 log-prob}`` rows the way ``beam_full_from_topk`` feeds it. What differs from ``beam_full_from_topk`` is
only what the contract says: the caller chooses the number of steps, there is no greedy end step and no empty-line
rule, and the first ``nbest`` hypotheses of the final list are returned with pb, pnb and totals instead of one string.
Labels stand for themselves: class c is the character chr(BASE + c), so prefixes map back to label lists exactly.
"""
import numpy as np

from oracle.ctc_ref import CtcCodecRef, Hyp, ZeroLM

BASE = 0x4E00
NEG_INF = float("-inf")


def make_codec(C, k, len_bonus):
    codec = CtcCodecRef("".join(chr(BASE + c) for c in range(1, C - 1)))
    assert len(codec.characters) == C
    codec.ngram = ZeroLM()
    codec.use_tfm_pred = False
    codec.use_tfm_score = False
    codec.search_depth = k
    codec.len_bonus = len_bonus
    codec.beam_size = 1 << 30                    # step() returns the whole sorted list; search_line cuts it
    return codec


def search_line(idx, lp, C, beam, nbest, len_bonus=0.0, steps=None):
    """One line. idx int [T, k], lp float32 [T, k]: the row lists. Returns (hyps, gap): hyps = the first ``nbest``
    hypotheses of the final list as dicts (labels, pb, pnb, logp, score); gap = the smallest nonzero finite gap between
    adjacent totals among the first ``beam + 1`` sorted entries over all steps (inf if there is none)."""
    idx, lp = np.asarray(idx), np.asarray(lp, np.float32)
    T = idx.shape[0] if steps is None else int(steps)
    codec = make_codec(C, idx.shape[1], len_bonus)
    beams, gap = [Hyp()], float("inf")
    with np.errstate(invalid="ignore"):
        for t in range(T):
            row = {int(c): np.float32(v) for c, v in zip(idx[t], lp[t])}
            full = codec.step(beams, idx[t], row, "") if beams else []
            tot = np.array([float(h.total()) for h in full[:beam + 1]], np.float64)
            d = tot[:-1] - tot[1:]
            d = d[np.isfinite(d) & (d != 0)]
            if d.size:
                gap = min(gap, float(d.min()))
            beams = full[:beam]
    out = []
    for h in beams[:nbest]:
        out.append(dict(labels=[ord(ch) - BASE for ch in h.prefix], pb=float(h.pb), pnb=float(h.pnb),
                        logp=float(h.prob()), score=float(h.total())))
    return out, gap


def search(idx, lp, C, beam, nbest, len_bonus=0.0, input_lengths=None):
    """A batch. idx / lp [W, B, k]. Returns (labels int32 [B, nbest, W], lengths int32 [B, nbest], logp, score float64
    [B, nbest], count int32 [B], gap) with the contract's fill of unused slots, and the per-hypothesis (pb, pnb) list."""
    idx, lp = np.asarray(idx), np.asarray(lp, np.float32)
    W, B, _ = idx.shape
    labels = np.zeros((B, nbest, W), np.int32)
    lengths = np.zeros((B, nbest), np.int32)
    logp = np.full((B, nbest), -np.inf)
    score = np.full((B, nbest), -np.inf)
    count = np.zeros((B,), np.int32)
    gap, parts = float("inf"), []
    for b in range(B):
        T = W if input_lengths is None else int(input_lengths[b])
        hyps, g = search_line(idx[:, b], lp[:, b], C, beam, nbest, len_bonus, T)
        gap = min(gap, g)
        count[b] = len(hyps)
        parts.append([(h["pb"], h["pnb"]) for h in hyps])
        for i, h in enumerate(hyps):
            n = len(h["labels"])
            labels[b, i, :n] = h["labels"]
            lengths[b, i] = n
            logp[b, i], score[b, i] = h["logp"], h["score"]
    return labels, lengths, logp, score, count, gap, parts


def topk_lists(logits, k):
    """The front end's lists of float32 logits [W, B, C] as float64 numpy gives them: classes by (log-prob descending,
    index ascending), log-probs rounded to float32. (The engine's own lists come from hctr_beam_frontend.)"""
    z = np.asarray(logits, np.float64)
    mx = z.max(axis=2, keepdims=True)
    lp = (z - (mx + np.log(np.exp(z - mx).sum(axis=2, keepdims=True)))).astype(np.float32)
    order = np.lexsort((np.broadcast_to(np.arange(z.shape[2]), z.shape), -lp.astype(np.float64)), axis=2)[:, :, :k]
    return order.astype(np.int32), np.take_along_axis(lp, order, axis=2)


def planted_lines(rng, W, B, C, density=0.3, boost=9.0):
    """[W, B, C] float32: N(0, 1) noise with ``boost`` on a planted class per column, blank with probability
    1 - density, never C-1: lines whose greedy text is the planted one."""
    z = rng.standard_normal((W, B, C)).astype(np.float32)
    cls = np.where(rng.rand(W, B) < density, rng.randint(1, C - 1, (W, B)), 0)
    for b in range(B):
        z[np.arange(W), b, cls[:, b]] += np.float32(boost)
    return z
