"""Float64 restatement of the device skip search (include/hctr_hip.h, hctr_nbest_skip*), the yardstick of
tests/test_gpu_nbest_skip.py and tests/test_skip_beam_host.py.

Like tests/lm_beam_ref.py it invents nothing: a ranked step is ``oracle.ctc_ref.CtcCodecRef.step`` with ``ngram =
ArpaRef(path)`` or ``ZeroLM()``, the greedy line, the suffixes and the end step are the codec's own ``_top_line / _suffix /
_end_step``, and an in-place step is the loop of ``oracle/ctc_ref.py:beam_skip``, fed the float32 candidate rows of the
front end (CSR lists in class-ascending order, the blank log-prob beside them). It does NOT fold equal texts: it goes the
reference's own way, in which the dict of the next ranked step sums them. What it adds is what the contract returns - the
first ``nbest`` hypotheses of the final list as the list stands, ``status`` and ``ranked`` - and what the tests need to
know about a line: the smallest nonzero gap between adjacent totals of its ranked steps, how many ranked steps started
from a list that held a text twice, and which of the four in-place branches were taken.
"""
import numpy as np

from oracle.ctc_ref import NEG_INF, CtcCodecRef, Hyp, ZeroLM

import lm_beam_ref as lr

BASE = lr.BASE
CAP = 32                                            # candidates of a ranked step the device search holds
THRESH = np.log(0.001)                              # utils/ctc_codec.py:128
OK, EMPTY_GREEDY, EMPTIED, OVERFLOW = 0, 1, 2, 3


def make_codec(C, arpa_path, lm_panelty, len_bonus, memo=True):
    """the codec of a search over C classes: ``arpa_path`` None is the zero LM (the reference's skip_zero setting)"""
    if arpa_path is not None:
        return lr.make_codec(C, CAP, arpa_path, lm_panelty, len_bonus, memo=memo)
    codec = CtcCodecRef(lr.chars_of(C))
    codec.ngram = ZeroLM()
    codec.use_tfm_pred = codec.use_tfm_score = False
    codec.lm_panelty, codec.len_bonus = lm_panelty, len_bonus
    codec.beam_size = 1 << 30
    return codec


def lists_of_logp(logp):
    """The front end's lists of float32 log-probs [W, B, C]: (top1 int32 [W, B], blank float32 [W, B], cand_off int64
    [W*B + 1], cand_idx int32, cand_logp float32), rows r = t*B + b, candidates = np.where(row > ln 0.001)"""
    logp = np.asarray(logp, np.float32)
    W, B, _ = logp.shape
    top1 = logp.argmax(axis=2).astype(np.int32)
    blank = np.ascontiguousarray(logp[:, :, 0])
    off, ci, cl = [0], [], []
    for t in range(W):
        for b in range(B):
            c = np.where(logp[t, b].astype(np.float64) > THRESH)[0]
            ci.append(c.astype(np.int32))
            cl.append(logp[t, b, c])
            off.append(off[-1] + c.size)
    return (top1, blank, np.asarray(off, np.int64), np.concatenate(ci).astype(np.int32) if ci else np.zeros(0, np.int32),
            np.concatenate(cl).astype(np.float32) if cl else np.zeros(0, np.float32))


def inplace_step(codec, beams, c, l, l0, taken=None):
    """oracle/ctc_ref.py:beam_skip's in-place update (utils/ctc_codec.py:147-171) by the single candidate c with
    log-prob l; l0 is the row's blank log-prob. ``taken`` collects the branches (1-4) hypotheses went through."""
    unk = len(codec.characters) - 1
    if c >= unk:
        return
    for h in beams:
        tail = None if h.prefix == "" else codec.dict[h.prefix[-1]]
        if c == 0:
            branch = 1
            h.pb = h.prob() + l
        elif c != tail:
            branch = 2
            h.prefix += codec.characters[c]
            h.pnb = h.prob() + l
            h.pb = NEG_INF
        elif h.pb != NEG_INF:
            branch = 3
            h.prefix += codec.characters[c]
            h.pnb = h.pb + l
            h.pb = NEG_INF
        else:
            branch = 4
            h.pb = h.prob() + l0
            h.pnb = h.pnb + l
        if taken is not None:
            taken.add((branch, len(beams) > 1))


def search_line(codec, top1, blank, rows, beam, nbest, L=None, cap=CAP):
    """One line over its first L columns. top1 int [T], blank float32 [T], rows: per step (classes ascending, float32
    log-probs). Returns a dict: hyps (the first ``nbest`` of the final list as dicts of labels, pb, pnb, logp, lm, score),
    status, ranked, end, gap, dup_steps, branches. ``cap`` None searches rows of any size, as the reference does."""
    T = len(rows)
    L = T if L is None else int(L)
    out = dict(hyps=[], status=OK, ranked=0, end=0, gap=float("inf"), dup_steps=0, branches=set())
    top_line = codec._top_line(np.asarray(top1)[:L])
    if not top_line:
        out["status"] = EMPTY_GREEDY
        return out
    end = out["end"] = codec._end_step(top_line, L)
    sizes = [len(rows[t][0]) for t in range(end)]
    out["ranked"] = sum(1 for m in sizes if m != 1)
    if cap is not None and any(m > cap for m in sizes):
        out["status"] = OVERFLOW
        return out
    beams = [Hyp()]
    with np.errstate(invalid="ignore"):
        for t in range(end):
            cls, lps = rows[t]
            if len(cls) == 1:
                inplace_step(codec, beams, int(cls[0]), np.float32(lps[0]), np.float32(blank[t]), out["branches"])
                continue
            texts = [h.prefix for h in beams]
            out["dup_steps"] += len(set(texts)) < len(texts)
            row = {int(c): np.float32(v) for c, v in zip(cls, lps)}
            full = codec.step(beams, [int(c) for c in cls], row, codec._suffix(top_line, t)) if beams else []
            tot = np.array([float(h.total()) for h in full[:beam + 1]], np.float64)
            d = tot[:-1] - tot[1:]
            d = d[np.isfinite(d) & (d != 0)]
            if d.size:
                out["gap"] = min(out["gap"], float(d.min()))
            beams = full[:beam]
    if not beams:
        out["status"] = EMPTIED
        return out
    for h in beams[:nbest]:
        logp, lm, n = float(h.prob()), float(codec._ngram_score(h.prefix, "")), len(h.prefix)
        score = logp + (lm * codec.lm_panelty + n * codec.len_bonus)
        out["hyps"].append(dict(labels=[ord(ch) - BASE for ch in h.prefix], pb=float(h.pb), pnb=float(h.pnb), logp=logp,
                                lm=lm, score=float(score)))
    return out


def search(codec, top1, blank, cand_off, cand_idx, cand_logp, beam, nbest, input_lengths=None, cap=CAP):
    """A batch of CSR lists (rows r = t*B + b). Returns a dict: labels int32 [B, nbest, W], lengths int32 [B, nbest],
    logp / score / lm float64 [B, nbest], count / status / ranked / ends / dup_steps int32 [B] with the contract's fill
    of unused slots, gap (over all lines), gaps [B], branches (the union) and pb / pnb float64 [B, nbest]."""
    top1, blank = np.asarray(top1), np.asarray(blank, np.float32)
    W, B = top1.shape
    r = dict(labels=np.zeros((B, nbest, W), np.int32), lengths=np.zeros((B, nbest), np.int32),
             logp=np.full((B, nbest), -np.inf), score=np.full((B, nbest), -np.inf), lm=np.full((B, nbest), -np.inf),
             pb=np.full((B, nbest), -np.inf), pnb=np.full((B, nbest), -np.inf),
             count=np.zeros((B,), np.int32), status=np.zeros((B,), np.int32), ranked=np.zeros((B,), np.int32),
             ends=np.zeros((B,), np.int32), dup_steps=np.zeros((B,), np.int32), gaps=np.full((B,), np.inf),
             gap=float("inf"), branches=set())
    for b in range(B):
        L = W if input_lengths is None else int(input_lengths[b])
        rows = [(cand_idx[cand_off[t * B + b]:cand_off[t * B + b + 1]], cand_logp[cand_off[t * B + b]:cand_off[t * B + b + 1]])
                for t in range(W)]
        one = search_line(codec, top1[:, b], blank[:, b], rows, beam, nbest, L, cap)
        r["gaps"][b] = one["gap"]
        r["gap"] = min(r["gap"], one["gap"])
        r["branches"] |= one["branches"]
        r["count"][b], r["status"][b], r["ranked"][b] = len(one["hyps"]), one["status"], one["ranked"]
        r["ends"][b], r["dup_steps"][b] = one["end"], one["dup_steps"]
        for i, h in enumerate(one["hyps"]):
            n = len(h["labels"])
            r["labels"][b, i, :n] = h["labels"]
            r["lengths"][b, i] = n
            for f in ("logp", "score", "lm", "pb", "pnb"):
                r[f][b, i] = h[f]
    return r
