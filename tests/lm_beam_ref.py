"""Float64 restatement of the device prefix beam search with an n-gram model (include/hctr_hip.h, hctr_nbest_lm*), the
yardstick of tests/test_gpu_nbest_lm.py and tests/test_lm_beam_host.py.

Like tests/nbest_ref.py it invents nothing: every step is ``oracle.ctc_ref.CtcCodecRef.step`` with ``ngram =
ArpaRef(path)`` and ``use_tfm_pred = False``, the greedy line, the suffixes and the end step are the codec's own
``_top_line / _suffix / _end_step`` - so a line is searched exactly as ``beam_full_from_topk`` searches it - fed ``{class:
float32 log-prob}`` rows. What it adds is what the contract returns: the first ``nbest`` hypotheses of the final list with
pb, pnb, logp, the n-gram score of the text and the total, and the smallest nonzero gap between adjacent totals. Labels
stand for themselves: class c is the character chr(BASE + c).

``ArpaRef.score`` re-scores the whole sentence for every entry of every step; ``MemoCodecRef`` keeps, per prefix, the
running sum and the context ``ArpaRef.score`` has after that prefix and adds the remaining ``ArpaRef._word`` terms to it
in the same order - the same float64 additions, hence the same bits (tests/test_lm_beam_host.py checks it against the
plain class).
"""
import numpy as np

from oracle.ctc_ref import ArpaRef, CtcCodecRef, Hyp

BASE = 0x4E00
NEG_INF = float("-inf")


def chars_of(C):
    return "".join(chr(BASE + c) for c in range(1, C - 1))


def write_arpa(path, order, n_chars, seed=7, unk=True):
    """Deterministic ARPA model of the given order (1, 2, 3, 5, 6 - or 7, which the flat table must refuse) over the
    characters of classes 1 .. n_chars - or the characters given in place of that number - (+ <s>, </s> and, unless
    ``unk`` is False, <unk>): every unigram, and of each higher order only SOME n-grams - extensions of n-grams of the
    order below - so every back-off branch is taken. Returns the number of n-grams."""
    rng = np.random.RandomState(1000 * order + seed)
    chars = [chr(BASE + c) for c in range(1, n_chars + 1)] if isinstance(n_chars, int) else list(n_chars)
    words = (["<unk>"] if unk else []) + ["<s>", "</s>"] + chars
    heads = [w for w in words if w != "</s>"]                       # may start or continue an n-gram
    tails = [w for w in words if w != "<s>"]                        # may end one
    keep = {2: 0.45, 3: 0.25, 4: 0.12, 5: 0.10, 6: 0.09, 7: 0.05}
    grams = [[(w,) for w in words]]
    for n in range(2, order + 1):
        prev = [g for g in grams[-1] if g[-1] != "</s>"]
        if n == 2:
            prev = [(w,) for w in heads]
        grams.append([g + (w,) for g in prev for w in tails if rng.rand() < keep[n]])
    with open(path, "w", encoding="utf-8") as f:
        f.write("\\data\\\n" + "".join("ngram %d=%d\n" % (n + 1, len(g)) for n, g in enumerate(grams)))
        for n, gs in enumerate(grams, 1):
            f.write("\n\\%d-grams:\n" % n)
            for g in gs:
                p = -0.2 - (4.0 - 0.5 * n) * rng.rand()
                if n < order and g[-1] != "</s>":
                    f.write("%.6f\t%s\t%.6f\n" % (p, " ".join(g), -0.1 - 0.6 * rng.rand()))
                else:
                    f.write("%.6f\t%s\n" % (p, " ".join(g)))
        f.write("\n\\end\\\n")
    return sum(len(g) for g in grams)


class MemoCodecRef(CtcCodecRef):
    """CtcCodecRef over an ArpaRef whose ``_ngram_score`` does not start from the beginning of the sentence"""

    def __init__(self, characters_str, arpa):
        super(MemoCodecRef, self).__init__(characters_str)
        self.ngram = arpa
        self._keep = max(arpa.order - 1, 0)
        first = ("<s>",) if ("<s>",) in arpa.grams else ()
        self._memo = {"": (0.0, first)}

    def _after(self, state, ch):
        total, ctx = state
        total += self.ngram._word(list(ctx), ch)
        ctx = ctx + ((ch if (ch,) in self.ngram.grams else "<unk>"),)
        return total, (ctx[-self._keep:] if self._keep else ())

    def _state(self, prefix):
        hit = self._memo.get(prefix)
        if hit is None:
            hit = self._memo[prefix] = self._after(self._state(prefix[:-1]), prefix[-1])
        return hit

    def _ngram_score(self, prefix, suffix):
        state = self._state(prefix)
        for ch in suffix:
            state = self._after(state, ch)
        return state[0]


def make_codec(C, k, arpa_path, lm_panelty, len_bonus, memo=True):
    arpa = arpa_path if isinstance(arpa_path, ArpaRef) else ArpaRef(arpa_path)
    codec = MemoCodecRef(chars_of(C), arpa) if memo else CtcCodecRef(chars_of(C))
    assert len(codec.characters) == C
    codec.ngram = arpa
    codec.use_tfm_pred = False
    codec.use_tfm_score = False
    codec.search_depth = k
    codec.lm_panelty = lm_panelty
    codec.len_bonus = len_bonus
    codec.beam_size = 1 << 30                    # step() returns the whole sorted list; search_line cuts it
    return codec


def search_line(codec, idx, lp, beam, nbest, L=None):
    """One line over its first L columns. idx int [T, k], lp float32 [T, k]: the row lists. Returns (hyps, gap, end):
    hyps = the first ``nbest`` hypotheses of the final list as dicts (labels, pb, pnb, logp, lm, score), [] for an empty
    greedy text; gap = the smallest nonzero finite gap between adjacent totals among the first ``beam + 1`` sorted
    entries over all steps (inf if there is none); end = the steps the line ran (0 for an empty greedy text)."""
    idx, lp = np.asarray(idx), np.asarray(lp, np.float32)
    L = idx.shape[0] if L is None else int(L)
    top_line = codec._top_line(idx[:L, 0])
    if not top_line:
        return [], float("inf"), 0
    end = codec._end_step(top_line, L)
    beams, gap = [Hyp()], float("inf")
    with np.errstate(invalid="ignore"):
        for t in range(end):
            row = {int(c): np.float32(v) for c, v in zip(idx[t], lp[t])}
            full = codec.step(beams, idx[t], row, codec._suffix(top_line, t)) if beams else []
            tot = np.array([float(h.total()) for h in full[:beam + 1]], np.float64)
            d = tot[:-1] - tot[1:]
            d = d[np.isfinite(d) & (d != 0)]
            if d.size:
                gap = min(gap, float(d.min()))
            beams = full[:beam]
    out = []
    for h in beams[:nbest]:
        out.append(dict(labels=[ord(ch) - BASE for ch in h.prefix], pb=float(h.pb), pnb=float(h.pnb),
                        logp=float(h.prob()), lm=float(codec._ngram_score(h.prefix, "")), score=float(h.total())))
    return out, gap, end


def search(codec, idx, lp, beam, nbest, input_lengths=None):
    """A batch. idx / lp [W, B, k]. Returns a dict: labels int32 [B, nbest, W], lengths int32 [B, nbest], logp, score, lm
    float64 [B, nbest], count int32 [B] with the contract's fill of unused slots, gap, and ends int32 [B]."""
    idx, lp = np.asarray(idx), np.asarray(lp, np.float32)
    W, B, _ = idx.shape
    r = dict(labels=np.zeros((B, nbest, W), np.int32), lengths=np.zeros((B, nbest), np.int32),
             logp=np.full((B, nbest), -np.inf), score=np.full((B, nbest), -np.inf), lm=np.full((B, nbest), -np.inf),
             count=np.zeros((B,), np.int32), ends=np.zeros((B,), np.int32), gap=float("inf"))
    for b in range(B):
        L = W if input_lengths is None else int(input_lengths[b])
        hyps, g, end = search_line(codec, idx[:, b], lp[:, b], beam, nbest, L)
        r["gap"] = min(r["gap"], g)
        r["count"][b], r["ends"][b] = len(hyps), end
        for i, h in enumerate(hyps):
            n = len(h["labels"])
            r["labels"][b, i, :n] = h["labels"]
            r["lengths"][b, i] = n
            r["logp"][b, i], r["score"][b, i], r["lm"][b, i] = h["logp"], h["score"], h["lm"]
    return r
