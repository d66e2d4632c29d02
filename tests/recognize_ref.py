"""numpy restatement of the greedy recognition the engine computes (include/hctr_hip.h, hctr_recognize*), the float64
yardstick of tests/test_gpu_recognize.py and tests/test_recognize_host.py. The reference project has no counterpart.

For row (t, b) with logits z over C classes: k1 = np.argmax(z) (first maximum, a NaN counts as the maximum), k2 = the
first index of the largest logit among the classes c != k1, lp = z - logsumexp(z) in float64. A column is kept iff
k1 != 0 and k1 != C-1 and k1 != k1[t-1] (compared raw); character j has the label of its kept column s_j and the span
[s_j, e_j), e_j the first t > s_j with k1[t] != label, or W. Per character: the sum of lp[t, label] over the span, and
k2 / lp[., k2] at the span's peak column (largest lp[t, label], first on ties). Per line: path_logp = the sum of
lp[t, k1[t]] over all W columns, text_nll = the CTC loss (blank 0) of the decoded labels over all W columns.
"""
import numpy as np


def lse64(z):
    """float64 log-sum-exp over the last axis; NaN for a row holding a NaN or +inf, or nothing but -inf"""
    z = np.asarray(z, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        mx = z.max(axis=-1)
        return mx + np.log(np.exp(z - mx[..., None]).sum(axis=-1))


def top2(row):
    """(k1, k2) of one row in np.argmax's order"""
    k1 = int(np.argmax(row))
    rest = np.delete(np.arange(len(row)), k1)
    return k1, int(rest[np.argmax(row[rest])])


def collapse(k1, C):
    """kept columns of one line's raw argmaxes"""
    k1 = np.asarray(k1)
    prev = np.concatenate([[-1], k1[:-1]])
    return np.flatnonzero((k1 != 0) & (k1 != C - 1) & (k1 != prev))


def ctc_nll64(lp, labels):
    """float64 CTC loss of one line: lp [T, C] log-probs, blank 0, every step counts"""
    T, L = lp.shape[0], len(labels)
    if L == 0:
        return -float(lp[:, 0].sum())
    ext = np.zeros(2 * L + 1, np.int64)
    ext[1::2] = labels
    skip = np.zeros(2 * L + 1, bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    with np.errstate(invalid="ignore"):
        a = np.full(2 * L + 1, -np.inf)
        a[0], a[1] = lp[0, 0], lp[0, ext[1]]
        for t in range(1, T):
            p1 = np.concatenate([[-np.inf], a[:-1]])
            p2 = np.where(skip, np.concatenate([[-np.inf, -np.inf], a[:-2]]), -np.inf)
            a = np.logaddexp(np.logaddexp(a, p1), p2) + lp[t, ext]
        return -float(np.logaddexp(a[-1], a[-2]))


def recognize_ref(logits):
    """logits [W, B, C] -> dict of float64 / int arrays shaped as ctc.Recognition's ([B, W] per character, zeros past a
    line's length; [B] per line) plus k1, k2 [B, W]"""
    z = np.asarray(logits, np.float32)
    W, B, C = z.shape
    z64 = z.astype(np.float64)
    with np.errstate(invalid="ignore"):
        lp = z64 - lse64(z)[..., None]                         # [W, B, C]
    out = {k: np.zeros((B, W), np.int32) for k in ("labels", "starts", "ends", "alt_labels", "k1", "k2")}
    out.update({k: np.zeros((B, W), np.float64) for k in ("logps", "alt_logps")})
    out.update(lengths=np.zeros(B, np.int32), path_logp=np.zeros(B), text_nll=np.zeros(B))
    for b in range(B):
        for t in range(W):
            out["k1"][b, t], out["k2"][b, t] = top2(z[t, b])
        k1, k2 = out["k1"][b], out["k2"][b]
        lp1 = lp[np.arange(W), b, k1]
        lp2 = lp[np.arange(W), b, k2]
        kept = collapse(k1, C)
        out["lengths"][b] = len(kept)
        for j, s in enumerate(kept):
            e = s + 1
            while e < W and k1[e] == k1[s]:
                e += 1
            run = lp1[s:e]
            peak = s if np.isnan(run).any() else s + int(np.argmax(run))
            out["labels"][b, j], out["starts"][b, j], out["ends"][b, j] = k1[s], s, e
            out["logps"][b, j] = run.sum()
            out["alt_labels"][b, j] = k2[peak]
            out["alt_logps"][b, j] = np.nan if np.isnan(run).any() else lp2[peak]
        out["path_logp"][b] = lp1.sum()
        out["text_nll"][b] = ctc_nll64(lp[:, b], k1[kept])
    return out


def planted(rng, W, C, labels, boost=12.0, alt_boost=6.0):
    """One line [W, C] of N(0, 1) noise with ``boost`` (plus |noise|) on a planted class per column - a random greedy path that
    collapses to ``labels`` (blanks part equal neighbours; no C-1) - and ``alt_boost`` on a planted runner-up.
    -> (logits float32, path [W] planted classes, alt [W] planted runners-up)"""
    L = len(labels)
    S = 2 * L + 1
    need = np.zeros(S, np.int64)
    need[1::2] = 1
    if L > 1:
        need[2:-1:2] = (np.asarray(labels[1:]) == np.asarray(labels[:-1])).astype(np.int64)
    spare = W - int(need.sum())
    assert spare >= 0
    dur = need + np.bincount(rng.randint(0, S, spare), minlength=S)
    ext = np.zeros(S, np.int64)
    ext[1::2] = labels
    path = ext[np.repeat(np.arange(S), dur)]
    alt = (path + 1 + rng.randint(0, C - 2, W)) % (C - 1)      # any class but the planted one and C-1 (C >= 3)
    z = rng.standard_normal((W, C)).astype(np.float32)
    for cls, up in ((path, boost), (alt, alt_boost)):          # |noise| on the planted two: no third class overtakes them
        z[np.arange(W), cls] = np.abs(z[np.arange(W), cls]) + np.float32(up)
    return z, path, alt


# hand-written collapse cases over C = 6 classes (0 = blank, 5 = C-1): the raw argmax of every column, and what the
# decode must make of it: (k1 per column, [(label, start, end), ...])
HAND_CASES = [
    ("adjacent repeats", [2, 2, 2, 3, 3, 0, 0], [(2, 0, 3), (3, 3, 5)]),
    ("repeat parted by a blank", [0, 4, 4, 0, 4, 0], [(4, 1, 3), (4, 4, 5)]),
    ("repeat parted by a run of C-1", [1, 5, 5, 5, 1, 1, 2], [(1, 0, 1), (1, 4, 6), (2, 6, 7)]),
    ("a character in the last column", [0, 0, 3, 0, 0, 1], [(3, 2, 3), (1, 5, 6)]),
    ("all blank", [0, 0, 0, 0, 0], []),
    ("W = 1, a character", [3], [(3, 0, 1)]),
    ("W = 1, blank", [0], []),
    ("W = 1, C-1", [5], []),
]
HAND_C = 6


def hand_logits(rng, k1, C=HAND_C, boost=9.0):
    """[W, 1, C] logits whose argmax per column is k1"""
    z = rng.standard_normal((len(k1), 1, C)).astype(np.float32)
    z[np.arange(len(k1)), 0, np.asarray(k1)] += np.float32(boost)
    return z


def _runs(W, runs):
    k1 = np.zeros(W, np.int64)
    for label, s, e in runs:
        k1[s:e] = label
    return k1.tolist()


# runs that straddle a 64-column chunk of the collapse: (W, k1 per column, [(label, start, end), ...])
STRADDLE_CASES = [
    (65, _runs(65, [(1, 3, 5), (2, 61, 65)]), [(1, 3, 5), (2, 61, 65)]),
    (129, _runs(129, [(1, 3, 5), (2, 62, 66), (2, 67, 69), (5, 100, 110), (4, 126, 129)]),
     [(1, 3, 5), (2, 62, 66), (2, 67, 69), (4, 126, 129)]),
]
