"""numpy restatement of the forced alignment the engine computes (include/hctr_hip.h, hctr_ctc_align*), the yardstick of
tests/test_gpu_ctc_align.py and tests/test_ctc_align_host.py. The reference project has no counterpart.

For one line of T steps over targets l_1..l_L, extended states blank, l_1, blank, ..., l_L, blank (S = 2L + 1) and
lp_t(c) = z_t[c] - logsumexp(z_t) (float64 log-softmax, then rounded to ``dtype``):
    v_0(0) = lp_0(blank), v_0(1) = lp_0(l_1), -inf elsewhere
    v_t(s) = max(v_{t-1}(s), v_{t-1}(s-1), [l_s != l_{s-2}] v_{t-1}(s-2)) + lp_t(class of s)      in ``dtype``
Ties: among equal predecessors s, then s-1, then s-2; the end state is S-1 if v_{T-1}(S-1) >= v_{T-1}(S-2), else S-2
(state 0 for L = 0). A line with L + adjacent repeats > T has no alignment, and neither has a line whose best score is
-inf (logits of -inf mask classes out; every path may go through one).
"""
import numpy as np


def log_softmax64(z):
    z = np.asarray(z, np.float64)
    mx = z.max(axis=-1, keepdims=True)
    return z - (mx + np.log(np.exp(z - mx).sum(axis=-1, keepdims=True)))


def feasible(targets, T):
    t = np.asarray(targets).reshape(-1)
    return len(t) + int((t[1:] == t[:-1]).sum()) <= T


def spans_of_states(states, L):
    """(starts, ends) of the labels along a state sequence; a label's steps are contiguous"""
    st, en = np.full(L, -1, np.int32), np.full(L, -1, np.int32)
    for t, s in enumerate(states):
        if s & 1:
            if st[s >> 1] < 0:
                st[s >> 1] = t
            en[s >> 1] = t + 1
    return st, en


def viterbi(logits, targets, dtype=np.float64):
    """logits [T, C] -> dict(states [T], path [T] classes, score, starts, ends, logps [L] in ``dtype``, lp64 [T, C]);
    for a line without an alignment: score -inf, path / starts / ends -1, logps -inf, states None"""
    dtype = np.dtype(dtype).type
    tg = np.asarray(targets, np.int64).reshape(-1)
    T, L = logits.shape[0], len(tg)
    lp64 = log_softmax64(logits)
    none = {"states": None, "path": np.full(T, -1, np.int32), "score": dtype(-np.inf),
            "starts": np.full(L, -1, np.int32), "ends": np.full(L, -1, np.int32),
            "logps": np.full(L, -np.inf, dtype), "lp64": lp64}
    if not feasible(tg, T):
        return none
    S = 2 * L + 1
    ext = np.zeros(S, np.int64)
    ext[1::2] = tg
    skip = np.zeros(S, bool)
    skip[3::2] = tg[1:] != tg[:-1]
    em = lp64[:, ext].astype(dtype)                    # [T, S]
    ninf = dtype(-np.inf)
    v = np.full(S, ninf, dtype)
    v[0] = em[0, 0]
    if S > 1:
        v[1] = em[0, 1]
    back = np.zeros((T, S), np.int8)
    for t in range(1, T):
        pad = np.concatenate([[ninf, ninf], v]).astype(dtype)
        c1 = pad[1:S + 1]
        c2 = np.where(skip, pad[:S], ninf)
        best, k = v.copy(), np.zeros(S, np.int8)
        m = c1 > best
        best[m], k[m] = c1[m], 1
        m = c2 > best
        best[m], k[m] = c2[m], 2
        v = (best + em[t]).astype(dtype)
        back[t] = k
    s = S - 1 if (L == 0 or v[S - 1] >= v[S - 2]) else S - 2
    score = v[s]
    if score == ninf:                                  # masked (-inf) logits leave the line no path
        return none
    states = np.zeros(T, np.int64)
    for t in range(T - 1, -1, -1):
        states[t] = s
        s -= int(back[t, s])
    st, en = spans_of_states(states, L)
    logps = np.full(L, ninf, dtype)
    for j in range(L):
        if st[j] >= 0:
            acc = em[st[j], 2 * j + 1]
            for t in range(st[j] + 1, en[j]):
                acc = dtype(acc + em[t, 2 * j + 1])
            logps[j] = acc
    return {"states": states, "path": ext[states].astype(np.int32), "score": score, "starts": st, "ends": en,
            "logps": logps, "lp64": lp64}


def path_score64(lp64, path):
    """float64 log-probability of a path of classes"""
    return float(lp64[np.arange(len(path)), np.asarray(path, np.int64)].sum())


def collapse(path):
    p = np.asarray(path)
    p = p[p >= 0]
    keep = np.ones(len(p), bool)
    keep[1:] = p[1:] != p[:-1]
    p = p[keep]
    return p[p != 0]


def random_target(rng, C, L, repeat=0.3):
    """L labels in [1, C-1], each equal to the one before with probability ``repeat``"""
    out = []
    for _ in range(L):
        if out and rng.rand() < repeat:
            out.append(out[-1])
        else:
            out.append(int(rng.randint(1, C)))
    return np.array(out, np.int32)


def planted(rng, T, C, targets, boost=12.0):
    """A random valid alignment of ``targets`` over T steps and logits that make it the best path by a wide margin:
    N(0, 1) noise plus ``boost`` on the planted class of every step. -> (logits float32 [T, C], states [T])"""
    tg = np.asarray(targets, np.int64).reshape(-1)
    L = len(tg)
    S = 2 * L + 1
    need = np.zeros(S, np.int64)
    need[1::2] = 1
    need[2:-1:2] = (tg[1:] == tg[:-1]).astype(np.int64)       # a blank must part equal neighbours
    spare = T - int(need.sum())
    assert spare >= 0, "no alignment"
    dur = need + np.bincount(rng.randint(0, S, spare), minlength=S)
    states = np.repeat(np.arange(S), dur)
    ext = np.zeros(S, np.int64)
    ext[1::2] = tg
    logits = rng.standard_normal((T, C)).astype(np.float32)
    logits[np.arange(T), ext[states]] += np.float32(boost)
    return logits, states


TIE_TABLE = [
    (20, [3, 3, 4, 5, 5], [3, 0, 3, 4, 5, 0, 5] + [0] * 13),
    (9, [1, 2, 3, 4], [1, 2, 3, 4, 0, 0, 0, 0, 0]),
    (20, [], [0] * 20),
]
