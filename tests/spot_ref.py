"""Float64 restatement of keyword spotting (include/hctr_hip.h ``hctr_spot*``): the containment posterior over the
query's KMP automaton lifted to CTC, the best tight segment with the documented tie rule, and a brute-force enumerator
of both for tiny shapes. Written from the definitions, independently of the engine's tables: ``automaton`` builds the
exported tables (``hctr_spot_automaton``) from a brute-force delta."""
import itertools

import numpy as np

NEG = -np.inf


def log_softmax(z):
    """float64 log-softmax over the last axis of float logits"""
    z = np.asarray(z, np.float64)
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def delta(q, j, c):
    """the longest k with q_1..q_k a suffix of q_1..q_j c"""
    s = list(q[:j]) + [c]
    for k in range(min(len(q), len(s)), 0, -1):
        if list(q[:k]) == s[len(s) - k:]:
            return k
    return 0


def automaton(q):
    """The tables of one query: states Z = 0, N_j = j, B_j = L-1+j, A = 2L-1; slots 0 = blank, 1..nq = the distinct
    classes ascending, nq+1 = rest, nq+2 = one. Returns a dict: classes, delta [L][nq], num_states, in_ptr, in_src,
    in_slot (a state's in-edges by (source, slot); Z has none), fall_mask [2L]."""
    q = [int(v) for v in q]
    L = len(q)
    classes = sorted(set(q))
    nq = len(classes)
    S, A = 2 * L, 2 * L - 1
    slot_of = {c: 1 + i for i, c in enumerate(classes)}
    d = [[delta(q, j, c) for c in classes] for j in range(L)]
    tgt = lambda k: 0 if k == 0 else (A if k == L else k)
    edges = [[] for _ in range(S)]
    mask = [0] * S
    rest = 1 << (nq + 1)

    def on_class(s, j, c):
        k = d[j][slot_of[c] - 1]
        if k:
            edges[tgt(k)].append((s, slot_of[c]))
        else:
            mask[s] |= 1 << slot_of[c]

    mask[0] = rest | 1
    for c in classes:
        on_class(0, 0, c)
    for j in range(1, L):
        n, b = j, L - 1 + j
        edges[n].append((n, slot_of[q[j - 1]]))
        edges[b].append((n, 0))
        edges[b].append((b, 0))
        mask[n] = mask[b] = rest
        for c in classes:
            if c != q[j - 1]:
                on_class(n, j, c)
            on_class(b, j, c)
    edges[A].append((A, nq + 2))
    ptr, src, slot = [0], [], []
    for s in range(S):
        for e in sorted(edges[s]):
            src.append(e[0])
            slot.append(e[1])
        ptr.append(len(src))
    return dict(classes=classes, delta=d, num_states=S, in_ptr=ptr, in_src=src, in_slot=slot, fall_mask=mask)


def _transition_basis(q):
    """E [nq + 2][S][S]: E[s] is the 0/1 matrix of the moves taken on slot s (blank, the classes, rest), from the
    transition table of the definition; A's loop is added by the caller."""
    a = automaton(q)
    S, nq = a["num_states"], len(a["classes"])
    E = np.zeros((nq + 2, S, S))
    for s in range(S):
        for e in range(a["in_ptr"][s], a["in_ptr"][s + 1]):
            if a["in_slot"][e] <= nq + 1:
                E[a["in_slot"][e], a["in_src"][e], s] = 1.0
    for s in range(S):
        for sl in range(nq + 2):
            if a["fall_mask"][s] >> sl & 1:
                E[sl, s, 0] = 1.0
    return a, E


def contain_logp(lp, q):
    """log P(the collapsed text contains q) over the rows lp [T][C] of float64 log-probs; rest is the exact sum of the
    other classes' probabilities"""
    lp = np.asarray(lp, np.float64)
    T, C = lp.shape
    a, E = _transition_basis(q)
    S, cls = a["num_states"], a["classes"]
    if T == 0:
        return NEG
    p = np.exp(lp)
    other = np.ones(C, bool)
    other[[0] + cls] = False
    P = np.concatenate([p[:, [0] + cls], p[:, other].sum(axis=1, keepdims=True)], axis=1)      # [T][nq + 2]
    v = np.zeros(S)
    v[0] = 1.0
    loop = np.zeros((S, S))
    loop[S - 1, S - 1] = 1.0
    for t in range(T):
        v = v @ (np.tensordot(P[t], E, axes=1) + loop)
    with np.errstate(divide="ignore"):
        return float(np.log(v[S - 1]))


def _better(c, cs, m, ms):
    """where candidate (c, cs) beats (m, ms): the strictly greater score, the larger start on equal scores"""
    return (c > m) | ((c == m) & (cs > ms))


def best_segment(lp, q):
    """(score, t0, t1) of the best tight segment reading q over the rows lp [T][C], with the documented tie rule;
    (-inf, -1, -1) where none fits"""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    q = [int(v) for v in q]
    L = len(q)
    SS = 2 * L - 1
    cls = np.array([q[s // 2] if s % 2 == 0 else 0 for s in range(SS)])
    skip = np.array([s % 2 == 0 and s >= 2 and q[s // 2] != q[s // 2 - 1] for s in range(SS)])
    sc = np.full(SS, NEG)
    st = np.full(SS, -1, np.int64)
    best, bs, be = NEG, -1, -1
    for t in range(T):
        c1 = np.concatenate([[0.0], sc[:-1]])
        s1 = np.concatenate([[t], st[:-1]])
        c2 = np.where(skip, np.concatenate([[NEG, NEG], sc[:-2]])[:SS], NEG)
        s2 = np.where(skip, np.concatenate([[-1, -1], st[:-2]])[:SS], -1)
        m, ms = sc.copy(), st.copy()
        for c, cs in ((c1, s1), (c2, s2)):
            w = _better(c, cs, m, ms)
            m, ms = np.where(w, c, m), np.where(w, cs, ms)
        sc = m + lp[t, cls]
        st = np.where(np.isneginf(sc), -1, ms)
        if sc[SS - 1] > best:
            best, bs, be = float(sc[SS - 1]), int(st[SS - 1]), t + 1
    return best, bs, be


def segment_score(lp, q, t0, t1):
    """the float64 score of the best segment path on exactly the columns [t0, t1): first column q_1, last q_L,
    collapse q; -inf when the window admits none (or is no window)"""
    lp = np.asarray(lp, np.float64)
    q = [int(v) for v in q]
    L = len(q)
    SS = 2 * L - 1
    if not (0 <= t0 < t1 <= lp.shape[0]):
        return NEG
    cls = [q[s // 2] if s % 2 == 0 else 0 for s in range(SS)]
    v = np.full(SS, NEG)
    v[0] = lp[t0, cls[0]]
    for t in range(t0 + 1, t1):
        n = np.full(SS, NEG)
        for s in range(SS):
            m = v[s]
            if s >= 1:
                m = max(m, v[s - 1])
            if s % 2 == 0 and s >= 2 and q[s // 2] != q[s // 2 - 1]:
                m = max(m, v[s - 2])
            n[s] = m + lp[t, cls[s]]
        v = n
    return float(v[SS - 1])


def spot(logits_wbc, queries, input_lengths=None):
    """(contain [B][Q], seg [B][Q], starts, ends) of float logits [W][B][C] and a list of label lists"""
    z = np.asarray(logits_wbc)
    W, B, _ = z.shape
    Q = len(queries)
    contain, seg = np.full((B, Q), NEG), np.full((B, Q), NEG)
    st, en = np.full((B, Q), -1, np.int64), np.full((B, Q), -1, np.int64)
    for b in range(B):
        T = W if input_lengths is None else int(input_lengths[b])
        lp = log_softmax(z[:T, b])
        for k, q in enumerate(queries):
            contain[b, k] = contain_logp(lp, q)
            seg[b, k], st[b, k], en[b, k] = best_segment(lp, q)
    return contain, seg, st, en


# ---- brute force over all paths (tiny shapes only) ----
def collapse(path):
    out, prev = [], 0
    for c in path:
        if c != 0 and c != prev:
            out.append(int(c))
        prev = c
    return out


def _contains(text, q):
    n = len(q)
    return any(text[i:i + n] == q for i in range(len(text) - n + 1))


def brute_contain(lp, q):
    """log of the summed probability of every path in {0..C-1}^T whose collapse contains q"""
    lp = np.asarray(lp, np.float64)
    T, C = lp.shape
    q = [int(v) for v in q]
    total = 0.0
    for path in itertools.product(range(C), repeat=T):
        if _contains(collapse(path), q):
            total += float(np.exp(sum(lp[t, c] for t, c in enumerate(path))))
    with np.errstate(divide="ignore"):
        return float(np.log(total)) if T else NEG


def brute_segment(lp, q):
    """(score, t0, t1): the maximum over every window and every path on it that starts on q_1, ends on q_L and
    collapses to q. Among equal scores the earliest end, then the larger start (the tie rule's outcome)."""
    lp = np.asarray(lp, np.float64)
    T, C = lp.shape
    q = [int(v) for v in q]
    best = (NEG, -1, -1)
    for t1 in range(1, T + 1):
        for t0 in range(t1):
            for path in itertools.product(range(C), repeat=t1 - t0):
                if path[0] != q[0] or path[-1] != q[-1] or collapse(path) != q:
                    continue
                s = sum(lp[t0 + i, c] for i, c in enumerate(path))
                if s > best[0] or (s == best[0] and t1 == best[2] and t0 > best[1]):
                    best = (float(s), t0, t1)
    return best
