"""Float64 yardstick of the set form of pattern-constrained recognition (include/hctr_hip.h ``hctr_pat_build_sets``): the
CTC lift of a deterministic automaton whose arcs carry label sets, and the sum and max recursions over it in block form.
The block of DFA state p is beta_p and every eps_(p,.). Per step the log-sum of every block and, for each member, the
log-sum of the block without it - by prefix and suffix log-sums, so nothing is subtracted and the exclusion is exact -
then every state from the totals of its source blocks. The max recursion keeps the two best values of a block and applies
the tie rule of the explicit form (the lowest state among the maximal sources); the walk back gives the path. Plain
numpy; tests/test_pattern_set_host.py checks it against tests/pattern_ref.py on the expanded automaton.
"""
import numpy as np

import pattern_ref

MAX_STATES, MAX_DFA_STATES, MAX_INARCS = 65535, 4096, 1 << 20


def expand(arcs, sets):
    """the single-label arcs (src, label, dst) of the set arcs (src, set, dst)"""
    return [(int(p), int(c), int(q)) for p, k, q in arcs for c in sets[int(k)]]


def tables(arcs, sets, finals, num_states):
    """dict: nQ, S, state_label [S], members (per block the states, ascending: beta_p first), arc_state / arc_p / arc_ex
    (per reduced in-arc the eps state it feeds, the source block, and eps_(p,c) or -1), start, finals, owner [S]"""
    live, fin, nQ = pattern_ref.prune(arcs, finals, num_states)           # (the set index rides in the label's place)
    into = {}
    for p, k, q in live:
        into.setdefault(q, []).append((p, k))
    labels = [sorted(set(int(c) for _, k in into.get(q, []) for c in sets[k])) for q in range(nQ)]
    first = np.concatenate([[nQ], nQ + np.cumsum([len(v) for v in labels])]).astype(np.int64)
    eps = [{c: int(first[q]) + j for j, c in enumerate(labels[q])} for q in range(nQ)]
    S = int(first[-1])
    label = np.array([0] * nQ + [c for v in labels for c in v], np.int64)
    owner = np.array(list(range(nQ)) + [q for q in range(nQ) for _ in labels[q]], np.int64)
    members = [np.concatenate([[q], np.arange(first[q], first[q + 1])]).astype(np.int64) for q in range(nQ)]
    arc_state, arc_p, arc_ex = [], [], []
    for q in range(nQ):
        for p, k in sorted(into.get(q, [])):
            for c in sets[k]:
                arc_state.append(eps[q][int(c)])
                arc_p.append(p)
                arc_ex.append(eps[p].get(int(c), -1))
    start = sorted(set([0] + [eps[q][int(c)] for p, k, q in live if p == 0 for c in sets[k]]))
    return {"nQ": nQ, "S": S, "state_label": label, "owner": owner, "members": members,
            "arc_state": np.array(arc_state, np.int64), "arc_p": np.array(arc_p, np.int64),
            "arc_ex": np.array(arc_ex, np.int64), "start": np.array(start, np.int64), "finals": list(fin)}


def _block_sums(a, mem):
    """(total, the total without each member) of a[mem], by prefix and suffix log-sums"""
    x = a[mem]
    n = len(x)
    pre = np.logaddexp.accumulate(x)
    suf = np.logaddexp.accumulate(x[::-1])[::-1]
    left = np.concatenate([[-np.inf], pre[:-1]])
    right = np.concatenate([suf[1:], [-np.inf]])
    return pre[n - 1], np.logaddexp(left, right)


def recurse(lp, t):
    """(logp, best_logp, path or None) of one line: lp float64 [T][C] log-probabilities, t the tables"""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    nQ, S, label, members = t["nQ"], t["S"], t["state_label"], t["members"]
    ast, ap, aex = t["arc_state"], t["arc_p"], t["arc_ex"]
    has = aex >= 0
    idx = np.arange(S)
    a = np.full(S, -np.inf)
    a[t["start"]] = lp[0][label[t["start"]]]
    v = a.copy()
    bp = np.zeros((T, S), np.int64)
    bp[0] = idx

    def totals():
        tot, excl = np.full(nQ, -np.inf), np.full(S, -np.inf)
        v1, v2 = np.full(nQ, -np.inf), np.full(nQ, -np.inf)
        i1, i2 = np.zeros(nQ, np.int64), np.zeros(nQ, np.int64)
        with np.errstate(invalid="ignore"):
            for p, mem in enumerate(members):
                tot[p], excl[mem] = _block_sums(a, mem)
                x = v[mem]
                k = int(np.argmax(x))                             # (the first: the lowest state)
                v1[p], i1[p] = x[k], mem[k]
                y = x.copy()
                y[k] = -np.inf
                k2 = int(np.argmax(y))                            # (a runner-up at -inf never wins: its state is moot)
                v2[p], i2[p] = y[k2], mem[k2]
        return tot, excl, v1, i1, v2, i2

    for k in range(1, T):
        tot, excl, v1, i1, v2, i2 = totals()
        na, nv, nb = a.copy(), v.copy(), idx.copy()
        na[:nQ] = tot
        nv[:nQ] = v1
        nb[:nQ] = np.where(np.isneginf(v1), idx[:nQ], i1)
        if len(ast):
            term = np.where(has, excl[np.maximum(aex, 0)], tot[ap])
            np.logaddexp.at(na, ast, term)
            top = has & (i1[ap] == aex)
            cv, ci = np.where(top, v2[ap], v1[ap]), np.where(top, i2[ap], i1[ap])
            np.maximum.at(nv, ast, cv)
            arg = np.where(v == nv, idx, S)                       # the lowest state among the maximal sources
            hit = np.nonzero(cv == nv[ast])[0]
            np.minimum.at(arg, ast[hit], ci[hit])
            nb[nQ:] = np.where(np.isneginf(nv[nQ:]), idx[nQ:], arg[nQ:])
        a, v = na + lp[k][label], nv + lp[k][label]
        bp[k] = nb
    tot, _, v1, i1, _, _ = totals()
    fin = np.array(t["finals"], np.int64)
    logp = pattern_ref.logsumexp(tot[fin])
    best = float(v1[fin].max())
    if best == -np.inf:
        return logp, best, None
    s = int(min(i1[q] for q in fin if v1[q] == best))             # ties to the lowest state
    path = []
    for k in range(T - 1, -1, -1):
        path.append(int(label[s]))
        s = int(bp[k][s])
    return logp, best, path[::-1]


def run(logits, arcs, sets, finals, num_states, input_lengths=None):
    """per line (logp, best_logp, path or None) for logits [W][B][C]"""
    logits = np.asarray(logits)
    W, B, _ = logits.shape
    t = tables(arcs, sets, finals, num_states)
    out = []
    for b in range(B):
        T = W if input_lengths is None else int(input_lengths[b])
        out.append(recurse(pattern_ref.log_softmax(logits[:T, b]), t))
    return out
