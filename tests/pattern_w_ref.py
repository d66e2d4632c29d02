"""Float64 restatement of weighted pattern recognition as include/hctr_hip.h defines it (hctr_pat_build_weighted): the
weights of the CTC lift's in-edges, start list and accepting list on top of pattern_ref.tables, the sum and max
recursions with the weights and the tie rule, the walk back, a text's weight, and enumeration of all C^T paths with
weights. Plain numpy and Python; tests/test_pattern_w_host.py checks it against the enumeration.
"""
import itertools

import numpy as np

import pattern_ref
from pattern_ref import collapse, log_softmax, logsumexp, spans  # noqa: F401  (re-exported for the tests)


def _survivors(arcs, finals):
    """old state -> new state of the states both reachable from 0 and able to reach a final state"""
    out, into = {}, {}
    for p, _, q in arcs:
        out.setdefault(int(p), []).append(int(q))
        into.setdefault(int(q), []).append(int(p))

    def closure(seed, nxt):
        seen, stack = set(seed), list(seed)
        while stack:
            for v in nxt.get(stack.pop(), []):
                if v not in seen:
                    seen.add(v)
                    stack.append(v)
        return seen

    return {s: i for i, s in enumerate(sorted(closure([0], out) & closure([int(f) for f in finals], into)))}


def tables(arcs, finals, num_states, weights=None, final_weights=None):
    """pattern_ref.tables of the automaton plus in_w (parallel to in_src), accept_w, start_w (float32) and the pruned
    automaton's weights: arc_w {(p, c): (q, w)} and final_w {q: w}"""
    arcs = [(int(p), int(c), int(q)) for p, c, q in arcs]
    finals = [int(f) for f in finals]
    w = np.zeros(len(arcs), np.float32) if weights is None else np.asarray(weights, np.float32)
    fw = np.zeros(len(finals), np.float32) if final_weights is None else np.asarray(final_weights, np.float32)
    t = pattern_ref.tables(arcs, finals, num_states)
    num = _survivors(arcs, finals)
    nQ = t["nQ"]
    assert len(num) == nQ
    arc_w = {(num[p], c): (num[q], np.float32(w[i])) for i, (p, c, q) in enumerate(arcs) if p in num and q in num}
    final_w = {num[f]: np.float32(fw[i]) for i, f in enumerate(finals) if f in num}
    label = t["state_label"]
    pairs = sorted(set((q, c) for (_, c), (q, _) in arc_w.items()))     # eps state nQ + i = pairs[i]
    assert [c for _, c in pairs] == label[nQ:].tolist()
    dfa = lambda s: s if s < nQ else pairs[s - nQ][0]
    in_w = np.zeros(len(t["in_src"]), np.float32)
    for s in range(nQ, len(label)):
        q, c = pairs[s - nQ]
        for j in range(t["in_ptr"][s], t["in_ptr"][s + 1]):
            u = int(t["in_src"][j])
            if u != s:
                dst, wt = arc_w[(dfa(u), c)]
                assert dst == q
                in_w[j] = wt
    t["in_w"] = in_w
    t["accept_w"] = np.array([final_w[dfa(int(s))] for s in t["accept"]], np.float32)
    t["start_w"] = np.array([0.0 if s < nQ else arc_w[(0, pairs[s - nQ][1])][1] for s in t["start"].tolist()], np.float32)
    t["arc_w"], t["final_w"] = arc_w, final_w
    return t


def text_weight(t, text):
    """the float64 sum, in text order, of the float32 arc weights plus the final weight; -inf outside the language"""
    q, w = 0, 0.0
    for c in text:
        if (q, int(c)) not in t["arc_w"]:
            return -np.inf
        q, wt = t["arc_w"][(q, int(c))]
        w += float(wt)
    return w + float(t["final_w"][q]) if q in t["final_w"] else -np.inf


def recurse(lp, t):
    """(logp, best_logp, path) of one line as pattern_ref.recurse gives them, with the weights: every in-edge adds its
    weight to its source's value, the start list and the accepting list add theirs"""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    label, ptr, src = t["state_label"].astype(np.int64), t["in_ptr"].astype(np.int64), t["in_src"].astype(np.int64)
    in_w, acc_w, st_w = (t[k].astype(np.float64) for k in ("in_w", "accept_w", "start_w"))
    S = len(label)
    seg = np.repeat(np.arange(S), np.diff(ptr))
    a = np.full(S, -np.inf)
    a[t["start"]] = lp[0][label[t["start"]]] + st_w
    v = a.copy()
    bp = np.zeros((T, S), np.int64)
    bp[0] = np.arange(S)
    for k in range(1, T):
        av, vv = a[src] + in_w, v[src] + in_w
        m = np.full(S, -np.inf)
        np.maximum.at(m, seg, av)
        with np.errstate(invalid="ignore"):
            ex = np.where(np.isneginf(m[seg]), 0.0, np.exp(av - m[seg]))
        sm = np.zeros(S)
        np.add.at(sm, seg, ex)
        with np.errstate(divide="ignore"):
            a = np.where(np.isneginf(m), -np.inf, m + np.log(sm)) + lp[k][label]
        vm = np.full(S, -np.inf)
        np.maximum.at(vm, seg, vv)
        first = np.full(S, len(src), np.int64)                # the first edge that attains the maximum
        hit = np.nonzero(vv == vm[seg])[0]
        np.minimum.at(first, seg[hit], hit)
        arg = src[np.minimum(first, len(src) - 1)]
        bp[k] = np.where(np.isneginf(vm), np.arange(S), arg)
        v = vm + lp[k][label]
    acc = t["accept"].astype(np.int64)
    logp = logsumexp(a[acc] + acc_w)
    fin = v[acc] + acc_w
    best = float(fin.max())
    if best == -np.inf:
        return logp, best, None
    s = int(acc[int(np.argmax(fin))])                         # (argmax: the first, so the lowest state)
    path = []
    for k in range(T - 1, -1, -1):
        path.append(int(label[s]))
        s = int(bp[k][s])
    return logp, best, path[::-1]


def run(logits, t, input_lengths=None):
    """per line (logp, best_logp, path or None) for logits [W][B][C] and the weighted tables t"""
    logits = np.asarray(logits)
    W, B, _ = logits.shape
    out = []
    for b in range(B):
        T = W if input_lengths is None else int(input_lengths[b])
        out.append(recurse(log_softmax(logits[:T, b]), t))
    return out


def enumerate_paths(lp, t):
    """(logp, best_logp, best paths) by visiting every path of C^T (tiny cases only): the log of the sum of
    exp(path score + w(collapse)) over the accepted paths, the best such figure and every path that attains it"""
    T, C = lp.shape
    total, best, best_paths = 0.0, -np.inf, []
    for path in itertools.product(range(C), repeat=T):
        w = text_weight(t, collapse(path))
        if w == -np.inf:
            continue
        s = float(sum(lp[k, c] for k, c in enumerate(path))) + w
        total += np.exp(s)
        if s > best + 1e-12:
            best, best_paths = s, [list(path)]
        elif abs(s - best) <= 1e-12:
            best_paths.append(list(path))
    with np.errstate(divide="ignore"):
        return float(np.log(total)), best, best_paths
