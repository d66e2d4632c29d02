"""Float64 restatement of pattern-constrained recognition as include/hctr_hip.h defines it (hctr_pattern*): the CTC lift
of a deterministic finite automaton (its states, in-edges, start and accepting lists), the sum and max recursions over
it with the tie rule, the walk back, the collapse and the spans. Plain numpy and Python; tests/test_pattern_host.py
checks it against enumeration of all paths, torch's float64 ctc_loss and the lexicon's and spotting's yardsticks.
"""
import itertools

import numpy as np

MAX_STATES, MAX_EDGES = 8192, 262144


def log_softmax(z):
    z = np.asarray(z, np.float64)
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


def collapse(path):
    out, prev = [], 0
    for c in path:
        if c != 0 and c != prev:
            out.append(int(c))
        prev = c
    return out


def accepts(arcs, finals, text):
    """whether the DFA (arcs from state 0) accepts the label sequence"""
    d = {(int(p), int(c)): int(q) for p, c, q in arcs}
    q = 0
    for c in text:
        if (q, int(c)) not in d:
            return False
        q = d[(q, int(c))]
    return q in set(int(f) for f in finals)


def prune(arcs, finals, num_states):
    """(arcs, finals, nQ) without the states that are not both reachable from state 0 and able to reach a final state,
    the survivors renumbered in their relative order; None for an empty language"""
    arcs = [(int(p), int(c), int(q)) for p, c, q in arcs]
    fwd, stack = {0}, [0]
    while stack:
        s = stack.pop()
        for p, _, q in arcs:
            if p == s and q not in fwd:
                fwd.add(q)
                stack.append(q)
    bwd, stack = set(int(f) for f in finals), [int(f) for f in finals]
    while stack:
        s = stack.pop()
        for p, _, q in arcs:
            if q == s and p not in bwd:
                bwd.add(p)
                stack.append(p)
    if 0 not in bwd:
        return None
    keep = sorted(fwd & bwd)
    num = {s: i for i, s in enumerate(keep)}
    return (sorted((num[p], c, num[q]) for p, c, q in arcs if p in num and q in num),
            sorted(num[f] for f in set(int(f) for f in finals) if f in num), len(keep))


def tables(arcs, finals, num_states):
    """dict of the tables of the definitions: state_label, state_slot, in_ptr, in_src, classes, accept, start (numpy
    arrays with the dtypes of hctr_pat_tables), plus nQ"""
    arcs, finals, nQ = prune(arcs, finals, num_states)
    pairs = sorted(set((q, c) for _, c, q in arcs))
    eps = {pc: nQ + i for i, pc in enumerate(pairs)}
    S = nQ + len(pairs)
    label = [0] * nQ + [c for _, c in pairs]
    classes = sorted(set(label[nQ:]))
    cls_at = {c: i for i, c in enumerate(classes)}
    slot = [0] * nQ + [1 + cls_at[c] for _, c in pairs]
    of = {}                                                   # DFA state -> its eps states as (label, state), ascending
    for pc in pairs:
        of.setdefault(pc[0], []).append((pc[1], eps[pc]))
    into = {}                                                 # (dst, label) -> the sources of its arcs
    for p, c, q in arcs:
        into.setdefault((q, c), []).append(p)
    ins = []
    for s in range(S):
        if s < nQ:
            src = [s] + [e for _, e in of.get(s, [])]
        else:
            q, c = pairs[s - nQ]
            src = [s]
            for p in into[(q, c)]:
                src.append(p)
                src += [e for c2, e in of.get(p, []) if c2 != c]
        assert len(src) == len(set(src))
        ins.append(sorted(src))
    fin = set(finals)
    accept = [q for q in range(nQ) if q in fin] + [eps[pc] for pc in pairs if pc[0] in fin]
    start = sorted(set([0] + [eps[(q, c)] for p, c, q in arcs if p == 0]))
    return {"state_label": np.array(label, np.int32), "state_slot": np.array(slot, np.int32),
            "in_ptr": np.concatenate([[0], np.cumsum([len(i) for i in ins])]).astype(np.int32),
            "in_src": np.array([v for i in ins for v in i], np.uint16), "classes": np.array(classes, np.int32),
            "accept": np.array(sorted(accept), np.int32), "start": np.array(start, np.int32), "nQ": nQ}


def logsumexp(r):
    r = np.asarray(r, np.float64)
    m = r.max() if r.size else -np.inf
    if m == -np.inf:
        return -np.inf
    return float(m + np.log(np.exp(r - m).sum()))


def recurse(lp, t):
    """(logp, best_logp, path) of one line: lp float64 [T][C] log-probabilities, t the tables. path = the class per
    column of the best accepted path under the tie rule (the first maximal source in edge order; the lowest accepting
    state), or None when no path of T columns is accepted."""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    label, ptr, src = t["state_label"].astype(np.int64), t["in_ptr"].astype(np.int64), t["in_src"].astype(np.int64)
    S = len(label)
    seg = np.repeat(np.arange(S), np.diff(ptr))
    a = np.full(S, -np.inf)
    a[t["start"]] = lp[0][label[t["start"]]]
    v = a.copy()
    bp = np.zeros((T, S), np.int64)
    bp[0] = np.arange(S)
    for k in range(1, T):
        av, vv = a[src], v[src]
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
    logp = logsumexp(a[acc])
    best = float(v[acc].max())
    if best == -np.inf:
        return logp, best, None
    s = int(acc[int(np.argmax(v[acc]))])                      # (argmax: the first, so the lowest state)
    path = []
    for k in range(T - 1, -1, -1):
        path.append(int(label[s]))
        s = int(bp[k][s])
    return logp, best, path[::-1]


def spans(path, lp):
    """(labels, starts, ends, float32 sums of lp over each run in ascending t) of a path"""
    labels, st, en, sums = [], [], [], []
    prev = 0
    for k, c in enumerate(path):
        if c != prev and prev != 0:
            en.append(k)
        if c != 0 and c != prev:
            labels.append(int(c))
            st.append(k)
            sums.append(np.float32(0))
        if c != 0:
            sums[-1] = np.float32(sums[-1] + np.float32(lp[k][c]))
        prev = c
    if prev != 0:
        en.append(len(path))
    return labels, st, en, sums


def run(logits, arcs, finals, num_states, input_lengths=None):
    """per line (logp, best_logp, path or None) for logits [W][B][C]"""
    logits = np.asarray(logits)
    W, B, _ = logits.shape
    t = tables(arcs, finals, num_states)
    out = []
    for b in range(B):
        T = W if input_lengths is None else int(input_lengths[b])
        out.append(recurse(log_softmax(logits[:T, b]), t))
    return out


def enumerate_paths(lp, arcs, finals):
    """(logp, best_logp, best path) by visiting every path of C^T (tiny cases only); ties in the best score are
    reported as the list of all best paths"""
    T, C = lp.shape
    total, best, best_paths = 0.0, -np.inf, []
    for path in itertools.product(range(C), repeat=T):
        if not accepts(arcs, finals, collapse(path)):
            continue
        s = float(sum(lp[k, c] for k, c in enumerate(path)))
        total += np.exp(s)
        if s > best + 1e-12:
            best, best_paths = s, [list(path)]
        elif abs(s - best) <= 1e-12:
            best_paths.append(list(path))
    with np.errstate(divide="ignore"):
        return float(np.log(total)), best, best_paths


# ---- automata used by several tests ----
def literal(text):
    return [(i, int(c), i + 1) for i, c in enumerate(text)], [len(text)], len(text) + 1


def trie(entries):
    """the DFA of a union of label sequences"""
    child, arcs, finals = {}, [], set()
    n = 1
    for e in entries:
        v = 0
        for c in e:
            if (v, int(c)) not in child:
                child[(v, int(c))] = n
                arcs.append((v, int(c), n))
                n += 1
            v = child[(v, int(c))]
        finals.add(v)
    return arcs, sorted(finals), n


def contains(q, C):
    """the DFA of "the text contains q" over labels 1..C-1: the KMP automaton of q with an absorbing final state"""
    q = [int(c) for c in q]
    L = len(q)
    arcs = []
    for j in range(L):
        for c in range(1, C):
            k = min(j + 1, L)
            seq = q[:j] + [c]
            while k > 0 and seq[len(seq) - k:] != q[:k]:
                k -= 1
            arcs.append((j, c, k))
    arcs += [(L, c, L) for c in range(1, C)]
    return arcs, [L], L + 1
