"""Float64 restatement of lexicon recognition as include/hctr_hip.h defines it (hctr_lexicon*): the trie of a lexicon,
the CTC forward recursion over it with two states per node, the partition into units, and the ranking. Plain numpy and
Python; tests/test_lexicon_host.py checks it against enumeration of all paths and against torch's float64 ctc_loss.
"""
import itertools

import numpy as np

MAX_LEN = 64
DEFAULT_UNIT = 4096
SKIP, FIRST, PARENT_MASK = 1 << 30, 1 << 29, 0xFFFF


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


def build_trie(entries):
    """(parent, label, entry_node): node 0 is the root, the others are numbered in the order in which inserting entry
    0, 1, .. first reaches them"""
    parent, label, child, entry_node = [-1], [0], {}, []
    for e in entries:
        v = 0
        for c in e:
            key = (v, int(c))
            if key not in child:
                child[key] = len(parent)
                parent.append(v)
                label.append(int(c))
            v = child[key]
        entry_node.append(v)
    return np.array(parent, np.int64), np.array(label, np.int64), np.array(entry_node, np.int64)


def _logadd3(a, b, c):
    with np.errstate(invalid="ignore"):
        return np.logaddexp(np.logaddexp(a, b), c)


def forward(lp, parent, label):
    """(a_n, a_b) float64 [nodes] after the T columns of lp [T][C] (log-probabilities): the recursion over any table of
    nodes in which node 0 is the root and parent[v] indexes the same table"""
    lp = np.asarray(lp, np.float64)
    nn = len(parent)
    par = np.where(np.arange(nn) == 0, 0, parent)
    first = (par == 0) & (np.arange(nn) != 0)
    skip = (par != 0) & (label[par] != label)
    ninf = np.full(nn, -np.inf)
    a_n = np.where(first, lp[0][label], -np.inf)
    a_b = ninf.copy()
    a_b[0] = lp[0][0]
    for t in range(1, lp.shape[0]):
        n1 = _logadd3(a_n, a_b[par], np.where(skip, a_n[par], -np.inf)) + lp[t][label]
        b1 = np.logaddexp(a_b, a_n) + lp[t][0]
        n1[0] = -np.inf
        a_n, a_b = n1, b1
    return a_n, a_b


def scores(logits, entries, input_lengths=None):
    """float64 [B][N]: log p(entry | line) for logits [W][B][C]"""
    logits = np.asarray(logits)
    W, B, _ = logits.shape
    parent, label, entry_node = build_trie(entries)
    out = np.empty((B, len(entries)))
    for b in range(B):
        T = W if input_lengths is None else int(input_lengths[b])
        a_n, a_b = forward(log_softmax(logits[:T, b]), parent, label)
        out[b] = np.logaddexp(a_b, a_n)[entry_node]
    return out


def enumerate_scores(lp, entries):
    """log p(entry | line) by adding up every path of C^T (tiny cases only)"""
    T, C = lp.shape
    mass = {}
    for path in itertools.product(range(C), repeat=T):
        key = tuple(collapse(path))
        mass[key] = mass.get(key, 0.0) + float(np.exp(sum(lp[t, c] for t, c in enumerate(path))))
    with np.errstate(divide="ignore"):
        return np.array([np.log(mass.get(tuple(int(c) for c in e), 0.0)) for e in entries])


def fits(entry, T):
    """L + adjacent equal labels <= T"""
    e = list(entry)
    return len(e) + sum(1 for a, b in zip(e, e[1:]) if a == b) <= T


def partition(parent, label, cap=DEFAULT_UNIT):
    """the units of the trie: a list of (nodes, owned) per unit, nodes = the trie nodes of the unit's local nodes (0
    first), owned = a flag per local node. The rule of include/hctr_hip.h, in plain Python."""
    nn = len(parent)
    kids = [[] for _ in range(nn)]
    depth, size = [0] * nn, [1] * nn
    for v in range(1, nn):
        kids[parent[v]].append(v)
        depth[v] = depth[parent[v]] + 1
    for v in range(nn - 1, 0, -1):
        size[parent[v]] += size[v]
    for k in kids:
        k.sort(key=lambda v: label[v])
    units, cur, own, inside = [], [0], [0], {0}

    def close():
        nonlocal cur, own, inside
        if len(cur) > 1:
            units.append((cur, own))
        cur, own, inside = [0], [0], {0}

    def chain(v):
        c, p = [], parent[v]
        while p > 0 and p not in inside:
            c.append(p)
            p = parent[p]
        return c[::-1]

    def add(v, o):
        cur.append(v)
        own.append(o)
        inside.add(v)

    def room(v, n):
        if len(cur) + len(chain(v)) + n > cap:
            close()
        for p in chain(v):
            add(p, 0)

    def pack(v):
        if 1 + (depth[v] - 1) + size[v] <= cap:
            room(v, size[v])
            stack = [v]
            while stack:
                g = stack.pop()
                add(g, 1)
                stack.extend(reversed(kids[g]))
            return
        room(v, 1)
        add(v, 1)
        for k in kids[v]:
            pack(k)

    for k in kids[0]:
        pack(k)
    close()
    return units


def rank(scores_b, prior, n):
    """(top_entry [n], top_rank [n], log_total, count) of one line: rank = score + prior, descending, ties to the lower
    index, -inf left out"""
    r = np.asarray(scores_b, np.float64) + (0.0 if prior is None else np.asarray(prior, np.float64))
    order = [int(e) for e in np.argsort(-r, kind="stable") if r[e] != -np.inf][:n]
    top = np.full(n, -1, np.int64)
    top[:len(order)] = order
    tr = np.full(n, -np.inf)
    tr[:len(order)] = r[order]
    return top, tr, logsumexp(r), len(order)


def logsumexp(r):
    r = np.asarray(r, np.float64)
    m = r.max() if r.size else -np.inf
    if m == -np.inf:
        return -np.inf
    return float(m + np.log(np.exp(r - m).sum()))
