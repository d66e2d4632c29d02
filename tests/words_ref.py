"""Float64 restatement of word-sequence recognition as include/hctr_hip.h defines it (hctr_words*): the word tables of
a lexicon's trie, token passing over the looped trie with origins and the two exit records per column, the walk back, a
brute force over all paths and segmentations, and the score of a given segmentation (the tests' sandwich). Plain numpy
and Python; tests/test_words_host.py checks the recursion against the brute force.
"""
import itertools

import numpy as np

from lexicon_ref import build_trie, collapse, log_softmax  # noqa: F401

SKIP, FIRST, PARENT_MASK = 1 << 30, 1 << 29, 0xFFFF
MAX_NODES, LDS_NODES = 65536, 4096


def word_tables(entries, priors=None, word_bonus=0.0):
    """dict: node (parent | SKIP | FIRST), slot, entry (e_v or -1), weight (x_v, float32), classes (0, then the distinct
    labels ascending) - what hctr_lex_word_tables exports"""
    parent, label, entry_node = build_trie(entries)
    nn = len(parent)
    classes = np.array([0] + sorted(set(int(c) for c in label[1:])), np.int64)
    pr = np.zeros(len(entries), np.float32) if priors is None else np.asarray(priors, np.float32)
    node, slot = np.zeros(nn, np.int64), np.zeros(nn, np.int64)
    for v in range(1, nn):
        p = int(parent[v])
        node[v] = p | (FIRST if p == 0 else SKIP if label[p] != label[v] else 0)
        slot[v] = int(np.searchsorted(classes, label[v]))
    entry = np.full(nn, -1, np.int64)
    for e, v in enumerate(entry_node):
        if entry[v] < 0 or pr[e] > pr[entry[v]]:
            entry[v] = e
    weight = np.zeros(nn, np.float32)
    ends = entry >= 0
    weight[ends] = (pr[entry[ends]].astype(np.float64) + np.float64(np.float32(word_bonus))).astype(np.float32)
    return {"node": node, "slot": slot, "entry": entry, "weight": weight, "classes": classes}


NONE = (-np.inf, 0x7FFFFFFF, -1, 0)          # an absent record: (score, node, last, origin)


def _best(score, node, last, origin):
    """the best candidate by (score descending, last == 0 first, node ascending), or NONE"""
    if score.size == 0:
        return NONE
    m = score.max()
    if not m > -np.inf:
        return NONE
    i = np.flatnonzero(score == m)
    if i.size > 1:
        z = last[i] == 0
        if z.any():
            i = i[z]
        i = i[np.argsort(node[i], kind="stable")]
    i = int(i[0])
    return (score[i], int(node[i]), int(last[i]), int(origin[i]))


def records(n, b, on, ob, ends, x, slot):
    """(R1, R2) of the states after a column; `last` is the emission slot of the label (0 = the blank state)"""
    score = np.concatenate([n[ends] + x, b[ends] + x])
    node = np.concatenate([ends, ends])
    last = np.concatenate([slot[ends], np.zeros(len(ends), np.int64)])
    origin = np.concatenate([on[ends], ob[ends]])
    r1 = _best(score, node, last, origin)
    keep = last != r1[2]
    return r1, _best(score[keep], node[keep], last[keep], origin[keep])


def decode(emis, tab, dtype=np.float64):
    """(score, words, starts, recs) of one line: emis [T][D] are the log-probabilities of the table's classes, column 0
    the blank. The recursion of include/hctr_hip.h in `dtype`; an origin is s * 4 + k."""
    emis = np.asarray(emis, dtype)
    T = emis.shape[0]
    node, slot = np.asarray(tab["node"], np.int64), np.asarray(tab["slot"], np.int64)
    nn = len(node)
    par = node & PARENT_MASK
    par[0] = 0
    first, skip = (node & FIRST) != 0, (node & SKIP) != 0
    ends = np.flatnonzero(np.asarray(tab["entry"]) >= 0)
    x = np.asarray(tab["weight"], np.float32)[ends].astype(dtype)
    ninf = dtype(-np.inf)
    n = np.where(first, emis[0][slot], ninf).astype(dtype)
    b = np.full(nn, ninf, dtype)
    b[0] = emis[0][0]
    on, ob = np.zeros(nn, np.int64), np.zeros(nn, np.int64)
    recs = [records(n, b, on, ob, ends, x, slot)]
    for t in range(1, T):
        r1, r2 = recs[-1]
        pb, pob = b[par], np.where(first, t * 4, ob[par])
        one = slot != r1[2]
        third = np.where(first, np.where(one, dtype(r1[0]), dtype(r2[0])), np.where(skip, n[par], ninf))
        third_o = np.where(first, t * 4 + np.where(one, 1, 2), on[par])
        m, o = n.copy(), on.copy()
        g = pb > m
        m, o = np.where(g, pb, m), np.where(g, pob, o)
        g = third > m
        m, o = np.where(g, third, m), np.where(g, third_o, o)
        n1 = (m + emis[t][slot]).astype(dtype)
        n1[0] = ninf
        g = n > b
        b1 = (np.where(g, n, b) + emis[t][0]).astype(dtype)
        ob1 = np.where(g, on, ob)
        n, b, on, ob = n1, b1, o, ob1
        recs.append(records(n, b, on, ob, ends, x, slot))
    r = recs[T - 1][0]
    words, starts = [], []
    while r[0] > -np.inf:
        s, k = r[3] >> 2, r[3] & 3
        words.append(int(tab["entry"][r[1]]))
        starts.append(int(s))
        if k == 0:
            break
        r = recs[s - 1][k - 1]
    return float(recs[T - 1][0][0]), words[::-1], starts[::-1], recs


def emissions(z, classes, dtype=np.float64):
    """[T][D]: the log-softmax of z [T][C] at the table's classes; float32 rounds the float64 value once, as ctc_lse"""
    return log_softmax(z)[:, np.asarray(classes, np.int64)].astype(dtype)


def words(logits, entries, priors=None, word_bonus=0.0, input_lengths=None):
    """per line of logits [W][B][C]: (score, words, starts) in float64"""
    logits = np.asarray(logits)
    W, B, _ = logits.shape
    tab = word_tables(entries, priors, word_bonus)
    out = []
    for b in range(B):
        T = W if input_lengths is None else int(input_lengths[b])
        out.append(decode(emissions(logits[:T, b], tab["classes"]), tab)[:3])
    return out


def best_weights(entries, priors=None, word_bonus=0.0):
    """text (tuple) -> float64(float32(best prior + bonus))"""
    pr = np.zeros(len(entries), np.float32) if priors is None else np.asarray(priors, np.float32)
    best = {}
    for e, p in zip(entries, pr):
        k = tuple(int(c) for c in e)
        best[k] = max(best.get(k, -np.inf), float(p))
    return {k: float(np.float32(np.float64(np.float32(p)) + np.float64(np.float32(word_bonus)))) for k, p in best.items()}


def brute_force(lp, entries, priors=None, word_bonus=0.0):
    """max over the C^T paths and the segmentations of their collapsed text into >= 1 entries of the path's
    log-probability + the sum of the words' weights (tiny cases only); -inf when no path has one"""
    T, C = lp.shape
    wt = best_weights(entries, priors, word_bonus)
    seg_cache = {}

    def seg(text):
        """the best sum of weights over the segmentations of text into entries, -inf if none (the empty text: 0)"""
        if text not in seg_cache:
            best = 0.0 if not text else -np.inf
            for k in range(1, len(text) + 1):
                if text[:k] in wt:
                    best = max(best, wt[text[:k]] + seg(text[k:]))
            seg_cache[text] = best
        return seg_cache[text]

    best = -np.inf
    for path in itertools.product(range(C), repeat=T):
        text = tuple(collapse(path))
        if not text:
            continue
        w = seg(text)
        if w > -np.inf:
            best = max(best, float(sum(lp[t, c] for t, c in enumerate(path))) + w)
    return best


def segmentation_score(lp, entry_labels, weights, starts, T):
    """The float64 score of a given segmentation: the best path of lp [T][C] that emits blanks before starts[0], first
    emits word j's first label at column starts[j] exactly, and reads the words in order (the CTC rule for equal adjacent
    labels holds across the boundaries as inside a word), plus the words' weights. -inf if there is none or no word."""
    if not entry_labels:
        return -np.inf
    text, first_at = [], {}
    for j, e in enumerate(entry_labels):
        first_at[2 * len(text) + 1] = int(starts[j])
        text += [int(c) for c in e]
    ext = [0]
    for c in text:
        ext += [c, 0]
    ext = np.array(ext, np.int64)
    S = len(ext)
    gate = np.full(S, -1, np.int64)
    for s, g in first_at.items():
        gate[s] = g
    skip = np.zeros(S, bool)
    skip[2:] = (ext[2:] != 0) & (ext[2:] != ext[:-2])
    lp = np.asarray(lp, np.float64)
    a = np.full(S, -np.inf)
    a[0] = lp[0][0]
    if gate[1] == 0:
        a[1] = lp[0][ext[1]]
    ninf = np.full(S, -np.inf)
    for t in range(1, T):
        stay = np.where((gate < 0) | (t > gate), a, ninf)
        from1, from2 = ninf.copy(), ninf.copy()
        from1[1:] = a[:-1]
        from2[2:] = np.where(skip[2:], a[:-2], -np.inf)
        enter = np.where((gate < 0) | (t == gate), np.maximum(from1, from2), ninf)
        a = np.maximum(stay, enter) + lp[t][ext]
    end = max(a[S - 1], a[S - 2])
    return float(end + sum(float(w) for w in weights)) if end > -np.inf else -np.inf
