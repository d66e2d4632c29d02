"""numpy restatement of the edit distance the engine computes (include/hctr_hip.h, hctr_edit_distance / hctr_evaluate*),
the yardstick of tests/test_edit_host.py and tests/test_gpu_evaluate.py. Integers throughout: everything compares with ==.

For a reference r_1..r_L and a hypothesis h_1..h_H:
    D[i][0] = i, D[0][j] = j, D[i][j] = min(D[i-1][j-1] + (r_i != h_j), D[i-1][j] + 1, D[i][j-1] + 1)
and the path walked back from (L, H): the diagonal first, then the deletion, then the insertion.

The row sweep is vectorised: with a_j = min(D[i-1][j-1] + neq_j, D[i-1][j] + 1) the in-row dependency
D[i][j] = min(a_j, D[i][j-1] + 1) unrolls to D[i][j] = min_{k <= j} (a_k + j - k) = j + min.accumulate(a - j), where a_0 = i.
"""
import numpy as np


def table(ref, hyp):
    """D int32 [L + 1, H + 1]"""
    r = np.asarray(ref, np.int64).reshape(-1)
    h = np.asarray(hyp, np.int64).reshape(-1)
    L, H = r.size, h.size
    D = np.empty((L + 1, H + 1), np.int32)
    j = np.arange(H + 1, dtype=np.int32)
    D[0] = j
    a = np.empty(H + 1, np.int32)
    for i in range(1, L + 1):
        prev = D[i - 1]
        a[0] = i
        np.minimum(prev[:-1] + (h != r[i - 1]), prev[1:] + 1, out=a[1:])
        D[i] = np.minimum.accumulate(a - j) + j
    return D


def align(ref, hyp):
    """(edits, counts [4] = hits, substitutions, deletions, insertions, ref_map [L], hyp_map [H])"""
    r = np.asarray(ref, np.int64).reshape(-1)
    h = np.asarray(hyp, np.int64).reshape(-1)
    D = table(r, h)
    i, j = r.size, h.size
    ref_map = np.full(i, -1, np.int32)
    hyp_map = np.full(j, -1, np.int32)
    hits = subs = dels = ins = 0
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i, j] == D[i - 1, j - 1] + (r[i - 1] != h[j - 1]):
            if r[i - 1] == h[j - 1]:
                hits += 1
            else:
                subs += 1
            ref_map[i - 1], hyp_map[j - 1] = j - 1, i - 1
            i, j = i - 1, j - 1
        elif i > 0 and D[i, j] == D[i - 1, j] + 1:
            dels += 1
            i -= 1
        else:
            ins += 1
            j -= 1
    return int(D[-1, -1]), np.array([hits, subs, dels, ins], np.int32), ref_map, hyp_map


def batch(hyp, hyp_lengths, ref, ref_lengths):
    """the C ABI's outputs for hyp [B, stride] / hyp_lengths [B] and concatenated ref / ref_lengths [B]:
    dict(edits [B], counts [B, 4], ref_map [sum L], hyp_map [B, stride] with zeros past a line's length)"""
    hyp = np.asarray(hyp, np.int32)
    B, stride = hyp.shape
    off = np.concatenate([[0], np.cumsum(np.asarray(ref_lengths, np.int64))])
    ref = np.asarray(ref, np.int32).reshape(-1)
    out = {"edits": np.zeros(B, np.int32), "counts": np.zeros((B, 4), np.int32),
           "ref_map": np.zeros(int(off[-1]), np.int32), "hyp_map": np.zeros((B, stride), np.int32)}
    for b in range(B):
        n = int(hyp_lengths[b])
        e, c, rm, hm = align(ref[off[b]:off[b + 1]], hyp[b, :n])
        out["edits"][b], out["counts"][b] = e, c
        out["ref_map"][off[b]:off[b + 1]] = rm
        out["hyp_map"][b, :n] = hm
    return out


def skewed(ref, hyp, NS):
    """D[L][H] by the engine's schedule, step by step: lane k owns rows k*NS+1 .. k*NS+NS, works at step d on column
    d - k + 1 and takes the row above its first from what lane k-1 finished a step earlier."""
    r = np.asarray(ref, np.int64).reshape(-1)
    h = np.asarray(hyp, np.int64).reshape(-1)
    L, H = r.size, h.size
    if L == 0 or H == 0:
        return max(L, H)
    lanes = (L + NS - 1) // NS
    left = [[k * NS + i + 1 for i in range(NS)] for k in range(lanes)]
    diag0 = [k * NS for k in range(lanes)]
    for d in range(H + lanes - 1):
        bottom = [row[NS - 1] for row in left]               # what every lane published a step earlier
        for k in range(lanes):
            j = d - k + 1
            if not 1 <= j <= H:
                continue
            top = j if k == 0 else bottom[k - 1]
            up, dg = top, diag0[k]
            for i in range(NS):
                row = k * NS + i + 1
                neq = int(row > L or r[row - 1] != h[j - 1])
                v = min(dg + neq, up + 1, left[k][i] + 1)
                dg, left[k][i], up = left[k][i], v, v
            diag0[k] = top
    return left[(L - 1) // NS][(L - 1) % NS]
