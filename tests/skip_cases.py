"""Seeded inputs shared by tests/test_skip_beam_host.py and tests/test_gpu_nbest_skip.py: float32 log-prob tensors whose
columns are "certain" (one class above probability 0.001: an in-place step of the skip search) or "open" (several), and
the crafted lines of the duplicate and in-place-branch cases. Labels stand for themselves (tests/lm_beam_ref.py)."""
import numpy as np
from scipy.special import log_softmax

FLOOR = np.float32(-12.0)                           # logit of a class that is no candidate


def logp_of(z):
    return log_softmax(np.asarray(z, np.float32), axis=2).astype(np.float32)


def certain(z, t, b, c, rng=None):
    z[t, b, c] = np.float32(12.0 + (4.0 * rng.rand() if rng is not None else 0.0))


def offer(z, t, b, classes, rng):
    """an open column: the classes get comparable logits, so all of them are candidates"""
    for c in classes:
        z[t, b, c] = np.float32(3.0 * rng.rand())


def mixed_lines(seed, T, B, C, p_certain=0.6, max_open=6):
    """Lines in the manner of codec_cases.gen_logits(style="mixed"): a current label that moves, goes blank or (rarely)
    <unknown>; certain columns interleaved with open ones of 2 .. max_open candidates (the current label among them).
    Returns float32 logits [T, B, C]."""
    rng = np.random.RandomState(seed)
    z = np.full((T, B, C), FLOOR, np.float32) + rng.rand(T, B, C).astype(np.float32)
    for b in range(B):
        cur = 1 + rng.randint(C - 2)
        for t in range(T):
            r = rng.rand()
            if r < 0.35:
                cur = rng.randint(C)
            elif r < 0.55:
                cur = 0
            elif r < 0.58:
                cur = C - 1
            if rng.rand() < p_certain:
                certain(z, t, b, cur, rng)
            else:
                others = rng.choice(C, size=rng.randint(1, max_open), replace=False)
                offer(z, t, b, sorted(set([cur] + others.tolist())), rng)
    return z


def quiet_tail(z, b, start):
    """nothing but certain blanks from column ``start`` on: the line's text ends there"""
    z[start:, b, :] = FLOOR
    z[start:, b, 0] = np.float32(12.0)


def duplicate_line(seed, T=24, C=6):
    """The duplicate case: columns 0-2 offer {blank, a}, column 3 is a certain a - the list then holds "aa" twice, from
    "a" (pb finite) and from "aa" (pb = -inf) -, columns 4-10 alternate two-candidate columns with certain ones over
    a b c, the rest is seeded up to the last four columns, which repeat the opening so that the line ENDS on an in-place
    step that doubles a text. a, b, c = classes 1, 2, 3. Returns float32 logits [T, 1, C]."""
    rng = np.random.RandomState(100 + seed)
    z = np.full((T, 1, C), FLOOR, np.float32) + rng.rand(T, 1, C).astype(np.float32)
    for t in range(3):
        offer(z, t, 0, [0, 1], rng)
    certain(z, 3, 0, 1)
    pairs = [(1, 2), (2, 3), (0, 1), (1, 3)]
    for t in range(4, 11):
        if t % 2 == 0:
            offer(z, t, 0, pairs[(t // 2) % 4], rng)
        else:
            certain(z, t, 0, 1 + (t // 2) % 3)
    for t in range(11, T - 4):
        if rng.rand() < 0.5:
            certain(z, t, 0, rng.randint(0, 4))
        else:
            offer(z, t, 0, sorted(rng.choice(4, size=2, replace=False).tolist()), rng)
    for t in range(T - 4, T - 1):                   # the opening once more at the end: the final list holds a text twice
        offer(z, t, 0, [0, 1], rng)
    z[T - 2, 0, 0] = max(z[T - 2, 0, 0], z[T - 2, 0, 1] + np.float32(0.5))      # (the greedy line keeps the last a)
    certain(z, T - 1, 0, 1)
    return z


def branch_line(T=12, C=6):
    """The in-place branches on a list of several hypotheses. Columns 0-1 offer {blank, a, b}: the list holds "", "a",
    "b", "ab", "ba", ... with pb and pnb finite. Column 2, a certain a: "b" takes branch 2 (append, c != tail), "a" with
    pb finite branch 3 (append the repeat). Column 3, a certain a again: every text now ends in a with pb = -inf -
    branch 4, which reads the row's blank log-prob though the blank is no candidate. Column 4, a certain blank: branch
    1. Then an open column, so a ranked step follows, and a certain tail. Returns float32 logits [T, 1, C]."""
    rng = np.random.RandomState(5)
    z = np.full((T, 1, C), FLOOR, np.float32) + rng.rand(T, 1, C).astype(np.float32)
    offer(z, 0, 0, [0, 1, 2], rng)
    offer(z, 1, 0, [0, 1, 2], rng)
    certain(z, 2, 0, 1)
    certain(z, 3, 0, 1)
    certain(z, 4, 0, 0)
    offer(z, 5, 0, [1, 3], rng)
    for t in range(6, T):
        certain(z, t, 0, [2, 2, 0, 3, 3, 1][(t - 6) % 6])
    return z
