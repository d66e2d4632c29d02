"""Host checks (no GPU) of tests/nbest_ref.py, the float64 yardstick of the device prefix beam search: what it returns
is the probability of each text when nothing is cut, and its 1-best is the reference's full search when it is given the
reference's end step."""
import itertools

import numpy as np
import pytest
import torch

import nbest_ref as nr
from oracle.ctc_ref import CtcCodecRef, ZeroLM


def _collapse(path):
    out, prev = [], 0
    for c in path:
        if c != 0 and c != prev:
            out.append(c)
        prev = c
    return tuple(out)


@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("style", ["flat", "peaky"])
def test_uncut_search_sums_all_alignments(T, style):
    """k = C, two usable labels, T <= 4: at most 1 + 2 + 4 + 8 + 16 = 31 prefixes exist, so beam = 32 never cuts and
    every returned logp is the log of the summed probability of ALL alignments of its text - the brute-force sum, and
    -ctc_loss in float64 - to 1e-12"""
    C, beam = 4, 32
    rng = np.random.RandomState(10 * T + len(style))
    z = rng.standard_normal((T, 1, C)).astype(np.float32) * (1.0 if style == "flat" else 4.0)
    idx, lp = nr.topk_lists(z, C)
    full = np.zeros((T, C), np.float64)
    full[np.arange(T)[:, None], idx[:, 0]] = lp[:, 0].astype(np.float64)
    hyps, _ = nr.search_line(idx[:, 0], lp[:, 0], C, beam, beam)
    brute = {}
    for path in itertools.product(range(C - 1), repeat=T):
        p = float(sum(full[t, c] for t, c in enumerate(path)))
        key = _collapse(path)
        brute[key] = np.logaddexp(brute.get(key, -np.inf), p)
    assert len(hyps) == sum(2 ** n for n in range(T + 1))            # every text of length <= T is an entry
    assert {tuple(h["labels"]) for h in hyps if h["logp"] > -np.inf} == set(brute)
    for h in hyps:
        lab = tuple(h["labels"])
        want = float(brute.get(lab, -np.inf))
        loss = torch.nn.functional.ctc_loss(torch.from_numpy(full).unsqueeze(1), torch.tensor([list(lab)], dtype=torch.long),
                                            torch.tensor([T]), torch.tensor([len(lab)]), blank=0, reduction="none")
        if want == -np.inf:
            assert h["logp"] == -np.inf and float(loss) == np.inf, lab
            continue
        assert abs(h["logp"] - want) <= 1e-12 * max(1.0, abs(want)), (lab, h["logp"], want)
        assert abs(h["logp"] + float(loss)) <= 1e-12 * max(1.0, abs(want)), (lab, h["logp"], float(loss))
    tot = [h["score"] for h in hyps]
    assert tot == sorted(tot, reverse=True)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_one_best_is_the_reference_full_search(seed):
    """input_lengths = the reference's end_step, len_bonus 5.8, 10/10: the 1-best is beam_full_from_topk's text"""
    W, B, C, k, beam = 60, 4, 30, 10, 10
    rng = np.random.RandomState(seed)
    z = nr.planted_lines(rng, W, B, C, density=0.35, boost=6.0)
    idx, lp = nr.topk_lists(z, k)
    codec = CtcCodecRef("".join(chr(nr.BASE + c) for c in range(1, C - 1)))
    codec.ngram, codec.use_tfm_pred, codec.use_tfm_score = ZeroLM(), False, False
    codec.search_depth, codec.beam_size, codec.len_bonus = k, beam, 5.8
    want = codec.beam_full_from_topk(idx, lp)
    ends = []
    for b in range(B):
        top_line = codec._top_line(idx[:, b, 0])
        assert top_line, "planted lines have a greedy text"
        ends.append(codec._end_step(top_line, W))
    labels, lengths, logp, score, count, _, _ = nr.search(idx, lp, C, beam, 1, 5.8, ends)
    assert (count == 1).all()
    got = ["".join(chr(nr.BASE + c) for c in labels[b, 0, :lengths[b, 0]]) for b in range(B)]
    assert got == want and any(len(t) for t in got)
    assert (score[:, 0] == logp[:, 0] + lengths[:, 0] * 5.8).all()


def test_degenerate_rows():
    """k = 1: a step whose only class is <unknown> empties the list for good; blank-only rows keep the empty text"""
    C = 5
    idx = np.array([[0], [4], [0]], np.int32)
    lp = np.array([[-0.5], [-0.25], [-0.125]], np.float32)
    hyps, _ = nr.search_line(idx, lp, C, 4, 4)
    assert hyps == []
    hyps, _ = nr.search_line(idx[[0, 2]], lp[[0, 2]], C, 4, 4)
    assert len(hyps) == 1 and hyps[0]["labels"] == [] and hyps[0]["logp"] == -0.625 and hyps[0]["pnb"] == -np.inf
