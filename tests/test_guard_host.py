"""CPU side of tests/test_gpu_guard.py: each quantity that file asserts on the engine, stated on the two CPU oracles.

oracle.hctr_ref.forward is fp32; forward_f16 carries the engine's rounding points and differs from the engine only in
fp32 summation order. On the checkpoints and batches of tests/guard_cases.py:
  * the lines the GPU test expects unflagged / flagged (guard_cases.SOLID_CERTAIN / SOLID_UNCERTAIN) are exactly the
    rounding oracle's solidly certain / uncertain ones at the engine's default criterion, and there are enough of each
    kind, in the places where they are hard to come by, for the GPU check to mean something;
  * the certificate's premise holds in the oracle pair: every rounding-oracle logit of a line is within
    GUARD_REL * (that line's max |logit|) + GUARD_ABS of the fp32 one;
  * the trunk variant's activations stay far inside fp16's range.
"""
import numpy as np
import pytest

import guard_cases as gc


@pytest.fixture(scope="module")
def figures(synth, state_dict):
    """{(checkpoint, batch): (rounding-oracle logits' min margins, their scales, max |l16 - l32|)} per line, and the
    largest |activation| among the fp32 oracle's taps of the trunk variant"""
    cache, out, tap_max = {}, {}, 0.0
    for ck, bt in gc.pairs():
        taps = {} if gc.trunk_of(ck) != "seed0" else None
        l32 = gc.host_logits32(ck, bt, state_dict, synth, cache, taps)
        l16 = gc.host_logits16(ck, bt, state_dict, synth, cache)
        if taps:
            tap_max = max([tap_max] + [float(v.abs().max()) for v in taps.values()])
        mg, sc = gc.line_figures(l16)
        out[(ck, bt)] = (mg.astype(np.float64), sc.astype(np.float64), np.abs(l16 - l32).max(axis=(0, 2)).astype(np.float64))
    return out, tap_max


def test_exported_populations_are_the_rounding_oracles(figures):
    fig, _ = figures
    certain, uncertain = {}, {}
    for key, (mg, sc, _) in fig.items():
        c, u = gc.populations(mg, sc)
        if c:
            certain[key] = c
        if u:
            uncertain[key] = u
    assert certain == gc.SOLID_CERTAIN
    assert uncertain == gc.SOLID_UNCERTAIN


def test_enough_certain_and_uncertain_lines_where_they_are_scarce():
    n = {key: len(v) for key, v in gc.SOLID_CERTAIN.items()}
    assert sum(n.values()) >= 40
    assert sum(v for (ck, _), v in n.items() if ck == "c7358") >= 3
    hard = 0
    for (ck, bt), v in n.items():
        _, C, s, _ = gc.CHECKPOINTS[ck]
        if s != 1.0 or (C >= 202 and gc.BATCHES[bt][2] >= 33):
            hard += v
    assert hard >= 8, hard
    assert sum(len(v) for v in gc.SOLID_UNCERTAIN.values()) >= 20
    # every checkpoint's context has certain lines to check the consequence on
    assert {ck for ck, _ in gc.SOLID_CERTAIN} == set(gc.CHECKPOINTS)


def test_premise_holds_in_the_oracle_pair_for_every_line(figures):
    fig, _ = figures
    bad, worst = [], {}
    for (ck, bt), (_, sc, err) in fig.items():
        tol = gc.GUARD_REL * sc + gc.GUARD_ABS
        w = worst.setdefault(ck, [0.0, 0.0])
        w[0], w[1] = max(w[0], float((err / sc).max())), max(w[1], float((err / tol).max()))
        bad += [(ck, bt, int(b), float(err[b] / tol[b])) for b in np.flatnonzero(~(err <= tol))]
    for ck, (r, t) in worst.items():
        print("%-10s worst err / scale_line %.5f, worst err / tol %.3f" % (ck, r, t))
    assert not bad, "(checkpoint, batch, line, err / tol): %r" % (bad,)


def test_trunk_variant_stays_inside_fp16_range(figures):
    _, tap_max = figures
    print("largest |activation| of the fp32 oracle's taps, %s x %g: %.1f" % (gc.TRUNK_BN, gc.TRUNK_BN_FACTOR, tap_max))
    assert 0.0 < tap_max < gc.TAP_LIMIT
