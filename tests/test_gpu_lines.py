"""GPU tests (-m gpu): a line in a batch gives the BYTES it gives alone.

Seed-0 synthetic checkpoint (dense weights, nothing exact), contrast batches (tests/line_cases.py; their host
precondition is tests/test_lines_host.py: every pair of lines has, in every block, a channel whose scales differ by
32 fp16 ulps or more). A line's result depends on nothing but its own pixels, its width and W (csrc/engine.cpp
run_passes says so and the several-pass tests rely on it), and no kernel adds up across lines, so the order of every
sum is the same in a batch as alone: logits, every readable buffer, the SE means and scales, the guard's figures, the
greedy labels and the beam front end's lists are compared with tobytes(). Anything per-line that is read from another
line - a scale, a mean, a tile sum, a guard margin, a row's top-2 - changes bits here. No tolerance anywhere.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import line_cases as lc
from test_gpu_exact import VARIANTS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def line_engines(pkg, state_dict):
    """the seed-0 synthetic checkpoint with a 202-class head, per precision"""
    sd = lc.head_202(state_dict)
    cache = {}

    def get(precision):
        if precision not in cache:
            m = pkg.hctr_model(202, precision=precision).cuda(0)
            m.load_state_dict(sd)
            cache[precision] = m.eval()
        return cache[precision]

    yield get
    cache.clear()


@pytest.mark.parametrize("precision", ["f16", "f16x3"])
@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_line_in_a_batch_equals_the_line_alone(line_engines, synth, case, precision):
    """Logits, the line's slice of all sixteen readable buffers and its SE means and scales of every block, in the
    batch as built, reversed and rotated by one, against the line alone at the same W (and width)."""
    B, W, widths = case
    model = line_engines(precision)
    x = lc.contrast_batch(synth, B, W)
    alone = lc.alone_snapshots(model, x, widths)
    for order in lc.orders(B):
        snap = lc.snapshot(model, x[order], None if widths is None else [widths[b] for b in order])
        diffs = lc.line_differences(snap, order, alone)
        assert not diffs, "order %s\n" % (order,) + "\n".join(diffs[:20])


@pytest.mark.parametrize("precision", ["f16", "f16x3"])
@pytest.mark.parametrize("case", [lc.CASES[1], lc.CASES[3], lc.CASES[4]], ids=lc.case_id)
def test_greedy_and_beam_front_end_per_line(line_engines, synth, case, precision):
    """The greedy labels and the fused beam front end's lists (k = 5: classes, log-probabilities, blank) of a line in
    the batch - as built, reversed, rotated - are those of the line alone."""
    B, W, widths = case
    model = line_engines(precision)
    x = lc.contrast_batch(synth, B, W)
    wd = (lambda idx: None) if widths is None else (lambda idx: [widths[b] for b in idx])
    lab1 = [model.greedy(x[b:b + 1], widths=wd([b]))[0] for b in range(B)]
    fe1 = [model.beam_frontend(x[b:b + 1], k=5, widths=wd([b])) for b in range(B)]
    for order in lc.orders(B):
        lab = model.greedy(x[order], widths=wd(order))
        fe = model.beam_frontend(x[order], k=5, widths=wd(order))
        for i, b in enumerate(order):
            assert lab[i].tobytes() == lab1[b].tobytes(), (order, b, lab[i].tolist(), lab1[b].tolist())
            for key in ("topk_idx", "topk_logp", "blank_logp"):
                assert fe[key][:, i].tobytes() == fe1[b][key][:, 0].tobytes(), (order, b, key)


def test_auto_mode_flags_and_margins_per_line(line_engines, synth):
    """Auto mode with a guard cut between two lines' smallest margins (chosen as
    test_gpu_auto.py::test_partly_flagged_batch_in_several_passes_equals_one_pass does), so that some lines but not all
    run again in f16x3: each line's flag, min_margin and logits are those of the line alone under the same cut."""
    B, W, widths = lc.CASES[3]
    model = line_engines("auto")
    x = lc.contrast_batch(synth, B, W)
    try:
        model(x)
        mg = np.sort(model.last_guard()["min_margin"].astype(np.float64))
        gaps = [i for i in range(B - 1) if mg[i] < 0.5 * (mg[i] + mg[i + 1]) < mg[i + 1]]
        assert gaps, mg.tolist()
        cut = 0.5 * (mg[gaps[len(gaps) // 2]] + mg[gaps[len(gaps) // 2] + 1])
        model.set_guard(0.0, cut / 2)                       # flagged unless min_margin > cut
        alone = []
        for b in range(B):
            lg = model(x[b:b + 1])
            g = model.last_guard()
            alone.append((lg[:, 0].copy(), int(g["flags"][0]), g["min_margin"][0]))
        for order in lc.orders(B):
            lg = model(x[order])
            g = model.last_guard()
            assert g["lines"] == B and 0 < g["flagged"] < B, (g["flagged"], mg.tolist(), cut)
            for i, b in enumerate(order):
                assert int(g["flags"][i]) == alone[b][1], (order, b)
                assert g["min_margin"][i].tobytes() == alone[b][2].tobytes(), (order, b)
                assert lg[:, i].tobytes() == alone[b][0].tobytes(), (order, b)
    finally:
        model.set_guard()


@pytest.mark.parametrize("env", VARIANTS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_kernel_families_line_by_line(env):
    """The f16 comparison at B = 3, W = 33 in every kernel family: one child per variant (tests/lines_child.py), one
    after the other. The generic family with the fusions off pins se_apply, HCTR_PERSIST=2 the tile queue that walks
    tiles of several lines."""
    from conftest import ROOT
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lines_child.py")], env=e, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
