"""Host tests (no GPU) of the LM weight sweep's fixture and of its host-side parts: the fixture of tests/lm_sweep_ref.py
is not vacuous by the yardstick alone; ``LMSweepTotals.best()`` applies the reference's rule (test.py:364-378: start
from min_cer = 1.0, min_params = (0, 0), replace only on strictly smaller) and ``report()`` yields the reference loop's
prints, whose strings are written out below; ``test.py --device-sweep`` refuses every option it does not serve.
"""
import importlib
import importlib.util
import os
import sys

import numpy as np
import pytest

import lm_sweep_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctc(pkg):
    return importlib.import_module(pkg.__name__ + ".ctc")


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("lm_sweep_host")


def sweep_of(ctc, grid, edits, ref_lengths):
    """an LMSweep as the engine returns it, from given distances [G, B]"""
    edits = np.asarray(edits, np.int32)
    al, be = np.array([a for a, _ in grid]), np.array([b for _, b in grid])
    return ctc.LMSweep(al, be, edits, np.zeros_like(edits), np.zeros((edits.shape[1],), np.uint8), ref_lengths)


def reference_loop(grid, cers):
    """the prints and the answer of the reference's loop (test.py:364-382), transcribed"""
    lines = []
    min_cer = 1.0
    min_params = (0, 0)
    for (a, b), cer in zip(grid, cers):
        lines.append('searching with a:{}, b:{}, '
                     'min params:{}, min cer:{}'
                     .format(a, b, min_params, min_cer))
        if cer < min_cer:
            min_cer = cer
            min_params = (a, b)
    lines.append('min params:{}, min cer: {}'
                 .format(min_params, min_cer))
    return lines, (min_params, min_cer)


def test_fixture_is_not_vacuous(work):
    idx, lp, il, tg, tl, _, grid, want = sr.fixture(work)
    assert idx.shape == (sr.W, sr.B, sr.K) and il.tolist() == list(sr.INPUT_LENGTHS)
    assert len(grid) == 6 and any(a == 0.0 for a, _ in grid) and any(b < 0 for _, b in grid)
    assert (idx[:, sr.EMPTY_LINE, 0] == 0).all()                       # the blank on top of every column
    assert want["empty"].tolist() == [int(b == sr.EMPTY_LINE) for b in range(sr.B)]
    assert (want["hyp_lengths"][:, sr.EMPTY_LINE] == 0).all()
    assert (want["edits"][:, sr.EMPTY_LINE] == tl[sr.EMPTY_LINE]).all()
    texts, totals = sr.properties(want)
    assert texts, "every pair reads the same text on every line"
    assert totals, "every pair has the same total distance"
    assert sr.settled(want), "the yardstick's own ranking is not settled at this seed"


def test_pairs_expand_alpha_major(ctc):
    al, be = ctc.sweep_pairs([0.5, 1.0], [4.0, 5.0, 6.0])
    assert list(zip(al.tolist(), be.tolist())) == [(a, b) for a in (0.5, 1.0) for b in (4.0, 5.0, 6.0)]
    assert list(zip(al.tolist(), be.tolist())) == sr.pairs((0.5, 1.0), (4.0, 5.0, 6.0))
    al, be = ctc.sweep_pairs(pairs=[(2.0, -1.0), (0.0, 3.0)])
    assert al.tolist() == [2.0, 0.0] and be.tolist() == [-1.0, 3.0]
    for kw in (dict(), dict(alphas=[1.0]), dict(alphas=[1.0], betas=[2.0], pairs=[(1.0, 2.0)]), dict(alphas=[], betas=[1.0])):
        with pytest.raises(ValueError):
            ctc.sweep_pairs(**kw)


def test_best_ties_take_the_first(ctc):
    grid = sr.pairs((0.5, 1.0), (4.0, 5.0))
    t = ctc.LMSweepTotals().update(sweep_of(ctc, grid, [[3, 2], [1, 1], [2, 0], [4, 4]], [5, 5]))
    assert t.total_edits.tolist() == [5, 2, 2, 8] and t.nchars == 10
    assert t.cer.tolist() == [0.5, 0.2, 0.2, 0.8]
    assert t.best() == ((0.5, 5.0), 0.2)                               # the first of the two equal minima
    assert t.best() == reference_loop(grid, t.cer.tolist())[1]


def test_best_when_no_pair_gets_below_one(ctc):
    grid = sr.pairs((0.5,), (4.0, 5.0))
    t = ctc.LMSweepTotals().update(sweep_of(ctc, grid, [[4, 6], [7, 9]], [5, 5]))
    assert t.cer.tolist() == [1.0, 1.6]
    assert t.best() == ((0, 0), 1.0)
    assert t.report()[-1] == "min params:(0, 0), min cer: 1.0"


def test_totals_accumulate_over_batches(ctc):
    grid = sr.pairs((0.5, 1.0), (4.0,))
    t = ctc.LMSweepTotals()
    t.update(sweep_of(ctc, grid, [[1, 0], [3, 3]], [4, 4]))
    assert t.best() == ((0.5, 4.0), 0.125)
    t.update(sweep_of(ctc, grid, [[9, 9, 0], [0, 0, 1]], [4, 4, 4]))      # the second batch turns the order round
    assert t.total_edits.tolist() == [19, 7] and t.nchars == 20 and t.nlines == 5
    assert t.best() == ((1.0, 4.0), 0.35)
    with pytest.raises(ValueError):
        t.update(sweep_of(ctc, sr.pairs((0.5, 2.0), (4.0,)), [[1, 0], [3, 3]], [4, 4]))


def test_report_is_the_reference_loops_output(ctc):
    grid = sr.pairs((0.7, 1.1), (4.2, 5.4, 6.6))
    edits = [[30, 20], [12, 9], [12, 9], [10, 2], [40, 40], [3, 9]]
    t = ctc.LMSweepTotals().update(sweep_of(ctc, grid, edits, [25, 25]))
    want = [
        "searching with a:0.7, b:4.2, min params:(0, 0), min cer:1.0",
        "searching with a:0.7, b:5.4, min params:(0, 0), min cer:1.0",
        "searching with a:0.7, b:6.6, min params:(0.7, 5.4), min cer:0.42",
        "searching with a:1.1, b:4.2, min params:(0.7, 5.4), min cer:0.42",
        "searching with a:1.1, b:5.4, min params:(1.1, 4.2), min cer:0.24",
        "searching with a:1.1, b:6.6, min params:(1.1, 4.2), min cer:0.24",
        "min params:(1.1, 4.2), min cer: 0.24",
    ]
    assert t.report() == want
    assert t.report() == reference_loop(grid, t.cer.tolist())[0]
    assert t.best() == ((1.1, 4.2), 0.24)


def test_sweep_result_figures(ctc, work):
    """LMSweep's derived figures on the yardstick's own distances"""
    _, _, _, _, tl, _, grid, want = sr.fixture(work)
    s = sweep_of(ctc, grid, want["edits"], tl)
    assert s.pairs == grid and len(s) == 6 and s.nchars == int(tl.sum())
    assert s.total_edits.dtype == np.int64 and s.total_edits.tolist() == want["edits"].sum(axis=1).tolist()
    np.testing.assert_array_equal(s.cer, want["edits"].sum(axis=1) / float(tl.sum()))
    plain_best, plain_cer = (0, 0), 1.0
    for pair, cer in zip(grid, s.cer.tolist()):
        if cer < plain_cer:
            plain_best, plain_cer = pair, cer
    assert ctc.LMSweepTotals().update(s).best() == (plain_best, plain_cer)


def _cli():
    sys.path.insert(0, ROOT)
    try:
        spec = importlib.util.spec_from_file_location("hctr_test_cli", os.path.join(ROOT, "test.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(ROOT)
    return mod


def test_cli_argument_checks(work):
    cli = _cli()
    arpa = sr.write_arpa(work)
    base = ["-m", "hctr", "-f", "synthetic", "-i", str(work), "--device-sweep"]
    ok = base + ["-gs", "-bm", "-dm", "beam-search", "-kp", arpa]
    cli.check_device_sweep(cli.build_argparser().parse_args(ok))
    assert not cli.build_argparser().parse_args(ok[:6] + ok[7:]).device_sweep        # off unless asked for
    drop = lambda flag, n=1: [a for i, a in enumerate(ok) if not (ok.index(flag) <= i < ok.index(flag) + n)]
    for argv, word in ((drop("-gs"), "-gs"), (drop("-bm"), "-bm"), (drop("-kp", 2), "-kp"),
                       (drop("-kp", 2) + ["-kp", "zero"], "-kp"), (drop("-kp", 2) + ["-kp", "toy"], "-kp"),
                       (drop("-kp", 2) + ["-kp", os.path.join(str(work), "missing.arpa")], "missing.arpa"),
                       (drop("-dm", 2) + ["-dm", "greedy-search"], "-dm"), (ok + ["-ss"], "-ss"), (ok + ["-utp"], "-utp"),
                       (ok + ["-uts"], "-uts"), (ok + ["-tp", "tfm.pth"], "-tp"), (ok + ["-uov"], "-uov")):
        with pytest.raises(ValueError) as e:
            cli.check_device_sweep(cli.build_argparser().parse_args(argv))
        assert "--device-sweep" in str(e.value) and word in str(e.value), (argv, str(e.value))
