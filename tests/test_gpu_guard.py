"""GPU tests (-m gpu): the premise of the auto mode's certificate, line by line, and what follows from it.

``precision="auto"`` keeps a line's f16 result when every column's top-1/top-2 margin exceeds 2 * (rel * scale + abs),
scale = the LINE's own max |logit|. That is sound only if every f16 logit of the line is within rel * scale + abs of
the fp32-grade value. tests/test_gpu_parity.py bounds the f16 error by the BATCH-wide scale, which is looser, so here

  * the premise is asserted for every line of tests/guard_cases.py - seven checkpoints whose logits span a factor of 32
    in scale, widths 4 to 131 and a ragged batch - with the engine's own f16x3 logits as the yardstick, rel / abs read
    from the engine (model.guard()) and scale from model.last_guard(); f16x3 is anchored to the fp32 oracle in the
    same test by test_gpu_parity.py's own rule (X3_RTOL over the batch's scale);
  * the consequence is checked on lines that ARE certain: the host lists of solidly certain / uncertain lines
    (tests/test_guard_host.py proves them on the CPU oracles) must come out unflagged / flagged, every unflagged line's
    f16 argmax equals the f16x3 one on every column, auto == f16x3 in greedy labels, auto logits are each line's own
    mode's bit for bit, and the number of unflagged lines looked at is asserted;
  * a line's scale, min_margin and flag in a batch are those of the line alone (every checkpoint, one batch each).

No tolerance appears here that the project does not already have: the guard's own criterion and X3_RTOL.
"""
import numpy as np
import pytest

import guard_cases as gc
from test_gpu_parity import X3_RTOL

pytestmark = pytest.mark.gpu

_HOST = {}          # trunk outputs of the fp32 oracle, shared by the checkpoints of one trunk


class _Runs(object):
    """one checkpoint's context (built in "auto": it serves all three modes) and what it gave per batch"""

    def __init__(self, pkg, synth, state_dict, ck):
        self.ck, self.synth = ck, synth
        self.model = pkg.hctr_model(gc.classes_of(ck), precision="auto").cuda(0)
        self.model.load_state_dict(gc.make_checkpoint(ck, state_dict, synth))
        self.fresh_guard = self.model.guard()
        self.done = {}

    def __call__(self, bt):
        if bt not in self.done:
            m = self.model
            x, wd = gc.make_batch(bt, self.synth)
            r = {"x": x, "widths": wd}
            for mode in ("f16", "f16x3", "auto"):
                m.set_precision(mode)
                r["logits " + mode] = m(x, widths=wd)
                if mode == "auto":
                    r["guard"] = m.last_guard()
                r["labels " + mode] = [lab.tolist() for lab in m.greedy(x, widths=wd)]
                if mode == "auto":
                    r["guard greedy"] = m.last_guard()
            self.done[bt] = r
        return self.done[bt]


@pytest.fixture(scope="module", params=list(gc.CHECKPOINTS))
def runs(request, pkg, synth, state_dict):
    """module-scoped per checkpoint: pytest runs all tests of one checkpoint, frees its context, builds the next"""
    r = _Runs(pkg, synth, state_dict, request.param)
    yield r
    r.done.clear()
    del r.model


def test_defaults_are_written_once(runs):
    """guard_cases.GUARD_REL / GUARD_ABS (what the host test asserts the premise with) are the engine's defaults, and
    model.set_guard() without arguments restores exactly them"""
    assert runs.fresh_guard == (gc.GUARD_REL, gc.GUARD_ABS)
    m = runs.model
    m.set_guard(0.5, 0.25)
    assert m.guard() == (0.5, 0.25)
    m.set_guard()
    assert m.guard() == runs.fresh_guard


def test_premise_every_f16_logit_within_the_guards_tolerance_of_its_line(runs, synth, state_dict):
    """max |f16 - f16x3| over ALL W columns of a line (pad columns included, as the guard takes them) and all classes
    <= rel * (the line's last_guard scale) + abs, rel / abs from the engine. f16x3 is the yardstick; on the (32, 4) and
    (16, 33) batches it is itself within X3_RTOL * max|reference logit| of the fp32 oracle."""
    rel, ab = runs.model.guard()
    worst_rel, worst_tol, bad = 0.0, 0.0, []
    for bt in gc.batches_of(runs.ck):
        r = runs(bt)
        lg16, lg3, scale = r["logits f16"], r["logits f16x3"], r["guard"]["scale"].astype(np.float64)
        assert np.isfinite(lg16).all() and np.isfinite(lg3).all(), bt
        assert np.array_equal(scale, np.abs(lg16).max(axis=(0, 2)).astype(np.float64)), bt
        if bt in gc.ANCHOR_BATCHES:
            ref = gc.host_logits32(runs.ck, bt, state_dict, synth, _HOST)
            err3, sc32 = float(np.abs(lg3 - ref).max()), float(np.abs(ref).max())
            print("%s %s: f16x3 vs fp32 oracle %.3g of the scale (X3_RTOL %.3g)" % (runs.ck, bt, err3 / sc32, X3_RTOL))
            assert err3 <= X3_RTOL * sc32, (bt, err3, sc32)
        err = np.abs(lg16.astype(np.float64) - lg3.astype(np.float64)).max(axis=(0, 2))
        tol = rel * scale + ab
        print("%s %s: per line err / scale %.5f .. %.5f, worst err / tol %.3f" %
              (runs.ck, bt, (err / scale).min(), (err / scale).max(), (err / tol).max()))
        worst_rel, worst_tol = max(worst_rel, float((err / scale).max())), max(worst_tol, float((err / tol).max()))
        bad += [(bt, int(b), float(err[b]), float(scale[b]), float(tol[b])) for b in np.flatnonzero(~(err <= tol))]
    print("%s: worst err / scale_line %.5f, worst err / tol %.3f (rel %g, abs %g)" % (runs.ck, worst_rel, worst_tol, rel, ab))
    assert not bad, "(batch, line, err, scale, tol): %r" % (bad,)


def test_consequence_on_lines_that_are_certain(runs):
    """The host lists' solidly certain lines are unflagged and the solidly uncertain ones flagged; every unflagged
    line's f16 argmax is the f16x3 one on every column; greedy labels of auto == f16x3 for the whole batch; auto logits
    are f16x3's for flagged lines and f16's for the others, bit for bit."""
    rel, ab = runs.model.guard()
    checked = expected = 0
    for bt in gc.batches_of(runs.ck):
        r = runs(bt)
        lg16, lg3, lga, g = r["logits f16"], r["logits f16x3"], r["logits auto"], r["guard"]
        flags = g["flags"].astype(bool)
        assert g["lines"] == lg16.shape[1] and g["flagged"] == int(flags.sum()), bt
        assert np.array_equal(r["guard greedy"]["flags"], g["flags"]), bt
        # the flag is the criterion applied to the line's own figures
        assert np.array_equal(flags, ~(g["min_margin"].astype(np.float64) > gc.threshold(g["scale"], rel, ab))), bt
        certain, uncertain = gc.SOLID_CERTAIN.get((runs.ck, bt), []), gc.SOLID_UNCERTAIN.get((runs.ck, bt), [])
        assert not flags[certain].any(), (bt, [b for b in certain if flags[b]])
        assert flags[uncertain].all(), (bt, [b for b in uncertain if not flags[b]])
        expected += len(certain)
        for b in range(lg16.shape[1]):
            if flags[b]:
                assert lga[:, b].tobytes() == lg3[:, b].tobytes(), (bt, b)
            else:
                assert lga[:, b].tobytes() == lg16[:, b].tobytes(), (bt, b)
                a16, a3 = lg16[:, b].argmax(axis=1), lg3[:, b].argmax(axis=1)
                assert np.array_equal(a16, a3), (bt, b, np.flatnonzero(a16 != a3).tolist())
                checked += 1
        assert r["labels auto"] == r["labels f16x3"], bt
    print("%s: %d unflagged lines checked (%d solidly certain on the host)" % (runs.ck, checked, expected))
    assert expected > 0 and checked >= expected, (checked, expected)


MIXED_PAIR = ("c12", "b16w33")          # certain and uncertain lines side by side (guard_cases.SOLID_*)


def test_a_lines_figures_in_the_batch_are_those_of_the_line_alone(runs):
    """scale, min_margin (bytes) and flag of every line of the checkpoint's W = 33 batch (W = 131 for the trained-like
    head), against the line run alone in auto mode; under the 12-class head the batch holds flagged and unflagged lines"""
    bt = [b for b in ("b16w33", "font131") if b in gc.batches_of(runs.ck)][0]
    r = runs(bt)
    g, m = r["guard"], runs.model
    if (runs.ck, bt) == MIXED_PAIR:
        assert 0 < g["flagged"] < g["lines"], g["flags"].tolist()
    m.set_precision("auto")
    for b in range(g["lines"]):
        m(r["x"][b:b + 1])
        g1 = m.last_guard()
        assert g1["lines"] == 1
        assert g1["scale"][0].tobytes() == g["scale"][b].tobytes(), b
        assert g1["min_margin"][0].tobytes() == g["min_margin"][b].tobytes(), b
        assert int(g1["flags"][0]) == int(g["flags"][b]), b
