"""CPU self-test of the beam front end's oracle and checker (tests/frontend_ref.py), no GPU.

The numpy emulation of the kernels' arithmetic passes the checker on every case the GPU test runs, every case that is
not built on exact ties keeps its ambiguity share within the cap (computed from the oracle alone), and each planted
defect makes the checker raise on at least one case: the evidence that tests/test_gpu_frontend.py would notice a
subtly wrong kernel."""
import numpy as np
import pytest

import frontend_ref as fr

CASES = fr.stored_cases()


@pytest.fixture(scope="module")
def logits():
    return {c.name: c.logits() for c in CASES}


def test_case_list_covers_the_shapes():
    assert {c.C for c in CASES} == {2, 3, 63, 64, 65, 255, 256, 257, 300, 1000, 1100, 7358, 12288}
    assert {(c.W, c.B) for c in CASES} == {(1, 1), (5, 3), (17, 2)}
    for C in (2, 3, 63, 64, 65):
        assert any(c.C == C and c.k == C for c in CASES), C            # k = C
    for C in (256, 257, 1000, 7358, 12288):
        assert {33, 64} <= {c.k for c in CASES if c.C == C}, C
    assert {1, 2, 10} <= {c.k for c in CASES}
    for C in (7358, 12288):
        assert any(c.C == C and (c.W, c.B) == (5, 3) for c in CASES)
    assert len({c.name for c in CASES}) == len(CASES) and all(c.W * c.B <= 100 for c in CASES)


def test_reference_is_the_log_softmax():
    from scipy.special import log_softmax
    x = fr.make_logits("g30", 5, 3, 257, 1)
    assert np.allclose(fr.reference(x), log_softmax(x.astype(np.float64), axis=2), rtol=0, atol=1e-12)
    x[0, 0, 5:] = -np.inf
    lp = fr.reference(x)
    assert np.isneginf(lp[0, 0, 5:]).all() and np.isfinite(lp[0, 0, :5]).all()
    assert abs(np.exp(lp[0, 0, :5]).sum() - 1) < 1e-12 and (fr.tolerance(x)[0, 0, 5:] == 0).all()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_emulation_passes_and_ambiguity_is_capped(case, logits):
    x = logits[case.name]
    share = fr.ambiguity(x, case.k, True)                     # from the oracle alone
    if not case.ties:
        assert share <= fr.AMBIGUITY_CAP, share
    stats = {}
    fe = fr.emulate(x, case.k, True)
    assert fr.check_frontend(fe, x, case.k, True, stats) == share
    fr.check_case_expectations(case, fe, x)
    print("%s: err/tol %.3f, ambiguity share %.3f" % (case.name, stats["worst"], share))
    assert stats["worst"] <= 1.0
    fe = fr.emulate(x, case.k, False)
    assert fe["cand_off"] is None
    fr.check_frontend(fe, x, case.k, False)


def test_threshold_row_sits_on_the_float32_threshold(logits):
    """1000 equal classes: the emulation's log-prob is -logf(1000.f), the float32 next to ln 0.001 from below, so a
    float32 `>=` lists what the double `>` does not."""
    x = logits["thr1000-w5b3-c1100-k10"]
    fe = fr.emulate(x, 10, True)
    assert (fe["topk_logp"] == np.float32(fr.LN_THRESH)).all() and float(np.float32(fr.LN_THRESH)) < fr.LN_THRESH
    assert int(fe["cand_off"][-1]) == 0


@pytest.mark.parametrize("defect", fr.DEFECTS)
def test_checker_catches_defect(defect, logits):
    caught = []
    for case in CASES:
        x = logits[case.name]
        with np.errstate(all="ignore"):
            fe = fr.emulate(x, case.k, True, defect)
        try:
            fr.check_frontend(fe, x, case.k, True)
        except AssertionError:
            caught.append(case.name)
    print("%s: caught on %d of %d cases" % (defect, len(caught), len(CASES)))
    assert caught, defect
    if defect == "thresh_ge_f32":
        assert "thr1000-w5b3-c1100-k10" in caught
    if defect == "no_max":
        assert any(n.startswith("g1000") for n in caught)
    if defect == "rows_bw":
        assert all("w1b1" not in n for n in caught)
