"""GPU tests (-m gpu): the engine against the CPU oracle on the exact-arithmetic checkpoint, BIT FOR BIT.

tests/exact_ckpt.py builds a checkpoint and images for which every product, sum and stored value of the forward is an
integer that fp16 and fp32 hold exactly; tests/test_exact_ckpt_host.py proves, for every case used here, that the
oracle's three formulations and a float64 run then agree bit for bit. The result cannot depend on the order of a sum,
on a rounding point or on the f16x3 split, so the engine has to EQUAL the oracle: on the logits, on every activation
buffer that can be read back, on the greedy labels, in every precision mode and kernel family. A wrong halo column,
channel group, tap, pad column, pooled row, residual or scale channel is a mismatch of at least 0.5, however small its
share of the logits; in the keyed cases, whose scale patterns differ from line to line, so is a wrong LINE. No assertion here has a tolerance, except the three derived bounds on the SE statistics of the
synthetic (inexact) checkpoint at the end.
On all of those every f16x3 lo plane and w_lo row holds zeros; the split-exact variants (images with a 12-bit
fraction, one layer's folded weights with a low part) fill them and are still exact, so f16x3 must equal
exact_ckpt.forward_split there, and a wrong lo term is a mismatch of at least 2^-12.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import exact_ckpt as ex
from oracle import hctr_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit roundoff of fp32


@pytest.fixture(scope="module")
def engines(pkg):
    """engine per (class count, seed, precision) of the exact checkpoint, made on first use"""
    cache = {}

    def get(nc, seed, precision="f16"):
        key = (nc, seed, precision)
        if key not in cache:
            m = pkg.hctr_model(nc, precision=precision).cuda(0)
            m.load_state_dict(ex.cached_state_dict(nc, seed))
            cache[key] = m.eval()
        return cache[key]

    yield get
    cache.clear()


def _ids(case):
    return "seed%d-C%d-B%d-W%d" % case


@pytest.mark.parametrize("case", ex.edge_cases(), ids=_ids)
def test_widths_at_the_tile_edges(engines, case):
    """Logits, all sixteen readable activation buffers and the greedy labels equal the oracle's at widths around the
    16- and 32-column conv tiles, for one line and for a ragged batch of three (replicate padding built here). The
    greedy labels pin the first-maximum rule: every column's maximum is tied between two classes."""
    seed, nc, B, W = case
    x, logits, taps = ex.oracle_case(*case)
    model = engines(nc, seed)
    diffs = ex.engine_differences(model, x, logits, taps)
    assert not diffs, "\n".join(diffs)
    if B > 1:
        # the same lines with something else in the padding and widths= given: the engine's own replicate padding
        widths = ex.ragged_widths(B, W)
        y = x.copy()
        for b, wi in enumerate(widths):
            y[b, 0, :, wi:] = 7.0
        d = ex.first_difference("logits with widths=", model(y, widths=widths), logits, ("column", "line", "class"))
        assert d is None, d


@pytest.mark.parametrize("precision", ["f16", "f16x3", "auto"])
@pytest.mark.parametrize("case", ex.child_cases(), ids=_ids)
def test_precision_modes(engines, case, precision):
    """f16, f16x3 (hi + lo planes, tripled K; the taps read hi + lo) and auto give the oracle's bits. In auto every line
    is run again in f16x3, since every column's top-1/top-2 margin is 0."""
    seed, nc, B, W = case
    x, logits, taps = ex.oracle_case(*case)
    model = engines(nc, seed, precision)
    diffs = ex.engine_differences(model, x, logits, taps)
    assert not diffs, "\n".join(diffs)
    if precision == "auto":
        assert model.last_guard()["flagged"] == B


VARIANTS = [{"HCTR_HALO": "0", "HCTR_FUSE_SE": "0", "HCTR_FUSE_DS": "0", "HCTR_FUSE_ARGMAX": "0", "HCTR_FUSE_STEM": "0"},
            {"HCTR_HALO": "1"}, {"HCTR_PERSIST": "2"}, {"HCTR_HALFHALO": "1"}, {"HCTR_RESPRE": "1"},
            {"HCTR_WS_ALIAS": "1"}]


@pytest.mark.parametrize("env", VARIANTS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_kernel_families(env):
    """The generic family with every fusion off, the 8-wave halo kernel, the persistent tile queue, the half-halo and
    residual-prefetch variants and the aliased workspace give the oracle's bits too. Kernel selection is read once per
    process: one child per variant (tests/exact_child.py), one after the other."""
    from conftest import ROOT
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "exact_child.py")], env=e, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------------------------
# The keyed checkpoints (tests/exact_ckpt.py, "SE, keyed"): every line of a batch has its own 0.5 / 1.0 scale pattern
# in every block, so a scale, mean or tile taken from another LINE is a mismatch of at least 0.5 as well
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16", "f16x3", "auto"])
@pytest.mark.parametrize("case", ex.keyed_cases(), ids=_ids)
def test_keyed_lines(pkg, case, precision):
    """Logits, all sixteen readable buffers, the SE scales of every block (per line) and the greedy labels equal the
    oracle's on contrasting ragged lines whose scale patterns differ from line to line; and the same batch with garbage
    in the padding and widths= given (the engine's own replicate padding) gives the same logits. Default kernel family:
    this pins the line index of the fused conv2+SE epilogue (every block buffer) and of the fused downsample path
    (p1.1, and through the stage outputs the first blocks of stages 2 and 3)."""
    seed, nc, B, W = case
    x, widths, logits, taps = ex.keyed_oracle_case(*case)
    model = pkg.hctr_model(nc, precision=precision).cuda(0)
    model.load_state_dict(ex.keyed_state_dict(nc, seed, B, W))
    diffs = ex.engine_differences(model.eval(), x, logits, taps, with_scales=True)
    assert not diffs, "\n".join(diffs)
    if precision == "auto":
        assert model.last_guard()["flagged"] == B
    y = x.copy()
    for b, wi in enumerate(widths):
        y[b, 0, :, wi:] = 7.0
    d = ex.first_difference("logits with widths=", model(y, widths=widths), logits, ("column", "line", "class"))
    assert d is None, d


def test_keyed_lines_in_several_passes():
    """The five-line keyed case in a context whose passes hold fewer lines (tests/exact_child.py passes): the lines of a
    later pass, at b0 + b of the caller's batch, against the ORACLE - not against another run of the engine."""
    from conftest import ROOT
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "exact_child.py"), "passes"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------------------------
# The split-exact variants (tests/exact_ckpt.py, "Split-exact"): on the checkpoints above every activation lo plane and
# every w_lo row of f16x3 holds zeros. Here they do not, and the forward is still exact: the oracle is
# exact_ckpt.forward_split, and tests/test_exact_ckpt_host.py proves for every case that it equals forward() and a
# float64 run bit for bit, and that the case cannot be passed without the lo terms. No tolerance anywhere. The SE means
# are not asserted (their image-wide sums are not exact with a 2^-12 quantum; the scales saturate and are), nor is f16
# mode (its roundings depend on the order of the sums here).
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ex.split_edge_cases(), ids=_ids)
def test_split_widths_at_the_tile_edges(engines, case):
    """f16x3 on images with a 12-bit fraction (activation lo planes in use from the stem on): logits, all sixteen
    readable buffers (hi + lo) and the greedy labels equal the split oracle's at every tile-edge width, for one line
    and a ragged batch of three; and the ragged batch again through the engine's own replicate padding."""
    seed, nc, B, W = case
    x, logits, taps = ex.split_oracle_case(*case)
    model = engines(nc, seed, "f16x3")
    diffs = ex.engine_differences(model, x, logits, taps)
    assert not diffs, "\n".join(diffs)
    if B > 1:
        widths = ex.ragged_widths(B, W)
        y = x.copy()
        for b, wi in enumerate(widths):
            y[b, 0, :, wi:] = 7.0
        d = ex.first_difference("logits with widths=", model(y, widths=widths), logits, ("column", "line", "class"))
        assert d is None, d


@pytest.mark.parametrize("case", ex.split_child_cases(), ids=_ids)
def test_split_auto_mode(engines, case):
    """auto on the fractional images: the head's exact ties send every line to the f16x3 re-run, so what comes back is
    the f16x3 result, equal to the split oracle's (the buffers hold the re-run)."""
    seed, nc, B, W = case
    x, logits, taps = ex.split_oracle_case(*case)
    model = engines(nc, seed, "auto")
    diffs = ex.engine_differences(model, x, logits, taps)
    assert not diffs, "\n".join(diffs)
    assert model.last_guard()["flagged"] == B


@pytest.fixture(scope="module")
def layer_engines(pkg):
    """one f16x3 engine per class count for the weight-lo variants, given each variant's weights by load_state_dict"""
    cache = {}

    def get(nc):
        if nc not in cache:
            cache[nc] = pkg.hctr_model(nc, precision="f16x3").cuda(0)
        return cache[nc]

    yield get
    cache.clear()


@pytest.mark.parametrize("case", ex.split_layer_cases(), ids=lambda c: "seed%d-C%d-%s" % (c[0], c[1], c[2].replace("cnn.", "")))
def test_split_weight_layer(layer_engines, case):
    """f16x3 with ONE layer's folded weights carrying lo = +-2^-12 / +-2^-11 on half of its output channels (every
    BatchNorm in turn, and the head), integer images, two ragged lines of 33 columns: logits, all sixteen buffers, the
    SE scales of every block and the greedy labels equal the split oracle's. Pins the packer's w_lo row of that layer
    and its pairing with the x_hi plane; every later layer runs on nonzero activation lo planes."""
    seed, nc, layer = case
    x, logits, taps = ex.split_layer_oracle_case(*case)
    model = layer_engines(nc)
    model.load_state_dict(ex.split_layer_state_dict(nc, seed, layer))
    diffs = ex.engine_differences(model.eval(), x, logits, taps, with_scales=True)
    assert not diffs, "\n".join(diffs)


@pytest.mark.parametrize("env", VARIANTS, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_split_kernel_families(env):
    """Every alternative kernel family in f16x3 against the split oracle (tests/exact_child.py split): the fractional
    images at three widths, and four weight-lo variants (a block conv1, a block conv2, a downsample, the head)."""
    from conftest import ROOT
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "exact_child.py"), "split"], env=e,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------------------------
# SE statistics (hctr_debug_se): the channel means se_border / se_premean derive from conv1's sums by inclusion-
# exclusion, and the scales computed from them
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16", "f16x3"])
@pytest.mark.parametrize("case", ex.se_cases(), ids=_ids)
def test_se_means_exact(engines, case, precision):
    """Exact checkpoint, every block: by the host conditions every sum inside se_border / se_premean is an exact
    integer, so the only roundings of mean = bias + total / (H*W) are the division and the addition (bias and quotient
    have one sign, tests/exact_ckpt.py): within 2 fp32 ulp of the float64 mean of the oracle's conv2 output. The scales
    are exactly the oracle's 0.5 / 1.0 pattern. Widths 1 and 2 make the border columns coincide or touch."""
    seed, nc, B, W = case
    x, logits, taps = ex.oracle_case(*case)
    model = engines(nc, seed, precision)
    model(x)
    worst = 0.0
    for nm in ex.BLOCK_NAMES:
        mean, scale = model.debug_se(nm, B)
        ref = taps[nm + ".conv2"].astype(np.float64).mean(axis=(2, 3))     # (conv2's output before rounding == after)
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        err = np.abs(mean.astype(np.float64) - ref) / ulp
        worst = max(worst, float(err.max()))
        b, c = np.unravel_index(int(err.argmax()), err.shape)
        assert err.max() <= 2.0, "%s: mean of line %d channel %d is %r, exact %r (%.1f ulp)" % (
            nm, b, c, float(mean[b, c]), float(ref[b, c]), float(err.max()))
        d = ex.first_difference(nm + " scales", scale, taps[nm + ".scale"], ("line", "channel"))
        assert d is None, d
    print("largest error of a mean: %.2f ulp" % worst)


@pytest.fixture(scope="module")
def synth_engines(pkg, synth, state_dict):
    """the seed-0 synthetic checkpoint with a 202-class head (the trunk is what is looked at), per precision"""
    sd = dict(state_dict)
    sd["linear.weight"] = np.ascontiguousarray(state_dict["linear.weight"][:202])
    sd["linear.bias"] = np.ascontiguousarray(state_dict["linear.bias"][:202])
    cache = {}

    def get(precision):
        if precision not in cache:
            m = pkg.hctr_model(202, precision=precision).cuda(0)
            m.load_state_dict(sd)
            cache[precision] = m.eval()
        return cache[precision]

    yield get
    cache.clear()


# last block of each stage, whose conv1 output t survives in a block buffer: (block, buffer of t, tile rows, tile columns)
LAST_BLOCKS = (("block1.1", "p1.2", 16, 16), ("block2.3", "p2.0", 16, 16), ("block3.4", "p3.2", 16, 16),
               ("block4.0", "p4.0", 8, 32))


def _conv2_weights(sd, nm, precision):
    """conv2's folded weights as the engine holds them (float64 values): rounded to fp16, or hi + lo in f16x3"""
    ck, bk = "cnn." + nm + ".conv2", "cnn." + nm + ".bn2"
    w, b = hctr_ref._fold(sd, ck, bk, True)
    w, b = w.double().numpy(), b.double().numpy()
    if precision == "f16x3":
        sc = sd[bk + ".weight"].astype(np.float64) / np.sqrt(sd[bk + ".running_var"].astype(np.float64) + hctr_ref.BN_EPS)
        v = sd[ck + ".weight"].astype(np.float64) * sc[:, None, None, None]
        hi = v.astype(np.float32).astype(np.float16).astype(np.float64)
        w = hi + (v - hi).astype(np.float32).astype(np.float16).astype(np.float64)
    return w, b


@pytest.mark.parametrize("precision", ["f16", "f16x3"])
@pytest.mark.parametrize("widths", [[67, 50, 33], [17]], ids=["b3w67u", "b1w17"])
def test_se_statistics_synthetic_checkpoint(synth_engines, synth, state_dict, widths, precision):
    """Seed-0 synthetic checkpoint (nothing is exact here), last block of each stage.

    Means: the engine's against the float64 mean of bn2(conv2(t)) computed from the engine's own t and the folded
    weights as the engine holds them. Bound: the worst case of fp32 summation, n * 2^-24 * sum|w||S| / (H*W) plus one ulp
    of the result, with n = 9*C + tiles + H + W additions on the longest path (conv1's tile sums and their reduction,
    a border line, the 9*C-term product with conv2's weights) and S the tap sums of |t|.
    Scales: the engine's against float64 FCs + sigmoid of the engine's own means. Bound: the first FC's worst case
    C * 2^-24 * sum|w1||mean| carried through |w2|, plus the second FC's (C/16) * 2^-24 * sum|w2||hidden|, times the
    sigmoid's slope of at most 1/4, plus 4 ulp of the result for expf, the addition and the division.
    In f16x3, se_premean takes its `split` branches (t and the weights as hi + lo).
    Largest ratio to the bound observed on an MI355X, over the four cases: means 0.040, scales 0.0031."""
    import torch
    import torch.nn.functional as F
    B, W = len(widths), max(widths)
    model = synth_engines(precision)
    model(synth.make_line_images(B, W, 22), widths=widths)
    worst_mean = worst_scale = 0.0
    for nm, buf, rows, cols in LAST_BLOCKS:
        t = torch.from_numpy(model.debug_activation(buf, B)).double()
        C, H = t.shape[1], t.shape[2]
        mean, scale = model.debug_se(nm, B)
        w, b = _conv2_weights(state_dict, nm, precision)
        ref = F.conv2d(t, torch.from_numpy(w), torch.from_numpy(b), padding=1).mean(dim=(2, 3)).numpy()
        mag = F.conv2d(t.abs(), torch.from_numpy(np.abs(w)), None, padding=1).sum(dim=(2, 3)).numpy()
        n = 9 * C + (H // rows) * ((W + cols - 1) // cols) + H + W
        tol = n * U * mag / (H * W) + np.spacing(np.abs(ref).astype(np.float32))
        ratio = np.abs(mean.astype(np.float64) - ref) / tol
        worst_mean = max(worst_mean, float(ratio.max()))
        assert ratio.max() <= 1.0, (nm, "mean", float(ratio.max()))
        m64 = mean.astype(np.float64)
        w1 = state_dict["cnn." + nm + ".se.fc.0.weight"].astype(np.float64)
        w2 = state_dict["cnn." + nm + ".se.fc.2.weight"].astype(np.float64)
        hid = np.maximum(m64 @ w1.T, 0.0)
        pre = hid @ w2.T
        want = 1.0 / (1.0 + np.exp(-pre))
        d_hid = C * U * (np.abs(m64) @ np.abs(w1).T)
        d_pre = d_hid @ np.abs(w2).T + (C // 16) * U * (hid @ np.abs(w2).T)
        tol = 0.25 * d_pre + 4 * np.spacing(want.astype(np.float32))
        ratio = np.abs(scale.astype(np.float64) - want) / tol
        worst_scale = max(worst_scale, float(ratio.max()))
        assert ratio.max() <= 1.0, (nm, "scale", float(ratio.max()))
    print("largest ratio to the bound: means %.4f, scales %.4f" % (worst_mean, worst_scale))
