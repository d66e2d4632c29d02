"""GPU tests (-m gpu) of the CTC loss gradient in caller logits (C ABI hctr_ctc_loss_logits_grad, ``CTCLoss`` with
autograd, ``CTCLoss.loss_and_grad``): what ``scaler.scale(loss).backward()`` (main.py:426) needs from the criterion.

The oracle is torch on the CPU in float64 (``x.requires_grad_(); ctc_loss(x.log_softmax(2), ..., reduction='none',
zero_infinity=True).sum().backward()``). The rule, per line b of weight w_b:

    max |grad - w_b * grad64| <= |w_b| * max(4 * e32, 2e-5),   e32 = max |torch float32 CPU backward - grad64|

e32 is computed by the test on the same inputs. The factor 4 is for a different summation order and the fast exp / log
of a float32 log-space recursion whose rounding is order-dependent; the floor covers lines where torch's float32
happens to land close: the occupancy is the exponential of a sum of float32 terms of magnitude up to ~56 (NLL <= 33 plus
|log-prob| <= 23), one ulp of which is 3.8e-6, and about four such roundings meet in the exponent of a quantity <= 1.
"""
import ctypes

import numpy as np
import pytest
import torch

import ctc_align_ref as align_ref

pytestmark = pytest.mark.gpu

FACTOR, FLOOR = 4.0, 2e-5


def _torch_grads(logits, targets, tl, il):
    """(grad64, grad32, nll64): torch CPU gradients of sum_b nll_b in the logits, zero_infinity on"""
    W, B, _ = logits.shape
    il_t = torch.full((B,), W, dtype=torch.long) if il is None else torch.as_tensor(np.asarray(il), dtype=torch.long)
    tg_t = torch.as_tensor(np.asarray(targets), dtype=torch.long)
    tl_t = torch.as_tensor(np.asarray(tl), dtype=torch.long)
    out = []
    for dt in (torch.float64, torch.float32):
        x = torch.from_numpy(np.asarray(logits)).to(dt).requires_grad_()
        nll = torch.nn.functional.ctc_loss(x.log_softmax(2), tg_t, il_t, tl_t, reduction="none", zero_infinity=True)
        nll.sum().backward()
        out.append(x.grad.numpy())
        if dt == torch.float64:
            nll64 = nll.detach().numpy()
    return out[0], out[1], nll64


def _check_rule(got, g64, g32, weights, what):
    """the module docstring's rule, line by line; returns [(err, e32)]"""
    B = g64.shape[1]
    w = np.ones(B) if weights is None else np.asarray(weights, np.float64)
    rep = []
    for b in range(B):
        e32 = float(np.abs(g32[:, b].astype(np.float64) - g64[:, b]).max())
        err = float(np.abs(np.asarray(got[:, b], np.float64) - w[b] * g64[:, b]).max())
        print("%s line %d: err %.3e, e32 %.3e, err / e32 %.3g, weight %g" % (what, b, err, e32, err / max(e32, 1e-300),
                                                                              w[b]))
        rep.append((err, e32, abs(w[b]) * max(FACTOR * e32, FLOOR)))
    for b, (err, e32, lim) in enumerate(rep):
        assert err <= lim, (what, b, err, e32, lim)
    return rep


def _repeating_target(rng, C, L):
    """L labels, one in ten repeating its predecessor"""
    t = []
    for j in range(L):
        if t and rng.rand() < 0.1:
            t.append(t[-1])
        else:
            t.append(int(rng.randint(1, C)))
    return t


def _alignment(rng, target, T):
    """a random monotone alignment of `target` over T steps: the shortest path (a blank between equal neighbours), its
    symbols then held for randomly chosen extra steps"""
    seq = []
    for j, v in enumerate(target):
        if j and target[j - 1] == v:
            seq.append(0)
        seq.append(v)
    if not seq:
        seq = [0]
    assert len(seq) <= T
    hold = np.bincount(rng.randint(0, len(seq), T - len(seq)), minlength=len(seq)) + 1
    return np.repeat(np.array(seq, np.int64), hold)


@pytest.fixture(scope="module")
def peaky(synth):
    """six lines, W = 2000, C = 7358: unit normal noise plus a boost of 14 on a random alignment of each target"""
    C, W = synth.DEFAULT_VOCAB + 2, 2000
    assert C == 7358
    rng = np.random.RandomState(5)
    lens = [0, 1, 40, 300, 700, 1030]
    il = np.array([W, W - 7, W, W // 2, W, W], np.int32)
    lines = [_repeating_target(rng, C, L) for L in lens]
    logits = rng.standard_normal((W, len(lens), C)).astype(np.float32)
    for b, t in enumerate(lines):
        path = _alignment(rng, t, int(il[b]))
        logits[np.arange(int(il[b])), b, path] += 14.0
    tl = np.array(lens, np.int32)
    targets = np.array(sum(lines, []), np.int32)
    g64, g32, nll64 = _torch_grads(logits, targets, tl, il)
    return dict(C=C, W=W, logits=logits, targets=targets, tl=tl, il=il, lines=lines, g64=g64, g32=g32, nll64=nll64)


@pytest.fixture(scope="module")
def crit_none(pkg):
    return pkg.CTCLoss(reduction="none", zero_infinity=True).cuda(0)


def _raw_grad(pkg, crit, logits, targets, tl, il, weights=None):
    """one call of the C entry on host pointers -> (nll, grad)"""
    return pkg.ctc.loss_grad_logits(crit._context(), np.ascontiguousarray(logits, np.float32), 0, targets, tl, il,
                                    weights)


def test_peaky_logits_match_torch_float64(pkg, crit_none, peaky):
    p = peaky
    print("NLL per line (float64):", np.array2string(p["nll64"], precision=3))
    assert (p["nll64"] > 5).all() and (p["nll64"] < 60).all(), p["nll64"]
    loss, grad = crit_none.loss_and_grad(p["logits"], p["targets"], p["il"], p["tl"])
    assert isinstance(grad, np.ndarray) and grad.shape == p["logits"].shape and grad.dtype == np.float32
    np.testing.assert_allclose(loss, p["nll64"], rtol=1e-5, atol=1e-3)
    _check_rule(grad, p["g64"], p["g32"], None, "peaky")


def _edge_targets(C, W, rng):
    """the forward test's hard case: L = 0; L = 1; adjacent repeats; exactly at the feasibility limit (L + repeats = T)
    with a short input; one step short of it (no alignment); a long target (2L + 1 > 2048 states) at L + repeats = W; a
    long random target"""
    def rnd(n):
        return list(rng.randint(1, C, n))
    rep = []
    for v in rnd(20):
        rep += [v] * int(rng.randint(1, 4))
    lim = [5, 5, 6, 6, 6, 7] + rnd(10)                     # 16 labels, 3 repeats: needs 19 steps
    inf = [9, 9, 9] + rnd(15)                              # 18 labels, 2 repeats: needs 20 > 19
    longt, cost = [], 0
    while cost < W:
        if longt and W - cost >= 2 and rng.rand() < 0.4:
            longt.append(longt[-1])                        # a repeat costs two steps (a blank between)
            cost += 2
        else:
            v = int(rng.randint(1, C))
            while longt and v == longt[-1]:
                v = int(rng.randint(1, C))
            longt.append(v)
            cost += 1
    assert 2 * len(longt) + 1 > 2048
    lines = [[], rnd(1), rep, lim, inf, longt, rnd(300)]
    il = [W, W - 7, W, 19, 19, W, W // 2]
    tl = np.array([len(t) for t in lines], np.int32)
    return np.array(sum(lines, []), np.int32), tl, np.array(il, np.int32)


@pytest.mark.parametrize("scale", [3.0, 30.0])
def test_hard_logits_match_torch_float64(pkg, synth, crit_none, scale):
    C, W = synth.DEFAULT_VOCAB + 2, 2000
    rng = np.random.RandomState(int(scale))
    targets, tl, il = _edge_targets(C, W, rng)
    B = len(tl)
    logits = (rng.standard_normal((W, B, C)) * scale).astype(np.float32)
    g64, g32, nll64 = _torch_grads(logits, targets, tl, il)
    assert nll64[4] == 0.0                                  # no alignment: zero_infinity
    nll, grad = _raw_grad(pkg, crit_none, logits, targets, tl, il)
    assert np.isposinf(nll[4]) and np.isfinite(np.delete(nll, 4)).all()
    assert not grad[:, 4].any()                             # exactly zero
    for b in range(B):
        assert not grad[int(il[b]):, b].any(), b            # rows t >= input_lengths[b] exactly zero
    _check_rule(grad, g64, g32, None, "scale %g" % scale)


def test_structure_without_an_oracle(pkg, crit_none, peaky):
    p = peaky
    logits, targets, tl, il, C = p["logits"], p["targets"], p["tl"], p["il"], p["C"]
    B = len(tl)
    nll, grad = _raw_grad(pkg, crit_none, logits, targets, tl, il)
    # nll: bit-identical to the forward-only entry
    fwd = pkg.ctc.loss_logits(crit_none._context(), logits, 0, targets, tl, il)
    np.testing.assert_array_equal(nll, fwd)
    # every live row sums to zero (7358 float32 terms, summed in float64)
    for b in range(B):
        s = grad[:int(il[b]), b].astype(np.float64).sum(axis=1)
        assert np.abs(s).max() <= 1e-5, (b, float(np.abs(s).max()))
        assert not grad[int(il[b]):, b].any()
    # classes outside {blank} + targets: w * softmax, to float32 rounding: the exponent z - lse, of magnitude <= 32 here,
    # is rounded to float32 (half an ulp = 1.9e-6, which is the relative error it leaves in the exponential), then the
    # exponential and the product round once more each
    lp = torch.from_numpy(logits).double().log_softmax(2)
    sm = lp.exp().numpy()
    for b in range(B):
        other = np.ones(C, bool)
        other[0] = False
        other[np.array(p["lines"][b], np.int64)] = False
        T = int(il[b])
        got = grad[:T, b][:, other].astype(np.float64)
        assert (got >= 0).all()
        np.testing.assert_allclose(got, sm[:T, b][:, other], rtol=5e-6, atol=1e-30)
    # L = 0: softmax - onehot(blank)
    want0 = sm[:, 0].copy()
    want0[:, 0] -= 1.0
    np.testing.assert_allclose(grad[:, 0].astype(np.float64), want0, rtol=5e-6, atol=3e-7)
    # host-pointer and device-pointer calls: bit-identical
    dev = torch.from_numpy(logits).cuda(0)
    nll_d, grad_d = pkg.ctc.loss_grad_logits(crit_none._context(), dev, 1, targets, tl, il, None)
    assert grad_d.is_cuda
    np.testing.assert_array_equal(nll_d, nll)
    np.testing.assert_array_equal(grad_d.cpu().numpy(), grad)
    # a buffer that is not cleared is overwritten everywhere
    junk = torch.full_like(dev, float("nan"))
    pkg.ctc.loss_grad_logits(crit_none._context(), dev, 1, targets, tl, il, None, grad=junk)
    np.testing.assert_array_equal(junk.cpu().numpy(), grad)
    del junk, grad_d
    # line_weight scales linearly; weight 0 gives exact zeros
    w = np.array([0.0, 1.0, -2.5, 0.0, -2.5, 1.0], np.float32)
    nll_w, grad_w = pkg.ctc.loss_grad_logits(crit_none._context(), dev, 1, targets, tl, il, w)
    np.testing.assert_array_equal(nll_w, nll)
    grad_w = grad_w.cpu().numpy()
    for b in range(B):
        if w[b] == 0:
            assert not grad_w[:, b].any(), b
        elif w[b] == 1:
            np.testing.assert_array_equal(grad_w[:, b], grad[:, b])
        else:
            np.testing.assert_allclose(grad_w[:, b], w[b] * grad[:, b], rtol=3e-7, atol=1e-37)   # one more rounding


def test_small_shapes(pkg, crit_none):
    """tiny C and T, every line at its own length, B = 1 (the forward test's shapes and lengths)"""
    rng = np.random.RandomState(4)
    for (W, B, C) in [(1, 1, 2), (2, 3, 3), (7, 5, 4), (64, 9, 5), (129, 4, 50)]:
        logits = (rng.standard_normal((W, B, C)) * 5).astype(np.float32)
        tl = rng.randint(0, min(W, 6) + 1, B).astype(np.int32)
        targets = rng.randint(1, C, int(tl.sum())).astype(np.int32)
        il = rng.randint(1, W + 1, B).astype(np.int32)
        g64, g32, nll64 = _torch_grads(logits, targets, tl, il)
        nll, grad = _raw_grad(pkg, crit_none, logits, targets, tl, il)
        fin = np.isfinite(nll)
        np.testing.assert_allclose(nll[fin], nll64[fin], rtol=1e-5, atol=1e-3)
        assert (nll64[~fin] == 0).all()
        _check_rule(grad, g64, g32, None, str((W, B, C)))


def test_every_ladder_instance(pkg, crit_none):
    """S = 2L + 1 = 41 .. 2201 reaches every bucket of the launch ladder (<= 64, 128, 256, 512, 1024, 2048, 4096) as the
    batch's largest; the prefixes make each bucket the launched one, since a batch launches the instance of its longest
    target. A line's loss and gradient do not depend on the rest of the batch, so one torch reference serves all."""
    W, C = 1200, 64
    Ls = [20, 50, 100, 200, 400, 900, 1100]
    Ts = [1000, W, W, 1111, W, W, W]
    reps = [0.3, 0.3, 0.3, 0.3, 0.3, 0.1, 0.04]
    rng = np.random.RandomState(5)
    lines = [align_ref.random_target(rng, C, L, r) for L, r in zip(Ls, reps)]
    for t, T in zip(lines, Ts):
        assert len(t) + int((t[1:] == t[:-1]).sum()) <= T   # every line has an alignment
    logits = (rng.standard_normal((W, len(Ls), C)) * 3).astype(np.float32)
    tl, il = np.array(Ls, np.int32), np.array(Ts, np.int32)
    g64, g32, nll64 = _torch_grads(logits, np.concatenate(lines), tl, il)
    for n in [len(Ls)] + list(range(1, len(Ls))):
        x, tg = np.ascontiguousarray(logits[:, :n]), np.concatenate(lines[:n]).astype(np.int32)
        nll, grad = _raw_grad(pkg, crit_none, x, tg, tl[:n], il[:n])
        np.testing.assert_allclose(nll, nll64[:n], rtol=1e-5, atol=1e-3)
        _check_rule(grad, g64[:, :n], g32[:, :n], None, "ladder, first %d" % n)
        np.testing.assert_array_equal(pkg.ctc.loss_logits(crit_none._context(), x, 0, tg, tl[:n], il[:n]), nll)


def _autograd_case():
    rng = np.random.RandomState(12)
    W, B, C = 300, 5, 200
    lines = [list(rng.randint(1, C, 30)), [], [7] * 160, list(rng.randint(1, C, 90)), list(rng.randint(1, C, 5))]
    il = np.array([W, W - 40, W, W, 11], np.int32)          # line 2: 160 equal labels need 319 > 300 steps
    tl = np.array([len(t) for t in lines], np.int32)
    targets = np.array(sum(lines, []), np.int32)
    logits = (rng.standard_normal((W, B, C)) * 4).astype(np.float32)
    return logits, targets, tl, il


@pytest.mark.parametrize("zero_infinity", [True, False])
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_autograd_matches_torch(pkg, reduction, zero_infinity):
    logits, targets, tl, il = _autograd_case()
    W, B, C = logits.shape
    g64, g32, _ = _torch_grads(logits, targets, tl, il)
    tg_t, il_t, tl_t = (torch.from_numpy(v).long() for v in (targets, il, tl))
    gout = torch.from_numpy(np.random.RandomState(1).standard_normal(B).astype(np.float32))
    # torch float64 for this reduction
    x64 = torch.from_numpy(logits).double().requires_grad_()
    want_loss = torch.nn.CTCLoss(reduction=reduction, zero_infinity=zero_infinity)(x64.log_softmax(2), tg_t, il_t, tl_t)
    if reduction == "none":
        want_loss.backward(gout.double())
    else:
        want_loss.backward()
    want = x64.grad.numpy()
    nan = np.isnan(want).any(axis=(0, 2))
    assert nan.tolist() == [False, False, not zero_infinity, False, False]
    weights = {"none": gout.numpy().astype(np.float64), "sum": np.ones(B),
               "mean": 1.0 / (B * np.maximum(tl, 1).astype(np.float64))}[reduction]
    np.testing.assert_allclose(want[:, ~nan], (g64 * weights[None, :, None])[:, ~nan], rtol=0, atol=1e-12)

    crit = pkg.CTCLoss(reduction=reduction, zero_infinity=zero_infinity).cuda(0)
    x = torch.from_numpy(logits).cuda(0).requires_grad_()
    loss = crit(x, tg_t, il_t, tl_t)
    assert loss.grad_fn is not None and loss.is_cuda
    if reduction == "none":
        loss.backward(gout.cuda(0))
    else:
        loss.backward()
    assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == x.dtype and x.grad.device == x.device
    got = x.grad.cpu().numpy()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    w_live = np.where(nan, 0.0, weights)
    _check_rule(np.nan_to_num(got, nan=0.0), g64, g32, w_live, "%s zi=%s" % (reduction, zero_infinity))

    # main.py's form: the criterion over log_softmax of a leaf
    x2 = torch.from_numpy(logits).cuda(0).requires_grad_()
    loss2 = crit(x2.log_softmax(2), tg_t, il_t, tl_t)
    if reduction == "none":
        loss2.backward(gout.cuda(0))
    else:
        loss2.backward()
    got2 = x2.grad.cpu().numpy()
    np.testing.assert_array_equal(np.isnan(got2), np.isnan(want))
    _check_rule(np.nan_to_num(got2, nan=0.0), g64, g32, w_live, "log_softmax leaf, %s zi=%s" % (reduction, zero_infinity))

    # without a gradient: no grad_fn, today's value bit for bit
    plain = crit(x.detach(), tg_t, il_t, tl_t)
    assert plain.grad_fn is None and not plain.requires_grad
    with torch.no_grad():
        quiet = crit(x, tg_t, il_t, tl_t)
    assert quiet.grad_fn is None and not quiet.requires_grad
    nll = pkg.ctc.loss_logits(crit._context(), logits, 0, targets, tl, il)
    today = pkg.ctc.reduce(nll, tl, reduction, zero_infinity)
    for v in (plain, quiet, loss.detach()):
        np.testing.assert_array_equal(v.cpu().numpy(), np.asarray(today))

    # loss_and_grad: the same gradient for an incoming gradient of ones; numpy in, numpy out
    if reduction != "none":
        l3, g3 = crit.loss_and_grad(logits, targets, il, tl)
        assert isinstance(g3, np.ndarray) and g3.dtype == np.float32
        np.testing.assert_array_equal(g3, got)
        np.testing.assert_array_equal(np.asarray(l3), np.asarray(today))


def test_autograd_other_dtypes_and_layouts(pkg):
    """a float64 leaf and a non-contiguous view get a gradient of their own dtype and shape"""
    logits, targets, tl, il = _autograd_case()
    crit = pkg.CTCLoss(reduction="sum", zero_infinity=True).cuda(0)
    x = torch.from_numpy(logits).cuda(0).requires_grad_()
    crit(x, targets, il, tl).backward()
    xd = torch.from_numpy(logits).double().cuda(0).requires_grad_()
    crit(xd, targets, il, tl).backward()
    assert xd.grad.dtype == torch.float64
    np.testing.assert_array_equal(xd.grad.float().cpu().numpy(), x.grad.cpu().numpy())
    xb = torch.from_numpy(np.ascontiguousarray(logits.transpose(1, 0, 2))).cuda(0).requires_grad_()   # [B, W, C] leaf
    crit(xb.transpose(0, 1), targets, il, tl).backward()
    np.testing.assert_array_equal(xb.grad.transpose(0, 1).cpu().numpy(), x.grad.cpu().numpy())


def test_on_the_engines_own_logits(pkg, synth):
    """trained-like checkpoint in f16x3, 8 font lines of width 2000 scored against their own text"""
    C, W = synth.DEFAULT_VOCAB + 2, 2000
    m = pkg.hctr_model(C, precision="f16x3").cuda(0)
    m.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    imgs, truth = synth.make_font_lines(8, W, 31, with_truth=True)
    texts = [synth.font_truth_text(b, W) for b in truth]
    targets, tl = pkg.ctc_codec(synth.characters()).encode(texts)
    logits = m(torch.from_numpy(imgs).cuda(0))
    assert logits.is_cuda and logits.shape[1] == 8
    crit = pkg.CTCLoss(reduction="sum", zero_infinity=True).attach(m)
    x = logits.clone().requires_grad_()
    loss = crit(x, targets, None, tl)
    loss.backward()
    g64, g32, nll64 = _torch_grads(logits.cpu().numpy(), targets, tl, None)
    print("engine logits: NLL per line", np.array2string(nll64, precision=3))
    np.testing.assert_allclose(float(loss.detach()), nll64.sum(), rtol=1e-5, atol=1e-3)
    _check_rule(x.grad.cpu().numpy(), g64, g32, None, "engine logits")


def test_nothing_else_moved_and_error_codes(pkg, synth, state_dict):
    C, W = synth.DEFAULT_VOCAB + 2, 640
    imgs = synth.make_line_images(4, W, seed=8)
    m = pkg.hctr_model(C).cuda(0)
    m.load_state_dict(state_dict)
    labels = m.greedy(imgs)
    tl = np.array([len(v) for v in labels], np.int32)
    targets = np.concatenate(labels).astype(np.int32)
    before = m.ctc_loss(imgs, targets, tl, reduction="none")
    crit = pkg.CTCLoss(reduction="mean", zero_infinity=True).attach(m)
    logits = m(imgs)
    for _ in range(2):
        loss, grad = crit.loss_and_grad(logits, targets, None, tl)
        assert np.isfinite(grad).all() and np.isfinite(loss)
    for a, b in zip(labels, m.greedy(imgs)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(before, m.ctc_loss(imgs, targets, tl, reduction="none"))
    # argument errors as the forward entry's
    Wl = logits.shape[0]
    small = np.zeros((Wl, 2, C), np.float32)
    tl2 = np.array([2, 1], np.int32)
    for bad in ([0, 1, 2], [1, C, 2], [1, -3, 2]):               # ids outside [1, C-1]
        with pytest.raises(ValueError):
            crit.loss_and_grad(small, np.array(bad, np.int32), None, tl2)
    with pytest.raises(ValueError):                             # length sum mismatch
        crit.loss_and_grad(small, np.array([1, 2], np.int32), None, tl2)
    for il in ([0, Wl], [Wl + 1, 5]):                           # input_lengths outside [1, W]
        with pytest.raises(ValueError):
            crit.loss_and_grad(small, np.array([1, 2, 3], np.int32), np.array(il, np.int32), tl2)
    lib = pkg.load_library()
    ctx = crit._context()
    tg = np.array([1, 2, 3], np.int32)
    vp = ctypes.c_void_p
    args = (small.ctypes.data_as(vp), 0, Wl, 2, C, tg.ctypes.data_as(vp), tl2.ctypes.data_as(vp), None, None, None)
    assert lib.hctr_ctc_loss_logits_grad(ctx, *args, None, 0) == -1                       # NULL grad_wbc
    assert lib.hctr_ctc_loss_logits_grad(ctx, *args, small.ctypes.data_as(vp), 0) == -1   # grad aliases the logits
    assert lib.hctr_ctc_loss_logits_grad(ctx, None, 0, Wl, 0, C, None, None, None, None, None, None, 0) == 0   # B = 0
    out = np.empty_like(small)
    assert lib.hctr_ctc_loss_logits_grad(ctx, *args, out.ctypes.data_as(vp), 0) == 0      # nll may be NULL
    assert np.isfinite(out).all()
    # the context is still usable after the errors
    np.testing.assert_array_equal(before, m.ctc_loss(imgs, targets, tl, reduction="none"))
