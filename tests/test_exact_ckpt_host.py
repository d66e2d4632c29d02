"""CPU proof that the oracle alone is exact on the exact-arithmetic checkpoint (tests/exact_ckpt.py).

These are the conditions that make the equalities of tests/test_gpu_exact.py legitimate: for every (seed, class count,
B, W) the GPU tests use, every value of the forward is an integer that fp16 and fp32 hold exactly, whatever the order
of summation and wherever a value is rounded - so the three formulations of the oracle and a float64 run agree bit for
bit, and an engine that adds up the right terms has to agree with them too."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_ckpt as ex
from oracle import hctr_ref

synth = ex.synth
F16_EXACT = 2048.0            # every integer of magnitude <= 2^11 is an fp16 value
F32_EXACT = float(1 << 24)    # every integer of magnitude <= 2^24 is an fp32 value
BLOCKS = [(s, i) for s, nb in enumerate(hctr_ref.STAGE_BLOCKS, start=1) for i in range(nb)]


def _is_int(t):
    return bool((t == t.round()).all())


@pytest.mark.parametrize("seed", ex.SEEDS)
def test_fold_returns_the_intended_integers(seed):
    """BN folds to scale exactly 1: the folded weights are the integer conv weights, the folded biases the integer BN
    biases, with and without the fp16 rounding of the weights - and the low part that the f16x3 mode would carry for
    a folded weight (the float64 product minus its fp16 value, rounded to fp16) is 0."""
    sd = ex.cached_state_dict(ex.CLASS_COUNTS[0], seed)
    for ck, bk, cin, cout, ks, has_bias in synth.conv_specs():
        for half in (False, True):
            w, b = hctr_ref._fold(sd, ck, bk, half)
            assert np.array_equal(w.numpy(), sd[ck + ".weight"]), (ck, half)
            assert np.array_equal(b.numpy(), sd[bk + ".bias"]), (ck, half)
        sc = 1.0 / np.sqrt(sd[bk + ".running_var"].astype(np.float64) + hctr_ref.BN_EPS)
        v = sd[ck + ".weight"].astype(np.float64) * sc[:, None, None, None]
        hi = v.astype(np.float32).astype(np.float16)
        assert not (v - hi.astype(np.float64)).astype(np.float32).astype(np.float16).any(), ck
        assert _is_int(w) and float(w.abs().sum(dim=(1, 2, 3)).max()) <= 2.0, ck
    head = sd["linear.weight"]
    assert np.array_equal(head.astype(np.float16).astype(np.float32), head)
    assert float(np.abs(head).sum(axis=1).max()) <= 3.0


def test_weights_cover_every_tap_group_and_channel():
    """Across the seeds used, every layer has a nonzero weight in each of its taps, in each 32-channel group of its
    input, and for every output channel (each seed on its own does, too)."""
    for seed in ex.SEEDS:
        sd = ex.cached_state_dict(ex.CLASS_COUNTS[0], seed)
        for ck, bk, cin, cout, ks, has_bias in synth.conv_specs():
            nz = sd[ck + ".weight"] != 0
            assert nz.any(axis=(1, 2, 3)).all(), (ck, "an output channel without a weight")
            assert nz.any(axis=(0, 1)).all(), (ck, "a tap without a weight")
            per_ci = nz.any(axis=(0, 2, 3))
            for g in range((cin + 31) // 32):
                assert per_ci[g * 32:(g + 1) * 32].any(), (ck, "input group %d without a weight" % g)
        for sk, c in synth.se_specs():
            p = ex.se_pattern(seed, sk, c)
            assert p.any() and not p.all()
            assert np.array_equal(sd[sk + ".fc.2.weight"][:, 0] != 0, p)
        for nc in ex.CLASS_COUNTS:
            head = ex.cached_state_dict(nc, seed)["linear.weight"]
            assert (head != 0).any(axis=1).all()
            f = (head != 0).any(axis=0).reshape(512, 4)           # feature d = c*4 + h
            assert f.any(axis=0).all() and f.reshape(16, 32, 4).any(axis=(1, 2)).all()


def _forward_f64(sd, x, rec, half_weights=True):
    """The folded forward in float64 (input and folded weights cast to double, no rounding anywhere). ``rec`` receives
    what the exactness conditions are stated on: every conv's pre-rounding output range, an upper bound of
    |bias| + sum|w||x| over the terms of one output per layer ("mag": the largest |bias|, plus the largest sum|w| of an
    output channel times the largest |x| of the layer's input), the per-image channel sums of every block's t and
    |conv2 output|, the SE pre-sigmoid values, and the taps. ``half_weights`` False: the fp32 fold, not its fp16
    value (the split-exact variants, whose folded weights are hi + lo)."""
    def conv(x, ck, bk, relu, pad, pool=False):
        w, b = hctr_ref._fold(sd, ck, bk, half_weights)
        y = F.conv2d(x, w.double(), b.double(), stride=1, padding=pad)
        rec["pre"][ck] = float(y.abs().max())
        rec["mag"][ck] = float(b.abs().max()) + float(w.abs().sum(dim=(1, 2, 3)).max()) * float(x.abs().max())
        z = F.relu(y) if relu else y
        return y, (hctr_ref._pool(z) if pool else z)

    taps = rec["taps"]
    x = torch.from_numpy(x).double()
    _, x = conv(x, "cnn.conv0_1", "cnn.bn0_1", True, 1)
    taps["conv0_1"] = x
    _, x = conv(x, "cnn.conv0_2", "cnn.bn0_2", True, 1, pool=True)
    taps["stage0"] = x
    for s, nb in enumerate(hctr_ref.STAGE_BLOCKS, start=1):
        for i in range(nb):
            p, nm = "cnn.block%d.%d" % (s, i), "block%d.%d" % (s, i)
            _, t = conv(x, p + ".conv1", p + ".bn1", True, 1)
            y, _ = conv(t, p + ".conv2", p + ".bn2", False, 1)
            rec["tsum"][nm] = float(t.abs().sum(dim=(2, 3)).max())
            rec["ysum"][nm] = float(y.abs().sum(dim=(2, 3)).max())
            m = y.mean(dim=(2, 3))
            w0 = hctr_ref._t(sd, p + ".se.fc.0.weight")
            w2 = hctr_ref._t(sd, p + ".se.fc.2.weight")
            rec["presig"][nm] = F.linear(F.relu(F.linear(m, w0.double())), w2.double())
            # the same value as the three fp32 runs compute it (they see this y, which fp32 holds exactly)
            rec["presig32"][nm] = F.linear(F.relu(F.linear(y.float().mean(dim=(2, 3)), w0)), w2)
            rec["mean"][nm] = m
            sc = torch.sigmoid(rec["presig"][nm])
            r = x
            if (p + ".downsample.0.weight") in sd:
                _, r = conv(x, p + ".downsample.0", p + ".downsample.1", False, 0)
            x = F.relu(y * sc[:, :, None, None] + r)
            taps[nm + ".conv1"], taps[nm + ".conv2"], taps[nm + ".res"], taps[nm] = t, y, r, x
            taps[nm + ".scale"] = sc
        _, x = conv(x, "cnn.conv%d" % s, "cnn.bn%d" % s, True, 1, pool=True)
        taps["stage%d" % s] = x
    f = x.flatten(1, 2).permute(0, 2, 1)
    hw, hb = hctr_ref._t(sd, "linear.weight"), hctr_ref._t(sd, "linear.bias")
    rec["mag"]["linear"] = float(hb.abs().max()) + float(hw.abs().sum(dim=1).max()) * float(f.abs().max())
    lg = F.linear(f, hw.double(), hb.double())
    return lg.permute(1, 0, 2).contiguous()


@pytest.mark.parametrize("seed,nc,B,W", ex.all_cases())
def test_oracle_is_exact(seed, nc, B, W):
    x, widths = ex.case_input(seed, B, W)

    def planted(nm, shape):
        want = np.where(ex.se_pattern(seed, "cnn." + nm + ".se", shape[1]), 1.0, 0.5).astype(np.float32)
        return np.broadcast_to(want, shape)

    _check_exact(ex.cached_state_dict(nc, seed), x, widths, planted, "case seed %d C %d B %d W %d" % (seed, nc, B, W))


def _check_exact(sd, x, widths, planted, label, split=None):
    """The exactness conditions of checkpoint ``sd`` on the images ``x``; ``planted(block, shape)`` is the scale pattern
    the checkpoint was built to give. Returns (logits, the fused run's taps, the float64 run's records).
    ``split``: None for an integer case; ("A", None) for fractional images, ("B", layer) for one layer with a weight lo
    (tests/exact_ckpt.py "Split-exact"). The oracle is then exact_ckpt.forward_split (f16x3 rounding points), the
    quantum of the conditions 2^-12 instead of 1, and the SE statistics are not claimed exact, only the scales."""
    B, W = x.shape[0], x.shape[3]
    q_img = ex.SPLIT_QUANTUM if split is not None and split[0] == "A" else 1.0
    assert x.shape == (B, 1, 128, W) and _is_int(torch.from_numpy(x) / q_img) and x.min() >= -1
    assert x.max() <= 2 if q_img == 1.0 else x.max() < 3
    if widths is not None:
        for b, wi in enumerate(widths):
            assert (x[b, 0, :, wi:] == x[b, 0, :, wi - 1:wi]).all()
    t_fused, t_unfused, t_plain = {}, {}, {}
    rec = {k: {} for k in ("pre", "mag", "tsum", "ysum", "presig", "presig32", "mean", "taps")}
    lg_p = hctr_ref.forward(sd, x, t_plain)
    if split is None:
        lg = hctr_ref.forward_f16(sd, x, t_fused, fused_se=True)
        lg_u = hctr_ref.forward_f16(sd, x, t_unfused, fused_se=False)
        lg_d = _forward_f64(sd, x, rec)
    else:
        # forward_f16 is NOT exact here (it has no lo); the split oracle takes its place, and the float64 run takes
        # the fp32 fold, which the split weights add up to (checked below)
        lg = lg_u = ex.forward_split(sd, x, t_fused)
        t_unfused = t_fused
        lg_d = _forward_f64(sd, x, rec, half_weights=False)
    # ---- the three formulations and the float64 run agree bit for bit, logits and every common tap
    assert torch.equal(lg, lg_u) and torch.equal(lg, lg_p) and torch.equal(lg.double(), lg_d)
    for k, v in t_fused.items():
        assert torch.equal(v, t_unfused[k]), k
        assert torch.equal(v.double(), rec["taps"][k]), k
        if k in t_plain:
            assert torch.equal(v, t_plain[k]), k
    assert set(t_plain) <= set(t_fused)
    # ---- every stored value is an integer that fp16 holds (split: a multiple of 2^-12 that is hi + lo of two fp16
    #      values exactly); every scale is exactly 0.5 or 1.0, in the planted pattern
    quantum = 1.0 if split is None else ex.SPLIT_QUANTUM
    biggest = 0.0
    for k, v in t_fused.items():
        if k.endswith(".scale"):
            assert np.array_equal(v.numpy(), planted(k[:-6], v.shape)), k
            continue
        assert _is_int(v / quantum), k
        if split is not None:
            assert torch.equal(ex.r_split(v), v), k
            if split[0] == "B" and _tap_index(k) < _first_fractional(split[1]):
                assert _is_int(v), k                               # integers up to the layer that carries the fraction
        biggest = max(biggest, float(v.abs().max()))
        assert float(v.abs().max()) <= F16_EXACT, (k, float(v.abs().max()))
    # ---- every sum is exact in fp32 in any order: |bias| + sum|w||x| over the terms of any output, and so every
    #      partial sum, stays below 2^24 quanta. Split cases: the budget of the 2^-12 quantum is asked of EVERY layer,
    #      also of those before the first fraction, which only need 2^24 (the stricter of the two)
    assert max(rec["mag"].values()) < F32_EXACT * quantum, max(rec["mag"].items(), key=lambda kv: kv[1])
    assert max(rec["pre"].values()) < F32_EXACT * quantum
    assert float(lg.abs().max()) < F32_EXACT * quantum
    if split is None:
        # a conv channel has at most two weights of total magnitude 2 (the head three of magnitude 1,
        # test_fold_returns_the_intended_integers), so every partial sum of a conv is bounded by 2 * 2048 + |bias|; the
        # SE statistics add up to H*W values of t or of conv2's output per image and channel, and se_premean doubles
        # them (conv2's weight) before it divides
        assert 2 * F16_EXACT + 3 < F32_EXACT and 3 * F16_EXACT + 3 < F32_EXACT
        assert 2 * max(rec["tsum"].values()) < F32_EXACT, max(rec["tsum"].values())
        assert max(rec["ysum"].values()) < F32_EXACT
    else:
        # every folded weight is w_hi + w_lo exactly (the fp32 fold: what forward() and the float64 run multiply by)
        for ck, bk, cin, cout, ks, has_bias in synth.conv_specs():
            w_hi, w_lo, b = ex.folded_split(sd, ck, bk)
            w32, b32 = hctr_ref._fold(sd, ck, bk, False)
            assert torch.equal(w_hi + w_lo, w32) and torch.equal(b, b32), ck
        w_hi, w_lo, _ = ex.folded_split(sd, "linear", "linear")
        assert torch.equal(w_hi + w_lo, hctr_ref._t(sd, "linear.weight"))
    # ---- SE: the pre-sigmoid value is exactly 0 or at least 40, in float64 and as the three fp32 runs compute it (an
    #      engine's differs from those by the rounding of the means and of their sum, a relative 1e-5 at most)
    for s, i in BLOCKS:
        nm = "block%d.%d" % (s, i)
        for v in (rec["presig"][nm], rec["presig32"][nm]):
            assert bool(((v == 0) | (v >= ex.PRESIG_FLOOR)).all()), (nm, float(v[v != 0].min()))
        if split is not None:          # the sums behind the means are not exact with a 2^-12 quantum: no claim on them
            continue
        # the engine's mean (bias + fp32(total) / fp32(H*W), total an exact integer) is within 2 fp32 ulp of the float64
        # mean: the reasoning behind the bound that test_gpu_exact.py::test_se_means_exact asserts, checked here
        H = rec["taps"][nm + ".conv2"].shape[2]
        bias = torch.from_numpy(sd["cnn." + nm + ".bn2.bias"])
        tot = (rec["taps"][nm + ".conv2"] - bias.double()[None, :, None, None]).sum(dim=(2, 3))
        assert float(tot.abs().max()) < F32_EXACT
        emu = bias[None, :] + tot.float() / (torch.tensor(float(H)) * torch.tensor(float(W)))
        ref = rec["mean"][nm]
        ulp = np.spacing(np.abs(ref.numpy()).astype(np.float32)).astype(np.float64)
        assert (np.abs(emu.double().numpy() - ref.numpy()) <= 2 * ulp).all(), nm
    # ---- the head input is busy, the logits are varied, and the row maximum is tied exactly in some columns
    srt = np.sort(lg.numpy(), axis=2)
    tied = srt[:, :, -1] == srt[:, :, -2]
    print("%s: largest stored |v| %d, head input nonzero %.2f, distinct logits %d, "
          "columns with a tied maximum %.2f" % (label, biggest, float((t_fused["stage4"] != 0).float().mean()),
                                                len(np.unique(lg.numpy())), float(tied.mean())))
    assert tied.any()
    assert float((t_fused["stage4"] != 0).float().mean()) >= 0.3
    return lg, t_fused, rec


# ------------------------------------------------------------------------------------------------------------------
# the keyed variant (tests/exact_ckpt.py, "SE, keyed"): scales that depend on the line
# ------------------------------------------------------------------------------------------------------------------
def test_keyed_checkpoint_changes_the_se_weights_only():
    """Every entry of a keyed checkpoint but the SE weights IS the unkeyed checkpoint's array; every 32-channel group
    of every SE layer holds channels of all eight sets; |a_c| <= 3 on two channels per keyed sum."""
    seed, nc, B, W = ex.KEYED_CHILD_CASE
    base, keyed = ex.cached_state_dict(nc, seed), ex.keyed_state_dict(nc, seed, B, W)
    assert set(base) == set(keyed)
    for k in base:
        if ".se.fc." in k:
            assert keyed[k].shape == base[k].shape and keyed[k].dtype == base[k].dtype, k
            assert not np.array_equal(keyed[k], base[k]), k
        else:
            assert keyed[k] is base[k], k
    for sk, c in synth.se_specs():
        sets = ex.keyed_sets(seed, sk, c)
        for g in range(c // 32):
            assert np.array_equal(np.bincount(sets[g * 32:(g + 1) * 32], minlength=8), np.full(8, 4)), (sk, g)
        w0 = keyed[sk + ".fc.0.weight"]
        assert np.array_equal(w0[2:8:2], -w0[3:8:2]) and not w0[8:].any()
        assert (np.abs(w0[2:8]) <= ex.KEYED_MAXW).all() and ((w0[2:8] != 0).sum(axis=1) == 2).all(), sk
        w2 = keyed[sk + ".fc.2.weight"]
        for u in range(2, 8):                               # unit u gains the channels of set u alone
            assert np.array_equal(w2[:, u] != 0, sets == u), (sk, u)
        assert np.array_equal(w2[:, 0] != 0, sets == ex.SET_ALWAYS) and np.array_equal(w2[:, 0], w2[:, 1])


@pytest.fixture(scope="module")
def keyed_runs():
    """per keyed case, made once: what _check_exact returns for it"""
    cache = {}

    def get(case):
        if case not in cache:
            seed, nc, B, W = case
            x, widths = ex.keyed_input(seed, B, W)
            infos = ex.keyed_se(seed, B, W)[1]
            assert len({tuple(np.unique(x[b])) for b in range(B)}) == B          # contrasting lines
            cache[case] = _check_exact(ex.keyed_state_dict(nc, seed, B, W), x, widths,
                                       lambda nm, shape: np.where(infos[nm]["pattern"], np.float32(1.0), np.float32(0.5)),
                                       "keyed case seed %d C %d B %d W %d" % case)
        return cache[case]

    yield get
    cache.clear()


@pytest.mark.parametrize("case", ex.keyed_cases(), ids=lambda c: "seed%d-C%d-B%d-W%d" % c)
def test_keyed_oracle_is_exact_and_keeps_its_margins(keyed_runs, case):
    """A keyed case meets every exactness condition of the unkeyed ones (formulations, magnitudes, scales exactly the
    planted 0.5 / 1.0 - here a pattern per line), and for every block, line and keyed sum d: |d| is at least 1000
    times the worst-case fp32 summation error C * 2^-24 * sum|a_c||mean_c|, and gain * |d| at least 40 - on the float64
    means and on the fp32 means of the oracle. The engine's differently ordered sum of differently rounded means
    (within 2 ulp each, test_oracle_is_exact) then cannot flip a sign or leave the saturated region."""
    seed, nc, B, W = case
    lg, taps, rec = keyed_runs(case)
    sd = ex.keyed_state_dict(nc, seed, B, W)
    infos = ex.keyed_se(seed, B, W)[1]
    assert torch.equal(lg, torch.from_numpy(ex.keyed_oracle_case(*case)[2]))
    worst_rel, worst_pre = np.inf, np.inf
    for nm in ex.BLOCK_NAMES:
        w0 = sd["cnn." + nm + ".se.fc.0.weight"].astype(np.float64)
        w2 = sd["cnn." + nm + ".se.fc.2.weight"].astype(np.float64)
        C = w0.shape[1]
        for mean in (rec["mean"][nm].numpy(), taps[nm + ".conv2"].mean(dim=(2, 3)).double().numpy()):
            for j in range(ex.KEYED_UNITS):
                a, gain = w0[2 + 2 * j], w2[:, 2 + 2 * j].max()
                d = mean @ a
                err = C * 2.0 ** -24 * (np.abs(mean) @ np.abs(a))
                assert (np.abs(d) >= ex.KEYED_MARGIN * err).all(), (nm, j, d.tolist(), err.tolist())
                assert (gain * np.abs(d) >= ex.PRESIG_FLOOR).all(), (nm, j, gain, d.tolist())
                assert (d > 0).any() and (d < 0).any(), (nm, j, "no sign change within the batch")
                worst_rel = min(worst_rel, float((np.abs(d) / err).min()))
                worst_pre = min(worst_pre, float(gain * np.abs(d).min()))
    print("smallest |d| / summation error %.0f, smallest keyed pre-sigmoid value %.0f" % (worst_rel, worst_pre))


@pytest.mark.parametrize("case", ex.keyed_cases(), ids=lambda c: "seed%d-C%d-B%d-W%d" % c)
def test_keyed_lines_differ_and_a_wrong_line_shows(keyed_runs, case):
    """Every pair of lines: in EVERY block the oracle's scale vectors differ in at least 8 channels, at least one of
    them in each 32-channel group. And with line b's scales replaced by those of line (b + r) % B in ONE block, for every
    block and every r = 1..B-1 (all ordered pairs of lines), the logits of every line b change: no (block, pair of
    lines) is left for which a scale taken from the other line would go unseen."""
    seed, nc, B, W = case
    lg, taps, _ = keyed_runs(case)
    for nm in ex.BLOCK_NAMES:
        sc = taps[nm + ".scale"].numpy()
        for b in range(B):
            for b2 in range(b + 1, B):
                diff = sc[b] != sc[b2]
                assert diff.sum() >= 8, (nm, b, b2, int(diff.sum()))
                assert diff.reshape(-1, 32).any(axis=1).all(), (nm, b, b2)
    sd = ex.keyed_state_dict(nc, seed, B, W)
    entries = []
    again = ex.oracle_from(sd, torch.from_numpy(ex.keyed_input(seed, B, W)[0]), entries=entries)
    assert torch.equal(again, lg) and len(entries) == len(ex.BLOCK_NAMES)        # the harness is the oracle
    unseen = []
    for n, nm in enumerate(ex.BLOCK_NAMES):
        # one run of B - 1 copies of the batch: in copy r - 1, line b gets line (b + r) % B's scales
        wrong = torch.cat([torch.roll(taps[nm + ".scale"], -r, 0) for r in range(1, B)])
        got = ex.oracle_from(sd, entries[n].repeat(B - 1, 1, 1, 1), first=n,
                             se=lambda k, name, y32: wrong if k == n else None)
        unseen += [(nm, b, (b + r) % B) for r in range(1, B) for b in range(B)
                   if torch.equal(got[:, (r - 1) * B + b], lg[:, b])]
    assert not unseen, unseen


# ------------------------------------------------------------------------------------------------------------------
# the split-exact variants (tests/exact_ckpt.py, "Split-exact"): nonzero f16x3 lo planes, still exact
# ------------------------------------------------------------------------------------------------------------------
LO_FLOOR = 8                   # elements with lo != 0 per (line, column) of every readable tap that carries fractions
SHARE_FLOOR = 0.10             # share of the logits that a lost lo term changes
SHARE_MIN_W = 15               # ... asked from this width on (at W = 1 the magnitudes stay below 14: only taps differ)


def _tap_index(k):
    """position in exact_ckpt.TAP_ORDER of tap ``k`` (a block's .conv2 / .res count as the block's output)"""
    for suffix in (".conv2", ".res"):
        if k.endswith(suffix):
            k = k[:-len(suffix)]
    return ex.TAP_ORDER.index(k)


def _first_fractional(layer):
    """index of the first tap with fractions for a weight-lo case of ``layer`` (past every tap: the head)"""
    t = ex.first_fractional_tap(layer)
    return len(ex.TAP_ORDER) if t is None else ex.TAP_ORDER.index(t)


def _share(a, b):
    return float((a != b).float().mean())


def _check_needs_lo(sd, x, lg, taps, split, label):
    """A split case cannot be passed without the lo planes: the floors of the module constants, which are conditions on
    the inputs (a case that misses one is to be changed, not the floor). Returns the figures it printed."""
    W = x.shape[3]
    first = 0 if split[0] == "A" else _first_fractional(split[1])
    fewest = None
    for buf, tap in ex.READABLE:
        if ex.TAP_ORDER.index(tap) < first:
            continue
        n = (ex.split16(taps[tap])[1] != 0).sum(dim=(1, 2))                  # [line, column]
        assert int(n.min()) >= LO_FLOOR, (tap, int(n.min()))
        fewest = int(n.min()) if fewest is None else min(fewest, int(n.min()))
    out = {"fewest lo per (line, column)": fewest}
    if W >= SHARE_MIN_W:
        out["vs f16"] = _share(lg, hctr_ref.forward_f16(sd, x))
        assert out["vs f16"] >= SHARE_FLOOR, out
        if split[0] == "A":
            out["vs no activation lo"] = _share(lg, ex.forward_split(sd, x, drop_lo_after_stem=True))
            assert out["vs no activation lo"] >= SHARE_FLOOR, out
    print("%s: %s" % (label, ", ".join("%s %s" % (k, v if isinstance(v, int) or v is None else "%.3f" % v)
                                       for k, v in out.items())))
    return out


def _split_a_cases():
    seen, out = set(), []
    for c in ex.split_edge_cases() + ex.split_child_cases():
        if c not in seen:
            seen.add(c)
            out.append(c)
    return out


@pytest.mark.parametrize("seed,nc,B,W", _split_a_cases())
def test_split_activation_cases_are_exact_and_need_lo(seed, nc, B, W):
    """Construction A (integer pixel + j * 2^-12, integer weights), every case of split_edge_cases() and
    split_child_cases(): the split oracle, forward() and the float64 run agree bit for bit on logits and taps; every
    stored value is a multiple of 2^-12 and hi + lo exactly; every layer keeps the 2^24-quanta budget; the scales are the
    planted 0.5 / 1.0. And the case needs lo: every (line, column) of every readable tap holds at least 8 elements
    with lo != 0 (smallest seen: 9 at W = 1, 79 at W = 2, 245 and more from W = 15 on), and from W = 15 on at least 10 %
    of the logits differ from forward_f16's and from a split oracle without activation lo planes (seen: 62 % and more).
    The two cases at W = 1 missed the floor of 8 with every seed of SEEDS (stage3 / block4.0 held no fraction at all):
    the case was changed, not the floor - they run with seed 9 (exact_ckpt.split_edge_cases)."""
    x, widths = ex.split_input(seed, B, W)
    sd = ex.cached_state_dict(nc, seed)

    def planted(nm, shape):
        want = np.where(ex.se_pattern(seed, "cnn." + nm + ".se", shape[1]), 1.0, 0.5).astype(np.float32)
        return np.broadcast_to(want, shape)

    label = "split A seed %d C %d B %d W %d" % (seed, nc, B, W)
    lg, taps, rec = _check_exact(sd, x, widths, planted, label, split=("A", None))
    _check_needs_lo(sd, x, lg, taps, ("A", None), label)


@pytest.mark.parametrize("seed,nc,layer", ex.split_layer_cases(), ids=lambda v: str(v).replace("cnn.", ""))
def test_split_weight_layer_cases_are_exact_and_need_lo(seed, nc, layer):
    """Construction B (integer images, ONE layer's folded weights with lo = +-2^-12 or +-2^-11), every entry of
    SPLIT_LAYERS at f = 12: exact as above, integers up to the changed layer and multiples of 2^-12 after it. The
    changed layer's w_lo is nonzero on exactly the intended output channels (0 and 1 mod 4; every class row of the
    head), and there wherever w_hi is - so in every tap and 32-channel input group the channel uses; w_lo is 0 in every
    other layer. From the changed layer on every (line, column) of every readable tap holds at least 8 elements with
    lo != 0, and at least 10 % of the logits differ from forward_f16's and from the integer checkpoint's, which are what
    an engine that lost w_lo would return (smallest seen: 12 %, block4.0.bn1)."""
    B, W = ex.SPLIT_LAYER_SHAPE
    x, widths = ex.case_input(seed, B, W)
    sd = ex.split_layer_state_dict(nc, seed, layer)

    def planted(nm, shape):
        want = np.where(ex.se_pattern(seed, "cnn." + nm + ".se", shape[1]), 1.0, 0.5).astype(np.float32)
        return np.broadcast_to(want, shape)

    label = "split B seed %d C %d %s" % (seed, nc, layer)
    lg, taps, rec = _check_exact(sd, x, widths, planted, label, split=("B", layer))
    _check_needs_lo(sd, x, lg, taps, ("B", layer), label)
    share = _share(lg, hctr_ref.forward_f16(ex.cached_state_dict(nc, seed), x))
    print("%s: logits that differ from the integer checkpoint's %.3f" % (label, share))
    assert share >= SHARE_FLOOR, share
    for ck, bk, cin, cout, ks, has_bias in synth.conv_specs():
        w_hi, w_lo, _ = ex.folded_split(sd, ck, bk)
        if bk != layer:
            assert not w_lo.any(), ck
            continue
        on = torch.zeros(cout, dtype=torch.bool)
        on[0::4], on[1::4] = True, True
        assert torch.equal((w_lo != 0).any(dim=(1, 2, 3)), on), ck
        assert torch.equal((w_lo != 0)[on], (w_hi != 0)[on]) and bool((w_hi != 0)[on].any(dim=(1, 2, 3)).all()), ck
        assert set(w_lo[on].abs().unique().tolist()) <= {0.0, 2.0 ** -ex.SPLIT_F, 2.0 ** (1 - ex.SPLIT_F)}, ck
    w_hi, w_lo, _ = ex.folded_split(sd, "linear", "linear")
    assert torch.equal(w_lo != 0, w_hi != 0) if layer == "linear" else not w_lo.any()


def test_split_layer_state_dict_changes_one_entry():
    """Every entry of a weight-lo checkpoint but the one changed IS the exact checkpoint's array, for every layer of
    SPLIT_LAYERS; the changed entry is 1 + 2^-12 / 1 - 2^-12 / 1 by channel mod 4 (the head: the integer weights times
    1 +- 2^-12 by feature parity); the list holds the 2 + 24 + 3 + 4 BatchNorms and the head."""
    assert len(ex.SPLIT_LAYERS) == 34 and len(set(ex.SPLIT_LAYERS)) == 34
    assert set(ex.SPLIT_LAYERS) == {bk for _, bk, _, _, _, _ in synth.conv_specs()} | {"linear"}
    assert set(ex.SPLIT_CHILD_LAYERS) <= set(ex.SPLIT_LAYERS)
    e = np.float32(2.0 ** -ex.SPLIT_F)
    for seed, nc, layer in ex.split_layer_cases():
        base, sd = ex.cached_state_dict(nc, seed), ex.split_layer_state_dict(nc, seed, layer)
        changed = "linear.weight" if layer == "linear" else layer + ".weight"
        assert set(base) == set(sd)
        for k in base:
            if k != changed:
                assert sd[k] is base[k], (layer, k)
        assert sd[changed].shape == base[changed].shape and sd[changed].dtype == base[changed].dtype
        if layer == "linear":
            assert np.array_equal(sd[changed][:, 0::2], base[changed][:, 0::2] * (1 + e))
            assert np.array_equal(sd[changed][:, 1::2], base[changed][:, 1::2] * (1 - e))
        else:
            g = sd[changed]
            assert (g[0::4] == 1 + e).all() and (g[1::4] == 1 - e).all() and (g[2::4] == 1).all() and (g[3::4] == 1).all()


def _planted_fault_figures(sd, x, fault):
    """(share of the logits, share of the readable tap values, smallest nonzero tap difference) by which the split oracle
    with ``fault`` planted differs from the right one"""
    taps, wrong = {}, {}
    lg = ex.forward_split(sd, x, taps)
    lg_w = ex.forward_split(sd, x, wrong, fault=fault)
    d = torch.cat([(taps[t] - wrong[t]).abs().flatten() for _, t in ex.READABLE])
    return _share(lg, lg_w), float((d != 0).float().mean()), float(d[d != 0].min()) if bool((d != 0).any()) else 0.0


def test_planted_lo_faults_show():
    """The new GPU tests can fail: three wrong lo terms planted in the ORACLE's model of block3.4.conv1 (whose output is
    readable buffer p3.2), each against the right oracle - the difference an engine with that fault would show.
      x_lo of ONE halo column (column 16 as the tile of columns 0..15 reads it, tap kx = 2) taken as 0, fractional images
      w_lo of ONE tap (ky = 0, kx = 2) taken as 0, weight-lo case of block3.4.bn1
      w_lo multiplied with the x_lo plane instead of x_hi, same case
    Each changes at least one readable tap and the logits. Seen: 0.8 % / 10.5 % / 26.0 % of the logits and 0.07 % / 0.66 % /
    3.1 % of the readable tap values differ, the smallest tap difference is 2^-12 in all three (one quantum: nothing
    smaller can occur, and the GPU tests have no tolerance to hide it in)."""
    ck = "cnn.block3.4.conv1"

    def right(xh, xl, wh, wl, b, pad):
        return F.conv2d(xh + xl, wh, b, padding=pad) + F.conv2d(xh, wl, None, padding=pad)

    def halo_column(k, xh, xl, wh, wl, b, pad):
        if k != ck:
            return None
        xm, wm = torch.zeros_like(xl), torch.zeros_like(wh)
        xm[..., 16], wm[..., 2] = xl[..., 16], wh[..., 2]              # column 16 reaches column 15 through kx = 2 only
        return right(xh, xl, wh, wl, b, pad) - F.conv2d(xm, wm, None, padding=pad)

    def one_tap(k, xh, xl, wh, wl, b, pad):
        if k != ck:
            return None
        wz = wl.clone()
        assert bool(wz[:, :, 0, 2].any())
        wz[:, :, 0, 2] = 0
        return right(xh, xl, wh, wz, b, pad)

    def wrong_plane(k, xh, xl, wh, wl, b, pad):
        return F.conv2d(xh + xl, wh, b, padding=pad) + F.conv2d(xl, wl, None, padding=pad) if k == ck else None

    seed, nc, B, W = ex.split_child_cases()[1]
    assert W == 33
    figures = [("x_lo of one halo column", _planted_fault_figures(ex.cached_state_dict(nc, seed), ex.split_input(seed, B, W)[0],
                                                                   halo_column))]
    seed, nc, layer = [c for c in ex.split_layer_cases() if c[2] == "cnn.block3.4.bn1"][0]
    sd, x = ex.split_layer_state_dict(nc, seed, layer), ex.case_input(seed, *ex.SPLIT_LAYER_SHAPE)[0]
    figures += [("w_lo of one tap", _planted_fault_figures(sd, x, one_tap)),
                ("w_lo with the x_lo plane", _planted_fault_figures(sd, x, wrong_plane))]
    for what, (logits, taps, smallest) in figures:
        print("%s: differing logits %.4f, differing readable tap values %.5f, smallest tap difference %g" % (
            what, logits, taps, smallest))
        assert logits > 0 and taps > 0 and smallest > 0, what
