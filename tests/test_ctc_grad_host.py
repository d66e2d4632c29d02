"""CPU tests of the CTC loss gradient's surface (hctr_ctc_loss_logits_grad, ``CTCLoss`` with autograd,
``ctc.line_weights``): the C ABI symbol, the new kernels' register budget, and the host-side per-line weights, which
follow torch.nn.CTCLoss's backward. The device results are checked by tests/test_gpu_ctc_grad.py."""
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT


@pytest.fixture(scope="module")
def ctc():
    return importlib.import_module(PKG + ".ctc")


def test_grad_symbol_exported_declared_and_bound(pkg):
    lib = pkg.load_library()
    with open(os.path.join(ROOT, "include", "hctr_hip.h")) as f:
        header = f.read()
    name = "hctr_ctc_loss_logits_grad"
    assert hasattr(lib, name)
    assert re.search(r"\bint %s\(" % name, header)
    _lib = importlib.import_module(PKG + "._lib")
    sig = [s for s in _lib.SIGNATURES if s[0] == name]
    assert len(sig) == 1 and len(sig[0][2]) == 13, sig
    assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 13


def test_grad_kernels_do_not_spill(pkg, tmp_path):
    """The storing forward recursion, the backward recursion (states, emission ring and alpha ring in registers), the
    lse-keeping row pass and the gradient row pass: no spilled vector register, no private segment."""
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(llvm + "/llvm-objdump") and os.path.exists(llvm + "/llvm-readelf")):
        pytest.skip("llvm-objdump / llvm-readelf not found")
    lib = tmp_path / "lib.so"
    shutil.copy(pkg.build(), lib)
    subprocess.run([llvm + "/llvm-objdump", "--offloading", str(lib)], check=True, capture_output=True, cwd=tmp_path)
    meta = {}
    for co in tmp_path.glob("lib.so.*gfx950"):
        notes = subprocess.run([llvm + "/llvm-readelf", "--notes", str(co)], check=True, capture_output=True,
                               text=True).stdout
        cur = None
        for line in notes.splitlines():
            m = re.match(r"\s*\.(name|private_segment_fixed_size|vgpr_spill_count):\s+(\S+)", line)
            if not m:
                continue
            if m.group(1) == "name":
                cur = meta.setdefault(m.group(2), {})
            elif cur is not None:
                cur[m.group(1)] = int(m.group(2))
    beta = [n for n in meta if "ctc_beta_kernel" in n]
    store = [n for n in meta if "ctc_alpha_store_kernel" in n]
    rows = [n for n in meta if "ctc_grad_rows_kernel" in n]
    rowlse = [n for n in meta if "ctc_rowlse_kernel" in n]
    assert len(beta) >= 1 and len(rows) >= 1, (beta, rows)
    assert len(beta) == len(store) == 7 and len(rowlse) == 1, (beta, store, rowlse)   # the forward recursion's instances
    for n in beta + store + rows + rowlse:
        assert meta[n]["vgpr_spill_count"] == 0 and meta[n]["private_segment_fixed_size"] == 0, (n, meta[n])


def _grad64(x, targets, il, tl, reduction, zero_infinity, g=None):
    x = x.clone().requires_grad_()
    loss = torch.nn.functional.ctc_loss(x.log_softmax(2), targets, il, tl, reduction=reduction,
                                        zero_infinity=zero_infinity)
    if reduction == "none":
        loss.backward(g)
    else:
        loss.backward()
    return x.grad


@pytest.mark.parametrize("zero_infinity", [False, True])
@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
def test_line_weights_follow_torch_autograd(ctc, reduction, zero_infinity):
    """torch's per-line gradient of the 'sum' reduction (zero_infinity on: finite everywhere) times the helper's weights,
    with the marked lines' rows filled, is torch's gradient for the reduction, to 1e-12 in float64. The weights are
    float32 (the C ABI's type), so the case keeps them exactly representable: B = 4, target lengths 0, 2, 8 and 4 make
    1 / (B * max(L, 1)) a power of two, and the incoming gradient of 'none' is drawn in float32."""
    g = torch.Generator().manual_seed(11)
    T, B, C = 14, 4, 9
    x = torch.randn(T, B, C, generator=g, dtype=torch.float64)
    tl = torch.tensor([0, 2, 8, 4])
    targets = torch.tensor([3, 4, 7, 7, 7, 7, 7, 7, 7, 7, 1, 2, 2, 5])      # line 2: 8 equal labels need 15 > 14 steps
    il = torch.tensor([T, T - 3, T, T - 1])
    nll = torch.nn.functional.ctc_loss(x.log_softmax(2), targets, il, tl, reduction="none").numpy()
    assert np.isinf(nll[2]) and np.isfinite(np.delete(nll, 2)).all()
    gout = torch.randn(B, generator=g, dtype=torch.float32).double() if reduction == "none" else None
    want = _grad64(x, targets, il, tl, reduction, zero_infinity, gout).numpy()
    per_line = _grad64(x, targets, il, tl, "sum", True).numpy()
    w, nan = ctc.line_weights(tl.numpy(), reduction, None if gout is None else gout.numpy(), nll, zero_infinity)
    assert w.dtype == np.float32 and w.shape == (B,) and nan.dtype == bool
    assert nan.tolist() == [False, False, not zero_infinity, False]
    got = ctc.fill_nan_rows(per_line * w.astype(np.float64)[None, :, None], nan, il.numpy())
    assert np.isnan(want[:, 2]).any() == (not zero_infinity)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    # without a grad_output the weights are those of an incoming gradient of ones
    w1, _ = ctc.line_weights(tl.numpy(), reduction, None, nll, zero_infinity)
    wg, _ = ctc.line_weights(tl.numpy(), reduction, np.ones(B) if reduction == "none" else 1.0, nll, zero_infinity)
    np.testing.assert_array_equal(w1, wg)


def test_line_weights_arguments(ctc):
    with pytest.raises(ValueError):
        ctc.line_weights([1, 2], "avg")
    with pytest.raises(ValueError):
        ctc.line_weights([1, 2], "none", np.ones(3))
    with pytest.raises(ValueError):
        ctc.line_weights([1, 2], "sum", np.ones(2))
    with pytest.raises(ValueError):
        ctc.line_weights([1, 2], "mean", None, np.zeros(3))
    w, nan = ctc.line_weights([0, 4], "mean")
    assert w.tolist() == [0.5, 0.125] and not nan.any()
