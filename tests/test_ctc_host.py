"""CPU tests of the CTC loss surface (hctr_ctc_loss / hctr_ctc_loss_logits, ``hctr_model.ctc_loss``, ``CTCLoss``):
the C ABI symbols, the new kernels' register budget, and the host-side target normalisation and reductions, which follow
torch.nn.CTCLoss. The device results are checked by tests/test_gpu_ctc.py."""
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


def test_ctc_symbols_exported_and_declared(pkg):
    lib = pkg.load_library()
    with open(os.path.join(ROOT, "include", "hctr_hip.h")) as f:
        header = f.read()
    for name in ("hctr_ctc_loss", "hctr_ctc_loss_logits"):
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, header), name
    assert "CTCLoss" in pkg.__all__
    import hctr_amd
    assert hctr_amd.CTCLoss is pkg.CTCLoss


def test_ctc_kernels_do_not_spill(pkg, tmp_path):
    """The recursion keeps a line's states and its prefetched emission ring in registers (statically indexed): no spilled
    vector register and no private segment in any instance, nor in the log-sum-exp / gather kernel."""
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
    alpha = [n for n in meta if "ctc_alpha_kernel" in n]
    lse = [n for n in meta if "ctc_lse_kernel" in n]
    assert len(alpha) == 7 and len(lse) == 1, (alpha, lse)
    for n in alpha + lse:
        assert meta[n]["vgpr_spill_count"] == 0 and meta[n]["private_segment_fixed_size"] == 0, (n, meta[n])


def test_padded_targets_become_concatenated(ctc):
    padded = np.array([[3, 4, 4, 0], [9, 0, 0, 0], [5, 6, 7, 8]], np.int64)
    tl = np.array([3, 0, 4])
    flat, lens = ctc.normalize_targets(padded, tl, 3)
    assert flat.dtype == np.int32 and lens.dtype == np.int32
    assert flat.tolist() == [3, 4, 4, 5, 6, 7, 8] and lens.tolist() == [3, 0, 4]
    flat2, _ = ctc.normalize_targets(torch.from_numpy(padded), torch.from_numpy(tl), 3)
    assert flat2.tolist() == flat.tolist()
    flat3, _ = ctc.normalize_targets(flat, lens, 3)              # 1-D passes through
    assert flat3.tolist() == flat.tolist()


@pytest.mark.parametrize("targets, lengths, B", [
    (np.array([1, 2, 3]), np.array([1, 1]), 2),                   # sum(target_lengths) != number of targets
    (np.array([1, 2, 3]), np.array([3]), 2),                      # target_lengths not [B]
    (np.array([[1, 2], [3, 4]]), np.array([3, 1]), 2),            # longer than the padded width
    (np.array([1, 2]), np.array([3, -1]), 2),                     # negative length
    (np.zeros((1, 1, 1), np.int64), np.array([1]), 1),            # 3-D targets
    (np.array([1.5, 2.0]), np.array([1, 1]), 2),                  # not integers
])
def test_bad_targets_raise(ctc, targets, lengths, B):
    with pytest.raises(ValueError):
        ctc.normalize_targets(targets, lengths, B)


@pytest.mark.parametrize("zero_infinity", [False, True])
def test_reductions_follow_torch(ctc, zero_infinity):
    """'none' / 'sum' / 'mean' (each loss over clamp(target_length, min=1), then the average) and zero_infinity, against
    torch.nn.CTCLoss on the same log-probs; the per-line losses come from torch's 'none' so no device is needed."""
    g = torch.Generator().manual_seed(3)
    T, B, C = 12, 5, 9
    lp = torch.randn(T, B, C, generator=g, dtype=torch.float64).log_softmax(2)
    tl = torch.tensor([0, 3, 5, 7, 2])
    targets = torch.tensor([1, 2, 2, 3, 4, 5, 6, 7, 7, 7, 7, 7, 7, 7, 7, 1, 1])    # line 3 (7 equal labels) is infeasible
    il = torch.full((B,), T, dtype=torch.long)
    none = torch.nn.functional.ctc_loss(lp, targets, il, tl, reduction="none", zero_infinity=False).float().numpy()
    assert np.isinf(none[3]) and np.isfinite(np.delete(none, 3)).all()
    for red in ("none", "sum", "mean"):
        want = torch.nn.CTCLoss(reduction=red, zero_infinity=zero_infinity)(lp.float(), targets, il, tl).numpy()
        got = ctc.reduce(none, tl.numpy(), red, zero_infinity)
        np.testing.assert_allclose(got, want, rtol=1e-5, err_msg=red)
    assert ctc.reduce(none, tl.numpy(), "none", zero_infinity).dtype == np.float32


def test_criterion_arguments(pkg, ctc):
    with pytest.raises(NotImplementedError):
        pkg.CTCLoss(blank=1)
    with pytest.raises(ValueError):
        pkg.CTCLoss(reduction="avg")
    with pytest.raises(ValueError):
        ctc.reduce(np.zeros(2, np.float32), [1, 1], "max")
    with pytest.raises(ValueError):
        ctc.normalize_input_lengths([3, 4, 5], 2)
    assert ctc.normalize_input_lengths(None, 2) is None
