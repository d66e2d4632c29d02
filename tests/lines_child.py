"""Child process of test_gpu_lines.py::test_kernel_families_line_by_line: the engine, under whatever HCTR_* kernel-
selection variables its environment sets (they are read once per process), on one contrast batch (tests/line_cases.py)
of the seed-0 synthetic checkpoint in f16. Every line's logits, its slice of every readable buffer and its SE means and
scales in the batch - as built, reversed, rotated - must be the bytes the line gives alone. With HCTR_WS_ALIAS=1 the
stages share their buffers, so no buffer is compared; with HCTR_FUSE_SE=0 there are no SE statistics to read.
Prints every difference and exits with 1 if there is one."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    import line_cases as lc
    pkg = importlib.import_module("handwritten-chinese-ocr-samples_amd")
    synth = importlib.import_module("handwritten-chinese-ocr-samples_amd.synth")
    kw = {"buffers": os.environ.get("HCTR_WS_ALIAS", "") != "1", "se": os.environ.get("HCTR_FUSE_SE", "") != "0"}
    B, W, widths = lc.CHILD_CASE
    model = pkg.hctr_model(202).cuda(0)
    model.load_state_dict(lc.head_202(synth.make_state_dict(synth.DEFAULT_VOCAB + 2, seed=0)))
    x = lc.contrast_batch(synth, B, W)
    alone = lc.alone_snapshots(model, x, widths, **kw)
    failed = False
    for order in lc.orders(B):
        diffs = lc.line_differences(lc.snapshot(model, x[order], widths, **kw), order, alone)
        print("order %s: %s" % (order, "equal" if not diffs else "DIFFERENT"), flush=True)
        for d in diffs[:20]:
            print("  " + d, flush=True)
        failed = failed or bool(diffs)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
