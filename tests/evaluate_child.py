"""Child process of test_gpu_evaluate.py::test_images_in_several_passes: with HCTR_MAX_COLS lowered in its environment
(read when the engine context is made) the batch runs in several internal passes. Evaluates the lines of
test_gpu_evaluate.image_case() in "auto" precision and writes the result arrays to the .npz named on the command line."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    pkg = importlib.import_module("handwritten-chinese-ocr-samples_amd")
    import test_gpu_evaluate as t
    synth = pkg.synth
    C = synth.DEFAULT_VOCAB + 2
    imgs, widths, truths = t.image_case(synth)
    m = pkg.hctr_model(C, precision="auto").cuda(0)
    m.load_state_dict(synth.make_state_dict(C, seed=0, head="trained"))
    passes = -(-len(widths) // m.lines_per_pass(len(widths), imgs.shape[-1]))
    tg, tl = pkg.ctc_codec(synth.characters()).encode(truths)
    ev = m.evaluate(imgs, tg, tl, widths=widths)
    np.savez(sys.argv[1], passes=passes, edits=ev.edits, counts=ev.counts, ref_map=ev.ref_map, hyp_map=ev.hyp_map,
             labels=ev.labels, lengths=ev.lengths)


if __name__ == "__main__":
    main()
