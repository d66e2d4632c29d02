"""CPU precondition of tests/test_gpu_lines.py: on the contrast batches (tests/line_cases.py) the f16 oracle gives every
pair of lines, in EVERY block, a channel whose SE scales differ by at least 2^-6 - 32 fp16 ulps of a value of that
size, so an engine that applied the other line's scale could not round its way back to the right bits."""
import numpy as np
import pytest

import line_cases as lc
from oracle import hctr_ref

BLOCKS = ["block%d.%d" % (s, i) for s, nb in enumerate(hctr_ref.STAGE_BLOCKS, start=1) for i in range(nb)]


@pytest.mark.parametrize("case", lc.CASES, ids=lc.case_id)
def test_contrast_lines_have_distinct_scales_in_every_block(synth, state_dict, case):
    B, W, widths = case
    x = synth.normalize_pad(lc.contrast_batch(synth, B, W), widths, max_w=W)
    taps = {}
    hctr_ref.forward_f16(lc.head_202(state_dict), x, taps)
    smallest = np.inf
    for nm in BLOCKS:
        sc = taps[nm + ".scale"].numpy().astype(np.float64)
        for b in range(B):
            for b2 in range(b + 1, B):
                gap = float(np.abs(sc[b] - sc[b2]).max())
                smallest = min(smallest, gap)
                assert gap >= lc.MIN_SCALE_GAP, (nm, b, b2, gap)
    print("smallest of the pairs' largest scale gaps: %.4f" % smallest)
