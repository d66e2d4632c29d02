"""Contrast batches for the batch-versus-alone tests (tests/test_gpu_lines.py, tests/lines_child.py; the host
precondition is in tests/test_lines_host.py).

The lines of a synth.make_line_images batch come from one distribution, and their SE scales differ by about one fp16 ulp
from line to line: a scale taken from the neighbouring line would round away. Here one line stays as generated, one is
constant background and one is negated (dark background, light strokes), which moves every block's channel means, and
with them its scales, by far more than a rounding error; lines 3 and 4 of a five-line batch are generated ones again."""
import numpy as np

SEED = 31
# (B, W, widths or None): the widths around the 16- and 32-column tiles, five lines, and one ragged batch
CASES = ((3, 17, None), (3, 33, None), (3, 65, None), (5, 33, None), (3, 65, (65, 41, 22)))
CHILD_CASE = CASES[1]
MIN_SCALE_GAP = 2.0 ** -6      # 32 fp16 ulps of a value in [0.5, 1): what two lines' scales differ by in some channel


def case_id(case):
    B, W, widths = case
    return "b%dw%d%s" % (B, W, "" if widths is None else "ragged")


def contrast_batch(synth, B, W):
    """uint8 [B,128,W]: line 0 as generated, line 1 constant background, line 2 negated, the others as generated"""
    x = synth.make_line_images(B, W, SEED).copy()
    x[1] = 255
    x[2] = 255 - x[2]
    return x


def orders(B):
    """the batch orders the tests run: as built, reversed, rotated by one"""
    ident = list(range(B))
    return [ident, ident[::-1], ident[1:] + ident[:1]]


def head_202(state_dict):
    """the seed-0 synthetic checkpoint with its head cut to 202 classes (the trunk is what is looked at)"""
    sd = dict(state_dict)
    sd["linear.weight"] = np.ascontiguousarray(state_dict["linear.weight"][:202])
    sd["linear.bias"] = np.ascontiguousarray(state_dict["linear.bias"][:202])
    return sd


# ---- what a forward leaves behind, line by line (GPU side) ----
def snapshot(model, x, widths=None, buffers=True, se=True):
    """{name: array with the line axis FIRST} of one forward of ``model`` on the batch ``x``: the logits, the sixteen
    readable activation buffers, and every block's SE means and scales"""
    import exact_ckpt as ex
    B = x.shape[0]
    out = {"logits": np.ascontiguousarray(np.swapaxes(model(x, widths=widths), 0, 1))}
    if buffers:
        for buf, _ in ex.READABLE:
            out["buffer " + buf] = model.debug_activation(buf, B)
    if se:
        for nm in ex.BLOCK_NAMES:
            out["means " + nm], out["scales " + nm] = model.debug_se(nm, B)
    return out


def alone_snapshots(model, x, widths=None, **kw):
    """snapshot() of every line of ``x`` run alone: the same bytes, the same W, the same width"""
    return [snapshot(model, x[b:b + 1], None if widths is None else [widths[b]], **kw) for b in range(x.shape[0])]


def line_differences(snap, order, alone):
    """Every array of the batch's snapshot whose row i is not, byte for byte, what line order[i] gave alone"""
    out = []
    for i, b in enumerate(order):
        for k, v in snap.items():
            if v[i].tobytes() != alone[b][k][0].tobytes():
                bad = np.argwhere(v[i] != alone[b][k][0])
                where = tuple(int(j) for j in bad[0]) if len(bad) else ()
                out.append("%s of line %d (at position %d of the batch): %d values differ, first at %s: %r in the batch, "
                           "%r alone" % (k, b, i, len(bad), where, v[i][where], alone[b][k][0][where]))
    return out
