"""Checkpoints, batches and line populations for the tests of the auto mode's guard (tests/test_guard_host.py on the
two CPU oracles, tests/test_gpu_guard.py on the engine).

The guard keeps a line's f16 result when every column's top-1/top-2 margin exceeds 2 * (rel * scale + abs), scale =
the LINE's max |logit|. That certificate is sound only if every f16 logit of the line is within rel * scale + abs of
the fp32-grade one - the premise these cases are built to stress: the f16 error is roughly proportional to a line's
scale (about 1 % of it from W = 33 on), so large logits (the x 8 head) leave the absolute term nothing to hide, small
ones (x 0.25) live on it, and narrow lines and small heads are where certain lines come from.

Every checkpoint is cut from the session's seed-0 state dict (as line_cases.head_202 does); all but one share its
trunk, so the oracles run a trunk once per batch (host_logits32 / host_logits16)."""
import numpy as np

# the engine's defaults (csrc/engine.cpp guard_rel / guard_abs), written here once: test_guard_host.py asserts the
# premise on the oracle pair with them, test_gpu_guard.py checks them against model.guard() of a fresh context
GUARD_REL, GUARD_ABS = 0.018, 0.05
SOLID = 0.10                    # a line is solidly certain / uncertain when its margin is 10 % clear of the threshold
TAP_LIMIT = 16384.0             # a quarter of fp16's largest finite value: what the scaled trunk's activations stay below

# name -> (trunk, classes, head scale, which head); the trunk variant multiplies one BatchNorm's weight and bias
CHECKPOINTS = {
    "c12": ("seed0", 12, 1.0, "random"),
    "c202": ("seed0", 202, 1.0, "random"),
    "c7358": ("seed0", 7358, 1.0, "random"),
    "c202x8": ("seed0", 202, 8.0, "random"),
    "c202x0.25": ("seed0", 202, 0.25, "random"),
    "trained": ("seed0", 7358, 1.0, "trained"),
    "bn2x4": ("bn2x4", 202, 1.0, "random"),
}
TRUNK_BN, TRUNK_BN_FACTOR = "cnn.block3.0.bn2", 4.0

# name -> (generator, B, W, seed, widths or None)
BATCHES = {
    "b32w4": ("lines", 32, 4, 904, None),
    "b16w33": ("lines", 16, 33, 933, None),
    "b8w131": ("lines", 8, 131, 1031, None),
    "ragged": ("lines", 3, 67, 967, (67, 50, 33)),
    "font131": ("font", 8, 131, 1031, None),
    "b32w4s906": ("lines", 32, 4, 906, None),
    "b32w4s919": ("lines", 32, 4, 919, None),
    "b32w4s920": ("lines", 32, 4, 920, None),
}
# further seeds of the (32, 4) shape for single checkpoints: under the full random head about one line in a hundred is
# solidly certain, and seed 904 has none
EXTRA_BATCHES = {"c7358": ("b32w4s906", "b32w4s919", "b32w4s920")}
_EXTRA = {bt for v in EXTRA_BATCHES.values() for bt in v}
ANCHOR_BATCHES = ("b32w4", "b16w33")            # where f16x3 itself is compared with the fp32 oracle


def pairs():
    """every (checkpoint, batch) the tests run: generated lines for the random heads, font lines for the trained one"""
    out = []
    for ck, (_, _, _, which) in CHECKPOINTS.items():
        for bt, (gen, _, _, _, _) in BATCHES.items():
            if bt in EXTRA_BATCHES.get(ck, ()) or (bt not in _EXTRA and (gen == "font") == (which == "trained")):
                out.append((ck, bt))
    return out


def batches_of(ck):
    return [bt for c, bt in pairs() if c == ck]


def trunk_of(ck):
    return CHECKPOINTS[ck][0]


def classes_of(ck):
    return CHECKPOINTS[ck][1]


_TRAINED_HEAD = {}


def make_checkpoint(ck, state_dict, synth):
    """the state dict of checkpoint ``ck``: the seed-0 one with its head cut / scaled / replaced, or one BatchNorm scaled"""
    trunk, C, s, which = CHECKPOINTS[ck]
    sd = dict(state_dict)
    if which == "trained":
        if not _TRAINED_HEAD:                      # (the trunk of make_state_dict(head="trained") is the seed-0 one)
            _TRAINED_HEAD.update({k: v for k, v in synth.make_state_dict(C, seed=0, head="trained").items()
                                  if k.startswith("linear.")})
        sd.update(_TRAINED_HEAD)
    else:
        sd["linear.weight"] = np.ascontiguousarray(state_dict["linear.weight"][:C] * np.float32(s))
        sd["linear.bias"] = np.ascontiguousarray(state_dict["linear.bias"][:C] * np.float32(s))
    if trunk != "seed0":
        for k in (".weight", ".bias"):
            sd[TRUNK_BN + k] = state_dict[TRUNK_BN + k] * np.float32(TRUNK_BN_FACTOR)
    return sd


def make_batch(bt, synth):
    """(uint8 [B,128,W], int32 widths or None)"""
    gen, B, W, seed, widths = BATCHES[bt]
    x = synth.make_font_lines(B, W, seed) if gen == "font" else synth.make_line_images(B, W, seed)
    return x, None if widths is None else np.array(widths, np.int32)


def line_figures(logits):
    """[W,B,C] logits -> per line (smallest top-1/top-2 margin over all W columns, max |logit|), as the guard takes them"""
    lg = np.asarray(logits)
    top2 = np.partition(lg, lg.shape[2] - 2, axis=2)[:, :, -2:]
    return (top2[:, :, 1] - top2[:, :, 0]).min(axis=0), np.abs(lg).max(axis=(0, 2))


def threshold(scale, rel=None, abs_=None):
    rel = GUARD_REL if rel is None else rel
    abs_ = GUARD_ABS if abs_ is None else abs_
    return 2.0 * (rel * np.asarray(scale, np.float64) + abs_)


def populations(min_margin, scale, rel=None, abs_=None):
    """line indices (solidly certain, solidly uncertain) from a batch's per-line figures"""
    thr = threshold(scale, rel, abs_)
    mg = np.asarray(min_margin, np.float64)
    return ([int(b) for b in np.flatnonzero(mg > (1.0 + SOLID) * thr)],
            [int(b) for b in np.flatnonzero(mg < (1.0 - SOLID) * thr)])


# ---- the two CPU oracles (host side only). ``cache`` (a dict the caller keeps) holds the trunk outputs per
# (trunk, batch): the checkpoints that differ only in their head share them. Both return [W,B,C] numpy logits. ----
def _trunk_output(ck, bt, sd, synth, cache, which, taps):
    import torch
    from oracle import hctr_ref
    key = (trunk_of(ck), bt, which)
    if key not in cache:
        x, widths = make_batch(bt, synth)
        xn = torch.from_numpy(synth.normalize_pad(x, widths, max_w=x.shape[2]))
        with torch.no_grad():
            cache[key] = hctr_ref.trunk(sd, xn, taps) if which == "fp32" else hctr_ref.trunk_f16(sd, xn)
    return cache[key]


def host_logits32(ck, bt, state_dict, synth, cache, taps=None):
    """oracle.hctr_ref.forward (fp32) of checkpoint ``ck`` on batch ``bt``; ``taps`` is filled on a cache miss only"""
    from oracle import hctr_ref
    sd = make_checkpoint(ck, state_dict, synth)
    return hctr_ref.head(sd, _trunk_output(ck, bt, sd, synth, cache, "fp32", taps)).numpy()


def host_logits16(ck, bt, state_dict, synth, cache):
    """oracle.hctr_ref.forward_f16 (the engine's rounding points) of checkpoint ``ck`` on batch ``bt``"""
    from oracle import hctr_ref
    sd = make_checkpoint(ck, state_dict, synth)
    return hctr_ref.head_f16(sd, _trunk_output(ck, bt, sd, synth, cache, "f16", None)).numpy()


# ---- the populations the GPU test relies on, from the rounding oracle at the defaults above (test_guard_host.py
# recomputes them and asserts equality): {(checkpoint, batch): line indices} ----
SOLID_CERTAIN = {
    ('c12', 'b32w4'): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31],
    ('c12', 'b16w33'): [0, 3, 4, 5, 7, 8, 9, 12, 15],
    ('c12', 'b8w131'): [2],
    ('c202', 'b32w4'): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31],
    ('c7358', 'b32w4s906'): [27],
    ('c7358', 'b32w4s919'): [3],
    ('c7358', 'b32w4s920'): [4, 11],
    ('c202x8', 'b32w4'): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31],
    ('c202x0.25', 'b32w4'): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31],
    ('trained', 'font131'): [0, 1, 2, 3, 4, 7],
    ('bn2x4', 'b32w4'): [0, 7, 9, 10, 11, 19, 28, 31],
}
SOLID_UNCERTAIN = {
    ('c12', 'b16w33'): [1, 2, 6, 10, 11, 13, 14],
    ('c12', 'b8w131'): [0, 1, 3, 4, 5, 6, 7],
    ('c12', 'ragged'): [0, 1, 2],
    ('c202', 'b16w33'): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14],
    ('c202', 'b8w131'): [0, 1, 2, 3, 4, 5, 6, 7],
    ('c202', 'ragged'): [0, 1, 2],
    ('c7358', 'b32w4'): [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31],
    ('c7358', 'b16w33'): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15],
    ('c7358', 'b8w131'): [0, 1, 2, 3, 4, 5, 6, 7],
    ('c7358', 'ragged'): [0, 1, 2],
    ('c7358', 'b32w4s906'): [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14, 15, 16, 17, 19, 20, 22, 23, 24, 25, 26, 28, 29, 30, 31],
    ('c7358', 'b32w4s919'): [0, 1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31],
    ('c7358', 'b32w4s920'): [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31],
    ('c202x8', 'b16w33'): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14],
    ('c202x8', 'b8w131'): [0, 1, 2, 3, 4, 5, 6, 7],
    ('c202x8', 'ragged'): [0, 1, 2],
    ('c202x0.25', 'b16w33'): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15],
    ('c202x0.25', 'b8w131'): [0, 1, 2, 3, 4, 5, 6, 7],
    ('c202x0.25', 'ragged'): [0, 1, 2],
    ('trained', 'font131'): [6],
    ('bn2x4', 'b32w4'): [1, 2, 4, 5, 6, 8, 12, 13, 14, 15, 16, 18, 20, 21, 22, 23, 24, 25, 27, 29, 30],
    ('bn2x4', 'b16w33'): [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15],
    ('bn2x4', 'b8w131'): [0, 1, 2, 3, 4, 5, 6, 7],
    ('bn2x4', 'ragged'): [0, 1, 2],
}


if __name__ == "__main__":          # prints the two tables above, for when the criterion's defaults or the cases change
    import importlib
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _synth = importlib.import_module("handwritten-chinese-ocr-samples_amd.synth")
    _sd, _cache = _synth.make_state_dict(_synth.DEFAULT_VOCAB + 2, seed=0), {}
    _tab = ({}, {})
    for _ck, _bt in pairs():
        for _t, _v in zip(_tab, populations(*line_figures(host_logits16(_ck, _bt, _sd, _synth, _cache)))):
            if _v:
                _t[(_ck, _bt)] = _v
    for _name, _t in zip(("SOLID_CERTAIN", "SOLID_UNCERTAIN"), _tab):
        print("%s = {\n%s}" % (_name, "".join("    %r: %r,\n" % kv for kv in _t.items())))
