"""Cross-check of two independent kernel families over many shapes (run on the GPU box):
    python tools/gpu_shape_sweep.py dump <file.npz>     (under whatever HCTR_* variables are set)
    python tools/gpu_shape_sweep.py compare a.npz b.npz
    python tools/gpu_shape_sweep.py identical a.npz b.npz      (two builds that must agree bit for bit)
`dump` stores, for ~30 random (lines, width, per-line widths) cases, the logits' per-column max / argmax and a
class subsample, and under ctc/ the results of the CTC family (loss, gradient, alignment) on a batch that reaches every
rung of the recursion kernels' instance ladder and on two of the image cases; `identical` covers all of it, `compare`
only the logits; `compare` requires the two runs (e.g. default halo kernels vs HCTR_HALO=0 generic kernels with
HCTR_FUSE_SE=0 HCTR_FUSE_DS=0 HCTR_FUSE_ARGMAX=0) to agree within fp16-pipeline noise on every case."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cases():
    rng = np.random.default_rng(2024)
    out = []
    for i in range(30):
        B = int(rng.integers(1, 7))
        W = int(rng.choice([int(rng.integers(1, 40)), int(rng.integers(40, 700)), 16 * int(rng.integers(1, 30)),
                            32 * int(rng.integers(1, 15)) + int(rng.integers(-1, 2))]))
        W = max(1, W)
        widths = [W] + [int(rng.integers(1, W + 1)) for _ in range(B - 1)]
        out.append((i, B, W, widths))
    return out


def ctc_ladder_batch():
    """tests/test_gpu_ctc_grad.py::test_every_ladder_instance's batch: S = 2L + 1 falls into each rung's bucket"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctc_align_ref
    W, C = 1200, 64
    Ls = [20, 50, 100, 200, 400, 900, 1100]
    Ts = [1000, W, W, 1111, W, W, W]
    rng = np.random.RandomState(5)
    lines = [ctc_align_ref.random_target(rng, C, L, r) for L, r in zip(Ls, [0.3, 0.3, 0.3, 0.3, 0.3, 0.1, 0.04])]
    logits = (rng.standard_normal((W, len(Ls), C)) * 3).astype(np.float32)
    return logits, lines, np.array(Ls, np.int32), np.array(Ts, np.int32)


def _put_alignment(d, key, a):
    for name in ("paths", "starts", "ends", "logps", "scores"):
        d["%s/%s" % (key, name)] = np.asarray(getattr(a, name))


def dump_ctc(d, hctr_amd, models):
    ctc = hctr_amd.package.ctc
    crit = hctr_amd.CTCLoss(reduction="none").cuda(0)      # owns the context: it lives as long as crit does
    ctx = crit._context()
    logits, lines, tl, il = ctc_ladder_batch()
    for n in range(1, len(lines) + 1):                      # the first n lines launch rung n
        x, tg = np.ascontiguousarray(logits[:, :n]), np.concatenate(lines[:n]).astype(np.int32)
        d["ctc/ladder%d/nll" % n] = ctc.loss_logits(ctx, x, 0, tg, tl[:n], il[:n])
        d["ctc/ladder%d/nll_grad" % n], d["ctc/ladder%d/grad" % n] = ctc.loss_grad_logits(ctx, x, 0, tg, tl[:n], il[:n], None)
        _put_alignment(d, "ctc/ladder%d" % n, ctc.align_logits(ctx, x, 0, tg, tl[:n], il[:n]))
    s = hctr_amd.synth
    for i, B, W, widths in sorted(cases(), key=lambda c: -c[2])[:2]:       # the two widest image cases
        imgs = s.make_line_images(B, W, seed=3000 + i)
        for name, m in models.items():
            lab = m.greedy(imgs, widths=widths)              # each line's own greedy text is its target
            tl = np.array([len(x) for x in lab], np.int32)
            tg = np.concatenate(lab).astype(np.int32) if tl.sum() else np.zeros((0,), np.int32)
            key = "ctc/img%d/%s" % (i, name)
            d[key + "/nll"] = m.ctc_loss(imgs, tg, tl, widths=widths, reduction="none")
            _put_alignment(d, key, m.align(imgs, tg, tl, widths=widths))


def dump(path):
    import hctr_amd
    s = hctr_amd.synth
    C = s.DEFAULT_VOCAB + 2
    m = hctr_amd.hctr_model(C).cuda(0)
    m.load_state_dict(s.make_state_dict(C, seed=0))
    d = {}
    for i, B, W, widths in cases():
        imgs = s.make_line_images(B, W, seed=3000 + i)
        lg = m(imgs, widths=widths)
        lab = m.greedy(imgs, widths=widths)
        d["%d/max" % i] = lg.max(axis=2)
        d["%d/arg" % i] = lg.argmax(axis=2).astype(np.int32)
        d["%d/sub" % i] = lg[:, :, ::97].copy()
        d["%d/len" % i] = np.array([len(x) for x in lab], np.int32)
        d["%d/lab" % i] = np.concatenate(lab) if sum(len(x) for x in lab) else np.zeros((0,), np.int32)
        # fused greedy must equal the decode of this run's own logits
        arg = lg.argmax(axis=2).T
        for b in range(B):
            t = arg[b]
            keep = (t != 0) & (t != C - 1) & np.concatenate(([True], t[1:] != t[:-1]))
            assert list(t[keep]) == list(lab[b]), ("fused greedy != decode of own logits", i, b)
    m3 = hctr_amd.hctr_model(C, precision="f16x3").cuda(0)
    m3.load_state_dict(s.make_state_dict(C, seed=0))
    dump_ctc(d, hctr_amd, {"f16": m, "f16x3": m3})
    np.savez_compressed(path, **d)
    print("dumped", len(cases()), "cases ->", path)


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    worst, agree_min = 0.0, 1.0
    for i, B, W, widths in cases():
        scale = float(np.abs(a["%d/max" % i]).max())
        err = float(np.abs(a["%d/sub" % i] - b["%d/sub" % i]).max())
        agree = float((a["%d/arg" % i] == b["%d/arg" % i]).mean())
        worst, agree_min = max(worst, err / scale), min(agree_min, agree)
        assert err <= 0.012 * scale + 0.05, (i, B, W, err, scale)
        assert agree >= 0.93, (i, B, W, agree)
    print("ok: %d cases, worst relative logit difference %.4f, minimum argmax agreement %.3f" %
          (len(cases()), worst, agree_min))


def identical(pa, pb):
    """bit-for-bit equality of two dumps (two builds of the SAME arithmetic, e.g. a re-scheduled epilogue)"""
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files)
    bad = [k for k in a.files if not np.array_equal(a[k], b[k])]
    assert not bad, bad[:8]
    print("identical: %d arrays of %d cases and the CTC section" % (len(a.files), len(cases())))


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif sys.argv[1] == "identical":
        identical(sys.argv[2], sys.argv[3])
    else:
        compare(sys.argv[2], sys.argv[3])
