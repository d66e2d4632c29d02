"""Time the CTC loss of the image path against greedy decoding on the same batch (run on the GPU box):

    python tools/bench_ctc.py [--lines 64] [--width 2000] [--steps 5] [--warmup 2] [--precision f16] [--layers]

The batch is BASELINE configs[1]'s shape (64 synthetic lines of 2000 columns, random-head checkpoint) and each line is
scored against its own greedy text, as a validation loss of decoded output would be. hctr_ctc_loss and hctr_greedy run
alternately (device-synchronised wall time per call; both are synchronous at return), after warm-up calls of each.
--layers adds the engine's per-launch device times of one call of each (HIP events; names as rocprofv3 groups them:
head.linear, ctc_lse, ctc_alpha vs head.linear+argmax). Prints one JSON line.

    python tools/bench_ctc.py --backward [--layers] ...

times the criterion on caller logits instead (the engine's own logits of that batch, a device tensor [W, lines, C], each
line's greedy text as targets): loss only (hctr_ctc_loss_logits), loss + gradient (hctr_ctc_loss_logits_grad into a
preallocated device tensor) and torch.nn.functional.ctc_loss over log_softmax, forward + backward, on the same device
tensors - alternately, after warm-up calls of each. --layers adds the device times of the gradient call's launches and
the bytes per second of its two row passes (ctc_rowlse reads the logits once; ctc_grad_rows reads them once and writes
the gradient once).

    python tools/bench_ctc.py --align [--layers] ...

times the forced alignment on the same caller logits and targets (hctr_ctc_align_logits, every output fetched) and, in
the same run, the loss (hctr_ctc_loss_logits), alternately after warm-up calls of each. --layers adds the device times
of the align call's launches: the emission pass, the recursion and the back-trace.

    python tools/bench_ctc.py --recognize [--layers] ...

times the greedy recognition on the same caller logits (hctr_recognize_logits, every output fetched) against the chain
of three calls it replaces - hctr_decode_greedy_logits, then hctr_ctc_loss_logits and hctr_ctc_align_logits with the
decoded labels as targets - alternately after warm-up calls of each. --layers adds the device times of every launch of
both, and greedy_rowstat's time against the sum of the two row passes it fuses (argmax_rows + ctc_lse).

    python tools/bench_ctc.py --evaluate [--host-lines 4] ...

times the edit distance on the device against the host loop it replaces (test.py's edit_distance, the pure-Python
two-row recursion) on the same label sequences, at two shapes: "short", font lines under the trained-like head with their
own texts as truths (a few dozen characters a line, what a trained model decodes), and "long", the random-head batch,
whose lines decode to about a thousand labels, against their own decode with a tenth of the labels altered. Per shape:
hctr_edit_distance distance-only and with counts and maps, the host loop, hctr_model.evaluate (distance-only and with
maps) and hctr_model.greedy followed by the host loop - alternately, after warm-up calls of each, medians. The host loop
of the long shape takes about a second per line: it is timed once on the first --host-lines lines and scaled to the
batch (reported as such).

    python tools/bench_ctc.py --nbest ...

times the device prefix beam search (hctr_nbest: forward, front end and search on the device, N-best labels and scores
fetched) against the path it spares LM-free callers - hctr_beam_frontend with its top-k copy to the host, then the host
search hctr_beam_search(builtin_lm = 1) on 16 threads on those lists - at beam 10 / depth 10, len_bonus 5.8, each line
over the host search's own number of steps (the reference's end step), alternately after warm-up calls of each, medians.
Three figures: the device search alone (its two launches' device time, and the wall time of hctr_nbest_topk on the same
lists, which adds their upload), the front end + D2H + host search, and the front end alone. The 1-best texts of the two
searches are compared.

    python tools/bench_ctc.py --nbest-lm ...

times the n-gram-scored device search (hctr_nbest_lm*) on the same batch against the host search it restates,
hctr_beam_search(builtin_lm = 3) on 16 threads on the same lists, at beam 10 / depth 10, lm_panelty 2, len_bonus 5.8. The
model is an ARPA file the tool writes itself: order 5 over the synthetic vocabulary, deterministic, about 330 000
n-grams (a 32 MB table, so the probes miss L2). Calls alternate after warm-up calls of each, medians; the device time of
the search's launches (pre-pass, search, backtrace) and of the zero-LM prefix_beam over the same end steps come from
profiled calls of the same run; the lines whose 1-best differs from the host search's are counted.

    python tools/bench_ctc.py --nbest-skip ...

times the device skip search (hctr_nbest_skip*) on the trained-like checkpoint's glyph-font lines (the random head is no
use here: its rows have no class above 0.001 and every line empties) with the same order-5 model at beam 10: the skip
search on the front end's lists (hctr_nbest_skip_lists) against the device full search (hctr_nbest_lm_topk) and the host
skip search (hctr_beam_search(skip_search = 1, builtin_lm = 3), 16 threads) on the same lists in the same process; calls
alternate after warm-up calls of each, medians. Reports the share of in-place steps, the largest row, the line statuses
and the device time of each search's launches from profiled calls.

    python tools/bench_ctc.py --lm-sweep --pairs 250 ...

times the LM weight sweep (hctr_lm_sweep_topk: G pairs of (lm_panelty, len_bonus) searched on one set of lists, the edit
distances taken on the device) on the batch, lists and order-5 model of --nbest-lm, against G successive calls of
hctr_nbest_lm_topk(nbest = 1) + hctr_edit_distance on the same lists in the same process - the way to the same numbers
without the sweep. The pairs are the first G of the reference's default grid (10 x 25, alpha-major); the transcriptions
are the lines' greedy texts. The two alternate after warm-up calls of each, medians of the wall time per call; the device
time of each one's launches comes from one profiled call of each in the same run. Every ``edits`` value of the two is
compared before anything is reported.

    python tools/bench_ctc.py --spot [--queries 16] [--layers] ...

times keyword spotting on the same caller logits (hctr_spot_logits, every output fetched) for --queries queries of
length 2-4, half of them drawn from the lines' greedy texts and half absent from every line, and in the same run the
loss (hctr_ctc_loss_logits, each line's greedy text as its target), alternately after warm-up calls of each, medians.
--layers adds the device time of the call's launches, which the engine sums per name over the chunks of queries
(ctc_lse: one pass over the logits per chunk; spot: the recursions).

    python tools/bench_ctc.py --lexicon [--entries 10000] [--unit-nodes 0] [--layers] ...

times lexicon recognition on the same caller logits (hctr_lexicon_logits, the 5 best of every line fetched) against
--entries synthetic entries of 2-6 labels, half of them cut from the lines' greedy texts, and in the same run the loss
(hctr_ctc_loss_logits, each line's greedy text as its target), alternately after warm-up calls of each, medians with
range, and the cost per (line, entry) next to the loss's per (line, target). --layers adds the device time of the call's
launches, summed per name over the chunks of units (lexicon_classes, ctc_lse, lexicon_trie; lexicon_rank).

    python tools/bench_ctc.py --words [--entries 1000] [--layers] ...

times word-sequence recognition (hctr_words_logits, every output fetched) against lexicon recognition
(hctr_lexicon_logits, the 5 best) on the same lexicon of --entries synthetic entries (as --lexicon's), the same caller
logits and in the same process, alternately after warm-up calls of each, medians with range; --entries 1000 gives a trie
of about 3 900 nodes (the LDS form), 10 000 one of about 34 000 (the scratch form). --layers adds the device time of each
call's launches (lexicon_classes, ctc_lse, words_trie, words_backtrace, ctc_alpha against lexicon_trie, lexicon_rank) and
the recursions' time per column.

    python tools/bench_ctc.py --pattern EXPR [--layers] ...

times pattern-constrained recognition on the same caller logits (hctr_pattern_logits) for the regular expression EXPR,
forward-only (logp alone) and full (every output fetched), and in the same run the loss (hctr_ctc_loss_logits, each
line's greedy text as its target), alternately after warm-up calls of each, medians with range. The expression is
compiled over a vocabulary whose labels 1..10 are the digits 0-9, 11-13 the year, month and day signs and the rest CJK
code points, e.g. '\\d{18}', '\\d{4}\u5e74\\d{1,2}\u6708\\d{1,2}\u65e5', '.\\d{3}'. --layers adds the device time of each call's
launches (pattern_classes, ctc_lse, pattern, pattern_trace, ctc_alpha) and the recursion's time per step. --sets builds
the set form (label-set arcs, the launch pattern_set), which a wildcard over the whole vocabulary needs ('.{2,4}',
'.*\u5e74.*'); where the explicit form builds as well ('.\\d{3}') both are timed alternately in the one process and their
Viterbi outputs compared bit for bit. --char-bonus X (with --pattern) builds the weighted form with X on every arc
(Pattern.compile(label_weights=X), the launch pattern_w) and --bigram N the dense weighted bigram over labels 1..N
(Pattern.bigram, random weights); the unweighted pattern of the same automaton is timed alternately in the same run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=64)
    ap.add_argument("--width", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--precision", default="f16", choices=["f16", "f16x3", "auto"])
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--backward", action="store_true")
    ap.add_argument("--align", action="store_true")
    ap.add_argument("--recognize", action="store_true")
    ap.add_argument("--evaluate", action="store_true")
    ap.add_argument("--nbest", action="store_true")
    ap.add_argument("--nbest-lm", action="store_true")
    ap.add_argument("--nbest-skip", action="store_true")
    ap.add_argument("--lm-sweep", action="store_true")
    ap.add_argument("--spot", action="store_true")
    ap.add_argument("--queries", type=int, default=16)
    ap.add_argument("--lexicon", action="store_true")
    ap.add_argument("--words", action="store_true")
    ap.add_argument("--entries", type=int, default=10000)
    ap.add_argument("--unit-nodes", type=int, default=0, help="--lexicon: trie nodes per workgroup (0 = the default)")
    ap.add_argument("--pattern", type=str, default="", help="a regular expression: time hctr_pattern_logits")
    ap.add_argument("--sets", action="store_true", help="with --pattern: build the set form (label-set arcs); where the "
                    "explicit form builds too, it is timed alternately in the same process")
    ap.add_argument("--char-bonus", type=float, default=0.0, help="with --pattern: a weight per character (the weighted "
                    "form); the unweighted pattern is timed alternately in the same process")
    ap.add_argument("--bigram", type=int, default=0, help="time the dense weighted bigram over labels 1..N beside the "
                    "unweighted pattern of the same automaton")
    ap.add_argument("--pairs", type=int, default=250)
    ap.add_argument("--host-lines", type=int, default=4)
    args = ap.parse_args()
    import torch
    import hctr_amd
    s = hctr_amd.synth
    C = s.DEFAULT_VOCAB + 2
    if args.nbest_skip:
        print(json.dumps(nbest_skip(args, hctr_amd)))
        return
    m = hctr_amd.hctr_model(C, precision=args.precision).cuda(0)
    m.load_state_dict(s.make_state_dict(C, seed=0))
    imgs = torch.from_numpy(s.make_line_images(args.lines, args.width, seed=2)).cuda(0)
    labels = m.greedy(imgs)
    tl = np.array([len(v) for v in labels], np.int32)
    targets = np.concatenate(labels).astype(np.int32)
    if args.backward:
        print(json.dumps(backward(args, hctr_amd, m, imgs, targets, tl)))
        return
    if args.align:
        print(json.dumps(align(args, hctr_amd, m, imgs, targets, tl)))
        return
    if args.recognize:
        print(json.dumps(recognize(args, hctr_amd, m, imgs)))
        return
    if args.spot:
        print(json.dumps(spot(args, hctr_amd, m, imgs, labels, targets, tl)))
        return
    if args.words:
        print(json.dumps(words(args, hctr_amd, m, imgs, labels)))
        return
    if args.lexicon:
        print(json.dumps(lexicon(args, hctr_amd, m, imgs, labels, targets, tl)))
        return
    if args.pattern or args.bigram:
        print(json.dumps(pattern(args, hctr_amd, m, imgs, targets, tl)))
        return
    if args.evaluate:
        print(json.dumps(evaluate(args, hctr_amd, m, imgs, labels)))
        return
    if args.nbest:
        print(json.dumps(nbest(args, hctr_amd, m, imgs)))
        return
    if args.nbest_lm:
        print(json.dumps(nbest_lm(args, hctr_amd, m, imgs)))
        return
    if args.lm_sweep:
        print(json.dumps(lm_sweep(args, hctr_amd, m, imgs, targets, tl)))
        return

    def t_greedy():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.greedy(imgs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def t_ctc():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        nll = m.ctc_loss(imgs, targets, tl, reduction="none", zero_infinity=False)
        torch.cuda.synchronize()
        assert torch.isfinite(nll).all()
        return time.perf_counter() - t0

    for _ in range(args.warmup):
        t_greedy()
        t_ctc()
    g, c = [], []
    for _ in range(args.steps):
        g.append(t_greedy())
        c.append(t_ctc())
    rec = {"lines": args.lines, "width": args.width, "precision": args.precision,
           "mean_target_length": float(tl.mean()), "max_target_length": int(tl.max()),
           "greedy_ms": [round(1e3 * v, 3) for v in g], "ctc_loss_ms": [round(1e3 * v, 3) for v in c],
           "greedy_ms_median": round(1e3 * float(np.median(g)), 3), "ctc_loss_ms_median": round(1e3 * float(np.median(c)), 3),
           "ratio_median": round(float(np.median(c) / np.median(g)), 4)}
    if args.layers:
        m.set_profiling(True)
        m.greedy(imgs)
        gprof = dict(m.last_profile())
        m.ctc_loss(imgs, targets, tl)
        prof = dict(m.last_profile())
        rec["greedy_layers_ms"] = {k: round(v, 4) for k, v in gprof.items() if "head" in k or "ctc" in k}
        rec["ctc_layers_ms"] = {k: round(v, 4) for k, v in prof.items() if "head" in k or "ctc" in k}
        rec["greedy_total_device_ms"] = round(sum(gprof.values()), 3)
        rec["ctc_total_device_ms"] = round(sum(prof.values()), 3)
        # every launch name whose time differs by more than 0.05 ms between the two calls (trunk layers are shared)
        rec["layer_delta_ms"] = {k: round(prof.get(k, 0.0) - gprof.get(k, 0.0), 4) for k in set(gprof) | set(prof)
                                 if abs(prof.get(k, 0.0) - gprof.get(k, 0.0)) > 0.05}
        m.set_profiling(False)
    print(json.dumps(rec))


def backward(args, hctr_amd, m, imgs, targets, tl):
    import torch
    ctc = hctr_amd.CTCLoss(reduction="none", zero_infinity=True).attach(m)
    mod = sys.modules[type(ctc).__module__]
    ctx = ctc._context()
    logits = m(imgs)                                             # device tensor [W, lines, C]
    W, B, C = (int(v) for v in logits.shape)
    grad = torch.empty_like(logits)
    tg_t, tl_t = torch.from_numpy(targets).long().cuda(0), torch.from_numpy(tl).long().cuda(0)
    il_t = torch.full((B,), W, dtype=torch.long, device="cuda:0")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def loss_only():
        assert np.isfinite(mod.loss_logits(ctx, logits, 1, targets, tl, None)).all()

    def loss_grad():
        assert np.isfinite(mod.loss_grad_logits(ctx, logits, 1, targets, tl, None, None, grad=grad)[0]).all()

    def torch_fb():
        x = logits.detach().requires_grad_()
        loss = torch.nn.functional.ctc_loss(x.log_softmax(2), tg_t, il_t, tl_t, reduction="sum", zero_infinity=True)
        loss.backward()
        assert x.grad is not None

    fns = (("loss_only", loss_only), ("loss_grad", loss_grad), ("torch_fwd_bwd", torch_fb))
    for _ in range(args.warmup):
        for _, fn in fns:
            fn()
    ms = {k: [] for k, _ in fns}
    for _ in range(args.steps):
        for k, fn in fns:
            ms[k].append(1e3 * timed(fn))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rec = {"mode": "backward", "lines": B, "width": W, "classes": C, "precision": args.precision,
           "mean_target_length": float(tl.mean()), "max_target_length": int(tl.max())}
    for k, v in ms.items():
        rec[k + "_ms"] = [round(x, 3) for x in v]
        rec[k + "_ms_median"] = round(med[k], 3)
    rec["loss_grad_over_loss_only"] = round(med["loss_grad"] / med["loss_only"], 4)
    rec["loss_grad_over_torch"] = round(med["loss_grad"] / med["torch_fwd_bwd"], 4)
    if args.layers:
        m.set_profiling(True)
        loss_only()
        fprof = dict(m.last_profile())
        loss_grad()
        gprof = dict(m.last_profile())
        m.set_profiling(False)
        rec["loss_only_layers_ms"] = {k: round(v, 4) for k, v in fprof.items()}
        rec["loss_grad_layers_ms"] = {k: round(v, 4) for k, v in gprof.items()}
        row = 4.0 * W * B * C
        if fprof.get("ctc_lse"):
            rec["ctc_lse_TBps"] = round(row / (1e-3 * fprof["ctc_lse"]) / 1e12, 3)
        if gprof.get("ctc_rowlse"):
            rec["ctc_rowlse_TBps"] = round(row / (1e-3 * gprof["ctc_rowlse"]) / 1e12, 3)
        if gprof.get("ctc_grad_rows"):
            rec["ctc_grad_rows_TBps"] = round(2 * row / (1e-3 * gprof["ctc_grad_rows"]) / 1e12, 3)
    return rec


def align(args, hctr_amd, m, imgs, targets, tl):
    import torch
    al = hctr_amd.CTCAligner().attach(m)
    mod = sys.modules[type(al).__module__]
    ctx = al._context()
    logits = m(imgs)                                             # device tensor [W, lines, C]
    W, B, C = (int(v) for v in logits.shape)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def loss_only():
        assert np.isfinite(mod.loss_logits(ctx, logits, 1, targets, tl, None)).all()

    def align_all():
        assert np.isfinite(mod.align_logits(ctx, logits, 1, targets, tl, None).scores).all()

    fns = (("loss_only", loss_only), ("align", align_all))
    for _ in range(args.warmup):
        for _, fn in fns:
            fn()
    ms = {k: [] for k, _ in fns}
    for _ in range(args.steps):
        for k, fn in fns:
            ms[k].append(1e3 * timed(fn))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rec = {"mode": "align", "lines": B, "width": W, "classes": C, "precision": args.precision,
           "mean_target_length": float(tl.mean()), "max_target_length": int(tl.max())}
    for k, v in ms.items():
        rec[k + "_ms"] = [round(x, 3) for x in v]
        rec[k + "_ms_median"] = round(med[k], 3)
    rec["align_over_loss_only"] = round(med["align"] / med["loss_only"], 4)
    if args.layers:
        m.set_profiling(True)
        loss_only()
        fprof = dict(m.last_profile())
        align_all()
        aprof = dict(m.last_profile())
        m.set_profiling(False)
        rec["loss_only_layers_ms"] = {k: round(v, 4) for k, v in fprof.items()}
        rec["align_layers_ms"] = {k: round(v, 4) for k, v in aprof.items()}
    return rec


def spot_queries(labels, C, Q, seed=3):
    """Q queries of length 2-4: the even ones cut from the lines' texts (line k mod B), the odd ones of classes no line
    decodes to (so they are absent from every 1-best text)"""
    rng = np.random.RandomState(seed)
    used = np.zeros(C, bool)
    for v in labels:
        used[np.asarray(v, np.int64)] = True
    free = np.flatnonzero(~used[1:C - 1]) + 1
    assert free.size >= 4, "every class is decoded somewhere: no absent query can be drawn"
    out = []
    for k in range(Q):
        n = int(rng.randint(2, 5))
        text = labels[k % len(labels)]
        if k % 2 == 0 and len(text) >= n:
            at = int(rng.randint(0, len(text) - n + 1))
            out.append([int(c) for c in text[at:at + n]])
        else:
            out.append([int(c) for c in rng.choice(free, size=n)])
    return out


def spot(args, hctr_amd, m, imgs, labels, targets, tl):
    import torch
    sp = hctr_amd.KeywordSpotter().attach(m)
    mod = sys.modules[type(sp).__module__]
    ctx = sp._context()
    logits = m(imgs)                                             # device tensor [W, lines, C]
    W, B, C = (int(v) for v in logits.shape)
    qs = spot_queries(labels, C, args.queries)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def loss_only():
        assert np.isfinite(mod.loss_logits(ctx, logits, 1, targets, tl, None)).all()

    last = {}

    def spot_all():
        last["r"] = mod.spot_logits(ctx, logits, 1, qs, None)
        assert not np.isnan(last["r"].logp).any()

    fns = (("loss_only", loss_only), ("spot", spot_all))
    for _ in range(args.warmup):
        for _, fn in fns:
            fn()
    ms = {k: [] for k, _ in fns}
    for _ in range(args.steps):
        for k, fn in fns:
            ms[k].append(1e3 * timed(fn))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    r = last["r"]
    drawn = np.arange(len(qs)) % 2 == 0
    rec = {"mode": "spot", "lines": B, "width": W, "classes": C, "precision": args.precision, "queries": len(qs),
           "chunk_classes": mod.spot_chunk_classes(B, W),
           "mean_prob_of_own_text_queries": round(float(np.mean([r.probs()[k % B, k] for k in np.flatnonzero(drawn)])), 4),
           "max_prob_of_absent_queries": float(r.probs()[:, ~drawn].max()) if (~drawn).any() else None}
    for k, v in ms.items():
        rec[k + "_ms"] = [round(x, 3) for x in v]
        rec[k + "_ms_median"] = round(med[k], 3)
    rec["spot_over_loss_only"] = round(med["spot"] / med["loss_only"], 4)
    if args.layers:
        m.set_profiling(True)
        loss_only()
        fprof = dict(m.last_profile())
        spot_all()
        sprof = dict(m.last_profile())
        m.set_profiling(False)
        rec["loss_only_layers_ms"] = {k: round(v, 4) for k, v in fprof.items()}
        rec["spot_layers_ms"] = {k: round(v, 4) for k, v in sprof.items()}
    return rec


def lexicon_entries(labels, C, N, seed=4):
    """N entries of 2-6 labels: the even ones cut from the lines' texts (line k mod B), the odd ones random"""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(N):
        n = int(rng.randint(2, 7))
        text = labels[k % len(labels)]
        if k % 2 == 0 and len(text) >= n:
            at = int(rng.randint(0, len(text) - n + 1))
            out.append([int(c) for c in text[at:at + n]])
        else:
            out.append([int(c) for c in rng.randint(1, C - 1, size=n)])
    return out


def lexicon(args, hctr_amd, m, imgs, labels, targets, tl):
    import torch
    rc = hctr_amd.LexiconRecognizer().attach(m)
    mod = sys.modules[type(rc).__module__]
    ctx = rc._context()
    logits = m(imgs)                                             # device tensor [W, lines, C]
    W, B, C = (int(v) for v in logits.shape)
    t0 = time.perf_counter()
    lex = mod.Lexicon(lexicon_entries(labels, C, args.entries), num_classes=C, unit_nodes=args.unit_nodes)
    build_ms = 1e3 * (time.perf_counter() - t0)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def loss_only():
        assert np.isfinite(mod.loss_logits(ctx, logits, 1, targets, tl, None)).all()

    last = {}

    def lexicon_all():
        last["r"] = mod.lexicon_logits(ctx, logits, 1, lex, 5, None, False)
        assert (last["r"].count > 0).all()

    fns = (("loss_only", loss_only), ("lexicon", lexicon_all))
    for _ in range(args.warmup):
        for _, fn in fns:
            fn()
    ms = {k: [] for k, _ in fns}
    for _ in range(args.steps):
        for k, fn in fns:
            ms[k].append(1e3 * timed(fn))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rec = {"mode": "lexicon", "lines": B, "width": W, "classes": C, "precision": args.precision, "build_ms": round(build_ms, 1),
           "chunk_classes": mod.lexicon_chunk_classes(B, W), "unit_nodes": args.unit_nodes}
    rec.update(lex.info())
    for k, v in ms.items():
        rec[k + "_ms"] = [round(x, 3) for x in v]
        rec[k + "_ms_median"] = round(med[k], 3)
    rec["lexicon_us_per_line_entry"] = round(1e3 * med["lexicon"] / (B * len(lex)), 5)
    rec["loss_us_per_line_target"] = round(1e3 * med["loss_only"] / B, 3)
    if args.layers:
        m.set_profiling(True)
        loss_only()
        fprof = dict(m.last_profile())
        lexicon_all()
        lprof = dict(m.last_profile())
        m.set_profiling(False)
        rec["loss_only_layers_ms"] = {k: round(v, 4) for k, v in fprof.items()}
        rec["lexicon_layers_ms"] = {k: round(v, 4) for k, v in lprof.items()}
    return rec


def words(args, hctr_amd, m, imgs, labels):
    import torch
    rc = hctr_amd.WordRecognizer().attach(m)
    mod = sys.modules[type(rc).__module__]
    ctx = rc._context()
    logits = m(imgs)                                             # device tensor [W, lines, C]
    W, B, C = (int(v) for v in logits.shape)
    lex = mod.Lexicon(lexicon_entries(labels, C, args.entries), num_classes=C)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    last = {}

    def lexicon_all():
        last["lexicon"] = mod.lexicon_logits(ctx, logits, 1, lex, 5, None, False)

    def words_all():
        last["words"] = mod.words_logits(ctx, logits, 1, lex, 0.0, None, None)

    fns = (("lexicon", lexicon_all), ("words", words_all))
    for _ in range(args.warmup):
        for _, fn in fns:
            fn()
    ms = {k: [] for k, _ in fns}
    for _ in range(args.steps):
        for k, fn in fns:
            ms[k].append(1e3 * timed(fn))
    rec = {"mode": "words", "lines": B, "width": W, "classes": C, "precision": args.precision,
           "form": "LDS" if lex.info()["nodes"] <= mod.WORDS_LDS_NODES and os.environ.get("HCTR_WORDS_LDS", "1") != "0"
           else "scratch"}
    rec.update(lex.info())
    for k, v in ms.items():
        rec[k + "_ms"] = [round(x, 3) for x in v]
        rec[k + "_ms_median"] = round(float(np.median(v)), 3)
    rec["lines_with_words"] = int((last["words"].count > 0).sum())
    rec["mean_words"] = round(float(last["words"].count.mean()), 1)
    if args.layers:
        m.set_profiling(True)
        lexicon_all()
        lprof = dict(m.last_profile())
        words_all()
        wprof = dict(m.last_profile())
        m.set_profiling(False)
        rec["lexicon_layers_ms"] = {k: round(v, 4) for k, v in lprof.items()}
        rec["words_layers_ms"] = {k: round(v, 4) for k, v in wprof.items()}
        rec["lexicon_trie_us_per_step"] = round(1e3 * lprof.get("lexicon_trie", 0.0) / W, 3)
        rec["words_trie_us_per_step"] = round(1e3 * wprof.get("words_trie", 0.0) / W, 3)
    return rec


def pattern_characters(vocab):
    """a vocabulary for --pattern: the digits, the year / month / day signs, then CJK code points from U+4E00"""
    head = "0123456789\u5e74\u6708\u65e5"
    out = list(head)
    cp = 0x4E00
    while len(out) < vocab:
        if chr(cp) not in head:
            out.append(chr(cp))
        cp += 1
    return "".join(out)


def pattern(args, hctr_amd, m, imgs, targets, tl):
    import torch
    rc = hctr_amd.PatternRecognizer().attach(m)
    mod = sys.modules[type(rc).__module__]
    ctx = rc._context()
    logits = m(imgs)                                             # device tensor [W, lines, C]
    W, B, C = (int(v) for v in logits.shape)
    t0 = time.perf_counter()
    codec = hctr_amd.ctc_codec(pattern_characters(C - 2))
    unweighted = None
    if args.bigram:
        rng, n = np.random.RandomState(7), args.bigram
        pat = mod.Pattern.bigram(np.arange(1, n + 1), rng.randn(n, n), rng.randn(n), rng.randn(n), num_classes=C)
    elif args.char_bonus != 0.0:
        pat = mod.Pattern.compile(args.pattern, codec, label_weights=args.char_bonus)
    else:
        pat = mod.Pattern.compile(args.pattern, codec, sets=True if args.sets else None)
    build_ms = 1e3 * (time.perf_counter() - t0)
    if pat.kind == 2:
        unweighted = mod.Pattern(pat.arcs, pat.finals, pat.num_states, C)
    explicit = None
    if args.sets and pat.kind == 1:
        try:
            explicit = mod.Pattern.compile(args.pattern, codec, sets=False)
        except ValueError:
            pass                                                 # beyond the explicit form's limits

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def loss_only():
        assert np.isfinite(mod.loss_logits(ctx, logits, 1, targets, tl, None)).all()

    last = {}

    def forward_only():
        last["f"] = mod.pattern_logits(ctx, logits, 1, pat, None, False)

    def full():
        last["r"] = mod.pattern_logits(ctx, logits, 1, pat, None, True)

    fns = (("loss_only", loss_only), ("pattern_forward", forward_only), ("pattern_full", full))
    if explicit is not None:
        fns += (("explicit_forward", lambda: last.update(ef=mod.pattern_logits(ctx, logits, 1, explicit, None, False))),
                ("explicit_full", lambda: last.update(er=mod.pattern_logits(ctx, logits, 1, explicit, None, True))))
    if unweighted is not None:
        fns += (("unweighted_forward", lambda: last.update(uf=mod.pattern_logits(ctx, logits, 1, unweighted, None, False))),
                ("unweighted_full", lambda: last.update(ur=mod.pattern_logits(ctx, logits, 1, unweighted, None, True))))
    for _ in range(args.warmup):
        for _, fn in fns:
            fn()
    ms = {k: [] for k, _ in fns}
    for _ in range(args.steps):
        for k, fn in fns:
            ms[k].append(1e3 * timed(fn))
    assert last["f"].logp.tobytes() == last["r"].logp.tobytes()
    info = pat.info()
    if explicit is not None:                                     # the Viterbi outputs of the two forms: the same bits
        for f in last["r"].FIELDS[1:]:
            assert getattr(last["r"], f).tobytes() == getattr(last["er"], f).tobytes(), f
    rec = {"mode": "pattern", "pattern": args.pattern or "bigram %d" % args.bigram, "kind": pat.kind,
           "instance": list(pat.instance(True)) + list(pat.instance(False)) if pat.kind != 1 else None, "lines": B, "width": W, "classes": C, "precision": args.precision,
           "build_ms": round(build_ms, 1), "group_lines": mod.pattern_group_lines(info["states"], info["classes"] + 1, W),
           "matching_lines": int(np.isfinite(last["r"].logp).sum())}
    rec.update(info)
    for k, v in ms.items():
        rec[k + "_ms"] = [round(x, 3) for x in v]
        rec[k + "_ms_median"] = round(float(np.median(v)), 3)
    if args.layers:
        m.set_profiling(True)
        prof = {}
        for k, fn in fns:
            fn()
            prof[k] = dict(m.last_profile())
        m.set_profiling(False)
        for k, v in prof.items():
            rec[k + "_layers_ms"] = {n: round(x, 4) for n, x in v.items()}
        groups = -(-B // rec["group_lines"])
        for k in prof:                                       # a group's lines run side by side, the groups in turn
            if k != "loss_only":
                kernel = ("pattern" if k.startswith("explicit") or k.startswith("unweighted") or not pat.kind else
                          "pattern_set" if pat.kind == 1 else "pattern_w")
                rec[k + "_us_per_step"] = round(1e3 * prof[k].get(kernel, 0.0) / (W * groups), 3)
    return rec


def recognize(args, hctr_amd, m, imgs):
    import torch
    al = hctr_amd.CTCAligner().attach(m)
    mod = sys.modules[type(al).__module__]
    lib, ptr = hctr_amd.load_library(), mod._lib.ptr
    ctx = al._context()
    logits = m(imgs)                                             # device tensor [W, lines, C]
    W, B, C = (int(v) for v in logits.shape)
    labels, lengths = np.empty((B, W), np.int32), np.empty((B,), np.int32)
    prof, profiling = {}, [False]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def keep(name):
        if profiling[0]:
            prof[name] = dict(m.last_profile())

    def fused():
        rec = mod.recognize_logits(ctx, logits, 1)
        keep("recognize")
        assert np.isfinite(rec.text_nll).all()
        return rec

    def chain():
        rc = lib.hctr_decode_greedy_logits(ctx, ptr(logits), 1, W, B, C, ptr(labels), ptr(lengths))
        assert rc == 0
        keep("decode")
        tg = np.concatenate([labels[b, :lengths[b]] for b in range(B)]).astype(np.int32)
        nll = mod.loss_logits(ctx, logits, 1, tg, lengths, None)
        keep("loss")
        a = mod.align_logits(ctx, logits, 1, tg, lengths, None)
        keep("align")
        assert np.isfinite(nll).all() and np.isfinite(a.scores).all()
        return nll

    fns = (("recognize", fused), ("chain", chain))
    for _ in range(args.warmup):
        for _, fn in fns:
            fn()
    ms = {k: [] for k, _ in fns}
    for _ in range(args.steps):
        for k, fn in fns:
            ms[k].append(1e3 * timed(fn))
    med = {k: float(np.median(v)) for k, v in ms.items()}
    rec = {"mode": "recognize", "lines": B, "width": W, "classes": C, "precision": args.precision,
           "mean_text_length": float(lengths.mean()), "max_text_length": int(lengths.max())}
    for k, v in ms.items():
        rec[k + "_ms"] = [round(x, 3) for x in v]
        rec[k + "_ms_median"] = round(med[k], 3)
    rec["recognize_over_chain"] = round(med["recognize"] / med["chain"], 4)
    assert fused().text_nll.tobytes() == chain().tobytes()       # the same loss, bit for bit
    if args.layers:
        m.set_profiling(True)
        profiling[0] = True
        rows = {"greedy_rowstat": [], "argmax_rows": [], "ctc_lse": []}
        for _ in range(args.steps):                              # alternating, median of each launch
            fused()
            chain()
            rows["greedy_rowstat"].append(prof["recognize"]["greedy_rowstat"])
            rows["argmax_rows"].append(prof["decode"]["argmax_rows"])
            rows["ctc_lse"].append(prof["loss"]["ctc_lse"])
        m.set_profiling(False)
        profiling[0] = False
        for k, v in prof.items():
            rec[k + "_layers_ms"] = {n: round(t, 4) for n, t in v.items()}
        for k, v in rows.items():
            rec[k + "_ms_median"] = round(float(np.median(v)), 4)
        two = float(np.median(rows["argmax_rows"])) + float(np.median(rows["ctc_lse"]))
        rec["rowstat_over_two_passes"] = round(float(np.median(rows["greedy_rowstat"])) / two, 4)
        rec["greedy_rowstat_TBps"] = round(4.0 * W * B * C / (1e-3 * float(np.median(rows["greedy_rowstat"]))) / 1e12, 3)
    return rec


def nbest(args, hctr_amd, m, imgs):
    import torch
    from hctr_amd import package
    ctc = sys.modules[package.__name__ + ".ctc"]
    B, W = int(imgs.shape[0]), int(imgs.shape[-1])
    C, k, beam, n, bonus = int(m.noutput), 10, 10, 5, 5.8
    codec = hctr_amd.ctc_codec(hctr_amd.synth.characters()).attach(m)
    codec.set_beam_search(ngram_path="zero", use_tfm_pred=False, len_bonus=bonus, beam_size=beam, search_depth=k)
    codec.num_threads = 16
    fe = m.beam_frontend(imgs, k)
    top1 = fe["topk_idx"][:, :, 0]
    ends = np.empty(B, np.int32)
    for b in range(B):                                             # the reference's end step: last greedy character + 4
        t = top1[:, b]
        keep = (t != 0) & (t != C - 1)
        keep[1:] &= t[1:] != t[:-1]
        ends[b] = min(int(np.flatnonzero(keep)[-1]) + 4, W)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    calls = {"nbest_images": lambda: m.nbest(imgs, n=n, beam=beam, depth=k, len_bonus=bonus, input_lengths=ends),
             "frontend": lambda: m.beam_frontend(imgs, k),
             "host_search": lambda: codec.decode_frontend(fe),
             "nbest_topk": lambda: ctc.nbest_topk(m._ctx, fe["topk_idx"], fe["topk_logp"], C, n, beam, bonus, ends)}
    for _ in range(args.warmup):
        for f in calls.values():
            f()
    ms = {name: [] for name in calls}
    out = {}
    for _ in range(args.steps):
        for name, f in calls.items():
            dt, out[name] = timed(f)
            ms[name].append(1e3 * dt)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    m.set_profiling(True)
    calls["nbest_images"]()
    prof = dict(m.last_profile())
    m.set_profiling(False)
    search_dev = prof.get("prefix_beam", 0.0) + prof.get("prefix_backtrace", 0.0)
    one_best = codec.labels_to_text([line[0] for line in out["nbest_topk"].label_lists()])
    return {"mode": "nbest", "lines": B, "width": W, "classes": C, "precision": args.precision, "beam": beam, "depth": k,
            "nbest": n, "host_threads": 16, "mean_steps": float(ends.mean()),
            "device_search_ms": round(search_dev, 3),
            "device_search_launches_ms": {key: round(prof.get(key, 0.0), 4) for key in ("prefix_beam", "prefix_backtrace")},
            "nbest_topk_call_ms_median": round(med["nbest_topk"], 3),
            "frontend_d2h_host_search_ms_median": round(med["frontend"] + med["host_search"], 3),
            "host_search_ms_median": round(med["host_search"], 3),
            "frontend_alone_ms_median": round(med["frontend"], 3),
            "nbest_images_call_ms_median": round(med["nbest_images"], 3),
            "nbest_images_device_ms": round(sum(prof.values()), 3),
            "ms": {name: [round(v, 3) for v in vals] for name, vals in ms.items()},
            "one_best_equals_host_search": one_best == out["host_search"],
            "mean_text_length": float(np.mean([len(t) for t in one_best]))}


def write_bench_arpa(path, chars, order=5, counts=(0, 100000, 100000, 70000, 50000), seed=5):
    """Deterministic ARPA model over ``chars`` (+ <unk>, <s>, </s>): every unigram, and counts[n-1] random n-grams of each
    higher order, each an n-gram of the order below plus one word. Returns the number of n-grams."""
    rng = np.random.RandomState(seed)
    words = ["<unk>", "<s>", "</s>"] + list(chars)
    V = len(words)
    grams = [[(i,) for i in range(V)]]
    for n in range(2, order + 1):
        prev = [g for g in grams[-1] if g[-1] != 2]                # (nothing follows </s>)
        pick = rng.randint(0, len(prev), counts[n - 1])
        tail = rng.randint(2, V, counts[n - 1])                    # (<unk> and <s> end no n-gram here)
        grams.append(sorted(set(prev[int(i)] + (int(w),) for i, w in zip(pick, tail))))
    with open(path, "w", encoding="utf-8") as f:
        f.write("\\data\\\n" + "".join("ngram %d=%d\n" % (n + 1, len(g)) for n, g in enumerate(grams)))
        for n, gs in enumerate(grams, 1):
            f.write("\n\\%d-grams:\n" % n)
            p = -0.2 - (5.0 - 0.8 * n) * rng.rand(len(gs))
            bo = -0.1 - 0.6 * rng.rand(len(gs))
            for g, pv, bv in zip(gs, p, bo):
                text = " ".join(words[i] for i in g)
                f.write("%.6f\t%s\t%.6f\n" % (pv, text, bv) if n < order and g[-1] != 2 else "%.6f\t%s\n" % (pv, text))
        f.write("\n\\end\\\n")
    return sum(len(g) for g in grams)


def nbest_lm(args, hctr_amd, m, imgs):
    import tempfile
    import torch
    from hctr_amd import package
    ctc = sys.modules[package.__name__ + ".ctc"]
    B, W = int(imgs.shape[0]), int(imgs.shape[-1])
    C, k, beam, n, pen, bonus = int(m.noutput), 10, 10, 5, 2.0, 5.8
    chars = hctr_amd.synth.characters()
    codec = hctr_amd.ctc_codec(chars).attach(m)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench5.arpa")
        ngrams = write_bench_arpa(path, chars)
        codec.set_beam_search(ngram_path=path, use_tfm_pred=False, lm_panelty=pen, len_bonus=bonus, beam_size=beam,
                              search_depth=k)                      # (an .arpa path: the native ArpaLM, read here)
    lm = codec.ngram
    codec.num_threads = 16
    flat = lm.flat(codec.characters)
    fe = m.beam_frontend(imgs, k)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def lm_topk():
        return ctc.nbest_topk(m._ctx, fe["topk_idx"], fe["topk_logp"], C, n, beam, bonus, None, lm=flat, lm_panelty=pen)

    calls = {"nbest_lm_images": lambda: m.nbest(imgs, n=n, beam=beam, depth=k, len_bonus=bonus, lm=lm, lm_panelty=pen,
                                                codec=codec),
             "host_search": lambda: codec.decode_frontend(fe),
             "nbest_lm_topk": lm_topk}
    for _ in range(args.warmup):
        for f in calls.values():
            f()
    ms = {name: [] for name in calls}
    out = {}
    for _ in range(args.steps):
        for name, f in calls.items():
            dt, out[name] = timed(f)
            ms[name].append(1e3 * dt)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    m.set_profiling(True)
    lm_topk()
    prof = dict(m.last_profile())
    top1 = fe["topk_idx"][:, :, 0]
    ends = np.empty(B, np.int32)
    for b in range(B):                                             # the reference's end step: last greedy character + 4
        t = top1[:, b]
        keep = (t != 0) & (t != C - 1)
        keep[1:] &= t[1:] != t[:-1]
        ends[b] = min(int(np.flatnonzero(keep)[-1]) + 4, W)
    ctc.nbest_topk(m._ctx, fe["topk_idx"], fe["topk_logp"], C, n, beam, bonus, ends)
    zero = dict(m.last_profile())
    m.set_profiling(False)
    names = ("beam_lm_prepass", "prefix_beam_lm", "prefix_backtrace")
    one_best = codec.labels_to_text([line[0] if line else [] for line in out["nbest_lm_topk"].label_lists()])
    differ = sum(a != b for a, b in zip(one_best, out["host_search"]))
    same_entries = all(getattr(out["nbest_lm_topk"], f).tobytes() == getattr(out["nbest_lm_images"], f).tobytes()
                       for f in ("labels", "lengths", "logps", "scores", "counts", "lm_scores"))
    return {"mode": "nbest-lm", "lines": B, "width": W, "classes": C, "precision": args.precision, "beam": beam, "depth": k,
            "nbest": n, "lm_order": lm.order, "lm_ngrams": ngrams, "lm_panelty": pen, "len_bonus": bonus,
            "host_threads": 16, "mean_steps": float(ends.mean()),
            "device_search_ms": round(sum(prof.get(key, 0.0) for key in names), 3),
            "device_search_launches_ms": {key: round(prof.get(key, 0.0), 4) for key in names},
            "zero_lm_prefix_beam_ms": round(zero.get("prefix_beam", 0.0), 3),
            "nbest_lm_topk_call_ms_median": round(med["nbest_lm_topk"], 3),
            "nbest_lm_images_call_ms_median": round(med["nbest_lm_images"], 3),
            "host_search_ms_median": round(med["host_search"], 3),
            "ms": {name: [round(v, 3) for v in vals] for name, vals in ms.items()},
            "one_best_lines_differing_from_host_search": int(differ),
            "images_entry_equals_topk_entry": bool(same_entries),
            "mean_text_length": float(np.mean([len(t) for t in one_best])),
            "mean_lm_score": float(np.mean(out["nbest_lm_topk"].lm_scores[:, 0]))}


def lm_sweep(args, hctr_amd, m, imgs, targets, tl):
    import tempfile
    import torch
    from hctr_amd import package
    ctc = sys.modules[package.__name__ + ".ctc"]
    B, W = int(imgs.shape[0]), int(imgs.shape[-1])
    C, k, beam, G = int(m.noutput), 10, 10, int(args.pairs)
    chars = hctr_amd.synth.characters()
    codec = hctr_amd.ctc_codec(chars)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench5.arpa")
        ngrams = write_bench_arpa(path, chars)
        lm = hctr_amd.ArpaLM(path)
    flat = lm.flat(codec.characters)
    fe = m.beam_frontend(imgs, k)
    idx, lp = fe["topk_idx"], fe["topk_logp"]
    al, be = ctc.sweep_pairs(np.linspace(0.7, 1.1, 10), np.linspace(4.2, 6.6, 25))      # the reference's default grid
    reps = -(-G // al.size)
    grid = list(zip(np.tile(al, reps)[:G].tolist(), np.tile(be, reps)[:G].tolist()))

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def sweep():
        return ctc.lm_sweep_topk(m._ctx, idx, lp, C, targets, tl, flat, pairs=grid, beam=beam).edits

    def successive():
        out = np.zeros((G, B), np.int32)
        for g, (a, b) in enumerate(grid):
            nb = ctc.nbest_topk(m._ctx, idx, lp, C, 1, beam, b, None, lm=flat, lm_panelty=a)
            out[g] = ctc.edit_distance_labels(m._ctx, nb.labels[:, 0], nb.lengths[:, 0], targets, tl, maps=False).edits
        return out

    calls = {"lm_sweep": sweep, "successive": successive}
    for _ in range(args.warmup):
        for f in calls.values():
            f()
    ms = {name: [] for name in calls}
    out = {}
    for step in range(args.steps):
        for name, f in calls.items():
            dt, out[name] = timed(f)
            ms[name].append(1e3 * dt)
            print("step %d %s: %.1f ms" % (step, name, 1e3 * dt), file=sys.stderr, flush=True)      # (a step takes a while)
    if not np.array_equal(out["lm_sweep"], out["successive"]):
        raise SystemExit("the sweep and the successive calls disagree on %d of %d edits values"
                         % (int((out["lm_sweep"] != out["successive"]).sum()), out["lm_sweep"].size))
    med = {name: float(np.median(v)) for name, v in ms.items()}
    m.set_profiling(True)
    sweep()
    prof = dict(m.last_profile())
    names = ("beam_lm_prepass", "prefix_beam_lm", "prefix_backtrace", "edit_distance")
    single = {key: 0.0 for key in names}
    for a, b in grid:
        nb = ctc.nbest_topk(m._ctx, idx, lp, C, 1, beam, b, None, lm=flat, lm_panelty=a)
        for key, v in dict(m.last_profile()).items():
            if key in single:
                single[key] += v
        ctc.edit_distance_labels(m._ctx, nb.labels[:, 0], nb.lengths[:, 0], targets, tl, maps=False)
        single["edit_distance"] += dict(m.last_profile()).get("edit_distance", 0.0)
    m.set_profiling(False)
    sweep_names = ("beam_lm_prepass", "prefix_beam_lm_grid", "prefix_backtrace", "edit_distance")
    chunk = ctc.lm_sweep_chunk(B, W, beam, G)
    cer = out["lm_sweep"].astype(np.int64).sum(axis=1) / float(max(int(np.sum(tl)), 1))
    return {"mode": "lm-sweep", "lines": B, "width": W, "classes": C, "precision": args.precision, "beam": beam, "depth": k,
            "pairs": G, "chunk": chunk, "launches": -(-G // chunk), "lm_order": lm.order, "lm_ngrams": ngrams,
            "edits_equal": True, "distinct_cer_values": int(np.unique(cer).size),
            "sweep_device_ms": round(sum(prof.get(key, 0.0) for key in sweep_names), 3),
            "sweep_device_launches_ms": {key: round(prof.get(key, 0.0), 4) for key in sweep_names},
            "successive_device_ms": round(sum(single.values()), 3),
            "successive_device_launches_ms": {key: round(v, 4) for key, v in single.items()},
            "sweep_call_ms_median": round(med["lm_sweep"], 3),
            "successive_calls_ms_median": round(med["successive"], 3),
            "successive_over_sweep_wall": round(med["successive"] / med["lm_sweep"], 3),
            "successive_over_sweep_device": round(sum(single.values()) / max(sum(prof.get(key, 0.0) for key in sweep_names), 1e-9), 3),
            "ms": {name: [round(v, 3) for v in vals] for name, vals in ms.items()}}


def nbest_skip(args, hctr_amd):
    import tempfile
    import torch
    from hctr_amd import package
    ctc = sys.modules[package.__name__ + ".ctc"]
    s = hctr_amd.synth
    C, k, beam, n, pen, bonus = s.DEFAULT_VOCAB + 2, 10, 10, 5, 2.0, 5.8
    m = hctr_amd.hctr_model(C, precision=args.precision).cuda(0)
    m.load_state_dict(s.make_state_dict(C, seed=0, head="trained"))
    imgs = torch.from_numpy(s.make_font_lines(args.lines, args.width, seed=2)).cuda(0)
    B, W = int(imgs.shape[0]), int(imgs.shape[-1])
    chars = s.characters()
    codec = hctr_amd.ctc_codec(chars).attach(m)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench5.arpa")
        ngrams = write_bench_arpa(path, chars)
        codec.set_beam_search(ngram_path=path, use_tfm_pred=False, lm_panelty=pen, len_bonus=bonus, beam_size=beam,
                              search_depth=k, skip_search=True)
    lm = codec.ngram
    codec.num_threads = 16
    flat = lm.flat(codec.characters)
    fe = m.beam_frontend(imgs, k, want_candidates=True)
    top1 = np.ascontiguousarray(fe["topk_idx"][:, :, 0])

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def skip_lists():
        return ctc.nbest_skip_lists(m._ctx, top1, fe["blank_logp"], fe["cand_off"], fe["cand_idx"], fe["cand_logp"], C, n,
                                    beam, bonus, None, lm=flat, lm_panelty=pen)

    def full_topk():
        return ctc.nbest_topk(m._ctx, fe["topk_idx"], fe["topk_logp"], C, n, beam, bonus, None, lm=flat, lm_panelty=pen)

    def host_skip():
        try:
            return codec.decode_frontend(fe)
        except IndexError:                                         # a line emptied: the reference's IndexError
            return None

    calls = {"nbest_skip_lists": skip_lists, "nbest_lm_topk": full_topk, "host_skip_search": host_skip,
             "nbest_skip_images": lambda: m.nbest(imgs, n=n, beam=beam, len_bonus=bonus, lm=lm, lm_panelty=pen, codec=codec,
                                                  skip_search=True)}
    for _ in range(args.warmup):
        for f in calls.values():
            f()
    ms = {name: [] for name in calls}
    out = {}
    for _ in range(args.steps):
        for name, f in calls.items():
            dt, out[name] = timed(f)
            ms[name].append(1e3 * dt)
    med = {name: float(np.median(v)) for name, v in ms.items()}
    m.set_profiling(True)
    skip_lists()
    prof_skip = dict(m.last_profile())
    full_topk()
    prof_full = dict(m.last_profile())
    m.set_profiling(False)
    res = out["nbest_skip_lists"]
    rows = np.diff(fe["cand_off"]).reshape(W, B)
    # the steps the skip search ran: the reference's end steps, from the front end's top-1 classes
    ends = np.zeros(B, np.int64)
    for b in range(B):
        t = top1[:, b]
        keep = (t != 0) & (t != C - 1)
        keep[1:] &= t[1:] != t[:-1]
        ends[b] = min(int(np.flatnonzero(keep)[-1]) + 4, W) if keep.any() else 0
    steps = int(ends.sum())
    one_best = codec.labels_to_text([line[0] if line else [] for line in res.label_lists()])
    host = out["host_skip_search"]
    full_best = codec.labels_to_text([line[0] if line else [] for line in out["nbest_lm_topk"].label_lists()])
    same_entries = all(getattr(res, f).tobytes() == getattr(out["nbest_skip_images"], f).tobytes()
                       for f in ("labels", "lengths", "logps", "scores", "counts", "lm_scores", "status", "ranked"))
    skip_names = ("beam_lm_prepass", "prefix_beam_skip", "prefix_backtrace")
    full_names = ("beam_lm_prepass", "prefix_beam_lm", "prefix_backtrace")
    return {"mode": "nbest-skip", "lines": B, "width": W, "classes": C, "precision": args.precision, "beam": beam,
            "nbest": n, "lm_order": lm.order, "lm_ngrams": ngrams, "lm_panelty": pen, "len_bonus": bonus,
            "host_threads": 16, "mean_steps": float(ends.mean()),
            "ranked_steps": int(res.ranked.sum()), "steps": steps,
            "in_place_share": round(1.0 - float(res.ranked.sum()) / max(steps, 1), 4),
            "largest_row": int(max(int(rows[:int(ends[b]), b].max()) if ends[b] else 0 for b in range(B))),
            "status_counts": {str(v): int((res.status == v).sum()) for v in range(4)},
            "skip_search_device_ms": round(sum(prof_skip.get(key, 0.0) for key in skip_names), 3),
            "skip_search_launches_ms": {key: round(prof_skip.get(key, 0.0), 4) for key in skip_names},
            "full_search_device_ms": round(sum(prof_full.get(key, 0.0) for key in full_names), 3),
            "full_search_launches_ms": {key: round(prof_full.get(key, 0.0), 4) for key in full_names},
            "nbest_skip_lists_call_ms_median": round(med["nbest_skip_lists"], 3),
            "nbest_lm_topk_call_ms_median": round(med["nbest_lm_topk"], 3),
            "host_skip_search_ms_median": round(med["host_skip_search"], 3),
            "nbest_skip_images_call_ms_median": round(med["nbest_skip_images"], 3),
            "ms": {name: [round(v, 3) for v in vals] for name, vals in ms.items()},
            "one_best_lines_differing_from_host_skip_search":
                None if host is None else int(sum(a != b for a, b in zip(one_best, host))),
            "one_best_lines_differing_from_full_search": int(sum(a != b for a, b in zip(one_best, full_best))),
            "images_entry_equals_lists_entry": bool(same_entries),
            "mean_text_length": float(np.mean([len(t) for t in one_best]))}


def evaluate(args, hctr_amd, m, imgs, labels):
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location("hctr_test_cli", os.path.join(ROOT, "test.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    s = hctr_amd.synth
    C = s.DEFAULT_VOCAB + 2
    mod = sys.modules[hctr_amd.CTCLoss.__module__]
    rng = np.random.RandomState(7)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def shape(name, model, images, widths, truths, host_lines):
        """truths: list of int label lists; the hypotheses are the model's greedy decode of images"""
        ctx = model._ctx
        hyps = [v.tolist() for v in model.greedy(images, widths=widths)]
        lab, n = mod.pad_sequences(hyps)
        tl = np.array([len(t) for t in truths], np.int32)
        tg = np.concatenate([np.asarray(t, np.int32) for t in truths]).astype(np.int32)
        nh = len(hyps) if host_lines <= 0 else min(host_lines, len(hyps))

        def host(k=nh):
            return [cli.edit_distance(hyps[b], truths[b]) for b in range(k)]

        fns = {"edit_distance_only": lambda: mod.edit_distance_labels(ctx, lab, n, tg, tl, maps=False).edits,
               "edit_distance_maps": lambda: mod.edit_distance_labels(ctx, lab, n, tg, tl).edits,
               "evaluate_only": lambda: model.evaluate(images, tg, tl, widths=widths, maps=False).edits,
               "evaluate_maps": lambda: model.evaluate(images, tg, tl, widths=widths).edits,
               "greedy": lambda: model.greedy(images, widths=widths)}
        if nh == len(hyps):
            fns["host_loop"] = host
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        ms = {k: [] for k in fns}
        outs = {}
        for _ in range(args.steps):
            for k, fn in fns.items():
                t, outs[k] = timed(fn)
                ms[k].append(t)
        rec = {"lines": len(hyps), "mean_hyp_length": float(n.mean()), "mean_ref_length": float(tl.mean()),
               "cells": int((n.astype(np.int64) * tl).sum())}
        for k, v in ms.items():
            rec[k + "_ms"] = [round(x, 3) for x in v]
            rec[k + "_ms_median"] = round(float(np.median(v)), 3)
        if nh == len(hyps):
            want, host_ms = outs["host_loop"], float(np.median(ms["host_loop"]))
        else:
            t, want = timed(host)
            host_ms = t * float((n.astype(np.int64) * tl).sum()) / float((n[:nh].astype(np.int64) * tl[:nh]).sum())
            rec["host_loop_ms_measured_on_%d_lines" % nh] = round(t, 3)
            rec["host_loop_ms_scaled_by_cells"] = round(host_ms, 3)
        for k in ("edit_distance_only", "edit_distance_maps", "evaluate_only", "evaluate_maps"):
            assert outs[k][:nh].tolist() == want, k
        rec["host_loop_over_edit_distance_only"] = round(host_ms / float(np.median(ms["edit_distance_only"])), 3)
        rec["host_loop_over_edit_distance_maps"] = round(host_ms / float(np.median(ms["edit_distance_maps"])), 3)
        rec["greedy_plus_host_loop_ms"] = round(float(np.median(ms["greedy"])) + host_ms, 3)
        rec["greedy_plus_host_loop_over_evaluate_only"] = round(
            rec["greedy_plus_host_loop_ms"] / float(np.median(ms["evaluate_only"])), 3)
        rec["greedy_plus_host_loop_over_evaluate_maps"] = round(
            rec["greedy_plus_host_loop_ms"] / float(np.median(ms["evaluate_maps"])), 3)
        model.set_profiling(True)
        model.evaluate(images, tg, tl, widths=widths)
        rec["evaluate_maps_layers_ms"] = {k: round(v, 4) for k, v in dict(model.last_profile()).items() if "edit" in k or "ctc" in k}
        model.set_profiling(False)
        return rec

    def altered(lab):
        out = [int(v) for v in lab]
        for i in np.flatnonzero(rng.rand(len(out)) < 0.1)[::-1]:
            kind = rng.randint(3)
            if kind == 0:
                out[i] = int(rng.randint(1, C - 1))
            elif kind == 1:
                del out[i]
            else:
                out.insert(i, int(rng.randint(1, C - 1)))
        return out

    rec = {"mode": "evaluate", "width": args.width, "precision": args.precision}
    rec["long"] = shape("long", m, imgs, None, [altered(v) for v in labels], args.host_lines)
    del m
    mt = hctr_amd.hctr_model(C, precision=args.precision).cuda(0)
    mt.load_state_dict(s.make_state_dict(C, seed=0, head="trained"))
    font, boxes = s.make_font_lines(args.lines, args.width, 11, with_truth=True)
    codec = hctr_amd.ctc_codec(s.characters())
    truths = [codec.encode([s.font_truth_text(bx, args.width)])[0].tolist() for bx in boxes]
    rec["short"] = shape("short", mt, torch.from_numpy(font).cuda(0), None, truths, 0)
    # the entry alone at the shape the reference's -bm loop sees: `lines` lines of exactly 40 characters
    refs = [rng.randint(1, C - 1, 40).tolist() for _ in range(args.lines)]
    hyps = [altered(r) for r in refs]
    lab, n = mod.pad_sequences(hyps)
    tl = np.full(args.lines, 40, np.int32)
    tg = np.asarray(refs, np.int32).reshape(-1)
    fns = {"edit_distance_only": lambda: mod.edit_distance_labels(mt._ctx, lab, n, tg, tl, maps=False).edits.tolist(),
           "edit_distance_maps": lambda: mod.edit_distance_labels(mt._ctx, lab, n, tg, tl).edits.tolist(),
           "host_loop": lambda: [cli.edit_distance(h, r) for h, r in zip(hyps, refs)]}
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
    ms, outs = {k: [] for k in fns}, {}
    for _ in range(max(args.steps, 20)):
        for k, fn in fns.items():
            t, outs[k] = timed(fn)
            ms[k].append(t)
    assert outs["edit_distance_only"] == outs["edit_distance_maps"] == outs["host_loop"]
    rec["lines40"] = {k + "_ms_median": round(float(np.median(v)), 4) for k, v in ms.items()}
    rec["lines40"].update({k + "_ms_min": round(float(np.min(v)), 4) for k, v in ms.items()})
    rec["lines40"]["lines"] = args.lines
    return rec


if __name__ == "__main__":
    main()
