"""bench.py - hot-path throughput of the hctr engine on MI355X (driver contract: see DESIGN.md section 5).

  python bench.py --gpus 1 --steps K --warmup W
  python bench.py --gpus N --steps K --warmup W          (N > 1: starts its own N ranks as child processes)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A step = one pass of the hot path (NormalizePAD -> hctr trunk -> head -> argmax -> CTC collapse -> labels on the host,
+ one RCCL gather to rank 0 when N > 1) over one batch of synthetic line images.
N = 1: BASELINE.json configs[1], B=64 lines of 1x128x2000, greedy decode. N > 1: configs[3], a FIXED global batch of
4096 lines cut into contiguous shards of 4096/N (strong scaling), every rank's labels gathered to rank 0 once per step.
Inputs are uint8 images already resident in HBM when the timed region starts, drawn from fixed seeds (identical from
run to run); value = global lines / max-over-ranks time, ms_per_step = that time / K. A plain run times the headline
mode only. With --full the line also carries roofline / whole_forward (per-layer HIP events on the engine's stream
during the timed steps) and, at N = 1, from the same process and the same timing loop:
  parity_vs_cpu                the headline's 64-line text parity against the REAL reference's strings
  value_f16x3 / value_auto     the two other precision modes (one context holds both weight sets), with the 64-line text
                               parity of each against the REAL reference's strings and auto's re-run line count
  value_incl_h2d               the reference's own bracket (test.py:189-195): u8 batch in pinned host memory -> labels
  trained_checkpoint           f16 and auto on the trained-like checkpoint (peaky logits)
  configs.c3 / configs.c5      BASELINE configs[2] (512 lines, 4 width buckets) and configs[4] (256 lines, beam 10/10)
  cpu_baseline                 the oracle on the host cores
--dump-outputs DIR writes the labels of the headline's last timed step (dump_outputs). Prints ONE JSON line on rank 0.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

W_LINE = 2000
B_PER_GPU = 64                        # BASELINE configs[1]: the 1-GPU workload
SEED = 2
B_GLOBAL_C4 = 4096                    # BASELINE configs[3]: the global batch sharded over N > 1 GPUs (strong scaling)
SEED_C4 = 4
FLOP_PER_COL_DOM = 75.497472e6        # one 3x3 512->512 @ H=16 layer, per pixel column
FLOP_PER_COL_ALL = 1358.838912e6      # whole forward per pixel column at C=7358
PEAK_F16_TFLOPS = 2500.0              # MI355X dense fp16/bf16 MFMA (MI355X_MICROARCH.md)
# the ten 3x3 512->512 @H=16 launches of a forward (conv2 is named "+se" when the SE apply is fused)
DOMINANT = tuple(n + sfx for n in ("block3.0.conv2", "block3.1.conv2", "block3.2.conv2", "block3.3.conv2",
                                   "block3.4.conv2") for sfx in ("", "+se")) + \
    ("block3.1.conv1", "block3.2.conv1", "block3.3.conv1", "block3.4.conv1", "conv3+pool")
DTYPE_NAME = {"f16": "f16 (f32 accumulate)", "f16x3": "f16x3 (hi+lo fp16 pairs, f32 accumulate)",
              "auto": "f16 with a top-2 margin guard, uncertain lines again in f16x3"}


# ---------------------------------------------------------------------------------------------------------------------
# host-side helpers (no GPU, no torch)
# ---------------------------------------------------------------------------------------------------------------------
def cpu_info():
    """CPU model, logical CPUs this process may run on, physical cores among them, cgroup CPU quota (None = unlimited)."""
    model, phys = "unknown", set()
    allowed = os.sched_getaffinity(0)
    try:
        cur = {}
        with open("/proc/cpuinfo") as f:
            for line in f.read().split("\n") + [""]:
                if ":" in line:
                    k, v = line.split(":", 1)
                    cur[k.strip().lower()] = v.strip()
                elif cur:
                    if cur.get("model name"):
                        model = cur["model name"]
                    if int(cur.get("processor", -1)) in allowed:
                        phys.add((cur.get("physical id", "0"), cur.get("core id", cur.get("processor"))))
                    cur = {}
    except (OSError, ValueError):
        pass
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()
            if q != "max":
                quota = float(q) / float(per)
    except (OSError, ValueError):
        pass
    return {"cpu": model, "logical_cpus": len(allowed), "physical_cores": len(phys) or len(allowed), "cgroup_cpu_quota": quota}


def host_workers():
    info = cpu_info()
    n = info["physical_cores"]
    if info["cgroup_cpu_quota"]:
        n = min(n, max(1, int(info["cgroup_cpu_quota"])))
    return max(1, min(16, n))


def _gen_lines_job(job):
    kind, n, width, seed, offset = job
    import hctr_amd
    synth = hctr_amd.synth
    if kind == "trained":
        return synth.make_font_lines(n, width, seed, line_offset=offset)
    return synth.make_line_images(n, width, seed, line_offset=offset)


def gen_lines(pool, kind, n, width, seed, offset=0):
    """uint8 [n,128,width] synthetic lines; every line is a pure function of (seed, line index), so the lines are drawn
    in chunks by the worker pool (identical to one serial call)."""
    if n == 0:
        return np.zeros((0, 128, width), np.uint8)
    if pool is None or n < 8:
        return _gen_lines_job((kind, n, width, seed, offset))
    per = max(2, -(-n // (4 * pool._processes)))
    jobs = [(kind, min(per, n - o), width, seed, offset + o) for o in range(0, n, per)]
    return np.concatenate(pool.map(_gen_lines_job, jobs), axis=0)


def _beam_check_job(job):
    """oracle prefix beam search (CPU restatement of utils/ctc_codec.py:183-285) on the engine's device top-k of a few lines"""
    topk, logp = job
    import hctr_amd
    from oracle import ctc_ref
    oc = ctc_ref.FastToyCodecRef(hctr_amd.synth.characters())     # (toy-bigram LM with memoised, bit-identical prefix sums)
    oc.use_beam_search, oc.use_tfm_pred, oc.skip_search = True, False, False
    oc.beam_size = oc.search_depth = 10
    oc.lm_panelty, oc.len_bonus = 0.8, 4.8
    return oc.beam_full_from_topk(topk, logp)


def edit_distance(a, b):
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def load_golden(name):
    """REAL-reference outputs for the 64 lines of config 2 (tests/golden/make_golden_c2.py)."""
    with open(os.path.join(ROOT, "tests", "golden", name + ".json")) as f:
        return json.load(f)


def text_parity(texts, meta, n, mode, kind):
    ref = meta["greedy"][:n]
    return {"lines": n, "exact_lines": int(sum(a == b for a, b in zip(texts, ref))),
            "char_edits": int(sum(edit_distance(a, b) for a, b in zip(texts, ref))),
            "ref_chars": int(sum(len(s) for s in ref)), "mode": mode,
            "source": "tests/golden/%s.json: REAL reference (fp32 CPU) greedy strings of these same lines"
                      % ("c2_lines" if kind == "random" else "c2_trained_lines")}


PARITY_NOTE = {
    "random": "random-head checkpoint: 69 of the 128000 reference columns have a top-2 margin below 1e-3 (scale 41.5), 8 "
              "below 1e-4 - closer than two fp32 summation orders agree; f16x3 is fp32-grade (|dlogit| ~5e-4), f16 has "
              "the 10-bit mantissa of the TF32 mode the reference enables on GPUs; auto re-runs every line with a column "
              "inside twice the f16 logit tolerance in f16x3 (all 64 here).",
    "trained": "trained-like checkpoint (synth.make_state_dict(head='trained')): same random trunk, classifier rows fitted "
               "by ridge regression on its features of glyph-font lines, so the logits are peaky like a trained CTC "
               "model's: of the reference's 128000 columns 3 have a top-2 margin below 1 % of the logit scale (random "
               "head: 22600); histogram in tests/golden/c2_trained_lines.json",
}


_T0 = time.perf_counter()


def log(msg):
    """progress line on stderr (rank 0 only): a long run must not look hung"""
    if int(os.environ.get("RANK", "0")) == 0:
        print("bench.py [%6.1f s] %s" % (time.perf_counter() - _T0, msg), file=sys.stderr, flush=True)


def maybe_spawn(args):
    """`python bench.py --gpus N` with N > 1 and no rank environment: start the N ranks as CHILD processes (one per
    GPU, torch.distributed.run) before anything here touches the GPU, relay rank 0's JSON line and exit with the
    children's code. (Never an exec of this process.)"""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print("bench.py: starting %d ranks: %s" % (args.gpus, " ".join(cmd)), file=sys.stderr, flush=True)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env)
    last = None
    for line in proc.stdout:
        if line.startswith("{"):
            last = line.strip()
        else:
            sys.stderr.write(line)
    rc = proc.wait()
    if last is not None:
        print(last, flush=True)
    if rc == 0 and last is None:
        print("bench.py: the ranks exited without a result line", file=sys.stderr)
        rc = 1
    sys.exit(rc)


# ---------------------------------------------------------------------------------------------------------------------
def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=0, help="lines per step (default: 64 at 1 GPU, 4096 globally at N > 1)")
    ap.add_argument("--width", type=int, default=W_LINE)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-lines", type=int, default=4, help="lines of the CPU baseline batch (BASELINE.md section 4: 4)")
    ap.add_argument("--layers", action="store_true", help="print the per-layer device-time table to stderr")
    ap.add_argument("--layer-file", default="", help="write the per-step launch order (layer names) to this file")
    ap.add_argument("--precision", default="f16", choices=["f16", "f16x3", "auto"],
                    help="engine precision mode of the headline timing (default f16)")
    ap.add_argument("--no-second-mode", action="store_true",
                    help="1 GPU: headline mode only (no other modes, no trained-like checkpoint, no extra configs: profiling runs)")
    ap.add_argument("--no-extra-configs", action="store_true", help="1 GPU: skip the configs[2] / configs[4] records")
    ap.add_argument("--checkpoint", default="random", choices=["random", "trained"],
                    help="synthetic checkpoint: near-tie-rich random head (default) or the trained-like head")
    ap.add_argument("--no-pipeline", action="store_true", help="c5: run front end and host search back to back")
    ap.add_argument("--chunk", type=int, default=64, help="c5: lines per pipeline chunk (the last chunks taper to 16)")
    ap.add_argument("--no-oracle-check", action="store_true",
                    help="c5: skip the oracle codec check of all beam strings (profiling runs: the worker pool must not be "
                         "used under rocprofv3, whose preloaded library has touched the GPU before the pool was forked)")
    ap.add_argument("--extra-steps", type=int, default=2, help="timed steps of the configs[2] / configs[4] records")
    ap.add_argument("--config", default="c2", choices=["c2", "c3", "c5"],
                    help="c2 (default, the driver's line): B=64 x W=2000 greedy at 1 GPU (+ the c3 / c5 records), configs[3] "
                         "(B=4096 sharded) at N > 1; c3 / c5: only that configuration (1 GPU)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: per-layer profile and roofline, text parity against the reference's "
                         "strings, and at 1 GPU the other precision modes, the pinned-host bracket, the configs[2] / "
                         "configs[4] records, the trained-like checkpoint and the CPU baseline (a plain run times the "
                         "headline mode only)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the labels the timed path returned in its last step to DIR/*.npy (float32)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if (args.layers or args.layer_file) and not args.full:
        ap.error("--layers / --layer-file need --full (the per-layer profile is taken only there)")
    if args.dump_outputs and args.config != "c2":
        ap.error("--dump-outputs covers the default configuration (--config c2) only")
    return args


def main():
    args = parse_args()
    maybe_spawn(args)
    t_start = time.perf_counter()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))

    # ---- synthetic inputs on the host, drawn by a worker pool that is created BEFORE this process touches the GPU ----
    import multiprocessing
    import hctr_amd                                            # (imports numpy code only; the library loads lazily)
    synth = hctr_amd.synth
    pool = multiprocessing.get_context("fork").Pool(host_workers()) if host_workers() > 1 else None
    C = synth.DEFAULT_VOCAB + 2
    W = args.width
    import importlib
    hdist = importlib.import_module(hctr_amd.package.__name__ + ".dist")
    if world == 1:
        n_global = args.batch or B_PER_GPU
        seed, cfg_name = SEED, "BASELINE configs[1]"
    else:
        n_global = args.batch or B_GLOBAL_C4
        seed, cfg_name = SEED_C4, "BASELINE configs[3]"
    lo, hi = hdist.shard_range(n_global, rank, world)
    B = hi - lo
    full_line = args.full and world == 1 and args.config == "c2" and not args.no_second_mode
    want_c3 = args.config == "c3" or (full_line and not args.no_extra_configs)
    want_c5 = args.config == "c5" or (full_line and not args.no_extra_configs)
    t0 = time.perf_counter()
    data = {}
    if args.config == "c2":
        data["c2"] = gen_lines(pool, args.checkpoint, B, W, seed, lo)
        if full_line and args.checkpoint == "random" and n_global == B_PER_GPU and W == W_LINE:
            data["c2_trained"] = gen_lines(pool, "trained", n_global, W, seed, 0)
    if want_c3:
        data["c3"] = [(w, gen_lines(pool, "random", 128, w, 3, bi * 128)) for bi, w in enumerate((800, 1600, 2400, 3200))]
    if want_c5:
        data["c5"] = gen_lines(pool, "random", 256, W_LINE, 5, 0)
    sd = make_checkpoint(synth, C, args.checkpoint)
    setup = {"host_data_and_checkpoint_s": round(time.perf_counter() - t0, 2)}
    log("synthetic lines + checkpoint on the host: %.1f s (%d workers)" % (setup["host_data_and_checkpoint_s"], host_workers()))

    # ---- GPU / process group ----
    import torch
    dist = None
    # Test hook (rehearsing the N > 1 flow on a 1-GPU box): HCTR_BENCH_BACKEND=gloo shares the visible
    # GPUs round-robin between ranks and gathers over gloo. The driver's runs use RCCL ("nccl").
    backend = os.environ.get("HCTR_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local = local % max(1, torch.cuda.device_count())
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend=backend)
        if dist.get_world_size() != args.gpus:
            raise SystemExit("bench.py: the %s backend reports world size %d, expected %d" % (backend, dist.get_world_size(), args.gpus))
        if rank == 0:
            print("bench.py: %s process group up, world size %d" % (backend, dist.get_world_size()), file=sys.stderr, flush=True)
    dev = torch.device("cuda", local)
    lib_override = os.environ.get("HCTR_LIB_PATH", "")
    if lib_override and rank == 0:
        print("bench.py: WARNING: HCTR_LIB_PATH=%s - timing an alternative build of the library, NOT the in-tree "
              "libhctr_hip.so" % lib_override, file=sys.stderr, flush=True)

    t0 = time.perf_counter()
    # one context with BOTH weight sets serves f16, f16x3 and auto when the full line is wanted
    build_prec = "auto" if (full_line or args.precision == "auto") else args.precision
    model = hctr_amd.hctr_model(C, precision=build_prec).cuda(local)
    model.load_state_dict(sd)
    model.set_precision(args.precision)
    model.eval()
    setup["model_build_s"] = round(time.perf_counter() - t0, 2)
    log("engine context + weights (%s) on cuda:%d: %.1f s" % (build_prec, local, setup["model_build_s"]))
    if args.config != "c2":
        res = extra_config(args, hctr_amd, model, dev, data, pool)
        print(json.dumps(res))
        return

    imgs_host = data["c2"]
    imgs = torch.from_numpy(imgs_host).to(dev)               # resident in HBM before timing
    torch.cuda.synchronize(dev)
    t_fwd, t_gather = [0.0], [0.0]

    def step(m, x):
        t0 = time.perf_counter()
        labels = m.greedy(x)                                 # synchronous at return (labels on the host)
        t1 = time.perf_counter()
        t_fwd[0] += t1 - t0
        if dist is not None:
            labels = hdist.gather_labels(labels, n_global, W, device=dev if backend == "nccl" else None)
            t_gather[0] += time.perf_counter() - t1
        return labels

    def timed(m, x, with_profile=False, steps=None, warmup=None):
        steps = args.steps if steps is None else steps
        for _ in range(args.warmup if warmup is None else warmup):
            out = step(m, x)
        prof = {}
        if with_profile:
            m.set_profiling(True)
        t_fwd[0] = t_gather[0] = 0.0
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            out = step(m, x)
            if with_profile:
                for name, ms in m.last_profile():
                    prof.setdefault(name, []).append(ms)
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        if with_profile:
            m.set_profiling(False)
        if dist is not None:
            t = torch.tensor([dt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return out, dt, prof

    setup["before_first_step_s"] = round(time.perf_counter() - t_start, 2)
    out, dt, prof = timed(model, imgs, args.full)
    fwd_ms, gather_ms = t_fwd[0] / args.steps * 1e3, t_gather[0] / args.steps * 1e3
    per_rank = None
    if dist is not None:                                      # every rank's own forward time, for the record
        t = torch.tensor([fwd_ms, gather_ms, setup["before_first_step_s"]], dtype=torch.float64,
                         device=dev if backend == "nccl" else "cpu")
        allt = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(allt, t)
        per_rank = [[round(float(v), 3) for v in x.cpu().tolist()] for x in allt]

    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        if pool is not None:
            pool.terminate()
        return

    lines_per_s = n_global * args.steps / dt
    log("headline (%s): %.1f lines/s, %.2f ms/step" % (args.precision, lines_per_s, dt / args.steps * 1e3))
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, out, W)
    result = {
        "metric": "text-lines/sec (1x128x2000 synth) greedy decode",
        "value": round(lines_per_s, 3), "unit": "lines/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True,
        "scaling": "weak" if world == 1 else "strong", "vs_baseline": None,
        "dtype": DTYPE_NAME[args.precision], "data": "synthetic",
        "config": {"workload": "%s: %d x 1x128x%d uint8 lines%s, %s hctr checkpoint (C=%d), forward + greedy CTC "
                               "decode, labels to host%s" %
                               (cfg_name, n_global, W, "" if world == 1 else " in contiguous shards of %d" % B,
                                "random-init" if args.checkpoint == "random" else "trained-like synthetic", C,
                                "" if world == 1 else ", one gather to rank 0"),
                   "global_lines": n_global, "lines_per_gpu": B, "width": W, "classes": C,
                   "checkpoint": args.checkpoint, "parallelism": "batch-shard x%d" % world},
        "setup_s": setup,
        "lib": lib_override or "in-tree libhctr_hip.so (source hash checked)",
    }
    if args.full:
        result.update(profile_records(args, model, prof, B, W, world))
    if world > 1:
        result["multi_gpu"] = {"world_size_reported_by_backend": dist.get_world_size(), "backend": backend,
                               "per_rank": {"columns": ["greedy ms (forward+decode+D2H)", "gather ms", "set-up s before the first step"],
                                            "rows": per_rank},
                               "gather_bytes_per_rank": int(-(-n_global // world) * (1 + W) * 4),
                               "gather_cap": "W labels per line: random-init weights emit a label on every second column (978 of 2000 on average), so no smaller constant is safe; 4.1 MB per rank at 512 lines"}

    if world == 1 and args.full:
        codec = hctr_amd.ctc_codec(synth.characters())
        std = n_global == B_PER_GPU and W == W_LINE
        meta = load_golden("c2_lines" if args.checkpoint == "random" else "c2_trained_lines") if std else None
        if meta is not None:
            result["parity_vs_cpu"] = text_parity(codec.labels_to_text(out), meta, n_global, args.precision, args.checkpoint)
            result["parity_note"] = PARITY_NOTE[args.checkpoint]
        if args.precision == "auto":
            result["flagged_lines"] = model.last_guard()["flagged"]
        if full_line:
            # the other precision modes: same context (both weight sets resident), same loop, K steps after W warm-ups
            for other in [m for m in ("f16", "f16x3", "auto") if m != args.precision]:
                model.set_precision(other)
                out2, dt2, _ = timed(model, imgs)
                result["value_" + other] = round(n_global * args.steps / dt2, 3)
                log("%s: %.1f lines/s" % (other, result["value_" + other]))
                result["ms_per_step_" + other] = round(dt2 / args.steps * 1e3, 3)
                result["dtype_" + other] = DTYPE_NAME[other]
                if other == "auto":
                    gd = model.last_guard()
                    result["flagged_lines_auto"] = {"flagged": gd["flagged"], "lines": gd["lines"],
                                                    "criterion": "min column margin <= 2 * (0.01 * max|logit of the line| + 0.05)"}
                if meta is not None:
                    result["parity_vs_cpu_" + other] = text_parity(codec.labels_to_text(out2), meta, n_global, other, args.checkpoint)
            model.set_precision(args.precision)
            # the reference's own bracket (test.py:189-195: .cuda() + forward + .cpu() + decode): the uint8 batch starts in
            # PINNED HOST memory, the labels end on the host; H2D of 16.4 MB per batch rides inside the timed region
            pinned = torch.from_numpy(imgs_host).pin_memory()
            _, dth, _ = timed(model, pinned)
            result["value_incl_h2d"] = round(n_global * args.steps / dth, 3)
            log("pinned host -> labels: %.1f lines/s" % result["value_incl_h2d"])
            result["ms_per_step_incl_h2d"] = round(dth / args.steps * 1e3, 3)
            del pinned
        if full_line and not args.no_extra_configs:
            model.set_precision("f16")
            result["configs"] = {"c3": run_c3(model, dev, data["c3"], args.extra_steps, 1)}
            log("configs[2]: %.1f lines/s" % result["configs"]["c3"]["value"])
            result["configs"]["c5"] = run_c5(args, hctr_amd, model, dev, data["c5"], args.extra_steps, 1, pool)
            log("configs[4]: %.1f lines/s pipelined" % result["configs"]["c5"]["value"])
        if full_line and "c2_trained" in data:
            # the same workload and kernels with the trained-like checkpoint (peaky logits, like a trained CTC model's):
            # f16 and auto timed by the same loop, their text compared with the REAL reference's for all 64 lines
            del model
            sd_t = make_checkpoint(synth, C, "trained")
            m3 = hctr_amd.hctr_model(C, precision="auto").cuda(local)
            m3.load_state_dict(sd_t)
            imgs_t = torch.from_numpy(data["c2_trained"]).to(dev)
            torch.cuda.synchronize(dev)
            meta_t = load_golden("c2_trained_lines")
            tc = {"unit": "lines/s", "steps": args.steps, "warmup": args.warmup, "note": PARITY_NOTE["trained"]}
            for mode in ("f16", "auto"):
                m3.set_precision(mode)
                out3, dt3, _ = timed(m3, imgs_t)
                sfx = "" if mode == "f16" else "_auto"
                tc["value" + sfx] = round(n_global * args.steps / dt3, 3)
                log("trained-like checkpoint, %s: %.1f lines/s" % (mode, tc["value" + sfx]))
                tc["ms_per_step" + sfx] = round(dt3 / args.steps * 1e3, 3)
                tc["dtype" + sfx] = DTYPE_NAME[mode]
                tc["parity_vs_cpu" + sfx] = text_parity(codec.labels_to_text(out3), meta_t, n_global, mode, "trained")
                if mode == "auto":
                    gd = m3.last_guard()
                    tc["flagged_lines_auto"] = {"flagged": gd["flagged"], "lines": gd["lines"],
                                                "min_margin_of_flagged": [round(float(v), 3) for v in gd["min_margin"][gd["flags"] > 0]]}
            result["trained_checkpoint"] = tc
            del m3
            # the figures that meet north_star's "decoded text exact", stated in one place
            pa = result.get("parity_vs_cpu_auto", {})
            result["text_exact_vs_reference"] = {
                "trained_like_checkpoint": {
                    "f16": "%s lines/s, %d/%d lines exact" % (tc["value"], tc["parity_vs_cpu"]["exact_lines"], n_global),
                    "auto": "%s lines/s, %d/%d lines exact, %d lines re-run in f16x3" % (
                        tc["value_auto"], tc["parity_vs_cpu_auto"]["exact_lines"], n_global, tc["flagged_lines_auto"]["flagged"])},
                "random_head_checkpoint": {
                    "f16": "%d/%d lines exact" % (result.get("parity_vs_cpu", {}).get("exact_lines", -1), n_global),
                    "f16x3": "%s lines/s, %d/%d" % (result.get("value_f16x3"), result.get("parity_vs_cpu_f16x3", {}).get("exact_lines", -1), n_global),
                    "auto": "%s lines/s, %d/%d (= f16x3's text; near-tie-rich logits, see parity_note)" % (
                        result.get("value_auto"), pa.get("exact_lines", -1), n_global)}}
    if args.full and not args.no_cpu_baseline and world == 1:     # reported baseline: rank 0 of the 1-GPU run only
        # the CPU restatement (bit-equal to the reference here) on B=4 lines of the same
        # workload, 1 warm-up + 3 timed passes, on the physical host cores this process may use
        from oracle import ctc_ref, hctr_ref
        info = cpu_info()
        ncores = info["physical_cores"]
        if info["cgroup_cpu_quota"]:
            ncores = max(1, min(ncores, int(round(info["cgroup_cpu_quota"]))))
        torch.set_num_threads(ncores)
        nl = max(1, min(args.cpu_lines, B))
        x = synth.normalize_pad(imgs_host[:nl])
        ocodec = ctc_ref.CtcCodecRef(synth.characters())
        times = []
        for it in range(4):
            t0 = time.perf_counter()
            ref_txt = ocodec.decode(hctr_ref.forward(sd, x).numpy())
            if it:
                times.append(time.perf_counter() - t0)
        cdt = float(np.median(times))
        log("CPU baseline: %.3f lines/s on %d threads" % (nl / cdt, ncores))
        gold = load_golden("c2_lines" if args.checkpoint == "random" else "c2_trained_lines") \
            if (n_global == B_PER_GPU and W == W_LINE) else None
        result["cpu_baseline"] = {"value": round(nl / cdt, 4), "unit": "lines/s", "cores": ncores,
                                  "threads": torch.get_num_threads(), "cpu": info["cpu"],
                                  "logical_cpus_visible": info["logical_cpus"], "cgroup_cpu_quota": info["cgroup_cpu_quota"],
                                  "kind": "port",
                                  "sample": "%d line(s) of 1x128x%d, oracle forward + greedy (torch CPU fp32), 1 warm-up + "
                                            "3 timed passes, median" % (nl, W),
                                  "oracle_equals_golden_reference_text": (ref_txt == gold["greedy"][:nl]) if gold else None}
    result["bench_wall_s"] = round(time.perf_counter() - t_start, 1)
    print(json.dumps(result))
    if dist is not None:
        dist.destroy_process_group()
    if pool is not None:
        pool.terminate()


def make_checkpoint(synth, C, kind):
    if kind == "trained":
        return synth.make_state_dict(C, seed=0, head="trained")
    return synth.make_state_dict(C, seed=0)


def profile_records(args, model, prof, B, W, world):
    """--full: the roofline and whole-forward records from the per-layer profile of the headline's timed steps."""
    # the dominant kernel's launch covers one internal pass of the engine (hctr_lines_per_pass: HCTR_MAX_COLS pixel
    # columns, a third of that in f16x3); last_profile adds the passes' entries of one name up
    x3 = args.precision == "f16x3"
    pass_lines = model.lines_per_pass(B, W, x3)
    n_pass = -(-B // pass_lines)
    dom_ms = [np.mean(prof[n]) / n_pass for n in DOMINANT if n in prof]
    dom_avg_ms = float(np.mean(dom_ms)) if dom_ms else float("nan")
    flop_per_launch = FLOP_PER_COL_DOM * (B * W / n_pass)
    dom_tflops = flop_per_launch / (dom_avg_ms * 1e-3) / 1e12
    kernel_ms = float(sum(np.mean(v) for v in prof.values()))
    # HBM-side traffic and matrix-pipe counters of the dominant kernel per launch: rocprofv3 PMC passes of this same
    # command (tools/profile_rocprof.sh: FETCH_SIZE, WRITE_SIZE and the SQ set in separate runs, KiB units, FETCH_SIZE x2
    # on gfx950 as MI355X_MICROARCH.md prescribes), summarised into profiles/per_layer_latest.json - NOT measured in
    # this run (a PMC pass cannot share a process with the timed region).
    traffic = traffic_src = busy = clock = None
    pj = os.path.join(ROOT, "profiles", "per_layer_latest.json")
    if os.path.isfile(pj) and world == 1 and B == B_PER_GPU and W == W_LINE and args.precision == "f16":
        with open(pj) as f:
            rows = [r for r in json.load(f) if r["layer"] in DOMINANT and r.get("fetch_gb_x2") is not None]
        if rows:
            traffic = float(np.mean([(r["fetch_gb_x2"] + r["write_gb"]) * 1e9 for r in rows]))
            traffic_src = "profiles/per_layer_latest.json (rocprofv3 --pmc, separate passes of this command; not this run)"
            b_ = [r["mfma_busy_pct"] for r in rows if r.get("mfma_busy_pct") is not None]
            c_ = [r["clock_ghz"] for r in rows if r.get("clock_ghz") is not None]
            busy = round(float(np.mean(b_)), 1) if b_ else None
            clock = round(float(np.mean(c_)), 3) if c_ else None
    if args.layers:
        for name, v in prof.items():
            print("%-24s %9.3f ms" % (name, float(np.mean(v))), file=sys.stderr)
    if args.layer_file:
        with open(args.layer_file, "w") as f:
            f.write("\n".join(prof.keys()) + "\n")
    return {
        "roofline": {"bound": "mfma", "kernel": "conv3x3_halo4 3x3 512->512 @H=16 (%d launches per pass averaged)" % len(dom_ms),
                     "achieved": round(dom_tflops, 2), "peak": PEAK_F16_TFLOPS, "unit": "TFLOP/s",
                     "frac": round(dom_tflops / PEAK_F16_TFLOPS, 4), "traffic": traffic,
                     "traffic_unit": "bytes/launch (algorithmic: 2.36e9 in + 2.36e9 out + 4.7e6 weights)",
                     "traffic_source": traffic_src, "mfma_busy_pct": busy, "clock_ghz": clock,
                     "avg_launch_ms": round(dom_avg_ms, 4), "flops_per_launch": flop_per_launch,
                     "launches_per_step_and_layer": n_pass,
                     "note": "algorithmic FLOPs (2*Cin*Cout*9 per output pixel); in f16x3 the kernel issues 3x that "
                             "in MFMA work" if x3 else None},
        "whole_forward": {"kernel_ms_per_step": round(kernel_ms, 3),
                          "tflops": round(FLOP_PER_COL_ALL * B * W / (kernel_ms * 1e-3) / 1e12, 2)},
    }


DUMP_BUDGET_BYTES = 60 << 20          # the .npy files of --dump-outputs stay below 64 MB in all


def dump_outputs(dirname, labels, width):
    """--dump-outputs: the label arrays the timed path returned in its last step (all lines, in batch order), as float32
    .npy files (exact: labels are below 2**24): labels.npy [lines, width] holds each line's labels followed by -1
    padding, lengths.npy [lines] their counts, line_index.npy [lines] the batch position of each row. A batch beyond
    the size budget is cut to a fixed sample of lines (seed 0, kept in batch order)."""
    n = len(labels)
    rows = np.arange(n)
    per_line = (width + 2) * 4
    if n * per_line > DUMP_BUDGET_BYTES:
        rows = np.sort(np.random.default_rng(0).choice(n, DUMP_BUDGET_BYTES // per_line, replace=False))
    padded = np.full((len(rows), width), -1, np.float32)
    for i, r in enumerate(rows):
        padded[i, :len(labels[r])] = labels[r]
    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, "labels.npy"), padded)
    np.save(os.path.join(dirname, "lengths.npy"), np.array([len(labels[r]) for r in rows], np.float32))
    np.save(os.path.join(dirname, "line_index.npy"), rows.astype(np.float32))
    log("outputs of the last timed step: %d of %d lines -> %s" % (len(rows), n, dirname))


# ---------------------------------------------------------------------------------------------------------------------
# BASELINE configs[2] and configs[4] on one GPU
# ---------------------------------------------------------------------------------------------------------------------
def run_c3(model, dev, buckets_host, steps, warmup):
    """configs[2]: 512 lines of mixed widths {800,1600,2400,3200}, one equal-width bucket of 128 lines per width."""
    import torch
    buckets = [(w, torch.from_numpy(h).to(dev)) for w, h in buckets_host]
    torch.cuda.synchronize(dev)

    def step():
        return [model.greedy(t) for _, t in buckets]
    for _ in range(warmup):
        step()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        out = step()
    torch.cuda.synchronize(dev)
    dt = time.perf_counter() - t0
    n_lines, cols = 512, sum(128 * w for w, _ in buckets)
    return {"workload": "BASELINE configs[2]: B=512 mixed widths {800,1600,2400,3200}, 4 equal-width buckets of 128, greedy, f16",
            "value": round(n_lines * steps / dt, 3), "unit": "lines/s", "steps": steps, "warmup": warmup,
            "ms_per_step": round(dt / steps * 1e3, 3), "columns_per_step": cols, "columns_per_s": round(cols * steps / dt, 1),
            "decoded_lines": int(sum(len(o) for o in out))}


def run_c5(args, hctr_amd, model, dev, host, steps, warmup, pool):
    """configs[4]: 256 lines x W=2000, cbs_full beam 10 / depth 10 with the toy-bigram LM: the device front end
    (log-softmax + top-k inside the head GEMM's epilogues) pipelined with the C++ host prefix search, plus the two
    stages back to back, plus the oracle codec on the engine's own top-k for ALL lines (outside the timed region)."""
    import importlib
    import torch
    synth = hctr_amd.synth
    pipe = importlib.import_module(hctr_amd.package.__name__ + ".pipeline")
    codec = hctr_amd.ctc_codec(synth.characters()).attach(model)
    dev_imgs = torch.from_numpy(host).to(dev)
    torch.cuda.synchronize(dev)
    codec.use_beam_search, codec.use_tfm_pred, codec.skip_search = True, False, False
    codec.beam_size = codec.search_depth = 10
    codec.lm_panelty, codec.len_bonus = 0.8, 4.8              # test.py:74-79 defaults
    codec.ngram = hctr_amd.ToyBigramLM()
    n_lines = host.shape[0]

    def timed(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            out = fn()
        torch.cuda.synchronize(dev)
        return out, (time.perf_counter() - t0) / steps
    res = {"workload": "BASELINE configs[4]: B=256 x 1x128x2000, cbs_full beam 10 / depth 10, toy-bigram LM, device "
                       "log-softmax+top-k, C++ host prefix search on %d threads, f16" % min(64, len(os.sched_getaffinity(0)), 4 * hctr_amd.package._lib.usable_cpus()),
           "unit": "lines/s", "steps": steps, "warmup": warmup}
    if not args.no_pipeline:
        out, dt = timed(lambda: pipe.recognize_beam(model, codec, dev_imgs, chunk=args.chunk))
        res["value"] = round(n_lines / dt, 3)
        res["ms_per_step"] = round(dt * 1e3, 3)
        res["pipeline"] = "front end of chunk i+1 (GPU) overlaps the host search of chunk i; chunks of %s lines" % \
            [hi - lo for lo, hi in pipe.chunk_schedule(n_lines, args.chunk)]
    # the two stages back to back, timed separately
    t_front, t_search, fe_keep = [0.0], [0.0], [None]

    def sequential():
        t0 = time.perf_counter()
        fe = model.beam_frontend(dev_imgs, k=10)
        t1 = time.perf_counter()
        txt = codec.decode_frontend(fe)
        t_front[0] += t1 - t0
        t_search[0] += time.perf_counter() - t1
        fe_keep[0] = fe
        return txt
    for _ in range(warmup):
        sequential()
    t_front[0] = t_search[0] = 0.0
    for _ in range(steps):
        out_seq = sequential()
    res["sequential"] = {"value": round(n_lines * steps / (t_front[0] + t_search[0]), 3),
                         "frontend_ms_per_step": round(t_front[0] / steps * 1e3, 2),
                         "host_search_ms_per_step": round(t_search[0] / steps * 1e3, 2)}
    if args.no_pipeline:
        out = out_seq
        res["value"] = res["sequential"]["value"]
        res["ms_per_step"] = round((t_front[0] + t_search[0]) / steps * 1e3, 3)
    res["pipelined_equals_sequential"] = bool(out == out_seq)
    # parity of ALL lines: the oracle codec (CPU restatement of the reference's prefix beam search) on the ENGINE's device
    # top-k / log-probs must give the same strings (worker pool, outside the timed region)
    if args.no_oracle_check:
        return res
    fe = fe_keep[0]
    log("configs[4]: checking all %d beam strings with the oracle codec on the engine's top-k ..." % n_lines)
    t0 = time.perf_counter()
    per = 4
    jobs = [(fe["topk_idx"][:, o:o + per], fe["topk_logp"][:, o:o + per]) for o in range(0, n_lines, per)]
    want = sum((pool.map(_beam_check_job, jobs) if pool is not None else [_beam_check_job(j) for j in jobs]), [])
    cdt = time.perf_counter() - t0
    res["beam_strings_equal_oracle_on_engine_topk"] = {"lines_checked": n_lines,
                                                       "equal": int(sum(a == b for a, b in zip(want, out_seq)))}
    res["cpu_codec_lines_per_s"] = round(n_lines / cdt, 3)
    res["cpu_codec_workers"] = pool._processes if pool is not None else 1
    return res


def extra_config(args, hctr_amd, model, dev, data, pool):
    """--config c3 / c5: only that configuration, as its own JSON line (builder runs, profiling)."""
    if args.config == "c3":
        rec = run_c3(model, dev, data["c3"], args.steps, args.warmup)
    else:
        rec = run_c5(args, hctr_amd, model, dev, data["c5"], args.steps, args.warmup, pool)
    res = {"metric": "text-lines/sec", "value": rec["value"], "unit": "lines/s", "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": rec["ms_per_step"], "higher_is_better": True,
           "dtype": DTYPE_NAME[args.precision], "data": "synthetic", "config": {"workload": rec["workload"]}}
    res.update({k: v for k, v in rec.items() if k not in res and k != "workload"})
    if pool is not None:
        pool.terminate()
    return res


if __name__ == "__main__":
    main()
