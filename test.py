#!/usr/bin/env python3
"""Evaluation / inference CLI for the MI355X hctr engine, flag-compatible with the reference's
``test.py`` (flags ``test.py:24-106``; flow ``test.py:109-201``; ``-bm`` CER loop ``test.py:230-306``;
``-gs`` grid search ``test.py:347-382``).

Differences from the reference, by design:
  * the model and codec are the engine-backed drop-ins (``hctr_amd``); ``--gpu`` defaults to 0 because
    there is no CPU execution path;
  * batches go through the fused device path (uint8 images + widths -> labels); the 29 kB-per-column
    logits never reach the host;
  * images are decoded with PIL (cv2 is not a dependency); gray conversion and the keep-ratio INTER_AREA
    resize to height 128 (test.py:204-216, utils/dataset.py:47-60) run on the device and the batch stays in
    HBM - pixel parity with cv2 is unpinned;
  * ``-bm`` applies AlignCollate's width cap of 1600 columns with its proportional label cut
    (utils/dataset.py:111-148, built with the default max_width at test.py:235);
  * ``-jw N`` decodes the next batches' image files on N host threads while the GPU works on the current one
    (the reference's DataLoader workers, test.py:240-245); ``-jw 0`` decodes inline;
  * ``-f synthetic[:seed]`` loads the package's deterministic synthetic checkpoint (no checkpoint files
    are bundled with the reference), and then the vocabulary defaults to the synthetic one;
  * ``-kp zero|toy`` selects a built-in language model for beam search when kenlm is not installed;
  * ``-gs --device-sweep`` answers the grid search with one pass over the dataset: one model, one forward per batch,
    every (lm_panelty, len_bonus) pair searched and scored on the device (``hctr_model.lm_sweep``), then the
    reference's lines. Without the flag ``-gs`` runs the reference's loop of complete evaluation runs.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

IMG_EXT = (".jpg", ".jpeg", ".png", ".bmp")
ALIGN_MAX_WIDTH = 1600            # AlignCollate(max_width=1600), utils/dataset.py:112, as built at test.py:235


def build_argparser():
    p = argparse.ArgumentParser(description="hctr inference on MI355X (reference test.py flags)")
    a = p.add_argument_group("Options")
    a.add_argument("-m", "--model-type", dest="model_type", type=str, required=True, choices=["hctr"])
    a.add_argument("-f", "--model-file", dest="model_file", type=str, required=True,
                   help="checkpoint (.pth.tar with 'state_dict') or 'synthetic[:seed]'")
    a.add_argument("-i", "--input", dest="input", type=str, required=True, help="image file or folder")
    a.add_argument("-b", "--batch-size", dest="batch_size", type=int, metavar="N", default=1)
    a.add_argument("--gpu", type=int, default=0)
    a.add_argument("-bm", "--benchmark-mode", dest="benchmark_mode", action="store_true")
    a.add_argument("-dm", "--decode-method", dest="decode_method", type=str, default="beam-search",
                   choices=["greedy-search", "beam-search", "lexicon", "pattern", "words"])
    a.add_argument("--lexicon", dest="lexicon", type=str, default="",
                   help="-dm lexicon / -dm words: a text file with one admissible text (one word) per line")
    a.add_argument("--word-bonus", dest="word_bonus", type=float, default=0.0,
                   help="-dm words: added to the score per word (negative: a penalty)")
    a.add_argument("--pattern", dest="pattern", type=str, default="",
                   help="-dm pattern: a regular expression the whole line must match, e.g. '\\d{18}'")
    a.add_argument("--char-bonus", dest="char_bonus", type=float, default=0.0,
                   help="-dm pattern: a weight per character of the reading (the len_bonus of the searches, in an exact "
                        "search); 0.0 builds the unweighted pattern")
    a.add_argument("-ss", "--skip-search", dest="skip_search", action="store_true")
    a.add_argument("-kp", "--kenlm-path", dest="kenlm_path", type=str, default="")
    a.add_argument("-utp", "--use-tfm-pred", dest="use_tfm_pred", action="store_true")
    a.add_argument("-tp", "--transformer-path", dest="tfm_path", type=str, default="")
    a.add_argument("-uts", "--use-tfm-score", dest="use_tfm_score", action="store_true")
    a.add_argument("-uov", "--use-openvino", dest="use_openvino", action="store_true")
    a.add_argument("-bs", "--beam-size", dest="beam_size", type=int, default=10)
    a.add_argument("-sd", "--search-depth", dest="search_depth", type=int, default=10)
    a.add_argument("-lp", "--lm-panelty", dest="lm_panelty", type=float, default=0.8)
    a.add_argument("-lb", "--len-bonus", dest="len_bonus", type=float, default=4.8)
    a.add_argument("-jw", "--workers", type=int, metavar="N", default=4)
    a.add_argument("-tv", "--test-verbose", dest="test_verbose", action="store_true")
    a.add_argument("-pf", "--print-freq", dest="print_freq", type=int, metavar="N", default=100)
    a.add_argument("-gs", "--grid-search", action="store_true")
    a.add_argument("-al", "--alpha-lower", type=float, default=0.7)
    a.add_argument("-au", "--alpha-upper", type=float, default=1.1)
    a.add_argument("-ac", "--alpha-count", type=int, default=10)
    a.add_argument("-bl", "--beta-lower", type=float, default=4.2)
    a.add_argument("-bu", "--beta-upper", type=float, default=6.6)
    a.add_argument("-bc", "--beta-count", type=int, default=25)
    # engine option (not a reference flag): the grid search in one pass over the dataset, all pairs on the device
    a.add_argument("--device-sweep", dest="device_sweep", action="store_true")
    # engine option (not a reference flag): f16 (default), f16x3, or auto = f16 with uncertain lines re-run in f16x3
    a.add_argument("--precision", type=str, default=os.environ.get("HCTR_PRECISION", "f16"), choices=["f16", "f16x3", "auto"])
    return p


def find_characters(input_path, synthetic):
    """chars_list.txt discovery chain of test.py:315-332; synthetic vocabulary as the last resort."""
    cands = []
    if input_path:
        cands.append(os.path.join(os.path.dirname(input_path.rstrip("/")), "chars_list.txt"))
    cands += ["./data/handwritten_ctr_data/chars_list.txt", "./data/hwdb2.0/chars_list.txt",
              "./data/demo_data/chars_list.txt"]
    for c in cands:
        if os.path.isfile(c):
            with open(c, "r") as f:
                return "".join(line.strip("\n") for line in f.readlines())
    if synthetic:
        import hctr_amd
        return hctr_amd.synth.characters()
    raise FileNotFoundError("chars_list.txt not found (looked in: %s)" % ", ".join(cands))


def list_inputs(path):
    import hctr_amd
    return hctr_amd.preprocess.list_inputs(path)


def prefetched(batches, workers):
    """Yield (batch, decoded images) with the NEXT batches' files already being decoded on ``workers`` host threads
    (the reference's DataLoader(num_workers=args.workers), test.py:240-245; PIL releases the GIL while decoding),
    so that JPEG/PNG decode overlaps the GPU work of the current batch."""
    import hctr_amd
    from concurrent.futures import ThreadPoolExecutor
    load = hctr_amd.preprocess.load_image
    if workers <= 0:
        for b in batches:
            yield b, [load(p) for p in b]
        return
    with ThreadPoolExecutor(max_workers=workers) as pool:
        depth = 2                                            # batches in flight beyond the current one
        queue = []
        it = iter(batches)
        for b in it:
            queue.append((b, [pool.submit(load, p) for p in b]))
            if len(queue) > depth:
                bb, futs = queue.pop(0)
                yield bb, [f.result() for f in futs]
        for bb, futs in queue:
            yield bb, [f.result() for f in futs]


def edit_distance(a, b):
    if len(a) < len(b):
        a, b = b, a
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def check_device_sweep(args):
    """--device-sweep is the grid search of the n-gram-scored full search only: -gs -bm -dm beam-search -kp <file.arpa>,
    without -ss and without the transformer options. Raises ValueError naming the option in the way."""
    def no(why):
        raise ValueError("--device-sweep " + why)
    if not args.grid_search:
        no("needs -gs (--grid-search): it is the grid search's device path")
    if not args.benchmark_mode:
        no("needs -bm (--benchmark-mode): the grid search scores against test_img_id_gt.txt")
    if args.decode_method != "beam-search":
        no("needs -dm beam-search, got -dm %s" % args.decode_method)
    if args.skip_search:
        no("does not take -ss (--skip-search): the skip search is not swept on the device")
    for on, flag in ((args.use_tfm_pred, "-utp (--use-tfm-pred)"), (args.use_tfm_score, "-uts (--use-tfm-score)"),
                     (bool(args.tfm_path), "-tp (--transformer-path)"), (args.use_openvino, "-uov (--use-openvino)")):
        if on:
            no("does not take %s: transformer language models are not swept on the device" % flag)
    if not args.kenlm_path or args.kenlm_path in ("zero", "toy"):
        no("needs -kp <file.arpa>: an n-gram model, got -kp %r" % args.kenlm_path)
    if not os.path.isfile(args.kenlm_path):
        no("needs -kp <file.arpa>: no file at %s" % args.kenlm_path)


def build(args):
    import hctr_amd
    synthetic = args.model_file.startswith("synthetic")
    if not synthetic and not os.path.isfile(args.model_file):
        raise FileNotFoundError("No model file found at: {}".format(args.model_file))
    if not (os.path.isdir(args.input) or os.path.isfile(args.input)):
        raise FileNotFoundError("Input is not found, expected file or folder.")
    characters = find_characters(args.input, synthetic)
    num_classes = 1 + len(characters) + 1                      # test.py:334
    print("Character vocabulary: {}, Model output classes: {}".format(len(characters), num_classes))
    model = hctr_amd.hctr_model(num_classes=num_classes, precision=args.precision)
    codec = hctr_amd.ctc_codec(characters)
    print("Use GPU: {} for testing".format(args.gpu))
    model = model.cuda(args.gpu)
    print("=> loading model file: {}".format(args.model_file))
    if synthetic:
        seed = int(args.model_file.split(":")[1]) if ":" in args.model_file else 0
        sd = hctr_amd.synth.make_state_dict(num_classes, seed=seed)
    else:
        import torch
        ckpt = torch.load(args.model_file, map_location="cpu", weights_only=True)
        sd = ckpt["state_dict"] if "state_dict" in ckpt else ckpt
    model.load_state_dict(sd)
    model.eval()
    codec.attach(model)
    if args.decode_method == "beam-search":
        codec.set_beam_search(args.skip_search, ngram_path=args.kenlm_path or "zero", tfm_path=args.tfm_path,
                              lm_panelty=args.lm_panelty, len_bonus=args.len_bonus, beam_size=args.beam_size,
                              search_depth=args.search_depth, use_tfm_score=args.use_tfm_score,
                              use_tfm_pred=args.use_tfm_pred, use_openvino=args.use_openvino)
    return model, codec


def load_lexicon(path, codec):
    """-dm lexicon / -dm words --lexicon FILE: the closed list of admissible texts, one per line (empty lines are
    skipped)"""
    import hctr_amd
    if not path or not os.path.isfile(path):
        raise FileNotFoundError("-dm lexicon needs --lexicon FILE with one entry per line")
    with open(path, "r", encoding="utf-8") as f:
        entries = [line.rstrip("\r\n") for line in f]
    return hctr_amd.Lexicon([e for e in entries if e], codec=codec)


def load_pattern(expr, codec, char_bonus=0.0):
    """-dm pattern --pattern EXPR [--char-bonus X]: the compiled pattern (hctr_amd.Pattern.compile; the whole line must
    match), with X on every arc where X is not 0"""
    import hctr_amd
    if not expr:
        raise ValueError("-dm pattern needs --pattern EXPR")
    if char_bonus == 0.0:
        return hctr_amd.Pattern.compile(expr, codec)
    return hctr_amd.Pattern.compile(expr, codec, label_weights=char_bonus)


def recognise(model, codec, imgs, widths, lexicon=None, pattern=None, word_bonus=None):
    if word_bonus is not None:          # per image: the words of the best segmentation into entries, separated by /
        res = model.words(imgs, lexicon, word_bonus, widths=widths)
        return ["/".join(w[1] for w in line) for line in res.lines(lexicon)]
    if pattern is not None:             # per image: the best matching text, p(the line matches), p(that text | it matches)
        res = model.pattern(imgs, pattern, widths=widths)
        return [(t, float(np.exp(np.float64(lp))), float(p)) for t, lp, p in zip(res.texts(codec), res.logp, res.posterior())]
    if lexicon is not None:                                     # the best entry of the list per image
        res = model.lexicon(imgs, lexicon, n=1, widths=widths)
        return [t if t is not None else "" for t in res.best()]
    if codec.use_beam_search and not codec.use_tfm_pred:
        fe = model.beam_frontend(imgs, k=min(codec.search_depth, model.noutput), widths=widths,
                                 want_candidates=codec.skip_search)
        return codec.decode_frontend(fe)
    if codec.use_beam_search:                                   # LM-proposed candidates need full log-probs
        return codec.decode(model(imgs, widths=widths))
    return codec.labels_to_text(model.greedy(imgs, widths=widths))


def test(args):
    model, codec = build(args)
    if args.benchmark_mode:
        return benchmark(model, codec, args)
    import hctr_amd
    pp = hctr_amd.preprocess
    lexicon = load_lexicon(args.lexicon, codec) if args.decode_method in ("lexicon", "words") else None
    word_bonus = args.word_bonus if args.decode_method == "words" else None
    pattern = load_pattern(args.pattern, codec, args.char_bonus) if args.decode_method == "pattern" else None
    paths = list_inputs(args.input)
    batches = [paths[i * args.batch_size:(i + 1) * args.batch_size] for i in range(len(paths) // args.batch_size)]
    for i, (_, arrs) in enumerate(prefetched(batches, args.workers)):
        print("batch {} is being processed...".format(i))
        imgs, widths = pp.resize_lines(model, arrs, model.img_height, "test", "rgb", None, device_out=True)
        t0 = time.time()
        result = recognise(model, codec, imgs, widths, lexicon, pattern, word_bonus)
        dt = time.time() - t0
        print("max_width: {}, throughput: {} ms/img".format(int(widths.max()), dt / args.batch_size * 1000))
        print("predicted results: {}".format(result))
    return None


def benchmark_batches(model, args):
    """The batches of ``-bm`` over ``<input>/test_img_id_gt.txt`` ('<image name>,<text>' per line, images under
    ``<input>/test/``; utils/dataset.py:31-37): yields (batch index, number of batches, [(name, truth)], device images,
    widths), the truths cut as AlignCollate cuts them."""
    if not os.path.isdir(args.input):
        raise AssertionError("Input should be a folder under benchmark mode.")
    import hctr_amd
    pp = hctr_amd.preprocess
    gt = os.path.join(args.input, "test_img_id_gt.txt")
    items = []
    with open(gt, "r", encoding="utf-8") as f:
        for line in f.readlines():
            parts = line.strip("\n").split(",", 1)
            if len(parts) != 2 or not parts[1]:
                continue
            for cand in (os.path.join(args.input, "test", parts[0]), os.path.join(args.input, parts[0])):
                hit = [cand + e for e in ("",) + IMG_EXT if os.path.isfile(cand + e)]
                if hit and os.stat(hit[0]).st_size > 0:
                    items.append((hit[0], parts[1]))
                    break
    items = items[:args.batch_size * (len(items) // args.batch_size)]      # ImageDataset.__len__
    chunks = [items[i:i + args.batch_size] for i in range(0, len(items), args.batch_size)]
    for bi, (names, arrs) in enumerate(prefetched([[n for n, _ in ch] for ch in chunks], args.workers)):
        chunk = chunks[bi]
        full = [pp.target_width(a.shape[0], a.shape[1], model.img_height, "dataset") for a in arrs]
        imgs, widths = pp.resize_lines(model, arrs, model.img_height, "dataset", "rgb", ALIGN_MAX_WIDTH, device_out=True)
        chunk = [(n, pp.truncate_label(tru, fw, int(imgs.shape[2]))) for (n, tru), fw in zip(chunk, full)]
        yield bi, len(chunks), chunk, imgs, widths


def benchmark(model, codec, args):
    """CER of ``-bm`` (test.py:230-306) over the batches of ``benchmark_batches``."""
    total = nchars = 0
    cer = 0.0
    t_all = time.time()
    for bi, nbatches, chunk, imgs, widths in benchmark_batches(model, args):
        i = bi * args.batch_size
        t0 = time.time()
        result = recognise(model, codec, imgs, widths)
        # editdistance.eval(pre, tru) of every line (test.py:275) in one call on the device, whatever decoded them
        _, ev = codec.evaluate(result, [tru for _, tru in chunk], maps=args.test_verbose)
        for j, (pre, (_, tru)) in enumerate(zip(result, chunk)):
            if args.test_verbose:
                print("TEST [{0}/{1}]\nTEST PRE {2}\nTEST TRU {3}".format(j, i // args.batch_size, pre, tru))
            nchars += len(tru)
        total += ev.total_edits
        if args.test_verbose:
            print("TEST [{0}] S {2} D {3} I {4}".format(i // args.batch_size, *ev.totals))
        if nchars == 0:
            raise ValueError("Number of label characters should not be 0.")
        cer = total * 1.0 / nchars
        if (i // args.batch_size) % args.print_freq == 0:
            print("TEST: [{0}/{1}]\tTime {2:.3f}\tErr {3:.4f}".format(i // args.batch_size, nbatches, time.time() - t0, cer))
    print("Total Test CER: {} ({:.1f}s)".format(cer, time.time() - t_all))
    return cer


def device_sweep(args):
    """``-gs --device-sweep``: the model is built once and the dataset walked once; every batch is searched under all
    alpha x beta pairs on the device and scored there (``hctr_model.lm_sweep``). Prints the reference loop's lines."""
    import hctr_amd
    check_device_sweep(args)
    alphas = np.linspace(args.alpha_lower, args.alpha_upper, args.alpha_count)
    betas = np.linspace(args.beta_lower, args.beta_upper, args.beta_count)
    args.kenlm_path, arpa = "", args.kenlm_path          # the codec's own host search is not used
    model, codec = build(args)
    lm = hctr_amd.ArpaLM(arpa)
    totals = hctr_amd.LMSweepTotals()
    empty = 0
    t_all = time.time()
    for bi, nbatches, chunk, imgs, widths in benchmark_batches(model, args):
        sweep = model.lm_sweep(imgs, [tru for _, tru in chunk], lm=lm, codec=codec, alphas=alphas, betas=betas,
                               beam=args.beam_size, depth=min(args.search_depth, model.noutput), widths=widths)
        totals.update(sweep)
        empty += int(sweep.empty.sum())
        if bi % args.print_freq == 0:
            print("SWEEP: [{0}/{1}]\tTime {2:.1f}s\tbest so far {3}".format(bi, nbatches, time.time() - t_all, totals.best()))
    if totals.nchars == 0:
        raise ValueError("Number of label characters should not be 0.")
    if empty:
        print("{} lines had an empty greedy text (the reference's search raises IndexError there); they count as empty "
              "predictions under every pair".format(empty))
    for line in totals.report():
        print(line)
    return totals


def main():
    args = build_argparser().parse_args()
    if args.device_sweep:
        device_sweep(args)
        return
    if not args.grid_search:
        test(args)
        return
    if not args.benchmark_mode:
        raise AssertionError(args.benchmark_mode)
    best, best_params = 1.0, (0, 0)
    for a in np.linspace(args.alpha_lower, args.alpha_upper, args.alpha_count):
        for b in np.linspace(args.beta_lower, args.beta_upper, args.beta_count):
            print("searching with a:{}, b:{}, min params:{}, min cer:{}".format(a, b, best_params, best))
            args.lm_panelty, args.len_bonus = a, b
            cer = test(args)
            if cer < best:
                best, best_params = cer, (a, b)
    print("min params:{}, min cer: {}".format(best_params, best))


if __name__ == "__main__":
    main()
