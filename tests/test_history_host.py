"""Host tests of tests/history_cases.py, the inputs of tests/test_gpu_history.py (no GPU): the premises that keep a byte
comparison of probe results meaningful and the dirtiers dirtier than the probes.

  * every probe's oracle holds no NaN: its figures are finite, or -inf / +inf where the contract documents them;
  * the big dirtier exceeds, and the small one stays below, every probe in every dimension a scratch layout is carved by
    (B, W, C, the longest sequence, the distinct classes, the total length, the trie nodes of a words call, and for the
    searches beam, depth and n), asserted on the numbers, so that a later edit of a case cannot silently void the GPU
    test; the big dirtier's large lexicon needs the scratch form of the words kernel and stays within the node limit;
  * the words probe's best segmentations have several words and differing counts, and the weighted pattern probes decode
    another text than the same automata without weights, by the float64 yardsticks alone: a call that ran the wrong
    tables cannot return the yardstick's result;
  * the big dirtier's non-finite rows are one NaN, one +inf and one row of nothing but -inf, one line each, inside the
    line's input length; every other line is finite;
  * the copy of the N-best logits is the one tests/test_gpu_nbest_lm.py builds its lists from;
  * the wide recognition probe's second scratch request exceeds its first, by the engine's own formulas, so that the call
    moves its kept log-sum-exps; the `vocab` probe's does not.
"""
import numpy as np
import pytest

import history_cases as hc
import masked_cases as mc


def _no_nan(x, what):
    a = np.asarray(x, np.float64)
    assert not np.isnan(a).any(), what
    return a


def test_masked_family_oracles_hold_no_nan():
    c, o = hc.vocab()
    assert c["logits"].shape == (40, 5, 12) and 0 in c["tl"].tolist() and len(set(c["il"].tolist())) > 1
    assert not np.isnan(c["logits"]).any() and not np.isposinf(c["logits"]).any() and c["mask"].any()
    nll = _no_nan(o["nll"], "loss")
    assert np.isposinf(nll[c["no_path"]]).all() and np.isfinite(np.delete(nll, c["no_path"])).all()
    for b, a in enumerate(o["align"]):
        _no_nan(a["score"], "alignment score")
        _no_nan(a["logps"], "span_logp")
        assert np.isfinite(a["score"]) == (b not in c["no_path"])
    for k, part in zip(("contain", "seg"), o["spot"][:2]):
        assert not np.isposinf(_no_nan(part, k)).any()
    lex = _no_nan(o["lex"], "lexicon scores")
    assert np.isfinite(lex).any() and np.isneginf(lex).any() and not np.isposinf(lex).any()
    for name, per_line in o["pat"].items():
        for logp, best, path in per_line:
            _no_nan([logp, best], name)
            assert np.isfinite(best) == (path is not None) and not np.isposinf(logp)
    g64, _ = mc.torch_grads(c)                       # torch leaves NaN at masked entries; the engine's contract is 0 there
    for b in range(5):
        T = int(c["il"][b])
        assert not np.isnan(g64[:T, b][~c["mask"][:T, b]]).any(), b
    import recognize_ref
    want = recognize_ref.recognize_ref(c["logits"])
    for k in ("logps", "alt_logps", "path_logp", "text_nll"):
        _no_nan(want[k], "recognition " + k)


def test_other_oracles_hold_no_nan():
    ps = hc.patset()
    assert ps["logits"].shape == (hc.PATSET_W, 4, 60) and np.isfinite(ps["logits"]).all()
    for logp, best, path in ps["want"]:
        _no_nan([logp, best], "set form")
        assert np.isfinite(logp) and path is not None            # `.` is feasible on every line, T = 1 included
    ed = hc.edit()
    assert 0 in ed["n"].tolist() and 0 in ed["tl"].tolist() and any(n and t for n, t in zip(ed["n"], ed["tl"]))
    assert ed["want"]["edits"].tolist()[:4] == [3, 2, 3, 0]
    ev = hc.evaluate_want()
    assert ev["labels"].shape == (5, 40) and (ev["lengths"] > 0).all() and ev["edits"].dtype == np.int32
    nb = hc.nbest()
    assert np.isfinite(nb["logits"]).all() and nb["logits"].shape == (63, 3, 18) and len(nb["grid"]) == 4
    assert (nb["tl"] > 0).all() and nb["tg"].min() >= 1 and nb["tg"].max() <= nb["C"] - 1
    # the list entry's oracle is the host's; the logits entries' oracles run on the engine's own front-end lists, on the GPU
    import nbest_ref
    _, lengths, logp, score, count, _, _ = nbest_ref.search(nb["idx"], nb["lp"], nb["C"], nb["beam"], nb["n"], nb["bonus"], nb["il"])
    _no_nan(logp, "nbest_topk logp")
    _no_nan(score, "nbest_topk score")
    assert (count == nb["n"]).all() and np.isfinite(logp).all() and np.isfinite(score).all() and (lengths > 0).any()
    wide = hc.recognize_wide()
    assert np.isfinite(wide["logits"]).all() and wide["want"]["lengths"].tolist() == [20, 6, 0]
    for k in ("logps", "alt_logps", "path_logp", "text_nll"):
        assert np.isfinite(_no_nan(wide["want"][k], "wide recognition " + k)).all()


def test_words_probe_has_several_words_and_differing_counts():
    """by words_ref alone: every line has a segmentation with a finite score, at least one has two or more words, the
    counts differ between lines, and two of the lexicon's entries need the masked class 9, which no line can read"""
    c, _ = hc.vocab()
    wd = hc.words()
    assert wd["entries"] == mc.entries(c) and sum(9 in e for e in wd["entries"]) >= 2
    assert wd["priors"].dtype == np.float32 and wd["priors"].shape == (len(wd["entries"]),) and wd["bonus"] == -0.5
    assert len(set(wd["priors"].tolist())) == len(wd["entries"]) and np.isfinite(wd["priors"]).all()
    scores = _no_nan([w[0] for w in wd["want"]], "words score")
    counts = [len(w[1]) for w in wd["want"]]
    print("words probe: scores", scores, "counts", counts)
    assert np.isfinite(scores).all() and max(counts) >= 2 and len(set(counts)) >= 2
    for b, (_, words, starts) in enumerate(wd["want"]):
        assert len(words) == len(starts) >= 1 and starts == sorted(set(starts)) and starts[-1] < c["il"][b], b
        assert not any(9 in wd["entries"][e] for e in words), b


def test_weighted_probes_decode_another_text_than_the_plain_ones():
    """by pattern_w_ref and pattern_ref alone: the weights are float32 in [-2, 2], not all zero, every line is feasible,
    and on at least one line the best text under the weights is not the best text without them"""
    c, o = hc.vocab()
    for name, p in hc.pattern_w().items():
        arcs, finals, ns = mc.patterns(c)[name]
        assert (p["arcs"], p["finals"], p["states"]) == (arcs, finals, ns)
        for w, n in ((p["weights"], len(arcs)), (p["final_weights"], len(finals))):
            assert w.dtype == np.float32 and w.shape == (n,) and (np.abs(w) <= 2).all() and np.abs(w).min() > 0
        differ = []
        for b, (want, plain) in enumerate(zip(p["want"], o["pat"][name])):
            _no_nan(want[:2], name)
            assert np.isfinite(want[0]) and np.isfinite(want[1]) and want[2] is not None and plain[2] is not None, (name, b)
            if hc.pattern_w_ref.collapse(want[2]) != hc.pattern_w_ref.collapse(plain[2]):
                differ.append(b)
            assert abs(want[0] - plain[0]) > 1e-2, (name, b)      # far beyond the base check's rule: logp tells the tables apart too
        print("pattern_w.%s: the weighted best text differs on lines %s" % (name, differ))
        assert differ, name


def test_big_dirtier_words_lexicon_needs_the_scratch_form(pkg):
    """more than 4096 trie nodes (the step buffers leave LDS for the call's scratch) and at most the engine's limit, by
    the engine's own count; the small dirtier's and the probe's tries are the python builder's sizes too"""
    import importlib
    import words_ref
    ctc = importlib.import_module(pkg.__name__ + ".ctc")
    d = hc.big()
    es = d["words_entries"]
    assert all(1 <= len(e) <= 4 and 1 <= min(e) and max(e) <= hc.BIG_C - 1 for e in es)
    assert len(set(c for e in es for c in e)) == hc.BIG_C - 1            # the 63 live labels
    nodes = ctc.Lexicon(es, num_classes=hc.BIG_C).info()["nodes"]
    print("the big dirtier's large lexicon: %d entries, %d nodes" % (len(es), nodes))
    assert nodes == len(words_ref.build_trie(es)[0]) == hc.dirtier_dims(d, max)["nodes"]
    assert ctc.WORDS_LDS_NODES == words_ref.LDS_NODES == 4096 < hc.BIG_WORDS_NODES[0] <= nodes < hc.BIG_WORDS_NODES[1]
    assert nodes <= ctc.WORDS_MAX_NODES == words_ref.MAX_NODES
    assert d["words_bonus"] != 0 and hc.small()["words_bonus"] != 0
    probe = hc.probe_dims()["words"]["nodes"]
    assert probe == len(words_ref.build_trie(hc.words()["entries"])[0]) <= 1024          # one node per thread, in LDS
    assert hc.dirtier_dims(hc.small(), min)["nodes"] == 2 < probe < len(words_ref.build_trie(d["entries"])[0]) <= 4096 < nodes
    for dirt in (d, hc.small()):                                                     # the weighted copies
        assert sorted(dirt["pattern_weights"]) == sorted(dirt["patterns"])
        for k, (w, fw) in dirt["pattern_weights"].items():
            arcs, finals, _ = dirt["patterns"][k]
            assert w.shape == (len(arcs),) and fw.shape == (len(finals),) and np.isfinite(w).all() and w.any()


def test_wide_recognition_grows_the_block_between_its_layouts():
    """csrc/engine.cpp's rec_pass asks for the row figures' layout first and the decoded text's loss layout second, and
    moves the kept log-sum-exps when the second outgrows the block: the wide probe's does, `vocab`'s cannot"""
    import recognize_ref
    wide = hc.recognize_wide()["want"]
    first, second, kept = hc.recognize_needs(wide["labels"], wide["lengths"], hc.WIDE_W)
    print("wide recognition: first %d, second %d, kept %d bytes" % (first, second, kept))
    assert second > first > kept > 0
    assert max(len(set(t)) for t in hc.recognize_wide()["texts"]) == 20
    v = recognize_ref.recognize_ref(hc.vocab()[0]["logits"])
    v_first, v_second, _ = hc.recognize_needs(v["labels"], v["lengths"], 40)
    assert v_second <= v_first, "the vocab probe now reaches the move as well"
    assert first <= v_first < second            # after `vocab`'s recognition the wide one's first request fits, its second does not
    s = recognize_ref.recognize_ref(hc.small()["logits"])
    assert max(hc.recognize_needs(s["labels"], s["lengths"], 2)[:2]) == 3328 < first       # the small case's own recognition


def test_nbest_logits_are_the_existing_case():
    import test_gpu_nbest_lm as tnl
    nb = hc.nbest()
    idx, lp, il = tnl.lists_of(hc.NBEST_NAME)
    assert idx.tobytes() == nb["idx"].tobytes() and lp.tobytes() == nb["lp"].tobytes() and il.tobytes() == nb["il"].tobytes()
    assert (nb["T"], nb["B"], nb["C"]) == (63, 3, 18)


def test_dirtiers_bracket_every_probe():
    dims = hc.probe_dims()
    big, small = hc.dirtier_dims(hc.big(), max), hc.dirtier_dims(hc.small(), min)
    print("big", big, "\nsmall", small)
    assert (big["W"], big["B"], big["C"]) == (hc.BIG_W, hc.BIG_B, hc.BIG_C) == (160, 8, 64)
    assert (small["W"], small["B"], small["C"]) == (2, 1, 3) and hc.small()["logits"].shape == (2, 1, 3)
    assert max(len(t) for t in hc.big()["lines"]) == 70 and max(len(r) for r in hc.big()["edit"][1]) == 300
    for name in hc.PROBES:
        for key, v in dims[name].items():
            assert small[key] < v < big[key], (name, key, small[key], v, big[key])
    assert small["nodes"] < dims["words"]["nodes"] < big["nodes"]       # (named: the words call's step buffers and records)
    for name in ("pattern_w.union", "pattern_w.live_plus", "pattern.union.fwd", "pattern_w.union.fwd"):
        assert dims[name] == dims["pattern." + name.split(".")[1]] and "states" in dims[name]
    # per family, not only over all calls: the targets, the queries, the entries and the references
    c, o = hc.vocab()
    for mine, theirs_big, theirs_small in ((c["lines"], hc.big()["lines"], hc.small()["lines"]),
                                           (o["queries"], hc.big()["queries"], hc.small()["queries"]),
                                           (o["entries"], hc.big()["entries"], hc.small()["entries"]),
                                           (hc.edit()["refs"], hc.big()["edit"][1], hc.small()["edit"][1])):
        m, b, s = hc._seq_dims(mine), hc._seq_dims(theirs_big), hc._seq_dims(theirs_small)
        assert len(theirs_small) < len(mine) < len(theirs_big)
        for key in m:
            if mine is hc.edit()["refs"] and key == "distinct":        # symbols are compared, never an index: no carve
                continue
            assert s[key] < m[key] < b[key], (key, s, m, b)
    assert sorted(set(v for h in hc.big()["edit"][0] + hc.big()["edit"][1] for v in h)) == sorted(hc.EDIT_SYMBOLS)


def test_big_dirtier_has_three_bad_lines():
    d = hc.big()
    z, il = d["logits"], d["il"]
    assert sorted(hc.BIG_BAD.values()) == ["nan", "posinf", "row_neginf"] == sorted(k for k in mc.POISON_KINDS if "late" not in k)
    for b in range(hc.BIG_B):
        bad_rows = np.flatnonzero(~np.isfinite(z[:, b]).all(axis=1))
        if b not in hc.BIG_BAD:
            assert bad_rows.size == 0, b
            continue
        assert bad_rows.tolist() == [hc.BAD_T] and hc.BAD_T < il[b], b
        row = z[hc.BAD_T, b]
        kind = hc.BIG_BAD[b]
        if kind == "nan":
            assert np.isnan(row).sum() == 1 and np.isfinite(np.delete(row, hc.BAD_C)).all()
        elif kind == "posinf":
            assert np.isposinf(row).sum() == 1 and np.isfinite(np.delete(row, hc.BAD_C)).all()
        else:
            assert np.isneginf(row).all()
    assert np.isfinite(d["clean"]).all() and (d["clean"][np.isfinite(z)] == z[np.isfinite(z)]).all()
    # every text fits its line: the dirtier scores real alignments, not the length test's early exit
    for t, T in zip(d["lines"], il):
        assert len(t) + sum(a == b for a, b in zip(t, t[1:])) <= T
    assert len(set(d["lines"][0])) == hc.BIG_C - 1
