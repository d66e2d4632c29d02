"""CTC loss on the engine: the criterion of the reference's evaluation stack (``CTCLoss(zero_infinity=True)`` over
``preds.log_softmax(2)``, main.py:205,379-409), and its gradient in caller logits (``loss.backward()``, main.py:426).

``CTCLoss`` is the drop-in for that criterion on caller logits (``criterion(preds, targets, input_lengths,
target_lengths)``), differentiable when its input requires a gradient; ``hctr_model.ctc_loss`` scores line images
without the logits ever leaving the device (forward only: the engine's trunk has no backward pass). All run the C ABI's
``hctr_ctc_loss*`` (include/hctr_hip.h); target normalisation, the reductions and the per-line gradient weights are the
host-side helpers below, with the semantics of ``torch.nn.CTCLoss``.

``CTCAligner`` and ``hctr_model.align`` are the third member: the best path of a known transcription
(``hctr_ctc_align*``), which says where in the line each character lies and how confident the engine is of it.

``KeywordSpotter`` and ``hctr_model.spot`` answer the word-spotting question (``hctr_spot*``): for every (line, query)
pair the posterior probability that the line's text contains the query, and the best segment that reads it.
"""
import ctypes

import numpy as np

from . import _lib

_REDUCTIONS = ("none", "mean", "sum")


def _is_torch(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def _host_int32(x, name):
    if _is_torch(x):
        x = x.detach().cpu().numpy()
    a = np.asarray(x)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s must hold integers, got %s" % (name, a.dtype))
    return a.astype(np.int64)


def normalize_targets(targets, target_lengths, B):
    """(concatenated int32 targets, int32 target_lengths [B]) from what torch.nn.CTCLoss accepts: 1-D concatenated
    targets (what ``codec.encode`` returns; their count must equal sum(target_lengths)) or 2-D padded ``[B, S]`` targets
    (line b's labels are targets[b, :target_lengths[b]])."""
    tl = _host_int32(target_lengths, "target_lengths").reshape(-1)
    if tl.shape != (B,):
        raise ValueError("target_lengths must have %d entries, got %d" % (B, tl.size))
    if (tl < 0).any():
        raise ValueError("target_lengths must be >= 0")
    tg = _host_int32(targets, "targets")
    if tg.ndim == 2:
        if tg.shape[0] != B:
            raise ValueError("2-D targets must have %d rows, got %d" % (B, tg.shape[0]))
        if (tl > tg.shape[1]).any():
            raise ValueError("a target length exceeds the padded targets' width %d" % tg.shape[1])
        flat = np.concatenate([tg[b, :tl[b]] for b in range(B)]) if B else np.zeros((0,), np.int64)
    elif tg.ndim == 1:
        if tg.size != int(tl.sum()):
            raise ValueError("1-D targets hold %d labels but sum(target_lengths) = %d" % (tg.size, int(tl.sum())))
        flat = tg
    else:
        raise ValueError("targets must be 1-D (concatenated) or 2-D (padded), got %d dimensions" % tg.ndim)
    if flat.size and (flat.min() < np.iinfo(np.int32).min or flat.max() > np.iinfo(np.int32).max):
        raise ValueError("target id out of the int32 range")
    return np.ascontiguousarray(flat, dtype=np.int32), np.ascontiguousarray(tl, dtype=np.int32)


def normalize_input_lengths(input_lengths, B):
    if input_lengths is None:
        return None
    il = _host_int32(input_lengths, "input_lengths").reshape(-1)
    if il.shape != (B,):
        raise ValueError("input_lengths must have %d entries, got %d" % (B, il.size))
    return np.ascontiguousarray(il, dtype=np.int32)


def reduce(nll, target_lengths, reduction="mean", zero_infinity=False):
    """torch.nn.CTCLoss's reduction of per-line losses (float32 [B]): zero_infinity replaces +inf by 0; 'mean' divides
    each loss by clamp(target_length, min=1) and averages over the lines; 'sum' adds; 'none' returns them."""
    if reduction not in _REDUCTIONS:
        raise ValueError("reduction must be one of %s" % (_REDUCTIONS,))
    loss = np.array(nll, dtype=np.float32).reshape(-1)
    if zero_infinity:
        loss[np.isinf(loss)] = 0.0
    if reduction == "none":
        return loss
    if reduction == "sum":
        return np.float32(loss.sum(dtype=np.float32))
    tl = np.maximum(np.asarray(target_lengths, dtype=np.float32).reshape(-1), np.float32(1))
    if loss.size == 0:
        return np.float32(np.nan)
    return np.float32((loss / tl).mean(dtype=np.float32))


def line_weights(target_lengths, reduction="mean", grad_output=None, nll=None, zero_infinity=False):
    """(w float32 [B], nan bool [B]): d(reduced loss)/d(nll_b) times the incoming gradient, i.e. the per-line weight
    hctr_ctc_loss_logits_grad takes, with torch.nn.CTCLoss's semantics: 'mean' gives line b ``g / (B * max(L_b, 1))``,
    'sum' ``g``, 'none' ``g_b`` (``grad_output`` None = 1). A line whose ``nll`` is +inf has an all-zero gradient under
    ``zero_infinity`` (weight 0; the engine writes its zeros whatever the weight) and otherwise the NaN rows torch's CPU
    kernel leaves there: ``nan[b]`` marks it, for ``fill_nan_rows``."""
    if reduction not in _REDUCTIONS:
        raise ValueError("reduction must be one of %s" % (_REDUCTIONS,))
    tl = np.asarray(target_lengths).reshape(-1)
    B = tl.size
    if grad_output is None:
        g = np.ones((B,) if reduction == "none" else (), np.float64)
    else:
        g = np.asarray(grad_output, dtype=np.float64)
    if reduction == "none":
        if g.shape != (B,):
            raise ValueError("grad_output of reduction 'none' must have %d entries, got shape %s" % (B, g.shape))
        w = g.copy()
    elif g.size != 1:
        raise ValueError("grad_output of reduction %r must be a scalar" % reduction)
    elif reduction == "sum":
        w = np.full((B,), float(g.reshape(())), np.float64)
    else:
        w = float(g.reshape(())) / (B * np.maximum(tl.astype(np.float64), 1.0))
    inf = np.zeros((B,), bool) if nll is None else np.isposinf(np.asarray(nll, dtype=np.float64).reshape(-1))
    if inf.shape != (B,):
        raise ValueError("nll must have %d entries" % B)
    w[inf] = 0.0
    return w.astype(np.float32), inf & (not zero_infinity)


def fill_nan_rows(grad, nan, input_lengths):
    """torch's CPU kernel on a line without an alignment and zero_infinity off: the line's rows t < input_length are
    NaN (rows past it stay zero). ``grad``: [T, B, C] numpy array or torch tensor, changed in place."""
    for b in np.flatnonzero(nan):
        T = grad.shape[0] if input_lengths is None else int(input_lengths[b])
        grad[:T, int(b)] = float("nan")
    return grad


def wrap(value, like):
    """numpy result -> a float32 torch tensor on `like`'s device when `like` is a torch tensor."""
    if not _is_torch(like):
        return value
    import torch
    return torch.as_tensor(np.asarray(value, dtype=np.float32), device=like.device)


def loss_logits(ctx, logits, on_dev, targets, target_lengths, input_lengths):
    """per-line NLL (float32 [B]) of caller logits / log-probs in WBC layout (hctr_ctc_loss_logits)."""
    W, B, C = (int(v) for v in logits.shape)
    tg, tl = normalize_targets(targets, target_lengths, B)
    il = normalize_input_lengths(input_lengths, B)
    nll = np.empty((B,), dtype=np.float32)
    if B == 0:
        return nll
    _lib.check(_lib.load().hctr_ctc_loss_logits(ctx, _lib.ptr(logits), on_dev, W, B, C, _lib.ptr(tg), _lib.ptr(tl),
                                                _lib.ptr(il), _lib.ptr(nll)), ctx)
    return nll


def loss_grad_logits(ctx, logits, on_dev, targets, target_lengths, input_lengths, weights, grad=None):
    """(per-line NLL float32 [B], gradient) of caller logits / log-probs in WBC layout (hctr_ctc_loss_logits_grad):
    grad[t, b] = weights[b] * (softmax(z[t, b]) - gamma[t, b]); ``weights`` None = 1 for every line. The gradient is a
    float32 tensor on the logits' device when they are a CUDA tensor, a numpy array otherwise (``grad``: a buffer of
    that kind to write into)."""
    W, B, C = (int(v) for v in logits.shape)
    tg, tl = normalize_targets(targets, target_lengths, B)
    il = normalize_input_lengths(input_lengths, B)
    nll = np.empty((B,), dtype=np.float32)
    if grad is None:
        if on_dev:
            import torch
            grad = torch.empty((W, B, C), dtype=torch.float32, device=logits.device)
        else:
            grad = np.empty((W, B, C), dtype=np.float32)
    if B == 0 or W == 0:
        return nll, grad
    wt = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
    if wt is not None and wt.shape != (B,):
        raise ValueError("weights must have %d entries, got %d" % (B, wt.size))
    _lib.check(_lib.load().hctr_ctc_loss_logits_grad(ctx, _lib.ptr(logits), on_dev, W, B, C, _lib.ptr(tg), _lib.ptr(tl),
                                                     _lib.ptr(il), _lib.ptr(wt), _lib.ptr(nll), _lib.ptr(grad),
                                                     on_dev), ctx)
    return nll, grad


class CTCAlignment(object):
    """Result of a forced alignment of B lines of W steps (numpy arrays, on the host):
    ``paths`` int32 [B, W], the class of the best path at every step (0 = blank, -1 past a line's input length);
    ``scores`` float32 [B], the best path's log-probability; ``starts`` / ``ends`` int32 and ``logps`` float32
    [sum L], per target position the first step, the step after the last and the sum of the label's log-probabilities
    over them; ``offsets`` int64 [B + 1], where each line's positions begin; ``targets`` int32 [sum L]. A line with no
    alignment - too short for its targets, or every path through a masked (-inf) logit - has score -inf, -1 everywhere
    and logps -inf."""

    def __init__(self, paths, scores, starts, ends, logps, targets, target_lengths):
        self.paths, self.scores = paths, scores
        self.starts, self.ends, self.logps = starts, ends, logps
        self.targets = targets
        self.offsets = np.concatenate([[0], np.cumsum(np.asarray(target_lengths, np.int64))]).astype(np.int64)

    def __len__(self):
        return len(self.offsets) - 1

    def lines(self):
        """yields per line the list of (label, start, end, confidence), one per character: its pixel-column span
        [start, end) and the geometric mean of its probability over the span, exp(logp / (end - start)), in (0, 1];
        (label, -1, -1, 0.0) for the characters of a line with no alignment."""
        for b in range(len(self)):
            out = []
            for j in range(int(self.offsets[b]), int(self.offsets[b + 1])):
                st, en = int(self.starts[j]), int(self.ends[j])
                conf = float(np.exp(np.float64(self.logps[j]) / (en - st))) if en > st else 0.0
                out.append((int(self.targets[j]), st, en, conf))
            yield out


def _align_outputs(B, W, total):
    return (np.empty((B, W), np.int32), np.empty((total,), np.int32), np.empty((total,), np.int32),
            np.empty((total,), np.float32), np.empty((B,), np.float32))


def align_logits(ctx, logits, on_dev, targets, target_lengths, input_lengths):
    """CTCAlignment of caller logits / log-probs in WBC layout (hctr_ctc_align_logits)."""
    W, B, C = (int(v) for v in logits.shape)
    tg, tl = normalize_targets(targets, target_lengths, B)
    il = normalize_input_lengths(input_lengths, B)
    path, st, en, lp, score = _align_outputs(B, W, int(tg.size))
    if B:
        _lib.check(_lib.load().hctr_ctc_align_logits(ctx, _lib.ptr(logits), on_dev, W, B, C, _lib.ptr(tg), _lib.ptr(tl),
                                                     _lib.ptr(il), _lib.ptr(path), _lib.ptr(st), _lib.ptr(en),
                                                     _lib.ptr(lp), _lib.ptr(score)), ctx)
    return CTCAlignment(path, score, st, en, lp, tg, tl)


def align_images(ctx, x, dt, on_dev, widths, B, W, targets, target_lengths, input_lengths):
    """CTCAlignment of line images (hctr_ctc_align); x, dt, on_dev, widths as hctr_model._img_args / _widths give them."""
    tg, tl = normalize_targets(targets, target_lengths, B)
    il = normalize_input_lengths(input_lengths, B)
    path, st, en, lp, score = _align_outputs(B, W, int(tg.size))
    if B:
        _lib.check(_lib.load().hctr_ctc_align(ctx, _lib.ptr(x), dt, on_dev, _lib.ptr(widths), B, W, _lib.ptr(tg),
                                              _lib.ptr(tl), _lib.ptr(il), _lib.ptr(path), _lib.ptr(st), _lib.ptr(en),
                                              _lib.ptr(lp), _lib.ptr(score)), ctx)
    return CTCAlignment(path, score, st, en, lp, tg, tl)


SPOT_MAX_LEN = 32      # HCTR_SPOT_MAX_LEN


def normalize_queries(queries):
    """(concatenated int32 labels, int32 query_lengths [Q]) from a sequence of label sequences (lists, arrays); every
    query has 1..32 labels. Label ranges are checked by the engine, which knows C."""
    qs = [np.asarray(_host_int32(q, "queries")).reshape(-1) for q in queries]
    if not qs:
        raise ValueError("need at least one query")
    ql = np.array([q.size for q in qs], dtype=np.int32)
    if (ql < 1).any() or (ql > SPOT_MAX_LEN).any():
        raise ValueError("every query must have 1..%d labels, got lengths %s" % (SPOT_MAX_LEN, ql.tolist()))
    flat = np.concatenate(qs)
    if flat.min() < np.iinfo(np.int32).min or flat.max() > np.iinfo(np.int32).max:
        raise ValueError("query id out of the int32 range")
    return np.ascontiguousarray(flat, dtype=np.int32), ql


class Spotting(object):
    """Result of keyword spotting of Q queries in B lines (numpy arrays, on the host; include/hctr_hip.h ``hctr_spot``):
    ``logp`` float32 [B, Q], the log of the probability that the line's text contains the query (an exact sum over all
    CTC paths; -inf where it cannot); ``seg_logp`` float32 [B, Q], ``starts`` / ``ends`` int32 [B, Q]: the best tight
    segment that reads the query, its log-probability and pixel-column span [start, end) (-inf, -1, -1 where none fits).
    The span runs from inside the first character's run to inside the last one's; ``align`` / ``recognize`` give full
    character extents."""

    def __init__(self, logp, seg_logp, starts, ends):
        self.logp, self.seg_logp, self.starts, self.ends = logp, seg_logp, starts, ends

    def __len__(self):
        return int(self.logp.shape[0])

    def probs(self):
        """float64 [B, Q]: the probability that line b contains query k"""
        return np.exp(self.logp.astype(np.float64))

    def hits(self, threshold=0.5):
        """the (line, query, prob, start, end) of every pair whose containment probability is >= threshold, by line
        then query"""
        p = self.probs()
        return [(int(b), int(k), float(p[b, k]), int(self.starts[b, k]), int(self.ends[b, k]))
                for b, k in zip(*np.nonzero(p >= threshold))]

    def lines(self):
        """yields per line the list of (query, prob, start, end), one per query"""
        p = self.probs()
        for b in range(len(self)):
            yield [(k, float(p[b, k]), int(self.starts[b, k]), int(self.ends[b, k])) for k in range(p.shape[1])]


def _spot_outputs(B, Q):
    return (np.full((B, Q), -np.inf, np.float32), np.full((B, Q), -np.inf, np.float32), np.full((B, Q), -1, np.int32),
            np.full((B, Q), -1, np.int32))


def spot_logits(ctx, logits, on_dev, queries, input_lengths=None):
    """Spotting of caller logits / log-probs in WBC layout (hctr_spot_logits); ``queries``: label sequences."""
    W, B, C = (int(v) for v in logits.shape)
    qf, ql = normalize_queries(queries)
    il = normalize_input_lengths(input_lengths, B)
    logp, seg, st, en = _spot_outputs(B, int(ql.size))
    if B and W:
        _lib.check(_lib.load().hctr_spot_logits(ctx, _lib.ptr(logits), on_dev, W, B, C, _lib.ptr(qf), _lib.ptr(ql),
                                                int(ql.size), _lib.ptr(il), _lib.ptr(logp), _lib.ptr(seg), _lib.ptr(st),
                                                _lib.ptr(en)), ctx)
    return Spotting(logp, seg, st, en)


def spot_images(ctx, x, dt, on_dev, widths, B, W, queries, input_lengths=None):
    """Spotting of line images (hctr_spot); x, dt, on_dev, widths as hctr_model._img_args / _widths give them."""
    qf, ql = normalize_queries(queries)
    il = normalize_input_lengths(input_lengths, B)
    logp, seg, st, en = _spot_outputs(B, int(ql.size))
    if B:
        _lib.check(_lib.load().hctr_spot(ctx, _lib.ptr(x), dt, on_dev, _lib.ptr(widths), B, W, _lib.ptr(qf), _lib.ptr(ql),
                                         int(ql.size), _lib.ptr(il), _lib.ptr(logp), _lib.ptr(seg), _lib.ptr(st),
                                         _lib.ptr(en)), ctx)
    return Spotting(logp, seg, st, en)


def spot_chunk_classes(lines, W):
    """classes (blank included) one chunk of queries may hold for `lines` lines of W columns (hctr_spot_chunk_classes)"""
    return int(_lib.load().hctr_spot_chunk_classes(int(lines), int(W)))


LEX_MAX_LEN = 64       # HCTR_LEX_MAX_LEN
LEX_MAX_TOP = 32       # HCTR_LEX_MAX_TOP
LEX_SKIP, LEX_FIRST, LEX_PARENT_MASK = 1 << 30, 1 << 29, 0xFFFF


class Lexicon(object):
    """A closed list of admissible texts for lexicon recognition (include/hctr_hip.h ``hctr_lex_build``): the trie of the
    entries and its partition into units, built on the host (no GPU needed). ``entries``: strings when a ``codec`` is
    given to encode them (a character outside its vocabulary is a ValueError), else label sequences of 1..64 labels in
    [1, C-1], with ``num_classes`` = C (with a codec, its character count). ``priors``: one finite log prior per entry,
    or None. ``unit_nodes``: trie nodes one workgroup holds (0 = the default; else 128..4096). Duplicates are separate
    entries. The object is immutable and serves any number of contexts."""

    def __init__(self, entries, codec=None, priors=None, unit_nodes=0, num_classes=None):
        entries = list(entries)
        self.texts = None
        if codec is not None:
            if any(not isinstance(s, str) for s in entries):
                raise ValueError("with a codec the entries are strings")
            flat, ln = codec.encode_queries(entries)
            labels = np.split(np.asarray(flat, dtype=np.int32), np.cumsum(ln)[:-1]) if len(entries) else []
            self.texts = entries
            if num_classes is None:
                num_classes = len(codec.characters)
        else:
            labels = [np.asarray(_host_int32(e, "entries")).reshape(-1) for e in entries]
        if num_classes is None:
            raise ValueError("num_classes is needed when the entries are label sequences")
        if not labels:
            raise ValueError("need at least one entry")
        ln = np.array([e.size for e in labels], dtype=np.int32)
        flat = np.concatenate(labels) if ln.sum() else np.zeros(0, np.int64)
        if flat.size and (flat.min() < np.iinfo(np.int32).min or flat.max() > np.iinfo(np.int32).max):
            raise ValueError("label out of the int32 range")
        flat = np.ascontiguousarray(flat, dtype=np.int32)
        pr = None
        if priors is not None:
            pr = np.ascontiguousarray(np.asarray(priors, dtype=np.float64).reshape(-1), dtype=np.float32)
            if pr.shape != (len(labels),):
                raise ValueError("priors must have one value per entry")
        self.labels = [np.asarray(e, dtype=np.int32) for e in labels]
        self.priors = pr
        self.num_classes = int(num_classes)
        lib = _lib.load()
        h = ctypes.c_void_p()
        rc = lib.hctr_lex_build(_lib.ptr(flat), _lib.ptr(ln), len(labels), self.num_classes, _lib.ptr(pr), int(unit_nodes),
                                ctypes.byref(h))
        self._h = h if rc == 0 else None
        _lib.check(rc, None)

    def __len__(self):
        return len(self.labels)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.load().hctr_lex_free(self._h)
                self._h = None
        except Exception:
            pass

    def entry(self, e):
        """entry e as the caller gave it: its string (built with a codec) or its labels as a list"""
        return self.texts[e] if self.texts is not None else self.labels[e].tolist()

    def info(self):
        """dict: entries, nodes (the trie's, root included), units, classes (distinct), max_len"""
        v = [ctypes.c_int32() for _ in range(5)]
        _lib.check(_lib.load().hctr_lex_info(self._h, *[ctypes.byref(x) for x in v]), None)
        return dict(zip(("entries", "nodes", "units", "classes", "max_len"), (int(x.value) for x in v)))

    def tables(self):
        """dict of numpy arrays: what ``hctr_lex_tables`` exports - the global trie (parent, label, entry_node) and the
        unit tables the kernel is given (unit_off, class_off, unit_node, unit_word, unit_owned, unit_kidx, unit_class,
        entry_ptr, entry_list)."""
        lib, i = _lib.load(), self.info()
        ut, ct = ctypes.c_int64(), ctypes.c_int64()
        none = [None] * 7
        _lib.check(lib.hctr_lex_tables(self._h, None, None, None, None, None, ctypes.byref(ut), ctypes.byref(ct), *none), None)
        ut, ct = int(ut.value), int(ct.value)
        t = {"parent": np.zeros(i["nodes"], np.int32), "label": np.zeros(i["nodes"], np.int32),
             "entry_node": np.zeros(i["entries"], np.int32), "unit_off": np.zeros(i["units"] + 1, np.int32),
             "class_off": np.zeros(i["units"] + 1, np.int32), "unit_node": np.zeros(ut, np.int32),
             "unit_word": np.zeros(ut, np.int32), "unit_owned": np.zeros(ut, np.uint8), "unit_kidx": np.zeros(ut, np.int32),
             "unit_class": np.zeros(ct, np.int32), "entry_ptr": np.zeros(ut + 1, np.int32),
             "entry_list": np.zeros(i["entries"], np.int32)}
        _lib.check(lib.hctr_lex_tables(self._h, _lib.ptr(t["parent"]), _lib.ptr(t["label"]), _lib.ptr(t["entry_node"]),
                                       _lib.ptr(t["unit_off"]), _lib.ptr(t["class_off"]), None, None,
                                       _lib.ptr(t["unit_node"]), _lib.ptr(t["unit_word"]), _lib.ptr(t["unit_owned"]),
                                       _lib.ptr(t["unit_kidx"]), _lib.ptr(t["unit_class"]), _lib.ptr(t["entry_ptr"]),
                                       _lib.ptr(t["entry_list"])), None)
        return t


class LexiconResult(object):
    """Result of lexicon recognition of B lines against N entries (numpy arrays, on the host; include/hctr_hip.h
    ``hctr_lexicon``): ``entries`` int32 [B, n], the best entries of each line in descending rank (ties to the lower
    index; -1 in unused places); ``logp`` float32 [B, n], their exact log p(entry | line); ``rank`` float64 [B, n] =
    logp + log prior; ``log_total`` float64 [B], the log of the lexicon's total mass on the line; ``count`` int32 [B];
    ``scores`` float32 [B, N], every entry's logp, or None."""

    def __init__(self, lex, entries, logp, rank, log_total, count, scores=None):
        self.lex = lex
        self.entries, self.logp, self.rank, self.log_total, self.count, self.scores = (entries, logp, rank, log_total,
                                                                                       count, scores)

    def __len__(self):
        return int(self.entries.shape[0])

    def posteriors(self):
        """float64 [B, n]: exp(rank - log_total), the probability of each returned entry within the lexicon (0 in unused
        places)"""
        with np.errstate(invalid="ignore"):
            p = np.exp(self.rank - self.log_total[:, None])
        return np.where(self.entries >= 0, p, 0.0)

    def best(self):
        """per line the best entry as the lexicon was given it (a string or a label list), None where no entry fits"""
        return [self.lex.entry(int(e)) if e >= 0 else None for e in self.entries[:, 0]]

    def lines(self):
        """yields per line the list of (entry_index, text_or_labels, logp, posterior) of its returned entries"""
        post = self.posteriors()
        for b in range(len(self)):
            yield [(int(self.entries[b, k]), self.lex.entry(int(self.entries[b, k])), float(self.logp[b, k]),
                    float(post[b, k])) for k in range(int(self.count[b]))]


def _lexicon_outputs(lex, B, n, scores):
    if not isinstance(lex, Lexicon):
        raise ValueError("lex must be a ctc.Lexicon")
    n = int(n)
    if n < 1 or n > LEX_MAX_TOP:
        raise ValueError("n must be in 1..%d, got %d" % (LEX_MAX_TOP, n))
    return (np.full((B, n), -1, np.int32), np.full((B, n), -np.inf, np.float32), np.full((B, n), -np.inf, np.float64),
            np.full(B, -np.inf, np.float64), np.zeros(B, np.int32),
            np.full((B, len(lex)), -np.inf, np.float32) if scores else None)


def lexicon_logits(ctx, logits, on_dev, lex, n=5, input_lengths=None, scores=False):
    """LexiconResult of caller logits / log-probs in WBC layout (hctr_lexicon_logits)"""
    W, B, C = (int(v) for v in logits.shape)
    il = normalize_input_lengths(input_lengths, B)
    ent, lp, rk, tot, cnt, sc = _lexicon_outputs(lex, B, n, scores)
    if B and W:
        _lib.check(_lib.load().hctr_lexicon_logits(ctx, lex._h, _lib.ptr(logits), on_dev, W, B, C, _lib.ptr(il), int(n),
                                                   _lib.ptr(ent), _lib.ptr(lp), _lib.ptr(rk), _lib.ptr(tot), _lib.ptr(cnt),
                                                   _lib.ptr(sc)), ctx)
    return LexiconResult(lex, ent, lp, rk, tot, cnt, sc)


def lexicon_images(ctx, x, dt, on_dev, widths, B, W, lex, n=5, input_lengths=None, scores=False):
    """LexiconResult of line images (hctr_lexicon); x, dt, on_dev, widths as hctr_model._img_args / _widths give them."""
    il = normalize_input_lengths(input_lengths, B)
    ent, lp, rk, tot, cnt, sc = _lexicon_outputs(lex, B, n, scores)
    if B:
        _lib.check(_lib.load().hctr_lexicon(ctx, lex._h, _lib.ptr(x), dt, on_dev, _lib.ptr(widths), B, W, _lib.ptr(il),
                                            int(n), _lib.ptr(ent), _lib.ptr(lp), _lib.ptr(rk), _lib.ptr(tot), _lib.ptr(cnt),
                                            _lib.ptr(sc)), ctx)
    return LexiconResult(lex, ent, lp, rk, tot, cnt, sc)


def lexicon_chunk_classes(lines, W):
    """classes (blank included) one chunk of units may hold for `lines` lines of W columns (hctr_lexicon_chunk_classes)"""
    return int(_lib.load().hctr_lexicon_chunk_classes(int(lines), int(W)))


WORDS_MAX_NODES = 65536    # HCTR_WORDS_MAX_NODES
WORDS_LDS_NODES = 4096     # HCTR_WORDS_LDS_NODES


def lex_word_tables(lex, word_bonus=0.0):
    """dict of numpy arrays: what ``hctr_lex_word_tables`` exports for word-sequence recognition - per trie node ``node``
    (parent | LEX_SKIP | LEX_FIRST), ``slot``, ``entry`` (e_v or -1) and ``weight`` (x_v), and ``classes`` (0, then the
    distinct labels ascending)."""
    if not isinstance(lex, Lexicon):
        raise ValueError("lex must be a ctc.Lexicon")
    lib = _lib.load()
    nn, nc = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(lib.hctr_lex_word_tables(lex._h, float(word_bonus), ctypes.byref(nn), ctypes.byref(nc), None, None, None, None,
                                        None), None)
    nn, nc = int(nn.value), int(nc.value)
    t = {"node": np.zeros(nn, np.int32), "slot": np.zeros(nn, np.int32), "entry": np.zeros(nn, np.int32),
         "weight": np.zeros(nn, np.float32), "classes": np.zeros(nc, np.int32)}
    _lib.check(lib.hctr_lex_word_tables(lex._h, float(word_bonus), None, None, _lib.ptr(t["node"]), _lib.ptr(t["slot"]),
                                        _lib.ptr(t["entry"]), _lib.ptr(t["weight"]), _lib.ptr(t["classes"])), None)
    return t


class WordsResult(object):
    """Result of word-sequence recognition of B lines of W steps (numpy arrays, on the host; include/hctr_hip.h
    ``hctr_words``): ``score`` float32 [B], the best path's log-probability plus the weights of its words; ``count`` int32
    [B], the number of words (it may exceed the returned ones); ``words`` / ``starts`` int32 [B, max_words], the entries
    in line order and the column at which each begins (-1 in unused places); ``labels`` int32 [B, W] / ``lengths`` int32
    [B], the concatenated text; ``text_nll`` float32 [B], the CTC loss of that text. Where no sequence of entries fits the
    line, score is -inf, count 0, lengths 0, text_nll +inf."""

    def __init__(self, score, count, words, starts, labels, lengths, text_nll, input_lengths=None):
        self.score, self.count, self.words, self.starts = score, count, words, starts
        self.labels, self.lengths, self.text_nll = labels, lengths, text_nll
        self.input_lengths = input_lengths

    def __len__(self):
        return len(self.score)

    def label_lists(self):
        return [self.labels[b, :int(self.lengths[b])].copy() for b in range(len(self))]

    def texts(self, codec):
        """the concatenated text of every line ('' where nothing fits)"""
        return codec.labels_to_text([l.tolist() for l in self.label_lists()])

    def posterior(self):
        """float64 [B]: exp(-text_nll), the probability of the concatenated text given the line (0 where nothing fits)"""
        with np.errstate(invalid="ignore", over="ignore"):
            p = np.exp(-np.asarray(self.text_nll, np.float64))
        return np.where(self.count > 0, p, 0.0)

    def lines(self, lex):
        """yields per line the list of (entry_index, entry, start, end) of its returned words: the entry as the lexicon
        was given it and its column span [start, end) - up to the next word's start, or the line's length for the line's
        last word; None for the end of the last returned word when ``count`` exceeds ``max_words``"""
        for b in range(len(self)):
            n = min(int(self.count[b]), self.words.shape[1])
            T = int(self.input_lengths[b]) if self.input_lengths is not None else int(self.labels.shape[1])
            out = []
            for j in range(n):
                end = int(self.starts[b, j + 1]) if j + 1 < n else T if n == int(self.count[b]) else None
                out.append((int(self.words[b, j]), lex.entry(int(self.words[b, j])), int(self.starts[b, j]), end))
            yield out


def _words_outputs(lex, B, W, max_words):
    if not isinstance(lex, Lexicon):
        raise ValueError("lex must be a ctc.Lexicon")
    mw = W if max_words is None else int(max_words)
    if B and W and (mw < 1 or mw > W):
        raise ValueError("max_words must be in 1..%d, got %d" % (W, mw))
    mw = max(mw, 1)
    i, f = np.int32, np.float32
    return mw, (np.full(B, -np.inf, f), np.zeros(B, i), np.full((B, mw), -1, i), np.full((B, mw), -1, i),
                np.zeros((B, W), i), np.zeros(B, i), np.full(B, np.inf, f))


def words_logits(ctx, logits, on_dev, lex, word_bonus=0.0, max_words=None, input_lengths=None):
    """WordsResult of caller logits / log-probs in WBC layout (hctr_words_logits)"""
    if len(logits.shape) != 3:
        raise ValueError("logits must be [W,B,C]")
    W, B, C = (int(v) for v in logits.shape)
    il = normalize_input_lengths(input_lengths, B)
    mw, out = _words_outputs(lex, B, W, max_words)
    if B and W:
        _lib.check(_lib.load().hctr_words_logits(ctx, lex._h, _lib.ptr(logits), on_dev, W, B, C, _lib.ptr(il),
                                                 float(word_bonus), mw, *[_lib.ptr(a) for a in out]), ctx)
    return WordsResult(*out, input_lengths=il if il is not None else np.full(B, W, np.int32))


def words_images(ctx, x, dt, on_dev, widths, B, W, lex, word_bonus=0.0, max_words=None, input_lengths=None):
    """WordsResult of line images (hctr_words); x, dt, on_dev, widths as hctr_model._img_args / _widths give them."""
    il = normalize_input_lengths(input_lengths, B)
    mw, out = _words_outputs(lex, B, W, max_words)
    if B:
        _lib.check(_lib.load().hctr_words(ctx, lex._h, _lib.ptr(x), dt, on_dev, _lib.ptr(widths), B, W, _lib.ptr(il),
                                          float(word_bonus), mw, *[_lib.ptr(a) for a in out]), ctx)
    return WordsResult(*out, input_lengths=il if il is not None else np.full(B, W, np.int32))


PAT_MAX_STATES = 8192      # HCTR_PAT_MAX_STATES
PAT_MAX_EDGES = 262144     # HCTR_PAT_MAX_EDGES


class _Regex(object):
    """The regular expressions ``Pattern.compile`` accepts, a subset of Python's ``re`` with ``re.fullmatch``'s meaning:
    literals and ``\\`` escapes, ``.``, ``[...]`` / ``[^...]`` with code-point ranges, ``\\d``, ``( )`` (and ``(?: )``),
    ``|``, ``?`` ``*`` ``+``, ``{m}`` ``{m,n}`` ``{m,}`` ``{,n}``. ``vocab`` maps a character to its label; ``.``,
    negated sets and ranges mean the characters of ``vocab`` only. parse() returns the syntax tree: ("set", frozenset of
    labels), ("cat", [nodes]), ("alt", [nodes]), ("rep", node, m, n or None)."""

    SPECIAL = set(".[]()|?*+{}\\^$")

    def __init__(self, expr, vocab):
        self.s, self.i, self.vocab = expr, 0, vocab

    def error(self, what):
        return ValueError("pattern %r, position %d: %s" % (self.s, self.i, what))

    def peek(self):
        return self.s[self.i] if self.i < len(self.s) else ""

    def take(self):
        ch = self.peek()
        if not ch:
            raise self.error("unexpected end")
        self.i += 1
        return ch

    def label(self, ch):
        if ch not in self.vocab:
            raise self.error("character %r is not in the vocabulary" % ch)
        return self.vocab[ch]

    def digits(self):
        d = frozenset(self.vocab[ch] for ch in "0123456789" if ch in self.vocab)
        if not d:
            raise self.error("\\d: the vocabulary has no digit")
        return d

    def parse(self):
        node = self.alt()
        if self.i != len(self.s):
            raise self.error("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.peek() not in ("", "|", ")"):
            items.append(self.repeat(self.atom()))
        return ("cat", items)

    def number(self):
        at = self.i
        while self.peek().isdigit() and self.peek().isascii():
            self.i += 1
        return int(self.s[at:self.i]) if self.i > at else None

    def repeat(self, node):
        while True:
            ch = self.peek()
            if ch == "?":
                m, n = 0, 1
            elif ch == "*":
                m, n = 0, None
            elif ch == "+":
                m, n = 1, None
            elif ch == "{":
                self.i += 1
                m = self.number()
                if self.peek() == ",":
                    self.i += 1
                    n = self.number()
                    m = 0 if m is None else m
                else:
                    n = m
                    if m is None:
                        raise self.error("'{' needs a count")
                if self.peek() != "}":
                    raise self.error("malformed {m,n}")
                if n is not None and n < m:
                    raise self.error("{m,n} with n < m")
            else:
                return node
            self.i += 1                        # the quantifier's last character
            if self.peek() in ("?", "+", "*", "{"):
                raise self.error("a quantifier after a quantifier is not supported")
            node = ("rep", node, m, n)

    def atom(self):
        ch = self.take()
        if ch == "(":
            if self.s.startswith("?:", self.i):
                self.i += 2
            elif self.peek() == "?":
                raise self.error("only (?: ) groups are supported")
            node = self.alt()
            if self.peek() != ")":
                raise self.error("missing ')'")
            self.i += 1
            return node
        if ch == "[":
            return ("set", self.char_set())
        if ch == ".":
            return ("set", frozenset(self.vocab.values()))
        if ch == "\\":
            e = self.take()
            if e == "d":
                return ("set", self.digits())
            if e.isalnum():
                raise self.error("escape \\%s is not supported" % e)
            return ("set", frozenset([self.label(e)]))
        if ch in self.SPECIAL:
            raise self.error("unexpected %r" % ch)
        return ("set", frozenset([self.label(ch)]))

    def char_set(self):
        negate = self.peek() == "^"
        if negate:
            self.i += 1
        members, first = set(), True
        while True:
            ch = self.take()
            if ch == "]" and not first:
                break
            first = False
            if ch == "\\":
                e = self.take()
                if e == "d":
                    members |= self.digits()
                    continue
                if e.isalnum():
                    raise self.error("escape \\%s is not supported" % e)
                ch = e
            if self.peek() == "-" and self.s[self.i + 1:self.i + 2] not in ("]", ""):
                self.i += 1
                hi = self.take()
                if hi == "\\":
                    hi = self.take()
                if ord(hi) < ord(ch):
                    raise self.error("bad character range %s-%s" % (ch, hi))
                members |= set(v for k, v in self.vocab.items() if ord(ch) <= ord(k) <= ord(hi))
            else:
                members.add(self.label(ch))
        if negate:
            members = set(self.vocab.values()) - members
        return frozenset(members)


def _regex_to_dfa(tree, sets=False):
    """(arcs, finals, num_states) of the minimal DFA of a ``_Regex`` tree, its states numbered breadth-first from the start
    over labels ascending - a function of the language, not of how it was spelt. arcs: int32 [n, 3] rows (src, label, dst)
    sorted by (src, label). An empty language gives one state without finals. ``sets=True``: (arcs, sets, finals,
    num_states) with the arcs before they are expanded - rows (src, set, dst) sorted by (src, the set's smallest label),
    ``sets`` the list of ascending int32 label arrays (the expression's alphabet classes) they index."""
    # atoms -> alphabet classes: labels with the same membership in every set of the expression behave alike
    atoms, eps, tr = [], [[]], [[]]

    def new():
        eps.append([])
        tr.append([])
        if len(eps) > 200000:
            raise ValueError("the pattern is too large (more than 200000 NFA states)")
        return len(eps) - 1

    def frag(node, s):
        kind = node[0]
        if kind == "set":
            e = new()
            atoms.append(node[1])
            tr[s].append((len(atoms) - 1, e))
            return e
        if kind == "cat":
            for child in node[1]:
                s = frag(child, s)
            return s
        if kind == "alt":
            e = new()
            for child in node[1]:
                a = new()
                eps[s].append(a)
                eps[frag(child, a)].append(e)
            return e
        _, child, m, n = node
        for _ in range(m):
            s = frag(child, s)
        if n is None:
            a, e = new(), new()
            eps[s].append(a)
            eps[frag(child, a)].append(a)
            eps[a].append(e)
            return e
        e = new()
        for _ in range(n - m):
            eps[s].append(e)
            s = frag(child, s)
        eps[s].append(e)
        return e

    accept = frag(tree, 0)
    sig = {}
    for i, atom in enumerate(atoms):
        for lab in atom:
            sig[lab] = sig.get(lab, 0) | (1 << i)
    by_sig = {}
    for lab, v in sig.items():
        by_sig.setdefault(v, []).append(lab)
    classes = [np.array(sorted(v), np.int32) for v in by_sig.values()]
    classes.sort(key=lambda c: int(c[0]))
    atom_classes = [[k for k, c in enumerate(classes) if int(c[0]) in atom] for atom in atoms]

    def closure(states):
        seen, stack = set(states), list(states)
        while stack:
            for v in eps[stack.pop()]:
                if v not in seen:
                    seen.add(v)
                    stack.append(v)
        return frozenset(seen)

    # subset construction over the classes
    start = closure([0])
    index, order, delta = {start: 0}, [start], []
    q = 0
    while q < len(order):
        move = {}
        for v in order[q]:
            for ai, dst in tr[v]:
                for k in atom_classes[ai]:
                    move.setdefault(k, set()).add(dst)
        row = {}
        for k, dsts in move.items():
            tgt = closure(dsts)
            if tgt not in index:
                index[tgt] = len(order)
                order.append(tgt)
                if len(order) > 50000:
                    raise ValueError("the pattern is too large (more than 50000 DFA states before minimisation)")
            row[k] = index[tgt]
        delta.append(row)
        q += 1
    nq = len(order)
    final = [accept in s for s in order]
    # trim: the states that can reach a final state
    back = [[] for _ in range(nq)]
    for s, row in enumerate(delta):
        for d in row.values():
            back[d].append(s)
    alive, stack = set(s for s in range(nq) if final[s]), [s for s in range(nq) if final[s]]
    while stack:
        for p in back[stack.pop()]:
            if p not in alive:
                alive.add(p)
                stack.append(p)
    if 0 not in alive:
        return (np.zeros((0, 3), np.int32), [], [], 1) if sets else (np.zeros((0, 3), np.int32), [], 1)
    # Moore's refinement on the trimmed (partial) automaton: a missing arc leads to the dead block -1
    block = {s: (1 if final[s] else 0) for s in alive}
    nk = len(classes)
    while True:
        keys = {}
        new_block = {}
        for s in sorted(alive):
            row = delta[s]
            key = (block[s],) + tuple(block[row[k]] if k in row and row[k] in alive else -1 for k in range(nk))
            new_block[s] = keys.setdefault(key, len(keys))
        stable = len(keys) == len(set(block.values()))
        block = new_block
        if stable:
            break
    rep = {}
    for s in sorted(alive):
        rep.setdefault(block[s], s)
    # breadth-first numbering over labels ascending (the classes are sorted by their smallest label, and every label of
    # a class leads to the same state, so the first label that reaches a state is its class's smallest)
    number, queue = {block[0]: 0}, [block[0]]
    rows = []
    for blk in queue:
        row = delta[rep[blk]]
        out = sorted((int(classes[k][0]), k, block[d]) for k, d in row.items() if d in alive)
        for _, _, d in out:
            if d not in number:
                number[d] = len(number)
                queue.append(d)
        rows.append([(k, d) for _, k, d in out])
    finals = sorted(number[b] for b in number if final[rep[b]])
    if sets:
        arcs = np.array([(number[blk], k, number[d]) for blk, row in zip(queue, rows) for k, d in row], np.int32)
        return np.ascontiguousarray(arcs.reshape(-1, 3)), classes, finals, len(number)
    arcs = []
    for blk, row in zip(queue, rows):
        for k, d in row:
            a = np.empty((len(classes[k]), 3), np.int32)
            a[:, 0], a[:, 1], a[:, 2] = number[blk], classes[k], number[d]
            arcs.append(a)
    arcs = np.concatenate(arcs) if arcs else np.zeros((0, 3), np.int32)
    arcs = arcs[np.lexsort((arcs[:, 1], arcs[:, 0]))]
    return np.ascontiguousarray(arcs), finals, len(number)


_PAT_MAX_EDGES = 262144                                    # HCTR_PAT_MAX_EDGES


def _expand_arcs(arcs, sets):
    """the single-label arcs of set arcs: int32 [n, 3] rows (src, label, dst) sorted by (src, label)"""
    out = []
    for p, k, q in np.asarray(arcs).reshape(-1, 3):
        a = np.empty((len(sets[k]), 3), np.int32)
        a[:, 0], a[:, 1], a[:, 2] = p, sets[k], q
        out.append(a)
    out = np.concatenate(out) if out else np.zeros((0, 3), np.int32)
    return np.ascontiguousarray(out[np.lexsort((out[:, 1], out[:, 0]))])


class Pattern(object):
    """A pattern for pattern-constrained recognition (include/hctr_hip.h ``hctr_pat_build``): a deterministic finite
    automaton over labels, lifted to CTC on the host (no GPU needed). ``arcs``: (src, label, dst) triples with labels in
    [1, C-1] and at most one arc per (src, label); ``finals``: the final states; state 0 is the start; ``num_classes`` =
    C. ``Pattern.compile(expr, codec)`` builds one from a regular expression. The object is immutable and serves any
    number of contexts. ``Pattern.from_sets`` builds the set form (``hctr_pat_build_sets``): arcs that carry label sets,
    the same language and results without the explicit edge list - what a wildcard over a large vocabulary needs.
    ``kind`` is 0 for the explicit form, 1 for the set form, 2 for the weighted form. ``weights`` (one float per arc)
    and ``final_weights`` (one per entry of ``finals``) build the weighted form (``hctr_pat_build_weighted``; either
    may be None = zeros): a text's weight is the sum of its arcs' weights plus its final state's, ``logp`` becomes
    log sum p(text | line) * exp(w(text)) and the best reading maximises path log-probability + w(text). Weights are
    finite; an arc that cannot be taken is left out. ``Pattern.compile(..., label_weights=)`` and ``Pattern.bigram``
    build such patterns."""

    def __init__(self, arcs, finals, num_states, num_classes, expr=None, sets=None, weights=None, final_weights=None):
        if sets is not None:
            if weights is not None or final_weights is not None:
                raise ValueError("the set form carries no weights: build the explicit form (sets=None)")
            self._init_sets(arcs, sets, finals, num_states, num_classes, expr)
            return
        self.sets = None
        a = np.asarray(arcs, dtype=np.int64).reshape(-1, 3)
        f = np.asarray(finals, dtype=np.int64).reshape(-1)
        for v in (a, f):
            if v.size and (v.min() < np.iinfo(np.int32).min or v.max() > np.iinfo(np.int32).max):
                raise ValueError("arc or state out of the int32 range")
        src, lab, dst = (np.ascontiguousarray(a[:, k], dtype=np.int32) for k in range(3))
        f = np.ascontiguousarray(f, dtype=np.int32)
        self.expr = expr
        self.arcs, self.finals, self.num_states = np.stack([src, lab, dst], axis=1), f, int(num_states)      # as given
        self.num_classes = int(num_classes)
        lib = _lib.load()
        h = ctypes.c_void_p()
        self.weights_given = self.final_weights_given = None
        if weights is None and final_weights is None:
            rc = lib.hctr_pat_build(_lib.ptr(src), _lib.ptr(lab), _lib.ptr(dst), int(a.shape[0]), _lib.ptr(f), int(f.size),
                                    int(num_states), self.num_classes, ctypes.byref(h))
        else:
            w = fw = None
            if weights is not None:
                w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
                if w.size != a.shape[0]:
                    raise ValueError("%d weights for %d arcs" % (w.size, a.shape[0]))
            if final_weights is not None:
                fw = np.ascontiguousarray(np.asarray(final_weights, dtype=np.float32).reshape(-1))
                if fw.size != f.size:
                    raise ValueError("%d final weights for %d final states" % (fw.size, f.size))
            self.weights_given, self.final_weights_given = w, fw
            rc = lib.hctr_pat_build_weighted(_lib.ptr(src), _lib.ptr(lab), _lib.ptr(dst), _lib.ptr(w), int(a.shape[0]),
                                             _lib.ptr(f), _lib.ptr(fw), int(f.size), int(num_states), self.num_classes,
                                             ctypes.byref(h))
        self._h = h if rc == 0 else None
        _lib.check(rc, None)

    def _init_sets(self, arcs, sets, finals, num_states, num_classes, expr):
        a = np.asarray(arcs, dtype=np.int64).reshape(-1, 3)
        f = np.asarray(finals, dtype=np.int64).reshape(-1)
        sets = [np.asarray(v, dtype=np.int64).reshape(-1) for v in sets]
        for v in [a, f] + sets:
            if v.size and (v.min() < np.iinfo(np.int32).min or v.max() > np.iinfo(np.int32).max):
                raise ValueError("arc, state or label out of the int32 range")
        src, st, dst = (np.ascontiguousarray(a[:, k], dtype=np.int32) for k in range(3))
        f = np.ascontiguousarray(f, dtype=np.int32)
        ptr = np.concatenate([[0], np.cumsum([len(v) for v in sets])]).astype(np.int32)
        lab = np.ascontiguousarray(np.concatenate(sets) if sets else np.zeros(0), dtype=np.int32)
        self.expr = expr
        self.arcs, self.finals, self.num_states = np.stack([src, st, dst], axis=1), f, int(num_states)      # as given
        self.sets = [v.astype(np.int32) for v in sets]
        self.num_classes = int(num_classes)
        lib = _lib.load()
        h = ctypes.c_void_p()
        rc = lib.hctr_pat_build_sets(_lib.ptr(src), _lib.ptr(st), _lib.ptr(dst), int(a.shape[0]), _lib.ptr(ptr), _lib.ptr(lab),
                                     len(sets), _lib.ptr(f), int(f.size), int(num_states), self.num_classes, ctypes.byref(h))
        self._h = h if rc == 0 else None
        _lib.check(rc, None)

    @classmethod
    def from_sets(cls, arcs, sets, finals, num_states, num_classes, expr=None):
        """The set form: ``arcs`` (src, set, dst) triples, ``sets`` the list of label sets they index - each ascending,
        non-empty, within [1, C-1]; the sets of the arcs that leave one state are pairwise disjoint."""
        return cls(arcs, finals, num_states, num_classes, expr=expr, sets=list(sets))

    @classmethod
    def compile(cls, expr, codec, sets=None, label_weights=None):
        """The pattern of the regular expression ``expr`` over ``codec``'s vocabulary; the whole line must match
        (``re.fullmatch``). The syntax is ``_Regex``'s subset of ``re``. ``.``, negated sets and ranges mean the codec's
        real characters (labels 1..C-2): <unknown> is never matched; a literal outside the vocabulary is a ValueError.
        ``sets=False``: the explicit form; ``True``: the set form, from the expression's alphabet classes; ``None``: the
        explicit form whenever it builds, the set form where the explicit build is refused for a limit.
        ``label_weights``: a scalar (a bonus per character), a dict character -> weight (0 for the others) or an array
        [C]; every arc on label c weighs ``label_weights[c]``, so a text's weight is the sum over its characters whatever
        automaton the expression gave. Always the explicit (weighted) form: ``sets=True`` is a ValueError, and so is a
        pattern that only the set form could hold, with the builder's message."""
        chars = codec.characters
        vocab = {ch: i for i, ch in enumerate(chars) if 1 <= i <= len(chars) - 2 and len(ch) == 1}
        if label_weights is not None:
            if sets:
                raise ValueError("label_weights need the explicit form: the set form (sets=True) carries no weights")
            if isinstance(label_weights, dict):
                lw = np.zeros(len(chars), np.float32)
                for ch, v in label_weights.items():
                    if ch not in vocab:
                        raise ValueError("label_weights names %r, which is not a character of the codec" % (ch,))
                    lw[vocab[ch]] = v
            elif np.ndim(label_weights) == 0:
                lw = np.full(len(chars), label_weights, np.float32)
            else:
                lw = np.asarray(label_weights, dtype=np.float32).reshape(-1)
                if lw.size != len(chars):
                    raise ValueError("label_weights has %d entries, the codec %d classes" % (lw.size, len(chars)))
            arcs, classes, finals, nq = _regex_to_dfa(_Regex(expr, vocab).parse(), sets=True)
            if sum(len(classes[k]) for k in arcs[:, 1]) > 4 * _PAT_MAX_EDGES:
                raise ValueError("hctr_pat_build_weighted: the pattern has more than %d edges (HCTR_PAT_MAX_EDGES): only the "
                                 "set form, which carries no weights, could hold it" % _PAT_MAX_EDGES)
            full = _expand_arcs(arcs, classes)
            return cls(full, finals, nq, len(chars), expr=expr, weights=lw[full[:, 1]])
        arcs, classes, finals, nq = _regex_to_dfa(_Regex(expr, vocab).parse(), sets=True)
        if sets:
            return cls.from_sets(arcs, classes, finals, nq, len(chars), expr=expr)
        # the explicit form's limits, decided before the arcs are expanded (a refused build may have 10^8 of them)
        expanded = sum(len(classes[k]) for k in arcs[:, 1])
        if sets is None and expanded > 4 * _PAT_MAX_EDGES:
            return cls.from_sets(arcs, classes, finals, nq, len(chars), expr=expr)
        try:
            return cls(_expand_arcs(arcs, classes), finals, nq, len(chars), expr=expr)
        except ValueError as exc:
            if sets is None and ("HCTR_PAT_MAX_STATES" in str(exc) or "HCTR_PAT_MAX_EDGES" in str(exc)):
                return cls.from_sets(arcs, classes, finals, nq, len(chars), expr=expr)
            raise

    @classmethod
    def bigram(cls, labels, trans, init=None, final=None, num_classes=None):
        """The weighted pattern of a label bigram over the n distinct ``labels``: every non-empty text over them, weighted
        ``init[i]`` for its first label ``labels[i]``, ``trans[j][i]`` for ``labels[i]`` after ``labels[j]`` and
        ``final[i]`` for ending on ``labels[i]`` (None = zeros). State 0 is the start, state i + 1 "the last label was
        labels[i]". A -inf entry of ``trans`` or ``init`` leaves the arc out. Dense, it has 2n + 1 CTC states and
        2n^2 + 3n + 1 edges: n <= 361 fits HCTR_PAT_MAX_EDGES."""
        lab = np.asarray(labels, dtype=np.int64).reshape(-1)
        n = int(lab.size)
        if num_classes is None:
            raise ValueError("num_classes is required")
        if n < 1 or len(set(lab.tolist())) != n:
            raise ValueError("labels must be n >= 1 distinct labels")
        tr = np.asarray(trans, dtype=np.float32)
        if tr.shape != (n, n):
            raise ValueError("trans must be [n, n] = [%d, %d], got %s" % (n, n, tr.shape))
        ini = np.zeros(n, np.float32) if init is None else np.asarray(init, dtype=np.float32).reshape(-1)
        fin = np.zeros(n, np.float32) if final is None else np.asarray(final, dtype=np.float32).reshape(-1)
        if ini.size != n or fin.size != n:
            raise ValueError("init and final must have n = %d entries" % n)
        w = np.concatenate([ini[None, :], tr], axis=0)                  # [n + 1, n]: row = source state, column = label
        src, col = np.nonzero(~np.isneginf(w))
        arcs = np.stack([src, lab[col], col + 1], axis=1)
        return cls(arcs, np.arange(1, n + 1), n + 1, int(num_classes), weights=w[src, col], final_weights=fin)

    @property
    def kind(self):
        """0 = the explicit form, 1 = the set form, 2 = the weighted form (``hctr_pat_kind``)"""
        return int(_lib.load().hctr_pat_kind(self._h))

    @property
    def weighted(self):
        return self.kind == 2

    def instance(self, full=True):
        """(states per thread, edge list in LDS, edge weights in LDS): the kernel instance a call with (``full``) or
        without the Viterbi outputs runs for this explicit or weighted pattern (``hctr_pattern_instance``, a pure
        function of the pattern's sizes)"""
        if self.kind == 1:
            raise ValueError("the set form has one kernel shape: no instance to select")
        i = self.info()
        v = int(_lib.load().hctr_pattern_instance(i["states"], i["edges"], int(bool(full)), int(self.kind == 2)))
        return v & 15, bool(v & 16), bool(v & 32)

    def weights(self):
        """dict of float32 arrays: what ``hctr_pat_weights`` exports, the weights the kernel is given beside ``tables()`` -
        in_w [E] parallel to in_src, accept_w parallel to accept, start_w parallel to start"""
        lib, i = _lib.load(), self.info()
        if self.kind != 2:
            _lib.check(lib.hctr_pat_weights(self._h, None, None, None), None)
        t = self.tables()
        w = {"in_w": np.zeros(i["edges"], np.float32), "accept_w": np.zeros(t["accept"].size, np.float32),
             "start_w": np.zeros(t["start"].size, np.float32)}
        _lib.check(lib.hctr_pat_weights(self._h, _lib.ptr(w["in_w"]), _lib.ptr(w["accept_w"]), _lib.ptr(w["start_w"])), None)
        return w

    def text_weight(self, labels):
        """float: the weight of the text ``labels`` (``hctr_pat_text_weight``): the float64 sum of its arcs' float32
        weights and its final state's; -inf for a text outside the pattern's language"""
        lab = np.ascontiguousarray(np.asarray(labels, dtype=np.int32).reshape(-1))
        w = ctypes.c_double()
        _lib.check(_lib.load().hctr_pat_text_weight(self._h, _lib.ptr(lab), int(lab.size), ctypes.byref(w)), None)
        return float(w.value)

    def expanded_arcs(self):
        """int32 [n, 3]: the single-label arcs (src, label, dst) of the same automaton, sorted by (src, label) - the set
        arcs expanded (for tests on small vocabularies), the arcs as given for the explicit form"""
        if self.sets is None:
            return self.arcs
        return _expand_arcs(self.arcs, self.sets)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.load().hctr_pat_free(self._h)
                self._h = None
        except Exception:
            pass

    def info(self):
        """dict: dfa_states (after pruning), states (the CTC states), edges, classes (distinct), max_in_degree. For the
        set form ``edges`` counts the reduced in-arcs (one per eps state and source DFA state) and ``max_in_degree`` the
        most of them one state has."""
        v = [ctypes.c_int32() for _ in range(5)]
        _lib.check(_lib.load().hctr_pat_info(self._h, *[ctypes.byref(x) for x in v]), None)
        return dict(zip(("dfa_states", "states", "edges", "classes", "max_in_degree"), (int(x.value) for x in v)))

    def tables(self):
        """dict of numpy arrays: what ``hctr_pat_tables`` exports, the tables the kernel is given - state_label,
        state_slot [S], in_ptr [S + 1], in_src uint16 [E], classes, accept, start."""
        lib, i = _lib.load(), self.info()
        na, ns = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(lib.hctr_pat_tables(self._h, None, None, None, None, None, ctypes.byref(na), None, ctypes.byref(ns), None),
                   None)
        t = {"state_label": np.zeros(i["states"], np.int32), "state_slot": np.zeros(i["states"], np.int32),
             "in_ptr": np.zeros(i["states"] + 1, np.int32), "in_src": np.zeros(i["edges"], np.uint16),
             "classes": np.zeros(i["classes"], np.int32), "accept": np.zeros(int(na.value), np.int32),
             "start": np.zeros(int(ns.value), np.int32)}
        _lib.check(lib.hctr_pat_tables(self._h, _lib.ptr(t["state_label"]), _lib.ptr(t["state_slot"]), _lib.ptr(t["in_ptr"]),
                                       _lib.ptr(t["in_src"]), _lib.ptr(t["classes"]), None, _lib.ptr(t["accept"]), None,
                                       _lib.ptr(t["start"])), None)
        return t


class PatternResult(object):
    """Result of pattern-constrained recognition of B lines of W steps (numpy arrays, on the host; include/hctr_hip.h
    ``hctr_pattern``): ``logp`` float32 [B], the log of the probability that the line's text matches the pattern;
    ``best_logp`` float32 [B], the best matching path's log-probability; ``path`` int32 [B, W], its class per column (-1
    beyond the line's length); ``labels`` int32 [B, W] / ``lengths`` int32 [B], the decoded text; ``starts`` / ``ends``
    int32 [B, W] and ``logps`` float32 [B, W], each character's column span and the sum of its label's log-probabilities
    over it; ``text_nll`` float32 [B], the CTC loss of the decoded text. A forward-only result holds ``logp`` alone (the
    rest None). Where no path of the line's length matches, logp and best_logp are -inf, lengths 0, text_nll +inf.
    ``weights`` float64 [B]: the decoded texts' weights under a weighted pattern (``Pattern.text_weight``; NaN where no
    path was accepted), zeros for an unweighted one; no field of the device call."""

    FIELDS = ("logp", "best_logp", "path", "labels", "lengths", "starts", "ends", "logps", "text_nll")

    def __init__(self, logp, best_logp=None, path=None, labels=None, lengths=None, starts=None, ends=None, logps=None,
                 text_nll=None, weights=None):
        self.logp, self.best_logp, self.path, self.labels, self.lengths = logp, best_logp, path, labels, lengths
        self.starts, self.ends, self.logps, self.text_nll = starts, ends, logps, text_nll
        self.weights = weights

    def __len__(self):
        return len(self.logp)

    def label_lists(self):
        return [self.labels[b, :int(self.lengths[b])].copy() for b in range(len(self))]

    def texts(self, codec):
        """the decoded text of every line ('' where nothing matches)"""
        return codec.labels_to_text([l.tolist() for l in self.label_lists()])

    def posterior(self):
        """float64 [B]: exp(-text_nll + weight - logp), the probability of the decoded text within the pattern, under its
        weights where it has any (0 where nothing matches)"""
        w = np.zeros(len(self)) if self.weights is None else np.where(np.isnan(self.weights), 0.0, self.weights)
        with np.errstate(invalid="ignore", over="ignore"):
            p = np.exp(-np.asarray(self.text_nll, np.float64) + w - np.asarray(self.logp, np.float64))
        return np.where(np.isneginf(self.logp), 0.0, p)

    def lines(self):
        """yields per line the list of (label, start, end, confidence), one per character: its column span [start, end)
        and the geometric mean of its probability over the span, exp(logp / (end - start))"""
        for b in range(len(self)):
            yield [(int(self.labels[b, j]), int(self.starts[b, j]), int(self.ends[b, j]),
                    float(np.exp(np.float64(self.logps[b, j]) / (int(self.ends[b, j]) - int(self.starts[b, j])))))
                   for j in range(int(self.lengths[b]))]


def _pattern_outputs(pat, B, W, full):
    if not isinstance(pat, Pattern):
        raise ValueError("pat must be a ctc.Pattern")
    i, f = np.int32, np.float32
    logp = np.full(B, -np.inf, f)
    if not full:
        return (logp,) + (None,) * 8
    return (logp, np.full(B, -np.inf, f), np.full((B, W), -1, i), np.zeros((B, W), i), np.zeros(B, i), np.zeros((B, W), i),
            np.zeros((B, W), i), np.zeros((B, W), f), np.full(B, np.inf, f))


def _pattern_result(pat, out):
    """the PatternResult of a call's outputs, with the decoded texts' weights (host side)"""
    res = PatternResult(*out)
    if res.lengths is None:
        return res
    res.weights = np.zeros(len(res), np.float64)
    if pat.kind == 2:
        for b in range(len(res)):
            res.weights[b] = (pat.text_weight(res.labels[b, :int(res.lengths[b])]) if np.isfinite(res.best_logp[b])
                              else np.nan)
    return res


def pattern_logits(ctx, logits, on_dev, pat, input_lengths=None, full=True):
    """PatternResult of caller logits / log-probs in WBC layout (hctr_pattern_logits); ``full=False`` asks for logp
    alone (the forward-only call)"""
    if len(logits.shape) != 3:
        raise ValueError("logits must be [W,B,C]")
    W, B, C = (int(v) for v in logits.shape)
    il = normalize_input_lengths(input_lengths, B)
    out = _pattern_outputs(pat, B, W, full)
    if B and W:
        _lib.check(_lib.load().hctr_pattern_logits(ctx, pat._h, _lib.ptr(logits), on_dev, W, B, C, _lib.ptr(il),
                                                   *[_lib.ptr(a) for a in out]), ctx)
    return _pattern_result(pat, out)


def pattern_images(ctx, x, dt, on_dev, widths, B, W, pat, input_lengths=None, full=True):
    """PatternResult of line images (hctr_pattern); x, dt, on_dev, widths as hctr_model._img_args / _widths give them."""
    il = normalize_input_lengths(input_lengths, B)
    out = _pattern_outputs(pat, B, W, full)
    if B:
        _lib.check(_lib.load().hctr_pattern(ctx, pat._h, _lib.ptr(x), dt, on_dev, _lib.ptr(widths), B, W, _lib.ptr(il),
                                            *[_lib.ptr(a) for a in out]), ctx)
    return _pattern_result(pat, out)


def pattern_group_lines(S, D, W):
    """lines one group holds for a pattern of S CTC states and D emission slots on W columns (hctr_pattern_group_lines)"""
    return int(_lib.load().hctr_pattern_group_lines(int(S), int(D), int(W)))


class Recognition(object):
    """Result of a greedy recognition of B lines of W steps (numpy arrays, on the host; include/hctr_hip.h
    ``hctr_recognize``): ``labels`` int32 [B, W] and ``lengths`` int32 [B], the decoded text as the greedy decode gives it
    (a line's first ``lengths[b]`` entries are valid, in every per-character array); ``starts`` / ``ends`` int32 [B, W],
    each character's pixel-column span; ``logps`` float32 [B, W], the sum of its label's log-probabilities over the span;
    ``alt_labels`` int32 / ``alt_logps`` float32 [B, W], the runner-up class at the span's peak column and its
    log-probability there; ``path_logp`` float32 [B], the greedy path's log-probability; ``text_nll`` float32 [B], the
    CTC loss of the decoded text (NaN for a text of more than 2047 labels)."""

    def __init__(self, labels, lengths, starts, ends, logps, alt_labels, alt_logps, path_logp, text_nll):
        self.labels, self.lengths = labels, lengths
        self.starts, self.ends, self.logps = starts, ends, logps
        self.alt_labels, self.alt_logps = alt_labels, alt_logps
        self.path_logp, self.text_nll = path_logp, text_nll

    def __len__(self):
        return len(self.lengths)

    @property
    def text_posterior(self):
        """float64 [B]: exp(-text_nll), the probability of the decoded text summed over all its alignments."""
        return np.exp(-np.asarray(self.text_nll, dtype=np.float64))

    def label_lists(self):
        return [self.labels[b, :int(self.lengths[b])].copy() for b in range(len(self))]

    def lines(self):
        """yields per line the list of (label, start, end, confidence, alt_label, alt_prob), one per character: its
        pixel-column span [start, end), the geometric mean of its probability over the span, exp(logp / (end - start)),
        and the likeliest substitution with its probability at the span's most confident column."""
        for b in range(len(self)):
            out = []
            for j in range(int(self.lengths[b])):
                st, en = int(self.starts[b, j]), int(self.ends[b, j])
                conf = float(np.exp(np.float64(self.logps[b, j]) / (en - st)))
                out.append((int(self.labels[b, j]), st, en, conf, int(self.alt_labels[b, j]),
                            float(np.exp(np.float64(self.alt_logps[b, j])))))
            yield out


def _recognize_outputs(B, W):
    """the output arrays in the order of the C ABI's arguments (and of Recognition's); zeros past a line's length"""
    i, f = np.int32, np.float32
    return tuple(np.zeros(shape, dt) for shape, dt in (((B, W), i), ((B,), i), ((B, W), i), ((B, W), i), ((B, W), f),
                                                       ((B, W), i), ((B, W), f), ((B,), f), ((B,), f)))


def recognize_logits(ctx, logits, on_dev):
    """Recognition of caller logits / log-probs in WBC layout (hctr_recognize_logits)."""
    if len(logits.shape) != 3:
        raise ValueError("logits must be [W,B,C]")
    W, B, C = (int(v) for v in logits.shape)
    if C < 2:
        raise ValueError("logits need at least 2 classes, got %d" % C)
    if B and W < 1:
        raise ValueError("logits have no steps (W = 0)")
    out = _recognize_outputs(B, W)
    if B:
        _lib.check(_lib.load().hctr_recognize_logits(ctx, _lib.ptr(logits), on_dev, W, B, C, *[_lib.ptr(a) for a in out]),
                   ctx)
    return Recognition(*out)


def recognize_images(ctx, x, dt, on_dev, widths, B, W):
    """Recognition of line images (hctr_recognize); x, dt, on_dev, widths as hctr_model._img_args / _widths give them."""
    out = _recognize_outputs(B, W)
    if B:
        _lib.check(_lib.load().hctr_recognize(ctx, _lib.ptr(x), dt, on_dev, _lib.ptr(widths), B, W,
                                              *[_lib.ptr(a) for a in out]), ctx)
    return Recognition(*out)


class Evaluation(object):
    """Result of scoring B decoded lines against their transcriptions (numpy arrays, on the host; include/hctr_hip.h
    ``hctr_edit_distance``): ``edits`` int32 [B], the Levenshtein distance of each line; ``counts`` int32 [B, 4] =
    (hits, substitutions, deletions, insertions); ``ref_map`` int32 [sum L], per reference character the position in
    the line's hypothesis it is aligned with (-1: deleted); ``hyp_map`` int32 [B, stride], per decoded character the
    position in the line's reference (-1: inserted; zeros past a line's length); ``labels`` int32 [B, stride] /
    ``lengths`` int32 [B], the hypotheses; ``targets`` int32 [sum L] / ``target_lengths`` int32 [B], the references;
    ``offsets`` int64 [B + 1], where each line's reference begins. ``counts``, ``ref_map`` and ``hyp_map`` are None
    after a distance-only call (``maps=False``); ``labels`` may be None when only the distances were asked for."""

    def __init__(self, edits, counts, ref_map, hyp_map, labels, lengths, targets, target_lengths):
        self.edits, self.counts, self.ref_map, self.hyp_map = edits, counts, ref_map, hyp_map
        self.labels, self.lengths = labels, lengths
        self.targets = targets
        self.target_lengths = np.asarray(target_lengths, np.int32)
        self.offsets = np.concatenate([[0], np.cumsum(self.target_lengths.astype(np.int64))]).astype(np.int64)

    def __len__(self):
        return len(self.edits)

    def _need_counts(self):
        if self.counts is None:
            raise ValueError("a distance-only Evaluation (maps=False) has no counts or maps")

    @property
    def total_edits(self):
        return int(np.asarray(self.edits, np.int64).sum())

    @property
    def total_chars(self):
        return int(self.offsets[-1])

    @property
    def totals(self):
        """(hits, substitutions, deletions, insertions) over all lines"""
        self._need_counts()
        return tuple(int(v) for v in np.asarray(self.counts, np.int64).reshape(-1, 4).sum(axis=0))

    @property
    def cer(self):
        """sum(edits) / sum(L): the reference's CER (test.py:285); NaN without a reference character"""
        n = self.total_chars
        return self.total_edits / n if n else float("nan")

    @property
    def cr(self):
        """correct rate (N - D - S) / N"""
        _, s, d, _ = self.totals
        n = self.total_chars
        return (n - d - s) / n if n else float("nan")

    @property
    def ar(self):
        """accurate rate (N - D - S - I) / N = 1 - cer"""
        _, s, d, i = self.totals
        n = self.total_chars
        return (n - d - s - i) / n if n else float("nan")

    def lines(self):
        """yields per line the list of (ref_symbol, hyp_symbol, ref_pos, hyp_pos) along the alignment, in reading order:
        a hit or a substitution has both, a deletion (ref_symbol, None, i, -1), an insertion (None, hyp_symbol, -1, j).
        Between two aligned pairs the insertions come first, then the deletions."""
        self._need_counts()
        for b in range(len(self)):
            o, L, H = int(self.offsets[b]), int(self.target_lengths[b]), int(self.lengths[b])
            out, i = [], 0
            for j in range(H):
                at = int(self.hyp_map[b, j])
                if at < 0:
                    out.append((None, int(self.labels[b, j]), -1, j))
                    continue
                for k in range(i, at):
                    out.append((int(self.targets[o + k]), None, k, -1))
                out.append((int(self.targets[o + at]), int(self.labels[b, j]), at, j))
                i = at + 1
            for k in range(i, L):
                out.append((int(self.targets[o + k]), None, k, -1))
            yield out

    def confusions(self):
        """{(ref_symbol, hyp_symbol): count} of the substitutions, built on the host from the maps"""
        self._need_counts()
        out = {}
        for b in range(len(self)):
            o, L = int(self.offsets[b]), int(self.target_lengths[b])
            rm = np.asarray(self.ref_map[o:o + L])
            pos = np.flatnonzero(rm >= 0)
            r, h = np.asarray(self.targets[o:o + L])[pos], np.asarray(self.labels[b])[rm[pos]]
            for x, y in zip(r[r != h].tolist(), h[r != h].tolist()):
                out[(x, y)] = out.get((x, y), 0) + 1
        return out


def _edit_outputs(B, stride, total, maps):
    """edits, counts, ref_map, hyp_map in the order of the C ABI's arguments (None: the distance-only call)"""
    if not maps:
        return np.zeros((B,), np.int32), None, None, None
    return (np.zeros((B,), np.int32), np.zeros((B, 4), np.int32), np.zeros((total,), np.int32),
            np.zeros((B, stride), np.int32))


def edit_distance_labels(ctx, labels, lengths, targets, target_lengths, maps=True):
    """Evaluation of hypotheses ``labels`` int32 [B, stride] / ``lengths`` [B] against concatenated ``targets`` /
    ``target_lengths`` [B] (hctr_edit_distance); the symbols are arbitrary int32 values."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    lengths = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
    B = int(lengths.size)
    if labels.ndim != 2 or labels.shape[0] != B:
        raise ValueError("labels must be [B, stride] with one row per length")
    tg, tl = normalize_targets(targets, target_lengths, B)
    out = _edit_outputs(B, int(labels.shape[1]), int(tg.size), maps)
    if B:
        _lib.check(_lib.load().hctr_edit_distance(ctx, _lib.ptr(labels), _lib.ptr(lengths), int(labels.shape[1]),
                                                  _lib.ptr(tg), _lib.ptr(tl), B, *[_lib.ptr(a) for a in out]), ctx)
    return Evaluation(*out, labels, lengths, tg, tl)


def pad_sequences(seqs):
    """(int32 [B, stride], int32 [B]) from a list of strings (their code points) or of int sequences"""
    rows = [np.fromiter((ord(ch) for ch in s), np.int64, len(s)) if isinstance(s, str)
            else np.asarray(s, dtype=np.int64).reshape(-1) for s in seqs]
    n = np.array([r.size for r in rows], np.int32)
    out = np.zeros((len(rows), max(1, int(n.max()) if len(rows) else 1)), np.int32)
    for b, r in enumerate(rows):
        out[b, :r.size] = r
    return out, n


def edit_distance_sequences(ctx, hyps, refs, maps=True):
    """Evaluation of two equally long lists of strings or int sequences, line by line (hctr_edit_distance). Strings
    are compared by code point, which is ``editdistance.eval`` on the strings, exactly."""
    if len(hyps) != len(refs):
        raise ValueError("%d hypotheses but %d references" % (len(hyps), len(refs)))
    lab, n = pad_sequences(hyps)
    ref, tl = pad_sequences(refs)
    tg = np.concatenate([ref[b, :tl[b]] for b in range(len(refs))] + [np.zeros((0,), np.int32)]).astype(np.int32)
    return edit_distance_labels(ctx, lab, n, tg, tl, maps)


def evaluate_logits(ctx, logits, on_dev, targets, target_lengths, maps=True):
    """Evaluation of the greedy decode of caller logits / log-probs in WBC layout (hctr_evaluate_logits)."""
    W, B, C = (int(v) for v in logits.shape)
    tg, tl = normalize_targets(targets, target_lengths, B)
    labels, lengths = np.zeros((B, W), np.int32), np.zeros((B,), np.int32)
    out = _edit_outputs(B, W, int(tg.size), maps)
    if B:
        _lib.check(_lib.load().hctr_evaluate_logits(ctx, _lib.ptr(logits), on_dev, W, B, C, _lib.ptr(tg), _lib.ptr(tl),
                                                    _lib.ptr(labels), _lib.ptr(lengths), *[_lib.ptr(a) for a in out]),
                   ctx)
    return Evaluation(*out, labels, lengths, tg, tl)


def evaluate_images(ctx, x, dt, on_dev, widths, B, W, targets, target_lengths, maps=True):
    """Evaluation of line images (hctr_evaluate); x, dt, on_dev, widths as hctr_model._img_args / _widths give them."""
    tg, tl = normalize_targets(targets, target_lengths, B)
    labels, lengths = np.zeros((B, W), np.int32), np.zeros((B,), np.int32)
    out = _edit_outputs(B, W, int(tg.size), maps)
    if B:
        _lib.check(_lib.load().hctr_evaluate(ctx, _lib.ptr(x), dt, on_dev, _lib.ptr(widths), B, W, _lib.ptr(tg),
                                             _lib.ptr(tl), _lib.ptr(labels), _lib.ptr(lengths),
                                             *[_lib.ptr(a) for a in out]), ctx)
    return Evaluation(*out, labels, lengths, tg, tl)


class NBest(object):
    """Result of the device prefix beam search over B lines (numpy arrays, on the host; include/hctr_hip.h
    ``hctr_nbest*``): ``labels`` int32 [B, n, W] and ``lengths`` int32 [B, n], line b's hypotheses best first (the first
    ``lengths[b, i]`` entries of a hypothesis are valid, the rest zeros); ``logps`` float64 [B, n], the log-probability of
    each text over the alignments the pruned search kept; ``scores`` float64 [B, n], what the search ranked by
    (``logp + length * len_bonus``); ``counts`` int32 [B], how many hypotheses a line really has (unused slots have
    length 0 and -inf). ``lm_scores`` is None without a language model; with one (``hctr_nbest_lm*``) it is float64
    [B, n], the n-gram log10 score of each text, and ``scores`` is ``logp + lm_score * lm_panelty + length * len_bonus``.
    ``status`` and ``ranked`` are None except for the skip search (``hctr_nbest_skip*``): int32 [B], per line 0 ok / 1
    empty greedy text / 2 list emptied by a row without usable candidates / 3 a row beyond 32 candidates (not searched),
    and how many of the line's steps were ranked ones (the others updated the list in place). A skip search returns the
    final list as it stands: after trailing in-place steps it need not be sorted and may hold a text twice."""

    def __init__(self, labels, lengths, logps, scores, counts, lm_scores=None, status=None, ranked=None):
        self.labels, self.lengths, self.logps, self.scores, self.counts = labels, lengths, logps, scores, counts
        self.lm_scores, self.status, self.ranked = lm_scores, status, ranked

    def __len__(self):
        return len(self.counts)

    def label_lists(self):
        """per line the list of its hypotheses' label arrays, best first"""
        return [[self.labels[b, i, :int(self.lengths[b, i])].copy() for i in range(int(self.counts[b]))]
                for b in range(len(self))]

    def lines(self):
        """yields per line the list of (labels, logp, score), best first"""
        for b in range(len(self)):
            yield [(self.labels[b, i, :int(self.lengths[b, i])].copy(), float(self.logps[b, i]), float(self.scores[b, i]))
                   for i in range(int(self.counts[b]))]

    def posteriors(self):
        """float64 [B, n]: each hypothesis's share of the probability mass of its line's list, softmax of ``logps``
        over the hypotheses returned (0 for unused slots; a line without a hypothesis is all zeros)."""
        lp = np.asarray(self.logps, np.float64)
        out = np.zeros(lp.shape, np.float64)
        for b in range(len(self)):
            n = int(self.counts[b])
            row = lp[b, :n]
            if n and np.isfinite(row.max()):
                e = np.exp(row - row.max())
                out[b, :n] = e / e.sum()
        return out


def _nbest_args(B, W, n, beam, depth, len_bonus, input_lengths):
    n, beam, depth = int(n), int(beam), int(depth)
    il = normalize_input_lengths(input_lengths, B)
    out = (np.zeros((B, n, W), np.int32), np.zeros((B, n), np.int32), np.full((B, n), -np.inf, np.float64),
           np.full((B, n), -np.inf, np.float64), np.zeros((B,), np.int32))
    return n, beam, depth, ctypes.c_double(float(len_bonus)), il, out


def _lm_args(lm, lm_panelty, out):
    """the extra arguments of hctr_nbest_lm*: ``lm`` is an ``hctr_lm`` handle (``codec.ArpaLM.flat``)"""
    lm_scores = np.full(out[2].shape, -np.inf, np.float64)
    return lm, ctypes.c_double(float(lm_panelty)), lm_scores


def nbest_topk(ctx, topk_idx, topk_logp, C, n=5, beam=10, len_bonus=0.0, input_lengths=None, lm=None, lm_panelty=2.0):
    """NBest of front-end lists ``topk_idx`` int32 / ``topk_logp`` float32 [W, B, k] over ``C`` classes
    (hctr_nbest_topk): the search alone. With ``lm`` (an ``hctr_lm`` handle, ``codec.ArpaLM.flat``) the search is the
    n-gram-scored one over the reference's own end steps (hctr_nbest_lm_topk), ranking by
    ``logp + lm_score * lm_panelty + length * len_bonus``; ``lm_scores`` is then filled."""
    idx = np.ascontiguousarray(topk_idx, dtype=np.int32)
    lp = np.ascontiguousarray(topk_logp, dtype=np.float32)
    if idx.ndim != 3 or idx.shape != lp.shape:
        raise ValueError("topk_idx and topk_logp must both be [W,B,k]")
    W, B, k = (int(v) for v in idx.shape)
    n, beam, _, bonus, il, out = _nbest_args(B, W, n, beam, k, len_bonus, input_lengths)
    if lm is not None:
        lm, pen, lms = _lm_args(lm, lm_panelty, out)
        _lib.check(_lib.load().hctr_nbest_lm_topk(ctx, lm, _lib.ptr(idx), _lib.ptr(lp), W, B, int(C), k, beam, n, pen, bonus,
                                                  _lib.ptr(il), *[_lib.ptr(a) for a in out + (lms,)]), ctx)
        return NBest(*out, lm_scores=lms)
    _lib.check(_lib.load().hctr_nbest_topk(ctx, _lib.ptr(idx), _lib.ptr(lp), W, B, int(C), k, beam, n, bonus,
                                           _lib.ptr(il), *[_lib.ptr(a) for a in out]), ctx)
    return NBest(*out)


def nbest_logits(ctx, logits, on_dev, n=5, beam=10, depth=10, len_bonus=0.0, input_lengths=None, lm=None, lm_panelty=2.0):
    """NBest of caller logits / log-probs in WBC layout (hctr_nbest_logits): top-``depth`` per column, then the search;
    ``lm`` / ``lm_panelty`` as in ``nbest_topk`` (hctr_nbest_lm_logits)."""
    if len(logits.shape) != 3:
        raise ValueError("logits must be [W,B,C]")
    W, B, C = (int(v) for v in logits.shape)
    n, beam, depth, bonus, il, out = _nbest_args(B, W, n, beam, depth, len_bonus, input_lengths)
    if lm is not None:
        lm, pen, lms = _lm_args(lm, lm_panelty, out)
        _lib.check(_lib.load().hctr_nbest_lm_logits(ctx, lm, _lib.ptr(logits), on_dev, W, B, C, depth, beam, n, pen, bonus,
                                                    _lib.ptr(il), *[_lib.ptr(a) for a in out + (lms,)]), ctx)
        return NBest(*out, lm_scores=lms)
    _lib.check(_lib.load().hctr_nbest_logits(ctx, _lib.ptr(logits), on_dev, W, B, C, depth, beam, n, bonus,
                                             _lib.ptr(il), *[_lib.ptr(a) for a in out]), ctx)
    return NBest(*out)


def nbest_images(ctx, x, dt, on_dev, widths, B, W, n=5, beam=10, depth=10, len_bonus=0.0, input_lengths=None, lm=None,
                 lm_panelty=2.0):
    """NBest of line images (hctr_nbest); x, dt, on_dev, widths as hctr_model._img_args / _widths give them; ``lm`` /
    ``lm_panelty`` as in ``nbest_topk`` (hctr_nbest_lm)."""
    n, beam, depth, bonus, il, out = _nbest_args(B, W, n, beam, depth, len_bonus, input_lengths)
    if lm is not None:
        lm, pen, lms = _lm_args(lm, lm_panelty, out)
        _lib.check(_lib.load().hctr_nbest_lm(ctx, lm, _lib.ptr(x), dt, on_dev, _lib.ptr(widths), B, W, depth, beam, n, pen,
                                             bonus, _lib.ptr(il), *[_lib.ptr(a) for a in out + (lms,)]), ctx)
        return NBest(*out, lm_scores=lms)
    _lib.check(_lib.load().hctr_nbest(ctx, _lib.ptr(x), dt, on_dev, _lib.ptr(widths), B, W, depth, beam, n, bonus,
                                      _lib.ptr(il), *[_lib.ptr(a) for a in out]), ctx)
    return NBest(*out)


def _skip_args(lm, lm_panelty, out, B):
    lms = np.full(out[2].shape, -np.inf, np.float64)
    return lm, ctypes.c_double(float(lm_panelty)), out + (lms, np.zeros((B,), np.int32), np.zeros((B,), np.int32))


def _skip_result(out):
    return NBest(*out[:5], lm_scores=out[5], status=out[6], ranked=out[7])


def nbest_skip_lists(ctx, top1_idx, blank_logp, cand_off, cand_idx, cand_logp, C, n=5, beam=10, len_bonus=0.0,
                     input_lengths=None, lm=None, lm_panelty=2.0):
    """NBest by the reference's skip search on front-end lists (hctr_nbest_skip_lists): ``top1_idx`` int32 / ``blank_logp``
    float32 [W, B] and the CSR candidate lists ``cand_off`` int64 [W*B + 1], ``cand_idx`` int32, ``cand_logp`` float32
    (row t*B + b, classes ascending) as ``codec.beam_frontend_call(..., want_candidates=True)`` returns them. ``lm`` is an
    ``hctr_lm`` handle (``codec.ArpaLM.flat``) or None, the zero LM."""
    top1 = np.ascontiguousarray(top1_idx, dtype=np.int32)
    bl = np.ascontiguousarray(blank_logp, dtype=np.float32)
    if top1.ndim != 2 or top1.shape != bl.shape:
        raise ValueError("top1_idx and blank_logp must both be [W,B]")
    W, B = (int(v) for v in top1.shape)
    off = np.ascontiguousarray(cand_off, dtype=np.int64)
    if off.shape != (W * B + 1,):
        raise ValueError("cand_off must be [W*B + 1]")
    ci = np.ascontiguousarray(cand_idx, dtype=np.int32)
    cl = np.ascontiguousarray(cand_logp, dtype=np.float32)
    if ci.ndim != 1 or ci.shape != cl.shape or (off.size and ci.size < int(off.max())):
        raise ValueError("cand_idx and cand_logp must be flat and hold cand_off's last offset")
    n, beam, _, bonus, il, out = _nbest_args(B, W, n, beam, 1, len_bonus, input_lengths)
    lm, pen, out = _skip_args(lm, lm_panelty, out, B)
    _lib.check(_lib.load().hctr_nbest_skip_lists(ctx, lm, _lib.ptr(top1), _lib.ptr(bl), _lib.ptr(off), _lib.ptr(ci),
                                                 _lib.ptr(cl), W, B, int(C), beam, n, pen, bonus, _lib.ptr(il),
                                                 *[_lib.ptr(a) for a in out]), ctx)
    return _skip_result(out)


def nbest_skip_logits(ctx, logits, on_dev, n=5, beam=10, len_bonus=0.0, input_lengths=None, lm=None, lm_panelty=2.0):
    """NBest by the skip search of caller logits / log-probs in WBC layout (hctr_nbest_skip_logits)"""
    if len(logits.shape) != 3:
        raise ValueError("logits must be [W,B,C]")
    W, B, C = (int(v) for v in logits.shape)
    n, beam, _, bonus, il, out = _nbest_args(B, W, n, beam, 1, len_bonus, input_lengths)
    lm, pen, out = _skip_args(lm, lm_panelty, out, B)
    _lib.check(_lib.load().hctr_nbest_skip_logits(ctx, lm, _lib.ptr(logits), on_dev, W, B, C, beam, n, pen, bonus,
                                                  _lib.ptr(il), *[_lib.ptr(a) for a in out]), ctx)
    return _skip_result(out)


def nbest_skip_images(ctx, x, dt, on_dev, widths, B, W, n=5, beam=10, len_bonus=0.0, input_lengths=None, lm=None,
                      lm_panelty=2.0):
    """NBest by the skip search of line images (hctr_nbest_skip); x, dt, on_dev, widths as in ``nbest_images``"""
    n, beam, _, bonus, il, out = _nbest_args(B, W, n, beam, 1, len_bonus, input_lengths)
    lm, pen, out = _skip_args(lm, lm_panelty, out, B)
    _lib.check(_lib.load().hctr_nbest_skip(ctx, lm, _lib.ptr(x), dt, on_dev, _lib.ptr(widths), B, W, beam, n, pen, bonus,
                                           _lib.ptr(il), *[_lib.ptr(a) for a in out]), ctx)
    return _skip_result(out)


def sweep_pairs(alphas=None, betas=None, pairs=None):
    """(lm_panelty [G], len_bonus [G]) float64 of a weight grid: ``alphas`` x ``betas`` expanded alpha-major, the order
    in which the reference's loops run (``for a in alphas: for b in betas``, test.py:352-353), or a flat ``pairs`` list
    of (lm_panelty, len_bonus)."""
    if pairs is not None:
        if alphas is not None or betas is not None:
            raise ValueError("give alphas and betas, or pairs, not both")
        pr = np.asarray(list(pairs), np.float64).reshape(-1, 2)
    else:
        if alphas is None or betas is None:
            raise ValueError("a sweep needs alphas and betas, or pairs")
        al, be = np.asarray(alphas, np.float64).reshape(-1), np.asarray(betas, np.float64).reshape(-1)
        pr = np.stack([np.repeat(al, be.size), np.tile(be, al.size)], axis=1)
    if pr.shape[0] < 1:
        raise ValueError("a sweep needs at least one (lm_panelty, len_bonus) pair")
    return np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])


class LMSweep(object):
    """Result of the LM weight sweep over B lines and G pairs (numpy arrays, on the host; include/hctr_hip.h
    ``hctr_lm_sweep*``): ``lm_panelty`` / ``len_bonus`` float64 [G], the pairs; ``edits`` int32 [G, B], the edit distance
    of line b's 1-best text under pair g to its transcription; ``hyp_lengths`` int32 [G, B]; ``empty`` uint8 [B], 1 for
    a line whose greedy text is empty (it contributes the empty text under every pair; the reference raises
    IndexError there); ``ref_lengths`` int32 [B]. With ``texts=True`` also ``labels`` int32 [G, B, W], ``logps``,
    ``scores``, ``lm_scores`` float64 [G, B], the 1-best's values as ``nbest(lm=, n=1)`` returns them; otherwise None."""

    def __init__(self, lm_panelty, len_bonus, edits, hyp_lengths, empty, ref_lengths, labels=None, logps=None, scores=None,
                 lm_scores=None):
        self.lm_panelty, self.len_bonus = np.asarray(lm_panelty, np.float64), np.asarray(len_bonus, np.float64)
        self.edits, self.hyp_lengths, self.empty = edits, hyp_lengths, empty
        self.ref_lengths = np.asarray(ref_lengths, np.int32)
        self.labels, self.logps, self.scores, self.lm_scores = labels, logps, scores, lm_scores

    def __len__(self):
        return len(self.lm_panelty)

    @property
    def pairs(self):
        return [(float(a), float(b)) for a, b in zip(self.lm_panelty, self.len_bonus)]

    @property
    def total_edits(self):
        """int64 [G]"""
        return np.asarray(self.edits, np.int64).reshape(len(self), -1).sum(axis=1)

    @property
    def nchars(self):
        return int(self.ref_lengths.astype(np.int64).sum())

    @property
    def cer(self):
        """float64 [G]: total_edits / nchars, the reference's CER (test.py:285); NaN without a reference character"""
        n = self.nchars
        return self.total_edits / n if n else np.full((len(self),), np.nan)

    def label_lists(self):
        """per pair, per line the 1-best's label array (``texts=True`` only)"""
        if self.labels is None:
            raise ValueError("the sweep was run without texts=True")
        return [[self.labels[g, b, :int(self.hyp_lengths[g, b])].copy() for b in range(self.labels.shape[1])]
                for g in range(len(self))]


class LMSweepTotals(object):
    """Sweeps of successive batches over one grid, added up: ``update(sweep)`` per batch, then ``cer`` [G], ``best()``
    and ``report()``, which are what the reference's grid search (test.py:347-382) computes and prints."""

    def __init__(self):
        self.lm_panelty = self.len_bonus = self.total_edits = None
        self.nchars = 0
        self.nlines = 0

    def update(self, sweep):
        if self.total_edits is None:
            self.lm_panelty, self.len_bonus = sweep.lm_panelty.copy(), sweep.len_bonus.copy()
            self.total_edits = np.zeros((len(sweep),), np.int64)
        elif not (np.array_equal(self.lm_panelty, sweep.lm_panelty) and np.array_equal(self.len_bonus, sweep.len_bonus)):
            raise ValueError("the sweep was run over another grid of pairs")
        self.total_edits += sweep.total_edits
        self.nchars += sweep.nchars
        self.nlines += int(sweep.ref_lengths.size)
        return self

    @property
    def pairs(self):
        return [] if self.total_edits is None else [(float(a), float(b)) for a, b in zip(self.lm_panelty, self.len_bonus)]

    @property
    def cer(self):
        if self.total_edits is None:
            return np.zeros((0,), np.float64)
        return self.total_edits / self.nchars if self.nchars else np.full(self.total_edits.shape, np.nan)

    def _walk(self):
        """per pair (pair, cer, running minimum before it), then the final minimum: the reference's rule - start from
        min_cer = 1.0, min_params = (0, 0), replace only on strictly smaller"""
        min_cer, min_params, steps = 1.0, (0, 0), []
        for pair, cer in zip(self.pairs, self.cer.tolist()):
            steps.append((pair, cer, min_params, min_cer))
            if cer < min_cer:
                min_cer, min_params = cer, pair
        return steps, min_params, min_cer

    def best(self):
        """((lm_panelty, len_bonus), cer) of the first pair with the lowest CER below 1.0; ((0, 0), 1.0) when none is"""
        _, params, cer = self._walk()
        return params, cer

    def report(self):
        """the lines the reference's loop prints (test.py:354-355, 382), the running minimum as it stood before each pair"""
        steps, params, cer = self._walk()
        out = ["searching with a:{}, b:{}, min params:{}, min cer:{}".format(a, b, mp, mc) for (a, b), _, mp, mc in steps]
        out.append("min params:{}, min cer: {}".format(params, cer))
        return out


def _sweep_args(B, W, targets, target_lengths, lm, alphas, betas, pairs, chunk, input_lengths, texts):
    if lm is None:
        raise ValueError("the sweep needs an n-gram model (lm=)")
    tg, tl = normalize_targets(targets, target_lengths, B)
    al, be = sweep_pairs(alphas, betas, pairs)
    G = int(al.size)
    il = normalize_input_lengths(input_lengths, B)
    out = [np.zeros((G, B), np.int32), np.zeros((G, B), np.int32), np.zeros((B,), np.uint8), None, None, None, None]
    if texts:
        out[3:] = [np.zeros((G, B, W), np.int32)] + [np.full((G, B), -np.inf, np.float64) for _ in range(3)]
    tail = [_lib.ptr(al), _lib.ptr(be), G, int(chunk), _lib.ptr(il), _lib.ptr(tg), _lib.ptr(tl)] + [_lib.ptr(a) for a in out]
    keep = (al, be, il, tg, tl)
    return tail, keep, lambda: LMSweep(al, be, out[0], out[1], out[2], tl, *out[3:])


def lm_sweep_chunk(lines, W, beam, G):
    """pairs per launch the engine chooses for ``chunk=0`` (hctr_lm_sweep_chunk)"""
    return int(_lib.load().hctr_lm_sweep_chunk(int(lines), int(W), int(beam), int(G)))


def lm_sweep_topk(ctx, topk_idx, topk_logp, C, targets, target_lengths, lm, alphas=None, betas=None, pairs=None, beam=10,
                  chunk=0, input_lengths=None, texts=False):
    """LMSweep of front-end lists ``topk_idx`` int32 / ``topk_logp`` float32 [W, B, k] over ``C`` classes
    (hctr_lm_sweep_topk): per pair what ``nbest_topk(lm=, n=1)`` + ``edit_distance_labels`` return, in one call."""
    idx = np.ascontiguousarray(topk_idx, dtype=np.int32)
    lp = np.ascontiguousarray(topk_logp, dtype=np.float32)
    if idx.ndim != 3 or idx.shape != lp.shape:
        raise ValueError("topk_idx and topk_logp must both be [W,B,k]")
    W, B, k = (int(v) for v in idx.shape)
    tail, keep, result = _sweep_args(B, W, targets, target_lengths, lm, alphas, betas, pairs, chunk, input_lengths, texts)
    _lib.check(_lib.load().hctr_lm_sweep_topk(ctx, lm, _lib.ptr(idx), _lib.ptr(lp), W, B, int(C), k, int(beam), *tail), ctx)
    return result()


def lm_sweep_logits(ctx, logits, on_dev, targets, target_lengths, lm, alphas=None, betas=None, pairs=None, beam=10, depth=10,
                    chunk=0, input_lengths=None, texts=False):
    """LMSweep of caller logits / log-probs in WBC layout (hctr_lm_sweep_logits)"""
    if len(logits.shape) != 3:
        raise ValueError("logits must be [W,B,C]")
    W, B, C = (int(v) for v in logits.shape)
    tail, keep, result = _sweep_args(B, W, targets, target_lengths, lm, alphas, betas, pairs, chunk, input_lengths, texts)
    _lib.check(_lib.load().hctr_lm_sweep_logits(ctx, lm, _lib.ptr(logits), on_dev, W, B, C, int(depth), int(beam), *tail), ctx)
    return result()


def lm_sweep_images(ctx, x, dt, on_dev, widths, B, W, targets, target_lengths, lm, alphas=None, betas=None, pairs=None,
                    beam=10, depth=10, chunk=0, input_lengths=None, texts=False):
    """LMSweep of line images (hctr_lm_sweep); x, dt, on_dev, widths as in ``nbest_images``"""
    tail, keep, result = _sweep_args(B, W, targets, target_lengths, lm, alphas, betas, pairs, chunk, input_lengths, texts)
    _lib.check(_lib.load().hctr_lm_sweep(ctx, lm, _lib.ptr(x), dt, on_dev, _lib.ptr(widths), B, W, int(depth), int(beam),
                                         *tail), ctx)
    return result()


_FN = None


def _autograd_fn():
    """The torch.autograd.Function behind CTCLoss on an input that requires a gradient (made on first use: the package
    imports without torch). forward is the forward-only entry, exactly what an input without requires_grad gets;
    backward runs the gradient entry once, with the final per-line weights, so nothing of the input's size is kept
    between the two and no pass over the gradient is needed to scale it."""
    global _FN
    if _FN is not None:
        return _FN
    import torch

    class _CtcFn(torch.autograd.Function):
        @staticmethod
        def forward(fn_ctx, log_probs, crit, targets, input_lengths, target_lengths):
            from .codec import ctc_codec
            logits, on_dev = ctc_codec._as_logits(log_probs)
            B = int(logits.shape[1])
            tg, tl = normalize_targets(targets, target_lengths, B)
            il = normalize_input_lengths(input_lengths, B)
            nll = loss_logits(crit._context(), logits, on_dev, tg, tl, il)
            fn_ctx.save_for_backward(log_probs)
            fn_ctx.hctr = (crit, tg, tl, il, nll)
            return wrap(reduce(nll, tl, crit.reduction, crit.zero_infinity), log_probs)

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(fn_ctx, grad_output):
            from .codec import ctc_codec
            (log_probs,) = fn_ctx.saved_tensors
            crit, tg, tl, il, nll = fn_ctx.hctr
            w, nan = line_weights(tl, crit.reduction, grad_output.detach().double().cpu().numpy(), nll,
                                  crit.zero_infinity)
            logits, on_dev = ctc_codec._as_logits(log_probs)
            _, grad = loss_grad_logits(crit._context(), logits, on_dev, tg, tl, il, w)
            grad = torch.as_tensor(grad, device=log_probs.device)
            fill_nan_rows(grad, nan, il)
            return grad.to(log_probs.dtype).reshape(log_probs.shape), None, None, None, None

    _FN = _CtcFn
    return _FN


class _EngineBound(object):
    """context handling shared by CTCLoss and CTCAligner: a lazy weightless context on a chosen GPU, or an attached
    hctr_model's"""

    def __init__(self):
        self._ctx = None
        self._model = None
        self._device = 0

    def cuda(self, device=0):
        if hasattr(device, "index"):
            device = device.index or 0
        self._drop_ctx()
        self._device = int(device or 0)
        return self

    def to(self, device):
        s = str(device)
        if s.startswith("cuda"):
            return self.cuda(int(s.split(":")[1]) if ":" in s else 0)
        raise ValueError("the engine's CTC kernels run on a GPU only")

    def attach(self, model):
        self._drop_ctx()
        if model._ctx is None:
            raise RuntimeError("model is not on a GPU")
        self._model = model
        return self

    def _context(self):
        if self._model is not None:
            if self._model._ctx is None:
                raise RuntimeError("the attached hctr_model is no longer on a GPU")
            return self._model._ctx
        if self._ctx is None:
            ctx = ctypes.c_void_p()
            _lib.check(_lib.load().hctr_create(ctypes.byref(ctx), self._device, 3))
            self._ctx = ctx
        return self._ctx

    def _drop_ctx(self):
        if self._ctx is not None:
            _lib.load().hctr_destroy(self._ctx)
        self._ctx, self._model = None, None

    def __del__(self):
        try:
            self._drop_ctx()
        except Exception:
            pass


class CTCAligner(_EngineBound):
    """Forced alignment on the engine: ``CTCAligner().cuda(0)(log_probs_or_logits, targets, input_lengths,
    target_lengths)`` with the arguments of ``CTCLoss`` (``[T, B, C]`` numpy array or torch tensor, a CUDA tensor is read
    in place; targets 1-D concatenated or 2-D padded) returns the ``CTCAlignment`` of every line's best path: per
    character its pixel-column span and log-probability, per line the path and its score. Only blank=0 is supported.
    Masked logits (-inf beside a finite logit in the row) mean probability 0: the best path avoids them, and a line
    they leave no path is a line with no alignment. A line with a non-finite row (a NaN, a +inf, nothing but -inf) in
    its input length has score NaN, a path and spans that are in range but mean nothing, and NaN for the ``logps`` of a
    span that holds the row; the other lines are untouched (include/hctr_hip.h, "masked and non-finite logits")."""

    def __init__(self, blank=0):
        if blank != 0:
            raise NotImplementedError("the engine's CTC kernels use blank = 0 (the reference's codec)")
        _EngineBound.__init__(self)
        self.blank = blank

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        from .codec import ctc_codec
        if _is_torch(log_probs):
            log_probs = log_probs.detach()
        logits, on_dev = ctc_codec._as_logits(log_probs)
        return align_logits(self._context(), logits, on_dev, targets, target_lengths, input_lengths)

    __call__ = forward


class KeywordSpotter(_EngineBound):
    """Keyword spotting on the engine: ``KeywordSpotter().cuda(0)(log_probs_or_logits, queries, input_lengths=None)``
    with ``[T, B, C]`` input (numpy array or torch tensor, a CUDA tensor is read in place) and ``queries`` a sequence of
    label sequences (1..32 labels each) returns the ``Spotting`` of every (line, query) pair: the posterior probability
    that the line's text contains the query, and the best segment that reads it. Only blank=0 is supported.
    Masked logits (-inf beside a finite logit in the row) mean probability 0; a pair they leave no path gets -inf, -inf,
    -1, -1. A line with a non-finite row (a NaN, a +inf, nothing but -inf) in its input length has ``logp`` NaN, and
    its segment is the best of those that end before the row (or none): a segment never spans such a row. The other
    lines are untouched (include/hctr_hip.h, "masked and non-finite logits")."""

    def __init__(self, blank=0):
        if blank != 0:
            raise NotImplementedError("the engine's CTC kernels use blank = 0 (the reference's codec)")
        _EngineBound.__init__(self)
        self.blank = blank

    def forward(self, log_probs, queries, input_lengths=None):
        from .codec import ctc_codec
        if _is_torch(log_probs):
            log_probs = log_probs.detach()
        logits, on_dev = ctc_codec._as_logits(log_probs)
        return spot_logits(self._context(), logits, on_dev, queries, input_lengths)

    __call__ = forward


class LexiconRecognizer(_EngineBound):
    """Lexicon recognition on the engine: ``LexiconRecognizer().cuda(0)(log_probs_or_logits, lex, n=5,
    input_lengths=None, scores=False)`` with ``[T, B, C]`` input (numpy array or torch tensor, a CUDA tensor is read in
    place) and ``lex`` a ``Lexicon`` returns the ``LexiconResult``: per line the ``n`` best entries with their exact
    log p(entry | line), ranks and the lexicon's total mass. Only blank=0 is supported.
    Masked logits (-inf beside a finite logit in the row) mean probability 0; an entry they leave no path scores -inf
    and is left out of the ranking and of ``count``. A line with a non-finite row (a NaN, a +inf, nothing but -inf) in
    its input length ranks nothing: ``count`` 0, ``log_total`` -inf, every score -inf or NaN. The other lines are
    untouched (include/hctr_hip.h, "masked and non-finite logits")."""

    def __init__(self, blank=0):
        if blank != 0:
            raise NotImplementedError("the engine's CTC kernels use blank = 0 (the reference's codec)")
        _EngineBound.__init__(self)
        self.blank = blank

    def forward(self, log_probs, lex, n=5, input_lengths=None, scores=False):
        from .codec import ctc_codec
        if _is_torch(log_probs):
            log_probs = log_probs.detach()
        logits, on_dev = ctc_codec._as_logits(log_probs)
        return lexicon_logits(self._context(), logits, on_dev, lex, n, input_lengths, scores)

    __call__ = forward


class WordRecognizer(_EngineBound):
    """Word-sequence recognition on the engine: ``WordRecognizer().cuda(0)(log_probs_or_logits, lex, word_bonus=0.0,
    max_words=None, input_lengths=None)`` with ``[T, B, C]`` input (numpy array or torch tensor, a CUDA tensor is read in
    place) and ``lex`` a ``Lexicon`` returns the ``WordsResult``: per line the best segmentation into entries with the
    column at which each word begins, the concatenated text and its loss. Only blank=0 is supported.
    Masked logits (-inf beside a finite logit in the row) mean probability 0; a line they leave no sequence of entries,
    and a line with a non-finite row (a NaN, a +inf, nothing but -inf) in its input length, get ``count`` 0, ``score``
    -inf, ``text_nll`` +inf. The other lines are untouched (include/hctr_hip.h, "masked and non-finite logits")."""

    def __init__(self, blank=0):
        if blank != 0:
            raise NotImplementedError("the engine's CTC kernels use blank = 0 (the reference's codec)")
        _EngineBound.__init__(self)
        self.blank = blank

    def forward(self, log_probs, lex, word_bonus=0.0, max_words=None, input_lengths=None):
        from .codec import ctc_codec
        if _is_torch(log_probs):
            log_probs = log_probs.detach()
        logits, on_dev = ctc_codec._as_logits(log_probs)
        return words_logits(self._context(), logits, on_dev, lex, word_bonus, max_words, input_lengths)

    __call__ = forward


class PatternRecognizer(_EngineBound):
    """Pattern-constrained recognition on the engine: ``PatternRecognizer().cuda(0)(log_probs_or_logits, pat,
    input_lengths=None, full=True)`` with ``[T, B, C]`` input (numpy array or torch tensor, a CUDA tensor is read in
    place) and ``pat`` a ``Pattern`` returns the ``PatternResult``: per line the log-probability that its text matches
    the pattern and, with ``full``, the best matching reading with spans and confidences. Only blank=0 is supported.
    Masked logits (-inf beside a finite logit in the row) mean probability 0; a line they leave no matching path, and a
    line with a non-finite row (a NaN, a +inf, nothing but -inf) in its input length, get what a line gets that nothing
    matches: ``logp`` = ``best_logp`` = -inf, path -1, lengths 0, ``text_nll`` +inf. The other lines are untouched
    (include/hctr_hip.h, "masked and non-finite logits")."""

    def __init__(self, blank=0):
        if blank != 0:
            raise NotImplementedError("the engine's CTC kernels use blank = 0 (the reference's codec)")
        _EngineBound.__init__(self)
        self.blank = blank

    def forward(self, log_probs, pat, input_lengths=None, full=True):
        from .codec import ctc_codec
        if _is_torch(log_probs):
            log_probs = log_probs.detach()
        logits, on_dev = ctc_codec._as_logits(log_probs)
        return pattern_logits(self._context(), logits, on_dev, pat, input_lengths, full)

    __call__ = forward


class CTCLoss(_EngineBound):
    """Drop-in for the reference's criterion ``CTCLoss(zero_infinity=True)`` (main.py:205) on the engine:
    ``criterion(log_probs_or_logits, targets, input_lengths, target_lengths)`` with ``[T, B, C]`` input - raw logits or
    log-probs give the same result (log_softmax is idempotent). A torch input that requires a gradient gets a loss with
    a ``grad_fn``: ``loss.backward()`` deposits ``w_b * (softmax - posterior occupancy)`` in the input's ``.grad``, the
    derivative in raw logits and, for log-probs, what torch's own ctc_loss hands to the ``log_softmax`` before it (which
    passes it through unchanged). ``loss_and_grad`` is the same without autograd. Bind it to a GPU with
    ``.cuda(device)``, or share an hctr_model's engine context with ``.attach(model)``. Only blank=0 is supported.
    Masked logits (-inf beside a finite logit in the row) mean probability 0: the loss is the defined one, +inf for a
    line whose every alignment goes through a masked entry (as for a line too short for its targets), and the gradient
    at a masked entry is exactly 0. This DIFFERS FROM TORCH, whose ``ctc_loss(x.log_softmax(2), ...)`` returns a NaN
    gradient for the whole tensor once one logit is -inf (and NaN at the masked entries when the log-probs are the
    leaf). A line with a non-finite row (a NaN, a +inf, nothing but -inf) in its input length has a loss of NaN or +inf,
    never a finite one: +inf, which ``zero_infinity`` turns into 0 with zero gradient rows, unless the row is one of the
    line's last two (NaN, with NaN in the gradient). The other lines are untouched (include/hctr_hip.h, "masked and
    non-finite logits")."""

    def __init__(self, blank=0, reduction="mean", zero_infinity=False):
        if blank != 0:
            raise NotImplementedError("the engine's CTC loss uses blank = 0 (the reference's codec)")
        if reduction not in _REDUCTIONS:
            raise ValueError("reduction must be one of %s" % (_REDUCTIONS,))
        _EngineBound.__init__(self)
        self.blank = blank
        self.reduction = reduction
        self.zero_infinity = zero_infinity

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        from .codec import ctc_codec
        if _is_torch(log_probs) and log_probs.requires_grad:
            import torch
            if torch.is_grad_enabled():
                return _autograd_fn().apply(log_probs, self, targets, input_lengths, target_lengths)
        logits, on_dev = ctc_codec._as_logits(log_probs)
        nll = loss_logits(self._context(), logits, on_dev, targets, target_lengths, input_lengths)
        tl = normalize_targets(targets, target_lengths, int(logits.shape[1]))[1]
        return wrap(reduce(nll, tl, self.reduction, self.zero_infinity), log_probs)

    __call__ = forward

    def loss_and_grad(self, log_probs, targets, input_lengths, target_lengths):
        """(loss, grad) without autograd, for numpy input and torch input alike: ``loss`` as ``forward`` returns it,
        ``grad`` = d(reduced loss)/d(input) (for 'none': of the sum of the lines' losses), of the input's shape, kind,
        device and dtype. With ``zero_infinity=False`` a line without an alignment has NaN rows, as in torch."""
        from .codec import ctc_codec
        logits, on_dev = ctc_codec._as_logits(log_probs)
        B = int(logits.shape[1])
        tg, tl = normalize_targets(targets, target_lengths, B)
        il = normalize_input_lengths(input_lengths, B)
        ctx = self._context()
        # the weights need the lines' losses only where one is +inf and zero_infinity is off: the engine writes zeros
        # for such a line, and its rows are filled afterwards
        w, _ = line_weights(tl, self.reduction, None, None, self.zero_infinity)
        nll, grad = loss_grad_logits(ctx, logits, on_dev, tg, tl, il, w)
        nan = line_weights(tl, self.reduction, None, nll, self.zero_infinity)[1]
        fill_nan_rows(grad, nan, il)
        loss = wrap(reduce(nll, tl, self.reduction, self.zero_infinity), log_probs)
        if _is_torch(log_probs):
            import torch
            grad = torch.as_tensor(grad, device=log_probs.device).to(log_probs.dtype)
        elif np.issubdtype(np.asarray(log_probs).dtype, np.floating):
            grad = grad.astype(np.asarray(log_probs).dtype, copy=False)
        return loss, grad
