"""CTC loss on the engine: the criterion of the reference's evaluation stack (``CTCLoss(zero_infinity=True)`` over
``preds.log_softmax(2)``, main.py:205,379-409), forward only.

``CTCLoss`` is the drop-in for that criterion on caller logits (``criterion(preds, targets, input_lengths,
target_lengths)``); ``hctr_model.ctc_loss`` scores line images without the logits ever leaving the device. Both run the
C ABI's ``hctr_ctc_loss*`` (include/hctr_hip.h); target normalisation and the reductions are the host-side helpers below,
with the semantics of ``torch.nn.CTCLoss``.
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


class CTCLoss(object):
    """Drop-in for the reference's criterion ``CTCLoss(zero_infinity=True)`` (main.py:205) on the engine:
    ``criterion(log_probs_or_logits, targets, input_lengths, target_lengths)`` with ``[T, B, C]`` input - raw logits or
    log-probs give the same result (log_softmax is idempotent). Forward only (no gradient). Bind it to a GPU with
    ``.cuda(device)``, or share an hctr_model's engine context with ``.attach(model)``. Only blank=0 is supported."""

    def __init__(self, blank=0, reduction="mean", zero_infinity=False):
        if blank != 0:
            raise NotImplementedError("the engine's CTC loss uses blank = 0 (the reference's codec)")
        if reduction not in _REDUCTIONS:
            raise ValueError("reduction must be one of %s" % (_REDUCTIONS,))
        self.blank = blank
        self.reduction = reduction
        self.zero_infinity = zero_infinity
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
        raise ValueError("the engine's CTC loss runs on a GPU only")

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

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        from .codec import ctc_codec
        logits, on_dev = ctc_codec._as_logits(log_probs)
        nll = loss_logits(self._context(), logits, on_dev, targets, target_lengths, input_lengths)
        tl = normalize_targets(targets, target_lengths, int(logits.shape[1]))[1]
        return wrap(reduce(nll, tl, self.reduction, self.zero_infinity), log_probs)

    __call__ = forward
