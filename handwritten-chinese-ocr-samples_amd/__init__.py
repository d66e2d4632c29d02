"""MI355X-native hctr inference engine (package root).

The directory name contains hyphens (it mirrors the reference repository's name), so import it with
``importlib.import_module("handwritten-chinese-ocr-samples_amd")`` or through the ``hctr_amd`` alias
module at the repository root.

Public surface = the reference's surface for this path:
  hctr_model   drop-in for models/handwritten_ctr_model.py:156 (engine-backed)
  ctc_codec    drop-in for utils/ctc_codec.py:14                (engine-backed)
  CTCLoss      drop-in for the criterion of main.py:205           (engine-backed, with backward())
  CTCAligner   forced alignment: character spans and confidences  (engine-backed; no counterpart)
  Evaluation   result of hctr_model.evaluate / ctc_codec.evaluate: edit distance, CER / CR / AR, error counts and the
               character alignment against the truth              (engine-backed; reference: editdistance.eval)
  edit_distance  per-line Levenshtein distance of two lists of strings or label sequences, on the device
  Recognition  result of hctr_model.recognize / ctc_codec.recognize: the greedy text with per-character spans,
               confidences and runners-up                          (engine-backed; no counterpart)
  NBest        result of hctr_model.nbest / ctc_codec.nbest: the N best texts of a line with their log-probabilities,
               by the device prefix beam search without a language model (engine-backed)
  KeywordSpotter  keyword spotting on logits: per (line, query) the posterior probability that the line's text contains
               the query, and the best segment that reads it; Spotting is its result and that of hctr_model.spot /
               ctc_codec.spot                                       (engine-backed; no counterpart)
  LexiconRecognizer  lexicon recognition on logits: which entry of a closed list (a Lexicon) each line is - the exact
               log p(entry | line) of every entry by one CTC forward over the lexicon's trie, the n best with ranks and
               posteriors; LexiconResult is its result and that of hctr_model.lexicon / ctc_codec.lexicon
                                                                    (engine-backed; no counterpart)
  PatternRecognizer  pattern-constrained recognition on logits: the exact probability that a line's text matches a
               Pattern (a DFA over labels, or Pattern.compile of a regular expression) by one CTC forward over the
               automaton, and the best matching reading with spans and confidences; PatternResult is its result and that
               of hctr_model.pattern / ctc_codec.pattern          (engine-backed; no counterpart)
  WordRecognizer  word-sequence recognition on logits: the line is a sequence of entries of a Lexicon - which, and
               where: the best segmentation by token passing over the lexicon's trie, with per-entry log priors and a
               word bonus; WordsResult is its result and that of hctr_model.words / ctc_codec.words
                                                                    (engine-backed; no counterpart)
  LMSweep      result of hctr_model.lm_sweep / ctc_codec.lm_sweep: edit distances of the LM-scored 1-best under a grid of
               (lm_panelty, len_bonus) pairs; LMSweepTotals adds batches up and answers the reference's test.py -gs
plus ``synth`` (deterministic synthetic checkpoints / line images) and ``build`` / ``load_library``.
"""
from . import preprocess, synth  # noqa: F401
from ._lib import build, load as load_library  # noqa: F401
from .codec import ArpaLM, ToyBigramLM, ZeroLM, ctc_codec  # noqa: F401
from .ctc import (CTCAligner, CTCAlignment, CTCLoss, Evaluation, KeywordSpotter, LMSweep, LMSweepTotals, NBest,  # noqa: F401
                  Lexicon, LexiconRecognizer, LexiconResult, Pattern, PatternRecognizer, PatternResult, Recognition,
                  Spotting, WordRecognizer, WordsResult)
from .model import hctr_model  # noqa: F401

_EDIT_BOUND = None


def edit_distance(hyps, refs, device=0):
    """Per-line Levenshtein distance (int32 array) of two equally long lists of strings or of int sequences, computed
    on the GPU (include/hctr_hip.h ``hctr_edit_distance``). Strings are compared by code point: ``editdistance.eval``
    on each pair, exactly. A distance between label sequences of a ``ctc_codec`` equals the distance between the
    strings they stand for when the codec's ``chars_list`` has no duplicate entries."""
    global _EDIT_BOUND
    from . import ctc
    if _EDIT_BOUND is None or _EDIT_BOUND._device != int(device):
        _EDIT_BOUND = ctc._EngineBound().cuda(device)
    return ctc.edit_distance_sequences(_EDIT_BOUND._context(), list(hyps), list(refs), maps=False).edits

__all__ = ["hctr_model", "ctc_codec", "CTCLoss", "CTCAligner", "CTCAlignment", "Recognition", "Evaluation", "NBest", "LMSweep", "LMSweepTotals", "KeywordSpotter", "Spotting", "Lexicon", "LexiconRecognizer", "LexiconResult", "Pattern", "PatternRecognizer", "PatternResult", "WordRecognizer", "WordsResult", "edit_distance", "ZeroLM", "ToyBigramLM", "ArpaLM", "synth", "preprocess", "build", "load_library"]
