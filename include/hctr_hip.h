/*
 * hctr_hip.h - C ABI of libhctr_hip.so, the MI355X (gfx950) engine for the reference's
 * hctr CNN+CTC inference path.
 *
 * The reference (AndrewCullacino/handwritten-chinese-ocr-samples) has no FFI layer: the seam
 * for this path is two Python classes plus a checkpoint dict. Each entry point
 * below names the reference interface it stands behind (file:line relative to the reference
 * root). The Python shims in handwritten-chinese-ocr-samples_amd/{model,codec}.py bind these
 * with ctypes and keep the reference's class/method signatures; INTEGRATION.md shows the stub a
 * reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; the caller owns every host buffer for the duration of a call;
 *     the library owns device memory, workspace and the context;
 *   - every function returns 0 (HCTR_OK) or a negative hctr_status; the message for the last
 *     failure on a context is hctr_last_error(ctx); no C++ exception crosses the ABI;
 *   - a context is bound to one device and one HIP stream and is NOT re-entrant; use one context
 *     per thread/GPU. Calls are synchronous at return unless documented otherwise;
 *   - "WBC" = [W][B][C] row-major float32, the layout hctr_model.forward returns
 *     (models/handwritten_ctr_model.py:171-178).
 */
#ifndef HCTR_HIP_H
#define HCTR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hctr_ctx hctr_ctx;

typedef enum {
    HCTR_OK = 0,
    HCTR_ERR_ARG = -1,        /* bad argument (-> ValueError) */
    HCTR_ERR_HIP = -2,        /* HIP runtime failure, message has file:line (-> RuntimeError) */
    HCTR_ERR_STATE = -3,      /* call order violated, e.g. forward before finalize (-> RuntimeError) */
    HCTR_ERR_KEY = -4,        /* unknown / missing state-dict key (-> KeyError, as load_state_dict strict) */
    HCTR_ERR_SHAPE = -5,      /* tensor shape mismatch (-> RuntimeError, as load_state_dict) */
    HCTR_ERR_EMPTY_LINE = -6, /* beam search on a line whose greedy decode is empty, or whose beam set
                                 became empty: the reference raises IndexError (utils/ctc_codec.py:143,198,179) */
    HCTR_ERR_NOMEM = -7
} hctr_status;

typedef enum { HCTR_U8 = 0, HCTR_F32 = 1, HCTR_I64 = 2 } hctr_dtype;

/* ---- context: replaces hctr_model(num_classes) + .cuda(gpu) ---------------------------------
 * models/handwritten_ctr_model.py:156-169, test.py:143-148. num_classes = 1 + len(chars) + 1. */
int hctr_create(hctr_ctx** out, int device, int num_classes);
void hctr_destroy(hctr_ctx* ctx);
const char* hctr_last_error(const hctr_ctx* ctx);   /* ctx may be NULL: last create() failure */
const char* hctr_version(void);

/* ---- weight ingest: replaces model.load_state_dict(checkpoint['state_dict']) -----------------
 * test.py:152-153; key schema main.py:349-356 / SURVEY.md 8b (254 entries). Call once per entry
 * (any order), then hctr_finalize_weights, which checks completeness, folds eval-mode BatchNorm
 * (eps 1e-5) into the preceding conv, converts to the kernel layouts and uploads. fp32 tensors are
 * HCTR_F32; num_batches_tracked entries are HCTR_I64 and ignored. */
int hctr_load_tensor(hctr_ctx* ctx, const char* key, const void* host_ptr,
                     const int64_t* shape, int ndim, int dtype);
int hctr_finalize_weights(hctr_ctx* ctx);

/* ---- precision mode ----------------------------------------------------------------------------------
 * 0 = f16 (default): fp16 storage and MFMA inputs, fp32 accumulation - the 10-bit mantissa of the TF32
 *     mode the reference enables on its GPUs (main.py:37-41).
 * 1 = f16x3: every activation and weight is carried as a hi + lo fp16 pair and each product is formed
 *     as w_hi*x_hi + w_hi*x_lo + w_lo*x_hi in fp32 (about 3x the matrix work and memory); logits then
 *     agree with the fp32 CPU reference to ~1e-5 relative: its argmax / text is the reference's wherever
 *     two fp32 summation orders agree.
 * 2 = guarded ("auto"): every line runs in f16 and the head's fused epilogue also yields, per pixel column,
 *     the margin between the largest and second largest logit. A line is CERTAIN when every one of its
 *     columns (pad columns included - the reference decodes them too, utils/ctc_codec.py:75 over the padded
 *     batch of test.py:170-186) has margin > 2 * (rel * max|logit of the line| + abs): no error within the
 *     f16 logit tolerance rel * scale + abs can then change an argmax. Every other line is run again in
 *     f16x3 at the same padded width (a line's result depends only on its own pixels and that width) and
 *     its results replace the f16 ones - in hctr_greedy, hctr_forward_logits and hctr_beam_frontend alike.
 *     Text is then the f16x3 mode's wherever f16 cannot be trusted, at f16 speed for lines with peaky
 *     logits. Both weight sets stay resident (about 0.42 GB).
 * Before hctr_finalize_weights the mode decides which weight set(s) are built (0: f16, 1: f16x3, 2: both);
 * afterwards it may still be changed among the modes whose set(s) are resident (a context finalized in
 * mode 2 serves all three).
 * hctr_set_guard / hctr_get_guard: rel / abs of mode 2's criterion (either output pointer may be NULL). The
 *     tolerance is the guard's OWN, taken per line: the certificate holds for a checkpoint whose f16 logits are
 *     within rel * (max|logit| of THAT line) + abs of the fp32-grade ones. It is not the parity suite's f16
 *     tolerance (tests/test_gpu_parity.py scales by the batch-wide max|logit|, a looser bound). The defaults
 *     (csrc/engine.cpp guard_rel / guard_abs, the one place that defines them; a fresh context's hctr_get_guard
 *     returns them) are derived from the per-line f16-versus-f16x3 error measured on the engine: rel = 1.5 x
 *     the largest max|f16 - f16x3| / max|logit of the line| seen, abs = 0.05 ("Guard
 *     defaults"; tests/test_gpu_guard.py asserts the premise per line). A checkpoint whose per-line relative
 *     f16 error is larger needs a larger rel.
 * hctr_last_guard: figures of the last mode-2 call, per line of its batch: flags[i] = 1 if line i was
 *     run again in f16x3, min_margin[i] = its smallest column margin, scale[i] = its largest |logit| (f16 sweep).
 *     Any output pointer may be NULL; at most cap entries are written. */
int hctr_set_precision(hctr_ctx* ctx, int mode);
int hctr_set_guard(hctr_ctx* ctx, double rel, double abs_tol);
int hctr_get_guard(hctr_ctx* ctx, double* rel, double* abs_tol);
int hctr_last_guard(hctr_ctx* ctx, int64_t* lines, int64_t* flagged, uint8_t* flags, float* min_margin,
                    float* scale, int64_t cap);

/* ---- forward: replaces hctr_model.forward --------------------------------------------------
 * models/handwritten_ctr_model.py:171-178 (trunk :115-153). Input: a batch of B line images of
 * height 128 and common width W, either HCTR_F32 [B][1][128][W] already normalised to [-1,1]
 * (what test.py:179-193 feeds), or HCTR_U8 [B][128][W] raw grey levels, in which case the engine
 * applies NormalizePAD itself (utils/dataset.py:83-93): x/255, (x-0.5)/0.5, and columns
 * >= widths[b] replicate column widths[b]-1 (widths may be NULL = all W).
 * img_on_device / out_on_device: the pointer is a device pointer on ctx's device.
 * Output: float32 logits in WBC layout, B*W*num_classes values. */
int hctr_forward_logits(hctr_ctx* ctx, const void* img, int img_dtype, int img_on_device,
                        const int32_t* widths, int B, int W,
                        float* out_wbc, int out_on_device);

/* ---- fused forward + greedy decode: replaces model(x) -> codec.decode(...) greedy ------------
 * test.py:191-194 with utils/ctc_codec.py:70-99. Logits never leave the device; argmax takes the
 * first maximum (np.argmax), a column is kept iff idx!=0 && idx!=C-1 && idx!=previous raw idx.
 * labels: int32 [B][W] (first lengths[b] entries valid, the rest written as zeros), lengths: int32 [B]; host pointers.
 * The same holds for the labels of hctr_decode_greedy_logits and hctr_evaluate*: the whole array is written. */
int hctr_greedy(hctr_ctx* ctx, const void* img, int img_dtype, int img_on_device,
                const int32_t* widths, int B, int W,
                int32_t* labels, int32_t* lengths);

/* ---- decode of caller-supplied logits: replaces ctc_codec.decode(ndarray) greedy -------------
 * utils/ctc_codec.py:63-99. logits: float32 WBC with C classes (host or device pointer).
 * Like every entry point that launches kernels it starts a new profile: hctr_last_profile afterwards names its two
 * launches, argmax_rows and ctc_collapse. */
int hctr_decode_greedy_logits(hctr_ctx* ctx, const float* logits_wbc, int on_device,
                              int W, int B, int C, int32_t* labels, int32_t* lengths);

/* ---- beam-search front end on the device -----------------------------------------------------
 * utils/ctc_codec.py:65 (log_softmax), :127/:186 (top search_depth by descending log-prob), :128,144
 * (candidates with log-prob > ln 0.001 for the "skip" variant).
 * Runs the forward on img (or, when img == NULL, takes caller logits in WBC layout), then
 * log-softmax and top-k per (t, b), and copies to the host buffers
 *   topk_idx  int32 [W][B][k], topk_logp float32 [W][B][k]   (descending; ties: lower index first)
 *   blank_logp float32 [W][B]                                 (log-prob of class 0).
 * With want_candidates != 0 it also builds, per (t, b), the ascending list of classes whose
 * log-prob exceeds ln(0.001); the context keeps those lists until hctr_beam_fetch_candidates copies
 * them out: cand_off int64 [W*B+1] (CSR, row r = t*B + b), cand_idx int32 / cand_logp float32 of
 * *num_candidates entries. */
int hctr_beam_frontend(hctr_ctx* ctx, const void* img, int img_dtype, int img_on_device,
                       const int32_t* widths, const float* logits_wbc, int logits_on_device,
                       int B, int W, int C, int k, int want_candidates,
                       int32_t* topk_idx, float* topk_logp, float* blank_logp,
                       int64_t* num_candidates);
int hctr_beam_fetch_candidates(hctr_ctx* ctx, int64_t* cand_off, int32_t* cand_idx, float* cand_logp);

/* ---- log-softmax of caller logits: replaces scipy.special.log_softmax(preds, axis=2) ------------
 * utils/ctc_codec.py:65. float32 WBC in (host or device), float32 WBC out (host). Only needed when
 * the language model proposes candidates (use_tfm_pred), because those can be any class. */
int hctr_log_softmax(hctr_ctx* ctx, const float* logits_wbc, int on_device, int W, int B, int C,
                     float* out_host);

/* ---- masked (-inf) and non-finite logits: what every *_logits entry point below makes of them ----------------------
 * (hctr_ctc_loss_logits, hctr_ctc_loss_logits_grad, hctr_ctc_align_logits, hctr_spot_logits, hctr_lexicon_logits,
 * hctr_pattern_logits, hctr_recognize_logits. The image entry points share the kernels; the engine's own logits are finite.)
 * MASKED CLASS: a logit of -inf in a row that also holds a finite logit. The class has probability 0 in that column -
 * the way to restrict a CTC model to a vocabulary, or to forbid the blank inside a forced region - and every result is
 * the mathematically defined one, to the entry's stated precision; no result is NaN. "No alignment" covers a line whose
 * every path has probability 0, whether or not it passes the length test (L + adjacent equal labels <= T): such a line
 * gets exactly what a line that fails the length test gets -
 *   loss +inf; gradient rows zero; alignment score -inf, path -1 everywhere, spans -1, span_logp -inf;
 *   spotting -inf, -inf, -1, -1; a lexicon score of -inf and the entry left out of the ranking and of count;
 *   pattern logp = best_logp = -inf, path -1, lengths 0, text_nll +inf.
 * The gradient at a masked entry is exactly 0 (line_weight * (exp(-inf) - 0)); torch's ctc_loss differentiated through
 * log_softmax returns NaN for the whole tensor there, and NaN at the masked entries with the log-probs as the leaf.
 * NON-FINITE ROW: a row t < T of a line that holds a NaN or a +inf, or nothing but -inf. Its log-sum-exp is not a number
 * (NaN; -inf for a row of nothing but -inf), so every log-probability of the row is NaN. The call returns HCTR_OK, the
 * outputs of every other line are bit-identical to a call without the bad row, and the context stays usable. On the
 * bad line no score is finite: each is NaN or the entry's "nothing" value, and every integer output is in range (path
 * entries in [-1, C), spans in [-1, T], entry indices in [-1, N), counts in [0, n]) -
 *   loss:       NaN when the row is one of the line's last two, else +inf (the recursion's max drops a NaN operand, and
 *               two columns after the row every state is -inf); never finite.
 *   gradient:   rows zero where the loss is +inf; where it is NaN, NaN in the bad row and in the columns of the blank and
 *               of the line's own labels, line_weight * softmax elsewhere.
 *   alignment:  score NaN; path, span_start, span_end in range and without meaning; span_logp NaN for a span that holds
 *               the row.
 *   spotting:   contain_logp NaN. The segment is the best among those that END BEFORE the row, bit for bit what a
 *               call with input_lengths = t returns (-inf, -1, -1 where none does): a segment never spans a bad row.
 *   lexicon:    every score -inf or NaN, no entry ranked: count 0, log_total -inf, top_entry -1.
 *   pattern:    logp = best_logp = -inf, no path, lengths 0, text_nll +inf.
 *   recognize:  as stated there (labels as the greedy decode gives them, the affected figures NaN).
 * A row t >= T is never read: whatever it holds, the results are bit-identical. (hctr_recognize_logits has no lengths:
 * every row counts.) Logits so large that float32 log-probabilities overflow are outside this contract. */

/* ---- CTC loss on the device: replaces CTCLoss(zero_infinity=True) over preds.log_softmax(2) ------------
 * main.py:205 (criterion), :379-409 (targets from codec.encode, preds_sizes = [W] * B). The gradient: hctr_ctc_loss_logits_grad below.
 * nll[b] = -log sum over the alignments pi of line b's targets of prod_t softmax(z_t)[pi_t], with blank = class 0:
 * torch.nn.functional.ctc_loss(log_softmax(z), ..., blank=0, reduction='none', zero_infinity=False). A line with no
 * alignment (L + number of adjacent equal labels > T, or masked logits that leave every alignment the probability 0:
 * see "masked and non-finite logits" above) gets +inf; a line with L = 0 gets -sum_t log p_t(blank).
 *   targets:        int32, the lines' labels back to back (what codec.encode returns), sum(target_lengths) entries;
 *                   every id in [1, C-1] (C-1 = the "<unknown>" id encode emits), else HCTR_ERR_ARG. Host pointer.
 *   target_lengths: int32 [B], >= 0; a line's 2L + 1 extended states must fit 4096 (L <= 2047) unless it has no alignment.
 *   input_lengths:  int32 [B] in [1, W] (steps 0..T-1 of the line count), or NULL = W for every line as main.py has it
 *                   (the pad columns count, as in the reference).
 *   nll:            float32 [B], host.
 * B == 0 is a no-op. hctr_ctc_loss runs the forward of img (arguments as hctr_greedy) and scores its logits on the device,
 * in internal passes like every other entry point; a line's result depends on its own pixels, W and its targets only.
 * Precision: mode 0 f16, mode 1 f16x3; mode 2 ("auto") scores EVERY line in f16x3 - its top-1/top-2 margin certificate
 * bounds argmax flips, not losses - and leaves hctr_last_guard's figures as they were.
 * Error of a loss from a logit error dz: |dNLL| <= 2 * sum_t max_c |dz_{t,c}| (the gradient of NLL in z_t is softmax
 * minus the posterior occupancy, of L1 norm <= 2).
 * hctr_ctc_loss_logits scores caller logits (or log-probs: log_softmax is idempotent) in WBC layout with C classes, host
 * or device pointer; it needs no weights (a context made for ctc_codec serves). */
int hctr_ctc_loss(hctr_ctx* ctx, const void* img, int img_dtype, int img_on_device, const int32_t* widths,
                  int B, int W, const int32_t* targets, const int32_t* target_lengths,
                  const int32_t* input_lengths, float* nll);
int hctr_ctc_loss_logits(hctr_ctx* ctx, const float* logits_wbc, int on_device, int W, int B, int C,
                         const int32_t* targets, const int32_t* target_lengths,
                         const int32_t* input_lengths, float* nll);

/* ---- gradient of the CTC loss in caller logits: what scaler.scale(loss).backward() needs (main.py:426) ----
 * Arguments, checks, error codes and the L <= 2047 limit as hctr_ctc_loss_logits. For line b with T = input_lengths[b]:
 *   grad[t][b][c] = line_weight[b] * (softmax(z_t)[c] - gamma_t(c))   for t < T
 *   grad[t][b][c] = 0                                                  for t >= T, and for every t of a line whose loss is
 *                                                                      +inf, whatever its weight (zero_infinity=True)
 * gamma_t(c) = sum over the extended-target states s of class c of exp(alpha_t(s) + beta_t(s) - lp_t(c) + nll_b), the
 * posterior occupancy (sum_c gamma_t(c) = 1); classes that are neither the blank nor a target of the line get
 * line_weight[b] * softmax exactly. Every element of grad_wbc is written (it need not be cleared).
 * With respect to what: for raw logits z this is the exact derivative d(sum_b line_weight[b] * nll_b) / dz. For log-probs
 * it is what torch.nn.functional.ctc_loss returns for its log_probs argument (softmax - gamma, not -gamma); its rows sum
 * to zero, so the log_softmax backward that follows in the caller's graph passes it through unchanged - one definition
 * serves both kinds of input.
 *   line_weight: float32 [B], host; NULL = 1 for every line.
 *   nll:         float32 [B], host, or NULL; bit-identical to hctr_ctc_loss_logits' for the same arguments.
 *   grad_wbc:    float32 [W][B][C], host (grad_on_device = 0) or device pointer; must not alias the logits.
 * Device scratch (the context's grow-only CTC scratch, as the forward's; HCTR_ERR_NOMEM leaves the context usable):
 *   4 * B*W*D (emissions, D = the largest number of distinct classes of a line, blank included) + 8 * B*W (log-sum-exp
 *   of every row) + 4 * sum_b T_b * (2 L_b + 1) (the alpha rows, overwritten by the states' posterior shares; lines
 *   without an alignment take none; worst case one line 2000 * 4095 * 4 = 33 MB) + the per-line tables; plus W*B*C
 *   floats for each of logits / gradient that is passed as a host pointer.
 * Precision: alpha and beta are float32 log-space recursions; each row's gamma is normalised by its own sum, so a
 * gradient row sums to zero to float32 rounding. Needs no weights, like hctr_ctc_loss_logits. */
int hctr_ctc_loss_logits_grad(hctr_ctx* ctx, const float* logits_wbc, int on_device, int W, int B, int C,
                              const int32_t* targets, const int32_t* target_lengths, const int32_t* input_lengths,
                              const float* line_weight, float* nll, float* grad_wbc, int grad_on_device);

/* ---- CTC forced alignment on the device: where each character of a known transcription lies -----------------
 * Steps are pixel columns (one logit row per column, preds_sizes = [W] * B in main.py), so the best CTC path of a line's
 * transcription gives each character's pixel span, a confidence for it, and the path's log-probability. The reference has
 * no counterpart (utils/ctc_codec.py only decodes). Arguments, checks, error codes and the L <= 2047 limit as
 * hctr_ctc_loss_logits / hctr_ctc_loss; B == 0 is a no-op.
 * With lp_t(c) = z_t[c] - logsumexp(z_t) in float32 (the loss's emissions, bit for bit) and the extended states blank,
 * l_1, blank, ..., l_L, blank (S = 2L + 1):
 *   v_0(0) = lp_0(blank), v_0(1) = lp_0(l_1), -inf elsewhere;
 *   v_t(s) = max(v_{t-1}(s), v_{t-1}(s-1), [l_s != l_{s-2}] v_{t-1}(s-2)) + lp_t(class of s), in float32.
 * Ties are part of the contract: among equal predecessors s wins, then s-1, then s-2; the path ends in state S-1 if
 * v_{T-1}(S-1) >= v_{T-1}(S-2), else in S-2 (state 0 for L = 0).
 *   path:       int32 [B][W], host, or NULL: the class of the best path at every step t < T (0 = blank), -1 for t >= T.
 *   span_start: int32 [sum L], host, in the order of `targets`, or NULL: the first step of each target position;
 *   span_end:   the step after its last (a label's steps are contiguous), or NULL;
 *   span_logp:  float32: the sum of lp_t(label) over those steps, ascending t (exp(span_logp / (end - start)) is the
 *               geometric-mean probability, a per-character confidence), or NULL;
 *   score:      float32 [B], host, or NULL: v_{T-1}(end state), the best path's log-probability (<= -nll).
 * A line with no alignment (L + number of adjacent equal labels > T, the loss's test; or a best score of -inf, when
 * masked logits leave no path a probability above 0) gets score -inf, path -1 everywhere, spans -1 and span_logp -inf.
 * A line with a non-finite row has a NaN score: see "masked and non-finite logits" above.
 * hctr_ctc_align runs the forward of img in internal passes and aligns the stored-logits head exactly as hctr_ctc_loss
 * scores it: mode 0 f16, mode 1 f16x3, mode 2 EVERY line in f16x3, hctr_last_guard's figures left as they were.
 * hctr_ctc_align_logits takes caller logits or log-probs in WBC layout, host or device pointer, and needs no weights.
 * Device scratch (the context's grow-only CTC scratch; HCTR_ERR_NOMEM leaves the context usable): 4 * n*W*D (emissions;
 * n = B, or the lines of one pass for images; D = the largest number of distinct classes of a line, blank included)
 * + sum_b T_b * ceil((2 L_b + 1) / NS) (2-bit backpointers, one byte per NS states and step; NS = 1, 2 or 4 for a
 * longest feasible target of <= 31, <= 1023 or more labels; lines without an alignment take none; 64 lines of 2000
 * steps and 100 labels: 13 MB; worst case one line 2000 * 1024 = 2 MB) + 4 * B*W (path) + 12 * sum L (spans) + the
 * per-line tables; plus W*B*C floats for logits passed as a host pointer. */
int hctr_ctc_align(hctr_ctx* ctx, const void* img, int img_dtype, int img_on_device, const int32_t* widths,
                   int B, int W, const int32_t* targets, const int32_t* target_lengths,
                   const int32_t* input_lengths, int32_t* path, int32_t* span_start, int32_t* span_end,
                   float* span_logp, float* score);
int hctr_ctc_align_logits(hctr_ctx* ctx, const float* logits_wbc, int on_device, int W, int B, int C,
                          const int32_t* targets, const int32_t* target_lengths, const int32_t* input_lengths,
                          int32_t* path, int32_t* span_start, int32_t* span_end, float* span_logp, float* score);

/* ---- keyword spotting on the device: which lines contain a query, how surely, and where ---------------------------
 * The word-spotting question of handwriting recognition, answered from the CTC posterior and not from the 1-best text.
 * The reference has no counterpart. A line has T = input_lengths[b] columns that count (NULL = W; 0 <= T <= W),
 * p_t(c) = softmax(z_t)[c] with lp_t(c) its log in float32 (the loss's emissions, bit for bit), blank = class 0, and
 * B(pi) is the CTC collapse of a path pi in {0..C-1}^T. A query is q = (q_1 .. q_L), 1 <= L <= HCTR_SPOT_MAX_LEN, labels
 * in [1, C-1]. Two results per (line b, query k), all outputs [B][Q] on the host, any of them NULL:
 *
 * 1. contain_logp = log sum over the paths pi with q a contiguous substring of B(pi) of prod_t p_t(pi_t): the
 *    probability that the line's text contains the query - an exact sum over all paths. It is the forward recursion over
 *    the Knuth-Morris-Pratt automaton of q lifted to CTC. delta(j, c) = the longest k with q_1..q_k a suffix of
 *    q_1..q_j c (0 for every c not in q). The 2L states: Z (nothing matched), N_j (j = 1..L-1: j characters matched, the
 *    last column emitted q_j), B_j (j matched, the last column was blank), A (accepting, absorbing). Mass 1 starts in Z.
 *    With tgt(k) = Z for k = 0, A for k = L, else N_k, and rest = the probability of the classes that are neither blank
 *    nor in q, one column moves
 *      Z   -> Z: p(0) + rest + sum of p(c) over c in q, c != q_1;            Z -> tgt(1): p(q_1)
 *      N_j -> N_j: p(q_j);   N_j -> B_j: p(0);   N_j -> tgt(delta(j,c)): p(c), c in q, c != q_j;   N_j -> Z: rest
 *      B_j -> B_j: p(0);     B_j -> tgt(delta(j,c)): p(c), c in q, q_j included;                   B_j -> Z: rest
 *      A   -> A: 1
 *    and contain_logp is the log of A's mass after T columns (-inf for T = 0 and wherever no path holds q; for L = 1 it
 *    is log(1 - prod_t (1 - p_t(q_1)))). The masses are float64 and linear (the matrix is stochastic, so the total stays 1);
 *    rest is formed per column as max(0, 1 - p(0) - sum of p(c) over the classes of q) from the float32 emissions. A
 *    result below float64's floor (about -700) comes back as -inf.
 * 2. seg_logp, seg_start, seg_end = the maximum over 0 <= t0 < t1 <= T and segment paths s on columns [t0, t1) with
 *    s_t0 = q_1, s_(t1-1) = q_L and B(s) = q of sum_t lp_t(s_t), and its (t0, t1); -inf, -1, -1 where none fits. The
 *    max-plus CTC recursion over the 2L - 1 extended states q_1, 0, q_2, .., q_L in float32: a fresh start (score 0, start
 *    t) is offered to the first state at every column, each state carries the start column of its best path, and the
 *    answer is the best value the last state ever holds. Ties are part of the contract: between predecessors the
 *    strictly greater score wins and equal scores prefer the larger start column; the running best is replaced only by a
 *    strictly greater score, so the earliest end wins. Because lp <= 0 the segment is tight - it runs from inside the
 *    first character's run to inside the last one's; hctr_ctc_align / hctr_recognize give full character extents.
 * contain_logp >= seg_logp, and contain_logp >= -nll of hctr_ctc_loss with q as the line's target.
 *   queries:       int32, the queries back to back, sum(query_lengths) entries, host.   query_lengths: int32 [Q], host.
 * L outside [1, 32], a label outside [1, C-1], Q < 1, an input length outside [0, W] -> HCTR_ERR_ARG; B == 0 is a no-op.
 * A pair's results depend on its own line and query only, bit for bit: not on the other queries, their order, the chunk
 * it lands in, host or device pointers.
 * Queries are processed in chunks whose classes, blank included, number at most hctr_spot_chunk_classes(lines, W) (the
 * environment variable HCTR_SPOT_CLASSES overrides it; a single query with more classes gets a chunk of its own); one
 * pass over the logits per chunk writes the emissions every query of the chunk reads.
 * Device scratch (the context's grow-only CTC scratch; HCTR_ERR_NOMEM leaves the context usable): 4 * n*W*D emissions
 * (n = B, or the lines of one pass for images; D = the largest chunk's classes) + 16 * B*Q results + the automata and
 * per-chunk tables (4 * B*D each); plus W*B*C floats for logits passed as a host pointer.
 * hctr_spot runs the forward of img in internal passes on the stored-logits head exactly as hctr_ctc_loss does: mode 0
 * f16, mode 1 f16x3, mode 2 EVERY line in f16x3, hctr_last_guard's figures left as they were. hctr_spot_logits takes
 * caller logits or log-probs in WBC layout, host or device pointer, and needs no weights.
 * hctr_spot_automaton (host only, no context; errors are read with hctr_last_error(NULL)) exports the tables the kernel
 * is given for one query, so that they can be checked without a GPU. States are numbered Z = 0, N_j = j, B_j = L-1+j,
 * A = 2L-1; slots 0 = blank, 1..nq = the query's distinct classes in ascending order, nq+1 = rest, nq+2 = the constant 1.
 *   classes [nq], num_classes = nq;  delta [L][nq]: delta(j, classes[i]) for j = 0..L-1;  num_states = 2L;
 *   in_ptr [2L+1], in_src / in_slot [num_edges <= HCTR_SPOT_MAX_EDGES]: the in-edges of every state but Z in CSR form,
 *   a state's edges ordered by (source, slot) - the order the kernel adds them in; edge_cap = the room in in_src / in_slot;
 *   fall_mask [2L]: bit s set = the state sends slot s to Z (Z's inflow is the sum of those flows). Any output may be NULL. */
#define HCTR_SPOT_MAX_LEN 32
#define HCTR_SPOT_MAX_EDGES 2080
int hctr_spot(hctr_ctx* ctx, const void* img, int img_dtype, int img_on_device, const int32_t* widths, int B, int W,
              const int32_t* queries, const int32_t* query_lengths, int Q, const int32_t* input_lengths,
              float* contain_logp, float* seg_logp, int32_t* seg_start, int32_t* seg_end);
int hctr_spot_logits(hctr_ctx* ctx, const float* logits_wbc, int on_device, int W, int B, int C,
                     const int32_t* queries, const int32_t* query_lengths, int Q, const int32_t* input_lengths,
                     float* contain_logp, float* seg_logp, int32_t* seg_start, int32_t* seg_end);
int hctr_spot_automaton(const int32_t* query, int L, int32_t* classes, int32_t* num_classes, int32_t* delta,
                        int32_t* num_states, int32_t* in_ptr, int32_t* in_src, int32_t* in_slot, int edge_cap,
                        int32_t* num_edges, uint64_t* fall_mask);
int hctr_spot_chunk_classes(int lines, int W);

/* ---- lexicon recognition on the device: which entry of a closed list a line is, how surely, and the runners-up ------
 * Reading a field whose value comes from a list (place names, surnames, amounts, form options): the exact
 * log p(entry | line) of EVERY entry at once, by one CTC forward pass over the trie of the lexicon. The reference has
 * no counterpart. The free-text searches are pruned to each column's top-k classes and hctr_spot answers containment;
 * this answers "the whole line is this text", unpruned.
 * Lexicon: N >= 1 entries; entry e is a sequence of 1..HCTR_LEX_MAX_LEN labels in [1, C-1]; log_prior[e] float32,
 *   finite (NULL = 0). Duplicates are allowed and are separate entries.
 * Trie: node 0 is the root, plus one node per distinct non-empty prefix, numbered in the order in which inserting entry
 *   0, 1, .. first reaches them (a parent has a lower number than its children). Node v has label c_v and parent p_v.
 * States: every non-root node has n_v (the last column emitted c_v) and b_v (the last column was a blank after the
 *   prefix); the root has b_0 only.
 * Emissions: lp_t(c) = float32((double)z_t[c] - lse_t), the loss's, bit for bit. T = input_lengths[b] in [1, W], NULL = W.
 *   t = 0:  a(b_0) = lp_0(0);  a(n_v) = lp_0(c_v) for the children of the root;  -inf elsewhere
 *   t >= 1: a'(n_v) = logsum3(a(n_v), a(b_p), [p != root and c_p != c_v] a(n_p)) + lp_t(c_v)
 *           a'(b_v) = logsum3(a(b_v), a(n_v), -inf) + lp_t(0)             (the root: a(b_0), -inf, -inf)
 *   score[b][e] = logadd(a_{T-1}(b_v), a_{T-1}(n_v)) for v = the node where e ends
 * in float32 with the loss's log-sum of three sorted arguments and its argument order. Hence
 * - score[b][e] equals, bit for bit, -nll of hctr_ctc_loss_logits for line b with entry e as its target, and is -inf
 *   exactly where the loss reports +inf (L + adjacent equal labels > T);
 * - a pair's score bits depend on the line and the entry's own labels only: not on the other entries or their order, the
 *   partition into units, the chunking of classes, host or device pointers, repetition. There are no atomics.
 * Ranking: rank[b][e] = (double)score[b][e] + (double)log_prior[e]. The first n (1 <= n <= 32) entries in descending
 *   rank, ties to the lower entry index, entries with rank -inf left out: top_entry int32 [B][n], top_logp float32 [B][n]
 *   (their scores), top_rank float64 [B][n]; count[b] = how many were returned, the unused places hold -1 and -inf.
 *   log_total[b] = log sum_e exp(rank[b][e]) in float64 as max + log(sum of exp(rank - max)): 256 partial sums, the i-th
 *   over the entries i, i + 256, .. in ascending order, added up by a butterfly within each group of 64 (distances 32, 16,
 *   .., 1) and then (g0 + g1) + (g2 + g3) - an order that is a function of N alone; -inf if no entry fits. The posterior
 *   of an entry within the lexicon is exp(rank - log_total). scores: float32 [B][N], every score. All outputs are host
 *   pointers and any may be NULL.
 * hctr_lex_build (host only, no GPU, no context; errors are read with hctr_last_error(NULL)) builds the lexicon object:
 *   entries int32, back to back, sum(entry_lengths) labels; entry_lengths int32 [N]; unit_nodes = 0 for the default
 *   (4096), else in [128, 4096]. HCTR_ERR_ARG with a message for a label outside [1, C-1], a length outside [1, 64],
 *   N < 1, a non-finite prior, unit_nodes outside its range; HCTR_ERR_NOMEM; no exception crosses the ABI. The object
 *   is immutable and may serve any number of contexts; a context uploads its tables on first use, keeps the device copy
 *   of the lexicon it used last (recognised by a serial number, not by address) and frees it with the context.
 * Units: a unit is what one workgroup computes for one line: at most unit_nodes local nodes, local node 0 being the
 *   root, stored parents before children. It consists of whole subtrees plus a private copy of each subtree root's
 *   ancestor chain. Copies compute the same bits as the originals and only owned nodes report scores. The root's
 *   children are walked in label order: a subtree that fits an empty unit together with its chain goes into the open
 *   unit, or into a new one when the open one lacks the room; a larger subtree places its root alone and is split among
 *   its children, in label order, by the same rule.
 * hctr_lex_info: N, the trie's nodes (root included), units, distinct classes, the longest entry.
 * hctr_lex_tables exports what the kernel is given (any pointer may be NULL; call once for the totals):
 *   parent, label [nodes] (parent[0] = -1, label[0] = 0); entry_node [N];
 *   unit_off, class_off [units + 1]: unit u's local nodes are [unit_off[u], unit_off[u+1]), its classes
 *   [class_off[u], class_off[u+1]); unit_total = unit_off[units], class_total = class_off[units];
 *   unit_node [unit_total]: the trie node of a local node; unit_word [unit_total]: the index of its parent within the
 *   unit | HCTR_LEX_SKIP (n_p feeds n_v) | HCTR_LEX_FIRST (the parent is the root); unit_owned [unit_total]: 1 = owned,
 *   0 = a copy; unit_kidx [unit_total]: the place of the node's label in the unit's class list; unit_class
 *   [class_total]: per unit 0 (the blank), then its labels ascending; entry_ptr [unit_total + 1], entry_list [N]: the
 *   entries that end on an owned local node i are entry_list[entry_ptr[i] .. entry_ptr[i+1]), ascending.
 * Units are processed in chunks of consecutive units whose classes, blank included, number at most
 * hctr_lexicon_chunk_classes(lines, W) (what keeps the emissions within 4 GiB, at least 64 - every class of 64 lines x
 * 2000 columns x 7358 classes, so the emissions never exceed the logits' own size there; the environment variable
 * HCTR_LEX_CLASSES overrides it at every call; a single unit with more classes gets a chunk of its own); one pass over
 * the logits per chunk writes the emissions its units read, and a chunk's units run in one launch.
 * Errors of hctr_lexicon*: HCTR_ERR_ARG with a message for a NULL lex, a lexicon built for another C, n outside [1, 32],
 * an input length outside [1, W]; B == 0 is a no-op.
 * Device scratch (the context's grow-only CTC scratch; HCTR_ERR_NOMEM leaves the context usable): 4 * n*W*D emissions
 * (n = B, or the lines of one pass for images; D = the largest chunk's classes) + 4 * B*N scores + 4 * B*D class tables
 * + the ranking's results + 4 bytes per unit class; plus W*B*C floats for logits passed as a host pointer. The lexicon's
 * device copy (about 16 bytes per local node + 8 per entry) is separate.
 * Launches (hctr_last_profile): per chunk lexicon_classes, ctc_lse, lexicon_trie; then one lexicon_rank.
 * hctr_lexicon runs the forward of img in internal passes on the stored-logits head exactly as hctr_ctc_loss does: mode 0
 * f16, mode 1 f16x3, mode 2 EVERY line in f16x3, hctr_last_guard's figures left as they were. hctr_lexicon_logits takes
 * caller logits or log-probs in WBC layout, host or device pointer, and needs no weights. */
#define HCTR_LEX_MAX_LEN 64
#define HCTR_LEX_MAX_TOP 32
#define HCTR_LEX_SKIP (1 << 30)
#define HCTR_LEX_FIRST (1 << 29)
#define HCTR_LEX_PARENT_MASK 0xFFFF
typedef struct hctr_lex hctr_lex;
int hctr_lex_build(const int32_t* entries, const int32_t* entry_lengths, int N, int C, const float* log_prior,
                   int unit_nodes, hctr_lex** out);
void hctr_lex_free(hctr_lex* lex);
int hctr_lex_info(const hctr_lex* lex, int32_t* num_entries, int32_t* num_nodes, int32_t* num_units, int32_t* num_classes,
                  int32_t* max_len);
int hctr_lex_tables(const hctr_lex* lex, int32_t* parent, int32_t* label, int32_t* entry_node, int32_t* unit_off,
                    int32_t* class_off, int64_t* unit_total, int64_t* class_total, int32_t* unit_node, int32_t* unit_word,
                    uint8_t* unit_owned, int32_t* unit_kidx, int32_t* unit_class, int32_t* entry_ptr, int32_t* entry_list);
int hctr_lexicon(hctr_ctx* ctx, const hctr_lex* lex, const void* img, int img_dtype, int img_on_device,
                 const int32_t* widths, int B, int W, const int32_t* input_lengths, int n, int32_t* top_entry,
                 float* top_logp, double* top_rank, double* log_total, int32_t* count, float* scores);
int hctr_lexicon_logits(hctr_ctx* ctx, const hctr_lex* lex, const float* logits_wbc, int on_device, int W, int B, int C,
                        const int32_t* input_lengths, int n, int32_t* top_entry, float* top_logp, double* top_rank,
                        double* log_total, int32_t* count, float* scores);
int hctr_lexicon_chunk_classes(int lines, int W);

/* ---- word-sequence recognition on the device: the best segmentation of a line into lexicon entries ----------------
 * The line is a sequence of words from a closed vocabulary - which words, and where? Token passing over the lexicon's
 * trie with every word end looped back to the root, Viterbi (max) only: a sum over the looped trie would count a text
 * once per segmentation, the best path and its best segmentation are defined for any lexicon.
 * Inputs: a hctr_lex as hctr_lex_build makes it (only the global trie is used: parent, label, entry_node, the priors;
 * the partition into units plays no part); word_bonus, float32, finite: the word insertion bonus or penalty;
 * input_lengths as everywhere (T in [1, W], NULL = W).
 * Emissions: lp_t(c) = float32((double)z_t[c] - lse_t), the loss's, over the lexicon's distinct classes plus the blank.
 * Node weight: for a node v on which at least one entry ends, e_v is the entry with the largest log_prior among those
 * ending on v (ties to the lower index; no other can ever win), x_v = float32((double)log_prior[e_v] + (double)word_bonus).
 * States: b_0 (leading blanks, no word begun) and n_v, b_v for every non-root node as for hctr_lexicon. Each carries a
 * float32 score a and an origin (s, k): s the column at which the current word's first label was first emitted, k where
 * the word came from - 0 the line's start or b_0, 1 or 2 which exit record of column s - 1.
 * Exit records of column t, from the states after it: the candidates are (a(n_v) + x_v, last = c_v) and (a(b_v) + x_v,
 * last = 0) of every end node v, those at -inf left out; total order: score descending, then last == 0 first, then node
 * ascending. R1(t) is the best candidate, R2(t) the best whose last differs from R1(t).last. Each keeps score, node, last
 * and the winning state's origin. The pair is a mergeable summary: any reduction tree gives the same records.
 * Recursion, all float32, max then one add, the earlier-listed source winning equal scores:
 *   t = 0:  a(b_0) = lp_0(0); a(n_u) = lp_0(c_u), origin (0, 0), for the root's children u; -inf elsewhere
 *   root's children u:  pick = R1(t-1) if R1(t-1).last != c_u, else R2(t-1)
 *                       a'(n_u) = max(a(n_u), a(b_0), pick.score) + lp_t(c_u); the origin is kept from n_u, or becomes
 *                       (t, 0) from b_0, (t, 1|2) from the record
 *   deeper v, parent p: a'(n_v) = max(a(n_v), a(b_p), [c_p != c_v] a(n_p)) + lp_t(c_v), the origin copied from the winner
 *   a'(b_v) = max(a(b_v), a(n_v)) + lp_t(0);  a'(b_0) = a(b_0) + lp_t(0)
 * "pick skips a record whose last label equals c_u" is the CTC rule that two equal labels need a blank between them,
 * applied across the word boundary.
 * Result: score[b] = R1(T-1).score, -inf if there is no candidate. The words come from walking origins back from
 * R1(T-1): word e_v, origin (s, k) -> record k of column s - 1, until k = 0; word_start = s of each word. A word's span
 * is [its start, the next word's start), [start, T) for the last: inter-word blanks belong to the preceding word, leading
 * blanks to none. Outputs, host pointers, any may be NULL: score float32 [B]; count int32 [B], the true number of words
 * even beyond max_words; words, starts int32 [B][max_words], the first min(count, max_words) words in line order, unused
 * places -1; labels [B][W] / lengths [B], the concatenated text (unused places 0); text_nll float32 [B], the CTC loss of
 * that text on the same emissions by the loss's kernels as hctr_pattern does for its reading (NaN for a text beyond the
 * loss's labels), so exp(-text_nll) is the text's posterior.
 * Masked and non-finite logits as stated above: a -inf beside a finite logit is probability 0; a line with a non-finite
 * row inside its length returns count 0, score -inf, text_nll +inf (a NaN state wins no comparison and is no candidate),
 * other lines are untouched, and no index is derived from a logit.
 * Limits and errors: 1 <= max_words <= W; the trie has at most HCTR_WORDS_MAX_NODES nodes (the root included), a larger
 * one is refused with HCTR_ERR_ARG and a message naming both numbers; a NULL lex, a lexicon built for another C, a
 * non-finite word_bonus, an input length outside [1, W]: HCTR_ERR_ARG with a message. B == 0 is a no-op.
 * HCTR_ERR_NOMEM leaves the context usable.
 * hctr_lex_word_tables (host only) exports what the kernel is given, [num_nodes] each: node = parent | HCTR_LEX_SKIP |
 * HCTR_LEX_FIRST; slot = the place of the node's label in classes; entry = e_v or -1; weight = x_v (0 where no entry
 * ends); classes [num_classes] = 0 (the blank), then the distinct labels ascending. Any pointer may be NULL.
 * Two storage forms with the same bits: tries of up to HCTR_WORDS_LDS_NODES nodes keep the two step buffers in LDS,
 * larger ones (and every one under HCTR_WORDS_LDS=0, read at every call) in the call's scratch. Lines run in groups that
 * keep emissions, records and step buffers within 4 GiB (HCTR_WORDS_LINES overrides the group's lines).
 * Launches (hctr_last_profile): lexicon_classes, then per group ctc_lse, words_trie, words_backtrace and, for text_nll,
 * ctc_alpha. hctr_words runs the forward of img in internal passes exactly as hctr_lexicon does (mode 0 f16, mode 1
 * f16x3, mode 2 EVERY line in f16x3, hctr_last_guard's figures left as they were); hctr_words_logits takes caller logits
 * or log-probs in WBC layout, host or device pointer, and needs no weights. */
#define HCTR_WORDS_MAX_NODES 65536
#define HCTR_WORDS_LDS_NODES 4096
int hctr_lex_word_tables(const hctr_lex* lex, float word_bonus, int32_t* num_nodes, int32_t* num_classes, int32_t* node,
                         int32_t* slot, int32_t* entry, float* weight, int32_t* classes);
int hctr_words(hctr_ctx* ctx, const hctr_lex* lex, const void* img, int img_dtype, int img_on_device,
               const int32_t* widths, int B, int W, const int32_t* input_lengths, float word_bonus, int max_words,
               float* score, int32_t* count, int32_t* words, int32_t* starts, int32_t* labels, int32_t* lengths,
               float* text_nll);
int hctr_words_logits(hctr_ctx* ctx, const hctr_lex* lex, const float* logits_wbc, int on_device, int W, int B, int C,
                      const int32_t* input_lengths, float word_bonus, int max_words, float* score, int32_t* count,
                      int32_t* words, int32_t* starts, int32_t* labels, int32_t* lengths, float* text_nll);

/* ---- pattern-constrained recognition on the device: CTC over a deterministic finite automaton ----------------------
 * Reading a field whose admissible texts form an open set with a known shape (a date, an identity number, a phone
 * number, an amount, a plate): the probability that the line's text matches the pattern - an exact sum over all CTC
 * paths - and the best reading that matches it, with character spans and confidences. The reference has no
 * counterpart. Spotting (one string's KMP automaton) and the lexicon (a trie) are special cases of this.
 * Pattern: a DFA over labels. States 0..nQ-1, state 0 the start; arcs (src, label, dst) with label in [1, C-1] and at
 *   most one arc per (src, label); a set of final states. L(A) = the label sequences that drive it from state 0 to a
 *   final state (the empty sequence iff state 0 is final).
 * hctr_pat_build (host only, no GPU, no context; errors are read with hctr_last_error(NULL)) validates determinism, the
 *   label range, the state range and num_states >= 1, and prunes the DFA states that are not both reachable from state 0
 *   and able to reach a final state (with their arcs); the survivors keep their relative order and state 0 is kept.
 *   HCTR_ERR_ARG with a message for each of those, for an empty language, for more than HCTR_PAT_MAX_STATES CTC states
 *   and for more than HCTR_PAT_MAX_EDGES edges (the message names the figure); HCTR_ERR_NOMEM; no exception crosses the
 *   ABI. The object is immutable and may serve any number of contexts; a context uploads its tables on first use, keeps
 *   the device copy of the pattern it used last (recognised by a serial number, not by address) and frees it with the
 *   context.
 * CTC states (after pruning): one blank state beta_q = q per DFA state q; one emitting state eps_(q,c) per distinct
 *   (destination q, label c) among the arcs, numbered nQ, nQ + 1, .. in ascending (q, c) - arcs (p,c,q) and (p',c,q)
 *   share it, their futures being identical. S = nQ + #pairs. label(beta_q) = 0, label(eps_(q,c)) = c.
 * In-edges, each state's list sorted by source index ascending (the order in which the kernel visits them):
 *   beta_q    <- beta_q and every eps_(q,.)
 *   eps_(q,c) <- itself; beta_p for every arc (p,c,q); for each such p every eps_(p,c') with c' != c
 * Start list: beta_0 and every eps_(q,c) with an arc (0,c,q), ascending. Accepting list: beta_q and every eps_(q,.) for
 *   every final q, ascending.
 * Emissions: lp_t(c) = float32((double)z_t[c] - lse_t), the loss's, bit for bit. T = input_lengths[b] in [1, W], NULL = W.
 *   t = 0:  a_0(s) = v_0(s) = lp_0(label(s)) for the states of the start list, -inf elsewhere
 *   t >= 1: a_t(s) = logsum over the in-edges of a_{t-1}(src) + lp_t(label(s))
 *           v_t(s) = max    over the in-edges of v_{t-1}(src) + lp_t(label(s)); the backpointer is the first maximal
 *           source in edge order, and the state's own index when every source is at -inf
 *   logp[b]      = logsum of a_{T-1} over the accepting list, in list order: the log of the summed probability of every
 *                  CTC path whose collapse is in L(A)
 *   best_logp[b] = max of v_{T-1} over the accepting list, ties to the lowest state: the best such path
 * Arithmetic: states are float32. logsum of x_1..x_n (in the order given): m = the float32 maximum; -inf if m is -inf;
 *   else sum = the float64 sum, in that order, of (double)exp32(x_i - m), where x_i - m is a float32 subtraction and
 *   exp32 the device's fast float32 exponential (the loss's); the result is the float32 sum m + log32((float)sum) with
 *   the device's fast float32 logarithm. The emission is then added in float32. The max-plus recursion is exact float32
 *   additions. logp[b] is returned as 0 where the final float32 sum rounds above 0 (a pattern that nearly every text of
 *   the line matches): best_logp <= logp <= 0 always.
 *   No atomics; every reduction runs in the order stated. Because the automaton is deterministic every
 *   accepted text has one arc sequence and every CTC path one state sequence: both recursions are exact.
 *   Hence a pair's bits are a function of its line and the pattern's tables only: not of the other lines, the grouping
 *   of lines (below), host or device pointers, repetition, or how the pattern was spelt when the tables are equal.
 * Viterbi outputs (all host pointers, any may be NULL; when every one of best_logp .. text_nll is NULL the call runs the
 *   sum alone, stores no backpointers, and logp has the bits of the full call's):
 *   path int32 [B][W]: the class of the best accepted path per column, -1 for t >= T;
 *   labels int32 [B][W], lengths int32 [B]: its collapse, the decoded text, which is in L(A) (zeros beyond lengths[b]);
 *   span_start, span_end int32 [B][W], char_logp float32 [B][W]: per character its first column, the column after its
 *   run, and the float32 sum of lp over the run in ascending t - layout and meaning of hctr_recognize: the first
 *   lengths[b] valid, the rest zeros;
 *   text_nll float32 [B]: the CTC loss of the decoded labels on the same logits, with the bits of
 *   hctr_ctc_loss_logits given them as targets (the existing ctc_alpha over the pattern's own emissions);
 *   NaN for a text longer than the loss's 2047 labels. exp(-text_nll - logp) is the posterior of the best text within
 *   the pattern.
 * No accepted path of length T (for example eight digits on 5 columns): logp = best_logp = -inf, path = -1 in every
 *   column, lengths = 0, text_nll = +inf.
 * hctr_pat_info: DFA states after pruning, CTC states S, edges E, distinct classes, the largest in-degree.
 * hctr_pat_tables exports exactly what the kernel is given (any pointer may be NULL; call once for the counts):
 *   state_label, state_slot int32 [S] (slot = the place of the label in the ascending class list, blank = 0);
 *   in_ptr int32 [S + 1], in_src uint16 [E]; classes int32 [distinct classes]; accept int32 [num_accept];
 *   start int32 [num_start].
 * Lines are processed in groups of hctr_pattern_group_lines(S, D, W) lines, D = classes + 1: what keeps a group's
 * emissions (4*W*D bytes a line) and backpointers (2*W*S bytes a line) within 2 GiB, at least 1; the environment
 * variable HCTR_PAT_LINES overrides it at every call. Results do not depend on it, bit for bit.
 * Errors of hctr_pattern*: HCTR_ERR_ARG with a message for a NULL pat, a pattern built for another C, an input length
 * outside [1, W]; B == 0 is a no-op. HCTR_ERR_NOMEM leaves the context usable.
 * Device scratch (the context's grow-only CTC scratch): per group 4*g*W*D emissions + 2*g*W*S backpointers + 8*g*W;
 * 20*B*W for the per-column results, 4*B*D class tables; plus W*B*C floats for logits passed as a host pointer. The
 * pattern's device copy (12 bytes per state + 2 per edge) is separate.
 * Launches (hctr_last_profile): pattern_classes; per group ctc_lse, pattern, and with Viterbi outputs pattern_trace and,
 * for text_nll, ctc_alpha.
 * hctr_pattern runs the forward of img in internal passes on the stored-logits head exactly as hctr_lexicon does: mode 0
 * f16, mode 1 f16x3, mode 2 EVERY line in f16x3, hctr_last_guard's figures left as they were. hctr_pattern_logits takes
 * caller logits or log-probs in WBC layout, host or device pointer, and needs no weights.
 *
 * THE SET FORM (hctr_pat_build_sets): arcs (src, set, dst) that carry label sets - a wildcard, a negated class, a name
 * field over the whole vocabulary - without the explicit edge list, whose size is what refuses such patterns above.
 *   Set k is set_labels[set_ptr[k] .. set_ptr[k + 1]): non-empty, labels ascending, in [1, C-1]. The sets of the arcs that
 *   leave one state are pairwise disjoint (determinism); several arcs between one pair of states are allowed.
 *   The language, the pruning, the CTC states and their numbering (beta_q = q, then eps_(q,c) in ascending (q, c)), the
 *   start and accepting states, the emissions and the meaning of every output are exactly those of hctr_pat_build on the
 *   same automaton with every arc expanded into single-label arcs. Only the tables and the order of the sums differ.
 *   The object is the same hctr_pat: hctr_pat_kind tells the forms apart, hctr_pattern* dispatch on it, hctr_pat_free
 *   frees both. Errors as hctr_pat_build's, one message each: an empty set, a label out of range, labels not ascending,
 *   an arc that names no set or no state, overlapping sets leaving one state, an empty language, an exceeded limit
 *   (the message names the figure).
 * Limits (nothing is approximated: a pattern beyond one is refused): HCTR_PATSET_MAX_STATES = 65535 CTC states (eight
 *   full-vocabulary positions; backpointers stay uint16), HCTR_PATSET_MAX_DFA_STATES = 4096 DFA states after pruning (the
 *   block totals of a step live in LDS, 40 bytes a block), HCTR_PATSET_MAX_INARCS = 1048576 entries of the reduced
 *   in-arc table: one entry per (state eps_(q,c), source DFA state p with an arc (p, A, q), c in A).
 * hctr_pat_info on a set pattern: dfa_states, ctc_states and num_classes as above; num_edges = the entries of the
 *   reduced in-arc table; max_in_degree = the most entries one state has (the most DFA states that feed one eps state).
 *   hctr_pat_tables on a set pattern returns HCTR_ERR_ARG: the edge list is what this form never builds.
 * The recursion in block form. The block of DFA state p is beta_p and every eps_(p,.). A state is fed by whole blocks
 *   less at most one state each: beta_q by block q; eps_(q,c) by itself and, for every arc (p, A, q) with c in A, by
 *   block p without eps_(p,c) (where the block holds such a state). Work per step is O(S + in-arcs).
 *   Block totals over a_{t-1}, per block p: its members in ascending state order are beta_p, then its eps states. Lane l
 *   of 64 takes the members l, l + 64, l + 128, .. in that order; the 64 lanes then combine by the butterfly over the lane
 *   distances 32, 16, 8, 4, 2, 1 (lane l with lane l xor d). m_p = the float32 maximum; i*_p = the lowest state that
 *   holds it; all_p = the float64 sum of (double)exp32(a - m_p) over the members, rest_p = the same sum without i*_p
 *   (both 0 where m_p is -inf). The order is a function of the tables alone: not of the thread count, of where the step
 *   buffers live, or of the grouping of lines.
 *   Tot_p = m_p + log32((float)all_p), -inf where m_p is. The source term of eps_(q,c) from block p is
 *   y = m_p + log32((float)X) with X = rest_p where eps_(p,c) is i*_p; all_p - (double)exp32(a(eps_(p,c)) - m_p) where
 *   eps_(p,c) exists and is not i*_p (the maximal term survives the subtraction: nothing cancels); all_p where it does
 *   not exist; y = -inf where X <= 0 or m_p is -inf.
 *   a_t(beta_q) = Tot_q + lp_t(0). a_t(eps_(q,c)) = the logsum above (the explicit form's n-ary logsum) over [its own
 *   a_{t-1}, then y of each in-arc in ascending p] + lp_t(c). logp[b] = that logsum over Tot_q of the final q, ascending,
 *   returned as 0 where it rounds above 0. logp is within the family's rule of the explicit form's, not bit-equal.
 *   Max: per block the two best v_{t-1} with their states, ties to the lower state. The candidate of block p for
 *   eps_(q,c) is the best, or the runner-up where the best is eps_(p,c) itself; among the own value and the candidates
 *   the greatest wins, ties to the lowest state; all at -inf: the state's own index. That is the explicit form's first
 *   maximal source in ascending order and the additions are exact, so best_logp, path, labels, lengths, span_start,
 *   span_end, char_logp and text_nll have the explicit form's bits wherever both forms build.
 *   When every Viterbi output is NULL the sum runs alone and logp has the full call's bits.
 * One workgroup per line, no atomics, no workgroup waits on another. The two step buffers of (a, v) live in LDS when
 *   they fit beside the block totals (16*S + 40*nQ <= 160 KB; 8*S + 24*nQ forward-only), else in the context's CTC
 *   scratch; the environment variable HCTR_PATSET_LDS=0, read at every call, keeps them in scratch. Results do not
 *   depend on it, bit for bit. hctr_pattern_group_lines is unchanged. Device scratch as above, plus 16*g*S for the step
 *   buffers kept out of LDS; the device copy is 20 bytes per state + 4 per DFA state + 4 per in-arc. Launches:
 *   pattern_set in the place of pattern.
 *
 * WEIGHTED ARCS (hctr_pat_build_weighted, hctr_pat_kind == 2): one float32 weight per arc and per final state - a prior
 * over the pattern's texts (a character bonus, a bigram, log priors of alternatives). The automaton is deterministic,
 * so a text has one arc sequence and one weight: w(text) = the sum of the weights of the arcs it takes plus the weight
 * of the final state it ends in.
 *   logp[b]      = log of the sum over the texts of L(A) of p(text | line) * exp(w(text)): no probability, and not
 *                  clamped to 0;
 *   best_logp[b] = the best accepted path's log-probability plus the weight of its text; best_logp <= logp still.
 *   Validation, pruning, CTC states, numbering, in-edges, accepting list, start list and the limits are hctr_pat_build's
 *   on the same arcs: hctr_pat_tables returns the tables of the kind-0 pattern of that automaton, byte for byte.
 *   arcs_weight == NULL or final_weight == NULL means zeros. Every weight must be finite: NaN, +inf and -inf are
 *   refused (an arc that cannot be taken is left out); a final state listed twice with different weights is refused.
 *   Every error of hctr_pat_build and these, one message each, under the prefix "hctr_pat_build_weighted:".
 * hctr_pat_weights exports what the kernel is given beside the tables (any pointer may be NULL):
 *   in_w float32 [E], parallel to in_src: for a state eps_(q,c) and a source beta_p or eps_(p,c'), the weight of arc
 *   (p,c,q) - every source belongs to one DFA state p, so this is one value even where several arcs share eps_(q,c); 0
 *   for a state's self edge and for every in-edge of a beta state;
 *   accept_w float32 [num_accept]: the final weight of the DFA state the accepting state belongs to;
 *   start_w float32 [num_start]: 0 for beta_0, the weight of arc (0,c,q) for eps_(q,c).
 *   Weights on pruned arcs and states are dropped. HCTR_ERR_ARG on a pattern of kind 0 or 1.
 * hctr_pat_text_weight: *w = the float64 sum, in text order, of the float32 weights of the arcs the n labels take from
 *   state 0, plus the final weight of the state reached; -inf (with HCTR_OK) for a text outside L(A). HCTR_ERR_ARG on a
 *   pattern of kind 0 or 1.
 * Arithmetic (the recursion, the order of every reduction and the tie rules are the explicit form's above):
 *   t = 0:  a_0(s) = v_0(s) = lp_0(label(s)) + start_w(s), one float32 addition, on the start list;
 *   t >= 1: x_j = a_{t-1}(src_j) + in_w[j], one float32 addition per in-edge; a_t(s) = the logsum above over the x_j
 *           in edge order (float32 max, float64 sum of (double)exp32(x_j - m), m + log32((float)sum)) + lp_t(label(s));
 *           v_t(s) = max_j (v_{t-1}(src_j) + in_w[j]) + lp_t(label(s)), the backpointer the first maximal edge, the
 *           state's own index when every source is at -inf;
 *   end:    the logsum and the max over a_{T-1}(s) + accept_w(s), v_{T-1}(s) + accept_w(s) in list order, ties to the
 *           lowest state.
 *   With every weight 0 every output has the bits of the kind-0 pattern's, except that logp is not clamped.
 *   path .. char_logp describe the best weighted path; char_logp stays the sum of emissions and text_nll the plain CTC
 *   loss of the decoded text: exp(-text_nll + w(text) - logp) is the text's posterior under the weights.
 * The edge weights are staged in LDS beside the edge list when 2*S*(8 or 4) + 6*E <= 160 KB, else read through L2 (the
 *   edge list alone stays in LDS where it fits as for kind 0). Results do not depend on it. The device copy grows by 4
 *   bytes per edge, accepting state and start state. Launches: pattern_w in the place of pattern. Grouping,
 *   HCTR_PAT_LINES, scratch and the errors of hctr_pattern* are unchanged.
 * Masked and non-finite logits: as stated above for hctr_pattern_logits, for every form. */
#define HCTR_PAT_MAX_STATES 8192
#define HCTR_PAT_MAX_EDGES 262144
typedef struct hctr_pat hctr_pat;
int hctr_pat_build(const int32_t* arcs_src, const int32_t* arcs_label, const int32_t* arcs_dst, int num_arcs,
                   const int32_t* finals, int num_finals, int num_states, int C, hctr_pat** out);
#define HCTR_PATSET_MAX_STATES 65535
#define HCTR_PATSET_MAX_DFA_STATES 4096
#define HCTR_PATSET_MAX_INARCS 1048576
int hctr_pat_build_sets(const int32_t* arcs_src, const int32_t* arcs_set, const int32_t* arcs_dst, int num_arcs,
                        const int32_t* set_ptr, const int32_t* set_labels, int num_sets, const int32_t* finals,
                        int num_finals, int num_states, int C, hctr_pat** out);
int hctr_pat_build_weighted(const int32_t* arcs_src, const int32_t* arcs_label, const int32_t* arcs_dst,
                            const float* arcs_weight, int num_arcs, const int32_t* finals, const float* final_weight,
                            int num_finals, int num_states, int C, hctr_pat** out);
int hctr_pat_weights(const hctr_pat* pat, float* in_w, float* accept_w, float* start_w);
int hctr_pat_text_weight(const hctr_pat* pat, const int32_t* labels, int n, double* w);
/* 0 = hctr_pat_build's, 1 = hctr_pat_build_sets's, 2 = hctr_pat_build_weighted's; HCTR_ERR_ARG for NULL */
int hctr_pat_kind(const hctr_pat* pat);
void hctr_pat_free(hctr_pat* pat);
int hctr_pat_info(const hctr_pat* pat, int32_t* dfa_states, int32_t* ctc_states, int32_t* num_edges, int32_t* num_classes,
                  int32_t* max_in_degree);
int hctr_pat_tables(const hctr_pat* pat, int32_t* state_label, int32_t* state_slot, int32_t* in_ptr, uint16_t* in_src,
                    int32_t* classes, int32_t* num_accept, int32_t* accept, int32_t* num_start, int32_t* start);
int hctr_pattern(hctr_ctx* ctx, const hctr_pat* pat, const void* img, int img_dtype, int img_on_device,
                 const int32_t* widths, int B, int W, const int32_t* input_lengths, float* logp, float* best_logp,
                 int32_t* path, int32_t* labels, int32_t* lengths, int32_t* span_start, int32_t* span_end,
                 float* char_logp, float* text_nll);
int hctr_pattern_logits(hctr_ctx* ctx, const hctr_pat* pat, const float* logits_wbc, int on_device, int W, int B, int C,
                        const int32_t* input_lengths, float* logp, float* best_logp, int32_t* path, int32_t* labels,
                        int32_t* lengths, int32_t* span_start, int32_t* span_end, float* char_logp, float* text_nll);
int hctr_pattern_group_lines(int S, int D, int W);
/* the kernel instance an explicit (weighted != 0: a weighted) pattern of S CTC states and E edges runs, a pure function:
 * states per thread (1, 2, 4 or 8) | 16 where the edge list is staged in LDS | 32 where the edge weights are too;
 * HCTR_ERR_ARG beyond the limits. For tests that mean to reach one instance. */
int hctr_pattern_instance(int S, int E, int viterbi, int weighted);

/* ---- greedy recognition: the decoded text with per-character spans, confidences and runners-up -------------------
 * What hctr_greedy / hctr_decode_greedy_logits decode, plus the figures the CTC family above gives only for a
 * transcription the caller already knows - in one pass over the logits, without a Viterbi recursion: the greedy path is
 * itself a CTC path. The reference has no counterpart. All W columns of every line count, pad columns included, exactly
 * as the greedy decode takes them; there is no input_lengths.
 * For row (t, b) with logits z over C classes:
 *   k1  = the argmax in np.argmax's order (the first maximum wins, a NaN counts as the maximum);
 *   k2  = the first index of the largest logit among the classes c != k1;
 *   lse = the row's log-sum-exp with the loss's arithmetic, bit for bit (float32 running max, float64 exp-sum and log);
 *   lp1 = (float)((double)z[k1] - lse), lp2 likewise for k2.
 * A column t is kept iff k1 != 0 && k1 != C-1 && k1 != k1[t-1] (the previous column is compared raw, as the greedy
 * decode does). Character j of line b has the label k1[s_j] of its kept column s_j and the span [s_j, e_j), e_j being the
 * first t > s_j with k1[t] != label, or W.
 * Outputs are host pointers and any may be NULL; the per-character arrays are [B][W] like labels, the first lengths[b]
 * entries of a line valid (the rest are written as zeros):
 *   labels, lengths:      identical to hctr_decode_greedy_logits on the same logits;
 *   span_start, span_end: int32, s_j and e_j;
 *   char_logp:            float32, the sum of lp1[t] over the span, ascending t, in float32 (exp(char_logp / (end - start))
 *                         is the geometric-mean probability, the confidence, as for hctr_ctc_align's span_logp);
 *   alt_label, alt_logp:  int32 / float32, k2 and lp2 at the span's peak column (the t with the largest lp1, the first
 *                         on ties): the likeliest substitution;
 *   path_logp:            float32 [B], the sum of lp1[t] over all W columns in a fixed order: the greedy path's log-prob;
 *   text_nll:             float32 [B], the CTC loss of the decoded labels on these logits, bit-identical to
 *                         hctr_ctc_loss_logits with labels / lengths as targets and input_lengths = NULL
 *                         (exp(-text_nll) is the posterior of the text; >= exp(path_logp) unless a column decodes to C-1,
 *                         which the collapse drops but the loss does not take for a blank). A line whose decoded length
 *                         exceeds the loss's 2047 labels gets NaN, not an error. NULL skips the loss part entirely.
 * A row holding a NaN: labels as the greedy decode gives them; the float figures of a character whose span holds such a
 * row, and that line's path_logp / text_nll, are NaN (text_nll's bit-identity with the loss is for the other lines: the
 * loss's recursion drops a NaN emission); alt_label there is unspecified. A row with +inf, or with nothing but -inf,
 * has a NaN log-sum-exp and counts as such a row.
 * No atomics: repeated calls, and host-pointer / device-pointer calls, agree bit for bit.
 * hctr_recognize runs the forward of img (arguments as hctr_greedy) with the stored-logits head in internal passes,
 * exactly as hctr_ctc_loss / hctr_ctc_align do: mode 0 f16, mode 1 f16x3, mode 2 EVERY line in f16x3 (the margin
 * certificate bounds argmax flips, not confidences), hctr_last_guard's figures left as they were. In modes 0 and 1 the
 * labels equal hctr_greedy's. hctr_recognize_logits takes caller logits or log-probs in WBC layout, host or device
 * pointer, and needs no weights (a context made for ctc_codec serves). Errors, B == 0 (a no-op) and HCTR_ERR_NOMEM as in
 * the family: the context stays usable.
 * Launches (hctr_last_profile): greedy_rowstat (one 256-thread block per row: argmax, runner-up and log-sum-exp in one
 * read), greedy_spans (one block per line), then for text_nll ctc_emis_gather (the emissions of the decoded text from
 * the kept log-sum-exps: D values read per row) and ctc_alpha.
 * Device scratch (the context's grow-only CTC scratch; n = B, or the lines of one pass for images):
 *   8 * n*W (log-sum-exps) + max(40 * n*W + 8 * n (row figures and spans), the loss's tables + 4 * n + 4 * n*W*D
 *   (emissions of the decoded text, D = the largest number of distinct classes of a line, blank included)), each array
 *   rounded up to 256 bytes; plus W*B*C floats for logits passed as a host pointer. D is known only once the text is
 *   decoded: when the second layout outgrows the block, the log-sum-exps are copied to a larger one, and for the length
 *   of that copy both blocks exist (a transient peak of old + new bytes, paid by the first call at a larger shape; if
 *   the larger block cannot be had, HCTR_ERR_NOMEM leaves the old one and the context as they were). */
int hctr_recognize(hctr_ctx* ctx, const void* img, int img_dtype, int img_on_device, const int32_t* widths, int B, int W,
                   int32_t* labels, int32_t* lengths, int32_t* span_start, int32_t* span_end, float* char_logp,
                   int32_t* alt_label, float* alt_logp, float* path_logp, float* text_nll);
int hctr_recognize_logits(hctr_ctx* ctx, const float* logits_wbc, int on_device, int W, int B, int C,
                          int32_t* labels, int32_t* lengths, int32_t* span_start, int32_t* span_end, float* char_logp,
                          int32_t* alt_label, float* alt_logp, float* path_logp, float* text_nll);

/* ---- evaluation: edit distance of a decoded text against its transcription, on the device -----
 * The reference's figure of merit, editdistance.eval(pre, tru) per line and CER = total edits / total characters
 * (test.py:266-285, main.py:506), with the breakdown its paper reports: substitutions, deletions, insertions and which
 * reference character went with which decoded character. Everything is int32 and exact.
 * For a reference r_1..r_L and a hypothesis h_1..h_H (int32 symbols of any value, compared with ==):
 *   D[i][0] = i, D[0][j] = j, D[i][j] = min(D[i-1][j-1] + (r_i != h_j), D[i-1][j] + 1, D[i][j-1] + 1);  edits = D[L][H].
 * The path is walked back from (L, H), ties decided in this order (part of the contract): the diagonal if i > 0, j > 0
 * and D[i][j] == D[i-1][j-1] + (r_i != h_j) - a hit when the symbols are equal, else a substitution; else a deletion
 * (r_i has no counterpart) if i > 0 and D[i][j] == D[i-1][j] + 1; else an insertion (h_j is spurious).
 * hctr_edit_distance: hyp is [B][hyp_stride] with the first hyp_lengths[b] entries of a line valid (the layout
 * hctr_greedy returns, hyp_stride = W); ref holds the lines' symbols back to back, ref_lengths[b] each (what
 * codec.encode returns). All pointers are host pointers. Outputs, any may be NULL:
 *   edits:   int32 [B];
 *   counts:  int32 [B][4] = {hits, substitutions, deletions, insertions}; hits + S + D = L, hits + S + I = H,
 *            S + D + I = edits;
 *   ref_map: int32 [sum L], in the order of ref: the 0-based position in the line's hypothesis the reference character
 *            is aligned with (hit or substitution), -1 for a deletion;
 *   hyp_map: int32 [B][hyp_stride]: the 0-based position in the line's reference, -1 for an insertion; entries beyond
 *            hyp_lengths[b] are written as zeros.
 * With counts, ref_map and hyp_map all NULL the distance-only instance runs and no backpointer scratch is taken; edits
 * is the same either way. Limits: every ref_lengths[b] in [0, 2047] (the family's limit), hyp_lengths[b] in
 * [0, hyp_stride]; anything else, a NULL hyp, hyp_lengths or ref_lengths (or ref where sum L > 0) with B > 0, is
 * HCTR_ERR_ARG with a message naming the line. B == 0 is a no-op. Needs no weights (a context made for ctc_codec
 * serves) and knows nothing of classes.
 * hctr_evaluate takes img .. W as hctr_greedy does and decodes exactly as hctr_greedy decodes - the mode's own
 * arithmetic, in mode 2 the guard sweep and the f16x3 re-run of the flagged lines; labels / lengths (either may be
 * NULL, labels only together with lengths) are identical to hctr_greedy's in all three modes and hctr_last_guard
 * advances as it does there. targets / target_lengths are the references (ids are not checked against the classes
 * here: they are compared, never used as an index). They are uploaded once; inside each pass, after ctc_collapse, the
 * edit kernels run on the pass's decoded labels where they lie on the device, and the results of re-run lines replace
 * the first sweep's. The maps' hyp_stride is W.
 * hctr_evaluate_logits is hctr_decode_greedy_logits on caller logits (WBC, host or device pointer) plus the same
 * stage; it needs no weights, and its targets follow hctr_ctc_loss_logits' check: ids in [1, C-1].
 * No atomics: repeated calls agree bit for bit. HCTR_ERR_NOMEM leaves the context usable.
 * Launches (hctr_last_profile): edit_distance (one workgroup per line: the lane-skewed sweep, lane k on reference rows
 * k*NS+1 .. k*NS+NS and, at step d, on hypothesis column d - k + 1, H + ceil(L/NS) - 1 steps; instances NS x waves of
 * 1x1, 2x1, 2x2, 2x4, 2x8, 4x8, the first whose 64*NS*waves rows hold the longest reference of the call) and, unless
 * distance-only, edit_backtrace (one 256-thread workgroup per line); hctr_evaluate* after their decode's launches.
 * Device scratch (the context's grow-only CTC scratch; n = B, for hctr_evaluate the lines of one pass):
 *   8 * B + 4 * sum L (references) + 8 * B (edits, re-run line numbers), and unless distance-only 16 * B + 4 * sum L +
 *   4 * B * hyp_stride + 8 * B (counts, maps, backpointer offsets) plus the backpointers of the n lines that need most:
 *   per line (H + lanes - 1) * lanes bytes with lanes = ceil(L / NS) - about L*H/NS, L*H/4 at the last instance - where
 *   H is hyp_lengths[b], for hctr_evaluate* W (the decoded length is known on the device only); hctr_edit_distance adds
 *   4 * B * hyp_stride + 4 * B for the hypotheses, hctr_evaluate_logits 8 * W*B + 4 * B for its decode (and W*B*C floats
 *   for logits passed as a host pointer). Each array is rounded up to 256 bytes. */
int hctr_edit_distance(hctr_ctx* ctx, const int32_t* hyp, const int32_t* hyp_lengths, int hyp_stride,
                       const int32_t* ref, const int32_t* ref_lengths, int B,
                       int32_t* edits, int32_t* counts, int32_t* ref_map, int32_t* hyp_map);
int hctr_evaluate(hctr_ctx* ctx, const void* img, int img_dtype, int img_on_device, const int32_t* widths, int B, int W,
                  const int32_t* targets, const int32_t* target_lengths,
                  int32_t* labels, int32_t* lengths,
                  int32_t* edits, int32_t* counts, int32_t* ref_map, int32_t* hyp_map);
int hctr_evaluate_logits(hctr_ctx* ctx, const float* logits_wbc, int on_device, int W, int B, int C,
                         const int32_t* targets, const int32_t* target_lengths,
                         int32_t* labels, int32_t* lengths,
                         int32_t* edits, int32_t* counts, int32_t* ref_map, int32_t* hyp_map);

/* ---- N-best texts with scores: the CTC prefix beam search without a language model, on the device -------------
 * The search of utils/ctc_codec.py:212-285 (__context_beam_search__) with a language model that scores everything 0 -
 * what hctr_beam_search does per step with builtin_lm == 1 - run where the front end's lists lie, over a caller-chosen
 * number of steps and without the greedy end-step / empty-line rules of __cbs_full__; it returns the first nbest
 * hypotheses of the final list with their log-probabilities instead of one string. An N-best list is what rescoring with
 * any language model needs (N calls per line); the n-gram-scored search on the device is hctr_nbest_lm* below, every
 * other LM-scored search stays on the host (hctr_beam_search).
 * Input per row (t, b): k classes in descending log-prob order (ties: lower index first), distinct, with float32
 * log-probs - hctr_beam_frontend's topk_idx / topk_logp. Line b runs T_b = input_lengths[b] steps, in [1, W]; NULL = W
 * for every line (all columns count, pad columns included, as in hctr_greedy and hctr_recognize).
 * Per line the state is an ordered list of at most `beam` hypotheses (prefix, pb, pnb) in float64, at first
 * [((), 0, -inf)]. Step t:
 *   1. pairs (i, j) are taken in lexicographic order, hypothesis i in list order, candidate j in list order; candidates
 *      with class >= C-1 (<unknown>) are skipped;
 *   2. with tot = logaddexp(pb, pnb), tail = the prefix's last label (or none) and the candidate's class c and log-prob
 *      l (widened to float64), the pair touches the entry of prefix and
 *        c == 0:     pb'(prefix) (+)= tot + l;
 *        c != tail:  touches prefix+c, pnb'(prefix+c) (+)= tot + l;
 *        c == tail:  touches prefix+c, pnb'(prefix+c) (+)= pb + l and pnb'(prefix) (+)= pnb + l;
 *      (+)= is logaddexp into an accumulator that starts at -inf (numpy's formula; logaddexp(-inf, -inf) = -inf, never
 *      NaN); entries are keyed by the label string, equal strings are one entry;
 *   3. the entries stand in first-touch order: an entry's position is that of the first pair that touched it, within a
 *      pair the prefix's own entry before the extension (Python dict insertion order, the gen vector of beam_step);
 *   4. they are sorted STABLY, descending, by total = logaddexp(pb', pnb') + len(prefix) * len_bonus and the first `beam`
 *      survive; an entry whose total is -inf sorts last but may survive if there is room;
 *   5. the blank takes part only when it is among the row's k classes (the reference's rule).
 * After T_b steps the first nbest hypotheses are the result, in that order; the tie rule of 3-4 is part of the contract.
 * Identity by label string is decided with a fingerprint (length, 64-bit hash of the labels) per hypothesis: two
 * different strings of one length in one list are taken for equal with probability 2^-64 per pair, below 1e-11 for a
 * whole call of 64 lines x 2000 steps at beam 32 - "equal strings", with that bound.
 * Outputs are host pointers; any may be NULL, except that labels needs lengths:
 *   labels  int32 [B][nbest][W]: the first lengths entries of a hypothesis valid, the rest zeros;
 *   lengths int32 [B][nbest];
 *   logp    float64 [B][nbest]: logaddexp(pb, pnb), the log-prob of the text over the alignments the pruned search kept,
 *           a lower bound of -nll of that text;
 *   score   float64 [B][nbest]: total;
 *   count   int32 [B]: hypotheses returned, below nbest when fewer exist, 0 when every candidate of some step was
 *           <unknown> (no error here, unlike hctr_beam_search's HCTR_ERR_EMPTY_LINE). Unused slots: length 0, logp and
 *           score -inf.
 * Limits: 1 <= nbest <= beam <= 32, 1 <= k <= min(C, 32) (the reference's defaults are 10 / 10); input_lengths outside
 * [1, W], a NaN len_bonus, labels without lengths, and for hctr_nbest_topk a class outside [0, C) or repeated in its
 * row: HCTR_ERR_ARG with a message. B == 0 is a no-op. A row holding a NaN leaves that line's outputs unspecified; the
 * call returns and the other lines are unaffected. No atomics: repeated calls, and host-pointer / device-pointer calls,
 * agree bit for bit. HCTR_ERR_NOMEM leaves the context usable.
 * hctr_nbest_topk takes the caller's lists, [W][B][k] host arrays: the search alone; needs no weights.
 * hctr_nbest_logits takes logits (or log-probs) in WBC layout, host or device pointer, and runs hctr_beam_frontend's
 *   stored-logits front end (wbc_to_rows, row_topk) and the search on its device lists; needs no weights.
 * hctr_nbest runs the forward of img (arguments as hctr_greedy) in internal passes with the front end hctr_beam_frontend
 *   uses - the fused head epilogues where they apply, stored logits + row_topk otherwise and when a row list overflows -
 *   and inside each pass the search on the pass's lists where they lie; no top-k array goes to the host. Mode 0 is f16,
 *   mode 1 f16x3; mode 2 runs EVERY line in f16x3 (the margin certificate bounds argmax flips, not beam scores) and
 *   leaves hctr_last_guard's figures as they were, exactly as hctr_ctc_loss / hctr_ctc_align do.
 * Launches (hctr_last_profile), after the front end's own: prefix_beam (one workgroup per line, sequential over its
 * steps, the list in LDS; instances (beam, k) <= (10, 10) on one wave64, (16, 16) and (32, 32) on four) and, when labels
 * are wanted, prefix_backtrace (one lane per returned hypothesis).
 * Device scratch (the context's grow-only CTC scratch; n = B, for hctr_nbest the lines of one pass): 4 * B (steps) +
 * 8 * n*W*beam (per step and place: parent place and appended label; 64 lines of 2000 steps at beam 32: 32 MB) +
 * 4 * n*nbest*W (labels) + 20 * n*nbest + 4 * n, each array rounded up to 256 bytes; hctr_nbest_topk adds 8 * W*B*k for
 * the lists, hctr_nbest_logits W*B*C floats for the rows (as many again for logits passed as a host pointer) and
 * 4 * W*B * (2k + 4) for the lists. */
int hctr_nbest_topk(hctr_ctx* ctx, const int32_t* topk_idx, const float* topk_logp, int W, int B, int C, int k,
                    int beam, int nbest, double len_bonus, const int32_t* input_lengths,
                    int32_t* labels, int32_t* lengths, double* logp, double* score, int32_t* count);
int hctr_nbest_logits(hctr_ctx* ctx, const float* logits_wbc, int on_device, int W, int B, int C, int k,
                      int beam, int nbest, double len_bonus, const int32_t* input_lengths,
                      int32_t* labels, int32_t* lengths, double* logp, double* score, int32_t* count);
int hctr_nbest(hctr_ctx* ctx, const void* img, int img_dtype, int img_on_device, const int32_t* widths, int B, int W,
               int k, int beam, int nbest, double len_bonus, const int32_t* input_lengths,
               int32_t* labels, int32_t* lengths, double* logp, double* score, int32_t* count);

/* ---- host prefix beam search: replaces ctc_codec.__cbs_full__/__cbs_skip__ -------------------
 * utils/ctc_codec.py:124-285 (Beam :288-307), float64 accumulators over float32 log-probs.
 * The language model stays behind callbacks, as in the reference (kenlm / transformer objects are
 * duck-typed there, utils/ctc_codec.py:216-219,269-281):
 *   score_cb: called once per time step with n sentences (label ids of prefix+suffix, CSR in
 *             ids/offs); must fill scores[n]. Replaces ngram.score(' '.join(chars), eos=False)
 *             / transformer.score(batch, char_based=True).
 *   next_cb:  optional (use_tfm_pred): for n beam prefixes fill out_ids[n][k] with the LM's next labels
 *             (utils/ctc_codec.py:216-227; k = search_depth on the first call of a step). The reference chains
 *             whatever list the LM returns (:225-226): pad a shorter list with the <unknown> id C-1 (skipped, :238-239)
 *             and return 0; if some list is LONGER than k return the number of slots needed (> k) and the search
 *             calls again with that k. Negative = failure (propagated). NULL disables.
 * builtin_lm: 0 = callbacks, 1 = zero LM, 2 = toy hashed bigram over code points (needs
 *             label_codepoints[C]), 3 = ARPA n-gram (needs ngram + label_words[C]); built-ins make
 *             the multi-threaded path callback-free.
 * full_logp_wbc: float32 [W][B][C] log-probs, required only with next_cb (LM-proposed labels can be
 *             any class); NULL otherwise. cand_* are required only when skip_search != 0.
 * Per-line results: out_labels int32 [B][W] + out_lengths [B]. line_status[b] is HCTR_OK or
 * HCTR_ERR_EMPTY_LINE; the return value is the first non-OK line status. */
typedef int (*hctr_lm_score_cb)(void* user, int n, const int32_t* ids, const int32_t* offs, double* scores);
typedef int (*hctr_lm_next_cb)(void* user, int n, const int32_t* ids, const int32_t* offs, int k, int32_t* out_ids);

/* ---- ARPA back-off n-gram LM: stands in for kenlm.Model (utils/ctc_codec.py:121-122,276-281) ---
 * hctr_ngram_score == kenlm.Model.score(sentence, bos, eos): log10 probability of a whitespace-
 * separated UTF-8 sentence (Katz back-off, OOV -> <unk>). hctr_ngram_word_id maps a token to the
 * model's word id (-1 = out of vocabulary) so the beam search can score label sequences natively
 * (hctr_beam_params.builtin_lm == 3, .ngram, .label_words). hctr_ngram_word_logp is one term of that score, log10
 * P(word | ctx): ctx holds the previous word ids, most recent last, only the last order - 1 count; word -1 = out of
 * vocabulary (NaN for a NULL lm or ctx). Parity with the kenlm binary: unpinned. */
typedef struct hctr_ngram hctr_ngram;
int hctr_ngram_load(const char* arpa_path, hctr_ngram** out);
void hctr_ngram_free(hctr_ngram* lm);
int hctr_ngram_order(const hctr_ngram* lm);
int32_t hctr_ngram_word_id(const hctr_ngram* lm, const char* word_utf8);
double hctr_ngram_score(const hctr_ngram* lm, const char* sentence_utf8, int bos, int eos);
double hctr_ngram_word_logp(const hctr_ngram* lm, const int32_t* ctx, int nctx, int32_t word);
const char* hctr_ngram_last_error(void);

typedef struct {
    int skip_search;        /* utils/ctc_codec.py:40,66 */
    int beam_size;          /* :37 */
    int search_depth;       /* :36 */
    double lm_panelty;      /* :34 (spelling is the reference's) */
    double len_bonus;       /* :35 */
    int builtin_lm;
    const int32_t* label_codepoints;  /* [C] unicode code point per label, for builtin_lm == 2 */
    hctr_lm_score_cb score_cb;
    hctr_lm_next_cb next_cb;
    void* user;
    int num_threads;        /* lines in parallel; forced to 1 when callbacks are used */
    const hctr_ngram* ngram;          /* builtin_lm == 3: ARPA model ... */
    const int32_t* label_words;       /* ... and [C] LM word id per label (-1 = OOV) */
} hctr_beam_params;

int hctr_beam_search(const hctr_beam_params* p, int W, int B, int C, int k,
                     const int32_t* topk_idx, const float* topk_logp, const float* blank_logp,
                     const int64_t* cand_off, const int32_t* cand_idx, const float* cand_logp,
                     const float* full_logp_wbc,
                     int32_t* out_labels, int32_t* out_lengths, int32_t* line_status);

/* ---- N-best texts with n-gram LM scores: the reference's LM-scored prefix beam search, on the device ------------
 * __cbs_full__ of utils/ctc_codec.py:183-285 with an ARPA n-gram model (what hctr_beam_search does with builtin_lm == 3)
 * run where the front end's lists lie, returning the first nbest hypotheses of the final list with their scores.
 * hctr_lm is a flat, pointer-free image of an hctr_ngram for one label set: one open-addressing table of 32-byte slots
 * (six word ids, logp, back-off; power-of-two capacity, load <= 0.5, linear probing; a probe compares every word id, so
 * lookups are exact) plus the label -> word map. hctr_lm_build is host only and needs no GPU: label_words[C] maps each
 * label to an LM word id, -1 = out of vocabulary, as hctr_beam_params.label_words does; it is copied. A model of order
 * above 6, or a label_words entry that is no word id of the model: HCTR_ERR_ARG with a message through
 * hctr_ngram_last_error; allocation failure: HCTR_ERR_NOMEM; no exception crosses the ABI. hctr_lm_word_logp is
 * log10 P(word | ctx) over the flat table - ctx: the previous word ids, most recent last, only the last order - 1 count;
 * word -1 = OOV - by the routine the device search runs, compiled for the host, bit-equal to the string-keyed scorer
 * behind hctr_ngram_score; it lets the table be checked without a GPU. The hctr_ngram may be freed after the build.
 * The search is the one of hctr_nbest* (steps 1-5 there, the same tie rule, fingerprints and limits) with three
 * additions, each as hctr_beam_search(builtin_lm = 3) has it:
 *   * the greedy line: over the first L_b = input_lengths[b] columns (NULL: W) the top-1 class of each row's list,
 *     keeping entries that are not blank, not <unknown> (C-1) and not a repeat of the previous column, with their time
 *     stamps. The line runs end_b = min(last stamp + 4, L_b) steps; at step t the SUFFIX is the first <= 4 greedy labels
 *     with a stamp > t. Computed on the device. A line whose greedy text is empty returns count[b] = 0 (the host search
 *     reports HCTR_ERR_EMPTY_LINE for it); the other lines are unaffected and the call returns HCTR_OK;
 *   * every hypothesis carries the n-gram score of its prefix - a float64 running sum, left to right from the <s>
 *     context, one log10 P(word | last order-1 words) term per label - and its last order-1 word ids;
 *   * every entry of a step is ranked by total = logaddexp(pb', pnb') + pt, pt = s * lm_panelty + len * len_bonus with
 *     each product rounded on its own, s = the prefix's score plus one term per suffix word in order.
 * At the last step the suffix is empty, so the score that decides the final order is that of the text itself.
 * Outputs as hctr_nbest* (logp = logaddexp(pb, pnb), score = total) plus
 *   lm_score float64 [B][nbest]: the n-gram log10 score of the text (bos, no eos) before lm_panelty; -inf in unused slots.
 * Limits and argument errors as hctr_nbest*; also HCTR_ERR_ARG for a NULL lm, a NaN lm_panelty and an lm built for a
 * different C. A context uploads the table (and the label map) on first use and keeps the device copy of the most
 * recently used hctr_lm, recognised by a serial number stored in the object, not by its address; it is replaced when
 * another model is used and freed with the context. An upload that does not fit is HCTR_ERR_NOMEM and leaves the context
 * usable. hctr_lm_free does not touch any context; a freed model's device copy stays until replaced.
 * Launches after the front end's own: beam_lm_prepass (one workgroup per line: word ids of the lists, the per-step
 * suffixes, the end step), prefix_beam_lm (the instances of prefix_beam) and prefix_backtrace.
 * Device scratch: that of the matching hctr_nbest* entry, plus 16 * n*W (per-step suffixes) + 4 * n*W*k (word ids of
 * the lists) + 4 * n (end steps) + 8 * n*nbest (lm_score) in the CTC scratch, plus, held by the context,
 * 32 * capacity + 4 * C bytes for the table, capacity = the power of two >= 2 * the model's n-gram count. */
typedef struct hctr_lm hctr_lm;
int hctr_lm_build(const hctr_ngram* lm, const int32_t* label_words, int C, hctr_lm** out);
int hctr_lm_order(const hctr_lm* lm);
double hctr_lm_word_logp(const hctr_lm* lm, const int32_t* ctx, int nctx, int32_t word);
void hctr_lm_free(hctr_lm* lm);
int hctr_nbest_lm_topk(hctr_ctx* ctx, const hctr_lm* lm, const int32_t* topk_idx, const float* topk_logp, int W, int B,
                       int C, int k, int beam, int nbest, double lm_panelty, double len_bonus,
                       const int32_t* input_lengths, int32_t* labels, int32_t* lengths, double* logp, double* score,
                       int32_t* count, double* lm_score);
int hctr_nbest_lm_logits(hctr_ctx* ctx, const hctr_lm* lm, const float* logits_wbc, int on_device, int W, int B, int C,
                         int k, int beam, int nbest, double lm_panelty, double len_bonus, const int32_t* input_lengths,
                         int32_t* labels, int32_t* lengths, double* logp, double* score, int32_t* count,
                         double* lm_score);
int hctr_nbest_lm(hctr_ctx* ctx, const hctr_lm* lm, const void* img, int img_dtype, int img_on_device,
                  const int32_t* widths, int B, int W, int k, int beam, int nbest, double lm_panelty, double len_bonus,
                  const int32_t* input_lengths, int32_t* labels, int32_t* lengths, double* logp, double* score,
                  int32_t* count, double* lm_score);

/* ---- LM weight sweep: the LM-scored search under a grid of (lm_panelty, len_bonus) pairs, with CER, on the device ---
 * What test.py -gs (test.py:347-382) computes with one complete evaluation run per pair: for every pair g = 0..G-1,
 * (lm_panelty[g], len_bonus[g]), the 1-best text of every line by the search of hctr_nbest_lm* and its edit distance
 * to the line's transcription. Nothing before the ranking depends on the weights, so a call runs the forward, the front
 * end and the pre-pass (word ids, greedy line, suffixes, end steps) once per pass, searches `chunk` pairs per launch on
 * the shared lists - one workgroup per (pair, line), grid line g * n + b - and takes the distances of the grid lines
 * against the references, which are uploaded once, with the distance-only instance of hctr_edit_distance.
 * CONTRACT: for every g, every output equals, bit for bit, what the matching hctr_nbest_lm* entry called with nbest = 1,
 * lm_panelty[g], len_bonus[g] returns, followed by hctr_edit_distance on its labels. Results do not depend on chunk;
 * there are no atomics, and repeated calls are bit-identical.
 * Arguments up to beam as the matching hctr_nbest_lm* entry; input_lengths likewise. targets / target_lengths: the
 * transcriptions back to back, as for hctr_evaluate* (codec.encode's layout); ids in [1, C-1], lengths in [0, 2047].
 * Outputs, host pointers, any may be NULL:
 *   edits       int32 [G][B]: editdistance.eval(1-best text of line b under pair g, transcription of line b);
 *   hyp_lengths int32 [G][B]: the length of that text;
 *   empty       uint8 [B]: 1 when the line's greedy text is empty. The greedy text does not depend on the pair. Such a
 *               line contributes the empty text under every pair (hyp_lengths = 0, edits = L_b, logp = score = lm_score
 *               = -inf, as hctr_nbest_lm* return count = 0 for it) and the call still returns HCTR_OK. The reference
 *               raises IndexError for such a line, and hctr_beam_search reports HCTR_ERR_EMPTY_LINE;
 *   labels      int32 [G][B][W], zero padded; logp, score, lm_score float64 [G][B]: the 1-best's values exactly as
 *               hctr_nbest_lm* with nbest = 1 returns them. They are large and exist so that the sweep can be checked;
 *               callers normally pass NULL.
 * chunk: pairs per launch. 0 = the engine's choice, hctr_lm_sweep_chunk(n, W, beam, G) =
 *   max(1, min(G, 8192 / n, 2^31 / (n * (8 * W*beam + 4 * W + 36)))), n = B, for hctr_lm_sweep the lines of its first
 *   (largest) pass: enough (pair, line) workgroups to fill the chip about four times over (about 2048 single-wave
 *   workgroups of the beam 10 / k 10 instance are resident at once), capped by G and by 2 GiB of per-chunk scratch.
 *   Any other value in [1, G] is used as given.
 * Errors: HCTR_ERR_ARG with a message for everything the matching hctr_nbest_lm* entry and hctr_evaluate_logits reject
 * (shapes, k, beam, input_lengths, lists, a NULL lm, an lm built for another C, NULL target_lengths, a target id outside
 * [1, C-1], a transcription longer than 2047), for G < 1, a NULL weight array, a NaN among the weights (the message
 * names the pair) and chunk outside [0, G]. B == 0 is a no-op. HCTR_ERR_NOMEM leaves the context usable.
 * hctr_lm_sweep runs the forward and the front end once, in internal passes as hctr_nbest_lm does; mode 2 runs every
 * line in f16x3 and hctr_last_guard is left as it was; no list goes to the host.
 * Launches after the front end's own: beam_lm_prepass (once per pass), then per chunk prefix_beam_lm_grid,
 * prefix_backtrace and edit_distance (hctr_last_profile adds up entries of one name).
 * Device scratch (the context's grow-only CTC scratch; n as above, c = the chunk): 4 * B (steps) + 4 * (2 * B + sum L)
 * (references) + 16 * G (pairs) + 16 * n*W (suffixes) + 4 * n*W*k (word ids) + 4 * n (end steps), held once per pass,
 * plus per chunk 8 * c*n*W*beam (history) + 4 * c*n*W (labels) + 36 * c*n (length, count, distance, logp, score,
 * lm_score), each array rounded up to 256 bytes; the lists and the table as hctr_nbest_lm* hold them. */
int hctr_lm_sweep_chunk(int lines, int W, int beam, int G);
int hctr_lm_sweep_topk(hctr_ctx* ctx, const hctr_lm* lm, const int32_t* topk_idx, const float* topk_logp, int W, int B,
                       int C, int k, int beam, const double* lm_panelty, const double* len_bonus, int G, int chunk,
                       const int32_t* input_lengths, const int32_t* targets, const int32_t* target_lengths,
                       int32_t* edits, int32_t* hyp_lengths, uint8_t* empty, int32_t* labels, double* logp, double* score,
                       double* lm_score);
int hctr_lm_sweep_logits(hctr_ctx* ctx, const hctr_lm* lm, const float* logits_wbc, int on_device, int W, int B, int C,
                         int k, int beam, const double* lm_panelty, const double* len_bonus, int G, int chunk,
                         const int32_t* input_lengths, const int32_t* targets, const int32_t* target_lengths,
                         int32_t* edits, int32_t* hyp_lengths, uint8_t* empty, int32_t* labels, double* logp,
                         double* score, double* lm_score);
int hctr_lm_sweep(hctr_ctx* ctx, const hctr_lm* lm, const void* img, int img_dtype, int img_on_device,
                  const int32_t* widths, int B, int W, int k, int beam, const double* lm_panelty, const double* len_bonus,
                  int G, int chunk, const int32_t* input_lengths, const int32_t* targets, const int32_t* target_lengths,
                  int32_t* edits, int32_t* hyp_lengths, uint8_t* empty, int32_t* labels, double* logp, double* score,
                  double* lm_score);

/* ---- N-best texts by the reference's SKIP search, on the device -------------------------------------------------
 * __cbs_skip__ of utils/ctc_codec.py:124-181 (test.py -ss; what hctr_beam_search does with skip_search != 0 and
 * builtin_lm == 3 or 1): the search of hctr_nbest_lm*, except that a column in which ONE class alone has probability above
 * 0.001 updates the kept hypotheses in place - no extension fan-out, no LM call, no sort. lm == NULL is the zero LM (the
 * reference's skip_zero setting); lm_panelty is then unused. Line numbers below refer to utils/ctc_codec.py.
 *   Greedy line, end step, suffix: exactly those of hctr_nbest_lm*, from the top-1 class of each row, computed on the
 *     device. An empty greedy text gives count[b] = 0 (status 1).
 *   Candidate set: at step t < end_b the row's candidate list, the m classes whose float32 log-prob exceeds ln(0.001), in
 *     class-ascending order (np.where, :144) - not the top-k list.
 *   In-place step (m == 1, :147-171). If the class c is >= C-1, nothing changes. Otherwise every hypothesis is updated on
 *     its own, in list order, with l the class's log-prob, l0 the row's blank log-prob and tot = logaddexp(pb, pnb):
 *       c == 0:                       pb = tot + l (pnb stays);
 *       c != tail:                    append c, pnb = tot + l, pb = -inf;
 *       c == tail and pb != -inf:     append c, pnb = pb + l, pb = -inf;
 *       c == tail and pb == -inf:     pb = tot + l0, pnb = pnb + l - pb first, from the old pnb; the blank is read though
 *                                     it is no candidate (:170).
 *     No merge, no LM ranking, no sort, no cut: the list keeps its order and may afterwards hold equal texts. An appended
 *     label advances the hypothesis' fingerprint, length, last label, running n-gram score (one term) and context.
 *   Ranked step (m != 1): steps 1-5 of hctr_nbest* with the ranking of hctr_nbest_lm* and the m candidates in list order
 *     (first-touch keys and the tie rule follow that order). Hypotheses with equal texts are FOLDED before the step: the
 *     first keeps its place and its LM state and takes pb = logaddexp over their pb in list order, pnb likewise; the
 *     later ones leave and the rest close up. This is the sum the reference's dict forms in that step - equal texts see
 *     the same candidates - with another order of additions: results agree with the reference's order of operations to
 *     rounding, not to the bit. m == 0 empties the list, as the reference's empty dict does: count[b] = 0 (status 2),
 *     where the reference raises IndexError at :179.
 *   Cap: a ranked step holds at most 32 candidates. A line with a row of m > 32 inside its end step is not searched:
 *     count[b] = 0, status 3; the other lines are unaffected and the call returns HCTR_OK. (Probabilities above 0.001
 *     allow m up to 999; searching such rows in chunks of 32 is the follow-up)
 *   Result: the first nbest hypotheses of the final list AS THE LIST STANDS. After a trailing run of in-place steps it
 *     is not sorted by score and may hold a text twice; the reference returns kept_beams[0] of exactly that list.
 * Outputs as hctr_nbest_lm*: logp = logaddexp(pb, pnb); lm_score = the running n-gram score of the text, 0 in used
 * slots for lm == NULL (-inf in unused ones); score = logp + lm_score * lm_panelty + len * len_bonus, each product rounded
 * on its own, computed at the end (logp + len * len_bonus for lm == NULL); and per line
 *   status int32 [B]: 0 ok, 1 empty greedy text, 2 list emptied by a row without usable candidates, 3 overflow;
 *   ranked int32 [B]: how many of the line's end_b steps have m != 1 (ranked steps); the others are in-place.
 * Any output may be NULL (labels needs lengths). Limits and errors as hctr_nbest_lm* (1 <= nbest <= beam <= 32, a NaN
 * len_bonus, with an lm a NaN lm_panelty and an lm built for another C); HCTR_ERR_NOMEM leaves the context usable. No
 * atomics: repeated calls are bit-identical. The context's device copy of the lm is the one hctr_nbest_lm* use.
 * hctr_nbest_skip_lists takes the caller's lists on the host, as hctr_beam_frontend(want_candidates = 1) and
 *   hctr_beam_fetch_candidates return them: top1_idx int32 [W][B] (the greedy line needs no more of the top-k),
 *   blank_logp float32 [W][B], cand_off int64 [W*B + 1] / cand_idx / cand_logp (row r = t*B + b). The search alone; needs
 *   no weights. HCTR_ERR_ARG for offsets that decrease, a class outside [0, C), classes of a row not strictly ascending.
 * hctr_nbest_skip_logits takes logits (or log-probs) in WBC layout, host or device pointer, runs the stored-logits
 *   front end and the search on its lists; needs no weights.
 * hctr_nbest_skip runs the forward of img (arguments as hctr_nbest_lm, without k: only the top-1 class is read) in
 *   internal passes; inside a pass the candidate counts stay on the device - the lists go to a padded layout, 32
 *   entries per row beside the row's count - so nothing visits the host between front end and search. Mode 2 runs
 *   every line in f16x3 and leaves the guard figures alone, as hctr_nbest* do.
 * Launches after the front end's own: skip_candidates (not for _lists), beam_lm_prepass, prefix_beam_skip,
 * prefix_backtrace.
 * Device scratch (the CTC scratch; n = B, for hctr_nbest_skip the lines of one pass): 4 * B (steps) + 8 * n*W*beam
 * (history: one {place, label} per step and place, in-place steps included) + 4 * n*nbest*W (labels) + 28 * n*nbest +
 * 16 * n*W (suffixes) + 16 * n (count, end step, status, ranked), each array rounded up to 256 bytes; besides, for
 * hctr_nbest_skip_lists 268 * W*B bytes for the uploaded lists (count, top-1, blank and 32 padded candidates per row),
 * for the other two 256 * n*W bytes of padded candidates beside the front end's own outputs, and for
 * hctr_nbest_skip_logits the rows as hctr_nbest_logits holds them. */
int hctr_nbest_skip_lists(hctr_ctx* ctx, const hctr_lm* lm, const int32_t* top1_idx, const float* blank_logp,
                          const int64_t* cand_off, const int32_t* cand_idx, const float* cand_logp, int W, int B, int C,
                          int beam, int nbest, double lm_panelty, double len_bonus, const int32_t* input_lengths,
                          int32_t* labels, int32_t* lengths, double* logp, double* score, int32_t* count, double* lm_score,
                          int32_t* status, int32_t* ranked);
int hctr_nbest_skip_logits(hctr_ctx* ctx, const hctr_lm* lm, const float* logits_wbc, int on_device, int W, int B, int C,
                           int beam, int nbest, double lm_panelty, double len_bonus, const int32_t* input_lengths,
                           int32_t* labels, int32_t* lengths, double* logp, double* score, int32_t* count, double* lm_score,
                           int32_t* status, int32_t* ranked);
int hctr_nbest_skip(hctr_ctx* ctx, const hctr_lm* lm, const void* img, int img_dtype, int img_on_device,
                    const int32_t* widths, int B, int W, int beam, int nbest, double lm_panelty, double len_bonus,
                    const int32_t* input_lengths, int32_t* labels, int32_t* lengths, double* logp, double* score,
                    int32_t* count, double* lm_score, int32_t* status, int32_t* ranked);

/* ---- line preprocessing on the device: replaces read_resize_image / pil_loader -----------------
 * test.py:207-216 (cv2.cvtColor BGR2GRAY + cv2.resize(src, (tw, 128), interpolation=cv2.INTER_AREA)) and
 * utils/dataset.py:47-60 (the same resize inside ImageDataset.pil_loader). Image files are decoded by
 * the caller; this call takes the decoded u8 pixels of n ragged images packed back to back in one host
 * buffer (image i: heights[i] x widths[i] x |channels[i]| bytes at offsets[i]; channels 1 = gray,
 * 3 = BGR as cv2.imread returns it, -3 = RGB as PIL returns it), converts colour to gray, resizes image i
 * to out_height x out_widths[i] and writes it into row i of out[n][out_height][out_W] (uint8). Columns
 * >= out_widths[i] are zero - hctr_greedy / hctr_forward_logits replicate the last real column from
 * `widths`, which is NormalizePAD, utils/dataset.py:83-93; columns >= out_W of a wider line are dropped,
 * which is AlignCollate's max_width crop, utils/dataset.py:118-145 (pass widths min(out_widths[i], out_W)
 * on). out may be device memory (out_on_device), so the resized batch feeds hctr_greedy without touching
 * the host again.
 * Pixel parity with OpenCV is unpinned (opencv-python is not installed here): the kernel follows the
 * published OpenCV 4.x algorithm as restated in oracle/resize_ref.py and is bit-exact against that. */
int hctr_resize_lines(hctr_ctx* ctx, const uint8_t* packed_src, int64_t packed_bytes, const int64_t* offsets,
                      const int32_t* heights, const int32_t* widths, const int32_t* channels, int n,
                      int out_height, const int32_t* out_widths, int out_W, uint8_t* out, int out_on_device);

/* ---- multi-GPU result gather for plain-C callers -----------------------------------
 * The path shards by lines: one process per GPU runs hctr_greedy on its contiguous range of the (globally padded)
 * batch, and the decoded label sequences meet in ONE collective. The reference has no counterpart (single-device
 * inference, test.py:143-148; NCCL only in training DDP, main.py:226-237). Python callers use torch.distributed
 * (handwritten-chinese-ocr-samples_amd/dist.py); these entry points do the same over RCCL (xGMI), which is bound
 * with dlopen at the first call. Protocol as in NCCL: rank 0 calls hctr_comm_unique_id and hands the 128 bytes to
 * the other ranks out of band (file, socket, MPI); every rank then calls hctr_comm_create.
 * hctr_gather_labels: every rank passes its n_local decoded lines (labels: int32 [n_local][row_stride], the first
 * lengths[i] entries of row i valid - exactly hctr_greedy's outputs with row_stride = W) and the common
 * lines_per_rank = ceil(global lines / world) and cap (longest label sequence allowed). One ncclAllGather of the
 * packed [lines_per_rank][1 + cap] int32 buffer; on return EVERY rank holds out_labels int32 [world*lines_per_rank][cap]
 * and out_lengths [world*lines_per_rank] in rank order (rows >= a rank's n_local have length 0). */
#define HCTR_COMM_ID_BYTES 128
typedef struct hctr_comm hctr_comm;
int hctr_comm_unique_id(void* id128);
int hctr_comm_create(hctr_comm** out, const void* id128, int rank, int world, int device);
void hctr_comm_destroy(hctr_comm* comm);
int hctr_gather_labels(hctr_comm* comm, const int32_t* labels, const int32_t* lengths, int n_local, int row_stride,
                       int lines_per_rank, int cap, int32_t* out_labels, int32_t* out_lengths);
const char* hctr_comm_last_error(void);

/* ---- introspection used by bench.py / tests ---------------------------------------------------
 * Per-layer device time of the last forward (HIP events on the context's stream), in call order.
 * names: '\n'-separated layer names written into buf (cap bytes); ms: float array of n entries.
 * Returns the number of layers recorded (or a negative status). Enabled by hctr_set_profiling. */
int hctr_set_profiling(hctr_ctx* ctx, int enabled);
int hctr_last_profile(hctr_ctx* ctx, char* names_buf, int cap, float* ms, int max_n);
/* Workspace arena of the context: bytes currently allocated, how often it was (re)allocated - it only ever grows, to
 * the largest layout seen - and how often its layout was re-carved for a new (lines, width, precision) shape. */
int hctr_workspace_stats(hctr_ctx* ctx, int64_t* arena_bytes, int64_t* arena_allocations, int64_t* recarves);
/* Lines per internal pass for a batch of B lines of width W (a batch beyond HCTR_MAX_COLS pixel columns - a third
 * of that in f16x3 - runs in balanced passes; hctr_last_profile adds the passes' entries of one name up). */
int hctr_lines_per_pass(hctr_ctx* ctx, int B, int W, int f16x3);
/* Diagnostic build of the 3x3 conv kernel: with layer != NULL, arms time-stamping of that layer's
 * workgroups (a separate kernel instance; results of the forward are unchanged) for up to cap_wgs
 * workgroups and returns 0. With layer == NULL copies the last forward's stamps to out[n][16]
 * (u64: entry, prologue issued, operands landed, K loop done, epilogue done, stores drained - 100 MHz
 * ticks - HW_ID and XCC_ID registers, then four stamps inside the epilogue) and returns n. tools/gpu_stamps.py is the consumer. */
int64_t hctr_debug_stamps(hctr_ctx* ctx, const char* layer, uint64_t* out, int64_t cap_wgs);

/* Debug taps for bisecting parity: copy an intermediate activation of the last forward to the host
 * as float32 NCHW [B][C][H][W]. name: "stage0".."stage4", "conv0_1". Returns element count or <0. */
int64_t hctr_debug_activation(hctr_ctx* ctx, const char* name, float* out, int64_t cap,
                              int* C, int* H);
/* SE statistics of block "block<s>.<i>" in the last forward (fused SE form, the default): the channel means of
 * bn2(conv2(t)) that se_premean derived from conv1's sums, and the channel scales it computed from them, each as
 * float32 [B][C] (C = the block's planes; either pointer may be NULL; cap = room in each, in floats). Every block
 * keeps its own slot in the workspace, so all twelve are readable after one forward. HCTR_ERR_STATE on the unfused
 * path (HCTR_FUSE_SE=0 in f16 mode), which computes no means ahead of conv2. */
int hctr_debug_se(hctr_ctx* ctx, const char* name, float* mean_out, float* scale_out, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* HCTR_HIP_H */
