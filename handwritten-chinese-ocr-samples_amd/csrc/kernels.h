// Launch interface between the engine (engine.cpp) and the gfx950 kernels (kernels.hip).
// Internal to libhctr_hip.so; the public C ABI is include/hctr_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lm_flat.h"
#include "lex_flat.h"
#include "lex_words.h"
#include "pat_flat.h"

namespace hctr {

typedef _Float16 half_t;

constexpr int kTileW = 16;      // output columns per pixel tile (all conv layers)
constexpr int kBK = 64;         // input channels per k-step

// One MFMA implicit-GEMM launch: 3x3 / 1x1 convolution over padded NHWC fp16 activations, or the
// head projection (MODE linear). See DESIGN.md "conv_mfma" for the tiling.
struct ConvArgs {
    const half_t* x;        // input base: padded NHWC [B][H+2][Wa][Cin] (conv) or [M][Cin] (linear)
    const half_t* w;        // [taps][CoutPad][Cin], rows permuted to MFMA order within 64-blocks
    const float* bias;      // [CoutPad] folded BatchNorm bias
    void* y;                // output base (fp16, or fp32 for the head)
    float* se_part;         // [B][tilesH*tilesW][Cout] per-tile channel sums of the STORED (fp16-rounded,
                            // post-ReLU, column-masked) outputs, or nullptr
    const float* se_scale;  // fused squeeze-excite: [B][Cout] channel scales, or nullptr
    const half_t* resid;    // fused residual (same geometry as the output), used with se_scale
    int H, W;               // conv output rows / valid columns (pre-pool)
    int Cin, Cout, CoutPad;
    int tilesW, tilesH;     // pixel tiles per image
    int64_t in_sb;          // input batch stride (elements)
    int in_sh;              // input row stride (elements); pixel stride is Cin
    int64_t out_sb;         // output batch stride (elements)
    int out_sh, out_sw;     // output row / column strides (elements); row index is post-pool
    int64_t out_off;        // element offset of output pixel (b=0,h=0,w=0)
    int out_wlimit;         // columns [W, out_wlimit) are written as zeros (keeps the zero border)
    int relu, pool;
    int64_t M;              // linear mode: number of rows
    int64_t ldo;            // linear mode: output leading dimension (elements)
    int mtiles, ntiles;
    // halo4 kernel prologue without runtime divisions (set by launch_conv): ntiles and tilesH as shifts when they are
    // powers of two (-1 otherwise: the kernel divides), mt / tilesW as (mt * tw_magic) >> 40 (exact for mt * tilesW < 2^40)
    int nt_shift, th_shift;
    uint64_t tw_magic;
    // linear mode, fused greedy argmax (np.argmax(preds, 2), utils/ctc_codec.py:75): when amax_idx is set the
    // logits are NOT stored; every wave column (nt, wn) writes its best (value, class) of each row to
    // amax_val/amax_idx[(nt*WN + wn) * M + m]; launch_argmax_partials picks the first maximum per row.
    float* amax_val;
    int32_t* amax_idx;
    // guarded precision (hctr_set_precision mode 2): when amax_val2 is set the same epilogue also writes, per
    // (part, row), the RUNNER-UP value of the part (amax_val2, -inf for a one-class part) and the part's largest
    // |logit| (amax_abs); launch_argmax_partials turns them into the row's top-1/top-2 margin and max |logit|.
    float* amax_val2;
    float* amax_abs;
    // linear mode, fused beam front end (log_softmax + top-k + p > 0.001 lists, utils/ctc_codec.py:65,127-128,144,186)
    // without storing the logits. PASS 1 = the argmax partials above plus, when psum is set, per (part, row) the sum of
    // expf(v - part max) and the logit of class 0 per row. launch_beam_thresholds turns those into per-row
    // {vmin, gmax}: every logit >= vmin is among the row's top-k or above the candidate threshold.
    // PASS 2 (emit_cnt set; the same GEMM again, 2.5 % of a forward) appends every (class, logit >= vmin) to the
    // row's list (atomic slot counter, emit_cap slots) and writes per (part, row) the float64 sum of
    // expf(v - gmax) - the same terms the unfused row_topk kernel sums. launch_beam_select finishes the rows.
    float* psum;
    float* blank_logit;
    const float* row_thr;     // [M][2] = {vmin, gmax}
    int32_t* emit_cnt;        // [M], zeroed by launch_beam_thresholds
    int32_t* emit_list;       // [M][emit_cap][2] = {class, float bits}
    int emit_cap;
    double* esum;             // [P][M]
    // launch_stem_conv0_2 only: the raw line images (u8 [B][128][W] or f32 [B][1][128][W]), each line's valid width
    // (NULL = W) and conv0_1's folded fp32 weights [64][9] / bias [64]; x is unused there
    const void* img;
    int img_f32;
    const int32_t* img_widths;
    const float* stem_w;
    const float* stem_b;
    int split;              // f16x3 mode: activations are [hi | lo | hi] fp16 planes of Cout channels each
                            // (input side: Cin already counts the tripled channels)
    int drop_lo;            // f16x3 diagnostic (HCTR_X3_MASK, precision attribution): round this layer's output to ONE fp16
                            // value like the f16 mode does (the lo plane is written as zeros)
    // fused 1x1 downsample of a block's input (first block of stages 1-3): the halo4 kernel first accumulates
    // ds_w * ds_x (centre tap, ds_cin channels, same H/W/Wa geometry as x), turns it into the residual term and
    // continues with the 3x3 taps; resid must then be NULL and se_scale set. NULL = not used.
    const half_t* ds_x;
    const half_t* ds_w;       // [1][CoutPad][ds_cin], rows permuted like w
    const float* ds_bias;     // folded BN of the downsample
    int ds_cin;
    int ds_in_sh;             // elements per image row of ds_x
    int64_t ds_in_sb;         // elements per image of ds_x
    int32_t* tile_counter;        // persistent halo4 variant with a dynamic tile queue: 8 ints (one per XCD), zero at launch
    unsigned long long* stamps;   // diagnostic instance only (hctr_debug_stamps): 16 x u64 per workgroup, else NULL
    // timing experiments only (HCTR_DBG), results INVALID. 8-wave/generic kernels: 1 = DMA from fixed hot addresses,
    // 2 = no DMA in the loop. halo4 kernel, bit mask: 32 = no halo reload at chunk boundaries, 64 = no K loop,
    // 128 = no epilogue, 256 = no output stores, 512 = no weight DMA inside the K loop, 1024 = no per-step barrier.
    // Bit 32 has NO effect on the instances that issue the halo reload inside tap 8 (the plain f16 / f16x3 / fused-
    // downsample instances, i.e. every default launch): it only reaches the persistent, RESPRE and STAMP instances.
    int dbg;
};

// tile configurations: (couts x pixels) per 256-thread block
// TILE_HALO4 / TILE_HALO4_8x32: 128 couts x (16x16 | 8x32) pixels, 4 waves, halo-reuse 3x3 kernel
// (two workgroups per CU)
enum ConvTile { TILE_64x256 = 0, TILE_128x128 = 1, TILE_256x256 = 2, TILE_HALO4 = 3, TILE_HALO4_8x32 = 4 };
inline int conv_tile_rows(ConvTile t) { return (t == TILE_128x128 || t == TILE_HALO4_8x32) ? 8 : 16; }
inline int conv_tile_cols(ConvTile t) { return t == TILE_HALO4_8x32 ? 32 : 16; }
inline int conv_tile_couts(ConvTile t) {
    return t == TILE_64x256 ? 64 : (t == TILE_256x256 ? 256 : 128);
}

hipError_t launch_conv(const ConvArgs& a, ConvTile tile, int taps, bool linear_f32, hipStream_t s);
constexpr int kLinearWN = 2;          // wave columns of both linear-mode tiles (partials per n-tile)
// rows [P][M] of (value, class) partials -> idx[M]: first maximum, 0 for an all-(-inf)/NaN row (idx may be NULL).
// With val2 / absp (the guard partials, see ConvArgs) also margin[M] = top-1 minus top-2 logit of the row over all
// classes (0 for an exact tie, NaN when a NaN is involved) and rowabs[M] = max |logit| of the row.
hipError_t launch_argmax_partials(const float* val, const int32_t* cls, int P, int64_t M, int32_t* idx, hipStream_t s,
                                  const float* val2 = nullptr, const float* absp = nullptr, float* margin = nullptr,
                                  float* rowabs = nullptr);
// the same two per-row figures from stored logits rows [M][ld] (hctr_forward_logits in guarded mode)
hipError_t launch_row_guard(const float* logits, int64_t ld, int64_t M, int C, float* margin, float* rowabs, hipStream_t s);
// per line b: out[b][0] = min over its W columns of margin (NaN if any is NaN), out[b][1] = max of rowabs
hipError_t launch_line_guard(const float* margin, const float* rowabs, int B, int W, float* out, hipStream_t s);
size_t conv_lds_bytes(ConvTile tile);

// NormalizePAD + conv0_1 + bn0_1 + ReLU computed into the LDS halo of conv0_2's tile, then conv0_2 + bn0_2 + ReLU +
// (2,1) max-pool from it: conv0_1's 16 kB-per-column output never exists in HBM (f16 mode; a.w/bias = conv0_2's)
hipError_t launch_stem_conv0_2(const ConvArgs& a, hipStream_t s);

// zero the stored conv border of a padded NHWC activation [B][H+2][Wa][C]: rows 0 and H+1, column 0 and columns
// > W of every other row (the interior is rewritten by every forward; see engine.cpp ensure_workspace)
hipError_t launch_zero_borders(half_t* p, int B, int H, int W, int Wa, int C, hipStream_t s);

// split: 0 = fp16 output, 1 = [hi | lo | hi] planes, 2 = planes with the lo plane zero (HCTR_X3_MASK diagnostic)
hipError_t launch_stem(const void* img, int img_f32, const int32_t* widths_dev, const float* w9,
                       const float* bias, half_t* y, int B, int W, int Wa, int split, hipStream_t s);

// statistics of a padded NHWC activation t for the fused squeeze-excite: out[b][5][8 segments][C] = channel sums of
// {row 0, row H-1, column 0, column W-1, the whole image}; the whole-image sums come from conv1's per-tile sums
hipError_t launch_se_border(const half_t* t, int B, int H, int W, int Wa, int C, int split, const float* tsum_part,
                            int tiles, float* out, hipStream_t s);
// SE mean of conv2(t) from those statistics (linearity of the convolution) and, by the last block of each image,
// the SELayer FCs -> channel scales; counter: int32 [B], zero before the first launch (the kernel re-zeroes it)
hipError_t launch_se_premean(const float* border, const half_t* t, const half_t* w, const float* bias, int B, int H,
                             int W, int Wa, int C, int CoutPad, int split, float* mean, const float* w1,
                             const float* w2, float* scale, int32_t* counter, hipStream_t s);

hipError_t launch_se_fc(const float* se_part, int tiles_per_img, const float* w1, const float* w2,
                        float* scale, int B, int C, float inv_hw, hipStream_t s);

hipError_t launch_se_apply(half_t* o, const half_t* r, const float* scale, int64_t img_elems,
                           int B, int C, hipStream_t s);

// tB > 0: rows are in WBC order (r = t*tB + b) and idx is written as [b][t] with row length tW
hipError_t launch_argmax_rows(const float* logits, int64_t ld, int64_t M, int C, int32_t* idx,
                              int tB, int tW, hipStream_t s);

// ---- fused beam front end (see ConvArgs): P = ntiles * kLinearWN class parts per row, rows m = b*W + t ----
constexpr int kBeamCap = 256;         // list slots per row; a row that needs more makes the engine fall back
constexpr int kBeamMaxK = 32;         // largest top-k the fused path serves
// after pass 1: row_thr[m] = {min(k-th largest part maximum, candidate value bound), row max}; emit_cnt[m] = 0.
// cand_thresh: log-prob threshold of the candidate lists (ln 0.001) or +inf when they are not wanted.
hipError_t launch_beam_thresholds(const float* pmax, const float* psum, int P, int64_t M, int k, double cand_thresh,
                                  int want_candidates, float* row_thr, int32_t* emit_cnt, hipStream_t s);
// after pass 2: exact float32 log-softmax terms of the listed classes (row max, float64 exp-sum as row_topk computes
// them), top-k by (log-prob desc, class asc), log-prob of class 0, count of classes above cand_thresh; outputs are
// indexed r = t*B + b like launch_row_topk's. overflow[0] is set to 1 if any row needed more than cap slots.
hipError_t launch_beam_select(const float* row_thr, const int32_t* emit_cnt, const int32_t* emit_list, int cap,
                              const double* esum, int P, const float* blank_logit, int B, int W, int k,
                              double cand_thresh, int32_t* topk_idx, float* topk_logp, float* blank_logp,
                              float* stats, int32_t* cand_count, int32_t* overflow, hipStream_t s);
// candidate lists (ascending class order, log-prob > cand_thresh) out of the per-row lists, to cand_off[r] (r = t*B + b);
// cand_off == null: the padded layout of the skip search, row r at r * pad, candidates beyond the first pad dropped
hipError_t launch_beam_candidates(const int32_t* emit_cnt, const int32_t* emit_list, int cap, const float* stats,
                                  int B, int W, double cand_thresh, const int64_t* cand_off, int pad, int32_t* cand_idx,
                                  float* cand_logp, hipStream_t s);

// raw per-column indices [B][W] (row m = b*W + t) -> collapsed labels [B][W] + lengths [B]
hipError_t launch_ctc_collapse(const int32_t* idx, int B, int W, int C, int32_t* labels,
                               int32_t* lengths, hipStream_t s);

// sub-batch rows [B*W][ld] -> out[t][b0 + b][C] of a [W][Bfull][C] tensor
hipError_t launch_logits_to_wbc(const float* logits, int64_t ld, int B, int W, int C, float* out,
                                int Bfull, int b0, hipStream_t s);
// [W][B][C] -> [B*W][ld] (for caller-supplied logits)
hipError_t launch_wbc_to_rows(const float* wbc, int B, int W, int C, float* rows, int64_t ld,
                              hipStream_t s);

// log-softmax + top-k (+ count of candidates above thresh) per (t,b) row of [B*W][ld]; outputs are
// indexed r = t*B + b. stats receives (row max, log-sum) pairs for launch_row_candidates (cand_off / pad as
// launch_beam_candidates takes them).
hipError_t launch_row_topk(const float* logits, int64_t ld, int B, int W, int C, int k, double thresh,
                           int32_t* topk_idx, float* topk_logp, float* blank_logp, float* stats,
                           int32_t* cand_count, hipStream_t s);
hipError_t launch_row_candidates(const float* logits, int64_t ld, int B, int W, int C, double thresh,
                                 const float* stats, const int64_t* cand_off, int pad, int32_t* cand_idx,
                                 float* cand_logp, hipStream_t s);

// contiguous rows [rows][C] -> float32 log-softmax per row
hipError_t launch_log_softmax_rows(const float* x, int64_t rows, int C, float* y, hipStream_t s);

// ---- CTC loss (hctr_ctc_loss*): per-line tables on the device, indexed by the line's place gb in the caller's batch ----
// kernels.hip's instance ladder of the recursions: the largest extended target 2L + 1 of one line, and the states per
// lane of the instance that max_states launches
extern const int kCtcMaxStates;
int ctc_viterbi_lane_states(int max_states);
struct CtcLines {
    const int32_t* T;       // [B] steps read (input_lengths); 0 = the line has no alignment (nll = +inf, nothing read)
    const int32_t* L;       // [B] target length
    const int32_t* off;     // [B] offset of the line's targets in slot
    const int32_t* nd;      // [B] |D_b| + 1: distinct target classes of the line plus the blank
    const int32_t* cls;     // [B][D] class of each emission slot (slot 0 = class 0, the blank)
    const int32_t* slot;    // [sum L] emission slot of every target position
    int D;                  // emission slots per row (max nd)
};
// rows of logits at x + (b*sb + t*st) * ld for the pass's lines b = 0..nb-1 (line gb = b0 + b of the tables), C classes:
// emis[(b*W + t) * D + j] = z[cls[gb][j]] - logsumexp(z) for t < T[gb], j < nd[gb]; lse (the gradient's pass, else null)
// keeps lse[b*W + t] = logsumexp(z) of those rows in float64
hipError_t launch_ctc_lse(const float* x, int64_t ld, int64_t sb, int64_t st, int C, const CtcLines& m, int b0, int nb,
                          int W, float* emis, double* lse, hipStream_t s);
// forward (alpha) recursion of the pass's lines over those emissions -> nll[b0 + b]; max_states = largest 2L + 1 among
// the lines with T > 0 (<= kCtcMaxStates). ast (the gradient's pass, else null) keeps the rows, ast[aoff[gb] + t*S_gb + s]
// (aoff[gb] = sum of T*S of the lines before gb); nll is bit-identical either way.
hipError_t launch_ctc_alpha(const float* emis, const CtcLines& m, int b0, int nb, int W, int max_states, float* nll,
                            const int64_t* aoff, float* ast, hipStream_t s);
// gradient of the per-line loss in caller logits (hctr_ctc_loss_logits_grad), whole batch (b0 = 0):
// launch_ctc_beta: the beta recursion, which overwrites the alpha rows with y = alpha + nll + (beta before its
//   emission), the log of each state's posterior share;
// launch_ctc_grad_rows: grad[t][b][c] = wt[b] * (softmax(z_t)[c] - gamma_t(c)) for t < T[b], zeros for t >= T[b] and for
//   lines with nll = +inf. soff[b][D + 1], pos[off[b] + ...]: target positions of line b grouped by emission slot
//   (slot j's are pos[off[b] + soff[b][j] .. off[b] + soff[b][j+1]), j >= 1). x and grad are contiguous [W][B][C].
hipError_t launch_ctc_beta(const float* emis, const CtcLines& m, int B, int W, int max_states, const float* nll,
                           const int64_t* aoff, float* ast, hipStream_t s);
hipError_t launch_ctc_grad_rows(const float* x, int C, int B, int W, const CtcLines& m, const double* lse,
                                const float* nll, const float* wt, const int64_t* aoff, const float* ast,
                                const int32_t* soff, const int32_t* pos, float* grad, hipStream_t s);

// forced alignment (hctr_ctc_align*) over the emissions of launch_ctc_lse:
// launch_ctc_viterbi: the max-plus recursion; the lane of states [i*NS, i*NS + NS) stores its 2-bit backpointers (0, 1
//   or 2 states down; state k of the lane at bits 2k) of step t >= 1 at bp[boff[gb] + t * ceil(S_gb / NS) + i], with
//   NS = ctc_viterbi_lane_states(max_states); score[gb] = the best path's log-probability, endst[gb] its last state
//   (-inf and -1 for a line with T = 0);
// launch_ctc_backtrace: path[gb*W + t] = class of the best path at step t (-1 for t >= T), and for target position j of
//   the line, at off[gb] + j: its first step, the step after its last and the float32 sum of its emissions (-1, -1,
//   -inf for a line with T = 0).
hipError_t launch_ctc_viterbi(const float* emis, const CtcLines& m, int b0, int nb, int W, int max_states,
                              const int64_t* boff, uint8_t* bp, float* score, int32_t* endst, hipStream_t s);
hipError_t launch_ctc_backtrace(const float* emis, const CtcLines& m, int b0, int nb, int W, int max_states,
                                const int64_t* boff, const uint8_t* bp, const int32_t* endst, int32_t* path,
                                int32_t* span_start, int32_t* span_end, float* span_logp, hipStream_t s);

// greedy recognition (hctr_recognize*), rows of logits at x + (b*sb + t*st) * ld for the pass's lines b = 0..nb-1, every
// one of the W columns; all per-column and per-character arrays are [nb][W]:
// launch_greedy_rowstat: one read of each row -> k1 (np.argmax), k2 (the first index of the largest logit among the other
//   classes), lp1 / lp2 = float32(z[k] - lse) and lse, the row's log-sum-exp with launch_ctc_lse's arithmetic, bit for bit;
// launch_greedy_spans: the greedy collapse of k1 (launch_ctc_collapse's labels and lengths) and per character j its first
//   column, the column after its run, the ascending-t float32 sum of lp1 over the run, and k2 / lp2 at the run's peak
//   column (largest lp1, first on ties); path_logp[b] = the sum of lp1 over the line's W columns, in a fixed order;
// launch_ctc_emis_gather: launch_ctc_lse's emissions, bit for bit, from kept log-sum-exps lse[b*W + t]: D values are read
//   per row, not the row.
hipError_t launch_greedy_rowstat(const float* x, int64_t ld, int64_t sb, int64_t st, int C, int nb, int W, int32_t* k1,
                                 int32_t* k2, float* lp1, float* lp2, double* lse, hipStream_t s);
hipError_t launch_greedy_spans(const int32_t* k1, const int32_t* k2, const float* lp1, const float* lp2, int nb, int W,
                               int C, int32_t* labels, int32_t* lengths, int32_t* span_start, int32_t* span_end,
                               float* char_logp, int32_t* alt_label, float* alt_logp, float* path_logp, hipStream_t s);
hipError_t launch_ctc_emis_gather(const float* x, int64_t ld, int64_t sb, int64_t st, const CtcLines& m, int b0, int nb,
                                  int W, const double* lse, float* emis, hipStream_t s);

// ---- edit distance (hctr_edit_distance, hctr_evaluate*): the references on the device, indexed by the line's place gb
// in the caller's batch; the hypotheses hyp[b][stride] / hlen[b], the backpointer offsets boff[b] and the launch's lines
// are the pass's own, b = 0..nb-1, line gb = line_of ? line_of[b] : b0 + b ----
// kernels.hip's instance ladder of the sweep: the reference rows of its last rung, and the rows per lane of the rung
// max_len launches
extern const int kEditMaxRows;
int edit_lane_rows(int max_len);
struct EditLines {
    const int32_t* L;       // [B] reference length
    const int32_t* off;     // [B] offset of the line's reference in ref
    const int32_t* ref;     // [sum L] reference symbols, any int32 values
    int32_t wrap = 0;       // > 0 (launch_edit_distance without bp only): line gb is measured against reference
                            // gb mod wrap - the G * wrap grid lines of hctr_lm_sweep* over wrap references
};
// launch_edit_distance: edits[gb] = D[L][H]; max_len = the longest reference of the launch's lines. bp (else null: the
//   distance-only instance, same arithmetic) keeps the 2-bit backpointers (0 diagonal, 1 deletion, 2 insertion; row i of
//   a lane at bits 2i) of step d = j - 1 + k of lane k = (row - 1) / NS at bp[boff[b] + d * lanes + k], lanes =
//   ceil(L / NS), NS = edit_lane_rows(max_len): (H + lanes - 1) * lanes bytes for the line;
// launch_edit_backtrace: counts[gb][4] = {hits, substitutions, deletions, insertions}, ref_map[off[gb] + i] = position
//   in the hypothesis (-1 deleted), hyp_map[gb * stride + j] = position in the reference (-1 inserted, 0 for j >= H).
hipError_t launch_edit_distance(const EditLines& m, int b0, const int32_t* line_of, int nb, const int32_t* hyp,
                                const int32_t* hlen, int stride, int max_len, const int64_t* boff, uint8_t* bp,
                                int32_t* edits, hipStream_t s);
hipError_t launch_edit_backtrace(const EditLines& m, int b0, const int32_t* line_of, int nb, const int32_t* hyp,
                                 const int32_t* hlen, int stride, int max_len, const int64_t* boff, const uint8_t* bp,
                                 int32_t* counts, int32_t* ref_map, int32_t* hyp_map, hipStream_t s);

// ---- prefix beam search without a language model (hctr_nbest*) on the front end's lists where they lie: idx / lp hold
// k classes (descending float32 log-probs) per row r = t*nb + b of the launch's lines b = 0..nb-1; T[b] in [1, W] steps
// of line b count. 1 <= nbest <= beam <= kBeamMaxK, k <= kBeamMaxK (the instance ladder in kernels.hip) ----
// launch_prefix_beam: per line the first nbest hypotheses of the final list, [nb][nbest]: len, logp = logaddexp(pb, pnb),
//   score = logp + len * len_bonus (0, -inf, -inf beyond cnt[b] = the number returned), and the history
//   hist[(b*W + t) * beam + place] = {parent place, appended label or -1} of every kept place of every step;
// launch_prefix_backtrace: labels[nb][nbest][W] (zero on entry) from that history, the first len entries of each.
hipError_t launch_prefix_beam(const int32_t* idx, const float* lp, int nb, int W, int k, int C, int beam, int nbest,
                              double len_bonus, const int32_t* T, int2* hist, int32_t* len, double* logp, double* score,
                              int32_t* cnt, hipStream_t s);
hipError_t launch_prefix_backtrace(const int2* hist, const int32_t* T, int nb, int W, int beam, int nbest,
                                   const int32_t* len, const int32_t* cnt, int32_t* labels, hipStream_t s, int wrap = 0);

// ---- the same search scored by an n-gram model (hctr_nbest_lm*; lm_flat.h has the table and the lookup) ----
// launch_beam_lm_prepass: from the lists and T[b] (the columns of line b that count) the word ids of every list entry
//   (wid, laid out as idx; words[C] = label -> word id), suffix[b * W + t] = the first <= 4 greedy entries with a stamp
//   > t as word ids (-2 = no more) and end[b] = min(last greedy stamp + 4, T[b]), 0 for an empty greedy text;
// launch_prefix_beam_lm: launch_prefix_beam over end[b] steps with every entry ranked by log-prob + (n-gram score of
//   prefix + suffix) * lm_panelty + len * len_bonus; score is that total, o_lm[nb][nbest] the n-gram score of the text
//   (-inf beyond cnt[b]); a line with end[b] = 0 returns cnt[b] = 0. launch_prefix_backtrace then takes end as its T.
struct BeamLm {
    LmView table{};               // device slots
    const int32_t* wid = nullptr;
    const int4* suffix = nullptr;
    double lm_panelty = 0.0;
    int32_t bos = -1;
    double* o_lm = nullptr;
    const double2* grid = nullptr;      // launch_prefix_beam_lm_grid: [G] {lm_panelty, len_bonus} on the device
};
hipError_t launch_beam_lm_prepass(const int32_t* idx, int nb, int W, int k, int C, const int32_t* T, const int32_t* words,
                                  int32_t* wid, int4* suffix, int32_t* end, hipStream_t s);
hipError_t launch_prefix_beam_lm(const int32_t* idx, const float* lp, int nb, int W, int k, int C, int beam, int nbest,
                                 double len_bonus, const int32_t* end, const BeamLm& lm, int2* hist, int32_t* len,
                                 double* logp, double* score, int32_t* cnt, hipStream_t s);
// launch_prefix_beam_lm_grid (hctr_lm_sweep*): the 1-best of launch_prefix_beam_lm for every line b = 0..nb-1 under
//   every pair g = 0..G-1 of lm.grid, in one launch of G * nb workgroups, b fastest. Grid line g * nb + b reads line b's
//   lists, lm.wid, lm.suffix and end[b] and owns hist[(g * nb + b) * W * beam ..] and place g * nb + b of len, logp,
//   score, cnt, lm.o_lm; lm.lm_panelty is unread. launch_prefix_backtrace then takes G * nb lines, end and wrap = nb.
hipError_t launch_prefix_beam_lm_grid(const int32_t* idx, const float* lp, int nb, int W, int k, int C, int beam, int G,
                                      const int32_t* end, const BeamLm& lm, int2* hist, int32_t* len, double* logp,
                                      double* score, int32_t* cnt, hipStream_t s);

// ---- the skip search (hctr_nbest_skip*): __cbs_skip__ on the thresholded candidate lists in the padded layout - row
// r = t*nb + b has cnt[r] candidates, the first min(cnt[r], kBeamMaxK) of them in ascending class order at
// ci / cl[r * kBeamMaxK ..], and its blank log-prob at bl[r] ----
// launch_beam_lm_prepass serves it with k = 1 lists of the top-1 classes; its wid may be null (no word ids of the lists
//   are written) and so may words (the zero LM: the suffixes are then unspecified and unread).
// launch_prefix_beam_skip: over end[b] steps, rows with one candidate update the list in place, the others are ranked
//   steps over the row's candidates; outputs as launch_prefix_beam_lm (lm.o_lm always written: 0 in used slots for the
//   zero LM, which is lm.table.slots == null and needs no words / suffix) plus status[nb] (0 ok, 1 empty greedy text, 2
//   the list emptied, 3 a row beyond kBeamMaxK candidates: not searched) and ranked[nb] (rows with cnt != 1 among the
//   end[b] steps). words[C] = label -> word id on the device. launch_prefix_backtrace takes end as its T.
hipError_t launch_prefix_beam_skip(const int32_t* cnt, const int32_t* ci, const float* cl, const float* bl, int nb, int W,
                                   int C, int beam, int nbest, double len_bonus, const int32_t* end, const int32_t* words,
                                   const BeamLm& lm, int2* hist, int32_t* len, double* logp, double* score,
                                   int32_t* o_cnt, int32_t* status, int32_t* ranked, hipStream_t s);

// ---- keyword spotting (hctr_spot*): one wave64 per (line, query) pair over the emissions of launch_ctc_lse, whose
// tables give every line the chunk's class list (slot 0 = blank). Local slots of a query: 0 = blank, 1..nq = its distinct
// classes in ascending order, nq + 1 = `rest` (formed per column), nq + 2 = the constant 1 (the accepting state's loop).
// A query's automaton in `blob`, at word qoff[k]:
//   L, nq, maxdeg, nedges | qslot[L] (local slot of q_j) | ptr[2L + 1] (in-edge CSR over the states Z, N_1..N_{L-1},
//   B_1..B_{L-1}, A) | mask_lo[2L], mask_hi[2L] (the local slots a state sends to Z) | edge[nedges] = src | slot << 8
constexpr int kSpotMaxLen = 32;                       // HCTR_SPOT_MAX_LEN: 2L states fill one wave
constexpr int kSpotSlots = kSpotMaxLen + 3;
constexpr int kSpotMaxEdges = (2 * kSpotMaxLen - 1) * (kSpotMaxLen + 1) + 1;      // one edge per (state, class) + A's loop
struct SpotArgs {
    const float* emis;        // [nb][W][D]
    const int32_t* T;         // [B] columns that count, indexed by b0 + b
    int b0, nb, W, D;
    const int32_t* blob;
    const int32_t* qoff;      // [Q]
    const int32_t* pair_q;    // [npairs] query of each of the launch's pairs
    const int32_t* gslot;     // [npairs][kSpotSlots] emission slot (of D) of the pair's local slots 0..nq
    int npairs, Q;
    float* contain;           // [B][Q] each, or null
    float* seg;
    int32_t* seg_start;
    int32_t* seg_end;
};
hipError_t launch_spot(const SpotArgs& a, hipStream_t s);

// ---- lexicon recognition (hctr_lexicon*): the CTC forward over the trie of a lexicon, one workgroup per (line, unit)
// over the emissions of launch_ctc_lse. The tables are those of lex_flat.h, flat over the units: unit u's local nodes are
// [uoff[u], uoff[u + 1]) (local node 0 = the root), its classes [coff[u], coff[u + 1]). ----
struct LexArgs {
    const float* emis;        // [nb][W][D]
    const int32_t* T;         // [B] columns that count, indexed by b0 + b
    int b0, nb, W, D;
    const int32_t* uoff;      // [units + 1]
    const int32_t* coff;      // [units + 1]
    const int32_t* node;      // [total] local parent | kLexSkip | kLexFirst
    const int32_t* kidx;      // [total] place of the node's label in its unit's class list (0 = the blank)
    const int32_t* eptr;      // [total + 1] the entries that end on an owned local node: elist[eptr[i] .. eptr[i + 1])
    const int32_t* elist;
    const int32_t* umap;      // [coff[units]] per call: the emission slot (of D) of every unit class in its chunk
    int u0, nu, max_unit;     // the launch's units [u0, u0 + nu); the largest unit of the lexicon
    int N;
    float* score;             // [B][N]
};
hipError_t launch_lexicon_trie(const LexArgs& a, hipStream_t s);
// cls[b][j] = list[j], nd[b] = D for b < B: the per-line tables launch_ctc_lse reads, for a chunk's class list
hipError_t launch_lexicon_classes(const int32_t* list, int D, int B, int32_t* cls, int32_t* nd, hipStream_t s);
// per line of score [B][N] (prior [N] or null): rank = (double)score + (double)prior; log_total; the n <= kLexMaxTop best
// entries by (rank descending, index ascending) without those at -inf, unused places -1 / -inf; count
constexpr int kLexMaxTop = 32;
hipError_t launch_lexicon_rank(const float* score, const float* prior, int B, int N, int n, int32_t* top_entry,
                               float* top_logp, double* top_rank, double* log_total, int32_t* count, hipStream_t s);

// ---- pattern-constrained recognition (hctr_pattern*): the CTC forward (sum) and Viterbi (max) recursions over the CTC
// lift of a DFA (pat_flat.h), one workgroup per line over the emissions of launch_ctc_lse; then the walk back. ----
struct PatArgs {
    const float* emis;        // [nb][W][D]
    const int32_t* T;         // [B] columns that count, indexed by b0 + b
    int b0, nb, W, D, S, E;
    const int32_t* slot;      // [S] emission slot of a state (0 = the blank)
    const int32_t* label;     // [S] its class
    const int32_t* in_ptr;    // [S + 1] state s is fed by in_src[in_ptr[s] .. in_ptr[s + 1]), sources ascending
    const uint16_t* in_src;   // [E]
    const int32_t* accept;    // [num_accept] ascending
    const int32_t* start;     // [num_start] ascending
    int num_accept, num_start;
    uint16_t* bp;             // [nb][W][S] backpointers of the launch's lines (Viterbi only)
    float* logp;              // [B], indexed by b0 + b, as are best and endst
    float* best;
    int32_t* endst;           // the best accepted path's last state, -1 = there is none
};
// viterbi = false: logp alone (no backpointers, best, endst), with the bits of the full launch's logp
hipError_t launch_pattern(const PatArgs& a, bool viterbi, hipStream_t s);
// whether launch_pattern stages the edge list of a pattern of S states and E edges in LDS
bool pattern_edges_in_lds(int S, int E, bool viterbi);
// NPT of the instance launch_pattern / launch_pattern_weighted run for S states: 1, 2, 4 or 8
int pattern_states_per_thread(int S);
// a weighted pattern (kind 2): PatArgs plus one float per in-edge, per accepting state and per start state.
//   x_j = a_{t-1}(src_j) + in_w[j] (one float32 addition), then the log-sum and the max over the x_j as above;
//   t = 0: lp_0 + start_w; the end: over a_{T-1}(s) + accept_w; logp is not clamped to 0.
struct PatWeights {
    const float* in_w = nullptr;      // [E] parallel to in_src
    const float* accept_w = nullptr;  // [num_accept]
    const float* start_w = nullptr;   // [num_start]
};
hipError_t launch_pattern_weighted(const PatArgs& a, const PatWeights& w, bool viterbi, hipStream_t s);
// whether launch_pattern_weighted stages the edge weights in LDS beside the edge list (2*S*(8 or 4) + 6*E <= 160 KiB);
// else the edge list alone where pattern_edges_in_lds says so, and the weights are read through L2
bool pattern_weights_in_lds(int S, int E, bool viterbi);
// the walk back from endst over bp, and what follows from the path, all [B][W] indexed by b0 + b: path = the class per
// column (-1 for t >= T and for a line without an accepted path); labels / lengths = its collapse; span_start, span_end
// = each character's first column and the column after its run; char_logp = the float32 sum of its emissions in
// ascending t; zeros beyond lengths. lpv [nb][W] is scratch.
struct PatTraceArgs {
    const float* emis;
    const int32_t* T;
    int b0, nb, W, D, S;
    const int32_t* slot;
    const int32_t* label;
    const uint16_t* bp;
    const int32_t* endst;
    float* lpv;
    int32_t *path, *labels, *lengths, *span_start, *span_end;
    float* char_logp;
};
hipError_t launch_pattern_trace(const PatTraceArgs& a, hipStream_t s);

// the set form of a pattern (pat_build_sets): the same recursions in block form - per step the totals of every block
// (beta_p and every eps_(p,.)), then the states from the totals of their source blocks. Outputs as PatArgs's.
struct PatSetArgs {
    const float* emis;        // [nb][W][D]
    const int32_t* T;         // [B]
    int b0, nb, W, D, S, nQ;
    const uint32_t* meta;     // [2 * S] slot | in-arcs << 16 | start << 31; the first in-arc
    const int32_t* blk_ptr;   // [nQ + 1] the eps states of block p are nQ + [blk_ptr[p], blk_ptr[p + 1])
    const uint32_t* in_arc;   // p | (eps_(p,c) or 0xFFFF) << 16, ascending p
    const int32_t* finals;    // [num_finals] the final DFA states, ascending
    int num_finals;
    float* states;            // [nb][2][S] float2 when the step buffers do not fit in LDS (or are kept out), else unused
    uint16_t* bp;
    float* logp;
    float* best;
    int32_t* endst;
};
// whether launch_pattern_set keeps the two step buffers of a pattern of S states and nQ blocks in LDS
// (HCTR_PATSET_LDS=0: never)
bool pattern_set_states_in_lds(int S, int nQ, bool viterbi);
hipError_t launch_pattern_set(const PatSetArgs& a, bool viterbi, hipStream_t s);

// ---- word-sequence recognition (hctr_words*): token passing over the looped trie (lex_words.h), Viterbi, one workgroup
// per line over the emissions of launch_ctc_lse; then the walk back over the columns' exit records. ----
struct WordsRec {             // an exit record: the best way to end a word after a column (16 bytes)
    float score;              // a(state) + x_v; -inf = none
    int32_t node;             // the end node v
    int32_t last;             // the emission slot of the column's label: slot[v], or 0 for the blank state
    uint32_t origin;          // the winning state's origin: s << 2 | k
};
struct WordsArgs {
    const float* emis;        // [nb][W][D]
    const int32_t* T;         // [B] columns that count, indexed by b0 + b
    int b0, nb, W, D, nn;     // nn trie nodes, the root included
    const int32_t* node;      // [nn] parent | kLexSkip | kLexFirst
    const int32_t* slot;      // [nn]
    const int32_t* entry;     // [nn] e_v or -1
    const float* weight;      // [nn] x_v
    void* states;             // [nb][2][nn] 16-byte states of the scratch form; null: the step buffers live in LDS
    WordsRec* rec;            // [nb][W][2]
};
constexpr int kWordsLdsNodes = 4096;          // the largest trie whose step buffers fit LDS
hipError_t launch_words_trie(const WordsArgs& a, hipStream_t s);
struct WordsTraceArgs {
    const WordsRec* rec;      // [nb][W][2]
    const int32_t* T;
    int b0, nb, W, nn, max_words;
    const int32_t *node, *slot, *entry, *cls;
    float* score;             // [B]
    int32_t *count, *words, *starts, *labels, *lengths;      // [B], [B][max_words] x 2, [B][W], [B]
};
hipError_t launch_words_backtrace(const WordsTraceArgs& a, hipStream_t s);

// ---- line preprocessing (preprocess.hip): cv2.resize(..., INTER_AREA) of ragged u8 images to height out_h ----
struct ResizeLine {
    int64_t src_off;          // byte offset of the image inside the packed source buffer
    int32_t sh, sw;           // source height, width
    int32_t ch;               // 1 = gray, 3 = BGR (cv2.imread order), -3 = RGB (PIL order)
    int32_t dw;               // destination width (columns >= dw of the line's output row are zeroed)
    int32_t mode;             // 0 area, 1 integer decimation (ix, iy), 2 enlarging bilinear variant
    int32_t ix, iy;
    double scale_x, scale_y;  // 1 / inv_*
    double inv_x, inv_y;      // dw / sw, out_h / sh
};
hipError_t launch_resize_lines(const uint8_t* packed, const ResizeLine* lines, int n, uint8_t* out, int out_h, int out_w,
                               hipStream_t s);

}  // namespace hctr
