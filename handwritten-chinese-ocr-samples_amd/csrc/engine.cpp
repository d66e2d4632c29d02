// libhctr_hip.so - host side of the MI355X hctr engine: context, checkpoint ingest (BatchNorm
// folding + repack to kernel layouts), workspace, forward orchestration, and the C ABI declared in
// include/hctr_hip.h. Reference citations are relative to the reference repository root.
#include "../../include/hctr_hip.h"
#include "kernels.h"

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <iterator>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <vector>

using namespace hctr;

namespace {

constexpr int kImgH = 128;                       // hctr_model.img_height, models/handwritten_ctr_model.py:159
constexpr int kFeat = 2048;                      // 512 channels x 4 rows, :168-169
constexpr double kBnEps = 1e-5;                  // nn.BatchNorm2d default
constexpr int kStagePlanes[4] = {128, 256, 512, 512};
constexpr int kStageBlocks[4] = {2, 4, 5, 1};    // ResNet(1, 512, BasicBlock, [2,4,5,1]), :166
constexpr int kSeBlocks = 2 + 4 + 5 + 1;         // SE layers = blocks of the trunk (one statistics slot each)
constexpr int kStageH[5] = {128, 64, 32, 16, 8}; // rows entering stage s (stage 0 = stem)
constexpr int64_t kDefaultMaxCols = 131072;      // pixel columns (B*W) per internal pass

std::string g_create_error;

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
    mutable bool used = false;
};

struct ConvW {
    half_t* w = nullptr;    // [taps][coutPad][cin] fp16, MFMA row order
    float* bias = nullptr;  // [coutPad]
    int cin = 0, cout = 0, coutPad = 0, taps = 0;
};

struct SeW {
    float* w1 = nullptr;    // [c/16][c]
    float* w2 = nullptr;    // [c][c/16]
    int c = 0;
};

struct BlockW {
    ConvW conv1, conv2, ds;
    SeW se;
    bool has_ds = false;
};

struct Workspace {
    int B = 0, W = 0, Wa = 0;
    void* img = nullptr;            // staged input (u8 or f32)
    int32_t* widths = nullptr;
    half_t* s0 = nullptr;           // conv0_1 output [B][130][Wa][64]
    half_t* x[5] = {};              // x[s]: input of stage s (s = 1..4), padded NHWC
    half_t* p[5][3] = {};           // rotating block buffers of stage s
    half_t* headin = nullptr;       // [B*W][2048], k = h*512 + c
    float* logits = nullptr;        // [B*W][Cpad]
    float* se_part = nullptr;
    float* se_scale = nullptr;      // [kSeBlocks][B][512]: one slot per block, so that hctr_debug_se can read them back
    float* se_border = nullptr;     // [B][4][8 segments][512]
    float* se_mean = nullptr;       // [kSeBlocks][B][512]
    int32_t* se_counter = nullptr;  // [B] last-block-done tickets of se_premean (zero between launches)
    int32_t* colidx = nullptr;      // [B*W]
    float* amax_val = nullptr;      // [P][B*W] fused head argmax partials, P <= Cpad/64
    int32_t* amax_idx = nullptr;
    int32_t* labels = nullptr;      // [B][W]
    int32_t* lengths = nullptr;     // [B]
    // fused beam front end (WS_BEAM, carved on first use): see ConvArgs in kernels.h
    float* psum = nullptr;          // [P][B*W]
    float* blank_logit = nullptr;   // [B*W]
    float* row_thr = nullptr;       // [B*W][2]
    int32_t* emit_cnt = nullptr;    // [B*W]
    int32_t* emit_list = nullptr;   // [B*W][kBeamCap][2]
    double* esum = nullptr;         // [P][B*W]
    int32_t* overflow = nullptr;    // [1]
    int32_t* bm_idx = nullptr;      // [B*W][kBeamMaxK] outputs of the fused front end (rows r = t*B + b), before the D2H
    float* bm_lp = nullptr;         // [B*W][kBeamMaxK]
    float* bm_bl = nullptr;         // [B*W]
    float* bm_st = nullptr;         // [B*W][2]
    int32_t* bm_cnt = nullptr;      // [B*W]
    int32_t* tile_ctrs = nullptr;   // [64 launches][8 XCDs] tile queues of the persistent conv variant (HCTR_PERSIST=2)
    // guarded precision (WS_GUARD): runner-up / |logit| partials of the fused head, per-column and per-line figures
    float* amax_val2 = nullptr;     // [P][B*W]
    float* amax_abs = nullptr;      // [P][B*W]
    float* col_margin = nullptr;    // [B*W] top-1 minus top-2 logit
    float* col_abs = nullptr;       // [B*W] max |logit|
    float* line_guard = nullptr;    // [B][2] = {min margin, max |logit|} per line
    int features = 0;               // WS_* sets carved into this layout
    bool split = false;             // layout of the f16x3 planes (3x the activation channels)
    bool aliased = false;           // activation buffers shared between the stages (see ensure_workspace)
};

// optional parts of a workspace layout (carved behind the core buffers, so adding one moves nothing)
enum WsFeature { WS_S0 = 1, WS_LOGITS = 2, WS_BEAM = 4, WS_GUARD = 8 };

// one resident set of device weights in kernel layouts; set 0 = f16, set 1 = f16x3 ([w_hi | w_hi | w_lo] rows)
struct WeightSet {
    float* stem_w = nullptr;
    float* stem_b = nullptr;
    ConvW conv0_2;
    std::vector<BlockW> blocks[4];
    ConvW stage_conv[4];
    ConvW head;
    bool built = false;
};

struct ProfEntry {
    std::string name;
    hipEvent_t e0, e1;
};

}  // namespace

struct hctr_ctx {
    int device = 0;
    int num_classes = 0;
    int cpad = 0;
    hipStream_t stream = nullptr;
    std::string err;
    std::map<std::string, HostTensor> host;
    bool finalized = false;
    // device weights: the sets the precision mode chosen before hctr_finalize_weights needs (mode 2 keeps both)
    WeightSet wset[2];
    const WeightSet& wts() const { return wset[split ? 1 : 0]; }
    std::vector<void*> wallocs;
    // ONE device arena holds the workspace of whatever (lines, width) shape is active: a new shape re-carves the
    // pointers and re-zeroes the stored conv borders (a small kernel), it does not allocate - ragged workloads present a
    // new padded width with almost every batch. The arena grows to the largest layout seen.
    Workspace ws;
    char* arena = nullptr;
    size_t arena_cap = 0;
    int ws_sticky = 0;                  // optional parts this context has needed so far (kept in later layouts)
    int64_t arena_reallocs = 0, ws_recarves = 0;
    int ws_alias = -1;                  // HCTR_WS_ALIAS: 1 = stages share four activation buffers, 0 = never, -1 (default) = when
                                        // the dedicated layout would exceed ws_dedicated_max bytes or the device's free memory
    size_t ws_dedicated_max = (size_t)16 << 30;      // HCTR_WS_DEDICATED_MAX_GB
    int64_t max_cols = kDefaultMaxCols;
    bool big_tiles = true;
    int halo_mode = 2;
    // f16x3 precision mode: every activation and weight is carried as hi + lo fp16 pairs; a conv sees
    // tripled input channels [x_hi | x_lo | x_hi] against weight rows [w_hi | w_hi | w_lo], so the MFMA
    // main loops are unchanged and the products w_hi*x_hi + w_hi*x_lo + w_lo*x_hi are summed in fp32.
    // `split` is the arithmetic of the pass being run; `mode` is what the caller asked for: 0 = f16, 1 = f16x3,
    // 2 = guarded ("auto"): every line runs in f16, the fused head also yields each column's top-1/top-2 logit margin,
    // and the lines with a column whose margin is within twice the guard's own tolerance (guard_rel * max|logit of the
    // line| + guard_abs, per line) are run again in f16x3 at the same padded width.
    int mode = 0;
    bool split = false;
    // HCTR_X3_MASK (diagnostic, tests/diag_precision_attribution.py): which classes of rounding points the f16x3 mode
    // carries as hi + lo; a cleared bit rounds that class to one fp16 value like the f16 mode. 1 = conv weights,
    // 2 = conv1 outputs of the blocks, 4 = block outputs (the residual stream), 8 = stem and stage-conv outputs,
    // 16 = head input and head weights. Default 31 = the f16x3 mode proper.
    int x3_mask = 31;
    int out_class = 8;               // rounding-point class of the conv being launched (set by run_block / run_forward)
    // mode 2's criterion, THE place its defaults are defined (hctr_get_guard reads them back). rel = 1.5 x 0.0114, the
    // largest per-line max|f16 - f16x3| / max|logit of the line| measured over tests/guard_cases.py, rounded up to two
    // digits ("Guard defaults"); abs covers the part of the error that does not shrink with a
    // line's scale.
    double guard_rel = 0.018, guard_abs = 0.05;
    // guard figures of the last call in mode 2 (per line of that call's batch)
    std::vector<float> g_margin, g_scale;
    std::vector<uint8_t> g_flag;
    int64_t g_flagged_total = 0, g_lines_total = 0;      // running totals over the context's lifetime
    std::vector<std::vector<int32_t>> h_widths;          // gathered widths of this call's passes (source of async copies:
                                                         // kept until the next call; every call drains the stream first)
    std::vector<int32_t> h_labels, h_lengths;            // labels of a re-run pass before they are scattered
    char* pin = nullptr;                                 // pinned host staging of the beam front end's D2H copies
    size_t pin_cap = 0;
    int chm() const { return split ? 3 : 1; }      // channel multiplier of activation buffers
    bool fuse_se = true;
    std::string stamp_layer;         // hctr_debug_stamps: layer whose workgroups are time-stamped (diagnostic)
    unsigned long long* stamp_buf = nullptr;
    int64_t stamp_cap = 0, stamp_n = 0;
    bool fuse_ds = true;             // 1x1 downsample inside conv2's K loop (HCTR_FUSE_DS=0: own launch + residual)
    bool fuse_argmax = true;         // greedy: argmax in the head GEMM's epilogue (HCTR_FUSE_ARGMAX=0: separate pass)
    bool persist_dynamic = false;    // HCTR_PERSIST=2: persistent conv workgroups drawing tiles from an atomic queue
    int conv_seq = 0;                // conv launches of the current forward (one queue each)
    bool fuse_stem = true;           // conv0_1 inside conv0_2's loader (HCTR_FUSE_STEM=0: own launch + 16 kB/column buffer)
    bool fuse_beam = true;           // beam front end without stored logits (HCTR_FUSE_BEAM=0: logits + row_topk)
    int64_t beam_fallbacks = 0;      // passes that overflowed a row list and were redone through the logits
    // profiling
    bool profiling = false;
    std::vector<ProfEntry> prof;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    // beam front-end scratch + the candidate lists of the last hctr_beam_frontend call
    std::vector<void*> beam_allocs;
    std::vector<int64_t> cand_off;
    std::vector<int32_t> cand_idx;
    std::vector<float> cand_logp;
    // CTC loss scratch (hctr_ctc_loss*): per-line tables, per-line results and the emission rows; grows, never shrinks
    char* ctc_buf = nullptr;
    size_t ctc_cap = 0;
    // device copy of the most recently used hctr_lm (hctr_nbest_lm*): its table and label -> word map, recognised by
    // the serial number stored in the object (0 = none)
    LmSlot* lm_slots = nullptr;
    int32_t* lm_words = nullptr;
    uint64_t lm_serial = 0;
    // device copy of the most recently used hctr_lex (hctr_lexicon*): its unit tables in one block, likewise
    int32_t* lex_dev = nullptr;
    uint64_t lex_serial = 0;
    // device copy of the most recently used hctr_pat (hctr_pattern*): its tables in one block, likewise
    int32_t* pat_dev = nullptr;
    uint64_t pat_serial = 0;
    // device copy of the word tables (hctr_words*) of the most recently used hctr_lex and word_bonus, likewise
    // and the host tables they were packed from (words_tab_serial = 0: none), kept so that a call on the same lexicon and
    // bonus builds nothing
    int32_t* words_dev = nullptr;
    uint64_t words_serial = 0;
    float words_bonus = 0.f;
    WordTables words_tab;
    uint64_t words_tab_serial = 0;
    float words_tab_bonus = 0.f;
};

namespace {

int fail(hctr_ctx* c, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

// The ABI promises that no C++ exception crosses it (include/hctr_hip.h): every extern "C" body runs inside
// guard(), which maps std::bad_alloc to HCTR_ERR_NOMEM and anything else to HCTR_ERR_STATE. Setting the message
// may itself allocate, so that is attempted under its own handler.
int fail_nothrow(hctr_ctx* c, int code, const char* what) noexcept {
    try {
        return fail(c, code, "%s", what);
    } catch (...) {
        return code;
    }
}

template <typename R = int, typename F>
R guard(hctr_ctx* c, F&& body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return (R)fail_nothrow(c, HCTR_ERR_NOMEM, "out of host memory (std::bad_alloc)");
    } catch (const std::exception& e) {
        return (R)fail_nothrow(c, HCTR_ERR_STATE, e.what());
    } catch (...) {
        return (R)fail_nothrow(c, HCTR_ERR_STATE, "unknown C++ exception");
    }
}

#define HIP_TRY(ctx, expr)                                                                        \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            return fail(ctx, HCTR_ERR_HIP, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr,          \
                        hipGetErrorString(_e));                                                   \
    } while (0)

// a launch (or copy) timed under a profile label
#define PROF_TRY(pf, name, expr) \
    do {                         \
        (pf).begin(name);        \
        HIP_TRY((pf).c, expr);   \
        (pf).end();              \
    } while (0)

#define TRY(expr)                   \
    do {                            \
        int _r = (expr);            \
        if (_r != HCTR_OK) return _r; \
    } while (0)

template <typename T>
int dev_alloc(hctr_ctx* c, std::vector<void*>& pool, T** out, size_t count, bool zero, size_t* acct = nullptr) {
    void* p = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess)
        return fail(c, HCTR_ERR_NOMEM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
    pool.push_back(p);
    if (acct) *acct += bytes;
    if (zero) HIP_TRY(c, hipMemsetAsync(p, 0, bytes, c->stream));
    *out = (T*)p;
    return HCTR_OK;
}

void free_pool(std::vector<void*>& pool) {
    for (void* p : pool) (void)hipFree(p);
    pool.clear();
}

struct PoolGuard {          // frees a call's temporaries on every exit path, exceptions included
    std::vector<void*>& pool;
    ~PoolGuard() { free_pool(pool); }
};

constexpr size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// caller logits of n floats on the device: the caller's own pointer, or a pooled copy of the host's, queued on the stream
int logits_on_device(hctr_ctx* c, std::vector<void*>& pool, const float* logits, int on_device, size_t n,
                     const float** dev) {
    *dev = logits;
    if (on_device) return HCTR_OK;
    float* up = nullptr;
    TRY(dev_alloc(c, pool, &up, n, false));
    *dev = up;
    HIP_TRY(c, hipMemcpyAsync(up, logits, n * 4, hipMemcpyHostToDevice, c->stream));
    return HCTR_OK;
}

// a result's copy to the host, queued on the stream; nothing when the caller does not want it (dst null) or it is empty
hipError_t fetch(hctr_ctx* c, void* dst, const void* src, size_t bytes) {
    return dst && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
}

// the end of a call that queued work: wait for the stream; a sync error does not mask an earlier one
int synced(hctr_ctx* c, int rc) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (rc == HCTR_OK && e != hipSuccess) rc = fail(c, HCTR_ERR_HIP, "stream sync: %s", hipGetErrorString(e));
    return rc;
}

// ---------------------------------------------------------------------------------------------
// checkpoint ingest
// ---------------------------------------------------------------------------------------------
const HostTensor* find(hctr_ctx* c, const std::string& key) {
    auto it = c->host.find(key);
    return it == c->host.end() ? nullptr : &it->second;
}

int need(hctr_ctx* c, const std::string& key, std::vector<int64_t> shape, const HostTensor** out) {
    const HostTensor* t = find(c, key);
    if (!t) return fail(c, HCTR_ERR_KEY, "Missing key(s) in state_dict: \"%s\"", key.c_str());
    if (t->shape != shape) {
        std::string got, want;
        for (auto v : t->shape) got += std::to_string(v) + ",";
        for (auto v : shape) want += std::to_string(v) + ",";
        return fail(c, HCTR_ERR_SHAPE, "size mismatch for %s: checkpoint [%s] vs model [%s]", key.c_str(),
                    got.c_str(), want.c_str());
    }
    t->used = true;
    *out = t;
    return HCTR_OK;
}

// stored row s of a 64-row block holds cout perm64(s): MFMA tile j = s/16, row ra = s%16 (lane group
// q = ra>>2, element i = ra&3) of that tile is cout (j>>1)*32 + q*8 + (j&1)*4 + i, so an accumulator lane
// owns two runs of 8 consecutive couts and the four lanes of a pixel store 64 contiguous bytes at a time.
inline int perm64(int s) {
    const int j = s >> 4, ra = s & 15;
    return (j >> 1) * 32 + (ra >> 2) * 8 + (j & 1) * 4 + (ra & 3);
}

// Conv2d + eval BatchNorm2d folded: w' = w * g/sqrt(v+eps), b' = (b - mean) * g/sqrt(v+eps) + beta
// (models/handwritten_ctr_model.py:37-40, 73-92, 104-108). Folded in float64, stored fp16 / fp32.
int build_conv(hctr_ctx* c, const std::string& ck, const std::string& bk, int cin, int cout, int ks,
               bool has_bias, int pad_to, ConvW* out) {
    const HostTensor *w, *b = nullptr, *g, *beta, *mean, *var;
    TRY(need(c, ck + ".weight", {cout, cin, ks, ks}, &w));
    if (has_bias) TRY(need(c, ck + ".bias", {cout}, &b));
    TRY(need(c, bk + ".weight", {cout}, &g));
    TRY(need(c, bk + ".bias", {cout}, &beta));
    TRY(need(c, bk + ".running_mean", {cout}, &mean));
    TRY(need(c, bk + ".running_var", {cout}, &var));
    const int taps = ks * ks;
    const int coutPad = (cout + pad_to - 1) / pad_to * pad_to;
    const int cinp = c->chm() * cin;               // stored row length ([w_hi | w_hi | w_lo] when split)
    std::vector<half_t> hw((size_t)taps * coutPad * cinp, (half_t)0.f);
    std::vector<float> hb(coutPad, 0.f);
    double wmax = 0.0;
    for (int blk = 0; blk < coutPad / 64; ++blk)
        for (int s = 0; s < 64; ++s) {
            const int co = blk * 64 + perm64(s);
            if (co >= cout) continue;
            const double sc = (double)g->data[co] / std::sqrt((double)var->data[co] + kBnEps);
            for (int t = 0; t < taps; ++t)
                for (int ci = 0; ci < cin; ++ci) {
                    const double v = (double)w->data[((size_t)co * cin + ci) * taps + t] * sc;
                    wmax = std::max(wmax, std::fabs(v));
                    half_t* row = &hw[((size_t)t * coutPad + blk * 64 + s) * cinp];
                    const half_t hi = (half_t)(float)v;
                    row[ci] = hi;
                    if (c->split) {
                        row[cin + ci] = hi;
                        row[2 * cin + ci] = (c->x3_mask & 1) ? (half_t)(float)(v - (double)(float)hi) : (half_t)0.f;
                    }
                }
        }
    for (int co = 0; co < cout; ++co) {
        const double sc = (double)g->data[co] / std::sqrt((double)var->data[co] + kBnEps);
        const double bb = has_bias ? (double)b->data[co] : 0.0;
        hb[co] = (float)((bb - (double)mean->data[co]) * sc + (double)beta->data[co]);
    }
    if (!(wmax < 65000.0))      // also catches NaN; fp16 storage cannot hold it (degenerate running_var?)
        return fail(c, HCTR_ERR_ARG, "%s: BatchNorm-folded weight magnitude %.3g does not fit fp16", ck.c_str(), wmax);
    out->cin = cinp; out->cout = cout; out->coutPad = coutPad; out->taps = taps;
    TRY(dev_alloc(c, c->wallocs, &out->w, hw.size(), false));
    TRY(dev_alloc(c, c->wallocs, &out->bias, hb.size(), false));
    HIP_TRY(c, hipMemcpyAsync(out->w, hw.data(), hw.size() * sizeof(half_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out->bias, hb.data(), hb.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // host vectors die at scope exit
    return HCTR_OK;
}

int build_se(hctr_ctx* c, const std::string& key, int ch, SeW* out) {
    const HostTensor *w1, *w2;
    TRY(need(c, key + ".fc.0.weight", {ch / 16, ch}, &w1));
    TRY(need(c, key + ".fc.2.weight", {ch, ch / 16}, &w2));
    out->c = ch;
    TRY(dev_alloc(c, c->wallocs, &out->w1, w1->data.size(), false));
    TRY(dev_alloc(c, c->wallocs, &out->w2, w2->data.size(), false));
    HIP_TRY(c, hipMemcpyAsync(out->w1, w1->data.data(), w1->data.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(out->w2, w2->data.data(), w2->data.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HCTR_OK;
}

int build_stem(hctr_ctx* c, WeightSet& ws) {
    const HostTensor *w, *b, *g, *beta, *mean, *var;
    TRY(need(c, "cnn.conv0_1.weight", {64, 1, 3, 3}, &w));
    TRY(need(c, "cnn.conv0_1.bias", {64}, &b));
    TRY(need(c, "cnn.bn0_1.weight", {64}, &g));
    TRY(need(c, "cnn.bn0_1.bias", {64}, &beta));
    TRY(need(c, "cnn.bn0_1.running_mean", {64}, &mean));
    TRY(need(c, "cnn.bn0_1.running_var", {64}, &var));
    std::vector<float> hw(64 * 9), hb(64);
    for (int co = 0; co < 64; ++co) {
        const double sc = (double)g->data[co] / std::sqrt((double)var->data[co] + kBnEps);
        for (int t = 0; t < 9; ++t) hw[co * 9 + t] = (float)((double)w->data[co * 9 + t] * sc);
        hb[co] = (float)(((double)b->data[co] - (double)mean->data[co]) * sc + (double)beta->data[co]);
    }
    TRY(dev_alloc(c, c->wallocs, &ws.stem_w, hw.size(), false));
    TRY(dev_alloc(c, c->wallocs, &ws.stem_b, hb.size(), false));
    HIP_TRY(c, hipMemcpyAsync(ws.stem_w, hw.data(), hw.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(ws.stem_b, hb.data(), hb.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HCTR_OK;
}

// self.linear (models/handwritten_ctr_model.py:169,175). The reference's feature index is
// d = c*4 + h (flatten(1,2) of [B,C,H,W], :173); the engine's head input is [pixel][h*512 + c].
int build_head(hctr_ctx* c, WeightSet& ws) {
    const HostTensor *w, *b;
    const int C = c->num_classes;
    TRY(need(c, "linear.weight", {C, kFeat}, &w));
    TRY(need(c, "linear.bias", {C}, &b));
    const int cpad = c->cpad;
    const int kf = c->chm() * kFeat;               // [h][hi | lo-slot | hi-slot][512] when split
    std::vector<half_t> hw((size_t)cpad * kf, (half_t)0.f);
    std::vector<float> hb(cpad, 0.f);
    for (int blk = 0; blk < cpad / 64; ++blk)
        for (int s = 0; s < 64; ++s) {
            const int n = blk * 64 + perm64(s);
            if (n >= C) continue;
            half_t* dst = &hw[(size_t)(blk * 64 + s) * kf];
            const float* src = &w->data[(size_t)n * kFeat];
            for (int ch = 0; ch < 512; ++ch)
                for (int h = 0; h < 4; ++h) {
                    const float v = src[ch * 4 + h];
                    const half_t hi = (half_t)v;
                    if (!c->split) {
                        dst[h * 512 + ch] = hi;
                    } else {                         // feature planes [x_hi | x_lo | x_hi] x [w_hi | w_hi | w_lo]
                        half_t* r = dst + h * 1536;
                        r[ch] = hi;
                        r[512 + ch] = hi;
                        r[1024 + ch] = (c->x3_mask & 16) ? (half_t)(v - (float)hi) : (half_t)0.f;
                    }
                }
        }
    for (int n = 0; n < C; ++n) hb[n] = b->data[n];
    ws.head.cin = kf; ws.head.cout = C; ws.head.coutPad = cpad; ws.head.taps = 1;
    TRY(dev_alloc(c, c->wallocs, &ws.head.w, hw.size(), false));
    TRY(dev_alloc(c, c->wallocs, &ws.head.bias, hb.size(), false));
    HIP_TRY(c, hipMemcpyAsync(ws.head.w, hw.data(), hw.size() * sizeof(half_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(ws.head.bias, hb.data(), hb.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return HCTR_OK;
}

// ---------------------------------------------------------------------------------------------
// workspace: padded NHWC fp16 activations, one set of buffers per stage (borders stay zero)
// ---------------------------------------------------------------------------------------------
inline int64_t act_elems(int B, int H, int Wa, int C) { return (int64_t)B * (H + 2) * Wa * C; }

// class parts per row written by the fused head epilogues: n-tiles x wave columns. The 256x256 head tile gives
// cpad/128 parts, the 128x128 tile (HCTR_BIG_TILES=0, or cpad not a multiple of 256) cpad/64: buffers are sized for
// the larger figure, launches use head_parts(c).
inline int head_parts_max(const hctr_ctx* c) { return c->cpad / 64; }
inline int head_parts(const hctr_ctx* c) {
    const int hbm = (c->big_tiles && c->cpad % 256 == 0) ? 256 : 128;
    return (c->cpad / hbm) * kLinearWN;
}

int ensure_workspace(hctr_ctx* c, int B, int W, int features = 0) {
    c->ws_sticky |= features;
    bool same_shape = c->ws.B == B && c->ws.W == W && c->ws.split == c->split;
    int feat = c->ws_sticky;
    if (c->fuse_stem && !c->split) feat &= ~WS_S0;        // (mode 2 alternates layouts: conv0_1's buffer only where it is used)
    if (same_shape && (c->ws.features & feat) == feat) return HCTR_OK;
    const int tilesW = (W + kTileW - 1) / kTileW;        // 16-column tiles (upper bound on tiles per row)
    const int Wa = (W + 31) / 32 * 32 + 2;               // room for the widest (32-column) tile + border
    const size_t cols = (size_t)B * W;
    const int m = c->chm();
    // ---- layout: byte offsets into the arena, 256-byte aligned; core buffers first, optional parts behind them.
    // Activation buffers, DEDICATED layout (default): every stage owns its input x[s] and three rotating block buffers,
    // so a buffer keeps one geometry and its stored zero border survives from forward to forward (~245 kB per pixel
    // column). ALIASED layout (HCTR_WS_ALIAS=1, or automatically when the dedicated one does not fit): four buffers of
    // the largest stage geometry serve all stages - x[s] is pool 0 for every s (a stage input is dead after the stage's
    // first block, long before conv_s+pool writes the next one), p[s][i] is pool 1 + i (dead once conv_s+pool has read
    // the stage's last output) - ~95 kB per column; a buffer then changes geometry from stage to stage, so run_forward
    // re-zeroes the borders at every stage entry (+15 small launches, ~0.5 % of a step).
    Workspace ws;
    size_t off = 0;
    std::vector<std::pair<void**, size_t>> slots;
    half_t* pool4[4] = {};
    auto layout = [&](bool alias) {
        ws = Workspace();
        ws.B = B; ws.W = W; ws.features = feat; ws.split = c->split; ws.Wa = Wa; ws.aliased = alias;
        off = 0;
        slots.clear();
        auto A = [&](auto** out, size_t count) {
            slots.emplace_back((void**)out, off);
            off += (std::max<size_t>(count * sizeof(**out), 16) + 255) & ~(size_t)255;
        };
        A((char**)&ws.img, cols * kImgH * 4);
        A(&ws.widths, (size_t)B);
        int cin = 64;
        size_t se_max = 0, pool_elems = 0;
        for (int s = 1; s <= 4; ++s) {
            const int H = kStageH[s], planes = kStagePlanes[s - 1];
            if (!alias) {
                A(&ws.x[s], (size_t)act_elems(B, H, Wa, cin * m));
                const int nbuf = (s == 4) ? 2 : 3;
                for (int i = 0; i < nbuf; ++i) A(&ws.p[s][i], (size_t)act_elems(B, H, Wa, planes * m));
            }
            pool_elems = std::max(pool_elems, (size_t)act_elems(B, H, Wa, std::max(cin, planes) * m));
            se_max = std::max(se_max, (size_t)B * (H / 8) * tilesW * planes);
            cin = planes;
        }
        if (alias)
            for (int i = 0; i < 4; ++i) A(&pool4[i], pool_elems);
        A(&ws.headin, cols * kFeat * m);
        A(&ws.se_part, se_max);
        A(&ws.se_scale, (size_t)kSeBlocks * B * 512);
        A(&ws.se_border, (size_t)B * 5 * 8 * 512);
        A(&ws.se_mean, (size_t)kSeBlocks * B * 512);
        A(&ws.se_counter, (size_t)B);
        A(&ws.colidx, cols);
        const size_t P = (size_t)head_parts_max(c);           // class parts per row of the fused head epilogues
        A(&ws.amax_val, cols * P);
        A(&ws.amax_idx, cols * P);
        A(&ws.labels, cols);
        A(&ws.lengths, (size_t)B);
        A(&ws.tile_ctrs, (size_t)64 * 8);
        // conv0_1's output (16 kB per column): only the unfused / f16x3 stem path
        if (feat & WS_S0) A(&ws.s0, (size_t)act_elems(B, 128, Wa, 64 * m));
        // [B*W][cpad] fp32 logits (3.8 GB at config 2): hctr_forward_logits and the HCTR_FUSE_* = 0 A/B paths only
        if (feat & WS_LOGITS) A(&ws.logits, cols * c->cpad);
        if (feat & WS_GUARD) {                               // guarded precision: runner-up / |logit| partials and figures
            A(&ws.amax_val2, cols * P);
            A(&ws.amax_abs, cols * P);
            A(&ws.col_margin, cols);
            A(&ws.col_abs, cols);
            A(&ws.line_guard, (size_t)2 * B);
        }
        if (feat & WS_BEAM) {                                // scratch of the fused beam front end (kernels.h ConvArgs)
            A(&ws.psum, P * cols);
            A(&ws.blank_logit, cols);
            A(&ws.row_thr, 2 * cols);
            A(&ws.emit_cnt, cols);
            A(&ws.esum, P * cols);
            A(&ws.overflow, (size_t)1);
            A(&ws.bm_idx, cols * kBeamMaxK);
            A(&ws.bm_lp, cols * kBeamMaxK);
            A(&ws.bm_bl, cols);
            A(&ws.bm_st, 2 * cols);
            A(&ws.bm_cnt, cols);
            A(&ws.emit_list, cols * kBeamCap * 2);
        }
    };
    bool alias = c->ws_alias == 1;
    layout(alias);
    if (c->ws_alias < 0) {
        // automatic: small shapes keep every stage's own buffers (no per-stage border zeroing, every debug tap readable);
        // a layout beyond ws_dedicated_max (16 GiB: about 30 lines of 2000 columns), or one that would not fit into the
        // device's free memory, uses the shared buffers (a third of the bytes, +0.3 % time)
        bool want = off > c->ws_dedicated_max;
        if (!want && off > c->arena_cap) {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && off > free_b + c->arena_cap) want = true;
        }
        if (want) {
            alias = true;
            layout(true);
        }
    }
    bool fresh = false;
    if (off > c->arena_cap) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (c->arena) (void)hipFree(c->arena);
        c->arena = nullptr; c->arena_cap = 0;
        c->ws = Workspace();
        const size_t want = off + off / 16;              // a little headroom: the next slightly wider batch fits too
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) e = hipMalloc(&p, off);
        if (e != hipSuccess)
            return fail(c, HCTR_ERR_NOMEM, "hipMalloc(%zu bytes) for the workspace of %d lines x %d columns failed: %s", off,
                        B, W, hipGetErrorString(e));
        c->arena = (char*)p;
        c->arena_cap = e == hipSuccess && want >= off ? want : off;
        ++c->arena_reallocs;
        fresh = true;
    }
    for (auto& sl : slots) *sl.first = c->arena + sl.second;
    if (ws.aliased) {
        for (int s = 1; s <= 4; ++s) {
            ws.x[s] = pool4[0];
            for (int i = 0; i < ((s == 4) ? 2 : 3); ++i) ws.p[s][i] = pool4[1 + i];
        }
    }
    if (c->ws.aliased != ws.aliased) same_shape = false;
    // ---- stored conv borders: every activation buffer's border rows / columns must read as zero. The interiors are
    //      rewritten by each forward, so after a shape change (or a new arena) only the borders are cleared. ----
    auto zero_act = [&](half_t* p, int H, int C) { return launch_zero_borders(p, B, H, W, Wa, C * m, c->stream); };
    if (fresh || !same_shape) {
        int ci = 64;
        for (int s = 1; s <= 4 && !ws.aliased; ++s) {        // (aliased layout: run_forward zeroes at every stage entry)
            const int H = kStageH[s], planes = kStagePlanes[s - 1];
            HIP_TRY(c, zero_act(ws.x[s], H, ci));
            const int nbuf = (s == 4) ? 2 : 3;
            for (int i = 0; i < nbuf; ++i) HIP_TRY(c, zero_act(ws.p[s][i], H, planes));
            ci = planes;
        }
        HIP_TRY(c, hipMemsetAsync(ws.se_counter, 0, (size_t)B * 4, c->stream));
        ++c->ws_recarves;
    }
    if (ws.s0 && (fresh || !same_shape || !c->ws.s0)) HIP_TRY(c, zero_act(ws.s0, 128, 64));
    c->ws = ws;
    return HCTR_OK;
}

// ---------------------------------------------------------------------------------------------
// forward orchestration
// ---------------------------------------------------------------------------------------------
struct Prof {
    hctr_ctx* c;
    bool on;
    explicit Prof(hctr_ctx* ctx) : c(ctx), on(ctx->profiling) {}
    hipEvent_t ev() {
        if (c->ev_used == c->ev_pool.size()) {
            hipEvent_t e;
            (void)hipEventCreate(&e);
            c->ev_pool.push_back(e);
        }
        return c->ev_pool[c->ev_used++];
    }
    void begin(const char* name) {
        if (!on) return;
        ProfEntry pe{name, ev(), ev()};
        (void)hipEventRecord(pe.e0, c->stream);
        c->prof.push_back(pe);
    }
    void end() {
        if (!on) return;
        (void)hipEventRecord(c->prof.back().e1, c->stream);
    }
};

// start of an API call: forget the previous call's per-layer events (a call may run several internal passes,
// whose entries of the same name hctr_last_profile adds up)
inline void prof_reset(hctr_ctx* c) {
    if (c->profiling) { c->prof.clear(); c->ev_used = 0; }
    c->h_widths.clear();                              // (the previous call drained the stream before it returned)
}

struct ActDesc {            // a padded NHWC activation
    half_t* p;
    int H, C;
};

// Block tile per layer: 256x256 (8 waves) halves the bytes staged per MFMA, so it is used wherever
// the layer shape allows (Cout % 256 == 0, H % 16 == 0: stages 2 and 3 = 82 % of the FLOPs).
ConvTile pick_tile(const hctr_ctx* c, const ConvW& cw, int H) {
    if (cw.cout == 64) return TILE_64x256;
    // 3x3 layers with Cout % 128 == 0 and H % 16 == 0 (stages 1-3): two 4-wave halo workgroups per CU
    if (c->halo_mode == 2 && cw.taps == 9 && cw.coutPad % 128 == 0 && H % 16 == 0) return TILE_HALO4;
    if (c->halo_mode == 2 && cw.taps == 9 && cw.coutPad % 128 == 0 && H % 8 == 0) return TILE_HALO4_8x32;   // stage 4
    if (c->big_tiles && cw.coutPad % 256 == 0 && H % 16 == 0) return TILE_256x256;
    return TILE_128x128;
}

int run_conv(hctr_ctx* c, Prof& pf, const char* name, const ConvW& cw, ActDesc in, half_t* out, int outH,
             bool relu, bool pool, float* se_part, bool to_head, const float* se_scale = nullptr,
             const half_t* resid = nullptr, const ConvW* ds = nullptr, const half_t* ds_in = nullptr,
             int stem_img_f32 = -1, bool stem_widths = false) {
    const Workspace& ws = c->ws;
    ConvArgs a{};
    a.x = in.p; a.w = cw.w; a.bias = cw.bias; a.y = out; a.se_part = se_part;
    a.se_scale = se_scale; a.resid = resid;
    a.split = c->split ? 1 : 0;
    a.drop_lo = (c->split && !(c->x3_mask & c->out_class)) ? 1 : 0;
    const int m = c->chm();                        // cw.cin already counts the tripled input channels
    a.H = in.H; a.W = ws.W; a.Cin = cw.cin; a.Cout = cw.cout; a.CoutPad = cw.coutPad;
    const ConvTile tile = pick_tile(c, cw, in.H);
    const int rows = conv_tile_rows(tile);
    if (in.H % rows != 0 || cw.cin % kBK != 0)
        return fail(c, HCTR_ERR_ARG, "conv %s: H=%d or Cin=%d not tileable", name, in.H, cw.cin);
    const int cols = conv_tile_cols(tile);
    a.tilesW = (ws.W + cols - 1) / cols;
    a.tilesH = in.H / rows;
    a.in_sb = (int64_t)(in.H + 2) * ws.Wa * cw.cin;
    a.in_sh = ws.Wa * cw.cin;
    if (a.in_sb * 2 >= ((int64_t)1 << 32) || (int64_t)(outH + 2) * ws.Wa * cw.cout * m * 2 >= ((int64_t)1 << 32))
        return fail(c, HCTR_ERR_ARG, "line width %d too large: one image's activation exceeds the kernels' 32-bit "
                    "in-image byte offsets (conv %s)", ws.W, name);
    if (to_head) {            // conv4 + pool -> head input [B][W][4][512] (x3 planes when split)
        a.out_sb = (int64_t)ws.W * kFeat * m; a.out_sh = 512 * m; a.out_sw = kFeat * m; a.out_off = 0;
        a.out_wlimit = ws.W;
    } else {
        a.out_sb = (int64_t)(outH + 2) * ws.Wa * cw.cout * m;
        a.out_sh = ws.Wa * cw.cout * m; a.out_sw = cw.cout * m;
        a.out_off = (int64_t)(ws.Wa + 1) * cw.cout * m;
        a.out_wlimit = a.tilesW * cols;
    }
    a.relu = relu; a.pool = pool;
    if (ds) {                 // fused 1x1 downsample of the block input (same H, W, Wa; ds->cin channels)
        if (tile != TILE_HALO4 || !se_scale || resid || ds->cin % kBK != 0 || ds->coutPad != cw.coutPad)
            return fail(c, HCTR_ERR_STATE, "conv %s: downsample fusion not applicable", name);
        a.ds_x = ds_in; a.ds_w = ds->w; a.ds_bias = ds->bias; a.ds_cin = ds->cin;
        a.ds_in_sh = ws.Wa * ds->cin;
        a.ds_in_sb = (int64_t)(in.H + 2) * ws.Wa * ds->cin;
    }
    a.mtiles = ws.B * a.tilesH * a.tilesW;
    a.ntiles = cw.coutPad / conv_tile_couts(tile);
    if (c->persist_dynamic && c->conv_seq < 64) a.tile_counter = ws.tile_ctrs + 8 * c->conv_seq++;
    if (c->stamp_buf && c->stamp_layer == name && (tile == TILE_HALO4 || tile == TILE_HALO4_8x32) &&
        (int64_t)a.mtiles * a.ntiles <= c->stamp_cap) {
        a.stamps = c->stamp_buf;
        c->stamp_n = (int64_t)a.mtiles * a.ntiles;
    }
    static const char* dbg_layer = getenv("HCTR_DBG_LAYER");          // timing experiments on ONE layer (kernels.hip env_dbg)
    if (dbg_layer && strcmp(dbg_layer, name) == 0)
        if (const char* e = getenv("HCTR_DBG")) a.dbg = atoi(e);
    pf.begin(name);
    if (stem_img_f32 >= 0) {      // conv0_2 with conv0_1 computed in its loader from the staged image (kernels.hip)
        if (tile != TILE_64x256 || cw.taps != 9 || cw.cin != 64 || cw.coutPad != 64 || c->split)
            return fail(c, HCTR_ERR_STATE, "conv %s: stem fusion not applicable", name);
        a.img = ws.img; a.img_f32 = stem_img_f32; a.img_widths = stem_widths ? ws.widths : nullptr;
        a.stem_w = c->wts().stem_w; a.stem_b = c->wts().stem_b;
        HIP_TRY(c, launch_stem_conv0_2(a, c->stream));
    } else {
        HIP_TRY(c, launch_conv(a, tile, cw.taps, false, c->stream));
    }
    pf.end();
    return HCTR_OK;
}

// BasicBlock.forward (models/handwritten_ctr_model.py:47-60). Fused form (default): the SE scale is
// computed from statistics of conv1's output before conv2 runs (kernels.hip, se_premean), and conv2's
// epilogue applies relu(acc * scale + residual) itself. HCTR_FUSE_SE=0 selects the unfused form
// (conv2 -> o, SE on sums of o, separate se_apply pass) for A/B runs.
int run_block(hctr_ctx* c, Prof& pf, const std::string& name, const BlockW& bw, ActDesc in, half_t* t,
              half_t* o, half_t* r, int planes, int se_slot) {
    const Workspace& ws = c->ws;
    const int H = in.H;
    float* const se_mean = ws.se_mean + (size_t)se_slot * ws.B * 512;       // this block's slot (hctr_debug_se)
    float* const se_scale = ws.se_scale + (size_t)se_slot * ws.B * 512;
    auto tiles_of = [&](const ConvW& cw) {
        const ConvTile t = pick_tile(c, cw, H);
        return (H / conv_tile_rows(t)) * ((ws.W + conv_tile_cols(t) - 1) / conv_tile_cols(t));
    };
    const float inv_hw = 1.0f / ((float)H * (float)ws.W);
    const half_t* res = in.p;
    // first block of stages 1-3: the 1x1 downsample branch runs inside conv2's K loop (kernels.hip DSFUSE) when
    // conv2 is on the default halo kernel; otherwise (A/B paths, f16x3) as its own launch writing the residual r
    const bool fuse_ds = bw.has_ds && c->fuse_ds && (c->fuse_se || c->split) && bw.ds.cin % kBK == 0 &&
                         pick_tile(c, bw.conv2, H) == TILE_HALO4;
    if (bw.has_ds && !fuse_ds) {
        c->out_class = 4;
        TRY(run_conv(c, pf, (name + ".downsample").c_str(), bw.ds, in, r, H, false, false, nullptr, false));
        res = r;
    }
    if (c->fuse_se || c->split) {
        const int tiles1 = tiles_of(bw.conv1);
        c->out_class = 2;
        TRY(run_conv(c, pf, (name + ".conv1").c_str(), bw.conv1, in, t, H, true, false, ws.se_part, false));
        c->out_class = 4;
        PROF_TRY(pf, (name + ".se_stats").c_str(), launch_se_border(t, ws.B, H, ws.W, ws.Wa, planes, c->split,
                                                                    ws.se_part, tiles1, ws.se_border, c->stream));
        PROF_TRY(pf, (name + ".se_scale").c_str(), launch_se_premean(ws.se_border, t, bw.conv2.w, bw.conv2.bias, ws.B,
                                                                     H, ws.W, ws.Wa, planes, bw.conv2.coutPad, c->split,
                                                                     se_mean, bw.se.w1, bw.se.w2, se_scale,
                                                                     ws.se_counter, c->stream));
        if (fuse_ds)
            TRY(run_conv(c, pf, (name + ".conv2+se+ds").c_str(), bw.conv2, ActDesc{t, H, planes}, o, H, true, false,
                         nullptr, false, se_scale, nullptr, &bw.ds, in.p));
        else
            TRY(run_conv(c, pf, (name + ".conv2+se").c_str(), bw.conv2, ActDesc{t, H, planes}, o, H, true, false,
                         nullptr, false, se_scale, res));
        return HCTR_OK;
    }
    c->out_class = 2;
    TRY(run_conv(c, pf, (name + ".conv1").c_str(), bw.conv1, in, t, H, true, false, nullptr, false));
    c->out_class = 4;
    TRY(run_conv(c, pf, (name + ".conv2").c_str(), bw.conv2, ActDesc{t, H, planes}, o, H, false, false,
                 ws.se_part, false));
    const int tiles = tiles_of(bw.conv2);
    PROF_TRY(pf, (name + ".se_fc").c_str(), launch_se_fc(ws.se_part, tiles, bw.se.w1, bw.se.w2, se_scale, ws.B,
                                                         planes, inv_hw, c->stream));
    PROF_TRY(pf, (name + ".se_apply").c_str(), launch_se_apply(o, res, se_scale, (int64_t)(H + 2) * ws.Wa * planes,
                                                               ws.B, planes, c->stream));
    return HCTR_OK;
}

// trunk + head for the staged batch in ws.img: leaves [B*W][cpad] fp32 logits in ws.logits, or - greedy
// decode, fused_argmax - only the per-column argmax in ws.colidx (the 29 kB-per-column logits never exist).
// ResNet.forward :115-153 and hctr_model.forward :171-176; np.argmax(preds, 2) utils/ctc_codec.py:75.
enum HeadMode { HEAD_LOGITS = 0, HEAD_ARGMAX = 1, HEAD_BEAM = 2 };

// optional workspace parts a forward in this head mode uses. Callers pass them to ensure_workspace BEFORE the input
// is staged: carving a part may move the arena, which would lose an image already copied into it.
int ws_need(const hctr_ctx* c, HeadMode mode, bool guarded = false) {
    int need = 0;
    if (mode == HEAD_LOGITS) need |= WS_LOGITS;
    if (mode == HEAD_BEAM) need |= WS_BEAM;
    if (!(c->fuse_stem && !c->split)) need |= WS_S0;
    if (guarded) need |= WS_GUARD;
    return need;
}

// the head projection's launch arguments for the active workspace (models/handwritten_ctr_model.py:175)
void head_args(hctr_ctx* c, ConvArgs* out, ConvTile* tile) {
    const Workspace& ws = c->ws;
    ConvArgs a{};
    a.x = ws.headin; a.w = c->wts().head.w; a.bias = c->wts().head.bias; a.y = ws.logits;
    a.Cin = c->wts().head.cin; a.Cout = c->num_classes; a.CoutPad = c->cpad;
    a.M = (int64_t)ws.B * ws.W; a.ldo = c->cpad;
    *tile = (c->big_tiles && c->cpad % 256 == 0) ? TILE_256x256 : TILE_128x128;
    const int hbm = *tile == TILE_256x256 ? 256 : 128;
    a.mtiles = (int)((a.M + hbm - 1) / hbm); a.ntiles = c->cpad / hbm;
    *out = a;
}

// guarded: also leave each line's {smallest top-1/top-2 logit margin, largest |logit|} in ws.line_guard (mode 2's
// f16 passes; the figures come from the head epilogue's partials, or from the stored logits in HEAD_LOGITS mode)
int run_forward(hctr_ctx* c, int img_f32, bool have_widths, HeadMode mode = HEAD_LOGITS, bool guarded = false) {
    if ((c->ws.features & ws_need(c, mode, guarded)) != ws_need(c, mode, guarded) || c->ws.split != c->split)
        return fail(c, HCTR_ERR_STATE, "workspace lacks a part this forward needs (ensure_workspace before staging)");
    Workspace& ws = c->ws;
    const WeightSet& wt = c->wts();
    if (!wt.built) return fail(c, HCTR_ERR_STATE, "the weight set of this precision mode is not resident");
    Prof pf(c);
    if (c->persist_dynamic) {
        HIP_TRY(c, hipMemsetAsync(ws.tile_ctrs, 0, 64 * 8 * 4, c->stream));
        c->conv_seq = 0;
    }
    // aliased workspace: a buffer changes geometry from stage to stage, so the stored zero borders of a stage's buffers
    // are re-established when the stage is entered (the buffers' previous users are dead by then, see ensure_workspace)
    auto zero_stage = [&](int s, bool input, bool blocks) -> int {
        if (!ws.aliased) return HCTR_OK;
        const int H = kStageH[s], planes = kStagePlanes[s - 1], cin_s = s == 1 ? 64 : kStagePlanes[s - 2];
        const int mm = c->chm();
        pf.begin("zero_borders");
        if (input) HIP_TRY(c, launch_zero_borders(ws.x[s], ws.B, H, ws.W, ws.Wa, cin_s * mm, c->stream));
        for (int i = 0; blocks && i < ((s == 4) ? 2 : 3); ++i)
            HIP_TRY(c, launch_zero_borders(ws.p[s][i], ws.B, H, ws.W, ws.Wa, planes * mm, c->stream));
        pf.end();
        return HCTR_OK;
    };
    TRY(zero_stage(1, true, true));
    c->out_class = 8;
    if (c->fuse_stem && !c->split) {
        // conv0_1's output (16 kB per pixel column) never reaches HBM: it is computed into conv0_2's LDS halo
        TRY(run_conv(c, pf, "stem+conv0_2+pool", wt.conv0_2, ActDesc{nullptr, 128, 64}, ws.x[1], 64, true, true, nullptr,
                     false, nullptr, nullptr, nullptr, nullptr, img_f32 ? 1 : 0, have_widths));
    } else {
        PROF_TRY(pf, "stem.conv0_1", launch_stem(ws.img, img_f32, have_widths ? ws.widths : nullptr, wt.stem_w,
                                                 wt.stem_b, ws.s0, ws.B, ws.W, ws.Wa,
                                                 c->split ? ((c->x3_mask & 8) ? 1 : 2) : 0, c->stream));
        TRY(run_conv(c, pf, "conv0_2+pool", wt.conv0_2, ActDesc{ws.s0, 128, 64}, ws.x[1], 64, true, true, nullptr, false));
    }
    int cin = 64, se_slot = 0;
    for (int s = 1; s <= 4; ++s) {
        const int H = kStageH[s], planes = kStagePlanes[s - 1];
        ActDesc cur{ws.x[s], H, cin};
        int ci = -1;                              // index of the buffer holding `cur`; -1 = stage input
        for (size_t i = 0; i < wt.blocks[s - 1].size(); ++i) {
            const BlockW& bw = wt.blocks[s - 1][i];
            char nm[48];
            snprintf(nm, sizeof(nm), "block%d.%zu", s, i);
            // three rotating buffers: t and o go to the two that do not hold the block input; the
            // 1x1-downsample residual (first block of stages 1-3 only) uses the third.
            const int ti = ci < 0 ? 0 : (ci + 1) % 3, oi = ci < 0 ? 1 : (ci + 2) % 3;
            if (bw.has_ds && ci >= 0) return fail(c, HCTR_ERR_STATE, "downsample only expected on a stage's first block");
            if (se_slot >= kSeBlocks) return fail(c, HCTR_ERR_STATE, "more blocks than SE slots");
            TRY(run_block(c, pf, nm, bw, cur, ws.p[s][ti], ws.p[s][oi], bw.has_ds ? ws.p[s][2] : nullptr, planes,
                          se_slot++));
            cur = ActDesc{ws.p[s][oi], H, planes};
            ci = oi;
        }
        char nm[32];
        snprintf(nm, sizeof(nm), "conv%d+pool", s);
        c->out_class = s < 4 ? 8 : 16;            // (conv4+pool writes the head input)
        if (s < 4) {
            TRY(zero_stage(s + 1, true, false));                 // x[s+1] = pool 0: dead since this stage's first block
            TRY(run_conv(c, pf, nm, wt.stage_conv[s - 1], cur, ws.x[s + 1], H / 2, true, true, nullptr, false));
            TRY(zero_stage(s + 1, false, true));                 // the block buffers: dead once the launch above has read `cur`
        } else
            TRY(run_conv(c, pf, nm, wt.stage_conv[s - 1], cur, ws.headin, H / 2, true, true, nullptr, true));
        cin = planes;
    }
    // head GEMM
    ConvArgs a;
    ConvTile htile;
    head_args(c, &a, &htile);
    auto line_guard = [&]() -> int {
        PROF_TRY(pf, "line_guard", launch_line_guard(ws.col_margin, ws.col_abs, ws.B, ws.W, ws.line_guard, c->stream));
        return HCTR_OK;
    };
    if (mode == HEAD_ARGMAX || mode == HEAD_BEAM) {
        a.y = nullptr;
        a.amax_val = ws.amax_val;
        a.amax_idx = ws.amax_idx;
        if (guarded) { a.amax_val2 = ws.amax_val2; a.amax_abs = ws.amax_abs; }
        if (mode == HEAD_BEAM) { a.psum = ws.psum; a.blank_logit = ws.blank_logit; }
        PROF_TRY(pf, mode == HEAD_BEAM ? "head.linear+partials" : "head.linear+argmax",
                 launch_conv(a, htile, 1, true, c->stream));
        if (mode == HEAD_BEAM && !guarded) return HCTR_OK;
        PROF_TRY(pf, "argmax_partials", launch_argmax_partials(ws.amax_val, ws.amax_idx, a.ntiles * kLinearWN, a.M,
                                                               mode == HEAD_BEAM ? nullptr : ws.colidx, c->stream,
                                                               a.amax_val2, a.amax_abs,
                                                               guarded ? ws.col_margin : nullptr,
                                                               guarded ? ws.col_abs : nullptr));
        if (guarded) TRY(line_guard());
        return HCTR_OK;
    }
    PROF_TRY(pf, "head.linear", launch_conv(a, htile, 1, true, c->stream));
    if (guarded) {
        PROF_TRY(pf, "row_guard", launch_row_guard(ws.logits, c->cpad, a.M, c->num_classes, ws.col_margin, ws.col_abs,
                                                   c->stream));
        TRY(line_guard());
    }
    return HCTR_OK;
}

// second half of the fused beam front end for the active workspace (after run_forward(HEAD_BEAM)): thresholds, the
// head GEMM once more with the list-emitting epilogue, selection. Device outputs are indexed r = t*B + b.
int beam_finish(hctr_ctx* c, int k, bool want_candidates, double thresh, int32_t* d_idx, float* d_lp, float* d_bl,
                float* d_st, int32_t* d_cnt) {
    Workspace& ws = c->ws;
    Prof pf(c);
    ConvArgs a;
    ConvTile htile;
    head_args(c, &a, &htile);
    const int P = a.ntiles * kLinearWN;
    PROF_TRY(pf, "beam_thresholds", launch_beam_thresholds(ws.amax_val, ws.psum, P, a.M, k, thresh,
                                                           want_candidates ? 1 : 0, ws.row_thr, ws.emit_cnt,
                                                           c->stream));
    a.y = nullptr;
    a.row_thr = ws.row_thr; a.emit_cnt = ws.emit_cnt; a.emit_list = ws.emit_list; a.emit_cap = kBeamCap;
    a.esum = ws.esum;
    PROF_TRY(pf, "head.linear+lists", launch_conv(a, htile, 1, true, c->stream));
    HIP_TRY(c, hipMemsetAsync(ws.overflow, 0, 4, c->stream));
    PROF_TRY(pf, "beam_select", launch_beam_select(ws.row_thr, ws.emit_cnt, ws.emit_list, kBeamCap, ws.esum, P,
                                                   ws.blank_logit, ws.B, ws.W, k, thresh, d_idx, d_lp, d_bl, d_st,
                                                   d_cnt, ws.overflow, c->stream));
    return HCTR_OK;
}

struct Batch {              // the caller's line images: [B][128][W] u8 or f32, on the host or the device; widths[B] or null
    const void* img;
    int dtype, on_device;
    const int32_t* widths;
    int B, W;
};

// f(first_index, run_length) for every run of consecutive line numbers in lines[0..nb), until one fails
template <class F>
int for_runs(const int* lines, int nb, F f) {
    for (int i = 0; i < nb;) {
        int j = i + 1;
        while (j < nb && lines[j] == lines[j - 1] + 1) ++j;
        TRY(f(i, j - i));
        i = j;
    }
    return HCTR_OK;
}

// Copy the lines `lines[0..nb)` of the caller's batch (and their widths) into the workspace. Runs of consecutive
// lines become one copy each, so an ordinary pass (a contiguous range) is a single copy.
int stage_input(hctr_ctx* c, const Batch& in, const int* lines, int nb) {
    Workspace& ws = c->ws;
    const size_t per = (size_t)kImgH * in.W * (in.dtype == HCTR_F32 ? 4 : 1);
    const hipMemcpyKind kind = in.on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    TRY(for_runs(lines, nb, [&](int i, int n) -> int {
        HIP_TRY(c, hipMemcpyAsync((char*)ws.img + (size_t)i * per, (const char*)in.img + (size_t)lines[i] * per,
                                  per * (size_t)n, kind, c->stream));
        return HCTR_OK;
    }));
    if (in.widths) {
        c->h_widths.emplace_back((size_t)nb);
        std::vector<int32_t>& hw = c->h_widths.back();
        for (int i = 0; i < nb; ++i) {
            const int32_t w = in.widths[lines[i]];
            if (w < 1 || w > in.W) return fail(c, HCTR_ERR_ARG, "widths[%d]=%d outside [1,%d]", lines[i], w, in.W);
            hw[(size_t)i] = w;
        }
        HIP_TRY(c, hipMemcpyAsync(ws.widths, hw.data(), (size_t)nb * 4, hipMemcpyHostToDevice, c->stream));
    }
    return HCTR_OK;
}

int check_forward_args(hctr_ctx* c, const void* img, int img_dtype, int B, int W) {
    if (!c) return HCTR_ERR_ARG;
    if (!c->finalized) return fail(c, HCTR_ERR_STATE, "weights not finalized: call hctr_finalize_weights first");
    if (!img) return fail(c, HCTR_ERR_ARG, "img is NULL");
    if (img_dtype != HCTR_U8 && img_dtype != HCTR_F32) return fail(c, HCTR_ERR_ARG, "img_dtype must be U8 or F32");
    if (B < 0 || W < 1) return fail(c, HCTR_ERR_ARG, "bad batch shape B=%d W=%d", B, W);
    return HCTR_OK;
}

// lines per internal pass: at most max_cols pixel columns, balanced so every pass of a batch has the
// same shape (one cached workspace per (B, W) instead of a second one for a short tail)
int sub_batch(hctr_ctx* c, int B, int W, bool split) {
    int64_t nb = (c->max_cols / (split ? 3 : 1)) / W;
    if (nb < 1) nb = 1;
    if (nb >= B) return B;
    const int64_t passes = (B + nb - 1) / nb;
    return (int)((B + passes - 1) / passes);
}

// mode 2: which lines of the finished f16 sweep must run again in f16x3. gbuf = [B][2] {min margin, max |logit|}.
// A line is certain when EVERY column's top-1/top-2 margin exceeds twice the guard's tolerance
// tol = guard_rel * (max |logit| of the line) + guard_abs: a flip needs err(top1) + err(other) > margin, so the
// certificate is sound where each f16 logit of the line is within tol of the fp32-grade one. That premise is the
// guard's own - per line, so a line's flag does not depend on its batch - and tighter than the parity suite's f16
// bound over the batch-wide scale; tests/test_gpu_guard.py asserts it line by line against f16x3, and the defaults
// come from that measurement ("Guard defaults"). NaN / inf figures flag.
std::vector<int> guard_decide(hctr_ctx* c, const std::vector<float>& gbuf, int B) {
    c->g_margin.resize((size_t)B); c->g_scale.resize((size_t)B); c->g_flag.assign((size_t)B, 0);
    std::vector<int> flagged;
    for (int b = 0; b < B; ++b) {
        const float mg = gbuf[2 * (size_t)b], sc = gbuf[2 * (size_t)b + 1];
        c->g_margin[(size_t)b] = mg;
        c->g_scale[(size_t)b] = sc;
        const double thr = 2.0 * (c->guard_rel * (double)sc + c->guard_abs);
        if (!((double)mg > thr)) {
            c->g_flag[(size_t)b] = 1;
            flagged.push_back(b);
        }
    }
    c->g_lines_total += B;
    c->g_flagged_total += (int64_t)flagged.size();
    return flagged;
}

void guard_clear(hctr_ctx* c) {
    c->g_margin.clear(); c->g_scale.clear(); c->g_flag.clear();
}

// the arithmetic of a call's passes returns to the mode's own on every exit path
struct SplitScope {
    hctr_ctx* c;
    explicit SplitScope(hctr_ctx* ctx) : c(ctx) { c->split = c->mode == 1; }
    ~SplitScope() { c->split = c->mode == 1; }
};

std::vector<int> line_indices(int B) {
    std::vector<int> all((size_t)B);
    for (int b = 0; b < B; ++b) all[(size_t)b] = b;
    return all;
}

// ---------------------------------------------------------------------------------------------
// the passes of a call on line images ("The pass skeleton")
// ---------------------------------------------------------------------------------------------
struct Pass {                // one internal pass: the lines lines[0..nb) of the caller's batch
    const int* lines;
    int nb;
    int first, total;        // the pass holds lines [first, first + nb) of its sweep's `total`
    bool rerun;              // second sweep of a guarded call: the flagged lines, in f16x3
    float* guard_dst;        // first sweep of a guarded call: where the lines' [nb][2] guard figures go on the host
};

// Stage the pass's lines and run trunk + head in head mode `hm`; a guard pass also queues its figures' copy back.
int forward_pass(hctr_ctx* c, const Batch& in, const Pass& p, HeadMode hm) {
    const bool guard_pass = p.guard_dst != nullptr;
    TRY(ensure_workspace(c, p.nb, in.W, ws_need(c, hm, guard_pass)));
    TRY(stage_input(c, in, p.lines, p.nb));
    TRY(run_forward(c, in.dtype == HCTR_F32, in.widths != nullptr, hm, guard_pass));
    if (guard_pass)
        HIP_TRY(c, hipMemcpyAsync(p.guard_dst, c->ws.line_guard, (size_t)p.nb * 8, hipMemcpyDeviceToHost, c->stream));
    return HCTR_OK;
}

// which arithmetic a call's lines run in. OWN: the mode's, and in mode 2 guarded - every line in f16, then the lines
// guard_decide flags once more in f16x3 (argmaxes and what derives from them). EXACT: figures (losses, alignments,
// confidences) that mode 2's guard does not certify - f16x3 unless the mode is 0, in one sweep.
enum PassPolicy { PASS_OWN, PASS_EXACT };

// Cut the batch into balanced passes of sub_batch() lines and hand each to pass(const Pass&), which runs forward_pass
// and queues what follows it. The first failure ends the call. Work may still be queued on return, failure included:
// the entry ends with synced(). The one exception, which entries may rely on: a guarded call that flags nothing
// returns drained (the guard figures had to come back).
template <class PassFn>
int run_passes(hctr_ctx* c, const Batch& in, PassPolicy policy, PassFn pass) {
    SplitScope scope(c);
    if (policy == PASS_EXACT) {
        c->split = c->mode != 0;
        if (!c->wts().built) return fail(c, HCTR_ERR_STATE, "the weight set of this precision mode is not resident");
    } else {
        guard_clear(c);
    }
    prof_reset(c);
    auto sweep = [&](const std::vector<int>& lines, bool rerun, float* gbuf) -> int {
        const int n = (int)lines.size(), nbmax = sub_batch(c, n, in.W, c->split);
        for (int o = 0; o < n; o += nbmax)
            TRY(pass(Pass{lines.data() + o, std::min(nbmax, n - o), o, n, rerun, gbuf ? gbuf + 2 * (size_t)o : nullptr}));
        return HCTR_OK;
    };
    if (policy == PASS_EXACT || c->mode != 2) return sweep(line_indices(in.B), false, nullptr);
    // guarded precision: the lines the f16 sweep cannot certify run again in f16x3 at the SAME padded width (a line's
    // result depends on nothing but its own pixels and W) and replace their rows of every output
    std::vector<float> gbuf((size_t)2 * in.B);
    TRY(synced(c, sweep(line_indices(in.B), false, gbuf.data())));
    const std::vector<int> flagged = guard_decide(c, gbuf, in.B);
    if (flagged.empty()) return HCTR_OK;
    c->split = true;
    return sweep(flagged, true, nullptr);
}

// ---------------------------------------------------------------------------------------------
// the logits of a scoring call ("The pass skeleton"): their source, the rows of one pass, the driver
// ---------------------------------------------------------------------------------------------
struct Source {              // line images that go through the forward (img.img != null), or the caller's [W][B][C] logits
    Batch img;
    const float* wbc;        // on the host or the device
    int on_device;
    int B, W, C;
    bool images() const { return img.img != nullptr; }
};

Source image_source(const hctr_ctx* c, const void* img, int dtype, int on_device, const int32_t* widths, int B, int W) {
    return Source{Batch{img, dtype, on_device, widths, B, W}, nullptr, 0, B, W, c->num_classes};
}

Source logits_source(const float* wbc, int on_device, int W, int B, int C) { return Source{Batch{}, wbc, on_device, B, W, C}; }

struct Rows {                // the logit rows of one pass: line b of the pass, column t lies at x + (b*sb + t*st) * ld
    const float* x;
    int64_t ld, sb, st;
    int C;
    Rows from_line(int l0) const { return Rows{x + (int64_t)l0 * sb * ld, ld, sb, st, C}; }
};

// The logit rows of pass p on the device: the forward of the pass's images into the workspace's stored logits, or the
// caller's tensor, whose rows are r = t*B + b (a host tensor is uploaded into `pool`, the driver's).
int pass_rows(hctr_ctx* c, const Source& src, const Pass& p, std::vector<void*>& pool, Rows* r) {
    if (src.images()) {
        TRY(forward_pass(c, src.img, p, HEAD_LOGITS));
        *r = Rows{c->ws.logits, c->cpad, src.W, 1, c->num_classes};
        return HCTR_OK;
    }
    const float* dev = nullptr;
    TRY(logits_on_device(c, pool, src.wbc, src.on_device, (size_t)src.W * src.B * src.C, &dev));
    *r = Rows{dev, src.C, 1, src.B, src.C};
    return HCTR_OK;
}

// the emissions of the lines [b0, b0 + nb), the pass's lines 0 .. nb of r, under the tables m
int lse_rows(Prof& pf, const Rows& r, const CtcLines& m, int b0, int nb, int W, float* emis) {
    PROF_TRY(pf, "ctc_lse", launch_ctc_lse(r.x, r.ld, r.sb, r.st, r.C, m, b0, nb, W, emis, nullptr, pf.c->stream));
    return HCTR_OK;
}

// The passes of a scoring call over its source, and its end. Images: PASS_EXACT passes (mode 2's guard certifies
// argmaxes, not probabilities). Caller logits: one pass of all lines. pass(p, pool) queues one pass: the family's scratch
// when p.first == 0 (no later pass is larger, so it is sized by p.nb), pass_rows, the launches on the rows. finish()
// queues what follows the last pass: rankings, the copies back. `pool` holds the call's device temporaries and outlives
// the wait the driver ends in; a failure ends the call at once, drained all the same. Pageable host tables that pass
// or finish queue were staged before hipMemcpyAsync returned.
template <class PassFn, class FinishFn>
int source_passes(hctr_ctx* c, const Source& src, PassFn pass, FinishFn finish) {
    std::vector<void*> pool;
    PoolGuard pool_guard{pool};
    return synced(c, [&]() -> int {
        if (src.images()) {
            TRY(run_passes(c, src.img, PASS_EXACT, [&](const Pass& p) -> int { return pass(p, pool); }));
        } else {
            prof_reset(c);
            const std::vector<int> all = line_indices(src.B);
            TRY(pass(Pass{all.data(), src.B, 0, src.B, false, nullptr}, pool));
        }
        return finish();
    }());
}

template <class PassFn>
int source_passes(hctr_ctx* c, const Source& src, PassFn pass) {
    return source_passes(c, src, pass, [] { return HCTR_OK; });
}

// ---------------------------------------------------------------------------------------------
// CTC loss (hctr_ctc_loss*): argument checks, the per-line tables of kernels.h CtcLines, scratch
// ---------------------------------------------------------------------------------------------
struct CtcHost {
    std::vector<int32_t> tab;     // T[B] | L[B] | off[B] | nd[B] | cls[B][D] | slot[sum L], uploaded as one block
    int B = 0, D = 1, max_states = 1;
    // the tables over a copy of tab at d: the host's own, or the device's
    CtcLines lines(const int32_t* d) const {
        const size_t b = (size_t)B;
        return CtcLines{d, d + b, d + 2 * b, d + 3 * b, d + 4 * b, d + 4 * b + b * D, D};
    }
    CtcLines host() const { return lines(tab.data()); }
    size_t total() const { return tab.size() - 4 * (size_t)B - (size_t)B * D; }      // sum L
};

// shape and pointer checks of the hctr_ctc_*_logits entries; B = 0 passes (the caller returns at once)
int check_logits_args(hctr_ctx* c, int W, int B, int C, bool have_pointers) {
    if (!c) return HCTR_ERR_ARG;
    if (W < 0 || B < 0 || C < 2 || (B > 0 && W < 1)) return fail(c, HCTR_ERR_ARG, "bad logits shape W=%d B=%d C=%d", W, B, C);
    if (B > 0 && !have_pointers) return fail(c, HCTR_ERR_ARG, "NULL pointer");
    return HCTR_OK;
}

// input_lengths (null: W for every line) held to [min_len, W], and the head of a family's upload made of them:
// T[B] | zero[B]
int lengths_head(hctr_ctx* c, int B, int W, const int32_t* input_lengths, int min_len, std::vector<int32_t>* up) {
    for (int b = 0; b < B && input_lengths; ++b)
        if (input_lengths[b] < min_len || input_lengths[b] > W)
            return fail(c, HCTR_ERR_ARG, "input_lengths[%d]=%d outside [%d,%d]", b, input_lengths[b], min_len, W);
    up->assign((size_t)2 * B, 0);
    for (int b = 0; b < B; ++b) (*up)[(size_t)b] = input_lengths ? input_lengths[b] : W;
    return HCTR_OK;
}

// torch.nn.functional.ctc_loss's conventions with blank 0: a target id outside [1, C-1] is an argument error; a line
// with L + (adjacent equal labels) > T has no alignment and gets T = 0 (the kernel writes +inf without reading a row)
int ctc_prepare(hctr_ctx* c, int B, int W, int C, const int32_t* targets, const int32_t* target_lengths,
                const int32_t* input_lengths, CtcHost* h) {
    if (!target_lengths) return fail(c, HCTR_ERR_ARG, "target_lengths is NULL");
    int64_t total = 0;
    for (int b = 0; b < B; ++b) {
        if (target_lengths[b] < 0) return fail(c, HCTR_ERR_ARG, "target_lengths[%d]=%d < 0", b, target_lengths[b]);
        total += target_lengths[b];
    }
    if (total > 0 && !targets) return fail(c, HCTR_ERR_ARG, "targets is NULL");
    if (total > INT32_MAX) return fail(c, HCTR_ERR_ARG, "too many targets (%lld)", (long long)total);
    std::vector<std::vector<int32_t>> dist((size_t)B);
    std::vector<int32_t> T((size_t)B), nd((size_t)B);
    int D = 1, max_states = 1;
    int64_t o = 0;
    for (int b = 0; b < B; ++b) {
        const int L = target_lengths[b];
        const int32_t* tg = targets + o;
        const int Tb = input_lengths ? input_lengths[b] : W;
        if (Tb < 1 || Tb > W) return fail(c, HCTR_ERR_ARG, "input_lengths[%d]=%d outside [1,%d]", b, Tb, W);
        int rep = 0;
        for (int j = 0; j < L; ++j) {
            if (tg[j] < 1 || tg[j] > C - 1)
                return fail(c, HCTR_ERR_ARG, "target id %d (line %d, position %d) outside [1,%d]", tg[j], b, j, C - 1);
            rep += (j > 0 && tg[j] == tg[j - 1]) ? 1 : 0;
        }
        const bool feasible = (int64_t)L + rep <= Tb;
        if (feasible && 2 * (int64_t)L + 1 > kCtcMaxStates)
            return fail(c, HCTR_ERR_ARG, "target_lengths[%d]=%d exceeds the %d labels one line supports", b, L,
                        (kCtcMaxStates - 1) / 2);
        std::vector<int32_t>& d = dist[(size_t)b];
        d.assign(tg, tg + L);
        std::sort(d.begin(), d.end());
        d.erase(std::unique(d.begin(), d.end()), d.end());
        T[(size_t)b] = feasible ? Tb : 0;
        nd[(size_t)b] = 1 + (int)d.size();
        if (feasible) {
            D = std::max(D, nd[(size_t)b]);
            max_states = std::max(max_states, 2 * L + 1);
        }
        o += L;
    }
    h->B = B; h->D = D; h->max_states = max_states;
    std::vector<int32_t>& tab = h->tab;
    tab.assign((size_t)4 * B + (size_t)B * D + (size_t)total, 0);
    int32_t* cls = tab.data() + 4 * (size_t)B;
    int32_t* slot = cls + (size_t)B * D;
    o = 0;
    for (int b = 0; b < B; ++b) {
        const int L = target_lengths[b];
        const std::vector<int32_t>& d = dist[(size_t)b];
        tab[(size_t)b] = T[(size_t)b];
        tab[(size_t)B + b] = L;
        tab[2 * (size_t)B + b] = (int32_t)o;
        tab[3 * (size_t)B + b] = T[(size_t)b] ? nd[(size_t)b] : 1;
        for (size_t j = 0; j < d.size() && T[(size_t)b]; ++j) cls[(size_t)b * D + 1 + j] = d[j];
        for (int j = 0; j < L; ++j)
            slot[o + j] = 1 + (int32_t)(std::lower_bound(d.begin(), d.end(), targets[o + j]) - d.begin());
        o += L;
    }
    return HCTR_OK;
}

// the context's grow-only CTC scratch with room for `need` bytes. When it has to grow, its first `keep` bytes move to
// the new block (recognition's kept log-sum-exps); with keep = 0 the old block is freed before the new one is asked for.
int ctc_reserve(hctr_ctx* c, size_t need, size_t keep = 0) {
    if (need <= c->ctc_cap) return HCTR_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!keep) {
        if (c->ctc_buf) (void)hipFree(c->ctc_buf);
        c->ctc_buf = nullptr; c->ctc_cap = 0;
    }
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, need);
    if (e != hipSuccess)
        return fail(c, HCTR_ERR_NOMEM, "hipMalloc(%zu bytes) for the CTC scratch failed: %s", need, hipGetErrorString(e));
    if (keep) {
        auto move = [&]() -> int {
            HIP_TRY(c, hipMemcpyAsync(p, c->ctc_buf, keep, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            return HCTR_OK;
        };
        if (const int rc = move()) {
            (void)hipFree(p);
            return rc;
        }
        (void)hipFree(c->ctc_buf);
    }
    c->ctc_buf = (char*)p;
    c->ctc_cap = need;
    return HCTR_OK;
}

// device scratch of a CTC call: the tables (uploaded), nll[B], `emis_floats` emission floats and, for the gradient,
// `extra_b` more bytes at *extra (256-byte aligned)
int ctc_scratch(hctr_ctx* c, const CtcHost& h, size_t emis_floats, CtcLines* m, float** nll, float** emis,
                size_t extra_b = 0, char** extra = nullptr) {
    const size_t tab_b = align256(h.tab.size() * 4), nll_b = align256((size_t)h.B * 4);
    const size_t emis_b = extra_b ? align256(emis_floats * 4) : emis_floats * 4;
    const size_t need = tab_b + nll_b + emis_b + extra_b;
    TRY(ctc_reserve(c, need));
    *m = h.lines((const int32_t*)c->ctc_buf);
    *nll = (float*)(c->ctc_buf + tab_b);
    *emis = (float*)(c->ctc_buf + tab_b + nll_b);
    if (extra) *extra = c->ctc_buf + tab_b + nll_b + emis_b;
    HIP_TRY(c, hipMemcpyAsync(c->ctc_buf, h.tab.data(), h.tab.size() * 4, hipMemcpyHostToDevice, c->stream));
    return HCTR_OK;
}

// forced alignment (hctr_ctc_align*): the scratch beyond the loss's, carved from ctc_scratch's `extra` block
struct AlignDev {
    std::vector<int64_t> boff;    // [B] byte offset of each line's backpointer rows (host copy)
    size_t total = 0;             // sum L
    int64_t* d_boff = nullptr;
    int32_t *d_end = nullptr, *d_path = nullptr, *d_st = nullptr, *d_en = nullptr;
    float* d_lp = nullptr;
    uint8_t* d_bp = nullptr;
    size_t boff_b = 0, end_b = 0, path_b = 0, span_b = 0, bp_b = 0;
    size_t bytes() const { return boff_b + end_b + path_b + 3 * span_b + bp_b; }
};

void align_layout(const CtcHost& h, int W, AlignDev* a) {
    const int B = h.B, ns = ctc_viterbi_lane_states(h.max_states);      // >= 1: ctc_prepare holds max_states to the ladder
    const int32_t *hT = h.host().T, *hL = h.host().L;
    a->total = h.total();
    a->boff.assign((size_t)B, 0);
    int64_t bytes = 0;
    for (int b = 0; b < B; ++b) {
        a->boff[(size_t)b] = bytes;
        bytes += (int64_t)hT[b] * ((2 * (int64_t)hL[b] + ns) / ns);     // T * ceil((2L + 1) / ns); none without an alignment
    }
    a->boff_b = align256((size_t)B * 8); a->end_b = align256((size_t)B * 4); a->path_b = align256((size_t)B * W * 4);
    a->span_b = align256(a->total * 4); a->bp_b = align256((size_t)bytes);
}

void align_carve(char* extra, AlignDev* a) {
    a->d_boff = (int64_t*)extra;
    a->d_end = (int32_t*)(extra + a->boff_b);
    a->d_path = (int32_t*)(extra + a->boff_b + a->end_b);
    char* sp = extra + a->boff_b + a->end_b + a->path_b;
    a->d_st = (int32_t*)sp; a->d_en = (int32_t*)(sp + a->span_b); a->d_lp = (float*)(sp + 2 * a->span_b);
    a->d_bp = (uint8_t*)(sp + 3 * a->span_b);
}

// recursion and back-trace of the pass's lines [b0, b0 + nb) over their emissions
int align_launch(hctr_ctx* c, Prof& pf, const float* emis, const CtcLines& m, const CtcHost& h, const AlignDev& a, int b0,
                 int nb, int W, float* d_score) {
    PROF_TRY(pf, "ctc_viterbi", launch_ctc_viterbi(emis, m, b0, nb, W, h.max_states, a.d_boff, a.d_bp, d_score, a.d_end,
                                                   c->stream));
    PROF_TRY(pf, "ctc_backtrace", launch_ctc_backtrace(emis, m, b0, nb, W, h.max_states, a.d_boff, a.d_bp, a.d_end,
                                                       a.d_path, a.d_st, a.d_en, a.d_lp, c->stream));
    return HCTR_OK;
}

int align_fetch(hctr_ctx* c, const AlignDev& a, int B, int W, const float* d_score, int32_t* path, int32_t* span_start,
                int32_t* span_end, float* span_logp, float* score) {
    HIP_TRY(c, fetch(c, path, a.d_path, (size_t)B * W * 4));
    HIP_TRY(c, fetch(c, span_start, a.d_st, a.total * 4));      // (nothing to fetch when every target is empty)
    HIP_TRY(c, fetch(c, span_end, a.d_en, a.total * 4));
    HIP_TRY(c, fetch(c, span_logp, a.d_lp, a.total * 4));
    HIP_TRY(c, fetch(c, score, d_score, (size_t)B * 4));
    return HCTR_OK;
}

// hctr_ctc_loss*: `nll` is the caller's [B]
int ctc_loss_call(hctr_ctx* c, const Source& src, const int32_t* targets, const int32_t* target_lengths,
                  const int32_t* input_lengths, float* nll) {
    const int B = src.B, W = src.W;
    if (B == 0) return HCTR_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    CtcHost h;
    TRY(ctc_prepare(c, B, W, src.C, targets, target_lengths, input_lengths, &h));
    CtcLines m;
    float *d_nll = nullptr, *emis = nullptr;
    return source_passes(
        c, src,
        [&](const Pass& p, std::vector<void*>& pool) -> int {
            if (p.first == 0) TRY(ctc_scratch(c, h, (size_t)p.nb * W * h.D, &m, &d_nll, &emis));
            Rows r;
            TRY(pass_rows(c, src, p, pool, &r));
            Prof pf(c);
            TRY(lse_rows(pf, r, m, p.first, p.nb, W, emis));
            PROF_TRY(pf, "ctc_alpha", launch_ctc_alpha(emis, m, p.first, p.nb, W, h.max_states, d_nll, nullptr, nullptr,
                                                       c->stream));
            return HCTR_OK;
        },
        [&]() -> int {
            HIP_TRY(c, hipMemcpyAsync(nll, d_nll, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
            return HCTR_OK;
        });
}

// hctr_ctc_align*: the outputs are the caller's host arrays, any may be null
int ctc_align_call(hctr_ctx* c, const Source& src, const int32_t* targets, const int32_t* target_lengths,
                   const int32_t* input_lengths, int32_t* path, int32_t* span_start, int32_t* span_end, float* span_logp,
                   float* score) {
    const int B = src.B, W = src.W;
    if (B == 0) return HCTR_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    CtcHost h;
    TRY(ctc_prepare(c, B, W, src.C, targets, target_lengths, input_lengths, &h));
    AlignDev a;
    align_layout(h, W, &a);
    CtcLines m;
    float *d_score = nullptr, *emis = nullptr;
    return source_passes(
        c, src,
        [&](const Pass& p, std::vector<void*>& pool) -> int {
            if (p.first == 0) {
                char* extra = nullptr;
                TRY(ctc_scratch(c, h, (size_t)p.nb * W * h.D, &m, &d_score, &emis, a.bytes() + 16, &extra));
                align_carve(extra, &a);
                HIP_TRY(c, hipMemcpyAsync(a.d_boff, a.boff.data(), (size_t)B * 8, hipMemcpyHostToDevice, c->stream));
            }
            Rows r;
            TRY(pass_rows(c, src, p, pool, &r));
            Prof pf(c);
            TRY(lse_rows(pf, r, m, p.first, p.nb, W, emis));
            return align_launch(c, pf, emis, m, h, a, p.first, p.nb, W, d_score);
        },
        [&] { return align_fetch(c, a, B, W, d_score, path, span_start, span_end, span_logp, score); });
}

// ---------------------------------------------------------------------------------------------
// keyword spotting (hctr_spot*): the queries' automata, the chunks of queries that share one emission pass, scratch
// ---------------------------------------------------------------------------------------------
// The KMP automaton of one query lifted to CTC (include/hctr_hip.h): states Z = 0, N_j = j, B_j = L - 1 + j, A = 2L - 1;
// local slots 0 = blank, 1..nq = the distinct classes ascending, nq + 1 = rest, nq + 2 = the constant 1.
struct SpotAuto {
    int L = 0, nq = 0, maxdeg = 0;
    std::vector<int32_t> cls, qslot, delta;       // [nq], [L], [L][nq]: delta(j, cls[i]) for j = 0..L-1
    std::vector<int32_t> ptr, src, slot;          // in-edge CSR over the 2L states, a state's edges by (src, slot)
    std::vector<uint64_t> mask;                   // [2L] the local slots a state sends to Z
};

void spot_automaton(const int32_t* q, int L, SpotAuto* a) {
    a->L = L;
    a->cls.assign(q, q + L);
    std::sort(a->cls.begin(), a->cls.end());
    a->cls.erase(std::unique(a->cls.begin(), a->cls.end()), a->cls.end());
    const int nq = a->nq = (int)a->cls.size(), S = 2 * L, A = S - 1;
    a->qslot.resize((size_t)L);
    for (int j = 0; j < L; ++j)
        a->qslot[(size_t)j] = 1 + (int32_t)(std::lower_bound(a->cls.begin(), a->cls.end(), q[j]) - a->cls.begin());
    std::vector<int> border((size_t)L + 1, 0);    // border[k] = the longest proper border of q_1..q_k
    for (int k = 2; k <= L; ++k) {
        int m = border[(size_t)k - 1];
        while (m > 0 && q[m] != q[k - 1]) m = border[(size_t)m];
        border[(size_t)k] = q[m] == q[k - 1] ? m + 1 : 0;
    }
    a->delta.assign((size_t)L * nq, 0);
    for (int j = 0; j < L; ++j)
        for (int i = 0; i < nq; ++i) {
            int m = j;
            while (m > 0 && q[m] != a->cls[(size_t)i]) m = border[(size_t)m];
            a->delta[(size_t)j * nq + i] = q[m] == a->cls[(size_t)i] ? m + 1 : 0;
        }
    std::vector<std::vector<std::pair<int, int>>> in((size_t)S);
    a->mask.assign((size_t)S, 0);
    const uint64_t rest = (uint64_t)1 << (nq + 1);
    auto tgt = [&](int k) { return k == 0 ? 0 : k == L ? A : k; };
    // out of a state with j characters matched on class slot i: to tgt(delta), or back to Z
    auto on_class = [&](int s, int j, int i) {
        const int d = a->delta[(size_t)j * nq + (i - 1)];
        if (d) in[(size_t)tgt(d)].push_back({s, i});
        else a->mask[(size_t)s] |= (uint64_t)1 << i;
    };
    a->mask[0] = rest | 1;                        // Z: the blank, rest and every class but q_1 stay
    for (int i = 1; i <= nq; ++i) on_class(0, 0, i);
    for (int j = 1; j < L; ++j) {                 // N_j: q_j repeats the character, the blank moves to B_j
        const int own = a->qslot[(size_t)j - 1];
        in[(size_t)j].push_back({j, own});
        in[(size_t)L - 1 + j].push_back({j, 0});
        a->mask[(size_t)j] = rest;
        for (int i = 1; i <= nq; ++i)
            if (i != own) on_class(j, j, i);
    }
    for (int j = 1; j < L; ++j) {                 // B_j: after a blank q_j is a new character too
        const int s = L - 1 + j;
        in[(size_t)s].push_back({s, 0});
        a->mask[(size_t)s] = rest;
        for (int i = 1; i <= nq; ++i) on_class(s, j, i);
    }
    in[(size_t)A].push_back({A, nq + 2});
    a->ptr.assign((size_t)S + 1, 0);
    a->src.clear(); a->slot.clear();
    a->maxdeg = 0;
    for (int s = 0; s < S; ++s) {
        std::sort(in[(size_t)s].begin(), in[(size_t)s].end());
        for (const auto& e : in[(size_t)s]) {
            a->src.push_back(e.first);
            a->slot.push_back(e.second);
        }
        a->ptr[(size_t)s + 1] = (int32_t)a->src.size();
        a->maxdeg = std::max(a->maxdeg, (int)in[(size_t)s].size());
    }
}

// classes (blank included) one chunk of queries may hold: HCTR_SPOT_CLASSES, else what keeps the emissions of `lines`
// lines of W columns within 256 MB, held to [64, 1024]. A single query that exceeds it gets a chunk of its own.
int spot_class_cap(int lines, int W) {
    if (const char* e = getenv("HCTR_SPOT_CLASSES")) {
        const int v = atoi(e);
        if (v >= 2) return v;
    }
    const int64_t rows = std::max<int64_t>(1, (int64_t)std::max(lines, 1) * std::max(W, 1));
    return (int)std::min<int64_t>(1024, std::max<int64_t>(64, ((int64_t)256 << 20) / (4 * rows)));
}

struct SpotChunk {
    int q0, n, D;                                 // queries [q0, q0 + n), D emission slots (blank first)
    size_t pair_off, gslot_off, nd_off, cls_off;  // words into SpotHost::up
};

struct SpotHost {
    int B = 0, Q = 0, Dmax = 1;
    std::vector<SpotAuto> autos;
    std::vector<SpotChunk> chunks;
    // the call's one upload: T[B] | zero[B] | qoff[Q] | blob | per chunk pair_q[n] | gslot[n][kSpotSlots] | nd[B] | cls[B][D]
    std::vector<int32_t> up;
    size_t qoff_off = 0, blob_off = 0;
    // the tables that make launch_ctc_lse write a chunk's classes for every line, over a copy of `up` at d
    CtcLines lines(const int32_t* d, const SpotChunk& ch) const {
        return CtcLines{d, d + B, d + B, d + ch.nd_off, d + ch.cls_off, d + B, ch.D};
    }
};

int spot_prepare(hctr_ctx* c, int B, int W, int C, const int32_t* queries, const int32_t* query_lengths, int Q,
                 const int32_t* input_lengths, int lines_per_launch, SpotHost* h) {
    if (Q < 1) return fail(c, HCTR_ERR_ARG, "need Q >= 1 queries, got Q=%d", Q);
    if (!queries || !query_lengths) return fail(c, HCTR_ERR_ARG, "queries/query_lengths is NULL");
    if ((int64_t)std::max(B, 1) * Q > INT32_MAX) return fail(c, HCTR_ERR_ARG, "B*Q=%lld too large", (long long)B * Q);
    int64_t o = 0;
    for (int k = 0; k < Q; ++k) {
        const int L = query_lengths[k];
        if (L < 1 || L > kSpotMaxLen) return fail(c, HCTR_ERR_ARG, "query_lengths[%d]=%d outside [1,%d]", k, L, kSpotMaxLen);
        for (int j = 0; j < L; ++j)
            if (queries[o + j] < 1 || queries[o + j] > C - 1)
                return fail(c, HCTR_ERR_ARG, "query id %d (query %d, position %d) outside [1,%d]", queries[o + j], k, j, C - 1);
        o += L;
    }
    std::vector<int32_t>& up = h->up;
    TRY(lengths_head(c, B, W, input_lengths, 0, &up));
    h->B = B; h->Q = Q;
    h->autos.resize((size_t)Q);
    h->qoff_off = up.size();
    up.resize(up.size() + (size_t)Q);
    h->blob_off = up.size();
    o = 0;
    for (int k = 0; k < Q; ++k) {
        SpotAuto& a = h->autos[(size_t)k];
        spot_automaton(queries + o, query_lengths[k], &a);
        o += a.L;
        up[h->qoff_off + k] = (int32_t)(up.size() - h->blob_off);
        const int32_t head[4] = {a.L, a.nq, a.maxdeg, (int32_t)a.src.size()};
        up.insert(up.end(), head, head + 4);
        up.insert(up.end(), a.qslot.begin(), a.qslot.end());
        up.insert(up.end(), a.ptr.begin(), a.ptr.end());
        for (uint64_t m : a.mask) up.push_back((int32_t)(uint32_t)m);
        for (uint64_t m : a.mask) up.push_back((int32_t)(uint32_t)(m >> 32));
        for (size_t e = 0; e < a.src.size(); ++e) up.push_back(a.src[e] | (a.slot[e] << 8));
    }
    // chunks of consecutive queries whose classes, with the blank, stay within the cap
    const int cap = spot_class_cap(lines_per_launch, W);
    h->Dmax = 1;
    for (int q0 = 0; q0 < Q;) {
        std::vector<int32_t> uni;
        int n = 0;
        while (q0 + n < Q) {
            const SpotAuto& a = h->autos[(size_t)q0 + n];
            std::vector<int32_t> merged;
            std::set_union(uni.begin(), uni.end(), a.cls.begin(), a.cls.end(), std::back_inserter(merged));
            if (n > 0 && (int)merged.size() + 1 > cap) break;
            uni.swap(merged);
            ++n;
        }
        SpotChunk ch;
        ch.q0 = q0; ch.n = n; ch.D = 1 + (int)uni.size();
        ch.pair_off = up.size();
        for (int i = 0; i < n; ++i) up.push_back(q0 + i);
        ch.gslot_off = up.size();
        for (int i = 0; i < n; ++i) {
            const SpotAuto& a = h->autos[(size_t)q0 + i];
            int32_t row[kSpotSlots] = {0};
            for (int j = 0; j < a.nq; ++j)
                row[1 + j] = 1 + (int32_t)(std::lower_bound(uni.begin(), uni.end(), a.cls[(size_t)j]) - uni.begin());
            up.insert(up.end(), row, row + kSpotSlots);
        }
        ch.nd_off = up.size();
        up.insert(up.end(), (size_t)B, ch.D);
        ch.cls_off = up.size();
        for (int b = 0; b < B; ++b) {
            up.push_back(0);
            up.insert(up.end(), uni.begin(), uni.end());
        }
        h->chunks.push_back(ch);
        h->Dmax = std::max(h->Dmax, ch.D);
        q0 += n;
    }
    return HCTR_OK;
}

struct SpotOut {             // the caller's host outputs, [B][Q]; any may be null
    float *contain, *seg;
    int32_t *seg_start, *seg_end;
};

struct SpotDev {
    const int32_t* up = nullptr;
    float *contain = nullptr, *seg = nullptr, *emis = nullptr;
    int32_t *seg_start = nullptr, *seg_end = nullptr;
};

// scratch of a spot call that launches n lines at a time: the upload, the four [B][Q] results, n*W*Dmax emissions
int spot_scratch(hctr_ctx* c, const SpotHost& h, int n, int W, SpotDev* d) {
    const size_t up_b = align256(h.up.size() * 4), out_b = align256((size_t)h.B * h.Q * 4);
    TRY(ctc_reserve(c, up_b + 4 * out_b + (size_t)n * W * h.Dmax * 4));
    char* p = c->ctc_buf;
    d->up = (const int32_t*)p;
    d->contain = (float*)(p + up_b);
    d->seg = (float*)(p + up_b + out_b);
    d->seg_start = (int32_t*)(p + up_b + 2 * out_b);
    d->seg_end = (int32_t*)(p + up_b + 3 * out_b);
    d->emis = (float*)(p + up_b + 4 * out_b);
    HIP_TRY(c, hipMemcpyAsync(p, h.up.data(), h.up.size() * 4, hipMemcpyHostToDevice, c->stream));
    return HCTR_OK;
}

// the lines [b0, b0 + nb), whose logit rows are r: per chunk the emissions, then the recursions
int spot_launch(hctr_ctx* c, const SpotHost& h, const SpotDev& d, const Rows& r, int b0, int nb, int W) {
    Prof pf(c);
    for (const SpotChunk& ch : h.chunks) {
        TRY(lse_rows(pf, r, h.lines(d.up, ch), b0, nb, W, d.emis));
        const SpotArgs a{d.emis, d.up, b0, nb, W, ch.D, d.up + h.blob_off, d.up + h.qoff_off, d.up + ch.pair_off,
                         d.up + ch.gslot_off, ch.n, h.Q, d.contain, d.seg, d.seg_start, d.seg_end};
        PROF_TRY(pf, "spot", launch_spot(a, c->stream));
    }
    return HCTR_OK;
}

int spot_fetch(hctr_ctx* c, const SpotHost& h, const SpotDev& d, const SpotOut& o) {
    const size_t bytes = (size_t)h.B * h.Q * 4;
    HIP_TRY(c, fetch(c, o.contain, d.contain, bytes));
    HIP_TRY(c, fetch(c, o.seg, d.seg, bytes));
    HIP_TRY(c, fetch(c, o.seg_start, d.seg_start, bytes));
    HIP_TRY(c, fetch(c, o.seg_end, d.seg_end, bytes));
    return HCTR_OK;
}

// hctr_spot*
int spot_call(hctr_ctx* c, const Source& src, const int32_t* queries, const int32_t* query_lengths, int Q,
              const int32_t* input_lengths, const SpotOut& o) {
    const int B = src.B, W = src.W;
    SpotHost h;
    TRY(spot_prepare(c, B, W, src.C, queries, query_lengths, Q, input_lengths, B, &h));
    if (B == 0) return HCTR_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    SpotDev d;
    return source_passes(
        c, src,
        [&](const Pass& p, std::vector<void*>& pool) -> int {
            if (p.first == 0) TRY(spot_scratch(c, h, p.nb, W, &d));
            Rows r;
            TRY(pass_rows(c, src, p, pool, &r));
            return spot_launch(c, h, d, r, p.first, p.nb, W);
        },
        [&] { return spot_fetch(c, h, d, o); });
}

// ---------------------------------------------------------------------------------------------
// lexicon recognition (hctr_lexicon*): the device copy of the lexicon, the chunks of units that share one emission
// pass, scratch
// ---------------------------------------------------------------------------------------------
// classes (blank included) one chunk of units may hold: HCTR_LEX_CLASSES, else what keeps the emissions of `lines`
// lines of W columns within 4 GiB, at least 64. A single unit that exceeds it gets a chunk of its own. The spot
// function's 256 MB (what the last-level cache holds) is the wrong budget here, by measurement: every
// chunk costs one read of all logits and launches its units alone, and a class-rich lexicon's units hold thousands of
// classes each, so the flagship shape ran one chunk per unit: 324 ms at 100 000 entries against 56 ms in one chunk.
// 4 GiB holds every class of the flagship shape (64 x 2000 x 7358): the emissions then never exceed the logits' size.
int lex_class_cap(int lines, int W) {
    if (const char* e = getenv("HCTR_LEX_CLASSES")) {
        const int v = atoi(e);
        if (v >= 2) return v;
    }
    const int64_t rows = std::max<int64_t>(1, (int64_t)std::max(lines, 1) * std::max(W, 1));
    return (int)std::min<int64_t>(1 << 20, std::max<int64_t>(64, ((int64_t)4 << 30) / (4 * rows)));
}

// the tables of a lexicon or a pattern as one device block of words: each table starts on a multiple of 64 words
struct WordTaker {
    size_t words = 0;
    size_t operator()(size_t n) { const size_t at = words; words += (n + 63) & ~(size_t)63; return at; }
};

// The context's device copy (*dev, of the object with *serial) of a caller's lexicon or pattern: `image`, the tables of
// the object with serial `want` packed on the host, replaces it. `what` names the object in the message.
int tables_on_device(hctr_ctx* c, uint64_t* serial, int32_t** dev, uint64_t want, const std::vector<int32_t>& image,
                     const char* what) {
    *serial = 0;
    if (*dev) (void)hipFree(*dev);
    *dev = nullptr;
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, image.size() * 4);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, HCTR_ERR_NOMEM, "no device memory for the %s tables (%zu bytes): %s", what, image.size() * 4,
                    hipGetErrorString(e));
    }
    *dev = (int32_t*)p;
    HIP_TRY(c, hipMemcpyAsync(p, image.data(), image.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the image is this call's, the object the caller's)
    *serial = want;
    return HCTR_OK;
}

// the words of the device block: uoff | coff | node | kidx | eptr | elist | prior (float bits)
struct LexLayout {
    size_t uoff, coff, node, kidx, eptr, elist, prior, words;
    explicit LexLayout(const hctr_lex& x) {
        WordTaker take;
        uoff = take(x.uoff.size()); coff = take(x.coff.size()); node = take(x.node.size()); kidx = take(x.kidx.size());
        eptr = take(x.eptr.size()); elist = take(x.elist.size()); prior = take(x.prior.size());
        words = take.words;
    }
};

// the context's device copy of the call's lexicon: uploaded when the context holds another one (or none)
int lex_on_device(hctr_ctx* c, const hctr_lex* x) {
    if (c->lex_serial == x->serial) return HCTR_OK;
    const LexLayout lay(*x);
    std::vector<int32_t> img(lay.words, 0);
    std::copy(x->uoff.begin(), x->uoff.end(), img.begin() + lay.uoff);
    std::copy(x->coff.begin(), x->coff.end(), img.begin() + lay.coff);
    std::copy(x->node.begin(), x->node.end(), img.begin() + lay.node);
    std::copy(x->kidx.begin(), x->kidx.end(), img.begin() + lay.kidx);
    std::copy(x->eptr.begin(), x->eptr.end(), img.begin() + lay.eptr);
    std::copy(x->elist.begin(), x->elist.end(), img.begin() + lay.elist);
    memcpy(img.data() + lay.prior, x->prior.data(), x->prior.size() * 4);
    return tables_on_device(c, &c->lex_serial, &c->lex_dev, x->serial, img, "lexicon");
}

struct LexChunk {
    int u0, nu, D;            // units [u0, u0 + nu), D emission slots (blank first)
    size_t cls_off;           // words into LexHost::up: the chunk's class list [D]
};

struct LexHost {
    const hctr_lex* lex = nullptr;
    int B = 0, n = 0, Dmax = 1;
    std::vector<LexChunk> chunks;
    std::vector<int32_t> up;  // the call's one upload: T[B] | zero[B] | umap[coff[units]] | per chunk cls[D]
    size_t umap_off = 0;
};

struct LexOut {               // the caller's host outputs; any may be null
    int32_t* top_entry;
    float* top_logp;
    double* top_rank;
    double* log_total;
    int32_t* count;
    float* scores;
};

int lex_prepare(hctr_ctx* c, const hctr_lex* lex, int B, int W, int C, const int32_t* input_lengths, int n,
                int lines_per_launch, LexHost* h) {
    if (!lex) return fail(c, HCTR_ERR_ARG, "lex is NULL");
    if (lex->C != C) return fail(c, HCTR_ERR_ARG, "the lexicon was built for %d classes, the call has %d", lex->C, C);
    if (n < 1 || n > kLexMaxTop) return fail(c, HCTR_ERR_ARG, "n=%d outside [1,%d]", n, kLexMaxTop);
    if ((int64_t)std::max(B, 1) * lex->N > INT32_MAX) return fail(c, HCTR_ERR_ARG, "B*N=%lld too large", (long long)B * lex->N);
    std::vector<int32_t>& up = h->up;
    TRY(lengths_head(c, B, W, input_lengths, 1, &up));
    h->lex = lex; h->B = B; h->n = n;
    h->umap_off = up.size();
    up.resize(up.size() + lex->ucls.size(), 0);
    // chunks of consecutive units whose classes, with the blank, stay within the cap
    const int cap = lex_class_cap(lines_per_launch, W), U = lex->units();
    for (int u0 = 0; u0 < U;) {
        std::vector<int32_t> uni{0};
        int nu = 0;
        while (u0 + nu < U) {
            const int32_t *f = lex->ucls.data() + lex->coff[(size_t)u0 + nu], *l = lex->ucls.data() + lex->coff[(size_t)u0 + nu + 1];
            std::vector<int32_t> merged;
            std::set_union(uni.begin(), uni.end(), f, l, std::back_inserter(merged));
            if (nu > 0 && (int)merged.size() > cap) break;
            uni.swap(merged);
            ++nu;
        }
        for (int u = u0; u < u0 + nu; ++u)
            for (int32_t k = lex->coff[(size_t)u]; k < lex->coff[(size_t)u + 1]; ++k)
                up[h->umap_off + (size_t)k] =
                    (int32_t)(std::lower_bound(uni.begin(), uni.end(), lex->ucls[(size_t)k]) - uni.begin());
        LexChunk ch{u0, nu, (int)uni.size(), up.size()};
        up.insert(up.end(), uni.begin(), uni.end());
        h->chunks.push_back(ch);
        h->Dmax = std::max(h->Dmax, ch.D);
        u0 += nu;
    }
    return HCTR_OK;
}

struct LexDev {
    const int32_t* up = nullptr;
    float *score = nullptr, *top_logp = nullptr, *emis = nullptr;
    int32_t *top_entry = nullptr, *count = nullptr, *cls = nullptr, *nd = nullptr;
    double *top_rank = nullptr, *log_total = nullptr;
};

// scratch of a lexicon call that launches nl lines at a time: the upload, the [B][N] scores, the ranking's results, the
// per-line class tables of one chunk, nl*W*Dmax emissions
int lex_scratch(hctr_ctx* c, const LexHost& h, int nl, int W, LexDev* d) {
    const size_t B = (size_t)h.B, n = (size_t)h.n;
    const size_t up_b = align256(h.up.size() * 4), sc_b = align256(B * h.lex->N * 4), top8 = align256(B * n * 8),
                 top4 = align256(B * n * 4), b8 = align256(B * 8), b4 = align256(B * 4), cls_b = align256(B * h.Dmax * 4);
    TRY(ctc_reserve(c, up_b + sc_b + top8 + 2 * top4 + b8 + 2 * b4 + cls_b + (size_t)nl * W * h.Dmax * 4));
    char* p = c->ctc_buf;
    d->up = (const int32_t*)p; p += up_b;
    d->score = (float*)p; p += sc_b;
    d->top_rank = (double*)p; p += top8;
    d->top_entry = (int32_t*)p; p += top4;
    d->top_logp = (float*)p; p += top4;
    d->log_total = (double*)p; p += b8;
    d->count = (int32_t*)p; p += b4;
    d->nd = (int32_t*)p; p += b4;
    d->cls = (int32_t*)p; p += cls_b;
    d->emis = (float*)p;
    HIP_TRY(c, hipMemcpyAsync(c->ctc_buf, h.up.data(), h.up.size() * 4, hipMemcpyHostToDevice, c->stream));
    return HCTR_OK;
}

// the lines [b0, b0 + nb), whose logit rows are r: per chunk the emissions, then the trie
int lex_launch(hctr_ctx* c, const LexHost& h, const LexDev& d, const Rows& r, int b0, int nb, int W) {
    Prof pf(c);
    const hctr_lex& lx = *h.lex;
    const LexLayout lay(lx);
    const int32_t* t = c->lex_dev;
    for (const LexChunk& ch : h.chunks) {
        PROF_TRY(pf, "lexicon_classes", launch_lexicon_classes(d.up + ch.cls_off, ch.D, h.B, d.cls, d.nd, c->stream));
        const CtcLines m{d.up, d.up + h.B, d.up + h.B, d.nd, d.cls, d.up + h.B, ch.D};
        TRY(lse_rows(pf, r, m, b0, nb, W, d.emis));
        const LexArgs a{d.emis, d.up, b0, nb, W, ch.D, t + lay.uoff, t + lay.coff, t + lay.node, t + lay.kidx, t + lay.eptr,
                        t + lay.elist, d.up + h.umap_off, ch.u0, ch.nu, lx.max_unit, lx.N, d.score};
        PROF_TRY(pf, "lexicon_trie", launch_lexicon_trie(a, c->stream));
    }
    return HCTR_OK;
}

// the ranking of every line once all scores are there, and the results to the host
int lex_finish(hctr_ctx* c, const LexHost& h, const LexDev& d, const LexOut& o) {
    Prof pf(c);
    const hctr_lex& lx = *h.lex;
    const float* prior = lx.has_prior ? (const float*)(c->lex_dev + LexLayout(lx).prior) : nullptr;
    PROF_TRY(pf, "lexicon_rank", launch_lexicon_rank(d.score, prior, h.B, lx.N, h.n, d.top_entry, d.top_logp, d.top_rank,
                                                     d.log_total, d.count, c->stream));
    const size_t B = (size_t)h.B, n = (size_t)h.n;
    HIP_TRY(c, fetch(c, o.top_entry, d.top_entry, B * n * 4));
    HIP_TRY(c, fetch(c, o.top_logp, d.top_logp, B * n * 4));
    HIP_TRY(c, fetch(c, o.top_rank, d.top_rank, B * n * 8));
    HIP_TRY(c, fetch(c, o.log_total, d.log_total, B * 8));
    HIP_TRY(c, fetch(c, o.count, d.count, B * 4));
    HIP_TRY(c, fetch(c, o.scores, d.score, B * lx.N * 4));
    return HCTR_OK;
}

// hctr_lexicon*
int lex_call(hctr_ctx* c, const Source& src, const hctr_lex* lex, const int32_t* input_lengths, int n, const LexOut& o) {
    const int B = src.B, W = src.W;
    LexHost h;
    TRY(lex_prepare(c, lex, B, W, src.C, input_lengths, n, B, &h));
    if (B == 0) return HCTR_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    TRY(lex_on_device(c, lex));
    LexDev d;
    return source_passes(
        c, src,
        [&](const Pass& p, std::vector<void*>& pool) -> int {
            if (p.first == 0) TRY(lex_scratch(c, h, p.nb, W, &d));
            Rows r;
            TRY(pass_rows(c, src, p, pool, &r));
            return lex_launch(c, h, d, r, p.first, p.nb, W);
        },
        [&] { return lex_finish(c, h, d, o); });
}

// ---------------------------------------------------------------------------------------------
// the loss of a decoded text over the emissions it was decoded from (hctr_pattern*, hctr_words*)
// ---------------------------------------------------------------------------------------------
// what a call that decodes texts in groups of lines keeps for their loss: the object's classes (ascending; every class
// a decoded text uses is among them) with D = classes + 1 emission slots, the call's upload (T[B] first), the group's
// decoded labels [B][W] and lengths [B] on the device, a per-line flag [B] (a line whose flag is below `have` has no
// text), the group's tables and emissions, and nll [B]. fix [B]: 0 = the kernel's nll, 1 = NaN (the text exceeds the
// loss's labels), 2 = +inf (no text).
struct TextNll {
    const std::vector<int32_t>* classes;
    int D;
    const std::vector<int32_t>* up;
    const int32_t *labels, *lengths, *flag;
    int have;
    int32_t* tab;
    const float* emis;
    float* nll;
    std::vector<uint8_t>* fix;
};

// The loss of the decoded texts of the group's lines [gb0, gb0 + n), over the group's own emissions: the loss's tables
// point into the object's classes and ctc_alpha reads what ctc_lse wrote for the object - the loss's emissions, bit for
// bit. The labels must be on the host: drains the stream.
int text_nll_group(hctr_ctx* c, Prof& pf, const TextNll& x, int gb0, int n, int W) {
    std::vector<int32_t> lab((size_t)n * W), len((size_t)n), flag((size_t)n);
    HIP_TRY(c, hipMemcpyAsync(lab.data(), x.labels + (size_t)gb0 * W, lab.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(len.data(), x.lengths + gb0, len.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(flag.data(), x.flag + gb0, flag.size() * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const std::vector<int32_t>& cls = *x.classes;
    std::vector<int32_t> tab((size_t)3 * n);
    int max_states = 1;
    for (int b = 0; b < n; ++b) {
        const int L = std::min(std::max(len[(size_t)b], 0), W);
        const bool none = flag[(size_t)b] < x.have, fits = 2 * (int64_t)L + 1 <= kCtcMaxStates;
        (*x.fix)[(size_t)gb0 + b] = none ? 2 : fits ? 0 : 1;
        const bool run = !none && fits;
        tab[(size_t)b] = run ? (*x.up)[(size_t)gb0 + b] : 0;          // T = 0: the kernel reads nothing of the line
        tab[(size_t)n + b] = run ? L : 0;
        tab[(size_t)2 * n + b] = (int32_t)(tab.size() - 3 * (size_t)n);
        for (int j = 0; j < L && run; ++j) {
            const size_t k = (size_t)(std::lower_bound(cls.begin(), cls.end(), lab[(size_t)b * W + j]) - cls.begin());
            tab.push_back(1 + (int32_t)std::min(k, cls.size() - 1));
        }
        if (run) max_states = std::max(max_states, 2 * L + 1);
    }
    HIP_TRY(c, hipMemcpyAsync(x.tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream));
    const int32_t* t = x.tab;
    const CtcLines m{t, t + n, t + 2 * n, t, t, t + 3 * n, x.D};
    PROF_TRY(pf, "ctc_alpha", launch_ctc_alpha(x.emis, m, 0, n, W, max_states, x.nll + gb0, nullptr, nullptr, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));          // (tab is this function's)
    return HCTR_OK;
}

// text_nll on the host once it is fetched: the lines whose figure is not the kernel's
void text_nll_fix(const std::vector<uint8_t>& fix, float* text_nll) {
    for (size_t b = 0; b < fix.size(); ++b) {
        if (fix[b] == 1) text_nll[b] = std::numeric_limits<float>::quiet_NaN();
        if (fix[b] == 2) text_nll[b] = std::numeric_limits<float>::infinity();
    }
}

// ---------------------------------------------------------------------------------------------
// word-sequence recognition (hctr_words*): the device copy of the word tables, the groups of lines that share one block
// of emissions, records and step buffers, scratch
// ---------------------------------------------------------------------------------------------
// whether a trie's two step buffers live in LDS: when they fit, unless HCTR_WORDS_LDS=0 keeps them in the call's scratch
// (for the tests: results do not depend on it)
bool words_lds(int nodes) {
    const char* e = getenv("HCTR_WORDS_LDS");
    if (e && *e && atoi(e) == 0) return false;
    return nodes <= kWordsLdsNodes;
}

// lines one group holds: HCTR_WORDS_LINES, else what keeps a group's emissions (4*W*D bytes a line), records (32*W) and
// scratch-form step buffers (32*nodes) within the 4 GiB of the lexicon call's emissions, at least 1. Results do not
// depend on it.
int words_group_lines(int nodes, int D, int W, bool lds) {
    if (const char* e = getenv("HCTR_WORDS_LINES")) {
        const int v = atoi(e);
        if (v >= 1) return v;
    }
    const int64_t per = (int64_t)std::max(W, 1) * (4 * (int64_t)std::max(D, 1) + 32) + (lds ? 0 : 32 * (int64_t)nodes);
    return (int)std::min<int64_t>(1 << 20, std::max<int64_t>(1, ((int64_t)4 << 30) / per));
}

// the words of the device block: node | slot | entry | weight (float bits) | cls
struct WordsLayout {
    size_t node, slot, entry, weight, cls, words;
    explicit WordsLayout(const WordTables& t) {
        WordTaker take;
        node = take(t.node.size()); slot = take(t.slot.size()); entry = take(t.entry.size());
        weight = take(t.weight.size()); cls = take(t.cls.size());
        words = take.words;
    }
};

struct WordsOut {             // the caller's host outputs; any may be null
    float* score;
    int32_t *count, *words, *starts, *labels, *lengths;
    float* text_nll;
};

struct WordsHost {
    const hctr_lex* lex = nullptr;
    const WordTables* tab = nullptr;      // the context's
    int B = 0, D = 1, max_words = 1, group = 1;
    bool lds = true;
    std::vector<int32_t> up;      // the call's upload: T[B] | zero[B]
    std::vector<uint8_t> nll_fix; // [B] text_nll: 0 = the kernel's, 1 = NaN (the text exceeds the loss's labels), 2 = +inf
};

int words_prepare(hctr_ctx* c, const hctr_lex* lex, float word_bonus, int max_words, int B, int W, int C,
                  const int32_t* input_lengths, WordsHost* h) {
    if (!lex) return fail(c, HCTR_ERR_ARG, "lex is NULL");
    if (lex->C != C) return fail(c, HCTR_ERR_ARG, "the lexicon was built for %d classes, the call has %d", lex->C, C);
    if (max_words < 1 || max_words > std::max(W, 1)) return fail(c, HCTR_ERR_ARG, "max_words=%d outside [1,%d]", max_words, W);
    if ((int64_t)std::max(B, 1) * std::max(max_words, W) > INT32_MAX)
        return fail(c, HCTR_ERR_ARG, "B*W=%lld too large", (long long)B * W);
    if (c->words_tab_serial != lex->serial || memcmp(&c->words_tab_bonus, &word_bonus, 4) != 0) {
        c->words_tab_serial = 0;
        std::string msg;
        if (!word_tables(*lex, word_bonus, &c->words_tab, &msg)) return fail(c, HCTR_ERR_ARG, "%s", msg.c_str());
        c->words_tab_serial = lex->serial;
        c->words_tab_bonus = word_bonus;
    }
    h->tab = &c->words_tab;
    TRY(lengths_head(c, B, W, input_lengths, 1, &h->up));
    h->lex = lex; h->B = B; h->D = h->tab->D(); h->max_words = max_words;
    h->lds = words_lds(h->tab->nodes());
    h->group = words_group_lines(h->tab->nodes(), h->D, W, h->lds);
    h->nll_fix.assign((size_t)B, 0);
    return HCTR_OK;
}

// the context's device copy of the call's word tables: uploaded when the context holds another lexicon's or bonus's
int words_on_device(hctr_ctx* c, const WordsHost& h, float word_bonus) {
    if (c->words_serial == h.lex->serial && memcmp(&c->words_bonus, &word_bonus, 4) == 0) return HCTR_OK;
    const WordTables& t = *h.tab;
    const WordsLayout lay(t);
    std::vector<int32_t> img(lay.words, 0);
    std::copy(t.node.begin(), t.node.end(), img.begin() + lay.node);
    std::copy(t.slot.begin(), t.slot.end(), img.begin() + lay.slot);
    std::copy(t.entry.begin(), t.entry.end(), img.begin() + lay.entry);
    memcpy(img.data() + lay.weight, t.weight.data(), t.weight.size() * 4);
    std::copy(t.cls.begin(), t.cls.end(), img.begin() + lay.cls);
    c->words_bonus = word_bonus;
    return tables_on_device(c, &c->words_serial, &c->words_dev, h.lex->serial, img, "word");
}

struct WordsDev {
    const int32_t* up = nullptr;
    int32_t *cls = nullptr, *nd = nullptr, *count = nullptr, *lengths = nullptr, *words = nullptr, *starts = nullptr,
            *labels = nullptr, *nll_tab = nullptr;
    float *score = nullptr, *nll = nullptr, *emis = nullptr;
    WordsRec* rec = nullptr;
    void* states = nullptr;       // the scratch form's step buffers, 32*nodes bytes a line
    int g = 1;                    // lines per group of this call's launches
};

// scratch of a words call that launches nl lines at a time, in groups of g = min(group, nl): the upload, the class
// tables, the results of all B lines, and per group the tables of the texts' loss, the emissions, the records and the
// step buffers that are not in LDS
int words_scratch(hctr_ctx* c, const WordsHost& h, int nl, int W, WordsDev* d) {
    const size_t B = (size_t)h.B, g = (size_t)std::max(1, std::min(h.group, nl)), nn = (size_t)h.tab->nodes();
    const size_t up_b = align256(h.up.size() * 4), cls_b = align256(B * h.D * 4), b4 = align256(B * 4),
                 w_b = align256(B * h.max_words * 4), col_b = align256(B * W * 4), tab_b = align256((3 * g + g * W) * 4),
                 emis_b = align256(g * W * h.D * 4), rec_b = align256(g * W * 2 * sizeof(WordsRec)),
                 st_b = h.lds ? 0 : align256(g * 2 * nn * 16);
    TRY(ctc_reserve(c, up_b + cls_b + 5 * b4 + 2 * w_b + col_b + tab_b + emis_b + rec_b + st_b));
    char* p = c->ctc_buf;
    auto take = [&](size_t bytes) { char* r = p; p += bytes; return r; };
    d->g = (int)g;
    d->up = (const int32_t*)take(up_b);
    d->cls = (int32_t*)take(cls_b);
    d->nd = (int32_t*)take(b4);
    d->score = (float*)take(b4); d->nll = (float*)take(b4);
    d->count = (int32_t*)take(b4); d->lengths = (int32_t*)take(b4);
    d->words = (int32_t*)take(w_b); d->starts = (int32_t*)take(w_b);
    d->labels = (int32_t*)take(col_b);
    d->nll_tab = (int32_t*)take(tab_b);
    d->emis = (float*)take(emis_b);
    d->rec = (WordsRec*)take(rec_b);
    d->states = st_b ? (void*)take(st_b) : nullptr;
    HIP_TRY(c, hipMemcpyAsync(c->ctc_buf, h.up.data(), h.up.size() * 4, hipMemcpyHostToDevice, c->stream));
    return HCTR_OK;
}

// the lines [b0, b0 + nb), whose logit rows are r, a group at a time: emissions, recursion, walk
int words_launch(hctr_ctx* c, WordsHost& h, const WordsDev& d, bool want_nll, const Rows& r, int b0, int nb, int W) {
    Prof pf(c);
    const WordsLayout lay(*h.tab);
    const int32_t* t = c->words_dev;
    const int nn = h.tab->nodes();
    PROF_TRY(pf, "lexicon_classes", launch_lexicon_classes(t + lay.cls, h.D, h.B, d.cls, d.nd, c->stream));
    const CtcLines m{d.up, d.up + h.B, d.up + h.B, d.nd, d.cls, d.up + h.B, h.D};
    for (int l0 = 0; l0 < nb; l0 += d.g) {
        const int n = std::min(d.g, nb - l0), gb0 = b0 + l0;
        TRY(lse_rows(pf, r.from_line(l0), m, gb0, n, W, d.emis));
        const WordsArgs a{d.emis, d.up, gb0, n, W, h.D, nn, t + lay.node, t + lay.slot, t + lay.entry,
                          (const float*)(t + lay.weight), d.states, d.rec};
        PROF_TRY(pf, "words_trie", launch_words_trie(a, c->stream));
        const WordsTraceArgs ta{d.rec, d.up, gb0, n, W, nn, h.max_words, t + lay.node, t + lay.slot, t + lay.entry,
                                t + lay.cls, d.score, d.count, d.words, d.starts, d.labels, d.lengths};
        PROF_TRY(pf, "words_backtrace", launch_words_backtrace(ta, c->stream));
        if (want_nll)
            TRY(text_nll_group(c, pf, TextNll{&h.lex->classes, h.D, &h.up, d.labels, d.lengths, d.count, 1, d.nll_tab,
                                              d.emis, d.nll, &h.nll_fix}, gb0, n, W));
    }
    return HCTR_OK;
}

int words_finish(hctr_ctx* c, const WordsHost& h, const WordsDev& d, const WordsOut& o, int W) {
    const size_t B = (size_t)h.B;
    HIP_TRY(c, fetch(c, o.score, d.score, B * 4));
    HIP_TRY(c, fetch(c, o.count, d.count, B * 4));
    HIP_TRY(c, fetch(c, o.words, d.words, B * h.max_words * 4));
    HIP_TRY(c, fetch(c, o.starts, d.starts, B * h.max_words * 4));
    HIP_TRY(c, fetch(c, o.labels, d.labels, B * W * 4));
    HIP_TRY(c, fetch(c, o.lengths, d.lengths, B * 4));
    HIP_TRY(c, fetch(c, o.text_nll, d.nll, B * 4));
    if (!o.text_nll) return HCTR_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    text_nll_fix(h.nll_fix, o.text_nll);
    return HCTR_OK;
}

// hctr_words*
int words_call(hctr_ctx* c, const Source& src, const hctr_lex* lex, float word_bonus, int max_words,
               const int32_t* input_lengths, const WordsOut& o) {
    const int B = src.B, W = src.W;
    WordsHost h;
    TRY(words_prepare(c, lex, word_bonus, max_words, B, W, src.C, input_lengths, &h));
    if (B == 0) return HCTR_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    TRY(words_on_device(c, h, word_bonus));
    WordsDev d;
    return source_passes(
        c, src,
        [&](const Pass& p, std::vector<void*>& pool) -> int {
            if (p.first == 0) TRY(words_scratch(c, h, p.nb, W, &d));
            Rows r;
            TRY(pass_rows(c, src, p, pool, &r));
            return words_launch(c, h, d, o.text_nll != nullptr, r, p.first, p.nb, W);
        },
        [&] { return words_finish(c, h, d, o, W); });
}

// ---------------------------------------------------------------------------------------------
// pattern-constrained recognition (hctr_pattern*): the device copy of the pattern, the groups of lines that share one
// block of emissions and backpointers, scratch
// ---------------------------------------------------------------------------------------------
// lines one group holds: HCTR_PAT_LINES, else what keeps a group's emissions (4*W*D bytes a line) and backpointers
// (2*W*S bytes a line) within 2 GiB, at least 1. Results do not depend on it.
constexpr int64_t kPatGroupBytes = (int64_t)2 << 30;
int pat_group_lines(int S, int D, int W) {
    if (const char* e = getenv("HCTR_PAT_LINES")) {
        const int v = atoi(e);
        if (v >= 1) return v;
    }
    const int64_t per = (int64_t)std::max(W, 1) * (4 * (int64_t)std::max(D, 1) + 2 * (int64_t)std::max(S, 1));
    return (int)std::min<int64_t>(1 << 20, std::max<int64_t>(1, kPatGroupBytes / per));
}

// the words of the device block: slot | label | in_ptr | accept | start | cls (0, then the classes) | in_src (uint16),
// and for a weighted pattern (kind 2) | in_w | accept_w | start_w (float)
struct PatLayout {
    size_t slot, label, in_ptr, accept, start, cls, in_src, in_w, accept_w, start_w, words;
    explicit PatLayout(const hctr_pat& x) {
        WordTaker take;
        slot = take(x.slot.size()); label = take(x.label.size()); in_ptr = take(x.in_ptr.size());
        accept = take(x.accept.size()); start = take(x.start.size()); cls = take(x.classes.size() + 1);
        in_src = take((x.in_src.size() + 1) / 2);
        in_w = take(x.in_w.size()); accept_w = take(x.accept_w.size()); start_w = take(x.start_w.size());
        words = take.words;
    }
};

// the set form's block: slot | label | meta (2 words a state) | blk_ptr | in_arc | finals | cls (0, then the classes)
struct PatSetLayout {
    size_t slot, label, meta, blk_ptr, in_arc, finals, cls, words;
    explicit PatSetLayout(const hctr_pat& x) {
        WordTaker take;
        slot = take(x.slot.size()); label = take(x.label.size()); meta = take(x.meta.size());
        blk_ptr = take(x.blk_ptr.size()); in_arc = take(x.in_arc.size()); finals = take(x.finals.size());
        cls = take(x.classes.size() + 1);
        words = take.words;
    }
};

// whether a set pattern's two step buffers live in LDS: when they fit beside the block totals, unless HCTR_PATSET_LDS=0
// keeps them in the call's scratch (for the tests: results do not depend on it)
bool pat_set_lds(const hctr_pat& x, bool vit) {
    const char* e = getenv("HCTR_PATSET_LDS");
    if (e && atoi(e) == 0 && *e) return false;
    return pattern_set_states_in_lds(x.S, x.nQ, vit);
}

// the context's device copy of the call's pattern: uploaded when the context holds another one (or none)
int pat_on_device(hctr_ctx* c, const hctr_pat* x) {
    if (c->pat_serial == x->serial) return HCTR_OK;
    if (x->kind == 1) {
        const PatSetLayout lay(*x);
        std::vector<int32_t> img(lay.words, 0);
        std::copy(x->slot.begin(), x->slot.end(), img.begin() + lay.slot);
        std::copy(x->label.begin(), x->label.end(), img.begin() + lay.label);
        memcpy(img.data() + lay.meta, x->meta.data(), x->meta.size() * 4);
        std::copy(x->blk_ptr.begin(), x->blk_ptr.end(), img.begin() + lay.blk_ptr);
        memcpy(img.data() + lay.in_arc, x->in_arc.data(), x->in_arc.size() * 4);
        std::copy(x->finals.begin(), x->finals.end(), img.begin() + lay.finals);
        std::copy(x->classes.begin(), x->classes.end(), img.begin() + lay.cls + 1);
        return tables_on_device(c, &c->pat_serial, &c->pat_dev, x->serial, img, "pattern");
    }
    const PatLayout lay(*x);
    std::vector<int32_t> img(lay.words, 0);
    std::copy(x->slot.begin(), x->slot.end(), img.begin() + lay.slot);
    std::copy(x->label.begin(), x->label.end(), img.begin() + lay.label);
    std::copy(x->in_ptr.begin(), x->in_ptr.end(), img.begin() + lay.in_ptr);
    std::copy(x->accept.begin(), x->accept.end(), img.begin() + lay.accept);
    std::copy(x->start.begin(), x->start.end(), img.begin() + lay.start);
    std::copy(x->classes.begin(), x->classes.end(), img.begin() + lay.cls + 1);
    memcpy(img.data() + lay.in_src, x->in_src.data(), x->in_src.size() * 2);
    if (x->kind == 2) {
        memcpy(img.data() + lay.in_w, x->in_w.data(), x->in_w.size() * 4);
        memcpy(img.data() + lay.accept_w, x->accept_w.data(), x->accept_w.size() * 4);
        memcpy(img.data() + lay.start_w, x->start_w.data(), x->start_w.size() * 4);
    }
    return tables_on_device(c, &c->pat_serial, &c->pat_dev, x->serial, img, "pattern");
}

struct PatOut {               // the caller's host outputs; any may be null
    float *logp, *best;
    int32_t *path, *labels, *lengths, *span_start, *span_end;
    float *char_logp, *text_nll;
    bool viterbi() const { return best || path || labels || lengths || span_start || span_end || char_logp || text_nll; }
};

struct PatHost {
    const hctr_pat* pat = nullptr;
    int B = 0, D = 1, group = 1;
    bool vit = false;
    std::vector<int32_t> up;      // the call's upload: T[B] | zero[B]
    std::vector<uint8_t> nll_fix; // [B] text_nll: 0 = the kernel's, 1 = NaN (the text exceeds the loss's labels), 2 = +inf
};

int pat_prepare(hctr_ctx* c, const hctr_pat* pat, int B, int W, int C, const int32_t* input_lengths, const PatOut& o,
                PatHost* h) {
    if (!pat) return fail(c, HCTR_ERR_ARG, "pat is NULL");
    if (pat->C != C) return fail(c, HCTR_ERR_ARG, "the pattern was built for %d classes, the call has %d", pat->C, C);
    TRY(lengths_head(c, B, W, input_lengths, 1, &h->up));
    h->pat = pat; h->B = B; h->D = (int)pat->classes.size() + 1; h->vit = o.viterbi();
    h->group = pat_group_lines(pat->S, h->D, W);
    h->nll_fix.assign((size_t)B, 0);
    return HCTR_OK;
}

struct PatDev {
    const int32_t* up = nullptr;
    int32_t *cls = nullptr, *nd = nullptr, *endst = nullptr, *lengths = nullptr, *path = nullptr, *labels = nullptr,
            *st = nullptr, *en = nullptr, *nll_tab = nullptr;
    float *logp = nullptr, *best = nullptr, *nll = nullptr, *clp = nullptr, *lpv = nullptr, *emis = nullptr;
    float* states = nullptr;      // a set pattern's step buffers, 16*S bytes a line, when they are not in LDS
    uint16_t* bp = nullptr;
    int g = 1;                    // lines per group of this call's launches
};

// scratch of a pattern call that launches nl lines at a time, in groups of g = min(group, nl): the upload, the class
// tables, the per-line and per-column results of all B lines, and per group the walk's scratch, the tables of the
// decoded texts' loss, the emissions, the backpointers and a set pattern's step buffers that are not in LDS
int pat_scratch(hctr_ctx* c, const PatHost& h, int nl, int W, PatDev* d) {
    const size_t B = (size_t)h.B, g = (size_t)std::max(1, std::min(h.group, nl)), S = (size_t)h.pat->S;
    const size_t up_b = align256(h.up.size() * 4), cls_b = align256(B * h.D * 4), b4 = align256(B * 4),
                 col_b = h.vit ? align256(B * W * 4) : 0, lpv_b = h.vit ? align256(g * W * 4) : 0,
                 tab_b = h.vit ? align256((3 * g + g * W) * 4) : 0, emis_b = align256(g * W * h.D * 4),
                 bp_b = h.vit ? align256(g * W * S * 2) : 0,
                 st_b = h.pat->kind == 1 && !pat_set_lds(*h.pat, h.vit) ? align256(g * S * 16) : 0;
    TRY(ctc_reserve(c, up_b + cls_b + 6 * b4 + 5 * col_b + lpv_b + tab_b + emis_b + bp_b + st_b));
    char* p = c->ctc_buf;
    auto take = [&](size_t bytes) { char* r = p; p += bytes; return r; };
    d->g = (int)g;
    d->up = (const int32_t*)take(up_b);
    d->cls = (int32_t*)take(cls_b);
    d->nd = (int32_t*)take(b4);
    d->logp = (float*)take(b4); d->best = (float*)take(b4); d->nll = (float*)take(b4);
    d->endst = (int32_t*)take(b4); d->lengths = (int32_t*)take(b4);
    d->path = (int32_t*)take(col_b); d->labels = (int32_t*)take(col_b); d->st = (int32_t*)take(col_b);
    d->en = (int32_t*)take(col_b); d->clp = (float*)take(col_b);
    d->lpv = (float*)take(lpv_b);
    d->nll_tab = (int32_t*)take(tab_b);
    d->emis = (float*)take(emis_b);
    d->bp = (uint16_t*)take(bp_b);
    d->states = st_b ? (float*)take(st_b) : nullptr;
    HIP_TRY(c, hipMemcpyAsync(c->ctc_buf, h.up.data(), h.up.size() * 4, hipMemcpyHostToDevice, c->stream));
    return HCTR_OK;
}

// the lines [b0, b0 + nb), whose logit rows are r, a group at a time: emissions, recursion, walk
int pat_launch(hctr_ctx* c, PatHost& h, const PatDev& d, bool want_nll, const Rows& r, int b0, int nb, int W) {
    Prof pf(c);
    const hctr_pat& px = *h.pat;
    const PatLayout lay(px);
    const PatSetLayout slay(px);
    const int32_t* t = c->pat_dev;
    const bool sets = px.kind == 1;
    const size_t cls = sets ? slay.cls : lay.cls, slot = sets ? slay.slot : lay.slot, label = sets ? slay.label : lay.label;
    PROF_TRY(pf, "pattern_classes", launch_lexicon_classes(t + cls, h.D, h.B, d.cls, d.nd, c->stream));
    const CtcLines m{d.up, d.up + h.B, d.up + h.B, d.nd, d.cls, d.up + h.B, h.D};
    for (int l0 = 0; l0 < nb; l0 += d.g) {
        const int n = std::min(d.g, nb - l0), gb0 = b0 + l0;
        TRY(lse_rows(pf, r.from_line(l0), m, gb0, n, W, d.emis));
        if (sets) {
            const PatSetArgs a{d.emis, d.up, gb0, n, W, h.D, px.S, px.nQ, (const uint32_t*)(t + slay.meta), t + slay.blk_ptr,
                               (const uint32_t*)(t + slay.in_arc), t + slay.finals, (int)px.finals.size(), d.states, d.bp,
                               d.logp, d.best, d.endst};
            PROF_TRY(pf, "pattern_set", launch_pattern_set(a, h.vit, c->stream));
        } else {
            const PatArgs a{d.emis, d.up, gb0, n, W, h.D, px.S, px.edges(), t + lay.slot, t + lay.label, t + lay.in_ptr,
                            (const uint16_t*)(t + lay.in_src), t + lay.accept, t + lay.start, (int)px.accept.size(),
                            (int)px.start.size(), d.bp, d.logp, d.best, d.endst};
            if (px.kind == 2) {
                const PatWeights w{(const float*)(t + lay.in_w), (const float*)(t + lay.accept_w),
                                   (const float*)(t + lay.start_w)};
                PROF_TRY(pf, "pattern_w", launch_pattern_weighted(a, w, h.vit, c->stream));
            } else {
                PROF_TRY(pf, "pattern", launch_pattern(a, h.vit, c->stream));
            }
        }
        if (!h.vit) continue;
        const PatTraceArgs ta{d.emis, d.up, gb0, n, W, h.D, px.S, t + slot, t + label, d.bp, d.endst, d.lpv,
                              d.path, d.labels, d.lengths, d.st, d.en, d.clp};
        PROF_TRY(pf, "pattern_trace", launch_pattern_trace(ta, c->stream));
        if (want_nll)
            TRY(text_nll_group(c, pf, TextNll{&px.classes, h.D, &h.up, d.labels, d.lengths, d.endst, 0, d.nll_tab, d.emis,
                                              d.nll, &h.nll_fix}, gb0, n, W));
    }
    return HCTR_OK;
}

int pat_finish(hctr_ctx* c, const PatHost& h, const PatDev& d, const PatOut& o, int W) {
    const size_t B = (size_t)h.B, cb = B * W * 4;
    HIP_TRY(c, fetch(c, o.logp, d.logp, B * 4));
    HIP_TRY(c, fetch(c, o.best, d.best, B * 4));
    HIP_TRY(c, fetch(c, o.path, d.path, cb));
    HIP_TRY(c, fetch(c, o.labels, d.labels, cb));
    HIP_TRY(c, fetch(c, o.lengths, d.lengths, B * 4));
    HIP_TRY(c, fetch(c, o.span_start, d.st, cb));
    HIP_TRY(c, fetch(c, o.span_end, d.en, cb));
    HIP_TRY(c, fetch(c, o.char_logp, d.clp, cb));
    HIP_TRY(c, fetch(c, o.text_nll, d.nll, B * 4));
    if (!o.text_nll) return HCTR_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    text_nll_fix(h.nll_fix, o.text_nll);
    return HCTR_OK;
}

// hctr_pattern*
int pat_call(hctr_ctx* c, const Source& src, const hctr_pat* pat, const int32_t* input_lengths, const PatOut& o) {
    const int B = src.B, W = src.W;
    PatHost h;
    TRY(pat_prepare(c, pat, B, W, src.C, input_lengths, o, &h));
    if (B == 0) return HCTR_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    TRY(pat_on_device(c, pat));
    PatDev d;
    return source_passes(
        c, src,
        [&](const Pass& p, std::vector<void*>& pool) -> int {
            if (p.first == 0) TRY(pat_scratch(c, h, p.nb, W, &d));
            Rows r;
            TRY(pass_rows(c, src, p, pool, &r));
            return pat_launch(c, h, d, o.text_nll != nullptr, r, p.first, p.nb, W);
        },
        [&] { return pat_finish(c, h, d, o, W); });
}

// ---------------------------------------------------------------------------------------------
// greedy recognition (hctr_recognize*)
// ---------------------------------------------------------------------------------------------
struct RecOut {              // the caller's host outputs, [B][W] / [B]; any may be null
    int32_t *labels, *lengths, *span_start, *span_end;
    float* char_logp;
    int32_t* alt_label;
    float *alt_logp, *path_logp, *text_nll;
};

struct RecCall {             // + where the batch's labels and lengths go on the host: the caller's arrays, or the call's
    RecOut o;                // own when only text_nll needs them (null when nobody does)
    std::vector<int32_t> own_lab, own_len;
    int32_t *h_lab, *h_len;
    RecCall(const RecOut& out, int B, int W) : o(out) {
        if (o.text_nll && !o.labels) own_lab.resize((size_t)B * W);
        if (o.text_nll && !o.lengths) own_len.resize((size_t)B);
        h_lab = o.labels ? o.labels : o.text_nll ? own_lab.data() : nullptr;
        h_len = o.lengths ? o.lengths : o.text_nll ? own_len.data() : nullptr;
    }
};

// One pass of nb lines, [b0, b0 + nb) of the caller's batch, whose logit rows are r. The CTC scratch holds lse[nb*W]
// first, which outlives the row figures and the spans; once those are on the host the tables, nll and emissions of the
// decoded text take their place. Returns with the stream drained when text_nll is wanted.
int rec_pass(hctr_ctx* c, const Rows& r, int b0, int nb, int W, const RecCall& rc) {
    const RecOut& o = rc.o;
    const int C = r.C;
    int32_t *const h_lab = rc.h_lab, *const h_len = rc.h_len;
    const size_t n = (size_t)nb, col_b = align256(n * W * 4), line_b = align256(n * 4), lse_b = align256(n * W * 8);
    TRY(ctc_reserve(c, lse_b + 10 * col_b + 2 * line_b));
    double* d_lse = (double*)c->ctc_buf;
    char* q = c->ctc_buf + lse_b;
    auto col = [&]() { char* at = q; q += col_b; return at; };
    int32_t *k1 = (int32_t*)col(), *k2 = (int32_t*)col();
    float *lp1 = (float*)col(), *lp2 = (float*)col();
    int32_t *d_lab = (int32_t*)col(), *d_st = (int32_t*)col(), *d_en = (int32_t*)col(), *d_alab = (int32_t*)col();
    float *d_clp = (float*)col(), *d_alp = (float*)col();
    int32_t* d_len = (int32_t*)q;
    float* d_plp = (float*)(q + line_b);
    Prof pf(c);
    PROF_TRY(pf, "greedy_rowstat", launch_greedy_rowstat(r.x, r.ld, r.sb, r.st, C, nb, W, k1, k2, lp1, lp2, d_lse,
                                                         c->stream));
    PROF_TRY(pf, "greedy_spans", launch_greedy_spans(k1, k2, lp1, lp2, nb, W, C, d_lab, d_len, d_st, d_en, d_clp,
                                                     d_alab, d_alp, d_plp, c->stream));
    const size_t co = (size_t)b0 * W, cb = n * W * 4;
    HIP_TRY(c, fetch(c, h_lab ? h_lab + co : nullptr, d_lab, cb));
    HIP_TRY(c, fetch(c, h_len ? h_len + b0 : nullptr, d_len, n * 4));
    HIP_TRY(c, fetch(c, o.span_start ? o.span_start + co : nullptr, d_st, cb));
    HIP_TRY(c, fetch(c, o.span_end ? o.span_end + co : nullptr, d_en, cb));
    HIP_TRY(c, fetch(c, o.char_logp ? o.char_logp + co : nullptr, d_clp, cb));
    HIP_TRY(c, fetch(c, o.alt_label ? o.alt_label + co : nullptr, d_alab, cb));
    HIP_TRY(c, fetch(c, o.alt_logp ? o.alt_logp + co : nullptr, d_alp, cb));
    HIP_TRY(c, fetch(c, o.path_logp ? o.path_logp + b0 : nullptr, d_plp, n * 4));
    if (!o.text_nll) return HCTR_OK;
    std::vector<float> plp(n);                 // a NaN here marks a line with a NaN row
    HIP_TRY(c, fetch(c, plp.data(), d_plp, n * 4));
    // the loss of the decoded text: its tables are built as the loss builds them, on labels that must be on the host
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<int32_t> tg, tl((size_t)nb);
    for (int b = 0; b < nb; ++b) {
        const int L = h_len[b0 + b];
        const bool fits = 2 * (int64_t)L + 1 <= kCtcMaxStates;      // a longer text gets NaN, not an error
        tl[(size_t)b] = fits ? L : 0;
        if (fits) tg.insert(tg.end(), h_lab + (co + (size_t)b * W), h_lab + (co + (size_t)b * W) + L);
    }
    CtcHost h;
    TRY(ctc_prepare(c, nb, W, C, tg.data(), tl.data(), nullptr, &h));
    const size_t tab_b = align256(h.tab.size() * 4);
    TRY(ctc_reserve(c, lse_b + tab_b + line_b + n * W * h.D * 4, lse_b));
    d_lse = (double*)c->ctc_buf;
    const CtcLines m = h.lines((const int32_t*)(c->ctc_buf + lse_b));
    float* d_nll = (float*)(c->ctc_buf + lse_b + tab_b);
    float* emis = (float*)(c->ctc_buf + lse_b + tab_b + line_b);
    HIP_TRY(c, hipMemcpyAsync(c->ctc_buf + lse_b, h.tab.data(), h.tab.size() * 4, hipMemcpyHostToDevice, c->stream));
    PROF_TRY(pf, "ctc_emis_gather", launch_ctc_emis_gather(r.x, r.ld, r.sb, r.st, m, 0, nb, W, d_lse, emis, c->stream));
    PROF_TRY(pf, "ctc_alpha", launch_ctc_alpha(emis, m, 0, nb, W, h.max_states, d_nll, nullptr, nullptr, c->stream));
    HIP_TRY(c, hipMemcpyAsync(o.text_nll + b0, d_nll, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // the recursion's max / min drop a NaN emission, so the loss of a line with a NaN row is no figure: NaN, by contract
    for (int b = 0; b < nb; ++b)
        if (tl[(size_t)b] != h_len[b0 + b] || plp[(size_t)b] != plp[(size_t)b])
            o.text_nll[b0 + b] = std::numeric_limits<float>::quiet_NaN();
    return HCTR_OK;
}

// hctr_recognize*: every pass sizes its own scratch and fetches its own lines
int rec_call(hctr_ctx* c, const Source& src, const RecOut& o) {
    if (src.B == 0) return HCTR_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const RecCall rc(o, src.B, src.W);
    return source_passes(c, src, [&](const Pass& p, std::vector<void*>& pool) -> int {
        Rows r;
        TRY(pass_rows(c, src, p, pool, &r));
        return rec_pass(c, r, p.first, p.nb, src.W, rc);
    });
}

// ---------------------------------------------------------------------------------------------
// greedy decode of line images (hctr_greedy, hctr_evaluate)
// ---------------------------------------------------------------------------------------------
// The passes of hctr_greedy: forward, argmax, collapse, labels and lengths copied to the host arrays (which may be null).
// A first-sweep pass's lines are consecutive rows of the caller's arrays; the flagged lines of the second sweep are not,
// so their labels are staged in the context and scattered by greedy_scatter once they are on the host. `redo` receives
// the lines of the second sweep. after(pf, p) queues what a caller adds behind a pass's collapse, on ws.labels / lengths.
template <class After>
int greedy_passes(hctr_ctx* c, const Batch& in, int32_t* labels, int32_t* lengths, std::vector<int>* redo, After after) {
    const int C = c->num_classes, W = in.W;
    const HeadMode hm = c->fuse_argmax ? HEAD_ARGMAX : HEAD_LOGITS;
    return run_passes(c, in, PASS_OWN, [&](const Pass& p) -> int {
        if (p.rerun && p.first == 0) {
            redo->assign(p.lines, p.lines + p.total);
            c->h_labels.resize((size_t)p.total * W);
            c->h_lengths.resize((size_t)p.total);
        }
        TRY(forward_pass(c, in, p, hm));
        Workspace& ws = c->ws;
        Prof pf(c);
        if (!c->fuse_argmax) {
            PROF_TRY(pf, "argmax_rows",
                     launch_argmax_rows(ws.logits, c->cpad, (int64_t)p.nb * W, C, ws.colidx, 0, 0, c->stream));
        }
        PROF_TRY(pf, "ctc_collapse", launch_ctc_collapse(ws.colidx, p.nb, W, C, ws.labels, ws.lengths, c->stream));
        int32_t* lab_dst = p.rerun ? c->h_labels.data() : labels;
        int32_t* len_dst = p.rerun ? c->h_lengths.data() : lengths;
        if (labels)
            HIP_TRY(c, hipMemcpyAsync(lab_dst + (size_t)p.first * W, ws.labels, (size_t)p.nb * W * 4, hipMemcpyDeviceToHost,
                                      c->stream));
        if (lengths)
            HIP_TRY(c, hipMemcpyAsync(len_dst + p.first, ws.lengths, (size_t)p.nb * 4, hipMemcpyDeviceToHost, c->stream));
        return after(pf, p);
    });
}

// the re-run lines' labels into the caller's rows (the stream is drained): whole rows, zeros beyond each length as
// ctc_collapse wrote them, so that nothing of the first sweep's longer text stays behind
void greedy_scatter(hctr_ctx* c, const std::vector<int>& redo, int W, int32_t* labels, int32_t* lengths) {
    for (size_t i = 0; i < redo.size() && lengths; ++i) {
        lengths[redo[i]] = c->h_lengths[i];
        if (labels) memcpy(labels + (size_t)redo[i] * W, c->h_labels.data() + i * W, (size_t)W * 4);
    }
}

// ---------------------------------------------------------------------------------------------
// edit distance (hctr_edit_distance, hctr_evaluate*)
// ---------------------------------------------------------------------------------------------
struct EditOut {             // the caller's host outputs; any may be null
    int32_t *edits, *counts, *ref_map, *hyp_map;
    bool maps() const { return counts || ref_map || hyp_map; }
};

// One call's references, its scratch layout and its device pointers. The scratch, in the context's CTC block:
// tab | edits[B] | line_of[B] | counts[B][4] | ref_map[sum L] | hyp_map[B][stride] | boff[B] | user | backpointers,
// counts to boff and the backpointers only with maps; the backpointers hold the `pass_lines` largest lines, which bounds every pass.
struct EditCall {
    std::vector<int32_t> tab;             // L[B] | off[B] | ref[sum L], uploaded as one block
    std::vector<int64_t> line_bytes;      // [B] backpointer bytes of each line at its bound on H (maps only)
    std::vector<std::vector<int64_t>> boffs;      // per pass: sources of queued copies, kept until the call ends
    int B = 0, stride = 0, max_len = 0;
    size_t total = 0;
    bool maps = false;
    EditLines m{};
    int32_t *d_edits = nullptr, *d_counts = nullptr, *d_rmap = nullptr, *d_hmap = nullptr, *d_line_of = nullptr;
    int64_t* d_boff = nullptr;
    char* d_user = nullptr;
    uint8_t* d_bp = nullptr;
    size_t bp_cap = 0;
};

// argument checks and the tables. hyp_bound[b] (null: `stride` for every line) bounds the line's hypothesis length
int edit_prepare(hctr_ctx* c, int B, int stride, const int32_t* ref, const int32_t* ref_lengths, const int32_t* hyp_bound,
                 bool maps, EditCall* e) {
    if (!ref_lengths) return fail(c, HCTR_ERR_ARG, "ref_lengths is NULL");
    const int limit = kEditMaxRows - 1;
    int64_t total = 0;
    int max_len = 0;
    for (int b = 0; b < B; ++b) {
        const int L = ref_lengths[b];
        if (L < 0 || L > limit) return fail(c, HCTR_ERR_ARG, "ref_lengths[%d]=%d outside [0,%d]", b, L, limit);
        total += L;
        max_len = std::max(max_len, L);
    }
    if (total > 0 && !ref) return fail(c, HCTR_ERR_ARG, "ref is NULL");
    if (total > INT32_MAX) return fail(c, HCTR_ERR_ARG, "too many reference symbols (%lld)", (long long)total);
    e->B = B; e->stride = stride; e->max_len = max_len; e->total = (size_t)total; e->maps = maps;
    e->tab.assign(2 * (size_t)B + (size_t)total, 0);
    int64_t o = 0;
    for (int b = 0; b < B; ++b) {
        e->tab[(size_t)b] = ref_lengths[b];
        e->tab[(size_t)B + b] = (int32_t)o;
        o += ref_lengths[b];
    }
    if (total) memcpy(e->tab.data() + 2 * (size_t)B, ref, (size_t)total * 4);
    if (maps) {
        const int ns = edit_lane_rows(max_len);
        e->line_bytes.assign((size_t)B, 0);
        for (int b = 0; b < B; ++b) {
            const int64_t L = ref_lengths[b], H = hyp_bound ? hyp_bound[b] : stride, lanes = (L + ns - 1) / ns;
            e->line_bytes[(size_t)b] = L > 0 && H > 0 ? (H + lanes - 1) * lanes : 0;
        }
    }
    return HCTR_OK;
}

// the scratch, with `user_b` bytes at d_user, and the tables' upload
int edit_scratch(hctr_ctx* c, EditCall* e, int pass_lines, size_t user_b) {
    const size_t B = (size_t)e->B;
    const size_t tab_b = align256(e->tab.size() * 4), line_b = align256(B * 4);
    size_t need = tab_b + 2 * line_b + align256(user_b), bp_b = 0;
    const size_t cnt_b = align256(B * 16), rmap_b = align256(e->total * 4), hmap_b = align256(B * e->stride * 4),
                 boff_b = align256(B * 8);
    if (e->maps) {
        std::vector<int64_t> big(e->line_bytes);
        const size_t n = std::min((size_t)std::max(pass_lines, 1), big.size());
        std::partial_sort(big.begin(), big.begin() + (std::ptrdiff_t)n, big.end(), std::greater<int64_t>());
        for (size_t i = 0; i < n; ++i) bp_b += (size_t)big[i];
        need += cnt_b + rmap_b + hmap_b + boff_b + align256(bp_b);
    }
    TRY(ctc_reserve(c, need));
    char* q = c->ctc_buf;
    auto take = [&](size_t bytes) { char* r = q; q += bytes; return r; };
    const int32_t* d_tab = (const int32_t*)take(tab_b);
    e->m = EditLines{d_tab, d_tab + B, d_tab + 2 * B};
    e->d_edits = (int32_t*)take(line_b);
    e->d_line_of = (int32_t*)take(line_b);
    if (e->maps) {
        e->d_counts = (int32_t*)take(cnt_b);
        e->d_rmap = (int32_t*)take(rmap_b);
        e->d_hmap = (int32_t*)take(hmap_b);
        e->d_boff = (int64_t*)take(boff_b);
    }
    e->d_user = take(align256(user_b));
    e->d_bp = e->maps ? (uint8_t*)q : nullptr;
    e->bp_cap = bp_b;
    HIP_TRY(c, hipMemcpyAsync(c->ctc_buf, e->tab.data(), e->tab.size() * 4, hipMemcpyHostToDevice, c->stream));
    return HCTR_OK;
}

// The kernels on the pass's lines lines[0..nb) of the batch, whose hypotheses lie at d_hyp[nb][stride] / d_hlen[nb]:
// d_line_of (the same numbers on the device) or, for consecutive lines, null.
int edit_launch(hctr_ctx* c, Prof& pf, EditCall* e, const int* lines, const int32_t* d_line_of, int nb,
                const int32_t* d_hyp, const int32_t* d_hlen) {
    const int b0 = lines[0];
    if (!e->maps) {
        PROF_TRY(pf, "edit_distance", launch_edit_distance(e->m, b0, d_line_of, nb, d_hyp, d_hlen, e->stride, e->max_len,
                                                           nullptr, nullptr, e->d_edits, c->stream));
        return HCTR_OK;
    }
    e->boffs.emplace_back((size_t)nb);
    std::vector<int64_t>& boff = e->boffs.back();
    int64_t bytes = 0;
    for (int b = 0; b < nb; ++b) {
        boff[(size_t)b] = bytes;
        bytes += e->line_bytes[(size_t)lines[b]];
    }
    if ((size_t)bytes > e->bp_cap) return fail(c, HCTR_ERR_STATE, "a pass of %d lines exceeds the backpointer scratch", nb);
    HIP_TRY(c, hipMemcpyAsync(e->d_boff, boff.data(), (size_t)nb * 8, hipMemcpyHostToDevice, c->stream));
    PROF_TRY(pf, "edit_distance", launch_edit_distance(e->m, b0, d_line_of, nb, d_hyp, d_hlen, e->stride, e->max_len,
                                                       e->d_boff, e->d_bp, e->d_edits, c->stream));
    PROF_TRY(pf, "edit_backtrace", launch_edit_backtrace(e->m, b0, d_line_of, nb, d_hyp, d_hlen, e->stride, e->max_len,
                                                         e->d_boff, e->d_bp, e->d_counts, e->d_rmap, e->d_hmap,
                                                         c->stream));
    return HCTR_OK;
}

int edit_fetch(hctr_ctx* c, const EditCall& e, const EditOut& o) {
    HIP_TRY(c, fetch(c, o.edits, e.d_edits, (size_t)e.B * 4));
    HIP_TRY(c, fetch(c, o.counts, e.d_counts, (size_t)e.B * 16));
    HIP_TRY(c, fetch(c, o.ref_map, e.d_rmap, e.total * 4));
    HIP_TRY(c, fetch(c, o.hyp_map, e.d_hmap, (size_t)e.B * e.stride * 4));
    return HCTR_OK;
}

// ---------------------------------------------------------------------------------------------
// the beam front end of one pass (hctr_beam_frontend, hctr_nbest*) and the prefix beam search on its lists (hctr_nbest*)
// ---------------------------------------------------------------------------------------------
struct BeamLists {           // one pass's lists on the device, rows r = t*nb + b: k classes / log-probs, blank log-prob,
    int32_t *idx = nullptr, *cnt = nullptr;      // (row max, log-sum) pairs, candidate counts
    float *lp = nullptr, *bl = nullptr, *st = nullptr;
    const float* rowsrc = nullptr;               // the logit rows [nb*W][ld] the lists were taken from (not when fused)
    int64_t ld = 0;
    bool fused = false;                          // the lists came out of the head GEMM's epilogues (ws.emit_* hold them)
};

// Log-softmax + top-k of the pass's lines: the forward of the source's images (or the caller's logits in WBC layout, one
// pass of all lines), then the fused front end or the stored-logits kernels. Temporaries live in c->beam_allocs, which
// the next pass (or the caller, at the end of its call) frees.
int beam_lists_pass(hctr_ctx* c, const Source& src, const Pass& p, int k, bool want_candidates, double thresh,
                    BeamLists* out) {
    std::vector<void*>& pool = c->beam_allocs;
    const int nb = p.nb, W = src.W, C = src.C;
    const int64_t rows = (int64_t)nb * W;
    const bool from_img = src.images();
    free_pool(pool);
    const float* rowsrc = nullptr;
    int64_t ld = 0;
    // fused front end (default): the logits are never stored; the head GEMM runs twice with reducing epilogues
    // (kernels.h ConvArgs). Not for k beyond the part count / kBeamMaxK, and a pass in which some row needed
    // more than kBeamCap list slots (near-uniform logits) is redone through the stored-logits kernels.
    bool fused = from_img && c->fuse_beam && k <= kBeamMaxK && k <= head_parts(c);
    if (from_img) {
        TRY(forward_pass(c, src.img, p, fused ? HEAD_BEAM : HEAD_LOGITS));
        rowsrc = c->ws.logits; ld = c->cpad;
    } else {
        float* rowsbuf = nullptr;
        const float* dev = nullptr;
        TRY(logits_on_device(c, pool, src.wbc, src.on_device, (size_t)rows * C, &dev));
        TRY(dev_alloc(c, pool, &rowsbuf, (size_t)rows * C, false));
        HIP_TRY(c, launch_wbc_to_rows(dev, nb, W, C, rowsbuf, C, c->stream));
        rowsrc = rowsbuf; ld = C;
    }
    // device outputs (rows r = t*nb + b): inside the arena on the fused path (no allocation per pass)
    int32_t *d_idx = nullptr, *d_cnt = nullptr;
    float *d_lp = nullptr, *d_bl = nullptr, *d_st = nullptr;
    auto own_outputs = [&]() -> int {
        TRY(dev_alloc(c, pool, &d_idx, (size_t)rows * k, false));
        TRY(dev_alloc(c, pool, &d_lp, (size_t)rows * k, false));
        TRY(dev_alloc(c, pool, &d_bl, (size_t)rows, false));
        TRY(dev_alloc(c, pool, &d_st, (size_t)rows * 2, false));
        TRY(dev_alloc(c, pool, &d_cnt, (size_t)rows, false));
        return HCTR_OK;
    };
    if (fused) {
        const Workspace& w0 = c->ws;
        d_idx = w0.bm_idx; d_lp = w0.bm_lp; d_bl = w0.bm_bl; d_st = w0.bm_st; d_cnt = w0.bm_cnt;
        TRY(beam_finish(c, k, want_candidates, thresh, d_idx, d_lp, d_bl, d_st, d_cnt));
        int32_t ovf = 0;
        HIP_TRY(c, hipMemcpyAsync(&ovf, c->ws.overflow, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (ovf) {                       // redo this pass with stored logits (re-staged: carving may move the arena)
            fused = false;
            ++c->beam_fallbacks;
            Pass redo = p;
            redo.guard_dst = nullptr;      // (the guard figures came back with the fused forward)
            TRY(forward_pass(c, src.img, redo, HEAD_LOGITS));
            rowsrc = c->ws.logits;
            TRY(own_outputs());
        }
    } else {
        TRY(own_outputs());
    }
    if (!fused) {
        Prof pf(c);
        PROF_TRY(pf, "row_topk", launch_row_topk(rowsrc, ld, nb, W, C, k, thresh, d_idx, d_lp, d_bl, d_st,
                                                 d_cnt, c->stream));
    }
    out->idx = d_idx; out->cnt = d_cnt; out->lp = d_lp; out->bl = d_bl; out->st = d_st;
    out->rowsrc = rowsrc; out->ld = ld; out->fused = fused;
    return HCTR_OK;
}

struct NbestOut {            // the caller's host outputs, [B][nbest][W] / [B][nbest] / [B]; any may be null
    int32_t *labels, *lengths;
    double *logp, *score;
    int32_t* count;
};

struct NbestCall {
    int B = 0, W = 0, C = 0, k = 0, beam = 0, nbest = 0;
    double len_bonus = 0.0;
    NbestOut o{};
    std::vector<int32_t> T;       // [B] steps of each line
    // device (the context's CTC scratch): T of the whole batch, the rest for the lines of one pass
    int32_t *d_T = nullptr, *d_lab = nullptr, *d_len = nullptr, *d_cnt = nullptr;
    double *d_logp = nullptr, *d_score = nullptr;
    int2* d_hist = nullptr;
    // the LM-scored search (hctr_nbest_lm*): lm == null is the zero-LM search, with none of the below
    const hctr_lm* lm = nullptr;
    double lm_panelty = 0.0;
    double* o_lm = nullptr;       // the caller's [B][nbest], may be null
    int32_t *d_end = nullptr, *d_wid = nullptr;
    int4* d_suf = nullptr;
    double* d_lm = nullptr;
    // the skip search (hctr_nbest_skip*): lm may be null (the zero LM); the pre-pass outputs and lm_score exist either way
    bool skip = false;
    int32_t *o_status = nullptr, *o_ranked = nullptr;      // the caller's [B], may be null
    int32_t *d_status = nullptr, *d_ranked = nullptr;
};

// the extra arguments of hctr_nbest_lm*
int nbest_lm_prepare(hctr_ctx* c, NbestCall* n, const hctr_lm* lm, double lm_panelty, double* lm_score) {
    if (!lm) return fail(c, HCTR_ERR_ARG, "lm is NULL");
    if (lm_panelty != lm_panelty) return fail(c, HCTR_ERR_ARG, "lm_panelty is NaN");
    if (lm->C != n->C) return fail(c, HCTR_ERR_ARG, "lm was built for %d classes, the call has %d", lm->C, n->C);
    n->lm = lm; n->lm_panelty = lm_panelty; n->o_lm = lm_score;
    return HCTR_OK;
}

// the context's device copy of the call's model: uploaded when the context holds another one (or none)
int lm_on_device(hctr_ctx* c, const hctr_lm* lm) {
    if (c->lm_serial == lm->serial) return HCTR_OK;
    c->lm_serial = 0;
    if (c->lm_slots) (void)hipFree(c->lm_slots);
    if (c->lm_words) (void)hipFree(c->lm_words);
    c->lm_slots = nullptr; c->lm_words = nullptr;
    const size_t slot_b = lm->slots.size() * sizeof(LmSlot), word_b = lm->label_words.size() * 4;
    void *ps = nullptr, *pw = nullptr;
    hipError_t e = hipMalloc(&ps, slot_b);
    if (e == hipSuccess) {
        e = hipMalloc(&pw, word_b);
        if (e != hipSuccess) (void)hipFree(ps);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, HCTR_ERR_NOMEM, "no device memory for the n-gram table (%zu bytes): %s", slot_b + word_b,
                    hipGetErrorString(e));
    }
    c->lm_slots = (LmSlot*)ps; c->lm_words = (int32_t*)pw;
    HIP_TRY(c, hipMemcpyAsync(ps, lm->slots.data(), slot_b, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(pw, lm->label_words.data(), word_b, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the model is the caller's: it may be freed after this call)
    c->lm_serial = lm->serial;
    return HCTR_OK;
}

int nbest_prepare(hctr_ctx* c, int B, int W, int C, int k, int beam, int nbest, double len_bonus,
                  const int32_t* input_lengths, const NbestOut& o, NbestCall* n) {
    if (nbest < 1 || nbest > beam || beam > kBeamMaxK)
        return fail(c, HCTR_ERR_ARG, "need 1 <= nbest <= beam <= %d, got nbest=%d beam=%d", kBeamMaxK, nbest, beam);
    if (k < 1 || k > C || k > kBeamMaxK)
        return fail(c, HCTR_ERR_ARG, "need 1 <= k <= min(C, %d), got k=%d C=%d", kBeamMaxK, k, C);
    if (len_bonus != len_bonus) return fail(c, HCTR_ERR_ARG, "len_bonus is NaN");
    if (o.labels && !o.lengths) return fail(c, HCTR_ERR_ARG, "labels needs lengths");
    n->B = B; n->W = W; n->C = C; n->k = k; n->beam = beam; n->nbest = nbest; n->len_bonus = len_bonus; n->o = o;
    n->T.assign((size_t)B, W);
    for (int b = 0; b < B && input_lengths; ++b) {
        const int Tb = input_lengths[b];
        if (Tb < 1 || Tb > W) return fail(c, HCTR_ERR_ARG, "input_lengths[%d]=%d outside [1,%d]", b, Tb, W);
        n->T[(size_t)b] = Tb;
    }
    return HCTR_OK;
}

// scratch for passes of at most `lines` lines; uploads T
int nbest_scratch(hctr_ctx* c, NbestCall* n, int lines) {
    const size_t ln = (size_t)lines * n->nbest;
    const size_t T_b = align256((size_t)n->B * 4), hist_b = align256((size_t)lines * n->W * n->beam * sizeof(int2)),
                 lab_b = align256(ln * n->W * 4), i32_b = align256(ln * 4), f64_b = align256(ln * 8),
                 cnt_b = align256((size_t)lines * 4);
    const size_t suf_b = align256((size_t)lines * n->W * sizeof(int4)), wid_b = align256((size_t)lines * n->W * n->k * 4);
    const bool pre = n->lm || n->skip, wids = n->lm && !n->skip;
    TRY(ctc_reserve(c, T_b + hist_b + lab_b + i32_b + 2 * f64_b + cnt_b + (pre ? cnt_b + suf_b + f64_b : 0) +
                           (wids ? wid_b : 0) + (n->skip ? 2 * cnt_b : 0)));
    if (n->lm) TRY(lm_on_device(c, n->lm));
    char* q = c->ctc_buf;
    n->d_T = (int32_t*)q; q += T_b;
    n->d_hist = (int2*)q; q += hist_b;
    n->d_lab = (int32_t*)q; q += lab_b;
    n->d_logp = (double*)q; q += f64_b;
    n->d_score = (double*)q; q += f64_b;
    n->d_len = (int32_t*)q; q += i32_b;
    n->d_cnt = (int32_t*)q; q += cnt_b;
    if (pre) {
        n->d_suf = (int4*)q; q += suf_b;
        n->d_lm = (double*)q; q += f64_b;
        if (wids) { n->d_wid = (int32_t*)q; q += wid_b; }
        n->d_end = (int32_t*)q; q += cnt_b;
    }
    if (n->skip) {
        n->d_status = (int32_t*)q; q += cnt_b;
        n->d_ranked = (int32_t*)q;
    }
    HIP_TRY(c, hipMemcpyAsync(n->d_T, n->T.data(), (size_t)n->B * 4, hipMemcpyHostToDevice, c->stream));
    return HCTR_OK;
}

// a search's results of the pass's lines [b0, b0 + nb), queued to the caller's rows; each exists in the searches that fill it
int nbest_fetch(hctr_ctx* c, const NbestCall& n, int b0, int nb) {
    const size_t ln = (size_t)nb * n.nbest, lo = (size_t)b0 * n.nbest;
    HIP_TRY(c, fetch(c, n.o.labels ? n.o.labels + lo * n.W : nullptr, n.d_lab, ln * n.W * 4));
    HIP_TRY(c, fetch(c, n.o.lengths ? n.o.lengths + lo : nullptr, n.d_len, ln * 4));
    HIP_TRY(c, fetch(c, n.o.logp ? n.o.logp + lo : nullptr, n.d_logp, ln * 8));
    HIP_TRY(c, fetch(c, n.o.score ? n.o.score + lo : nullptr, n.d_score, ln * 8));
    HIP_TRY(c, fetch(c, n.o.count ? n.o.count + b0 : nullptr, n.d_cnt, (size_t)nb * 4));
    if (n.lm || n.skip) HIP_TRY(c, fetch(c, n.o_lm ? n.o_lm + lo : nullptr, n.d_lm, ln * 8));
    if (n.skip) {
        HIP_TRY(c, fetch(c, n.o_status ? n.o_status + b0 : nullptr, n.d_status, (size_t)nb * 4));
        HIP_TRY(c, fetch(c, n.o_ranked ? n.o_ranked + b0 : nullptr, n.d_ranked, (size_t)nb * 4));
    }
    return HCTR_OK;
}

// the search of the pass's lines [b0, b0 + nb) on their lists (rows r = t*nb + b), results queued to the caller's rows
int nbest_launch(hctr_ctx* c, const NbestCall& n, const int32_t* d_idx, const float* d_lp, int b0, int nb) {
    const size_t ln = (size_t)nb * n.nbest;
    Prof pf(c);
    if (n.o.labels) HIP_TRY(c, hipMemsetAsync(n.d_lab, 0, ln * n.W * 4, c->stream));
    const int32_t* d_steps = n.d_T + b0;
    if (n.lm) {
        PROF_TRY(pf, "beam_lm_prepass", launch_beam_lm_prepass(d_idx, nb, n.W, n.k, n.C, n.d_T + b0, c->lm_words, n.d_wid,
                                                               n.d_suf, n.d_end, c->stream));
        BeamLm lm;
        lm.table = LmView{c->lm_slots, (uint32_t)n.lm->slots.size() - 1u, n.lm->order, n.lm->unk};
        lm.wid = n.d_wid; lm.suffix = n.d_suf; lm.lm_panelty = n.lm_panelty; lm.bos = n.lm->bos; lm.o_lm = n.d_lm;
        d_steps = n.d_end;
        PROF_TRY(pf, "prefix_beam_lm", launch_prefix_beam_lm(d_idx, d_lp, nb, n.W, n.k, n.C, n.beam, n.nbest, n.len_bonus,
                                                             d_steps, lm, n.d_hist, n.d_len, n.d_logp, n.d_score, n.d_cnt,
                                                             c->stream));
    } else {
        PROF_TRY(pf, "prefix_beam", launch_prefix_beam(d_idx, d_lp, nb, n.W, n.k, n.C, n.beam, n.nbest, n.len_bonus,
                                                       d_steps, n.d_hist, n.d_len, n.d_logp, n.d_score, n.d_cnt, c->stream));
    }
    if (n.o.labels)
        PROF_TRY(pf, "prefix_backtrace", launch_prefix_backtrace(n.d_hist, d_steps, nb, n.W, n.beam, n.nbest, n.d_len,
                                                                 n.d_cnt, n.d_lab, c->stream));
    return nbest_fetch(c, n, b0, nb);
}

// the extra arguments of hctr_nbest_skip*: lm == null is the zero LM, lm_panelty then unused
int nbest_skip_prepare(hctr_ctx* c, NbestCall* n, const hctr_lm* lm, double lm_panelty, double* lm_score, int32_t* status,
                       int32_t* ranked) {
    if (lm) TRY(nbest_lm_prepare(c, n, lm, lm_panelty, lm_score));
    n->skip = true; n->o_lm = lm_score; n->o_status = status; n->o_ranked = ranked;
    return HCTR_OK;
}

// the skip search of the pass's lines [b0, b0 + nb) on device lists, rows r = t*nb + b: the top-1 classes at top1[r * ks],
// the blank log-probs, and the candidates in the padded layout (kernels.h); results queued to the caller's rows
int skip_launch(hctr_ctx* c, const NbestCall& n, const int32_t* d_top1, int ks, const float* d_bl, const int32_t* d_cc,
                const int32_t* d_ci, const float* d_cl, int b0, int nb) {
    const size_t ln = (size_t)nb * n.nbest;
    Prof pf(c);
    if (n.o.labels) HIP_TRY(c, hipMemsetAsync(n.d_lab, 0, ln * n.W * 4, c->stream));
    PROF_TRY(pf, "beam_lm_prepass", launch_beam_lm_prepass(d_top1, nb, n.W, ks, n.C, n.d_T + b0, n.lm ? c->lm_words : nullptr,
                                                           nullptr, n.d_suf, n.d_end, c->stream));
    BeamLm lm;
    if (n.lm) {
        lm.table = LmView{c->lm_slots, (uint32_t)n.lm->slots.size() - 1u, n.lm->order, n.lm->unk};
        lm.bos = n.lm->bos;
    }
    lm.suffix = n.d_suf; lm.lm_panelty = n.lm_panelty; lm.o_lm = n.d_lm;
    PROF_TRY(pf, "prefix_beam_skip", launch_prefix_beam_skip(d_cc, d_ci, d_cl, d_bl, nb, n.W, n.C, n.beam, n.nbest,
                                                             n.len_bonus, n.d_end, n.lm ? c->lm_words : nullptr, lm, n.d_hist,
                                                             n.d_len, n.d_logp, n.d_score, n.d_cnt, n.d_status, n.d_ranked,
                                                             c->stream));
    if (n.o.labels)
        PROF_TRY(pf, "prefix_backtrace", launch_prefix_backtrace(n.d_hist, n.d_end, nb, n.W, n.beam, n.nbest, n.d_len,
                                                                 n.d_cnt, n.d_lab, c->stream));
    return nbest_fetch(c, n, b0, nb);
}

// ---------------------------------------------------------------------------------------------
// the LM weight sweep (hctr_lm_sweep*): the 1-best of the LM-scored search under G pairs of weights and its edit distance
// to the line's transcription, on one pre-pass and one set of lists per pass
// ---------------------------------------------------------------------------------------------
struct SweepArgs {           // what hctr_lm_sweep* take beyond hctr_nbest_lm*; the outputs are host pointers, any may be null
    const double *lm_panelty, *len_bonus;
    int G, chunk;
    const int32_t *targets, *target_lengths;
    int32_t *edits, *hyp_lengths;
    uint8_t* empty;
    int32_t* labels;
    double *logp, *score, *lm_score;
};

// pairs per launch when the caller leaves the choice to the engine (hctr_hip.h states the formula)
constexpr int64_t kSweepFillGroups = 8192;               // four times the ~2048 workgroups of the 10/10 rung the chip holds
constexpr int64_t kSweepChunkBytes = (int64_t)2 << 30;
int64_t sweep_pair_bytes(int lines, int W, int beam) { return (int64_t)lines * (8 * (int64_t)W * beam + 4 * (int64_t)W + 36); }
int sweep_chunk(int lines, int W, int beam, int G) {
    const int64_t l = std::max(lines, 1);
    const int64_t fill = std::max<int64_t>(1, kSweepFillGroups / l),
                  fit = std::max<int64_t>(1, kSweepChunkBytes / sweep_pair_bytes((int)l, std::max(W, 1), std::max(beam, 1)));
    return (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)G, fill, fit}));
}

struct SweepCall {
    bool on = false;
    SweepArgs a{};
    EditCall e;                   // the references (tab), their checks and max_len
    std::vector<double2> grid;    // [G] {lm_panelty, len_bonus}
    std::vector<int32_t> end;     // [B] the end steps, fetched for `empty`
    int Gc = 0;                   // pairs per launch
    const int32_t* d_tab = nullptr;
    double2* d_grid = nullptr;
    int32_t* d_edits = nullptr;
};

int sweep_prepare(hctr_ctx* c, const NbestCall& n, const SweepArgs& a, SweepCall* s) {
    if (a.G < 1) return fail(c, HCTR_ERR_ARG, "need G >= 1, got G=%d", a.G);
    if (!a.lm_panelty || !a.len_bonus) return fail(c, HCTR_ERR_ARG, "lm_panelty/len_bonus is NULL");
    for (int g = 0; g < a.G; ++g)
        if (a.lm_panelty[g] != a.lm_panelty[g] || a.len_bonus[g] != a.len_bonus[g])
            return fail(c, HCTR_ERR_ARG, "pair %d: %s is NaN", g, a.lm_panelty[g] != a.lm_panelty[g] ? "lm_panelty" : "len_bonus");
    if (a.chunk < 0 || a.chunk > a.G) return fail(c, HCTR_ERR_ARG, "chunk=%d outside [0,%d]", a.chunk, a.G);
    if ((int64_t)a.G * std::max(n.B, 1) > INT32_MAX) return fail(c, HCTR_ERR_ARG, "G*B=%lld too large", (long long)a.G * n.B);
    s->on = true; s->a = a;
    if (n.B == 0) return HCTR_OK;
    TRY(edit_prepare(c, n.B, n.W, a.targets, a.target_lengths, nullptr, false, &s->e));
    for (size_t j = 0; j < s->e.total; ++j)              // hctr_evaluate_logits' check of the ids
        if (a.targets[j] < 1 || a.targets[j] > n.C - 1)
            return fail(c, HCTR_ERR_ARG, "target id %d (position %zu) outside [1,%d]", a.targets[j], j, n.C - 1);
    s->grid.resize((size_t)a.G);
    for (int g = 0; g < a.G; ++g) s->grid[(size_t)g] = make_double2(a.lm_panelty[g], a.len_bonus[g]);
    s->end.assign((size_t)n.B, 0);
    return HCTR_OK;
}

// scratch for passes of at most `lines` lines, in the context's CTC block:
// T[B] | tab | grid[G] | suffix | wid | end (one pass's) | history | labels | len | cnt | edits | logp | score | lm (one chunk's);
// uploads T, the references and the pairs
int sweep_scratch(hctr_ctx* c, NbestCall* n, SweepCall* s, int lines) {
    s->Gc = s->a.chunk ? s->a.chunk : sweep_chunk(lines, n->W, n->beam, s->a.G);
    const size_t gl = (size_t)s->Gc * lines;
    const size_t T_b = align256((size_t)n->B * 4), tab_b = align256(s->e.tab.size() * 4),
                 grid_b = align256((size_t)s->a.G * sizeof(double2)),
                 suf_b = align256((size_t)lines * n->W * sizeof(int4)), wid_b = align256((size_t)lines * n->W * n->k * 4),
                 end_b = align256((size_t)lines * 4), hist_b = align256(gl * n->W * n->beam * sizeof(int2)),
                 lab_b = align256(gl * n->W * 4), i32_b = align256(gl * 4), f64_b = align256(gl * 8);
    TRY(ctc_reserve(c, T_b + tab_b + grid_b + suf_b + wid_b + end_b + hist_b + lab_b + 3 * i32_b + 3 * f64_b));
    TRY(lm_on_device(c, n->lm));
    char* q = c->ctc_buf;
    auto take = [&](size_t bytes) { char* r = q; q += bytes; return r; };
    n->d_T = (int32_t*)take(T_b);
    s->d_tab = (const int32_t*)take(tab_b);
    s->d_grid = (double2*)take(grid_b);
    n->d_suf = (int4*)take(suf_b);
    n->d_wid = (int32_t*)take(wid_b);
    n->d_end = (int32_t*)take(end_b);
    n->d_hist = (int2*)take(hist_b);
    n->d_lab = (int32_t*)take(lab_b);
    n->d_len = (int32_t*)take(i32_b);
    n->d_cnt = (int32_t*)take(i32_b);
    s->d_edits = (int32_t*)take(i32_b);
    n->d_logp = (double*)take(f64_b);
    n->d_score = (double*)take(f64_b);
    n->d_lm = (double*)take(f64_b);
    HIP_TRY(c, hipMemcpyAsync(n->d_T, n->T.data(), (size_t)n->B * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync((void*)s->d_tab, s->e.tab.data(), s->e.tab.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(s->d_grid, s->grid.data(), s->grid.size() * sizeof(double2), hipMemcpyHostToDevice, c->stream));
    return HCTR_OK;
}

// the sweep of the pass's lines [b0, b0 + nb) on their lists (rows r = t*nb + b): the pre-pass once, then per chunk of
// pairs the grid search, the backtrace and the distances of its gc * nb grid lines, queued to rows [g][b0 ..] of the outputs
int sweep_launch(hctr_ctx* c, const NbestCall& n, SweepCall& s, const int32_t* d_idx, const float* d_lp, int b0, int nb) {
    Prof pf(c);
    const SweepArgs& a = s.a;
    const size_t B = (size_t)n.B;
    PROF_TRY(pf, "beam_lm_prepass", launch_beam_lm_prepass(d_idx, nb, n.W, n.k, n.C, n.d_T + b0, c->lm_words, n.d_wid, n.d_suf,
                                                           n.d_end, c->stream));
    HIP_TRY(c, hipMemcpyAsync(s.end.data() + b0, n.d_end, (size_t)nb * 4, hipMemcpyDeviceToHost, c->stream));
    BeamLm lm;
    lm.table = LmView{c->lm_slots, (uint32_t)n.lm->slots.size() - 1u, n.lm->order, n.lm->unk};
    lm.wid = n.d_wid; lm.suffix = n.d_suf; lm.bos = n.lm->bos; lm.o_lm = n.d_lm;
    // grid line g * nb + b is measured against the reference of batch line b0 + b
    EditLines m{s.d_tab + b0, s.d_tab + B + b0, s.d_tab + 2 * B, nb};
    // rows [g0 .. g0 + gc) of a host array [G][B][per], columns of lines [b0, b0 + nb): one strided copy
    auto fetch = [&](void* dst, const void* src, int g0, int gc, size_t per, size_t elem) {
        if (!dst) return hipSuccess;
        return hipMemcpy2DAsync((char*)dst + ((size_t)g0 * B + b0) * per * elem, B * per * elem, src, (size_t)nb * per * elem,
                                (size_t)nb * per * elem, (size_t)gc, hipMemcpyDeviceToHost, c->stream);
    };
    for (int g0 = 0; g0 < a.G; g0 += s.Gc) {
        const int gc = std::min(s.Gc, a.G - g0), gl = gc * nb;
        HIP_TRY(c, hipMemsetAsync(n.d_lab, 0, (size_t)gl * n.W * 4, c->stream));
        lm.grid = s.d_grid + g0;
        PROF_TRY(pf, "prefix_beam_lm_grid", launch_prefix_beam_lm_grid(d_idx, d_lp, nb, n.W, n.k, n.C, n.beam, gc, n.d_end, lm,
                                                                       n.d_hist, n.d_len, n.d_logp, n.d_score, n.d_cnt,
                                                                       c->stream));
        PROF_TRY(pf, "prefix_backtrace", launch_prefix_backtrace(n.d_hist, n.d_end, gl, n.W, n.beam, 1, n.d_len, n.d_cnt,
                                                                 n.d_lab, c->stream, nb));
        PROF_TRY(pf, "edit_distance", launch_edit_distance(m, 0, nullptr, gl, n.d_lab, n.d_len, n.W, s.e.max_len, nullptr,
                                                           nullptr, s.d_edits, c->stream));
        HIP_TRY(c, fetch(a.edits, s.d_edits, g0, gc, 1, 4));
        HIP_TRY(c, fetch(a.hyp_lengths, n.d_len, g0, gc, 1, 4));
        HIP_TRY(c, fetch(a.labels, n.d_lab, g0, gc, (size_t)n.W, 4));
        HIP_TRY(c, fetch(a.logp, n.d_logp, g0, gc, 1, 8));
        HIP_TRY(c, fetch(a.score, n.d_score, g0, gc, 1, 8));
        HIP_TRY(c, fetch(a.lm_score, n.d_lm, g0, gc, 1, 8));
    }
    return HCTR_OK;
}

// after the stream has drained: the empty-greedy flags from the end steps
int sweep_finish(int rc, const SweepCall& s) {
    if (rc == HCTR_OK && s.on && s.a.empty)
        for (size_t b = 0; b < s.end.size(); ++b) s.a.empty[b] = s.end[b] == 0;
    return rc;
}

// the skip search on the lists of one front-end pass (made with k = 1 and candidates wanted): the candidates go to the
// padded layout where the counts already lie - no count visits the host - and the search follows in stream order
int skip_on_lists(hctr_ctx* c, const NbestCall& n, const BeamLists& L, int b0, int nb) {
    const size_t rows = (size_t)nb * n.W;
    int32_t* d_ci = nullptr;
    float* d_cl = nullptr;
    TRY(dev_alloc(c, c->beam_allocs, &d_ci, rows * kBeamMaxK, false));
    TRY(dev_alloc(c, c->beam_allocs, &d_cl, rows * kBeamMaxK, false));
    const double thresh = std::log(0.001);
    {
        Prof pf(c);
        PROF_TRY(pf, "skip_candidates",
                 L.fused ? launch_beam_candidates(c->ws.emit_cnt, c->ws.emit_list, kBeamCap, L.st, nb, n.W, thresh, nullptr,
                                                  kBeamMaxK, d_ci, d_cl, c->stream)
                         : launch_row_candidates(L.rowsrc, L.ld, nb, n.W, n.C, thresh, L.st, nullptr, kBeamMaxK, d_ci, d_cl,
                                                 c->stream));
    }
    return skip_launch(c, n, L.idx, 1, L.bl, L.cnt, d_ci, d_cl, b0, nb);
}

}  // namespace

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

#ifndef HCTR_SRC_HASH
#define HCTR_SRC_HASH "unhashed-build000"
#endif
// ends in the hash of the sources this binary was built from (_lib.py source_hash: stale-binary detection)
const char* hctr_version(void) {
    return "hctr-hip 0.3 (gfx950, f16 storage / f16 MFMA / f32 accumulate; f16x3 split precision; guarded mode) "
           "hctr-src=" HCTR_SRC_HASH;
}

int hctr_create(hctr_ctx** out, int device, int num_classes) {
    return guard(nullptr, [&]() -> int {
        if (!out) return fail(nullptr, HCTR_ERR_ARG, "out is NULL");
        *out = nullptr;
        if (num_classes < 3) return fail(nullptr, HCTR_ERR_ARG, "num_classes must be >= 3 (blank + chars + unknown)");
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev == 0)
            return fail(nullptr, HCTR_ERR_HIP, "no HIP device available (%s): the hctr engine has no CPU fallback",
                        hipGetErrorString(e));
        if (device < 0 || device >= ndev) return fail(nullptr, HCTR_ERR_ARG, "device %d out of range [0,%d)", device, ndev);
        e = hipSetDevice(device);
        if (e != hipSuccess) return fail(nullptr, HCTR_ERR_HIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
        hctr_ctx* c = new hctr_ctx();
        c->device = device;
        c->num_classes = num_classes;
        c->cpad = (num_classes + 255) / 256 * 256;
        e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete c;
            return fail(nullptr, HCTR_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
        }
        if (const char* bt = getenv("HCTR_BIG_TILES")) c->big_tiles = atoi(bt) != 0;
        if (const char* hm = getenv("HCTR_HALO")) c->halo_mode = atoi(hm);
        if (const char* pr = getenv("HCTR_PRECISION")) {
            const std::string m(pr);
            c->mode = m == "f16x3" ? 1 : (m == "auto" ? 2 : 0);
            c->split = c->mode == 1;
        }
        if (const char* fs = getenv("HCTR_FUSE_SE")) c->fuse_se = atoi(fs) != 0;
        if (const char* fa = getenv("HCTR_FUSE_ARGMAX")) c->fuse_argmax = atoi(fa) != 0;
        if (const char* fd = getenv("HCTR_FUSE_DS")) c->fuse_ds = atoi(fd) != 0;
        if (const char* fb = getenv("HCTR_FUSE_BEAM")) c->fuse_beam = atoi(fb) != 0;
        if (const char* fs2 = getenv("HCTR_FUSE_STEM")) c->fuse_stem = atoi(fs2) != 0;
        if (const char* ps = getenv("HCTR_PERSIST")) c->persist_dynamic = atoi(ps) == 2;
        if (const char* xm = getenv("HCTR_X3_MASK")) c->x3_mask = atoi(xm) & 31;
        if (const char* wa = getenv("HCTR_WS_ALIAS")) c->ws_alias = atoi(wa) != 0 ? 1 : 0;
        if (const char* wd = getenv("HCTR_WS_DEDICATED_MAX_GB")) {
            const double g = atof(wd);
            if (g >= 0) c->ws_dedicated_max = (size_t)(g * 1073741824.0);
        }
        if (const char* mc = getenv("HCTR_MAX_COLS")) {
            const long long v = atoll(mc);
            if (v > 0) c->max_cols = v;
        }
        *out = c;
        return HCTR_OK;
    });
}

void hctr_destroy(hctr_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->arena) (void)hipFree(c->arena);
    if (c->pin) (void)hipHostFree(c->pin);
    free_pool(c->wallocs);
    free_pool(c->beam_allocs);
    if (c->ctc_buf) (void)hipFree(c->ctc_buf);
    if (c->lm_slots) (void)hipFree(c->lm_slots);
    if (c->lm_words) (void)hipFree(c->lm_words);
    if (c->lex_dev) (void)hipFree(c->lex_dev);
    if (c->pat_dev) (void)hipFree(c->pat_dev);
    if (c->words_dev) (void)hipFree(c->words_dev);
    if (c->stamp_buf) (void)hipFree(c->stamp_buf);
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* hctr_last_error(const hctr_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int hctr_load_tensor(hctr_ctx* c, const char* key, const void* host_ptr, const int64_t* shape, int ndim, int dtype) {
    return guard(c, [&]() -> int {
        if (!c) return HCTR_ERR_ARG;
        if (!key || (!host_ptr && ndim > 0) || ndim < 0 || ndim > 8) return fail(c, HCTR_ERR_ARG, "bad tensor arguments");
        if (c->finalized) return fail(c, HCTR_ERR_STATE, "weights already finalized");
        const std::string k(key);
        if (dtype == HCTR_I64) {       // num_batches_tracked: accepted, unused in eval mode
            if (k.size() < 19 || k.compare(k.size() - 19, 19, "num_batches_tracked") != 0)
                return fail(c, HCTR_ERR_KEY, "Unexpected key(s) in state_dict: \"%s\" (int64)", key);
            return HCTR_OK;
        }
        if (dtype != HCTR_F32) return fail(c, HCTR_ERR_ARG, "tensor %s: only float32 parameters are supported", key);
        HostTensor t;
        int64_t n = 1;
        for (int i = 0; i < ndim; ++i) {
            if (shape[i] < 0) return fail(c, HCTR_ERR_ARG, "negative dimension");
            t.shape.push_back(shape[i]);
            n *= shape[i];
        }
        t.data.assign((const float*)host_ptr, (const float*)host_ptr + n);
        c->host[k] = std::move(t);
        return HCTR_OK;
    });
}

int hctr_finalize_weights(hctr_ctx* c) {
    return guard(c, [&]() -> int {
        if (!c) return HCTR_ERR_ARG;
        if (c->finalized) return fail(c, HCTR_ERR_STATE, "weights already finalized");
        HIP_TRY(c, hipSetDevice(c->device));
        // the f16 set for modes 0 and 2, the f16x3 set for modes 1 and 2 (build_* read c->split for the row layout)
        auto build_set = [&](bool split) -> int {
            c->split = split;
            WeightSet& ws = c->wset[split ? 1 : 0];
            TRY(build_stem(c, ws));
            TRY(build_conv(c, "cnn.conv0_2", "cnn.bn0_2", 64, 64, 3, true, 64, &ws.conv0_2));
            int inpl = 64;
            for (int s = 0; s < 4; ++s) {
                const int planes = kStagePlanes[s];
                ws.blocks[s].assign(kStageBlocks[s], BlockW());
                for (int i = 0; i < kStageBlocks[s]; ++i) {
                    BlockW& bw = ws.blocks[s][i];
                    const std::string p = "cnn.block" + std::to_string(s + 1) + "." + std::to_string(i);
                    if (i == 0 && inpl != planes) {
                        bw.has_ds = true;
                        TRY(build_conv(c, p + ".downsample.0", p + ".downsample.1", inpl, planes, 1, false, 128, &bw.ds));
                    }
                    TRY(build_conv(c, p + ".conv1", p + ".bn1", inpl, planes, 3, true, 128, &bw.conv1));
                    TRY(build_conv(c, p + ".conv2", p + ".bn2", planes, planes, 3, true, 128, &bw.conv2));
                    TRY(build_se(c, p + ".se", planes, &bw.se));
                    inpl = planes;
                }
                const std::string k = "cnn.conv" + std::to_string(s + 1);
                TRY(build_conv(c, k, "cnn.bn" + std::to_string(s + 1), planes, planes, 3, true, 128, &ws.stage_conv[s]));
            }
            TRY(build_head(c, ws));
            ws.built = true;
            return HCTR_OK;
        };
        int rc = HCTR_OK;
        if (c->mode != 1) rc = build_set(false);
        if (rc == HCTR_OK && c->mode != 0) rc = build_set(true);
        c->split = c->mode == 1;
        TRY(rc);
        // strict load: no unexpected float keys (load_state_dict(strict=True), test.py:153)
        for (auto& kv : c->host)
            if (!kv.second.used)
                return fail(c, HCTR_ERR_KEY, "Unexpected key(s) in state_dict: \"%s\"", kv.first.c_str());
        c->host.clear();
        c->finalized = true;
        return HCTR_OK;
    });
}

int hctr_set_precision(hctr_ctx* c, int mode) {
    return guard(c, [&]() -> int {
        if (!c) return HCTR_ERR_ARG;
        if (mode < 0 || mode > 2) return fail(c, HCTR_ERR_ARG, "precision mode must be 0 (f16), 1 (f16x3) or 2 (guarded: f16, "
                                                                 "uncertain lines again in f16x3)");
        if (c->finalized) {
            // after the weights are resident the mode may still move between the modes whose weight set(s) exist
            // (a context finalized in mode 2 holds both sets and serves all three)
            const bool need0 = mode != 1, need1 = mode != 0;
            if ((need0 && !c->wset[0].built) || (need1 && !c->wset[1].built))
                return fail(c, HCTR_ERR_STATE, "precision mode %d needs a weight set this context did not build: choose it "
                                               "(or mode 2) before hctr_finalize_weights", mode);
        }
        c->mode = mode;
        c->split = mode == 1;
        return HCTR_OK;
    });
}

int hctr_set_guard(hctr_ctx* c, double rel, double abs_tol) {
    return guard(c, [&]() -> int {
        if (!c) return HCTR_ERR_ARG;
        if (!(rel >= 0.0) || !(abs_tol >= 0.0)) return fail(c, HCTR_ERR_ARG, "guard tolerances must be >= 0");
        c->guard_rel = rel;
        c->guard_abs = abs_tol;
        return HCTR_OK;
    });
}

int hctr_get_guard(hctr_ctx* c, double* rel, double* abs_tol) {
    return guard(c, [&]() -> int {
        if (!c) return HCTR_ERR_ARG;
        if (rel) *rel = c->guard_rel;
        if (abs_tol) *abs_tol = c->guard_abs;
        return HCTR_OK;
    });
}

int hctr_last_guard(hctr_ctx* c, int64_t* lines, int64_t* flagged, uint8_t* flags, float* min_margin, float* scale,
                    int64_t cap) {
    return guard(c, [&]() -> int {
        if (!c) return HCTR_ERR_ARG;
        const int64_t n = (int64_t)c->g_flag.size();
        int64_t nf = 0;
        for (uint8_t f : c->g_flag) nf += f ? 1 : 0;
        if (lines) *lines = n;
        if (flagged) *flagged = nf;
        const int64_t m = n < cap ? n : (cap < 0 ? 0 : cap);
        if (flags && m) memcpy(flags, c->g_flag.data(), (size_t)m);
        if (min_margin && m) memcpy(min_margin, c->g_margin.data(), (size_t)m * 4);
        if (scale && m) memcpy(scale, c->g_scale.data(), (size_t)m * 4);
        return HCTR_OK;
    });
}

int hctr_workspace_stats(hctr_ctx* c, int64_t* arena_bytes, int64_t* arena_allocations, int64_t* recarves) {
    if (!c) return HCTR_ERR_ARG;
    if (arena_bytes) *arena_bytes = (int64_t)c->arena_cap;
    if (arena_allocations) *arena_allocations = c->arena_reallocs;
    if (recarves) *recarves = c->ws_recarves;
    return HCTR_OK;
}

int hctr_lines_per_pass(hctr_ctx* c, int B, int W, int f16x3) {
    return guard(c, [&]() -> int {
        if (!c) return HCTR_ERR_ARG;
        if (B < 1 || W < 1) return fail(c, HCTR_ERR_ARG, "bad batch shape B=%d W=%d", B, W);
        return sub_batch(c, B, W, f16x3 != 0);
    });
}

int hctr_set_profiling(hctr_ctx* c, int enabled) {
    if (!c) return HCTR_ERR_ARG;
    c->profiling = enabled != 0;
    return HCTR_OK;
}

int hctr_last_profile(hctr_ctx* c, char* names_buf, int cap, float* ms, int max_n) {
    return guard(c, [&]() -> int {
        if (!c) return HCTR_ERR_ARG;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::string names;
        std::vector<std::string> order;
        int n = 0;
        for (auto& pe : c->prof) {
            float t = 0.f;
            HIP_TRY(c, hipEventElapsedTime(&t, pe.e0, pe.e1));
            size_t i = 0;
            while (i < order.size() && order[i] != pe.name) ++i;      // internal passes repeat the layer names
            if (i == order.size()) {
                if (n >= max_n) break;
                order.push_back(pe.name);
                ms[n++] = 0.f;
                names += pe.name;
                names += '\n';
            }
            ms[i] += t;
        }
        if (names_buf && cap > 0) {
            strncpy(names_buf, names.c_str(), (size_t)cap - 1);
            names_buf[cap - 1] = 0;
        }
        return n;
    });
}

int hctr_forward_logits(hctr_ctx* c, const void* img, int img_dtype, int img_on_device, const int32_t* widths,
                        int B, int W, float* out_wbc, int out_on_device) {
    return guard(c, [&]() -> int {
        TRY(check_forward_args(c, img, img_dtype, B, W));
        if (!out_wbc) return fail(c, HCTR_ERR_ARG, "out_wbc is NULL");
        if (B == 0) return HCTR_OK;
        HIP_TRY(c, hipSetDevice(c->device));
        const int C = c->num_classes;
        const Batch in{img, img_dtype, img_on_device, widths, B, W};
        float* dev_out = out_wbc;
        std::vector<void*> tmp;
        PoolGuard tmp_guard{tmp};
        return synced(c, [&]() -> int {
            if (!out_on_device) TRY(dev_alloc(c, tmp, &dev_out, (size_t)B * W * C, false));
            // one pass: the lines' rows of the [W][B][C] output (a re-run overwrites them in stream order)
            TRY(run_passes(c, in, PASS_OWN, [&](const Pass& p) -> int {
                TRY(forward_pass(c, in, p, HEAD_LOGITS));
                // [nb*W][cpad] -> out[t][line][C], one launch per run of consecutive lines
                return for_runs(p.lines, p.nb, [&](int i, int n) -> int {
                    HIP_TRY(c, launch_logits_to_wbc(c->ws.logits + (size_t)i * W * c->cpad, c->cpad, n, W, C, dev_out, B,
                                                    p.lines[i], c->stream));
                    return HCTR_OK;
                });
            }));
            if (!out_on_device)
                HIP_TRY(c, hipMemcpyAsync(out_wbc, dev_out, (size_t)B * W * C * 4, hipMemcpyDeviceToHost, c->stream));
            return HCTR_OK;
        }());
    });
}

int hctr_greedy(hctr_ctx* c, const void* img, int img_dtype, int img_on_device, const int32_t* widths, int B, int W,
                int32_t* labels, int32_t* lengths) {
    return guard(c, [&]() -> int {
        TRY(check_forward_args(c, img, img_dtype, B, W));
        if (!labels || !lengths) return fail(c, HCTR_ERR_ARG, "labels/lengths is NULL");
        if (B == 0) return HCTR_OK;
        HIP_TRY(c, hipSetDevice(c->device));
        const Batch in{img, img_dtype, img_on_device, widths, B, W};
        std::vector<int> redo;                     // the lines of the second sweep
        int rc = greedy_passes(c, in, labels, lengths, &redo, [](Prof&, const Pass&) { return HCTR_OK; });
        // every pass queued async copies into host buffers: also after a failure the stream is drained before
        // returning, so nothing is in flight into (or out of) caller memory. Only a guarded call that flagged nothing
        // comes back drained (run_passes).
        if (rc != HCTR_OK || c->mode != 2 || !redo.empty()) rc = synced(c, rc);
        TRY(rc);
        greedy_scatter(c, redo, W, labels, lengths);
        return HCTR_OK;
    });
}

int hctr_decode_greedy_logits(hctr_ctx* c, const float* logits_wbc, int on_device, int W, int B, int C,
                              int32_t* labels, int32_t* lengths) {
    return guard(c, [&]() -> int {
        if (!c) return HCTR_ERR_ARG;
        if (W < 0 || B < 0 || C < 2) return fail(c, HCTR_ERR_ARG, "bad logits shape W=%d B=%d C=%d", W, B, C);
        if ((int64_t)W * B == 0) return HCTR_OK;     // reference: zero-length lines produce no output (:85-86)
        if (!logits_wbc || !labels || !lengths) return fail(c, HCTR_ERR_ARG, "NULL pointer");
        HIP_TRY(c, hipSetDevice(c->device));
        prof_reset(c);
        std::vector<void*> tmp;
        PoolGuard tmp_guard{tmp};
        return synced(c, [&]() -> int {
            const float* dev = nullptr;
            int32_t *idx = nullptr, *dl = nullptr, *dn = nullptr;
            TRY(logits_on_device(c, tmp, logits_wbc, on_device, (size_t)W * B * C, &dev));
            TRY(dev_alloc(c, tmp, &idx, (size_t)W * B, false));
            TRY(dev_alloc(c, tmp, &dl, (size_t)W * B, false));
            TRY(dev_alloc(c, tmp, &dn, (size_t)B, false));
            // rows of the WBC tensor are r = t*B + b; the argmax kernel writes idx as [b][t]
            Prof pf(c);
            PROF_TRY(pf, "argmax_rows", launch_argmax_rows(dev, C, (int64_t)W * B, C, idx, B, W, c->stream));
            PROF_TRY(pf, "ctc_collapse", launch_ctc_collapse(idx, B, W, C, dl, dn, c->stream));
            HIP_TRY(c, hipMemcpyAsync(labels, dl, (size_t)W * B * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(lengths, dn, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
            return HCTR_OK;
        }());
    });
}

int hctr_beam_frontend(hctr_ctx* c, const void* img, int img_dtype, int img_on_device, const int32_t* widths,
                       const float* logits_wbc, int logits_on_device, int B, int W, int C, int k,
                       int want_candidates, int32_t* topk_idx, float* topk_logp, float* blank_logp,
                       int64_t* num_candidates) {
    return guard(c, [&]() -> int {
        if (!c) return HCTR_ERR_ARG;
        if (B < 0 || W < 0 || k < 1) return fail(c, HCTR_ERR_ARG, "bad shape B=%d W=%d k=%d", B, W, k);
        if (!topk_idx || !topk_logp || !blank_logp) return fail(c, HCTR_ERR_ARG, "NULL output pointer");
        c->cand_off.assign((size_t)W * B + 1, 0);
        c->cand_idx.clear();
        c->cand_logp.clear();
        if (num_candidates) *num_candidates = 0;
        if ((int64_t)B * W == 0) return HCTR_OK;
        HIP_TRY(c, hipSetDevice(c->device));
        const bool from_img = img != nullptr;
        if (from_img) {
            TRY(check_forward_args(c, img, img_dtype, B, W));
            if (C != c->num_classes) return fail(c, HCTR_ERR_ARG, "C=%d differs from the model's %d classes", C, c->num_classes);
        } else if (!logits_wbc) {
            return fail(c, HCTR_ERR_ARG, "neither img nor logits given");
        }
        if (k > C) return fail(c, HCTR_ERR_ARG, "k=%d exceeds C=%d", k, C);
        const double thresh = std::log(0.001);        // utils/ctc_codec.py:128
        const Source src = from_img ? image_source(c, img, img_dtype, img_on_device, widths, B, W)
                                    : logits_source(logits_wbc, logits_on_device, W, B, C);
        // candidate lists of one pass (lines in pass order); owner[line] = the pass whose lists are current for the line
        struct PassOut { std::vector<int> lines; std::vector<int64_t> loff; std::vector<int32_t> ci; std::vector<float> cl; };
        std::vector<PassOut> outs;
        std::vector<int> owner((size_t)B, -1);
        std::vector<int32_t> counts((size_t)W * B, 0);
        // one pass over the lines `lines[0..nb)`: forward (or the caller's logits), log-softmax + top-k (+ lists), results
        // scattered to the lines' (t, line) rows of the host outputs
        std::vector<void*>& pool = c->beam_allocs;
        auto run_pass = [&](const Pass& p) -> int {
            const int* lines = p.lines;
            const int nb = p.nb;
            const int64_t rows = (int64_t)nb * W;
            BeamLists L;
            TRY(beam_lists_pass(c, src, p, k, want_candidates != 0, thresh, &L));
            const bool fused = L.fused;
            const float* rowsrc = L.rowsrc;
            const int64_t ld = L.ld;
            int32_t *d_idx = L.idx, *d_cnt = L.cnt;
            float *d_lp = L.lp, *d_bl = L.bl, *d_st = L.st;
            // D2H through a pinned staging buffer (grown on demand): a pageable destination is copied in small staged pieces
            const size_t nk = (size_t)rows * k, need_pin = (2 * nk + 2 * (size_t)rows) * 4;
            if (c->pin_cap < need_pin) {
                HIP_TRY(c, hipStreamSynchronize(c->stream));
                if (c->pin) (void)hipHostFree(c->pin);
                c->pin = nullptr; c->pin_cap = 0;
                void* hp = nullptr;
                if (hipHostMalloc(&hp, need_pin + need_pin / 8, hipHostMallocDefault) != hipSuccess)
                    return fail(c, HCTR_ERR_NOMEM, "hipHostMalloc(%zu bytes) failed", need_pin);
                c->pin = (char*)hp; c->pin_cap = need_pin + need_pin / 8;
            }
            int32_t* p_idx = (int32_t*)c->pin;
            float* p_lp = (float*)(p_idx + nk);
            float* p_bl = p_lp + nk;
            int32_t* p_cnt = (int32_t*)(p_bl + rows);
            HIP_TRY(c, hipMemcpyAsync(p_idx, d_idx, nk * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(p_lp, d_lp, nk * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(p_bl, d_bl, (size_t)rows * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipMemcpyAsync(p_cnt, d_cnt, (size_t)rows * 4, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            const int32_t* h_idx_p = p_idx; const float* h_lp_p = p_lp; const float* h_bl_p = p_bl; const int32_t* h_cnt_p = p_cnt;
            for (int t = 0; t < W; ++t)
                for (int b = 0; b < nb; ++b) {
                    const size_t src = (size_t)t * nb + b, dst = (size_t)t * B + lines[b];
                    memcpy(topk_idx + dst * k, h_idx_p + src * k, (size_t)k * 4);
                    memcpy(topk_logp + dst * k, h_lp_p + src * k, (size_t)k * 4);
                    blank_logp[dst] = h_bl_p[src];
                    counts[dst] = h_cnt_p[src];
                }
            if (!want_candidates) return HCTR_OK;
            outs.emplace_back();
            PassOut& po = outs.back();
            po.lines.assign(lines, lines + nb);
            for (int b = 0; b < nb; ++b) owner[(size_t)lines[b]] = (int)outs.size() - 1;
            po.loff.resize(rows + 1);
            int64_t tot = 0;
            for (int64_t r = 0; r < rows; ++r) { po.loff[r] = tot; tot += h_cnt_p[r]; }
            po.loff[rows] = tot;
            po.ci.resize(tot); po.cl.resize(tot);
            int64_t* d_off = nullptr;
            int32_t* d_ci = nullptr;
            float* d_cl = nullptr;
            TRY(dev_alloc(c, pool, &d_off, (size_t)rows + 1, false));
            TRY(dev_alloc(c, pool, &d_ci, (size_t)std::max<int64_t>(tot, 1), false));
            TRY(dev_alloc(c, pool, &d_cl, (size_t)std::max<int64_t>(tot, 1), false));
            HIP_TRY(c, hipMemcpyAsync(d_off, po.loff.data(), (size_t)(rows + 1) * 8, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, fused ? launch_beam_candidates(c->ws.emit_cnt, c->ws.emit_list, kBeamCap, d_st, nb, W, thresh, d_off, 0,
                                                      d_ci, d_cl, c->stream)
                             : launch_row_candidates(rowsrc, ld, nb, W, C, thresh, d_st, d_off, 0, d_ci, d_cl, c->stream));
            if (tot) {
                HIP_TRY(c, hipMemcpyAsync(po.ci.data(), d_ci, (size_t)tot * 4, hipMemcpyDeviceToHost, c->stream));
                HIP_TRY(c, hipMemcpyAsync(po.cl.data(), d_cl, (size_t)tot * 4, hipMemcpyDeviceToHost, c->stream));
            }
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            return HCTR_OK;
        };
        // from images: the passes of the mode (lines with a column the f16 sweep cannot certify - same criterion as
        // hctr_greedy - once more in f16x3, their rows of every output replaced); caller logits: one pass, no forward
        int rc;
        if (from_img) {
            rc = run_passes(c, src.img, PASS_OWN, run_pass);
        } else {
            prof_reset(c);
            guard_clear(c);
            const std::vector<int> all = line_indices(B);
            rc = run_pass(Pass{all.data(), B, 0, B, false, nullptr});
        }
        rc = synced(c, rc);
        free_pool(pool);
        if (rc != HCTR_OK || !want_candidates) return rc;
        // merge the per-pass lists into one CSR in (t*B + b) order, held by the context until fetched
        int64_t tot = 0;
        for (int64_t r = 0; r < (int64_t)W * B; ++r) { c->cand_off[r] = tot; tot += counts[r]; }
        c->cand_off[(size_t)W * B] = tot;
        c->cand_idx.resize(tot); c->cand_logp.resize(tot);
        for (size_t pi = 0; pi < outs.size(); ++pi) {
            const PassOut& po = outs[pi];
            const int nb = (int)po.lines.size();
            for (int t = 0; t < W; ++t)
                for (int b = 0; b < nb; ++b) {
                    if (owner[(size_t)po.lines[(size_t)b]] != (int)pi) continue;      // a later (f16x3) pass re-did this line
                    const size_t src = (size_t)t * nb + b, dst = (size_t)t * B + po.lines[(size_t)b];
                    const int64_t n = po.loff[src + 1] - po.loff[src];
                    if (n) {
                        memcpy(c->cand_idx.data() + c->cand_off[dst], po.ci.data() + po.loff[src], (size_t)n * 4);
                        memcpy(c->cand_logp.data() + c->cand_off[dst], po.cl.data() + po.loff[src], (size_t)n * 4);
                    }
                }
        }
        if (num_candidates) *num_candidates = tot;
        return HCTR_OK;
    });
}

// The three N-best entry points, each with and without an n-gram model: `lm` (null or the three extra arguments of
// hctr_nbest_lm*) is all that tells the two apart. With lm->sweep they are the entry points of hctr_lm_sweep*: the same
// checks, lists and passes, the sweep's scratch and launches in place of the single search's. The caller's lists have a
// body of their own (nbest_topk_impl); caller logits and line images share nbest_call.
struct NbestLmArgs {
    const hctr_lm* lm;
    double lm_panelty;
    double* lm_score;
    const SweepArgs* sweep = nullptr;
};

static int nbest_topk_impl(hctr_ctx* c, const NbestLmArgs* lm, const int32_t* topk_idx, const float* topk_logp, int W, int B,
                           int C, int k, int beam, int nbest, double len_bonus, const int32_t* input_lengths,
                           const NbestOut& o) {
    return guard(c, [&]() -> int {
        TRY(check_logits_args(c, W, B, C, topk_idx && topk_logp));
        NbestCall n;
        TRY(nbest_prepare(c, B, W, C, k, beam, nbest, len_bonus, input_lengths, o, &n));
        if (lm) TRY(nbest_lm_prepare(c, &n, lm->lm, lm->lm_panelty, lm->lm_score));
        SweepCall sw;
        if (lm && lm->sweep) TRY(sweep_prepare(c, n, *lm->sweep, &sw));
        if (B == 0) return HCTR_OK;
        // the lists are the caller's: classes in [0, C) and distinct within a row, as the front end produces them
        const size_t rows = (size_t)W * B;
        for (size_t r = 0; r < rows; ++r) {
            const int32_t* row = topk_idx + r * k;
            for (int j = 0; j < k; ++j) {
                bool bad = row[j] < 0 || row[j] >= C;
                for (int i = 0; i < j && !bad; ++i) bad = row[i] == row[j];
                if (bad)
                    return fail(c, HCTR_ERR_ARG, "topk_idx row (t=%zu, b=%zu) entry %d: class %d outside [0,%d) or repeated",
                                r / B, r % B, j, row[j], C);
            }
        }
        HIP_TRY(c, hipSetDevice(c->device));
        prof_reset(c);
        std::vector<void*> tmp;
        PoolGuard tmp_guard{tmp};
        return sweep_finish(synced(c, [&]() -> int {
            int32_t* d_idx = nullptr;
            float* d_lp = nullptr;
            TRY(sw.on ? sweep_scratch(c, &n, &sw, B) : nbest_scratch(c, &n, B));
            TRY(dev_alloc(c, tmp, &d_idx, rows * k, false));
            TRY(dev_alloc(c, tmp, &d_lp, rows * k, false));
            HIP_TRY(c, hipMemcpyAsync(d_idx, topk_idx, rows * k * 4, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(d_lp, topk_logp, rows * k * 4, hipMemcpyHostToDevice, c->stream));
            return sw.on ? sweep_launch(c, n, sw, d_idx, d_lp, 0, B) : nbest_launch(c, n, d_idx, d_lp, 0, B);
        }()), sw);
    });
}

// hctr_nbest* / hctr_nbest_lm* / hctr_lm_sweep* on a source: inside each pass the search runs on the front end's lists
// where they lie; only its results go to the host
static int nbest_call(hctr_ctx* c, const NbestLmArgs* lm, const Source& src, int k, int beam, int nbest, double len_bonus,
                      const int32_t* input_lengths, const NbestOut& o) {
    NbestCall n;
    TRY(nbest_prepare(c, src.B, src.W, src.C, k, beam, nbest, len_bonus, input_lengths, o, &n));
    if (lm) TRY(nbest_lm_prepare(c, &n, lm->lm, lm->lm_panelty, lm->lm_score));
    SweepCall sw;
    if (lm && lm->sweep) TRY(sweep_prepare(c, n, *lm->sweep, &sw));
    if (src.B == 0) return HCTR_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const int rc = source_passes(c, src, [&](const Pass& p, std::vector<void*>&) -> int {
        if (p.first == 0) TRY(sw.on ? sweep_scratch(c, &n, &sw, p.nb) : nbest_scratch(c, &n, p.nb));
        BeamLists L;
        TRY(beam_lists_pass(c, src, p, k, false, std::log(0.001), &L));
        return sw.on ? sweep_launch(c, n, sw, L.idx, L.lp, p.first, p.nb) : nbest_launch(c, n, L.idx, L.lp, p.first, p.nb);
    });
    free_pool(c->beam_allocs);
    return sweep_finish(rc, sw);
}

static int nbest_logits_impl(hctr_ctx* c, const NbestLmArgs* lm, const float* logits_wbc, int on_device, int W, int B, int C,
                             int k, int beam, int nbest, double len_bonus, const int32_t* input_lengths,
                             const NbestOut& o) {
    return guard(c, [&]() -> int {
        TRY(check_logits_args(c, W, B, C, logits_wbc != nullptr));
        return nbest_call(c, lm, logits_source(logits_wbc, on_device, W, B, C), k, beam, nbest, len_bonus, input_lengths, o);
    });
}

static int nbest_images_impl(hctr_ctx* c, const NbestLmArgs* lm, const void* img, int img_dtype, int img_on_device,
                             const int32_t* widths, int B, int W, int k, int beam, int nbest, double len_bonus,
                             const int32_t* input_lengths, const NbestOut& o) {
    return guard(c, [&]() -> int {
        TRY(check_forward_args(c, img, img_dtype, B, W));
        return nbest_call(c, lm, image_source(c, img, img_dtype, img_on_device, widths, B, W), k, beam, nbest, len_bonus,
                          input_lengths, o);
    });
}

int hctr_nbest_topk(hctr_ctx* c, const int32_t* topk_idx, const float* topk_logp, int W, int B, int C, int k, int beam,
                    int nbest, double len_bonus, const int32_t* input_lengths, int32_t* labels, int32_t* lengths,
                    double* logp, double* score, int32_t* count) {
    return nbest_topk_impl(c, nullptr, topk_idx, topk_logp, W, B, C, k, beam, nbest, len_bonus, input_lengths,
                           NbestOut{labels, lengths, logp, score, count});
}

int hctr_nbest_logits(hctr_ctx* c, const float* logits_wbc, int on_device, int W, int B, int C, int k, int beam, int nbest,
                      double len_bonus, const int32_t* input_lengths, int32_t* labels, int32_t* lengths, double* logp,
                      double* score, int32_t* count) {
    return nbest_logits_impl(c, nullptr, logits_wbc, on_device, W, B, C, k, beam, nbest, len_bonus, input_lengths,
                             NbestOut{labels, lengths, logp, score, count});
}

int hctr_nbest(hctr_ctx* c, const void* img, int img_dtype, int img_on_device, const int32_t* widths, int B, int W, int k,
               int beam, int nbest, double len_bonus, const int32_t* input_lengths, int32_t* labels, int32_t* lengths,
               double* logp, double* score, int32_t* count) {
    return nbest_images_impl(c, nullptr, img, img_dtype, img_on_device, widths, B, W, k, beam, nbest, len_bonus,
                             input_lengths, NbestOut{labels, lengths, logp, score, count});
}

int hctr_nbest_lm_topk(hctr_ctx* c, const hctr_lm* lm, const int32_t* topk_idx, const float* topk_logp, int W, int B, int C,
                       int k, int beam, int nbest, double lm_panelty, double len_bonus, const int32_t* input_lengths,
                       int32_t* labels, int32_t* lengths, double* logp, double* score, int32_t* count, double* lm_score) {
    const NbestLmArgs a{lm, lm_panelty, lm_score};
    return nbest_topk_impl(c, &a, topk_idx, topk_logp, W, B, C, k, beam, nbest, len_bonus, input_lengths,
                           NbestOut{labels, lengths, logp, score, count});
}

int hctr_nbest_lm_logits(hctr_ctx* c, const hctr_lm* lm, const float* logits_wbc, int on_device, int W, int B, int C, int k,
                         int beam, int nbest, double lm_panelty, double len_bonus, const int32_t* input_lengths,
                         int32_t* labels, int32_t* lengths, double* logp, double* score, int32_t* count,
                         double* lm_score) {
    const NbestLmArgs a{lm, lm_panelty, lm_score};
    return nbest_logits_impl(c, &a, logits_wbc, on_device, W, B, C, k, beam, nbest, len_bonus, input_lengths,
                             NbestOut{labels, lengths, logp, score, count});
}

int hctr_nbest_lm(hctr_ctx* c, const hctr_lm* lm, const void* img, int img_dtype, int img_on_device, const int32_t* widths,
                  int B, int W, int k, int beam, int nbest, double lm_panelty, double len_bonus,
                  const int32_t* input_lengths, int32_t* labels, int32_t* lengths, double* logp, double* score,
                  int32_t* count, double* lm_score) {
    const NbestLmArgs a{lm, lm_panelty, lm_score};
    return nbest_images_impl(c, &a, img, img_dtype, img_on_device, widths, B, W, k, beam, nbest, len_bonus, input_lengths,
                             NbestOut{labels, lengths, logp, score, count});
}

#define SWEEP_TAIL_PARAMS                                                                                             \
    const double *lm_panelty, const double *len_bonus, int G, int chunk, const int32_t *input_lengths,               \
        const int32_t *targets, const int32_t *target_lengths, int32_t *edits, int32_t *hyp_lengths, uint8_t *empty, \
        int32_t *labels, double *logp, double *score, double *lm_score
#define SWEEP_TAIL_ARGS \
    SweepArgs { lm_panelty, len_bonus, G, chunk, targets, target_lengths, edits, hyp_lengths, empty, labels, logp, score, lm_score }

int hctr_lm_sweep_chunk(int lines, int W, int beam, int G) { return G < 1 ? 0 : sweep_chunk(lines, W, beam, G); }

int hctr_lm_sweep_topk(hctr_ctx* c, const hctr_lm* lm, const int32_t* topk_idx, const float* topk_logp, int W, int B, int C,
                       int k, int beam, SWEEP_TAIL_PARAMS) {
    const SweepArgs s = SWEEP_TAIL_ARGS;
    const NbestLmArgs a{lm, 0.0, nullptr, &s};
    return nbest_topk_impl(c, &a, topk_idx, topk_logp, W, B, C, k, beam, 1, 0.0, input_lengths, NbestOut{});
}

int hctr_lm_sweep_logits(hctr_ctx* c, const hctr_lm* lm, const float* logits_wbc, int on_device, int W, int B, int C, int k,
                         int beam, SWEEP_TAIL_PARAMS) {
    const SweepArgs s = SWEEP_TAIL_ARGS;
    const NbestLmArgs a{lm, 0.0, nullptr, &s};
    return nbest_logits_impl(c, &a, logits_wbc, on_device, W, B, C, k, beam, 1, 0.0, input_lengths, NbestOut{});
}

int hctr_lm_sweep(hctr_ctx* c, const hctr_lm* lm, const void* img, int img_dtype, int img_on_device, const int32_t* widths,
                  int B, int W, int k, int beam, SWEEP_TAIL_PARAMS) {
    const SweepArgs s = SWEEP_TAIL_ARGS;
    const NbestLmArgs a{lm, 0.0, nullptr, &s};
    return nbest_images_impl(c, &a, img, img_dtype, img_on_device, widths, B, W, k, beam, 1, 0.0, input_lengths, NbestOut{});
}
#undef SWEEP_TAIL_PARAMS
#undef SWEEP_TAIL_ARGS

int hctr_nbest_skip_lists(hctr_ctx* c, const hctr_lm* lm, const int32_t* top1_idx, const float* blank_logp,
                          const int64_t* cand_off, const int32_t* cand_idx, const float* cand_logp, int W, int B, int C,
                          int beam, int nbest, double lm_panelty, double len_bonus, const int32_t* input_lengths,
                          int32_t* labels, int32_t* lengths, double* logp, double* score, int32_t* count, double* lm_score,
                          int32_t* status, int32_t* ranked) {
    return guard(c, [&]() -> int {
        TRY(check_logits_args(c, W, B, C, top1_idx && blank_logp && cand_off));
        NbestCall n;
        TRY(nbest_prepare(c, B, W, C, 1, beam, nbest, len_bonus, input_lengths, NbestOut{labels, lengths, logp, score, count},
                          &n));
        TRY(nbest_skip_prepare(c, &n, lm, lm_panelty, lm_score, status, ranked));
        if (B == 0) return HCTR_OK;
        // the lists are the caller's: offsets that do not decrease, classes in [0, C) and strictly ascending within a row
        const size_t rows = (size_t)W * B;
        if (cand_off[0] < 0) return fail(c, HCTR_ERR_ARG, "cand_off[0]=%lld is negative", (long long)cand_off[0]);
        for (size_t r = 0; r < rows; ++r)
            if (cand_off[r + 1] < cand_off[r])
                return fail(c, HCTR_ERR_ARG, "cand_off decreases at row (t=%zu, b=%zu)", r / B, r % B);
        if (cand_off[rows] > cand_off[0] && (!cand_idx || !cand_logp)) return fail(c, HCTR_ERR_ARG, "NULL candidate lists");
        std::vector<int32_t> pci(rows * kBeamMaxK, 0), pcnt(rows);
        std::vector<float> pcl(rows * kBeamMaxK, 0.f);
        for (size_t r = 0; r < rows; ++r) {
            if (top1_idx[r] < 0 || top1_idx[r] >= C)
                return fail(c, HCTR_ERR_ARG, "top1_idx (t=%zu, b=%zu): class %d outside [0,%d)", r / B, r % B, top1_idx[r], C);
            const int64_t o = cand_off[r], m = cand_off[r + 1] - o;
            for (int64_t j = 0; j < m; ++j) {
                const int32_t cls = cand_idx[o + j];
                if (cls < 0 || cls >= C || (j > 0 && cls <= cand_idx[o + j - 1]))
                    return fail(c, HCTR_ERR_ARG, "cand_idx row (t=%zu, b=%zu) entry %lld: class %d outside [0,%d) or not "
                                "above the one before it", r / B, r % B, (long long)j, cls, C);
                if (j < kBeamMaxK) { pci[r * kBeamMaxK + j] = cls; pcl[r * kBeamMaxK + j] = cand_logp[o + j]; }
            }
            pcnt[r] = (int32_t)std::min<int64_t>(m, INT32_MAX);
        }
        HIP_TRY(c, hipSetDevice(c->device));
        prof_reset(c);
        std::vector<void*> tmp;
        PoolGuard tmp_guard{tmp};
        return synced(c, [&]() -> int {
            int32_t *d_top1 = nullptr, *d_cc = nullptr, *d_ci = nullptr;
            float *d_bl = nullptr, *d_cl = nullptr;
            TRY(nbest_scratch(c, &n, B));
            TRY(dev_alloc(c, tmp, &d_top1, rows, false));
            TRY(dev_alloc(c, tmp, &d_bl, rows, false));
            TRY(dev_alloc(c, tmp, &d_cc, rows, false));
            TRY(dev_alloc(c, tmp, &d_ci, rows * kBeamMaxK, false));
            TRY(dev_alloc(c, tmp, &d_cl, rows * kBeamMaxK, false));
            HIP_TRY(c, hipMemcpyAsync(d_top1, top1_idx, rows * 4, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(d_bl, blank_logp, rows * 4, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(d_cc, pcnt.data(), rows * 4, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(d_ci, pci.data(), rows * kBeamMaxK * 4, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(d_cl, pcl.data(), rows * kBeamMaxK * 4, hipMemcpyHostToDevice, c->stream));
            return skip_launch(c, n, d_top1, 1, d_bl, d_cc, d_ci, d_cl, 0, B);
        }());
    });
}

// hctr_nbest_skip / hctr_nbest_skip_logits on a source: inside each pass the front end's lists stay where they lie, the
// candidate counts included
static int nbest_skip_call(hctr_ctx* c, const Source& src, const hctr_lm* lm, int beam, int nbest, double lm_panelty,
                           double len_bonus, const int32_t* input_lengths, const NbestOut& o, double* lm_score,
                           int32_t* status, int32_t* ranked) {
    NbestCall n;
    TRY(nbest_prepare(c, src.B, src.W, src.C, 1, beam, nbest, len_bonus, input_lengths, o, &n));
    TRY(nbest_skip_prepare(c, &n, lm, lm_panelty, lm_score, status, ranked));
    if (src.B == 0) return HCTR_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const int rc = source_passes(c, src, [&](const Pass& p, std::vector<void*>&) -> int {
        if (p.first == 0) TRY(nbest_scratch(c, &n, p.nb));
        BeamLists L;
        TRY(beam_lists_pass(c, src, p, 1, true, std::log(0.001), &L));
        return skip_on_lists(c, n, L, p.first, p.nb);
    });
    free_pool(c->beam_allocs);
    return rc;
}

int hctr_nbest_skip_logits(hctr_ctx* c, const hctr_lm* lm, const float* logits_wbc, int on_device, int W, int B, int C,
                           int beam, int nbest, double lm_panelty, double len_bonus, const int32_t* input_lengths,
                           int32_t* labels, int32_t* lengths, double* logp, double* score, int32_t* count, double* lm_score,
                           int32_t* status, int32_t* ranked) {
    return guard(c, [&]() -> int {
        TRY(check_logits_args(c, W, B, C, logits_wbc != nullptr));
        return nbest_skip_call(c, logits_source(logits_wbc, on_device, W, B, C), lm, beam, nbest, lm_panelty, len_bonus,
                               input_lengths, NbestOut{labels, lengths, logp, score, count}, lm_score, status, ranked);
    });
}

int hctr_nbest_skip(hctr_ctx* c, const hctr_lm* lm, const void* img, int img_dtype, int img_on_device, const int32_t* widths,
                    int B, int W, int beam, int nbest, double lm_panelty, double len_bonus, const int32_t* input_lengths,
                    int32_t* labels, int32_t* lengths, double* logp, double* score, int32_t* count, double* lm_score,
                    int32_t* status, int32_t* ranked) {
    return guard(c, [&]() -> int {
        TRY(check_forward_args(c, img, img_dtype, B, W));
        return nbest_skip_call(c, image_source(c, img, img_dtype, img_on_device, widths, B, W), lm, beam, nbest, lm_panelty,
                               len_bonus, input_lengths, NbestOut{labels, lengths, logp, score, count}, lm_score, status,
                               ranked);
    });
}

int hctr_ctc_loss(hctr_ctx* c, const void* img, int img_dtype, int img_on_device, const int32_t* widths, int B, int W,
                  const int32_t* targets, const int32_t* target_lengths, const int32_t* input_lengths, float* nll) {
    return guard(c, [&]() -> int {
        TRY(check_forward_args(c, img, img_dtype, B, W));
        if (B > 0 && !nll) return fail(c, HCTR_ERR_ARG, "nll is NULL");
        return ctc_loss_call(c, image_source(c, img, img_dtype, img_on_device, widths, B, W), targets, target_lengths,
                             input_lengths, nll);
    });
}

int hctr_ctc_loss_logits(hctr_ctx* c, const float* logits_wbc, int on_device, int W, int B, int C, const int32_t* targets,
                         const int32_t* target_lengths, const int32_t* input_lengths, float* nll) {
    return guard(c, [&]() -> int {
        TRY(check_logits_args(c, W, B, C, logits_wbc && nll));
        return ctc_loss_call(c, logits_source(logits_wbc, on_device, W, B, C), targets, target_lengths, input_lengths, nll);
    });
}

int hctr_ctc_loss_logits_grad(hctr_ctx* c, const float* logits_wbc, int on_device, int W, int B, int C,
                              const int32_t* targets, const int32_t* target_lengths, const int32_t* input_lengths,
                              const float* line_weight, float* nll, float* grad_wbc, int grad_on_device) {
    return guard(c, [&]() -> int {
        TRY(check_logits_args(c, W, B, C, logits_wbc && grad_wbc));
        if (B == 0) return HCTR_OK;
        if ((const float*)grad_wbc == logits_wbc) return fail(c, HCTR_ERR_ARG, "grad_wbc aliases the logits");
        HIP_TRY(c, hipSetDevice(c->device));
        CtcHost h;
        TRY(ctc_prepare(c, B, W, C, targets, target_lengths, input_lengths, &h));
        prof_reset(c);
        // host side of the gradient's tables: where each line's alpha rows start, and its target positions grouped by
        // emission slot (a counting sort of the slot table ctc_prepare made)
        const CtcLines hl = h.host();
        const size_t D1 = (size_t)h.D + 1;
        std::vector<int64_t> aoff((size_t)B);
        std::vector<int32_t> gtab((size_t)B * D1 + h.total(), 0);      // soff[B][D + 1] | pos[sum L]
        std::vector<float> wt((size_t)B, 1.f);
        int64_t ast_floats = 0;
        for (int b = 0; b < B; ++b) {
            aoff[(size_t)b] = ast_floats;
            ast_floats += (int64_t)hl.T[b] * (2 * (int64_t)hl.L[b] + 1);
            if (line_weight) wt[(size_t)b] = line_weight[b];
            if (!hl.T[b]) continue;
            int32_t* so = gtab.data() + (size_t)b * D1;
            int32_t* ps = gtab.data() + (size_t)B * D1 + hl.off[b];
            const int32_t* sl = hl.slot + hl.off[b];
            for (int j = 0; j < hl.L[b]; ++j) ++so[sl[j] + 1];
            so[0] = so[1] = 0;
            for (size_t j = 2; j < D1; ++j) so[j] += so[j - 1];     // so[j] = end of slot j - 1 = start of slot j
            std::vector<int32_t> fill(so, so + D1);
            for (int j = 0; j < hl.L[b]; ++j) ps[fill[(size_t)sl[j]]++] = j;
        }
        const size_t BW = (size_t)B * W;
        const size_t lse_b = align256(BW * 8), aoff_b = align256((size_t)B * 8), wt_b = align256((size_t)B * 4),
                     gtab_b = align256(gtab.size() * 4);
        std::vector<void*> tmp;
        PoolGuard tmp_guard{tmp};
        // the host tables above are pageable: their copies are staged before hipMemcpyAsync returns
        return synced(c, [&]() -> int {
            CtcLines m;
            float *d_nll = nullptr, *emis = nullptr, *dgrad = grad_wbc;
            char* extra = nullptr;
            TRY(ctc_scratch(c, h, BW * h.D, &m, &d_nll, &emis, lse_b + aoff_b + wt_b + gtab_b + (size_t)ast_floats * 4 + 16,
                            &extra));
            double* d_lse = (double*)extra;
            int64_t* d_aoff = (int64_t*)(extra + lse_b);
            float* d_wt = (float*)(extra + lse_b + aoff_b);
            int32_t* d_soff = (int32_t*)(extra + lse_b + aoff_b + wt_b);
            int32_t* d_pos = d_soff + (size_t)B * D1;
            float* d_ast = (float*)(extra + lse_b + aoff_b + wt_b + gtab_b);
            const size_t n = (size_t)W * B * C;
            const float* dev = nullptr;
            TRY(logits_on_device(c, tmp, logits_wbc, on_device, n, &dev));
            if (!grad_on_device) TRY(dev_alloc(c, tmp, &dgrad, n, false));
            HIP_TRY(c, hipMemcpyAsync(d_aoff, aoff.data(), (size_t)B * 8, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(d_wt, wt.data(), (size_t)B * 4, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(d_soff, gtab.data(), gtab.size() * 4, hipMemcpyHostToDevice, c->stream));
            Prof pf(c);
            // rows of the WBC tensor are r = t*B + b
            PROF_TRY(pf, "ctc_rowlse", launch_ctc_lse(dev, C, 1, B, C, m, 0, B, W, emis, d_lse, c->stream));
            PROF_TRY(pf, "ctc_alpha_store", launch_ctc_alpha(emis, m, 0, B, W, h.max_states, d_nll, d_aoff, d_ast,
                                                             c->stream));
            PROF_TRY(pf, "ctc_beta", launch_ctc_beta(emis, m, B, W, h.max_states, d_nll, d_aoff, d_ast, c->stream));
            PROF_TRY(pf, "ctc_grad_rows", launch_ctc_grad_rows(dev, C, B, W, m, d_lse, d_nll, d_wt, d_aoff, d_ast,
                                                               d_soff, d_pos, dgrad, c->stream));
            if (nll) HIP_TRY(c, hipMemcpyAsync(nll, d_nll, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
            if (!grad_on_device) HIP_TRY(c, hipMemcpyAsync(grad_wbc, dgrad, n * 4, hipMemcpyDeviceToHost, c->stream));
            return HCTR_OK;
        }());
    });
}

int hctr_ctc_align(hctr_ctx* c, const void* img, int img_dtype, int img_on_device, const int32_t* widths, int B, int W,
                   const int32_t* targets, const int32_t* target_lengths, const int32_t* input_lengths, int32_t* path,
                   int32_t* span_start, int32_t* span_end, float* span_logp, float* score) {
    return guard(c, [&]() -> int {
        TRY(check_forward_args(c, img, img_dtype, B, W));
        return ctc_align_call(c, image_source(c, img, img_dtype, img_on_device, widths, B, W), targets, target_lengths,
                              input_lengths, path, span_start, span_end, span_logp, score);
    });
}

int hctr_ctc_align_logits(hctr_ctx* c, const float* logits_wbc, int on_device, int W, int B, int C, const int32_t* targets,
                          const int32_t* target_lengths, const int32_t* input_lengths, int32_t* path, int32_t* span_start,
                          int32_t* span_end, float* span_logp, float* score) {
    return guard(c, [&]() -> int {
        TRY(check_logits_args(c, W, B, C, logits_wbc != nullptr));
        return ctc_align_call(c, logits_source(logits_wbc, on_device, W, B, C), targets, target_lengths, input_lengths, path,
                              span_start, span_end, span_logp, score);
    });
}

int hctr_spot_chunk_classes(int lines, int W) { return spot_class_cap(lines, W); }

int hctr_spot_automaton(const int32_t* query, int L, int32_t* classes, int32_t* num_classes, int32_t* delta,
                        int32_t* num_states, int32_t* in_ptr, int32_t* in_src, int32_t* in_slot, int edge_cap,
                        int32_t* num_edges, uint64_t* fall_mask) {
    return guard((hctr_ctx*)nullptr, [&]() -> int {
        if (!query) return fail(nullptr, HCTR_ERR_ARG, "query is NULL");
        if (L < 1 || L > kSpotMaxLen) return fail(nullptr, HCTR_ERR_ARG, "query length %d outside [1,%d]", L, kSpotMaxLen);
        for (int j = 0; j < L; ++j)
            if (query[j] < 1) return fail(nullptr, HCTR_ERR_ARG, "query id %d (position %d) is not a label (>= 1)", query[j], j);
        SpotAuto a;
        spot_automaton(query, L, &a);
        const int ne = (int)a.src.size();
        if ((in_src || in_slot) && edge_cap < ne)
            return fail(nullptr, HCTR_ERR_ARG, "edge_cap=%d is less than the automaton's %d edges", edge_cap, ne);
        if (classes) std::copy(a.cls.begin(), a.cls.end(), classes);
        if (num_classes) *num_classes = a.nq;
        if (delta) std::copy(a.delta.begin(), a.delta.end(), delta);
        if (num_states) *num_states = 2 * L;
        if (in_ptr) std::copy(a.ptr.begin(), a.ptr.end(), in_ptr);
        if (in_src) std::copy(a.src.begin(), a.src.end(), in_src);
        if (in_slot) std::copy(a.slot.begin(), a.slot.end(), in_slot);
        if (num_edges) *num_edges = ne;
        if (fall_mask) std::copy(a.mask.begin(), a.mask.end(), fall_mask);
        return HCTR_OK;
    });
}

int hctr_spot(hctr_ctx* c, const void* img, int img_dtype, int img_on_device, const int32_t* widths, int B, int W,
              const int32_t* queries, const int32_t* query_lengths, int Q, const int32_t* input_lengths,
              float* contain_logp, float* seg_logp, int32_t* seg_start, int32_t* seg_end) {
    return guard(c, [&]() -> int {
        TRY(check_forward_args(c, img, img_dtype, B, W));
        return spot_call(c, image_source(c, img, img_dtype, img_on_device, widths, B, W), queries, query_lengths, Q,
                         input_lengths, SpotOut{contain_logp, seg_logp, seg_start, seg_end});
    });
}

int hctr_spot_logits(hctr_ctx* c, const float* logits_wbc, int on_device, int W, int B, int C, const int32_t* queries,
                     const int32_t* query_lengths, int Q, const int32_t* input_lengths, float* contain_logp,
                     float* seg_logp, int32_t* seg_start, int32_t* seg_end) {
    return guard(c, [&]() -> int {
        TRY(check_logits_args(c, W, B, C, logits_wbc != nullptr));
        return spot_call(c, logits_source(logits_wbc, on_device, W, B, C), queries, query_lengths, Q, input_lengths,
                         SpotOut{contain_logp, seg_logp, seg_start, seg_end});
    });
}

int hctr_lexicon_chunk_classes(int lines, int W) { return lex_class_cap(lines, W); }

int hctr_lex_build(const int32_t* entries, const int32_t* entry_lengths, int N, int C, const float* log_prior,
                   int unit_nodes, hctr_lex** out) {
    if (out) *out = nullptr;
    return guard((hctr_ctx*)nullptr, [&]() -> int {
        if (!out) return fail(nullptr, HCTR_ERR_ARG, "hctr_lex_build: out is NULL");
        static std::atomic<uint64_t> serial{0};
        std::unique_ptr<hctr_lex> x(new hctr_lex());
        std::string msg;
        if (!lex_build(entries, entry_lengths, N, C, log_prior, unit_nodes, x.get(), &msg))
            return fail(nullptr, HCTR_ERR_ARG, "%s", msg.c_str());
        x->serial = ++serial;
        *out = x.release();
        return HCTR_OK;
    });
}

void hctr_lex_free(hctr_lex* lex) { delete lex; }

int hctr_lex_info(const hctr_lex* lex, int32_t* num_entries, int32_t* num_nodes, int32_t* num_units, int32_t* num_classes,
                  int32_t* max_len) {
    return guard((hctr_ctx*)nullptr, [&]() -> int {
        if (!lex) return fail(nullptr, HCTR_ERR_ARG, "lex is NULL");
        if (num_entries) *num_entries = lex->N;
        if (num_nodes) *num_nodes = lex->nodes();
        if (num_units) *num_units = lex->units();
        if (num_classes) *num_classes = (int32_t)lex->classes.size();
        if (max_len) *max_len = lex->max_len;
        return HCTR_OK;
    });
}

int hctr_lex_tables(const hctr_lex* lex, int32_t* parent, int32_t* label, int32_t* entry_node, int32_t* unit_off,
                    int32_t* class_off, int64_t* unit_total, int64_t* class_total, int32_t* unit_node, int32_t* unit_word,
                    uint8_t* unit_owned, int32_t* unit_kidx, int32_t* unit_class, int32_t* entry_ptr, int32_t* entry_list) {
    return guard((hctr_ctx*)nullptr, [&]() -> int {
        if (!lex) return fail(nullptr, HCTR_ERR_ARG, "lex is NULL");
        auto put = [](auto* dst, const auto& v) { if (dst) std::copy(v.begin(), v.end(), dst); };
        put(parent, lex->parent); put(label, lex->label); put(entry_node, lex->entry_node);
        put(unit_off, lex->uoff); put(class_off, lex->coff);
        if (unit_total) *unit_total = (int64_t)lex->gnode.size();
        if (class_total) *class_total = (int64_t)lex->ucls.size();
        put(unit_node, lex->gnode); put(unit_word, lex->node); put(unit_owned, lex->owned); put(unit_kidx, lex->kidx);
        put(unit_class, lex->ucls); put(entry_ptr, lex->eptr); put(entry_list, lex->elist);
        return HCTR_OK;
    });
}

int hctr_lexicon(hctr_ctx* c, const hctr_lex* lex, const void* img, int img_dtype, int img_on_device,
                 const int32_t* widths, int B, int W, const int32_t* input_lengths, int n, int32_t* top_entry,
                 float* top_logp, double* top_rank, double* log_total, int32_t* count, float* scores) {
    return guard(c, [&]() -> int {
        TRY(check_forward_args(c, img, img_dtype, B, W));
        return lex_call(c, image_source(c, img, img_dtype, img_on_device, widths, B, W), lex, input_lengths, n,
                        LexOut{top_entry, top_logp, top_rank, log_total, count, scores});
    });
}

int hctr_lexicon_logits(hctr_ctx* c, const hctr_lex* lex, const float* logits_wbc, int on_device, int W, int B, int C,
                        const int32_t* input_lengths, int n, int32_t* top_entry, float* top_logp, double* top_rank,
                        double* log_total, int32_t* count, float* scores) {
    return guard(c, [&]() -> int {
        TRY(check_logits_args(c, W, B, C, logits_wbc != nullptr));
        return lex_call(c, logits_source(logits_wbc, on_device, W, B, C), lex, input_lengths, n,
                        LexOut{top_entry, top_logp, top_rank, log_total, count, scores});
    });
}

int hctr_lex_word_tables(const hctr_lex* lex, float word_bonus, int32_t* num_nodes, int32_t* num_classes, int32_t* node,
                         int32_t* slot, int32_t* entry, float* weight, int32_t* classes) {
    return guard((hctr_ctx*)nullptr, [&]() -> int {
        if (!lex) return fail(nullptr, HCTR_ERR_ARG, "lex is NULL");
        WordTables t;
        std::string msg;
        if (!word_tables(*lex, word_bonus, &t, &msg)) return fail(nullptr, HCTR_ERR_ARG, "hctr_lex_word_tables: %s", msg.c_str());
        auto put = [](auto* dst, const auto& v) { if (dst) std::copy(v.begin(), v.end(), dst); };
        if (num_nodes) *num_nodes = t.nodes();
        if (num_classes) *num_classes = t.D();
        put(node, t.node); put(slot, t.slot); put(entry, t.entry); put(weight, t.weight); put(classes, t.cls);
        return HCTR_OK;
    });
}

int hctr_words(hctr_ctx* c, const hctr_lex* lex, const void* img, int img_dtype, int img_on_device, const int32_t* widths,
               int B, int W, const int32_t* input_lengths, float word_bonus, int max_words, float* score, int32_t* count,
               int32_t* words, int32_t* starts, int32_t* labels, int32_t* lengths, float* text_nll) {
    return guard(c, [&]() -> int {
        TRY(check_forward_args(c, img, img_dtype, B, W));
        return words_call(c, image_source(c, img, img_dtype, img_on_device, widths, B, W), lex, word_bonus, max_words,
                          input_lengths, WordsOut{score, count, words, starts, labels, lengths, text_nll});
    });
}

int hctr_words_logits(hctr_ctx* c, const hctr_lex* lex, const float* logits_wbc, int on_device, int W, int B, int C,
                      const int32_t* input_lengths, float word_bonus, int max_words, float* score, int32_t* count,
                      int32_t* words, int32_t* starts, int32_t* labels, int32_t* lengths, float* text_nll) {
    return guard(c, [&]() -> int {
        TRY(check_logits_args(c, W, B, C, logits_wbc != nullptr));
        return words_call(c, logits_source(logits_wbc, on_device, W, B, C), lex, word_bonus, max_words, input_lengths,
                          WordsOut{score, count, words, starts, labels, lengths, text_nll});
    });
}

int hctr_pattern_group_lines(int S, int D, int W) { return pat_group_lines(S, D, W); }

int hctr_pattern_instance(int S, int E, int viterbi, int weighted) {
    if (S < 1 || S > kPatMaxStates || E < 0 || E > kPatMaxEdges) return HCTR_ERR_ARG;
    return pattern_states_per_thread(S) | (pattern_edges_in_lds(S, E, viterbi != 0) ? 16 : 0) |
           (weighted && pattern_weights_in_lds(S, E, viterbi != 0) ? 32 : 0);
}

static uint64_t next_pat_serial() {          // one sequence for every kind: a context tells patterns apart by it
    static std::atomic<uint64_t> serial{0};
    return ++serial;
}

int hctr_pat_build(const int32_t* arcs_src, const int32_t* arcs_label, const int32_t* arcs_dst, int num_arcs,
                   const int32_t* finals, int num_finals, int num_states, int C, hctr_pat** out) {
    if (out) *out = nullptr;
    return guard((hctr_ctx*)nullptr, [&]() -> int {
        if (!out) return fail(nullptr, HCTR_ERR_ARG, "hctr_pat_build: out is NULL");
        std::unique_ptr<hctr_pat> x(new hctr_pat());
        std::string msg;
        if (!pat_build(arcs_src, arcs_label, arcs_dst, num_arcs, finals, num_finals, num_states, C, x.get(), &msg))
            return fail(nullptr, HCTR_ERR_ARG, "%s", msg.c_str());
        x->serial = next_pat_serial();
        *out = x.release();
        return HCTR_OK;
    });
}

int hctr_pat_build_weighted(const int32_t* arcs_src, const int32_t* arcs_label, const int32_t* arcs_dst,
                            const float* arcs_weight, int num_arcs, const int32_t* finals, const float* final_weight,
                            int num_finals, int num_states, int C, hctr_pat** out) {
    if (out) *out = nullptr;
    return guard((hctr_ctx*)nullptr, [&]() -> int {
        if (!out) return fail(nullptr, HCTR_ERR_ARG, "hctr_pat_build_weighted: out is NULL");
        std::unique_ptr<hctr_pat> x(new hctr_pat());
        std::string msg;
        if (!pat_build_weighted(arcs_src, arcs_label, arcs_dst, arcs_weight, num_arcs, finals, final_weight, num_finals,
                                num_states, C, x.get(), &msg))
            return fail(nullptr, HCTR_ERR_ARG, "%s", msg.c_str());
        x->serial = next_pat_serial();
        *out = x.release();
        return HCTR_OK;
    });
}

int hctr_pat_weights(const hctr_pat* pat, float* in_w, float* accept_w, float* start_w) {
    return guard((hctr_ctx*)nullptr, [&]() -> int {
        if (!pat) return fail(nullptr, HCTR_ERR_ARG, "pat is NULL");
        if (pat->kind != 2)
            return fail(nullptr, HCTR_ERR_ARG, "hctr_pat_weights: the pattern has no weights (hctr_pat_build_weighted builds one that has)");
        auto put = [](float* dst, const std::vector<float>& v) { if (dst) std::copy(v.begin(), v.end(), dst); };
        put(in_w, pat->in_w); put(accept_w, pat->accept_w); put(start_w, pat->start_w);
        return HCTR_OK;
    });
}

int hctr_pat_text_weight(const hctr_pat* pat, const int32_t* labels, int n, double* w) {
    return guard((hctr_ctx*)nullptr, [&]() -> int {
        if (!pat) return fail(nullptr, HCTR_ERR_ARG, "pat is NULL");
        if (pat->kind != 2)
            return fail(nullptr, HCTR_ERR_ARG, "hctr_pat_text_weight: the pattern has no weights (hctr_pat_build_weighted builds one that has)");
        if (n < 0 || (n > 0 && !labels) || !w) return fail(nullptr, HCTR_ERR_ARG, "hctr_pat_text_weight: labels / w is NULL or n < 0");
        *w = pat_text_weight(*pat, labels, n);
        return HCTR_OK;
    });
}

int hctr_pat_build_sets(const int32_t* arcs_src, const int32_t* arcs_set, const int32_t* arcs_dst, int num_arcs,
                        const int32_t* set_ptr, const int32_t* set_labels, int num_sets, const int32_t* finals,
                        int num_finals, int num_states, int C, hctr_pat** out) {
    if (out) *out = nullptr;
    return guard((hctr_ctx*)nullptr, [&]() -> int {
        if (!out) return fail(nullptr, HCTR_ERR_ARG, "hctr_pat_build_sets: out is NULL");
        std::unique_ptr<hctr_pat> x(new hctr_pat());
        std::string msg;
        if (!pat_build_sets(arcs_src, arcs_set, arcs_dst, num_arcs, set_ptr, set_labels, num_sets, finals, num_finals,
                            num_states, C, x.get(), &msg))
            return fail(nullptr, HCTR_ERR_ARG, "%s", msg.c_str());
        x->serial = next_pat_serial();
        *out = x.release();
        return HCTR_OK;
    });
}

int hctr_pat_kind(const hctr_pat* pat) { return pat ? pat->kind : HCTR_ERR_ARG; }

void hctr_pat_free(hctr_pat* pat) { delete pat; }

int hctr_pat_info(const hctr_pat* pat, int32_t* dfa_states, int32_t* ctc_states, int32_t* num_edges, int32_t* num_classes,
                  int32_t* max_in_degree) {
    return guard((hctr_ctx*)nullptr, [&]() -> int {
        if (!pat) return fail(nullptr, HCTR_ERR_ARG, "pat is NULL");
        if (dfa_states) *dfa_states = pat->nQ;
        if (ctc_states) *ctc_states = pat->S;
        if (num_edges) *num_edges = pat->edges();
        if (num_classes) *num_classes = (int32_t)pat->classes.size();
        if (max_in_degree) *max_in_degree = pat->max_deg;
        return HCTR_OK;
    });
}

int hctr_pat_tables(const hctr_pat* pat, int32_t* state_label, int32_t* state_slot, int32_t* in_ptr, uint16_t* in_src,
                    int32_t* classes, int32_t* num_accept, int32_t* accept, int32_t* num_start, int32_t* start) {
    return guard((hctr_ctx*)nullptr, [&]() -> int {
        if (!pat) return fail(nullptr, HCTR_ERR_ARG, "pat is NULL");
        if (pat->kind == 1)
            return fail(nullptr, HCTR_ERR_ARG, "hctr_pat_tables: a set pattern (hctr_pat_build_sets) has no edge list");
        auto put = [](auto* dst, const auto& v) { if (dst) std::copy(v.begin(), v.end(), dst); };
        put(state_label, pat->label); put(state_slot, pat->slot); put(in_ptr, pat->in_ptr); put(in_src, pat->in_src);
        put(classes, pat->classes); put(accept, pat->accept); put(start, pat->start);
        if (num_accept) *num_accept = (int32_t)pat->accept.size();
        if (num_start) *num_start = (int32_t)pat->start.size();
        return HCTR_OK;
    });
}

int hctr_pattern(hctr_ctx* c, const hctr_pat* pat, const void* img, int img_dtype, int img_on_device,
                 const int32_t* widths, int B, int W, const int32_t* input_lengths, float* logp, float* best_logp,
                 int32_t* path, int32_t* labels, int32_t* lengths, int32_t* span_start, int32_t* span_end,
                 float* char_logp, float* text_nll) {
    return guard(c, [&]() -> int {
        TRY(check_forward_args(c, img, img_dtype, B, W));
        return pat_call(c, image_source(c, img, img_dtype, img_on_device, widths, B, W), pat, input_lengths,
                        PatOut{logp, best_logp, path, labels, lengths, span_start, span_end, char_logp, text_nll});
    });
}

int hctr_pattern_logits(hctr_ctx* c, const hctr_pat* pat, const float* logits_wbc, int on_device, int W, int B, int C,
                        const int32_t* input_lengths, float* logp, float* best_logp, int32_t* path, int32_t* labels,
                        int32_t* lengths, int32_t* span_start, int32_t* span_end, float* char_logp, float* text_nll) {
    return guard(c, [&]() -> int {
        TRY(check_logits_args(c, W, B, C, logits_wbc != nullptr));
        return pat_call(c, logits_source(logits_wbc, on_device, W, B, C), pat, input_lengths,
                        PatOut{logp, best_logp, path, labels, lengths, span_start, span_end, char_logp, text_nll});
    });
}

int hctr_recognize(hctr_ctx* c, const void* img, int img_dtype, int img_on_device, const int32_t* widths, int B, int W,
                   int32_t* labels, int32_t* lengths, int32_t* span_start, int32_t* span_end, float* char_logp,
                   int32_t* alt_label, float* alt_logp, float* path_logp, float* text_nll) {
    return guard(c, [&]() -> int {
        TRY(check_forward_args(c, img, img_dtype, B, W));
        return rec_call(c, image_source(c, img, img_dtype, img_on_device, widths, B, W),
                        RecOut{labels, lengths, span_start, span_end, char_logp, alt_label, alt_logp, path_logp, text_nll});
    });
}

int hctr_recognize_logits(hctr_ctx* c, const float* logits_wbc, int on_device, int W, int B, int C, int32_t* labels,
                          int32_t* lengths, int32_t* span_start, int32_t* span_end, float* char_logp, int32_t* alt_label,
                          float* alt_logp, float* path_logp, float* text_nll) {
    return guard(c, [&]() -> int {
        TRY(check_logits_args(c, W, B, C, logits_wbc != nullptr));
        return rec_call(c, logits_source(logits_wbc, on_device, W, B, C),
                        RecOut{labels, lengths, span_start, span_end, char_logp, alt_label, alt_logp, path_logp, text_nll});
    });
}

int hctr_edit_distance(hctr_ctx* c, const int32_t* hyp, const int32_t* hyp_lengths, int hyp_stride, const int32_t* ref,
                       const int32_t* ref_lengths, int B, int32_t* edits, int32_t* counts, int32_t* ref_map,
                       int32_t* hyp_map) {
    return guard(c, [&]() -> int {
        if (!c) return HCTR_ERR_ARG;
        if (B < 0 || hyp_stride < 0) return fail(c, HCTR_ERR_ARG, "bad shape B=%d hyp_stride=%d", B, hyp_stride);
        if (B == 0) return HCTR_OK;
        if (!hyp || !hyp_lengths) return fail(c, HCTR_ERR_ARG, "hyp/hyp_lengths is NULL");
        for (int b = 0; b < B; ++b)
            if (hyp_lengths[b] < 0 || hyp_lengths[b] > hyp_stride)
                return fail(c, HCTR_ERR_ARG, "hyp_lengths[%d]=%d outside [0,%d]", b, hyp_lengths[b], hyp_stride);
        const EditOut out{edits, counts, ref_map, hyp_map};
        EditCall e;
        TRY(edit_prepare(c, B, hyp_stride, ref, ref_lengths, hyp_lengths, out.maps(), &e));
        HIP_TRY(c, hipSetDevice(c->device));
        prof_reset(c);
        return synced(c, [&]() -> int {
            const size_t hyp_b = align256((size_t)B * hyp_stride * 4);
            TRY(edit_scratch(c, &e, B, hyp_b + (size_t)B * 4));
            int32_t *d_hyp = (int32_t*)e.d_user, *d_hlen = (int32_t*)(e.d_user + hyp_b);
            if (hyp_stride)
                HIP_TRY(c, hipMemcpyAsync(d_hyp, hyp, (size_t)B * hyp_stride * 4, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(d_hlen, hyp_lengths, (size_t)B * 4, hipMemcpyHostToDevice, c->stream));
            const std::vector<int> lines = line_indices(B);
            Prof pf(c);
            TRY(edit_launch(c, pf, &e, lines.data(), nullptr, B, d_hyp, d_hlen));
            return edit_fetch(c, e, out);
        }());
    });
}

int hctr_evaluate(hctr_ctx* c, const void* img, int img_dtype, int img_on_device, const int32_t* widths, int B, int W,
                  const int32_t* targets, const int32_t* target_lengths, int32_t* labels, int32_t* lengths, int32_t* edits,
                  int32_t* counts, int32_t* ref_map, int32_t* hyp_map) {
    return guard(c, [&]() -> int {
        TRY(check_forward_args(c, img, img_dtype, B, W));
        if (B == 0) return HCTR_OK;
        if (labels && !lengths) return fail(c, HCTR_ERR_ARG, "labels without lengths");
        const EditOut out{edits, counts, ref_map, hyp_map};
        EditCall e;
        TRY(edit_prepare(c, B, W, targets, target_lengths, nullptr, out.maps(), &e));
        HIP_TRY(c, hipSetDevice(c->device));
        const Batch in{img, img_dtype, img_on_device, widths, B, W};
        std::vector<int> redo;
        bool reserved = false;
        // the edit kernels of a pass read the decoded labels where the collapse left them; a re-run pass names its lines
        // through line_of, and its results replace the first sweep's in the device arrays, which come back once
        int rc = greedy_passes(c, in, labels, lengths, &redo, [&](Prof& pf, const Pass& p) -> int {
            if (!reserved) {
                TRY(edit_scratch(c, &e, sub_batch(c, B, W, c->mode == 1), 0));
                reserved = true;
            }
            if (p.rerun && p.first == 0)
                HIP_TRY(c, hipMemcpyAsync(e.d_line_of, p.lines, (size_t)p.total * 4, hipMemcpyHostToDevice, c->stream));
            return edit_launch(c, pf, &e, p.lines, p.rerun ? e.d_line_of + p.first : nullptr, p.nb, c->ws.labels,
                               c->ws.lengths);
        });
        if (rc == HCTR_OK) rc = edit_fetch(c, e, out);
        TRY(synced(c, rc));
        greedy_scatter(c, redo, W, labels, lengths);
        return HCTR_OK;
    });
}

int hctr_evaluate_logits(hctr_ctx* c, const float* logits_wbc, int on_device, int W, int B, int C, const int32_t* targets,
                         const int32_t* target_lengths, int32_t* labels, int32_t* lengths, int32_t* edits, int32_t* counts,
                         int32_t* ref_map, int32_t* hyp_map) {
    return guard(c, [&]() -> int {
        TRY(check_logits_args(c, W, B, C, logits_wbc != nullptr));
        if (B == 0) return HCTR_OK;
        const EditOut out{edits, counts, ref_map, hyp_map};
        EditCall e;
        TRY(edit_prepare(c, B, W, targets, target_lengths, nullptr, out.maps(), &e));
        for (size_t j = 0; j < e.total; ++j)              // hctr_ctc_loss_logits' check of the ids
            if (targets[j] < 1 || targets[j] > C - 1)
                return fail(c, HCTR_ERR_ARG, "target id %d (position %zu) outside [1,%d]", targets[j], j, C - 1);
        HIP_TRY(c, hipSetDevice(c->device));
        prof_reset(c);
        std::vector<void*> tmp;
        PoolGuard tmp_guard{tmp};
        return synced(c, [&]() -> int {
            const float* dev = nullptr;
            const size_t col_b = align256((size_t)W * B * 4);
            TRY(edit_scratch(c, &e, B, 2 * col_b + (size_t)B * 4));
            int32_t *idx = (int32_t*)e.d_user, *dl = (int32_t*)(e.d_user + col_b), *dn = (int32_t*)(e.d_user + 2 * col_b);
            TRY(logits_on_device(c, tmp, logits_wbc, on_device, (size_t)W * B * C, &dev));
            Prof pf(c);
            // rows of the WBC tensor are r = t*B + b; the argmax kernel writes idx as [b][t]
            PROF_TRY(pf, "argmax_rows", launch_argmax_rows(dev, C, (int64_t)W * B, C, idx, B, W, c->stream));
            PROF_TRY(pf, "ctc_collapse", launch_ctc_collapse(idx, B, W, C, dl, dn, c->stream));
            if (labels) HIP_TRY(c, hipMemcpyAsync(labels, dl, (size_t)W * B * 4, hipMemcpyDeviceToHost, c->stream));
            if (lengths) HIP_TRY(c, hipMemcpyAsync(lengths, dn, (size_t)B * 4, hipMemcpyDeviceToHost, c->stream));
            const std::vector<int> lines = line_indices(B);
            TRY(edit_launch(c, pf, &e, lines.data(), nullptr, B, dl, dn));
            return edit_fetch(c, e, out);
        }());
    });
}

int hctr_beam_fetch_candidates(hctr_ctx* c, int64_t* cand_off, int32_t* cand_idx, float* cand_logp) {
    return guard(c, [&]() -> int {
        if (!c) return HCTR_ERR_ARG;
        if (c->cand_off.empty()) return fail(c, HCTR_ERR_STATE, "no candidate lists: call hctr_beam_frontend(want_candidates=1)");
        if (!cand_off) return fail(c, HCTR_ERR_ARG, "cand_off is NULL");
        memcpy(cand_off, c->cand_off.data(), c->cand_off.size() * 8);
        if (!c->cand_idx.empty()) {
            if (!cand_idx || !cand_logp) return fail(c, HCTR_ERR_ARG, "cand_idx/cand_logp is NULL");
            memcpy(cand_idx, c->cand_idx.data(), c->cand_idx.size() * 4);
            memcpy(cand_logp, c->cand_logp.data(), c->cand_logp.size() * 4);
        }
        return HCTR_OK;
    });
}

int hctr_log_softmax(hctr_ctx* c, const float* logits_wbc, int on_device, int W, int B, int C, float* out_host) {
    return guard(c, [&]() -> int {
        if (!c) return HCTR_ERR_ARG;
        if (W < 0 || B < 0 || C < 1) return fail(c, HCTR_ERR_ARG, "bad shape");
        const int64_t rows = (int64_t)W * B;
        if (rows == 0) return HCTR_OK;
        if (!logits_wbc || !out_host) return fail(c, HCTR_ERR_ARG, "NULL pointer");
        HIP_TRY(c, hipSetDevice(c->device));
        std::vector<void*> tmp;
        PoolGuard tmp_guard{tmp};
        return synced(c, [&]() -> int {
            const float* dev = nullptr;
            float* y = nullptr;
            TRY(logits_on_device(c, tmp, logits_wbc, on_device, (size_t)rows * C, &dev));
            TRY(dev_alloc(c, tmp, &y, (size_t)rows * C, false));
            HIP_TRY(c, launch_log_softmax_rows(dev, rows, C, y, c->stream));
            HIP_TRY(c, hipMemcpyAsync(out_host, y, (size_t)rows * C * 4, hipMemcpyDeviceToHost, c->stream));
            return HCTR_OK;
        }());
    });
}

int hctr_resize_lines(hctr_ctx* c, const uint8_t* packed_src, int64_t packed_bytes, const int64_t* offsets,
                      const int32_t* heights, const int32_t* widths, const int32_t* channels, int n, int out_height,
                      const int32_t* out_widths, int out_W, uint8_t* out, int out_on_device) {
    return guard(c, [&]() -> int {
        if (!c) return HCTR_ERR_ARG;
        if (n < 0 || out_height < 1 || out_W < 0 || packed_bytes < 0) return fail(c, HCTR_ERR_ARG, "bad shape");
        if (n == 0 || out_W == 0) return HCTR_OK;
        if (!packed_src || !offsets || !heights || !widths || !channels || !out_widths || !out)
            return fail(c, HCTR_ERR_ARG, "NULL pointer");
        if (n > 65535) return fail(c, HCTR_ERR_ARG, "at most 65535 images per call");
        std::vector<ResizeLine> lines((size_t)n);
        for (int i = 0; i < n; ++i) {
            const int ch = channels[i];
            if (ch != 1 && ch != 3 && ch != -3) return fail(c, HCTR_ERR_ARG, "image %d: channels must be 1, 3 (BGR) or -3 (RGB)", i);
            if (heights[i] < 1 || widths[i] < 1) return fail(c, HCTR_ERR_SHAPE, "image %d: empty source", i);
            // cv2.resize asserts !dsize.empty(): a line so narrow that int(128 * w / h) == 0 fails there too
            if (out_widths[i] < 1) return fail(c, HCTR_ERR_SHAPE, "image %d: destination width %d < 1", i, out_widths[i]);
            const int64_t bytes = (int64_t)heights[i] * widths[i] * (ch < 0 ? -ch : ch);
            if (offsets[i] < 0 || offsets[i] + bytes > packed_bytes)
                return fail(c, HCTR_ERR_ARG, "image %d: [%lld, +%lld) outside the packed buffer of %lld bytes", i,
                            (long long)offsets[i], (long long)bytes, (long long)packed_bytes);
            ResizeLine& L = lines[(size_t)i];
            L.src_off = offsets[i];
            L.sh = heights[i];
            L.sw = widths[i];
            L.ch = ch;
            L.dw = out_widths[i];
            // dispatch of cv::resize for INTER_AREA (oracle/resize_ref.py resize_area)
            L.inv_x = (double)L.dw / (double)L.sw;
            L.inv_y = (double)out_height / (double)L.sh;
            L.scale_x = 1.0 / L.inv_x;
            L.scale_y = 1.0 / L.inv_y;
            L.ix = (int)std::nearbyint(L.scale_x);
            L.iy = (int)std::nearbyint(L.scale_y);
            if (L.scale_x >= 1.0 && L.scale_y >= 1.0) {
                const bool fast = std::fabs(L.scale_x - L.ix) < DBL_EPSILON && std::fabs(L.scale_y - L.iy) < DBL_EPSILON;
                L.mode = fast ? 1 : 0;
            } else {
                L.mode = 2;
            }
        }
        HIP_TRY(c, hipSetDevice(c->device));
        std::vector<void*> tmp;
        PoolGuard tmp_guard{tmp};
        return synced(c, [&]() -> int {
            uint8_t *src = nullptr, *dst = out;
            ResizeLine* dl = nullptr;
            const size_t out_bytes = (size_t)n * out_height * out_W;
            TRY(dev_alloc(c, tmp, &src, (size_t)std::max<int64_t>(packed_bytes, 1), false));
            TRY(dev_alloc(c, tmp, &dl, (size_t)n, false));
            if (!out_on_device) TRY(dev_alloc(c, tmp, &dst, out_bytes, false));
            HIP_TRY(c, hipMemcpyAsync(src, packed_src, (size_t)packed_bytes, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipMemcpyAsync(dl, lines.data(), sizeof(ResizeLine) * (size_t)n, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, launch_resize_lines(src, dl, n, dst, out_height, out_W, c->stream));
            if (!out_on_device) HIP_TRY(c, hipMemcpyAsync(out, dst, out_bytes, hipMemcpyDeviceToHost, c->stream));
            return HCTR_OK;
        }());
    });
}

int64_t hctr_debug_stamps(hctr_ctx* c, const char* layer, uint64_t* out, int64_t cap_wgs) {
    return guard<int64_t>(c, [&]() -> int64_t {
        if (!c || cap_wgs < 0) return HCTR_ERR_ARG;
        if (hipSetDevice(c->device) != hipSuccess) return fail(c, HCTR_ERR_HIP, "hipSetDevice");
        if (layer) {                                  // arm: later forwards stamp this layer's workgroups
            if (c->stamp_buf) { (void)hipFree(c->stamp_buf); c->stamp_buf = nullptr; }
            c->stamp_layer = layer;
            c->stamp_cap = cap_wgs;
            c->stamp_n = 0;
            if (cap_wgs > 0 && hipMalloc((void**)&c->stamp_buf, (size_t)cap_wgs * 128) != hipSuccess)
                return fail(c, HCTR_ERR_NOMEM, "stamp buffer");
            return 0;
        }
        if (!out || !c->stamp_buf) return fail(c, HCTR_ERR_STATE, "stamping not armed");
        const int64_t n = std::min(c->stamp_n, cap_wgs);
        if (hipMemcpy(out, c->stamp_buf, (size_t)n * 128, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, HCTR_ERR_HIP, "stamp copy");
        return n;
    });
}

int64_t hctr_debug_activation(hctr_ctx* c, const char* name, float* out, int64_t cap, int* Cout, int* Hout) {
    return guard<int64_t>(c, [&]() -> int64_t {
        if (!c || !name) return HCTR_ERR_ARG;
        const Workspace& ws = c->ws;
        if (ws.B == 0) return fail(c, HCTR_ERR_STATE, "no forward has run");
        const half_t* p = nullptr;
        int H = 0, C = 0;
        bool head = false;
        const std::string n(name);
        if (n == "conv0_1") {
            if (!ws.s0) return fail(c, HCTR_ERR_STATE, "conv0_1 is fused into conv0_2 (no buffer): use HCTR_FUSE_STEM=0");
            p = ws.s0; H = 128; C = 64;
        }
        else if (n == "stage0") { p = ws.x[1]; H = 64; C = 64; }
        else if (n == "stage1") { p = ws.x[2]; H = 32; C = 128; }
        else if (n == "stage2") { p = ws.x[3]; H = 16; C = 256; }
        else if (n == "stage3") { p = ws.x[4]; H = 8; C = 512; }
        else if (n == "stage4") { p = ws.headin; H = 4; C = 512; head = true; }
        else if (n.size() == 4 && n[0] == 'p' && n[2] == '.' && n[1] >= '1' && n[1] <= '4' && n[3] >= '0' && n[3] <= '2') {
            // raw rotating block buffer i of stage s ("p<s>.<i>"): what it holds depends on the block count
            const int st = n[1] - '0', bi = n[3] - '0';
            p = ws.p[st][bi]; H = kStageH[st]; C = kStagePlanes[st - 1];
            if (!p) return fail(c, HCTR_ERR_ARG, "buffer %s not allocated", name);
        }
        else return fail(c, HCTR_ERR_ARG, "unknown activation '%s'", name);
        if (ws.aliased && !(n == "stage3" || n == "stage4" || (n.size() == 4 && n[0] == 'p' && n[1] == '4')))
            return fail(c, HCTR_ERR_STATE, "activation '%s' was overwritten by a later stage: the stages share their buffers "
                        "in this workspace layout (HCTR_WS_ALIAS=0 keeps every stage's own)", name);
        const int64_t total = (int64_t)ws.B * C * H * ws.W;
        if (Cout) *Cout = C;
        if (Hout) *Hout = H;
        if (!out || cap < total) return total;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        const int m = ws.split ? 3 : 1;                // [hi | lo | hi] planes in f16x3 mode: report hi + lo
        const int64_t elems = head ? (int64_t)ws.B * ws.W * kFeat * m : act_elems(ws.B, H, ws.Wa, C * m);
        std::vector<half_t> host((size_t)elems);
        HIP_TRY(c, hipMemcpy(host.data(), p, (size_t)elems * sizeof(half_t), hipMemcpyDeviceToHost));
        for (int b = 0; b < ws.B; ++b)
            for (int ch = 0; ch < C; ++ch)
                for (int h = 0; h < H; ++h)
                    for (int w = 0; w < ws.W; ++w) {
                        const int64_t src = head ? (((int64_t)b * ws.W + w) * 4 + h) * (512 * m) + ch
                                                 : (((int64_t)b * (H + 2) + h + 1) * ws.Wa + w + 1) * (C * m) + ch;
                        float v = (float)host[(size_t)src];
                        if (m == 3) v += (float)host[(size_t)src + C];
                        out[(((int64_t)b * C + ch) * H + h) * ws.W + w] = v;
                    }
        return total;
    });
}

int hctr_debug_se(hctr_ctx* c, const char* name, float* mean_out, float* scale_out, int64_t cap) {
    return guard<int>(c, [&]() -> int {
        if (!c || !name) return HCTR_ERR_ARG;
        const Workspace& ws = c->ws;
        if (ws.B == 0) return fail(c, HCTR_ERR_STATE, "no forward has run");
        int st = 0, bi = 0, slot = 0;
        char tail = 0;
        if (sscanf(name, "block%d.%d%c", &st, &bi, &tail) != 2 || st < 1 || st > 4 || bi < 0 ||
            bi >= (int)c->wts().blocks[st - 1].size())
            return fail(c, HCTR_ERR_ARG, "unknown block '%s'", name);
        for (int s = 1; s < st; ++s) slot += (int)c->wts().blocks[s - 1].size();
        slot += bi;
        if (slot >= kSeBlocks) return fail(c, HCTR_ERR_STATE, "more blocks than SE slots");
        // (f16x3 passes always take the fused form, see run_block)
        if (!c->fuse_se && !ws.split)
            return fail(c, HCTR_ERR_STATE, "the unfused SE path (HCTR_FUSE_SE=0) computes no channel means ahead of conv2");
        const int C = kStagePlanes[st - 1];
        const int64_t total = (int64_t)ws.B * C;
        if (cap < total || (!mean_out && !scale_out))
            return fail(c, HCTR_ERR_ARG, "hctr_debug_se(%s): room for %lld values needed", name, (long long)total);
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        const size_t off = (size_t)slot * ws.B * 512;
        if (mean_out)
            HIP_TRY(c, hipMemcpy(mean_out, ws.se_mean + off, (size_t)total * sizeof(float), hipMemcpyDeviceToHost));
        if (scale_out)
            HIP_TRY(c, hipMemcpy(scale_out, ws.se_scale + off, (size_t)total * sizeof(float), hipMemcpyDeviceToHost));
        return HCTR_OK;
    });
}

}  // extern "C"
