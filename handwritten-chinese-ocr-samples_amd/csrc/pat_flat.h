// The pattern object behind the C ABI's hctr_pat (include/hctr_hip.h): a deterministic finite automaton over labels,
// lifted to CTC, as the flat tables pattern_kernel is given. Host only and header only: engine.cpp builds it
// (hctr_pat_build), tests read it back (hctr_pat_tables), and a stand-alone program can include it without the GPU
// runtime.
//
// DFA: states 0..nQ-1 (0 = the start), arcs (src, label, dst) with at most one arc per (src, label), final states.
// States that are not both reachable from state 0 and able to reach a final state are pruned with their arcs; the
// survivors keep their relative order.
// CTC states: beta_q = q, one per DFA state (the last column was a blank, or nothing was read, in DFA state q); then one
// eps_(q,c) per distinct (destination q, label c) among the arcs, in ascending (q, c) (the last column emitted c and
// the text read so far leads to q). Arcs (p,c,q) and (p',c,q) share eps_(q,c): their futures are the same.
// In-edges, sorted by source ascending: beta_q <- beta_q, every eps_(q,.);  eps_(q,c) <- itself, beta_p for every arc
// (p,c,q), and for each such p every eps_(p,c') with c' != c.
// Weighted (kind 2, pat_build_weighted): the same automaton and tables with one float per arc and per final state. The
// weight of arc (p,c,q) sits on every in-edge of eps_(q,c) whose source is beta_p or an eps_(p,.) - every source belongs
// to one DFA state, so one edge has one weight - and, for p = 0, on eps_(q,c)'s place in the start list; self edges and
// the in-edges of beta states weigh 0; an accepting state carries the final weight of its DFA state.
#pragma once
#include <cmath>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

namespace hctr {

constexpr int kPatMaxStates = 8192;              // HCTR_PAT_MAX_STATES
constexpr int kPatMaxEdges = 262144;             // HCTR_PAT_MAX_EDGES
constexpr int kPatSetMaxStates = 65535;          // HCTR_PATSET_MAX_STATES (backpointers are uint16; 65535 = "no state")
constexpr int kPatSetMaxDfaStates = 4096;        // HCTR_PATSET_MAX_DFA_STATES (the block totals live in LDS)
constexpr int kPatSetMaxInArcs = 1 << 20;        // HCTR_PATSET_MAX_INARCS
constexpr uint32_t kPatSetNone = 0xFFFFu;        // an in-arc whose source block has no state of the label

}  // namespace hctr

struct hctr_pat {
    int C = 0, nQ = 0, S = 0, max_deg = 0;
    int kind = 0;                                // 0 = explicit edges (pat_build), 1 = label-set arcs (pat_build_sets),
                                                 // 2 = explicit edges with weights (pat_build_weighted)
    uint64_t serial = 0;
    std::vector<int32_t> classes;                // the distinct labels, ascending
    std::vector<int32_t> label, slot;            // [S] label (0 = blank); its place in (0, classes..)
    std::vector<int32_t> in_ptr;                 // [S + 1]
    std::vector<uint16_t> in_src;                // [E] a state's sources, ascending
    std::vector<int32_t> accept;                 // the accepting states, ascending
    std::vector<int32_t> start;                  // beta_0, then the eps states of the arcs that leave state 0, ascending
    // kind 1 only (label, slot and classes as above; in_ptr, in_src, accept and start stay empty). The block of DFA
    // state p is beta_p = p and its eps states nQ + [blk_ptr[p], blk_ptr[p + 1]), in ascending label.
    std::vector<int32_t> blk_ptr;                // [nQ + 1]
    std::vector<uint32_t> meta;                  // [2 * S] per state: slot | in-arcs << 16 | start << 31; its first in-arc
    std::vector<uint32_t> in_arc;                // [R] per eps_(q,c) the p with an arc (p, A, q), c in A, ascending:
                                                 // p | (eps_(p,c) or kPatSetNone) << 16
    std::vector<int32_t> finals;                 // the final DFA states, ascending
    // kind 2 only, beside the tables of kind 0
    std::vector<float> in_w, accept_w, start_w;  // parallel to in_src, accept, start
    struct WArc { int32_t src, label, dst; float w; };
    std::vector<WArc> warcs;                     // the pruned automaton's arcs by (src, label), renumbered
    std::vector<int32_t> warc_ptr;               // [nQ + 1] the arcs that leave state p are warcs[warc_ptr[p] .. warc_ptr[p + 1])
    std::vector<uint8_t> is_final;               // [nQ]
    std::vector<float> final_w;                  // [nQ] (0 where the state is not final)
    int edges() const { return kind == 1 ? (int)in_arc.size() : (int)in_src.size(); }
};

namespace hctr {

inline std::string pat_float_str(float v) { return std::isnan(v) ? "nan" : v > 0 ? "+inf" : "-inf"; }      // (of a non-finite v)

// pat_build and pat_build_weighted: *out from checked arguments; false with a message under `who` for the caller's
// mistakes (std::bad_alloc passes through). weighted = false ignores the weight arguments and leaves kind 0.
inline bool pat_build_explicit(const char* who, bool weighted, const int32_t* arcs_src, const int32_t* arcs_label,
                               const int32_t* arcs_dst, const float* arcs_weight, int num_arcs, const int32_t* finals,
                               const float* final_weight, int num_finals, int num_states, int C, hctr_pat* out,
                               std::string* msg) {
    auto bad = [&](const std::string& m) { *msg = std::string(who) + ": " + m; return false; };
    auto str = [](int64_t v) { return std::to_string(v); };
    if (num_arcs < 0 || num_finals < 0) return bad("negative count");
    if (num_arcs > 0 && (!arcs_src || !arcs_label || !arcs_dst)) return bad("arcs_src / arcs_label / arcs_dst is NULL");
    if (num_finals > 0 && !finals) return bad("finals is NULL");
    if (C < 2) return bad("need C >= 2 classes, got C=" + str(C));
    if (num_states < 1) return bad("need num_states >= 1, got " + str(num_states));
    if (num_states > (1 << 24)) return bad("num_states=" + str(num_states) + " exceeds " + str(1 << 24));
    const size_t nq0 = (size_t)num_states;
    using Arc = hctr_pat::WArc;
    std::vector<Arc> arcs((size_t)num_arcs);
    for (int i = 0; i < num_arcs; ++i) {
        const Arc a{arcs_src[i], arcs_label[i], arcs_dst[i], weighted && arcs_weight ? arcs_weight[i] : 0.f};
        if (a.src < 0 || a.src >= num_states || a.dst < 0 || a.dst >= num_states)
            return bad("arc " + str(i) + " (" + str(a.src) + " -> " + str(a.dst) + ") names a state outside [0," +
                       str(num_states - 1) + "]");
        if (a.label < 1 || a.label > C - 1)
            return bad("label " + str(a.label) + " (arc " + str(i) + ") outside [1," + str(C - 1) + "]");
        if (!std::isfinite(a.w))
            return bad("arcs_weight[" + str(i) + "] is " + pat_float_str(a.w) +
                       ": a weight must be finite (an arc that cannot be taken is left out)");
        arcs[(size_t)i] = a;
    }
    std::sort(arcs.begin(), arcs.end(), [](const Arc& a, const Arc& b) {
        return a.src != b.src ? a.src < b.src : a.label != b.label ? a.label < b.label : a.dst < b.dst;
    });
    for (size_t i = 1; i < arcs.size(); ++i)
        if (arcs[i].src == arcs[i - 1].src && arcs[i].label == arcs[i - 1].label)
            return bad("not deterministic: two arcs leave state " + str(arcs[i].src) + " on label " + str(arcs[i].label));
    std::vector<uint8_t> fin(nq0, 0);
    std::vector<float> finw(weighted ? nq0 : 0, 0.f);
    for (int i = 0; i < num_finals; ++i) {
        if (finals[i] < 0 || finals[i] >= num_states)
            return bad("finals[" + str(i) + "]=" + str(finals[i]) + " outside [0," + str(num_states - 1) + "]");
        if (weighted) {
            const float w = final_weight ? final_weight[i] : 0.f;
            if (!std::isfinite(w))
                return bad("final_weight[" + str(i) + "] is " + pat_float_str(w) +
                           ": a weight must be finite (a state that cannot end a text is not final)");
            if (fin[(size_t)finals[i]] && finw[(size_t)finals[i]] != w)
                return bad("final state " + str(finals[i]) + " is listed twice with different weights (" +
                           std::to_string(finw[(size_t)finals[i]]) + " and " + std::to_string(w) + ")");
            finw[(size_t)finals[i]] = w;
        }
        fin[(size_t)finals[i]] = 1;
    }
    // prune: forward from state 0, backward from the final states
    std::vector<int32_t> optr(nq0 + 1, 0), iptr(nq0 + 1, 0), isrc(arcs.size());
    for (const Arc& a : arcs) { ++optr[(size_t)a.src + 1]; ++iptr[(size_t)a.dst + 1]; }
    for (size_t q = 0; q < nq0; ++q) { optr[q + 1] += optr[q]; iptr[q + 1] += iptr[q]; }
    {
        std::vector<int32_t> at(iptr.begin(), iptr.end() - 1);
        for (const Arc& a : arcs) isrc[(size_t)at[(size_t)a.dst]++] = a.src;
    }
    std::vector<uint8_t> fwd(nq0, 0), bwd(nq0, 0);
    std::vector<int32_t> stack{0};
    fwd[0] = 1;
    while (!stack.empty()) {
        const int32_t q = stack.back();
        stack.pop_back();
        for (int32_t j = optr[(size_t)q]; j < optr[(size_t)q + 1]; ++j)
            if (!fwd[(size_t)arcs[(size_t)j].dst]) { fwd[(size_t)arcs[(size_t)j].dst] = 1; stack.push_back(arcs[(size_t)j].dst); }
    }
    for (size_t q = 0; q < nq0; ++q)
        if (fin[q]) { bwd[q] = 1; stack.push_back((int32_t)q); }
    while (!stack.empty()) {
        const int32_t q = stack.back();
        stack.pop_back();
        for (int32_t j = iptr[(size_t)q]; j < iptr[(size_t)q + 1]; ++j)
            if (!bwd[(size_t)isrc[(size_t)j]]) { bwd[(size_t)isrc[(size_t)j]] = 1; stack.push_back(isrc[(size_t)j]); }
    }
    if (!bwd[0]) return bad("the pattern's language is empty: no final state can be reached from state 0");
    std::vector<int32_t> renum(nq0, -1);
    int nQ = 0;
    for (size_t q = 0; q < nq0; ++q)
        if (fwd[q] && bwd[q]) renum[q] = nQ++;
    std::vector<Arc> live;
    for (const Arc& a : arcs)
        if (renum[(size_t)a.src] >= 0 && renum[(size_t)a.dst] >= 0)
            live.push_back(Arc{renum[(size_t)a.src], a.label, renum[(size_t)a.dst], a.w});      // (still sorted by src, label)
    // the eps states: the distinct (dst, label), ascending
    std::vector<std::pair<int32_t, int32_t>> pairs;
    for (const Arc& a : live) pairs.emplace_back(a.dst, a.label);
    std::sort(pairs.begin(), pairs.end());
    pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
    const int64_t S64 = (int64_t)nQ + (int64_t)pairs.size();
    if (S64 > kPatMaxStates)
        return bad("the pattern has " + str(S64) + " CTC states (" + str(nQ) + " DFA states + " + str((int64_t)pairs.size()) +
                   " (state, label) pairs), HCTR_PAT_MAX_STATES is " + str(kPatMaxStates));
    hctr_pat& x = *out;
    x.kind = weighted ? 2 : 0; x.C = C; x.nQ = nQ; x.S = (int)S64;
    const size_t S = (size_t)S64;
    auto eps = [&](int32_t q, int32_t c) {
        return nQ + (int32_t)(std::lower_bound(pairs.begin(), pairs.end(), std::make_pair(q, c)) - pairs.begin());
    };
    std::vector<int32_t> pptr((size_t)nQ + 1, 0);     // the eps states of DFA state q are nQ + [pptr[q], pptr[q + 1])
    for (const auto& p : pairs) ++pptr[(size_t)p.first + 1];
    for (int q = 0; q < nQ; ++q) pptr[(size_t)q + 1] += pptr[(size_t)q];
    x.label.assign(S, 0);
    for (size_t i = 0; i < pairs.size(); ++i) x.label[(size_t)nQ + i] = pairs[i].second;
    x.classes.assign(x.label.begin() + nQ, x.label.end());
    std::sort(x.classes.begin(), x.classes.end());
    x.classes.erase(std::unique(x.classes.begin(), x.classes.end()), x.classes.end());
    x.slot.assign(S, 0);
    for (size_t s = (size_t)nQ; s < S; ++s)
        x.slot[s] = 1 + (int32_t)(std::lower_bound(x.classes.begin(), x.classes.end(), x.label[s]) - x.classes.begin());
    // the arcs by (dst, label): the sources p of eps_(q,c)
    std::vector<Arc> by_dst(live);
    std::sort(by_dst.begin(), by_dst.end(), [](const Arc& a, const Arc& b) {
        return a.dst != b.dst ? a.dst < b.dst : a.label != b.label ? a.label < b.label : a.src < b.src;
    });
    x.in_ptr.assign(1, 0);
    std::vector<std::pair<int32_t, float>> srcs;      // (source, the edge's weight); the sources of a state are distinct
    size_t k = 0;                                     // walks by_dst along with the pairs
    for (size_t s = 0; s < S; ++s) {
        srcs.clear();
        srcs.emplace_back((int32_t)s, 0.f);
        if (s < (size_t)nQ) {
            for (int32_t j = pptr[s]; j < pptr[s + 1]; ++j) srcs.emplace_back(nQ + j, 0.f);
        } else {
            const int32_t q = pairs[s - (size_t)nQ].first, c = pairs[s - (size_t)nQ].second;
            for (; k < by_dst.size() && by_dst[k].dst == q && by_dst[k].label == c; ++k) {
                const int32_t p = by_dst[k].src;
                srcs.emplace_back(p, by_dst[k].w);
                for (int32_t j = pptr[(size_t)p]; j < pptr[(size_t)p + 1]; ++j)
                    if (pairs[(size_t)j].second != c) srcs.emplace_back(nQ + j, by_dst[k].w);
            }
        }
        std::sort(srcs.begin(), srcs.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        if (x.in_src.size() + srcs.size() > (size_t)kPatMaxEdges)
            return bad("the pattern has more than " + str(kPatMaxEdges) + " edges (HCTR_PAT_MAX_EDGES); " + str((int64_t)s) +
                       " of its " + str(S64) + " CTC states reach that figure");
        for (const auto& v : srcs) {
            x.in_src.push_back((uint16_t)v.first);
            if (weighted) x.in_w.push_back(v.second);
        }
        x.in_ptr.push_back((int32_t)x.in_src.size());
        x.max_deg = std::max(x.max_deg, (int)srcs.size());
    }
    std::vector<uint8_t> nfin((size_t)nQ, 0);
    for (size_t q = 0; q < nq0; ++q)
        if (renum[q] >= 0 && fin[q]) nfin[(size_t)renum[q]] = 1;
    for (int q = 0; q < nQ; ++q)
        if (nfin[(size_t)q]) x.accept.push_back(q);
    for (size_t i = 0; i < pairs.size(); ++i)
        if (nfin[(size_t)pairs[i].first]) x.accept.push_back(nQ + (int32_t)i);
    x.start.assign(1, 0);
    for (const Arc& a : live)
        if (a.src == 0) x.start.push_back(eps(a.dst, a.label));
    std::sort(x.start.begin(), x.start.end());
    x.start.erase(std::unique(x.start.begin(), x.start.end()), x.start.end());
    if (!weighted) return true;
    x.is_final = nfin;
    x.final_w.assign((size_t)nQ, 0.f);
    for (size_t q = 0; q < nq0; ++q)
        if (renum[q] >= 0 && fin[q]) x.final_w[(size_t)renum[q]] = finw[q];
    for (int32_t s : x.accept) x.accept_w.push_back(x.final_w[(size_t)(s < nQ ? s : pairs[(size_t)(s - nQ)].first)]);
    x.start_w.assign(x.start.size(), 0.f);            // (0, c) names one arc: one weight per start state
    for (const Arc& a : live)
        if (a.src == 0)
            x.start_w[(size_t)(std::lower_bound(x.start.begin(), x.start.end(), eps(a.dst, a.label)) - x.start.begin())] = a.w;
    x.warc_ptr.assign((size_t)nQ + 1, 0);
    for (const Arc& a : live) ++x.warc_ptr[(size_t)a.src + 1];
    for (int q = 0; q < nQ; ++q) x.warc_ptr[(size_t)q + 1] += x.warc_ptr[(size_t)q];
    x.warcs = std::move(live);
    return true;
}

inline bool pat_build(const int32_t* arcs_src, const int32_t* arcs_label, const int32_t* arcs_dst, int num_arcs,
                      const int32_t* finals, int num_finals, int num_states, int C, hctr_pat* out, std::string* msg) {
    return pat_build_explicit("hctr_pat_build", false, arcs_src, arcs_label, arcs_dst, nullptr, num_arcs, finals, nullptr,
                              num_finals, num_states, C, out, msg);
}

// kind 2: pat_build's automaton and tables with a finite weight per arc and per final state (NULL = zeros)
inline bool pat_build_weighted(const int32_t* arcs_src, const int32_t* arcs_label, const int32_t* arcs_dst,
                               const float* arcs_weight, int num_arcs, const int32_t* finals, const float* final_weight,
                               int num_finals, int num_states, int C, hctr_pat* out, std::string* msg) {
    return pat_build_explicit("hctr_pat_build_weighted", true, arcs_src, arcs_label, arcs_dst, arcs_weight, num_arcs, finals,
                              final_weight, num_finals, num_states, C, out, msg);
}

// the weight of a text under a kind-2 pattern: the float64 sum, in text order, of its arcs' float32 weights, then the
// final weight of the state it ends in; -inf for a text outside the language
inline double pat_text_weight(const hctr_pat& x, const int32_t* labels, int n) {
    double w = 0.0;
    int32_t q = 0;
    for (int i = 0; i < n; ++i) {
        const hctr_pat::WArc *f = x.warcs.data() + x.warc_ptr[(size_t)q], *l = x.warcs.data() + x.warc_ptr[(size_t)q + 1];
        const hctr_pat::WArc* at =
            std::lower_bound(f, l, labels[i], [](const hctr_pat::WArc& a, int32_t c) { return a.label < c; });
        if (at == l || at->label != labels[i]) return -INFINITY;
        w += (double)at->w;
        q = at->dst;
    }
    return x.is_final[(size_t)q] ? w + (double)x.final_w[(size_t)q] : -INFINITY;
}

// The set form: arcs (src, set, dst) that carry label sets, set k = set_labels[set_ptr[k] .. set_ptr[k + 1]). The
// language and the CTC lift (the states and their numbering) are those of pat_build on the same automaton with every
// arc expanded into single-label arcs; what is built instead of the edge list is, per eps_(q,c), the source DFA states p
// with an arc (p, A, q), c in A - pattern_set_kernel sums a block (beta_p and every eps_(p,.)) once per step and takes
// the one state of the block that may not feed eps_(q,c), eps_(p,c), out of the total.
inline bool pat_build_sets(const int32_t* arcs_src, const int32_t* arcs_set, const int32_t* arcs_dst, int num_arcs,
                           const int32_t* set_ptr, const int32_t* set_labels, int num_sets, const int32_t* finals,
                           int num_finals, int num_states, int C, hctr_pat* out, std::string* msg) {
    auto bad = [&](const std::string& m) { *msg = "hctr_pat_build_sets: " + m; return false; };
    auto str = [](int64_t v) { return std::to_string(v); };
    if (num_arcs < 0 || num_finals < 0 || num_sets < 0) return bad("negative count");
    if (num_arcs > 0 && (!arcs_src || !arcs_set || !arcs_dst)) return bad("arcs_src / arcs_set / arcs_dst is NULL");
    if (num_sets > 0 && (!set_ptr || !set_labels)) return bad("set_ptr / set_labels is NULL");
    if (num_finals > 0 && !finals) return bad("finals is NULL");
    if (C < 2) return bad("need C >= 2 classes, got C=" + str(C));
    if (num_states < 1) return bad("need num_states >= 1, got " + str(num_states));
    if (num_states > (1 << 24)) return bad("num_states=" + str(num_states) + " exceeds " + str(1 << 24));
    if (num_sets > 0 && set_ptr[0] != 0) return bad("set_ptr[0] must be 0, got " + str(set_ptr[0]));
    for (int k = 0; k < num_sets; ++k) {
        const int32_t f = set_ptr[k], l = set_ptr[k + 1];
        if (l <= f) return bad("set " + str(k) + " is empty");
        for (int32_t j = f; j < l; ++j) {
            if (set_labels[j] < 1 || set_labels[j] > C - 1)
                return bad("label " + str(set_labels[j]) + " (set " + str(k) + ") outside [1," + str(C - 1) + "]");
            if (j > f && set_labels[j] <= set_labels[j - 1])
                return bad("the labels of set " + str(k) + " are not ascending: " + str(set_labels[j - 1]) + " before " +
                           str(set_labels[j]));
        }
    }
    const size_t nq0 = (size_t)num_states;
    struct Arc { int32_t src, set, dst; };
    std::vector<Arc> arcs((size_t)num_arcs);
    for (int i = 0; i < num_arcs; ++i) {
        const Arc a{arcs_src[i], arcs_set[i], arcs_dst[i]};
        if (a.src < 0 || a.src >= num_states || a.dst < 0 || a.dst >= num_states)
            return bad("arc " + str(i) + " (" + str(a.src) + " -> " + str(a.dst) + ") names a state outside [0," +
                       str(num_states - 1) + "]");
        if (a.set < 0 || a.set >= num_sets)
            return bad("arc " + str(i) + " names set " + str(a.set) + " outside [0," + str((int64_t)num_sets - 1) + "]");
        arcs[(size_t)i] = a;
    }
    std::sort(arcs.begin(), arcs.end(), [](const Arc& a, const Arc& b) {
        return a.src != b.src ? a.src < b.src : a.dst != b.dst ? a.dst < b.dst : a.set < b.set;
    });
    {   // determinism: the sets that leave one state are pairwise disjoint
        std::vector<int32_t> seen((size_t)C, -1);
        for (const Arc& a : arcs)
            for (int32_t j = set_ptr[a.set]; j < set_ptr[a.set + 1]; ++j) {
                if (seen[(size_t)set_labels[j]] == a.src)
                    return bad("not deterministic: the sets of two arcs that leave state " + str(a.src) + " overlap on label " +
                               str(set_labels[j]));
                seen[(size_t)set_labels[j]] = a.src;
            }
    }
    std::vector<uint8_t> fin(nq0, 0);
    for (int i = 0; i < num_finals; ++i) {
        if (finals[i] < 0 || finals[i] >= num_states)
            return bad("finals[" + str(i) + "]=" + str(finals[i]) + " outside [0," + str(num_states - 1) + "]");
        fin[(size_t)finals[i]] = 1;
    }
    // prune: forward from state 0, backward from the final states
    std::vector<int32_t> optr(nq0 + 1, 0), iptr(nq0 + 1, 0), isrc(arcs.size());
    for (const Arc& a : arcs) { ++optr[(size_t)a.src + 1]; ++iptr[(size_t)a.dst + 1]; }
    for (size_t q = 0; q < nq0; ++q) { optr[q + 1] += optr[q]; iptr[q + 1] += iptr[q]; }
    {
        std::vector<int32_t> at(iptr.begin(), iptr.end() - 1);
        for (const Arc& a : arcs) isrc[(size_t)at[(size_t)a.dst]++] = a.src;
    }
    std::vector<uint8_t> fwd(nq0, 0), bwd(nq0, 0);
    std::vector<int32_t> stack{0};
    fwd[0] = 1;
    while (!stack.empty()) {
        const int32_t q = stack.back();
        stack.pop_back();
        for (int32_t j = optr[(size_t)q]; j < optr[(size_t)q + 1]; ++j)
            if (!fwd[(size_t)arcs[(size_t)j].dst]) { fwd[(size_t)arcs[(size_t)j].dst] = 1; stack.push_back(arcs[(size_t)j].dst); }
    }
    for (size_t q = 0; q < nq0; ++q)
        if (fin[q]) { bwd[q] = 1; stack.push_back((int32_t)q); }
    while (!stack.empty()) {
        const int32_t q = stack.back();
        stack.pop_back();
        for (int32_t j = iptr[(size_t)q]; j < iptr[(size_t)q + 1]; ++j)
            if (!bwd[(size_t)isrc[(size_t)j]]) { bwd[(size_t)isrc[(size_t)j]] = 1; stack.push_back(isrc[(size_t)j]); }
    }
    if (!bwd[0]) return bad("the pattern's language is empty: no final state can be reached from state 0");
    std::vector<int32_t> renum(nq0, -1);
    int nQ = 0;
    for (size_t q = 0; q < nq0; ++q)
        if (fwd[q] && bwd[q]) renum[q] = nQ++;
    if (nQ > kPatSetMaxDfaStates)
        return bad("the pattern has " + str(nQ) + " DFA states, HCTR_PATSET_MAX_DFA_STATES is " + str(kPatSetMaxDfaStates));
    std::vector<Arc> live;                            // by (dst, src): the order of every state's in-arcs
    for (const Arc& a : arcs)
        if (renum[(size_t)a.src] >= 0 && renum[(size_t)a.dst] >= 0)
            live.push_back(Arc{renum[(size_t)a.src], a.set, renum[(size_t)a.dst]});
    std::stable_sort(live.begin(), live.end(), [](const Arc& a, const Arc& b) {
        return a.dst != b.dst ? a.dst < b.dst : a.src < b.src;
    });
    // the eps states: per destination q the union of the sets of the arcs into q, ascending
    hctr_pat& x = *out;
    x.kind = 1; x.C = C; x.nQ = nQ;
    x.blk_ptr.assign((size_t)nQ + 1, 0);
    std::vector<int32_t> plab;                        // the label of eps state nQ + i
    {
        std::vector<int32_t> seen((size_t)C, -1), got;
        size_t k = 0;
        for (int q = 0; q < nQ; ++q) {
            got.clear();
            for (; k < live.size() && live[k].dst == q; ++k)
                for (int32_t j = set_ptr[live[k].set]; j < set_ptr[live[k].set + 1]; ++j)
                    if (seen[(size_t)set_labels[j]] != q) { seen[(size_t)set_labels[j]] = q; got.push_back(set_labels[j]); }
            std::sort(got.begin(), got.end());
            plab.insert(plab.end(), got.begin(), got.end());
            x.blk_ptr[(size_t)q + 1] = (int32_t)plab.size();
            if ((int64_t)nQ + (int64_t)plab.size() > kPatSetMaxStates)
                return bad("the pattern has more than " + str(kPatSetMaxStates) + " CTC states (HCTR_PATSET_MAX_STATES): " +
                           str(nQ) + " DFA states + " + str((int64_t)plab.size()) + " (state, label) pairs up to DFA state " +
                           str(q) + " of " + str(nQ));
        }
    }
    const size_t S = (size_t)nQ + plab.size();
    x.S = (int)S;
    x.label.assign(S, 0);
    std::copy(plab.begin(), plab.end(), x.label.begin() + nQ);
    x.classes = plab;
    std::sort(x.classes.begin(), x.classes.end());
    x.classes.erase(std::unique(x.classes.begin(), x.classes.end()), x.classes.end());
    if (x.classes.size() > 0xFFFFu) return bad("the pattern uses " + str((int64_t)x.classes.size()) + " classes, more than 65535");
    x.slot.assign(S, 0);
    for (size_t s = (size_t)nQ; s < S; ++s)
        x.slot[s] = 1 + (int32_t)(std::lower_bound(x.classes.begin(), x.classes.end(), x.label[s]) - x.classes.begin());
    auto eps = [&](int32_t q, int32_t c) -> uint32_t {      // eps_(q,c), or kPatSetNone
        const int32_t *f = plab.data() + x.blk_ptr[(size_t)q], *l = plab.data() + x.blk_ptr[(size_t)q + 1];
        const int32_t* at = std::lower_bound(f, l, c);
        return at != l && *at == c ? (uint32_t)(nQ + (at - plab.data())) : kPatSetNone;
    };
    // the reduced in-arcs: count, then fill in the arcs' order (ascending source within a destination)
    std::vector<int64_t> deg(S, 0);
    int64_t R = 0;
    for (const Arc& a : live) R += set_ptr[a.set + 1] - set_ptr[a.set];
    if (R > kPatSetMaxInArcs)
        return bad("the pattern has " + str(R) + " in-arcs ((state, label) pairs summed over their source states), "
                   "HCTR_PATSET_MAX_INARCS is " + str(kPatSetMaxInArcs));
    for (const Arc& a : live)
        for (int32_t j = set_ptr[a.set]; j < set_ptr[a.set + 1]; ++j) ++deg[eps(a.dst, set_labels[j])];
    std::vector<uint32_t> first(S + 1, 0);
    for (size_t s = 0; s < S; ++s) first[s + 1] = first[s] + (uint32_t)deg[s];
    x.in_arc.assign((size_t)R, 0);
    {
        std::vector<uint32_t> at(first.begin(), first.end() - 1);
        for (const Arc& a : live)
            for (int32_t j = set_ptr[a.set]; j < set_ptr[a.set + 1]; ++j) {
                const int32_t c = set_labels[j];
                x.in_arc[at[eps(a.dst, c)]++] = (uint32_t)a.src | eps(a.src, c) << 16;
            }
    }
    x.meta.assign(2 * S, 0);
    for (size_t s = 0; s < S; ++s) {
        x.meta[2 * s] = (uint32_t)x.slot[s] | (uint32_t)deg[s] << 16;      // (deg <= nQ <= 4096 < 2^15)
        x.meta[2 * s + 1] = first[s];
        x.max_deg = std::max(x.max_deg, (int)deg[s]);
    }
    x.meta[0] |= 1u << 31;                            // the start list: beta_0 and the eps states of the arcs that leave 0
    for (const Arc& a : live)
        if (a.src == 0)
            for (int32_t j = set_ptr[a.set]; j < set_ptr[a.set + 1]; ++j) x.meta[2 * (size_t)eps(a.dst, set_labels[j])] |= 1u << 31;
    for (size_t q = 0; q < nq0; ++q)
        if (renum[q] >= 0 && fin[q]) x.finals.push_back(renum[q]);
    return true;
}

}  // namespace hctr
