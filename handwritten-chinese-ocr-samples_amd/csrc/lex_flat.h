// The lexicon object behind the C ABI's hctr_lex (include/hctr_hip.h): the trie of a closed list of admissible texts,
// its partition into units (what one workgroup of lexicon_trie_kernel computes for one line) and the flat tables the
// kernel is given. Host only and header only: engine.cpp builds it (hctr_lex_build), tests read it back
// (hctr_lex_tables), and a stand-alone program can include it without the GPU runtime.
//
// Trie: node 0 is the root; the other nodes are numbered in the order in which inserting entry 0, 1, .. first reaches
// them, so a parent always has a lower number than its children.
// Units: a unit holds at most unit_nodes local nodes, local node 0 being the root (its blank state). It consists of
// whole subtrees plus a private copy of each subtree root's ancestor chain; copies compute the same bits as the
// originals and only owned nodes report scores, so a score does not depend on the partition. pack() walks the root's
// children in label order: a subtree that fits an empty unit (with its chain) goes into the open unit, or into a new one
// when the open one lacks the room; a larger subtree places its root alone and is split among its children, in label
// order, by the same rule. Local nodes are stored parents before children.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <unordered_map>
#include <vector>

namespace hctr {

constexpr int kLexMaxLen = 64;                   // HCTR_LEX_MAX_LEN
constexpr int kLexMinUnit = 128, kLexMaxUnit = 4096, kLexDefaultUnit = 4096;
// a local node's word in `node`: the local index of its parent, and
constexpr int32_t kLexSkip = 1 << 30;            // the parent is not the root and carries another label (n_p feeds n_v)
constexpr int32_t kLexFirst = 1 << 29;           // the parent is the root: the node starts at lp_0(c_v)
constexpr int32_t kLexParMask = 0xFFFF;

}  // namespace hctr

struct hctr_lex {
    int N = 0, C = 0, max_len = 0, unit_cap = 0, max_unit = 0;
    uint64_t serial = 0;
    bool has_prior = false;
    std::vector<float> prior;                    // [N] (zeros without priors)
    // the global trie
    std::vector<int32_t> parent, label;          // [nodes]; parent[0] = -1, label[0] = 0
    std::vector<int32_t> entry_node;             // [N]
    std::vector<int32_t> classes;                // the distinct labels, ascending
    // the units, flat: unit u's local nodes are [uoff[u], uoff[u + 1]), its classes [coff[u], coff[u + 1])
    std::vector<int32_t> uoff, coff;             // [units + 1]
    std::vector<int32_t> gnode;                  // [total] the global node of a local node
    std::vector<int32_t> node;                   // [total] local parent | kLexSkip | kLexFirst
    std::vector<uint8_t> owned;                  // [total] 1 = the unit owns the node, 0 = a copy of an ancestor
    std::vector<int32_t> kidx;                   // [total] the place of the node's label in the unit's class list
    std::vector<int32_t> ucls;                   // [sum] per unit: 0 (the blank), then its nodes' labels ascending
    std::vector<int32_t> eptr, elist;            // [total + 1], [N]: the entries that end on an owned local node
    int units() const { return (int)uoff.size() - 1; }
    int nodes() const { return (int)parent.size(); }
};

namespace hctr {

struct LexPacker {
    hctr_lex& x;
    int cap;
    std::vector<std::vector<int32_t>> kids;      // children by label
    std::vector<int32_t> size, depth, local;     // subtree size; depth (root 0); local index in the open unit or -1
    std::vector<int32_t> open;                   // the open unit's global nodes
    std::vector<uint8_t> open_owned;

    void close() {
        if (open.size() <= 1) return;
        for (size_t i = 0; i < open.size(); ++i) {
            const int32_t g = open[i];
            int32_t w = 0;
            if (g != 0) {
                const int32_t p = x.parent[(size_t)g];
                w = local[(size_t)p];
                if (p == 0) w |= kLexFirst;
                else if (x.label[(size_t)p] != x.label[(size_t)g]) w |= kLexSkip;
            }
            x.gnode.push_back(g);
            x.node.push_back(w);
            x.owned.push_back(open_owned[i]);
        }
        std::vector<int32_t> cls;
        for (size_t i = 1; i < open.size(); ++i) cls.push_back(x.label[(size_t)open[i]]);
        std::sort(cls.begin(), cls.end());
        cls.erase(std::unique(cls.begin(), cls.end()), cls.end());
        x.kidx.push_back(0);
        for (size_t i = 1; i < open.size(); ++i)
            x.kidx.push_back(1 + (int32_t)(std::lower_bound(cls.begin(), cls.end(), x.label[(size_t)open[i]]) - cls.begin()));
        x.ucls.push_back(0);
        x.ucls.insert(x.ucls.end(), cls.begin(), cls.end());
        x.uoff.push_back((int32_t)x.gnode.size());
        x.coff.push_back((int32_t)x.ucls.size());
        x.max_unit = std::max(x.max_unit, (int)open.size());
        for (int32_t g : open) local[(size_t)g] = -1;
        open.clear();
        open_owned.clear();
    }
    void begin() {
        if (!open.empty()) return;
        open.push_back(0);
        open_owned.push_back(0);
        local[0] = 0;
    }
    void add(int32_t g, bool own) {
        local[(size_t)g] = (int32_t)open.size();
        open.push_back(g);
        open_owned.push_back(own ? 1 : 0);
    }
    // the ancestors of v that the open unit lacks, top down
    int missing(int32_t v, std::vector<int32_t>* chain) const {
        int n = 0;
        for (int32_t p = x.parent[(size_t)v]; p > 0 && local[(size_t)p] < 0; p = x.parent[(size_t)p]) {
            if (chain) chain->push_back(p);
            ++n;
        }
        if (chain) std::reverse(chain->begin(), chain->end());
        return n;
    }
    void add_chain(int32_t v) {
        std::vector<int32_t> chain;
        missing(v, &chain);
        for (int32_t p : chain) add(p, false);
    }
    void add_subtree(int32_t v) {                // preorder: parents before children
        std::vector<int32_t> stack{v};
        while (!stack.empty()) {
            const int32_t g = stack.back();
            stack.pop_back();
            add(g, true);
            const auto& k = kids[(size_t)g];
            for (size_t i = k.size(); i-- > 0;) stack.push_back(k[i]);
        }
    }
    // make room for `own` owned nodes below v's chain in the open unit, or open a new one
    void room(int32_t v, int own) {
        begin();
        if ((int)open.size() + missing(v, nullptr) + own > cap) {
            close();
            begin();
        }
        add_chain(v);
    }
    void pack(int32_t v) {
        if (1 + (depth[(size_t)v] - 1) + size[(size_t)v] <= cap) {
            room(v, size[(size_t)v]);
            add_subtree(v);
            return;
        }
        room(v, 1);
        add(v, true);
        for (int32_t k : kids[(size_t)v]) pack(k);
    }
};

// builds *out from checked arguments; false with a message for the caller's mistakes (std::bad_alloc passes through)
inline bool lex_build(const int32_t* entries, const int32_t* entry_lengths, int N, int C, const float* log_prior,
                      int unit_nodes, hctr_lex* out, std::string* msg) {
    auto bad = [&](const std::string& m) { *msg = "hctr_lex_build: " + m; return false; };
    if (!entries || !entry_lengths) return bad("entries / entry_lengths is NULL");
    if (N < 1) return bad("need N >= 1 entries, got N=" + std::to_string(N));
    if (C < 2) return bad("need C >= 2 classes, got C=" + std::to_string(C));
    if (unit_nodes != 0 && (unit_nodes < kLexMinUnit || unit_nodes > kLexMaxUnit))
        return bad("unit_nodes=" + std::to_string(unit_nodes) + " outside [" + std::to_string(kLexMinUnit) + "," +
                   std::to_string(kLexMaxUnit) + "] (0 = the default)");
    hctr_lex& x = *out;
    x.N = N; x.C = C;
    x.unit_cap = unit_nodes ? unit_nodes : kLexDefaultUnit;
    x.has_prior = log_prior != nullptr;
    x.prior.assign((size_t)N, 0.f);
    for (int e = 0; e < N && log_prior; ++e) {
        if (!std::isfinite(log_prior[e])) return bad("log_prior[" + std::to_string(e) + "] is not finite");
        x.prior[(size_t)e] = log_prior[e];
    }
    x.parent.assign(1, -1);
    x.label.assign(1, 0);
    x.entry_node.resize((size_t)N);
    std::unordered_map<uint64_t, int32_t> child;      // (parent, label) -> node
    int64_t o = 0;
    for (int e = 0; e < N; ++e) {
        const int L = entry_lengths[e];
        if (L < 1 || L > kLexMaxLen)
            return bad("entry_lengths[" + std::to_string(e) + "]=" + std::to_string(L) + " outside [1," +
                       std::to_string(kLexMaxLen) + "]");
        int32_t v = 0;
        for (int j = 0; j < L; ++j) {
            const int32_t c = entries[o + j];
            if (c < 1 || c > C - 1)
                return bad("label " + std::to_string(c) + " (entry " + std::to_string(e) + ", position " +
                           std::to_string(j) + ") outside [1," + std::to_string(C - 1) + "]");
            const uint64_t key = ((uint64_t)(uint32_t)v << 32) | (uint32_t)c;
            auto it = child.find(key);
            if (it == child.end()) {
                if (x.parent.size() >= (size_t)INT32_MAX / 4) return bad("the lexicon has too many trie nodes");
                it = child.emplace(key, (int32_t)x.parent.size()).first;
                x.parent.push_back(v);
                x.label.push_back(c);
            }
            v = it->second;
        }
        x.entry_node[(size_t)e] = v;
        x.max_len = std::max(x.max_len, L);
        o += L;
    }
    const size_t nn = x.parent.size();
    x.classes.assign(x.label.begin() + 1, x.label.end());
    std::sort(x.classes.begin(), x.classes.end());
    x.classes.erase(std::unique(x.classes.begin(), x.classes.end()), x.classes.end());

    LexPacker pk{x, x.unit_cap, {}, {}, {}, {}, {}, {}};
    pk.kids.resize(nn);
    pk.size.assign(nn, 1);
    pk.depth.assign(nn, 0);
    pk.local.assign(nn, -1);
    for (size_t v = 1; v < nn; ++v) {
        pk.kids[(size_t)x.parent[v]].push_back((int32_t)v);
        pk.depth[v] = pk.depth[(size_t)x.parent[v]] + 1;
    }
    for (size_t v = nn; v-- > 1;) pk.size[(size_t)x.parent[v]] += pk.size[v];
    for (auto& k : pk.kids)
        std::sort(k.begin(), k.end(), [&](int32_t a, int32_t b) { return x.label[(size_t)a] < x.label[(size_t)b]; });
    x.uoff.assign(1, 0);
    x.coff.assign(1, 0);
    for (int32_t k : pk.kids[0]) pk.pack(k);
    pk.close();

    // the entries that end on each owned local node, in ascending entry order
    const size_t total = x.gnode.size();
    std::vector<int32_t> owner(nn, -1);               // global node -> the local place that owns it
    for (size_t i = 0; i < total; ++i)
        if (x.owned[i]) owner[(size_t)x.gnode[i]] = (int32_t)i;
    x.eptr.assign(total + 1, 0);
    for (int e = 0; e < N; ++e) ++x.eptr[(size_t)owner[(size_t)x.entry_node[(size_t)e]] + 1];
    for (size_t i = 0; i < total; ++i) x.eptr[i + 1] += x.eptr[i];
    x.elist.resize((size_t)N);
    std::vector<int32_t> at(x.eptr.begin(), x.eptr.end() - 1);
    for (int e = 0; e < N; ++e) x.elist[(size_t)at[(size_t)owner[(size_t)x.entry_node[(size_t)e]]]++] = e;
    return true;
}

}  // namespace hctr
