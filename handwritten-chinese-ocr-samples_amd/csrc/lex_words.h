// The tables of word-sequence recognition (hctr_words*, include/hctr_hip.h) over the global trie of a hctr_lex
// (lex_flat.h): what words_trie_kernel is given and what hctr_lex_word_tables exports. Host only and header only, no GPU
// runtime: a stand-alone program can include it.
//
// Per trie node v (node 0 is the root, a parent has a lower number than its children):
//   node[v]  parent | kLexSkip (the parent is not the root and carries another label: n_p feeds n_v)
//                   | kLexFirst (the parent is the root); the root's own word is 0
//   slot[v]  the place of the node's label in cls (0 for the root: the blank)
//   entry[v] e_v, the entry with the largest log_prior among those that end on v (ties to the lower index), or -1
//   weight[v] x_v = float32((double)log_prior[e_v] + (double)word_bonus); 0 where no entry ends
// cls: 0 (the blank), then the lexicon's distinct labels ascending.
#pragma once
#include "lex_flat.h"

namespace hctr {

constexpr int kWordsMaxNodes = 65536;            // HCTR_WORDS_MAX_NODES: a parent index fits kLexParMask

struct WordTables {
    std::vector<int32_t> node, slot, entry, cls;
    std::vector<float> weight;
    int nodes() const { return (int)node.size(); }
    int D() const { return (int)cls.size(); }
};

// false with a message for a trie beyond the limit or a non-finite bonus
inline bool word_tables(const hctr_lex& x, float word_bonus, WordTables* out, std::string* msg) {
    if (!std::isfinite(word_bonus)) {
        *msg = "word_bonus is not finite";
        return false;
    }
    const int nn = x.nodes();
    if (nn > kWordsMaxNodes) {
        *msg = "the lexicon's trie has " + std::to_string(nn) + " nodes, word-sequence recognition supports " +
               std::to_string(kWordsMaxNodes);
        return false;
    }
    WordTables& w = *out;
    w.cls.assign(1, 0);
    w.cls.insert(w.cls.end(), x.classes.begin(), x.classes.end());
    w.node.assign((size_t)nn, 0);
    w.slot.assign((size_t)nn, 0);
    w.entry.assign((size_t)nn, -1);
    w.weight.assign((size_t)nn, 0.f);
    for (int v = 1; v < nn; ++v) {
        const int32_t p = x.parent[(size_t)v];
        int32_t word = p;
        if (p == 0) word |= kLexFirst;
        else if (x.label[(size_t)p] != x.label[(size_t)v]) word |= kLexSkip;
        w.node[(size_t)v] = word;
        w.slot[(size_t)v] =
            1 + (int32_t)(std::lower_bound(x.classes.begin(), x.classes.end(), x.label[(size_t)v]) - x.classes.begin());
    }
    for (int e = 0; e < x.N; ++e) {
        const size_t v = (size_t)x.entry_node[(size_t)e];
        if (w.entry[v] < 0 || x.prior[(size_t)e] > x.prior[(size_t)w.entry[v]]) w.entry[v] = e;
    }
    for (int v = 1; v < nn; ++v)
        if (w.entry[(size_t)v] >= 0)
            w.weight[(size_t)v] = (float)((double)x.prior[(size_t)w.entry[(size_t)v]] + (double)word_bonus);
    return true;
}

}  // namespace hctr
