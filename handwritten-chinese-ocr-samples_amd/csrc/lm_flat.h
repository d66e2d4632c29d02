// Flat, pointer-free image of an ARPA n-gram model (hctr_lm, include/hctr_hip.h) and THE lookup routine over it,
// compiled for the host (ngram_lm.cpp: hctr_lm_build, hctr_lm_word_logp) and for the device (kernels.hip: the
// LM-scored prefix beam search). One open-addressing table holds the n-grams of every order: power-of-two capacity,
// load <= 0.5, linear probing, 32-byte slots. A probe compares all six word ids (unused positions hold -1, so the
// n-gram's length is part of the comparison): lookups are exact, never by fingerprint.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define HCTR_HD __host__ __device__ __forceinline__
#else
#define HCTR_HD inline
#endif

#ifndef __cplusplus
#error "lm_flat.h is C++"
#endif

#include <vector>

namespace hctr {

constexpr int kLmMaxOrder = 6;
constexpr int32_t kLmEmpty = -2;                 // ids[0] of a free slot (word ids are >= 0, padding is -1)

struct alignas(32) LmSlot {
    int32_t ids[kLmMaxOrder];                    // the n-gram's word ids, then -1
    float logp, backoff;
};
static_assert(sizeof(LmSlot) == 32, "one slot is one 32-byte read");

struct LmView {                                  // what a lookup needs; slots may be host or device memory
    const LmSlot* slots;
    uint32_t mask;                               // capacity - 1
    int32_t order, unk;
};

struct LmKey {
    int32_t w[kLmMaxOrder];
};

// The hash of an n-gram folds its word ids from the LAST to the first, so the keys of one lookup routine call share
// their work: the n-gram "n context words + word" continues the fold of "n - 1 context words + word" by one id, and
// the back-off entries' keys form a second such chain. 32-bit arithmetic (a 64-bit multiply is several instructions
// on the device); lm_hash_end scatters the running value before it is masked.
constexpr uint32_t kLmHashSeed = 0x243F6A88u;
HCTR_HD uint32_t lm_hash_fold(uint32_t h, int32_t w) {
    h = (h ^ (uint32_t)w) * 0x9E3779B1u;
    return h ^ (h >> 15);
}
HCTR_HD uint32_t lm_hash_end(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    return h ^ (h >> 13);
}
HCTR_HD uint32_t lm_hash(const int32_t* w, int n) {      // of the n-gram w[0 .. n)
    uint32_t h = kLmHashSeed;
    for (int i = n - 1; i >= 0; --i) h = lm_hash_fold(h, w[i]);
    return lm_hash_end(h);
}

HCTR_HD bool lm_same(const LmSlot& s, const LmKey& k) {
    bool eq = true;
#pragma unroll
    for (int i = 0; i < kLmMaxOrder; ++i) eq = eq && s.ids[i] == k.w[i];
    return eq;
}

// The end of one lookup whose first slot `s` (at place `at` of the probe sequence) has been read already: walks on only
// when that slot holds another n-gram. A lookup that is not `live` (its key has a negative id: padding, or an OOV word
// of a model without <unk>) is in no table.
HCTR_HD bool lm_probe_finish(const LmView& v, const LmKey& key, bool live, uint32_t at, LmSlot s, float* logp,
                             float* backoff) {
    bool hit = false;
    while (live) {
        if (lm_same(s, key)) { *logp = s.logp; *backoff = s.backoff; hit = true; break; }
        if (s.ids[0] == kLmEmpty) break;
        at = (at + 1) & v.mask;
        s = v.slots[at];
    }
    return hit;
}

// log10 P(word | context): the arithmetic of hctr::ngram_word_logp (ngram_lm.cpp), operation for operation - from the
// longest context down, the first n-gram found ends the walk with backoff + (double)logp; every context that had to
// be shortened pays its back-off weight into `backoff`, a double that starts at 0.0; word id -1 is <unk>, or -100
// when the model has none; a word without a unigram scores as <unk>'s unigram.
// cx is the context in its fixed form: the previous word ids right-aligned, most recent at cx[kLmMaxOrder - 2], -1 in
// front of a shorter one; only the last order - 1 count. A negative id (that padding, or an OOV word of a model without
// <unk>) matches no n-gram and no back-off entry - what the string-keyed tables answer for it, and what a walk that
// starts at the shorter context computes: a miss adds nothing. All 2 * order - 1 (+ 1) lookups have their keys before
// any is made: they are started together and combined afterwards, in the order of the walk. Every index is a
// compile-time constant, so on the device the keys and slots stay in registers.
HCTR_HD double lm_word_logp(const LmView& v, const int32_t (&cx)[kLmMaxOrder - 1], int32_t word) {
    if (word < 0) word = v.unk;
    if (word < 0) return -100.0;
    const int use = v.order - 1;
    // lookup 2n: the n-gram of n context words + the word; 2n + 1 (n >= 1): the back-off entry of those n context words;
    // lookup 1: <unk>'s unigram, for a word that has none
    constexpr int NP = 2 * kLmMaxOrder;
    LmKey key[NP];
    bool live[NP];
    uint32_t at[NP];
    LmSlot first[NP];
    uint32_t hg = lm_hash_fold(kLmHashSeed, word), hb = kLmHashSeed;      // the two chains of lm_hash
    at[0] = lm_hash_end(hg) & v.mask;
#pragma unroll
    for (int n = 0; n < kLmMaxOrder; ++n) {
        bool ok = n <= use;
#pragma unroll
        for (int i = 0; i < kLmMaxOrder; ++i) {
            const int32_t cw = i < n ? cx[kLmMaxOrder - 1 - n + i] : -1;
            key[2 * n].w[i] = i < n ? cw : (i == n ? word : -1);
            if (n > 0) key[2 * n + 1].w[i] = cw;
            if (i < n && cw < 0) ok = false;
        }
        live[2 * n] = ok;
        if (n > 0) {
            live[2 * n + 1] = ok;
            hg = lm_hash_fold(hg, cx[kLmMaxOrder - 1 - n]);
            hb = lm_hash_fold(hb, cx[kLmMaxOrder - 1 - n]);
            at[2 * n] = lm_hash_end(hg) & v.mask;
            at[2 * n + 1] = lm_hash_end(hb) & v.mask;
        }
    }
#pragma unroll
    for (int i = 0; i < kLmMaxOrder; ++i) key[1].w[i] = i == 0 ? v.unk : -1;
    live[1] = word != v.unk && v.unk >= 0;
    at[1] = lm_hash_end(lm_hash_fold(kLmHashSeed, v.unk)) & v.mask;
#pragma unroll
    for (int p = 0; p < NP; ++p) {                 // every first slot is read before any is looked at
        first[p] = live[p] ? v.slots[at[p]] : LmSlot{};
    }
    bool hit[NP];
    float lp[NP], bo[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        lp[p] = 0.f; bo[p] = 0.f;
        hit[p] = lm_probe_finish(v, key[p], live[p], at[p], first[p], &lp[p], &bo[p]);
    }
    double backoff = 0.0, res = 0.0;
    bool done = false;
#pragma unroll
    for (int n = kLmMaxOrder - 1; n >= 0; --n) {
        if (done || n > use) continue;
        if (hit[2 * n]) { res = backoff + (double)lp[2 * n]; done = true; }
        else if (n > 0 && hit[2 * n + 1]) backoff += (double)bo[2 * n + 1];
    }
    if (!done) res = hit[1] ? backoff + (double)lp[1] : backoff - 100.0;
    return res;
}

// the context after `word`: one place to the left
HCTR_HD void lm_roll(int32_t (&cx)[kLmMaxOrder - 1], int32_t word) {
#pragma unroll
    for (int i = 0; i + 1 < kLmMaxOrder - 1; ++i) cx[i] = cx[i + 1];
    cx[kLmMaxOrder - 2] = word;
}

}  // namespace hctr

// the object behind the C ABI's hctr_lm: the table, the label -> word map it was built for, and a serial number by
// which a context recognises the model whose device copy it holds (an address can be reused by a later model)
struct hctr_lm {
    int order = 0, C = 0;
    int32_t bos = -1, unk = -1;
    uint64_t serial = 0;
    std::vector<hctr::LmSlot> slots;             // power-of-two capacity
    std::vector<int32_t> label_words;            // [C]
    hctr::LmView view() const { return hctr::LmView{slots.data(), (uint32_t)slots.size() - 1u, order, unk}; }
};
