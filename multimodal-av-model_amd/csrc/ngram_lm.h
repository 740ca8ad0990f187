// The token n-gram model on the device (lm.py: NGramLM): its tables, one lookup, the scoring law and the argument checks.  Used by the
// batched scoring of ngram_lm.hip and by the fused instantiation of the search kernel in ctc_beam.hip.
//
// The n-gram scoring law (lm.py).  s(c | ctx), for m from min(N - 1, tokens available) down to 1: look up the (m + 1)-gram
// "last m context tokens, c"; found: return acc + logp.  Not found: acc += backoff(the m-gram that is the context), then drop the context's
// oldest token; a context that is absent adds nothing.  At m = 0 return acc + unigram(c).  acc starts at 0; the additions are float32, in
// that order, and there is nothing else - no multiply, no libm - so the host and the device give the same bits.
//
// Tables.  unigrams float32 [V + 1][2] = (logp, backoff), row V = bos.  n-grams of order >= 2: open-addressing hash table of 16-byte slots
// {u64 key, f32 logp, f32 backoff}, power-of-two size, key 0 = empty, linear probing from splitmix64(key) & (slots - 1).  Keys are exact:
// tokens oldest first as id + 1 in 16-bit fields, the newest in the low field; a prefix's context is its last N - 1 tokens in the same packing,
// ctx' = ((ctx << 16) | (c + 1)) & mask(N - 1); the empty prefix has ctx = bos + 1, or 0 without bos; a zero field means "context shorter than
// this order".  A lookup makes at most `probe_bound` probes (the longest run of a stored key, recorded when the table was built) at masked
// indices: a corrupt table cannot make it run away or read out of bounds.
#pragma once
#include "ctc_beam_common.h"

namespace {

struct LmTables {
    const float* uni;                               // [V + 1][2]
    const uint4* tab;                               // [slots] {key lo, key hi, logp, backoff}
    unsigned long long smask, cmask;                // slots - 1; mask of the N - 1 context fields
    int order, V, probe;
};

// One lookup in a table of this contract (also the phrase automaton's edge table, context_bias.h): the two value words of the slot that
// holds `key`, in at most `probe` probes at masked indices.
__device__ __forceinline__ bool slot_find(const uint4* tab, unsigned long long smask, int probe, unsigned long long key, unsigned& v0,
                                          unsigned& v1) {
    unsigned long long i = mix64(key + MIX64_STEP) & smask;                    // splitmix64(key)
    for (int p = 0; p < probe; ++p) {
        const uint4 s = tab[i];
        const unsigned long long k = (unsigned long long)s.x | ((unsigned long long)s.y << 32);
        if (k == key) { v0 = s.z; v1 = s.w; return true; }
        if (k == 0ull) return false;
        i = (i + 1) & smask;
    }
    return false;
}

__device__ __forceinline__ bool lm_find(const LmTables& lm, unsigned long long key, float& logp, float& backoff) {
    unsigned z, w;
    if (!slot_find(lm.tab, lm.smask, lm.probe, key, z, w)) return false;
    logp = __uint_as_float(z); backoff = __uint_as_float(w);
    return true;
}

// s(c | ctx); 0 <= c < V
__device__ __forceinline__ float lm_score(const LmTables& lm, unsigned long long ctx, int c) {
    float acc = 0.f, lp, bo;
    int m = lm.order - 1;
    while (m >= 1 && ((ctx >> (16 * (m - 1))) & 0xffffull) == 0ull) --m;
    for (; m >= 1; --m) {
        const unsigned long long cm = ctx & ((1ull << (16 * m)) - 1ull);
        if (lm_find(lm, (cm << 16) | (unsigned long long)(c + 1), lp, bo)) return __fadd_rn(acc, lp);
        if (m == 1) {
            if (cm - 1ull <= (unsigned long long)lm.V) acc = __fadd_rn(acc, lm.uni[2 * (cm - 1ull) + 1]);
        } else if (lm_find(lm, cm, lp, bo)) {
            acc = __fadd_rn(acc, bo);
        }
    }
    return __fadd_rn(acc, lm.uni[2 * c]);
}

static int lm_check(const char* who, const float* uni, const void* tab, long long slots, int order, int vocab, int bos, int probe, LmTables* lm) {
    AV_CHECK(uni && tab, "%s: null language-model table", who);
    AV_CHECK(order >= 1 && order <= 4, "%s: lm_order %d outside [1, 4]", who, order);
    AV_CHECK(vocab >= 2 && vocab <= 65533, "%s: lm_vocab %d outside [2, 65533]", who, vocab);
    AV_CHECK(bos == -1 || bos == vocab, "%s: lm_bos %d is neither -1 (none) nor lm_vocab %d", who, bos, vocab);
    AV_CHECK(slots >= 1 && slots <= (1ll << 40) && (slots & (slots - 1)) == 0, "%s: lm_slots %lld is not a power of two", who, slots);
    AV_CHECK(probe >= 1 && probe <= slots, "%s: lm_probe_bound %d outside [1, lm_slots %lld]", who, probe, slots);
    AV_CHECK(((uintptr_t)tab & 15) == 0, "%s: the language-model table is not 16-byte aligned", who);
    lm->uni = uni; lm->tab = (const uint4*)tab; lm->smask = (unsigned long long)slots - 1;
    lm->cmask = (1ull << (16 * (order - 1))) - 1ull;
    lm->order = order; lm->V = vocab; lm->probe = probe;
    return AV_OK;
}

}  // namespace
