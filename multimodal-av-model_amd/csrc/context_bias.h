// The phrase automaton of contextual biasing on the device (bias.py: ContextBias): its tables, one transition and the argument checks.
// Used by the counting kernel of context_bias.hip and by the biased instantiation of the search kernel in ctc_beam.hip.
//
// The law (bias.py).  P is a set of distinct phrases of 1..32 token ids, none of them the blank.  The state of a prefix is
// (k, tail), (0, ()) for the empty prefix.  Per token c: tail <- the longest suffix of tail + (c) that is a prefix of some phrase of P
// (it may be empty); if tail is in P, k <- k + |tail| and tail <- ().  Matches are leftmost and non-overlapping.  m = k + |tail|: k is the
// banked credit, |tail| the refundable credit of a running partial match.  A function of the prefix's content alone.
//
// Tables.  The trie of P, the root is node 0, a tail is the node it spells.  nodes int32 [node_count][2] = (failure link, depth |
// terminal << 16): the failure link is the deepest node that spells a proper suffix of this node's path (0 for the root and its children).
// Edges: the open-addressing table of ngram_lm.h - 16-byte slots {u64 key, i32 child, i32 0}, power-of-two size, key 0 = empty, linear
// probing from splitmix64(key) & (slots - 1), at most `probe` probes at masked indices - with the exact key (node << 16) | (c + 1).
// The tables hold integers only; the weight is an argument of the search.  Every node index that is read from a table is clamped to
// [0, node_count) before it is used: a corrupt table gives wrong counts, never an access out of bounds.
#pragma once
#include "ngram_lm.h"

namespace {

constexpr int BIAS_MAXLEN = 32;                     // ids in a phrase; a walk down the failure links takes at most this many steps

struct BiasTables {
    const int2* nodes;                              // [n] {failure link, depth | terminal << 16}
    const uint4* tab;                               // [slots] {key lo, key hi, child, 0}
    unsigned long long smask;                       // slots - 1
    int n, probe;
};

__device__ __forceinline__ int bias_node(const BiasTables& t, int x) { return min(max(x, 0), t.n - 1); }

// |tail| of the state `node` (a valid node index)
__device__ __forceinline__ int bias_depth(const BiasTables& t, int node) { return t.nodes[node].y & 63; }

// one token: (node, k) <- the state after c; 0 <= c < V, c is not the blank, node is a valid node index
__device__ __forceinline__ void bias_step(const BiasTables& t, int& node, int& k, int c) {
    bool found = false;
    for (int it = 0; it <= BIAS_MAXLEN && !found; ++it) {
        unsigned child, unused;
        if (slot_find(t.tab, t.smask, t.probe, ((unsigned long long)node << 16) | (unsigned long long)(c + 1), child, unused)) {
            node = bias_node(t, (int)child);
            found = true;
        } else if (node == 0) {
            break;
        } else {
            node = bias_node(t, t.nodes[node].x);
        }
    }
    if (!found) node = 0;                           // no suffix of tail + (c) starts a phrase (or a corrupt table's walk ran out)
    const int info = t.nodes[node].y;
    if ((info >> 16) & 1) { k += info & 63; node = 0; }
}

static int bias_check(const char* who, const void* nodes, const void* edges, int node_count, long long slots, int probe, int V,
                      BiasTables* t) {
    AV_CHECK(nodes && edges, "%s: null bias table", who);
    AV_CHECK(V >= 2 && V <= 65533, "%s: the bias tables need 2 <= V <= 65533, got %d", who, V);
    AV_CHECK(node_count >= 1, "%s: bias_node_count %d < 1", who, node_count);
    AV_CHECK(slots >= 1 && slots <= (1ll << 40) && (slots & (slots - 1)) == 0, "%s: bias_slots %lld is not a power of two", who, slots);
    AV_CHECK(probe >= 1 && probe <= slots, "%s: bias_probe_bound %d outside [1, bias_slots %lld]", who, probe, slots);
    AV_CHECK(((uintptr_t)edges & 15) == 0 && ((uintptr_t)nodes & 7) == 0, "%s: the bias tables are not aligned (edges 16 bytes, nodes 8)", who);
    t->nodes = (const int2*)nodes; t->tab = (const uint4*)edges; t->smask = (unsigned long long)slots - 1;
    t->n = node_count; t->probe = probe;
    return AV_OK;
}

}  // namespace
