// CTC prefix beam search on the device (the decoder the reference's beam_search.py:2-48 is named after but does not implement; opt-in in
// evaluate(), model/trainer.py:230,237 of the reference), without a language model, with n-gram shallow fusion, and with contextual phrase
// biasing on top of either: one search kernel, template <int F>, instantiated three times.  float32 in both libraries.  The small parts are
// in ctc_beam_common.h, the n-gram model in ngram_lm.h, the phrase automaton in context_bias.h.
//
// Law.  A beam entry is a prefix l with two log-masses: p_b (alignments ending in blank) and p_nb (ending in last(l)); start {(): (0, -inf)}.
// Per consumed frame, with tot = p_b (+) p_nb and (+) = logaddexp:
//   stay:        l   gets p_b' (+)= tot + row[blank], and, if l is not empty, p_nb' (+)= p_nb + row[last(l)]
//   extend by c: l+c gets p_nb' (+)= (c == last(l) ? p_b : tot) + row[c]                      for every c != blank
// Contributions to the same prefix BY CONTENT are combined, the W entries with the largest p_b' (+) p_nb' survive.
//
// Two facts the kernels rely on (DESIGN "CTC prefix beam search"):
//  1. Exact token pruning: per frame it is enough to extend by the W + 1 best non-blank tokens plus, for every live prefix l, every token c
//     for which l+c is itself live.  The second clause is the merge of an extension into a live entry; without it merged mass is lost.
//  2. Prefix identity is by content, not by arena node: l+c can drop out of the beam while l+c+d survives, and a later re-extension of l by c
//     makes a second node for the same prefix.  Prefixes are compared by (length, last token, 64-bit hash).  The hash is a chain of a
//     64-bit bijective mixer (splitmix64's finaliser) over the tokens, so two different prefixes of one length collide with probability
//     about 2^-64 per compared pair; a frame compares at most W^2 = 2^12 pairs, an utterance at most T W^2 <= 2^24: below 2^-40 per utterance
//     at the largest supported shape.
//
// Two passes.  Frame pass: grid over (b, t), one wave per row; the row is read once and its K = min(W + 1, V - 1) best non-blank
// (value, token) pairs go to the workspace in the order (value descending, token ascending).  Search pass: one workgroup of 256 threads per
// utterance, sequential in t, beam state in LDS; per frame it resolves the merges, forms the n (K + 1) candidates (candidate id =
// slot * (K + 1) + r; r = 0: stay, r >= 1: extension by the token of rank r - 1), selects the W best with a 4 x 8-bit radix select on
// the order-preserving integer image of the score and stores them in rank order, so the beam is always sorted.
//
// Tie rule: equal scores are ordered by candidate id, ascending (a function of the inputs alone: slots are in rank order, ranks of tokens
// are (value descending, token ascending)).  Everything is deterministic: no floating-point atomics, no order that depends on scheduling.
//
// The fused law (LM = true; the n-gram scores s are those of ngram_lm.h).  An entry also carries g(l) = sum_i (alpha s(l_i | l_<i) + beta),
// g(()) = 0, and its n-gram context.  Entries are ranked by (p_b (+) p_nb) + g, which is also the returned score; out_lm_score is g.  Stay
// keeps g; extension by c gives g' = g + (alpha s + beta), every operation rounded on its own, so g is a function of the prefix's content
// alone, bit for bit, and the two halves of a merge agree on it.  Token pruning is part of this law (with prefix-dependent scores it is not
// exact any more): a frame extends by its K = min(tokens, V - 1) best non-blank ACOUSTIC tokens plus every c for which l+c is live, merged
// into that entry's stay; the frame pass runs at width wf = max(tokens - 1, 1).  g' of every candidate is kept in LDS.
//
// The biased law (F = BIASED; the phrase automaton and its state (k, tail) are those of context_bias.h).  An entry carries g_lm (the g
// above, +0 throughout when no language model is given: lm_order 0, no lookups) and the automaton state of its prefix, (node, k).  With
// m = k + |tail|, g_b = w (x) float(m) and g = g_lm (+) g_b, one multiply and one add, each rounded on its own; entries are ranked by
// (p_b (+) p_nb) + g during the search, so a partial match that fails loses its credit by itself.  All of it is a function of the
// prefix's content alone, so the two halves of a merge agree on it.  Token pruning is the fused law's: biasing re-ranks among the
// acoustically plausible tokens, it injects none.  Only g_lm' of a candidate is kept in LDS; the automaton state of the <= W selected
// candidates is recomputed in step 5 (the transition is deterministic).  Finalisation: after the last consumed frame the refundable
// credit is taken back, g_fin = g_lm (+) (w (x) float(k)), the n surviving entries are re-ranked by (p_b (+) p_nb) + g_fin (descending,
// ties to the entry that ranked earlier) and the first nbest are emitted with that score, g_lm and k.
#include "context_bias.h"

namespace {

constexpr int ROW_REGS = 16;                        // a row of V <= 64 * 16 floats is held in registers by the frame pass

// (value, token) a precedes (value, token) b in the frame pass's order
__device__ __forceinline__ bool before(float av, int at, float bv, int bt) { return av > bv || (av == bv && at < bt); }

// ---- frame pass: the K best non-blank tokens of every consumed row ----
__global__ __launch_bounds__(256) void ctc_beam_frame_kernel(const float* __restrict__ lp, long long stride_b, long long stride_t,
                                                             const long long* __restrict__ lengths, float* __restrict__ topv,
                                                             int* __restrict__ topt, int T, int V, int blank, int K, int K1) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    if (t >= T) return;
    if (t >= ctc_clamp_len(lengths, b, T)) return;
    const float* row = lp + (long long)b * stride_b + (long long)t * stride_t;
    const bool in_regs = V <= 64 * ROW_REGS;
    float r[ROW_REGS];
    if (in_regs) {
#pragma unroll
        for (int j = 0; j < ROW_REGS; ++j) {
            const int v = lane + 64 * j;
            r[j] = v < V ? row[v] : 0.f;
        }
    }
    float pv = INFINITY;                            // the previous pick: the next one is the first entry strictly after it in the order
    int pt = -1;
    const long long o = ((long long)b * T + t) * K1;
    for (int k = 0; k < K; ++k) {
        float bv = 0.f;
        int bt = 0x7fffffff;                        // none yet
        if (in_regs) {
#pragma unroll
            for (int j = 0; j < ROW_REGS; ++j) {
                const int v = lane + 64 * j;
                const float x = r[j];
                if (v < V && v != blank && before(pv, pt, x, v) && (bt == 0x7fffffff || before(x, v, bv, bt))) { bv = x; bt = v; }
            }
        } else {
            for (int v = lane; v < V; v += 64) {
                const float x = row[v];
                if (v != blank && before(pv, pt, x, v) && (bt == 0x7fffffff || before(x, v, bv, bt))) { bv = x; bt = v; }
            }
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            const float ov = __shfl_xor(bv, s, 64);
            const int ot = __shfl_xor(bt, s, 64);
            if (ot != 0x7fffffff && (bt == 0x7fffffff || before(ov, ot, bv, bt))) { bv = ov; bt = ot; }
        }
        const bool none = bt == 0x7fffffff;         // fewer than K comparable entries (NaN in the row): the rest of the list is empty
        if (lane == 0) { topv[o + k] = none ? -INFINITY : bv; topt[o + k] = none ? -1 : bt; }
        if (none) {
            for (int k2 = k + 1 + lane; k2 < K; k2 += 64) { topv[o + k2] = -INFINITY; topt[o + k2] = -1; }
            break;
        }
        pv = bv; pt = bt;
    }
}

// ---- search pass ----
enum { PLAIN = 0, FUSED = 1, BIASED = 2 };           // the three laws of the header: each holds what the one before it holds

template <int F> struct BeamState {
    float pb[MAXW], pnb[MAXW];
    int last[MAXW], len[MAXW], node[MAXW];
    unsigned long long hash[MAXW];
};
template <> struct BeamState<FUSED> : BeamState<PLAIN> {
    float g[MAXW];
    unsigned long long ctx[MAXW];                   // the n-gram context: the prefix's last N - 1 tokens (ngram_lm.h)
};
template <> struct BeamState<BIASED> : BeamState<FUSED> {
    int bnode[MAXW], bk[MAXW];                      // the phrase automaton's state: the tail's node and the banked credit k
};

// what only the fused search is given: nothing without a language model
template <int F> struct Fusion {};
template <> struct Fusion<FUSED> {
    LmTables lm;                                    // BIASED: lm.order = 0 is "no language model"
    unsigned long long ctx0;                        // the empty prefix's context
    float alpha, beta;
    float* out_g;
};
template <> struct Fusion<BIASED> : Fusion<FUSED> {
    BiasTables bias;
    float w;
    int* out_k;
};

template <int F>
__global__ __launch_bounds__(256) void ctc_beam_search_kernel(const float* __restrict__ lp, long long stride_b, long long stride_t,
                                                              const long long* __restrict__ lengths, const float* __restrict__ topv,
                                                              const int* __restrict__ topt, int* __restrict__ apar, int* __restrict__ atok,
                                                              int* __restrict__ out_ids, int* __restrict__ out_len,
                                                              float* __restrict__ out_score, int T, int V, int blank, int W, int K, int K1,
                                                              int nbest, Fusion<F> f) {
    constexpr bool LM = F >= FUSED, BIAS = F == BIASED;
    __shared__ BeamState<F> st[2];
    __shared__ unsigned keys[MAXCAND];
    __shared__ float tot[MAXW], rlast[MAXW], spb[MAXW], spnb[MAXW], tokv[MAXK];
    __shared__ int tokt[MAXK], parent[MAXW], mrank[MAXW], sel[MAXW], hist[256], wsum[4], pick[2], nvalid;
    __shared__ unsigned selkey[MAXW];
    __shared__ float rblank;
    float* gcand = nullptr;                          // g' of every extension candidate
    if constexpr (LM) { __shared__ float gc[MAXCAND]; gcand = gc; }
    float* gtot = nullptr;                           // g = g_lm (+) g_b of every live entry
    if constexpr (BIAS) { __shared__ float gt[MAXW]; gtot = gt; }
    bool has_lm = LM;
    if constexpr (BIAS) has_lm = f.lm.order > 0;

    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tb = ctc_clamp_len(lengths, b, T);
    const float* base = lp + (long long)b * stride_b;
    const long long tb = (long long)b * T;
    const int C = K + 1;                             // candidates per live entry

    if (tid == 0) {
        st[0].pb[0] = 0.f; st[0].pnb[0] = -INFINITY; st[0].last[0] = -1; st[0].len[0] = 0; st[0].node[0] = -1; st[0].hash[0] = 0;
        if constexpr (LM) { st[0].g[0] = 0.f; st[0].ctx[0] = f.ctx0; }
        if constexpr (BIAS) { st[0].bnode[0] = 0; st[0].bk[0] = 0; }
    }
    int n = 1;
    // the top list of the next frame travels in registers while the current frame is searched
    float nv = -INFINITY;
    int nt = -1;
    if (tid < K && Tb > 0) { nv = topv[tb * K1 + tid]; nt = topt[tb * K1 + tid]; }
    __syncthreads();

    for (int t = 0; t < Tb; ++t) {
        const BeamState<F>& cur = st[t & 1];
        BeamState<F>& nxt = st[(t & 1) ^ 1];
        const float* row = base + (long long)t * stride_t;
        // 1. this frame's inputs
        if (tid < K) { tokv[tid] = nv; tokt[tid] = nt; }
        if (tid < K && t + 1 < Tb) { nv = topv[(tb + t + 1) * K1 + tid]; nt = topt[(tb + t + 1) * K1 + tid]; }
        if (tid >= 64 && tid < 64 + n) {
            const int i = tid - 64, c = cur.last[i];
            rlast[i] = c >= 0 ? row[c] : -INFINITY;
            tot[i] = logaddexp_f(cur.pb[i], cur.pnb[i]);
            parent[i] = -1; mrank[i] = -1;
            if constexpr (BIAS)
                gtot[i] = __fadd_rn(cur.g[i], __fmul_rn(f.w, (float)(cur.bk[i] + bias_depth(f.bias, cur.bnode[i]))));
        }
        if (tid == 128) { rblank = row[blank]; nvalid = 0; }
        __syncthreads();
        // 2. merges by content: entry j is the extension of entry i by last(j)
        for (int p = tid; p < n * n; p += 256) {
            const int j = p / n, i = p - j * n;
            if (cur.len[j] == cur.len[i] + 1 && cur.hash[j] == hash_push(cur.hash[i], cur.last[j])) {
                parent[j] = i;                       // at most one i per j: live prefixes are distinct
                const int c = cur.last[j];
                int r = -1;
                for (int k = 0; k < K; ++k) if (tokt[k] == c) r = k;
                mrank[j] = r;
            }
        }
        __syncthreads();
        // 3. candidate scores: acoustic, + g with a language model
        const int N = n * C;
        for (int q = tid; q < N; q += 256) {
            const int i = q / C, r = q - i * C;
            if (r == 0) {
                const float pb = tot[i] + rblank;
                float pnb = cur.len[i] > 0 ? cur.pnb[i] + rlast[i] : -INFINITY;
                const int pi = parent[i];
                if (pi >= 0) pnb = logaddexp_f(pnb, (cur.last[pi] == cur.last[i] ? cur.pb[pi] : tot[pi]) + rlast[i]);
                spb[i] = pb; spnb[i] = pnb;
                float s = logaddexp_f(pb, pnb);
                if constexpr (BIAS) s = __fadd_rn(s, gtot[i]);
                else if constexpr (LM) s = __fadd_rn(s, cur.g[i]);
                keys[q] = key_of(s);
            } else {
                const int c = tokt[r - 1];
                unsigned k = 0u;
                if (c >= 0) {
                    float s = (c == cur.last[i] ? cur.pb[i] : tot[i]) + tokv[r - 1];
                    if constexpr (LM) {
                        float gq = cur.g[i];
                        if (has_lm) gq = __fadd_rn(gq, __fadd_rn(__fmul_rn(f.alpha, lm_score(f.lm, cur.ctx[i], c)), f.beta));
                        gcand[q] = gq;
                        if constexpr (BIAS) {
                            int nd = cur.bnode[i], kb = cur.bk[i];
                            bias_step(f.bias, nd, kb, c);
                            gq = __fadd_rn(gq, __fmul_rn(f.w, (float)(kb + bias_depth(f.bias, nd))));
                        }
                        s = __fadd_rn(s, gq);
                    }
                    k = key_of(s);
                }
                keys[q] = k;
            }
        }
        __syncthreads();
        if (tid < n && parent[tid] >= 0 && mrank[tid] >= 0) keys[parent[tid] * C + 1 + mrank[tid]] = 0u;      // merged into entry tid's stay
        // 4. the W best keys: radix select and compaction (ctc_beam_common.h)
        const int want = beam_select(keys, N, W, hist, wsum, pick, sel, selkey);
        // 5. rank the selected entries (key descending, candidate id ascending) and store them in that order
        if (tid < want) {
            const unsigned k = selkey[tid];
            const int q = sel[tid];
            int rank = 0;
            for (int u = 0; u < want; ++u) rank += selkey[u] > k || (selkey[u] == k && sel[u] < q);
            if (k != 0u) {
                atomicAdd(&nvalid, 1);
                const int i = q / C, r = q - i * C;
                if (r == 0) {
                    nxt.pb[rank] = spb[i]; nxt.pnb[rank] = spnb[i]; nxt.last[rank] = cur.last[i]; nxt.len[rank] = cur.len[i];
                    nxt.node[rank] = cur.node[i]; nxt.hash[rank] = cur.hash[i];
                    if constexpr (LM) { nxt.g[rank] = cur.g[i]; nxt.ctx[rank] = cur.ctx[i]; }
                    if constexpr (BIAS) { nxt.bnode[rank] = cur.bnode[i]; nxt.bk[rank] = cur.bk[i]; }
                } else {
                    const int c = tokt[r - 1];
                    const long long node = (tb + t) * W + rank;
                    apar[node] = cur.node[i]; atok[node] = c;
                    nxt.pb[rank] = -INFINITY; nxt.pnb[rank] = (c == cur.last[i] ? cur.pb[i] : tot[i]) + tokv[r - 1];   // as in step 3
                    nxt.last[rank] = c; nxt.len[rank] = cur.len[i] + 1;
                    nxt.node[rank] = t * W + rank; nxt.hash[rank] = hash_push(cur.hash[i], c);
                    if constexpr (LM) {
                        nxt.g[rank] = gcand[q];
                        nxt.ctx[rank] = ((cur.ctx[i] << 16) | (unsigned long long)(c + 1)) & f.lm.cmask;
                    }
                    if constexpr (BIAS) {
                        int nd = cur.bnode[i], kb = cur.bk[i];
                        bias_step(f.bias, nd, kb, c);                          // as in step 3
                        nxt.bnode[rank] = nd; nxt.bk[rank] = kb;
                    }
                }
            }
        }
        __syncthreads();
        n = nvalid;                                  // invalid candidates have the lowest key: the valid ones fill slots 0 .. n-1
        __syncthreads();                             // nvalid is reset by the next frame's step 1
    }

    // 6. emit: entries are in rank order; walk the back-pointers of the first nbest
    const BeamState<F>& fin = st[Tb & 1];
    int* ids = out_ids + (long long)b * nbest * T;
    int slot = tid;                                  // where entry tid is emitted
    if constexpr (BIAS) {
        // finalisation: the refundable credit is taken back and the n entries are ranked again, by counting as in step 5
        if (tid < n)
            selkey[tid] = key_of(__fadd_rn(logaddexp_f(fin.pb[tid], fin.pnb[tid]), __fadd_rn(fin.g[tid], __fmul_rn(f.w, (float)fin.bk[tid]))));
        __syncthreads();
        if (tid < n) {
            const unsigned k = selkey[tid];
            slot = 0;
            for (int u = 0; u < n; ++u) slot += selkey[u] > k || (selkey[u] == k && u < tid);
        }
    }
    if (slot < nbest) {
        int len = -1;                                // fewer than nbest hypotheses exist: length -1, score -inf, lm score 0, count 0
        float score = -INFINITY, g = 0.f;
        int kb = 0;
        if (tid < n) {
            len = fin.len[tid];
            score = logaddexp_f(fin.pb[tid], fin.pnb[tid]);
            if constexpr (BIAS) { g = fin.g[tid]; kb = fin.bk[tid]; score = __fadd_rn(score, __fadd_rn(g, __fmul_rn(f.w, (float)kb))); }
            else if constexpr (LM) { g = fin.g[tid]; score = __fadd_rn(score, g); }
            int node = fin.node[tid];
            for (int p = len - 1; p >= 0 && node >= 0; --p) {
                ids[(long long)slot * T + p] = atok[tb * W + node];
                node = apar[tb * W + node];
            }
        }
        out_len[b * nbest + slot] = len;
        out_score[b * nbest + slot] = score;
        if constexpr (LM) f.out_g[b * nbest + slot] = g;
        if constexpr (BIAS) f.out_k[b * nbest + slot] = kb;
        sel[slot] = len;
    }
    __syncthreads();
    for (int x = tid; x < nbest * T; x += 256) {
        const int k = x / T, p = x - k * T;
        if (p >= sel[k]) ids[x] = -1;
    }
}

// The argument checks of the launching entry points, in the order in which their errors are reported: beam_check, then the fused search's
// own arguments, then beam_check_memory.
static int beam_check(const char* who, const float* log_probs, void* workspace, int B, int T, int V, int blank, int beam_width) {
    AV_CHECK(log_probs && workspace, "%s: null pointer", who);
    AV_CHECK(B >= 0 && B <= 65535 && T >= 1 && T <= MAXT && V >= 2, "%s: bad shape B=%d T=%d V=%d (B <= 65535, 1 <= T <= %d, V >= 2)", who, B,
             T, V, MAXT);
    if (int rc = ctc_check_blank(who, blank, V)) return rc;
    AV_CHECK(beam_width >= 1 && beam_width <= MAXW, "%s: beam_width %d outside [1, %d]", who, beam_width, MAXW);
    return AV_OK;
}
static int beam_check_memory(const char* who, bool rows, long long stride_b, long long stride_t, long long workspace_bytes, int B, int T,
                             int V, int beam_width, int wf) {
    AV_CHECK(!rows || ctc_rows_fit(stride_b, stride_t, T, V), "%s: strides (%lld, %lld) overlap rows of [%d][%d][%d]", who,
             stride_b, stride_t, B, T, V);
    const long long need = beam_workspace(B, T, beam_width, wf).total;
    AV_CHECK(workspace_bytes >= need, "%s: workspace of %lld bytes is too small, %lld needed", who, workspace_bytes, need);
    return AV_OK;
}

// the frame pass's width for `tokens` expanded tokens per frame; without a language model the width is W: that is tokens = W + 1
static int frame_width(int tokens) { return tokens - 1 > 1 ? tokens - 1 : 1; }

// the frame pass at width wf, then the search pass over its top lists (K of the wf + 1 of a row are read); arguments checked by the caller
template <int F>
static int beam_launch(const float* log_probs, long long stride_b, long long stride_t, const long long* lengths, int* out_ids, int* out_len,
                       float* out_score, void* workspace, long long workspace_bytes, int B, int T, int V, int blank, int beam_width,
                       int tokens, int nbest, const Fusion<F>& f, void* stream) {
    const int wf = frame_width(tokens), K = tokens < V - 1 ? tokens : V - 1;      // tokens > V - 1: every non-blank token is expanded
    const int rc = av_ctc_beam_frame_pass(log_probs, stride_b, stride_t, lengths, workspace, workspace_bytes, B, T, V, blank, wf, stream);
    if (rc != AV_OK) return rc;
    const BeamWorkspace w = beam_workspace(B, T, beam_width, wf);
    char* ws = (char*)workspace;
    hipLaunchKernelGGL(ctc_beam_search_kernel<F>, dim3(B), dim3(256), 0, (hipStream_t)stream, log_probs, stride_b, stride_t, lengths,
                       (const float*)(ws + w.topv), (const int*)(ws + w.topt), (int*)(ws + w.apar), (int*)(ws + w.atok), out_ids, out_len,
                       out_score, T, V, blank, beam_width, K, wf + 1, nbest, f);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

static int workspace_bytes_of(const char* who, int B, int T, int V, int beam_width, int tokens, long long* bytes) {
    AV_CHECK(bytes, "%s: null pointer", who);
    AV_CHECK(B >= 0 && T >= 1 && T <= MAXT && V >= 2, "%s: bad shape B=%d T=%d V=%d (1 <= T <= %d, V >= 2)", who, B, T, V, MAXT);
    AV_CHECK(beam_width >= 1 && beam_width <= MAXW, "%s: beam_width %d outside [1, %d]", who, beam_width, MAXW);
    AV_CHECK(tokens >= 1 && tokens <= MAXK, "%s: tokens %d outside [1, %d]", who, tokens, MAXK);
    *bytes = beam_workspace(B, T, beam_width, frame_width(tokens)).total;
    return AV_OK;
}

}  // namespace

extern "C" int av_ctc_beam_workspace_bytes(int B, int T, int V, int beam_width, long long* bytes) {
    return workspace_bytes_of("av_ctc_beam_workspace_bytes", B, T, V, beam_width, beam_width + 1, bytes);
}

extern "C" int av_ctc_beam_lm_workspace_bytes(int B, int T, int V, int beam_width, int tokens, long long* bytes) {
    return workspace_bytes_of("av_ctc_beam_lm_workspace_bytes", B, T, V, beam_width, tokens, bytes);
}

extern "C" int av_ctc_beam_frame_pass(const float* log_probs, long long stride_b, long long stride_t, const long long* lengths,
                                      void* workspace, long long workspace_bytes, int B, int T, int V, int blank, int beam_width,
                                      void* stream) {
    const char* who = "av_ctc_beam_frame_pass";
    int rc = beam_check(who, log_probs, workspace, B, T, V, blank, beam_width);
    if (rc == AV_OK) rc = beam_check_memory(who, true, stride_b, stride_t, workspace_bytes, B, T, V, beam_width, beam_width);
    if (rc != AV_OK || B == 0) return rc;
    const BeamWorkspace w = beam_workspace(B, T, beam_width, beam_width);
    const int K1 = beam_width + 1, K = K1 < V - 1 ? K1 : V - 1;      // W + 1 > V - 1: every non-blank token is expanded
    char* ws = (char*)workspace;
    hipLaunchKernelGGL(ctc_beam_frame_kernel, dim3((T + 3) / 4, B), dim3(256), 0, (hipStream_t)stream, log_probs, stride_b, stride_t, lengths,
                       (float*)(ws + w.topv), (int*)(ws + w.topt), T, V, blank, K, K1);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_ctc_beam_search(const float* log_probs, long long stride_b, long long stride_t, const long long* lengths, int* out_ids,
                                  int* out_len, float* out_score, void* workspace, long long workspace_bytes, int B, int T, int V,
                                  int blank, int beam_width, int nbest, void* stream) {
    const char* who = "av_ctc_beam_search";
    AV_CHECK(out_ids && out_len && out_score, "%s: null pointer", who);
    int rc = beam_check(who, log_probs, workspace, B, T, V, blank, beam_width);
    if (rc == AV_OK) rc = beam_check_memory(who, true, stride_b, stride_t, workspace_bytes, B, T, V, beam_width, beam_width);
    if (rc != AV_OK) return rc;
    AV_CHECK(nbest >= 1 && nbest <= beam_width, "%s: nbest %d outside [1, beam_width %d]", who, nbest, beam_width);
    if (B == 0) return AV_OK;
    return beam_launch<PLAIN>(log_probs, stride_b, stride_t, lengths, out_ids, out_len, out_score, workspace, workspace_bytes, B, T, V, blank,
                              beam_width, beam_width + 1, nbest, Fusion<PLAIN>{}, stream);
}

extern "C" int av_ctc_beam_search_lm(const float* log_probs, long long stride_b, long long stride_t, const long long* lengths, int* out_ids,
                                     int* out_len, float* out_score, float* out_lm_score, void* workspace, long long workspace_bytes, int B,
                                     int T, int V, int blank, int beam_width, int nbest, int tokens, const float* lm_unigrams,
                                     const void* lm_table, long long lm_slots, int lm_order, int lm_vocab, int lm_bos, int lm_probe_bound,
                                     float lm_weight, float token_bonus, void* stream) {
    const char* who = "av_ctc_beam_search_lm";
    AV_CHECK(out_ids && out_len && out_score && out_lm_score, "%s: null pointer", who);
    int rc = beam_check(who, log_probs, workspace, B, T, V, blank, beam_width);
    if (rc != AV_OK) return rc;
    AV_CHECK(nbest >= 1 && nbest <= beam_width, "%s: nbest %d outside [1, beam_width %d]", who, nbest, beam_width);
    AV_CHECK(tokens >= 1 && tokens <= MAXK, "%s: tokens %d outside [1, %d]", who, tokens, MAXK);
    AV_CHECK(lm_vocab == V, "%s: the language model's vocabulary %d is not V = %d", who, lm_vocab, V);
    AV_CHECK(lm_weight == lm_weight && token_bonus == token_bonus && fabsf(lm_weight) <= 3.0e38f && fabsf(token_bonus) <= 3.0e38f,
             "%s: lm_weight and token_bonus must be finite", who);
    Fusion<FUSED> f;
    rc = lm_check(who, lm_unigrams, lm_table, lm_slots, lm_order, lm_vocab, lm_bos, lm_probe_bound, &f.lm);
    // rows = false: the strides are left to the frame pass, which reports them after the workspace and not at all for B = 0
    if (rc == AV_OK) rc = beam_check_memory(who, false, stride_b, stride_t, workspace_bytes, B, T, V, beam_width, frame_width(tokens));
    if (rc != AV_OK || B == 0) return rc;
    f.ctx0 = lm_bos >= 0 ? ((unsigned long long)(lm_bos + 1) & f.lm.cmask) : 0ull;
    f.alpha = lm_weight; f.beta = token_bonus; f.out_g = out_lm_score;
    return beam_launch<FUSED>(log_probs, stride_b, stride_t, lengths, out_ids, out_len, out_score, workspace, workspace_bytes, B, T, V, blank,
                             beam_width, tokens, nbest, f, stream);
}

extern "C" int av_ctc_beam_search_bias(const float* log_probs, long long stride_b, long long stride_t, const long long* lengths, int* out_ids,
                                       int* out_len, float* out_score, float* out_lm_score, int* out_bias_count, void* workspace,
                                       long long workspace_bytes, int B, int T, int V, int blank, int beam_width, int nbest, int tokens,
                                       const float* lm_unigrams, const void* lm_table, long long lm_slots, int lm_order, int lm_vocab,
                                       int lm_bos, int lm_probe_bound, float lm_weight, float token_bonus, const void* bias_nodes,
                                       const void* bias_edges, int bias_node_count, long long bias_slots, int bias_probe_bound,
                                       float bias_weight, void* stream) {
    const char* who = "av_ctc_beam_search_bias";
    AV_CHECK(out_ids && out_len && out_score && out_lm_score && out_bias_count, "%s: null pointer", who);
    int rc = beam_check(who, log_probs, workspace, B, T, V, blank, beam_width);
    if (rc != AV_OK) return rc;
    AV_CHECK(nbest >= 1 && nbest <= beam_width, "%s: nbest %d outside [1, beam_width %d]", who, nbest, beam_width);
    AV_CHECK(tokens >= 1 && tokens <= MAXK, "%s: tokens %d outside [1, %d]", who, tokens, MAXK);
    AV_CHECK(bias_weight == bias_weight && fabsf(bias_weight) <= 3.0e38f, "%s: bias_weight must be finite", who);
    Fusion<BIASED> f;
    const bool has_lm = lm_order != 0 || lm_unigrams || lm_table;              // all three absent: no language model, no lookups
    if (has_lm) {
        AV_CHECK(lm_vocab == V, "%s: the language model's vocabulary %d is not V = %d", who, lm_vocab, V);
        AV_CHECK(lm_weight == lm_weight && token_bonus == token_bonus && fabsf(lm_weight) <= 3.0e38f && fabsf(token_bonus) <= 3.0e38f,
                 "%s: lm_weight and token_bonus must be finite", who);
        rc = lm_check(who, lm_unigrams, lm_table, lm_slots, lm_order, lm_vocab, lm_bos, lm_probe_bound, &f.lm);
        if (rc != AV_OK) return rc;
        f.ctx0 = lm_bos >= 0 ? ((unsigned long long)(lm_bos + 1) & f.lm.cmask) : 0ull;
        f.alpha = lm_weight; f.beta = token_bonus;
    } else {
        f.lm = LmTables{nullptr, nullptr, 0ull, 0ull, 0, V, 0};
        f.ctx0 = 0ull; f.alpha = 0.f; f.beta = 0.f;
    }
    rc = bias_check(who, bias_nodes, bias_edges, bias_node_count, bias_slots, bias_probe_bound, V, &f.bias);
    // rows = false: the strides are left to the frame pass, which reports them after the workspace and not at all for B = 0
    if (rc == AV_OK) rc = beam_check_memory(who, false, stride_b, stride_t, workspace_bytes, B, T, V, beam_width, frame_width(tokens));
    if (rc != AV_OK || B == 0) return rc;
    f.out_g = out_lm_score; f.w = bias_weight; f.out_k = out_bias_count;
    return beam_launch<BIASED>(log_probs, stride_b, stride_t, lengths, out_ids, out_len, out_score, workspace, workspace_bytes, B, T, V, blank,
                               beam_width, tokens, nbest, f, stream);
}
