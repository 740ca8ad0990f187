// CTC prefix beam search with n-gram language-model shallow fusion on the device, and batched n-gram scoring (lm.py: NGramLM).
// float32 in both libraries.  ctc_beam.hip is the search without a language model; its frame pass is reused, its search kernel is not touched.
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
//
// The fused law.  An entry carries the acoustic p_b, p_nb of ctc_beam.hip and g(l) = sum_i (alpha s(l_i | l_<i) + beta), g(()) = 0.  Entries
// are ranked by (p_b (+) p_nb) + g, which is also the returned score; out_lm_score is g.  Stay keeps g; extension by c gives
// g' = g + (alpha s + beta), every operation rounded on its own, so g is a function of the prefix's content alone, bit for bit, and the two
// halves of a merge agree on it.  Token pruning is part of the law (with prefix-dependent scores it is not exact any more): a frame extends
// by its K = min(tokens, V - 1) best non-blank ACOUSTIC tokens plus every c for which l+c is live, merged into that entry's stay.
// Tie rule, radix select, arena, emission, length clamping and NaN handling are those of ctc_beam.hip.  The acoustic mass of a new extension
// is recomputed for the survivors (the key holds acoustic + g); g' of every candidate is kept in LDS.
#include "ctc_beam_common.h"

namespace {

struct LmTables {
    const float* uni;                               // [V + 1][2]
    const uint4* tab;                               // [slots] {key lo, key hi, logp, backoff}
    unsigned long long smask, cmask;                // slots - 1; mask of the N - 1 context fields
    int order, V, probe;
};

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ bool lm_find(const LmTables& lm, unsigned long long key, float& logp, float& backoff) {
    unsigned long long i = splitmix64(key) & lm.smask;
    for (int p = 0; p < lm.probe; ++p) {
        const uint4 s = lm.tab[i];
        const unsigned long long k = (unsigned long long)s.x | ((unsigned long long)s.y << 32);
        if (k == key) { logp = __uint_as_float(s.z); backoff = __uint_as_float(s.w); return true; }
        if (k == 0ull) return false;
        i = (i + 1) & lm.smask;
    }
    return false;
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

// ---- batched scoring: one thread per token ----
__global__ __launch_bounds__(256) void ngram_score_kernel(const int* __restrict__ ids, const long long* __restrict__ lens,
                                                          float* __restrict__ out, int B, int Lmax, LmTables lm, int bos) {
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x >= (long long)B * Lmax) return;
    const int b = (int)(x / Lmax), i = (int)(x - (long long)b * Lmax);
    const int len = lens ? (int)min(max(lens[b], 0ll), (long long)Lmax) : Lmax;
    if (i >= len) { out[x] = 0.f; return; }
    const int* row = ids + (long long)b * Lmax;
    const int have = min(i, lm.order - 1);
    unsigned long long ctx = (have < lm.order - 1 && bos >= 0) ? (unsigned long long)(bos + 1) : 0ull;
    for (int j = i - have; j < i; ++j) {
        const int w = row[j];
        ctx = (ctx << 16) | (w >= 0 && w < lm.V ? (unsigned long long)(w + 1) : 0xffffull);       // 0xffff is no token's field: it matches nothing
    }
    ctx &= lm.cmask;
    const int c = row[i];
    out[x] = c >= 0 && c < lm.V ? lm_score(lm, ctx, c) : __uint_as_float(0x7fc00000u);
}

// ---- fused search pass ----
struct BeamStateLm {
    float pb[MAXW], pnb[MAXW], g[MAXW];
    int last[MAXW], len[MAXW], node[MAXW];
    unsigned long long hash[MAXW], ctx[MAXW];
};

__global__ __launch_bounds__(256) void ctc_beam_search_lm_kernel(const float* __restrict__ lp, long long stride_b, long long stride_t,
                                                                 const long long* __restrict__ lengths, const float* __restrict__ topv,
                                                                 const int* __restrict__ topt, int* __restrict__ apar, int* __restrict__ atok,
                                                                 int* __restrict__ out_ids, int* __restrict__ out_len,
                                                                 float* __restrict__ out_score, float* __restrict__ out_lm, int T, int V,
                                                                 int blank, int W, int K, int K1, int nbest, LmTables lm,
                                                                 unsigned long long ctx0, float alpha, float beta) {
    __shared__ BeamStateLm st[2];
    __shared__ unsigned keys[MAXCAND];
    __shared__ float gcand[MAXCAND];                 // g' of every extension candidate
    __shared__ float tot[MAXW], rlast[MAXW], spb[MAXW], spnb[MAXW], tokv[MAXK];
    __shared__ int tokt[MAXK], parent[MAXW], mrank[MAXW], sel[MAXW], hist[256], wsum[4], pick[2], nvalid;
    __shared__ unsigned selkey[MAXW];
    __shared__ float rblank;

    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tb = lengths ? (int)min(max(lengths[b], 0ll), (long long)T) : T;
    const float* base = lp + (long long)b * stride_b;
    const long long tb = (long long)b * T;
    const int C = K + 1;                             // candidates per live entry

    if (tid == 0) {
        st[0].pb[0] = 0.f; st[0].pnb[0] = -INFINITY; st[0].g[0] = 0.f; st[0].last[0] = -1; st[0].len[0] = 0; st[0].node[0] = -1;
        st[0].hash[0] = 0; st[0].ctx[0] = ctx0;
    }
    int n = 1;
    float nv = -INFINITY;
    int nt = -1;
    if (tid < K && Tb > 0) { nv = topv[tb * K1 + tid]; nt = topt[tb * K1 + tid]; }
    __syncthreads();

    for (int t = 0; t < Tb; ++t) {
        const BeamStateLm& cur = st[t & 1];
        BeamStateLm& nxt = st[(t & 1) ^ 1];
        const float* row = base + (long long)t * stride_t;
        // 1. this frame's inputs
        if (tid < K) { tokv[tid] = nv; tokt[tid] = nt; }
        if (tid < K && t + 1 < Tb) { nv = topv[(tb + t + 1) * K1 + tid]; nt = topt[(tb + t + 1) * K1 + tid]; }
        if (tid >= 64 && tid < 64 + n) {
            const int i = tid - 64, c = cur.last[i];
            rlast[i] = c >= 0 ? row[c] : -INFINITY;
            tot[i] = logaddexp_f(cur.pb[i], cur.pnb[i]);
            parent[i] = -1; mrank[i] = -1;
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
        // 3. candidate scores: acoustic + g
        const int N = n * C;
        for (int q = tid; q < N; q += 256) {
            const int i = q / C, r = q - i * C;
            if (r == 0) {
                const float pb = tot[i] + rblank;
                float pnb = cur.len[i] > 0 ? cur.pnb[i] + rlast[i] : -INFINITY;
                const int pi = parent[i];
                if (pi >= 0) pnb = logaddexp_f(pnb, (cur.last[pi] == cur.last[i] ? cur.pb[pi] : tot[pi]) + rlast[i]);
                spb[i] = pb; spnb[i] = pnb;
                keys[q] = key_of(__fadd_rn(logaddexp_f(pb, pnb), cur.g[i]));
            } else {
                const int c = tokt[r - 1];
                unsigned k = 0u;
                if (c >= 0) {
                    const float am = (c == cur.last[i] ? cur.pb[i] : tot[i]) + tokv[r - 1];
                    const float gq = __fadd_rn(cur.g[i], __fadd_rn(__fmul_rn(alpha, lm_score(lm, cur.ctx[i], c)), beta));
                    gcand[q] = gq;
                    k = key_of(__fadd_rn(am, gq));
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
                    nxt.pb[rank] = spb[i]; nxt.pnb[rank] = spnb[i]; nxt.g[rank] = cur.g[i]; nxt.last[rank] = cur.last[i];
                    nxt.len[rank] = cur.len[i]; nxt.node[rank] = cur.node[i]; nxt.hash[rank] = cur.hash[i]; nxt.ctx[rank] = cur.ctx[i];
                } else {
                    const int c = tokt[r - 1];
                    const long long node = (tb + t) * W + rank;
                    apar[node] = cur.node[i]; atok[node] = c;
                    nxt.pb[rank] = -INFINITY; nxt.pnb[rank] = (c == cur.last[i] ? cur.pb[i] : tot[i]) + tokv[r - 1];   // as in step 3
                    nxt.g[rank] = gcand[q]; nxt.last[rank] = c; nxt.len[rank] = cur.len[i] + 1;
                    nxt.node[rank] = t * W + rank; nxt.hash[rank] = hash_push(cur.hash[i], c);
                    nxt.ctx[rank] = ((cur.ctx[i] << 16) | (unsigned long long)(c + 1)) & lm.cmask;
                }
            }
        }
        __syncthreads();
        n = nvalid;                                  // invalid candidates have the lowest key: the valid ones fill slots 0 .. n-1
        __syncthreads();                             // nvalid is reset by the next frame's step 1
    }

    // 6. emit: entries are in rank order; walk the back-pointers of the first nbest
    const BeamStateLm& fin = st[Tb & 1];
    int* ids = out_ids + (long long)b * nbest * T;
    if (tid < nbest) {
        int len = -1;                                // fewer than nbest hypotheses exist: length -1, score -inf, lm score 0
        float score = -INFINITY, g = 0.f;
        if (tid < n) {
            len = fin.len[tid];
            g = fin.g[tid];
            score = __fadd_rn(logaddexp_f(fin.pb[tid], fin.pnb[tid]), g);
            int node = fin.node[tid];
            for (int p = len - 1; p >= 0 && node >= 0; --p) {
                ids[(long long)tid * T + p] = atok[tb * W + node];
                node = apar[tb * W + node];
            }
        }
        out_len[b * nbest + tid] = len;
        out_score[b * nbest + tid] = score;
        out_lm[b * nbest + tid] = g;
        sel[tid] = len;
    }
    __syncthreads();
    for (int x = tid; x < nbest * T; x += 256) {
        const int k = x / T, p = x - k * T;
        if (p >= sel[k]) ids[x] = -1;
    }
}

// workspace of the fused search: the frame pass's top lists at its own width wf = max(tokens - 1, 1) in the layout of beam_workspace(wf),
// then the arena int32 [B][T][W] x 2 where that layout has its own (sized for the larger of the two, so that the frame pass accepts it)
struct LmWorkspace {
    long long wf, topt, apar, atok, total;
};
static LmWorkspace lm_workspace(long long B, long long T, long long W, long long tokens) {
    LmWorkspace w;
    w.wf = tokens - 1 > 1 ? tokens - 1 : 1;
    const BeamWorkspace f = beam_workspace(B, T, w.wf);
    w.topt = f.topt; w.apar = f.apar; w.atok = f.apar + B * T * W * 4;
    w.total = f.apar + 2 * B * T * (W > w.wf ? W : w.wf) * 4;
    return w;
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

extern "C" int av_ngram_score(const int* ids, const long long* lens, float* out, int B, int Lmax, const float* lm_unigrams, const void* lm_table,
                              long long lm_slots, int lm_order, int lm_vocab, int lm_bos, int lm_probe_bound, void* stream) {
    AV_CHECK(ids && out, "av_ngram_score: null pointer");
    AV_CHECK(B >= 0 && Lmax >= 1 && (long long)B * Lmax <= (1ll << 31) * 255, "av_ngram_score: bad shape B=%d Lmax=%d", B, Lmax);
    LmTables lm;
    const int rc = lm_check("av_ngram_score", lm_unigrams, lm_table, lm_slots, lm_order, lm_vocab, lm_bos, lm_probe_bound, &lm);
    if (rc != AV_OK) return rc;
    if (B == 0) return AV_OK;
    hipLaunchKernelGGL(ngram_score_kernel, dim3(av_cdiv((long long)B * Lmax, 256)), dim3(256), 0, (hipStream_t)stream, ids, lens, out, B, Lmax,
                       lm, lm_bos);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_ctc_beam_lm_workspace_bytes(int B, int T, int V, int beam_width, int tokens, long long* bytes) {
    AV_CHECK(bytes, "av_ctc_beam_lm_workspace_bytes: null pointer");
    AV_CHECK(B >= 0 && T >= 1 && T <= MAXT && V >= 2, "av_ctc_beam_lm_workspace_bytes: bad shape B=%d T=%d V=%d (1 <= T <= %d, V >= 2)", B, T, V, MAXT);
    AV_CHECK(beam_width >= 1 && beam_width <= MAXW, "av_ctc_beam_lm_workspace_bytes: beam_width %d outside [1, %d]", beam_width, MAXW);
    AV_CHECK(tokens >= 1 && tokens <= MAXK, "av_ctc_beam_lm_workspace_bytes: tokens %d outside [1, %d]", tokens, MAXK);
    *bytes = lm_workspace(B, T, beam_width, tokens).total;
    return AV_OK;
}

extern "C" int av_ctc_beam_search_lm(const float* log_probs, long long stride_b, long long stride_t, const long long* lengths, int* out_ids,
                                     int* out_len, float* out_score, float* out_lm_score, void* workspace, long long workspace_bytes, int B,
                                     int T, int V, int blank, int beam_width, int nbest, int tokens, const float* lm_unigrams,
                                     const void* lm_table, long long lm_slots, int lm_order, int lm_vocab, int lm_bos, int lm_probe_bound,
                                     float lm_weight, float token_bonus, void* stream) {
    const char* who = "av_ctc_beam_search_lm";
    AV_CHECK(log_probs && workspace && out_ids && out_len && out_score && out_lm_score, "%s: null pointer", who);
    AV_CHECK(B >= 0 && B <= 65535 && T >= 1 && T <= MAXT && V >= 2, "%s: bad shape B=%d T=%d V=%d (B <= 65535, 1 <= T <= %d, V >= 2)", who, B,
             T, V, MAXT);
    AV_CHECK(blank >= 0 && blank < V, "%s: blank %d outside [0, %d)", who, blank, V);
    AV_CHECK(beam_width >= 1 && beam_width <= MAXW, "%s: beam_width %d outside [1, %d]", who, beam_width, MAXW);
    AV_CHECK(nbest >= 1 && nbest <= beam_width, "%s: nbest %d outside [1, beam_width %d]", who, nbest, beam_width);
    AV_CHECK(tokens >= 1 && tokens <= MAXK, "%s: tokens %d outside [1, %d]", who, tokens, MAXK);
    AV_CHECK(lm_vocab == V, "%s: the language model's vocabulary %d is not V = %d", who, lm_vocab, V);
    AV_CHECK(lm_weight == lm_weight && token_bonus == token_bonus && fabsf(lm_weight) <= 3.0e38f && fabsf(token_bonus) <= 3.0e38f,
             "%s: lm_weight and token_bonus must be finite", who);
    LmTables lm;
    int rc = lm_check(who, lm_unigrams, lm_table, lm_slots, lm_order, lm_vocab, lm_bos, lm_probe_bound, &lm);
    if (rc != AV_OK) return rc;
    const LmWorkspace w = lm_workspace(B, T, beam_width, tokens);
    AV_CHECK(workspace_bytes >= w.total, "%s: workspace of %lld bytes is too small, %lld needed", who, workspace_bytes, w.total);
    if (B == 0) return AV_OK;
    // the top lists: the frame pass of ctc_beam.hip at width wf writes wf + 1 = K1 entries per row, of which the first K are read (strides checked there)
    rc = av_ctc_beam_frame_pass(log_probs, stride_b, stride_t, lengths, workspace, workspace_bytes, B, T, V, blank, (int)w.wf, stream);
    if (rc != AV_OK) return rc;
    const int K1 = (int)w.wf + 1, K = tokens < V - 1 ? tokens : V - 1;
    char* ws = (char*)workspace;
    const unsigned long long ctx0 = lm_bos >= 0 ? ((unsigned long long)(lm_bos + 1) & lm.cmask) : 0ull;
    hipLaunchKernelGGL(ctc_beam_search_lm_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, log_probs, stride_b, stride_t, lengths,
                       (const float*)ws, (const int*)(ws + w.topt), (int*)(ws + w.apar), (int*)(ws + w.atok), out_ids, out_len, out_score,
                       out_lm_score, T, V, blank, beam_width, K, K1, nbest, lm, ctx0, lm_weight, token_bonus);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
