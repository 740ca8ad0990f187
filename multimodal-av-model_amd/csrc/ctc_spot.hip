// CTC keyword spotting on the device: was this phrase said, where, and how sure - K keywords against every utterance of one block of CTC
// log-probs (the posteriors of forward_log_probs for clips, of longform.stitch for recordings).  Lengths and keywords are read from
// DEVICE memory: nothing travels to the host and nothing synchronises.  fp32 throughout (the same code in both libraries); the host path
// of spot.py restates this law and agrees bit for bit - every operation is a float32 max, compare, subtraction or addition in a fixed order.
//
// The law, for utterance b (T_b = input_lengths[b] clamped to [0, T], T without lengths) and keyword y_1..y_L (1 <= L <= 32, no id the
// blank, every id in [0, V)):
//   costs    m[t] = max_v lp[t][v] (a NaN never wins) ; c[t][v] = lp[t][v] - m[t], one subtraction, c <= 0 ; if m[t] is not finite every
//            cost of frame t is -inf.  A path's score is the sum of c along it in frame order: the log-likelihood ratio of the path
//            against the best unconstrained path over the same frames, 0.0 exactly when the path is an argmax path.
//   lattice  S = 2 L - 1 states y_1, blank, y_2, ..., blank, y_L: no leading or trailing blank, a hit starts on the first frame of y_1 and
//            ends on the last frame of y_L.  The skip s-2 -> s exists for even s >= 2 where y differs from the label two states back.
//   walk     each cell carries (d, start); before frame 0 d = -inf and start = -1 everywhere.  At frame t state s sets best = d[t-1][s],
//            takes d[t-1][s-1] only if strictly greater, then the skip predecessor d[t-1][s-2] only if the skip exists and it is strictly
//            greater than the better of those two; state 0 alone then takes a fresh start (0, start = t) only if 0 > best strictly (ties
//            keep the earlier start).  d[t][s] = best + c[t][label_s], start carried from the chosen predecessor.
//            e[t] = d[t][S-1], es[t] = start[t][S-1].
//   hits     a candidate is a frame t < T_b with e[t] > -inf and e[t] >= min_score.  Up to N times: the candidate with the greatest e[t]
//            (ties: the greater t) is reported as (es[t], t + 1, e[t]) and every candidate whose interval [es[u], u + 1) overlaps the
//            reported one is dropped.  Hits come out in the order found: scores descend.
// An invalid keyword (length < 1 after clamping to [0, L_max], an id outside [0, V) or equal to the blank) and T_b = 0 give no hits.
//
// Three kernels, all launched on the caller's stream:
//   ctc_spot_rowmax_kernel   one wavefront per frame row, four rows per workgroup, 16-byte loads where ctc_vec_ok allows: m [B][T].
//   ctc_spot_walk_kernel     one wavefront per (utterance, keyword), lane s = state s; the four wavefronts of a workgroup walk four
//                            keywords of ONE utterance, so their gathers hit the same rows.  (d, start) of s-1 and s-2 arrive by DPP
//                            wave shifts (v_mov_b32_dpp wave_shr:1, a vector-ALU move; the second is the shift of the first): the frame loop
//                            has no LDS access and no barrier.  The emissions of the next 16 frames and their m (one coalesced load by
//                            lanes 0..15) are fetched as one batch of independent loads while the current 16 frames are walked.  Lane S-1's
//                            (d, start) is read out once per frame into lane (t mod 16) and leaves as one coalesced store pair per chunk:
//                            workspace e fp32 / es int32 [B][K][T].
//   ctc_spot_select_kernel   one wavefront per (utterance, keyword): N rounds of a lane-strided argmax over t with the tie rule above, the
//                            chosen intervals kept in registers for the overlap test.  A kernel of its own, so the end series written by
//                            sixteen lanes of the walk are visible to all 64 lanes here without any cache-scope argument; it is tiny.
// Determinism: no atomics, every reduction has a fixed order.  Out-of-range data cannot cause out-of-bounds accesses: T_b is clamped to
// [0, T] and L to [0, L_max]; a bad id ends the keyword before any emission is gathered; frame loads are clamped to T_b - 1.
#include "ctc_common.h"

namespace {

constexpr int SPOT_ROWS = 4;                      // frame rows (wavefronts) per workgroup of the row-max pass
constexpr int SPOT_WAVES = 4;                     // keywords (wavefronts) of one utterance per workgroup
constexpr int SPOT_TCHUNK = 16;                   // frames per batch of loads = end values per coalesced store
constexpr int SPOT_MAXL = 32;                     // ids per keyword: S = 2 L - 1 <= 63 states, one per lane
constexpr int SPOT_MAXN = 8;                      // hits per (utterance, keyword)
constexpr int SPOT_SBATCH = 8;                    // end values a lane of the selection loads per batch

template <bool VEC>
__global__ __launch_bounds__(64 * SPOT_ROWS) void ctc_spot_rowmax_kernel(const float* __restrict__ lp, long long stride_b, long long stride_t,
                                                                         const long long* __restrict__ lengths, int B, int T, int V,
                                                                         float* __restrict__ rowmax) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * SPOT_ROWS + w;
    if (i >= (long long)B * T) return;
    const int b = (int)(i / T), t = (int)(i % T);
    if (t >= ctc_clamp_len(lengths, b, T)) return;                    // never read by the walk
    const float* row = lp + (long long)b * stride_b + (long long)t * stride_t;
    float best = -INFINITY;                                           // x > best: a NaN never wins
    if (VEC) {
        const f32x4* p = (const f32x4*)row;
        const int n = V >> 2;
#pragma unroll 4
        for (int c = lane; c < n; c += AV_WAVE) {
            const f32x4 v = p[c];
            if (v.x > best) best = v.x;
            if (v.y > best) best = v.y;
            if (v.z > best) best = v.z;
            if (v.w > best) best = v.w;
        }
    } else {
#pragma unroll 4
        for (int c = lane; c < V; c += AV_WAVE) {
            const float x = row[c];
            if (x > best) best = x;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        if (ob > best) best = ob;
    }
    if (lane == 0) rowmax[i] = best;
}

// the value of lane - 1 (lane 0: `edge`): a DPP wave shift, a vector-ALU move - no LDS crossbar, no wait
__device__ __forceinline__ float spot_shr1(float v, float edge) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, edge), __builtin_bit_cast(int, v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ int spot_shr1(int v, int edge) { return __builtin_amdgcn_update_dpp(edge, v, 0x138, 0xf, 0xf, false); }

// Keyword k for one wavefront -> its number of states S = 2 L - 1 (the same in every lane), 0 for an invalid keyword; lab = the class of
// this lane's state (a lane without a state holds the blank, a valid column), skip = its transition from two states back exists.
__device__ __forceinline__ int spot_keyword(const int* __restrict__ keywords, long long kw_ld, const int* __restrict__ kw_lengths, int k, int L_max,
                                            int V, int blank, int lane, int& lab, bool& skip) {
    const int L = ctc_clamp_len((long long)kw_lengths[k], L_max);
    const int S = 2 * L - 1;
    const bool label = !(lane & 1) && lane < S;
    const int y = label ? keywords[(long long)k * kw_ld + (lane >> 1)] : blank;
    const bool bad = label && (y < 0 || y >= V || y == blank);
    lab = bad ? blank : y;
    const int y2 = __shfl_up(lab, 2, 64);                            // once per keyword
    skip = label && lane >= 2 && y2 != lab;
    return (L < 1 || __ballot(bad) != 0ull) ? 0 : S;
}

__global__ __launch_bounds__(64 * SPOT_WAVES) void ctc_spot_walk_kernel(const float* __restrict__ lp, long long stride_b, long long stride_t,
                                                                        const long long* __restrict__ lengths,
                                                                        const int* __restrict__ keywords, long long kw_ld,
                                                                        const int* __restrict__ kw_lengths, int T, int V, int K, int L_max,
                                                                        int blank, int kblocks, const float* __restrict__ rowmax,
                                                                        float* __restrict__ end_score, int* __restrict__ end_start) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = (int)(blockIdx.x / (unsigned)kblocks);
    const int k = (int)(blockIdx.x % (unsigned)kblocks) * SPOT_WAVES + w;
    if (k >= K) return;                                               // no barrier below: a wavefront may leave
    const int Tb = ctc_clamp_len(lengths, b, T);
    int lab;
    bool skip;
    const int S = spot_keyword(keywords, kw_ld, kw_lengths, k, L_max, V, blank, lane, lab, skip);
    if (S == 0 || Tb == 0) return;
    const int last = __builtin_amdgcn_readfirstlane(S - 1);
    const float* col = lp + (long long)b * stride_b + lab;            // this state's column
    const float* mrow = rowmax + (long long)b * T;
    float* eo = end_score + ((long long)b * K + k) * T;
    int* so = end_start + ((long long)b * K + k) * T;
    float d = -INFINITY;
    int st = -1;
    float ev[SPOT_TCHUNK], nev[SPOT_TCHUNK], mm, nmm = 0.f;
#pragma unroll
    for (int i = 0; i < SPOT_TCHUNK; ++i) ev[i] = col[(long long)min(i, Tb - 1) * stride_t];     // clamped: unused past the end, never out of bounds
    mm = mrow[min(lane & (SPOT_TCHUNK - 1), Tb - 1)];
    for (long long t0 = 0; t0 < Tb; t0 += SPOT_TCHUNK) {
        if (t0 + SPOT_TCHUNK < Tb) {                                  // the next chunk: independent loads, in flight during this chunk's walk
#pragma unroll
            for (int i = 0; i < SPOT_TCHUNK; ++i) nev[i] = col[min(t0 + SPOT_TCHUNK + i, (long long)Tb - 1) * stride_t];
            nmm = mrow[min(t0 + SPOT_TCHUNK + (lane & (SPOT_TCHUNK - 1)), (long long)Tb - 1)];
        } else {
#pragma unroll
            for (int i = 0; i < SPOT_TCHUNK; ++i) nev[i] = 0.f;
        }
        float ke = -INFINITY;
        int ks = -1;
#pragma unroll
        for (int i = 0; i < SPOT_TCHUNK; ++i) {                       // frames past T_b - 1 walk on clamped loads; nothing of them is stored
            const float m = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mm), i));
            float c = ev[i] - m;
            if (!(fabsf(m) < INFINITY)) c = -INFINITY;
            const float p1 = spot_shr1(d, -INFINITY);
            const int s1 = spot_shr1(st, -1);
            const float p2 = spot_shr1(p1, -INFINITY);
            const int s2 = spot_shr1(s1, -1);
            float best = d;
            int bs = st;
            if (p1 > best) { best = p1; bs = s1; }
            if (skip && p2 > best) { best = p2; bs = s2; }
            if (lane == 0 && 0.f > best) { best = 0.f; bs = (int)t0 + i; }
            d = best + c;
            st = bs;
            const float le = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, d), last));
            const int ls = __builtin_amdgcn_readlane(st, last);
            if (lane == i) { ke = le; ks = ls; }
        }
        if (lane < SPOT_TCHUNK && t0 + lane < Tb) {
            eo[t0 + lane] = ke;
            so[t0 + lane] = ks;
        }
#pragma unroll
        for (int i = 0; i < SPOT_TCHUNK; ++i) ev[i] = nev[i];
        mm = nmm;
    }
}

// (e, t) beats (be, bt): the greater score, ties to the greater frame; bt = -1 is "none" and loses to every candidate (e > -inf)
__device__ __forceinline__ bool spot_beats(float e, long long t, float be, long long bt) { return t >= 0 && (bt < 0 || e > be || (e == be && t > bt)); }

__global__ __launch_bounds__(64 * SPOT_WAVES) void ctc_spot_select_kernel(const long long* __restrict__ lengths, const int* __restrict__ keywords,
                                                                          long long kw_ld, const int* __restrict__ kw_lengths, int T, int V,
                                                                          int K, int L_max, int blank, int kblocks, int N, float min_score,
                                                                          const float* __restrict__ end_score,
                                                                          const int* __restrict__ end_start, int* __restrict__ out_hits,
                                                                          float* __restrict__ out_scores, int* __restrict__ out_counts) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = (int)(blockIdx.x / (unsigned)kblocks);
    const int k = (int)(blockIdx.x % (unsigned)kblocks) * SPOT_WAVES + w;
    if (k >= K) return;
    const int Tb = ctc_clamp_len(lengths, b, T);
    int lab;
    bool skip;
    const int S = spot_keyword(keywords, kw_ld, kw_lengths, k, L_max, V, blank, lane, lab, skip);
    const long long bk = (long long)b * K + k;
    const float* e = end_score + bk * T;
    const int* es = end_start + bk * T;
    int ha[SPOT_MAXN], hb[SPOT_MAXN];                                // the reported intervals [ha, hb)
    int count = 0;
    bool open = S != 0;                                              // an invalid keyword's end series were never written
#pragma unroll
    for (int r = 0; r < SPOT_MAXN; ++r) {
        ha[r] = hb[r] = -1;
        if (open && r < N) {
            float be = -INFINITY;
            long long bt = -1;
            int ba = -1;
            for (long long t0 = lane; t0 < Tb; t0 += AV_WAVE * SPOT_SBATCH) {
                float x[SPOT_SBATCH];                                // independent loads, all in flight before the first is used
                int a[SPOT_SBATCH];
#pragma unroll
                for (int u = 0; u < SPOT_SBATCH; ++u) {
                    const long long t = t0 + AV_WAVE * u;
                    x[u] = t < Tb ? e[t] : -INFINITY;                // -inf is no candidate
                    a[u] = t < Tb ? es[t] : -1;
                }
#pragma unroll
                for (int u = 0; u < SPOT_SBATCH; ++u) {              // ascending t, as a plain loop over this lane's frames
                    const long long t = t0 + AV_WAVE * u;
                    bool cand = x[u] > -INFINITY && x[u] >= min_score;
#pragma unroll
                    for (int j = 0; j < r; ++j) cand = cand && !(a[u] < hb[j] && ha[j] < t + 1);
                    if (cand && spot_beats(x[u], t, be, bt)) { be = x[u]; bt = t; ba = a[u]; }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float oe = __shfl_xor(be, o, 64);
                const int ot = __shfl_xor((int)bt, o, 64);
                const int oa = __shfl_xor(ba, o, 64);
                if (spot_beats(oe, ot, be, bt)) { be = oe; bt = ot; ba = oa; }
            }
            if (bt < 0) {
                open = false;                                        // the same in every lane
            } else {
                ha[r] = ba;
                hb[r] = (int)bt + 1;
                if (lane == 0) {
                    out_hits[(bk * N + r) * 2] = ba;
                    out_hits[(bk * N + r) * 2 + 1] = (int)bt + 1;
                    out_scores[bk * N + r] = be;
                }
                count = r + 1;
            }
        }
    }
    if (lane < N && lane >= count) {
        out_hits[(bk * N + lane) * 2] = -1;
        out_hits[(bk * N + lane) * 2 + 1] = -1;
        out_scores[bk * N + lane] = -INFINITY;
    }
    if (lane == 0) out_counts[bk] = count;
}

long long spot_ws_bytes(int B, int T, int K) { return 4LL * B * T * (1LL + 2LL * K); }

}  // namespace

extern "C" int av_ctc_spot_workspace_bytes(int B, int T, int K, long long* bytes) {
    AV_CHECK(bytes, "av_ctc_spot_workspace_bytes: null pointer");
    AV_CHECK(B >= 1 && T >= 1 && K >= 1, "av_ctc_spot_workspace_bytes: bad shape B=%d T=%d K=%d (all >= 1)", B, T, K);
    *bytes = spot_ws_bytes(B, T, K);
    return AV_OK;
}

extern "C" int av_ctc_spot(const float* log_probs, long long stride_b, long long stride_t, const long long* input_lengths, const int* keywords,
                           long long kw_ld, const int* kw_lengths, int B, int T, int V, int K, int L_max, int blank, int N, float min_score,
                           int* out_hits, float* out_scores, int* out_counts, void* workspace, long long workspace_bytes, void* stream) {
    AV_CHECK(log_probs && keywords && kw_lengths && out_hits && out_scores && out_counts && workspace, "av_ctc_spot: null pointer");
    AV_CHECK(B >= 1 && T >= 1 && V >= 1 && K >= 1, "av_ctc_spot: bad shape B=%d T=%d V=%d K=%d (all >= 1)", B, T, V, K);
    if (int rc = ctc_check_blank("av_ctc_spot", blank, V)) return rc;
    AV_CHECK(L_max >= 1 && L_max <= SPOT_MAXL, "av_ctc_spot: L_max %d outside [1, %d]", L_max, SPOT_MAXL);
    AV_CHECK(kw_ld >= L_max, "av_ctc_spot: kw_ld %lld < L_max %d", kw_ld, L_max);
    AV_CHECK(N >= 1 && N <= SPOT_MAXN, "av_ctc_spot: N = %d hits per keyword outside [1, %d]", N, SPOT_MAXN);
    AV_CHECK(min_score == min_score, "av_ctc_spot: min_score is NaN");
    if (int rc = ctc_check_rows("av_ctc_spot", stride_b, stride_t, B, T, V, true, "btBT")) return rc;
    const long long need = spot_ws_bytes(B, T, K);
    AV_CHECK(workspace_bytes >= need, "av_ctc_spot: workspace of %lld bytes is too small, %lld needed", workspace_bytes, need);
    AV_CHECK((uintptr_t)workspace % sizeof(float) == 0, "av_ctc_spot: workspace must be 4-byte aligned");
    const int kblocks = av_cdiv(K, SPOT_WAVES);
    const long long rows = (long long)B * T, row_blocks = (rows + SPOT_ROWS - 1) / SPOT_ROWS, walk_blocks = (long long)B * kblocks;
    AV_CHECK(row_blocks <= 0x7fffffffLL && walk_blocks <= 0x7fffffffLL, "av_ctc_spot: B=%d T=%d K=%d needs more workgroups than one launch holds", B,
             T, K);
    float* rowmax = (float*)workspace;
    float* end_score = rowmax + rows;
    int* end_start = (int*)(end_score + rows * K);
    if (ctc_vec_ok(log_probs, nullptr, stride_b, stride_t, V))
        hipLaunchKernelGGL(ctc_spot_rowmax_kernel<true>, dim3((unsigned)row_blocks), dim3(64 * SPOT_ROWS), 0, (hipStream_t)stream, log_probs,
                           stride_b, stride_t, input_lengths, B, T, V, rowmax);
    else
        hipLaunchKernelGGL(ctc_spot_rowmax_kernel<false>, dim3((unsigned)row_blocks), dim3(64 * SPOT_ROWS), 0, (hipStream_t)stream, log_probs,
                           stride_b, stride_t, input_lengths, B, T, V, rowmax);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ctc_spot_walk_kernel, dim3((unsigned)walk_blocks), dim3(64 * SPOT_WAVES), 0, (hipStream_t)stream, log_probs, stride_b,
                       stride_t, input_lengths, keywords, kw_ld, kw_lengths, T, V, K, L_max, blank, kblocks, rowmax, end_score, end_start);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(ctc_spot_select_kernel, dim3((unsigned)walk_blocks), dim3(64 * SPOT_WAVES), 0, (hipStream_t)stream, input_lengths, keywords,
                       kw_ld, kw_lengths, T, V, K, L_max, blank, kblocks, N, min_score, end_score, end_start, out_hits, out_scores, out_counts);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
