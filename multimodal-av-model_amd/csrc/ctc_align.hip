// CTC forced alignment on the device: the best frame path (Viterbi) of a given transcript through the CTC lattice, the frames each target
// position occupies and their scores - "when" to the loss's "how likely" (the log-probs and lengths of model/trainer.py:116-117, 229-242).
// Lengths and labels are read from DEVICE memory: nothing travels to the host and nothing synchronises.  fp32 throughout (the same code in
// both libraries); the host path of align.py restates this law and agrees bit for bit.
//
// Lattice: extended label row l' of S = 2 L + 1 states (blank, l1, blank, ..., lL, blank); the skip s-2 -> s exists where l'_s != l'_{s-2}.
//   d[0][0] = lp[0][blank], d[0][1] = lp[0][l1], the rest -inf
//   d[t][s] = max(d[t-1][s], d[t-1][s-1], skip ? d[t-1][s-2] : -inf) + lp[t][l'_s]            one max, one add per cell, nothing else
//   move[t][s]: ties go to the smaller move - 1 only if d[t-1][s-1] > d[t-1][s] strictly, 2 only if d[t-1][s-2] > the better of those two
//   final state S-1 if d[T_b-1][S-1] > d[T_b-1][S-2] strictly, else S-2 (S = 1: state 0); the score is d[T_b-1][final]
// An utterance is infeasible (score -inf, states and spans -1, token scores 0) if a label is outside [0, V) or equal to the blank (its path
// could not collapse to the target) or if the final score is -inf (too few frames, -inf emissions on every path).  T_b = 0 with L_b = 0 is
// feasible with score 0 and an empty path.
//
// ctc_align_kernel, one workgroup per utterance, three phases:
//   forward     the walk of ctc_lattice_kernel (csrc/ctc_loss.hip) with max for log-sum-exp: previous row ping-ponged in LDS, the S gathered
//               emissions of the next 16 frames staged by one batch of independent loads.  The 16 moves of a state within such a chunk are
//               packed two bits each into one register and leave as ONE coalesced 4-byte store per state and chunk: workspace
//               [B][ceil(T / 16)][S_max] words.
//   back-trace  the only serial part.  The move words of 256 frames (16 chunk rows) are pulled into LDS by one batch of coalesced loads,
//               then one lane walks them: a dependent LDS read per frame instead of a dependent global load.  The path stays in LDS.
//   outputs     in parallel over frames: out_state, and the first / end frame of each label state's run (on a feasible path every label
//               state is visited and its run is contiguous); then one thread per target position adds its emissions in frame order.
// Determinism: no atomics, every sum has a fixed order.  Out-of-range data cannot cause out-of-bounds accesses: T_b is clamped to [0, T],
// L_b to [0, Lmax], a bad label ends the item before any emission is gathered, and the walk clamps its state at 0.
#include "ctc_common.h"

namespace {

constexpr int ALN_TCHUNK = 16;                    // frames per staged batch of emissions = moves per packed word (2 bits each)
constexpr int ALN_BT_ROWS = 16;                   // chunk rows of move words staged per back-trace batch (the emission buffer, reused)
constexpr int ALN_MAXTRIP = 4;                    // trips of the state loop at 256 threads: S_max <= 1024 (the LDS limit allows 818)
constexpr int ALN_MAXT = 4096;

__host__ __device__ __forceinline__ long long aln_chunks(int T) { return (T + ALN_TCHUNK - 1) / ALN_TCHUNK; }

__global__ __launch_bounds__(256) void ctc_align_kernel(const float* __restrict__ lp, long long stride_b, long long stride_t,
                                                        const long long* __restrict__ targets, long long target_ld,
                                                        const long long* __restrict__ input_lengths,
                                                        const long long* __restrict__ target_lengths, int T, int V, int S_max, int blank,
                                                        int* __restrict__ out_state, int* __restrict__ out_span,
                                                        float* __restrict__ out_token_score, float* __restrict__ out_score,
                                                        unsigned* __restrict__ moves) {
    extern __shared__ float smem[];
    float* rowA = smem;                                   // [S_max] lattice row t-1 / t (ping-pong); later the span starts / ends
    float* rowB = smem + S_max;
    float* em = smem + 2 * S_max;                         // [ALN_TCHUNK][S_max] gathered emissions; later [ALN_BT_ROWS][S_max] move words
    int* lab = (int*)(em + ALN_TCHUNK * S_max);           // [S_max] class of each state
    int* skip = lab + S_max;                              // [S_max] 1 = the transition from two states back exists
    short* path = (short*)(skip + S_max);                 // [T] state of the best path per frame
    __shared__ int bad, feasible, final_state;
    __shared__ float final_score;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int b = blockIdx.x;
    const int Lmax = (S_max - 1) / 2;
    const int Tb = ctc_clamp_len(input_lengths[b], T);
    const int Lb = ctc_clamp_len(target_lengths[b], Lmax);
    const int S = 2 * Lb + 1;
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int s = tid; s < S; s += nt) {
        long long c = (s & 1) ? targets[(long long)b * target_ld + (s >> 1)] : (long long)blank;
        if ((s & 1) && (c < 0 || c >= V || c == blank)) { bad = 1; c = blank; }
        lab[s] = (int)c;
    }
    __syncthreads();
    for (int s = tid; s < S; s += nt) skip[s] = (s >= 2 && lab[s] != lab[s - 2]) ? 1 : 0;
    const bool dead = bad != 0;
    const float* base = lp + (long long)b * stride_b;
    unsigned* mv_b = moves + (long long)b * aln_chunks(T) * S_max;
    float* prev = rowA;
    float* cur = rowB;
    // ---- forward ----
    for (int t0 = 0; t0 < (dead ? 0 : Tb); t0 += ALN_TCHUNK) {
        __syncthreads();                                  // the previous chunk's emissions are no longer read (and skip[] is visible)
        for (int s = tid; s < S; s += nt) {
            const int c = lab[s];
            float ev[ALN_TCHUNK];                         // independent loads, all in flight before the first is used
#pragma unroll
            for (int i = 0; i < ALN_TCHUNK; ++i) {
                const int t = min(t0 + i, Tb - 1);        // clamped: loads past the end are unused, never out of bounds
                ev[i] = base[(long long)t * stride_t + c];
            }
#pragma unroll
            for (int i = 0; i < ALN_TCHUNK; ++i) em[i * S_max + s] = ev[i];
        }
        __syncthreads();
        const int n = min(ALN_TCHUNK, Tb - t0);
        unsigned word[ALN_MAXTRIP] = {0u, 0u, 0u, 0u};    // the chunk's moves of this thread's states
        for (int i = 0; i < n; ++i) {
#pragma unroll
            for (int k = 0; k < ALN_MAXTRIP; ++k) {
                const int s = tid + k * nt;
                if (s < S) {
                    float v;
                    if (t0 + i == 0) {
                        v = s < 2 ? em[s] : -INFINITY;    // the first frame reaches the leading blank and the first label only
                    } else {
                        float best = prev[s];
                        unsigned mv = 0u;
                        if (s >= 1) {
                            const float a2 = prev[s - 1];
                            if (a2 > best) { best = a2; mv = 1u; }
                        }
                        if (skip[s]) {
                            const float a3 = prev[s - 2];
                            if (a3 > best) { best = a3; mv = 2u; }
                        }
                        v = best + em[i * S_max + s];
                        word[k] |= mv << (2 * i);
                    }
                    cur[s] = v;
                }
            }
            __syncthreads();
            float* tmp = prev; prev = cur; cur = tmp;
        }
#pragma unroll
        for (int k = 0; k < ALN_MAXTRIP; ++k) {
            const int s = tid + k * nt;
            if (s < S) mv_b[(long long)(t0 / ALN_TCHUNK) * S_max + s] = word[k];
        }
    }
    // ---- end ----
    if (tid == 0) {
        int fs = 0;
        float sc;
        if (dead) {
            sc = -INFINITY;
        } else if (Tb == 0) {
            sc = Lb == 0 ? 0.f : -INFINITY;
        } else {
            if (S > 1) fs = prev[S - 1] > prev[S - 2] ? S - 1 : S - 2;
            sc = prev[fs];
        }
        final_state = fs;
        final_score = sc;
        feasible = sc != -INFINITY;
        out_score[b] = sc;
    }
    __syncthreads();                                      // also: the forward's move words are visible to the whole workgroup
    const bool ok = feasible != 0;
    // ---- back-trace ----
    if (ok && Tb > 0) {
        unsigned* stage = (unsigned*)em;
        const int ncb = (int)aln_chunks(Tb);              // chunk rows the forward wrote
        int s = final_state;                              // lives in thread 0
        for (int g = (ncb - 1) / ALN_BT_ROWS; g >= 0; --g) {
            const int c0 = g * ALN_BT_ROWS;
            __syncthreads();                              // the previous batch has been walked
            for (int x = tid; x < S; x += nt) {
                unsigned w[ALN_BT_ROWS];
#pragma unroll
                for (int r = 0; r < ALN_BT_ROWS; ++r) w[r] = mv_b[(long long)min(c0 + r, ncb - 1) * S_max + x];
#pragma unroll
                for (int r = 0; r < ALN_BT_ROWS; ++r) stage[r * S_max + x] = w[r];
            }
            __syncthreads();
            if (tid == 0) {
                const int lo = c0 * ALN_TCHUNK;
                for (int t = min(Tb, lo + ALN_BT_ROWS * ALN_TCHUNK) - 1; t >= lo; --t) {
                    path[t] = (short)s;
                    const unsigned w = stage[((t - lo) / ALN_TCHUNK) * S_max + s];
                    s = max(s - (int)((w >> (2 * (t % ALN_TCHUNK))) & 3u), 0);       // frame 0 holds move 0
                }
            }
        }
    }
    __syncthreads();
    // ---- outputs ----
    int* first = (int*)rowA;                              // [Lmax] first frame of target position j
    int* end = (int*)rowB;                                // [Lmax] end frame (exclusive)
    const int Tp = ok ? Tb : 0;                           // frames on the path
    for (int j = tid; j < Lmax; j += nt) { first[j] = -1; end[j] = -1; }
    for (int t = tid; t < T; t += nt) out_state[(long long)b * T + t] = t < Tp ? (int)path[t] : -1;
    __syncthreads();
    for (int t = tid; t < Tp; t += nt) {
        const int s = path[t];
        if (s & 1) {
            if (t == 0 || path[t - 1] != s) first[s >> 1] = t;
            if (t == Tp - 1 || path[t + 1] != s) end[s >> 1] = t + 1;
        }
    }
    __syncthreads();
    for (int j = tid; j < Lmax; j += nt) {
        int f = first[j], e = end[j];
        if (f < 0 || e < 0) f = e = -1;                   // (a path with NaN scores may leave a label state out)
        float acc = 0.f;
        if (f >= 0) {
            const int c = lab[2 * j + 1];
            for (int t = f; t < e; ++t) acc += base[(long long)t * stride_t + c];
        }
        out_span[((long long)b * Lmax + j) * 2] = f;
        out_span[((long long)b * Lmax + j) * 2 + 1] = e;
        out_token_score[(long long)b * Lmax + j] = acc;
    }
}

long long aln_lds_bytes(int T, int S_max) {
    return ((long long)(2 + ALN_TCHUNK) * S_max) * sizeof(float) + 2LL * S_max * sizeof(int) + (((long long)T + 1) / 2 * 2) * sizeof(short);
}

}  // namespace

extern "C" int av_ctc_align_workspace_bytes(int B, int T, int S_max, long long* bytes) {
    AV_CHECK(bytes, "av_ctc_align_workspace_bytes: null pointer");
    AV_CHECK(B >= 1 && T >= 1 && T <= ALN_MAXT, "av_ctc_align_workspace_bytes: bad shape B=%d T=%d (B >= 1, 1 <= T <= %d)", B, T, ALN_MAXT);
    if (int rc = ctc_check_smax("av_ctc_align_workspace_bytes", S_max)) return rc;
    *bytes = (long long)B * aln_chunks(T) * S_max * (long long)sizeof(unsigned);
    return AV_OK;
}

extern "C" int av_ctc_align(const float* log_probs, long long stride_b, long long stride_t, const long long* targets, long long target_ld,
                            const long long* input_lengths, const long long* target_lengths, int B, int T, int V, int S_max, int blank,
                            int* out_state, int* out_span, float* out_token_score, float* out_score, void* workspace,
                            long long workspace_bytes, void* stream) {
    AV_CHECK(log_probs && targets && input_lengths && target_lengths && out_state && out_score && workspace, "av_ctc_align: null pointer");
    AV_CHECK(B >= 1 && T >= 1 && T <= ALN_MAXT && V >= 1, "av_ctc_align: bad shape B=%d T=%d V=%d (1 <= T <= %d)", B, T, V, ALN_MAXT);
    if (int rc = ctc_check_blank("av_ctc_align", blank, V)) return rc;
    if (int rc = ctc_check_smax("av_ctc_align", S_max)) return rc;
    AV_CHECK(S_max == 1 || (out_span && out_token_score), "av_ctc_align: null pointer (out_span / out_token_score with Lmax = %d)",
             (S_max - 1) / 2);
    AV_CHECK(target_ld >= (S_max - 1) / 2, "av_ctc_align: target_ld %lld < Lmax %d", target_ld, (S_max - 1) / 2);
    if (int rc = ctc_check_rows("av_ctc_align", stride_b, stride_t, B, T, V, true, "btBT")) return rc;
    const long long lds = aln_lds_bytes(T, S_max);
    AV_CHECK(lds <= CTC_LDS_LIMIT && S_max <= 256 * ALN_MAXTRIP, "av_ctc_align: S_max %d at T %d needs %lld bytes of LDS (limit %lld)", S_max, T,
             lds, CTC_LDS_LIMIT);
    const long long need = (long long)B * aln_chunks(T) * S_max * (long long)sizeof(unsigned);
    AV_CHECK(workspace_bytes >= need, "av_ctc_align: workspace of %lld bytes is too small, %lld needed", workspace_bytes, need);
    AV_CHECK((uintptr_t)workspace % sizeof(unsigned) == 0, "av_ctc_align: workspace must be 4-byte aligned");
    const int threads = S_max >= 256 ? 256 : (S_max + 63) / 64 * 64;
    hipLaunchKernelGGL(ctc_align_kernel, dim3(B), dim3(threads), (size_t)lds, (hipStream_t)stream, log_probs, stride_b, stride_t, targets,
                       target_ld, input_lengths, target_lengths, T, V, S_max, blank, out_state, out_span, out_token_score, out_score,
                       (unsigned*)workspace);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
