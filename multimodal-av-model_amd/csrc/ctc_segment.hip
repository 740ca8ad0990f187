// CTC segmentation on the device: a known transcript laid over a recording of any length - forced alignment (csrc/ctc_align.hip) without
// its limits (T <= 4096, about 400 labels) and with ends that may float, a score per frame and a confidence per utterance (the
// min-of-window-means of CTC segmentation, Kuerzinger et al. 2020).  Lengths, labels and utterance ranges are read from DEVICE memory:
// nothing travels to the host and nothing synchronises.  fp32 throughout (the same code in both libraries); the host path of
// segmentation.py restates the law and agrees bit for bit - every operation is a float32 max, compare, add, subtract or one division.
//
// The law (segmentation.py has it in full).  Lattice of S = 2 L_b + 1 states as in ctc_align.hip, ties to the smaller move.
//   emissions  free = 0: e[t][s] = lp[t][l'_s].  free != 0: m[t] = max_v lp[t][v] (a NaN never wins), e[t][s] = lp[t][l'_s] - m[t]; every
//              e of a frame whose m[t] is not finite is -inf.
//   walk       d[0][0] = e[0][0], d[0][1] = e[0][1], the rest -inf.  t >= 1: best = d[t-1][s], then d[t-1][s-1] if strictly greater
//              (move 1), then d[t-1][s-2] if the skip exists and it is strictly greater (move 2); free start (bit 0): states 0 and 1 then
//              take a fresh start (best = 0, move 3) if 0 > best strictly.  d[t][s] = best + e[t][s].
//   end        c[t] = the better of d[t][S-1], d[t][S-2] (S-1 only if strictly greater; S = 1: state 0).  Fixed end: frame T_b - 1.  Free
//              end (bit 1): the first t with the greatest c[t].  The score is c there; -inf = infeasible.
//   back-trace from the end; stop at move 3 or frame 0.  Frames off the path have state -1 and frame score 0.
//   outputs    state, spans, frame_scores[t] = e[t][state[t]], token scores = sums of frame scores over the span in frame order, and per
//              utterance (a token range [b, e), valid if 0 <= b < e <= L_b) its frames [f, g) = first frame of token b to end frame of
//              token e-1, the mean frame score and the least mean of its consecutive windows of w frames.
//
// ctc_segment_kernel<R>, one workgroup per item, thread i owns the R contiguous states i R .. i R + R - 1 (R = 1, 4 or 16 by S_max):
//   forward     the lattice row, the labels and the skip bits of the owned states live in registers for the whole walk; the row never goes
//               to LDS.  Per frame a thread publishes its last two values in a double-buffered LDS array and reads its left neighbour's:
//               one barrier per frame.  Whole lp rows are staged in LDS by coalesced loads, up to 16 per batch (fewer for a large V), the
//               owned labels gathered from there; every even state is the blank: one broadcast read.  In free mode m[t] is a wave
//               reduction over the staged row (it is parked in out_frame_score[t] until the output phase replaces it).  Moves: 2 bits per
//               cell, 16 frames per word, workspace [B][ceil(T / 16)][S_max] words, 64-bit indexing.
//   back-trace  one lane walks the path.  A path moves at most 2 states per frame, so a batch of 256 frames needs the move words of the
//               513 states below the current one only: that window is staged in LDS (16 x 513 words).  States go straight to out_state.
//   outputs     out_state is read back after a barrier; spans, frame scores and token scores in parallel; then one thread per utterance.
// Determinism: no atomics, every sum has a fixed order.  Out-of-range data cannot cause out-of-bounds accesses: T_b is clamped to [0, T],
// L_b to [0, Lmax], a bad label ends the item before any emission is gathered, staged rows are clamped to T_b - 1, the walk clamps its state
// at 0, and an utterance range is used only if 0 <= b < e <= L_b.
#include "ctc_common.h"

namespace {

constexpr int SEG_TCHUNK = 16;                    // frames per move word (2 bits each) = the most lp rows staged per batch
constexpr int SEG_BT_ROWS = 16;                   // chunk rows of move words per back-trace batch: 256 frames
constexpr int SEG_BT_WIN = 2 * SEG_BT_ROWS * SEG_TCHUNK + 1;      // states a path can visit in one batch: 513
constexpr int SEG_MAXTHREADS = 1024;
constexpr int SEG_MAXR = 16;
constexpr int SEG_MAXS = SEG_MAXTHREADS * SEG_MAXR - 1;           // 16383 states: Lmax 8191
constexpr int SEG_MAXV = 12000;                   // one staged row of V floats beside the exchange buffers and the back-trace window
constexpr int SEG_UBATCH = 8;                     // frame scores an utterance's thread loads per batch

__host__ __device__ __forceinline__ long long seg_chunks(int T) { return ((long long)T + SEG_TCHUNK - 1) / SEG_TCHUNK; }
inline int seg_r(int S_max) { return S_max <= SEG_MAXTHREADS ? 1 : (S_max <= 4 * SEG_MAXTHREADS ? 4 : SEG_MAXR); }
inline int seg_threads(int S_max) { return (av_cdiv(S_max, seg_r(S_max)) + 63) / 64 * 64; }
// floats of LDS before the staged rows: two exchange buffers of 2 threads + 2 values, and m of the staged rows
inline long long seg_lds_head(int threads) { return 2LL * (2 * threads + 2) + SEG_TCHUNK; }
// lp rows staged per batch
inline int seg_rows(int threads, int V) {
    const long long room = (CTC_LDS_LIMIT - 256) / 4 - seg_lds_head(threads);
    return (int)(room / V < SEG_TCHUNK ? room / V : SEG_TCHUNK);
}

template <int R>
__global__ __launch_bounds__(SEG_MAXTHREADS) void ctc_segment_kernel(
    const float* __restrict__ lp, long long stride_b, long long stride_t, const long long* __restrict__ targets, long long target_ld,
    const long long* __restrict__ input_lengths, const long long* __restrict__ target_lengths, const int* __restrict__ utterances, int T,
    int V, int S_max, int U, int blank, int free_ends, int window, int NB, int* __restrict__ out_state, int* __restrict__ out_span,
    float* __restrict__ out_token_score, float* __restrict__ out_score, float* __restrict__ out_frame_score, int* __restrict__ out_utt_span,
    float* __restrict__ out_utt_mean, float* __restrict__ out_utt_score, unsigned* __restrict__ moves) {
    constexpr int NL = R == 1 ? 1 : R / 2;                // labels a thread owns
    extern __shared__ float smem[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int XS = 2 * nt + 2;
    float* xch = smem;                                    // [2][XS]: slots 0, 1 = -inf, then every thread's last two values (R = 1: its one)
    float* mrow = smem + 2 * XS;                          // [SEG_TCHUNK] m of the staged rows
    float* rows = mrow + SEG_TCHUNK;                      // [NB][V] staged lp rows; later [SEG_BT_ROWS][SEG_BT_WIN] move words
    __shared__ int bad, feasible, end_state, end_t, start_t, bt_s, bt_t, bt_done;
    const int b = blockIdx.x;
    const int Lmax = (S_max - 1) / 2;
    const int Tb = ctc_clamp_len(input_lengths[b], T);
    const int Lb = ctc_clamp_len(target_lengths[b], Lmax);
    const int S = 2 * Lb + 1;
    const int s0 = tid * R;
    const bool fstart = (free_ends & 1) != 0, fend = (free_ends & 2) != 0, rel = free_ends != 0;
    const long long* tg = targets + (long long)b * target_ld;
    if (tid == 0) {
        bad = 0;
        xch[0] = xch[1] = xch[XS] = xch[XS + 1] = -INFINITY;
    }
    __syncthreads();
    // ---- the owned states: labels and skip bits, in registers ----
    int labs[NL];
    unsigned skipbits = 0u;
#pragma unroll
    for (int k = 0; k < NL; ++k) {
        const int s = R == 1 ? s0 : s0 + 2 * k + 1;
        labs[k] = blank;                                  // an even state, or one past S: the blank, a valid column
        if ((s & 1) && s < S) {
            const int j = s >> 1;
            const long long c = tg[j];
            if (c < 0 || c >= V || c == blank) bad = 1;
            else labs[k] = (int)c;
            if (j >= 1 && tg[j - 1] != c) skipbits |= 1u << (R == 1 ? 0 : 2 * k + 1);
        }
    }
    __syncthreads();
    const bool dead = bad != 0;
    const float* base = lp + (long long)b * stride_b;
    unsigned* mv_b = moves + (long long)b * seg_chunks(T) * S_max;
    float* fsc = out_frame_score + (long long)b * T;
    int* ost = out_state + (long long)b * T;
    float d[R];
    unsigned mvw[R];
#pragma unroll
    for (int i = 0; i < R; ++i) { d[i] = -INFINITY; mvw[i] = 0u; }
    const bool owner = S - 1 >= s0 && S - 1 < s0 + R;     // of state S-1: it follows c[t]
    float best_c = -INFINITY;
    int best_t = 0, best_s = 0;
    // c[t] and its state from this thread's row of frame t and p1 = d[t][s0 - 1]
    auto end_of = [&](float p1, float& cv, int& cs) {
        float last = -INFINITY, pen = p1;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            if (s0 + i == S - 1) last = d[i];
            if (s0 + i == S - 2) pen = d[i];
        }
        if (S == 1 || last > pen) { cv = last; cs = S - 1; }
        else { cv = pen; cs = S - 2; }
    };
    // ---- forward ----
    for (int t0 = 0; t0 < (dead ? 0 : Tb); t0 += NB) {
        // (the barrier that ended the previous frame: its rows are no longer read)
        for (int c = tid; c < V; c += nt) {
            float v[SEG_TCHUNK];                          // independent loads, all in flight before the first is used
#pragma unroll
            for (int r = 0; r < SEG_TCHUNK; ++r)          // clamped: rows past the end are unused, never out of bounds
                v[r] = r < NB ? base[(long long)min(t0 + r, Tb - 1) * stride_t + c] : 0.f;
#pragma unroll
            for (int r = 0; r < SEG_TCHUNK; ++r)
                if (r < NB) rows[r * V + c] = v[r];
        }
        __syncthreads();
        const int n = min(NB, Tb - t0);
        if (rel) {
            const int lane = tid & 63;
            for (int r = tid >> 6; r < n; r += nt >> 6) {
                float best = -INFINITY;                   // x > best: a NaN never wins
                for (int c = lane; c < V; c += AV_WAVE) {
                    const float x = rows[r * V + c];
                    if (x > best) best = x;
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const float ob = __shfl_xor(best, o, 64);
                    if (ob > best) best = ob;
                }
                if (lane == 0) { mrow[r] = best; fsc[t0 + r] = best; }
            }
            __syncthreads();
        }
        for (int i0 = 0; i0 < n; ++i0) {
            const int t = t0 + i0;
            const float* row = rows + i0 * V;
            const float m = rel ? mrow[i0] : 0.f;         // x - 0 = x: the fixed ends' emissions are lp itself
            const bool fin = fabsf(m) < INFINITY;
            const float eb = fin ? row[blank] - m : -INFINITY;
            float ex[NL];
#pragma unroll
            for (int k = 0; k < NL; ++k) ex[k] = fin ? row[labs[k]] - m : -INFINITY;
            float* pub = xch + ((t + 1) & 1) * XS;
            if (t == 0) {
#pragma unroll
                for (int i = 0; i < R; ++i)
                    if (s0 + i < 2) d[i] = (R == 1 || (i & 1)) ? ex[R == 1 ? 0 : i >> 1] : eb;
            } else {
                const float* nb = xch + (t & 1) * XS;
                const float p2 = nb[R == 1 ? tid : 2 * tid], p1 = nb[R == 1 ? tid + 1 : 2 * tid + 1];
                if (fend && owner) {                      // c[t-1], one frame late: d[t-1][S-2] may be the neighbour's
                    float cv;
                    int cs;
                    end_of(p1, cv, cs);
                    if (t == 1 || cv > best_c) { best_c = cv; best_t = t - 1; best_s = cs; }
                }
#pragma unroll
                for (int i = R - 1; i >= 0; --i) {        // downwards: d[i-1] and d[i-2] still hold frame t-1
                    const float a1 = i >= 1 ? d[i - 1] : p1;
                    const float a2 = i >= 2 ? d[i - 2] : (i == 1 ? p1 : p2);
                    float best = d[i];
                    unsigned mv = 0u;
                    if (a1 > best) { best = a1; mv = 1u; }
                    if (((skipbits >> i) & 1u) && a2 > best) { best = a2; mv = 2u; }
                    if (fstart && s0 + i < 2 && 0.f > best) { best = 0.f; mv = 3u; }
                    d[i] = best + ((R == 1 || (i & 1)) ? ex[R == 1 ? 0 : i >> 1] : eb);
                    mvw[i] |= mv << (2 * (t & (SEG_TCHUNK - 1)));
                }
            }
            if (R == 1) pub[tid + 2] = d[0];
            else { pub[2 * tid + 2] = d[R >= 2 ? R - 2 : 0]; pub[2 * tid + 3] = d[R - 1]; }
            if ((t & (SEG_TCHUNK - 1)) == SEG_TCHUNK - 1 || t == Tb - 1) {
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    if (s0 + i < S_max) mv_b[(long long)(t / SEG_TCHUNK) * S_max + s0 + i] = mvw[i];
                    mvw[i] = 0u;
                }
            }
            __syncthreads();                              // the one barrier of a frame
        }
    }
    // ---- end ----
    if (tid == 0) {                                       // the items without a walk
        end_state = 0;
        end_t = start_t = -1;
        if (dead || Tb == 0) {
            const float sc = (!dead && Lb == 0) ? 0.f : -INFINITY;
            out_score[b] = sc;
            feasible = sc != -INFINITY;
        }
    }
    __syncthreads();
    if (!dead && Tb > 0 && owner) {
        const float* nb = xch + (Tb & 1) * XS;
        float cv;
        int cs;
        end_of(nb[R == 1 ? tid + 1 : 2 * tid + 1], cv, cs);
        if (!fend || Tb == 1 || cv > best_c) { best_c = cv; best_t = Tb - 1; best_s = cs; }
        end_state = best_s;
        end_t = best_t;
        out_score[b] = best_c;
        feasible = best_c != -INFINITY;
    }
    __syncthreads();                                      // also: the forward's move words are visible to the whole workgroup
    const bool ok = feasible != 0 && Tb > 0;              // there is a path
    // ---- back-trace ----
    if (ok) {
        unsigned* stage = (unsigned*)rows;
        const int ncb = (int)seg_chunks(Tb);              // chunk rows the forward wrote
        if (tid == 0) { bt_s = end_state; bt_t = end_t; bt_done = 0; }
        for (;;) {
            __syncthreads();                              // the previous batch has been walked
            if (bt_done) break;
            const int t_hi = bt_t, s_hi = bt_s;
            const int c0 = (t_hi / (SEG_BT_ROWS * SEG_TCHUNK)) * SEG_BT_ROWS, lo = c0 * SEG_TCHUNK;
            const int s_lo = s_hi - (SEG_BT_WIN - 1);
            for (int x = tid; x < SEG_BT_WIN; x += nt) {
                const int s = s_lo + x;
                if (s >= 0) {
                    unsigned w[SEG_BT_ROWS];
#pragma unroll
                    for (int r = 0; r < SEG_BT_ROWS; ++r) w[r] = mv_b[(long long)min(c0 + r, ncb - 1) * S_max + s];
#pragma unroll
                    for (int r = 0; r < SEG_BT_ROWS; ++r) stage[r * SEG_BT_WIN + x] = w[r];
                }
            }
            __syncthreads();
            if (tid == 0) {
                int s = s_hi, t = t_hi, done = 0;
                for (; t >= lo; --t) {
                    ost[t] = s;
                    const unsigned w = stage[((t - lo) / SEG_TCHUNK) * SEG_BT_WIN + (s - s_lo)];
                    const int mv = (int)((w >> (2 * (t % SEG_TCHUNK))) & 3u);
                    if (mv == 3 || t == 0) { done = 1; start_t = t; break; }
                    s = max(s - mv, 0);
                }
                bt_s = s;
                bt_t = t;
                bt_done = done;
            }
        }
    }
    __threadfence_block();
    __syncthreads();                                      // out_state of the path and start_t are visible
    // ---- outputs ----
    const int pa = ok ? start_t : 0, pz = ok ? end_t + 1 : 0;                  // the path's frames [pa, pz)
    for (int t = tid; t < T; t += nt) {
        float x = 0.f;
        if (t >= pa && t < pz) {
            const int s = ost[t];
            const int c = (s & 1) ? (int)tg[s >> 1] : blank;
            x = base[(long long)t * stride_t + c];
            if (rel) {
                const float m = fsc[t];
                x = fabsf(m) < INFINITY ? x - m : -INFINITY;
            }
        } else {
            ost[t] = -1;
        }
        fsc[t] = x;
    }
    for (int j = tid; j < Lmax; j += nt) {
        out_span[((long long)b * Lmax + j) * 2] = -1;
        out_span[((long long)b * Lmax + j) * 2 + 1] = -1;
    }
    __threadfence_block();
    __syncthreads();
    for (int t = pa + tid; t < pz; t += nt) {
        const int s = ost[t];
        if (s & 1) {
            if (t == pa || ost[t - 1] != s) out_span[((long long)b * Lmax + (s >> 1)) * 2] = t;
            if (t == pz - 1 || ost[t + 1] != s) out_span[((long long)b * Lmax + (s >> 1)) * 2 + 1] = t + 1;
        }
    }
    __threadfence_block();
    __syncthreads();
    for (int j = tid; j < Lmax; j += nt) {
        const int f = out_span[((long long)b * Lmax + j) * 2], e = out_span[((long long)b * Lmax + j) * 2 + 1];
        float acc = 0.f;
        if (f < 0 || e < 0) {                             // (a path with NaN scores may leave a label state out)
            out_span[((long long)b * Lmax + j) * 2] = -1;
            out_span[((long long)b * Lmax + j) * 2 + 1] = -1;
        } else {
            for (int t = f; t < e; ++t) acc += fsc[t];
        }
        out_token_score[(long long)b * Lmax + j] = acc;
    }
    __threadfence_block();
    __syncthreads();
    // ---- utterances ----
    for (int u = tid; u < U; u += nt) {
        const long long bu = (long long)b * U + u;
        const int j0 = utterances[bu * 2], j1 = utterances[bu * 2 + 1];
        int f = -1, g = -1;
        if (ok && j0 >= 0 && j0 < j1 && j1 <= Lb) {
            f = out_span[((long long)b * Lmax + j0) * 2];
            g = out_span[((long long)b * Lmax + j1 - 1) * 2 + 1];
            if (f < 0 || g <= f) f = g = -1;
        }
        float mean = 0.f, low = 0.f;
        if (f >= 0) {
            float tot = 0.f, wsum = 0.f;
            int cnt = 0;
            bool first = true;
            for (int t0 = f; t0 < g; t0 += SEG_UBATCH) {
                float x[SEG_UBATCH];                      // independent loads, then the adds in frame order
#pragma unroll
                for (int i = 0; i < SEG_UBATCH; ++i) x[i] = fsc[min(t0 + i, g - 1)];
#pragma unroll
                for (int i = 0; i < SEG_UBATCH; ++i) {
                    if (t0 + i < g) {
                        tot += x[i];
                        wsum += x[i];
                        ++cnt;
                        if (cnt == window || t0 + i == g - 1) {
                            const float wm = wsum / (float)cnt;
                            if (first || wm < low) low = wm;
                            first = false;
                            wsum = 0.f;
                            cnt = 0;
                        }
                    }
                }
            }
            mean = tot / (float)(g - f);
        }
        out_utt_span[bu * 2] = f;
        out_utt_span[bu * 2 + 1] = g;
        out_utt_mean[bu] = mean;
        out_utt_score[bu] = low;
    }
}

long long seg_ws_bytes(int B, int T, int S_max) { return (long long)B * seg_chunks(T) * S_max * (long long)sizeof(unsigned); }

int seg_check_shape(const char* who, int B, int T, int S_max) {
    AV_CHECK(B >= 1 && T >= 1, "%s: bad shape B=%d T=%d (both >= 1)", who, B, T);
    if (int rc = ctc_check_smax(who, S_max)) return rc;
    AV_CHECK(S_max <= SEG_MAXS, "%s: S_max %d above the limit %d (Lmax %d)", who, S_max, SEG_MAXS, (SEG_MAXS - 1) / 2);
    return AV_OK;
}

}  // namespace

extern "C" int av_ctc_segment_workspace_bytes(int B, int T, int S_max, long long* bytes) {
    AV_CHECK(bytes, "av_ctc_segment_workspace_bytes: null pointer");
    if (int rc = seg_check_shape("av_ctc_segment_workspace_bytes", B, T, S_max)) return rc;
    *bytes = seg_ws_bytes(B, T, S_max);
    return AV_OK;
}

extern "C" int av_ctc_segment(const float* log_probs, long long stride_b, long long stride_t, const long long* targets, long long target_ld,
                              const long long* input_lengths, const long long* target_lengths, const int* utterances, int B, int T, int V,
                              int S_max, int U, int blank, int free_ends, int score_window, int* out_state, int* out_span,
                              float* out_token_score, float* out_score, float* out_frame_score, int* out_utt_span, float* out_utt_mean,
                              float* out_utt_score, void* workspace, long long workspace_bytes, void* stream) {
    AV_CHECK(log_probs && targets && input_lengths && target_lengths && out_state && out_score && out_frame_score && workspace,
             "av_ctc_segment: null pointer");
    if (int rc = seg_check_shape("av_ctc_segment", B, T, S_max)) return rc;
    AV_CHECK(V >= 1 && V <= SEG_MAXV, "av_ctc_segment: V = %d outside [1, %d] (one row of log-probs is staged in LDS)", V, SEG_MAXV);
    if (int rc = ctc_check_blank("av_ctc_segment", blank, V)) return rc;
    AV_CHECK(free_ends >= 0 && free_ends <= 3, "av_ctc_segment: free = %d outside [0, 3] (bit 0: free start, bit 1: free end)", free_ends);
    AV_CHECK(score_window >= 1, "av_ctc_segment: score_window %d < 1", score_window);
    AV_CHECK(U >= 0, "av_ctc_segment: U = %d utterances < 0", U);
    AV_CHECK(S_max == 1 || (out_span && out_token_score), "av_ctc_segment: null pointer (out_span / out_token_score with Lmax = %d)",
             (S_max - 1) / 2);
    AV_CHECK(U == 0 || (utterances && out_utt_span && out_utt_mean && out_utt_score),
             "av_ctc_segment: null pointer (utterances / out_utt_span / out_utt_mean / out_utt_score with U = %d)", U);
    AV_CHECK(target_ld >= (S_max - 1) / 2, "av_ctc_segment: target_ld %lld < Lmax %d", target_ld, (S_max - 1) / 2);
    if (int rc = ctc_check_rows("av_ctc_segment", stride_b, stride_t, B, T, V, true, "btBT")) return rc;
    const long long need = seg_ws_bytes(B, T, S_max);
    AV_CHECK(workspace_bytes >= need, "av_ctc_segment: workspace of %lld bytes is too small, %lld needed", workspace_bytes, need);
    AV_CHECK((uintptr_t)workspace % sizeof(unsigned) == 0, "av_ctc_segment: workspace must be 4-byte aligned");
    const int R = seg_r(S_max), threads = seg_threads(S_max), NB = seg_rows(threads, V);
    const long long body = (long long)NB * V > (long long)SEG_BT_ROWS * SEG_BT_WIN ? (long long)NB * V : (long long)SEG_BT_ROWS * SEG_BT_WIN;
    const long long lds = (seg_lds_head(threads) + body) * (long long)sizeof(float);
    AV_CHECK(NB >= 1 && lds <= CTC_LDS_LIMIT - 256, "av_ctc_segment: V %d at S_max %d needs %lld bytes of LDS (limit %lld)", V, S_max, lds,
             CTC_LDS_LIMIT - 256);
#define SEG_LAUNCH(RR)                                                                                                                     \
    hipLaunchKernelGGL(ctc_segment_kernel<RR>, dim3(B), dim3(threads), (size_t)lds, (hipStream_t)stream, log_probs, stride_b, stride_t,    \
                       targets, target_ld, input_lengths, target_lengths, utterances, T, V, S_max, U, blank, free_ends, score_window, NB,  \
                       out_state, out_span, out_token_score, out_score, out_frame_score, out_utt_span, out_utt_mean, out_utt_score,        \
                       (unsigned*)workspace)
    if (R == 1) SEG_LAUNCH(1);
    else if (R == 4) SEG_LAUNCH(4);
    else SEG_LAUNCH(16);
#undef SEG_LAUNCH
    AV_LAUNCH_CHECK();
    return AV_OK;
}
