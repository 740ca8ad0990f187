// CTC loss on the device: forward (negative log-likelihood per utterance) and the gradient with respect to the log-probabilities, with the
// semantics of torch.nn.functional.ctc_loss(log_probs, targets [B, Lmax] int64, input_lengths, target_lengths, blank, reduction="none",
// zero_infinity) - the call of model/trainer.py:25,116-117 (nn.CTCLoss(blank=3, zero_infinity=True)).  Lengths and labels are read from
// DEVICE memory: nothing travels to the host and nothing synchronises.  fp32 throughout (the same code in both libraries).
//
// Extended label row l' of S = 2 L + 1 states (blank, l1, blank, ..., lL, blank); the skip s-2 -> s exists where l'_s != l'_{s-2}.
//   ctc_lattice_kernel   one workgroup per (utterance, direction): log alpha (first B workgroups) and, when a gradient is wanted, log beta
//                        (second B workgroups, the same recursion on the mirrored lattice) -> workspaces [B][T][S_max]; the previous
//                        lattice row lives in LDS, the S gathered emissions of the next 16 frames are staged in LDS by one batch of
//                        independent loads (the V-wide row of log_probs is never read here).
//   ctc_grad_kernel      no serial chain: one wavefront per [b, t] row.  occ[c] = sum over the states with label c of
//                        exp(alpha + beta + nll - lp[c]) is gathered into an LDS row of V floats, then the row
//                        grad = g_b (exp(lp) - occ) is written with 16-byte stores (zeros for t >= T_b and for infeasible items).
//                        This is torch's form of the gradient (rows sum to zero), not the textbook one.
// Determinism: no floating-point atomics.  The first occurrence of a label owns that label's sum and walks a next-same-label chain in
// position order; the blank states are summed per lane in position order and combined by a fixed butterfly.
// Out-of-range data cannot cause out-of-bounds accesses: T_b is clamped to [0, T], L_b to [0, Lmax], and an utterance with a label
// outside [0, V) is infeasible (every emission -inf => nll = +inf, zero gradient).
//
// N-best form (av_ctc_nbest_fwd / _bwd: minimum word error rate training, mwer.py): N label sequences per utterance against ONE [T, V] block
// of log-probs.  The forward is the SAME lattice kernel, instantiated with items = B N (item b N + n reads utterance b's rows and T_b, int32
// labels at b ld_b + n ld_n): a present hypothesis is bit for bit an item of av_ctc_loss_fwd.  An item is OUT (nll = +inf, no gradient, its
// grad_nll never read) when its length is < 0 (absent) or > Lmax (not clamped: a cut hypothesis is another hypothesis), when an id is
// outside [0, V) or when no path exists.
//   ctc_nbest_grad_kernel  the shape of ctc_grad_kernel, one wavefront per [b, t] row that loops over the N hypotheses in ascending n: the
//                          label chains of all N hypotheses are built once per workgroup, g_n occ_n is accumulated into the LDS row in
//                          hypothesis order (each class has one owner lane per hypothesis: no atomics), the log-prob row is read once and
//                          grad = G_b exp(lp) - sum_n g_n occ_n, G_b = sum_n g_n over the items that are not out, is written once.
#include "ctc_common.h"

namespace {

constexpr int CTC_TCHUNK = 16;       // frames of gathered emissions staged per batch of loads (forward)
constexpr int CTC_BWD_ROWS = 4;      // [b, t] rows per wavefront (backward): the label chain is built once per workgroup

// log(exp(a) + exp(b) + exp(c)) in torch's order (aten/native/LossCTC.cpp): the maximum is taken out, an all -inf triple gives -inf
__device__ __forceinline__ float ctc_lse3(float a, float b, float c) {
    float m = fmaxf(fmaxf(a, b), c);
    if (m == -INFINITY) m = 0.f;
    return logf(expf(a - m) + expf(b - m) + expf(c - m)) + m;
}

// NBEST = false: the items are the B utterances, labels int64 [B][ld_b] (av_ctc_loss_fwd).  NBEST = true: items = B N, item b N + n reads
// the log-probs and T_b of utterance b and the int32 labels at b ld_b + n ld_n; a length < 0 or > Lmax makes it out (never clamped).
template <bool NBEST>
__global__ __launch_bounds__(256) void ctc_lattice_kernel(const float* __restrict__ lp, long long stride_b, long long stride_t,
                                                          const void* __restrict__ labels, long long ld_b, long long ld_n,
                                                          const long long* __restrict__ input_lengths,
                                                          const long long* __restrict__ label_lengths, int items, int N, int T, int V,
                                                          int S_max, int blank, int zero_infinity, float* __restrict__ nll,
                                                          float* __restrict__ log_alpha, float* __restrict__ log_beta) {
    extern __shared__ float smem[];
    float* rowA = smem;                                   // [S_max] lattice row t-1 / t (ping-pong)
    float* rowB = smem + S_max;
    float* em = smem + 2 * S_max;                         // [CTC_TCHUNK][S_max] gathered emissions
    int* lab = (int*)(em + CTC_TCHUNK * S_max);           // [S_max] class of each (mirrored) state
    int* skip = lab + S_max;                              // [S_max] 1 = the transition from two states back exists
    __shared__ int bad;
    const int tid = threadIdx.x, nt = blockDim.x;
    const bool mirror = blockIdx.x >= items;              // beta: the alpha recursion with time and states reversed
    const int item = mirror ? blockIdx.x - items : blockIdx.x;
    const int b = NBEST ? item / N : item;                // the utterance whose log-probs and T_b the item reads
    const int Tb = ctc_clamp_len(input_lengths[b], T);
    const long long Lraw = label_lengths[item];
    const bool out_len = NBEST && (Lraw < 0 || Lraw > (S_max - 1) / 2);
    const int Lb = out_len ? 0 : ctc_clamp_len(Lraw, (S_max - 1) / 2);
    const int S = 2 * Lb + 1;
    float* out = mirror ? log_beta : log_alpha;
    const long long lab0 = NBEST ? (long long)b * ld_b + (long long)(item - b * N) * ld_n : (long long)item * ld_b;
    if (tid == 0) bad = out_len ? 1 : 0;
    __syncthreads();
    for (int s = tid; s < S; s += nt) {
        const int so = mirror ? S - 1 - s : s;            // state of the original lattice
        long long c = blank;
        if (so & 1) c = NBEST ? (long long)((const int*)labels)[lab0 + (so >> 1)] : ((const long long*)labels)[lab0 + (so >> 1)];
        if (c < 0 || c >= V) { bad = 1; c = blank; }
        lab[s] = (int)c;
    }
    __syncthreads();
    for (int s = tid; s < S; s += nt) skip[s] = (s >= 2 && lab[s] != lab[s - 2]) ? 1 : 0;
    const bool dead = bad != 0;
    const float* base = lp + (long long)b * stride_b;
    float* prev = rowA;
    float* cur = rowB;
    for (int t0 = 0; t0 < Tb; t0 += CTC_TCHUNK) {
        __syncthreads();                                  // the previous chunk's emissions are no longer read (and skip[] is visible)
        for (int s = tid; s < S; s += nt) {
            const int c = lab[s];
            float ev[CTC_TCHUNK];                         // independent loads, all in flight before the first is used
#pragma unroll
            for (int i = 0; i < CTC_TCHUNK; ++i) {
                const int ts = min(t0 + i, Tb - 1);       // step of the recursion (clamped: loads past the end are unused, never out of
                ev[i] = base[(long long)(mirror ? Tb - 1 - ts : ts) * stride_t + c];      // bounds); frame Tb-1-ts on the mirrored lattice
            }
#pragma unroll
            for (int i = 0; i < CTC_TCHUNK; ++i) em[i * S_max + s] = dead ? -INFINITY : ev[i];
        }
        __syncthreads();
        const int n = min(CTC_TCHUNK, Tb - t0);
        for (int i = 0; i < n; ++i) {
            const int ts = t0 + i;
            const int t = mirror ? Tb - 1 - ts : ts;
            float* orow = out ? out + ((long long)item * T + t) * S_max : nullptr;
            for (int s = tid; s < S; s += nt) {
                float v;
                if (ts == 0) {
                    v = s < 2 ? em[s] : -INFINITY;        // the first frame reaches the leading blank and the first label only
                } else {
                    const float a1 = prev[s];
                    const float a2 = s >= 1 ? prev[s - 1] : -INFINITY;
                    const float a3 = skip[s] ? prev[s - 2] : -INFINITY;
                    v = ctc_lse3(a1, a2, a3) + em[i * S_max + s];
                }
                cur[s] = v;
                if (orow) orow[mirror ? S - 1 - s : s] = v;
            }
            __syncthreads();
            float* tmp = prev; prev = cur; cur = tmp;
        }
    }
    if (!mirror && tid == 0) {
        float r;
        if (Tb == 0) {
            r = Lb == 0 ? 0.f : INFINITY;
        } else {
            const float l1 = prev[S - 1], l2 = S > 1 ? prev[S - 2] : -INFINITY;
            float m = fmaxf(l1, l2);
            if (m == -INFINITY) m = 0.f;
            r = -(logf(expf(l1 - m) + expf(l2 - m)) + m);
        }
        if (NBEST && dead) r = INFINITY;                  // an out item with T_b = 0 too
        if (zero_infinity && r == INFINITY) r = 0.f;
        nll[item] = r;
    }
}

__global__ __launch_bounds__(256) void ctc_grad_kernel(const float* __restrict__ lp, long long stride_b, long long stride_t,
                                                       const long long* __restrict__ targets, long long target_ld,
                                                       const long long* __restrict__ input_lengths,
                                                       const long long* __restrict__ target_lengths, int T, int V, int S_max, int blank,
                                                       const float* __restrict__ nll, const float* __restrict__ log_alpha,
                                                       const float* __restrict__ log_beta, const float* __restrict__ grad_nll,
                                                       float* __restrict__ grad, int vec) {
    extern __shared__ float smem[];
    const int W = blockDim.x >> 6;
    const int Lmax = (S_max - 1) / 2;
    float* occ_all = smem;                                // [W][V]     per-class occupancy of the wavefront's row
    float* ab_all = smem + (long long)W * V;              // [W][S_max] alpha + beta + nll of the row
    int* lab = (int*)(ab_all + W * S_max);                // [Lmax] labels
    int* nxt = lab + Lmax;                                // [Lmax] next position with the same label (-1: none)
    int* own = nxt + Lmax;                                // [Lmax] 1 = first occurrence of its label (and not the blank class)
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.y;
    const int Tb = ctc_clamp_len(input_lengths[b], T);
    const int Lb = ctc_clamp_len(target_lengths[b], Lmax);
    const int S = 2 * Lb + 1;
    // feasible <=> the forward reached one of the two final states (an utterance with a bad label has an all -inf lattice)
    bool feasible = false;
    if (Tb > 0) {
        const float* last = log_alpha + ((long long)b * T + (Tb - 1)) * S_max;
        const float l1 = last[S - 1], l2 = S > 1 ? last[S - 2] : -INFINITY;
        feasible = l1 > -INFINITY || l2 > -INFINITY;
    }
    const float g = grad_nll[b];
    // with zero_infinity the forward returned 0 for an infeasible item; for a feasible one nll[b] is the value itself
    const float nl = feasible ? nll[b] : 0.f;
    for (int i = tid; i < W * V; i += nt) occ_all[i] = 0.f;
    for (int k = tid; k < Lb; k += nt) {
        const long long c = targets[(long long)b * target_ld + k];
        lab[k] = (c < 0 || c >= V) ? blank : (int)c;      // (a bad label makes the item infeasible: never used then)
    }
    __syncthreads();
    if (feasible) {
        for (int k = tid; k < Lb; k += nt) {
            const int mine = lab[k];
            int nx = -1, first = mine != blank;           // a label equal to the blank class is summed with the blank states
            for (int kp = Lb - 1; kp >= 0; --kp) {        // uniform trip count, broadcast LDS reads
                const int l = lab[kp];
                if (l == mine && kp > k) nx = kp;
                if (l == mine && kp < k) first = 0;
            }
            nxt[k] = nx;
            own[k] = first;
        }
    }
    float* occ = occ_all + (long long)w * V;
    float* ab = ab_all + w * S_max;
    const float* base = lp + (long long)b * stride_b;
    for (int it = 0; it < CTC_BWD_ROWS; ++it) {
        const int t = (blockIdx.x * CTC_BWD_ROWS + it) * W + w;
        const bool act = feasible && t < Tb;
        const float* row = base + (long long)t * stride_t;
        if (act) {
            const float* ar = log_alpha + ((long long)b * T + t) * S_max;
            const float* br = log_beta + ((long long)b * T + t) * S_max;
            for (int s = lane; s < S; s += 64) ab[s] = (ar[s] + br[s]) + nl;
        }
        __syncthreads();
        if (act) {
            const float lpb = row[blank];
            float acc = 0.f;
            for (int s = lane; s < S; s += 64) {
                const int c = (s & 1) ? lab[s >> 1] : blank;
                if (c == blank) acc += expf(ab[s] - lpb);
            }
            acc = wave_sum(acc);
            if (lane == 0) occ[blank] = acc;
            for (int k = lane; k < Lb; k += 64) {
                if (own[k]) {
                    const int c = lab[k];
                    const float l = row[c];
                    float sum = 0.f;
                    int j = k;
                    do {
                        sum += expf(ab[2 * j + 1] - l);
                        j = nxt[j];
                    } while (j >= 0);
                    occ[c] = sum;
                }
            }
        }
        __syncthreads();
        if (t < T) {
            float* orow = grad + ((long long)b * T + t) * V;
            if (vec) {
                const f32x4* r4 = (const f32x4*)row;
                const f32x4* o4 = (const f32x4*)occ;
                f32x4* d4 = (f32x4*)orow;
                for (int i = lane; i < (V >> 2); i += 64) {
                    f32x4 d = {0.f, 0.f, 0.f, 0.f};
                    if (act) {
                        const f32x4 x = r4[i], o = o4[i];
                        d.x = g * (expf(x.x) - o.x); d.y = g * (expf(x.y) - o.y);
                        d.z = g * (expf(x.z) - o.z); d.w = g * (expf(x.w) - o.w);
                    }
                    d4[i] = d;
                }
            } else {
                for (int i = lane; i < V; i += 64) orow[i] = act ? g * (expf(row[i]) - occ[i]) : 0.f;
            }
        }
        __syncthreads();
        if (act) {                                        // leave the occupancy row zero for the next frame: S stores instead of V
            if (lane == 0) occ[blank] = 0.f;
            for (int k = lane; k < Lb; k += 64)
                if (own[k]) occ[lab[k]] = 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void ctc_nbest_grad_kernel(const float* __restrict__ lp, long long stride_b, long long stride_t,
                                                             const int* __restrict__ hyp_ids, long long ld_b, long long ld_n,
                                                             const long long* __restrict__ hyp_lens,
                                                             const long long* __restrict__ input_lengths, int N, int T, int V, int S_max,
                                                             int blank, const float* __restrict__ nll, const float* __restrict__ log_alpha,
                                                             const float* __restrict__ log_beta, const float* __restrict__ grad_nll,
                                                             float* __restrict__ grad, int vec) {
    extern __shared__ float smem[];
    const int W = blockDim.x >> 6;
    const int Lmax = (S_max - 1) / 2;
    float* occ_all = smem;                                // [W][V]     sum over the hypotheses of g_n occ_n of the wavefront's row
    float* ab_all = smem + (long long)W * V;              // [W][S_max] alpha + beta + nll of the row and the current hypothesis
    int* lab = (int*)(ab_all + W * S_max);                // [N][Lmax] labels; nxt, own as in ctc_grad_kernel, per hypothesis
    int* nxt = lab + N * Lmax;
    int* own = nxt + N * Lmax;
    int* hl = own + N * Lmax;                             // [N] length of the hypothesis, -1 = out
    float* hg = (float*)(hl + N);                         // [N] its grad_nll (0 when out: the value is never read then)
    float* hn = hg + N;                                   // [N] its nll
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.y;
    const int Tb = ctc_clamp_len(input_lengths[b], T);
    for (int n = tid; n < N; n += nt) {
        const long long item = (long long)b * N + n;
        const long long Lraw = hyp_lens[item];
        // not out <=> the length is in [0, Lmax] and the forward reached one of the two final states (a bad id leaves the lattice all -inf)
        bool ok = Lraw >= 0 && Lraw <= Lmax && Tb > 0;
        if (ok) {
            const int S = 2 * (int)Lraw + 1;
            const float* last = log_alpha + (item * T + (Tb - 1)) * S_max;
            const float l1 = last[S - 1], l2 = S > 1 ? last[S - 2] : -INFINITY;
            ok = l1 > -INFINITY || l2 > -INFINITY;
        }
        hl[n] = ok ? (int)Lraw : -1;
        hg[n] = ok ? grad_nll[item] : 0.f;
        hn[n] = ok ? nll[item] : 0.f;
    }
    for (int i = tid; i < W * V; i += nt) occ_all[i] = 0.f;
    __syncthreads();
    float G = 0.f;                                        // sum of g_n over the items that are not out, ascending n
    bool any = false;
    for (int n = 0; n < N; ++n)
        if (hl[n] >= 0) { G += hg[n]; any = true; }
    for (int i = tid; i < N * Lmax; i += nt) {
        const int n = i / Lmax, k = i - n * Lmax;
        if (k < hl[n]) {
            const int c = hyp_ids[(long long)b * ld_b + (long long)n * ld_n + k];
            lab[i] = (c < 0 || c >= V) ? blank : c;       // (a bad id makes the item out: never reached with the forward's own lattice)
        }
    }
    __syncthreads();
    for (int i = tid; i < N * Lmax; i += nt) {
        const int n = i / Lmax, k = i - n * Lmax, Ln = hl[n];
        if (k < Ln) {
            const int* ln = lab + n * Lmax;
            const int mine = ln[k];
            int nx = -1, first = mine != blank;           // a label equal to the blank class is summed with the blank states
            for (int kp = Ln - 1; kp >= 0; --kp) {
                const int l = ln[kp];
                if (l == mine && kp > k) nx = kp;
                if (l == mine && kp < k) first = 0;
            }
            nxt[i] = nx;
            own[i] = first;
        }
    }
    float* occ = occ_all + (long long)w * V;
    float* ab = ab_all + w * S_max;
    const float* base = lp + (long long)b * stride_b;
    for (int it = 0; it < CTC_BWD_ROWS; ++it) {
        const int t = (blockIdx.x * CTC_BWD_ROWS + it) * W + w;
        const bool act = any && t < Tb;
        const float* row = base + (long long)t * stride_t;
        for (int n = 0; n < N; ++n) {                     // hl[] is the same for every wavefront: the barriers below are uniform
            const int Ln = hl[n];
            if (Ln < 0) continue;
            const int S = 2 * Ln + 1;
            __syncthreads();                              // ab (previous hypothesis) is no longer read; first pass: chains are visible
            if (act) {
                const long long r = (((long long)b * N + n) * T + t) * S_max;
                const float nl = hn[n];
                for (int s = lane; s < S; s += 64) ab[s] = (log_alpha[r + s] + log_beta[r + s]) + nl;
            }
            __syncthreads();
            if (act) {
                const int* ln = lab + n * Lmax;
                const int* nn = nxt + n * Lmax;
                const int* on = own + n * Lmax;
                const float g = hg[n];
                const float lpb = row[blank];
                float acc = 0.f;
                for (int s = lane; s < S; s += 64) {
                    const int c = (s & 1) ? ln[s >> 1] : blank;
                    if (c == blank) acc += expf(ab[s] - lpb);
                }
                acc = wave_sum(acc);
                if (lane == 0) occ[blank] += g * acc;
                for (int k = lane; k < Ln; k += 64) {
                    if (on[k]) {
                        const int c = ln[k];
                        const float l = row[c];
                        float sum = 0.f;
                        int j = k;
                        do {
                            sum += expf(ab[2 * j + 1] - l);
                            j = nn[j];
                        } while (j >= 0);
                        occ[c] += g * sum;                // one owner lane per class and hypothesis; hypotheses in ascending n
                    }
                }
            }
        }
        __syncthreads();
        if (t < T) {                                      // every row is written; the occupancy row is left zero for the next frame
            float* orow = grad + ((long long)b * T + t) * V;
            if (vec) {
                const f32x4* r4 = (const f32x4*)row;
                f32x4* o4 = (f32x4*)occ;
                f32x4* d4 = (f32x4*)orow;
                for (int i = lane; i < (V >> 2); i += 64) {
                    f32x4 d = {0.f, 0.f, 0.f, 0.f};
                    if (act) {
                        const f32x4 x = r4[i], o = o4[i];
                        d.x = G * expf(x.x) - o.x; d.y = G * expf(x.y) - o.y;
                        d.z = G * expf(x.z) - o.z; d.w = G * expf(x.w) - o.w;
                        o4[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                    d4[i] = d;
                }
            } else {
                for (int i = lane; i < V; i += 64) {
                    float d = 0.f;
                    if (act) { d = G * expf(row[i]) - occ[i]; occ[i] = 0.f; }
                    orow[i] = d;
                }
            }
        }
    }
}

// The argument law of the four entry points.  The single-item pair is N = 1 with target_ld in the role of hyp_ld_b (nbest = false: it is
// reported under that name).  B_max: the gradient kernels put B in grid y (65535) and the n-best lattice launches 2 B N workgroups in x
// (B N <= 2^30); the single-item lattice launches 2 B in x and has no limit of its own (B_max = 0).
int ctc_loss_check(const char* fn, bool nbest, int B_max, long long stride_b, long long stride_t, long long ld_b, long long ld_n, int B, int N,
                   int T, int V, int S_max, int blank) {
    AV_CHECK(N >= 1 && N <= 64, "%s: N = %d hypotheses per utterance outside [1, 64]", fn, N);
    const bool shape = B >= 1 && (!B_max || B <= B_max) && T >= 1 && V >= 1;
    if (!B_max) AV_CHECK(shape, "%s: bad shape B=%d T=%d V=%d", fn, B, T, V);
    AV_CHECK(shape, nbest ? "%s: bad shape B=%d T=%d V=%d (1 <= B <= %d: the grid limit)" : "%s: bad shape B=%d T=%d V=%d (B <= %d)", fn, B, T, V,
             B_max);
    if (int rc = ctc_check_blank(fn, blank, V)) return rc;
    if (int rc = ctc_check_smax(fn, S_max)) return rc;
    const int Lmax = (S_max - 1) / 2;
    if (nbest) {
        AV_CHECK(ld_n >= Lmax, "%s: hyp_ld_n %lld < Lmax %d", fn, ld_n, Lmax);
        AV_CHECK(ld_b >= (long long)(N - 1) * ld_n + Lmax, "%s: hyp_ld_b %lld does not cover N = %d rows of hyp_ld_n %lld", fn, ld_b, N, ld_n);
    } else {
        AV_CHECK(ld_b >= Lmax, "%s: target_ld %lld < Lmax %d", fn, ld_b, Lmax);
    }
    return ctc_check_rows(fn, stride_b, stride_t, B, T, V, true, "btBT");
}

// the lattice launch: two lattice rows, CTC_TCHUNK rows of emissions, lab[] and skip[]; one thread per state, 256 at the most
int ctc_lattice_geometry(const char* fn, int S_max, long long* lds, int* threads) {
    *lds = ((long long)(2 + CTC_TCHUNK) * S_max) * sizeof(float) + 2LL * S_max * sizeof(int);
    AV_CHECK(*lds <= CTC_LDS_LIMIT, "%s: S_max %d needs %lld bytes of LDS (limit %lld)", fn, S_max, *lds, CTC_LDS_LIMIT);
    *threads = S_max >= 256 ? 256 : (S_max + 63) / 64 * 64;
    return AV_OK;
}

// the gradient launch: W wavefronts (= rows in flight) per workgroup, as many of 4, 2, 1 as the LDS allows beside the workgroup's
// label_ints ints; every wavefront holds V + S_max floats and walks CTC_BWD_ROWS rows.  Returns W, 0 when not even one row fits
int ctc_grad_geometry(int V, int S_max, long long label_ints, long long* lds, int* rows) {
    int W = 4;
    for (; W >= 1; W >>= 1) {
        *lds = (long long)W * ((long long)V + S_max) * sizeof(float) + label_ints * sizeof(int);
        if (*lds <= CTC_LDS_LIMIT) break;
    }
    *rows = W * CTC_BWD_ROWS;
    return W;
}

}  // namespace

extern "C" int av_ctc_loss_fwd(const float* log_probs, long long stride_b, long long stride_t, const long long* targets,
                               long long target_ld, const long long* input_lengths, const long long* target_lengths, int B, int T, int V,
                               int S_max, int blank, int zero_infinity, float* nll, float* log_alpha, float* log_beta, void* stream) {
    const char* fn = "av_ctc_loss_fwd";
    AV_CHECK(log_probs && targets && input_lengths && target_lengths && nll, "%s: null pointer", fn);
    AV_CHECK(log_alpha || !log_beta, "%s: log_beta without log_alpha (null pointer)", fn);
    if (int rc = ctc_loss_check(fn, false, 0, stride_b, stride_t, target_ld, target_ld, B, 1, T, V, S_max, blank)) return rc;
    long long lds;
    int threads;
    if (int rc = ctc_lattice_geometry(fn, S_max, &lds, &threads)) return rc;
    hipLaunchKernelGGL(ctc_lattice_kernel<false>, dim3(log_beta ? 2 * B : B), dim3(threads), (size_t)lds, (hipStream_t)stream, log_probs,
                       stride_b, stride_t, (const void*)targets, target_ld, 0LL, input_lengths, target_lengths, B, 1, T, V, S_max, blank,
                       zero_infinity, nll, log_alpha, log_beta);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_ctc_loss_bwd(const float* log_probs, long long stride_b, long long stride_t, const long long* targets,
                               long long target_ld, const long long* input_lengths, const long long* target_lengths, int B, int T, int V,
                               int S_max, int blank, const float* nll, const float* log_alpha, const float* log_beta,
                               const float* grad_nll, float* grad, void* stream) {
    const char* fn = "av_ctc_loss_bwd";
    AV_CHECK(log_probs && targets && input_lengths && target_lengths && nll && log_alpha && log_beta && grad_nll && grad, "%s: null pointer", fn);
    if (int rc = ctc_loss_check(fn, false, 65535, stride_b, stride_t, target_ld, target_ld, B, 1, T, V, S_max, blank)) return rc;
    int rows;
    long long lds;
    const int W = ctc_grad_geometry(V, S_max, 3LL * ((S_max - 1) / 2), &lds, &rows);
    AV_CHECK(W >= 1, "%s: V %d + S_max %d floats exceed the LDS row (limit %lld bytes)", fn, V, S_max, CTC_LDS_LIMIT);
    hipLaunchKernelGGL(ctc_grad_kernel, dim3((T + rows - 1) / rows, B), dim3(64 * W), (size_t)lds, (hipStream_t)stream, log_probs, stride_b,
                       stride_t, targets, target_ld, input_lengths, target_lengths, T, V, S_max, blank, nll, log_alpha, log_beta, grad_nll,
                       grad, (int)ctc_vec_ok(log_probs, grad, stride_b, stride_t, V));
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_ctc_nbest_fwd(const float* log_probs, long long stride_b, long long stride_t, const int* hyp_ids, long long hyp_ld_b,
                                long long hyp_ld_n, const long long* hyp_lens, const long long* input_lengths, int B, int N, int T, int V,
                                int S_max, int blank, float* nll, float* log_alpha, float* log_beta, void* stream) {
    const char* fn = "av_ctc_nbest_fwd";
    AV_CHECK(log_probs && hyp_ids && hyp_lens && input_lengths && nll, "%s: null pointer", fn);
    AV_CHECK(log_alpha || !log_beta, "%s: log_beta without log_alpha (null pointer)", fn);
    if (int rc = ctc_loss_check(fn, true, 65535, stride_b, stride_t, hyp_ld_b, hyp_ld_n, B, N, T, V, S_max, blank)) return rc;
    long long lds;
    int threads;
    if (int rc = ctc_lattice_geometry(fn, S_max, &lds, &threads)) return rc;
    const int items = B * N;                              // <= 65535 * 64
    hipLaunchKernelGGL(ctc_lattice_kernel<true>, dim3(log_beta ? 2 * items : items), dim3(threads), (size_t)lds, (hipStream_t)stream, log_probs,
                       stride_b, stride_t, (const void*)hyp_ids, hyp_ld_b, hyp_ld_n, input_lengths, hyp_lens, items, N, T, V, S_max, blank, 0,
                       nll, log_alpha, log_beta);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_ctc_nbest_bwd(const float* log_probs, long long stride_b, long long stride_t, const int* hyp_ids, long long hyp_ld_b,
                                long long hyp_ld_n, const long long* hyp_lens, const long long* input_lengths, int B, int N, int T, int V,
                                int S_max, int blank, const float* nll, const float* log_alpha, const float* log_beta, const float* grad_nll,
                                float* grad, void* stream) {
    const char* fn = "av_ctc_nbest_bwd";
    AV_CHECK(log_probs && hyp_ids && hyp_lens && input_lengths && nll && log_alpha && log_beta && grad_nll && grad, "%s: null pointer", fn);
    if (int rc = ctc_loss_check(fn, true, 65535, stride_b, stride_t, hyp_ld_b, hyp_ld_n, B, N, T, V, S_max, blank)) return rc;
    int rows;
    long long lds;
    const long long labels = 3LL * N * ((S_max - 1) / 2);
    const int W = ctc_grad_geometry(V, S_max, labels + 3LL * N, &lds, &rows);
    AV_CHECK(W >= 1, "%s: V %d + S_max %d floats and 3 N Lmax = %lld label ints exceed the LDS (limit %lld bytes)", fn, V, S_max, labels,
             CTC_LDS_LIMIT);
    hipLaunchKernelGGL(ctc_nbest_grad_kernel, dim3((T + rows - 1) / rows, B), dim3(64 * W), (size_t)lds, (hipStream_t)stream, log_probs,
                       stride_b, stride_t, hyp_ids, hyp_ld_b, hyp_ld_n, hyp_lens, input_lengths, N, T, V, S_max, blank, nll, log_alpha, log_beta,
                       grad_nll, grad, (int)ctc_vec_ok(log_probs, grad, stride_b, stride_t, V));
    AV_LAUNCH_CHECK();
    return AV_OK;
}
