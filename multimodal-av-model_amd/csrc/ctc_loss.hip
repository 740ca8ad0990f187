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
#include "av_common.h"

namespace {

constexpr int CTC_TCHUNK = 16;       // frames of gathered emissions staged per batch of loads (forward)
constexpr int CTC_BWD_ROWS = 4;      // [b, t] rows per wavefront (backward): the label chain is built once per workgroup

__device__ __forceinline__ int ctc_clamp_len(long long v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }

// log(exp(a) + exp(b) + exp(c)) in torch's order (aten/native/LossCTC.cpp): the maximum is taken out, an all -inf triple gives -inf
__device__ __forceinline__ float ctc_lse3(float a, float b, float c) {
    float m = fmaxf(fmaxf(a, b), c);
    if (m == -INFINITY) m = 0.f;
    return logf(expf(a - m) + expf(b - m) + expf(c - m)) + m;
}

__global__ __launch_bounds__(256) void ctc_lattice_kernel(const float* __restrict__ lp, long long stride_b, long long stride_t,
                                                          const long long* __restrict__ targets, long long target_ld,
                                                          const long long* __restrict__ input_lengths,
                                                          const long long* __restrict__ target_lengths, int B, int T, int V, int S_max,
                                                          int blank, int zero_infinity, float* __restrict__ nll,
                                                          float* __restrict__ log_alpha, float* __restrict__ log_beta) {
    extern __shared__ float smem[];
    float* rowA = smem;                                   // [S_max] lattice row t-1 / t (ping-pong)
    float* rowB = smem + S_max;
    float* em = smem + 2 * S_max;                         // [CTC_TCHUNK][S_max] gathered emissions
    int* lab = (int*)(em + CTC_TCHUNK * S_max);           // [S_max] class of each (mirrored) state
    int* skip = lab + S_max;                              // [S_max] 1 = the transition from two states back exists
    __shared__ int bad;
    const int tid = threadIdx.x, nt = blockDim.x;
    const bool mirror = blockIdx.x >= B;                  // beta: the alpha recursion with time and states reversed
    const int b = mirror ? blockIdx.x - B : blockIdx.x;
    const int Tb = ctc_clamp_len(input_lengths[b], T);
    const int Lb = ctc_clamp_len(target_lengths[b], (S_max - 1) / 2);
    const int S = 2 * Lb + 1;
    float* out = mirror ? log_beta : log_alpha;
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int s = tid; s < S; s += nt) {
        const int so = mirror ? S - 1 - s : s;            // state of the original lattice
        long long c = (so & 1) ? targets[(long long)b * target_ld + (so >> 1)] : (long long)blank;
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
            float* orow = out ? out + ((long long)b * T + t) * S_max : nullptr;
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
        if (zero_infinity && r == INFINITY) r = 0.f;
        nll[b] = r;
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

constexpr long long CTC_LDS_LIMIT = 64 * 1024;

}  // namespace

extern "C" int av_ctc_loss_fwd(const float* log_probs, long long stride_b, long long stride_t, const long long* targets,
                               long long target_ld, const long long* input_lengths, const long long* target_lengths, int B, int T, int V,
                               int S_max, int blank, int zero_infinity, float* nll, float* log_alpha, float* log_beta, void* stream) {
    AV_CHECK(log_probs && targets && input_lengths && target_lengths && nll, "av_ctc_loss_fwd: null pointer");
    AV_CHECK(log_alpha || !log_beta, "av_ctc_loss_fwd: log_beta without log_alpha (null pointer)");
    AV_CHECK(B >= 1 && T >= 1 && V >= 1, "av_ctc_loss_fwd: bad shape B=%d T=%d V=%d", B, T, V);
    AV_CHECK(blank >= 0 && blank < V, "av_ctc_loss_fwd: blank %d outside [0, %d)", blank, V);
    AV_CHECK(S_max >= 1 && (S_max & 1), "av_ctc_loss_fwd: S_max = 2 Lmax + 1 must be odd and >= 1, got %d", S_max);
    AV_CHECK(target_ld >= (S_max - 1) / 2, "av_ctc_loss_fwd: target_ld %lld < Lmax %d", target_ld, (S_max - 1) / 2);
    AV_CHECK(stride_b >= 0 && stride_t >= 0 && ((stride_t >= V && stride_b >= (long long)T * stride_t) ||
                                                 (stride_b >= V && stride_t >= (long long)B * stride_b)),
             "av_ctc_loss_fwd: strides (b %lld, t %lld) do not cover [B=%d][T=%d][V=%d] rows", stride_b, stride_t, B, T, V);
    const long long lds = ((long long)(2 + CTC_TCHUNK) * S_max) * sizeof(float) + 2LL * S_max * sizeof(int);
    AV_CHECK(lds <= CTC_LDS_LIMIT, "av_ctc_loss_fwd: S_max %d needs %lld bytes of LDS (limit %lld)", S_max, lds, CTC_LDS_LIMIT);
    const int threads = S_max >= 256 ? 256 : (S_max + 63) / 64 * 64;
    const int grid = log_beta ? 2 * B : B;
    hipLaunchKernelGGL(ctc_lattice_kernel, dim3(grid), dim3(threads), (size_t)lds, (hipStream_t)stream, log_probs, stride_b, stride_t, targets,
                       target_ld, input_lengths, target_lengths, B, T, V, S_max, blank, zero_infinity, nll, log_alpha, log_beta);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_ctc_loss_bwd(const float* log_probs, long long stride_b, long long stride_t, const long long* targets,
                               long long target_ld, const long long* input_lengths, const long long* target_lengths, int B, int T, int V,
                               int S_max, int blank, const float* nll, const float* log_alpha, const float* log_beta,
                               const float* grad_nll, float* grad, void* stream) {
    AV_CHECK(log_probs && targets && input_lengths && target_lengths && nll && log_alpha && log_beta && grad_nll && grad,
             "av_ctc_loss_bwd: null pointer");
    AV_CHECK(B >= 1 && B <= 65535 && T >= 1 && V >= 1, "av_ctc_loss_bwd: bad shape B=%d T=%d V=%d (B <= 65535)", B, T, V);
    AV_CHECK(blank >= 0 && blank < V, "av_ctc_loss_bwd: blank %d outside [0, %d)", blank, V);
    AV_CHECK(S_max >= 1 && (S_max & 1), "av_ctc_loss_bwd: S_max = 2 Lmax + 1 must be odd and >= 1, got %d", S_max);
    AV_CHECK(target_ld >= (S_max - 1) / 2, "av_ctc_loss_bwd: target_ld %lld < Lmax %d", target_ld, (S_max - 1) / 2);
    AV_CHECK(stride_b >= 0 && stride_t >= 0 && ((stride_t >= V && stride_b >= (long long)T * stride_t) ||
                                                 (stride_b >= V && stride_t >= (long long)B * stride_b)),
             "av_ctc_loss_bwd: strides (b %lld, t %lld) do not cover [B=%d][T=%d][V=%d] rows", stride_b, stride_t, B, T, V);
    const int Lmax = (S_max - 1) / 2;
    int W = 4;                                            // wavefronts (= rows in flight) per workgroup: as many as the LDS rows allow
    long long lds = 0;
    for (; W >= 1; W >>= 1) {
        lds = (long long)W * ((long long)V + S_max) * sizeof(float) + 3LL * Lmax * sizeof(int);
        if (lds <= CTC_LDS_LIMIT) break;
    }
    AV_CHECK(W >= 1, "av_ctc_loss_bwd: V %d + S_max %d floats exceed the LDS row (limit %lld bytes)", V, S_max, CTC_LDS_LIMIT);
    // 16-byte loads / stores need every row start on a 16-byte boundary (LDS rows: V % 4 == 0 keeps occ rows aligned)
    const int vec = (V % 4 == 0) && (stride_b % 4 == 0) && (stride_t % 4 == 0) && ((uintptr_t)log_probs % 16 == 0) && ((uintptr_t)grad % 16 == 0);
    const int rows = W * CTC_BWD_ROWS;
    hipLaunchKernelGGL(ctc_grad_kernel, dim3((T + rows - 1) / rows, B), dim3(64 * W), (size_t)lds, (hipStream_t)stream, log_probs, stride_b,
                       stride_t, targets, target_ld, input_lengths, target_lengths, T, V, S_max, blank, nll, log_alpha, log_beta, grad_nll,
                       grad, vec);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
