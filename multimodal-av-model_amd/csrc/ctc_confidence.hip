// CTC confidences on the device: how sure the model is of each frame, each token and each word of a hypothesis - the entropy-based frame
// confidence of Laptev & Ginsburg 2022 and its aggregation over a token's frames.  fp32 throughout (the same code in both libraries), no
// atomics, every sum in a fixed order, lengths read from DEVICE memory: nothing travels to the host and nothing synchronises.  The host
// path of confidence.py restates the laws in float32 numpy.
//
// Frame law for one row x[0..V) (it renormalises, so the row need not sum to 1):
//   m = max x ; d = x - m ; e = exp(d) ; s = sum e
//   max_prob   c = (V / s - 1) / (V - 1)
//   entropy    c = 1 + (sum_{e > 0} e d / s - ln s) / ln V
//   tsallis a  c = (sum exp(a d) / exp(a ln s) - u) / (1 - u),  u = exp((1 - a) ln V)
//   result     c >= 0 ? min(c, 1) : 0;  a NaN entry and a row without a finite maximum give 0, a -inf entry adds 0 to every sum
// conf_row is that law for ONE wavefront and one row, and the argmax of av_ctc_greedy (first maximal index) from the same registers; both
// kernels below call it, so the fused kernel's confidences are the frame kernel's bit for bit.  A row of V <= 2048 is loaded once into
// registers (16-byte loads where the row base and V allow them, 4-byte loads otherwise), its maximum taken, then every sum from those
// registers; a longer row is read a second time.  Reductions across the wave are shuffles: no LDS, no cross-workgroup state.
//   ctc_frame_conf_kernel     four rows (wavefronts) per workgroup
//   ctc_span_conf_kernel      one thread per (utterance, span): the aggregation in frame order
//   ctc_greedy_timed_kernel   ctc_greedy_kernel's structure (csrc/decode.hip), one workgroup per utterance: a wavefront per frame leaves argmax and
//                             confidence in LDS, one lane collapses the path into runs, then every thread writes one output position
// Out-of-range data cannot cause out-of-bounds accesses: T_b is clamped to [0, T], spans are clipped to [0, T_b).
#include "ctc_common.h"

namespace {

constexpr int CONF_MAXT = 4096;
constexpr int CONF_REGS = 32;                     // row elements a lane keeps in registers: 64 lanes x 32 = rows of up to 2048
constexpr int CONF_ROWS = 4;                      // frame rows (wavefronts) per workgroup

// first maximal index, as torch.argmax and ctc_greedy_kernel: a NaN never wins
__device__ __forceinline__ void conf_take(float x, int v, float& best, int& bi) {
    if (x > best || (x == best && v < bi)) { best = x; bi = v; }
}

template <int METHOD> __device__ __forceinline__ void conf_add(float x, float m, float alpha, float& s, float& r) {
    const float d = x - m;
    const float e = expf(d);
    s += e;
    if (METHOD == AV_CONF_ENTROPY) { if (e > 0.f) r += e * d; }
    if (METHOD == AV_CONF_TSALLIS) r += expf(alpha * d);
}

template <int METHOD> __device__ __forceinline__ float conf_finish(float s, float r, int V, float alpha) {
    const float fV = (float)V;
    float c;
    if (METHOD == AV_CONF_MAX_PROB) {
        c = (fV / s - 1.f) / (fV - 1.f);
    } else if (METHOD == AV_CONF_ENTROPY) {
        c = 1.f + (r / s - logf(s)) / logf(fV);
    } else {
        const float u = expf((1.f - alpha) * logf(fV));
        c = (r / expf(alpha * logf(s)) - u) / (1.f - u);
    }
    return c >= 0.f ? fminf(c, 1.f) : 0.f;        // NaN fails the comparison
}

// One wavefront, one row -> its confidence (the same value in every lane) and its argmax.  VEC: row is 16-byte aligned and V % 4 == 0.
template <bool VEC, int METHOD>
__device__ __forceinline__ float conf_row(const float* __restrict__ row, int V, int lane, float alpha, int& arg) {
    float best = -INFINITY, s = 0.f, r = 0.f;
    int bi = 0x7fffffff;
    const bool fits = V <= AV_WAVE * CONF_REGS;
    float x[CONF_REGS];
    const int n = VEC ? V >> 2 : V;                // loads of the row
    const int nk = (n + AV_WAVE - 1) / AV_WAVE;    // loads per lane, the same in every lane
    if (fits) {
        if (VEC) {
            const f32x4* p = (const f32x4*)row;
#pragma unroll
            for (int k = 0; k < CONF_REGS / 4; ++k) {
                if (k < nk) {
                    const int c = lane + AV_WAVE * k;
                    const f32x4 v = c < n ? p[c] : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                    x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
                }
            }
#pragma unroll
            for (int k = 0; k < CONF_REGS / 4; ++k) {
                const int c = lane + AV_WAVE * k;
                if (k < nk && c < n) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) conf_take(x[4 * k + e], 4 * c + e, best, bi);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < CONF_REGS; ++k) {
                if (k < nk) {
                    const int c = lane + AV_WAVE * k;
                    x[k] = c < n ? row[c] : -INFINITY;
                }
            }
#pragma unroll
            for (int k = 0; k < CONF_REGS; ++k) {
                const int c = lane + AV_WAVE * k;
                if (k < nk && c < n) conf_take(x[k], c, best, bi);
            }
        }
    } else if (VEC) {
        const f32x4* p = (const f32x4*)row;
        for (int c = lane; c < n; c += AV_WAVE) {
            const f32x4 v = p[c];
            conf_take(v.x, 4 * c, best, bi); conf_take(v.y, 4 * c + 1, best, bi);
            conf_take(v.z, 4 * c + 2, best, bi); conf_take(v.w, 4 * c + 3, best, bi);
        }
    } else {
        for (int c = lane; c < n; c += AV_WAVE) conf_take(row[c], c, best, bi);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        conf_take(ob, oi, best, bi);
    }
    arg = bi == 0x7fffffff ? 0 : bi;
    const float m = best;
    if (!(fabsf(m) < INFINITY)) return 0.f;        // all -inf (or all NaN), or a +inf entry; m is the same in every lane
    if (fits) {
        if (VEC) {
#pragma unroll
            for (int k = 0; k < CONF_REGS / 4; ++k) {
                if (k < nk) {                      // a lane without this load holds -inf: 0 to every sum
#pragma unroll
                    for (int e = 0; e < 4; ++e) conf_add<METHOD>(x[4 * k + e], m, alpha, s, r);
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < CONF_REGS; ++k) {
                if (k < nk) conf_add<METHOD>(x[k], m, alpha, s, r);
            }
        }
    } else if (VEC) {
        const f32x4* p = (const f32x4*)row;
        for (int c = lane; c < n; c += AV_WAVE) {
            const f32x4 v = p[c];
            conf_add<METHOD>(v.x, m, alpha, s, r); conf_add<METHOD>(v.y, m, alpha, s, r);
            conf_add<METHOD>(v.z, m, alpha, s, r); conf_add<METHOD>(v.w, m, alpha, s, r);
        }
    } else {
        for (int c = lane; c < n; c += AV_WAVE) conf_add<METHOD>(row[c], m, alpha, s, r);
    }
    s = wave_sum(s);
    if (METHOD != AV_CONF_MAX_PROB) r = wave_sum(r);
    return conf_finish<METHOD>(s, r, V, alpha);
}

// The aggregation of conf[f, e), f < e, in frame order (conf may live in LDS or in global memory).
__device__ __forceinline__ float conf_aggregate(const float* conf, int f, int e, int aggregation) {
    float acc = conf[f];
    if (aggregation == AV_AGG_MEAN) {
        for (int t = f + 1; t < e; ++t) acc += conf[t];
        return acc / (float)(e - f);
    }
    if (aggregation == AV_AGG_MIN) {
        for (int t = f + 1; t < e; ++t) acc = fminf(acc, conf[t]);
        return acc;
    }
    for (int t = f + 1; t < e; ++t) acc *= conf[t];
    return acc;
}

template <bool VEC, int METHOD>
__global__ __launch_bounds__(64 * CONF_ROWS) void ctc_frame_conf_kernel(const float* __restrict__ lp, long long stride_b, long long stride_t,
                                                                        const long long* __restrict__ lengths, int B, int T, int V, float alpha,
                                                                        float* __restrict__ conf) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * CONF_ROWS + w;
    if (i >= (long long)B * T) return;
    const int b = (int)(i / T), t = (int)(i % T);
    float c = 0.f;
    if (t < ctc_clamp_len(lengths, b, T)) {
        int arg;
        c = conf_row<VEC, METHOD>(lp + (long long)b * stride_b + (long long)t * stride_t, V, lane, alpha, arg);
    }
    if (lane == 0) conf[i] = c;
}

__global__ __launch_bounds__(256) void ctc_span_conf_kernel(const float* __restrict__ conf, const int* __restrict__ spans,
                                                            const long long* __restrict__ lengths, int B, int T, int L, int aggregation,
                                                            float* __restrict__ token_conf) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)B * L) return;
    const int b = (int)(i / L);
    const int f = max(spans[2 * i], 0), e = min(spans[2 * i + 1], ctc_clamp_len(lengths, b, T));
    token_conf[i] = f < e ? conf_aggregate(conf + (long long)b * T, f, e, aggregation) : 0.f;
}

template <bool VEC, int METHOD>
__global__ __launch_bounds__(256) void ctc_greedy_timed_kernel(const float* __restrict__ lp, long long stride_b, long long stride_t,
                                                               const long long* __restrict__ lengths, int T, int V, int blank, float alpha,
                                                               int aggregation, int* __restrict__ out_ids, int* __restrict__ out_len,
                                                               int* __restrict__ out_span, float* __restrict__ token_conf,
                                                               float* __restrict__ frame_conf) {
    __shared__ int ids[CONF_MAXT];                     // argmax per frame
    __shared__ float cf[CONF_MAXT];                    // confidence per frame
    __shared__ unsigned short first[CONF_MAXT], end[CONF_MAXT];      // the run of equal argmax frames behind emitted id j
    __shared__ int count;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int Tb = ctc_clamp_len(lengths, b, T);
    const float* base = lp + (long long)b * stride_b;
    for (int t = w; t < Tb; t += 4) {
        int arg;
        const float c = conf_row<VEC, METHOD>(base + (long long)t * stride_t, V, lane, alpha, arg);
        if (lane == 0) { ids[t] = arg; cf[t] = c; }
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0, prev = -1;
        bool open = false;
        for (int t = 0; t < Tb; ++t) {
            const int i = ids[t];
            if (i != prev) {                           // repeats collapsed, blanks dropped: av_ctc_greedy's ids
                if (open) end[n - 1] = (unsigned short)t;
                open = i != blank;
                if (open) first[n++] = (unsigned short)t;
                prev = i;
            }
        }
        if (open) end[n - 1] = (unsigned short)Tb;
        count = n;
        out_len[b] = n;
    }
    __syncthreads();
    const int n = count;
    for (int j = tid; j < T; j += blockDim.x) {
        const long long o = (long long)b * T + j;
        const int f = j < n ? (int)first[j] : -1, e = j < n ? (int)end[j] : -1;
        out_ids[o] = j < n ? ids[f] : -1;
        out_span[2 * o] = f;
        out_span[2 * o + 1] = e;
        token_conf[o] = j < n ? conf_aggregate(cf, f, e, aggregation) : 0.f;
        frame_conf[o] = j < Tb ? cf[j] : 0.f;
    }
}

int conf_check_rows(const char* who, const float* lp, long long stride_b, long long stride_t, int B, int T, int V, int method, float alpha) {
    AV_CHECK(B >= 0 && T >= 1 && T <= CONF_MAXT && V >= 2, "%s: bad shape B=%d T=%d V=%d (B >= 0, 1 <= T <= %d, V >= 2)", who, B, T, V, CONF_MAXT);
    AV_CHECK(method == AV_CONF_MAX_PROB || method == AV_CONF_ENTROPY || method == AV_CONF_TSALLIS,
             "%s: unknown method %d (0 max_prob, 1 entropy, 2 tsallis)", who, method);
    if (method == AV_CONF_TSALLIS) {
        AV_CHECK(alpha > 0.f && alpha < INFINITY, "%s: the tsallis alpha must be finite and > 0, got %g", who, (double)alpha);
        AV_CHECK(fabsf(alpha - 1.f) >= 1.f / 64.f, "%s: tsallis alpha %g is within 1/64 of 1, where the law loses its digits: use the entropy "
                 "method, its alpha -> 1 limit", who, (double)alpha);
    }
    return ctc_check_rows(who, stride_b, stride_t, B, T, V, true, "btBT");
}

bool conf_agg_ok(int a) { return a == AV_AGG_MEAN || a == AV_AGG_MIN || a == AV_AGG_PROD; }

// KERNEL<vec, method> by the runtime pair
#define CONF_DISPATCH(KERNEL, vec, method, ...)                                                               \
    do {                                                                                                      \
        if (vec) {                                                                                            \
            if (method == AV_CONF_MAX_PROB) KERNEL(true, AV_CONF_MAX_PROB, __VA_ARGS__);                      \
            else if (method == AV_CONF_ENTROPY) KERNEL(true, AV_CONF_ENTROPY, __VA_ARGS__);                   \
            else KERNEL(true, AV_CONF_TSALLIS, __VA_ARGS__);                                                  \
        } else {                                                                                              \
            if (method == AV_CONF_MAX_PROB) KERNEL(false, AV_CONF_MAX_PROB, __VA_ARGS__);                     \
            else if (method == AV_CONF_ENTROPY) KERNEL(false, AV_CONF_ENTROPY, __VA_ARGS__);                  \
            else KERNEL(false, AV_CONF_TSALLIS, __VA_ARGS__);                                                 \
        }                                                                                                     \
    } while (0)

}  // namespace

extern "C" int av_ctc_frame_conf(const float* log_probs, long long stride_b, long long stride_t, const long long* lengths, int B, int T, int V,
                                 int method, float alpha, float* conf, void* stream) {
    AV_CHECK(log_probs && conf, "av_ctc_frame_conf: null pointer");
    if (int rc = conf_check_rows("av_ctc_frame_conf", log_probs, stride_b, stride_t, B, T, V, method, alpha)) return rc;
    if (B == 0) return AV_OK;
    const bool vec = ctc_vec_ok(log_probs, nullptr, stride_b, stride_t, V);
    const unsigned grid = (unsigned)av_cdiv((long long)B * T, CONF_ROWS);
#define CONF_FRAME(VEC_, METHOD_, ...)                                                                                                     \
    hipLaunchKernelGGL((ctc_frame_conf_kernel<VEC_, METHOD_>), dim3(grid), dim3(64 * CONF_ROWS), 0, (hipStream_t)stream, __VA_ARGS__)
    CONF_DISPATCH(CONF_FRAME, vec, method, log_probs, stride_b, stride_t, lengths, B, T, V, alpha, conf);
#undef CONF_FRAME
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_ctc_span_conf(const float* conf, const int* spans, const long long* lengths, int B, int T, int L, int aggregation,
                                float* token_conf, void* stream) {
    AV_CHECK(B >= 0 && T >= 1 && T <= CONF_MAXT && L >= 0, "av_ctc_span_conf: bad shape B=%d T=%d L=%d (B >= 0, 1 <= T <= %d, L >= 0)", B, T, L,
             CONF_MAXT);
    AV_CHECK(conf_agg_ok(aggregation), "av_ctc_span_conf: unknown aggregation %d (0 mean, 1 min, 2 prod)", aggregation);
    if (B == 0 || L == 0) return AV_OK;
    AV_CHECK(conf && spans && token_conf, "av_ctc_span_conf: null pointer");
    hipLaunchKernelGGL(ctc_span_conf_kernel, dim3((unsigned)av_cdiv((long long)B * L, 256)), dim3(256), 0, (hipStream_t)stream, conf, spans,
                       lengths, B, T, L, aggregation, token_conf);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_ctc_greedy_timed(const float* log_probs, long long stride_b, long long stride_t, const long long* lengths, int B, int T, int V,
                                   int blank, int method, float alpha, int aggregation, int* out_ids, int* out_len, int* out_span,
                                   float* token_conf, float* frame_conf, void* stream) {
    AV_CHECK(log_probs && out_ids && out_len && out_span && token_conf && frame_conf, "av_ctc_greedy_timed: null pointer");
    if (int rc = conf_check_rows("av_ctc_greedy_timed", log_probs, stride_b, stride_t, B, T, V, method, alpha)) return rc;
    if (int rc = ctc_check_blank("av_ctc_greedy_timed", blank, V)) return rc;
    AV_CHECK(conf_agg_ok(aggregation), "av_ctc_greedy_timed: unknown aggregation %d (0 mean, 1 min, 2 prod)", aggregation);
    if (B == 0) return AV_OK;
    const bool vec = ctc_vec_ok(log_probs, nullptr, stride_b, stride_t, V);
#define CONF_GREEDY(VEC_, METHOD_, ...)                                                                                                    \
    hipLaunchKernelGGL((ctc_greedy_timed_kernel<VEC_, METHOD_>), dim3(B), dim3(256), 0, (hipStream_t)stream, __VA_ARGS__)
    CONF_DISPATCH(CONF_GREEDY, vec, method, log_probs, stride_b, stride_t, lengths, T, V, blank, alpha, aggregation, out_ids, out_len, out_span,
                  token_conf, frame_conf);
#undef CONF_GREEDY
    AV_LAUNCH_CHECK();
    return AV_OK;
}
