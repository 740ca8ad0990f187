// The optimizer: fused Adam step (torch.optim.Adam defaults, model/trainer.py:34-39) with optional gradient scaling, and opt-in global-norm
// gradient clipping and learning-rate schedule decided on the device (av_adam_multi_ex), an opt-in exponential moving average of the
// weights kept by the same launch (av_adam_multi_ema), opt-in decoupled weight decay (AdamW) and a cosine schedule (av_adam_multi_wd) and
// the in-place exchange of weights and averages (av_param_swap_multi), and the accumulation of micro-batch gradients (av_grad_accum_multi).
// The four av_adam_multi* entry points fill one AdamLaunch record; adam_check validates it and adam_launch is the launch sequence.
#include "av_common.h"

namespace {

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long long n,
                            float lr, float b1, float b2, float eps, float bc1, float bc2_sqrt, float gscale) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float gi = g[i] * gscale;
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] -= (lr / bc1) * (mi / denom);
    }
}

// Multi-tensor kernels: one launch for every tensor of a table, one workgroup of 256 threads per chunk.  Chunk c covers elements
// [chunk_start[c], +chunk_elems) of tensor chunk_tensor[c], cut at the tensor's size.
struct ChunkSpan {
    int t;                 // tensor of this workgroup's chunk
    long long s0, s1;      // its elements [s0, s1)
};
__device__ __forceinline__ ChunkSpan chunk_span(const long long* __restrict__ sizes, const int* __restrict__ chunk_tensor,
                                                const long long* __restrict__ chunk_start, int chunk_elems) {
    const int c = blockIdx.x;
    const int t = chunk_tensor[c];
    const long long n = sizes[t];
    const long long s0 = chunk_start[c];
    long long s1 = s0 + chunk_elems;
    if (s1 > n) s1 = n;
    return {t, s0, s1};
}
// quad(e) for every group of 4 consecutive elements [e, e + 4) of the span - 16-byte accesses, so only where the caller's pointers are
// aligned and the span starts on a multiple of 4 - and one(i) for every element that is left: the tail, or the whole span.  UNROLL > 0
// asks for that unrolling of the quad loop.
template <int UNROLL = 0, class Quad, class One>
__device__ __forceinline__ void chunk_walk(const ChunkSpan& sp, bool aligned, Quad quad, One one) {
    long long i = sp.s0;
    if (aligned && (sp.s0 % 4 == 0)) {
        const long long nv = (sp.s1 - sp.s0) / 4;
        if constexpr (UNROLL > 0) {
#pragma unroll UNROLL
            for (long long q = threadIdx.x; q < nv; q += 256) quad(sp.s0 + 4 * q);
        } else {
            for (long long q = threadIdx.x; q < nv; q += 256) quad(sp.s0 + 4 * q);
        }
        i = sp.s0 + 4 * nv;
    }
    for (i += threadIdx.x; i < sp.s1; i += 256) one(i);
}

// Adam tables: ptrs[t] = {param, grad, exp_avg, exp_avg_sq, shadow}.  shadow (optional, 0 = none) is a bf16 copy of the parameter in the
// layout the compute kernels read (the perf path's cached weight): writing it here saves the separate cast pass over every trainable
// weight after each step.
__device__ __forceinline__ float adam_one(float& p, float g, float& m, float& v, float b1, float b2, float eps, float step_size, float bc2_sqrt,
                                          float gscale) {
    const float gi = g * gscale;
    m = b1 * m + (1.f - b1) * gi;
    v = b2 * v + (1.f - b2) * gi * gi;
    p -= step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
    return p;
}
// Loss-scaling state on the device (torch.amp.GradScaler semantics without the host synchronisation of its found_inf.item()):
// gs[0] scale, gs[1] 1/scale, gs[2] found_inf (0/1), gs[3] growth tracker, gs[4] optimizer steps actually taken.
enum { GS_SCALE = 0, GS_INV = 1, GS_INF = 2, GS_TRACK = 3, GS_STEP = 4 };

// any non-finite gradient element -> gs[GS_INF] = 1   (torch/amp/grad_scaler.py:_unscale_grads_: _amp_foreach_non_finite_check_and_unscale_;
// the unscale itself is folded into the Adam kernel)
__global__ __launch_bounds__(256) void grad_check_multi_kernel(const unsigned long long* __restrict__ ptrs, const long long* __restrict__ sizes,
                                                               const int* __restrict__ chunk_tensor, const long long* __restrict__ chunk_start,
                                                               int chunk_elems, float* __restrict__ gs) {
    const ChunkSpan sp = chunk_span(sizes, chunk_tensor, chunk_start, chunk_elems);
    const float* g = (const float*)ptrs[5 * sp.t + 1];
    bool bad = false;                                             // "x || bad": kept as a lane mask in scalar registers; "bad |= x" is not
    chunk_walk(sp, (uintptr_t)g % 16 == 0,
        [&](long long e) {
            const f32x4 gg = *(const f32x4*)(g + e);
            // x - x is 0 for finite x and NaN for +-inf / NaN
            const float z = (gg[0] - gg[0]) + (gg[1] - gg[1]) + (gg[2] - gg[2]) + (gg[3] - gg[3]);
            bad = !(z == 0.f) || bad;
        },
        [&](long long i) { const float x = g[i]; bad = !((x - x) == 0.f) || bad; });
    if (__any(bad) && (threadIdx.x & 63) == 0) gs[GS_INF] = 1.0f;          // every writer stores the same value
}

// Global-norm gradient clipping and the learning-rate schedule of av_adam_multi_ex.  Clip / schedule state on the device, four 32-bit
// words:
//   cs[CS_NORM]  float  L2 norm of the gradients as the Adam kernel sees them (grad * grad_scale, / scale under loss scaling),
//   cs[CS_COEF]  float  min(1, max_norm / (norm + 1e-6)) in fp32 - torch.nn.utils.clip_grad_norm_ with error_if_nonfinite=False; nothing
//                       is special-cased: a NaN norm gives NaN, an infinite one 0; 1 when clipping is off,
//   cs[CS_LRM]   float  learning-rate multiplier of this step (lr_multiplier below),
//   cs[CS_K]     int32  optimizer steps taken so far on the schedule (advanced by adam_finish_kernel, not by a skipped step).
enum { CS_NORM = 0, CS_COEF = 1, CS_LRM = 2, CS_K = 3 };

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// sum over the workgroup in a fixed order (valid in thread 0)
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    v = wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// partial[c] = sum of g^2 over chunk c of the Adam launch's tables, accumulated in double: the square of an fp32 value is exact in fp64
// and cannot overflow it, so the sum is non-finite if and only if an element is, and the norm is good to an fp32 ulp.  The kernel is
// bound by reading the gradients; no atomics, a fixed order of additions: the same bits on every run.
__global__ __launch_bounds__(256) void grad_sumsq_multi_kernel(const unsigned long long* __restrict__ ptrs, const long long* __restrict__ sizes,
                                                               const int* __restrict__ chunk_tensor, const long long* __restrict__ chunk_start,
                                                               int chunk_elems, double* __restrict__ partial) {
    __shared__ double red[4];
    const ChunkSpan sp = chunk_span(sizes, chunk_tensor, chunk_start, chunk_elems);
    const float* g = (const float*)ptrs[5 * sp.t + 1];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    chunk_walk<4>(sp, (uintptr_t)g % 16 == 0,
        [&](long long e) {
            const f32x4 gg = *(const f32x4*)(g + e);
            const double x0 = gg[0], x1 = gg[1], x2 = gg[2], x3 = gg[3];
            a0 = fma(x0, x0, a0); a1 = fma(x1, x1, a1); a2 = fma(x2, x2, a2); a3 = fma(x3, x3, a3);
        },
        [&](long long i) { const double x = g[i]; a0 = fma(x, x, a0); });
    const double s = block_sum_f64((a0 + a1) + (a2 + a3), red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// HF get_linear_schedule_with_warmup under LambdaLR: step k (0-based, steps actually taken) runs at k / warmup below warmup, then at
// max(0, (total - k) / (total - warmup)); total == 0: constant 1 after the warmup.  schedule == LR_COSINE (av_adam_multi_wd; total > warmup):
// after the same warmup max(0, 0.5 * (1 + cos(pi * x))), x = (k - warmup) / (total - warmup) - HF get_cosine_schedule_with_warmup with
// num_cycles = 0.5 - and 0 from k = total on (HF's lambda rises again there).  optim.lr_multiplier is the same law on the host.
enum { LR_LINEAR = 0, LR_COSINE = 1 };
__device__ __forceinline__ float lr_multiplier(int k, int warmup, int total, int schedule) {
    if (k < warmup) return (float)((double)k / (double)warmup);
    if (schedule == LR_COSINE) {
        if (k >= total) return 0.f;
        const double x = (double)(k - warmup) / (double)(total - warmup);
        const double m = 0.5 * (1.0 + cos(3.14159265358979323846 * x));
        return (float)(m > 0.0 ? m : 0.0);
    }
    if (total == 0) return 1.f;
    const double m = (double)(total - k) / (double)(total - warmup);
    return (float)(m > 0.0 ? m : 0.0);
}

// one workgroup: the chunk partials summed in a fixed order -> norm, clip coefficient, found_inf (with clipping this pass replaces
// grad_check_multi_kernel), and this step's learning-rate multiplier.  partial == NULL: clipping is off (schedule only).
__global__ __launch_bounds__(256) void clip_finalize_kernel(const double* __restrict__ partial, int n_chunks, float gscale, float max_norm,
                                                            int warmup, int total, float* __restrict__ gs, float* __restrict__ cs,
                                                            int schedule) {
    __shared__ double red[4];
    double a = 0.0;
    if (partial)
        for (int i = threadIdx.x; i < n_chunks; i += 256) a += partial[i];
    const double ss = block_sum_f64(a, red);
    if (threadIdx.x != 0) return;
    float norm = 0.f, coef = 1.f;
    if (partial) {
        if (gs) {
            if (!(ss - ss == 0.0)) gs[GS_INF] = 1.0f;
            gscale *= gs[GS_INV];
        }
        norm = (float)(sqrt(ss) * (double)fabsf(gscale));
        coef = max_norm / (norm + 1e-6f);
        coef = coef > 1.f ? 1.f : coef;                           // a NaN stays (torch.clamp(max=1.0))
    }
    cs[CS_NORM] = norm;
    cs[CS_COEF] = coef;
    cs[CS_LRM] = lr_multiplier(((const int*)cs)[CS_K], warmup, total, schedule);
}

// Exponential moving average of the weights (av_adam_multi_ema).  EMA state on the device, two 32-bit words:
//   es[ES_DECAY] float  decay d_k of this step's update (ema_decay_kernel below; every workgroup reads it from here),
//   es[ES_K]     int32  EMA updates so far (advanced by adam_finish_kernel, not by a skipped step).
enum { ES_DECAY = 0, ES_K = 1 };

// one thread, the one-thread sibling of clip_finalize_kernel: d_0 = 0 (the first update copies the parameters:
// torch.optim.swa_utils.AveragedModel's n_averaged == 0), then d_k = decay, or min(decay, (1 + k) / (10 + k)) with the warmup of
// TensorFlow's ExponentialMovingAverage and timm's ModelEmaV2; in double, stored as a float.  optim.ema_decay is the same law on the host.
__global__ void ema_decay_kernel(float decay, int warmup, float* __restrict__ es) {
    const int k = ((const int*)es)[ES_K];
    double d = 0.0;
    if (k >= 1) {
        d = (double)decay;
        if (warmup) {
            const double w = (1.0 + (double)k) / (10.0 + (double)k);
            d = w < d ? w : d;
        }
    }
    es[ES_DECAY] = (float)d;
}

// torch.lerp(ema, p, w) written out (ATen/native/Lerp.h), w = 1 - d: below 0.5 from the start point, otherwise from the end point, so
// that w == 1 gives p exactly.  omw = 1 - w.
__device__ __forceinline__ float ema_one(float ema, float p, float w, float omw) {
    const float diff = p - ema;
    return w < 0.5f ? ema + w * diff : p - diff * omw;
}

// torch/amp/grad_scaler.py:update (_amp_update_scale_) is applied by adam_finish_kernel below: found_inf -> scale *= backoff, tracker = 0;
// otherwise tracker += 1 and scale *= growth when it reaches the interval; it also counts the optimizer steps that were not skipped.

// Per-tensor step counts live on the device (int32 table; tensor t of a launch owns slot step_slot[t]): a parameter that received no
// gradient in some step (LayerDrop skipped its layer in both passes: torch.optim.Adam leaves its state['step'] behind) keeps its own bias
// corrections, every step goes through THIS kernel, and under loss scaling a skipped (overflowing) step advances no counter - all without
// the host knowing.  hyper[t] = {lr, beta1, beta2, eps}.  Bias corrections in double (1 - beta2^step loses half its digits in fp32).
// EMA (av_adam_multi_ema): ema_ptrs[t] is the fp32 average of tensor t, moved towards the updated parameter while that is still in a
// register; the EMA = false instantiation is the kernel of av_adam_multi / av_adam_multi_ex, statement for statement.
// WD (av_adam_multi_wd): decoupled weight decay, torch.optim.AdamW's param.mul_(1 - lr * weight_decay) ahead of the update: wd[t] = lambda_t
// and f_t = 1 - lr_t * lr_mult * lambda_t, once per workgroup in double, stored as a float; p * f_t is rounded on its own (__fmul_rn: never
// contracted into the update), the gradient and the moments do not see it, shadow and EMA are written from the decayed, updated value.
// The WD = false instantiations do not read wd and are the kernels they were.
template <bool EMA, bool WD>
__global__ __launch_bounds__(256) void adam_multi_kernel(const unsigned long long* __restrict__ ptrs, const long long* __restrict__ sizes,
                                                         const f32x4* __restrict__ hyper, const int* __restrict__ chunk_tensor,
                                                         const long long* __restrict__ chunk_start, int chunk_elems,
                                                         const int* __restrict__ steps, const int* __restrict__ step_slot, float gscale,
                                                         const float* __restrict__ gs, const float* __restrict__ cs,
                                                         const unsigned long long* __restrict__ ema_ptrs, const float* __restrict__ es,
                                                         const float* __restrict__ wd) {
    if (gs) {                                                    // loss scaling: skip on overflow, unscale
        if (gs[GS_INF] != 0.f) return;
        gscale *= gs[GS_INV];
    }
    float lr_mult = 1.f;
    if (cs) {                                                    // av_adam_multi_ex: clip by the global norm, follow the schedule
        gscale *= cs[CS_COEF];
        lr_mult = cs[CS_LRM];
    }
    const ChunkSpan sp = chunk_span(sizes, chunk_tensor, chunk_start, chunk_elems);
    const int t = sp.t;
    const f32x4 hp = hyper[t];
    const float b1 = hp[1], b2 = hp[2], eps = hp[3];
    const double step = (double)(steps[step_slot[t]] + 1);
    const float bc1 = (float)(1.0 - pow((double)b1, step));
    const float bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, step));
    float* p = (float*)ptrs[5 * t + 0];
    const float* g = (const float*)ptrs[5 * t + 1];
    float* m = (float*)ptrs[5 * t + 2];
    float* v = (float*)ptrs[5 * t + 3];
    bf16_t* sh = (bf16_t*)ptrs[5 * t + 4];
    const float step_size = cs ? hp[0] * lr_mult / bc1 : hp[0] / bc1;
    float* ema = nullptr;
    float ew = 0.f, eomw = 0.f;                                  // lerp weight 1 - d_k and 1 - weight
    if constexpr (EMA) {
        ema = (float*)ema_ptrs[t];
        ew = 1.f - es[ES_DECAY];
        eomw = 1.f - ew;
    }
    float wf = 1.f;                                              // decay factor f_t
    if constexpr (WD) wf = (float)(1.0 - (double)hp[0] * (double)lr_mult * (double)wd[t]);
    chunk_walk(sp, (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) % 16 == 0) && ((uintptr_t)sh % 8 == 0),
        [&](long long e) {
            f32x4 pp = *(const f32x4*)(p + e), mm = *(const f32x4*)(m + e), vv = *(const f32x4*)(v + e);
            const f32x4 gg = *(const f32x4*)(g + e);
            f32x4 ee;
            if constexpr (EMA) ee = *(const f32x4*)(ema + e);
            bf16x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float pk = pp[k], mk = mm[k], vk = vv[k];
                if constexpr (WD) pk = __fmul_rn(pk, wf);
                o[k] = (bf16_t)adam_one(pk, gg[k], mk, vk, b1, b2, eps, step_size, bc2_sqrt, gscale);
                pp[k] = pk; mm[k] = mk; vv[k] = vk;
                if constexpr (EMA) ee[k] = ema_one(ee[k], pk, ew, eomw);
            }
            *(f32x4*)(p + e) = pp; *(f32x4*)(m + e) = mm; *(f32x4*)(v + e) = vv;
            if (sh) *(bf16x4*)(sh + e) = o;
            if constexpr (EMA) *(f32x4*)(ema + e) = ee;
        },
        [&](long long i) {
            float pp = p[i], mm = m[i], vv = v[i];
            if constexpr (WD) pp = __fmul_rn(pp, wf);
            const float r = adam_one(pp, g[i], mm, vv, b1, b2, eps, step_size, bc2_sqrt, gscale);
            p[i] = pp; m[i] = mm; v[i] = vv;
            if (sh) sh[i] = (bf16_t)r;
            if constexpr (EMA) ema[i] = ema_one(ema[i], r, ew, eomw);
        });
}

// tensors that have an EMA but received no gradient in this step (LayerDrop skipped their layer in both passes: the Adam launch does not
// see them): ptrs[t] = {param, ema}, their own chunk tables; the average moves towards the unchanged parameter.  Skipped with the step.
__global__ __launch_bounds__(256) void ema_only_multi_kernel(const unsigned long long* __restrict__ ptrs, const long long* __restrict__ sizes,
                                                             const int* __restrict__ chunk_tensor, const long long* __restrict__ chunk_start,
                                                             int chunk_elems, const float* __restrict__ gs, const float* __restrict__ es) {
    if (gs && gs[GS_INF] != 0.f) return;
    const float ew = 1.f - es[ES_DECAY], eomw = 1.f - ew;
    const ChunkSpan sp = chunk_span(sizes, chunk_tensor, chunk_start, chunk_elems);
    const float* p = (const float*)ptrs[2 * sp.t + 0];
    float* ema = (float*)ptrs[2 * sp.t + 1];
    chunk_walk(sp, ((uintptr_t)p | (uintptr_t)ema) % 16 == 0,
        [&](long long e) {
            const f32x4 pp = *(const f32x4*)(p + e);
            f32x4 ee = *(const f32x4*)(ema + e);
#pragma unroll
            for (int k = 0; k < 4; ++k) ee[k] = ema_one(ee[k], pp[k], ew, eomw);
            *(f32x4*)(ema + e) = ee;
        },
        [&](long long i) { ema[i] = ema_one(ema[i], p[i], ew, eomw); });
}

// av_param_swap_multi: ptrs[t] = {param, ema, shadow}; param and ema change places element by element (both in registers: no temporary copy
// of the model), and the 16-bit image of the new parameter goes to shadow (optional, 0 = none), as the Adam kernel writes it.
__global__ __launch_bounds__(256) void param_swap_multi_kernel(const unsigned long long* __restrict__ ptrs, const long long* __restrict__ sizes,
                                                               const int* __restrict__ chunk_tensor, const long long* __restrict__ chunk_start,
                                                               int chunk_elems) {
    const ChunkSpan sp = chunk_span(sizes, chunk_tensor, chunk_start, chunk_elems);
    float* p = (float*)ptrs[3 * sp.t + 0];
    float* ema = (float*)ptrs[3 * sp.t + 1];
    bf16_t* sh = (bf16_t*)ptrs[3 * sp.t + 2];
    chunk_walk(sp, (((uintptr_t)p | (uintptr_t)ema) % 16 == 0) && ((uintptr_t)sh % 8 == 0),
        [&](long long e) {
            const f32x4 pp = *(const f32x4*)(p + e), ee = *(const f32x4*)(ema + e);
            *(f32x4*)(p + e) = ee; *(f32x4*)(ema + e) = pp;
            if (sh) {
                bf16x4 o;
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = (bf16_t)ee[k];
                *(bf16x4*)(sh + e) = o;
            }
        },
        [&](long long i) {
            const float pp = p[i], ee = ema[i];
            p[i] = ee; ema[i] = pp;
            if (sh) sh[i] = (bf16_t)ee;
        });
}

// av_grad_accum_multi: ptrs[t] = {grad, acc}, both fp32, not overlapping.  mode[t] == 0: acc = grad, the tensor's first contribution of an
// accumulation cycle - no clearing pass, no read of stale memory, and the bits of the gradient (a -0.0 stays -0.0, which 0 + g would not
// keep): autograd's first .grad is the gradient itself.  mode[t] == 1: acc = acc + grad, one fp32 add per element: nothing to contract,
// non-finite values propagate by IEEE arithmetic, no LDS, no atomics, every element written by one thread: the same bits whatever the grid.
// The mode is uniform over a workgroup.  Bound by 12 B (add) or 8 B (copy) per element.  The quad loop is not unrolled: on the headline
// configuration's 64.9 M elements chunk_walk<4> (30 VGPRs instead of 16) measured 0.159 / 0.101 ms for add / copy against 0.159 / 0.102 ms
// without, 4.9 and 5.1 TB/s either way (tools/accum_timing.py, profiles/grad_accum_timing.txt): eight waves per SIMD keep enough loads in flight.
__global__ __launch_bounds__(256) void grad_accum_multi_kernel(const unsigned long long* __restrict__ ptrs, const int* __restrict__ mode,
                                                               const long long* __restrict__ sizes, const int* __restrict__ chunk_tensor,
                                                               const long long* __restrict__ chunk_start, int chunk_elems) {
    const ChunkSpan sp = chunk_span(sizes, chunk_tensor, chunk_start, chunk_elems);
    const float* g = (const float*)ptrs[2 * sp.t + 0];
    float* a = (float*)ptrs[2 * sp.t + 1];
    const bool aligned = ((uintptr_t)g | (uintptr_t)a) % 16 == 0;
    if (mode[sp.t] == 0)
        chunk_walk(sp, aligned,
            [&](long long e) { *(f32x4*)(a + e) = *(const f32x4*)(g + e); },
            [&](long long i) { a[i] = g[i]; });
    else
        chunk_walk(sp, aligned,
            [&](long long e) { *(f32x4*)(a + e) = *(const f32x4*)(a + e) + *(const f32x4*)(g + e); },
            [&](long long i) { a[i] = a[i] + g[i]; });
}

// after the Adam launch (stream order): the tensors of that launch have taken one more step - unless the step was skipped for overflow.
// With a scaler this launch also applies the GradScaler update law (one thread); sched_k (optional) is the schedule's step counter, ema_k
// (optional) the count of EMA updates.
__global__ void adam_finish_kernel(int* __restrict__ steps, const int* __restrict__ step_slot, int n_tensors, float* __restrict__ gs,
                                   float growth, float backoff, int interval, int* __restrict__ sched_k, int* __restrict__ ema_k) {
    const bool skipped = gs && gs[GS_INF] != 0.f;
    __syncthreads();                                              // everyone has read found_inf before thread 0 clears it
    if (!skipped) {
        for (int t = threadIdx.x; t < n_tensors; t += blockDim.x) steps[step_slot[t]] += 1;
        if (sched_k && threadIdx.x == 0) sched_k[0] += 1;
        if (ema_k && threadIdx.x == 0) ema_k[0] += 1;
    }
    if (gs && threadIdx.x == 0) {
        if (skipped) {
            gs[GS_SCALE] *= backoff;
            gs[GS_TRACK] = 0.f;
        } else {
            gs[GS_STEP] += 1.f;
            const float tr = gs[GS_TRACK] + 1.f;
            if (tr >= (float)interval) { gs[GS_SCALE] *= growth; gs[GS_TRACK] = 0.f; }
            else gs[GS_TRACK] = tr;
        }
        gs[GS_INV] = 1.0f / gs[GS_SCALE];
        gs[GS_INF] = 0.f;
    }
}

inline int ew_grid(long long n) {
    long long b = (n + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// One fused step, as the four av_adam_multi* entry points describe it.  An entry point fills the members it has arguments for; the rest
// stay zero, which is "off" for each of them (max_norm 0: no clipping, both step counts 0: no schedule, decay 0: no EMA, weight_decay NULL:
// no decay, lr_schedule 0: the linear law).
struct EmaArgs {
    const void* ema_ptrs;
    const void* only_ptrs;
    const long long* only_sizes;
    const int* only_chunk_tensor;
    const long long* only_chunk_start;
    int n_only_chunks;
    float decay;
    int warmup;
    float* state;
};
struct AdamLaunch {
    // av_adam_multi: the Adam tables, the step table, and the loss-scaling block with the constants of its update law
    const unsigned long long* ptrs; const long long* sizes; const float* hyper; const int* chunk_tensor; const long long* chunk_start;
    int n_chunks, chunk_elems; int* steps; const int* step_slot; int n_tensors;
    float grad_scale; float* scaler_state; float growth, backoff; int growth_interval;
    // av_adam_multi_ex: clipping and schedule
    float max_norm; int warmup_steps, total_steps; void* workspace; long long workspace_bytes; float* clip_state;
    // av_adam_multi_ema
    EmaArgs ema;
    // av_adam_multi_wd
    const float* weight_decay; int lr_schedule;

    bool clip() const { return max_norm > 0.f; }
    bool sched() const { return warmup_steps > 0 || total_steps > 0; }
    bool averaging() const { return ema.decay > 0.f; }
};

int adam_check(const char* who, const AdamLaunch& a) {
    const EmaArgs& ea = a.ema;
    AV_CHECK(a.ptrs && a.sizes && a.hyper && a.chunk_tensor && a.chunk_start && a.steps && a.step_slot && a.n_chunks >= 0 && a.n_tensors >= 0 &&
                 a.chunk_elems > 0,
             "%s: bad args", who);
    AV_CHECK(((uintptr_t)a.hyper % 16) == 0, "%s: hyper must be 16-byte aligned ([n_tensors][4] floats)", who);
    AV_CHECK(!a.scaler_state || a.growth_interval >= 1, "%s: bad growth interval", who);
    AV_CHECK(a.max_norm >= 0.f, "%s: max_norm must be >= 0 and not NaN (0 = no clipping)", who);
    AV_CHECK(a.warmup_steps >= 0 && a.total_steps >= 0 && (a.total_steps == 0 || a.total_steps > a.warmup_steps),
             "%s: bad schedule (warmup_steps %d, total_steps %d: total_steps must be 0 or above warmup_steps)", who, a.warmup_steps, a.total_steps);
    AV_CHECK(a.lr_schedule == LR_LINEAR || a.lr_schedule == LR_COSINE, "%s: lr_schedule must be 0 (linear) or 1 (cosine), got %d", who,
             a.lr_schedule);
    AV_CHECK(a.lr_schedule != LR_COSINE || a.total_steps > 0, "%s: the cosine schedule needs total_steps > warmup_steps", who);
    AV_CHECK(a.lr_schedule != LR_COSINE || a.clip_state, "%s: the cosine schedule needs the state block", who);
    AV_CHECK(((uintptr_t)a.weight_decay % 4) == 0, "%s: the weight_decay table must be 4-byte aligned ([n_tensors] floats)", who);
    const bool clip = a.clip(), sched = a.sched();
    AV_CHECK(!(clip || sched) || a.clip_state, "%s: clipping or a schedule needs the state block", who);
    AV_CHECK(!(clip || sched) || ((uintptr_t)a.clip_state % 4) == 0, "%s: the state block must be 4-byte aligned", who);
    AV_CHECK(!clip || (a.workspace && ((uintptr_t)a.workspace % 8) == 0 && a.workspace_bytes >= 8LL * a.n_chunks),
             "%s: clipping needs a workspace of av_grad_norm_workspace_bytes(n_chunks) bytes, 8-byte aligned", who);
    AV_CHECK(ea.decay >= 0.f && ea.decay < 1.f, "%s: ema_decay must be in [0, 1) and not NaN (0 = no EMA), got %g", who, (double)ea.decay);
    const bool ema = a.averaging();
    AV_CHECK(ema || (!ea.ema_ptrs && !ea.only_ptrs && ea.n_only_chunks == 0), "%s: EMA tables without an ema_decay", who);
    AV_CHECK(!ema || ea.ema_ptrs, "%s: ema_decay > 0 needs the EMA pointer table", who);
    AV_CHECK(!ema || (ea.n_only_chunks >= 0 && (ea.n_only_chunks == 0 || (ea.only_ptrs && ea.only_sizes && ea.only_chunk_tensor &&
                                                                          ea.only_chunk_start))),
             "%s: bad EMA-only tables (%d chunks)", who, ea.n_only_chunks);
    AV_CHECK(!ema || ea.state, "%s: ema_decay > 0 needs the EMA state block", who);
    AV_CHECK(!ema || ((uintptr_t)ea.state % 4) == 0, "%s: the EMA state block must be 4-byte aligned", who);
    return AV_OK;
}

// The launches of one step, in the order they run.  With clipping, schedule and EMA off only the lines of av_adam_multi are left:
// [grad_check, with a scaler] -> adam_multi_kernel<false, false> -> adam_finish.
int adam_launch(const AdamLaunch& a, hipStream_t st) {
    const EmaArgs& ea = a.ema;
    const bool clip = a.clip(), sched = a.sched(), ema = a.averaging();
    const bool adam = a.n_chunks > 0;                            // some tensor has a gradient
    const bool ema_run = ema && (adam || ea.n_only_chunks > 0);
    float* const gs = a.scaler_state;
    float* const cs = (clip || sched) ? a.clip_state : nullptr;
    const dim3 chunks(adam ? a.n_chunks : 1), one(1), wg(256);

    // 1. one read of the gradients: their sum of squares (which also finds a non-finite element), or only the non-finite check
    if (adam && clip)
        hipLaunchKernelGGL(grad_sumsq_multi_kernel, chunks, wg, 0, st, a.ptrs, a.sizes, a.chunk_tensor, a.chunk_start, a.chunk_elems,
                           (double*)a.workspace);
    else if (adam && gs)
        hipLaunchKernelGGL(grad_check_multi_kernel, chunks, wg, 0, st, a.ptrs, a.sizes, a.chunk_tensor, a.chunk_start, a.chunk_elems, gs);
    // 2. norm, clip coefficient and learning-rate multiplier of this step
    if (adam && cs)
        hipLaunchKernelGGL(clip_finalize_kernel, one, wg, 0, st, clip ? (const double*)a.workspace : (const double*)nullptr, a.n_chunks,
                           a.grad_scale, a.max_norm, a.warmup_steps, a.total_steps, gs, cs, a.lr_schedule);
    // 3. EMA decay of this step
    if (ema_run) hipLaunchKernelGGL(ema_decay_kernel, one, one, 0, st, ea.decay, ea.warmup, ea.state);
    // 4. Adam, with the decay and the EMA of the tensors it updates
    if (adam) {
        const bool wd = a.weight_decay != nullptr;
        auto* const kernel = ema ? (wd ? adam_multi_kernel<true, true> : adam_multi_kernel<true, false>)
                                 : (wd ? adam_multi_kernel<false, true> : adam_multi_kernel<false, false>);
        hipLaunchKernelGGL(kernel, chunks, wg, 0, st, a.ptrs, a.sizes, (const f32x4*)a.hyper, a.chunk_tensor, a.chunk_start, a.chunk_elems,
                           (const int*)a.steps, a.step_slot, a.grad_scale, (const float*)gs, (const float*)cs,
                           (const unsigned long long*)(ema ? ea.ema_ptrs : nullptr), (const float*)(ema ? ea.state : nullptr),
                           a.weight_decay);
    }
    // 5. EMA of the tensors without a gradient
    if (ema && ea.n_only_chunks > 0)
        hipLaunchKernelGGL(ema_only_multi_kernel, dim3(ea.n_only_chunks), wg, 0, st, (const unsigned long long*)ea.only_ptrs, ea.only_sizes,
                           ea.only_chunk_tensor, ea.only_chunk_start, a.chunk_elems, (const float*)gs, (const float*)ea.state);
    // 6. step counts, schedule step, EMA count, loss-scale update
    if (a.n_tensors > 0 || gs || ema_run)
        hipLaunchKernelGGL(adam_finish_kernel, one, wg, 0, st, a.steps, a.step_slot, a.n_tensors, gs, a.growth, a.backoff, a.growth_interval,
                           (sched && adam) ? (int*)cs + CS_K : (int*)nullptr, ema_run ? (int*)ea.state + ES_K : (int*)nullptr);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

int adam_step(const char* who, const AdamLaunch& a, void* stream) {
    const int rc = adam_check(who, a);
    return rc != AV_OK ? rc : adam_launch(a, (hipStream_t)stream);
}

}  // namespace

extern "C" int av_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                            int step, float grad_scale, void* stream) {
    AV_CHECK(p && g && m && v && step >= 1, "av_adam_step: bad args");
    if (n == 0) return AV_OK;
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    const float bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    hipLaunchKernelGGL(adam_kernel, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, lr, beta1, beta2, eps, bc1, bc2s, grad_scale);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
extern "C" int av_adam_multi(const void* ptrs, const long long* sizes, const float* hyper, const int* chunk_tensor, const long long* chunk_start,
                             int n_chunks, int chunk_elems, int* steps, const int* step_slot, int n_tensors, float grad_scale,
                             float* scaler_state, float growth, float backoff, int growth_interval, void* stream) {
    const AdamLaunch a = {(const unsigned long long*)ptrs, sizes, hyper, chunk_tensor, chunk_start, n_chunks, chunk_elems, steps, step_slot,
                          n_tensors, grad_scale, scaler_state, growth, backoff, growth_interval};
    return adam_step("av_adam_multi", a, stream);
}
extern "C" int av_grad_norm_workspace_bytes(int n_chunks, long long* bytes) {
    AV_CHECK(bytes && n_chunks >= 0, "av_grad_norm_workspace_bytes: bad args");
    *bytes = 8LL * (n_chunks > 0 ? n_chunks : 1);
    return AV_OK;
}
extern "C" int av_adam_multi_ex(const void* ptrs, const long long* sizes, const float* hyper, const int* chunk_tensor,
                                const long long* chunk_start, int n_chunks, int chunk_elems, int* steps, const int* step_slot, int n_tensors,
                                float grad_scale, float* scaler_state, float growth, float backoff, int growth_interval, float max_norm,
                                int warmup_steps, int total_steps, void* workspace, long long workspace_bytes, float* clip_state,
                                void* stream) {
    const AdamLaunch a = {(const unsigned long long*)ptrs, sizes, hyper, chunk_tensor, chunk_start, n_chunks, chunk_elems, steps, step_slot,
                          n_tensors, grad_scale, scaler_state, growth, backoff, growth_interval,
                          max_norm, warmup_steps, total_steps, workspace, workspace_bytes, clip_state};
    return adam_step("av_adam_multi_ex", a, stream);
}
extern "C" int av_adam_multi_ema(const void* ptrs, const long long* sizes, const float* hyper, const int* chunk_tensor,
                                 const long long* chunk_start, int n_chunks, int chunk_elems, int* steps, const int* step_slot, int n_tensors,
                                 float grad_scale, float* scaler_state, float growth, float backoff, int growth_interval, float max_norm,
                                 int warmup_steps, int total_steps, void* workspace, long long workspace_bytes, float* clip_state,
                                 const void* ema_ptrs, const void* ema_only_ptrs, const long long* ema_only_sizes,
                                 const int* ema_only_chunk_tensor, const long long* ema_only_chunk_start, int n_ema_only_chunks,
                                 float ema_decay, int ema_warmup, float* ema_state, void* stream) {
    const AdamLaunch a = {(const unsigned long long*)ptrs, sizes, hyper, chunk_tensor, chunk_start, n_chunks, chunk_elems, steps, step_slot,
                          n_tensors, grad_scale, scaler_state, growth, backoff, growth_interval,
                          max_norm, warmup_steps, total_steps, workspace, workspace_bytes, clip_state,
                          {ema_ptrs, ema_only_ptrs, ema_only_sizes, ema_only_chunk_tensor, ema_only_chunk_start, n_ema_only_chunks, ema_decay,
                           ema_warmup, ema_state}};
    return adam_step("av_adam_multi_ema", a, stream);
}
extern "C" int av_adam_multi_wd(const void* ptrs, const long long* sizes, const float* hyper, const int* chunk_tensor,
                                const long long* chunk_start, int n_chunks, int chunk_elems, int* steps, const int* step_slot, int n_tensors,
                                float grad_scale, float* scaler_state, float growth, float backoff, int growth_interval, float max_norm,
                                int warmup_steps, int total_steps, void* workspace, long long workspace_bytes, float* clip_state,
                                const void* ema_ptrs, const void* ema_only_ptrs, const long long* ema_only_sizes,
                                const int* ema_only_chunk_tensor, const long long* ema_only_chunk_start, int n_ema_only_chunks,
                                float ema_decay, int ema_warmup, float* ema_state, const float* weight_decay, int lr_schedule,
                                void* stream) {
    const AdamLaunch a = {(const unsigned long long*)ptrs, sizes, hyper, chunk_tensor, chunk_start, n_chunks, chunk_elems, steps, step_slot,
                          n_tensors, grad_scale, scaler_state, growth, backoff, growth_interval,
                          max_norm, warmup_steps, total_steps, workspace, workspace_bytes, clip_state,
                          {ema_ptrs, ema_only_ptrs, ema_only_sizes, ema_only_chunk_tensor, ema_only_chunk_start, n_ema_only_chunks, ema_decay,
                           ema_warmup, ema_state},
                          weight_decay, lr_schedule};
    return adam_step("av_adam_multi_wd", a, stream);
}
extern "C" int av_param_swap_multi(const void* ptrs, const long long* sizes, const int* chunk_tensor, const long long* chunk_start,
                                   int n_chunks, int chunk_elems, void* stream) {
    AV_CHECK(ptrs && sizes && chunk_tensor && chunk_start && n_chunks >= 0 && chunk_elems > 0, "av_param_swap_multi: bad args");
    if (n_chunks == 0) return AV_OK;
    hipLaunchKernelGGL(param_swap_multi_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)ptrs, sizes,
                       chunk_tensor, chunk_start, chunk_elems);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
extern "C" int av_grad_accum_multi(const void* ptrs, const int* mode, const long long* sizes, const int* chunk_tensor,
                                   const long long* chunk_start, int n_chunks, int chunk_elems, void* stream) {
    AV_CHECK(ptrs && mode && sizes && chunk_tensor && chunk_start && n_chunks >= 0 && chunk_elems > 0, "av_grad_accum_multi: bad args");
    if (n_chunks == 0) return AV_OK;
    hipLaunchKernelGGL(grad_accum_multi_kernel, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned long long*)ptrs, mode, sizes, chunk_tensor, chunk_start, chunk_elems);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
