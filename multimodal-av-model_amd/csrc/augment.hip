// Training-time data augmentation on the device (augment.py): the lip clips are shifted, mirrored and have frames frozen, the
// waveform gets additive noise at a drawn signal-to-noise ratio.  Every random choice is a draw of the counter-hash generator of av_common.h
// (drop_draw): a pure function of (seed, stream, index), so augment.py restates both laws on the host bit for bit and nothing is drawn, kept
// or transferred by the host.  Two HBM-bound passes (one read, one write of the tensor), no LDS and no atomics in them; the clip's plan is
// evaluated from workgroup-uniform values only, i.e. once per workgroup on the scalar unit.
//
//   index packing   c = step * 65536 + b  (b < 65536, step < 2^24): the "clip counter" of clip b at step `step`
//     lips   block c * 64 + g, g = 0 .. 63, of the speaker's stream                      (block < 2^46)
//     SNR    block c of AV_AUG_STREAM_SNR
//     noise  block (c << 24) + i of AV_AUG_STREAM_NOISE, i < N <= 2^24 the sample        (block < 2^64)
//   a block yields four 16-bit integers k0 .. k3 (low / high half of drop_draw's first word, then of its second); an integer in 0 .. R-1
//   is drawn as (k * R) >> 16.
#include "av_common.h"

namespace {

// the four 16-bit integers of block `blk`: drop_draw(seed, stream, 4 * blk) - restated from the block index because the noise blocks reach
// 2^64, where 4 * blk no longer fits the generator's 64-bit element index
__device__ __forceinline__ void aug_draw_block(unsigned key, unsigned k2, unsigned long long blk, unsigned& o0, unsigned& o1) {
    const unsigned c1 = (unsigned)(blk >> 32);
    const unsigned x = (unsigned)blk ^ key ^ c1 ^ __builtin_rotateleft32(c1, 11) ^ __builtin_rotateleft32(c1, 23);
    o0 = mix32(x, k2); o1 = mix32(x + 0x9E3779B9u, k2);
}
__device__ __forceinline__ int aug_range(unsigned k16, int R) { return (int)((k16 * (unsigned)R) >> 16); }
__device__ __forceinline__ int aug_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---- lips -------------------------------------------------------------------------------------------------------------------------
// One workgroup per output frame (b, t); a lane owns groups of four consecutive elements of the flattened H x W frame (they may straddle
// a row) and stores each group with one 16-byte store when VEC (H * W a multiple of 4, dst 16-byte aligned), element by element otherwise.
// The source pixels are read as single dwords: contiguous across lanes up to the shift, reversed under a flip.
template <bool VEC>
__global__ __launch_bounds__(256) void augment_lips_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                           const long long* __restrict__ lengths, int T, int H, int W,
                                                           unsigned long long seed, unsigned long long step, unsigned stream_id, int max_shift,
                                                           unsigned flip_thr, int mask_max, int mask_every) {
    const int b = blockIdx.x / T, t = blockIdx.x - b * T;
    const int HW = H * W;
    float* out = dst + (long long)blockIdx.x * HW;
    long long n64 = lengths ? lengths[b] : (long long)T;
    const int n = (int)(n64 < 0 ? 0 : (n64 > T ? T : n64));
    if (t >= n) {                                                          // padding: zeros, nothing is read
        if (VEC) {
            for (int q = threadIdx.x; q < HW / 4; q += 256) ((f32x4*)out)[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        } else {
            for (int i = threadIdx.x; i < HW; i += 256) out[i] = 0.f;
        }
        return;
    }
    // the plan of (b, t): uniform over the workgroup
    const unsigned long long c = step * 65536ull + (unsigned long long)b;
    unsigned o0, o1;
    drop_draw(seed, stream_id, 4ull * (c * 64ull), o0, o1);
    const int dx = aug_range(o0 & 0xFFFFu, 2 * max_shift + 1) - max_shift;
    const int dy = aug_range(o0 >> 16, 2 * max_shift + 1) - max_shift;
    const bool flip = (o1 & 0xFFFFu) < flip_thr;
    int ts = t;
    if (mask_max > 0) {
        const int j = t / mask_every;
        bool hit = false;
        // the own segment's span first, then the previous segment's (a span is at most mask_every long: no older one reaches t)
        for (int back = 0; back < 2 && !hit && j - back >= 0; ++back) {
            const int jj = j - back;
            drop_draw(seed, stream_id, 4ull * (c * 64ull + 1ull + (unsigned long long)(jj >> 1)), o0, o1);
            const unsigned w32 = (jj & 1) ? o1 : o0;
            const int start = jj * mask_every + aug_range(w32 & 0xFFFFu, mask_every);
            int end = start + aug_range(w32 >> 16, mask_max + 1);
            end = end > n ? n : end;
            if (t >= start && t < end) { ts = start > 0 ? start - 1 : 0; hit = true; }
        }
    }
    const float* in = src + ((long long)b * T + ts) * HW;
    const int Wm = W - 1, Hm = H - 1;
    for (int q = threadIdx.x; q < (HW + 3) / 4; q += 256) {
        const int i0 = 4 * q;
        int y = i0 / W, x = i0 - y * W;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (VEC || i0 + e < HW) {
                const int xs = aug_clamp((flip ? Wm - x : x) - dx, Wm);
                const int ys = aug_clamp(y - dy, Hm);
                v[e] = in[ys * W + xs];
            }
            if (++x == W) { x = 0; ++y; }
        }
        if (VEC) {
            ((f32x4*)out)[q] = f32x4{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < HW) out[i0 + e] = v[e];
        }
    }
}

// ---- noise ------------------------------------------------------------------------------------------------------------------------
constexpr int AUG_CHUNK = AV_AUG_NOISE_CHUNK;

__device__ __forceinline__ double aug_wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// pass 1a: partial[b][ch] = sum of x^2 over the valid samples of chunk ch of row b, in double (the square of an fp32 value is exact
// there), a fixed order of additions and no atomics: the same bits on every run
__global__ __launch_bounds__(256) void augment_power_kernel(const float* __restrict__ x, const long long* __restrict__ lengths, int N, int nch,
                                                            double* __restrict__ partial) {
    __shared__ double red[4];
    const int b = blockIdx.y, ch = blockIdx.x;
    long long n64 = lengths[b];
    const int n = (int)(n64 < 0 ? 0 : (n64 > N ? N : n64));
    const float* row = x + (long long)b * N;
    const int s0 = ch * AUG_CHUNK;
    int s1 = s0 + AUG_CHUNK;
    s1 = s1 > n ? n : s1;
    double a = 0.0;
    for (int i = s0 + (int)threadIdx.x; i < s1; i += 256) { const double v = row[i]; a = fma(v, v, a); }
    a = aug_wave_sum_f64(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) partial[(long long)b * nch + ch] = (red[0] + red[1]) + (red[2] + red[3]);
}

// pass 1b, one wave per row: P_b = sum of the chunk partials (fixed order) / valid samples; the SNR of (step, b) and the noise level
__global__ __launch_bounds__(64) void augment_sigma_kernel(const double* __restrict__ partial, const long long* __restrict__ lengths, int N, int nch,
                                                           unsigned long long seed, unsigned long long step, float snr_lo, float snr_hi,
                                                           double* __restrict__ power, float* __restrict__ sigma_out) {
    const int b = blockIdx.x;
    double a = 0.0;
    for (int i = threadIdx.x; i < nch; i += 64) a += partial[(long long)b * nch + i];
    a = aug_wave_sum_f64(a);
    if (threadIdx.x != 0) return;
    long long n64 = lengths[b];
    const int n = (int)(n64 < 0 ? 0 : (n64 > N ? N : n64));
    const double P = n > 0 ? a / (double)n : 0.0;
    unsigned o0, o1;
    drop_draw(seed, AV_AUG_STREAM_SNR, 4ull * (step * 65536ull + (unsigned long long)b), o0, o1);
    const float u = (float)(o0 & 0xFFFFu) * (1.0f / 65536.0f);
    const float span = snr_hi - snr_lo;
    const float snr = snr_lo + u * span;                                  // -ffp-contract=off: a rounded product, then a rounded sum
    power[b] = P;
    sigma_out[b] = P > 0.0 ? (float)sqrt(P * pow(10.0, -(double)snr / 10.0)) : (P == 0.0 ? 0.f : (float)P);   // a NaN power stays NaN
}

// pass 2: y = x + sigma_b z_i on the valid samples, y = x beyond; z_i = the centred sum of the four 16-bit integers of the sample's block,
// scaled to unit variance.  A lane owns four consecutive samples (one 16-byte load and store when VEC: N a multiple of 4, aligned rows).
template <bool VEC>
__global__ __launch_bounds__(256) void augment_noise_kernel(const float* __restrict__ x, float* __restrict__ y, const long long* __restrict__ lengths,
                                                            int N, unsigned long long seed, unsigned long long step,
                                                            const float* __restrict__ sigma) {
    const int b = blockIdx.y;
    const int i0 = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (i0 >= N) return;
    long long n64 = lengths[b];
    const int n = (int)(n64 < 0 ? 0 : (n64 > N ? N : n64));
    const float sg = sigma[b];
    const float inv_std = 0x1.bb67aep-16f;                                 // fp32(1 / sqrt((65536^2 - 1) / 3))
    const unsigned key = drop_key(seed, AV_AUG_STREAM_NOISE), k2 = drop_key2(key);
    const unsigned long long base = (step * 65536ull + (unsigned long long)b) << 24;
    const float* xr = x + (long long)b * N;
    float* yr = y + (long long)b * N;
    float v[4];
    if (VEC) {
        const f32x4 xv = *(const f32x4*)(xr + i0);
        v[0] = xv[0]; v[1] = xv[1]; v[2] = xv[2]; v[3] = xv[3];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = i0 + e < N ? xr[i0 + e] : 0.f;
    }
    if (sg != 0.f) {                                                      // sigma 0 (a silent or empty row): the row is copied, bit for bit
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (i0 + e < n) {
                unsigned o0, o1;
                aug_draw_block(key, k2, base + (unsigned long long)(i0 + e), o0, o1);
                const int s = (int)((o0 & 0xFFFFu) + (o0 >> 16) + (o1 & 0xFFFFu) + (o1 >> 16)) - 131070;
                const float z = (float)s * inv_std;
                const float nz = sg * z;
                v[e] = v[e] + nz;
            }
        }
    }
    if (VEC) {
        *(f32x4*)(yr + i0) = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i0 + e < N) yr[i0 + e] = v[e];
    }
}

}  // namespace

extern "C" int av_augment_lips(const float* src, float* dst, const long long* lengths, int B, int T, int H, int W, unsigned long long seed,
                               long long step, unsigned stream_id, int max_shift, int flip_thr, int mask_max, int mask_every, void* stream) {
    AV_CHECK(src && dst, "av_augment_lips: null pointer");
    AV_CHECK(B >= 0 && B <= 65536 && T >= 0 && H >= 1 && W >= 1 && (long long)H * W <= (1 << 24),
             "av_augment_lips: bad shape B=%d T=%d H=%d W=%d (B <= 65536, H * W <= 2^24)", B, T, H, W);
    AV_CHECK(step >= 0 && step < (1ll << 24), "av_augment_lips: step %lld outside [0, 2^24)", step);
    AV_CHECK(max_shift >= 0 && max_shift < (H < W ? H : W), "av_augment_lips: max_shift %d must be in [0, min(H, W) = %d)", max_shift,
             H < W ? H : W);
    AV_CHECK(flip_thr >= 0 && flip_thr <= 65536, "av_augment_lips: flip_thr %d outside [0, 65536]", flip_thr);
    AV_CHECK(mask_every >= 1 && mask_max >= 0 && mask_max <= mask_every, "av_augment_lips: need 0 <= mask_max <= mask_every, got %d and %d",
             mask_max, mask_every);
    AV_CHECK(av_cdiv(T, mask_every) <= 126, "av_augment_lips: T=%d frames in segments of %d are %d segments (limit 126)", T, mask_every,
             av_cdiv(T, mask_every));
    const long long frames = (long long)B * T, elems = frames * H * W;
    AV_CHECK(frames <= 0x7FFFFFFFll, "av_augment_lips: B * T = %lld frames exceed the grid limit", frames);
    // out of place only: a shifted or frozen read would see pixels this launch has already overwritten
    AV_CHECK(src == dst ? false : (src + elems <= dst || dst + elems <= src), "av_augment_lips: src == dst or the two clips overlap (out of place only)");
    if (frames == 0) return AV_OK;
    const bool vec = ((long long)H * W) % 4 == 0 && (uintptr_t)dst % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(augment_lips_kernel<true>, dim3((unsigned)frames), dim3(256), 0, (hipStream_t)stream, src, dst, lengths, T, H, W, seed,
                           (unsigned long long)step, stream_id, max_shift, (unsigned)flip_thr, mask_max, mask_every);
    else
        hipLaunchKernelGGL(augment_lips_kernel<false>, dim3((unsigned)frames), dim3(256), 0, (hipStream_t)stream, src, dst, lengths, T, H, W, seed,
                           (unsigned long long)step, stream_id, max_shift, (unsigned)flip_thr, mask_max, mask_every);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_augment_noise(const float* x, float* y, const long long* lengths, int B, int N, unsigned long long seed, long long step,
                                float snr_lo, float snr_hi, double* power_ws, float* sigma_out, void* stream) {
    AV_CHECK(x && y && lengths && power_ws && sigma_out, "av_augment_noise: null pointer");
    AV_CHECK(B >= 0 && B <= 65535 && N >= 0 && N <= (1 << 24), "av_augment_noise: bad shape B=%d N=%d (B <= 65535, N <= 2^24)", B, N);
    AV_CHECK(step >= 0 && step < (1ll << 24), "av_augment_noise: step %lld outside [0, 2^24)", step);
    AV_CHECK(snr_lo <= snr_hi && snr_hi - snr_lo < INFINITY, "av_augment_noise: need finite snr_lo <= snr_hi, got %g and %g", (double)snr_lo,
             (double)snr_hi);
    AV_CHECK((uintptr_t)power_ws % 8 == 0, "av_augment_noise: power_ws must be 8-byte aligned");
    const long long elems = (long long)B * N;
    AV_CHECK(x == y || x + elems <= y || y + elems <= x, "av_augment_noise: x and y overlap without being the same tensor");
    if (B == 0) return AV_OK;
    const int nch = N > 0 ? av_cdiv(N, AUG_CHUNK) : 1;
    double* partial = power_ws + B;
    if (N > 0)
        hipLaunchKernelGGL(augment_power_kernel, dim3(nch, B), dim3(256), 0, (hipStream_t)stream, x, lengths, N, nch, partial);
    else
        hipMemsetAsync(partial, 0, sizeof(double) * B, (hipStream_t)stream);
    hipLaunchKernelGGL(augment_sigma_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const double*)partial, lengths, N, nch, seed,
                       (unsigned long long)step, snr_lo, snr_hi, power_ws, sigma_out);
    if (N > 0) {
        const bool vec = N % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)y % 16 == 0;
        const dim3 grid(av_cdiv(av_cdiv(N, 4), 256), B);
        if (vec)
            hipLaunchKernelGGL(augment_noise_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, y, lengths, N, seed,
                               (unsigned long long)step, (const float*)sigma_out);
        else
            hipLaunchKernelGGL(augment_noise_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, y, lengths, N, seed,
                               (unsigned long long)step, (const float*)sigma_out);
    }
    AV_LAUNCH_CHECK();
    return AV_OK;
}
