// Small kernels of the loss side (the optimizer is optim.hip):
//   * row L2-normalise fwd/bwd (F.normalize, contrastive.py:22),
//   * row log-sum-exp + row sum of the similarity matrix and the softmax-minus-uniform gradient of
//     -log_softmax(sim).mean() (contrastive.py:33-34,41-42),
//   * scalar reductions and the combination of the loss terms.
#include "av_common.h"

namespace {

constexpr int MAXIT = 32;

__global__ __launch_bounds__(256) void l2norm_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ nrm,
                                                         long long rows, int cols, float eps) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long long base = row * cols;
    float q = 0.f;
    for (int c = lane; c < cols; c += 64) { const float v = x[base + c]; q += v * v; }
    const float n = sqrtf(wave_sum(q));
    const float inv = 1.f / fmaxf(n, eps);
    for (int c = lane; c < cols; c += 64) y[base + c] = x[base + c] * inv;
    if (lane == 0) nrm[row] = n;
}
// dx = (dy - y (y . dy)) / max(n, eps)
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy, const float* __restrict__ nrm,
                                                         float* __restrict__ dx, long long rows, int cols, float eps) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const long long base = row * cols;
    float d = 0.f;
    for (int c = lane; c < cols; c += 64) d += y[base + c] * dy[base + c];
    d = wave_sum(d);
    const float inv = 1.f / fmaxf(nrm[row], eps);
    for (int c = lane; c < cols; c += 64) dx[base + c] = (dy[base + c] - y[base + c] * d) * inv;
}

__global__ __launch_bounds__(256) void lse_rows_kernel(const float* __restrict__ s, float* __restrict__ lse, float* __restrict__ rsum,
                                                       long long rows, int cols, int ld, int accumulate) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* p = s + row * ld;
    float mx = -INFINITY, sm = 0.f;
    for (int c = lane; c < cols; c += 64) { const float v = p[c]; mx = fmaxf(mx, v); sm += v; }
    mx = wave_max(mx);
    float e = 0.f;
    for (int c = lane; c < cols; c += 64) e += expf(p[c] - mx);
    e = wave_sum(e);
    sm = wave_sum(sm);
    if (lane == 0) {
        float l = mx + logf(e);
        if (accumulate) {                                        // merge with the row's running values (earlier column chunks)
            const float lo = lse[row], hi = fmaxf(lo, l);
            l = hi + logf(expf(lo - hi) + expf(l - hi));
            sm += rsum[row];
        }
        lse[row] = l; rsum[row] = sm;
    }
}

// dsim = coef * (exp(sim - lse_row) - 1/cols)
__global__ __launch_bounds__(256) void contrastive_dsim_kernel(const float* __restrict__ s, const float* __restrict__ lse, void* __restrict__ out,
                                                               int odt, long long rows, int cols, int ld, float coef, float u) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float l = lse[row];
    for (int c = lane; c < ld; c += 64) st_any(out, row * ld + c, odt, c < cols ? coef * (expf(s[row * ld + c] - l) - u) : 0.f);
}

__global__ __launch_bounds__(256) void reduce_sum_kernel(const float* __restrict__ x, long long n, float* __restrict__ out, float scale, int accumulate) {
    __shared__ float red[4];
    float s = 0.f;
    for (long long i = threadIdx.x; i < n; i += 256) s += x[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float v = scale * (red[0] + red[1] + red[2] + red[3]);
        out[0] = accumulate ? out[0] + v : v;
    }
}

// total = sum_i nll[i] * w[i] + half_lambda * (c1 + c2);  l1 / l2 = 2 x the two halves of the weighted sum (the per-speaker CTC means of
// model/trainer.py:111-118 with w[i] = 1 / (2 B clamp(target_len_i, 1))); one launch instead of a dozen scalar torch ops
__global__ __launch_bounds__(256) void loss_combine_kernel(const float* __restrict__ nll, const float* __restrict__ w, const float* __restrict__ c1,
                                                           const float* __restrict__ c2, float half_lambda, int n, float* __restrict__ out) {
    __shared__ float red[2][4];
    const int hn = n / 2;
    float s0 = 0.f, s1 = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float v = nll[i] * w[i];
        if (i < hn) s0 += v; else s1 += v;
    }
    s0 = wave_sum(s0); s1 = wave_sum(s1);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s0; red[1][threadIdx.x >> 6] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float a = red[0][0] + red[0][1] + red[0][2] + red[0][3], b = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        out[0] = a + b + half_lambda * ((c1 ? c1[0] : 0.f) + (c2 ? c2[0] : 0.f));
        out[1] = 2.f * a;
        out[2] = 2.f * b;
    }
}

}  // namespace

extern "C" int av_l2norm_fwd(const float* x, float* y, float* nrm, long long rows, int cols, float eps, void* stream) {
    AV_CHECK(x && y && nrm && cols > 0, "av_l2norm_fwd: bad args");
    if (rows == 0) return AV_OK;
    hipLaunchKernelGGL(l2norm_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, y, nrm, rows, cols, eps);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
extern "C" int av_l2norm_bwd(const float* y, const float* dy, const float* nrm, float* dx, long long rows, int cols, float eps, void* stream) {
    AV_CHECK(y && dy && nrm && dx && cols > 0, "av_l2norm_bwd: bad args");
    if (rows == 0) return AV_OK;
    hipLaunchKernelGGL(l2norm_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, y, dy, nrm, dx, rows, cols, eps);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
extern "C" int av_lse_rows(const float* s, float* lse, float* rowsum, long long rows, int cols, int ld, void* stream) {
    AV_CHECK(s && lse && rowsum && cols > 0 && ld >= cols, "av_lse_rows: bad args");
    if (rows == 0) return AV_OK;
    hipLaunchKernelGGL(lse_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, s, lse, rowsum, rows, cols, ld, 0);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
extern "C" int av_lse_rows_chunk(const float* s, float* lse, float* rowsum, long long rows, int cols, int ld, int accumulate, void* stream) {
    AV_CHECK(s && lse && rowsum && cols > 0 && ld >= cols, "av_lse_rows_chunk: bad args");
    if (rows == 0) return AV_OK;
    hipLaunchKernelGGL(lse_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, s, lse, rowsum, rows, cols, ld, accumulate);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
extern "C" int av_contrastive_dsim(const float* s, const float* lse, void* out, int odt, long long rows, int cols, int ld, float coef, void* stream) {
    AV_CHECK(s && lse && out && cols > 0 && ld >= cols, "av_contrastive_dsim: bad args");
    if (rows == 0) return AV_OK;
    hipLaunchKernelGGL(contrastive_dsim_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, s, lse, out, odt, rows, cols, ld, coef,
                       1.f / (float)cols);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
extern "C" int av_contrastive_dsim_chunk(const float* s, const float* lse, void* out, int odt, long long rows, int cols, int ld, float coef,
                                         int total_cols, void* stream) {
    AV_CHECK(s && lse && out && cols > 0 && ld >= cols && total_cols >= cols, "av_contrastive_dsim_chunk: bad args");
    if (rows == 0) return AV_OK;
    hipLaunchKernelGGL(contrastive_dsim_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, s, lse, out, odt, rows, cols, ld, coef,
                       1.f / (float)total_cols);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
extern "C" int av_loss_combine(const float* nll, const float* w, const float* c1, const float* c2, float half_lambda, int n, float* out3,
                               void* stream) {
    AV_CHECK(nll && w && out3 && n >= 2 && n % 2 == 0, "av_loss_combine: bad args (n=%d)", n);
    hipLaunchKernelGGL(loss_combine_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, nll, w, c1, c2, half_lambda, n, out3);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
extern "C" int av_reduce_sum(const float* x, long long n, float* out, float scale, int accumulate, void* stream) {
    AV_CHECK(x && out, "av_reduce_sum: bad args");
    hipLaunchKernelGGL(reduce_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, x, n, out, scale, accumulate);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
