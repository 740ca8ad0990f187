// Long-form transcription on the device: the log-probs of overlapping windows are stitched into one sequence, the sequence is cut at blank
// frames, and the pieces are gathered into one padded batch that the CTC decoders of this library take as it is.  fp32 throughout (the same
// code in both libraries), no atomics, every output element written by exactly one thread, cuts and lengths read from and written to
// DEVICE memory: nothing travels to the host and nothing synchronises.  longform.py restates the three laws in float32 numpy.
//
// Stitch law for output row [s][t] with its sources k = 0 .. n-1 (n = 1 .. 4 window rows, ascending window index, and their normalised
// float32 weights wn_k; both from a table the host builds from the window plan):
//   centre    the owner's row, copied bit for bit (the table holds one source per frame)
//   average   n == 1: that row, copied bit for bit.  Otherwise per class  M = max_k x_k,  out = M + log(sum_k wn_k exp(x_k - M)), the sum
//             in source order; M = -inf gives -inf, a NaN source gives NaN
// Classes are independent, so a row needs no reduction: a wavefront walks the row in chunks of 64 x 4 classes, reads the chunk of every source
// before it computes (up to four 16-byte loads in flight per lane) and every source row exactly once.
//   ctc_stitch_kernel          four output rows (wavefronts) per workgroup
//   ctc_cut_points_kernel      one wavefront per (speaker, boundary): strided reads of the blank column, argmax with ties to the first frame
//   ctc_segment_gather_kernel  four output rows per workgroup: the source row's copy or the zero fill; the first row of a segment also
//                              writes the segment's length
// Out-of-range data cannot cause out-of-bounds accesses: a table index outside [0, R) counts as no source, cuts are clamped to [0, F] and a
// segment's length to [0, segment].
#include "ctc_common.h"

namespace {

constexpr int LF_ROWS = 4;                         // rows (wavefronts) per workgroup
constexpr int LF_SRC = AV_LONGFORM_MAX_SOURCES;    // sources per stitched frame

// a NaN in either argument wins
__device__ __forceinline__ float lf_max_nan(float m, float x) { return (x > m || x != x) ? x : m; }

__device__ __forceinline__ float lf_average(const float (&x)[LF_SRC], const float (&wn)[LF_SRC], int n) {
    float M = x[0];
#pragma unroll
    for (int k = 1; k < LF_SRC; ++k) if (k < n) M = lf_max_nan(M, x[k]);
    if (M == -INFINITY) return -INFINITY;
    float acc = wn[0] * expf(x[0] - M);
#pragma unroll
    for (int k = 1; k < LF_SRC; ++k) if (k < n) acc += wn[k] * expf(x[k] - M);
    return M + logf(acc);
}

// VEC: every row base is 16-byte aligned and V % 4 == 0
template <bool VEC>
__global__ __launch_bounds__(64 * LF_ROWS) void ctc_stitch_kernel(const float* __restrict__ win, long long stride_s, long long stride_r,
                                                                  const int* __restrict__ src_row, const float* __restrict__ src_w,
                                                                  int S, int R, int F, int V, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * LF_ROWS + w;
    if (i >= (long long)S * F) return;
    const int s = (int)(i / F), t = (int)(i % F);
    const float* row[LF_SRC];
    float wn[LF_SRC];
    int n = 0;
#pragma unroll
    for (int k = 0; k < LF_SRC; ++k) {             // the table is the same for every lane: sources are packed in front
        const int r = src_row[(long long)t * LF_SRC + k];
        const bool ok = r >= 0 && r < R && n == k;
        row[k] = win + (long long)s * stride_s + (long long)(ok ? r : 0) * stride_r;
        wn[k] = ok ? src_w[(long long)t * LF_SRC + k] : 0.f;
        if (ok) ++n;
    }
    float* o = out + i * (long long)V;
    if (n == 0) {                                  // no window covers the frame (a table that does not come from a plan): a defined value
        for (int c = lane; c < V; c += AV_WAVE) o[c] = -INFINITY;
        return;
    }
    if (VEC) {
        const int nv = V >> 2;
        for (int c = lane; c < nv; c += AV_WAVE) {
            f32x4 x[LF_SRC];
#pragma unroll
            for (int k = 0; k < LF_SRC; ++k) if (k < n) x[k] = ((const f32x4*)row[k])[c];
            f32x4 y = x[0];
            if (n > 1) {
                float e[LF_SRC];
#pragma unroll
                for (int k = 0; k < LF_SRC; ++k) e[k] = k < n ? x[k].x : 0.f;
                y.x = lf_average(e, wn, n);
#pragma unroll
                for (int k = 0; k < LF_SRC; ++k) e[k] = k < n ? x[k].y : 0.f;
                y.y = lf_average(e, wn, n);
#pragma unroll
                for (int k = 0; k < LF_SRC; ++k) e[k] = k < n ? x[k].z : 0.f;
                y.z = lf_average(e, wn, n);
#pragma unroll
                for (int k = 0; k < LF_SRC; ++k) e[k] = k < n ? x[k].w : 0.f;
                y.w = lf_average(e, wn, n);
            }
            ((f32x4*)o)[c] = y;
        }
    } else {
        for (int c = lane; c < V; c += AV_WAVE) {
            float x[LF_SRC];
#pragma unroll
            for (int k = 0; k < LF_SRC; ++k) x[k] = k < n ? row[k][c] : 0.f;
            o[c] = n > 1 ? lf_average(x, wn, n) : x[0];
        }
    }
}

__global__ __launch_bounds__(64 * LF_ROWS) void ctc_cut_points_kernel(const float* __restrict__ lp, long long stride_s, long long stride_t,
                                                                      int S, int F, int V, int blank, int N, int radius, int nb,
                                                                      int* __restrict__ cuts) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * LF_ROWS + w;
    if (i >= (long long)S * (nb + 2)) return;
    const int s = (int)(i / (nb + 2)), j = (int)(i % (nb + 2));
    if (j == 0 || j == nb + 1) {
        if (lane == 0) cuts[i] = j == 0 ? 0 : F;
        return;
    }
    const long long mid = (long long)j * N;        // j <= nb, so mid + radius < F: no overflow past F
    const int lo = (int)max(mid - radius, 1LL), hi = (int)min(mid + radius, (long long)F - 1);
    const float* col = lp + (long long)s * stride_s + blank;
    float best = -INFINITY;
    int bt = 0x7fffffff;
    for (int t = lo + lane; t <= hi; t += AV_WAVE) {
        float x = col[(long long)t * stride_t];
        if (x != x) x = -INFINITY;                 // a NaN ranks as -inf
        if (x > best || (x == best && t < bt)) { best = x; bt = t; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int ot = __shfl_xor(bt, o, 64);
        if (ob > best || (ob == best && ot < bt)) { best = ob; bt = ot; }
    }
    if (lane == 0) cuts[i] = bt == 0x7fffffff ? lo : bt;
}

template <bool VEC>
__global__ __launch_bounds__(64 * LF_ROWS) void ctc_segment_gather_kernel(const float* __restrict__ lp, long long stride_s, long long stride_t,
                                                                          const int* __restrict__ cuts, int S, int F, int V, int nb, int segment,
                                                                          float* __restrict__ seg_lp, long long* __restrict__ seg_len) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * LF_ROWS + w;
    const long long nseg = (long long)S * (nb + 1);
    if (i >= nseg * segment) return;
    const long long q = i / segment;               // segment index s * (nb + 1) + j
    const int r = (int)(i % segment);
    const int s = (int)(q / (nb + 1)), j = (int)(q % (nb + 1));
    const int c0 = min(max(cuts[(long long)s * (nb + 2) + j], 0), F);
    const int c1 = min(max(cuts[(long long)s * (nb + 2) + j + 1], c0), F);
    const int len = min(c1 - c0, segment);
    if (r == 0 && lane == 0) seg_len[q] = len;
    float* o = seg_lp + i * (long long)V;
    if (r < len) {
        const float* src = lp + (long long)s * stride_s + (long long)(c0 + r) * stride_t;
        if (VEC) {
            for (int c = lane; c < (V >> 2); c += AV_WAVE) ((f32x4*)o)[c] = ((const f32x4*)src)[c];
        } else {
            for (int c = lane; c < V; c += AV_WAVE) o[c] = src[c];
        }
    } else if (VEC) {
        for (int c = lane; c < (V >> 2); c += AV_WAVE) ((f32x4*)o)[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    } else {
        for (int c = lane; c < V; c += AV_WAVE) o[c] = 0.f;
    }
}

long long lf_grid(long long rows) { return (rows + LF_ROWS - 1) / LF_ROWS; }

}  // namespace

extern "C" int av_ctc_stitch(const float* windows, long long stride_s, long long stride_r, const int* src_row, const float* src_weight, int S,
                             int R, int F, int V, float* out, void* stream) {
    AV_CHECK(S >= 0 && R >= 1 && F >= 1 && V >= 2, "av_ctc_stitch: bad shape S=%d R=%d F=%d V=%d (S >= 0, R >= 1, F >= 1, V >= 2)", S, R, F, V);
    if (S == 0) return AV_OK;
    AV_CHECK(windows && src_row && src_weight && out, "av_ctc_stitch: null pointer");
    if (S == 1) stride_s = 0;                      // never multiplied by anything but 0
    if (int rc = ctc_check_rows("av_ctc_stitch", stride_s, stride_r, S, R, V, false, "srSR")) return rc;
    const long long grid = lf_grid((long long)S * F);
    AV_CHECK(grid <= 0x7fffffffLL, "av_ctc_stitch: S * F = %lld rows exceed one launch", (long long)S * F);
    if (ctc_vec_ok(windows, out, stride_s, stride_r, V))
        hipLaunchKernelGGL(ctc_stitch_kernel<true>, dim3((unsigned)grid), dim3(64 * LF_ROWS), 0, (hipStream_t)stream, windows, stride_s, stride_r,
                           src_row, src_weight, S, R, F, V, out);
    else
        hipLaunchKernelGGL(ctc_stitch_kernel<false>, dim3((unsigned)grid), dim3(64 * LF_ROWS), 0, (hipStream_t)stream, windows, stride_s, stride_r,
                           src_row, src_weight, S, R, F, V, out);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_ctc_cut_points(const float* log_probs, long long stride_s, long long stride_t, int S, int F, int V, int blank, int segment,
                                 int radius, int* cuts, void* stream) {
    AV_CHECK(S >= 0 && F >= 1 && V >= 2, "av_ctc_cut_points: bad shape S=%d F=%d V=%d (S >= 0, F >= 1, V >= 2)", S, F, V);
    if (int rc = ctc_check_blank("av_ctc_cut_points", blank, V)) return rc;
    AV_CHECK(radius >= 0 && segment >= 1 && segment <= AV_LONGFORM_MAX_SEGMENT && (long long)segment - 2LL * radius >= 2LL * radius + 1,
             "av_ctc_cut_points: need radius >= 0, segment <= %d and segment - 2 radius >= 2 radius + 1, got segment=%d radius=%d",
             AV_LONGFORM_MAX_SEGMENT, segment, radius);
    if (S == 0) return AV_OK;
    AV_CHECK(log_probs && cuts, "av_ctc_cut_points: null pointer");
    if (S == 1) stride_s = 0;
    if (int rc = ctc_check_rows("av_ctc_cut_points", stride_s, stride_t, S, F, V, false, "stSF")) return rc;
    const int N = segment - 2 * radius;
    const int nb = F - 1 - radius >= 0 ? (F - 1 - radius) / N : 0;
    const long long grid = lf_grid((long long)S * (nb + 2));
    AV_CHECK(grid <= 0x7fffffffLL, "av_ctc_cut_points: too many boundaries for one launch");
    hipLaunchKernelGGL(ctc_cut_points_kernel, dim3((unsigned)grid), dim3(64 * LF_ROWS), 0, (hipStream_t)stream, log_probs, stride_s, stride_t, S,
                       F, V, blank, N, radius, nb, cuts);
    AV_LAUNCH_CHECK();
    return AV_OK;
}

extern "C" int av_ctc_segment_gather(const float* log_probs, long long stride_s, long long stride_t, const int* cuts, int S, int F, int V,
                                     int nb, int segment, float* seg_log_probs, long long* seg_lengths, void* stream) {
    AV_CHECK(S >= 0 && F >= 1 && V >= 2 && nb >= 0 && nb < F, "av_ctc_segment_gather: bad shape S=%d F=%d V=%d nb=%d (S >= 0, F >= 1, V >= 2, "
             "0 <= nb < F)", S, F, V, nb);
    AV_CHECK(segment >= 1 && segment <= AV_LONGFORM_MAX_SEGMENT, "av_ctc_segment_gather: segment %d outside [1, %d]", segment,
             AV_LONGFORM_MAX_SEGMENT);
    if (S == 0) return AV_OK;
    AV_CHECK(log_probs && cuts && seg_log_probs && seg_lengths, "av_ctc_segment_gather: null pointer");
    if (S == 1) stride_s = 0;
    if (int rc = ctc_check_rows("av_ctc_segment_gather", stride_s, stride_t, S, F, V, false, "stSF")) return rc;
    const long long grid = lf_grid((long long)S * (nb + 1) * segment);
    AV_CHECK(grid <= 0x7fffffffLL, "av_ctc_segment_gather: S * (nb + 1) * segment = %lld rows exceed one launch",
             (long long)S * (nb + 1) * segment);
    if (ctc_vec_ok(log_probs, seg_log_probs, stride_s, stride_t, V))
        hipLaunchKernelGGL(ctc_segment_gather_kernel<true>, dim3((unsigned)grid), dim3(64 * LF_ROWS), 0, (hipStream_t)stream, log_probs, stride_s,
                           stride_t, cuts, S, F, V, nb, segment, seg_log_probs, seg_lengths);
    else
        hipLaunchKernelGGL(ctc_segment_gather_kernel<false>, dim3((unsigned)grid), dim3(64 * LF_ROWS), 0, (hipStream_t)stream, log_probs, stride_s,
                           stride_t, cuts, S, F, V, nb, segment, seg_log_probs, seg_lengths);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
