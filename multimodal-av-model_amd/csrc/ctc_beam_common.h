// The small parts of the CTC prefix beam search (ctc_beam.hip) that are not the search itself: the limits, the workspace layout, the
// log-sum, the order-preserving key of a score, the 64-bit mixer (also the n-gram table's hash, ngram_lm.h), the content
// hash of a prefix, the workgroup scan and the radix select.
#pragma once
#include "ctc_common.h"

namespace {

constexpr int MAXT = 4096;
constexpr int MAXW = 64;
constexpr int MAXK = MAXW + 1;
constexpr int MAXCAND = MAXW * (MAXK + 1);          // W (W + 2)

struct BeamWorkspace {
    long long topv, topt, apar, atok, total;        // byte offsets: top values fp32 [B][T][wf+1], top tokens int32 [B][T][wf+1], arena int32 [B][T][W] x 2
};

// wf is the width of the frame pass that fills the top lists: W without a language model, max(tokens - 1, 1) with one.  The arena is sized
// for the larger of W and wf, so that the frame pass at width wf accepts the same workspace.
static BeamWorkspace beam_workspace(long long B, long long T, long long W, long long wf) {
    BeamWorkspace w;
    const long long top = B * T * (wf + 1) * 4, arena = B * T * W * 4;
    w.topv = 0; w.topt = top; w.apar = 2 * top; w.atok = 2 * top + arena; w.total = 2 * top + 2 * B * T * (W > wf ? W : wf) * 4;
    return w;
}

__device__ __forceinline__ float logaddexp_f(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == -INFINITY) return -INFINITY;           // (-inf) (+) (-inf): never NaN
    return m + log1pf(expf(-fabsf(a - b)));
}

// order-preserving image of a float in the unsigned integers; 0 is below every float (-inf maps to 0x007fffff) and marks "no candidate"
__device__ __forceinline__ unsigned key_of(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// splitmix64: the finaliser, a bijection of the 64-bit integers, and the increment its generator adds before it
constexpr unsigned long long MIX64_STEP = 0x9E3779B97F4A7C15ull;
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ unsigned long long hash_push(unsigned long long h, int c) { return mix64(h + MIX64_STEP * (unsigned long long)(c + 1)); }

// inclusive prefix sum of one int per thread over the 256 threads of the workgroup (wsum: 4 ints of LDS); ends with the data visible
__device__ __forceinline__ int block_scan_incl(int v, int* wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_up(v, s, 64);
        if (lane >= s) v += o;
    }
    __syncthreads();                                // the previous use of wsum is over
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    for (int i = 0; i < w; ++i) v += wsum[i];
    return v;
}

// Step 4 of the search.  The want = min(W, N) largest of keys[0 .. N): the want-th largest key by a 4 x 8-bit radix select (LDS histogram
// and one workgroup scan per pass), then every key above it and the first equal ones in candidate order into sel[] / selkey[] (in no order
// among themselves); called by all 256 threads, ends with the selection visible.  hist: 256 ints, wsum: 4, pick: 2, sel / selkey: MAXW.
__device__ __forceinline__ int beam_select(const unsigned* keys, int N, int W, int* hist, int* wsum, int* pick, int* sel, unsigned* selkey) {
    const int tid = threadIdx.x;
    // the want-th largest key: radix select, 8 bits a pass
    const int want = min(W, N);
    unsigned prefix = 0, mask = 0;
    int remaining = want;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();                         // also orders the write of step 3's tail before the first read of keys
        for (int q = tid; q < N; q += 256) {
            const unsigned k = keys[q];
            if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1);
        }
        __syncthreads();
        const int h = hist[255 - tid];
        const int incl = block_scan_incl(h, wsum);         // entries in digits >= 255 - tid
        if (incl - h < remaining && remaining <= incl) { pick[0] = 255 - tid; pick[1] = remaining - (incl - h); }
        __syncthreads();
        prefix |= (unsigned)pick[0] << shift; mask |= 255u << shift;
        remaining = pick[1];
    }
    // prefix = the want-th largest key; take every key above it and the first `remaining` equal to it, in candidate order
    const int per = (N + 255) / 256, q0 = tid * per, q1 = min(N, q0 + per);
    int gt = 0, eq = 0;
    for (int q = q0; q < q1; ++q) { const unsigned k = keys[q]; gt += k > prefix; eq += k == prefix; }
    const int packed = block_scan_incl(gt | (eq << 16), wsum);
    if (tid == 255) pick[0] = packed & 0xffff;   // all keys above the threshold
    __syncthreads();
    {
        const int ngt = pick[0];
        int og = (packed & 0xffff) - gt, oe = (packed >> 16) - eq;
        for (int q = q0; q < q1; ++q) {
            const unsigned k = keys[q];
            if (k > prefix) { sel[og] = q; selkey[og] = k; ++og; }
            else if (k == prefix) { if (oe < remaining) { sel[ngt + oe] = q; selkey[ngt + oe] = k; } ++oe; }
        }
    }
    __syncthreads();
    return want;
}

}  // namespace
