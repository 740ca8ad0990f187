// Phrase counts of given token sequences on the device (bias.py: ContextBias.count_batch): one thread per sequence, the law and the
// tables of context_bias.h.  Integers only; the same in both libraries.
#include "context_bias.h"

namespace {

__global__ __launch_bounds__(256) void context_bias_count_kernel(const int* __restrict__ ids, const long long* __restrict__ lens,
                                                                 int* __restrict__ out, int B, int Lmax, BiasTables t, int V, int blank) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int len = ctc_clamp_len(lens, b, Lmax);
    const int* row = ids + (long long)b * Lmax;
    int2* o = (int2*)out + (long long)b * Lmax;
    int node = 0, k = 0;
    for (int i = 0; i < len; ++i) {
        const int c = row[i];
        if (c >= 0 && c < V && c != blank) bias_step(t, node, k, c);
        else node = 0;                              // no phrase holds such an id: it matches nothing and ends a running match
        o[i] = make_int2(k, bias_depth(t, node));
    }
    for (int i = len; i < Lmax; ++i) o[i] = make_int2(0, 0);
}

}  // namespace

extern "C" int av_context_bias_count(const int* ids, const long long* lens, int* out, int B, int Lmax, int V, int blank,
                                     const void* bias_nodes, const void* bias_edges, int bias_node_count, long long bias_slots,
                                     int bias_probe_bound, void* stream) {
    const char* who = "av_context_bias_count";
    AV_CHECK(ids && out, "%s: null pointer", who);
    AV_CHECK(B >= 0 && Lmax >= 1, "%s: bad shape B=%d Lmax=%d", who, B, Lmax);
    AV_CHECK(((uintptr_t)out & 7) == 0, "%s: out is not 8-byte aligned", who);
    BiasTables t;
    const int rc = bias_check(who, bias_nodes, bias_edges, bias_node_count, bias_slots, bias_probe_bound, V, &t);
    if (rc != AV_OK) return rc;
    AV_CHECK(blank >= 0 && blank < V, "%s: blank %d outside [0, %d)", who, blank, V);
    if (B == 0) return AV_OK;
    hipLaunchKernelGGL(context_bias_count_kernel, dim3(av_cdiv(B, 256)), dim3(256), 0, (hipStream_t)stream, ids, lens, out, B, Lmax, t, V, blank);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
