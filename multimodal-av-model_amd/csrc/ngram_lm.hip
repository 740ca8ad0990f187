// Batched n-gram scoring on the device (lm.py: NGramLM.score_batch): one thread per token, the law and the tables of ngram_lm.h.
// float32 in both libraries.
#include "ngram_lm.h"

namespace {

__global__ __launch_bounds__(256) void ngram_score_kernel(const int* __restrict__ ids, const long long* __restrict__ lens,
                                                          float* __restrict__ out, int B, int Lmax, LmTables lm, int bos) {
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x >= (long long)B * Lmax) return;
    const int b = (int)(x / Lmax), i = (int)(x - (long long)b * Lmax);
    const int len = ctc_clamp_len(lens, b, Lmax);
    if (i >= len) { out[x] = 0.f; return; }
    const int* row = ids + (long long)b * Lmax;
    const int have = min(i, lm.order - 1);
    unsigned long long ctx = (have < lm.order - 1 && bos >= 0) ? (unsigned long long)(bos + 1) : 0ull;
    for (int j = i - have; j < i; ++j) {
        const int w = row[j];
        ctx = (ctx << 16) | (w >= 0 && w < lm.V ? (unsigned long long)(w + 1) : 0xffffull);       // 0xffff is no token's field: it matches nothing
    }
    ctx &= lm.cmask;
    const int c = row[i];
    out[x] = c >= 0 && c < lm.V ? lm_score(lm, ctx, c) : __uint_as_float(0x7fc00000u);
}

}  // namespace

extern "C" int av_ngram_score(const int* ids, const long long* lens, float* out, int B, int Lmax, const float* lm_unigrams, const void* lm_table,
                              long long lm_slots, int lm_order, int lm_vocab, int lm_bos, int lm_probe_bound, void* stream) {
    AV_CHECK(ids && out, "av_ngram_score: null pointer");
    AV_CHECK(B >= 0 && Lmax >= 1 && (long long)B * Lmax <= (1ll << 31) * 255, "av_ngram_score: bad shape B=%d Lmax=%d", B, Lmax);
    LmTables lm;
    const int rc = lm_check("av_ngram_score", lm_unigrams, lm_table, lm_slots, lm_order, lm_vocab, lm_bos, lm_probe_bound, &lm);
    if (rc != AV_OK) return rc;
    if (B == 0) return AV_OK;
    hipLaunchKernelGGL(ngram_score_kernel, dim3(av_cdiv((long long)B * Lmax, 256)), dim3(256), 0, (hipStream_t)stream, ids, lens, out, B, Lmax,
                       lm, lm_bos);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
