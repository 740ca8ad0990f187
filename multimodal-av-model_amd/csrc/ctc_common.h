// The small laws every CTC source shares (loss, alignment, confidences, long-form, beam search, error counts): on the device the length
// clamp; on the host the LDS limit, the row law of a strided block of log-probs, the 16-byte predicate and the scalar argument checks.
#pragma once
#include "av_common.h"

namespace {

constexpr long long CTC_LDS_LIMIT = 64 * 1024;

// a length clamped to [0, hi]
__device__ __forceinline__ int ctc_clamp_len(long long v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }
// frames (or tokens) of item b that are consumed: lengths[b] clamped to [0, hi], hi without lengths
__device__ __forceinline__ int ctc_clamp_len(const long long* lengths, int b, int hi) {
    return lengths ? ctc_clamp_len(lengths[b], hi) : hi;
}

// n >= 1 rows of V >= 1 contiguous floats, stride_row apart, lie inside one step of stride_outer without overlap - as a quotient, which no
// stride can overflow (a negative stride fails it)
inline bool ctc_rows_fit(long long stride_outer, long long stride_row, long long n, int V) {
    return stride_row >= V && stride_outer / n >= stride_row;
}

// The row law of a block [n_outer][n_rows][V] behind (stride_outer, stride_row).  either_order: the block may also be laid out rows first
// ([T][B][V] seen as [B][T][V]).  One order only: a block of one outer item never steps by stride_outer, which is then free.  names: the
// letters of the two strides and of the two dimensions in the message ("btBT").
inline int ctc_check_rows(const char* who, long long stride_outer, long long stride_row, int n_outer, int n_rows, int V, bool either_order,
                          const char* names) {
    const bool ok = either_order ? ctc_rows_fit(stride_outer, stride_row, n_rows, V) || ctc_rows_fit(stride_row, stride_outer, n_outer > 0 ? n_outer : 1, V)
                                 : (n_outer == 1 ? stride_row >= V : ctc_rows_fit(stride_outer, stride_row, n_rows, V));
    AV_CHECK(ok, "%s: strides (%c %lld, %c %lld) do not cover [%c=%d][%c=%d][V=%d] rows", who, names[0], stride_outer, names[1], stride_row,
             names[2], n_outer, names[3], n_rows, V);
    return AV_OK;
}

// 16-byte loads / stores: every row of the block behind `in` starts on a 16-byte boundary, and so do the dense rows of V floats behind
// `out` (null: no such block) and in LDS
inline bool ctc_vec_ok(const void* in, const void* out, long long stride_outer, long long stride_row, int V) {
    return (uintptr_t)in % 16 == 0 && (uintptr_t)out % 16 == 0 && stride_outer % 4 == 0 && stride_row % 4 == 0 && V % 4 == 0;
}

inline int ctc_check_blank(const char* who, int blank, int V) {
    AV_CHECK(blank >= 0 && blank < V, "%s: blank %d outside [0, %d)", who, blank, V);
    return AV_OK;
}

inline int ctc_check_smax(const char* who, int S_max) {
    AV_CHECK(S_max >= 1 && (S_max & 1), "%s: S_max = 2 Lmax + 1 must be odd and >= 1, got %d", who, S_max);
    return AV_OK;
}

}  // namespace
