// Word, character and token error counts on the device: batched edit distance WITH operation counts between one reference and N
// hypotheses per utterance, computed straight from token ids through a device copy of the tokenizer's piece table - the metric of
// MultimodalTrainer.evaluate() (model/trainer.py word_error_rate, the jiwer.wer stand-in) without a string on the host.  Lengths are read
// from DEVICE memory, nothing synchronises, no atomics: the output is the same from run to run.  Integers throughout (the same code in both
// libraries); the host path of error_rate.py restates this law and agrees exactly.
//
// Text of a sequence of ids (tokenizer.decode / beam_search.fast_decode, then .split()):
//   with a piece table, ids outside [0, V) are dropped; an id equal to the sequence's skip id is dropped (skip < 0: none);
//   the code points of the remaining pieces are concatenated, U+2581 read as U+0020; leading and trailing U+0020 are stripped.
//   token level: the kept ids.  character level: the stripped text, inner spaces included.  word level: maximal runs of non-space code
//   points, two words being equal when their code points are (a 32-bit hash filters, the content decides).
//   Without a table the ids are the symbols as given (only the skip id is dropped) and the character / word levels are -1.
// Counts of a pair (reference r, hypothesis h): among all alignments (match, substitution, deletion of a reference symbol, insertion of a
//   hypothesis symbol) the lexicographically smallest (cost = S + D + I, S, D).  The recurrence runs over the packed key
//   cost << 32 | S << 16 | D with plain signed 64-bit min (adding a step's key is monotone in that order; S, D <= 4096 < 2^16):
//     a[j]   = min(prev[j] + DEL, prev[j-1] + (r_i == h_j ? 0 : SUB))
//     cur[j] = min over k <= j of a[k] + (j - k) INS = j INS + prefix-min of (a[k] - k INS)           one scan per row, no serial walk
// Limits: up to 4096 ids per sequence; a sequence whose expanded text (before the strip) exceeds 4096 code points has character and word
//   levels -1 in every pair it takes part in; a hypothesis length < 0 means absent (all levels -1); lengths are clamped to [0, L].
//
// erc_expand_kernel    one workgroup of 256 per sequence (B (N + 1) of them): per tile of 256 ids one block scan of (kept, piece length)
//                      places the kept ids in the workspace and the code points in LDS; then strip (block min / max of the non-space
//                      positions), the stripped text to the workspace, and per word start (block scan of the start flags) one thread walks
//                      its word for the length and the hash.  Ids at or past a sequence's length are never read.
// erc_distance_kernel  one wave64 per (pair, level).  The hypothesis lies along the columns; the row of packed keys lives in LDS, column j
//                      always in lane j % 64, so every LDS word has ONE owner lane and the row loop needs no barrier.  Per chunk of 64
//                      columns: the diagonal neighbour by a lane shift, six shift-and-min steps for the prefix-min (DPP moves of the two
//                      halves of a key: no LDS round trip), the last lane's value carried into the next chunk.
#include "ctc_common.h"

namespace {

constexpr int ERC_MAXL = 4096;                    // ids per sequence, code points per text
constexpr int ERC_THREADS = 256;
constexpr int ERC_META = 4;                       // per sequence: kept ids (-1: absent), code points (-1: none), words (-1: none), unused
constexpr int ERC_SPACE = 0x20;
constexpr long long ERC_INS = 1LL << 32;
constexpr long long ERC_DEL = (1LL << 32) | 1LL;
constexpr long long ERC_SUB = (1LL << 32) | (1LL << 16);
constexpr long long ERC_INF = 1LL << 60;          // cost <= 8192 << 32: sums with it stay far from the sign bit

// Workspace of one sequence, in ints: meta [4] | kept ids [Lt] | stripped text [Cmax] | word (start, length) [Wmax][2] | word hash [Wmax]
struct ErcLayout {
    int Lt, Cmax, Wmax;
    long long per;
};

ErcLayout erc_layout(int Lr, int Lh, int max_piece) {
    ErcLayout l;
    l.Lt = Lr > Lh ? Lr : Lh;
    const long long c = (long long)l.Lt * max_piece;
    l.Cmax = (int)(c > ERC_MAXL ? ERC_MAXL : c);
    l.Wmax = (l.Cmax + 1) / 2;                    // words are separated by at least one space
    l.per = ERC_META + (long long)l.Lt + l.Cmax + 3LL * l.Wmax;
    return l;
}

// exclusive scan of (a, b) over the 256 threads of the workgroup and the totals; wt: LDS [2 * 4].  Two barriers, uniform call sites only
__device__ __forceinline__ void erc_block_scan(int a, int b, int* wt, int& ex_a, int& ex_b, int& tot_a, int& tot_b) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int ia = a, ib = b;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int ua = __shfl_up(ia, o, 64), ub = __shfl_up(ib, o, 64);
        if (lane >= o) { ia += ua; ib += ub; }
    }
    if (lane == 63) { wt[2 * wave] = ia; wt[2 * wave + 1] = ib; }
    __syncthreads();
    int pa = 0, pb = 0, ta = 0, tb = 0;
#pragma unroll
    for (int w = 0; w < ERC_THREADS / 64; ++w) {
        const int xa = wt[2 * w], xb = wt[2 * w + 1];
        if (w < wave) { pa += xa; pb += xb; }
        ta += xa; tb += xb;
    }
    __syncthreads();                              // wt may be written again
    ex_a = pa + ia - a; ex_b = pb + ib - b; tot_a = ta; tot_b = tb;
}

__global__ __launch_bounds__(ERC_THREADS) void erc_expand_kernel(const int* __restrict__ ref_ids, long long ref_ld,
                                                                 const long long* __restrict__ ref_lens, const int* __restrict__ hyp_ids,
                                                                 long long hyp_ld_b, long long hyp_ld_n,
                                                                 const long long* __restrict__ hyp_lens, int N, int Lr, int Lh,
                                                                 int ref_skip, int hyp_skip, const int* __restrict__ offsets,
                                                                 const int* __restrict__ pchars, int V, int max_piece, int Lt, int Cmax,
                                                                 int Wmax, long long per, int* __restrict__ ws) {
    __shared__ int s_text[ERC_MAXL];              // the expanded text before the strip
    __shared__ int s_wt[2 * (ERC_THREADS / 64)];
    __shared__ int s_lo[ERC_THREADS / 64], s_hi[ERC_THREADS / 64];
    const int tid = threadIdx.x;
    const int s = blockIdx.x, b = s / (N + 1), k = s % (N + 1);
    const bool table = offsets != nullptr;
    int* meta = ws + (long long)s * per;
    int* tok = meta + ERC_META;
    int* text = tok + Lt;
    int* wpos = text + Cmax;
    int* whash = wpos + 2 * Wmax;
    const int* ids;
    int L, skip;
    long long raw;
    if (k == 0) {
        ids = ref_ids + (long long)b * ref_ld; L = Lr; skip = ref_skip; raw = ref_lens[b];
    } else {
        ids = hyp_ids + (long long)b * hyp_ld_b + (long long)(k - 1) * hyp_ld_n; L = Lh; skip = hyp_skip;
        raw = hyp_lens[(long long)b * N + (k - 1)];
        if (raw < 0) {                            // absent hypothesis
            if (tid == 0) { meta[0] = -1; meta[1] = -1; meta[2] = -1; meta[3] = 0; }
            return;
        }
    }
    const int len = ctc_clamp_len(raw, L);
    int base_k = 0, base_c = 0;
    for (int t0 = 0; t0 < len; t0 += ERC_THREADS) {
        const int i = t0 + tid;
        int id = 0, keep = 0, pl = 0, o0 = 0;
        if (i < len) {
            id = ids[i];
            keep = (skip < 0 || id != skip) && (!table || (id >= 0 && id < V)) ? 1 : 0;
            if (keep && table) {
                o0 = offsets[id];
                pl = offsets[id + 1] - o0;
                pl = pl < 0 ? 0 : (pl > max_piece ? max_piece : pl);
            }
        }
        int ek, ec, tk, tc;
        erc_block_scan(keep, pl, s_wt, ek, ec, tk, tc);
        if (keep) {
            tok[base_k + ek] = id;
            const int c0 = base_c + ec;
            for (int q = 0; q < pl; ++q) {
                if (c0 + q < ERC_MAXL) {          // a longer text has no character level: what does not fit is not kept
                    const int cp = pchars[o0 + q];
                    s_text[c0 + q] = cp == 0x2581 ? ERC_SPACE : cp;
                }
            }
        }
        base_k += tk; base_c += tc;
    }
    __syncthreads();
    if (!table || base_c > ERC_MAXL) {
        if (tid == 0) { meta[0] = base_k; meta[1] = -1; meta[2] = -1; meta[3] = 0; }
        return;
    }
    // ---- strip: first and last non-space position ----
    int lo = ERC_MAXL, hi = -1;
    for (int p = tid; p < base_c; p += ERC_THREADS) {
        if (s_text[p] != ERC_SPACE) { lo = min(lo, p); hi = max(hi, p); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = min(lo, __shfl_xor(lo, o, 64)); hi = max(hi, __shfl_xor(hi, o, 64)); }
    if ((tid & 63) == 0) { s_lo[tid >> 6] = lo; s_hi[tid >> 6] = hi; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < ERC_THREADS / 64; ++w) { lo = min(lo, s_lo[w]); hi = max(hi, s_hi[w]); }
    const int nc = hi >= lo ? hi - lo + 1 : 0;    // nc <= base_c <= Cmax: each kept id brings at most max_piece code points
    const int* st = s_text + (nc ? lo : 0);
    for (int p = tid; p < nc; p += ERC_THREADS) text[p] = st[p];
    // ---- words ----
    int base_w = 0;
    for (int t0 = 0; t0 < nc; t0 += ERC_THREADS) {
        const int p = t0 + tid;
        const int flag = (p < nc && st[p] != ERC_SPACE && (p == 0 || st[p - 1] == ERC_SPACE)) ? 1 : 0;
        int ew, e2, tw, t2;
        erc_block_scan(flag, 0, s_wt, ew, e2, tw, t2);
        if (flag) {
            unsigned h = 2166136261u;             // FNV-1a over the code points: a filter, never the decision
            int e = p;
            for (; e < nc && st[e] != ERC_SPACE; ++e) h = (h ^ (unsigned)st[e]) * 16777619u;
            const int w = base_w + ew;            // w < Wmax: at most (nc + 1) / 2 words
            wpos[2 * w] = p;
            wpos[2 * w + 1] = e - p;
            whash[w] = (int)h;
        }
        base_w += tw;
    }
    if (tid == 0) { meta[0] = base_k; meta[1] = nc; meta[2] = base_w; meta[3] = 0; }
}

// Cross-lane moves of a 64-bit key as two data-parallel-primitive moves (no LDS round trip); a lane without a source keeps `old`.
constexpr int ERC_ROW_SHR = 0x110;                // + n: shift right by n lanes within each row of 16
constexpr int ERC_WAVE_SHR1 = 0x138;              // shift right by one lane across the whole wave
constexpr int ERC_ROW_BCAST15 = 0x142;            // lane 15 of each row to the next row
constexpr int ERC_ROW_BCAST31 = 0x143;            // lane 31 to rows 2 and 3

template <int CTRL, int ROW_MASK> __device__ __forceinline__ long long erc_dpp(long long old, long long src) {
    const int lo = __builtin_amdgcn_update_dpp((int)old, (int)src, CTRL, ROW_MASK, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(old >> 32), (int)(src >> 32), CTRL, ROW_MASK, 0xF, false);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

__device__ __forceinline__ long long erc_min(long long a, long long b) { return b < a ? b : a; }

// inclusive prefix-min over the 64 lanes: four steps inside each row of 16, then the rows' last lanes passed on
__device__ __forceinline__ long long erc_prefix_min(long long v) {
    v = erc_min(v, erc_dpp<ERC_ROW_SHR + 1, 0xF>(ERC_INF, v));
    v = erc_min(v, erc_dpp<ERC_ROW_SHR + 2, 0xF>(ERC_INF, v));
    v = erc_min(v, erc_dpp<ERC_ROW_SHR + 4, 0xF>(ERC_INF, v));
    v = erc_min(v, erc_dpp<ERC_ROW_SHR + 8, 0xF>(ERC_INF, v));
    v = erc_min(v, erc_dpp<ERC_ROW_BCAST15, 0xA>(ERC_INF, v));               // rows 1 and 3 take the row before them
    v = erc_min(v, erc_dpp<ERC_ROW_BCAST31, 0xC>(ERC_INF, v));               // rows 2 and 3 take everything up to lane 31
    return v;
}

__device__ __forceinline__ long long erc_last_lane(long long v) {
    const int lo = __builtin_amdgcn_readlane((int)v, 63), hi = __builtin_amdgcn_readlane((int)(v >> 32), 63);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

__global__ __launch_bounds__(64) void erc_distance_kernel(int N, int Lt, int Cmax, int Wmax, long long per, int cols,
                                                          const int* __restrict__ ws, int* __restrict__ out) {
    extern __shared__ long long erc_smem[];
    long long* row = erc_smem;                    // [cols] packed keys of the current row; column j belongs to lane j % 64
    int* hsym = (int*)(row + cols);               // [cols - 1] the hypothesis' symbols
    const int lane = threadIdx.x;
    const int unit = blockIdx.x, level = unit % 3, pair = unit / 3, b = pair / N, n = pair % N;
    const int* rm = ws + ((long long)b * (N + 1)) * per;
    const int* hm = ws + ((long long)b * (N + 1) + 1 + n) * per;
    int* o = out + (long long)unit * 4;
    const int nr = rm[level], nh = hm[0] < 0 ? -1 : hm[level];
    if (nr < 0 || nh < 0 || nh >= cols) {         // (nh < cols by the layout: a guard, not a case)
        if (lane == 0) { o[0] = -1; o[1] = -1; o[2] = -1; o[3] = -1; }
        return;
    }
    const int sym_off = level == 0 ? ERC_META : (level == 1 ? ERC_META + Lt : ERC_META + Lt + Cmax + 2 * Wmax);
    const int* rs = rm + sym_off;
    const int* hs = hm + sym_off;
    const int* rtext = rm + ERC_META + Lt;
    const int* htext = hm + ERC_META + Lt;
    const int* rw = rtext + Cmax;                 // word (start, length)
    const int* hw = htext + Cmax;
    const bool words = level == 2;
    for (int j = lane; j < nh; j += 64) hsym[j] = hs[j];
    for (int j = lane; j <= nh; j += 64) row[j] = (long long)j * ERC_INS;
    __syncthreads();                              // hsym is read across lanes (the block is one wave)
    int r_next = 0, rp_next = 0, rl_next = 0;
    if (nr > 0) {
        r_next = rs[0];
        if (words) { rp_next = rw[0]; rl_next = rw[1]; }
    }
    for (int i = 0; i < nr; ++i) {
        const int r = r_next, rp = rp_next, rl = rl_next;
        if (i + 1 < nr) {                         // the next row's symbol is in flight while this row runs
            r_next = rs[i + 1];
            if (words) { rp_next = rw[2 * (i + 1)]; rl_next = rw[2 * (i + 1) + 1]; }
        }
        long long diag_carry = ERC_INF;           // prev[c0 - 1]
        long long min_carry = ERC_INF;            // prefix-min over the columns before c0
        for (int c0 = 0; c0 <= nh; c0 += 64) {
            const int j = c0 + lane;
            const bool live = j <= nh;
            const long long p = live ? row[j] : ERC_INF;
            const long long pl = erc_dpp<ERC_WAVE_SHR1, 0xF>(diag_carry, p);        // prev[j - 1]; lane 0 keeps the carry
            diag_carry = erc_last_lane(p);
            long long a = p + ERC_DEL;
            if (live && j >= 1) {
                bool eq = hsym[j - 1] == r;
                if (words && eq) {                // the hash matched: the content decides
                    const int hp = hw[2 * (j - 1)], hl = hw[2 * (j - 1) + 1];
                    eq = hl == rl;
                    for (int q = 0; eq && q < rl; ++q) eq = rtext[rp + q] == htext[hp + q];
                }
                const long long d = pl + (eq ? 0LL : ERC_SUB);
                a = d < a ? d : a;
            }
            long long v = erc_prefix_min(a - (long long)j * ERC_INS);
            if (min_carry < v) v = min_carry;
            min_carry = erc_last_lane(v);
            if (live) row[j] = v + (long long)j * ERC_INS;
        }
    }
    __syncthreads();
    if (lane == (nh & 63)) {                      // the owner of column nh
        const long long key = row[nh];
        const int cost = (int)(key >> 32), S = (int)((key >> 16) & 0xFFFF), D = (int)(key & 0xFFFF);
        o[0] = S; o[1] = D; o[2] = cost - S - D; o[3] = nr;
    }
}

int erc_check_shape(const char* who, int B, int N, int Lr, int Lh, int max_piece) {
    AV_CHECK(B >= 1 && N >= 1, "%s: bad shape B=%d N=%d (both >= 1)", who, B, N);
    AV_CHECK(Lr >= 0 && Lr <= ERC_MAXL && Lh >= 0 && Lh <= ERC_MAXL, "%s: bad shape Lr=%d Lh=%d (0 <= L <= %d ids per sequence)", who, Lr,
             Lh, ERC_MAXL);
    AV_CHECK(max_piece >= 0 && max_piece <= ERC_MAXL, "%s: max_piece %d outside [0, %d]", who, max_piece, ERC_MAXL);
    AV_CHECK((long long)B * (N + 1LL) <= 0x7FFFFFFFLL / 3, "%s: B (N + 1) = %lld sequences are too many for one launch", who,
             (long long)B * (N + 1LL));
    return AV_OK;
}

long long erc_bytes(int B, int N, const ErcLayout& l) { return ((long long)B * (N + 1) * l.per * (long long)sizeof(int) + 15) / 16 * 16; }

}  // namespace

extern "C" int av_error_counts_workspace_bytes(int B, int N, int Lr, int Lh, int max_piece, long long* bytes) {
    AV_CHECK(bytes, "av_error_counts_workspace_bytes: null pointer");
    if (int rc = erc_check_shape("av_error_counts_workspace_bytes", B, N, Lr, Lh, max_piece)) return rc;
    *bytes = erc_bytes(B, N, erc_layout(Lr, Lh, max_piece));
    return AV_OK;
}

extern "C" int av_error_counts(const int* ref_ids, long long ref_ld, const long long* ref_lens, const int* hyp_ids, long long hyp_ld_b,
                               long long hyp_ld_n, const long long* hyp_lens, int B, int N, int Lr, int Lh, int ref_skip_id,
                               int hyp_skip_id, const int* piece_offsets, const int* piece_chars, int V, int max_piece, int* out_counts,
                               void* workspace, long long workspace_bytes, void* stream) {
    AV_CHECK(ref_lens && hyp_lens && out_counts && workspace, "av_error_counts: null pointer");
    AV_CHECK((ref_ids || Lr == 0) && (hyp_ids || Lh == 0), "av_error_counts: null pointer (ids with Lr=%d Lh=%d)", Lr, Lh);
    const bool table = piece_offsets != nullptr;
    AV_CHECK(table == (piece_chars != nullptr), "av_error_counts: null pointer (piece_offsets and piece_chars go together)");
    if (!table) max_piece = 0;
    if (int rc = erc_check_shape("av_error_counts", B, N, Lr, Lh, max_piece)) return rc;
    AV_CHECK(!table || (V >= 1 && max_piece >= 1), "av_error_counts: a piece table needs V >= 1 and max_piece >= 1, got V=%d max_piece=%d", V,
             max_piece);
    AV_CHECK(ref_ld >= Lr && hyp_ld_n >= Lh && hyp_ld_b >= (long long)(N - 1) * hyp_ld_n + Lh,
             "av_error_counts: leading dimensions (ref %lld, hyp b %lld, hyp n %lld) do not cover [B][%d] and [B][%d][%d]", ref_ld, hyp_ld_b,
             hyp_ld_n, Lr, N, Lh);
    const ErcLayout l = erc_layout(Lr, Lh, max_piece);
    const long long need = erc_bytes(B, N, l);
    AV_CHECK(workspace_bytes >= need, "av_error_counts: workspace of %lld bytes is too small, %lld needed", workspace_bytes, need);
    AV_CHECK((uintptr_t)workspace % 16 == 0, "av_error_counts: workspace must be 16-byte aligned");
    const int maxn = l.Lt > l.Cmax ? l.Lt : l.Cmax;                          // symbols of a hypothesis at any level
    const int cols = (maxn + 1 + 1) / 2 * 2;                                 // even: the int array behind the row stays 8-byte aligned
    const long long lds = (long long)cols * sizeof(long long) + (long long)cols * sizeof(int);
    AV_CHECK(lds <= CTC_LDS_LIMIT, "av_error_counts: %d columns need %lld bytes of LDS (limit %lld)", cols, lds, CTC_LDS_LIMIT);
    hipLaunchKernelGGL(erc_expand_kernel, dim3(B * (N + 1)), dim3(ERC_THREADS), 0, (hipStream_t)stream, ref_ids, ref_ld, ref_lens, hyp_ids,
                       hyp_ld_b, hyp_ld_n, hyp_lens, N, Lr, Lh, ref_skip_id, hyp_skip_id, piece_offsets, piece_chars, V, max_piece, l.Lt,
                       l.Cmax, l.Wmax, l.per, (int*)workspace);
    AV_LAUNCH_CHECK();
    hipLaunchKernelGGL(erc_distance_kernel, dim3(B * N * 3), dim3(64), (size_t)lds, (hipStream_t)stream, N, l.Lt, l.Cmax, l.Wmax, l.per, cols,
                       (const int*)workspace, out_counts);
    AV_LAUNCH_CHECK();
    return AV_OK;
}
