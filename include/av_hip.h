/* C-ABI of libavhip.so — the MI355X (gfx950) kernels behind the audio-visual CTC path.
 *
 * The reference (limeorange1102/multimodal-av-model) has no FFI of its own: every device op is a PyTorch /
 * HuggingFace call.  Each entry point below therefore cites the reference call site (file:line, `hf:` =
 * transformers/models/wav2vec2/modeling_wav2vec2.py 5.15.0, `torch:` = torch/nn 2.10) whose arithmetic it
 * replaces.  Conventions:
 *   - plain pointers + sizes only, no torch types; all buffers are owned by the caller (PyTorch caching
 *     allocator) and outlive the call; workspaces are passed in;
 *   - every call enqueues on the given hipStream_t (passed as void*) and returns immediately;
 *   - return 0 on success, non-zero on error with a message in av_last_error(); never abort();
 *   - dtype codes: AV_F32 = 0 (parity mode), AV_BF16 = 1 (perf mode).  Accumulation is always fp32.
 */
#ifndef AV_HIP_H
#define AV_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define AV_OK 0
#define AV_ERR_ARG 1
#define AV_ERR_LAUNCH 2

#define AV_F32 0
#define AV_BF16 1

/* A-operand addressing modes of av_gemm */
#define AV_A_ROWMAJOR 0 /* A[m][k] at A + m*lda + k                                   */
#define AV_A_TRANS 1    /* A[m][k] at A + k*lda + m           (dW = dY^T X)           */
#define AV_A_CONV2D 2   /* implicit im2col of an NHWC image (ResNet convs, pos-conv)  */
#define AV_A_CONV3D1 3  /* implicit im2col of a 1-channel [N,T,H,W] volume (front-end) */
/* B-operand modes */
#define AV_B_NK 0 /* B[n][k] at B + n*ldb + k  (nn.Linear weight layout)  */
#define AV_B_KN 1 /* B[k][n] at B + k*ldb + n                             */
/* epilogue activation */
#define AV_ACT_NONE 0
#define AV_ACT_GELU 1          /* v = gelu(v)                     hf:565-572, hf:291-299 */
#define AV_ACT_MUL_GELU_GRAD 2 /* v = v * gelu'(aux[m][n])        backward of the above  */
#define AV_ACT_GELU_GF 3       /* m = dropout multiplier; C2 = gelu'(v) * m (the "gradient factor"), v = gelu(v) * m: the
                                  backward of this activation + dropout site is then ONE multiply, AV_ACT_MUL_AUX        */
#define AV_ACT_MUL_AUX 4       /* v = v * aux[m][n]               backward of AV_ACT_GELU_GF (aux = its C2)              */

const char* av_last_error(void);
int av_version(void);

/* ---- MFMA GEMM family: C = epilogue(alpha * A x B) ------------------------------------------------------
 * replaces: nn.Linear (hf:522-527,546,565-572,429-434; model/fusion_module.py:57-58,63; model/decoder.py:24),
 * F.conv1d of the wav2vec2 feature encoder layers 1-6 as a strided GEMM (hf:291-299), the grouped positional
 * conv (hf:360-368), nn.Conv2d of the ResNet trunk (model/encoder.py:9-12,36), nn.Conv3d front-end
 * (model/encoder.py:61), and all the dX / dW products of their backward passes.
 * epilogue, in order: v = alpha*acc; v += bias[n]; C2[m][n] = v (optional pre-activation copy);
 * act; optional dropout; v += R[m][n] (fp32 residual, may alias C); C[m][n] = v;  optional per-column sum / sum-of-squares
 * partials for train-mode BatchNorm statistics (model/trainer.py:54): stats[blockRow][0/1][n].               */
typedef struct av_gemm_args {
    const void* A;
    const void* B;
    void* C;
    void* C2;          /* optional, same dtype/ld as C */
    const float* bias; /* optional [N] */
    const float* R;    /* optional fp32 residual, ld = ldr */
    const void* aux;   /* AV_ACT_MUL_GELU_GRAD / AV_ACT_MUL_AUX operand, dtype = aux_dtype, ld = ldc */
    float* stats;      /* optional [ceil(M/128)][2][N] fp32 partials (batch must be 1) */
    int M, N, K, batch;
    long long lda, ldb, ldc, ldr;
    long long sA, sB, sC, sR, sBias; /* batch strides in elements */
    int a_mode, b_mode, in_dtype, out_dtype, aux_dtype, act;
    float alpha;
    /* implicit-im2col geometry (a_mode 2/3): input [img][T][H][W][Ctot] (T = 1 for 2-D) */
    int cT, cH, cW, cCtot, cCin, cCoff;
    int cKt, cKh, cKw, cSh, cSw, cPt, cPh, cPw, cOh, cOw;
    /* optional two-level batch: z = zo*batch_inner + zi; offsets zo*o? + zi*s? (batch_inner = 0: one level) */
    int batch_inner;
    long long oA, oB, oC;
    /* optional dropout in the epilogue (hf:628-633,565-572 hidden / activation dropout): after the activation and BEFORE the
     * residual, v *= mask(seed, stream, idx) in {0, 1/(1-p)}, idx = the element's offset from C: batch offset (zo*oC + zi*sC, or
     * z*sC with one level) + m*ldc + n; with AV_ACT_MUL_GELU_GRAD the same mask multiplies the gradient.  drop_p = 0 disables it. */
    float drop_p;
    unsigned int drop_stream;
    unsigned long long drop_seed;
    /* optional split-K over the (one-level) batch: when k_total > 0, batch z multiplies k in [z*K, min((z+1)*K, k_total)).
     * Only with both operands k-major (a_mode 1, b_mode 1, bf16 fast kernel): dW = dY^T X with few output tiles; the
     * partial products C + z*sC are summed with av_sum_slices. */
    int k_total;
    /* position-major pixel order for 2-D implicit-im2col products (a_mode 2, bf16 fast path).  Images are taken in blocks of cNF (the
     * image count must be a multiple of it); inside a block the rows are ordered [pixel position][image of the block]: image q's pixel
     * `pos` of a P-pixel map is row ((q / cNF) * P + pos) * cNF + q % cNF.  cPM bit 0: the INPUT is in that order (P = cH * cW), bit 1:
     * the OUTPUT is (P = cOh * cOw).  With cNF a multiple of the row tile (256) every row tile lies at one output position, so filter taps
     * that fall outside the image for that position are skipped as whole K-tiles (3 x 3 images under a 3 x 3 filter, model/encoder.py:36
     * layer4: 49 of 81 taps do work), and consecutive row tiles re-read the same images' pixels from L2.  0 / 0 = frame-major order. */
    int cNF, cPM;
} av_gemm_args;
int av_gemm(const av_gemm_args* args, void* stream);

/* Launch record of av_gemm: a test and diagnostic aid.  Every av_gemm call of a thread clears that thread's record and, when it launches
 * a kernel, fills it in next to the launch; nothing reads it back inside the library, and no dispatch decision depends on it.  Tests assert
 * it so that a case whose shape no longer reaches the kernel it was written for fails instead of silently testing another one. */
#define AV_GEMM_KERNEL_NONE 0    /* no launch by the last call (M or N zero, or an error before the launch) */
#define AV_GEMM_KERNEL_GENERIC 1 /* gemm.hip: 128 x bn tile; in16 = 16-bit operands (else fp32), bn = 64 / 128 */
#define AV_GEMM_KERNEL_FAST128 2 /* gemm_fast.hip 128 x bn kernel: bn = its BNT (64 / 128), conv, akm, bkm = its template form */
#define AV_GEMM_KERNEL_V2 3      /* 256 x 128 three-stage kernel */
#define AV_GEMM_KERNEL_V4 4      /* 8-phase 256 x 256 kernel, plain form */
#define AV_GEMM_KERNEL_V4_CONV 5 /* 8-phase kernel, implicit-im2col form */
#define AV_GEMM_KERNEL_V4_KM 6   /* 8-phase kernel, both operands k-major */
#define AV_GEMM_KERNEL_V6 7      /* four-wavefront kernel behind its switch */
#define AV_GEMM_KERNEL_V7 8      /* persistent kernel: act, out_dtype, nm1 = its instantiation */
typedef struct av_gemm_launch_info {
    int kernel;              /* AV_GEMM_KERNEL_* */
    int in16, bn;            /* generic / 128 x bn kernels */
    int conv, akm, bkm;      /* operand form of the 128 x bn and 8-phase kernels */
    int act, out_dtype, nm1; /* the v7 instantiation (act and out_dtype are filled in for every kernel; nm1 = 0 elsewhere) */
    int bm_eff;              /* rows a row tile owns (v4 / v7: 160 .. 256; the tile height elsewhere) */
    int nbM, nbN;            /* row and column tiles */
    int nfull;               /* v4 / v7: tiles run whole; the nbM * nbN - nfull tiles after them run as four quadrant jobs each */
    int grid_x, grid_z;      /* the launch grid */
    int c_vec, r_vec, aux_vec; /* the fast path's FastFlags: 16-byte stores of C / C2, loads of R, loads of aux (0 on the generic kernel) */
} av_gemm_launch_info;
/* copies the calling thread's record; returns AV_OK, or AV_ERR_ARG for a null pointer */
int av_gemm_last_launch(av_gemm_launch_info* out);

/* out[i] = (accumulate ? out[i] : 0) + alpha * sum_s parts[s*stride + i], i < n (fp32): the split-K partials of av_gemm */
int av_sum_slices(const float* parts, int n_slices, long long n, long long stride, float alpha, float* out, int accumulate,
                  void* stream);
/* out[C][Rpad] = in[R][C]^T (zero-filled for r >= R): brings dX / dW products to the fast K-contiguous form */
int av_transpose(const void* in, int idt, void* out, int odt, int R, int C, long long ldi, int Rpad, void* stream);

/* ---- row kernels (one wavefront per row, shuffle reductions) ------------------------------------------- */
/* nn.LayerNorm over the last dim (hf:297,431,638,644,791), eps 1e-5, optional exact-erf GELU (hf:298).
 * x [rows][cols] (dtype xdt), y (dtype ydt); mean/rstd [rows] fp32 optional (saved for backward). */
int av_layernorm_fwd(const void* x, int xdt, const float* gamma, const float* beta, void* y, int ydt,
                     float* mean, float* rstd, long long rows, int cols, float eps, int act, void* stream);
/* dx = dres + LN'(dy) (dres optional fp32); dgamma/dbeta partials [nblk][2][cols] (optional; reduce with
 * av_colsum). x fp32/bf16 (xdt), dy dtype dydt, dx fp32; dx_bf16 (optional): bf16 copy of dx for the next GEMM. */
int av_layernorm_bwd(const void* x, int xdt, const void* dy, int dydt, const float* gamma, const float* mean,
                     const float* rstd, const float* dres, float* dx, float* dgb_partial, int nblk,
                     long long rows, int cols, void* dx_bf16, void* stream);
/* the same with dropout folded into the bf16 copy: dx_bf16 = bf16(dx o mask / (1 - p)), mask = Philox(seed, stream, element index):
 * the backward of a dropout that sits between this LayerNorm's input and the next dX GEMM (hf:633,648: hidden dropout) */
int av_layernorm_bwd_drop(const void* x, int xdt, const void* dy, int dydt, const float* gamma, const float* mean,
                          const float* rstd, const float* dres, float* dx, float* dgb_partial, int nblk,
                          long long rows, int cols, void* dx_bf16, float drop_p, unsigned long long drop_seed,
                          unsigned int drop_stream, void* stream);
/* F.log_softmax(dim=-1) (model/decoder.py:25) and its backward: dx = dy - exp(y) * sum(dy) */
int av_log_softmax_fwd(const void* x, int xdt, float* y, long long rows, int cols, void* stream);
int av_log_softmax_bwd(const float* y, const float* dy, void* dx, int dxdt, long long rows, int cols, void* stream);
/* the same with a row stride ldx >= cols for dx; columns [cols, ldx) are written as zeros, so that dx can feed a GEMM whose K is padded to a
 * multiple of 64 (the CTC head's dX product: vocabulary 800 -> 832) */
int av_log_softmax_bwd_ld(const float* y, const float* dy, void* dx, int dxdt, long long rows, int cols, int ldx, void* stream);
/* column sums of a [rows][cols] matrix (bias gradients): out[cols] (+)= sum_rows x */
int av_colsum(const void* x, int xdt, float* out, long long rows, int cols, long long ld, int accumulate,
              void* stream);
/* elementwise */
int av_cast(const void* x, int xdt, void* y, int ydt, long long n, void* stream);
/* y = cast(x * dropout_mask(seed, stream, i)) — forward dropout and its backward (same mask) in one kernel; p = 0: plain cast */
int av_cast_dropout(const void* x, int xdt, void* y, int ydt, long long n, float p, unsigned long long seed, unsigned int stream_id,
                    void* stream);
/* debug / test: u[i] = the uniform number behind the mask of element i */
int av_dropout_uniform(float* u, long long n, unsigned long long seed, unsigned int stream_id, void* stream);
/* SpecAugment time masking (hf:1272-1296): x[row][:] = embed[:] where mask[row] != 0 */
/* fused cross-attention block of CrossAttentionFusion (model/fusion_module.py:57-61; nn.MultiheadAttention need-weights path,
 * torch:functional.py:6206,6576-6606): packed in-projection + attention core of one (batch item, head) per workgroup.
 * a, v [B, T, 512] bf16 (audio / visual projections); w_in [1536, 512] bf16, b_in [1536] fp32 (in_proj_weight / in_proj_bias);
 * o [B, T, 512] bf16 = concat_h softmax(scale q_h k_h^T) v_h; q_out [B, T, 512], kv_out [B, T, 2, 512], lse [B, H, T] are optional
 * (what the backward reads).  embed_dim 512, 4 heads x 128, T <= 112 */
int av_fusion_xattn_fwd(const void* a, const void* v, const void* w_in, const float* b_in, void* q_out, void* kv_out, void* o,
                        float* lse, int B, int T, int E, int H, float scale, void* stream);
/* backward of that attention core (P recomputed from the row LSE): q, o, dout [B, T, 512], kv [B, T, 2, 512] bf16, lse [B, H, T] ->
 * dq [B, T, 512], dkv [B, T, 2, 512]; one workgroup per (item, head), every operand staged once, no atomics (T <= 112) */
int av_fusion_xattn_bwd(const void* q, const void* kv, const void* o, const void* dout, const float* lse, void* dq, void* dkv, int B, int T,
                        int E, int H, float scale, void* stream);
/* SpecAugment feature-axis masking (hf:1298-1316): x[b, t, c] = 0 for all t where mask[b * H + c] != 0 */
int av_zero_feature_cols(void* x, int xdt, const unsigned char* mask, int B, int T, int H, void* stream);
int av_overwrite_rows(void* x, int xdt, const unsigned char* mask, const float* embed, long long rows, int cols, void* stream);
int av_axpby(float a, const void* x, int xdt, float b, float* y, long long n, void* stream); /* y = a*x + b*y */
int av_mask_rows(void* x, int xdt, const unsigned char* keep, long long rows, int cols, void* stream); /* hf:752-755 */
int av_mul_scalar_dev(const float* x, const float* scalar, float* y, long long n, void* stream); /* y = scalar[0]*x, scalar on device */

/* ---- fused attention (flash-style forward) ---------------------------------------------------------------
 * O = softmax(scale*Q K^T + key-padding mask) V, LSE saved.  Replaces hf:438-463 (sdpa, 16 heads x 64) and the
 * need_weights path of nn.MultiheadAttention (torch:functional.py:6576-6606; fusion_module.py:61, 4 heads x 128).
 * Element (b, t, h, d) of Q at q + b*q_bs + t*q_rs + h*D + d (same for K, V, O).  klen[b] = number of valid
 * keys (NULL: all Tk).  lse [B][H][Tq] fp32 (optional).  D in {16,32,64,128}. */
int av_attention_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int dtype, int B, int H, int Tq,
                     int Tk, int D, long long q_bs, long long q_rs, long long k_bs, long long k_rs, long long v_bs,
                     long long v_rs, long long o_bs, long long o_rs, const int* klen, float scale, float drop_p,
                     unsigned long long drop_seed, unsigned int drop_stream, void* stream);
/* fused (flash-style) attention backward, bf16: recomputes P from Q, K and the forward's LSE; dq/dk/dv written in place.
 * strides[16] = (batch stride, row stride) of q, k, v, o, dout, dq, dk, dv (elements; head stride = D);
 * delta_ws: B*H*Tq floats of workspace.  Backward of hf:438-463 / fusion_module.py:61. */
int av_attention_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                     float* delta_ws, void* dq, void* dk, void* dv, int B, int H, int Tq, int Tk, int D,
                     const long long* strides, const int* klen, float scale, float drop_p, unsigned long long drop_seed,
                     unsigned int drop_stream, void* stream);
/* Attention-probability dropout with PRECOMPUTED keep bits (whole-sequence bf16 kernels only: head_dim 64, Tq, Tk <= 256).
 * av_attention_dropmask evaluates the (seed, stream, index) Philox masks once: mask = [B][H][ceil(Tq / 16)][64] 64-bit words, 32-byte
 * aligned; bit 4 t + e of lane (r, g)'s word of query tile qt <-> (query 16 qt + r, key 16 t + 4 g + e).  The _mask forms of the
 * forward and the backward read 1 bit per probability instead of evaluating the generator (once in the forward, twice in the
 * backward).  Results are bit-identical to the calls without a mask. */
int av_attention_dropmask(void* mask, int B, int H, int Tq, int Tk, float drop_p, unsigned long long drop_seed, unsigned int drop_stream,
                          void* stream);
int av_attention_fwd_mask(const void* q, const void* k, const void* v, void* o, float* lse, int dtype, int B, int H, int Tq,
                          int Tk, int D, long long q_bs, long long q_rs, long long k_bs, long long k_rs, long long v_bs,
                          long long v_rs, long long o_bs, long long o_rs, const int* klen, float scale, float drop_p,
                          unsigned long long drop_seed, unsigned int drop_stream, const void* drop_mask, void* stream);
int av_attention_bwd_mask(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                          float* delta_ws, void* dq, void* dk, void* dv, int B, int H, int Tq, int Tk, int D,
                          const long long* strides, const int* klen, float scale, float drop_p, unsigned long long drop_seed,
                          unsigned int drop_stream, const void* drop_mask, void* stream);
/* rows of the (unfused, fp32 parity mode) attention backward: P = softmax(scale*S) with key mask; dS = scale * P o (dP - sum(dP o P)) */
int av_softmax_rows(const float* s, void* p, int pdt, long long rows, int cols, float scale, const int* klen,
                    int rows_per_batch, int ld, void* stream);
int av_softmax_bwd_rows(const void* p, int pdt, const float* dp, void* ds, int dsdt, long long rows, int cols,
                        float scale, int ld, void* stream);

/* ---- wav2vec2 feature-encoder layer 0, fused Conv1d(1->C,k,stride)+bias -> LayerNorm(C) -> GELU (hf:291-299).
 * wav [B][T_in] fp32 -> out [B][L_out][C] channel-last in out_dtype; w [C][k] fp32. */
int av_conv0_ln_gelu(const float* wav, const float* w, const float* bias, const float* gamma, const float* beta, void* out,
                     int out_dtype, int B, int T_in, int L_out, int C, int k, int stride, float eps, void* stream);

/* ---- bidirectional LSTM time steps (nn.LSTM(512,512,2,bidirectional), model/fusion_module.py:21-27,64) ----
 * Time-major internal buffers; both directions advance in one launch (step s: fwd chain at time s, reverse
 * chain at T-1-s).  gx = x W_ih^T + b_ih + b_hh for all steps comes from av_gemm.  fwd: h,c,(gates) of step s;
 * bwd (s counts from the END of each chain): dgates[t] from dout[t] + dgates[t_next] W_hh, running dc in place. */
int av_lstm_fwd_step(const float* gx, const void* whh, void* hseq, float* cseq, void* gates, void* out_bt, int dtype,
                     int T, int B, int H, int s, void* stream);
int av_lstm_bwd_step(const void* dout, int dout_dtype, long long do_bs, long long do_ts, void* dgates, const void* whhT,
                     const void* gates, const float* cseq, float* dc, int dtype, int T, int B, int H, int s, void* stream);

/* persistent form (bf16, H = 512): ONE launch per layer for all T steps of both directions.  Grid = 32 unit tiles x 2 directions x
 * up to 4 row groups of 16 batch rows; every (direction, row group) is an independent chain of 32 resident workgroups whose steps
 * are separated by an arrival counter (agent-coherent stores / loads, bounded spins: counters[2] is set on timeout).  W_hh slices
 * stay in registers for the whole sequence.  counters: AV_LSTM_COUNTER_INTS ints of device workspace (zeroed by the call).
 * Same buffers as the step kernels; results agree with them to fp32 rounding of the K-quarter partial sums. */
#define AV_LSTM_COUNTER_INTS 1024
int av_lstm_fwd_layer(const float* gx, const void* whh, void* hseq, float* cseq, void* gates, void* out_bt, int* counters,
                      int T, int B, int H, void* stream);
int av_lstm_bwd_layer(const void* dout, int dout_dtype, long long do_bs, long long do_ts, void* dgates, const void* whhT,
                      const void* gates, const float* cseq, float* dc, int* counters, int T, int B, int H, void* stream);

/* ---- fusion glue without host syncs (model/fusion_module.py:40-55,66; model/trainer.py:98,102) ------------- */
int av_mask_downsample(const long long* mask, long long* out, int B, int Tin, int Tout, void* stream);
/* ws_i32: B*Ta + B + groups ints (compaction index, counts, per-group batch max) kept for the backward;
 * the reference's "pad to the batch maximum" is evaluated per group of B/groups consecutive items */
int av_fusion_gather_lerp_fwd(const float* feat, const long long* mask, int* ws_i32, float* out, long long* mask_out,
                              long long* lens, int B, int Ta, int Tv, int D, int groups, void* stream);
int av_fusion_gather_lerp_bwd(const float* dout, const int* ws_i32, float* dfeat, int B, int Ta, int Tv, int D, int groups,
                              void* stream);
int av_permute_bt(const void* in, int idt, void* out, int odt, int B, int T, int D, void* stream); /* [B,T,D]->[T,B,D] */
int av_gather_rows(const void* src, int sdt, const long long* idx, void* out, int odt, long long n, int D, void* stream);
int av_scatter_rows(const float* src, const long long* idx, float* out, long long n, int D, float alpha, int accumulate,
                    void* stream);
/* contrastive.py:24-26 class order (anchors = mask 1, positives = 2, negatives = 0, anything else last), stable: order[] = what a stable
 * argsort of the class rank gives; int64 in, int64 out, one launch */
int av_class_order(const long long* mask, long long n, long long* order, void* stream);

/* ---- lip-frame encoder glue (model/encoder.py:6-75): train-mode BatchNorm, PReLU, pooling; NHWC ------------ */
/* bf16 fast path of the Conv3d(1->64,(5,7,7),(1,2,2),(2,3,3)) front-end (model/encoder.py:61): x [B*T][H][W] fp32,
 * w bf16 [64][288] with k = (kt*7+ky)*8+kx (kx padded to 8, K padded to 288), y bf16 [B*T][H/2][W/2][64],
 * stats [B*T*(H/16)*(W/32)][2][64] BatchNorm partials (optional). */
int av_conv3d_front(const float* x, const void* w, void* y, float* stats, int B, int T, int H, int W, void* stream);
/* the same convolution fused with the first half of model/encoder.py:62-64 (BatchNorm3d + PReLU + MaxPool3d((1,3,3),(1,2,2),(0,1,1))):
 * instead of the conv output it writes, per 3 x 3 / stride 2 / pad 1 pooling window and channel, the MAXIMUM and the MINIMUM of the
 * (bf16-rounded) conv output: ymax, ymin bf16 [B*T][H/4][W/4][64].  Train-mode BatchNorm needs the whole batch before it can be applied,
 * but bn followed by prelu is monotone or V-shaped per channel, so max over the window of prelu(bn(x)) = max(prelu(bn(max x)), prelu(bn(min x)))
 * exactly; av_bn_prelu_minmax evaluates that once scale / shift exist.  stats as above (partials of the UNPOOLED output). */
int av_conv3d_front_pool(const float* x, const void* w, void* ymax, void* ymin, float* stats, int B, int T, int H, int W, void* stream);
/* out[i] = max(prelu(ymax[i] * scale[c] + shift[c]), prelu(ymin[i] * scale[c] + shift[c])), c = i % 64; bf16, n elements (a multiple of 64) */
int av_bn_prelu_minmax(const void* ymax, const void* ymin, const float* scale, const float* shift, const float* slope, void* out, long long n,
                       void* stream);
/* bf16 fast path of the 3x3 / stride 1 / pad 1, 64 -> 64 channel convolutions of ResNet-18 layer1 (model/encoder.py:44-57):
 * x bf16 NHWC [n_img][H][W][64], w bf16 [64][9*64] with k = (ky*3+kx)*64 + c, y bf16 [n_img*H*W][64],
 * stats [ceil(n_img*H*W/256)][2][64] BatchNorm partials (optional).  Weights stay in LDS, the input is staged once per filter row. */
int av_conv3x3_c64(const void* x, const void* w, void* y, float* stats, int n_img, int H, int W, const float* in_scale,
                   const float* in_shift, const float* in_slope, void* stream);
/* ws: 2C + 1 doubles of workspace (2C accumulators + an arrival ticket: train mode is ONE launch, the last workgroup finalizes).
 * ws_zeroed = 1: the caller guarantees ws is zero on entry (the kernel leaves it zero on exit, so one buffer zeroed once serves every
 * BatchNorm of a stream); 0: it is cleared here first. */
int av_bn_finalize(const float* partial, int nblk, long long count, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float momentum, float eps, int training, float* scale,
                   float* shift, int C, double* ws, int ws_zeroed, void* stream);
int av_bn_act(const void* x, const float* scale, const float* shift, const void* res, const float* rscale,
              const float* rshift, const float* slope, void* out, int dtype, long long n, int C, void* stream);
int av_bn_prelu_maxpool(const void* x, const float* scale, const float* shift, const float* slope, void* out, int dtype,
                        long long N, int H, int W, int C, void* stream);
int av_avgpool(const void* x, int dtype, float* out, long long N, int HW, int C, int pm_block, void* stream);   /* pm_block: 0 = frame-major, else images per position-major block (av_gemm_args.cNF) */

/* ---- loss / optimizer side (contrastive.py:8-44; torch.optim.Adam, model/trainer.py:34-39) ------------------ */
int av_l2norm_fwd(const float* x, float* y, float* nrm, long long rows, int cols, float eps, void* stream);
int av_l2norm_bwd(const float* y, const float* dy, const float* nrm, float* dx, long long rows, int cols, float eps,
                  void* stream);
int av_lse_rows(const float* s, float* lse, float* rowsum, long long rows, int cols, int ld, void* stream);
int av_contrastive_dsim(const float* s, const float* lse, void* out, int odt, long long rows, int cols, int ld, float coef,
                        void* stream);
/* column-chunked forms (the N1 x N2 similarity matrix of contrastive.py:30-43 is never materialised whole: S is produced and
 * consumed one [row chunk] x [column chunk] block at a time and recomputed in the backward): av_lse_rows_chunk merges the chunk's
 * row LSE / row sum into the running values when accumulate != 0; av_contrastive_dsim_chunk uses the row LSE over ALL columns
 * and 1 / total_cols */
int av_lse_rows_chunk(const float* s, float* lse, float* rowsum, long long rows, int cols, int ld, int accumulate, void* stream);
int av_contrastive_dsim_chunk(const float* s, const float* lse, void* out, int odt, long long rows, int cols, int ld, float coef,
                              int total_cols, void* stream);
int av_reduce_sum(const float* x, long long n, float* out, float scale, int accumulate, void* stream);
/* loss combination of the trainer (model/trainer.py:111-119): out3 = {sum_i nll[i] w[i] + half_lambda (c1 + c2), 2 x first-half sum,
 * 2 x second-half sum}; nll, w fp32 [n] (n even: speaker 1 then speaker 2), c1 / c2 optional device scalars */
int av_loss_combine(const float* nll, const float* w, const float* c1, const float* c2, float half_lambda, int n, float* out3,
                    void* stream);
/* greedy CTC decoding (beam_search.py:2-48; the reference's beam search returns the per-frame argmax path): log_probs fp32
 * [B][T][V], lengths optional int64 [B] (frames to decode); out_ids int32 [B][T] = collapsed ids padded with -1, out_len int32 [B] */
int av_ctc_greedy(const float* log_probs, const long long* lengths, int* out_ids, int* out_len, int B, int T, int V, int blank,
                  void* stream);
/* CTC prefix beam search without a language model (with one: av_ctc_beam_search_lm below), n-best (the decoder the reference's beam_search.py:2-48 is named after; opt-in
 * in evaluate(), trainer.py:230,237): per prefix the blank-ending and non-blank-ending log-masses, equal prefixes merged by content,
 * the beam_width best kept per frame.  log_probs fp32, element [b][t][v] at b * stride_b + t * stride_t + v; lengths optional
 * int64 [B] on the DEVICE (frames to consume, clamped to [0, T]); no host synchronisation.  1 <= beam_width <= 64,
 * 1 <= nbest <= beam_width, T <= 4096, V >= 2, 0 <= blank < V.  out_ids int32 [B][nbest][T] = the hypotheses in descending score
 * order, each padded with -1; out_len int32 [B][nbest] (-1: fewer than nbest hypotheses exist); out_score fp32 [B][nbest] =
 * log-likelihood summed over the alignments the search kept.  Equal scores are ordered by candidate id (csrc/ctc_beam.hip).
 * workspace: av_ctc_beam_workspace_bytes(B, T, V, beam_width) bytes, 8-byte aligned; a smaller one is an error status.
 * av_ctc_beam_frame_pass (the first of the two passes alone: the beam_width + 1 best non-blank tokens of every consumed frame into the
 * workspace) is what av_ctc_beam_search runs first; it is exported for tools/beam_timing.py (beam_search.py:2-48). */
int av_ctc_beam_workspace_bytes(int B, int T, int V, int beam_width, long long* bytes);
int av_ctc_beam_frame_pass(const float* log_probs, long long stride_b, long long stride_t, const long long* lengths, void* workspace,
                           long long workspace_bytes, int B, int T, int V, int blank, int beam_width, void* stream);
int av_ctc_beam_search(const float* log_probs, long long stride_b, long long stride_t, const long long* lengths, int* out_ids,
                       int* out_len, float* out_score, void* workspace, long long workspace_bytes, int B, int T, int V, int blank,
                       int beam_width, int nbest, void* stream);
/* Token n-gram language model (lm.py: NGramLM) and CTC prefix beam search with its shallow fusion (csrc/ngram_lm.h, csrc/ngram_lm.hip;
 * the fused search is the other instantiation of the search kernel of csrc/ctc_beam.hip).
 * Tables: lm_unigrams fp32 [lm_vocab + 1][2] = (logp, backoff), natural log, row lm_vocab = begin of sentence; lm_table = lm_slots
 * 16-byte slots {u64 key, f32 logp, f32 backoff}, 16-byte aligned, lm_slots a power of two, key 0 = empty, linear probing from
 * splitmix64(key) & (lm_slots - 1), every stored key within lm_probe_bound probes (lookups make no more, at masked indices); keys = the
 * n-gram's tokens oldest first as id + 1 in 16-bit fields.  1 <= lm_order <= 4, 2 <= lm_vocab <= 65533, lm_bos = lm_vocab or -1 (none).
 * s(c | ctx): for m from min(lm_order - 1, tokens available) down to 1, the (m + 1)-gram's logp if it is stored, else add the context
 * m-gram's backoff (nothing if absent) and shorten the context; at m = 0 the unigram.  float32 additions in that order only: the bits of
 * NGramLM.score.
 * av_ngram_score: ids int32 [B][Lmax], lens optional int64 [B] on the device (clamped to [0, Lmax]); out fp32 [B][Lmax],
 * out[b][i] = s(ids[b][i] | ids[b][<i]) for i < lens[b], 0 after; an id outside [0, lm_vocab) gives NaN at its place and matches
 * nothing as context.  One thread per token.
 * av_ctc_beam_search_lm: the arguments and outputs of av_ctc_beam_search, and: an entry also carries g = sum over its tokens of
 * (lm_weight * s(token | tokens before it) + token_bonus), each operation rounded to fp32 on its own; entries are ranked by
 * (p_b (+) p_nb) + g, which is out_score; out_lm_score fp32 [B][nbest] = g (0 where out_len is -1).  Per frame an entry is extended by
 * the min(tokens, V - 1) best non-blank acoustic tokens (1 <= tokens <= 65) and by every token that leads to a live prefix.
 * lm_vocab must equal V.  workspace: av_ctc_beam_lm_workspace_bytes(B, T, V, beam_width, tokens) bytes, 8-byte aligned. */
int av_ngram_score(const int* ids, const long long* lens, float* out, int B, int Lmax, const float* lm_unigrams, const void* lm_table,
                   long long lm_slots, int lm_order, int lm_vocab, int lm_bos, int lm_probe_bound, void* stream);
int av_ctc_beam_lm_workspace_bytes(int B, int T, int V, int beam_width, int tokens, long long* bytes);
int av_ctc_beam_search_lm(const float* log_probs, long long stride_b, long long stride_t, const long long* lengths, int* out_ids,
                          int* out_len, float* out_score, float* out_lm_score, void* workspace, long long workspace_bytes, int B, int T,
                          int V, int blank, int beam_width, int nbest, int tokens, const float* lm_unigrams, const void* lm_table,
                          long long lm_slots, int lm_order, int lm_vocab, int lm_bos, int lm_probe_bound, float lm_weight,
                          float token_bonus, void* stream);
/* Contextual phrase biasing (bias.py: ContextBias; csrc/context_bias.h, csrc/context_bias.hip; the biased search is the third
 * instantiation of the search kernel of csrc/ctc_beam.hip).
 * Law: P = a set of distinct phrases of 1..32 token ids in [0, V), none the blank.  The state of a prefix is (k, tail), (0, ()) for the
 * empty one; per token c: tail <- the longest suffix of tail + (c) that is a prefix of some phrase (possibly empty); if tail is in P,
 * k <- k + |tail| and tail <- ().  m = k + |tail| (k banked, |tail| refundable).
 * Tables: the trie of P, node 0 = root.  bias_nodes int32 [bias_node_count][2] = (failure link = the deepest node that spells a proper
 * suffix of the node's path, depth | terminal << 16), 8-byte aligned; bias_edges = bias_slots 16-byte slots {u64 key, i32 child, i32 0},
 * 16-byte aligned, bias_slots a power of two, key 0 = empty, key = (node << 16) | (token + 1), linear probing from
 * splitmix64(key) & (bias_slots - 1), every stored key within bias_probe_bound probes (lookups make no more, at masked indices).
 * 2 <= V <= 65533.  Node indices read from the tables are clamped to [0, bias_node_count): a corrupt table gives wrong counts only.
 * av_context_bias_count: ids int32 [B][Lmax], lens optional int64 [B] on the device (clamped to [0, Lmax]); out int32 [B][Lmax][2],
 * 8-byte aligned, = (k, |tail|) after each token, 0 past the length; an id outside [0, V) or equal to the blank matches nothing and
 * resets the tail.  One thread per sequence.
 * av_ctc_beam_search_bias: the arguments and outputs of av_ctc_beam_search_lm; the language model is optional (lm_unigrams = lm_table
 * = NULL and lm_order = 0: none, no lookups, g_lm = +0, the other lm_ arguments are ignored).  An entry also carries (node, k);
 * g = g_lm (+) (bias_weight (x) float(m)), one multiply and one add rounded to fp32 each, g_lm = the g of av_ctc_beam_search_lm, and
 * entries are ranked by (p_b (+) p_nb) + g during the search.  Token pruning is av_ctc_beam_search_lm's: biasing re-ranks the
 * min(tokens, V - 1) best acoustic tokens and the live extensions, it injects no token.  After the last consumed frame
 * g_fin = g_lm (+) (bias_weight (x) float(k)) and the surviving entries are ranked again by (p_b (+) p_nb) + g_fin (descending, ties
 * to the earlier rank); that is out_score, out_lm_score = g_lm, out_bias_count int32 [B][nbest] = k (0 where out_len is -1).
 * bias_weight: fp32, finite, nats per matched token, may be negative.  workspace: av_ctc_beam_lm_workspace_bytes(B, T, V, beam_width,
 * tokens) bytes, 8-byte aligned. */
int av_context_bias_count(const int* ids, const long long* lens, int* out, int B, int Lmax, int V, int blank, const void* bias_nodes,
                          const void* bias_edges, int bias_node_count, long long bias_slots, int bias_probe_bound, void* stream);
int av_ctc_beam_search_bias(const float* log_probs, long long stride_b, long long stride_t, const long long* lengths, int* out_ids,
                            int* out_len, float* out_score, float* out_lm_score, int* out_bias_count, void* workspace,
                            long long workspace_bytes, int B, int T, int V, int blank, int beam_width, int nbest, int tokens,
                            const float* lm_unigrams, const void* lm_table, long long lm_slots, int lm_order, int lm_vocab, int lm_bos,
                            int lm_probe_bound, float lm_weight, float token_bonus, const void* bias_nodes, const void* bias_edges,
                            int bias_node_count, long long bias_slots, int bias_probe_bound, float bias_weight, void* stream);
/* CTC loss on the device, opt-in replacement of nn.CTCLoss(blank, zero_infinity=True) (model/trainer.py:25,116-117): the semantics of
 * torch.nn.functional.ctc_loss(..., reduction="none") with padded 2-D targets.  log_probs fp32, element [b][t][v] at
 * b * stride_b + t * stride_t + v (element strides: [B][T][V] and the [T][B][V] view are both taken without a copy); targets int64
 * [B][target_ld]; input_lengths / target_lengths int64 [B].  Labels and lengths are read from DEVICE memory (no host copy, no
 * synchronisation); T_b is clamped to [0, T], L_b to [0, Lmax = (S_max - 1) / 2], an item with a label outside [0, V) is infeasible.
 * av_ctc_loss_fwd: nll fp32 [B] (+inf for an infeasible item, 0 with zero_infinity); log_alpha / log_beta = workspaces fp32
 * [B][T][S_max] for the gradient (log_beta NULL: loss only, log_alpha may then be NULL too).
 * av_ctc_loss_bwd: grad fp32 [B][T][V] contiguous = grad_nll[b] * (exp(log_probs) - occupancy) for t < T_b (torch's form: rows sum to
 * zero), exactly 0 for t >= T_b and for every frame of an infeasible item; nll / log_alpha / log_beta as written by the forward.
 * Deterministic: no floating-point atomics (bit-identical results for identical inputs). */
int av_ctc_loss_fwd(const float* log_probs, long long stride_b, long long stride_t, const long long* targets, long long target_ld,
                    const long long* input_lengths, const long long* target_lengths, int B, int T, int V, int S_max, int blank,
                    int zero_infinity, float* nll, float* log_alpha, float* log_beta, void* stream);
int av_ctc_loss_bwd(const float* log_probs, long long stride_b, long long stride_t, const long long* targets, long long target_ld,
                    const long long* input_lengths, const long long* target_lengths, int B, int T, int V, int S_max, int blank,
                    const float* nll, const float* log_alpha, const float* log_beta, const float* grad_nll, float* grad, void* stream);
/* N-best form of the CTC loss, for minimum word error rate training (mwer.py): the negative log-likelihood and the gradient of N label
 * sequences per utterance against ONE shared [T][V] block of log-probs, which is read once and whose gradient is written once.
 * log_probs and the strides are as for av_ctc_loss_fwd; hyp_ids int32, element [b][n][i] at b * hyp_ld_b + n * hyp_ld_n + i (the out_ids
 * block of av_ctc_beam_search is taken as it is), hyp_lens int64 [B][N] (as for av_error_counts), input_lengths int64 [B]: one T_b per
 * utterance, shared by its N hypotheses, clamped to [0, T].  Lmax = (S_max - 1) / 2.  Everything is read from DEVICE memory.
 * A present hypothesis is exactly an item of av_ctc_loss_fwd with zero_infinity = 0 (the same kernel: bit-identical nll).  An item is OUT
 * when hyp_lens < 0 (absent), hyp_lens > Lmax (NOT clamped: a cut hypothesis is a different hypothesis), an id is outside [0, V) or no
 * path exists; ids at or past a length are never read.
 * av_ctc_nbest_fwd: nll fp32 [B][N], +inf for an out item; log_alpha / log_beta = workspaces fp32 [B][N][T][S_max] for the gradient
 * (log_beta NULL: values only, log_alpha may then be NULL too).
 * av_ctc_nbest_bwd: grad fp32 [B][T][V] contiguous = G_b exp(log_probs) - sum_n grad_nll[b][n] occupancy_{b,n} for t < T_b, the sum over
 * the items that are not out in ascending n and G_b = sum_n grad_nll[b][n] in the same order; exactly 0 for t >= T_b and for every row
 * of an utterance whose items are all out; every element is written.  grad_nll of an out item is never read into any sum (an inf or
 * NaN there cannot reach grad).
 * Limits: 1 <= N <= 64, 1 <= B <= 65535 (the gradient's grid y; the lattice launches 2 B N workgroups), T, V >= 1, 0 <= blank < V, S_max
 * odd, hyp_ld_n >= Lmax, hyp_ld_b >= (N - 1) hyp_ld_n + Lmax; LDS: that of av_ctc_loss_fwd for the forward, W (V + S_max) floats plus
 * 3 N Lmax + 3 N ints for the gradient (W = 4, 2 or 1 wavefronts), both within 64 KiB - otherwise an error status.
 * Deterministic: no floating-point atomics (bit-identical results for identical inputs). */
int av_ctc_nbest_fwd(const float* log_probs, long long stride_b, long long stride_t, const int* hyp_ids, long long hyp_ld_b,
                     long long hyp_ld_n, const long long* hyp_lens, const long long* input_lengths, int B, int N, int T, int V, int S_max,
                     int blank, float* nll, float* log_alpha, float* log_beta, void* stream);
int av_ctc_nbest_bwd(const float* log_probs, long long stride_b, long long stride_t, const int* hyp_ids, long long hyp_ld_b,
                     long long hyp_ld_n, const long long* hyp_lens, const long long* input_lengths, int B, int N, int T, int V, int S_max,
                     int blank, const float* nll, const float* log_alpha, const float* log_beta, const float* grad_nll, float* grad,
                     void* stream);
/* CTC forced alignment on the device: the best frame path (Viterbi) of each transcript through the CTC lattice of the log-probs and
 * lengths the trainer hands to its loss and decoder (model/trainer.py:116-117, 229-242), for word timestamps and alignment scores.
 * log_probs, strides, targets, target_ld, lengths, the clamping of T_b / L_b and odd S_max = 2 Lmax + 1 are as for av_ctc_loss_fwd
 * ([B][T][V] and the [T][B][V] view are both taken without a copy; labels and lengths are read from DEVICE memory, no synchronisation);
 * 1 <= T <= 4096.  The law (csrc/ctc_align.hip): d[t][s] = max(d[t-1][s], d[t-1][s-1], skip ? d[t-1][s-2] : -inf) + lp[t][l'_s] in
 * fp32, ties to the smaller move, final state S-1 only if strictly better than S-2.  An item is infeasible if a label is outside
 * [0, V) or EQUAL TO THE BLANK (the loss accepts that; its path could not collapse to the target) or if its final score is -inf.
 * out_state int32 [B][T]: extended-state index per frame, -1 for t >= T_b and for every frame of an infeasible item;
 * out_span int32 [B][Lmax][2]: first frame and end frame (exclusive) of target position j (the frames of state 2j+1: contiguous and
 *   non-empty), -1, -1 for j >= L_b and for infeasible items;  out_token_score fp32 [B][Lmax]: sum of lp[t][l_j] over the span, added in
 *   frame order, 0 where the span is -1 (both may be NULL when Lmax = 0);
 * out_score fp32 [B]: the path's log-probability, -inf if infeasible (T_b = 0 with L_b = 0: 0 and an empty path).
 * workspace: av_ctc_align_workspace_bytes(B, T, S_max) bytes (two bits per frame and state), 4-byte aligned; a smaller one is an error
 * status.  LDS: that of av_ctc_loss_fwd plus 2 T bytes for the path, same 64 KiB limit.  Deterministic: no atomics. */
int av_ctc_align_workspace_bytes(int B, int T, int S_max, long long* bytes);
int av_ctc_align(const float* log_probs, long long stride_b, long long stride_t, const long long* targets, long long target_ld,
                 const long long* input_lengths, const long long* target_lengths, int B, int T, int V, int S_max, int blank,
                 int* out_state, int* out_span, float* out_token_score, float* out_score, void* workspace, long long workspace_bytes,
                 void* stream);
/* CTC confidences on the device (csrc/ctc_confidence.hip; the entropy-based frame confidence of Laptev & Ginsburg 2022 and its
 * aggregation over a token's frames): fp32, no atomics, no synchronisation, lengths read from DEVICE memory (NULL: T), clamped to [0, T].
 * Frame law for a row x[0..V), m = max x, d = x - m, e = exp(d), s = sum e (it renormalises):
 *   AV_CONF_MAX_PROB  c = (V / s - 1) / (V - 1)
 *   AV_CONF_ENTROPY   c = 1 + (sum_{e > 0} e d / s - ln s) / ln V
 *   AV_CONF_TSALLIS   c = (sum exp(alpha d) / exp(alpha ln s) - u) / (1 - u), u = exp((1 - alpha) ln V); alpha finite, > 0, |alpha - 1| >= 1/64
 * result c >= 0 ? min(c, 1) : 0; a NaN entry, a row without a finite maximum and every frame t >= T_b give 0.
 * av_ctc_frame_conf: log_probs and strides as for av_ctc_align, V >= 2, 1 <= T <= 4096 -> conf fp32 [B][T].
 * av_ctc_span_conf: conf fp32 [B][T], spans int32 [B][L][2] (first frame, end exclusive; clipped to [0, T_b)) -> token_conf fp32 [B][L]:
 *   AV_AGG_MEAN the fp32 sum in frame order divided once by the count, AV_AGG_MIN the minimum, AV_AGG_PROD the fp32 product in frame
 *   order; 0 for a span of -1 and for one that is empty after clipping.  L = 0: nothing is launched.
 * av_ctc_greedy_timed: ONE read of log_probs for av_ctc_greedy's out_ids / out_len, the run of equal argmax frames behind every emitted
 *   id (out_span int32 [B][T][2], -1 padded: the spans av_ctc_align finds for these ids), av_ctc_span_conf over those runs (token_conf
 *   fp32 [B][T], 0 padded) and av_ctc_frame_conf (frame_conf fp32 [B][T]); the two agree with the separate calls bit for bit. */
#define AV_CONF_MAX_PROB 0
#define AV_CONF_ENTROPY 1
#define AV_CONF_TSALLIS 2
#define AV_AGG_MEAN 0
#define AV_AGG_MIN 1
#define AV_AGG_PROD 2
int av_ctc_frame_conf(const float* log_probs, long long stride_b, long long stride_t, const long long* lengths, int B, int T, int V,
                      int method, float alpha, float* conf, void* stream);
int av_ctc_span_conf(const float* conf, const int* spans, const long long* lengths, int B, int T, int L, int aggregation,
                     float* token_conf, void* stream);
int av_ctc_greedy_timed(const float* log_probs, long long stride_b, long long stride_t, const long long* lengths, int B, int T, int V,
                        int blank, int method, float alpha, int aggregation, int* out_ids, int* out_len, int* out_span,
                        float* token_conf, float* frame_conf, void* stream);
/* Long-form transcription on the device (csrc/ctc_longform.hip; longform.py holds the window plan and restates the three laws in float32
 * numpy): fp32, no atomics, no synchronisation, every output element written, cuts and lengths stay in DEVICE memory.
 * S is the speaker axis; rows are addressed as base + s * stride_s + row * stride_r (floats), stride_r >= V, rows contiguous.
 * av_ctc_stitch: windows = the R = nw * W rows of every speaker's window log-probs; src_row int32 [F][4] and src_weight fp32 [F][4]: per
 *   output frame its 1 .. 4 source rows in ascending window order (-1 = none, packed in front) and their normalised weights -> out fp32
 *   [S][F][V].  One source: the row copied bit for bit.  n > 1 sources, per class: M = max_k x_k, out = M + log(sum_k wn_k exp(x_k - M))
 *   in source order; M = -inf gives -inf, a NaN source gives NaN.  (The "centre" policy is a table with one source per frame.)  A frame
 *   without a source is filled with -inf.
 * av_ctc_cut_points: log_probs [S][F][V], N = segment - 2 radius >= 2 radius + 1, segment <= 408; nb = number of j >= 1 with
 *   j N + radius < F -> cuts int32 [S][nb + 2]: cuts[0] = 0, cuts[nb + 1] = F, cuts[j] = the frame t of [j N - radius, j N + radius]
 *   intersected with [1, F - 1] with the largest log_probs[t][blank] (fp32 compare, a NaN ranks as -inf, ties go to the smallest t).
 * av_ctc_segment_gather: cuts as above (clamped to [0, F] and made monotone, a segment cut at `segment` frames) -> seg_log_probs fp32
 *   [S * (nb + 1)][segment][V]: row i of segment j is log_probs[cuts[j] + i] for i < cuts[j + 1] - cuts[j] and 0.0 after it;
 *   seg_lengths int64 [S * (nb + 1)]: the lengths the other CTC entries of this header read from device memory. */
#define AV_LONGFORM_MAX_SOURCES 4
#define AV_LONGFORM_MAX_SEGMENT 408
int av_ctc_stitch(const float* windows, long long stride_s, long long stride_r, const int* src_row, const float* src_weight, int S, int R,
                  int F, int V, float* out, void* stream);
int av_ctc_cut_points(const float* log_probs, long long stride_s, long long stride_t, int S, int F, int V, int blank, int segment, int radius,
                      int* cuts, void* stream);
int av_ctc_segment_gather(const float* log_probs, long long stride_s, long long stride_t, const int* cuts, int S, int F, int V, int nb,
                          int segment, float* seg_log_probs, long long* seg_lengths, void* stream);
/* CTC keyword spotting on the device (csrc/ctc_spot.hip; spot.py restates the law in float32 numpy, bit for bit): was this
 * phrase said, where, and how sure - K keywords against every utterance of one block of log-probs.  fp32, no atomics, no synchronisation.
 * log_probs and strides as for av_ctc_align ([B][T][V] and the [T][B][V] view are both taken without a copy); input_lengths int64 [B] in
 * DEVICE memory or NULL (= T), clamped to [0, T]; there is no limit on T other than memory.  keywords int32 [K][kw_ld] and kw_lengths
 * int32 [K] in DEVICE memory: keyword k is its first L_k = kw_lengths[k] clamped to [0, L_max] ids; it is INVALID - no hits - if
 * L_k < 1, if an id is outside [0, V) or if an id equals the blank.  1 <= L_max <= 32 (one lattice state per lane), kw_ld >= L_max.
 * The law: m[t] = max_v lp[t][v] (a NaN never wins), c[t][v] = lp[t][v] - m[t] (every cost of a frame whose m is not finite is -inf).
 * Lattice of S = 2 L - 1 states y_1, blank, y_2, ..., blank, y_L; the skip s-2 -> s exists for even s >= 2 with y differing from the
 * label two states back.  Each cell carries (d, start), (-inf, -1) before frame 0; at frame t state s takes d[t-1][s], then
 * d[t-1][s-1] if strictly greater, then the skip predecessor if it exists and is strictly greater, and state 0 alone a fresh start
 * (0, t) if 0 is strictly greater; d[t][s] = best + c[t][label_s].  e[t] = d[t][S-1], es[t] = start[t][S-1].  Hits: among the frames
 * t < T_b with e[t] > -inf and e[t] >= min_score, up to N times the greatest e[t] (ties: the greater t) is reported as
 * (es[t], t + 1, e[t]) and every frame u whose interval [es[u], u + 1) overlaps it is dropped.  A score is the log-likelihood ratio of
 * the path against the best unconstrained path over the same frames: <= 0, and 0.0 exactly on an argmax path.
 * out_hits int32 [B][K][N][2] (first frame, end frame exclusive; -1 padded), out_scores fp32 [B][K][N] (descending; -inf padded),
 * out_counts int32 [B][K].  1 <= N <= 8; min_score may be -inf, not NaN.
 * workspace: av_ctc_spot_workspace_bytes(B, T, K) = 4 B T (1 + 2 K) bytes (m [B][T], then e fp32 and es int32 [B][K][T]), 4-byte
 * aligned; a smaller one is an error status. */
int av_ctc_spot_workspace_bytes(int B, int T, int K, long long* bytes);
int av_ctc_spot(const float* log_probs, long long stride_b, long long stride_t, const long long* input_lengths, const int* keywords,
                long long kw_ld, const int* kw_lengths, int B, int T, int V, int K, int L_max, int blank, int N, float min_score,
                int* out_hits, float* out_scores, int* out_counts, void* workspace, long long workspace_bytes, void* stream);
/* CTC segmentation on the device (csrc/ctc_segment.hip; segmentation.py holds the law in full and restates it in float32 numpy, bit for
 * bit): a known transcript laid over a recording of any length - av_ctc_align without its limits, with ends that may float, a
 * score per frame and a confidence per utterance.  fp32, no atomics, no synchronisation.  log_probs, strides, targets, target_ld and the
 * two length arrays as for av_ctc_align; there is no limit on T other than memory, S_max = 2 Lmax + 1 <= 16383 (Lmax 8191), V <= 12000
 * (whole rows of log-probs are staged in LDS).  free_ends: bit 0 = the path may start at any frame, bit 1 = it may end at any frame;
 * with free_ends = 0 out_state, out_span, out_token_score and out_score are bit for bit av_ctc_align's, otherwise emissions are
 * lp[t][c] - max_v lp[t][v] and the score is a log-likelihood ratio against the best unconstrained path over the same frames.
 * utterances int32 [B][U][2] in DEVICE memory: token ranges [begin, end) into the target, used only if 0 <= begin < end <= L_b; U may
 * be 0 (then utterances and the three out_utt_* may be NULL).  score_window >= 1: frames per window of out_utt_score.
 * out_state int32 [B][T] (-1 off the path), out_span int32 [B][Lmax][2], out_token_score fp32 [B][Lmax], out_score fp32 [B] (-inf:
 * infeasible), out_frame_score fp32 [B][T] (the path's emission per frame, 0 off the path), out_utt_span int32 [B][U][2] (first frame
 * of token begin, end frame of token end-1; -1, -1 where there is none), out_utt_mean fp32 [B][U] (mean frame score over the span),
 * out_utt_score fp32 [B][U] (the least mean over its consecutive windows of score_window frames).
 * workspace: av_ctc_segment_workspace_bytes(B, T, S_max) = 4 B ceil(T / 16) S_max bytes (2 bits per frame and state), 4-byte aligned; a
 * smaller one is an error status. */
int av_ctc_segment_workspace_bytes(int B, int T, int S_max, long long* bytes);
int av_ctc_segment(const float* log_probs, long long stride_b, long long stride_t, const long long* targets, long long target_ld,
                   const long long* input_lengths, const long long* target_lengths, const int* utterances, int B, int T, int V, int S_max,
                   int U, int blank, int free_ends, int score_window, int* out_state, int* out_span, float* out_token_score,
                   float* out_score, float* out_frame_score, int* out_utt_span, float* out_utt_mean, float* out_utt_score, void* workspace,
                   long long workspace_bytes, void* stream);
/* Word, character and token error counts on the device: edit distance with operation counts between ONE reference and N hypotheses per
 * utterance, from token ids through a device copy of the tokenizer's piece table - what MultimodalTrainer.evaluate() measures
 * (word_error_rate of model/trainer.py, the jiwer.wer stand-in), plus the character and token levels and the S / D / I breakdown.
 * ref_ids int32 [B][ref_ld] (Lr used), ref_lens int64 [B]; hyp_ids int32, element [b][n][i] at b * hyp_ld_b + n * hyp_ld_n + i (Lh used:
 * the out_ids block of av_ctc_beam_search is taken as it is), hyp_lens int64 [B][N], < 0 = absent hypothesis (that kernel's out_len).
 * Ids and lengths are read from DEVICE memory (no host copy, no synchronisation); lengths are clamped to [0, L]; ids at or past a
 * sequence's length are never read.  0 <= Lr, Lh <= 4096 (ids may be NULL where L = 0).
 * Text of a sequence (csrc/error_counts.hip): ids outside [0, V) and ids equal to the sequence's skip id (ref_skip_id / hyp_skip_id; < 0:
 * none) are dropped; the code points of the remaining pieces - piece i = piece_chars[piece_offsets[i] .. piece_offsets[i + 1]), offsets
 * int32 [V + 1] non-decreasing, at most max_piece code points per piece (longer ones are cut there) - are concatenated, U+2581 read as
 * U+0020, and leading / trailing U+0020 stripped.  Level 0 (token): the kept ids.  Level 1 (character): the stripped text, inner spaces
 * included.  Level 2 (word): maximal runs of non-space code points, equal when their code points are equal (a hash filters, the content
 * decides).  piece_offsets = piece_chars = NULL: levels 1 and 2 are -1, V and max_piece are ignored and the ids are compared as given
 * (only the skip id is dropped): the entry for callers that bring their own symbols.
 * Counts of a pair: among all alignments (match, substitution, deletion of a reference symbol, insertion of a hypothesis symbol) the
 * lexicographically smallest (S + D + I, S, D) - minimum edits, then fewest substitutions, then fewest deletions: a property of the pair.
 * out_counts int32 [B][N][3][4]: level x (S, D, I, R = reference length at that level); hits = R - S - D, hypothesis length = R - D + I.
 * All four are -1 at every level of an absent hypothesis, and at levels 1 and 2 of a pair one of whose texts exceeds 4096 code points
 * before the strip (its level 0 is still computed).  Every element is written.
 * workspace: av_error_counts_workspace_bytes(B, N, Lr, Lh, max_piece) bytes (max_piece = 0: no table), 16-byte aligned; a smaller one is
 * an error status.  Two launches (expansion: one workgroup per sequence; distance: one wave per pair and level, at most 48 KiB of LDS).
 * Deterministic: no atomics, integers only. */
int av_error_counts_workspace_bytes(int B, int N, int Lr, int Lh, int max_piece, long long* bytes);
int av_error_counts(const int* ref_ids, long long ref_ld, const long long* ref_lens, const int* hyp_ids, long long hyp_ld_b,
                    long long hyp_ld_n, const long long* hyp_lens, int B, int N, int Lr, int Lh, int ref_skip_id, int hyp_skip_id,
                    const int* piece_offsets, const int* piece_chars, int V, int max_piece, int* out_counts, void* workspace,
                    long long workspace_bytes, void* stream);
/* Training-time augmentation on the device (csrc/augment.hip; augment.py restates both laws on the host bit for bit).
 * Every random choice is a draw of the dropout generator (drop_draw of csrc/av_common.h), a pure function of (seed, stream, block): a
 * block yields four 16-bit integers k0..k3, an integer in 0..R-1 is (k * R) >> 16.  Clip b at step `step` has the counter
 * c = step * 65536 + b (b < 65536, 0 <= step < 2^24).  Nothing synchronises, nothing is drawn on the host.
 * av_augment_lips: src, dst fp32 [B][T][H][W] (the [B][1][T][H][W] view of the trainer is the same bytes), out of place (src == dst or an
 *   overlap is an error status); lengths int64 [B] on the device or NULL (= T), clamped to [0, T].
 *     dst[b][t][y][x] = src[b][tsrc(t)][clamp(y - dy, 0, H-1)][clamp((flip ? W-1-x : x) - dx, 0, W-1)],  0 for t >= lengths[b] (not read)
 *   block c * 64 + 0 of stream_id: dx = draw(k0, 2 S + 1) - S, dy = draw(k1, 2 S + 1) - S with S = max_shift < min(H, W),
 *     flip = k2 < flip_thr (flip_thr = ceil(65536 p) in [0, 65536]).
 *   frame freeze (dropped video frames): segment j = 0 .. ceil(n / E) - 1 of the n valid frames (E = mask_every >= 1) takes k[2 (j % 2)] and
 *     k[2 (j % 2) + 1] of block c * 64 + 1 + j / 2: s_j = draw(., E), w_j = draw(., mask_max + 1), span_j = [j E + s_j, min(j E + s_j + w_j, n)).
 *     0 <= mask_max <= E and ceil(T / E) <= 126, so a frame lies at most in its own segment's span and the previous one's; inside a span
 *     it reads input frame max(start - 1, 0) (the own segment's span wins), every other frame reads itself; freezes do not chain.
 *   Nothing is computed in floating point.  max_shift = flip_thr = mask_max = 0 is a copy.
 * av_augment_noise: x, y fp32 [B][N] (N <= 2^24; y may be x), lengths int64 [B] = valid samples (required), clamped to [0, N].
 *   P_b = mean of x^2 over the valid samples, in double, fixed order, no atomics (the same bits on every run);
 *   snr_b = fl(snr_lo + fl(u fl(snr_hi - snr_lo))) in fp32, u = k0 / 65536 of block c of AV_AUG_STREAM_SNR;
 *   sigma_b = (float)sqrt(P_b 10^(-snr_b / 10)) in double -> sigma_out[b];  0 for P_b = 0 or no valid sample: that row is copied.
 *   y[b][i] = fl(x + fl(sigma_b z_i)) for i < lengths[b], x beyond;  z_i = (float)(k0 + k1 + k2 + k3 - 131070) * fp32(1 / sqrt((65536^2 - 1) / 3))
 *   from block (c << 24) + i of AV_AUG_STREAM_NOISE: zero mean, unit variance, |z| <= 3.47, exact in integers.
 *   power_ws: B * (1 + ceil(N / AV_AUG_NOISE_CHUNK)) doubles (at least 2 B), 8-byte aligned; P_b is left in power_ws[b]. */
#define AV_AUG_STREAM_LIP1 0xF0000011u
#define AV_AUG_STREAM_LIP2 0xF0000012u
#define AV_AUG_STREAM_SNR 0xF0000013u
#define AV_AUG_STREAM_NOISE 0xF0000014u
#define AV_AUG_NOISE_CHUNK 8192
int av_augment_lips(const float* src, float* dst, const long long* lengths, int B, int T, int H, int W, unsigned long long seed,
                    long long step, unsigned stream_id, int max_shift, int flip_thr, int mask_max, int mask_every, void* stream);
int av_augment_noise(const float* x, float* y, const long long* lengths, int B, int N, unsigned long long seed, long long step,
                     float snr_lo, float snr_hi, double* power_ws, float* sigma_out, void* stream);
/* device side of the input pipeline (dataset/multi_speaker_dataset.py:13-59; decoding wav / npy files stays on the host):
 * av_lip_gray_resize: src [T][Hs][Ws][C] (uint8 if src_is_u8 else fp32) -> dst fp32 [T][Hd][Wd] = bilinear(mean over C) / divisor
 *   (:49-58: .astype(float32).mean(-1), cv2.resize INTER_LINEAR law, / 255), float32 operation order of the reference;
 * av_mix_pair: mixed[i] = (a1[i] + a2[i]) / (max|a1 + a2| + 1e-6) over n = max(len1, len2) samples with zero padding (:21-32),
 *   mask1 / mask2 int64 [n]: 1 = both speakers, 2 = only this speaker, 0 = otherwise (:35-45); peak_ws: 4 bytes of workspace */
int av_lip_gray_resize(const void* src, int src_is_u8, float* dst, int T, int Hs, int Ws, int C, int Hd, int Wd, float divisor,
                       void* stream);
int av_mix_pair(const float* a1, long long len1, const float* a2, long long len2, float* mixed, long long* mask1, long long* mask2,
                unsigned* peak_ws, void* stream);
int av_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                 int step, float grad_scale, void* stream);
/* multi-tensor form (every optimizer step of the trainer): ptrs [n_tensors][5] device pointers {param, grad, exp_avg, exp_avg_sq,
 * shadow}; shadow = optional (0 = none) bf16 copy of the updated parameter, same element order (the perf path's cached compute-dtype
 * weight); hyper [n_tensors][4] floats {lr, beta1, beta2, eps} (torch.optim.Adam param-group values, model/trainer.py:34-39); chunk c =
 * elements [chunk_start[c], +chunk_elems) of tensor chunk_tensor[c]; steps = device int32 table of PER-TENSOR step counts
 * (torch.optim.Adam's state[p]['step']: a parameter without a gradient in some step - LayerDrop - falls behind the others), tensor t
 * owns steps[step_slot[t]]: read for the bias corrections, incremented by a trailing one-block launch.  All arrays live on the device.
 * scaler_state != NULL = the same step under loss scaling (replaces torch.amp.GradScaler.step + .update, model/trainer.py:40,121-123
 * of the reference; torch/amp/grad_scaler.py:126-129 defaults): 5 device floats {scale, 1/scale, found_inf, growth tracker, steps
 * taken}; non-finite check over every gradient -> Adam with grad * grad_scale / scale, skipped (no counter advances) when found_inf
 * -> scale update (x backoff on overflow, x growth after growth_interval clean steps).  No host synchronisation in either form */
int av_adam_multi(const void* ptrs, const long long* sizes, const float* hyper, const int* chunk_tensor, const long long* chunk_start,
                  int n_chunks, int chunk_elems, int* steps, const int* step_slot, int n_tensors, float grad_scale,
                  float* scaler_state, float growth, float backoff, int growth_interval, void* stream);
/* av_adam_multi with global-norm gradient clipping and a linear warmup / decay schedule of the learning rate, both decided on the device
 * (csrc/optim.hip; optim.AvAdam).  The arguments of av_adam_multi, and:
 * max_norm > 0: clip.  One more pass reads the gradients (sum of squares per chunk in double, no atomics: the same bits on every run),
 *   one workgroup adds the chunk sums in a fixed order, and the Adam kernel multiplies grad * grad_scale (/ scale) by
 *   min(1, max_norm / (norm + 1e-6)), the law of torch.nn.utils.clip_grad_norm_ with error_if_nonfinite=False (a NaN norm gives a NaN
 *   coefficient, an infinite one 0).  Under loss scaling that pass also is the non-finite check.  0: no clipping, no such pass.
 * warmup_steps, total_steps: optimizer step k (0-based, skipped steps not counted) runs at lr * k / warmup_steps while k < warmup_steps,
 *   then at lr * max(0, (total_steps - k) / (total_steps - warmup_steps)); total_steps == 0: lr after the warmup; both 0: no schedule.
 *   total_steps must be 0 or above warmup_steps.  One multiplier for all tensors; hyper keeps the per-tensor lr.
 * clip_state: 4 device words, 4-byte aligned, needed when either is on: float norm of the gradients as Adam sees them, float clip
 *   coefficient (1 without clipping), float learning-rate multiplier of this step, int32 k (the caller zeroes or restores it; the launch
 *   advances it when a schedule is on and the step was not skipped).
 * workspace: av_grad_norm_workspace_bytes(n_chunks) bytes, 8-byte aligned, needed when clipping; a smaller one is an error status.
 * With max_norm, warmup_steps and total_steps all 0 this is av_adam_multi.  No host synchronisation. */
int av_grad_norm_workspace_bytes(int n_chunks, long long* bytes);
int av_adam_multi_ex(const void* ptrs, const long long* sizes, const float* hyper, const int* chunk_tensor, const long long* chunk_start,
                     int n_chunks, int chunk_elems, int* steps, const int* step_slot, int n_tensors, float grad_scale,
                     float* scaler_state, float growth, float backoff, int growth_interval, float max_norm, int warmup_steps,
                     int total_steps, void* workspace, long long workspace_bytes, float* clip_state, void* stream);
/* av_adam_multi_ex that also keeps an exponential moving average (EMA) of the weights, updated inside the same Adam launch while the new
 * parameter is still in a register (csrc/optim.hip; optim.AvAdam(ema_decay=...)).  The arguments of av_adam_multi_ex, and:
 * ema_ptrs: [n_tensors] device pointers, the fp32 average of tensor t of the launch (a table of its own: ptrs stays [n_tensors][5]).
 * ema_only_ptrs [n_only][2] device pointers {param, ema}, ema_only_sizes [n_only], ema_only_chunk_tensor / ema_only_chunk_start
 *   [n_ema_only_chunks] (chunks of chunk_elems, as above): tensors that have an average but no gradient in this step (LayerDrop); a light
 *   kernel moves their average towards the unchanged parameter.  n_ema_only_chunks == 0: none, the four tables may be NULL.
 * ema_decay in (0, 1), ema_warmup 0 / 1: update k (0-based, skipped steps not counted) runs at d_0 = 0 - the first update copies the
 *   parameters, torch.optim.swa_utils.AveragedModel's n_averaged == 0 - then d_k = ema_decay, or min(ema_decay, (1 + k) / (10 + k)) with
 *   ema_warmup (TensorFlow's ExponentialMovingAverage, timm's ModelEmaV2).  Per element, in fp32, after that element's Adam update:
 *   torch.lerp(ema, p_new, w) with w = 1 - d_k, i.e. ema += w * (p_new - ema) if w < 0.5, else ema = p_new - (p_new - ema) * (1 - w).
 * ema_state: 2 device words, 4-byte aligned: float d_k of this step (computed in double by one thread, read from here by every
 *   workgroup), int32 k (the caller zeroes or restores it; the launch advances it unless the step was skipped).
 * Under loss scaling a skipped step updates no average and leaves k.  No atomics: the same bits on every run.  ema_decay == 0 with no EMA
 * tables is av_adam_multi_ex; a decay outside [0, 1) or NaN, tables without a decay, a decay without ema_ptrs or ema_state are error
 * statuses.  No host synchronisation. */
int av_adam_multi_ema(const void* ptrs, const long long* sizes, const float* hyper, const int* chunk_tensor, const long long* chunk_start,
                      int n_chunks, int chunk_elems, int* steps, const int* step_slot, int n_tensors, float grad_scale,
                      float* scaler_state, float growth, float backoff, int growth_interval, float max_norm, int warmup_steps,
                      int total_steps, void* workspace, long long workspace_bytes, float* clip_state, const void* ema_ptrs,
                      const void* ema_only_ptrs, const long long* ema_only_sizes, const int* ema_only_chunk_tensor,
                      const long long* ema_only_chunk_start, int n_ema_only_chunks, float ema_decay, int ema_warmup, float* ema_state,
                      void* stream);
/* av_adam_multi_ema with decoupled weight decay (AdamW) and a choice of schedule (csrc/optim.hip; optim.AvAdam(weight_decay=...,
 * lr_schedule=...)).  The arguments of av_adam_multi_ema, and:
 * weight_decay: [n_tensors] device floats lambda_t >= 0, 4-byte aligned, or NULL for none.  In a step that is not skipped tensor t is
 *   multiplied by f_t = 1 - lr_t * m_k * lambda_t before its Adam update - torch.optim.AdamW's param.mul_(1 - lr * weight_decay) - with
 *   lr_t = hyper[t][0] and m_k this step's learning-rate multiplier from clip_state (1 without a schedule).  f_t is computed once per
 *   workgroup in double and stored as a float; p * f_t is rounded on its own, never contracted into the update.  The gradient and the
 *   moments do not see the decay; shadow and EMA are written from the decayed, updated value.  A skipped step decays nothing, nor does a
 *   warmup step at multiplier 0; a tensor that is not in the launch (no gradient) is not decayed; the clip coefficient scales the
 *   gradient only.
 * lr_schedule: 0 = the linear law of av_adam_multi_ex; 1 = cosine: k / warmup_steps while k < warmup_steps, then
 *   max(0, 0.5 * (1 + cos(pi * (k - warmup_steps) / (total_steps - warmup_steps)))) - HF get_cosine_schedule_with_warmup with num_cycles = 0.5
 *   - and 0 for k >= total_steps (HF's lambda rises again there), in double by the thread that computes the linear law.  Cosine needs
 *   total_steps > warmup_steps and therefore clip_state.
 * A misaligned table, an lr_schedule outside {0, 1}, cosine without total_steps or without clip_state are error statuses.  With
 * weight_decay == NULL and lr_schedule == 0 this is av_adam_multi_ema: the same kernels are launched.  No host synchronisation. */
int av_adam_multi_wd(const void* ptrs, const long long* sizes, const float* hyper, const int* chunk_tensor, const long long* chunk_start,
                     int n_chunks, int chunk_elems, int* steps, const int* step_slot, int n_tensors, float grad_scale,
                     float* scaler_state, float growth, float backoff, int growth_interval, float max_norm, int warmup_steps,
                     int total_steps, void* workspace, long long workspace_bytes, float* clip_state, const void* ema_ptrs,
                     const void* ema_only_ptrs, const long long* ema_only_sizes, const int* ema_only_chunk_tensor,
                     const long long* ema_only_chunk_start, int n_ema_only_chunks, float ema_decay, int ema_warmup, float* ema_state,
                     const float* weight_decay, int lr_schedule, void* stream);
/* one multi-tensor launch that exchanges parameters and their averages: ptrs [n_tensors][3] device pointers {param, ema, shadow}, sizes
 * [n_tensors], chunk tables as av_adam_multi.  param and ema (fp32) change places element by element, without a temporary copy; where
 * shadow != 0 the new parameter's 16-bit image (bf16 in libavhip.so, half in libavhip_f16.so) is written there, as the Adam kernel does.
 * Calling it twice restores every bit. */
int av_param_swap_multi(const void* ptrs, const long long* sizes, const int* chunk_tensor, const long long* chunk_start, int n_chunks,
                        int chunk_elems, void* stream);
/* one multi-tensor launch that folds the gradients of a micro-batch into their accumulators (optim.AvAdam.accumulate): ptrs [n_tensors][2]
 * device pointers {grad, acc}, both fp32; grad and acc of a tensor may not overlap.  mode [n_tensors] device ints: 0 = acc := grad, the
 * tensor's first contribution of a cycle (no clearing pass, no read of acc, the gradient's own bits: autograd's first .grad is the gradient,
 * not 0 + g); 1 = acc := acc + grad, one fp32 add per element.  sizes [n_tensors], chunk tables as av_adam_multi: one 256-thread workgroup
 * per chunk, 16-byte accesses where both pointers are 16-byte aligned and the span starts on a multiple of 4, element by element otherwise.
 * No LDS, no atomics: the same bits whatever the grid.  Non-finite values propagate by IEEE arithmetic; nothing is checked.  NULL tables,
 * n_chunks < 0 or chunk_elems <= 0 are an error status ("av_grad_accum_multi: bad args"); n_chunks == 0 returns AV_OK without a launch.
 * No host synchronisation. */
int av_grad_accum_multi(const void* ptrs, const int* mode, const long long* sizes, const int* chunk_tensor, const long long* chunk_start,
                        int n_chunks, int chunk_elems, void* stream);

/* ---- legacy mel + GRU model (reference: "이전 버전/multimodal_ctc_korean.py":8-55, train loop
 * "이전 버전/train_ctc_korea.py":82-109).  Its convolutions (nn.Conv2d 3x3, :12,15) and all input / weight-gradient products run on
 * av_gemm; these entry points are the rest of it:
 * av_nchw_to_nhwc:      frames [N][C][H][W] fp32 (the (B*T, C, H, W) view of :23) -> [N][H][W][Cp] channel-last, zero padded to Cp
 * av_relu_maxpool2_fwd: y = MaxPool2d(2)(ReLU(x)) (:13-14,16-17), x [N][H][W][C]; y [N][H/2][W/2][C] or, nchw_out = 1,
 *                       [N][C][H/2][W/2] = the (C, H', W') flatten order the GRU input uses (:25)
 * av_relu_maxpool2_bwd: dx = dy routed to the first maximum of each 2x2 window where x > 0 (torch max_pool2d / relu backward)
 * av_im2col3:           cols [(n,h,w)][(ky,kx,c)] of a 3x3 / stride 1 / pad 1 window: k-major operand of dW = dY^T cols
 * av_gru_fwd_step / av_gru_bwd_step: nn.GRU(hidden, 2 layers, bidirectional) time steps (:19,32; gate order r, z, n;
 *   h = (1 - z) n + z h_prev), both directions per launch, time-major buffers as av_lstm_*_step: gx [T][B][2][3H] = x W_ih^T + b_ih
 *   from av_gemm; hseq [T][B][2H] compute dtype; hf [T][B][2][H] fp32 state; gates [T][B][2][4H] = (r, z, n, W_hn h + b_hn);
 *   backward (s counts from the END of each chain): dgi / dgh [T][B][2][3H] from dout[t] + dgh[t_next] W_hh + the direct path
 *   dh o z carried in dhc [2][B][H] */
int av_nchw_to_nhwc(const float* in, void* out, int out_dtype, long long N, int C, int H, int W, int Cp, void* stream);
int av_relu_maxpool2_fwd(const void* x, void* y, int dtype, long long N, int H, int W, int C, int nchw_out, void* stream);
int av_relu_maxpool2_bwd(const void* x, const void* dy, void* dx, int dtype, long long N, int H, int W, int C, int nchw_dy, void* stream);
int av_im2col3(const void* x, void* cols, int dtype, long long N, int H, int W, int C, void* stream);
int av_gru_fwd_step(const float* gx, const void* whh, const float* bhh, void* hseq, float* hf, float* gates, void* out_bt, int dtype,
                    int T, int B, int H, int s, void* stream);
int av_gru_bwd_step(const void* dout, int dout_dtype, long long do_bs, long long do_ts, void* dgi, void* dgh, const void* whhT,
                    const float* gates, const float* hf, float* dhc, int dtype, int T, int B, int H, int s, void* stream);

/* file decoding + resampling of the input pipeline (dataset/multi_speaker_dataset.py:15-19 `librosa.load(path, sr=16000)`):
 * av_wav_info / av_wav_read_mono_f32 are HOST-side file I/O (RIFF/WAVE: PCM 8/16/24/32 bit, IEEE float 32/64; float32 mono =
 *   mean over channels of libsndfile-scaled samples, i.e. what librosa holds before it resamples); `out` is HOST memory;
 * av_resample_sinc (device): Kaiser-windowed-sinc interpolation with a linearly interpolated filter table (win / delta [nwin],
 *   num_table entries per zero crossing, already scaled by min(1, sr_out / sr_in)); n_out = ceil(n_in * sr_out / sr_in).
 *   librosa resamples with soxr_hq, whose filter is not published as a formula: this stage is "parity unpinned" (DESIGN 0, (f)-2). */
int av_wav_info(const char* path, int* sample_rate, int* channels, long long* frames, int* bits, int* is_float);
int av_wav_read_mono_f32(const char* path, long long frame0, long long n, float* out);
int av_resample_sinc(const float* x, long long n_in, float* y, long long n_out, const float* win, const float* delta, int nwin, int num_table,
                     int sr_in, int sr_out, void* stream);

/* ---- one wav2vec2 encoder layer, forward, as ONE call ------------------------------------------------------------------------------------
 * replaces: Wav2Vec2EncoderLayerStableLayerNorm.forward (hf:611-640: layer_norm -> attention (hf:438-463: q/k/v projections, softmax(QK^T)V with
 * probability dropout, out_proj) -> hidden dropout -> + residual -> final_layer_norm -> feed_forward (hf:565-572: intermediate_dense, GELU,
 * activation dropout, output_dense, hidden dropout) -> + residual), 16-bit compute type, fp32 residual stream.
 * The entry point enqueues the same seven kernels with the same arguments as av_layernorm_fwd / av_gemm / av_attention_fwd_mask called one by one
 * (bit-identical results); it exists because at small batches the step is bound by host round trips, not by the device.
 * Buffers (caller-allocated, M = B * T rows): h [M][hidden] fp32 in; x1, x2 [M][hidden], qkv [M][3 hidden] (= [B][T][3][heads][hidden / heads]),
 * ao [M][hidden], g [M][inter], u [M][inter] (optional: the pre-activation, or with gf != 0 the saved gradient factor gelu'(.) o mask / keep)
 * in the 16-bit type; h2, h3 [M][hidden] fp32; mu1 / rs1 / mu2 / rs2 [M] and lse [B][heads][T] fp32 (optional: saved for the backward).
 * Weights in nn.Linear layout in the 16-bit type (w_qkv = the packed [3 hidden][hidden] q / k / v projection), biases and LayerNorm parameters fp32.
 * Dropout masks: the counter-hash streams stream_base + 0 (after out_proj), + 1 (after GELU), + 2 (after output_dense), + 3 (attention
 * probabilities; amask = optional precomputed keep bits of av_attention_dropmask) under `seed`; a probability of 0 disables a site. */
typedef struct av_w2v2_layer_args {
    int B, T, hidden, heads, inter;
    int lp;                      /* dtype code of the 16-bit tensors (AV_BF16 = "the library's 16-bit type") */
    int gf;                      /* != 0: FFN-up runs AV_ACT_GELU_GF (u receives the gradient factor) instead of AV_ACT_GELU (u receives the pre-activation) */
    int stream_base;
    float eps, scale;            /* LayerNorm epsilon; softmax scale (head_dim^-0.5) */
    float hd_p, at_p, ac_p;      /* hidden / attention / activation dropout probabilities */
    unsigned long long seed;
    const float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *b_qkv, *b_o, *b_1, *b_2;
    const void *w_qkv, *w_o, *w_1, *w_2;
    const float* h;
    const int* klen;             /* [B] valid key counts or NULL */
    const void* amask;           /* optional keep bits for the attention probabilities */
    void *x1, *qkv, *ao, *x2, *u, *g;
    float *mu1, *rs1, *lse, *h2, *mu2, *rs2, *h3;
} av_w2v2_layer_args;
int av_w2v2_layer_fwd(const av_w2v2_layer_args* args, void* stream);

/* Backward of the same layer when its weights take no gradient (frozen layers above the lowest trainable one: the gradient only passes through):
 * dh [M][hidden] fp32 = gradient of the layer's output h3; dh_lp = optional 16-bit copy of it with THIS layer's FFN-output dropout mask already
 * applied (written by the LayerNorm backward of the layer above; NULL: the entry point makes it in dh3_t).  Saved tensors of av_w2v2_layer_fwd:
 * h, mu1, rs1, qkv, ao, lse, amask, h2, mu2, rs2, u (+ gf).  Weights TRANSPOSED to the K-contiguous form of the dX products, 16-bit:
 * w_2t [inter][hidden] = output_dense^T, w_1t [hidden][inter] = intermediate_dense^T, w_ot [hidden][hidden] = out_proj^T, w_qkvt [hidden][3 hidden].
 * Work / output buffers (caller-allocated): du [M][inter], dx2, dh2_lp, dao, dx1 [M][hidden], dqkv [M][3 hidden] 16-bit; dh2, dh_out [M][hidden] fp32;
 * delta [B][heads][T] fp32; dh_out_lp (optional) = 16-bit copy of dh_out with the dropout mask of stream `lower_stream` (the FFN-output site of the
 * layer below) applied.  Same kernels, same arguments as the per-kernel path of model/w2v2.py::_layer_backward: bit-identical. */
typedef struct av_w2v2_layer_bwd_args {
    int B, T, hidden, heads, inter;
    int lp, gf, stream_base, lower_stream;
    float scale, hd_p, at_p, ac_p;
    unsigned long long seed;
    const float *ln1_g, *ln2_g;
    const void *w_2t, *w_1t, *w_ot, *w_qkvt;
    const float *dh, *h, *mu1, *rs1, *lse, *h2, *mu2, *rs2;
    const void *dh_lp, *qkv, *ao, *amask, *u;
    const int* klen;
    void *dh3_t, *du, *dx2, *dh2_lp, *dao, *dqkv, *dx1, *dh_out_lp;
    float *dh2, *delta, *dh_out;
} av_w2v2_layer_bwd_args;
int av_w2v2_layer_bwd_dx(const av_w2v2_layer_bwd_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif
