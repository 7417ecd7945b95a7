/* mtmp.h -- C ABI of libmtmp_hip.so: the MI355X (gfx950) kernels behind the tri-modal
 * training hot path of AITRICS/Medical_Tri_Modal_Pilot (model tri_mbt_vsltcls).
 *
 * The reference is 100 % Python/PyTorch: there is no FFI in it to mirror.  The boundary it
 * does have is the sequence of ATen calls made by its nn.Modules; each entry point below
 * replaces one such chain and cites it (paths relative to the reference root).
 *
 * Conventions
 *   - plain pointers + sizes, no torch types.  All pointers are DEVICE pointers owned by the
 *     caller (including workspaces and saved-for-backward buffers); nothing here allocates,
 *     synchronises or keeps global state.  Calls are asynchronous on `stream` (a hipStream_t
 *     passed as void*), re-entrant across streams/devices.
 *   - dtype: MTMP_F32 = parity build (fp32 storage, v_mfma_f32_32x32x2_f32, exact fp32 fma
 *     chains), MTMP_BF16 = performance build (bf16 storage, v_mfma_f32_32x32x16_bf16, fp32
 *     accumulate / softmax / LayerNorm statistics).  Same kernels, same indexing.
 *   - return 0 on success; non-zero = argument or launch error, text via mtmp_last_error()
 *     (thread-local).  Row strides ("ld") are in elements.
 *   - d_model = 256 = 4 heads x 64 is fixed on this path (tri_mbt_vsltcls.py:117,227-228).
 */
#ifndef MTMP_H
#define MTMP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MTMP_F32 0
#define MTMP_BF16 1

/* What mtmp_abi_version() returns.  This header is the one place the interface is written down: the library's sources are
 * compiled against it, and the Python binding reads its argument types from it. */
#define MTMP_ABI_VERSION 6

int mtmp_abi_version(void);
const char* mtmp_last_error(void);

/* Modality-aware multi-head attention forward.
 * Replaces builder/models/src/transformer/attention.py:24-49 (bmm, /sqrt(d), masked_fill(-65504),
 * softmax, bmm), the head split/merge of attention.py:72-82 and the key-pad mask of
 * builder/models/src/transformer/utils.py:79-125.
 * q,k,v: [B,N,ld_qkv] (head h = columns [64h,64h+64)); o: [B,N,ld_o]; kv_len: int32[B] valid
 * keys per sample (NULL = unmasked; 0 = fully masked -> uniform average, as the reference);
 * lse: float[B,H,N] out (log2 units, consumed by mtmp_attn_bwd).  If res/o_res are non-NULL,
 * o_res = o + res (the "outputs += residual" of encoder.py:27).
 * key_norms (may be NULL): float[ceil(B N / 32)][H], max ||k_h||_2 over each block of 32 consecutive rows of the [B N] token
 * space (mtmp_key_norms, or the epilogue of the projection that produced k).  With it a wave whose queries satisfy
 * ||q|| max||k|| scale log2(e) <= 64 skips the running maximum of the softmax altogether (exp2 cannot leave the f32 range
 * and the softmax is shift invariant: same result, ~40 % fewer vector instructions); other waves, and every wave when it is
 * NULL, run the online-maximum form. */
int mtmp_attn_fwd(int dtype, const void* q, const void* k, const void* v, void* o, const void* res, void* o_res,
                  float* lse, const int32_t* kv_len, const float* key_norms, int B, int N, int H, int ld_qkv, int ld_o,
                  float scale, void* stream);
/* Grouped forms: up to three token streams (vital signs / image / text of one fusion layer) in ONE launch -- the blocks of the
 * short streams follow the long stream's in the same grid instead of occupying workgroup slots beside it from other HIP
 * streams.  All pointer / int arrays are HOST arrays of n entries (1 <= n <= 3); res / o_res / kv_len / key_norms may be NULL
 * as a whole or per entry; B, H, scale are common.  Same kernels, same results as n calls of the single forms.
 * row_start (may be NULL as a whole or per entry): stream i is PACKED -- row_start[i] is int32[B] on the device
 * (mtmp_row_starts), sample b's kv_len[i][b] tokens are rows row_start[i][b] .. of the q / k / v / o / res / d_o / dq / dk / dv
 * buffers, with no pad rows between samples (kv_len[i][b] is then also the sample's query count); N[i] is the longest
 * sample the buffers were sized for, and stays the stride of lse / delta_ws ([B, H, N[i]]). */
int mtmp_attn_fwd_grouped(int dtype, int n, const void* const* q, const void* const* k, const void* const* v, void* const* o,
                          const void* const* res, void* const* o_res, float* const* lse, const int32_t* const* kv_len,
                          const int32_t* const* row_start, const float* const* key_norms, const int* N, const int* ld_qkv,
                          const int* ld_o, int B, int H, float scale, void* stream);
int mtmp_attn_bwd_grouped(int dtype, int n, const void* const* q, const void* const* k, const void* const* v,
                          const void* const* o, const void* const* d_o, const float* const* lse, const int32_t* const* kv_len,
                          const int32_t* const* row_start, void* const* dq, void* const* dk, void* const* dv,
                          float* const* delta_ws, const int* N, const int* ld_qkv, const int* ld_o, const int* ld_do,
                          const int* ld_dqkv, int B, int H, float scale, void* stream);
/* Prefix-masked forms of the four entries above, for the multi-token bottleneck encoder (mbt_encoder.py:64-94: a fixed boolean
 * block over the first rows and keys of the score matrix, OR-ed onto the key-pad mask).  Same arguments plus, per stream,
 * qk_mask (P HOST words, copied into the kernel arguments by the call) and P (0..16): bit j of word i set = query row i does
 * not attend key j, for i, j < P; the mask is the same for every sample and head of the stream.  Per (b, h):
 *     O = softmax(Q K^T scale + keymask(kv_len[b]) + prefixmask) V
 * i.e. the reference's masked_fill_(mask, -65504) + softmax (attention.py:38-41) on every row that keeps a visible key; a
 * masked pair has probability exactly 0 and no gradient.  Rows >= P of o / o_res / lse / dq are bit-identical to the plain
 * entries; qk_mask NULL (as a whole or per entry) or P = 0 gives the plain entries' result everywhere.  Refused: P > 16, N < P,
 * and a mask row that hides all of keys 0..P-1 (so the kernels never meet an empty key set; callers keep kv_len[b] >= P -- the
 * prefix rows are never pad rows).  The grouped forms take HOST arrays qk_mask[n] / P[n] like their other arrays. */
int mtmp_attn_prefix_fwd(int dtype, const void* q, const void* k, const void* v, void* o, const void* res, void* o_res,
                         float* lse, const int32_t* kv_len, const float* key_norms, const uint16_t* qk_mask, int P, int B, int N,
                         int H, int ld_qkv, int ld_o, float scale, void* stream);
int mtmp_attn_prefix_bwd(int dtype, const void* q, const void* k, const void* v, const void* o, const void* d_o,
                         const float* lse, const int32_t* kv_len, const uint16_t* qk_mask, int P, void* dq, void* dk, void* dv,
                         float* delta_ws, int B, int N, int H, int ld_qkv, int ld_o, int ld_do, int ld_dqkv, float scale,
                         void* stream);
int mtmp_attn_prefix_fwd_grouped(int dtype, int n, const void* const* q, const void* const* k, const void* const* v,
                                 void* const* o, const void* const* res, void* const* o_res, float* const* lse,
                                 const int32_t* const* kv_len, const int32_t* const* row_start, const float* const* key_norms,
                                 const uint16_t* const* qk_mask, const int* P, const int* N, const int* ld_qkv, const int* ld_o,
                                 int B, int H, float scale, void* stream);
int mtmp_attn_prefix_bwd_grouped(int dtype, int n, const void* const* q, const void* const* k, const void* const* v,
                                 const void* const* o, const void* const* d_o, const float* const* lse,
                                 const int32_t* const* kv_len, const int32_t* const* row_start, const uint16_t* const* qk_mask,
                                 const int* P, void* const* dq, void* const* dk, void* const* dv, float* const* delta_ws,
                                 const int* N, const int* ld_qkv, const int* ld_o, const int* ld_do, const int* ld_dqkv, int B,
                                 int H, float scale, void* stream);
/* Attention of ONE query row per sample -- the CLS token of the last fusion layer of the vital-sign stream: tri_mbt_vsltcls.py:248
 * reads nothing of the encoder's result but outputs[0][:, 0, :], so in the LAST layer only that row's attention output, FFN and
 * residuals feed the loss (its keys / values still come from all rows).  q / k / v [rows, ld_qkv], res [rows, ld_res] (the layer
 * input: residual of encoder.py:27); kv_len / row_start as in mtmp_attn_fwd_grouped (both may be NULL: padded [B, N], all keys
 * valid); cls_tok = the query's token index inside a sample.  _fwd: o_cls, r1_cls [B, H * 64] (the attention output and output +
 * residual, both in `dtype`), lse float[B, H].  _bwd: d_o [B, H * 64] = gradient w.r.t. o_cls -> dq, dk, dv written for EVERY row
 * of every sample (dense [rows, ld_dqkv]; dq is zero outside row cls_tok, rows past kv_len are zero): what mtmp_gemm_tn /
 * mtmp_gemm_lnbwd read next.  Replaces attention.py:24-84 (+ autograd) for that one row. */
int mtmp_attn_cls_fwd(int dtype, const void* q, const void* k, const void* v, int ld_qkv, const void* res, int ld_res, void* o_cls,
                      void* r1_cls, float* lse, const int32_t* kv_len, const int32_t* row_start, int B, int N, int H, int cls_tok,
                      float scale, void* stream);
int mtmp_attn_cls_bwd(int dtype, const void* q, const void* k, const void* v, int ld_qkv, const void* o_cls, const void* d_o,
                      const float* lse, const int32_t* kv_len, const int32_t* row_start, void* dq, void* dk, void* dv, int ld_dqkv,
                      int B, int N, int H, int cls_tok, float scale, void* stream);
/* out[ceil(rows / 32)][H] = max over each 32-row block of ||k[row, 64h : 64h + 64]||_2 (k: [rows, ld]). */
long long mtmp_key_norms_floats(long long rows, int H);
int mtmp_key_norms(int dtype, const void* k, float* out, long long rows, int H, int ld, void* stream);

/* Backward of the above: dq,dk,dv [B,N,ld_dqkv] from d_o [B,N,ld_do]; o is the forward output.
 * delta_ws: float[B*H*N] scratch. */
int mtmp_attn_bwd(int dtype, const void* q, const void* k, const void* v, const void* o, const void* d_o,
                  const float* lse, const int32_t* kv_len, void* dq, void* dk, void* dv, float* delta_ws, int B,
                  int N, int H, int ld_qkv, int ld_o, int ld_do, int ld_dqkv, float scale, void* stream);

/* y[M,N] = act(LN(x[M,256]) w[N,256]^T + bias): custom LayerNorm (module.py:138-144: unbiased
 * std, eps added to std) fused into the Q/K/V projections (attention.py:60-62,68-70; w = [Wq;Wk;Wv])
 * or the first FFN conv + ReLU (module.py:74-77).  gamma/beta/bias fp32; w in `dtype`.
 * N % 64 == 0 (bf16) / N % 32 == 0 (fp32): features are walked in whole weight panels.
 * Optional outputs: xn[M,256] = LN(x) (dtype), stats[M,2] = (mean, 1/(std+eps)).
 * drop_p > 0 applies nn.Dropout (module.py:77-79 drop1) to the activated output with the
 * counter-based mask keep(seed ^ *seed_dev, row*N+col); the backward regenerates it (mtmp_dropout_bwd).
 * seed_dev (may be NULL) is a device word the host advances every step, so that a captured hipGraph
 * (whose scalar arguments are frozen) still draws fresh masks on every replay. */
int mtmp_ln_gemm(int dtype, const void* x, const float* gamma, const float* beta, const void* w, const float* bias,
                 void* y, void* xn, float* stats, int M, int N, int ldx, int ldy, float eps, int relu, float drop_p,
                 unsigned seed, const unsigned* seed_dev, void* stream);

/* mtmp_ln_gemm for the Q/K/V projection of an encoder layer (w = [Wq; Wk; Wv], N = 768, ldy = 768, no activation) that
 * also fills the key-norm table of mtmp_attn_fwd from its epilogue: key_norms[ceil(M / 32)][4] (mtmp_key_norms_floats(M, 4)
 * floats).  Replaces module.py:138-144 + attention.py:68-70. */
int mtmp_ln_gemm_qkv(int dtype, const void* x, const float* gamma, const float* beta, const void* w, const float* bias,
                     void* y, void* xn, float* stats, float* key_norms, int M, int ldx, float eps, void* stream);

/* y[M,N] = drop(act(a[M,K] w[N,K]^T + bias)) (+ res[M,N]); K % 8 == 0, N % 32 == 0; res must not alias y.
 * Second FFN conv + drop2 + residual (module.py:78-80, encoder.py:32).  With gate[M,N] != NULL the
 * result is gated: y = gate > 0 ? y * gate_scale : 0 -- the backward of ReLU (+ drop1) applied to
 * dH = dY W2 in the same pass (gate = the stored post-dropout activations). */
/* act: 0 none, 1 ReLU, 2 exact GELU; K % 8 == 0 (a 64-wide chunk's tail reads as zero);
 * row_scale[M / rows_per_scale] (may be NULL) multiplies row blocks before the residual add
 * (row-mode StochasticDepth of the Swin blocks). */
int mtmp_gemm_nt(int dtype, const void* a, const void* w, const float* bias, const void* res, void* y, int M, int N,
                 int K, int lda, int ldy, int ldr, int act, float drop_p, unsigned seed, const unsigned* seed_dev,
                 const void* gate, float gate_scale, const float* row_scale, int rows_per_scale, void* stream);

/* Sign bits of a ReLU projection (bf16 build, N % 64 == 0): one bit per output, "y > 0", in the row-panel kernels' private
 * order; mtmp_sign_bits_bytes(M, N) bytes (= M N / 8).
 *   mtmp_ln_gemm_signs  = mtmp_ln_gemm with relu = 1 (module.py:74-77 + drop1) that also writes them;
 *   mtmp_gemm_nt_signs  : y[M,N] = signs ? (a[M,256] w[N,256]^T) * gate_scale : 0 -- the FFN backward's dH = dY W2 taken
 *     through the ReLU + drop1 of module.py:77-79 (autograd) without re-reading the M x N hidden activation, whose sign is
 *     all that step needs: 4 MB of gate traffic per launch at config 2 instead of 132 MB.
 * Other dtypes return MTMP_ERR_ARG (the fp32 build gates on the stored activation through mtmp_gemm_nt). */
long long mtmp_sign_bits_bytes(int M, int N);
int mtmp_ln_gemm_signs(int dtype, const void* x, const float* gamma, const float* beta, const void* w, const float* bias,
                       void* y, void* xn, float* stats, int M, int N, int ldx, int ldy, float eps, float drop_p,
                       unsigned seed, const unsigned* seed_dev, void* signs, void* stream);
int mtmp_gemm_nt_signs(int dtype, const void* a, const void* w, void* y, int M, int N, int lda, int ldy,
                       const void* signs, float gate_scale, void* stream);
/* mtmp_gemm_nt_signs with the backward of a dropout on its A operand folded in (autograd of module.py:78-80 in front of dH):
 * a' = keep ? a / (1 - drop_p) : 0 with mtmp_dropout_bwd's mask for (seed, seed_dev, drop_p) on the contiguous [M,256] tensor,
 * y = signs ? (a' w^T) * gate_scale : 0, a_out [M,256] (may be NULL) = a' (the weight-gradient product's operand). */
int mtmp_gemm_nt_signs_drop(int dtype, const void* a, const void* w, void* y, int M, int N, int lda, int ldy,
                            const void* signs, float gate_scale, float drop_p, unsigned seed, const unsigned* seed_dev,
                            void* a_out, void* stream);

/* Weight / bias gradient of the Linear and k=1 Conv1d layers (attention.py:60-62, module.py:74-78):
 * dw[N,K] (fp32) = dy[M,N]^T x[M,K];  db[N] (fp32, may be NULL) = column sums of dy.
 * and of the trainable image encoder's Linear layers (stem, Swin blocks, patch merging):
 * dw[N,K] (fp32) = dy[M,N]^T x[M,K];  db[N] (fp32, may be NULL) = column sums of dy.
 * M >= 1, N % 8 == 0, K % 8 == 0, ldy >= N, ldx >= K, ldy % 8 == 0, ldx % 8 == 0, dy and x 16-byte aligned; anything else
 * returns MTMP_ERR_ARG.  Columns past N / K of the operands are neither used nor written.  N and K both multiples of 128 run
 * the tuned kernels of the fusion layers; every other shape runs one kernel with 128 x 128 tiles whose columns past N / K are
 * masked.  The contraction runs over the M tokens (split over workgroups, no atomics: a call is reproducible bit for bit):
 * partial slabs [mtmp_gemm_tn_slab_rows(dtype,M,N,K)][N K + N] in ws, then one reduce pass -- or, with dw == NULL, left in
 * ws for mtmp_reduce_batch.  ws: mtmp_gemm_tn_ws_floats(M,N,K) floats (enough for either dtype). */
long long mtmp_gemm_tn_ws_floats(int M, int N, int K);
int mtmp_gemm_tn(int dtype, const void* dy, const void* x, float* dw, float* db, float* ws, int M, int N, int K,
                 int ldy, int ldx, void* stream);
/* The same with rows_live (may be NULL): a DEVICE word with the rows in use (<= M) -- a packed token stream, see the grouped
 * forms below; split count, workspace and grid stay those of M, the splits share the live rows. */
int mtmp_gemm_tn_live(int dtype, const void* dy, const void* x, float* dw, float* db, float* ws, int M, int N, int K,
                      int ldy, int ldx, const int32_t* rows_live, void* stream);

/* g_out[i] = keep(seed,i) ? g_in[i]/(1-p) : 0 over n contiguous elements: backward of the epilogue
 * dropout above (n = M*N of that call, n % 4 == 0). */
int mtmp_dropout_bwd(int dtype, const void* g_in, void* g_out, long long n, unsigned seed, const unsigned* seed_dev,
                     float p, void* stream);

/* Backward of the custom LayerNorm (module.py:138-144), plus the residual-branch gradient:
 * dz[M,256] = LNbwd(dy[M,256]; z, stats, gamma) (+ d_res); dgamma_dbeta float[512] overwritten.
 * ws: mtmp_ln_bwd_ws_floats(M) floats. */
int mtmp_ln_bwd_ws_floats(int M);
int mtmp_ln_bwd(int dtype, const void* z, int ldz, const float* stats, const float* gamma, const void* dy,
                const void* d_res, int ldr, void* dz, float* dgamma_dbeta, float* ws, int M, float eps, void* stream);

/* The dX product of a LayerNorm-fed projection fused with that LayerNorm's backward -- autograd of
 * module.py:138-144 in front of attention.py:68-70 (K = 768) / module.py:74-77 (K = 1024):
 * dz[M,256] = LNbwd(dy[M,K] wt[256,K]^T; z, stats, gamma) (+ d_res); dgamma_dbeta float[512] overwritten.
 * wt = W^T of y = LN(z) W^T, K-contiguous; the M x 256 product never goes to HBM.
 * ws: mtmp_gemm_lnbwd_ws_floats(M) floats. */
int mtmp_gemm_lnbwd_ws_floats(int M);
int mtmp_gemm_lnbwd(int dtype, const void* dy, const void* wt, const void* z, int ldz, const float* stats,
                    const float* gamma, const void* d_res, int ldr, void* dz, float* dgamma_dbeta, float* ws, int M,
                    int K, int ldy, float eps, void* stream);

/* TIE/UMSE event embedding (tri_mbt_vsltcls.py:59-71,183-190):
 * out[n,256] = ReLU(LN(value*w_v+b_v)) + ReLU(LN(time*w_t+b_t)) + ftab[feature].
 * events float[n,3] = (time, value, feature index); params float[8][256] = ie_vslt.{0.weight,0.bias,
 * 1.weight,1.bias} then ie_time.{same}; ftab float[20][256] = ie_feat.weight. */
int mtmp_tie_embed_fwd(int dtype, const float* events, const float* params, const float* ftab, void* out, int n,
                       void* stream);
/* grads float[28][256] overwritten (8 parameter vectors in `params` order, then d ftab). */
int mtmp_tie_bwd_ws_floats(int n);
int mtmp_tie_embed_bwd(int dtype, const float* events, const float* params, const void* d_out, float* grads,
                       float* ws, int n, void* stream);

/* Time + modality-id embedding added to every image / text token (tri_mbt_vsltcls.py:216-224):
 * out[n,256] = ReLU(LN(time*w_t+b_t)) + ftab[feature], i.e. the event embedding without its value chain;
 * same events / params / grads layout as above (ws: mtmp_tie_bwd_ws_floats(n)). */
int mtmp_time_embed_fwd(int dtype, const float* events, const float* params, const float* ftab, void* out, int n,
                        void* stream);
int mtmp_time_embed_bwd(int dtype, const float* events, const float* params, const void* d_out, float* grads,
                        float* ws, int n, void* stream);

/* The same on the PACKED (ragged) batch layout of the collate (replaces the zero-padded
 * [B, TIE_len, 3] tensor of dataset_new.py:2177 + the [:, :max_len] trim of trainer.py:41-42):
 * events float[cu[B]][3] back to back, cu_seqlens int32[B+1] (device), out / d_out [B, t_pad, 256];
 * output rows past a sample's length are zero and receive no gradient.
 * ws: mtmp_tie_bwd_ws_floats(B * t_pad) floats. */
int mtmp_tie_embed_packed_fwd(int dtype, const float* events, const int32_t* cu_seqlens, int B, int t_pad,
                              const float* params, const float* ftab, void* out, void* stream);
int mtmp_tie_embed_packed_bwd(int dtype, const float* events, const int32_t* cu_seqlens, int B, int t_pad,
                              const float* params, const void* d_out, float* grads, float* ws, void* stream);

/* Stream input of the fusion encoder (mbt_encoder.py:697-729 and the concatenation of :745) in one launch:
 * out[b] = [ bott (nb rows) | dropout(LN(cls) + pe[0]) | dropout(LN(x[b,t]) + pe[t+1]), t = 0..N-1 ],
 * nn.LayerNorm semantics (biased variance, eps inside the root) in fp32; x, out, dz, dx in `dtype`;
 * cls / gamma / beta float[256], pe float[>= N+1][256] or NULL, bott float[nb][256] (nb <= 4);
 * stats float[B*(N+1)][2] is written by the forward and read by the backward; dropout as in mtmp_dropout_bwd
 * (seed ^ *seed_dev). grads float[7][256] = dgamma, dbeta, dcls, dbott[0..3], overwritten.
 * ws: mtmp_stream_input_ws_floats(B * (nb+1+N)) floats.
 * row_start / kv_len (int32 device, NULL together): PACKED output -- row r < kv_len[b] of sample b is written to row
 * row_start[b] + r of `out` (read from there in dz), the other rows are not written; x / dx keep the padded [B,N,256]
 * layout (dx rows of pad events are written as zeros). */
int mtmp_stream_input_ws_floats(int rows);
int mtmp_stream_input_fwd(int dtype, const void* x, const float* cls, const float* gamma, const float* beta,
                          const float* pe, const float* bott, void* out, float* stats, int B, int N, int nb, float eps,
                          float p, unsigned seed, const unsigned* seed_dev, const int32_t* row_start, const int32_t* kv_len,
                          void* stream);
int mtmp_stream_input_bwd(int dtype, const void* dz, const void* x, const float* cls, const float* gamma,
                          const float* stats, void* dx, float* grads, float* ws, int B, int N, int nb, float p,
                          unsigned seed, const unsigned* seed_dev, const int32_t* row_start, const int32_t* kv_len,
                          void* stream);

/* Classification head (tri_mbt_vsltcls.py:59-76 ie_demo, :248-255): out[b] = fc3(ReLU(BatchNorm1d(fc0([LN(cls[b]) |
 * ReLU(LN(ie_demo.0(age, gender)))])))), fp32, B <= 256, six launches forward + backward instead of ~65 torch kernels.
 * params: 14 device pointers (float): ie_demo.0.weight[256][2], ie_demo.0.bias, ie_demo.1.weight, ie_demo.1.bias,
 * layer_norms_after_concat.{weight,bias}, fc_list.0.{weight[256][512],bias}, fc_list.1.{weight,bias,running_mean,
 * running_var} (the running statistics are updated in place when training != 0), fc_list.3.{weight[256],bias[1]}.
 * ws_fwd: mtmp_head_ws_floats(B) floats, written by the forward and read by the backward.
 * backward outputs (overwritten): dcls[B][256]; g_rows[7][256] = d layer_norms_after_concat.{weight,bias}, d ie_demo.1.{weight,
 * bias}, d ie_demo.0.weight[:,0], [:,1], d ie_demo.0.bias; dw1[256][512]; g_feat[4][256] = d fc_list.0.bias, d fc_list.1.{weight,
 * bias}, d fc_list.3.weight; db2[1].  ws_bwd: B*256*8 floats. */
int mtmp_head_ws_floats(int B);
int mtmp_head_fwd(const float* cls, const float* age, const float* gender, const void* const* params, float* out, float* ws,
                  int B, float ln_eps, float bn_eps, float momentum, int training, void* stream);
int mtmp_head_bwd(const float* d_out, const float* cls, const float* age, const float* gender, const void* const* params,
                  const float* ws_fwd, float* dcls, float* g_rows, float* dw1, float* g_feat, float* db2, float* ws_bwd, int B,
                  float ln_eps, int training, void* stream);
/* The head with the CLS vectors in the fusion stack's own type (ABI 6): cls / dcls [B][256] in cls_dtype (no cast launch on either
 * side of the head), num_batches_tracked (device int64, may be NULL) incremented by the first launch, and every parameter's
 * gradient written to a destination of its own: dst[12] in the order of the 12 trained parameters of `params` (ie_demo.0.weight
 * [256][2], ie_demo.0.bias, ie_demo.1.{weight,bias}, layer_norms_after_concat.{weight,bias}, fc_list.0.{weight,bias},
 * fc_list.1.{weight,bias}, fc_list.3.{weight,bias}) -- slices of the flat gradient buffer, or scratch.  Same math, workspaces and
 * limits as mtmp_head_fwd / mtmp_head_bwd. */
int mtmp_head_fwd_t(int cls_dtype, const void* cls, const float* age, const float* gender, const void* const* params, float* out,
                    float* ws, int B, float ln_eps, float bn_eps, float momentum, int training, long long* num_batches_tracked,
                    void* stream);
int mtmp_head_bwd_scatter(int cls_dtype, const float* d_out, const void* cls, const float* age, const float* gender,
                          const void* const* params, const float* ws_fwd, void* dcls, float* const* dst, float* ws_bwd, int B,
                          float ln_eps, int training, void* stream);

/* The same head with --vslt-type QIE (tri_mbt_vsltcls.py:148-151, 248-250; csrc/head.hip at width 256): nothing is concatenated, the
 * head reads the 256 columns of LN(cls): out[b] = fc3(ReLU(BatchNorm1d(fc0(LN(cls[b]))))).  mtmp_head_fwd_t / mtmp_head_bwd_scatter without
 * age, gender and the four ie_demo parameters.  params: 10 device pointers (float): layer_norms_after_concat.{weight,bias},
 * fc_list.0.{weight[256][256],bias}, fc_list.1.{weight,bias,running_mean,running_var}, fc_list.3.{weight[256],bias[1]}.
 * dst[8]: the gradients of the eight trained ones in that order (overwritten).  ws_fwd: mtmp_headq_ws_floats(B) floats, written by
 * the forward and read by the backward; ws_bwd: B*256*8 floats.  1 <= B <= 256, B > 1 in training mode. */
int mtmp_headq_ws_floats(int B);
int mtmp_headq_fwd_t(int cls_dtype, const void* cls, const void* const* params, float* out, float* ws, int B, float ln_eps,
                     float bn_eps, float momentum, int training, long long* num_batches_tracked, void* stream);
int mtmp_headq_bwd_scatter(int cls_dtype, const float* d_out, const void* cls, const void* const* params, const float* ws_fwd,
                           void* dcls, float* const* dst, float* ws_bwd, int B, float ln_eps, int training, void* stream);

/* The QIE input (tri_mbt_vsltcls.py:191-198, 216-221; csrc/qie.hip): demo[b] = ReLU(LN(ie_demo.0(age[b], gender[b]))) in fp32 is
 * added to every token of the three streams.  Forward, one launch: add_v[b] = demo[b], add_i[b] = it[b] + demo[b], add_t[b] =
 * tt[b] + demo[b], all [B][256] in `dtype` (what mtmp_stream_input_fwd_add takes as `add`, add_L = the stream's token count); it /
 * tt are NULL together (--imgtxt-time 0): add_i / add_t are then left alone.  params: 4 device pointers (float):
 * ie_demo.0.weight[256][2], ie_demo.0.bias, ie_demo.1.{weight,bias}.
 * Backward, two launches, no float atomics, bit-identical between runs: dx_v [B][N_v][256], dx_i [B][N_i][256], dx_t [B][N_t][256]
 * in `dtype` are the stream inputs' gradients as mtmp_stream_input_bwd_grouped leaves them (dx_i / dx_t / d_it / d_tt NULL together);
 * kv_len (device int32[B], may be NULL) with kv_off: sample b's dx_v rows from max(kv_len[b] - kv_off, 0) on are zeros (a packed
 * stream's pad rows) and are skipped.  d_it[b] = sum_j dx_i[b][j], d_tt[b] = sum_j dx_t[b][j] in `dtype` (mtmp_token_sums' values);
 * dst[4]: the gradients of the four parameters (overwritten) from d_demo[b] = sum_t dx_v + sum_j dx_i + sum_j dx_t, kept in fp32.
 * ws: mtmp_qie_adds_bwd_ws_floats(B, N_v, dx_i != NULL) floats. */
int mtmp_qie_adds_fwd(int dtype, const float* age, const float* gender, const void* const* params, const void* it, const void* tt,
                      void* add_v, void* add_i, void* add_t, int B, float ln_eps, void* stream);
long long mtmp_qie_adds_bwd_ws_floats(int B, int N_v, int with_time);
int mtmp_qie_adds_bwd(int dtype, const void* dx_v, const void* dx_i, const void* dx_t, const int32_t* kv_len, int kv_off,
                      const float* age, const float* gender, const void* const* params, void* d_it, void* d_tt, float* const* dst,
                      float* ws, int B, int N_v, int N_i, int N_t, float ln_eps, void* stream);

/* BCEWithLogitsLoss(reduction="mean") (2_train.py:76, trainer.py:128): loss[0] = mean_b [max(o,0) - o t + log1p(exp(-|o|))],
 * dlogit[b] = (sigmoid(o_b) - t_b) / n; logits / target / dlogit float[n]. */
int mtmp_bce_logits_mean(const float* logits, const float* target, float* loss, float* dlogit, int n, void* stream);

/* Three-row LayerNorm head (tri_mbt_v1.py:154-159,271-281; tri_mbt_vnoshavgtr.py / tri_mbt_vnoshnoavgtr.py: one head per row):
 * out[m][b] = fc_m(cat[LN(cls_m[b]), ReLU(LN(ie_demo.0(age, gender)))]), fc_m = Linear(512,256) -> LayerNorm -> ReLU -> Linear(256,1),
 * rows m = 0, 1, 2 = vslt, image, text; fp32, 1 <= B <= 256; three launches forward, four backward, no float atomics.
 * cls[3]: the CLS rows of the three streams in cls_dtype (MTMP_F32 | MTMP_BF16), row b of stream m at cls[m] + b * cls_ld[m]
 * elements (16-byte aligned base, cls_ld[m] >= 256 and a multiple of 4).  params: 6 + 6 * n_sets device pointers (float):
 * ie_demo.0.weight[256][2], ie_demo.0.bias, ie_demo.1.{weight,bias}, layer_norms_after_concat.{weight,bias}, then per set
 * {0.weight[256][512], 0.bias, 1.weight, 1.bias, 3.weight[256], 3.bias[1]}; n_sets = 3: set m for row m, n_sets = 1: one set
 * shared by the three rows.  out float[3][B].  ws_fwd: mtmp_head3_ws_floats(B) floats, written by the forward, read by the backward.
 * backward: d_out float[3][B]; dcls[3]: [B][256] contiguous each, in cls_dtype; dst: one destination per entry of params
 * (overwritten; slices of the flat gradient buffer, or scratch) -- a shared set and the first six get the three rows' contributions
 * summed in the fixed order m = 0, 1, 2.  ws_bwd: mtmp_head3_bwd_ws_floats(B) floats. */
int mtmp_head3_ws_floats(int B);
int mtmp_head3_bwd_ws_floats(int B);
int mtmp_head3_fwd(int cls_dtype, const void* const* cls, const long long* cls_ld, const float* age, const float* gender,
                   const void* const* params, int n_sets, float* out, float* ws, int B, float ln_eps, void* stream);
int mtmp_head3_bwd(int cls_dtype, const float* d_out, const void* const* cls, const long long* cls_ld, const float* age,
                   const float* gender, const void* const* params, int n_sets, const float* ws_fwd, void* const* dcls,
                   float* const* dst, float* ws_bwd, int B, float ln_eps, void* stream);

/* The same head on R rows, 1 <= R <= 4 (csrc/headr.hip), whose inputs are BLOCKS: blocks[s] (s < n_blocks <= 3) is a strided view
 * [B][block_rows[s]][256] in `dtype` (0 fp32, 1 bf16; one for all blocks) at blocks[s] + b * block_ld[s] + row * row_ld[s] in
 * elements (16-byte aligned base, 1 .. 4 rows, both strides >= 256 and multiples of 4).  Head row m reads n_src[m] in {1, 2, 3}
 * sources (block, row) = (src[2 * (3 m + i)], src[2 * (3 m + i) + 1]) for i < n_src[m] (src: int[R][3][2]; blocks, block_ld,
 * row_ld, block_rows, n_src and src are host arrays) and takes the LayerNorm of their fp32 mean ((a + b) + c) / n.  A (block, row)
 * pair may feed at most one head row; anything else is refused by message.  params: as mtmp_head3_fwd, n_sets in {1, R} (one set
 * shared by the R rows, or set m for row m).  out float[R][B].  ws_fwd: mtmp_headr_ws_floats(R, B) floats, written by the
 * forward, read by the backward.
 * backward: d_out float[R][B]; dblocks[s]: [B][block_rows[s]][256] contiguous, in `dtype`, EVERY row written: a source row gets
 * d(head row) / n_src, a row that is no source exact zeros.  dst: one destination per entry of params (overwritten) -- a shared
 * set and the first six get the rows' contributions, each finished on its own, added in the order m = 0 .. R-1.
 * ws_bwd: mtmp_headr_bwd_ws_floats(R, B) floats.  1 <= B <= 256.  Three launches forward, four backward, no float atomics. */
int mtmp_headr_ws_floats(int R, int B);
int mtmp_headr_bwd_ws_floats(int R, int B);
int mtmp_headr_fwd(int dtype, int n_blocks, const void* const* blocks, const long long* block_ld, const long long* row_ld,
                   const int* block_rows, int R, const int* n_src, const int* src, const float* age, const float* gender,
                   const void* const* params, int n_sets, float* out, float* ws, int B, float ln_eps, void* stream);
int mtmp_headr_bwd(int dtype, const float* d_out, int n_blocks, const void* const* blocks, const long long* block_ld,
                   const long long* row_ld, const int* block_rows, int R, const int* n_src, const int* src, const float* age,
                   const float* gender, const void* const* params, int n_sets, const float* ws_fwd, void* const* dblocks,
                   float* const* dst, float* ws_bwd, int B, float ln_eps, void* stream);

/* Learned weighting of R <= 4 logits over the modalities present (tri_mbt_vflexible.py:276-286, bitxt_ / biimg_mbt_vflexible1.py):
 * p[m][b] = softmax over the present rows of temperature * a[m], exactly 0 on absent rows; out[b] = sum_m p[m][b] o[m][b].
 * o / d_o float[R][B], a / d_a float[R], out / d_out float[B], missing_num int64[B] (read as id & 3: nothing is indexed by it);
 * table: bit 4 * pattern + row set = row `row` is present under that pattern id.  backward: d_o[m][b] = p[m][b] d_out[b],
 * d_a[m] = temperature * sum_b p[m][b] d_out[b] (o[m][b] - out[b]), summed over the batch in a fixed order (one workgroup, no
 * atomics).  One launch each way, any B > 0, no host synchronisation. */
int mtmp_flex_combine_fwd(const float* o, const float* a, float temperature, const long long* missing_num, unsigned table,
                          float* out, int R, int B, void* stream);
int mtmp_flex_combine_bwd(const float* d_out, const float* o, const float* a, float temperature, const long long* missing_num,
                          unsigned table, float* d_o, float* d_a, int R, int B, void* stream);

/* Mean of the three logits over the modalities present under the pattern id missing_num[b] (trainer.py:68-77,224-229;
 * tri_mbt_v1.py:272-281): S(0) = {0,1,2}, S(1) = {0,1}, S(2) = {0,2}, S(3) = {0}; o / d_o float[3][B], out / d_out float[B],
 * missing_num int64[B] (read as id & 3: nothing is indexed by it).  d_o[m][b] = d_out[b] / |S| inside the set, 0 outside. */
int mtmp_candidate_mean_fwd(const float* o, const long long* missing_num, float* out, int B, void* stream);
int mtmp_candidate_mean_bwd(const float* d_out, const long long* missing_num, float* d_o, int B, void* stream);

/* BCEWithLogitsLoss(reduction="mean") over the present (row, sample) pairs (trainer.py:169-174): loss[0] = (1/n) sum_b sum_{m in
 * S(missing_num[b])} bce(logits[m][b], target[b]) with n = sum_b |S| counted on the device; dlogit float[3][B] = (sigmoid - target) / n
 * inside the sets, 0 outside.  One launch, any B > 0, no host synchronisation. */
int mtmp_bce_masked_mean(const float* logits, const float* target, const long long* missing_num, float* loss, float* dlogit, int B,
                         void* stream);

/* The same over R <= 4 logit rows with a table of trained rows (the multi-token models: trainer.py:79-83 and 164-168,
 * ``criterion(output[missing == 0], target.repeat(4)[missing == 0])`` with missing = missing_multitoken[missing_num]): bit
 * 4 * pattern + row of `table` set = row `row` is trained on a sample with that pattern id (ids are taken & 3).  logits / dlogit
 * float[R][B]; n is counted on the device.  One launch, any B > 0, no host synchronisation. */
int mtmp_bce_rows_masked_mean(const float* logits, const float* target, const long long* missing_num, unsigned table, float* loss,
                              float* dlogit, int R, int B, void* stream);

/* Stream-ordered time stamp: a one-lane kernel on `stream` stores the 100 MHz wall clock into *slot.  Also works inside a
 * captured hipGraph, where HIP events cannot be timed -- bench.py brackets the roofline kernel of the replayed steps with it. */
int mtmp_timestamp(unsigned long long* slot, void* stream);

/* Swin-T patch-embedding stem: Conv2d(1,96,4,stride 4) -> NHWC -> LayerNorm(96)
 * (builder/models/src/swin_transformer.py:559-567,646) as an implicit GEMM.
 * img float[n_img,1,H,W]; out [n_img,H/4,W/4,96] in `dtype`. */
int mtmp_swin_stem_fwd(int dtype, const float* img, const float* w, const float* bias, const float* ln_w,
                       const float* ln_b, void* out, int n_img, int H, int W, void* stream);

/* nn.LayerNorm(C) over rows (Swin norm1/norm2/final norm, swin_transformer.py:428-449,611-612);
 * merge != 0 fuses the 2x2 patch-merging gather of swin_transformer.py:34-44: x is [n,H,W,C/4],
 * rows = n*(H/2)*(W/2).  w,b fp32; C even, <= 1536. */
int mtmp_layernorm_rows(int dtype, const void* x, const float* w, const float* b, void* y, long long rows, int C,
                        float eps, int merge, int H, int W, void* stream);

/* y[M,N] = LayerNorm(x[M,C]; ln_w, ln_b, eps) W[N,C]^T + bias: norm1 + the qkv projection of a Swin block in one launch
 * (swin_transformer.py:428-449 + :115-225; replaces mtmp_layernorm_rows + mtmp_gemm_nt for the narrow stages).
 * bf16 only (dtype 1), C = 96 or 192, N % 32 == 0; W bf16; ln_w, ln_b, bias fp32 (bias may be NULL). */
int mtmp_swin_ln_linear(int dtype, const void* x, const float* ln_w, const float* ln_b, const void* w, const float* bias,
                        void* y, long long M, int C, int N, float eps, void* stream);

/* MLP half of a Swin block in one launch (swin_transformer.py:428-449, torchvision MLP keys mlp.0 / mlp.3):
 * y[M,C] = x + row_scale[row / rows_per_scale] * (gelu(LayerNorm(x; ln_w, ln_b, eps) W1^T + b1) W2^T + b2).
 * Replaces mtmp_layernorm_rows + mtmp_gemm_nt(act = GELU) + mtmp_gemm_nt(residual, row_scale) for the narrow stages, whose
 * 4C-wide hidden activation then never reaches HBM.  bf16 only (dtype 1), C = 96 or 192; w1 [4C,C], w2 [C,4C] bf16;
 * ln_w, ln_b, b1, b2 fp32; row_scale (per-image StochasticDepth factor) may be NULL; y must not alias x. */
int mtmp_swin_mlp(int dtype, const void* x, const float* ln_w, const float* ln_b, const void* w1, const float* b1,
                  const void* w2, const float* b2, const float* row_scale, int rows_per_scale, void* y, long long M, int C,
                  float eps, void* stream);

/* Shifted-window attention (swin_transformer.py:115-225, V1 branch) on the un-shifted NHWC map:
 * qkv [n,H,W,3C] -> out [n,H,W,C]; window 7x7, head_dim 32, H % 7 == W % 7 == 0.
 * table [4 window types][heads][64][64] in `dtype` = relative-position bias + shift mask
 * (type = 2*(last window row) + (last window col), 0 when shift == 0), -30000 on pad keys.
 * shift > 0 needs H > 7 and W > 7: the reference does not shift an axis of one window (:155-160), so such a call is refused
 * (the caller passes shift 0 for a 7x7 map); the same holds for mtmp_swin_window_attn_live / _bwd and mtmp_swin_attn_block. */
int mtmp_swin_window_attn(int dtype, const void* qkv, const void* table, void* out, int n_img, int H, int W, int C,
                          int heads, int shift, float scale, void* stream);

/* Fused AdamW (2_train.py:110, torch.optim.AdamW math) over flat fp32 buffers of n elements
 * (n % 4 == 0); optional bf16 shadow copy of the parameters; grad is multiplied by grad_scale
 * first (1/world_size after an RCCL all-reduce SUM). */
int mtmp_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, void* bf16_shadow,
                    long long n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                    float grad_scale, void* stream);

/* Bottleneck exchange between the modality streams (mbt_encoder.py:764-779), in place on the stream
 * buffers z_m [B, n_m, 256] whose rows 0..3 are the four bottleneck tokens (n_m = 4 + 1 + tokens):
 * rows 0..3 of all three become the per-sample weighted mean over the present modalities
 * (missing[b] 0: vslt+img+txt, 1: vslt+img, 2: vslt+txt, 3: vslt) -- with resbottle != 0 averaged with
 * prev [B,4,256] fp32 (mbt_encoder.py:741-742,778-779).  keep (may be NULL) receives the fp32 result.
 * _bwd transforms the gradient buffers dz_m the same way in place: rows 0..3 hold the consumers'
 * gradients on entry and each stream's own bottleneck-output gradient on exit; d_prev_in (may be NULL) /
 * d_prev_out carry the residual path between consecutive exchanges.
 * z_t / dz_t may be NULL: the two-stream encoder (BimodalTransformerEncoder_MBT, mbt_encoder.py:519-634), whose
 * patterns {0: mean of both, 1: stream 0} the caller passes as rows 1 and 3.
 * row_start_v (int32[B] device, may be NULL): the first buffer is PACKED, its sample b starts at row row_start_v[b]. */
int mtmp_bottleneck_exchange_fwd(int dtype, void* z_v, void* z_i, void* z_t, int B, int n_v, int n_i, int n_t,
                                 const long long* missing, int resbottle, const float* prev, float* keep,
                                 const int32_t* row_start_v, void* stream);
int mtmp_bottleneck_exchange_bwd(int dtype, void* dz_v, void* dz_i, void* dz_t, int B, int n_v, int n_i, int n_t,
                                 const long long* missing, int resbottle, const float* d_prev_in, float* d_prev_out,
                                 const int32_t* row_start_v, void* stream);

/* Multi-set bottleneck exchange of TrimodalTransformerEncoder_Multitokens_MBTVSLTMAIN (mbt_encoder.py:98-101, 178-191), in place:
 * every stream buffer z_m [B, n_m, 256] (n_m >= 12) carries three of the four bottleneck sets (vit, vi, vt, it) in rows 4 i ..
 * 4 i + 3, i indexing bottlenecks_map[m] = {0,1,2} / {0,1,3} / {0,2,3}.  New set s of sample b = sum_m weights[s][missing[b]][m] *
 * (stream m's rows of set s), written into every holder's rows.  weights: float[4][4][3] on the device (set, pattern, stream;
 * 0 where a stream does not hold the set or b_out_mean_map does not select it); missing: int64[B] in 0..3 (clamped).
 * _bwd, on the gradient buffers: every holder's rows of set s <- (sum over the holders' rows) * weights[s][missing[b]][m]. */
int mtmp_bottleneck_exchange_multi_fwd(int dtype, void* z_v, void* z_i, void* z_t, int B, int n_v, int n_i, int n_t,
                                       const long long* missing, const float* weights, void* stream);
int mtmp_bottleneck_exchange_multi_bwd(int dtype, void* dz_v, void* dz_i, void* dz_t, int B, int n_v, int n_i, int n_t,
                                       const long long* missing, const float* weights, void* stream);

/* Grouped forms of the fusion layer's row-wise kernels (bf16): the same operation of up to three token streams (vital signs /
 * image / text) in ONE launch -- see mtmp_attn_fwd_grouped.  All pointer / int arrays are HOST arrays of n entries (1 <= n <= 3),
 * scalars are common to the streams; same kernels and results as n calls of the single forms.  The parity (fp32) build keeps
 * the single forms (these return an error for dtype 0).
 *   mtmp_ln_gemm_qkv_grouped        = mtmp_ln_gemm_qkv per stream
 *   mtmp_ln_gemm_signs_grouped      = mtmp_ln_gemm_signs per stream (one dropout seed per stream)
 *   mtmp_gemm_nt_grouped            = mtmp_gemm_nt per stream without gate / row scale (FFN2 + drop2 + residual)
 *   mtmp_gemm_nt_signs_drop_grouped = mtmp_gemm_nt_signs_drop per stream
 *   mtmp_gemm_lnbwd_grouped         = mtmp_gemm_lnbwd per stream, partial slabs only (reduce with mtmp_reduce_batch)
 *   mtmp_gemm_tn_grouped            = mtmp_gemm_tn per stream on the LDS-DMA kernel, partial slabs only: ws[i] holds
 *                                     splits[i] x (N K + N) floats with splits from mtmp_gemm_tn_group_plan (non-zero return:
 *                                     these shapes have no grouped form -- call mtmp_gemm_tn per stream)
 * rows_live (may be NULL as a whole or per entry): rows_live[i] is a DEVICE word holding the rows of stream i that are in use
 * this step (<= M[i]) -- the packed vital-sign stream (mtmp_row_starts), whose buffers and launch grids keep the padded size
 * M[i] so that a captured hipGraph replays for any lengths: rows past it are neither read nor written, workgroups that own
 * none return at once (their gradient partials count as zeros), and mtmp_gemm_tn_grouped's splits share the live rows. */
int mtmp_ln_gemm_qkv_grouped(int dtype, int n, const void* const* x, const float* const* gamma, const float* const* beta,
                             const void* const* w, const float* const* bias, void* const* y, void* const* xn, float* const* stats,
                             float* const* key_norms, const int* M, const int* ldx, float eps, const int32_t* const* rows_live,
                             void* stream);
int mtmp_ln_gemm_signs_grouped(int dtype, int n, const void* const* x, const float* const* gamma, const float* const* beta,
                               const void* const* w, const float* const* bias, void* const* y, void* const* xn, float* const* stats,
                               void* const* signs, const int* M, int N, const int* ldx, float eps, float drop_p,
                               const unsigned* seeds, const unsigned* seed_dev, const int32_t* const* rows_live, void* stream);
int mtmp_gemm_nt_grouped(int dtype, int n, const void* const* a, const void* const* w, const float* const* bias,
                         const void* const* res, void* const* y, const int* M, int N, int K, const int* lda, const int* ldy,
                         const int* ldr, int act, float drop_p, const unsigned* seeds, const unsigned* seed_dev,
                         const int32_t* const* rows_live, void* stream);
int mtmp_gemm_nt_signs_drop_grouped(int dtype, int n, const void* const* a, const void* const* w, void* const* y, const int* M, int N,
                                    const int* lda, const void* const* signs, float gate_scale, float drop_p, const unsigned* seeds,
                                    const unsigned* seed_dev, void* const* a_out, const int32_t* const* rows_live, void* stream);
int mtmp_gemm_lnbwd_grouped(int dtype, int n, const void* const* dy, const void* const* wt, const void* const* z, const int* ldz,
                            const float* const* stats, const float* const* gamma, const void* const* d_res, const int* ldr,
                            void* const* dz, float* const* ws, const int* M, int K, const int* ldy, float eps,
                            const int32_t* const* rows_live, void* stream);
int mtmp_gemm_tn_group_plan(int n, const int* M, int N, int K, int* splits_out);
int mtmp_gemm_tn_grouped(int dtype, int n, const void* const* dy, const void* const* x, float* const* ws, const int* M, int N, int K,
                         const int* ldy, const int* ldx, const int* splits, const int32_t* const* rows_live, void* stream);

/* Deferred reductions: mtmp_gemm_tn with dw == NULL (and db == NULL) and mtmp_gemm_lnbwd with dgamma_dbeta == NULL leave their
 * partial slabs in ws -- [mtmp_gemm_tn_slab_rows(dtype,M,N,K)][N K + N] and [mtmp_gemm_lnbwd_slab_rows(M)][512] floats -- and
 * mtmp_reduce_batch sums up to 8 such slabs in ONE launch: out_a[i][c] = sum_r slab[i][r][c] for c < split[i], the remaining
 * columns go to out_b[i] (may be NULL).  The gradient reductions of one encoder layer's backward (autograd of attention.py:60-62,
 * module.py:74-78, :138-144): seven launches become one.  All arrays are HOST arrays of n entries. */
int mtmp_gemm_tn_slab_rows(int dtype, int M, int N, int K);
int mtmp_gemm_lnbwd_slab_rows(int M);
int mtmp_reduce_batch(const float* const* slab, const int* rows, const long long* cols, float* const* out_a, const long long* split,
                      float* const* out_b, int n, void* stream);

/* ---- The input nodes' backward with ONE closing launch (ABI 6).  The backward of the three stream-input launches and of the event /
 * time embeddings (autograd of mbt_encoder.py:697-729,745 and tri_mbt_vsltcls.py:183-190,216-224) is the tail of a training step,
 * where nothing else runs; each of them used to end in two reduction levels + a multi-tensor copy into the flat gradient, and the
 * parameters the nodes share (ie_time, ie_feat, the bottleneck tokens) in accumulation launches.
 * mtmp_stream_input_bwd_partials = mtmp_stream_input_bwd without the reduction: ws receives
 *   [mtmp_stream_input_slab_rows(B * (nb+1+N))][7][256] floats of partial sums (dgamma, dbeta, dcls, dbott[0..3]).
 * mtmp_tie_time_embed_bwd_partials = mtmp_tie_embed_bwd of events[n][3] / d_out[n][256] AND mtmp_time_embed_bwd of
 *   time_events[n_time][3], whose gradient rows are d_time_a[n_time_a][256] followed by d_time_b[n_time - n_time_a][256], as one
 *   launch: ws receives [mtmp_tie_bwd_slab_rows(n + n_time)][28][256] floats (grads layout of mtmp_tie_embed_bwd).
 * mtmp_reduce_scatter: out[i][c] = sum_{r < rows[i]} src[i][r * ld[i] + c], c < cols[i], for up to 12 column ranges of such slabs
 *   in one launch (src[i] = first column of the range inside its slab, ld[i] = the slab's row length in floats; HOST arrays) --
 *   every destination is a parameter's slice of the flat gradient buffer, or scratch. */
int mtmp_stream_input_slab_rows(int rows);
int mtmp_stream_input_bwd_partials(int dtype, const void* dz, const void* x, const float* cls, const float* gamma, const float* stats,
                                   void* dx, float* ws, int B, int N, int nb, float p, unsigned seed, const unsigned* seed_dev,
                                   const int32_t* row_start, const int32_t* kv_len, void* stream);
/* mtmp_stream_input_bwd_partials of up to three token streams as ONE launch: ws receives the streams' slabs back to back (stream i's
 * mtmp_stream_input_slab_rows(B[i] * (nb[i]+1+N[i])) rows behind those in front of it), so one mtmp_reduce_scatter entry over all
 * rows sums the bottleneck tokens' columns (768..) of all streams.  HOST arrays of n <= 3 entries; row_start / kv_len may be NULL
 * as a whole or per entry. */
int mtmp_stream_input_bwd_grouped(int dtype, int n, const void* const* dz, const void* const* x, const float* const* cls,
                                  const float* const* gamma, const float* const* stats, void* const* dx, float* ws, const int* B,
                                  const int* N, const int* nb, const float* p, const unsigned* seed, const unsigned* seed_dev,
                                  const int32_t* const* row_start, const int32_t* const* kv_len, const void* const* add,
                                  const int* add_L, void* stream);
/* mtmp_stream_input_fwd with `add` [B N / add_L][256] (dtype; may be NULL): row (b N + t) / add_L is added to input token (b, t) in
 * front of the LayerNorm, the sum rounded to dtype -- the time + modality embedding of the token's image / report
 * (tri_mbt_vsltcls.py:216-224) without a torch add launch or a second copy of the tokens; mtmp_stream_input_bwd_grouped takes the
 * same add / add_L (per stream, NULL entries allowed) and recomputes the sum; x then is the tensor WITHOUT the add. */
int mtmp_stream_input_fwd_add(int dtype, const void* x, const float* cls, const float* gamma, const float* beta, const float* pe,
                              const float* bott, void* out, float* stats, int B, int N, int nb, float eps, float p, unsigned seed,
                              const unsigned* seed_dev, const int32_t* row_start, const int32_t* kv_len, const void* add,
                              int add_L, void* stream);
/* out[i][j][:] = sum_{t < L[i]} dx[i][j L[i] + t][:] (256 columns, fp32 accumulation, `dtype` in and out) for n <= 2 tensors in one
 * launch: the gradient of the per-image / per-report time embedding that was added to each of its L tokens
 * (tri_mbt_vsltcls.py:216-224) -- torch autograd's sum over the token axis.  rows[i] = output rows of tensor i.  HOST arrays. */
int mtmp_token_sums(int dtype, int n, const void* const* dx, void* const* out, const int* rows, const int* L, void* stream);
int mtmp_tie_bwd_slab_rows(int n);
int mtmp_tie_time_embed_bwd_partials(int dtype, const float* events, int n, const float* time_events, int n_time, int n_time_a,
                                     const float* params, const void* d_out, const void* d_time_a, const void* d_time_b, float* ws,
                                     void* stream);
int mtmp_reduce_scatter(const float* const* src, const int* rows, const long long* ld, const long long* cols, float* const* out, int n,
                        void* stream);

/* pair[0] <- bit pattern of *value (fp32), pair[1] += 1 (both uint32, device memory): a scalar and a sequence number published
 * together.  The training step copies the pair to pinned host memory right behind its loss (2_train.py:76, trainer.py:128), so the
 * reference's `loss.item()` hands the value over when the forward pass is done instead of when the whole step has drained. */
int mtmp_publish_scalar(const float* value, unsigned* pair, void* stream);

/* Up to 16 device-to-device copies in one launch: dst[i] <- src[i] (bytes[i] bytes, both 16-byte aligned); round16[i] != 0: the
 * buffer holds fp32 values and is written as float(half(x)) -- the fp16 round trip the reference applies to its event / time
 * inputs (trainer.py:26-27, 2_train.py:164).  All arrays are HOST arrays of n entries, read at launch time. */
int mtmp_copy_batch(const void* const* src, void* const* dst, const long long* bytes, const int* round16, int n, void* stream);

/* Batched 2-D transposes in one launch: dst[i] [cols[i]][rows[i]] = src[i] [rows[i]][cols[i]]^T, elements of elem_bytes = 2 | 4.
 * src / dst / rows / cols are HOST arrays of n entries (read at launch time; the pointers travel in the kernel arguments).
 * The K-contiguous backward operands (W2^T, Wqkv^T, W1^T: autograd of attention.py:60-62 / module.py:74-78) of all encoder
 * blocks, rebuilt after every optimizer step. */
int mtmp_transpose_batch(int elem_bytes, const void* const* src, void* const* dst, const int* rows, const int* cols, int n,
                         void* stream);

/* Valid-key counts of the three streams in one launch (mbt_encoder.py:703-714): plain = len + 1 (CLS), stream txt_idx's
 * 3 -> 0; fused = plain + n_bott.  len_*: int64 [B] or NULL (unmasked stream: rows left untouched); out: int32 [2][3][B]. */
int mtmp_stream_lengths(const long long* len_v, const long long* len_i, const long long* len_t, int* out, int B, int n_bott,
                        int txt_idx, void* stream);
/* The frozen image encoder on a batch in which some samples have no image.  Their encoder output is read by nothing (the
 * bottleneck exchange gives the image stream weight 0 for missing_num 2 / 3, mbt_encoder.py:764-779; the reference pushes a zero
 * image through all of swin_transformer.py:503-654 for them).  mtmp_image_slots moves the present images to the front of the
 * encoder's batch and tabulates the rows in use per encoder stage; the *_live forms of the encoder's kernels take one word of that
 * table as `rows_live` (DEVICE pointer, may be NULL = all rows): buffers and grids keep the size of the whole batch, so a captured
 * hipGraph replays for any number of present images; rows past the live ones are neither read nor written.
 *   pattern: int64[B] device, the step's missing_num ids; sample b has an image iff 0 <= pattern[b] < present_below (2 for the
 *   tri-modal ids: 0 all three, 1 vslt + image).  out: int32[2 B + 16] device:
 *     out[i], i < B            slot i of the encoder's batch works on image out[i] (present images first, in batch order)
 *     out[B + b]               the slot of sample b's image, or B (a slot the caller keeps zero) when it has none
 *     out[2 B]                 number of present images
 *     out[2 B + 1 + 5 p + s]   rows in use at stage s = 0..3 (hw0 >> 2 s rows per image; s = 4: one row per image), p = 0: the whole
 *                              batch, p = 1 / 2: its first / second half of B / 2 slots (the encoder's two-stream tail)
 * mtmp_swin_stem_fwd_live: `order` (= out, may be NULL) maps slot -> image.  mtmp_swin_window_attn_live: rows_live counts token
 * rows (live images = *rows_live / (H W)). */
int mtmp_image_slots(const long long* pattern, int present_below, int32_t* out, int B, int hw0, void* stream);
int mtmp_swin_stem_fwd_live(int dtype, const float* img, const float* w, const float* bias, const float* ln_w, const float* ln_b,
                            void* out, int n_img, int H, int W, const int32_t* order, const int32_t* rows_live, void* stream);
int mtmp_layernorm_rows_live(int dtype, const void* x, const float* w, const float* b, void* y, long long rows, int C, float eps,
                             int merge, int H, int W, const int32_t* rows_live, void* stream);
int mtmp_swin_ln_linear_live(int dtype, const void* x, const float* ln_w, const float* ln_b, const void* w, const float* bias,
                             void* y, long long M, int C, int N, float eps, const int32_t* rows_live, void* stream);
int mtmp_swin_mlp_live(int dtype, const void* x, const float* ln_w, const float* ln_b, const void* w1, const float* b1,
                       const void* w2, const float* b2, const float* row_scale, int rows_per_scale, void* y, long long M, int C,
                       float eps, const int32_t* rows_live, void* stream);
int mtmp_swin_window_attn_live(int dtype, const void* qkv, const void* table, void* out, int n_img, int H, int W, int C, int heads,
                               int shift, float scale, const int32_t* rows_live, void* stream);

/* ---- Backward of the image encoder's building blocks (ABI 5): the sibling models that TRAIN the Swin-T encoder -- the reference
 * calls self.img_encoder(img) without torch.no_grad() in builder/models/8_missing_models/bi_vsltimg_mbt_v1.py:203-206,
 * tri_mbt_v2.py:208-211, tri_mbt_vmulti.py:145 -- replace torch autograd of builder/models/src/swin_transformer.py as follows
 * (the GEMM-shaped parts, dX = dY W and dW = dY^T X, run on mtmp_gemm_nt / mtmp_gemm_tn):
 *
 * mtmp_layernorm_rows_bwd: autograd of nn.LayerNorm(C, eps) as mtmp_layernorm_rows computes it (:428-449 norm1 / norm2, :34-85
 *   the patch-merging norm, :611 the final norm).  x, dy, dx [rows, C] (dtype), w float[C]; slab float[slab_rows][2][C] receives one
 *   row of partial (dw | db) sums per workgroup -- the caller adds the rows (mtmp_layernorm_rows_bwd_slab_rows tells how many).
 * mtmp_gelu_fwd / mtmp_gelu_bwd: nn.GELU of the MLP (:437-439) as its own pass, and dx = dy GELU'(x); n % 8 == 0.
 * mtmp_swin_window_attn_bwd: autograd of mtmp_swin_window_attn (:115-225).  dout [n,H,W,C] -> dqkv [n,H,W,3C] (every element
 *   written once; H, W multiples of 7) and dtab float[4][heads][64][64], the gradient of the additive table, which the caller
 *   ZEROES first (float atomics).  shift > 0 with H == 7 or W == 7 is refused, as in the forward. */
int mtmp_layernorm_rows_bwd_slab_rows(long long rows, int C);
int mtmp_layernorm_rows_bwd(int dtype, const void* x, const float* w, const void* dy, void* dx, float* slab, long long rows, int C,
                            float eps, void* stream);
int mtmp_gelu_fwd(int dtype, const void* x, void* y, long long n, void* stream);
int mtmp_gelu_bwd(int dtype, const void* x, const void* dy, void* dx, long long n, void* stream);
int mtmp_swin_window_attn_bwd(int dtype, const void* qkv, const void* table, const void* dout, void* dqkv, float* dtab, int n_img,
                              int H, int W, int C, int heads, int shift, float scale, void* stream);

/* ---- Shifted-window attention on maps of ANY size (swin_transformer.py:150-225 pads the normalised map with zeros to whole 7x7
 * windows in front of the qkv projection, rolls the PADDED map and crops the result): the padded map never exists in memory.
 * qkv / out / dout / dqkv stay [n,H,W,3C | C] on the un-padded, un-shifted map.  The window grid covers Hp x Wp = ceil(H/7) 7 x
 * ceil(W/7) 7 and the cyclic shift is modulo Hp / Wp; a token whose pixel lies at y >= H or x >= W is a PAD token: its q / k / v
 * are qkv_bias (float[3C]) rounded to `dtype`, made in registers; it is an ordinary (unmasked) key; its output row is not
 * stored.  The caller passes shift 0 for a padded map of one window; one axis of a single window and the other of several is
 * refused.  rows_live as in mtmp_swin_window_attn_live (may be NULL).
 * mtmp_swin_window_attn_pad_bwd: every element of dqkv is written once; dtab as in mtmp_swin_window_attn_bwd (caller zeroes;
 * pad keys' columns included).  dbias float[3C], which the caller ZEROES first (float atomics): the pad tokens' dk and dv, i.e.
 * THEIR share of the gradient of the qkv bias (a pad token's dout is zero, so its dq is: dbias[0..C) stays zero) -- the real
 * tokens' share is the column sum of dqkv, which the backward of the projection forms as ever.
 * H and W multiples of 7: both entries run the kernels of mtmp_swin_window_attn_live / _bwd themselves (bit-identical; dbias is
 * left untouched). */
int mtmp_swin_window_attn_pad(int dtype, const void* qkv, const float* qkv_bias, const void* table, void* out, int n_img, int H,
                              int W, int C, int heads, int shift, float scale, const int32_t* rows_live, void* stream);
int mtmp_swin_window_attn_pad_bwd(int dtype, const void* qkv, const float* qkv_bias, const void* table, const void* dout,
                                  void* dqkv, float* dtab, float* dbias, int n_img, int H, int W, int C, int heads, int shift,
                                  float scale, void* stream);

/* Attention half of a Swin block in ONE launch (ABI 4): out = x + row_scale[image] * (proj(window_attention(qkv(norm1(x)))) + b_proj).
 * Replaces builder/models/src/swin_transformer.py:428-449 (norm1, attn, stochastic_depth, residual) with :115-225
 * (shifted_window_attention) for maps that are multiples of the 7x7 window.  bf16 only (dtype MTMP_BF16); x, out [n_img, H, W, C]
 * (out != x), C = 96 or 192, heads = C / 32; wqkv [3C][C], wproj [C][C] bf16; ln_w, ln_b [C], bqkv [3C], bproj [C] fp32; table
 * [4 window types][heads][64][64] bf16 as mtmp_swin_window_attn's, but with the KEY columns of every group of 16 keys in
 * accumulator-register order: position 8 h + j (h = 0, 1; j = 0..7) of group g holds key 16 g + (j & 3) + 8 (j >> 2) + 4 h.
 * row_scale: fp32[n_img] (row-mode StochasticDepth) or NULL; rows_live: NULL or the device word of mtmp_image_slots.
 * shift > 0 with H == 7 or W == 7 is refused (an axis of one window is not shifted, :155-160). */
int mtmp_swin_attn_block(int dtype, const void* x, const float* ln_w, const float* ln_b, float eps, const void* wqkv,
                         const float* bqkv, const void* table, const void* wproj, const float* bproj, const float* row_scale,
                         void* out, int n_img, int H, int W, int C, int heads, int shift, float scale, const int32_t* rows_live,
                         void* stream);
/* mtmp_swin_attn_block on a map of ANY size, by the rules of mtmp_swin_window_attn_pad: the window grid covers Hp x Wp = ceil(H/7) 7
 * x ceil(W/7) 7, the cyclic shift is modulo Hp / Wp, x / out stay [n_img, H, W, C].  A token whose pixel lies at y >= H or x >= W is
 * a PAD token: a zero row BEHIND norm1 (swin_transformer.py:150-152 pads the normalised map), so its q / k / v are bqkv; it is an
 * ordinary (unmasked) key; nothing is read or stored at its pixel.  Same arguments and table as mtmp_swin_attn_block.  The caller
 * passes shift 0 for a padded map of one window; one axis of a single window and the other of several is refused.  H and W
 * multiples of 7: the kernel of mtmp_swin_attn_block itself (bit-identical). */
int mtmp_swin_attn_block_pad(int dtype, const void* x, const float* ln_w, const float* ln_b, float eps, const void* wqkv,
                             const float* bqkv, const void* table, const void* wproj, const float* bproj, const float* row_scale,
                             void* out, int n_img, int H, int W, int C, int heads, int shift, float scale, const int32_t* rows_live,
                             void* stream);
int mtmp_gemm_nt_live(int dtype, const void* a, const void* w, const float* bias, const void* res, void* y, int M, int N, int K,
                      int lda, int ldy, int ldr, int act, float drop_p, unsigned seed, const unsigned* seed_dev, const void* gate,
                      float gate_scale, const float* row_scale, int rows_per_scale, const int32_t* rows_live, void* stream);

/* Row map of a PACKED token stream ("skip padded key tiles and padded query rows"; the reference pads every sample to
 * the batch maximum, trainer.py:41-42, and masks keys, utils.py:79-125): out[b] = sum of min(max(kv_len[0..b), 0), n_max) =
 * sample b's first row when the samples' valid rows are stored back to back; out[B] = the rows in use (the `rows_live` word of
 * the grouped kernels); out[B + 1 .. 2 B + 1) = the order in which the attention kernels walk the samples of a packed stream
 * (ranked by length, dealt round-robin over the eight XCD chunks of their grids).  kv_len: int32[B] device (a fused count of
 * mtmp_stream_lengths); out: int32[2 B + 1] device -- the `row_start` argument of the packed forms is this whole array. */
int mtmp_row_starts(const int32_t* kv_len, int32_t* out, int B, int n_max, void* stream);

/* ---- Chest X-ray input chain (additive; ABI stays 6): the reference's loader runs, per image and on CPU workers, PIL's
 * ImageOps.equalize and one of the torchvision chains of builder/data/dataset_new.py:91-160 (antialiased bilinear Resize,
 * RandomAffine, CenterCrop, ToTensor; :2094-2096, :2110-2112).  All of it is integer arithmetic in PIL and is reproduced here bit
 * for bit from the decoded uint8 pixels.
 *   pixels: uint8 device buffer, the batch's images back to back at arbitrary byte offsets.
 *   desc:   int32 [n][24] device, one row per image: 0 source byte offset, 1 h, 2 w, 3 Rh, 4 Rw (resized map), 5 / 6 / 7 word offset
 *           of the horizontal bounds table, of the horizontal weights, taps per weight row (ksize), 8 / 9 / 10 the same for the
 *           vertical pass, 11 flags (bit 0: apply the affine map), 12..17 the 16.16 words a0..a5 of PIL's nearest-neighbour affine
 *           (xin = (a2 + a0 x + a1 y) >> 16, yin = (a5 + a3 x + a4 y) >> 16), 18 / 19 crop top / left, 20 output slot, 21 byte offset
 *           of the resized map in `scratch`, 22..23 zero.
 *   tables: int32 device; per axis bounds [out][2] = (first source index, taps) and weights [out][ksize] with 22 fractional bits
 *           (PIL's precompute_coeffs / normalize_coeffs_8bpc), built on the host.
 * mtmp_cxr_hist: hist uint32 [n][256] += the images' histograms (the caller ZEROES it; integer atomics, order-independent);
 *   max_pixels = the largest h w of the batch.
 * mtmp_cxr_resize: scratch uint8 <- equalised (ImageOps.equalize's table from hist, saturated at 255) and resized maps, horizontal
 *   pass rounded to uint8 before the vertical one.  max_rh / max_rw: the largest Rh / Rw; lds_rows: the most source rows any tile of
 *   32 resized rows reads (<= 960), i.e. the maximum over images and tiles [r0, r1) of vbounds[r1-1].first + vbounds[r1-1].taps -
 *   vbounds[r0].first.  The entry point cannot see the tables: a smaller lds_rows than that is a broken precondition (the kernel
 *   then writes past its LDS rows; the output is undefined).  builder/data/cxr_transform.py computes it with the tables.
 * mtmp_cxr_affine_crop: out float [n_slots][S][S]; slot_map int32 [n_slots] = image of the slot or -1 (written as zeros).  Per
 *   pixel: crop offset, affine map if flagged, fetch from scratch (0 outside the map), float / 255 with IEEE division. */
int mtmp_cxr_hist(const uint8_t* pixels, const int32_t* desc, uint32_t* hist, int n, int max_pixels, void* stream);
int mtmp_cxr_resize(const uint8_t* pixels, const int32_t* desc, const int32_t* tables, const uint32_t* hist, uint8_t* scratch,
                    int n, int max_rh, int max_rw, int lds_rows, void* stream);
int mtmp_cxr_affine_crop(const uint8_t* scratch, const int32_t* desc, const int32_t* slot_map, float* out, int n_slots, int S,
                         void* stream);

/* ---- The random chains of the chest X-ray input (additive; ABI stays 6): --image-train-type random = RandomResizedCrop(S, scale
 * (0.8, 1.1), ratio (3/4, 4/3)), randaug = RandAugment() in front of it (builder/data/dataset_new.py:60-89), behind the loader's
 * equalisation.  Per image: equalise, two ops, crop box (i, j, ch, cw), PIL's resize of the box to S x S, / 255 -- bit for bit what
 * PIL computes (csrc/image_aug.hip states each rule).  pixels / tables / slot_map as above; the histograms of the source pixels come
 * from mtmp_cxr_hist with a desc row per image that holds words 0..2.
 *   aug:     int32 [max(n, 1)][64] device, one row per image: 0 source byte offset, 1 h, 2 w, 3 output slot, 4 byte offset of the
 *            image's map inside each scratch half (a multiple of 16), 5..8 crop box i, j, ch, cw, 9 / 10 / 11 word offset of the
 *            horizontal bounds table, of the weights, taps per weight row of the (cw -> S) resize, 12 / 13 / 14 the same for
 *            (ch -> S); 16 + 8 k (k = 0, 1): stage k, the RandAugment op k + 1 when it writes a map: kind (0 none, 1 affine, 2
 *            Sharpness), then the 16.16 words a0..a5 or the float32 bits of the blend factor; 32 + 8 r (r = 0, 1: stage r, r = 2: the
 *            resize): what reader r reads: base (0 source pixels, 1 + k map of stage k), number of pending table ops (0..3), their
 *            three codes (1 Equalize, 2 Brightness, 3 Contrast, 4 Posterize, 5 Solarize, 6 AutoContrast), their three parameters
 *            (float32 bits of the blend factor; Posterize's mask; Solarize's threshold rounded up); every other word zero.
 *   hist:    uint32 [3][n][256] device: [0] the source pixels' histograms (mtmp_cxr_hist), [1 + k] those of the maps of stage k,
 *            added by mtmp_cxr_aug_stage (the caller ZEROES all three; integer atomics, order-independent).
 *   scratch: uint8 [2][half_bytes] device, 16-byte aligned, half_bytes a multiple of 16: map of stage k of image m at
 *            k half_bytes + aug[m][4], h w bytes.
 * mtmp_cxr_aug_stage: runs stage `stage` (0, then 1) of every image that has one: reads its base map through the composed pending
 *   table, writes its map (0 outside the source for the affine kind) and that map's histogram.  max_pixels = the largest h w.  A
 *   batch in which no image has stage k needs no launch for k.  The affine words must keep |a2| + |a0| w + |a1| h and the same for
 *   a3..a5 below 2^31 (the host checks).
 * mtmp_cxr_crop_resize: out float [n_slots][S][S] <- for every slot with an image (slot_map >= 0) the crop box of its last map through
 *   the pending table, resized in two passes (horizontal pass rounded to uint8), float / 255 with IEEE division; zeros for the
 *   other slots.  n may be 0 (no image: all zeros; hist and scratch are then not read but must be non-null).  lds_rows: the most
 *   box rows any tile of 32 output rows reads (<= 960), the maximum over images and tiles [r0, r1) of vbounds[r1-1].first +
 *   vbounds[r1-1].taps - vbounds[r0].first; with a smaller value than that the tile's rows past lds_rows are left out (wrong
 *   pixels, no access outside the LDS rows).  builder/data/cxr_transform.py computes it with the tables. */
int mtmp_cxr_aug_stage(const uint8_t* pixels, const int32_t* aug, uint32_t* hist, uint8_t* scratch, int n, int max_pixels,
                       long long half_bytes, int stage, void* stream);
int mtmp_cxr_crop_resize(const uint8_t* pixels, const uint8_t* scratch, const int32_t* aug, const int32_t* tables,
                         const uint32_t* hist, const int32_t* slot_map, float* out, int n, int n_slots, int S, long long half_bytes,
                         int lds_rows, void* stream);

/* ---- Baseline greyscale JPEG decoding (additive; ABI stays 6): the reference's loader opens every image with PIL's Image.open
 * (builder/data/dataset_new.py:2094); the files are what PIL wrote (1_mimic_cxr_preprocess.py:81-82): 8-bit, one component,
 * baseline sequential (SOF0), Huffman coded.  The host (builder/data/jpeg.py) parses the markers and REMOVES the stuffed FF 00
 * zero bytes and the RSTn markers from the entropy-coded data; the device does the rest -- Huffman decoding, integer
 * dequantisation, libjpeg's jpeg_idct_islow, the range limit -- and equals PIL bit for bit.  The coefficient buffer is int16
 * (DC absolute, natural order) and holds the UNdequantised values: the quantiser product is part of mtmp_jpeg_idct.
 *   streams: uint8 device buffer, every segment's de-stuffed bytes (segments of an image back to back, images back to back).
 *   desc:    int32 [n][16] device, one row per image: 0 byte offset of its first segment in `streams`, 1 its first row in `segs`,
 *            2 its number of segments, 3 h, 4 w, 5 blocks per row = ceil(w / 8), 6 blocks = ceil(h / 8) ceil(w / 8), 7 byte offset
 *            of its first pixel in `pixels` (row stride w, any alignment), 8 word offset of its quantisation table in `tables`
 *            (64 words, natural order), 9 / 10 word offset of its DC / AC decode table, 11 its first block in `coef`, 12 restart
 *            interval in blocks (0: none), 13..15 zero.
 *   segs:    int32 [n_seg][4] device, one row per restart segment: 0 byte offset in `streams`, 1 bytes (<= 2^22), 2 image, 3 its
 *            first block within the image.  A segment holds min(restart interval, blocks - first block) blocks (all of them
 *            without an interval); every segment starts with a zero DC predictor.
 *   tables:  int32 device.  A decode table is 1316 words: look[1024], indexed by the next 10 bits of the stream: (code length << 8)
 *            | symbol, 0 where the code is longer or there is none; maxcode[18], indexed by the code length: the largest code of
 *            that length, -1 for none, [17] = 0x7fffffff; valoff[18]: index of that length's first symbol minus its first code;
 *            huffval[256]: the symbols in code order.  Tables are shared between images that carry the same payload.
 *   status:  int32 [n] device, ZEROED by the caller: bit 0 a segment did not yield its block count (truncated or corrupt data),
 *            bit 1 a segment has more subsequences than the launch has lanes, bit 2 the image's segments do not cover its blocks.
 * mtmp_jpeg_entropy: coef int16 [blocks of the batch][64], ZEROED by the caller, <- the coefficients.  One workgroup per segment,
 *   one lane per subsequence of subseq_bits bits (0: one lane decodes the whole segment); max_seg_bytes = the largest segment
 *   (at most 1024 subsequences; the entry refuses more); stage_bytes (0..32768): dynamic LDS of a workgroup, a segment of at
 *   most that many bytes is copied into it and decoded from there, a larger one is read from global memory.  The lanes find their entry states by decoding in rounds inside the
 *   workgroup (csrc/jpeg.hip); rounds: int32 [n_seg] or NULL, receives the number of rounds that moved an exit state.  Every loop
 *   is bounded by the segment's bits and the lane count: a truncated or corrupt stream ends and sets its image's status.  Nothing
 *   outside the image's blocks of coef is written.
 * mtmp_jpeg_idct: pixels <- the decoded images (only bytes of rows < h, columns < w at the image's offset are written); an image
 *   whose status word is set is written as zeros.  max_blocks = the largest block count of an image. */
int mtmp_jpeg_entropy(const uint8_t* streams, const int32_t* desc, const int32_t* segs, const int32_t* tables, int16_t* coef,
                      int32_t* status, int32_t* rounds, int n_seg, int max_seg_bytes, int subseq_bits, int stage_bytes, void* stream);
int mtmp_jpeg_idct(const int16_t* coef, const int32_t* desc, const int32_t* tables, const int32_t* status, uint8_t* pixels, int n,
                   int max_blocks, void* stream);

/* ---- Chest X-rays from a device-resident JPEG store (additive; ABI stays 6): builder/data/cxr_store.py parses every file once
 * and keeps its de-stuffed bytes on the device; the entry state of every subsequence of every restart segment -- which
 * mtmp_jpeg_entropy finds again for every batch, in rounds -- is a property of the file and is found once, into the SYNC TABLE.
 * A batch is then decoded by one pass over a flat grid of subsequences.
 *   streams: uint8 device buffer, the de-stuffed segments of ALL images back to back (may exceed 2^31 bytes).
 *   An image row is a `desc` row of mtmp_jpeg_entropy (int32 [16]) with two more words: 13 the image's OWN subsequence length in
 *            bits (a multiple of 32 with at most 1024 subsequences in its largest segment), 14 its number of sync rows (the sum
 *            over its segments of max(ceil(8 bytes / word 13), 1)).  Word 1 is its first row in the store's `segs`.  Its two
 *            64-bit offsets live beside it in
 *   wide:    int64 [n][2]: 0 the byte offset of the image's first segment in `streams` (word 0 of the row is then unused),
 *            1 its first row in `sync`.  Everything inside one image is 32-bit.
 *   segs:    (store form) int32 [n_segs][4] device, one row per restart segment, all relative to its image: 0 byte offset behind
 *            the image's first byte, 1 bytes (<= 2^22), 2 its first block within the image, 3 its first sync row behind the
 *            image's first.
 *   sync:    int32 [n_sync][4] device, 16-byte aligned, one row per subsequence, segments and images in order: 0 the entry state
 *            (bit position within the segment << 6) | coefficient index (0: a DC code is next) of the first symbol that starts
 *            at or behind the subsequence's nominal start (0 for the first subsequence of a segment), 1 the block that symbol
 *            belongs to, relative to the segment's first block, 2 the DC predictor at that point, 3 the segment, relative to the
 *            image's first -- a decoder lane finds its segment row through it without a search.
 * mtmp_jpeg_sync_points: the build pass over one CHUNK of images (the store is built chunk by chunk so that every offset of a
 *   launch is 32-bit): the launch shape and the rounds of mtmp_jpeg_entropy (the same kernel body), each lane writing its sync row
 *   in place of coefficients.  streams / sync / status point at the chunk's first byte / sync row / image; desc: int32 [images of
 *   the chunk][16] with word 0 the image's byte offset and word 1 its first segment row WITHIN THE CHUNK; segs: int32
 *   [n_seg][4] in the form of mtmp_jpeg_entropy (offset within the chunk, bytes, image within the chunk, first block); sync0:
 *   int32 [n_seg], every segment's first sync row within the chunk; max_lanes: the most subsequences of a segment (<= 1024);
 *   n_sync: sync rows of the chunk (a row at or behind it is not written); status as for mtmp_jpeg_entropy, ZEROED by the caller.
 * mtmp_jpeg_store_entropy: the per-batch decoder.  desc: int32 [n][16], the store's rows of the batch's images with word 7
 *   (pixel offset) and word 11 (first block in `coef`) filled in -- also what mtmp_jpeg_idct reads next; wide: int64 [n][2],
 *   8-byte aligned, their rows of the store's `wide`; prefix: int32 [n + 1], exclusive prefix sum of word 14 over the batch;
 *   total_lanes = prefix[n] (the host's copy).  256 lanes per workgroup, lane g decodes subsequence g - prefix[b] of batch image
 *   b (found by bisection of `prefix`): ONE pass from its sync row's entry state up to the first symbol at or behind its
 *   subsequence's end, into coef (ZEROED by the caller) at the image's blocks.  No rounds, no scan, no status: the build refused
 *   every image that does not decode.  stream_bytes / n_segs / n_sync / table_words: the sizes of streams / segs / sync /
 *   tables; a lane whose rows point outside any of them writes nothing, and nothing outside the image's blocks of coef is
 *   written. */
int mtmp_jpeg_sync_points(const uint8_t* streams, const int32_t* desc, const int32_t* segs, const int32_t* tables,
                          const int32_t* sync0, int32_t* sync, int32_t* status, int n_seg, int max_lanes, long long n_sync,
                          int stage_bytes, void* stream);
int mtmp_jpeg_store_entropy(const uint8_t* streams, const int32_t* segs, const int32_t* sync, const int32_t* tables,
                            const int32_t* desc, const long long* wide, const int32_t* prefix, int16_t* coef, int n,
                            int total_lanes, long long stream_bytes, long long n_segs, long long n_sync, long long table_words,
                            void* stream);

/* ---- TIE event windows from a device-resident event store (additive; ABI stays 6): the reference builds every window on the
 * host (builder/data/dataset_new.py:1969-2030, restated by builder/data/tie_dataset.py tie_window).  Here the data set is stored
 * once (builder/data/tie_store.py: CSR over patients -> hours -> events) and a window is a row of `desc`; ONE launch writes the
 * batch in the layout mtmp_tie_embed_packed_fwd reads, bit-identical to tie_window (+ the trainer's fp16 rounding).
 *   ev_time / ev_val / ev_feat: float64 / float32 / uint8 [n_events], the events of all hours back to back (time, normalised
 *            value, feature index); may be NULL when n_events is 0.
 *   norm:    float32 [n_hours][18], the normalised carry-forward table; delta: float64 [n_hours][18], hours since measurement;
 *   hour_min: float64 [n_hours], the earliest event time of the hour (+inf without one).
 *   desc:    int64 [B][8] device, one row per window: 0 its first event, 1 its number of events (before the TIE-len cut), 2 the
 *            hour whose norm / delta rows make the initial rows, 3 its first hour and 4 its number of hours after the trimming,
 *            5 the mask of the features that come as initial rows (bit f = feature f), 6 t0, the first hour of the trimmed
 *            window relative to the admission, 7 the (moved) prediction hour.
 *   cu_seqlens: int32 [B + 1] device, prefix sums of the lengths AFTER the cut (row b of the batch has cu[b+1] - cu[b] rows:
 *            its initial rows in feature order, then its events).  max_len / total_rows: the host's copy of the largest length
 *            and of cu[B] (they size the launch; no device value is waited for).
 *   Row r < popcount(mask): time = (-delta[f] + (t0 + 1)) - shift, value = norm[f], index = f for the r-th set bit f; row r beyond:
 *   event first + r - popcount(mask), time - shift.  shift = desc[7] for realtime == 1, otherwise the minimum time over all rows
 *   of the uncut window (recomputed per workgroup from the initial rows and hour_min).  float64 arithmetic, then float32, then
 *   with round_fp16 float32 -> fp16 -> float32.
 *   padded == 0: out float32 [out_rows][3], rows cu[B] .. out_rows - 1 are written as zeros (out_rows >= total_rows);
 *   padded == 1: out float32 [B][t_pad][3], rows behind a sample's length are written as zeros (t_pad >= max_len).
 *   A descriptor row that points outside the store's arrays has its rows written as zeros (both forms), not read out of bounds. */
int mtmp_tie_window_gather(const double* ev_time, const float* ev_val, const uint8_t* ev_feat, const float* norm,
                           const double* delta, const double* hour_min, long long n_events, long long n_hours,
                           const long long* desc, const int32_t* cu_seqlens, float* out, int B, int max_len, int t_pad,
                           long long total_rows, long long out_rows, int padded, int realtime, int round_fp16, void* stream);

/* ---- hourly carry-forward windows and their embedding, --vslt-type carryforward (additive; ABI stays 6).  The reference's loader
 * cuts a [window_size][16] table of hourly carry-forward values per sample out of the patient's normalised table and pads it with
 * zero rows (builder/data/dataset_new.py:2006-2011); its model embeds every row by Linear(16, 256) -> nn.LayerNorm -> ReLU
 * (tri_mbt_vsltcls.py:51-57,179-181).  The table is `norm` of the event store above: a window is a row of `desc`.
 *   mtmp_hourly_window_gather: desc int64 [B][2] device = (first_row, n_rows); out float32 [B][W][F].  Row r < n_rows of sample b
 *   is norm[first_row + r][f_j], f_j = the j-th set bit of keep_bits (popcount(keep_bits) == F <= 18, else MTMP_ERR_ARG); with
 *   round_fp16 float32 -> fp16 -> float32; every other row zeros.  ONE launch writes every element (no memset).  A descriptor row
 *   with first_row < 0, n_rows < 0, n_rows > W or first_row + n_rows > n_hours has its sample written as zeros, not read out of
 *   bounds. */
int mtmp_hourly_window_gather(const float* norm, long long n_hours, const long long* desc, float* out, int B, int W, int F,
                              unsigned keep_bits, int round_fp16, void* stream);
/*   mtmp_hourly_embed_fwd: out[n][256] = ReLU(LN(x[n][F] . w[256][F]^T + b)) in `dtype`, 1 <= F <= 18; w = nn.Linear.weight as
 *   stored; params float [3][256] = Linear bias, LayerNorm weight, LayerNorm bias; fp32 arithmetic, nn.LayerNorm semantics (biased
 *   variance, eps 1e-5 inside the root).  One launch.
 *   mtmp_hourly_embed_bwd: grads float [F + 3][256] overwritten = dW^T rows, db, dgamma, dbeta (x is data: no gradient).  Nothing
 *   is saved by the forward but x: the pre-activation, the statistics and the ReLU gate are recomputed.  Two launches: per-workgroup
 *   partial slabs in ws (mtmp_hourly_embed_bwd_ws_floats(n, F) floats), then their sum in a fixed order -- no float atomics,
 *   bit-identical between runs. */
int mtmp_hourly_embed_fwd(int dtype, const float* x, const float* w, const float* params, void* out, int n, int F, void* stream);
int mtmp_hourly_embed_bwd_ws_floats(int n, int F);
int mtmp_hourly_embed_bwd(int dtype, const float* x, const float* w, const float* params, const void* d_out, float* grads,
                          float* ws, int n, int F, void* stream);

/* ---- report token embeddings from a device-resident embedding store (additive; ABI stays 6): the reference reads a report's
 * [len][768] BioBERT embeddings from an h5 file per sample, appends zeros up to [128][768] and stacks the batch on the host
 * (builder/data/dataset_new.py:2135-2155).  Here every report is stored once (builder/data/report_store.py: CSR over reports ->
 * token rows) and a sample is a row of `desc`; ONE launch writes the batch the text projection reads.
 *   emb:   [total_tokens][W] in emb_dtype (MTMP_F32 | MTMP_BF16), the reports' token rows back to back; may be NULL when
 *          total_tokens is 0.
 *   desc:  int64 [B][2] device, one row per sample: 0 its first token row in emb, 1 its number of tokens n (0: a missing report).
 *   out:   [B][L][W] in out_dtype.  Row t < n of sample b is row desc[b][0] + t of emb; every other row is written as zeros (no
 *          memset is needed in front) and reads nothing from emb.  MTMP_F32 -> MTMP_BF16 rounds to nearest even with the bits of
 *          torch's .to(torch.bfloat16) (a NaN stays a NaN); MTMP_BF16 -> MTMP_F32 is exact; equal types copy.
 *   W % 8 == 0 (a row is a whole number of 16-byte pieces in either type: every global access is 16 bytes per lane); emb and out
 *   16-byte aligned.  A descriptor row with first < 0, n < 0, n > L or first + n > total_tokens has its sample written as zeros,
 *   not read out of bounds. */
int mtmp_report_gather(const void* emb, int emb_dtype, long long total_tokens, const long long* desc, void* out, int out_dtype,
                       int B, int L, int W, void* stream);

/* ---- token-id reports (--berttype bert) from a device-resident store, the embedding lookup and its gradient (additive; ABI
 * stays 6).  The reference's loader puts a BOS (2) in front of a report's ids, trims, appends an EOS (3), pads and replaces every
 * 1 by 0 (builder/data/dataset_new.py:2157-2175, clinical_note_transform :186-192); its model looks the ids up in a trained
 * nn.Embedding(30000, 256).  builder/data/report_store.py (TokenReportStore) keeps every report's ids once, CSR.
 *
 * mtmp_report_ids_gather: ONE launch writes out int32 [B][L], every element (no memset in front).
 *   ids:   int32 [total], the reports' ids back to back; may be NULL when total is 0.
 *   desc:  int64 [B][2] device, one row per sample: 0 its first id in `ids`, 1 its number of ids n, UNTRIMMED (0: missing).
 *   out:   with k = min(n, L - 2): [2, t_0 .. t_{k-1}, 3, 0 .. 0], every t_i == 1 written as 0; all zeros when n == 0.
 *   L >= 3; out 16-byte aligned.  A row with first < 0, n < 0 or first + n > total has its sample written as zeros.
 *
 * mtmp_token_embed_fwd: out[t] = table[ids[t]], t < T; table [V][D] and out [T][D] in MTMP_F32 | MTMP_BF16 each.  MTMP_F32 ->
 *   MTMP_BF16 rounds to nearest even with the bits of torch's .to(torch.bfloat16); MTMP_BF16 -> MTMP_F32 is exact; equal types
 *   copy.  Every lane moves 16-byte pieces.  An id outside [0, V) gives a zero row and reads nothing.  D == 256 only.
 *
 * mtmp_token_embed_bwd: dw[v] = sum over {t : ids[t] == v} of dy[t] in float32; dy [T][D] in dy_dtype, dw float32 [V][D].
 *   Only the rows v that have a token are WRITTEN (overwritten, not accumulated into); the caller hands over a zeroed dw if it
 *   wants zeros elsewhere.  No float atomics: the order of every sum depends on the positions t alone -- rows in ascending t
 *   inside chunks of mtmp_token_embed_bwd_chunk() rows of an id's position list, then the chunks' partial sums in chunk order --
 *   so equal inputs give equal bits.  Ids outside [0, V) contribute nothing.  Two launches.  workspace: device memory of
 *   mtmp_token_embed_bwd_workspace(T, V) bytes, 16-byte aligned, contents irrelevant before and after.  D == 256 only;
 *   T <= 2^24. */
int mtmp_report_ids_gather(const int32_t* ids, long long total, const long long* desc, int32_t* out, int B, int L, void* stream);
int mtmp_token_embed_fwd(const int32_t* ids, long long T, const void* table, int table_dtype, void* out, int out_dtype, int V,
                         int D, void* stream);
long long mtmp_token_embed_bwd_workspace(long long T, int V);
int mtmp_token_embed_bwd_chunk(void);
int mtmp_token_embed_bwd(const int32_t* ids, long long T, const void* dy, int dy_dtype, float* dw, void* workspace, int V, int D,
                         void* stream);

/* ---- the device-side evaluator of a validation pass (additive; ABI stays 6).  builder/utils/device_evaluator.py owns the state:
 *   pred float32 [capacity], tgt uint8 [capacity], logit float32 [capacity] (optional), ctr int64 [4] = predictions stored,
 *   batches added, predictions dropped for lack of room, reserved; loss_sum float64 [1].  capacity <= 2^24.
 *
 * mtmp_eval_append: ONE launch of one workgroup per validation batch, capturable in a hipGraph: the cursor is ctr[0], read on the
 *   device.  values / targets: float32 [count].  mode 0: values are logits, the stored prediction is 1 / (1 + exp(-x)) evaluated in
 *   float64 and rounded once to float32 (and the raw logit goes to `logit` when that is given); mode 1: values are probabilities,
 *   stored as they are.  Both then: NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX (torch.nan_to_num), -0.0 -> +0.0.  The target is
 *   stored as t != 0.  Element i goes to slot ctr[0] + i when that is below capacity, otherwise it is dropped and counted in
 *   ctr[2]; nothing is written out of range.  loss (may be NULL): the batch's float32 mean loss on the device; with it
 *   loss_sum += (double)*loss and ctr[1] += 1.
 *
 * mtmp_eval_metrics: once per pass.  n is the HOST's count of stored predictions (launch geometry: nothing waits for the device).
 *   out: float64 [8] device = auroc, ap, f1 at 0.01, best f1 over 0.01 .. 0.99, mean loss (loss_sum / ctr[1], NaN without a
 *   batch that carried a loss), n, positives, status (bit 0: ctr[0] != n, bit 1: ctr[2] != 0).  The definitions are those of
 *   builder/utils/metrics.py: exact curves over the distinct prediction values, AUROC 0 when a class is absent or n == 0, AP NaN
 *   without positives, F1 = 2 tp / (predicted + positives) or 0, thresholds (double)p >= i / 100.0.  AUROC and the F1 values are
 *   integer counts and one float64 division; AP is a float64 sum in a fixed order.  Equal inputs, in any order, give equal bits.
 *   workspace: device memory of mtmp_eval_workspace_bytes(n) bytes (-1 for n outside 0 .. 2^24), 16-byte aligned, contents
 *   irrelevant before and after.  A stable LSD radix sort by workgroups of mtmp_eval_sort_tile() keys; 18 launches.
 * All argument errors return before anything touches a GPU. */
int mtmp_eval_append(const float* values, const float* targets, long long count, int mode, const float* loss, float* pred,
                     uint8_t* tgt, float* logit, long long capacity, long long* ctr, double* loss_sum, void* stream);
int mtmp_eval_sort_tile(void);
long long mtmp_eval_workspace_bytes(long long n);
int mtmp_eval_metrics(const float* pred, const uint8_t* tgt, long long n, const long long* ctr, const double* loss_sum,
                      void* workspace, long long workspace_bytes, double* out, void* stream);

/* The position-wise FFN block of an encoder layer as ONE launch, for forwards that nobody differentiates (csrc/ffn_infer.hip):
 *     out[M,256] = x + relu(LN(x) W1^T + c1) W2^T + c2
 * LN = the custom LayerNorm of builder/models/src/transformer/module.py:138-144 (unbiased std, eps added to the std), W1 [1024,256],
 * W2 [256,1024] in the compute dtype, gamma / beta / c1 / c2 fp32, no dropout.  The hidden activation never reaches memory: the
 * kernel writes nothing but out.  ldx / ldo: row strides of x / out in elements (>= 256, multiples of 8); out must not overlap x.
 * mtmp_ffn_block: fp32 (the parity build) and bf16.  mtmp_ffn_block_grouped: bf16, up to three token streams in one grid; all
 * pointer / int arrays are HOST arrays of n entries, rows_live as in the grouped row kernels above (may be NULL as a whole or per
 * entry).  Same kernel, same results as n single calls.  All argument errors return before anything touches a GPU. */
int mtmp_ffn_block(int dtype, const void* x, int ldx, const float* gamma, const float* beta, const void* w1, const float* c1,
                   const void* w2, const float* c2, void* out, int ldo, int M, float eps, void* stream);
int mtmp_ffn_block_grouped(int dtype, int n, const void* const* x, const int* ldx, const float* const* gamma,
                           const float* const* beta, const void* const* w1, const float* const* c1, const void* const* w2,
                           const float* const* c2, void* const* out, const int* ldo, const int* M, float eps,
                           const int32_t* const* rows_live, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MTMP_H */
