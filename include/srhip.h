/* libsrhip -- C ABI of the MI355X (gfx950) SemiReward hot path.
 *
 * The reference (Westlake-AI/SemiReward) is 100 % Python on ATen; it has no FFI of its own.  The
 * "interface each entry point replaces" is therefore the ATen op sequence at the cited reference
 * call site (paths relative to the reference root; K-numbers = SURVEY.md section 2c).
 *
 * Conventions
 *   - plain C: raw DEVICE pointers + sizes, no torch types.  Buffers are borrowed for the call.
 *   - every function enqueues on `stream` (a hipStream_t passed as void*; NULL = default stream) and
 *     returns immediately:  0 = ok, -1 = invalid argument, <= -2 = -(2 + hipError_t) launch failure.
 *     Nothing throws across the boundary; nothing allocates; no host synchronisation.
 *   - bf16 buffers are raw uint16 bit patterns (void*), row-major, 16-byte aligned.
 *   - int64 index tensors keep the reference's dtype (torch.long) so no host-side conversion is needed.
 *   - single thread per process / one process per GPU, like the reference (train.py:344).
 */
#ifndef SRHIP_H
#define SRHIP_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Dense contractions (MFMA).  C[M,N] (+)= A[M,K] . B[N,K]^T, bf16 in, fp32 accumulate.
 * Replaces nn.Linear forward/backward of the backbone:
 *   qkv / proj   semilearn/nets/vit/vit.py:93-98, :105          (K3, K5)
 *   fc1 / fc2    semilearn/nets/vit/vit.py:69-75                (K6)
 * Requirements: K % 32 == 0, N % 4 == 0, lda/ldb % 8 == 0, ldc % 4 == 0, 16-byte aligned bases.
 */
enum {
  SRHIP_EPI_BF16 = 0,       /* C(bf16) = acc + bias                                              */
  SRHIP_EPI_GELU_BF16 = 1,  /* C(bf16) = gelu_erf(acc + bias); aux_out(bf16) = acc + bias if set */
  SRHIP_EPI_RESID_F32 = 2,  /* C(f32) = R + row_scale[m / rows_per_sample] * (acc + bias), R = aux_in (f32, ldaux) if set else C
                               (DropPath + residual add, vit.py:164-165)                            */
  SRHIP_EPI_DGELU_BF16 = 3, /* C(bf16) = acc * gelu_erf'(aux_in)                                 */
  SRHIP_EPI_F32 = 4         /* C(f32) = alpha * acc + beta * C                                   */
};
int srhip_gemm_nt(int epilogue, const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                  const float* bias, const float* row_scale, int rows_per_sample, const void* aux_in, void* aux_out,
                  int ldaux, float alpha, float beta, void* stream);
/* The tile kernel srhip_gemm_nt picks for a product (host logic only, no launch): the 128 x 128 LDS-DMA ring kernel, the 64 x 64 deep-ring kernel
 * for launches that would leave most CUs idle, or one of the persistent 256-row kernels.  Exported so that a test can pin the decision per shape family
 * (the nn.Linear products of vit.py:93-98,105,69-75 at ViT-S width and of the HF encoders behind bert.py:34 / wave2vecv2.py:44 at D = 768). */
#define SRHIP_GEMM_PLAN_TILE128 0
#define SRHIP_GEMM_PLAN_SMALL64 1
#define SRHIP_GEMM_PLAN_BIG256 2
#define SRHIP_GEMM_PLAN_BIG128 3
#define SRHIP_GEMM_PLAN_BIG2WG 4
#define SRHIP_GEMM_PLAN_PP256 5      /* 256 x 256 x 64 tiles, two wave groups half a phase apart (K % 64 == 0, operands < 2 GiB); else BIG256 = its lockstep predecessor */
int srhip_gemm_nt_plan(int epilogue, int M, int N, int K, float beta);
/* srhip_gemm_nt with the tile kernel chosen for a launch of plan_M >= M rows (srhip_gemm_nt_plan(epilogue, plan_M, ...)) and launched over the
 * M real rows: rows split off a larger launch keep that launch's kernel, so each row's result is the same bit for bit (share_pass_prefixes).
 * The split-K accumulating product (SRHIP_EPI_F32 with beta = 1) is refused. */
int srhip_gemm_nt_planned(int epilogue, const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                          const float* bias, const float* row_scale, int rows_per_sample, const void* aux_in, void* aux_out,
                          int ldaux, float alpha, float beta, int plan_M, void* stream);
/* Launches of fewer than n 128 x 128 tiles go to the 64 x 64 deep-ring kernel (default 256 = one round of the chip; K >= 768 products at N >= 768
 * excepted).  The small tiles are the latency choice for a chain of dependent launches that has the chip to itself; a training step whose
 * row-streaming inference launches own most CUs meanwhile sets a low n (fewer, fatter workgroups).  n < 0: query only.  Returns the previous value.
 * Process-wide (one process per GPU, train.py:344), not thread-safe. */
int srhip_gemm_small_max_grid(int n);


/* SRHIP_EPI_RESID_F32 with nn.Dropout on the branch: C(f32)[M,N] = resid (f32, ldresid; NULL: C) + dropout(acc + bias) -- the
 * ``LayerNorm(x + dropout(dense(.)))`` of BertSelfOutput / BertOutput (reached from semilearn/nets/bert/bert.py:34) before the LayerNorm.
 * Mask element index i = m * N + n (ldc == N and N even required); decision per element pair i >> 1 as described at srhip_attn_masked_fwd. */
int srhip_gemm_nt_resid_dropout(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K,
                                const float* bias, const float* resid, int ldresid, unsigned drop_key, unsigned drop_thresh,
                                float drop_scale, void* stream);
/* The same product with the residual taken as LayerNorm(C) of the PRE-LayerNorm sums C holds (in place):
 *   C = (C - ln_mean[m]) * ln_rstd[m] * ln_gamma[n] + ln_beta[n] + dropout(A B^T + bias)
 * -- the post-LN sub-layer chain of the HF encoders (BertSelfOutput / BertOutput behind bert.py:34, Wav2Vec2EncoderLayer behind
 * wave2vecv2.py:44) for the rows without a backward: srhip_postln_fwd(x = NULL) then writes only the bf16 operand and the statistics. */
int srhip_gemm_nt_resid_ln_dropout(const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int N, int K,
                                   const float* bias, const float* ln_mean, const float* ln_rstd, const float* ln_gamma,
                                   const float* ln_beta, unsigned drop_key, unsigned drop_thresh, float drop_scale, void* stream);

/* Grouped variant for the fp32 weight-gradient products (dW = dY^T X of every block, reference: autograd of the same
 * nn.Linear call sites): C_p = alpha * A_p . B_p^T + beta * C_p for n_problems independent products in ONE launch.
 * desc_dev: DEVICE array; tile_start = running sum of ceil(M/128)*ceil(N/128) over the preceding problems;
 * total_tiles = that sum over all problems.  Same operand requirements as srhip_gemm_nt (K % 32 == 0 ...). */
typedef struct srhip_group_desc {
  const void* A; const void* B; float* C;
  int M, N, K, lda, ldb, ldc, tile_start, pad0, pad1, pad2;
} srhip_group_desc;                      /* 64 bytes */
int srhip_gemm_nt_grouped_f32(const srhip_group_desc* desc_dev, int n_problems, int total_tiles, float alpha, float beta,
                              void* stream);
/* The same launch over 128 x 64 tiles (tile_start / total_tiles count ceil(M / 128) * ceil(N / 64) per problem): products whose N is at most a few
 * dozen columns -- the grouped positional convolution of Wav2Vec2 / HuBERT (16 groups x 48 output channels, K = 6144; the HF
 * Wav2Vec2PositionalConvEmbedding behind wave2vecv2.py:44), forward and input gradient. */
int srhip_gemm_nt_grouped_n64_f32(const srhip_group_desc* desc_dev, int n_problems, int total_tiles, float alpha, float beta,
                                  void* stream);

/* Grouped weight-gradient products from ROW-MAJOR operands (no transposes): for each problem
 *   C[M,N] = alpha * A^T . B + beta * C,  A bf16 [K, M] (lda), B bf16 [K, N] (ldb), C fp32 [M, N] (ldc);  dbias[M] += colsum(A)
 * i.e. dW = dY^T X and db = sum_tokens dY of an nn.Linear (autograd of vit.py:69-75, :95-112) with K = tokens.
 * K is arbitrary (rows past K read as zero); M % 8 == 0, N % 8 == 0, lda/ldb % 8 == 0, operands 16-byte aligned.
 * tile_start / total_tiles as in srhip_group_desc.  dbias may be NULL.
 * flags & SRHIP_TN_ATOMIC: the entry is one K slice of a product the caller split along the token axis (A, B point at the slice's first
 * row, K = its rows): C += alpha * A^T B and dbias += column sums through fp32 atomic adds; beta is ignored for the entry (the sum over
 * the slices is then order-dependent in the last bits, like any split-K reduction). */
#define SRHIP_TN_ATOMIC 1
/* flags & SRHIP_TN_OVERWRITE: the entry is a token slice with a slab of its OWN (C, dbias point into scratch): C = alpha * A^T B and dbias =
 * column sums are written, not accumulated (beta ignored); srhip_slab_reduce_f32 then adds the slabs of a product into its gradient.  An fp32
 * atomic add is a memory transaction of its own on this chip: with 14 M of them per WideResNet backward the sliced weight gradients spent more time
 * in their epilogues than in their products (profiles/r06_wrn_dw_slabs_ab.txt). */
#define SRHIP_TN_OVERWRITE 2
typedef struct srhip_group_tn_desc {
  const void* A; const void* B; float* C; float* dbias;
  int M, N, K, lda, ldb, ldc, tile_start, flags;
} srhip_group_tn_desc;                   /* 64 bytes */
int srhip_gemm_tn_grouped_f32(const srhip_group_tn_desc* desc_dev, int n_problems, int total_tiles, float alpha, float beta,
                              void* stream);
/* dst[i] += sum_{s < n_slabs} src[s * stride + i], i < count, for every entry (16-byte aligned dst / src, stride in elements); block_start = first
 * workgroup of the entry, 1024 elements per workgroup; total_blocks = their sum. */
typedef struct srhip_slab_desc {
  float* dst; const float* src; long long stride;
  int count, n_slabs, block_start, pad0;
} srhip_slab_desc;                       /* 40 bytes */
int srhip_slab_reduce_f32(const srhip_slab_desc* desc_dev, int n, int total_blocks, void* stream);
/* The same products through 256 x 256 output tiles (persistent workgroups, 64-token K-tiles, two wave groups half a phase apart): the kernel for
 * the wide layers' weight gradients (D = 768: autograd of the HF encoder Linears behind semilearn/nets/bert/bert.py:34 and
 * wave2vecv2/wave2vecv2.py:44; 8192 tokens per step) and for ViT-S tables whose problems 256-tiles cover well.  Same descriptor, same
 * arithmetic (bf16 operands, fp32 accumulation, dbias += column sums of A) -- but tile_start / total_tiles count 256 x 256 tiles:
 * ceil(M / 256) * ceil(N / 256) per entry; K >= 1 for every entry (the refill cursor runs one K-tile ahead of the multiplying waves).  The walk is static (workgroup w takes tiles w, w + 256, ...): the caller balances a short last
 * round by handing the last entries over as SRHIP_TN_ATOMIC token slices (ops.make_group_tn_desc(tile=256) does). */
int srhip_gemm_tn_grouped_pp_f32(const srhip_group_tn_desc* desc_dev, int n_problems, int total_tiles, float alpha, float beta,
                                 void* stream);

/* Fused attention, head_dim 64.  qkv bf16 [B*N, 3*H*64] as written by the qkv Linear; out bf16 [B*N, H*64];
 * lse fp32 [B,H,N] (NULL when no backward is needed).  Replaces vit.py:100-104 (K4).  N <= 512. */
int srhip_attn_fwd(const void* qkv, void* out, float* lse, int B, int N, int H, float scale, void* stream);
/* dqkv bf16 [B*N, 3*H*64]; delta_ws fp32 [B,H,N] scratch.  Autograd backward of vit.py:100-104.  N <= 512. */
int srhip_attn_bwd(const void* qkv, const void* out, const void* d_out, const float* lse, void* dqkv, float* delta_ws,
                   int B, int N, int H, float scale, void* stream);

/* Host logic of the four entry points above and below, no launch: what a (B, N, H) launch reaches.  nkt = the key-tile instantiation
 * (2, 8, 14, 18 or 32 tiles of 16 keys: the smallest that holds N), fwd_pair = 1 when the forward is attn_fwd_pair_kernel (N > 288),
 * bwd_l2 = 1 when the backward reads its V / (q, dO) row fragments from L2 (N > 288), bwd_split = the backward grid's blockIdx.y extent
 * (query / key tiles split over extra workgroups while B*H*split*2 < 128).  Any out pointer may be NULL.  SR_EINVAL exactly where the
 * launchers refuse the shape. */
int srhip_attn_plan(int B, int N, int H, int* nkt, int* fwd_pair, int* bwd_l2, int* bwd_split);

/* Padding-aware variants for the BERT / Wav2Vec2 encoders (semilearn/nets/bert/bert.py:34 -> transformers BertSelfAttention;
 * wave2vecv2/wave2vecv2.py:44 -> Wav2Vec2Attention): key_len int32 [B] = number of valid (non-padding) keys of every sequence of a
 * right-padded batch (NULL: all N), equivalent to the additive -inf attention mask; every query row is computed.  drop_*: train-mode
 * nn.Dropout on the probabilities from the counter-based generator of all dropout sites: ONE hash h = fmix32(pair * 0x9E3779B1 + drop_key)
 * decides TWO neighbouring elements -- the even one is kept iff (h & 0xFFFF) >= drop_thresh >> 16, the odd one iff (h >> 16) is; kept values
 * * drop_scale; drop_thresh == 0: none (the hash, two quarter-rate multiplies, was 74 % of this forward's vector-ALU work at N = 512;
 * oracle/bert_ref.keep_mask restates it).  At THIS site the pairs are taken within a query row: pair = ((b*H + h)*N + q) * ceil(N / 2) +
 * (key >> 1); at every other site (srhip_gemm_nt_resid_dropout, embeddings, post-LN, pooling) pair = i >> 1 of the row-major element index i.
 * N <= 512 forward AND backward (N > 288: the forward walks two query tiles per wave through 128-key blocks, attn_fwd_pair_kernel; the V
 * fragments of the dQ pass come from L2 instead of LDS).  B*H*N*N < 2^32.
 * key_len contract: 1 <= key_len[b] <= N for every sequence; the kernels do not check it on the device.  A sequence without a valid key has
 * no softmax (the whole-row forward would write NaN rows, the paired forward walks no key block), a length above N reads no further than N but
 * is not a supported argument.  The range is the caller's to keep: the BERT engine takes key_len = the row sums of the prefix mask it is handed
 * (srhip_mask_lengths; TokenBatch.from_dict accepts any attention_mask), so key_len <= L always holds, and key_len >= 1 is ASSUMED of the
 * tokenizer -- every tokenised sequence holds at least [CLS] and [SEP] -- and not checked: an all-zero mask row would break the contract; the
 * Wav2Vec2 engine passes the frame count of the clip length for every clip, 1 <= T <= the frame pitch it launches as N.  Padded rows (key_len[b] <= row < N) of K and V
 * may hold any finite values: they never reach a result, and their dK and dV rows are written as zeros. */
int srhip_attn_masked_fwd(const void* qkv, void* out, float* lse, const int* key_len, int B, int N, int H, float scale,
                          unsigned drop_key, unsigned drop_thresh, float drop_scale, void* stream);
int srhip_attn_masked_bwd(const void* qkv, const void* out, const void* d_out, const float* lse, void* dqkv, float* delta_ws,
                          const int* key_len, int B, int N, int H, float scale, unsigned drop_key, unsigned drop_thresh,
                          float drop_scale, void* stream);

/* nn.LayerNorm over the last dim (vit.py:135,150,268; eps 1e-6 :222) (K2).  x fp32 [M,D] -> out bf16 [M,D];
 * mean/rstd fp32 [M] are written when non-NULL (needed by the backward).  D in {128, 384, 768}. */
int srhip_layernorm_fwd(const float* x, const float* gamma, const float* beta, float eps, void* out, float* mean,
                        float* rstd, int M, int D, void* stream);
/* dx (fp32) += LN'(dy bf16); dgamma/dbeta (fp32) += column sums (atomic). */
int srhip_layernorm_bwd(const void* dy, const float* x, const float* mean, const float* rstd, const float* gamma,
                        float* dx, float* dgamma, float* dbeta, int M, int D, void* stream);
/* ... and also out_bf16[m, :] = bf16(row_scale[m / rows_per_sample] * dx[m, :]) of the UPDATED dx: the DropPath-scaled output gradient of the
 * next branch (vit.py:164-165 backward), i.e. srhip_layernorm_bwd + srhip_cast_scale_rows in one launch.  row_scale NULL = 1. */
int srhip_layernorm_bwd_cast(const void* dy, const float* x, const float* mean, const float* rstd, const float* gamma, float* dx, float* dgamma,
                             float* dbeta, void* out_bf16, const float* row_scale, int rows_per_sample, int M, int D, void* stream);
/* The same with the column sums spread over n_rep partial copies, part fp32 [n_rep][2][D] (copy = workgroup % n_rep; [.][0] dgamma, [.][1]
 * dbeta): the 2 * D words of one LayerNorm are otherwise hit by every workgroup of the launch, and same-address device-scope atomics
 * serialise (measured: 11 of 19 us at M = 4112).  out_bf16 may be NULL.  srhip_ln_grad_reduce adds the copies of n_ln LayerNorms
 * (part [n_ln][n_rep][2][D]) to their dgamma / dbeta (torch.autograd's accumulation into .grad of vit.py:135,150) and clears them:
 * one launch per step, after the last LayerNorm backward. */
int srhip_layernorm_bwd_part(const void* dy, const float* x, const float* mean, const float* rstd, const float* gamma, float* dx, float* part,
                             int n_rep, void* out_bf16, const float* row_scale, int rows_per_sample, int M, int D, void* stream);
typedef struct srhip_ln_reduce_desc { float* dgamma; float* dbeta; } srhip_ln_reduce_desc;   /* 16 bytes */
int srhip_ln_grad_reduce(const srhip_ln_reduce_desc* desc_dev, float* part, int n_ln, int n_rep, int D, void* stream);
/* srhip_gemm_tn_grouped_f32 with the ViT backward's small sums over all rows as extra workgroups behind its tiles (one launch instead of five;
 * the small workgroups fill the slots the last round of tiles leaves empty).  The tail (a HOST struct, passed by value to the kernel) names
 *   - srhip_ln_grad_reduce(ln_desc, ln_part, n_ln, n_rep, D)                                   (n_ln = 0: none),
 *   - the dWh / dbh half of srhip_cls_head_bwd(dlogits [B,C], feat [B,D])                       (C = 0: none),
 *   - the dpos / dcls launch and stage 1 (partial sums into pe_ws) of srhip_patch_embed_bwd_ws  (dx = NULL: none); stage 2 reads what stage 1
 *     wrote and stays a launch behind this one: srhip_patch_embed_bwd_fold.
 * Every element is summed by one thread in the order of the separate launches: same bits.  None of the tail's outputs may alias a C / dbias of
 * the table. */
typedef struct srhip_dw_tail {
  const srhip_ln_reduce_desc* ln_desc; float* ln_part;
  const float* dlogits; const float* feat; float* dWh; float* dbh;
  const float* dx; const float* img; const int* img_index; float* dpos; float* dcls; float* pe_ws;
  int n_ln, n_rep, C, B, D, in_chans, HW, ps;
} srhip_dw_tail;                         /* 128 bytes */
int srhip_gemm_tn_grouped_tail_f32(const srhip_group_tn_desc* desc_dev, int n_problems, int total_tiles, float alpha, float beta,
                                   const srhip_dw_tail* tail, void* stream);
int srhip_patch_embed_bwd_fold(const float* ws, float* dWp, float* dbp, int B, int C, int HW, int ps, int D, void* stream);

/* Fused MLP half of a transformer block on the fp32 residual stream (x -> x_out, both [M, D]; x_out may equal x):
 *   x_out = x + row_scale[m / rows_per_sample] * ( fc2( GELU( fc1( LayerNorm(x) ) ) ) + b2 )
 * = Block.forward's second residual (vit.py:165) with Mlp.forward (vit.py:69-75), norm2 (vit.py:150) and DropPath
 * (row_scale, NULL = 1).  W1 bf16 [Hd, D], W2 bf16 [D, Hd], biases / LN affine fp32.  The hidden activation stays in registers.
 * save_rows > 0: the first save_rows rows carry a gradient (they lead a mixed batch); for them the kernel also writes what the
 * hand-written backward needs -- norm2 output (save_ln2 bf16 [save_rows, D]), fc1 pre-activation and GELU output (save_pre,
 * save_h bf16 [save_rows, Hd]) and the LayerNorm statistics (save_mean, save_rstd fp32 [save_rows]) -- exactly the values
 * layernorm_fwd + gemm_nt(GELU, aux_out) would have stored.
 * D == 384 (ViT-S width), Hd % 128 == 0, Hd <= 4096.  Same rounding points as layernorm_fwd + gemm_nt(GELU) + gemm_nt(RESID). */
int srhip_mlp_fused(const float* x, float* x_out, const float* ln_gamma, const float* ln_beta, float eps, const void* W1,
                    const float* b1, const void* W2, const float* b2, const float* row_scale, int rows_per_sample, int save_rows,
                    void* save_ln2, void* save_pre, void* save_h, float* save_mean, float* save_rstd, int M, int D, int Hd,
                    void* stream);
/* The same with the attention output projection and the first residual of the block in front (rows without a backward):
 *   x1 = x + row_scale1 * (ao Wp^T + bp);  x_out = x1 + row_scale2 * (fc2(GELU(fc1(LayerNorm(x1)))) + b2)
 * -- vit.py:105-106 (proj) + :163 (drop_path1, residual) + :165 in ONE launch; replaces srhip_gemm_nt(EPI_RESID_F32) + srhip_mlp_fused.
 * ao bf16 [M, D] (attention output, heads concatenated), Wp bf16 [D, D]; x_out may alias x.  The residual stream makes no round trip inside
 * the launch (x is the start value of the accumulators, x1 stays in them), so the DropPath factors act on the bf16 B operands of the products:
 * row_scale2 on the GELU output before its (single) rounding; row_scale1 on ao -- ao_scaled != 0 says the launch that wrote ao applied it
 * before rounding (srhip_attn_block_fused out_scale: one rounding, as in the unfused path), 0 has it applied here (a second rounding of ao).
 * ln_next (bf16 [M, D], may be NULL): LayerNorm(x_out) with (next_gamma, next_beta) = the NEXT block's norm1 -- the operand of its
 * srhip_attn_block_fused -- written by the same launch (replaces that block's srhip_layernorm_fwd). */
/* GELU inside srhip_mlp_fused_proj: x * Phi(x) with Phi = 1/2 + xc R(xc^2), xc = x clamped to +-4.252893, R a degree-8 polynomial (no
 * v_rcp / v_exp: the kernel's main loop is bound by the vector ALU).  |result - exact-erf GELU| <= max(7e-5, 5e-6 |x|), below half a bf16
 * quantum of the result wherever |GELU| >= 0.03; the result is rounded to bf16 right after.  srhip_gelu_eval evaluates both forms of the
 * library (y_erf: the 1.5e-7 form every other path uses) on n values. */
int srhip_gelu_eval(const float* x, float* y_erf, float* y_poly, int n, void* stream);
int srhip_mlp_fused_proj(const float* x, float* x_out, const void* ao, const void* Wp, const float* bp, const float* row_scale1,
                         int ao_scaled, const float* ln_gamma, const float* ln_beta, float eps, const void* W1, const float* b1, const void* W2,
                         const float* b2, const float* row_scale2, int rows_per_sample, void* ln_next, const float* next_gamma,
                         const float* next_beta, int M, int D, int Hd, void* stream);
/* srhip_mlp_fused_proj over M rows that lie row_pitch elements apart in x, x_out and ao: logical row m at element m * row_pitch of each.  For the
 * last block of a forward whose only reader is the head (srhip_cls_head_fwd reads row b * N of image b): M = images, rows_per_sample = 1,
 * row_pitch = N * D computes the class-token rows in place and neither reads nor writes the rows in between.  Everything per row is
 * srhip_mlp_fused_proj's, so a row's result is bit for bit the one of the dense launch that contains it.
 * SR_EINVAL: row_pitch < D, row_pitch % 8 != 0 (16-byte row starts of the bf16 operand), ln_next with row_pitch != D. */
int srhip_mlp_fused_proj_strided(const float* x, float* x_out, const void* ao, const void* Wp, const float* bp, const float* row_scale1,
                                 int ao_scaled, const float* ln_gamma, const float* ln_beta, float eps, const void* W1, const float* b1,
                                 const void* W2, const float* b2, const float* row_scale2, int rows_per_sample, void* ln_next,
                                 const float* next_gamma, const float* next_beta, int M, int D, int Hd, int row_pitch, void* stream);
/* srhip_mlp_fused_proj whose rows follow one block's row of a DropPath plan (srhip_vit_droppath_plan): plan_row int32 [1 + B], plan_row[0] =
 * n_mlp, plan_row[1 ..] = a permutation of the B samples with the n_mlp samples whose row_scale2 is not 0 first.  Virtual row v of the launch
 * is row v % rows_per_sample of sample plan_row[1 + v / rows_per_sample] in x, x_out, ao and ln_next, and takes that sample's two factors.
 * A 128-row tile that starts below virtual row n_mlp * rows_per_sample runs what srhip_mlp_fused_proj runs; the others hold only rows whose
 * MLP branch is dropped (row_scale2 == 0, vit.py:165: x1 + 0 * (...) = x1) and stop after the projection: x_out = x1, ln_next = LayerNorm(x1).
 * Every row is still written, M and the grid do not depend on device data, and a row's values do not depend on the tile that carries it:
 * bit for bit srhip_mlp_fused_proj's, except that a skipped branch adds nothing where that launch adds products of +-0 (the sign of an
 * exactly-zero element may differ; an Inf / NaN inside a dropped branch does not reach the row).  row_scale2 must be given.
 * SR_EINVAL: plan_row NULL, B <= 0, M != B * rows_per_sample, and whatever srhip_mlp_fused_proj refuses. */
int srhip_mlp_fused_proj_planned(const float* x, float* x_out, const void* ao, const void* Wp, const float* bp, const float* row_scale1,
                                 int ao_scaled, const float* ln_gamma, const float* ln_beta, float eps, const void* W1, const float* b1,
                                 const void* W2, const float* b2, const float* row_scale2, int rows_per_sample, void* ln_next,
                                 const float* next_gamma, const float* next_beta, int M, int D, int Hd, const int* plan_row, int B, void* stream);

/* Fused qkv projection + attention of a ViT block for rows without a backward: ao = softmax(q k^T * scale) v with [q | k | v] = xn Wqkv^T +
 * bqkv -- Attention.forward up to the output projection (semilearn/nets/vit/vit.py:93-104) on the norm1 output (:163) in ONE launch, one
 * workgroup per image; replaces srhip_gemm_nt(qkv) + srhip_attn_fwd for inference rows (the [M, 3D] qkv activation never reaches HBM).
 * xn_bf16 [B*N, D]: the rows normalised by srhip_layernorm_fwd; Wqkv bf16 [3D, D] (q | k | v rows, head-major); out bf16 [B*N, D].
 * Built for D = 384, H = 6 and N in {257, 197} (ViT-S/2 at 32x32, ViT-S/16 at 224x224): srhip_attn_block_supported() tells, anything else
 * is an argument error.  N = 257 = 16 token tiles + one token: qkv_extra bf16 [B, 3D] = q | k | v of token 256 of every image (one
 * srhip_gemm_nt over the B rows xn_bf16 + 256 * D with lda = N * D) must be given; ignored for N = 197.
 * out_scale fp32 [B] or NULL: factor on every output row of image b, applied before the bf16 rounding -- the DropPath factor of the attention
 * branch (vit.py:163) when the consumer is srhip_mlp_fused_proj(ao_scaled = 1).  An image whose factor is exactly 0 (a dropped branch) gets
 * +0 in all of its output rows without its projections or its softmax being computed. */
int srhip_attn_block_supported(int N, int D, int H);
int srhip_attn_block_fused(const void* xn_bf16, const void* Wqkv, const float* bqkv, const void* qkv_extra, void* out, const float* out_scale,
                           int B, int N, int D, int H, float scale, void* stream);

/* PatchEmbed conv (kernel = stride = ps) + cls token + pos_embed (vit.py:39-44, :277-280) (K1).
 * img fp32 [*, C, HW, HW]; img_index int32 [B] maps batch row -> image (NULL = identity; lets the K+1 passes of
 * one SemiReward step share one copy of the images); x fp32 [B, N, D], N = (HW/ps)^2 + 1.  C*ps*ps <= 64. */
int srhip_patch_embed_fwd(const float* img, const int* img_index, const float* Wp, const float* bp, const float* cls,
                          const float* pos, float* x, int B, int C, int HW, int ps, int D, void* stream);
/* all outputs are accumulated (+=). */
int srhip_patch_embed_bwd(const float* dx, const float* img, const int* img_index, float* dWp, float* dbp, float* dcls,
                          float* dpos, int B, int C, int HW, int ps, int D, void* stream);
/* The same without atomics on the filter: per-(token chunk, image) partial sums in ws (srhip_patch_embed_bwd_ws_floats(...) floats), folded
 * by a second launch in a fixed order (deterministic; the one-launch form ends every workgroup in D * (K + 1) same-address atomics).
 * srhip_patch_embed_bwd_ws_floats returns -1 for a shape the launches refuse (K > 64, ps <= 0, D % 64 != 0, D > 1024, ...). */
long srhip_patch_embed_bwd_ws_floats(int B, int C, int HW, int ps, int D);
int srhip_patch_embed_bwd_ws(const float* dx, const float* img, const int* img_index, float* dWp, float* dbp, float* dcls,
                             float* dpos, float* ws, int B, int C, int HW, int ps, int D, void* stream);

/* Large-patch PatchEmbed (C * ps * ps > 64, e.g. ViT-S/16 at 224 x 224, vit.py:358-371): the conv of vit.py:39-44 as a GEMM.
 *   patch_im2col : col[b * Np + p][(c,i,j)] = img[img_index[b]][c][py*ps+i][px*ps+j] as bf16 (ps even); then
 *                  srhip_gemm_nt(EPI_F32): tok[B*Np, D] = col . Wp^T with Wp = patch_embed.proj.weight viewed [D, C*ps*ps];
 *   patch_assemble: x[b,0,:] = cls + pos[0], x[b,1+p,:] = tok[b*Np+p,:] + bp + pos[1+p]                       (vit.py:277-280)
 *   patch_grad_operands (backward): dpos += sum_b dx[b,:,:], dcls += sum_b dx[b,0,:], and the patch-token rows of dx as bf16
 *                  [B*Np, D] -- the A operand of srhip_gemm_tn_grouped_f32 with B = col: dWp += dx_tok^T col, dbp += colsum dx_tok. */
int srhip_patch_im2col(const float* img, const int* img_index, void* out, int B, int C, int HW, int ps, void* stream);
int srhip_patch_assemble(const float* tok, const float* bp, const float* cls, const float* pos, float* x, int B, int Np, int D,
                         void* stream);
int srhip_patch_grad_operands(const float* dx, void* dx_tok_bf16, float* dpos, float* dcls, int B, int Np, int D, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Split-bf16 ("bf16x3") forward of the rows that decide the pseudo-label masks (read_rows_precision = bf16x3; csrc/x3.hip).
 * Every fp32 operand x is split into hi = bf16_rne(x), lo = bf16_rne(x - hi); a product is hi.hi + hi.lo + lo.hi on the bf16 MFMA with fp32
 * accumulation (lo.lo dropped): ~4e-6 relative error against fp64 where the bf16 operands of srhip_gemm_nt give ~2e-3.  Activations are fp32.
 *
 * srhip_gemm_nt_x3: C(f32)[M,N] = epilogue(A(f32)[M,K] . W(f32)[N,K]^T) -- the nn.Linear forwards of vit.py:93-98,105 (qkv, proj),
 * :69-75 (fc1, fc2) and the patch-embedding conv as a GEMM (:39-44), W read straight from the fp32 parameter block.
 *   SRHIP_X3_EPI_F32       : C = acc + bias
 *   SRHIP_X3_EPI_GELU_F32  : C = gelu_erf(acc + bias)                                               (nn.GELU(), vit.py:63,72)
 *   SRHIP_X3_EPI_RESID_F32 : C = C + row_scale[m / rows_per_sample] * (acc + bias), row_scale NULL = 1  (DropPath + residual, vit.py:164-165)
 * The three are epilogues of the 128 x 128-tile engine that srhip_gemm_x3 and srhip_gemm_tn_x3_grouped launch too (gemm_x3_kernel, one main loop).
 * bias may be NULL.  Requirements: K % 32 == 0, lda >= K and ldw >= K multiples of 4, ldc >= N, A and W 16-byte aligned; any M (ragged tails
 * included) up to 65535 * 128 rows, any N.  row_scale only with SRHIP_X3_EPI_RESID_F32.
 * srhip_attn_fwd_x3: head_dim 64, qkv fp32 [B*N, 3*H*64] as srhip_gemm_nt_x3 writes it, out fp32 [B*N, H*64]; QK^T and PV as bf16x3 products,
 * softmax in fp32 (accurate expf; the row sum over the unrounded probabilities).  Replaces vit.py:100-104.  N <= 512, B <= 65535.
 * srhip_layernorm_fwd_f32: srhip_layernorm_fwd with an fp32 output [M, D] (same statistics, same kernel body).
 * srhip_patch_im2col_f32: srhip_patch_im2col with fp32 output (the A operand of srhip_gemm_nt_x3). */
enum {
  SRHIP_X3_EPI_F32 = 0,
  SRHIP_X3_EPI_GELU_F32 = 1,
  SRHIP_X3_EPI_RESID_F32 = 2
};
int srhip_gemm_nt_x3(int epilogue, const float* A, int lda, const float* W, int ldw, float* C, int ldc, int M, int N, int K,
                     const float* bias, const float* row_scale, int rows_per_sample, void* stream);
int srhip_attn_fwd_x3(const float* qkv, float* out, int B, int N, int H, float scale, void* stream);
int srhip_layernorm_fwd_f32(const float* x, const float* gamma, const float* beta, float eps, float* out, float* mean, float* rstd, int M,
                            int D, void* stream);
int srhip_patch_im2col_f32(const float* img, const int* img_index, float* out, int B, int C, int HW, int ps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Split-bf16 ("bf16x3") kernels of the gradient rows (grad_rows_precision = bf16x3; csrc/x3.hip, same product scheme and same kernels as above).
 *
 * srhip_attn_fwd_x3_lse: srhip_attn_fwd_x3 (the same kernel template, the same out bits) that also writes lse fp32 [B,H,N] = rowmax + log(rowsum) of the scaled scores (the backward's
 *   statistic).  Same requirements.
 * srhip_gemm_x3: the 128 x 128-tile engine of srhip_gemm_nt_x3 (NT GELU_PRE and NT GELU_F32 write the same C bits), fp32 operands, fp32 C.
 *   SRHIP_X3B_NT: C[M,N] = A[M,K] . B[N,K]^T; epilogue SRHIP_X3B_EPI_GELU_PRE only: v = acc + bias, aux_out[m*ldaux+n] = v, C = gelu_erf(v)
 *     (fc1 of a row that keeps its activations, vit.py:69-72).  lda, ldb >= K.
 *   SRHIP_X3B_NN: C[M,N] = epi(A[M,K] . B[K,N]) -- the input gradient dY . W with W read from the fp32 parameter block as it is stored.
 *     SRHIP_X3B_EPI_F32: C = acc;  SRHIP_X3B_EPI_ACC: C += acc;  SRHIP_X3B_EPI_DGELU: C = acc * gelu_erf'(aux[m*ldaux+n]) (exact-erf derivative).
 *     No bias.  lda >= K, ldb >= N, N % 4 == 0.
 *   Both: K % 32 == 0, lda, ldb multiples of 4, A and B 16-byte aligned, ldc >= N, any M up to 65535 * 128.
 * srhip_gemm_tn_x3_grouped: for every entry of a srhip_group_tn_desc table (tile_start in 128 x 128 tiles, flags 0, A, B fp32):
 *   C[M,N] += A[K,M]^T . B[K,N], dbias[M] += colsum A (dbias may be NULL) -- dW += dY^T X, db += sum of dY over the tokens.  Any K >= 1 (ragged
 *   token tails are zero-filled); M, N multiples of 4; lda, ldb multiples of 4; 16-byte aligned A, B.  Deterministic: every output element
 *   and every bias sum is owned by one workgroup.
 * srhip_attn_bwd_x3: qkv fp32 [B*N, 3*H*64], out / d_out fp32 [B*N, H*64], lse as srhip_attn_fwd_x3_lse wrote it -> dqkv fp32 [B*N, 3*H*64]
 *   (every element written); delta_ws fp32 [B,H,N] scratch.  S = Q K^T recomputed, P = exp(S scale - lse), delta = rowsum(dO o O),
 *   dV = P^T dO, dP = dO V^T, dS = P o (dP - delta), dQ = scale dS K, dK = scale dS^T Q, every product bf16x3.  Two launches.  N <= 512.
 * srhip_layernorm_bwd_part_f32: srhip_layernorm_bwd_part with fp32 dy and an fp32 out (= row_scale * the updated dx; NULL: not written).
 * srhip_patch_grad_operands_f32: srhip_patch_grad_operands with an fp32 dx_tok.
 * srhip_scale_rows_f32: out[m, :] = row_scale[m / rows_per_sample] * x[m, :] (row_scale NULL = 1), fp32, D % 4 == 0, 16-byte aligned. */
enum { SRHIP_X3B_NT = 0, SRHIP_X3B_NN = 1 };
enum {
  SRHIP_X3B_EPI_F32 = 0,
  SRHIP_X3B_EPI_ACC = 1,
  SRHIP_X3B_EPI_DGELU = 2,
  SRHIP_X3B_EPI_GELU_PRE = 3
};
int srhip_attn_fwd_x3_lse(const float* qkv, float* out, float* lse, int B, int N, int H, float scale, void* stream);
int srhip_gemm_x3(int layout, int epilogue, const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M, int N, int K,
                  const float* bias, const float* aux, float* aux_out, int ldaux, void* stream);
int srhip_gemm_tn_x3_grouped(const srhip_group_tn_desc* desc_dev, int n_problems, int total_tiles, void* stream);
int srhip_attn_bwd_x3(const float* qkv, const float* out, const float* d_out, const float* lse, float* dqkv, float* delta_ws, int B, int N,
                      int H, float scale, void* stream);
int srhip_layernorm_bwd_part_f32(const float* dy, const float* x, const float* mean, const float* rstd, const float* gamma, float* dx,
                                 float* part, int n_rep, float* out, const float* row_scale, int rows_per_sample, int M, int D, void* stream);
int srhip_patch_grad_operands_f32(const float* dx, float* dx_tok, float* dpos, float* dcls, int B, int Np, int D, void* stream);
int srhip_scale_rows_f32(const float* x, const float* scale, int rows_per_sample, float* out, long M, int D, void* stream);

/* Final norm on the cls token, global_pool='token', classifier head (vit.py:282, :296-305) (K7).
 * feat fp32 [B,D], logits fp32 [B,C]; xhat [B,D] / rstd [B] saved for the backward when non-NULL. */
int srhip_cls_head_fwd(const float* x, const float* gamma, const float* beta, float eps, const float* Wh, const float* bh,
                       float* feat, float* logits, float* xhat, float* rstd, int B, int N, int D, int C, void* stream);
/* The same, ALSO (or only: feat / logits may then be NULL) writing image b's outputs to row out_rows[b] of feat_all [*, D] / logits_all [*, C]:
 * the step's buffers over all (pass, image) rows, filled by the launch trains directly instead of by an index_copy_ each. */
int srhip_cls_head_fwd_scatter(const float* x, const float* gamma, const float* beta, float eps, const float* Wh, const float* bh,
                               float* feat, float* logits, float* xhat, float* rstd, float* feat_all, float* logits_all,
                               const long long* out_rows, int B, int N, int D, int C, void* stream);
/* dx[b,0,:] = ...(rows other than the cls row are left untouched: zero dx first); dWh/dbh/dgamma/dbeta +=.
 * dx == NULL: only the head weight / bias gradients (they sum over ALL images of the backward); dWh == NULL: only dx and the final-norm affine
 * gradients (atomic adds) of the B images handed in -- the two halves of a backward whose images are back-propagated in separate row chains. */
int srhip_cls_head_bwd(const float* dlogits, const float* Wh, const float* gamma, const float* feat, const float* xhat,
                       const float* rstd, float* dx, float* dWh, float* dbh, float* dgamma, float* dbeta, int B, int N,
                       int D, int C, void* stream);

/* glue feeding the GEMM: fp32 -> bf16 with optional per-sample (DropPath) scale; transposes with zero padding,
 * optional exact-erf GELU, optional column sums (bias gradients, atomic +=); flat cast. */
int srhip_cast_scale_rows(const float* x, const float* scale, int rows_per_sample, void* out, long M, int D, void* stream);
int srhip_transpose_to_bf16(const void* in, int in_is_f32, int ld_in, void* out, int ld_out, int M, int Mp, int C,
                            int apply_gelu, float* colsum, void* stream);
/* Batched srhip_transpose_to_bf16 (no column sums): one launch over all 64x64 tiles of n transposes.
 * tile_start = running sum of ceil(Mp/64) * (C/64) over the preceding entries. */
typedef struct srhip_transpose_desc {
  const void* in; void* out;
  int in_is_f32, ld_in, ld_out, M, Mp, C, apply_gelu, tile_start;
  long pad;
} srhip_transpose_desc;                  /* 56 bytes */
int srhip_transpose_batched(const srhip_transpose_desc* desc_dev, int n, int total_tiles, void* stream);
int srhip_cast_f32_bf16(const float* x, void* out, long n, void* stream);
/* timm DropPath (vit.py:148,161): out[depth,2,B] = Bernoulli(1-p_l)/(1-p_l), counter-based RNG. */
int srhip_droppath_fill(float* out, const float* probs, int depth, int B, unsigned long long seed, void* stream);
/* The same draw, but only (and in the order of) the columns cols[0 .. n_cols): out [depth, 2, n_cols], out[l, j, q] = table[l, j, cols[q]].
 * One launch lays the table out in the order of the step's launch trains (gradient rows | read rows | deferred rows), each of which then
 * takes a contiguous column slice -- instead of an index_select per train on the step's critical path. */
int srhip_droppath_fill_cols(float* out, const float* probs, const long long* cols, int depth, int B, int n_cols, unsigned long long seed,
                             void* stream);
/* DropPath plan of one forward, built on the device from the table its launches read: dp[l * stride_block + j * stride_branch + b] (strides
 * in elements: a contiguous [depth, 2, B] table or a column slice of a wider one).  plan int32 [depth, 1 + B]: plan[l][0] = n_mlp, the number
 * of samples whose MLP factor dp[l, 1, b] is not 0; plan[l][1 .. B] = a stable partition of 0 .. B-1, those samples first in ascending
 * order, then the others in ascending order (srhip_mlp_fused_proj_planned takes row l).  Reads device memory only, so it replays inside a
 * captured step.  One workgroup per block, any B. */
int srhip_vit_droppath_plan(const float* dp, long long stride_block, long long stride_branch, int depth, int B, int* plan, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pass-prefix sharing of ViT inference rows (share_pass_prefixes, csrc/pass_tree.hip).  The K + 1 passes of a step forward the same images
 * and differ only by their DropPath draws: each (image, draws so far) is computed once, as a node of a pass-prefix tree.
 *   srhip_vit_fork:   in front of the block where nodes split, node dst0 + g (g < n_new) becomes a copy of node parent[g] < dst0: the fp32
 *                     residual x [*, rows_per_node, D] and, if ln != NULL, the bf16 norm1 output ln [*, rows_per_node, D] the previous fused
 *                     launch already wrote.  In place: sources and destinations are disjoint.
 *   srhip_vit_fanout: after the head, column g (g < n_cols) of the step's tables takes its node's outputs:
 *                     logits_all[col_rows[g], :C] = node_logits[col_node[g], :], feat_all[col_rows[g], :D] = node_feat[col_node[g], :]
 *                     (node tables [n_nodes, .], step tables [rows_all, .]: rows_all bounds both, so pass the shorter table's rows).
 * Index entries out of range copy nothing.  Pure copies (16-byte accesses where slabs and bases allow): results are the unshared launch's. */
int srhip_vit_fork(float* x, void* ln, const int* parent, int n_new, int dst0, int rows_per_node, int D, void* stream);
int srhip_vit_fanout(const float* node_logits, const float* node_feat, int n_nodes, const int* col_node, const long long* col_rows,
                     int n_cols, float* logits_all, float* feat_all, long long rows_all, int C, int D, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Score filter (K8, K9, K11, K12, K13).
 * srhip_row_max: softmax (compute_prob, semilearn/core/algorithmbase.py:332-333) + torch.max / argmax
 *   (semilearn/algorithms/hooks/pseudo_label.py:40, srflexmatch/utils.py:50).  in fp32 [B,C] = logits
 *   (in_is_probs = 0) or probabilities (1); probs_out optional. */
int srhip_row_max(const float* in, int in_is_probs, float* probs_out, float* max_probs, long long* max_idx, int B, int C,
                  void* stream);
/* The same on rows read in place from a [groups, rows, C] buffer: input row r = in + (r / rows_per_group) * group_stride +
 * (r % rows_per_group) * C (elements) -- the weak rows of every pass inside the step's logits (srflexmatch.py:75-104 takes them pass by pass
 * out of separate forward calls); outputs dense. */
int srhip_row_max_strided(const float* in, int in_is_probs, float* probs_out, float* max_probs, long long* max_idx, int B, int C,
                          int rows_per_group, long long group_stride, void* stream);
/* FlexMatchThresholdingHook.masking + update (semilearn/algorithms/srflexmatch/utils.py:24-63).  State on device:
 * selected_label int64 [ulb_dest_len] (-1 = unused), classwise_acc fp32 [C], hist int32 [C+1] (bin C = unused).
 * idx_ulb must be unique within the batch (reference sampler property). */
int srhip_flexmatch_mask(const float* max_probs, const long long* max_idx, const long long* idx_ulb, float p_cutoff,
                         long long* selected_label, int* hist, float* classwise_acc, float* mask, int B, int C,
                         int ulb_dest_len, int thresh_warmup, void* stream);
/* n_pass consecutive masking calls on the same idx_ulb (the data_generator passes of one step, srflexmatch.py:75-104) in one launch, in
 * order: max_probs / max_idx / mask are [n_pass, B]; identical to n_pass srhip_flexmatch_mask calls. */
int srhip_flexmatch_mask_passes(const float* max_probs, const long long* max_idx, const long long* idx_ulb, float p_cutoff,
                                long long* selected_label, int* hist, float* classwise_acc, float* mask, int n_pass, int B, int C,
                                int ulb_dest_len, int thresh_warmup, void* stream);
/* bit 0: an idx_ulb entry outside [0, ulb_dest_len) reached srhip_flexmatch_mask[_passes] since the last reset (the reference raises
 * IndexError from the index_put at srflexmatch/utils.py:59; here the entry is skipped).  SYNCHRONISES the stream. */
int srhip_index_error(int* bits_out, int reset, void* stream);
int srhip_flexmatch_rebuild_hist(const long long* selected_label, int* hist, int ulb_dest_len, int C, void* stream);
/* FixedThresholdingHook.masking (semilearn/algorithms/hooks/masking.py:42-57). */
int srhip_fixed_mask(const float* max_probs, float p_cutoff, float* mask, int B, void* stream);
/* FreeMatchThresholdingHook (semilearn/algorithms/freematch/utils.py:24-66), split so that data-parallel ranks can all-reduce
 * the sufficient statistics instead of all-gathering probabilities:
 *   stats : colsum[c] = sum_i probs[i,c], hist[c] = #{i : argmax_i = c} of the LOCAL batch;
 *   update: time_p / p_model / label_hist EMA from the GLOBAL statistics (maxp_all [n_all] = gathered max-probs, colsum, hist),
 *           then mask[i] = max_probs[i] >= time_p * p_model[idx_i] / max(p_model) for the local rows.  n_all <= 1024. */
int srhip_freematch_stats(const float* probs, const long long* max_idx, float* colsum, float* hist, int B, int C, void* stream);
int srhip_freematch_update(const float* maxp_all, int n_all, const float* colsum, const float* hist, const float* max_probs,
                           const long long* max_idx, float* time_p, float* p_model, float* label_hist, float* mask, int B, int C,
                           float momentum, float one_minus_momentum, int use_quantile, int clip_thresh, void* stream);
/* SoftMatch.  Distributed ranks all-reduce the column sums / gather the max-probs (as for FreeMatch) and call these.
 * distalign: DistAlignEMAHook.dist_align (semilearn/algorithms/hooks/dist_align.py:26-56): p_model <- EMA of colsum_ulb / n_ulb (first call:
 *   plain mean; *inited is a device flag, 0 before the first call), p_target <- EMA of colsum_lb / n_lb when colsum_lb != NULL
 *   (p_target_type 'model'); aligned[i,:] = probs[i,:] * (p_target + 1e-6) / (p_model + 1e-6), renormalised; max_probs / max_idx of it.
 * softmatch_mask: SoftMatchWeightingHook.update + masking (semilearn/algorithms/srsoftmatch/utils.py:32-76, per_class False): mu_var[0..1]
 *   <- EMA of mean / unbiased variance of maxp_all [n_all] (.item() double arithmetic reproduced), mask[i] = exp(-clamp(p_i - mu, max 0)^2 /
 *   (2 var / n_sigma^2)). */
int srhip_distalign(const float* probs, const float* colsum_ulb, int n_ulb, const float* colsum_lb, int n_lb, float* p_model,
                    float* p_target, int* inited, double momentum, float* aligned, float* max_probs, long long* max_idx, int B, int C,
                    void* stream);
int srhip_softmatch_mask(const float* maxp_all, int n_all, const float* max_probs, float* mu_var, double momentum, int n_sigma, float* mask,
                         int B, void* stream);
/* entropy_loss (semilearn/algorithms/srfreematch/srfreematch.py:16-44) forward + analytic backward on the masked rows of the strong
 * logits; loss = 0 and no gradient when the mask is empty (:216-219).  ws: B*C floats.  accumulate != 0: dlogits += . */
int srhip_freematch_entropy(const float* logits, const float* mask, const float* p_model, const float* label_hist, float grad_scale,
                            float* loss_out, float* dlogits, float* ws, int B, int C, int accumulate, void* stream);
/* mask2 = (reward >= reward.mean()) per independent group of B rows (srflexmatch.py:100-101) (K11).
 * mean_in (optional, [groups]) overrides the local mean: data-parallel global-threshold extension.  groups * B < 2^31. */
int srhip_reward_mask2(const float* reward, float* mask2, float* mean_out, const float* mean_in, int groups, int B,
                       void* stream);
/* ce_loss / consistency_loss forward + analytic backward (semilearn/core/criterions/cross_entropy.py:11-31,
 * consistency.py:38-45): loss = mean_B(nll*mask*mask2); dlogits = grad_scale*(softmax-onehot)*mask*mask2/B. */
int srhip_masked_ce(const float* logits, const long long* targets, const float* mask, const float* mask2, float grad_scale,
                    float* loss_out, float* dlogits, int B, int C, void* stream);
/* The rest of the criterion surface (criterions.hip), forward + analytic backward, one wave per row, fp32, fixed-order batch reduction
 * (run-to-run bit-identical).  Per row b, with w_b = mask[b] * mask2[b] (each optional):
 *   ce_hard:          l_b = -log_softmax(z_b)[y_b]                       d l_b / d z = softmax(z_b) - onehot(y_b)
 *   ce_soft:          l_b = sum_c -t_bc log_softmax(z_b)_c               d l_b / d z = softmax(z_b) * sum_c t_bc - t_b   (t not normalised)
 *   consistency_mse:  p = softmax(z_b), l_b = mean_c (p_c - t_bc)^2      d l_b / d z = (2 / C) p * ((p - t_b) - sum_c p_c (p_c - t_bc))
 *   consistency_l1:   l_b = mean_c |z_bc - t_bc|                         d l_b / d z = sign(z_b - t_b) / C, sign(0) = 0
 * logits fp32 [B, C] with row stride ld (elements, >= C); soft targets fp32 [B, C] with row stride ldt; hard targets int64 [B].
 * loss_rows (optional, [B]) = l_b * w_b.  loss (optional, [1]) = sum_b l_b w_b, divided by B for SRHIP_REDUCE_MEAN (over ALL rows, as
 * consistency.py:45).  dlogits (optional, row stride ldd; NULL = no gradient) = grad_scale * w_b * r * d l_b / d z with r = 1 / B for
 * MEAN and 1 for SUM and NONE (for NONE the caller's per-row upstream weights go in through mask).  B <= 64 rows, or loss without
 * loss_rows, run as ONE workgroup and one launch; otherwise one row per wave across the device plus a one-workgroup reduction of loss_rows. */
#define SRHIP_REDUCE_NONE 0
#define SRHIP_REDUCE_MEAN 1
#define SRHIP_REDUCE_SUM 2
int srhip_ce_hard(const float* logits, long long ld, const long long* targets, const float* mask, const float* mask2, float grad_scale,
                  int reduction, float* loss_rows, float* loss, float* dlogits, long long ldd, int B, int C, void* stream);
int srhip_ce_soft(const float* logits, long long ld, const float* targets, long long ldt, const float* mask, const float* mask2,
                  float grad_scale, int reduction, float* loss_rows, float* loss, float* dlogits, long long ldd, int B, int C, void* stream);
int srhip_consistency_mse(const float* logits, long long ld, const float* targets, long long ldt, const float* mask, const float* mask2,
                          float grad_scale, int reduction, float* loss_rows, float* loss, float* dlogits, long long ldd, int B, int C,
                          void* stream);
int srhip_consistency_l1(const float* logits, long long ld, const float* targets, long long ldt, const float* mask, const float* mask2,
                         float grad_scale, int reduction, float* loss_rows, float* loss, float* dlogits, long long ldd, int B, int C,
                         void* stream);

/* Evaluation tail (semilearn/core/algorithmbase.py:377-457) of one batch in ONE launch, accumulated on the device (eval.hip).  logits fp32
 * [B, C] with row stride ld (elements, >= C), y int64 [B].  Per row b, in fp32 with the row maximum subtracted first:
 *   loss_b = logsumexp(z_b) - z_b[y_b]              pred_b = the first maximal column, a NaN counting as maximal (numpy / torch argmax)
 * The caller owns and zeroes the accumulators:
 *   confusion int32 [C + 1, C]: += 1 at [y_b, pred_b]; rows with y_b == -1 (ignore_index, :407) count in row C and stay out of the loss.
 *   state (8-byte aligned) = { double loss_sum, nll_sum; long long rows, kept; }:
 *     loss_sum += (sum of loss_b over the kept rows, y_b >= 0) / max(kept_in_batch, 1) * B   -- `loss.item() * num_batch` (:413), 0 for a batch
 *     without kept rows; nll_sum += the same sum undivided; rows += rows counted in confusion; kept += kept_in_batch.
 *   pred_out (optional, NULL = none) int64: pred_out[row_offset + b] = pred_b, for every row.
 * A label < -1 or >= C (F.cross_entropy raises) sets bit 4 of the word srhip_label_error reads and the row reaches no accumulator.
 * One workgroup, one wave per row; the batch sum is added in a fixed order in fp64 by one thread and launches of one stream are ordered:
 * run-to-run bit-identical, no float atomics (the confusion counts are integer atomics).  1 <= B <= 65535, C >= 1. */
int srhip_eval_accumulate(const float* logits, long long ld, const long long* y, int* confusion, void* state, long long* pred_out,
                          long long row_offset, int B, int C, void* stream);

/* Pseudo-label quality monitor (``monitor_pseudo_labels: True``, pl_monitor.hip): what ONE training step's masks, pseudo labels, rewards and
 * reward filter say about the true labels of the unlabelled rows, added into device-resident counters by one launch.  K = P - 1 is the step's
 * number of data_generator passes (srflexmatch.py:72-104); the step keeps the loss of pass K.
 *   pseudo      int64 [P * nu]   argmax of the weak rows of every pass (pass p at p * nu)
 *   mask0       fp32 [nu]        the confidence mask of pass 0 (what util_ratio describes)
 *   mask_kept   fp32 [nu]        the confidence mask of pass K (== mask0 when K == 0); the masks of the passes between are not read
 *   mask2       fp32 [K * nu]    the reward filter of the data_generator passes; NULL when K == 0
 *   reward      fp32 [K * nu]    the rewarder's scores of the data_generator passes; NULL when K == 0
 *   idx_ulb     int64 [nu]       the rows' positions in the unlabelled set
 *   ulb_targets int64 [n_ulb]    the true labels of the unlabelled set, -1 = unknown
 * Weak row j, y = ulb_targets[idx_ulb[j]]:
 *   idx_ulb[j] outside [0, n_ulb) or y >= C: the row reaches no counter and bit 5 of the word srhip_label_error reads is set; nothing is read
 *   out of bounds.  y < 0: rows_unknown += 1 and the row reaches nothing else.  Otherwise
 *   kept pass   pl = pseudo[K * nu + j]; w = mask_kept[j] (K == 0) or mask_kept[j] * mask2[(K - 1) * nu + j], ONE fp32 product as the
 *               consistency loss takes it.  rows += 1, rows_correct += (pl == y), sel += (w > 0), sel_correct += (w > 0 && pl == y),
 *               sum_w += w, sum_w_correct += w where pl == y, and for w > 0 and 0 <= pl < C: sel_by_class[pl] += 1,
 *               sel_correct_by_class[pl] += (pl == y)
 *   pass 0      conf_sel += (mask0[j] > 0), conf_sel_correct += (mask0[j] > 0 && pseudo[j] == y)
 *   every data_generator pass g = 0 .. K - 1:  r = reward[g * nu + j], ok = (pseudo[(g + 1) * nu + j] == y):
 *               gen_rows += 1, gen_correct += ok, m2 += (mask2[g * nu + j] > 0), m2_correct += (mask2 > 0 && ok);
 *               0 <= r <= 1: hist[ok][min((int)(r * 32.0f), 31)] += 1 (r * 32 is exact in fp32) and sum_r[ok] += r;
 *               any other r (NaN included): reward_bad += 1, neither binned nor summed
 * and steps += 1 per launch.
 * State, the caller's, zeroed by the caller, both blocks 8-byte aligned:
 *   istate int64 [16 + 2 * C + 64]:
 *     [0] steps  [1] rows  [2] rows_correct  [3] sel  [4] sel_correct  [5] conf_sel  [6] conf_sel_correct  [7] rows_unknown  [8] gen_rows
 *     [9] gen_correct  [10] reward_bad  [11] m2  [12] m2_correct  [13 .. 15] reserved (never written)
 *     [16, 16 + C) sel_by_class   [16 + C, 16 + 2 C) sel_correct_by_class
 *     [16 + 2 C, + 32) hist[0] (wrong pseudo labels)   [16 + 2 C + 32, + 32) hist[1] (right pseudo labels)
 *   fstate double [4]: sum_w, sum_w_correct, sum_r[0] (wrong), sum_r[1] (right)
 * One workgroup; the rows' true labels staged in LDS once (rows j < 2048; gathered at every use beyond); integer counters in registers /
 * LDS (per-class counters in LDS for C <= 2048, global 64-bit integer atomics beyond); the fp64
 * sums are added per thread in element order, then over a fixed tree: no float atomics, a launch on equal inputs gives equal bits, whether
 * reward / mask2 are 16-byte aligned (16-byte loads, the end peeled) or not.  Launches that share a state must be ordered (one stream).
 * SR_EINVAL before any launch: a null pointer other than mask2 / reward, P <= 0, nu <= 0, C <= 0, n_ulb <= 0, P > 1 with a NULL mask2 or
 * reward, P * nu >= 2^31, C > 2^28, a state / int64 pointer that is not 8-byte aligned. */
int srhip_pl_monitor(const long long* pseudo, const float* mask0, const float* mask_kept, const float* mask2, const float* reward,
                     const long long* idx_ulb, const long long* ulb_targets, long long n_ulb, int P, int nu, int C, long long* istate,
                     double* fstate, void* stream);

/* Scoring a whole unlabelled set without touching training state (AlgorithmBase.score_unlabeled, score_rows.hip).
 *
 * srhip_score_rows: one batch of logits, fp32 [B, C] with row stride ld (elements, >= C; the base need not be 16-byte aligned), and the
 * threshold rule's state, READ ONLY.  Per row b, all outputs dense [B]:
 *   label int64, conf fp32   argmax and max of softmax(z_b): the bits srhip_row_max gives (the row-softmax body is shared, csrc/row_softmax.h;
 *                            the first column wins a tie; a row of NaNs gives 0x7fffffff / -inf as there).  SOFT with the three da_*
 *                            pointers and *da_inited != 0: taken from the aligned, renormalised probabilities
 *                            q_c = p_c (da_p_target[c] + 1e-6) / (da_p_model[c] + 1e-6), q / sum(q), the bits srhip_distalign gives; so are margin
 *                            and entropy.  *da_inited == 0: unaligned.  da_p_model / da_p_target are not written.
 *   margin fp32              conf - the second largest probability: 0 for a tie at the top, conf for C == 1
 *   entropy fp32             -sum_c p_c ln p_c with 0 ln 0 = 0
 *   weight fp32              the rule's mask / weight from the state as it stands, no update, in the expression order of the hook kernels:
 *     SRHIP_SCORE_FIXED  conf >= p_cutoff                                                   (masking.py:42-57, srhip_fixed_mask)
 *     SRHIP_SCORE_FLEX   conf >= p_cutoff * (acc / (2 - acc)), acc = classwise_acc[label]   (srflexmatch/utils.py:50-56, srhip_flexmatch_mask)
 *     SRHIP_SCORE_FREE   conf >= time_p[0] * (p_model[label] / max(0, max_c p_model[c]))    (freematch/utils.py:24-66, srhip_freematch_update)
 *     SRHIP_SCORE_SOFT   exp(-(min(conf - mu, 0)^2 / ((2 var) / n_sigma^2))), (mu, var) = mu_var[0..1]   (srsoftmatch/utils.py:32-76)
 *     a label outside [0, C) (the row of NaNs) gives weight 0 in FLEX and FREE.
 * One wave per row, four rows per workgroup; rows of C <= 1024 live in registers, longer ones are re-read; 16-byte loads with head and tail
 * peeled; no atomics: equal inputs give equal bits.
 * SR_EINVAL before any launch: a NULL logits / output pointer, B outside 1 .. 65535, C < 1, ld < C, an unknown mode, a state pointer the mode
 * needs that is NULL (FLEX classwise_acc; FREE time_p, p_model; SOFT mu_var, n_sigma >= 1; the da_* pointers all three or none), label not
 * 8-byte aligned.
 *
 * srhip_score_commit: scatters one scored batch into device tables of length n.  Row b goes to entry j = idx[b], or row_offset + b when idx is
 * NULL: t_label / t_conf / t_margin / t_entropy / t_weight / t_reward [j] = the batch's values, t_reward_keep[j] = (reward_keep[b] > 0) with
 * reward_keep the fp32 mask srhip_reward_mask2 wrote for the row's reward group, t_selected[j] = (weight[b] > 0 && reward_keep[b] > 0),
 * t_count[j] += 1 (integer atomic).  A j outside [0, n) is skipped and sets bit 6 of the word srhip_label_error reads.  idx must be unique
 * within a launch; across launches of one stream the later one wins, and t_count > 1 shows the repeat.
 * SR_EINVAL before any launch: a NULL pointer other than idx, B outside 1 .. 65535, n < 1, idx NULL with row_offset < 0, label / t_label /
 * idx not 8-byte aligned. */
#define SRHIP_SCORE_FIXED 0
#define SRHIP_SCORE_FLEX 1
#define SRHIP_SCORE_FREE 2
#define SRHIP_SCORE_SOFT 3
int srhip_score_rows(const float* logits, long long ld, int B, int C, int mode, float p_cutoff, const float* classwise_acc,
                     const float* time_p, const float* p_model, const float* mu_var, int n_sigma, const float* da_p_model,
                     const float* da_p_target, const int* da_inited, long long* label, float* conf, float* margin, float* entropy,
                     float* weight, void* stream);
int srhip_score_commit(const long long* label, const float* conf, const float* margin, const float* entropy, const float* weight,
                       const float* reward, const float* reward_keep, const long long* idx, long long row_offset, int B, long long n,
                       long long* t_label, float* t_conf, float* t_margin, float* t_entropy, float* t_weight, float* t_reward,
                       unsigned char* t_reward_keep, unsigned char* t_selected, int* t_count, void* stream);
/* srhip_reward_mask2 over `total` rows in groups of B, the last group holding the rows that are left (its own mean over those rows). */
int srhip_reward_mask2_ragged(const float* reward, float* mask2, float* mean_out, int total, int B, void* stream);
/* The opt-in top-k reward filter (reward_filter: topk; the reference has the mean rule only).  `total` rows in `groups` groups of B, the last
 * group holding the total - (groups - 1) * B rows that are left.  Per group, the rows are ordered: non-NaN before NaN, larger reward first
 * with -0 == +0, lower index first among equal rewards; mask2[i] = 1.0 for the first min(kk, non-NaN rows of the group) rows of that order
 * and 0.0 for the rest, with kk = k, and k_last for the last group.  A NaN reward is never kept; kk >= rows keeps every non-NaN row.
 * Equivalently rank(i) = #{j : c(j) > c(i)} on c = (ordered_key(reward) << 32) | (0xFFFFFFFF - index), ordered_key the sign-flip map of the
 * fp32 bits with NaN mapped to 0 and -0 canonicalised, and row i is kept iff rank(i) < kk and reward[i] is no NaN.
 * peers (optional, fp32 [n_peers, groups * B], the tables of the data-parallel ranks, peers[self_peer] equal to reward): the candidates of a
 * group are its rows on ALL peers, the index of a candidate is peer * B + row, kk counts over all of them, and the mask is written for the
 * caller's own rows only.  peers NULL: n_peers 0 or 1, self_peer 0.
 * One launch, no atomics, no sort, no host synchronisation, no allocation: capturable, equal inputs give equal bits; exactly the `total`
 * words of mask2 are written.  O(B * B * n_peers) compares per group.
 * SR_EINVAL before any launch: reward or mask2 NULL, groups / B / total < 1, k or k_last < 1, groups != ceil(total / B), groups * B >= 2^31,
 * B * n_peers > 65536, self_peer outside [0, n_peers). */
int srhip_reward_topk_mask(const float* reward, float* mask2, int groups, int B, int total, int k, int k_last, const float* peers,
                           int n_peers, int self_peer, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Rewarder / Generator (K10, K14, K15).  params: flat fp32 block in named_parameters() order.
 * Rewarder.forward (semilearn/algorithms/semireward/semireward.py:52-72) for G independent groups of B rows
 * (each group has its own softmax over its 2B rows): feats [G*B,F], labels int64 [G*B] -> reward [G*B].
 * ws: fp32 scratch of srhip_rewarder_ws_floats(G,B) floats; save_for_bwd needs G == 1. */
long srhip_rewarder_param_count(int F, int L);
long srhip_rewarder_ws_floats(int G, int B);
long srhip_generator_param_count(int F);
/* params_t: transposed copies of the 2-D weights, streamed coalesced by the forward kernels; size
 * srhip_rewarder_t_floats(F) / srhip_generator_t_floats(F); refresh with *_prepare after every parameter change. */
long srhip_rewarder_t_floats(int F);
long srhip_generator_t_floats(int F);
int srhip_rewarder_prepare(const float* params, float* params_t, int F, int L, void* stream);
int srhip_generator_prepare(const float* params, float* params_t, int F, void* stream);
int srhip_rewarder_fwd(const float* params, const float* params_t, const float* feats, const long long* labels, float* reward,
                       float* ws, int G, int B, int F, int L, int save_for_bwd, void* stream);
/* The same with the feature rows of group g at feats + g * feat_group_stride (elements; >= B * F): the weak-row block of every pass read in
 * place from the step's [passes, batch, F] feature buffer.  Both entries run as ONE launch when a group is one row tile (B <= 8, the
 * reference batch), two otherwise (the batch softmax over a group's 2B attention logits, semireward.py:60-62, is the only dependency
 * between workgroups).  max_reward_inout (device scalar or NULL; G == 1 and B <= 8 only): *max_reward = max(*max_reward, mean(reward)) in
 * the same launch -- `reward.mean()` and the running maximum of srflexmatch.py:166-170. */
int srhip_rewarder_fwd_strided(const float* params, const float* params_t, const float* feats, long long feat_group_stride,
                               const long long* labels, float* reward, float* ws, float* max_reward_inout, int G, int B, int F, int L,
                               int save_for_bwd, void* stream);
/* Gradient of MSE(r,1) + MSE(r,target) w.r.t. every rewarder parameter (srflexmatch.py:183-190 / :198-205);
 * grads is overwritten; losses[0..1] = (generator_loss, rewarder_loss) when non-NULL. */
int srhip_rewarder_bwd(const float* params, const float* feats, const long long* labels, const float* target, float* ws,
                       float* grads, float* losses, int B, int F, int L, void* stream);
/* Generator.forward (semireward.py:21-24) and the .long() cast (srflexmatch.py:158-159). */
int srhip_generator_fwd(const float* params, const float* params_t, const float* x, float* out, long long* label, int B, int F,
                        void* stream);
/* (cosine_similarity_n(one_hot, one_hot)+1)/2 (semireward.py:130-139, srflexmatch.py:180-182): 1.0 / 0.5. */
int srhip_sr_target(const long long* gen, const long long* ref, float* target, int B, int num_classes, void* stream);
/* Label-range errors of the launches above since the last reset.  The reference raises from nn.Embedding / F.one_hot when a (generated or
 * pseudo) label is outside [0, label_dim) (semireward.py:57, srflexmatch.py:180-181); the kernels stay memory safe (row 0 is read, the
 * gradient scatter is skipped), set a bit in a device word and the host raises when it reads it here (SYNCHRONISES the stream):
 * bit 0 embedding lookup, bit 1 embedding-gradient scatter, bit 2 generator output NaN / not representable as int64, bit 3 a label outside
 * [0, num_classes) in srhip_sr_target (F.one_hot; num_classes <= 0 disables that check), bit 4 an evaluation label outside [-1, C) in
 * srhip_eval_accumulate, bit 5 an idx_ulb outside [0, n_ulb) or a true label >= C in srhip_pl_monitor, bit 6 a table index outside [0, n) in
 * srhip_score_commit. */
int srhip_label_error(int* bits_out, int reset, void* stream);
/* torch.optim.Adam step on a flat block (srflexmatch.py:54, :192-193). */
/* "_dyn" entry points: the scalars that change from step to step -- the scheduler's lr factor and Adam's bias corrections (param_update.py:33-40,
 * build.py:227-251), the DropPath seed (vit.py:148,161) -- are read from DEVICE memory written by the host before the step, so that the launches
 * of a training step can be captured once in a HIP graph and replayed (semireward_amd/core/stepgraph.py).  Same arithmetic as the by-value forms.
 *   srhip_adamw_flat_dyn: dyn fp32 [3] = {lr_factor, 1 - beta1^step, sqrt(1 - beta2^step)};  srhip_adam_flat_dyn: dyn fp32 [2] = the two corrections;
 *   srhip_droppath_fill_cols_dyn: seed = *seed_dev + seed_offset. */
int srhip_adam_bias_corrections(float beta1, float beta2, int step, float* out2_host);   /* host helper: the two fp32 values of a dyn block */
int srhip_adamw_flat_dyn(float* p, float* g, float* m, float* v, void* p_bf16, float* ema, const int* chunk_table, int n_chunks,
                         const float* lr_t, const float* wd_t, const float* dyn, float beta1, float beta2, float eps, double ema_m,
                         float grad_scale, const float* clip_coef, int zero_grad, void* stream);
int srhip_adam_flat_dyn(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps, const float* dyn,
                        void* stream);
int srhip_droppath_fill_cols_dyn(float* out, const float* probs, const long long* cols, int depth, int B, int n_cols,
                                 const unsigned long long* seed_dev, unsigned long long seed_offset, void* stream);
int srhip_adam_flat(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                    int step, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Backbone optimizer (K16, K17): ParamUpdateHook (semilearn/core/hooks/param_update.py:33-40) with the AdamW
 * param groups of semilearn/core/utils/build.py:193-224 + semilearn/nets/utils.py:143-204, fused with the bf16
 * operand refresh, EMA.update (semilearn/core/utils/misc.py:152-155) and model.zero_grad().
 * chunk_table int32 [n_chunks][4] = (offset, length, tensor id, 0); lr_t / wd_t fp32 per tensor;
 * grad_scale multiplies g first (1/world_size after a data-parallel SUM all-reduce); clip_coef (device, 1 float, may be NULL) multiplies
 * it once more: the clip_grad_norm_ coefficient of this step.  ema (may be NULL) <- (1 - ema_m) * p_new + ema_m * ema, op for op as
 * semilearn/core/utils/misc.py:152-155 (ema_m is a double because the reference forms 1 - decay in double before rounding). */
int srhip_adamw_flat(float* p, float* g, float* m, float* v, void* p_bf16, float* ema, const int* chunk_table, int n_chunks,
                     const float* lr_t, const float* wd_t, float lr_factor, float beta1, float beta2, float eps, int step,
                     double ema_m, float grad_scale, const float* clip_coef, int zero_grad, void* stream);
/* torch.nn.utils.clip_grad_norm_(model.parameters(), clip_grad) of ParamUpdateHook (semilearn/core/hooks/param_update.py:34-35) on the flat
 * gradient block: coef_out[0] = min(1, max_norm / (|| pre_scale * g ||_2 + 1e-6)), coef_out[1] = that norm; ws = srhip_clip_grad_ws_floats()
 * floats.  The gradients are NOT rewritten: the optimizer launch takes coef_out as ``clip_coef``. */
int srhip_clip_grad_ws_floats(void);
int srhip_clip_grad_coef(const float* g, long long n, float pre_scale, float max_norm, float* ws, float* coef_out, void* stream);

/* ---- post-LN transformer encoder glue (BERT / Wav2Vec2 backbones; semilearn/nets/bert/bert.py, wave2vecv2/wave2vecv2.py and the HF modules
 * they call).  D in {128, 384, 768}; dropout arguments as in srhip_gemm_nt_resid_dropout (one 32-bit decision per element) with element index = row * D + column.
 *   embed_ln_fwd : BertEmbeddings -- x = dropout(LayerNorm(word[ids[seq][p]] + pos[p] + type0)) for row (b, p) of a [B, L] batch; ids int64
 *                  [*, ld_ids], seq_index int32 [B] picks the row of ids (NULL: identity); x fp32 and bf16 [B*L, D]; mean/rstd [B*L] optional
 *   embed_ln_bwd : its backward from dy = d/dx: dword[id] += (rows with id == pad_id excluded: nn.Embedding(padding_idx)), dpos[p] +=,
 *                  dtype0 +=, dgamma +=, dbeta +=  (atomic)
 *   postln_fwd   : x = LayerNorm(y) as fp32 (next residual) and bf16 (next GEMM operand); x may alias y
 *   postln_bwd   : dy = d/d(LayerNorm output) -> dx = d/dy fp32 (may alias dy) and dx_bf16 = dropout-masked dx (the gradient of the branch that
 *                  was added under dropout: operand of its dX / dW products); dgamma +=, dbeta += (atomic)
 *   meanpool_fwd : feat[b] = mean over ALL L rows of dropout(x[b])  (bert.py:36-37, padding included);  meanpool_bwd: dx = its adjoint.
 *                  seq_len int32 [B] (NULL: L): the padded length of every sequence's OWN batch when differently padded batches (x_lb, x_ulb_w,
 *                  x_ulb_s of a use_cat=False config) share one launch padded to L -- rows >= seq_len[b] are filler: not averaged, zero gradient
 *   gelu_f32 / gelu_bwd_f32 : nn.GELU() between the classifier Linears (bert.py:16-20; the Linears are srhip_fc_fwd / srhip_fc_bwd)
 *   mask_lengths : key_len[b] = sum(attention_mask[b, :]) for the right-padded batches of nlp_collactor.py:63-69 */
int srhip_embed_ln_fwd(const long long* ids, int ld_ids, const int* seq_index, const float* word, const float* pos, const float* type0,
                       const float* gamma, const float* beta, float eps, float* x, void* x_bf16, float* mean, float* rstd, int B, int L, int D,
                       unsigned drop_key, unsigned drop_thresh, float drop_scale, void* stream);
int srhip_embed_ln_bwd(const float* dy, const long long* ids, int ld_ids, const int* seq_index, const float* word, const float* pos,
                       const float* type0, const float* mean, const float* rstd, const float* gamma, float* dword, float* dpos, float* dtype0,
                       float* dgamma, float* dbeta, int B, int L, int D, int pad_id, unsigned drop_key, unsigned drop_thresh, float drop_scale,
                       void* stream);
/* The same backward with ONE summation order: two launches and no atomics (csrc/enc_ops.hip) -- every table row is summed over the token rows
 * that hold its id in row order, every position over the sequences in order, dgamma / dbeta / dtype0 over workgroups of 32 rows in order.  Equal
 * inputs give equal bits, and a row whose upstream gradient is exactly zero changes no bit whatever id it holds.  ws: scratch of
 * srhip_embed_ln_bwd_ws_floats(B, L, D) floats, 16-byte aligned, nothing kept between calls.  SR_EINVAL as srhip_embed_ln_bwd, and a null or
 * misaligned ws. */
long srhip_embed_ln_bwd_ws_floats(int B, int L, int D);
int srhip_embed_ln_bwd_ordered(const float* dy, const long long* ids, int ld_ids, const int* seq_index, const float* word, const float* pos,
                               const float* type0, const float* mean, const float* rstd, const float* gamma, float* dword, float* dpos,
                               float* dtype0, float* dgamma, float* dbeta, float* ws, int B, int L, int D, int pad_id, unsigned drop_key,
                               unsigned drop_thresh, float drop_scale, void* stream);
int srhip_postln_fwd(const float* y, const float* gamma, const float* beta, float eps, float* x, void* x_bf16, float* mean, float* rstd, int M,
                     int D, void* stream);
int srhip_postln_bwd(const float* dy, const float* y, const float* mean, const float* rstd, const float* gamma, float* dx, void* dx_bf16,
                     float* dgamma, float* dbeta, int M, int D, unsigned drop_key, unsigned drop_thresh, float drop_scale, void* stream);
/* postln_bwd with dgamma / dbeta spread over n_rep partial copies part fp32 [n_rep][2][D] (see srhip_layernorm_bwd_part; folded by
 * srhip_ln_grad_reduce after the last layer). */
int srhip_postln_bwd_part(const float* dy, const float* y, const float* mean, const float* rstd, const float* gamma, float* dx, void* dx_bf16,
                          float* part, int n_rep, int M, int D, unsigned drop_key, unsigned drop_thresh, float drop_scale, void* stream);
int srhip_meanpool_fwd(const float* x, float* feat, const int* seq_len, int B, int L, int D, unsigned drop_key, unsigned drop_thresh,
                       float drop_scale, void* stream);
int srhip_meanpool_bwd(const float* dfeat, float* dx, const int* seq_len, int B, int L, int D, unsigned drop_key, unsigned drop_thresh,
                       float drop_scale, void* stream);
int srhip_gelu_f32(const float* pre, float* out, long n, void* stream);
int srhip_gelu_bwd_f32(const float* dout, const float* pre, float* dpre, long n, void* stream);
int srhip_mask_lengths(const long long* mask, int ld, int* key_len, int B, int L, void* stream);
/* out(bf16)[i] = dropout'(x[i]): the gradient of a branch that sat under nn.Dropout, cast for its dX / dW products (element index i) */
int srhip_dropout_cast(const float* x, void* out_bf16, long n, unsigned drop_key, unsigned drop_thresh, float drop_scale, void* stream);

/* gemm_nt with nn.Dropout in the epilogue (generator / index as srhip_attn_masked_fwd, element index m * N + n, ldc == N):
 *   SRHIP_EPI_GELU_BF16  : C = dropout(GELU(acc + bias)), aux_out = acc + bias        (Wav2Vec2FeedForward.intermediate_dropout)
 *   SRHIP_EPI_DGELU_BF16 : C = dropout'(acc) * GELU'(aux_in)                           (its adjoint)
 *   SRHIP_EPI_RESID_F32  : as srhip_gemm_nt_resid_dropout */
int srhip_gemm_nt_dropout(int epilogue, const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K, const float* bias,
                          const void* aux_in, void* aux_out, int ldaux, unsigned drop_key, unsigned drop_thresh, float drop_scale, void* stream);

/* ---- Wav2Vec2 front end (semilearn/nets/wave2vecv2/wave2vecv2.py:44 -> transformers Wav2Vec2Model: feature encoder, feature projection,
 * SpecAugment, positional conv embedding).  Activations are channel-last [clip, frame, channel] with a per-layer frame pitch P_l (P_{l-1} =
 * stride_l * P_l, P_l >= T_l + 1): the conv layers 1.. are srhip_gemm_nt products whose A operand is the previous activation read with
 * lda = stride * C (overlapping rows) against the tap-major filter; rows >= T_l are filler (finite forward, zero in every gradient).
 *   w2v_conv0            : layer 0 (1 input channel) + GroupNorm(groups == channels) + GELU.  mode 0: statistics into ws (2 doubles per (clip,
 *                          channel), zeroed by the caller); 1: out bf16 [B*P0, C]; 2: backward statistics into ws2 from dY (bf16, d/d out),
 *                          dgamma +=, dbeta +=; 3: dW0 [C, k] +=
 *   w2v_conv_weight_prep : Conv1d filter fp32 [Cout, Cin, k] -> bf16 Wr [Cout, k*Cin] (tap-major) and WrT [k*Cin, Cout]; wgrad_add: the inverse
 *                          permutation, dW += sum of the n_part partial products dWr [n_part, Cout, k*Cin] (the weight-gradient product is
 *                          split over the frames to fill the chip)
 *   w2v_col2im_dgelu     : adjoint of the overlapping-row read: dpre_prev = GELU'(pre_prev) * fold(dcol)   (pre_prev NULL: no GELU factor)
 *   w2v_featln_fwd/bwd   : feature_projection.layer_norm on the bf16 conv output; the backward also applies GELU'(pre) of the last conv layer
 *   w2v_spec_mask_fwd/bwd: masked frames <- masked_spec_embed; backward: dx (+= add, the positional-conv input gradient with pitch Padd),
 *                          masked rows -> dembed, filler rows -> 0
 *   w2v_pos_stage        : group-major zero-padded bf16 copy [groups][rows_total][D/groups] of fp32 rows (frame t lands on row clip*Pp + t +
 *                          pad_left): operand of the grouped positional conv (srhip_gemm_nt_grouped_f32, lda = D/groups)
 *   w2v_weightnorm_prep  : weight_norm(dim=2) filter -> bf16 operands Wf [groups][cg][k][cg] and the tap-reversed transpose Wb; norms [k]
 *   w2v_weightnorm_bwd   : dv +=, dg += from dWf (fp32, Wf layout); ws: caller-owned workspace of (D + 1) * k floats
 *   w2v_pos_finish_fwd   : x0 = dropout(LayerNorm(x + GELU(conv + bias))) fp32 + bf16 (filler rows zero); saves y, mean, rstd
 *   w2v_pos_finish_bwd   : dx0 -> dy (in place), dconv = dy * GELU'(conv + bias) fp32 [B*P, D]; dgamma +=, dbeta += */
int srhip_w2v_conv0(int mode, const float* wave, const float* W0, const float* gamma, const float* beta, double* ws, double* ws2, void* out_bf16,
                    const void* dY, float* dW0, float* dgamma, float* dbeta, int B, int S, int T0, int P0, int C, int k, int stride, float eps,
                    void* stream);
int srhip_w2v_conv_weight_prep(const float* W, void* Wr, void* WrT, int Cout, int Cin, int k, void* stream);
int srhip_w2v_conv_wgrad_add(const float* dWr, float* dW, int Cout, int Cin, int k, int n_part, void* stream);
int srhip_w2v_col2im_dgelu(const void* dcol, const void* pre_prev, void* out, int B, int Pl, int Pprev, int C, int k, int stride, void* stream);
int srhip_w2v_featln_fwd(const void* x, const float* gamma, const float* beta, float eps, void* out, float* mean, float* rstd, int B, int T, int P,
                         int C, void* stream);
int srhip_w2v_featln_bwd(const void* dy, const void* x, const void* pre, const float* mean, const float* rstd, const float* gamma, void* dpre,
                         float* dgamma, float* dbeta, int B, int T, int P, int C, void* stream);
int srhip_w2v_spec_mask_fwd(float* x, const unsigned char* mask, const float* embed, long M, int D, void* stream);
int srhip_w2v_spec_mask_bwd(float* dx, const float* add, const unsigned char* mask, float* dembed, int B, int T, int P, int Padd, int D, void* stream);
int srhip_w2v_pos_stage(const float* src, void* out, int B, int T, int P, int Pp, int D, int groups, int pad_left, long rows_total, void* stream);
int srhip_w2v_weightnorm_prep(const float* v, const float* g, float* norms, void* Wf, void* Wb, int D, int groups, int k, void* stream);
int srhip_w2v_weightnorm_bwd(const float* dWf, const float* v, const float* g, const float* norms, float* dv, float* dg, float* ws, int D,
                             int groups, int k, void* stream);
int srhip_w2v_pos_finish_fwd(const float* x, const float* conv, const float* conv_bias, const float* gamma, const float* beta, float eps, float* x0,
                             void* x0_bf16, float* ysave, float* mean, float* rstd, int B, int T, int P, int Pp, int D, unsigned drop_key,
                             unsigned drop_thresh, float drop_scale, void* stream);
int srhip_w2v_pos_finish_bwd(float* dx0, const float* ysave, const float* conv, const float* conv_bias, const float* mean, const float* rstd,
                             const float* gamma, float* dconv, float* dgamma, float* dbeta, int B, int T, int P, int Pp, int D, unsigned drop_key,
                             unsigned drop_thresh, float drop_scale, void* stream);

/* ---- device-side augmentation: semilearn/datasets/cv_datasets/cifar.py:34-49 transform_weak / transform_strong and
 * semilearn/datasets/augmentation/randaugment.py:16-196, one launch per batch.  src uint8 [n_src, H0, W0, 3]; per output image b a parameter
 * block ip[b*64..] (int32) / dp[b*32..] (float64):
 *   ip[0..2] crop offset (row, column) in the reflect-padded image and flip flag; ip[3] number of RandAugment ops (<= 4);
 *   ip[4..7] Cutout rectangle x0, y0, x1, y1, both ends inclusive (x0 < 0: none); ip[8] source image index;
 *   op k at ip[16 + 12k]: [0] op id in augment_list() order, [1] 1 = pure translation (float64 walk: dp xo, yo, step x, step y at [1..4]),
 *   [2..7] the 16.16 fixed-point coefficients a0, a1, a2', a3, a4, a5' of Pillow's nearest-neighbour affine walk, [8] Posterize mask;
 *   dp[8k] the magnitude.
 * scratch: 2 * S * S * 3 bytes per image.  out fp32 [B, 3, S, S] = (x / 255 - mean) / std; out_u8 (optional) uint8 [B, S, S, 3] before that.
 * mean3 / std3: HOST pointers to 3 floats.  Bit-exact with Pillow (12.2.0) for every op. */
int srhip_augment(const unsigned char* src, int n_src, int H0, int W0, int B, int S, int pad, const int* ip, const double* dp,
                  unsigned char* scratch, float* out, unsigned char* out_u8, const float* mean3, const float* std3, void* stream);

/* ---- Pillow-exact bilinear resize of a stored uint8 image stack: transforms.Resize(crop_size) on a PIL image, the first op of
 * transform_weak / transform_strong / transform_val (semilearn/datasets/cv_datasets/eurosat.py:66,76,87, cifar.py:35,43,52,
 * stl10.py:43,51,60) = Image.resize((S, S), BILINEAR).  src uint8 [N, H0, W0, 3] -> dst uint8 [N, S, S, 3]; square sources only
 * (H0 != W0: SR_EINVAL).  H0 == S copies the bytes (Pillow skips both passes; the tables may be NULL).  Otherwise
 *   bounds int32 [S, 2]     : first source index and tap count of output index s (the same table serves both axes),
 *   coefs  int32 [S, ksize] : the taps' weights in 22-bit fixed point (Pillow's precompute_coeffs + normalize_coeffs_8bpc, computed in
 *                             float64 on the host: semireward_amd/data/resize.py),
 *   tmp    uint8 [N, H0, S, 3] scratch for the horizontal pass.
 * Integer arithmetic only; byte-exact with Pillow 12.2.0 for shrinking (antialiased) and enlarging. */
int srhip_resize_bilinear_u8(const unsigned char* src, int N, int H0, int W0, unsigned char* dst, int S, const int* bounds, const int* coefs,
                             int ksize, unsigned char* tmp, void* stream);

/* ---- one view of a waveform batch from the device-resident clip store (``device_audio: True``, semireward_amd/data/device_audio.py):
 * random_subsample's window (semilearn/datasets/utils.py:177-183, the offset drawn on the host), the collator's zero padding to S samples and
 * Wav2Vec2FeatureExtractor's normalisation without an attention mask (audio_collactor.py:61-83), one launch.
 *   store    fp32, every clip starts at a multiple of 4 floats;  row_off int64 [n_rows] first float of a clip, row_len int32 [n_rows] its samples
 *   src_row  int64 [B] store row of output row b;  crop_off int32 [B] first sample of its window
 *   out      fp32 [B, ldo], 16-byte aligned, ldo % 4 == 0, ldo >= S; columns S .. ldo are not written
 * With r = src_row[b], n = min(row_len[r] - crop_off[b], S): v[t] = store[row_off[r] + crop_off[b] + t] for t < n, 0 for n <= t < S (a row or an
 * offset outside the store gives n = 0: the kernel never reads past a row; the Python wrapper refuses such arguments on the host).
 *   normalize = 0: out[b, t] = v[t], bit for bit.
 *   normalize = 1: m = sum(v) / S, var = sum((v - m)^2) / S over all S positions, out[b, t] = (v[t] - m) / sqrt(var + 1e-7) -- the padded
 *                  positions too (they become -m / sqrt(var + 1e-7)).  Two passes in fp64 with a fixed reduction order and no atomics
 *                  (run-to-run bit-identical); an element is one fp32 rounding of the float64 value.
 * One workgroup per row.  SR_EINVAL: a null pointer, n_rows <= 0, B <= 0, B > 65535, S <= 0, S > 2^30, ldo < S, ldo % 4, out not 16-byte
 * aligned, normalize not 0 / 1. */
int srhip_wave_view(const float* store, const long long* row_off, const int* row_len, int n_rows, const long long* src_row,
                    const int* crop_off, int B, int S, int normalize, float* out, int ldo, void* stream);

/* ---- one effect slot of the device-made strong waveform view (``device_audio_strong: True``, semireward_amd/data/device_audio.py,
 * csrc/wave_strong.hip).  The chain is the engine's own (tests/_wave_strong_cases.py restates it in float64 numpy and is its specification):
 * it keeps the structure and the draw distributions of the reference's WaveformTransforms (datasetbase.py:12-39), not sox's filters.
 * Addressing as srhip_wave_view: with r = src_row[b], the source is the n = row_len[r] floats at store + row_off[r] (slot 0: the resident clip
 * store; a later slot: the scratch rows the previous slot wrote).  Output row b is dst + b * pitch (fp32, 16-byte aligned, pitch % 4 == 0); the
 * kernel writes exactly dst_len[b] floats of it and nothing else.  op / param / dst_len are DEVICE arrays [B]; host_op / host_param /
 * host_dst_len are the HOST arrays they were copied from, which the entry checks before it launches (the device arrays ride in a loader's one
 * copy per epoch; the kernel writes nothing for a row whose device values the entry would have refused).
 *   SR_WAVE_COPY      out = x, m = n
 *   SR_WAVE_GAIN      param = the fp32 bits of g = 10^(att / 20): out = clamp(x * (g / max |x|), -1, 1), m = n (sox ``gain -n``); an all-zero row is
 *                     copied.  The maximum is exact; an element is the fp32 rounding of the fp64 product x * (g / peak).
 *   SR_WAVE_RESAMPLE  param = step = round(s * 2^32), 2^31 <= step <= 2^33 (speed: s = speed; pitch: s = 2^(cents / 1200), a resample, not
 *                     WSOLA).  m = max(1, (n << 32) / step).  Output j sits at p = j * step (64-bit integers): i0 = p >> 32,
 *                     f = (p & 0xffffffff) 2^-32; c = min(1, 2^32 / step), T = 16 / c;  out[j] = sum_k x[k] h(i0 + f - k) over the integers k of
 *                     [0, n - 1] with |i0 + f - k| < T, k ascending, h(u) = c sinc(c u) (0.5 + 0.5 cos(pi u / T)), weights and sum in fp32, no
 *                     renormalisation at the edges.  step == 2^32 copies bit for bit.
 *   SR_WAVE_REVERB    Freeverb (public domain), mono, wet only, empty state, the tail past n dropped, m = n: in = 0.015 x; eight parallel combs
 *                     (y = buf[idx]; st = 0.8 y + 0.2 st; buf[idx] = in + 0.84 st) summed in comb order; four series allpasses
 *                     (b = buf[idx]; out = b - in; buf[idx] = in + 0.5 b); out * 3.  delays12: HOST pointer to the eight comb and four allpass
 *                     delays in samples (max(1, round(d * sample_rate / 44100)), d = 1116 1188 1277 1356 1422 1491 1557 1617 / 556 441 341 225),
 *                     passed to the kernel by value.  Evaluated in chunks of the shortest delay with the damping recursion as its first 24 terms
 *                     (the remainder is below 0.2^24 of the signal); delay lines in LDS.
 * One 1024-thread workgroup per row, rows of different ops share the launch; no atomics, fixed summation order (run-to-run bit-identical).
 * SR_EINVAL: a null pointer, n_rows <= 0, B <= 0, B > 65535, pitch <= 0, pitch % 4, dst not 16-byte aligned, a host_op outside 0..3, a
 * host_dst_len <= 0 or above pitch, a resample step outside [2^31, 2^33], a delay <= 0, delays whose lines (sum of the comb delays + 8 (23 + C) +
 * sum of the allpass delays + 4 C + 16 C floats, C the shortest delay) do not fit 64 KiB - 256 B of LDS, a shortest delay above 256.  The Python wrapper also checks the rows
 * and lengths against the store, dst_len against the op's length rule and that source and destination are different buffers. */
enum { SR_WAVE_COPY = 0, SR_WAVE_GAIN = 1, SR_WAVE_RESAMPLE = 2, SR_WAVE_REVERB = 3 };
int srhip_wave_effect(const float* store, const long long* row_off, const int* row_len, int n_rows, const long long* src_row, const int* op,
                      const long long* param, const int* dst_len, int B, float* dst, int pitch, const int* host_op, const long long* host_param,
                      const int* host_dst_len, const int* delays12, void* stream);

/* ---- one view of a token batch from the device-resident token store (``device_tokens: True``, semireward_amd/data/device_tokens.py): the
 * collator's ``tokenizer.pad(padding=True)`` (nlp_collactor.py:63-110) on rows tokenised once, and the lengths srhip_mask_lengths would
 * recover from its attention mask, one launch.
 *   store    int32, 16-byte aligned, every row starts at a multiple of 4 ints (a row_off that is no multiple of 4 is still read correctly,
 *            with single loads instead of 16-byte ones);  row_off int64 [n_rows] first int of a row, row_len int32
 *            [n_rows] its tokens;  src_row int64 [B] store row of output row b
 *   ids      int64 [B, ld_ids] (what srhip_embed_ln_fwd takes), ld_ids >= L; columns L .. ld_ids are not written;  key_len int32 [B]
 * With r = src_row[b], n = min(row_len[r], L): ids[b, t] = store[row_off[r] + t] for t < n, pad_id for n <= t < L, key_len[b] = n (a row
 * longer than L is truncated: key_len = L).  A src_row outside [0, n_rows) gives n = 0: an all-pad row, nothing read (the Python wrapper
 * refuses such a row on the host).  The kernel never reads past a row: quads inside a row are aligned 16-byte loads, the quad holding the
 * row's end is peeled.  16-byte stores where the output address allows (ld_ids even), 8-byte stores otherwise.  One workgroup per row, no
 * LDS, no atomics.  SR_EINVAL: a null pointer, n_rows <= 0, B <= 0, B > 65535, L <= 0, ld_ids < L, store not 16-byte aligned,
 * ids not 8-byte aligned. */
int srhip_token_view(const int* store, const long long* row_off, const int* row_len, int n_rows, const long long* src_row, int B, int L,
                     int pad_id, long long* ids, int ld_ids, int* key_len, void* stream);

/* ---- the strong view of a token batch made on the device from the CLEAN sentence (``device_tokens_strong: True``,
 * semireward_amd/data/device_tokens.py): a srhip_token_view row after two token-level slots, one launch.  The chain is the engine's own -- not
 * the reference's back-translation --; tests/_token_strong_cases.py restates it in integers (strong_row_ref).
 *   store / row_off / row_len / src_row / ids / ld_ids / key_len   as srhip_token_view
 *   slot0, slot1   int64 [B]: bits 0..7 op, bits 8..31 the count c, bits 32..63 seed;  Lsrc the longest source row taken (1 .. 4096: the
 *                  row and its keys share LDS, 32 KiB at the cap);  mask_id what SR_TOKEN_MASK writes
 * A row is t[0 .. n - 1], n = min(row_len[r], Lsrc); t[0] ([CLS]) and t[n - 1] ([SEP]) are never moved, changed or removed; the interior is
 * positions 1 .. n - 2, ni = max(0, n - 2) of them.  Slot 0, then slot 1 on the row and the ni that slot 0 left; c is clamped to 0 .. ni:
 *   SR_TOKEN_COPY    nothing (an op above 4 acts the same)
 *   SR_TOKEN_DELETE  interior position i is removed iff rank_i < c, with key_i = fmix32(seed + i * 0x9E3779B1) (csrc/common.h, mod 2^32) and
 *                    rank_i = the number of interior j with key_j < key_i (the keys of a row are pairwise distinct); n -= c
 *   SR_TOKEN_MASK    the same selection; the selected tokens become mask_id
 *   SR_TOKEN_CUTOFF  the c positions from start = 1 + fmix32(seed) % (ni - c + 1) on are removed; n -= c
 *   SR_TOKEN_SWAP    for k = 0 .. c - 1 in order: a = 1 + fmix32(seed + 2k * 0x9E3779B1) % ni, b = 1 + fmix32(seed + (2k + 1) * 0x9E3779B1) % ni,
 *                    t[a] <-> t[b]; nothing when ni < 2
 * Then ids[b, t] = t[t] for t < m = min(n, L), pad_id for m <= t < L, key_len[b] = m; columns L .. ld_ids are not written.  A src_row outside
 * [0, n_rows) gives an all-pad row of length 0.  Nothing past a stored row is read.  One workgroup per row, no atomics: equal inputs give
 * equal bits.  SR_EINVAL: a null pointer, n_rows <= 0, B outside 1 .. 65535, Lsrc outside 1 .. 4096, L <= 0, ld_ids < L, store not 16-byte
 * aligned, ids not 8-byte aligned, a negative pad_id or mask_id. */
enum { SR_TOKEN_COPY = 0, SR_TOKEN_DELETE = 1, SR_TOKEN_MASK = 2, SR_TOKEN_CUTOFF = 3, SR_TOKEN_SWAP = 4 };
enum { SR_TOKEN_STRONG_MAX_LSRC = 4096 };
int srhip_token_strong(const int* store, const long long* row_off, const int* row_len, int n_rows, const long long* src_row,
                       const long long* slot0, const long long* slot1, int B, int Lsrc, int L, int pad_id, int mask_id, long long* ids,
                       int ld_ids, int* key_len, void* stream);

/* ---- the views of one step joined into one token batch (nets/bert.py TokenBatch.cat with unequal padded lengths, ``token_len_bucket``),
 * one launch.  tests/_token_cat_cases.py restates it (token_cat_ref).
 *   src      HOST array of n_src (1 .. 4) sources, copied into the kernel's arguments: ids int64 [S, L] contiguous (8-byte aligned),
 *            key_len int32 [S], seq_len int32 [S] or NULL, all on the device
 *   ids      int64 [sum S, L_out] contiguous, L_out >= every source's L;  key_len, seq_len int32 [sum S]
 * Output row b is row r of source j (sources in order, their rows in order): ids[b, t] = src[j].ids[r, t] for t < L_j, pad_id for
 * L_j <= t < L_out; key_len[b] = src[j].key_len[r]; seq_len[b] = src[j].seq_len[r] when the source has one, else L_j.  16-byte loads and
 * stores where the source row and the output row are both 16-byte aligned, 8-byte ones otherwise; the pair that holds a row's end is peeled:
 * nothing past a source row is read, nothing past an output row written.  One workgroup per output row, no LDS, no atomics, no
 * synchronisation, no allocation: it can be captured in a graph.  SR_EINVAL: a null pointer (seq_len of a source excepted), n_src outside
 * 1 .. 4, an S or L <= 0, an L above L_out, sum S > 65535, ids (source or output) not 8-byte aligned, a negative pad_id. */
enum { SR_TOKEN_CAT_MAX_SRC = 4 };
typedef struct {
  const long long* ids;
  const int* key_len;
  const int* seq_len;
  int S, L;
} srhip_token_src;
int srhip_token_cat(const srhip_token_src* src, int n_src, int pad_id, long long* ids, int L_out, int* key_len, int* seq_len, void* stream);

/* ---- WideResNet building blocks (classic_cv backbone, semilearn/nets/wrn/wrn.py; BASELINE.json configs[0], parity configuration) ----
 * Feature maps are NHWC = row-major [rows = B*H*W, C].  conv = im2col (bf16) + srhip_gemm_nt; dW = srhip_gemm_tn_grouped_f32(dY, col);
 * dX = srhip_gemm_nt(dY, W^T) + col2im.
 *   nchw_to_nhwc_bf16 : the input batch [B,C,H,W] fp32 -> bf16 [B,H,W,C]
 *   im2col            : col[(b,yo,xo)][(i*k + j)*C + c] = act[b][yo*s+i-p][xo*s+j-p][c]  (k in {1,3}, p = k/2, zero fill, Kpad % 32 == 0;
 *                       column order == Conv2d weight.flatten(1), wrn.py:33-43)
 *   col2im            : the adjoint gather: dact (= | +=) sum of the dcol entries that read each input pixel
 *   conv_weight_prep  : W fp32 [Cout, C, k, k] -> bf16 [Cout, Kpad] in col's tap-major K order and its transpose bf16 [Kpad, Cout];
 *   add_unpad         : the inverse for the gradient: dW[Cout, C, k, k] += dWpad[Cout, Kpad]
 *   bn_fwd            : nn.BatchNorm2d + LeakyReLU(slope) (wrn.py:32-38, :104-105).  training != 0: statistics of THIS batch (saved in
 *                       save_mean / save_invstd), running_mean / running_var moved with ``momentum`` (unbiased variance) unless
 *                       update_running == 0 (Bn_Controller.freeze_bn, core/utils/misc.py:105-129); training == 0: running statistics.
 *                       Outputs: act_bf16 and/or act_f32 (either may be NULL).  256 % C == 0.  ws: srhip_bn_ws_doubles() doubles of scratch the
 *                       caller ZEROES ONCE (every launch leaves its accumulator copies and arrival counter at zero: no memset per call).
 *   bn_bwd            : dx = resid (or 0) + BN'(LeakyReLU'(dact)); dgamma += , dbeta += .
 *   avgpool_fwd/bwd   : F.adaptive_avg_pool2d(.,1) (wrn.py:121);  fc_fwd/bwd: the classifier Linear (wrn.py:106, :126)
 *   sgd_flat          : torch.optim.SGD(momentum, nesterov=True) on a flat block (core/utils/build.py:193-224, optim 'SGD'); chunk table =
 *                       {int64 end, float weight_decay, float pad} per parameter; optional EMA shadow; first_step: buf = d. */
int srhip_nchw_to_nhwc_bf16(const float* img, void* out, int B, int C, int H, int W, void* stream);
int srhip_im2col(const void* act, void* col, int B, int H, int W, int C, int ksize, int stride, int Kpad, void* stream);
/* im2col_bn : col = im2col(bf16(f(x))) from the fp32 tensor in front of the BatchNorm, f = LeakyReLU(BatchNorm(x; mean, invstd)) (mode 0) or
 * identity (mode 2) -- the filter-gradient operand of the backward without a materialised activation.  C % 8 == 0, C <= 256. */
int srhip_im2col_bn(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta, float slope, int mode,
                    void* col, int B, int H, int W, int C, int ksize, int stride, int Kpad, void* stream);
int srhip_col2im(const float* dcol, float* dact, int B, int H, int W, int C, int ksize, int stride, int Kpad, int accumulate, void* stream);
int srhip_conv_weight_prep(const float* Wf, void* Wb, void* WbT, int Cout, int C, int ksize, int Kpad, void* stream);
int srhip_add_unpad(const float* src, float* dst, int Cout, int C, int ksize, int Kpad, void* stream);
/* conv_weight_prep / add_unpad for every convolution of a network in ONE launch each: entry p covers [start_p, start_{p+1}) of a flat index
 * space of `total` elements (prep: Cout * Kpad per entry, a = W fp32, b = Wb, c = WbT; unpad: Cout * C * kk per entry, a = dWpad, b = dW). */
typedef struct srhip_conv_desc {
  const void* a; void* b; void* c;
  int Cout, C, kk, Kpad;
  long long start;
} srhip_conv_desc;                       /* 48 bytes */
int srhip_conv_weight_prep_grouped(const srhip_conv_desc* desc_dev, int n, long long total, void* stream);
int srhip_add_unpad_grouped(const srhip_conv_desc* desc_dev, int n, long long total, void* stream);
/* conv_weight_flip_grouped : the filters of the INPUT-gradient convolutions (stride-1 3x3 layers): dX = srhip_wrn_conv_bn(dY, raw mode, W') with
 * W' bf16 [Cin, Kpad], W'[ci][(8 - t) * Cout + co] = W[co][ci][t] -- the adjoint as one more implicit-GEMM launch instead of GEMM + col2im.
 * Entry: a = W fp32 [Cout, C, 3, 3], b = W', kk = 9, Kpad = round32(9 * Cout); Cin * Kpad elements per entry. */
int srhip_conv_weight_flip_grouped(const srhip_conv_desc* desc_dev, int n, long long total, void* stream);
long long srhip_bn_ws_doubles(void);
/* The same BasicBlock as ONE launch per convolution (csrc/wrn_conv.hip; wrn.py:41-60):
 *   wrn_conv_bn : y fp32 [B*Ho*Wo, Cout] = conv_{k,stride,pad k/2}( f(xin) ) (+ resid), xin fp32 NHWC [B,H,W,Cin] read in place (implicit GEMM);
 *                 f by in_mode: 0 = LeakyReLU(BatchNorm(x; in_mean, in_isd = invstd)), 1 = the same from running statistics (in_isd = running
 *                 VAR, in_eps), 2 = identity (the raw-x path of wrn.py:50), 3 = LeakyReLU(BatchNorm(x)) with the batch statistics folded
 *                 from in_acc (the accumulator the launch that produced xin filled).  pub_mean != NULL (with in_acc, any mode): workgroup
 *                 (0,0) publishes mean / invstd of that BatchNorm (the backward reads them) and moves its running statistics when
 *                 update_running (momentum; unbiased variance).  Wb = conv_weight_prep's bf16 [Cout, Kpad].  acc_out != NULL: per-channel
 *                 sum / sum of squares of y are ADDED into it (srhip_bn_acc_doubles(Cout) doubles, zeroed by the caller before the forward)
 *                 for the BatchNorm that reads y next.  stat_ranks: ranks whose sums in_acc holds (1, or the world size under SyncBatchNorm).
 *                 Cin a power of two in [8,128]; Cout in {16, 32, 64} or a multiple of 64.
 *   bn_stats    : the statistics of a tensor no wrn_conv_bn produced: mean / invstd / running update of x fp32 [rows, C] (ws as for bn_fwd).
 *   bn_act      : act bf16 [rows, C] = f(x) by modes 0-2 -- the backward's im2col operand, recomputed instead of stored. */
int srhip_wrn_conv_supported(int Cin, int Cout, int ksize);
/* Diagnostic (no reference counterpart): the kernel template the last srhip_wrn_conv_bn[_passes] call of this process launched -- 100 + 10 NT + PG
 * for wrn_conv_tile_kernel<NT, PG> (input block in LDS), 10 NT + KS for wrn_conv_kernel<NT, KS>; 0 before the first call.  bench.py names the
 * kernel of the WideResNet leg's roofline object with it. */
int srhip_wrn_conv_last_plan(void);
/* The host decisions of srhip_wrn_conv_bn[_passes] for a shape, without a launch (the launcher takes its decisions from the same function):
 * *kernel in the code of srhip_wrn_conv_last_plan, *grid_x = gridDim.x (gridDim.y = Cout / (16 NT), gridDim.z = passes), *rounds = the direct
 * kernel's grid-stride loop count (1 for the tile kernel).  Kpad is taken as K = Cin k k rounded up to 32.  Any out pointer may be NULL.
 * SR_EINVAL where the launcher refuses the shape. */
int srhip_wrn_conv_plan(int B, int H, int W, int Cin, int Cout, int ksize, int stride, int passes, int* kernel, int* grid_x, int* rounds);
long long srhip_bn_acc_doubles(int C);
int srhip_wrn_conv_bn(const float* xin, int in_mode, const float* in_mean, const float* in_isd, const double* in_acc, const float* in_gamma,
                      const float* in_beta, float in_eps, float slope, float* pub_mean, float* pub_invstd, float* running_mean,
                      float* running_var, float momentum, int update_running, const void* Wb, const float* resid, float* y, int B, int H,
                      int W, int Cin, int Cout, int ksize, int stride, int Kpad, double* acc_out, int stat_ranks, void* stream);
/* The same launch for `passes` independent forwards of B images each (pass-major tensors: xin [passes, B, H, W, Cin], y / resid [passes,
 * B*Ho*Wo, Cout], in_acc / acc_out [passes, srhip_bn_acc_doubles(C)], pub_mean / pub_invstd [passes, Cin]): every pass is its own BatchNorm
 * statistics group, exactly as separate model() calls are -- the K + 1 forwards of x_ulb_w per step of SRPseudoLabel.data_generator under
 * Bn_Controller.freeze_bn (semilearn/algorithms/srpseudolabel/srpseudolabel.py:59-90) share one launch per convolution instead of K + 1.
 * in_mode 2 or 3 only (handed-in statistics would be one group's); update_running moves the running statistics from pass 0 only. */
int srhip_wrn_conv_bn_passes(const float* xin, int in_mode, const float* in_mean, const float* in_isd, const double* in_acc, const float* in_gamma,
                             const float* in_beta, float in_eps, float slope, float* pub_mean, float* pub_invstd, float* running_mean,
                             float* running_var, float momentum, int update_running, const void* Wb, const float* resid, float* y, int B, int H,
                             int W, int Cin, int Cout, int ksize, int stride, int Kpad, double* acc_out, int stat_ranks, int passes, void* stream);
/* "All groups" running statistics for a shared-launch forward: with update_running = 0 in srhip_wrn_conv_bn_passes / srhip_wrn_head_passes,
 * ONE launch after the forward moves the running statistics of every BatchNorm of the table once per statistics group, in group order --
 * running = (1 - momentum) * running + momentum * stat_g for g = 0 .. groups - 1, in fp32, stat_g = mean / unbiased variance from group g's
 * fp64 sums (under SyncBatchNorm the exchanged sums; rows = this rank's rows * ranks).  This is what `groups` model() calls in training mode
 * without Bn_Controller do (semilearn/algorithms/srfixmatch/fixmatch.py:62-146 forwards the concatenated batch K + 1 times per step).  Entry:
 * acc = the accumulators [groups, srhip_bn_acc_doubles(C)] the forward filled (complete once its last launch is enqueued), C <= 256.  One
 * workgroup per entry, one thread per channel carries the chain (no atomics, no reduction across threads); a step is the expression of the
 * publishing launch, so groups = 1 gives the bits of update_running = 1 there. */
typedef struct srhip_bn_chain_desc {
  const double* acc; float* running_mean; float* running_var;
  int C, rows;
} srhip_bn_chain_desc;                   /* 32 bytes */
int srhip_bn_running_chain(const srhip_bn_chain_desc* desc_dev, int n, int groups, float momentum, void* stream);
/* wrn_head : the network's tail (wrn.py:119-126) in one launch: feat [B, C] = mean over the HW2 pixels of LeakyReLU(BatchNorm(x)), logits [B, K] =
 * feat Wc^T + bc; in_mode 0 / 1 / 3 and the publishing arguments as for wrn_conv_bn (workgroup 0 publishes).  C <= 256. */
int srhip_wrn_head(const float* x, int in_mode, const float* in_mean, const float* in_isd, const double* in_acc, const float* gamma,
                   const float* beta, float eps, float slope, float* pub_mean, float* pub_invstd, float* running_mean, float* running_var,
                   float momentum, int update_running, const float* Wc, const float* bc, float* feat, float* logits, int B, int HW2, int C,
                   int K, int stat_ranks, void* stream);
/* ... and for `passes` forwards of B images (x [passes * B, HW2, C]; in_acc / published statistics per pass; in_mode 3). */
int srhip_wrn_head_passes(const float* x, int in_mode, const float* in_mean, const float* in_isd, const double* in_acc, const float* gamma,
                   const float* beta, float eps, float slope, float* pub_mean, float* pub_invstd, float* running_mean, float* running_var,
                   float momentum, int update_running, const float* Wc, const float* bc, float* feat, float* logits, int B, int HW2, int C,
                   int K, int stat_ranks, int passes, void* stream);
int srhip_bn_stats(const float* x, float eps, float momentum, int update_running, float* running_mean, float* running_var, float* out_mean,
                   float* out_invstd, double* ws, int rows, int C, void* stream);
int srhip_bn_act(const float* x, const float* mean, const float* invstd_or_var, const float* gamma, const float* beta, float eps, float slope,
                 int mode, void* act_bf16, float* act_f32, int rows, int C, void* stream);
/* SyncBatchNorm (the reference converts the WideResNet's BatchNorms under DDP: core/utils/misc.py:55): the statistics are sums, so the ranks
 * exchange the ACCUMULATOR between the launch that fills it and the launch that folds it (wrn_conv_bn: stat_ranks = world size scales the row
 * count; the caller all-reduces acc in between), and the backward's two column sums between its reduce and apply halves:
 *   bn_accumulate : sums of x fp32 [rows, C] ADDED into acc (srhip_bn_acc_doubles(C) doubles) -- the statistics of a tensor no wrn_conv_bn produced
 *   bn_fold       : acc -> mean / invstd (+ running update with momentum, unbiased variance) and / or the 2C totals; rows_total = rows of all ranks
 *   bn_bwd_reduce : the backward's sums (dy', dy' * xhat) of this rank into ws[0..2C) (ws as for bn_fwd)
 *   bn_bwd_apply  : dx from `totals` over rows_total rows; d(gamma) / d(beta) += local_totals (NULL: totals) -- per-rank, as torch's
 *                   batch_norm_backward_reduce / _elemt split; dx_bf16 (may be NULL): a bf16 copy of dx, the operand of the convolution
 *                   backward that reads it next.  srhip_bn_bwd = reduce + apply on one rank. */
int srhip_bn_accumulate(const float* x, double* acc, int rows, int C, void* stream);
int srhip_bn_fold(const double* acc, double rows_total, float eps, float momentum, int update_running, float* running_mean, float* running_var,
                  float* out_mean, float* out_invstd, double* totals, int C, void* stream);
int srhip_bn_bwd_reduce(const float* dact, const float* x, const float* save_mean, const float* save_invstd, const float* gamma, const float* beta,
                        float slope, double* ws, int rows, int C, void* stream);
int srhip_bn_bwd_apply(const float* dact, const float* x, const float* save_mean, const float* save_invstd, const float* gamma, const float* beta,
                       float slope, const float* resid, float* dx, float* dgamma, float* dbeta, const double* totals, const double* local_totals,
                       double rows_total, void* dx_bf16, int rows, int C, void* stream);
int srhip_bn_fwd(const float* x, const float* gamma, const float* beta, float eps, float slope, float momentum, int training,
                 int update_running, float* running_mean, float* running_var, float* save_mean, float* save_invstd, void* act_bf16,
                 float* act_f32, double* ws, int rows, int C, void* stream);
int srhip_bn_bwd(const float* dact, const float* x, const float* save_mean, const float* save_invstd, const float* gamma, const float* beta,
                 float slope, const float* resid, float* dx, float* dgamma, float* dbeta, double* ws, int rows, int C, void* stream);
int srhip_avgpool_fwd(const float* act, float* feat, int B, int HW2, int C, void* stream);
int srhip_avgpool_bwd(const float* dfeat, float* dact, int B, int HW2, int C, void* stream);
int srhip_fc_fwd(const float* feat, const float* Wc, const float* bc, float* logits, int B, int F, int K, void* stream);
int srhip_fc_bwd(const float* dlogits, const float* feat, const float* Wc, float* dfeat, float* dWc, float* dbc, int B, int F, int K,
                 void* stream);
int srhip_sgd_flat(float* p, float* g, float* buf, float* ema, const void* chunk_table, int nchunks, long long n, float lr, float momentum,
                   float grad_scale, const float* clip_coef, double ema_m, int first_step, int zero_grad, void* stream);

/* Kernel-execution timing for the benchmark's roofline object (no counterpart in the reference, which times whole iterations:
 * semilearn/core/hooks/timer.py).  While enabled, every launch of this library is issued with a (start, stop) event pair bound to the
 * dispatch itself, so srhip_prof_elapsed_ms returns what `rocprofv3 --kernel-trace` reports for the same launches: execution time
 * without dispatch latency or event packets.  Entry points are numbered in launch order since the last srhip_prof_enable(1).
 * These three calls are host-side only (no stream argument); srhip_prof_elapsed_ms needs a synchronised device. */
int srhip_prof_enable(int on);                                   /* returns the number of launches recorded so far */
int srhip_prof_count(void);
int srhip_prof_elapsed_ms(int first, int last, float* ms_sum);   /* HOST pointer: sum over the launches [first, last) */

#ifdef __cplusplus
}
#endif
#endif
