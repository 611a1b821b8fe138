/* iadr1_hip.h -- C ABI of libiadr1_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the IAD-R1
 * post-training hot path (PA-SFT / SC-GRPO on Qwen2.5-VL).
 *
 * The reference (Yanhui-Lee/IAD-R1) is pure Python and has no FFI of its own;
 * each entry point below replaces the third-party kernel the reference reaches at the cited call site
 * (TF: = transformers/models/qwen2_5_vl/modeling_qwen2_5_vl.py as installed, 5.15.0 line numbers;
 * REF: = /root/reference).  INTEGRATION.md shows the ctypes / AttentionInterface stubs a maintainer
 * of the reference would add to bind them.
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch types.  All pointers are DEVICE pointers unless noted.
 *   - the caller owns every buffer; nothing here allocates, frees or synchronises.
 *   - asynchronous and stream-ordered on `stream` (a hipStream_t, passed as void*); legal inside
 *     hipGraph capture; re-entrant: no mutable global state (the IADR1_* A/B switches
 *     of the launchers are read once, at first use, into constants).
 *   - bf16 tensors are raw uint16 bit patterns; arithmetic is fp32; row strides (`ld*`) are in elements.
 *   - return 0 on success, negative on error; iadr1_last_error() returns the thread-local message.
 */
#ifndef IADR1_HIP_H
#define IADR1_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

typedef void* iadr1_stream_t; /* hipStream_t */

int iadr1_version(void);
const char* iadr1_last_error(void);
/* Co-scheduling of the rollout and the teacher-forced training forward (round 5).  The reference runs its rollout engine and its training ranks on
 * DIFFERENT GPUs at the same time (REF:scripts/train/SC_GRPO/SC_GRPO_Qwen_Instruct_2_5_VL_3B.sh:40-42: 3 training ranks + one vLLM GPU,
 * REF:train/stage_rl/trainer/sc_grpo_trainer.py:637-683 || :737-743); here one MI355X is split by CU masks instead: the latency-bound decode
 * replay keeps most CUs, the MFMA-bound forward over the tokens already sampled runs on the rest, each on its own HIP stream.
 *   iadr1_stream_create_cu_mask: hipExtStreamCreateWithCUMask.  `cu_mask` is a HOST array of `n_words` 32-bit words; bit i enables CU i in the
 *     driver's numbering (round-robin over the 8 XCDs: bits [8k, 8k+8) are one CU of every XCD).  `stream_out` (HOST) receives the hipStream_t.
 *   iadr1_stream_destroy: hipStreamDestroy of such a stream.
 *   iadr1_set_decode_cus: the number of CUs the decode-step launchers (iadr1_gemm_skinny_bf16, iadr1_gemm_qkv_rope_kv_bf16, iadr1_gemm_skinny_fp8w)
 *     size their persistent one-block-per-CU grids for; 0 = the device's CU count.  THREAD-LOCAL launcher configuration (like iadr1_last_error): the thread
 *     that captures or launches a decode step sets it right before and resets it to 0 right after; other threads and other engines never see it. */
int iadr1_stream_create_cu_mask(const unsigned* cu_mask, int n_words, void** stream_out);
int iadr1_stream_destroy(void* stream);
int iadr1_set_decode_cus(int n_cus);
/* Rollout -> training hand-over.  The four decode-step entry points that take a trailing `side` argument can ALSO write what they compute into
 * row-major training buffers, at row  base + s * seq_stride + *step  for sequence s (`step`: device-resident decode step counter).  `side` is a
 * HOST pointer to this struct, read during the call (NULL: no side outputs); the struct holds DEVICE pointers:
 *   iadr1_rmsnorm_fwd (T <= 256)        p0 = residual stream rows [.., ld0] (bf16), p1 = normalised rows [.., ld1], p2 = rstd (fp32, one per row)
 *   iadr1_gemm_qkv_rope_kv_bf16         p0 = roped q|k|v rows [.., ld0]
 *   iadr1_attn_decode                   p0 = attention output rows [.., ld0], p1 = log-sum-exp fp32 [Hq][ld1]
 *   iadr1_gemm_skinny_bf16 out_mode 3   p0 = gate|up rows [.., ld0], p1 = SwiGLU rows [.., ld1]   (persistent kernel shapes only)
 * Decode step t processes completion token t of every sequence = row (s, t) of the completion block of the shared-prefix training batch, so the
 * policy's teacher-forced forward over the completions (REF:505-513 on the policy model) need not be run again before backward.  Unused p*: NULL. */
typedef struct iadr1_side_out {
    void* p0; long long ld0;
    void* p1; long long ld1;
    void* p2; long long ld2;
    const unsigned* step;
    long long base, seq_stride;
} iadr1_side_out_t;

/* ---- dense contractions ----------------------------------------------------------------------------
 * C[M,N] (+)= act(A[M,K] . B[N,K]^T + bias[N]).  out_mode: 0 = bf16 store, 1 = fp32 store, 2 = fp32
 * accumulate (C += ...).  act: 0 none, 1 exact GELU.  K, lda, ldb multiples of 8; A/B 16-byte aligned.
 * Replaces every nn.Linear / the stride==kernel Conv3d of the path: TF:85-96 (ViT MLP), :116-122 (patch
 * embed), :148-150 (merger), :218-219 (ViT qkv/proj), :552-554 (decoder MLP), :634-637 (q/k/v/o),
 * :1386-1387 (lm_head), and their autograd backward (dgrad / wgrad run on transposed operands). */
int iadr1_gemm_nt_bf16(const void* A, const void* B, void* C, const void* bias, int M, int N, int K, long long lda,
                       long long ldb, long long ldc, int out_mode, int act, iadr1_stream_t stream);
/* C[M,N] (fp32) += A[M,K] . B[N,K]^T for contractions with few output tiles and a long K (the weight gradients dW = dY^T . X of the narrow projections: 64-80 tiles
 * of 256 x 256 on 256 CUs): `ksplit` K slices per tile, fp32 partial tiles in `workspace` (iadr1_gemm_nt_splitk_workspace_bytes, 16-byte aligned), summed into C
 * in slice order by a second launch -- bit-reproducible, no atomics.  Same operand rules as iadr1_gemm_nt_bf16; N, ldc multiples of 4.  Replaces the autograd
 * weight-gradient GEMMs of TF:634-637 (q/k/v/o), :552-554 (MLP), :85-96,218-219 (ViT). */
long long iadr1_gemm_nt_splitk_workspace_bytes(int M, int N, int ksplit);
int iadr1_gemm_nt_splitk_acc_bf16(const void* A, const void* B, float* C, void* workspace, int M, int N, int K, long long lda, long long ldb,
                                  long long ldc, int ksplit, iadr1_stream_t stream);
/* Weight gradients WITHOUT transposed copies:  C[M,N] (fp32) += A[K,M]^T . B[K,N]  with A (= dY) and B (= X) row-major as the backward holds them, the contraction over
 * their K rows (the 256 x 256 kernel with hardware transpose reads out of LDS, ds_read_b64_tr_b16).  ksplit >= 2: K slices of whole 64-row tiles, fp32 partial tiles in
 * `workspace` (iadr1_gemm_nt_splitk_workspace_bytes(M, N, ksplit)), added to C in slice order; ksplit <= 1: one accumulating launch (workspace unused).  M, N >= 256 and
 * multiples of 8.  Bit-equal to iadr1_gemm_nt_bf16 (out_mode 2) / iadr1_gemm_nt_splitk_acc_bf16 on transposed copies.  Replaces autograd's weight-gradient matmuls of every
 * Linear on the path (TF:552-554, 660-700 backward; REF:train/stage_rl/trainer/sc_grpo_trainer.py:794 `loss.backward()` via accelerate). */
int iadr1_gemm_tn_acc_bf16(const void* A, const void* B, float* C, void* workspace, int M, int N, int K, long long lda, long long ldb, long long ldc,
                           int ksplit, iadr1_stream_t stream);
/* gate|up projection + SwiGLU in one launch (training / prefill shapes): GU[M, 2I] = A[M,K] . W[2I,K]^T is stored when GU != NULL (the backward
 * pass reads it), Aout[M, I] = bf16(silu(gate)) * up with gate = GU[:, :I], up = GU[:, I:], computed in the GEMM epilogue from the rounded gate|up
 * values: bit-identical to iadr1_gemm_nt_bf16 followed by iadr1_swiglu_fwd.  M %% 256 == 0, I %% 128 == 0.  Replaces TF:552-554
 * (down_proj(act_fn(gate_proj(x)) * up_proj(x))) up to the down projection. */
int iadr1_gemm_swiglu_bf16(const void* A, const void* W, void* GU, void* Aout, int M, int I, int K, long long lda, long long ldw,
                           long long ldgu, long long ldaout, iadr1_stream_t stream);
/* The same contraction over ROW BLOCKS of larger matrices: GEMM row r (0 <= r < M) is row (r / block) * block_stride + r % block of A, GU and Aout, counted from
 * the given base pointers (block: a power of two >= 16 dividing M; M %% 256 == 0).  Per row the arithmetic is iadr1_gemm_swiglu_bf16's, bit for bit.  Used by the
 * co-scheduled pass (iad-r1_amd/overlap.py) to rebuild the POLICY's gate|up and SwiGLU rows of a chunk of decode steps -- `block` steps of every sequence,
 * sequences `block_stride` rows apart in the sequence-major training arena -- on the side stream, so that the decode step's gate|up kernel need not store them
 * (the same mlp rows of REF:train/stage_rl/trainer/sc_grpo_trainer.py:722-735's policy forward, TF:552-554). */
int iadr1_gemm_swiglu_rows_bf16(const void* A, const void* W, void* GU, void* Aout, int M, int I, int K, long long lda, long long ldw,
                                long long ldgu, long long ldaout, int block, long long block_stride, iadr1_stream_t stream);
/* Decode-time skinny GEMM: Y[M,N] = X[M,K] . W[N,K]^T (M small, 64 rows per pass); HBM-bound weight stream,
 * K spread over 8-16 waves per block (+ optional grid split `ksplit`), no atomics.  out_mode 0: bf16 + bias;
 * 1: fp32 (logits); 2: fp32 partial slabs Y[ksplit][M][ldy] summed by iadr1_rmsnorm_fwd (x32 path); 3: fused
 * SwiGLU over a gate|up matrix packed with iadr1_pack_gateup_bf16 (N = 2*I rows in, Y is [M, I]).
 * ldx == 0: X is DECODE-PACKED (MFMA B-fragment order, rows padded to 64: Xp[m/64][k/32][(m%64)/16][m%16 + 16*((k%32)/8)][k%8],
 * see iadr1_pack_act_bf16) -- every X fragment load is then 1 KiB contiguous like the weights; iadr1_rmsnorm_fwd (ldy == 0),
 * iadr1_attn_decode (ldo == 0) and out_mode 3 here (ldy == 0) emit that layout directly, so the decode step never repacks.
 * Replaces the same Linears inside vLLM's decode step (REF:train/stage_rl/trainer/sc_grpo_trainer.py:667). */
int iadr1_gemm_skinny_bf16(const void* X, const void* W, void* Y, const void* bias, int M, int N, int K, long long ldx,
                           long long ldw, long long ldy, int out_mode, int ksplit, const iadr1_side_out_t* side, iadr1_stream_t stream);
/* W[N,K] row-major -> decode-packed MFMA-fragment order Wp[N/16][K/32][64 lanes][8] (what iadr1_gemm_skinny_bf16 reads:
 * every wave-level load of the weight stream is then 1 KiB contiguous).  N % 16 == 0, K % 32 == 0. */
int iadr1_pack_weight_bf16(const void* W, long long ldw, void* Wp, int N, int K, iadr1_stream_t stream);
/* gate|up matrix W[2I,K] -> decode-packed with gate/up 16-row tiles interleaved, for out_mode 3 (fused SwiGLU) of
 * iadr1_gemm_skinny_bf16: Y[M, I] = silu(X.Wgate^T) * (X.Wup^T).  I % 64 == 0. */
int iadr1_pack_gateup_bf16(const void* W, long long ldw, void* Wp, int I, int K, iadr1_stream_t stream);
/* Decode-step fusion of the q|k|v projection with iadr1_rope_kv_store: Y = X.Wqkv^T + b, rotary on the q and k heads (fp32 on the
 * bf16-rounded projections, TF:153-171), q heads -> q_out[M, >= Hq*D] (row stride ldq), new K / V rows -> the paged cache at slot[m]
 * (< 0: skipped).  Wp / bias_p come from iadr1_pack_qkv_rope_bf16: decode-packed with the rotary partners (d, d+64) of every q / k
 * head dealt into the same 16-column tile.  ldx == 0: X decode-packed.  One launch instead of two per layer of the rollout. */
int iadr1_gemm_qkv_rope_kv_bf16(const void* X, const void* Wp, const void* bias_p, void* q_out, const float* rope_cos,
                                const float* rope_sin, const long long* slot, void* kcache, void* vcache, int M, int Hq, int Hkv,
                                int D, int K, long long ldx, long long ldq, const iadr1_side_out_t* side, iadr1_stream_t stream);
int iadr1_pack_qkv_rope_bf16(const void* W, long long ldw, const void* bias, void* Wp, void* bias_p, int Hq, int Hkv, int D, int K,
                             iadr1_stream_t stream);
/* FP8 weights for the decode stream (BASELINE config 5: "fp8 weights"; opt-in, the rollout only -- the training passes and the log-probs of the loss stay
 * bf16).  iadr1_pack_weight_fp8: W[N,K] bf16 -> OCP e4m3 with ONE fp32 scale per output row (scale[n] = max_k |w[n][k]| / 448, round to nearest even),
 * decode-packed so that a lane's 16-byte load holds its 8 weights of TWO consecutive 32-deep k-steps: Wp8[N/16][K/64][64 lanes][16 B].  gateup_I > 0:
 * W is a gate|up matrix [2I, K], tiles interleaved as by iadr1_pack_gateup_bf16.  K % 64 == 0.
 * iadr1_gemm_skinny_fp8w: Y = (X . dequant(Wp8)^T) with the out_modes 0-3 of iadr1_gemm_skinny_bf16 (the fragments are widened to bf16 in registers --
 * exact, every e4m3 value is a bf16 value -- and fed to the bf16 MFMA; columns are multiplied by wscale in the epilogue).  N % 64 == 0.
 * Stated tolerance of the format: |w - dequant(quant(w))| <= 2^-4 |w| + scale * 2^-10 per weight (3 mantissa bits); the kernel adds nothing to it
 * (tests/test_hip_kernels.py::test_fp8_weight_gemm compares against the dequantised weights at the bf16 GEMM's own tolerance). */
int iadr1_pack_weight_fp8(const void* W, long long ldw, void* Wp8, float* scale, int N, int K, int gateup_I, iadr1_stream_t stream);
int iadr1_gemm_skinny_fp8w(const void* X, const void* Wp8, const float* wscale, void* Y, const void* bias, int M, int N, int K, long long ldx,
                           long long ldy, int out_mode, int ksplit, iadr1_stream_t stream);
/* X[M,K] row-major -> decode-packed activations Xp (buffer of roundup(M,64)*K elements; pad rows zeroed).  K % 32 == 0. */
int iadr1_pack_act_bf16(const void* X, long long ldx, void* Xp, int M, int K, iadr1_stream_t stream);
int iadr1_transpose_bf16(const void* in, long long ldi, void* out, long long ldo, int R, int C, iadr1_stream_t stream);

/* ---- RMSNorm (TF:65-79) --------------------------------------------------------------------------------
 * y = w * bf16((x [+ res]) * rsqrt(mean((x+res)^2) + eps)).  Exactly one of x (bf16) / x32 is given; x32 =
 * `nsplit` fp32 partial slabs [nsplit][T][ldx] from the split-K skinny GEMM (summed here, optional bias xbias).
 * res_out receives x+res (new residual stream), rstd the per-row statistic for the backward.  Any output
 * pointer may be NULL. */
int iadr1_rmsnorm_fwd(const void* x, const float* x32, int nsplit, const void* xbias, const void* res, void* res_out,
                      const void* w, void* y, float* rstd, int T, int H, long long ldx, long long ldr, long long ldy,
                      float eps, const iadr1_side_out_t* side, iadr1_stream_t stream);
/* dx = dres + d rmsnorm / dx ; dw (fp32, may be NULL) += sum_t dy * x * rstd.  The sum over token rows is two-stage and ORDERED (round 5): every block writes its
 * partial gain gradient to `workspace` (iadr1_rmsnorm_bwd_workspace_bytes, fp32, needed when dw != NULL), a second launch adds the partials in block order -- no float
 * atomics anywhere in the backward path, two runs of the same step give the same bits. */
long long iadr1_rmsnorm_bwd_workspace_bytes(int T, int H);
int iadr1_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, void* dx,
                      float* dw, float* workspace, int T, int H, long long ld, iadr1_stream_t stream);

/* ---- LayerNorm with bias (Qwen2-VL vision tower: nn.LayerNorm(eps=1e-6), TF:models/qwen2_vl/modeling_qwen2_vl.py:281,428-429)
 * y = ((x [+ res]) - mean) * rstd * w + b; backward returns dx (+ dres) and accumulates dw, db (fp32). */
int iadr1_layernorm_fwd(const void* x, const void* res, void* res_out, const void* w, const void* b, void* y, float* mean,
                        float* rstd, int T, int H, long long ldx, long long ldr, long long ldy, float eps, iadr1_stream_t stream);
long long iadr1_layernorm_bwd_workspace_bytes(int T, int H);
int iadr1_layernorm_bwd(const void* dy, const void* x, const void* w, const float* mean, const float* rstd, const void* dres,
                        void* dx, float* dw, float* db, float* workspace, int T, int H, long long ld, iadr1_stream_t stream);

/* ---- rotary embeddings: vision 2-D rotary TF:153-171 and decoder M-RoPE TF:557-599 -----------------------
 * In place on `nheads` consecutive heads of width D per token row; cos/sin fp32 [T, D/2] (the M-RoPE
 * t/h/w section select is folded into the table by the host).  backward != 0 applies the transpose. */
int iadr1_rope_inplace(void* x, long long ld, const float* cos_t, const float* sin_t, int T, int nheads, int D,
                       int backward, iadr1_stream_t stream);

/* ---- activations ---------------------------------------------------------------------------------------
 * SwiGLU TF:95-96,552-554 over gu = [gate | up] (width 2*I); exact GELU of the patch merger TF:143. */
int iadr1_swiglu_fwd(const void* gu, long long ldg, void* a, long long lda, int T, int I, iadr1_stream_t stream);
int iadr1_swiglu_bwd(const void* da, long long lda, const void* gu, long long ldg, void* dgu, long long ldd, int T, int I,
                     iadr1_stream_t stream);
int iadr1_gelu_fwd(const void* z, void* a, long long n, iadr1_stream_t stream);
int iadr1_gelu_bwd(const void* da, const void* z, void* dz, long long n, iadr1_stream_t stream);
/* GELU, tanh approximation: SigLIP vision MLP of the LLaVA-OneVision branch (transformers/models/siglip/modeling_siglip.py:310-322) */
int iadr1_gelu_tanh_fwd(const void* z, void* a, long long n, iadr1_stream_t stream);
int iadr1_gelu_tanh_bwd(const void* da, const void* z, void* dz, long long n, iadr1_stream_t stream);
/* QuickGELU x*sigmoid(1.702x): Qwen2-VL vision MLP (TF:models/qwen2_vl/modeling_qwen2_vl.py:293-301) */
int iadr1_quick_gelu_fwd(const void* z, void* a, long long n, iadr1_stream_t stream);
int iadr1_quick_gelu_bwd(const void* da, const void* z, void* dz, long long n, iadr1_stream_t stream);
/* out[n] (fp32) += sum_t dy[t][n]   (bias gradients); partial sums of <= 64 row groups in `workspace` (iadr1_colsum_workspace_bytes), added in group order: no atomics */
long long iadr1_colsum_workspace_bytes(int T, int N);
int iadr1_colsum_acc(const void* dy, long long ld, float* out, float* workspace, int T, int N, iadr1_stream_t stream);

/* ---- embedding lookup + image-feature scatter (TF:1204-1215 masked_scatter) -----------------------------------
 * out[t] = img_index[t] >= 0 ? img[img_index[t]] : E[ids[t]].
 * Backward = iadr1_rows_scatter_acc: dst[rows[u]] (fp32 [., H]) += sum_{k in [ptr[u], ptr[u+1])} src[idx[k]] (src bf16 [T, H]) for the U DISTINCT destination rows `rows`
 * (embedding rows by token id / image-embedding rows), the token rows of each listed by a host-built CSR; one block per destination row adds them in list order:
 * single writer, fixed order, no atomics (round 5: replaces iadr1_embed_bwd's float atomics). */
int iadr1_embed_fwd(const long long* ids, const int* img_index, const void* E, const void* img, void* out, int T, int H,
                    iadr1_stream_t stream);
int iadr1_rows_scatter_acc(const void* src, const long long* rows, const int* ptr, const int* idx, float* dst, int U, int H, iadr1_stream_t stream);

/* out[t] (bf16 [T,H]) = sum_k weights[k] * src[idx[k]], k in [ptr[t], ptr[t+1]) (fp32 sum, one rounding; an empty list gives zeros; weights NULL = 1).
 * Two uses: (1) the gradient of the rows the lm_head consumed (REF:...sc_grpo_trainer.py:505-513 only reads P-1 .. S-2 of each row; PA-SFT the
 * supervised positions) scattered back onto the token rows of the decoder output, several selected rows may share one token row; (2) the
 * LLaVA-OneVision feature packing (transformers/models/llava_onevision/modeling_llava_onevision.py:280-348: crop grid, unpad, bilinear shrink,
 * image_newline per row) and its transpose, as a sparse linear map built on the host.  ptr: [T+1], idx / weights: [ptr[T]], src rows contiguous. */
int iadr1_rows_gather_sum(const void* src, const int* ptr, const int* idx, const float* weights, void* out, int T, int H, iadr1_stream_t stream);

/* ---- casts ---------------------------------------------------------------------------------------------- */
int iadr1_cast_f32_to_bf16(const float* in, long long ldi, void* out, long long ldo, int R, int C, int Cpad,
                           iadr1_stream_t stream);
int iadr1_cast_bf16_to_f32(const void* in, float* out, long long n, iadr1_stream_t stream);
int iadr1_f32_bias_to_bf16(float* in_zeroed_after, const void* bias, void* out, long long R, int C, iadr1_stream_t stream);

/* ---- attention -------------------------------------------------------------------------------------------
 * Flash-style varlen attention over explicit segments [seg_start[i], seg_end[i]) of the flat token axis;
 * D in {128, 80}; GQA via Hq/Hkv.  Replaces flash-attn / eager attention at TF:186-208,225-291 (ViT,
 * non-causal windows) and TF:641-689 (decoder, causal, left padding = segments that start late).
 * lse: [Hq, T] fp32.  Backward also needs a delta scratch [Hq, T] fp32.
 * seg_prefix: NULL, or [nseg][4] int32 {prefix_start, prefix_len, child_first, child_count} for SHARED-PREFIX attention: the
 * keys of segment i are tokens [prefix_start, +prefix_len) (all visible) followed by its own tokens (causal).  Used for
 * the SC-GRPO policy / reference passes: the G completions of a prompt (REF:...sc_grpo_trainer.py:705-746 runs the prompt G
 * times inside [B*G, P+C] rows) attend to ONE copy of the prompt's keys/values -- same math, the prompt tokens go through
 * every layer once per group instead of G times.  Segments [child_first, +child_count) are those whose prefix is segment i
 * (their queries contribute to segment i's dK/dV); segments must be non-empty; max_seqlen covers own lengths only.
 * dkv_ws / head_splits (backward): NULL / 1, or an fp32 scratch of head_splits*T*Hkv*2*D floats: the q heads of each GQA group
 * are then split over head_splits dK/dV blocks (the query loop of a shared prefix block is G+1 segments long) and the partials
 * are summed in a fixed order -- deterministic, no atomics.
 * nseg_head / max_seqlen_tail: 0 / 0, or a hint about the segment lengths: the first nseg_head segments are at most max_seqlen long, the
 * others at most max_seqlen_tail (<= max_seqlen).  The two ranges are then launched with their own grids (no empty blocks for the short
 * segments; with shared prefixes the head split applies to the head range, which must hold every segment that has children). */
int iadr1_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, const int* seg_start,
                   const int* seg_end, const int* seg_prefix, int nseg, int max_seqlen, int nseg_head, int max_seqlen_tail, int T, int Hq, int Hkv, int D, long long ldq,
                   long long ldk, long long ldv, long long ldo, int causal, float scale, iadr1_stream_t stream);
/* Chunked teacher-forced forward (round 5: the frozen reference's pass over the completion tokens runs UNDER the rollout, a few decode steps' worth of rows
 * at a time, REF:train/stage_rl/trainer/sc_grpo_trainer.py:737-743 next to :637-683).  Same kernel and arithmetic as iadr1_attn_fwd (causal), plus per segment
 * seg_view[i] = {q_first, q_count, blk_log2, blk_stride}: only the query rows [q_first, +q_count) of segment i are computed -- against its prefix and ALL its
 * own rows [0, seg_end - seg_start) written so far (causal) -- and logical row j of the segment lives at flat row
 *     seg_start + (j >> blk_log2) * blk_stride + (j & (2^blk_log2 - 1))
 * (time-blocked completion rows: the rows all sequences produce in the same 2^blk_log2 decode steps are contiguous, so every token-wise kernel and GEMM of a
 * chunk runs on one contiguous row range; blk_log2 = 31, blk_stride = 0: a plain contiguous segment).  A query row's result is bit-identical to the one
 * iadr1_attn_fwd computes for it over the whole sequence: same 64-key tiles in the same order.  max_q_count >= every q_count.  Prefix ranges are plain. */
int iadr1_attn_fwd_chunk(const void* q, const void* k, const void* v, void* o, float* lse, const int* seg_start, const int* seg_end,
                         const int* seg_prefix, const int* seg_view, int nseg, int max_q_count, int T, int Hq, int Hkv, int D, long long ldq,
                         long long ldk, long long ldv, long long ldo, float scale, iadr1_stream_t stream);
int iadr1_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                   float* delta, void* dq, void* dk, void* dv, float* dkv_ws, int head_splits, const int* seg_start,
                   const int* seg_end, const int* seg_prefix, int nseg, int max_seqlen, int nseg_head, int max_seqlen_tail, int T, int Hq, int Hkv, int D, long long ldq, long long ldk, long long ldv,
                   long long ldo, long long lddo, long long lddq, long long lddk, long long lddv, int causal,
                   float scale, iadr1_stream_t stream);
/* Paged-KV decode attention + cache writes for the group rollout (vLLM's role at REF:...sc_grpo_trainer.py:
 * 343-358,667).  Pages hold 32 keys: K page [Hkv][32 x D in the MFMA-fragment order
 * attn_decode reads, private to these three entry points], V page [Hkv][D][32].  slot = page*32 + offset. */
int iadr1_attn_decode(const void* q, const void* kcache, const void* vcache, const int* block_table, const int* ctx_len,
                      void* o, int B, int Hq, int Hkv, int D, int max_pages, long long ldq, long long ldo, float scale, int seqs_per_group,
                      const iadr1_side_out_t* side, iadr1_stream_t stream);
/* seqs_per_group > 1 (a hint, results do not depend on it): sequences [g*n, (g+1)*n) share their prompt pages through the block table (group rollout); the blocks of
 * one prompt group are then placed on ONE XCD so that its L2 serves all but the first reader of a shared page. */
/* The same attention for prompt GROUPS with long shared prompts (LLaVA families, MHA decoders): sequences [g*G, (g+1)*G) share their first shared_pages[g] block-table
 * entries (the full prompt pages, as the rollout lays them out); one block per (group, kv head) reads those pages ONCE for all G * Hq/Hkv (<= 64) query rows, then
 * every sequence's private pages, and merges.  Same results as iadr1_attn_decode up to fp32 summation order; G times less K/V traffic for the shared part.
 * chunks > 1 (few groups x kv heads, very long prompts): the shared pages are split over `chunks` blocks in a first launch whose partial states go through
 * `ws` (fp32 [B/G][Hkv][chunks][64 or 32 or 16 rows][D + 2], rows = the tile-rounded G * Hq/Hkv) to a second launch that merges them in chunk order. */
int iadr1_attn_decode_group(const void* q, const void* kcache, const void* vcache, const int* block_table, const int* ctx_len, const int* shared_pages,
                            void* o, int B, int G, int Hq, int Hkv, int D, int max_pages, long long ldq, long long ldo, float scale, int chunks, float* ws,
                            const iadr1_side_out_t* side, iadr1_stream_t stream);
int iadr1_kv_store(const void* k, long long ldk, const void* v, long long ldv, const long long* slot, void* kcache,
                   void* vcache, int T, int Hkv, int D, iadr1_stream_t stream);
/* decode-step fusion of iadr1_rope_inplace (q,k heads) + iadr1_kv_store for one new token per sequence */
int iadr1_rope_kv_store(void* qkv, long long ld, const float* cos_t, const float* sin_t, const long long* slot, void* kcache,
                        void* vcache, int T, int Hq, int Hkv, int D, iadr1_stream_t stream);

/* ---- log-probs / losses -----------------------------------------------------------------------------------
 * logprob_rows: REF:train/stage_rl/trainer/sc_grpo_trainer.py:510-513 (log_softmax + gather, no temperature)
 * and PA-SFT cross entropy TF:loss/loss_utils.py:32-71 (logp = -CE; target < 0 is ignored).
 * dlogits_rows: g[row] * (onehot - softmax) in bf16.   grpo_loss: REF:...sc_grpo_trainer.py:746,796-798,816.
 * -inf logits (masked vocabulary entries) are legal in both: such an id has probability 0 -- it adds nothing to lse, its dlogit is 0, and a target that
 * points at it gets logp = -inf.  A row must hold at least one finite logit; +inf and NaN logits are not supported. */
int iadr1_logprob_rows(const float* logits, long long ld, const long long* targets, float* logp, float* lse, int R, int V,
                       iadr1_stream_t stream);
int iadr1_dlogits_rows(const float* logits, long long ld, const long long* targets, const float* lse, const float* g,
                       void* dl, long long ldd, int R, int V, iadr1_stream_t stream);
/* linear_logprob -- SURVEY section 8(b).5 "fused K15+K16, returns per-token logp and lse" (and linear_ce: logp = -CE, target < 0 ignored):
 *   logp[r] = log_softmax(H[r,:K] . W[V,K]^T)[targets[r]],  lse[r] = logsumexp of that row    (REF:505-513 lm_head + log_softmax + gather; PA-SFT CE TF:loss/loss_utils.py:32-71)
 * without the [M, V] logits reaching HBM: the GEMM's epilogue reduces every 64-column slice to (max, sum exp) and picks the target logit, a second launch
 * merges the slices in a fixed order (deterministic).  `workspace`: iadr1_linear_logprob_workspace_bytes(M, V) bytes, caller-owned, 8-byte aligned.
 * iadr1_linear_logprob_dlogits: the backward's first half -- the logits are recomputed and leave as dl[M, V] = g[r] * (onehot(target) - exp(x - lse[r])) in bf16
 * (the arithmetic of iadr1_dlogits_rows); dH = dl . W and dW += dl^T . H are iadr1_gemm_nt_bf16 calls.  K, ldh, ldw multiples of 8.  ldd: any value >= V; with ldd a
 * multiple of 8 and dl 16-byte aligned the rows leave as 16-byte stores (the hot path), otherwise element by element. */
long long iadr1_linear_logprob_workspace_bytes(int M, int V);
int iadr1_linear_logprob_fwd(const void* H, const void* W, const long long* targets, float* logp, float* lse, void* workspace, int M, int V, int K,
                             long long ldh, long long ldw, iadr1_stream_t stream);
int iadr1_linear_logprob_dlogits(const void* H, const void* W, const long long* targets, const float* lse, const float* g, void* dl, long long ldd,
                                 int M, int V, int K, long long ldh, long long ldw, iadr1_stream_t stream);
/* The same pair at a temperature (REF:trl/trl/trainer/grpo_trainer.py:818-821: trl divides the logits by the sampling temperature before the log-softmax, for the
 * policy, the old policy and the reference model alike).  With inv_t = 1.0f / temperature, formed once on the host in fp32, and y = x * inv_t:
 *   iadr1_linear_logprob_fwd_t:      lse[r] = logsumexp(y[r, :]),  logp[r] = y[r, target] - lse[r]  (ignored targets: 0)
 *   iadr1_linear_logprob_dlogits_t:  dl[r, j] = (g[r] * inv_t) * (onehot(target) - exp(y[r, j] - lse[r])): the extra 1 / T is the chain rule through y; lse is the one
 *                                    the _t forward returned
 * The same two kernels, workspace and launches: both epilogues multiply every accumulator element by inv_t once, one fp32 multiply in registers, before anything else
 * reads it, and the backward takes rg = g[r] * inv_t; everything after that is the plain pair's code on y.  The plain pair passes 1 (a product by 1.0f is exact), so
 * temperature = 1 gives the plain pair's bits.  Refused on the host before any launch (prefix "linear_logprob_fwd_t:" / "linear_logprob_dlogits_t:"): a temperature
 * that is not finite or <= 0, and everything the plain pair refuses. */
int iadr1_linear_logprob_fwd_t(const void* H, const void* W, const long long* targets, float* logp, float* lse, void* workspace, int M, int V, int K,
                               long long ldh, long long ldw, float temperature, iadr1_stream_t stream);
int iadr1_linear_logprob_dlogits_t(const void* H, const void* W, const long long* targets, const float* lse, const float* g, void* dl, long long ldd,
                                   int M, int V, int K, long long ldh, long long ldw, float temperature, iadr1_stream_t stream);
/* The GRPO loss: five entry points, ONE kernel body and ONE host function behind them (csrc/loss.hip).  Over one rank's [N, C] completion block, mask m,
 * cnt = sum_i m_i, kl_i = exp(d) - d - 1 with d = ref_logp_i - logp_i, the per-token term is  w_i * (-(q_i s_i - beta * kl_i))  and its derivative in logp_i is
 * g_i = w_i * (beta * (1 - exp(ref_logp_i - logp_i)) - q_i s'_i);  w_i is a constant under differentiation, kl and row_kl stay unweighted.  Three forms differ in
 * s and w only, and the inputs select the form:
 *   plain (neither old_logp nor rollout_logp; iadr1_grpo_loss):  s_i = A, s'_i = A, w_i = 1   (REF:...sc_grpo_trainer.py:746,796-798,816; exp(p - sg p) = 1 in value)
 *   IS    (rollout_logp; iadr1_grpo_loss_is):    s_i = s'_i = A, w_i the truncated importance weight (cap, level, w_out, row_stats [N, 5])
 *   clip  (old_logp; iadr1_grpo_loss_clip):      s_i = min(r_i A, rc_i A), s'_i = r_i A or 0 where clipped, w_i = w[i] or 1 (eps_low, eps_high, row_stats [N, 4])
 * iadr1_grpo_loss, _is and _clip demand their form; iadr1_grpo_loss_ex and _sel deduce it from old_logp / rollout_logp and add row_scale and (_sel) q_i = sel_i.
 *   s = row_scale > 0 ? row_scale : (cnt > 0 ? 1 / cnt : 0)      (the three older calls: row_scale 0)
 *   row_loss = s * sum_i m_i * term_i,   dlogp_i = m_i * s / n_total_rows * g_i,   row_kl = sum_i m_i kl_i / cnt  whatever row_scale is
 * n_total_rows: number of sequences the batch mean runs over (>= N when the step is micro-batched).  Log-probs at m_i == 0 (rollout_logp, old_logp) may hold
 * anything, NaN included: they are never exponentiated.  One block per row, fixed-order block reductions, no float atomics: run-to-run bit-identical.
 * Bit-equality where a newer call's additions are neutral: _ex with row_scale == 0 is the form's own entry point on every output (reference given or not); _sel with sel
 * NULL is _ex (same kernels and arguments) and with sel all ones equals it; IS with rollout_logp == logp bitwise and clip with old_logp == logp bitwise (w NULL, or w = an IS
 * call's w_out) give the four shared outputs of the plain form (of that IS call).
 * Refused on the host by every entry point, with its own prefix ("grpo_loss_is: ..."): N <= 0, C <= 0, n_total_rows < N; ref_logp NULL with beta != 0 (with beta == 0 it
 * is legal everywhere: no reference log-prob is read, kl_i = 0, kl (if given) and row_kl are written as 0, and on finite inputs dlogp and row_loss equal those of a call
 * with any ref_logp); the input the demanded form reads NULL (rollout_logp for _is, old_logp for _clip); row_stats NULL where the form writes it; cap < 1 or not finite,
 * level not in {0, 1} (IS); eps_low not in [0, 1), eps_high < 0 or not finite (clip); and by _ex / _sel: row_scale negative or not finite, old_logp together with
 * rollout_logp, w without old_logp. */
int iadr1_grpo_loss(const float* logp, const float* ref_logp /* may be NULL */, const float* adv, const int* mask, float beta, int n_total_rows,
                    float* dlogp, float* kl, float* row_loss, float* row_kl, int N, int C, iadr1_stream_t stream);
/* grpo_loss_is: the truncated importance weight per token against the rollout's log-probs (the sampler's and the loss's kernels -- and, with FP8 decode weights,
 * their weights -- differ, so the scored tokens are slightly off-policy).  Over the mask m, with d_i = logp_i - rollout_logp_i:
 *   level 0 (token):    w_i = min(exp(d_i), cap)        level 1 (sequence): w_i = min(exp(sum_i m_i d_i / cnt), cap), one value per row (a mean over cnt whatever row_scale)
 * Both log-probs are temperature-1, unfiltered (iadr1_sample_logp's logp_out against iadr1_logprob_rows): the ratio corrects the engine mismatch, not the sampler's
 * temperature / top-k / top-p filter.
 *   w_out (may be NULL): [N, C], 0 where the mask is 0.
 *   row_stats: [N, 5] per-row partials { sum m w, live tokens whose untruncated ratio exceeded cap, sum m |d|, max m |d|, sum m (exp(d) - d - 1) }. */
int iadr1_grpo_loss_is(const float* logp, const float* ref_logp /* may be NULL */, const float* rollout_logp, const float* adv, const int* mask, float beta, float cap,
                       int level, int n_total_rows, float* dlogp, float* kl, float* row_loss, float* row_kl, float* w_out, float* row_stats, int N, int C,
                       iadr1_stream_t stream);
/* grpo_loss_clip: the clipped surrogate of trl's GRPOTrainer (REF:trl/trl/trainer/grpo_trainer.py:1203-1213, loss_type "grpo") for optimizer steps that reuse a
 * rollout (num_iterations > 1; REF:...grpo_trainer.py:741-755).  old_logp: the log-probs of the policy that sampled, scored once per generation (REF:995-1002).
 * Over the mask m, with d_i = logp_i - old_logp_i, r_i = exp(d_i), rc_i = clamp(r_i, 1 - eps_low, 1 + eps_high):
 *   a token is clipped when r_i < 1 - eps_low and A < 0 (low) or r_i > 1 + eps_high and A > 0 (high), both strict
 * w (may be NULL: 1): [N, C] per-token weights -- the w_out of the iadr1_grpo_loss_is call of the step that sampled.
 *   row_stats: [N, 4] per-row partials { low-clipped live tokens, high-clipped live tokens, sum m r, max m |d| }. */
int iadr1_grpo_loss_clip(const float* logp, const float* old_logp, const float* ref_logp /* may be NULL */, const float* adv, const int* mask, const float* w /* may be NULL */,
                         float beta, float eps_low, float eps_high, int n_total_rows, float* dlogp, float* kl, float* row_loss, float* row_kl,
                         float* row_stats /* [N,4] */, int N, int C, iadr1_stream_t stream);
/* grpo_loss_ex: any of the three forms, with the two things trl's GRPOTrainer has beyond them: the row normaliser of its `loss_type`
 * (REF:trl/trl/trainer/grpo_trainer.py:1212-1219) and a step without a reference model (beta == 0: REF:...grpo_trainer.py:407, 1004-1005, 1193, 1209, 1224).
 * mean(row_loss) over the N = n_total_rows rows of a step is trl's loss for
 *   row_scale 0 ("grpo", REF:1213: every row a mean over its own live tokens),   row_scale N / max(live tokens of the batch, 1) ("bnpo", REF:1215),
 *   row_scale 1 / max_completion_length ("dr_grpo", REF:1217).
 * kl, w_out may be NULL; row_stats: [N, 5] (IS form), [N, 4] (clipped form), unused (may be NULL) otherwise. */
int iadr1_grpo_loss_ex(const float* logp, const float* ref_logp /* may be NULL */, const float* old_logp /* may be NULL */, const float* rollout_logp /* may be NULL */,
                       const float* w /* may be NULL */, const float* adv, const int* mask, float beta, float cap, int level, float eps_low, float eps_high,
                       float row_scale, int n_total_rows, float* dlogp, float* kl /* may be NULL */, float* row_loss, float* row_kl, float* w_out /* may be NULL */,
                       float* row_stats, int N, int C, iadr1_stream_t stream);
/* grpo_loss_sel: iadr1_grpo_loss_ex with a per-token selector on the ADVANTAGE term -- trl's top_entropy_quantile, which trains the policy term on the
 * highest-entropy share of the completion tokens only (trl's GRPOTrainer get_high_entropy_mask; the mask multiplies per_token_loss1 / per_token_loss2 there and
 * the KL term is added behind it).  sel: [N, C] int32 of 0 / 1 in the layout of mask, q_i = sel_i.  Everything else stays over the LIVE tokens (mask): the KL part of
 * the term and of g_i, kl, row_kl, the row normaliser (cnt, row_scale), the sequence-level importance ratio, w_out and every column of row_stats (the clip counts
 * included).  The gate is a select in front of the advantage operand, never a product by 1.0. */
int iadr1_grpo_loss_sel(const float* logp, const float* ref_logp /* may be NULL */, const float* old_logp /* may be NULL */, const float* rollout_logp /* may be NULL */,
                        const float* w /* may be NULL */, const float* adv, const int* mask, float beta, float cap, int level, float eps_low, float eps_high,
                        float row_scale, int n_total_rows, float* dlogp, float* kl /* may be NULL */, float* row_loss, float* row_kl, float* w_out /* may be NULL */,
                        float* row_stats, int N, int C, const int* sel /* may be NULL */, iadr1_stream_t stream);

/* ---- optimizer (HF Trainer default AdamW + clip_grad_norm_, TF:trainer.py:1168) ------------------------------- */
/* out[0] = sum(g^2), deterministic (fixed-order two-stage reduction; scratch = 2048 floats) so that data-parallel
 * replicas derive a bit-identical clip coefficient */
int iadr1_sumsq(const float* g, long long n, float* partials2048, float* out, iadr1_stream_t stream);
int iadr1_adamw_flat(float* master, float* m, float* v, float* grad_zeroed_after, void* param_bf16, long long n, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                     const float* norm2, float max_norm, iadr1_stream_t stream);
/* iadr1_ref_mix: the TR-DPO reference update of trl's GRPOConfig(sync_ref_model, ref_model_mixup_alpha, ref_model_sync_steps) -- SyncRefModelCallback,
 * REF:trl/trl/trainer/callbacks.py:107-109 `target_param.data.mul_(1.0 - alpha).add_(copy_param.data, alpha=alpha)` in a loop over the parameters (added to the
 * trainer at REF:trl/trl/trainer/grpo_trainer.py:666) -- over the flat bf16 parameter buffer, in place in `ref`:
 *   ref[i] = bf16_rn( fl(c * ref[i]) + fl(a * pol[i]) ),  a = (float)alpha,  c = (float)(1.0 - (double)alpha), formed on the host; fp32 products and sum, never
 *     contracted, ONE rounding to bf16 (trl's in-place bf16 arithmetic rounds twice, and how depends on the device: the formula is restated, not a backend's rounding).
 *   An element whose ref and pol hold the same bits keeps them (a select in front of the arithmetic, not a property of the rounding): zero padding and tensors the
 *     optimizer never moved stay bit-identical.  alpha == 1 copies pol.  pol is read only.
 *   dist2 (may be NULL): [2] fp32, written by the same pass from the reference BEFORE it is overwritten: dist2[0] = sum (pol - ref)^2, dist2[1] = sum ref^2 (fp32;
 *     sqrt(dist2[0] / dist2[1]) is the relative L2 distance of the policy from its reference).  Two-stage ordered reduction like iadr1_sumsq, no float atomics,
 *     run-to-run bit-identical; `partials`: a scratch of iadr1_ref_mix_partials() floats (8192).  Summation depth D = 8 T + ceil(B / 256) + 23 with
 *     B = min(ceil(n / 2048), 4096) blocks and T = ceil(n / (2048 B)) trips; relative error <= D * 2^-24 (non-negative terms).  With dist2 NULL no partial is written,
 *     partials may be NULL, and ref gets the same bits.
 *   One launch of 256-thread blocks, 16-byte loads and stores, grid-stride, grid capped at 4096 blocks like iadr1_adamw_flat (+ a one-block launch with dist2).
 *   Refused on the host, before any launch (prefix "ref_mix:"): n <= 0; n not a multiple of 8 (no scalar tail: the parameter store's offsets are multiples of 64);
 *     ref or pol NULL or not 16-byte aligned; alpha not finite or outside (0, 1]; dist2 without partials. */
int iadr1_ref_mix_partials(void);
int iadr1_ref_mix(void* ref_bf16, const void* pol_bf16, long long n, float alpha, float* partials, float* dist2, iadr1_stream_t stream);

/* ---- sampler (vLLM SamplingParams(temperature, top_p, top_k), REF:...sc_grpo_trainer.py:353-358) -------------- */
long long iadr1_sample_workspace_bytes(int B);
int iadr1_sample_topk_topp(const float* logits, long long ld, long long* out, void* workspace, int B, int V, float temperature,
                           int top_k, float top_p, int suppress_token, unsigned long long seed, unsigned step,
                           const unsigned* step_ptr, const unsigned long long* seed_ptr, iadr1_stream_t stream);
/* step_ptr / seed_ptr: optional device-resident step counter / seed that replace the scalar arguments (a captured hipGraph freezes
 * kernel arguments: the rollout replays one graph for every decode step of every optimizer step). */
/* The five entry points of this section are one device body per stage behind six kernel pairs (csrc/sample.hip: stage1 / stage2 <LP, EX, GD, EN>, each entry point launches
 * its own instantiations) and one host function: two of them give the same bits wherever what the newer one adds is neutral, and every refusal carries its entry point's
 * prefix ("sample:", "sample_logp:", "sample_ex:", "sample_guided:", "sample_ent:").  top_k <= 0 means 64 candidates in iadr1_sample_topk_topp and the whole vocabulary from
 * iadr1_sample_logp onwards. */
/* iadr1_sample_logp: the same sampler, plus what vLLM returns beside the token ids and what its evaluation callers sample with.
 *   top_k in 1..64: filter semantics, Philox stream and token ids of iadr1_sample_topk_topp, bit for bit (greedy, suppress_token, step_ptr, seed_ptr included).
 *   top_k <= 0: the WHOLE vocabulary -- vLLM SamplingParams(temperature=T, top_p=1.0) of the LLaVA evaluation script
 *     (REF:scripts/Inference/IAD-R1-Inference/vLLM_LLaVA_detect_format.py:37-39,203-205,252): one inverse-CDF draw over all V tokens in ascending id order with
 *     the uniform philox(seed; row, step): the first id whose cumulative weight sum_{i <= id} exp((x_i - max) / T) exceeds u * total.  The summation tree is fixed
 *     (run-to-run identical ids).  temperature == 0: greedy.  A suppressed token has weight 0.  top_p < 1 with top_k <= 0 is REFUSED (error through
 *     iadr1_last_error): an exact nucleus over 152 k tokens is a different kernel (a full sort or a threshold search), not built here.
 *   logp_out (may be NULL): logp_out[row * ld_logp + col] = log_softmax(logits[row, :])[picked] at temperature 1 over the full row, no filter, no suppression --
 *     the quantity the loss scores (iadr1_logprob_rows; REF:...sc_grpo_trainer.py:505-513 _get_per_token_logps), vLLM's SamplingParams(logprobs=...).
 *     col = *step_ptr (else step), the column iadr1_decode_advance writes in out_tokens; nothing is written when col >= logp_cols.
 *   workspace: iadr1_sample_logp_workspace_bytes(B) bytes.  No allocation, no float atomics, no host sync: legal under hipGraph capture. */
long long iadr1_sample_logp_workspace_bytes(int B);
int iadr1_sample_logp(const float* logits, long long ld, long long* out, float* logp_out, long long ld_logp, int logp_cols, void* workspace, int B,
                      int V, float temperature, int top_k, float top_p, int suppress_token, unsigned long long seed, unsigned step,
                      const unsigned* step_ptr, const unsigned long long* seed_ptr, iadr1_stream_t stream);
/* iadr1_sample_ex: iadr1_sample_logp with trl's GRPOConfig(repetition_penalty, min_p) in the filter.  Order as in transformers' processors and warpers:
 * repetition penalty -> temperature -> top-k -> top-p -> min_p.
 *   seen: [B, ld_seen] 32-bit words, ld_seen >= ceil(V / 32); bit (id & 31) of word (id >> 5) of row b set = sequence b has seen token id (prompt or completion).
 *   repetition_penalty (finite, > 0; 1 = off): RepetitionPenaltyLogitsProcessor -- for a seen id  x' = x < 0 ? x * pen : x / pen, one IEEE fp32 multiply or
 *     divide (no reciprocal); unseen ids keep x; -inf stays -inf; suppress_token is forced to -inf AFTER the penalty.  Everything the filter reads is x': the
 *     top-k candidates, the whole-vocabulary weights, the greedy argmax (temperature <= 0 honours the penalty and ignores min_p).
 *   min_p in [0, 1) (0 = off): MinPLogitsWarper -- with w_i = exp((x'_i - max x') / T), a token is kept iff w_i >= min_p.  top_k in 1..64: a further cut of the
 *     rank-ordered candidates behind the top-p cut (both are prefixes, the shorter wins, rank 0 always stays).  top_k <= 0 (top_p must be 1): dropped tokens
 *     have weight 0 in the inverse CDF in id order over the kept ones; this is the truncation the whole-vocabulary path has (min_p needs no sort).
 *   logp_out: UNCHANGED in meaning -- the temperature-1 log-softmax of the RAW logits at the pick (no penalty, no filter, no suppression), what
 *     iadr1_logprob_rows scores; an importance weight against it (iadr1_grpo_loss_is) keeps correcting the engine mismatch only, not the penalty or min_p.
 *   mark_seen != 0: after the pick, one thread per row sets the pick's bit in seen[row] (inside stage 2, on the sampler's stream, graph-capturable).  Rows the
 *     caller regards as finished are marked with whatever was drawn for them: harmless, their draws are discarded.
 *   min_p == 0, repetition_penalty == 1, mark_seen == 0: ids and logp_out are bit-equal to iadr1_sample_logp (the same device code), seen is not touched and
 *     may be NULL.  Refused on the host, before any launch, one message each: min_p outside [0, 1); repetition_penalty not finite or <= 0;
 *     repetition_penalty != 1 or mark_seen without seen or with ld_seen < ceil(V / 32); and everything iadr1_sample_logp refuses.
 *   Same Philox stream (seed; row, step), step_ptr / seed_ptr, two launches; workspace: iadr1_sample_ex_workspace_bytes(B).  No allocation, no host sync, no
 *     float atomics: legal under hipGraph capture. */
long long iadr1_sample_ex_workspace_bytes(int B);
int iadr1_sample_ex(const float* logits, long long ld, long long* out, float* logp_out, long long ld_logp, int logp_cols, void* workspace, int B,
                    int V, float temperature, int top_k, float top_p, float min_p, float repetition_penalty, unsigned* seen, long long ld_seen,
                    int mark_seen, int suppress_token, unsigned long long seed, unsigned step, const unsigned* step_ptr,
                    const unsigned long long* seed_ptr, iadr1_stream_t stream);
/* iadr1_sample_guided: iadr1_sample_ex with an automaton over the vocabulary in front of the filter -- trl's GRPOConfig(vllm_guided_decoding_regex), which the
 * reference hands to vLLM as a per-step allowed-token mask (REF:trl/trl/trainer/grpo_trainer.py:629,945).  Mask and state live on the device and advance inside
 * the call, so a captured decode step needs no host in the loop.
 *   state: [B] int32, read and written; row b is in automaton state state[b], 0 <= state[b] < S (a value outside is clamped into the table, never used as it is).
 *   allow: [S, ld_allow] 32-bit words, ld_allow >= ceil(V / 32), read only; bit (id & 31) of word (id >> 5) of row s set = token id may follow state s (the
 *     layout and bit order of `seen`).
 *   trans: [S, ld_trans] int16, ld_trans >= V, read only; the state after emitting id from s, or -1 where id is not allowed.  1 <= S <= 32767.
 *   Filter: a token whose bit is clear in allow[state[row]] has filter logit -inf, exactly as suppress_token does, BEFORE the repetition penalty, temperature,
 *     top-k, top-p and min_p (vLLM's order: the mask is a logits processor; -inf stays -inf through penalty and temperature).  Everything the filter reads is
 *     masked: the top-k candidates, the greedy argmax, the whole-vocabulary chunk masses and weights.  Ids are bit-equal to iadr1_sample_ex on a copy of the
 *     logits whose disallowed entries are -inf.
 *   logp_out: UNCHANGED in meaning -- the temperature-1 log-softmax of the RAW logits at the pick (no mask, no penalty, no filter): an importance weight against
 *     it keeps correcting the engine mismatch only.
 *   After the pick, one thread per row does  n = trans[state * ld_trans + pick];  state[row] = n >= 0 ? n : state  (inside stage 2, on the sampler's stream,
 *     graph-capturable; plain load and store).  The guard matters: when every allowed logit is -inf the sampler's fallbacks may return a disallowed id, and the
 *     state then stays where it was, in range.  state[row] is read once, at kernel entry, in both launches.
 *   allow == NULL (state and trans must then be NULL too): iadr1_sample_ex's own kernels are launched -- ids and logp_out bit-equal, nothing else touched.
 *   Refused on the host, before any launch, one message each (prefix "sample_guided:"): allow without state or trans; state or trans without allow; S outside
 *     1..32767; ld_allow < ceil(V / 32); ld_trans < V; and everything iadr1_sample_ex refuses.
 *   Same Philox stream (seed; row, step), step_ptr / seed_ptr, two launches; workspace: iadr1_sample_guided_workspace_bytes(B).  No allocation, no host sync,
 *     no float atomics: legal under hipGraph capture. */
long long iadr1_sample_guided_workspace_bytes(int B);
int iadr1_sample_guided(const float* logits, long long ld, long long* out, float* logp_out, long long ld_logp, int logp_cols, void* workspace, int B,
                        int V, float temperature, int top_k, float top_p, float min_p, float repetition_penalty, unsigned* seen, long long ld_seen,
                        int mark_seen, int suppress_token, unsigned long long seed, unsigned step, const unsigned* step_ptr,
                        const unsigned long long* seed_ptr, int* state, const unsigned* allow, long long ld_allow, const short* trans,
                        long long ld_trans, int S, iadr1_stream_t stream);
/* iadr1_sample_ent: iadr1_sample_guided plus the entropy of the distribution every token was sampled from -- what trl logs as `entropy` and ranks tokens by for
 * top_entropy_quantile -- out of the slices stage 1 already holds in registers.
 *   ent_out: [B, ld_ent] fp32.  ent_out[row * ld_ent + col] = H(row) = -sum_v p_v ln p_v,  p = softmax(logits[row, :]) over the RAW fp32 row at temperature 1: no
 *     suppressed token (its logit counts), no guide mask, no repetition penalty, no temperature, no top-k / top-p / min_p -- the distribution logp_out is the
 *     log-prob under.  Logits equal to -inf contribute 0; a row of -inf only gives 0.  col = *step_ptr (else step), nothing is written when col >= ent_cols: the
 *     column rule of logp_out.
 *   How: per (row, chunk) stage 1 adds  u1 = sum e_i (x_i - m1),  e_i = exp(x_i - m1)  to the partials (m1, s1); stage 2 merges, with a_c = exp(m1_c - M1),
 *     S = sum s1_c a_c,  U = sum (u1_c + (m1_c - M1) s1_c) a_c,  H = ln S - U / S.  ln S >= 0 and U <= 0: sums of same-signed terms, no cancellation; fixed trees
 *     (<= 20 serial adds, 6 shuffle levels, 3 adds over the waves, 6 shuffle levels over the chunks), no float atomics: run-to-run bit-identical.
 *   ids, logp_out, seen and state are bit-equal to iadr1_sample_guided on the same arguments (the same device code).
 *   ent_out == NULL: iadr1_sample_guided's own launch (without a guide iadr1_sample_ex's): the same kernels, the same bits; that call's workspace is enough.
 *   Otherwise the <1, 1, 0, 1> pair without a guide and the <1, 1, 1, 1> pair with one; workspace: iadr1_sample_ent_workspace_bytes(B) = the guided size +
 *     B * 32 * 4 bytes (the fifth partial lies BEHIND everything the other entry points use).
 *   Refused on the host, before any launch, one message each (prefix "sample_ent:"): ent_out with ent_cols <= 0; ent_out with ld_ent < ent_cols; and everything
 *     iadr1_sample_guided refuses (top_k <= 0 with top_p < 1 included).
 *   Same Philox stream, step_ptr / seed_ptr, two launches.  No allocation, no host sync: legal under hipGraph capture. */
long long iadr1_sample_ent_workspace_bytes(int B);
int iadr1_sample_ent(const float* logits, long long ld, long long* out, float* logp_out, long long ld_logp, int logp_cols, void* workspace, int B,
                     int V, float temperature, int top_k, float top_p, float min_p, float repetition_penalty, unsigned* seen, long long ld_seen,
                     int mark_seen, int suppress_token, unsigned long long seed, unsigned step, const unsigned* step_ptr,
                     const unsigned long long* seed_ptr, int* state, const unsigned* allow, long long ld_allow, const short* trans,
                     long long ld_trans, int S, float* ent_out, long long ld_ent, int ent_cols, iadr1_stream_t stream);
/* iadr1_sample_ent_t: iadr1_sample_ent with logp_out and ent_out taken under softmax(x / logp_temperature) of the raw row -- the quantities trl's per-token log-probs
 * and entropies are (REF:trl/trl/trainer/grpo_trainer.py:818-821), so that a rollout's log-probs compare with scores from iadr1_linear_logprob_fwd_t.
 *   With inv_tl = 1.0f / logp_temperature (host, fp32): stage 1  s1 = sum exp((x - m1) * inv_tl),  u1 = sum e * d with d = (x - m1) * inv_tl,  m1 stays the raw maximum;
 *     stage 2  a_c = exp((m1_c - M1) * inv_tl),  lse = M1 * inv_tl + ln S,  U = sum (u1_c + ((m1_c - M1) * inv_tl) * s1_c) * a_c,  H = ln S - U / S;  the pick's
 *     logp = raw * inv_tl - lse.  Still the raw row: no suppression, mask, penalty or filter -- only the temperature changes.
 *   logp_temperature touches nothing else: the filter, the whole-vocabulary masses (mT, sT) (the SAMPLING temperature), the Philox draw, `seen` and the automaton read
 *     what they read in iadr1_sample_ent, so ids, seen and state are bit-equal to that call's.  The older entry points pass inv_tl = 1: logp_temperature = 1 gives
 *     iadr1_sample_ent's bits on every output.  The same kernels (no template flag of its own) and iadr1_sample_ent's workspace.
 *   ent_out == NULL && logp_out == NULL is legal: iadr1_sample_ent's launch.
 *   Refused on the host, before any launch (prefix "sample_ent_t:"): logp_temperature not finite or <= 0, and everything iadr1_sample_ent refuses (the whole-vocabulary
 *     nucleus included).  Two launches, no allocation, no host sync: legal under hipGraph capture. */
int iadr1_sample_ent_t(const float* logits, long long ld, long long* out, float* logp_out, long long ld_logp, int logp_cols, void* workspace, int B,
                       int V, float temperature, int top_k, float top_p, float min_p, float repetition_penalty, unsigned* seen, long long ld_seen,
                       int mark_seen, int suppress_token, unsigned long long seed, unsigned step, const unsigned* step_ptr,
                       const unsigned long long* seed_ptr, int* state, const unsigned* allow, long long ld_allow, const short* trans,
                       long long ld_trans, int S, float* ent_out, long long ld_ent, int ent_cols, float logp_temperature, iadr1_stream_t stream);
/* iadr1_seen_init: the seen bitmap of a rollout's Bp * G sequences from its Bp left-padded prompts ids [Bp, S]: zeroes rows [0, Bp * G) (ld_seen words each) and,
 * for sequence r, sets the bits of the lengths[r / G] live tokens of prompt row r / G (columns [S - len, S): image placeholder ids included, left padding
 * not).  Ids outside [0, V) are ignored, never written.  One launch; integer atomic OR on global memory. */
int iadr1_seen_init(const long long* ids, int S, const int* lengths, int Bp, int G, int V, unsigned* seen, long long ld_seen, iadr1_stream_t stream);

/* ---- device-resident rollout bookkeeping (one decode step = a fixed, graph-replayable launch sequence) ------
 * rope_table: cos/sin [B, half] for the current text positions (TF:1165-1176: pos = kv_len + rope_delta).
 * decode_advance: append sampled token (EOS -> finished, then pad; REF:...sc_grpo_trainer.py:680-683,722-726),
 * bump pos / ctx_len / cache slot / step.  B <= 256 (one block). */
int iadr1_rope_table(const int* pos, const float* inv_freq, float* cos_t, float* sin_t, int B, int half,
                     iadr1_stream_t stream);
int iadr1_decode_advance(const long long* sampled, long long* cur_tok, long long* out_tokens, int C, int* pos, int* ctx_len,
                         long long* slot, const int* block_table, int max_pages, int* finished, unsigned* step, int eos,
                         int pad, int B, int* all_done, const float* inv_freq, float* cos_t, float* sin_t, int half,
                         iadr1_stream_t stream);
/* wait_counter: stream-ordered wait until the device counter `counter` (the decode step counter iadr1_decode_advance bumps, on another stream) has reached
 * `target`: one wave polls it with agent-scope loads.  `timed_out` (optional, device int) is set to 1 when `timeout_ms` (<= 60000) elapsed first -- the wait then
 * returns anyway, a counter that never arrives cannot hang the queue.  The chunked reference pass (iadr1_attn_fwd_chunk) gates each chunk on the decode
 * step that produced its last target token with this instead of an event recorded between two hipGraph launches (0.06 ms per decode step cheaper). */
int iadr1_wait_counter(const unsigned* counter, unsigned target, int timeout_ms, int* timed_out, iadr1_stream_t stream);
/* all_done (optional): 1 when every sequence has finished after this token -- the host polls it through pinned memory without draining the
 * queue (the reference's vLLM stops a request at EOS, REF:343-358).  inv_freq (optional, with cos_t / sin_t [B, half]): the rotary table
 * of the NEXT step's positions is written here, bit-identical to iadr1_rope_table on the bumped positions (one launch less per decode step). */

#ifdef __cplusplus
}
#endif
#endif
