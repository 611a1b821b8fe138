// Log-prob / cross-entropy / GRPO-loss kernels (gfx950).
//
// logprob_rows: per row of an fp32 logit chunk [R,V] (written by gemm_nt with out_mode=1, never by
// the reference's bf16 [B,S,V] tensor): lse = logsumexp(row), logp = row[target] - lse
//   == `logits_row.log_softmax(-1)` + gather, /root/reference/train/stage_rl/trainer/sc_grpo_trainer.py:510-513
//   (no temperature division), and == -CE for PA-SFT (TF:loss/loss_utils.py:32-71).
// dlogits_rows: dlogit = g[row] * (onehot(target) - softmax(row)) in bf16, in a form ready for the two
// backward GEMMs (dH = dlogits . W, dW = dlogits^T . H).
// grpo_loss: sc_grpo_trainer.py:746,796-798,816 for one rank's [N,C] completion block.  grpo_loss_is: the same with a truncated importance weight per token.
// grpo_loss_clip: the clipped surrogate of trl's GRPOTrainer (trl/trl/trainer/grpo_trainer.py:1203-1213) for optimizer steps that reuse a rollout (num_iterations > 1).
// grpo_loss_ex: the same three kernels behind one entry point, with the row normaliser of trl's loss_type (grpo_trainer.py:1212-1219) and an optional reference.
// grpo_loss_sel: grpo_loss_ex with a per-token 0/1 selector on the advantage term (trl's top_entropy_quantile mask, grpo_trainer.py get_high_entropy_mask).
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void logprob_rows_kernel(const float* logits, long long ld, const long long* targets, float* logp,
                                                           float* lse_out, int R, int V) {
    __shared__ float scratch[16];
    const int row = blockIdx.x;
    const float* x = logits + (long long)row * ld;
    float m = -INFINITY, s = 0.f;
    const int n4 = V >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) {
        const f32x4_t v = *(const f32x4_t*)(x + i * 4);
        const float mx = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
        if (mx == -INFINITY) continue;      // a group of masked (-inf) logits adds nothing; with m still -inf, exp(-inf - -inf) would be NaN
        if (mx > m) { s *= __expf(m - mx); m = mx; }
        s += __expf(v[0] - m) + __expf(v[1] - m) + __expf(v[2] - m) + __expf(v[3] - m);
    }
    for (int i = n4 * 4 + threadIdx.x; i < V; i += 256) {
        const float v = x[i];
        if (v == -INFINITY) continue;
        if (v > m) { s *= __expf(m - v); m = v; }
        s += __expf(v - m);
    }
    const float gm = block_max<256>(m, scratch);
    s = (m == -INFINITY) ? 0.f : s * __expf(m - gm);
    const float gs = block_sum<256>(s, scratch);
    if (threadIdx.x == 0) {
        const float lse = gm + logf(gs);
        if (lse_out) lse_out[row] = lse;
        const long long tgt = targets[row];
        logp[row] = (tgt >= 0 && tgt < V) ? x[tgt] - lse : 0.f;  // ignored rows (target < 0, e.g. -100) contribute 0
    }
}

__global__ __launch_bounds__(256) void dlogits_rows_kernel(const float* logits, long long ld, const long long* targets, const float* lse,
                                                           const float* g, bf16_t* dl, long long ldd, int R, int V) {
    const int row = blockIdx.y;
    const float* x = logits + (long long)row * ld;
    const float l = lse[row], gr = g[row];
    const long long tgt = targets[row];
    const int n8 = V >> 3;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n8; i += gridDim.x * 256) {
        const f32x4_t a = *(const f32x4_t*)(x + i * 8), b = *(const f32x4_t*)(x + i * 8 + 4);
        float o[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) { o[e] = -gr * __expf(a[e] - l); o[4 + e] = -gr * __expf(b[e] - l); }
        if (tgt >= (long long)i * 8 && tgt < (long long)i * 8 + 8) {
#pragma unroll
            for (int e = 0; e < 8; ++e) if (tgt == (long long)i * 8 + e) o[e] += gr;
        }
        *(u32x4_t*)(dl + (long long)row * ldd + i * 8) = (u32x4_t){pack2bf(o[0], o[1]), pack2bf(o[2], o[3]), pack2bf(o[4], o[5]), pack2bf(o[6], o[7])};
    }
}

// ref_logp - logp of one token.  REF false (no reference model, beta == 0): the constant 0, so kl = exp(0) - 0 - 1 = 0 and the KL part of the gradient is
// beta (1 - exp(0)) = 0 at compile time, and no load through ref_logp exists in that instantiation.
template <bool REF>
__device__ __forceinline__ float ref_gap(const float* ref_logp, const float* logp, int i) {
    if constexpr (REF) return ref_logp[i] - logp[i];
    else return 0.f;
}

// The three loss kernels share two parameters.  REF: see ref_gap.  row_scale: 0 = every row's sums are divided by its live-token count (inv = 1 / cnt, trl's
// loss_type "grpo"); > 0 = this factor instead, the same for every row ("bnpo": rows / live tokens of the batch, "dr_grpo": 1 / max_completion_length).  It
// replaces inv in row_loss and dlogp only: row_kl and the sequence-level importance ratio stay means over cnt.
// SEL (iadr1_grpo_loss_sel): sel [N, C] of 0 / 1 in the layout of mask gates the ADVANTAGE part of a token's term and of its gradient -- with q = sel_i the term
// is w (-(q s - beta kl)), s = A or min(r A, rc A).  The KL part, kl_out, row_kl, cnt, the importance ratio, row_stats and the clip counts keep running over the
// live tokens.  The gate is a select in front of the expression (never a product by 1.0f), so that with q = 1 every expression is the SEL = false one on the
// same operands.  SEL false: no load through sel exists.
template <bool SEL>
__device__ __forceinline__ float gated(const int* sel, int i, float a) {
    if constexpr (SEL) return sel[i] != 0 ? a : 0.f;
    else return a;
}

// One block per sequence row.  Outputs: dlogp [N,C] (gradient of the batch loss w.r.t. the policy
// log-probs), per-token kl [N,C], and per-row partials row_loss[N], row_kl[N] (means over the mask).
template <bool REF, bool SEL = false>
__global__ __launch_bounds__(256) void grpo_loss_kernel(const float* logp, const float* ref_logp, const float* adv, const int* mask,
                                                        float beta, float inv_nrows, float row_scale, float* dlogp, float* kl_out, float* row_loss,
                                                        float* row_kl, int N, int C, const int* sel = nullptr) {
    __shared__ float scratch[16];
    const int n = blockIdx.x;
    const float A = adv[n];
    float cnt = 0.f, sl = 0.f, sk = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) {
        const int i = n * C + c;
        const float d = ref_gap<REF>(ref_logp, logp, i);
        const float e = __expf(d);
        const float kl = e - d - 1.f;
        const float m = (float)mask[i];
        if (kl_out) kl_out[i] = kl;
        cnt += m;
        const float Aq = gated<SEL>(sel, i, A);
        sl += m * (-(Aq - beta * kl));  // exp(p - p.detach()) == 1 in value
        sk += m * kl;
    }
    cnt = block_sum<256>(cnt, scratch);
    sl = block_sum<256>(sl, scratch);
    sk = block_sum<256>(sk, scratch);
    const float inv = cnt > 0.f ? 1.f / cnt : 0.f;
    const float scale = row_scale > 0.f ? row_scale : inv;
    if (threadIdx.x == 0) {
        row_loss[n] = sl * scale;
        row_kl[n] = sk * inv;
    }
    for (int c = threadIdx.x; c < C; c += 256) {
        const int i = n * C + c;
        const float d = ref_gap<REF>(ref_logp, logp, i);
        // d/dp [ -(exp(p - sg p) A - beta (exp(r-p) - (r-p) - 1)) ] = -A + beta (1 - exp(r-p))
        const float Aq = gated<SEL>(sel, i, A);
        dlogp[i] = (float)mask[i] * scale * inv_nrows * (-Aq + beta * (1.f - __expf(d)));
    }
}

// grpo_loss with a truncated importance weight per token (rollout / trainer log-prob mismatch).  d = logp - rollout_logp over the mask;
//   level 0 (token):    w_i = min(exp(d_i), cap)          level 1 (sequence): w_i = min(exp(sum m d / cnt), cap) for every token of the row
// w multiplies the whole per-token term (advantage and KL parts) and is a constant under differentiation; row_kl / kl_out stay unweighted.  Masked positions
// (rollout_logp == 0 there by the rollout's contract) get d = 0 by a select and never reach an exp that feeds a sum.  With w == 1 every expression below rounds
// as grpo_loss_kernel's does (1 * x is exact), so the four shared outputs are then bit-equal to that kernel's.
// row_stats[n][5] = { sum m w, live tokens whose untruncated ratio exceeded cap, sum m |d|, max m |d|, sum m (exp(d) - d - 1) }.
template <bool REF, bool SEL = false>
__global__ __launch_bounds__(256) void grpo_loss_is_kernel(const float* logp, const float* ref_logp, const float* rollout_logp, const float* adv,
                                                           const int* mask, float beta, float cap, int level, float inv_nrows, float row_scale, float* dlogp,
                                                           float* kl_out, float* row_loss, float* row_kl, float* w_out, float* row_stats, int N, int C,
                                                           const int* sel = nullptr) {
    __shared__ float scratch[16];
    const int n = blockIdx.x;
    const float A = adv[n];
    float cnt = 0.f, sd = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) {
        const int i = n * C + c;
        const int live = mask[i] != 0;
        cnt += (float)mask[i];
        sd += live ? logp[i] - rollout_logp[i] : 0.f;
    }
    cnt = block_sum<256>(cnt, scratch);
    sd = block_sum<256>(sd, scratch);
    const float inv = cnt > 0.f ? 1.f / cnt : 0.f;
    const float scale = row_scale > 0.f ? row_scale : inv;
    const float ratio_row = __expf(sd * inv);
    const float w_row = ratio_row > cap ? cap : ratio_row;
    float sl = 0.f, sk = 0.f, sw = 0.f, nclip = 0.f, sabs = 0.f, mabs = 0.f, sk3 = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) {
        const int i = n * C + c;
        const float d = ref_gap<REF>(ref_logp, logp, i);
        const float e = __expf(d);
        const float kl = e - d - 1.f;
        const float m = (float)mask[i];
        if (kl_out) kl_out[i] = kl;
        const int live = mask[i] != 0;
        const float dq = live ? logp[i] - rollout_logp[i] : 0.f;
        const float ratio = __expf(dq);
        const float w = level == 0 ? (ratio > cap ? cap : ratio) : w_row;
        const float Aq = gated<SEL>(sel, i, A);
        const float t = -(Aq - beta * kl);
        sl += m * (w * t);
        sk += m * kl;
        if (live) {
            sw += w;
            nclip += (level == 0 ? ratio : ratio_row) > cap ? 1.f : 0.f;
            sabs += fabsf(dq);
            mabs = fmaxf(mabs, fabsf(dq));
            sk3 += ratio - dq - 1.f;
        }
    }
    sl = block_sum<256>(sl, scratch);
    sk = block_sum<256>(sk, scratch);
    sw = block_sum<256>(sw, scratch);
    nclip = block_sum<256>(nclip, scratch);
    sabs = block_sum<256>(sabs, scratch);
    mabs = block_max<256>(mabs, scratch);
    sk3 = block_sum<256>(sk3, scratch);
    if (threadIdx.x == 0) {
        row_loss[n] = sl * scale;
        row_kl[n] = sk * inv;
        float* st = row_stats + (long long)n * 5;
        st[0] = sw; st[1] = nclip; st[2] = sabs; st[3] = mabs; st[4] = sk3;
    }
    for (int c = threadIdx.x; c < C; c += 256) {
        const int i = n * C + c;
        const float d = ref_gap<REF>(ref_logp, logp, i);
        const int live = mask[i] != 0;
        const float ratio = __expf(live ? logp[i] - rollout_logp[i] : 0.f);
        const float w = level == 0 ? (ratio > cap ? cap : ratio) : w_row;
        // grpo_loss_kernel's expression, then the weight: the product by w stays outside so that nothing of the unweighted value is contracted differently
        const float Aq = gated<SEL>(sel, i, A);
        const float g = (float)mask[i] * scale * inv_nrows * (-Aq + beta * (1.f - __expf(d)));
        dlogp[i] = w * g;
        if (w_out) w_out[i] = live ? w : 0.f;
    }
}

// grpo_loss with the clipped surrogate against OLD log-probs (a rollout scored once, then used for several optimizer steps).  d = logp - old_logp over the mask;
//   r = exp(d),  rc = clamp(r, 1 - eps_low, 1 + eps_high),  s = min(r A, rc A),  per-token loss  w (-(s - beta kl)),  w = 1 without w[]
// A token is clipped when the min took the clamped (constant) branch: r < 1 - eps_low with A < 0, or r > 1 + eps_high with A > 0 (both strict); its advantage
// term then has no gradient.  w (grpo_loss_is's w_out of the step that sampled) is a constant under differentiation; row_kl / kl_out stay unweighted.  Masked
// positions get d = 0 by a select: old_logp there may hold anything (NaN included) and never reaches a sum.  On policy (old_logp == logp bitwise) r = rc = 1
// and s = A exactly, so every expression below rounds as grpo_loss_is_kernel's (and, with w == 1, grpo_loss_kernel's) does: the products r * A sit behind a
// min / a select, where nothing contracts them into the sums that follow.
// row_stats[n][4] = { low-clipped live tokens, high-clipped live tokens, sum m r, max m |d| }.
template <bool REF, bool SEL = false>
__global__ __launch_bounds__(256) void grpo_loss_clip_kernel(const float* logp, const float* old_logp, const float* ref_logp, const float* adv, const int* mask,
                                                             const float* w_in, float beta, float lo, float hi, float inv_nrows, float row_scale, float* dlogp, float* kl_out,
                                                             float* row_loss, float* row_kl, float* row_stats, int N, int C, const int* sel = nullptr) {
    __shared__ float scratch[16];
    const int n = blockIdx.x;
    const float A = adv[n];
    float cnt = 0.f, sl = 0.f, sk = 0.f, nlo = 0.f, nhi = 0.f, sr = 0.f, mabs = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) {
        const int i = n * C + c;
        const float d = ref_gap<REF>(ref_logp, logp, i);
        const float e = __expf(d);
        const float kl = e - d - 1.f;
        const float m = (float)mask[i];
        if (kl_out) kl_out[i] = kl;
        const int live = mask[i] != 0;
        const float dq = live ? logp[i] - old_logp[i] : 0.f;
        const float r = __expf(dq);
        const float rc = fminf(fmaxf(r, lo), hi);
        const float s = gated<SEL>(sel, i, fminf(r * A, rc * A));
        const float w = w_in ? w_in[i] : 1.f;
        const float t = -(s - beta * kl);
        cnt += m;
        sl += m * (w * t);
        sk += m * kl;
        if (live) {
            nlo += (r < lo && A < 0.f) ? 1.f : 0.f;
            nhi += (r > hi && A > 0.f) ? 1.f : 0.f;
            sr += r;
            mabs = fmaxf(mabs, fabsf(dq));
        }
    }
    cnt = block_sum<256>(cnt, scratch);
    sl = block_sum<256>(sl, scratch);
    sk = block_sum<256>(sk, scratch);
    nlo = block_sum<256>(nlo, scratch);
    nhi = block_sum<256>(nhi, scratch);
    sr = block_sum<256>(sr, scratch);
    mabs = block_max<256>(mabs, scratch);
    const float inv = cnt > 0.f ? 1.f / cnt : 0.f;
    const float scale = row_scale > 0.f ? row_scale : inv;
    if (threadIdx.x == 0) {
        row_loss[n] = sl * scale;
        row_kl[n] = sk * inv;
        float* st = row_stats + (long long)n * 4;
        st[0] = nlo; st[1] = nhi; st[2] = sr; st[3] = mabs;
    }
    for (int c = threadIdx.x; c < C; c += 256) {
        const int i = n * C + c;
        const float d = ref_gap<REF>(ref_logp, logp, i);
        const int live = mask[i] != 0;
        const float r = __expf(live ? logp[i] - old_logp[i] : 0.f);
        const bool clipped = (r < lo && A < 0.f) || (r > hi && A > 0.f);
        // d/dp min(r A, rc A) = r A where the unclamped branch is the min, 0 where the clamped one is
        const float ga = gated<SEL>(sel, i, clipped ? 0.f : r * A);
        const float w = w_in ? w_in[i] : 1.f;
        // grpo_loss_kernel's expression with r A for A, then the weight (as in grpo_loss_is_kernel).  Both of those compile -A + beta (1 - e) to a rounded product
        // and a subtraction (the two products of the line pair up into packed multiplies, which leaves nothing to contract); the select in front of ga would let
        // this one become an fma, one rounding fewer, so contraction is switched off for it
        float g;
        {
#pragma clang fp contract(off)
            const float bk = beta * (1.f - __expf(d));
            g = (float)mask[i] * scale * inv_nrows * (bk - ga);
        }
        dlogp[i] = w * g;
    }
}

}  // namespace

extern "C" int iadr1_logprob_rows(const float* logits, long long ld, const long long* targets, float* logp, float* lse, int R, int V,
                                  hipStream_t stream) {
    IADR1_REQUIRE(R > 0 && V > 0 && (ld % 4) == 0, "logprob_rows: ld must be a multiple of 4");
    hipLaunchKernelGGL(logprob_rows_kernel, dim3(R), dim3(256), 0, stream, logits, ld, targets, logp, lse, R, V);
    return iadr1_check_launch("logprob_rows");
}
extern "C" int iadr1_dlogits_rows(const float* logits, long long ld, const long long* targets, const float* lse, const float* g, void* dl,
                                  long long ldd, int R, int V, hipStream_t stream) {
    IADR1_REQUIRE(R > 0 && V > 0 && (V % 8) == 0 && (ld % 4) == 0 && (ldd % 8) == 0, "dlogits_rows: V, ldd multiples of 8, ld multiple of 4");
    int gx = (V / 8 + 255) / 256;
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(dlogits_rows_kernel, dim3(gx, R), dim3(256), 0, stream, logits, ld, targets, lse, g, (bf16_t*)dl, ldd, R, V);
    return iadr1_check_launch("dlogits_rows");
}
extern "C" int iadr1_grpo_loss(const float* logp, const float* ref_logp, const float* adv, const int* mask, float beta, int n_total_rows,
                               float* dlogp, float* kl, float* row_loss, float* row_kl, int N, int C, hipStream_t stream) {
    IADR1_REQUIRE(N > 0 && C > 0 && n_total_rows >= N, "grpo_loss: need 0 < N <= n_total_rows");
    hipLaunchKernelGGL(grpo_loss_kernel<true>, dim3(N), dim3(256), 0, stream, logp, ref_logp, adv, mask, beta, 1.f / (float)n_total_rows, 0.f, dlogp, kl, row_loss, row_kl, N, C);
    return iadr1_check_launch("grpo_loss");
}
extern "C" int iadr1_grpo_loss_is(const float* logp, const float* ref_logp, const float* rollout_logp, const float* adv, const int* mask, float beta,
                                  float cap, int level, int n_total_rows, float* dlogp, float* kl, float* row_loss, float* row_kl, float* w_out,
                                  float* row_stats, int N, int C, hipStream_t stream) {
    IADR1_REQUIRE(N > 0, "grpo_loss_is: N must be > 0 (got %d)", N);
    IADR1_REQUIRE(rollout_logp != nullptr, "grpo_loss_is: rollout_logp is null (the weight needs the rollout's log-probs)");
    IADR1_REQUIRE(cap >= 1.f && cap <= 3.402823466e38f /* false for NaN and +inf */, "grpo_loss_is: cap must be finite and >= 1 (got %g): a smaller cap would down-weight on-policy tokens", (double)cap);
    IADR1_REQUIRE(level == 0 || level == 1, "grpo_loss_is: unknown level %d (0 = token, 1 = sequence)", level);
    IADR1_REQUIRE(C > 0 && n_total_rows >= N, "grpo_loss_is: need C > 0 and N <= n_total_rows");
    IADR1_REQUIRE(row_stats != nullptr, "grpo_loss_is: row_stats is null");
    hipLaunchKernelGGL(grpo_loss_is_kernel<true>, dim3(N), dim3(256), 0, stream, logp, ref_logp, rollout_logp, adv, mask, beta, cap, level,
                       1.f / (float)n_total_rows, 0.f, dlogp, kl, row_loss, row_kl, w_out, row_stats, N, C);
    return iadr1_check_launch("grpo_loss_is");
}
extern "C" int iadr1_grpo_loss_clip(const float* logp, const float* old_logp, const float* ref_logp, const float* adv, const int* mask, const float* w,
                                    float beta, float eps_low, float eps_high, int n_total_rows, float* dlogp, float* kl, float* row_loss, float* row_kl,
                                    float* row_stats, int N, int C, hipStream_t stream) {
    IADR1_REQUIRE(N > 0, "grpo_loss_clip: N must be > 0 (got %d)", N);
    IADR1_REQUIRE(old_logp != nullptr, "grpo_loss_clip: old_logp is null (the ratio needs the log-probs of the policy that sampled)");
    IADR1_REQUIRE(row_stats != nullptr, "grpo_loss_clip: row_stats is null");
    IADR1_REQUIRE(eps_low >= 0.f && eps_low < 1.f /* false for NaN */, "grpo_loss_clip: eps_low must be in [0, 1) (got %g)", (double)eps_low);
    IADR1_REQUIRE(eps_high >= 0.f && eps_high <= 3.402823466e38f /* false for NaN and +inf */, "grpo_loss_clip: eps_high must be finite and >= 0 (got %g)", (double)eps_high);
    IADR1_REQUIRE(C > 0 && n_total_rows >= N, "grpo_loss_clip: need C > 0 and N <= n_total_rows");
    hipLaunchKernelGGL(grpo_loss_clip_kernel<true>, dim3(N), dim3(256), 0, stream, logp, old_logp, ref_logp, adv, mask, w, beta, 1.f - eps_low, 1.f + eps_high,
                       1.f / (float)n_total_rows, 0.f, dlogp, kl, row_loss, row_kl, row_stats, N, C);
    return iadr1_check_launch("grpo_loss_clip");
}
// The three forms above behind one entry point: which one runs follows from which of old_logp / rollout_logp is given, REF from ref_logp, and row_scale is
// handed through.  With ref_logp given and row_scale == 0 the launch is the old entry point's, argument for argument.
// SEL: iadr1_grpo_loss_sel's selector; `name` is the entry point's, the prefix of its refusals.
namespace {
template <bool SEL>
int grpo_loss_ex_launch(const char* name, const float* logp, const float* ref_logp, const float* old_logp, const float* rollout_logp, const float* w, const float* adv,
                        const int* mask, float beta, float cap, int level, float eps_low, float eps_high, float row_scale, int n_total_rows, float* dlogp, float* kl,
                        float* row_loss, float* row_kl, float* w_out, float* row_stats, int N, int C, const int* sel, hipStream_t stream) {
    IADR1_REQUIRE(N > 0, "%s: N must be > 0 (got %d)", name, N);
    IADR1_REQUIRE(C > 0, "%s: C must be > 0 (got %d)", name, C);
    IADR1_REQUIRE(n_total_rows >= N, "%s: n_total_rows (%d) is smaller than N (%d): it is the row count of the whole step", name, n_total_rows, N);
    IADR1_REQUIRE(ref_logp != nullptr || beta == 0.f, "%s: ref_logp is null with beta = %g: the KL term needs the reference's log-probs (only beta == 0 runs without them)", name, (double)beta);
    IADR1_REQUIRE(row_scale >= 0.f && row_scale <= 3.402823466e38f /* false for NaN and +inf */, "%s: row_scale must be 0 (1 / live tokens of the row) or finite and > 0 (got %g)", name, (double)row_scale);
    IADR1_REQUIRE(old_logp == nullptr || rollout_logp == nullptr, "%s: old_logp and rollout_logp are both given: a reuse step takes the cached weights as w, not the rollout's log-probs", name);
    IADR1_REQUIRE(w == nullptr || old_logp != nullptr, "%s: w is given without old_logp (the weights belong to the clipped form)", name);
    IADR1_REQUIRE(row_stats != nullptr || (old_logp == nullptr && rollout_logp == nullptr), "%s: row_stats is null (the %s form writes [N, %d] partials)", name, old_logp ? "clip" : "IS", old_logp ? 4 : 5);
    const float inv_nrows = 1.f / (float)n_total_rows;
    if (old_logp != nullptr) {
        IADR1_REQUIRE(eps_low >= 0.f && eps_low < 1.f /* false for NaN */, "%s: eps_low must be in [0, 1) (got %g)", name, (double)eps_low);
        IADR1_REQUIRE(eps_high >= 0.f && eps_high <= 3.402823466e38f /* false for NaN and +inf */, "%s: eps_high must be finite and >= 0 (got %g)", name, (double)eps_high);
        if (ref_logp != nullptr)
            hipLaunchKernelGGL((grpo_loss_clip_kernel<true, SEL>), dim3(N), dim3(256), 0, stream, logp, old_logp, ref_logp, adv, mask, w, beta, 1.f - eps_low, 1.f + eps_high,
                               inv_nrows, row_scale, dlogp, kl, row_loss, row_kl, row_stats, N, C, sel);
        else
            hipLaunchKernelGGL((grpo_loss_clip_kernel<false, SEL>), dim3(N), dim3(256), 0, stream, logp, old_logp, ref_logp, adv, mask, w, beta, 1.f - eps_low, 1.f + eps_high,
                               inv_nrows, row_scale, dlogp, kl, row_loss, row_kl, row_stats, N, C, sel);
    } else if (rollout_logp != nullptr) {
        IADR1_REQUIRE(cap >= 1.f && cap <= 3.402823466e38f /* false for NaN and +inf */, "%s: cap must be finite and >= 1 (got %g): a smaller cap would down-weight on-policy tokens", name, (double)cap);
        IADR1_REQUIRE(level == 0 || level == 1, "%s: unknown level %d (0 = token, 1 = sequence)", name, level);
        if (ref_logp != nullptr)
            hipLaunchKernelGGL((grpo_loss_is_kernel<true, SEL>), dim3(N), dim3(256), 0, stream, logp, ref_logp, rollout_logp, adv, mask, beta, cap, level, inv_nrows, row_scale,
                               dlogp, kl, row_loss, row_kl, w_out, row_stats, N, C, sel);
        else
            hipLaunchKernelGGL((grpo_loss_is_kernel<false, SEL>), dim3(N), dim3(256), 0, stream, logp, ref_logp, rollout_logp, adv, mask, beta, cap, level, inv_nrows, row_scale,
                               dlogp, kl, row_loss, row_kl, w_out, row_stats, N, C, sel);
    } else {
        if (ref_logp != nullptr)
            hipLaunchKernelGGL((grpo_loss_kernel<true, SEL>), dim3(N), dim3(256), 0, stream, logp, ref_logp, adv, mask, beta, inv_nrows, row_scale, dlogp, kl, row_loss, row_kl, N, C, sel);
        else
            hipLaunchKernelGGL((grpo_loss_kernel<false, SEL>), dim3(N), dim3(256), 0, stream, logp, ref_logp, adv, mask, beta, inv_nrows, row_scale, dlogp, kl, row_loss, row_kl, N, C, sel);
    }
    return iadr1_check_launch(name);
}
}  // namespace
extern "C" int iadr1_grpo_loss_ex(const float* logp, const float* ref_logp, const float* old_logp, const float* rollout_logp, const float* w, const float* adv,
                                  const int* mask, float beta, float cap, int level, float eps_low, float eps_high, float row_scale, int n_total_rows, float* dlogp,
                                  float* kl, float* row_loss, float* row_kl, float* w_out, float* row_stats, int N, int C, hipStream_t stream) {
    return grpo_loss_ex_launch<false>("grpo_loss_ex", logp, ref_logp, old_logp, rollout_logp, w, adv, mask, beta, cap, level, eps_low, eps_high, row_scale, n_total_rows, dlogp, kl,
                                      row_loss, row_kl, w_out, row_stats, N, C, nullptr, stream);
}
// iadr1_grpo_loss_ex with the selector.  sel == NULL: that entry point's kernels and arguments.
extern "C" int iadr1_grpo_loss_sel(const float* logp, const float* ref_logp, const float* old_logp, const float* rollout_logp, const float* w, const float* adv,
                                   const int* mask, float beta, float cap, int level, float eps_low, float eps_high, float row_scale, int n_total_rows, float* dlogp,
                                   float* kl, float* row_loss, float* row_kl, float* w_out, float* row_stats, int N, int C, const int* sel, hipStream_t stream) {
    return (sel != nullptr ? grpo_loss_ex_launch<true> : grpo_loss_ex_launch<false>)("grpo_loss_sel", logp, ref_logp, old_logp, rollout_logp, w, adv, mask, beta, cap, level, eps_low,
                                                                                     eps_high, row_scale, n_total_rows, dlogp, kl, row_loss, row_kl, w_out, row_stats, N, C, sel, stream);
}
