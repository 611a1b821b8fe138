// Log-prob / cross-entropy / GRPO-loss kernels (gfx950).
//
// logprob_rows: per row of an fp32 logit chunk [R,V] (written by gemm_nt with out_mode=1, never by
// the reference's bf16 [B,S,V] tensor): lse = logsumexp(row), logp = row[target] - lse
//   == `logits_row.log_softmax(-1)` + gather, REF:train/stage_rl/trainer/sc_grpo_trainer.py:510-513
//   (no temperature division), and == -CE for PA-SFT (TF:loss/loss_utils.py:32-71).
// dlogits_rows: dlogit = g[row] * (onehot(target) - softmax(row)) in bf16, in a form ready for the two
// backward GEMMs (dH = dlogits . W, dW = dlogits^T . H).
// grpo_loss: sc_grpo_trainer.py:746,796-798,816 for one rank's [N,C] completion block, in three forms computed by ONE kernel body (grpo_loss_kernel<FORM, REF, SEL>)
// behind ONE host function (grpo_loss_launch) and five entry points:
//   plain (iadr1_grpo_loss);  IS: a truncated importance weight per token (iadr1_grpo_loss_is);  clip: the clipped surrogate of trl's GRPOTrainer
//   (trl/trl/trainer/grpo_trainer.py:1203-1213) for optimizer steps that reuse a rollout, num_iterations > 1 (iadr1_grpo_loss_clip);
//   iadr1_grpo_loss_ex: any of the three, with the row normaliser of trl's loss_type (grpo_trainer.py:1212-1219);
//   iadr1_grpo_loss_sel: that with a per-token 0/1 selector on the advantage term (trl's top_entropy_quantile mask, grpo_trainer.py get_high_entropy_mask).
// Every entry point runs without a reference (ref_logp NULL) when beta == 0.
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

// ---- GRPO loss: one device body, one host function ------------------------------------------------------------------------------------------------------
// One block per sequence row of one rank's [N, C] completion block.  Outputs: dlogp [N,C] (gradient of the batch loss w.r.t. the policy log-probs), per-token
// kl [N,C] (optional), per-row partials row_loss[N], row_kl[N], and the form's w_out / row_stats.  Per live token (mask m), with kl = exp(d) - d - 1 and
// d = ref_logp - logp, the term is  w (-(q s - beta kl))  and the three forms differ in s and w only:
//   PLAIN: s = A (exp(p - sg p) == 1 in value), no w.
//   IS:    s = A, w a truncated importance weight against the rollout's log-probs (rollout / trainer mismatch).  dq = logp - rollout_logp over the mask;
//          level 0 (token): w_i = min(exp(dq_i), cap)     level 1 (sequence): w_i = min(exp(sum m dq / cnt), cap) for every token of the row.
//          row_stats[n][5] = { sum m w, live tokens whose untruncated ratio exceeded cap, sum m |dq|, max m |dq|, sum m (exp(dq) - dq - 1) }.
//   CLIP:  the clipped surrogate against OLD log-probs (a rollout scored once, then used for several optimizer steps).  dq = logp - old_logp over the mask,
//          r = exp(dq), rc = clamp(r, lo = 1 - eps_low, hi = 1 + eps_high), s = min(r A, rc A), w = w_in[] or 1 (the IS form's w_out of the step that sampled).
//          A token is clipped when the min took the clamped (constant) branch: r < lo with A < 0, or r > hi with A > 0 (both strict); its advantage term then
//          has no gradient.  row_stats[n][4] = { low-clipped live tokens, high-clipped live tokens, sum m r, max m |dq| }.
// w is a constant under differentiation and multiplies the whole term (advantage and KL parts); kl_out and row_kl stay unweighted.  Masked positions get dq = 0
// by a select: rollout_logp / old_logp there may hold anything (NaN included) and never reach an exp that feeds a sum.
// row_scale: 0 = every row's sums are divided by its live-token count (inv = 1 / cnt, trl's loss_type "grpo"); > 0 = this factor instead, the same for every
// row ("bnpo": rows / live tokens of the batch, "dr_grpo": 1 / max_completion_length).  It replaces inv in row_loss and dlogp only: row_kl and the sequence-level
// importance ratio stay means over cnt.
enum { PLAIN, IS, CLIP };

struct GrpoLossArgs {
    const float *logp, *ref_logp, *q_logp /* IS: rollout_logp, CLIP: old_logp */, *adv, *w_in;
    const int *mask, *sel;
    float beta, cap, lo, hi, inv_nrows, row_scale;
    int level;
    float *dlogp, *kl_out, *row_loss, *row_kl, *w_out, *row_stats;
    int C;
};

// ref_logp - logp of one token.  REF false (no reference model, beta == 0): the constant 0, so kl = exp(0) - 0 - 1 = 0 and the KL part of the gradient is
// beta (1 - exp(0)) = 0 at compile time, and no load through ref_logp exists in that instantiation.
template <bool REF>
__device__ __forceinline__ float ref_gap(const float* ref_logp, const float* logp, int i) {
    if constexpr (REF) return ref_logp[i] - logp[i];
    else return 0.f;
}

// SEL (iadr1_grpo_loss_sel): sel [N, C] of 0 / 1 in the layout of mask gates the ADVANTAGE part of a token's term and of its gradient -- with q = sel_i the term
// is w (-(q s - beta kl)).  The KL part, kl_out, row_kl, cnt, the importance ratio, row_stats and the clip counts keep running over the live tokens.  The gate
// is a select in front of the expression (never a product by 1.0f), so that with q = 1 every expression is the SEL = false one on the same operands.  SEL
// false: no load through sel exists.
template <bool SEL>
__device__ __forceinline__ float gated(const int* sel, int i, float a) {
    if constexpr (SEL) return sel[i] != 0 ? a : 0.f;
    else return a;
}

__device__ __forceinline__ float inv_or_zero(float cnt) { return cnt > 0.f ? 1.f / cnt : 0.f; }

template <int FORM, bool REF, bool SEL>
__global__ __launch_bounds__(256) void grpo_loss_kernel(const GrpoLossArgs a) {
    __shared__ float scratch[16];
    const int n = blockIdx.x, C = a.C;
    const float A = a.adv[n], beta = a.beta, cap = a.cap, lo = a.lo, hi = a.hi;
    float cnt = 0.f, ratio_row = 0.f, w_row = 0.f;
    if constexpr (FORM == IS) {     // the sequence-level ratio needs the row's count and sum m dq before the main pass
        float sd = 0.f;
        for (int c = threadIdx.x; c < C; c += 256) {
            const int i = n * C + c;
            const int live = a.mask[i] != 0;
            cnt += (float)a.mask[i];
            sd += live ? a.logp[i] - a.q_logp[i] : 0.f;
        }
        cnt = block_sum<256>(cnt, scratch);
        sd = block_sum<256>(sd, scratch);
        ratio_row = __expf(sd * inv_or_zero(cnt));
        w_row = ratio_row > cap ? cap : ratio_row;
    }
    float sl = 0.f, sk = 0.f;
    float sw = 0.f, nclip = 0.f, sabs = 0.f, mabs = 0.f, sk3 = 0.f;     // IS statistics (mabs: CLIP's too)
    float nlo = 0.f, nhi = 0.f, sr = 0.f;                               // CLIP statistics
    for (int c = threadIdx.x; c < C; c += 256) {
        const int i = n * C + c;
        const float d = ref_gap<REF>(a.ref_logp, a.logp, i);
        const float e = __expf(d);
        const float kl = e - d - 1.f;
        const float m = (float)a.mask[i];
        if (a.kl_out) a.kl_out[i] = kl;
        if constexpr (FORM != IS) cnt += m;
        const int live = a.mask[i] != 0;
        float dq = 0.f, r = 1.f, s = A, w = 1.f;
        if constexpr (FORM != PLAIN) {
            dq = live ? a.logp[i] - a.q_logp[i] : 0.f;
            r = __expf(dq);
        }
        if constexpr (FORM == IS) w = a.level == 0 ? (r > cap ? cap : r) : w_row;
        if constexpr (FORM == CLIP) {
            s = fminf(r * A, fminf(fmaxf(r, lo), hi) * A);   // the products sit behind a min / a select, where nothing contracts them into the sums that follow
            w = a.w_in ? a.w_in[i] : 1.f;
        }
        const float t = -(gated<SEL>(a.sel, i, s) - beta * kl);
        // the product by w stays outside the finished unweighted value, and PLAIN has none (not 1.f * t), so that nothing of that value is contracted differently
        if constexpr (FORM == PLAIN) sl += m * t;
        else sl += m * (w * t);
        sk += m * kl;
        if constexpr (FORM == IS) {
            if (live) {
                sw += w;
                nclip += (a.level == 0 ? r : ratio_row) > cap ? 1.f : 0.f;
                sabs += fabsf(dq);
                mabs = fmaxf(mabs, fabsf(dq));
                sk3 += r - dq - 1.f;
            }
        }
        if constexpr (FORM == CLIP) {
            if (live) {
                nlo += (r < lo && A < 0.f) ? 1.f : 0.f;
                nhi += (r > hi && A > 0.f) ? 1.f : 0.f;
                sr += r;
                mabs = fmaxf(mabs, fabsf(dq));
            }
        }
    }
    if constexpr (FORM != IS) cnt = block_sum<256>(cnt, scratch);
    sl = block_sum<256>(sl, scratch);
    sk = block_sum<256>(sk, scratch);
    if constexpr (FORM == IS) {
        sw = block_sum<256>(sw, scratch);
        nclip = block_sum<256>(nclip, scratch);
        sabs = block_sum<256>(sabs, scratch);
        mabs = block_max<256>(mabs, scratch);
        sk3 = block_sum<256>(sk3, scratch);
    }
    if constexpr (FORM == CLIP) {
        nlo = block_sum<256>(nlo, scratch);
        nhi = block_sum<256>(nhi, scratch);
        sr = block_sum<256>(sr, scratch);
        mabs = block_max<256>(mabs, scratch);
    }
    const float inv = inv_or_zero(cnt);
    const float scale = a.row_scale > 0.f ? a.row_scale : inv;
    if (threadIdx.x == 0) {
        a.row_loss[n] = sl * scale;
        a.row_kl[n] = sk * inv;
        if constexpr (FORM == IS) {
            float* st = a.row_stats + (long long)n * 5;
            st[0] = sw; st[1] = nclip; st[2] = sabs; st[3] = mabs; st[4] = sk3;
        }
        if constexpr (FORM == CLIP) {
            float* st = a.row_stats + (long long)n * 4;
            st[0] = nlo; st[1] = nhi; st[2] = sr; st[3] = mabs;
        }
    }
    for (int c = threadIdx.x; c < C; c += 256) {
        const int i = n * C + c;
        const float d = ref_gap<REF>(a.ref_logp, a.logp, i);
        const int live = a.mask[i] != 0;
        float r = 1.f, ga = A, w = 1.f;
        if constexpr (FORM != PLAIN) r = __expf(live ? a.logp[i] - a.q_logp[i] : 0.f);
        if constexpr (FORM == IS) w = a.level == 0 ? (r > cap ? cap : r) : w_row;
        if constexpr (FORM == CLIP) {
            const bool clipped = (r < lo && A < 0.f) || (r > hi && A > 0.f);
            ga = clipped ? 0.f : r * A;      // d/dp min(r A, rc A) = r A where the unclamped branch is the min, 0 where the clamped one is
            w = a.w_in ? a.w_in[i] : 1.f;
        }
        ga = gated<SEL>(a.sel, i, ga);
        // d/dp [ -(exp(p - sg p) A - beta (exp(ref - p) - (ref - p) - 1)) ] = -A + beta (1 - exp(ref - p)), with the form's ga for A.  Contraction is off: the
        // value is a rounded product and a subtraction, and a select in front of ga would otherwise let it become an fma, one rounding fewer
        float g;
        {
#pragma clang fp contract(off)
            const float bk = beta * (1.f - __expf(d));
            g = (float)a.mask[i] * scale * a.inv_nrows * (bk - ga);
        }
        if constexpr (FORM == PLAIN) a.dlogp[i] = g;
        else a.dlogp[i] = w * g;        // as in the sums: the weight outside the finished unweighted value
        if constexpr (FORM == IS) {
            if (a.w_out) a.w_out[i] = live ? w : 0.f;
        }
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
// The one host function behind the five entry points: validates, fills GrpoLossArgs, picks the instantiation and launches.  `name` is the entry point's, the
// prefix of its refusals.  `form` is the form that entry point demands (PLAIN, IS, CLIP: iadr1_grpo_loss, _is, _clip, which refuse a NULL in the input their form
// reads) or DEDUCE (iadr1_grpo_loss_ex, _sel): old_logp -> CLIP, rollout_logp -> IS, neither -> PLAIN.  REF follows from ref_logp (NULL needs beta == 0) and SEL
// from sel, for every entry point.
namespace {
enum { DEDUCE = -1 };
using GrpoLossKernel = void (*)(GrpoLossArgs);
const GrpoLossKernel grpo_loss_kernels[3][2][2] = {    // [form][REF][SEL]
    {{grpo_loss_kernel<PLAIN, false, false>, grpo_loss_kernel<PLAIN, false, true>}, {grpo_loss_kernel<PLAIN, true, false>, grpo_loss_kernel<PLAIN, true, true>}},
    {{grpo_loss_kernel<IS, false, false>, grpo_loss_kernel<IS, false, true>}, {grpo_loss_kernel<IS, true, false>, grpo_loss_kernel<IS, true, true>}},
    {{grpo_loss_kernel<CLIP, false, false>, grpo_loss_kernel<CLIP, false, true>}, {grpo_loss_kernel<CLIP, true, false>, grpo_loss_kernel<CLIP, true, true>}},
};

int grpo_loss_launch(const char* name, int form, const float* logp, const float* ref_logp, const float* old_logp, const float* rollout_logp, const float* w,
                     const float* adv, const int* mask, float beta, float cap, int level, float eps_low, float eps_high, float row_scale, int n_total_rows, float* dlogp,
                     float* kl, float* row_loss, float* row_kl, float* w_out, float* row_stats, int N, int C, const int* sel, hipStream_t stream) {
    IADR1_REQUIRE(N > 0, "%s: N must be > 0 (got %d)", name, N);
    IADR1_REQUIRE(C > 0, "%s: C must be > 0 (got %d)", name, C);
    IADR1_REQUIRE(n_total_rows >= N, "%s: n_total_rows (%d) is smaller than N (%d): it is the row count of the whole step", name, n_total_rows, N);
    IADR1_REQUIRE(ref_logp != nullptr || beta == 0.f, "%s: ref_logp is null with beta = %g: the KL term needs the reference's log-probs (only beta == 0 runs without them)", name, (double)beta);
    IADR1_REQUIRE(row_scale >= 0.f && row_scale <= 3.402823466e38f /* false for NaN and +inf */, "%s: row_scale must be 0 (1 / live tokens of the row) or finite and > 0 (got %g)", name, (double)row_scale);
    IADR1_REQUIRE(form != CLIP || old_logp != nullptr, "%s: old_logp is null (the ratio needs the log-probs of the policy that sampled)", name);
    IADR1_REQUIRE(form != IS || rollout_logp != nullptr, "%s: rollout_logp is null (the weight needs the rollout's log-probs)", name);
    IADR1_REQUIRE(old_logp == nullptr || rollout_logp == nullptr, "%s: old_logp and rollout_logp are both given: a reuse step takes the cached weights as w, not the rollout's log-probs", name);
    IADR1_REQUIRE(w == nullptr || old_logp != nullptr, "%s: w is given without old_logp (the weights belong to the clipped form)", name);
    if (form == DEDUCE) form = old_logp != nullptr ? CLIP : rollout_logp != nullptr ? IS : PLAIN;
    IADR1_REQUIRE(row_stats != nullptr || form == PLAIN, "%s: row_stats is null (the %s form writes [N, %d] partials)", name, form == CLIP ? "clip" : "IS", form == CLIP ? 4 : 5);
    if (form == CLIP) {
        IADR1_REQUIRE(eps_low >= 0.f && eps_low < 1.f /* false for NaN */, "%s: eps_low must be in [0, 1) (got %g)", name, (double)eps_low);
        IADR1_REQUIRE(eps_high >= 0.f && eps_high <= 3.402823466e38f /* false for NaN and +inf */, "%s: eps_high must be finite and >= 0 (got %g)", name, (double)eps_high);
    } else if (form == IS) {
        IADR1_REQUIRE(cap >= 1.f && cap <= 3.402823466e38f /* false for NaN and +inf */, "%s: cap must be finite and >= 1 (got %g): a smaller cap would down-weight on-policy tokens", name, (double)cap);
        IADR1_REQUIRE(level == 0 || level == 1, "%s: unknown level %d (0 = token, 1 = sequence)", name, level);
    }
    GrpoLossArgs a;
    a.logp = logp; a.ref_logp = ref_logp; a.q_logp = form == CLIP ? old_logp : rollout_logp; a.adv = adv; a.w_in = w;
    a.mask = mask; a.sel = sel;
    a.beta = beta; a.cap = cap; a.lo = 1.f - eps_low; a.hi = 1.f + eps_high; a.inv_nrows = 1.f / (float)n_total_rows; a.row_scale = row_scale;
    a.level = level;
    a.dlogp = dlogp; a.kl_out = kl; a.row_loss = row_loss; a.row_kl = row_kl; a.w_out = w_out; a.row_stats = row_stats;
    a.C = C;
    hipLaunchKernelGGL(grpo_loss_kernels[form][ref_logp != nullptr][sel != nullptr], dim3(N), dim3(256), 0, stream, a);
    return iadr1_check_launch(name);
}
}  // namespace
extern "C" int iadr1_grpo_loss(const float* logp, const float* ref_logp, const float* adv, const int* mask, float beta, int n_total_rows,
                               float* dlogp, float* kl, float* row_loss, float* row_kl, int N, int C, hipStream_t stream) {
    return grpo_loss_launch("grpo_loss", PLAIN, logp, ref_logp, nullptr, nullptr, nullptr, adv, mask, beta, 0.f, 0, 0.f, 0.f, 0.f, n_total_rows, dlogp, kl, row_loss, row_kl, nullptr,
                            nullptr, N, C, nullptr, stream);
}
extern "C" int iadr1_grpo_loss_is(const float* logp, const float* ref_logp, const float* rollout_logp, const float* adv, const int* mask, float beta,
                                  float cap, int level, int n_total_rows, float* dlogp, float* kl, float* row_loss, float* row_kl, float* w_out,
                                  float* row_stats, int N, int C, hipStream_t stream) {
    return grpo_loss_launch("grpo_loss_is", IS, logp, ref_logp, nullptr, rollout_logp, nullptr, adv, mask, beta, cap, level, 0.f, 0.f, 0.f, n_total_rows, dlogp, kl, row_loss, row_kl,
                            w_out, row_stats, N, C, nullptr, stream);
}
extern "C" int iadr1_grpo_loss_clip(const float* logp, const float* old_logp, const float* ref_logp, const float* adv, const int* mask, const float* w,
                                    float beta, float eps_low, float eps_high, int n_total_rows, float* dlogp, float* kl, float* row_loss, float* row_kl,
                                    float* row_stats, int N, int C, hipStream_t stream) {
    return grpo_loss_launch("grpo_loss_clip", CLIP, logp, ref_logp, old_logp, nullptr, w, adv, mask, beta, 0.f, 0, eps_low, eps_high, 0.f, n_total_rows, dlogp, kl, row_loss, row_kl,
                            nullptr, row_stats, N, C, nullptr, stream);
}
extern "C" int iadr1_grpo_loss_ex(const float* logp, const float* ref_logp, const float* old_logp, const float* rollout_logp, const float* w, const float* adv,
                                  const int* mask, float beta, float cap, int level, float eps_low, float eps_high, float row_scale, int n_total_rows, float* dlogp,
                                  float* kl, float* row_loss, float* row_kl, float* w_out, float* row_stats, int N, int C, hipStream_t stream) {
    return grpo_loss_launch("grpo_loss_ex", DEDUCE, logp, ref_logp, old_logp, rollout_logp, w, adv, mask, beta, cap, level, eps_low, eps_high, row_scale, n_total_rows, dlogp, kl,
                            row_loss, row_kl, w_out, row_stats, N, C, nullptr, stream);
}
extern "C" int iadr1_grpo_loss_sel(const float* logp, const float* ref_logp, const float* old_logp, const float* rollout_logp, const float* w, const float* adv,
                                   const int* mask, float beta, float cap, int level, float eps_low, float eps_high, float row_scale, int n_total_rows, float* dlogp,
                                   float* kl, float* row_loss, float* row_kl, float* w_out, float* row_stats, int N, int C, const int* sel, hipStream_t stream) {
    return grpo_loss_launch("grpo_loss_sel", DEDUCE, logp, ref_logp, old_logp, rollout_logp, w, adv, mask, beta, cap, level, eps_low, eps_high, row_scale, n_total_rows, dlogp, kl,
                            row_loss, row_kl, w_out, row_stats, N, C, sel, stream);
}
