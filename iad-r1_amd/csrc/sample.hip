// Fused sampler for the group rollout (gfx950): temperature -> top-k -> top-p -> multinomial over fp32
// logits [B, V].  Same filter semantics as the sampler the reference drives (vLLM SamplingParams(temperature,
// top_p=0.9, top_k=50), its train/stage_rl/trainer/sc_grpo_trainer.py:353-358): top-p is evaluated on the
// top-k-renormalised distribution and always keeps the most likely token.  Randomness is a counter-based
// Philox4x32-10 stream keyed by (seed; row, step), so token ids are reproducible run-to-run and checkable on the
// CPU.  temperature == 0 selects greedy argmax (lowest index wins ties), the mode used for bit-exact parity
// against the oracle.
//
// HBM/L2-bound selection problem, two launches so that a 64-row batch still fills the chip:
//   stage 1: grid (NCHUNK, B): each block reads its slice of the row ONCE into registers and extracts its local
//            top-K with an exact radix select (11+11+10 bits, LDS histograms) + index-ordered compaction;
//   stage 2: grid (B): the NCHUNK*K survivors -> exact global top-K (same routine) -> rank sort -> softmax,
//            top-p cut, inverse-CDF draw.
//
// ONE body per stage, stage1<LP, EX, GD, EN> and stage2<LP, EX, GD, EN>, behind all six entry points; a flag that is off compiles its code out:
//   LP  the log-prob of the pick + whole-vocabulary sampling for top_k <= 0     iadr1_sample_topk_topp: sample_stage1/2 <0, 0, 0>; iadr1_sample_logp: sample_logp_stage1/2 <1, 0, 0>
//   EX  a repetition penalty in front of the filter and a min_p cut behind it   iadr1_sample_ex: sample_ex_stage1/2 <1, 1, 0>
//   GD  a per-row automaton's mask in front of everything the filter does       iadr1_sample_guided: sample_guided_stage1/2 <1, 1, 1>; without a guide sample_ex's pair
//   EN  the entropy of the raw row's softmax beside the log-prob of the pick     iadr1_sample_ent: sample_ent_stage1/2 <1, 1, 0, 1>, with a guide sample_ent_guided_stage1/2 <1, 1, 1, 1>; without ent_out sample_guided's launch
// iadr1_sample_ent_t is iadr1_sample_ent's launch with LogpArgs.inv_tl = 1 / logp_temperature: the log-prob and the entropy at that temperature, no flag of its own.
// The ids of two entry points are bit-equal wherever the newer one's additions are neutral, because they are this code.  The host side is one function too.
#include <string.h>

#include "common.h"

namespace {

constexpr int NT = 256, MAXK = 64, NCHUNK = 32, ITEMS = 20;  // V <= NCHUNK*NT*ITEMS = 163840

__device__ __forceinline__ uint32_t okey(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // order-preserving map float -> uint
}

__device__ __forceinline__ float philox_uniform(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1) {
    uint32_t c[4] = {c0, c1, 0u, 0u};
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return (float)(c[0] >> 8) * (1.0f / 16777216.0f);
}

// exclusive block scan of one int per thread (NT=256); returns offset, total in *total
__device__ __forceinline__ int block_exscan(int v, int* sh, int* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, WAVE);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) sh[wv] = inc;
    __syncthreads();
    int base = 0;
    for (int i = 0; i < wv; ++i) base += sh[i];
    *total = sh[0] + sh[1] + sh[2] + sh[3];
    return base + inc - v;
}

// Exact top-K of the block's register-resident items (thread t owns the CONTIGUOUS items [t*NI, (t+1)*NI), so
// that index order == (thread, item) order).  Survivors are written in index order to oval/oidx[0..n).
// Ties at the K-th value are resolved towards the lowest index.  Returns n (<= K).
template <int NI>
__device__ __forceinline__ int block_topk(const float (&val)[NI], const int (&idx)[NI], int K, int* hist, int* sh_i, float* oval, int* oidx) {
    const int t = threadIdx.x;
    uint32_t prefix = 0, pmask = 0;
    int need = K;
    const int shifts[3] = {21, 10, 0}, widths[3] = {11, 11, 10};
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
        const int nb = 1 << widths[pass];
        for (int i = t; i < nb; i += NT) hist[i] = 0;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (idx[i] >= 0) {
                const uint32_t k = okey(val[i]);
                if ((k & pmask) == prefix) atomicAdd(&hist[(k >> shifts[pass]) & (nb - 1)], 1);
            }
        }
        __syncthreads();
        if (t < 64) {
            // one wave scans the histogram from the top: lane owns nb/64 consecutive bins (descending order)
            const int per = nb / 64;
            const int hi_bin = nb - 1 - t * per;
            int s = 0;
            for (int b = 0; b < per; ++b) s += hist[hi_bin - b];
            int inc = s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int u = __shfl_up(inc, o, WAVE);
                if (t >= o) inc += u;
            }
            const int before = inc - s;  // elements in bins above this lane's range
            const unsigned long long hit = __ballot(inc >= need);
            const int first = hit ? (int)__builtin_ctzll(hit) : 63;
            if (t == first) {
                int acc = before, b = hi_bin;
                for (int j = 0; j < per; ++j, --b) {
                    if (acc + hist[b] >= need || (b == 0)) break;
                    acc += hist[b];
                }
                if (b < 0) b = 0;
                sh_i[4] = b;
                sh_i[5] = need - acc;
            }
        }
        __syncthreads();
        prefix |= ((uint32_t)sh_i[4]) << shifts[pass];
        pmask |= ((uint32_t)(nb - 1)) << shifts[pass];
        need = sh_i[5];
        __syncthreads();
    }
    const uint32_t tau = prefix;
    int ngt = 0, neq = 0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        if (idx[i] >= 0) {
            const uint32_t k = okey(val[i]);
            ngt += k > tau;
            neq += k == tau;
        }
    }
    int tot_gt, tot_eq;
    int off_gt = block_exscan(ngt, sh_i, &tot_gt);
    int off_eq = block_exscan(neq, sh_i, &tot_eq);
    const int take_eq = min(need, tot_eq);
    // merge ">" and the first `need` "==" in index order: an element's output slot is
    //   (# of '>' before it) + (# of taken '==' before it)
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        if (idx[i] >= 0) {
            const uint32_t k = okey(val[i]);
            if (k > tau) {
                const int slot = off_gt + min(off_eq, take_eq);
                oval[slot] = val[i]; oidx[slot] = idx[i];
                ++off_gt;
            } else if (k == tau) {
                if (off_eq < take_eq) {
                    const int slot = off_gt + off_eq;
                    oval[slot] = val[i]; oidx[slot] = idx[i];
                }
                ++off_eq;
            }
        }
    }
    __syncthreads();
    return tot_gt + take_eq;
}

struct SampleArgs {
    const float* logits;
    long long ld;
    long long* out;     // [B] sampled token ids
    float* cand_val;    // scratch [B][NCHUNK][MAXK]
    int* cand_idx;      // scratch [B][NCHUNK][MAXK]
    int B, V;
    float temperature, top_p;
    int top_k;
    int suppress;       // token id forced to -inf (e.g. EOS for fixed-length benchmarking), -1 = none
    uint32_t seed_lo, seed_hi, step;
    const unsigned* step_ptr;  // optional device-resident step counter (hipGraph replays freeze kernel arguments)
    const unsigned long long* seed_ptr;  // optional device-resident seed, same reason: a new seed per rollout must not force a re-capture
};

__device__ __forceinline__ int eff_k(const SampleArgs& p) {
    if (p.temperature <= 0.f) return 1;  // greedy == top-1 with lowest-index tie break
    return min(min(p.top_k > 0 ? p.top_k : MAXK, MAXK), p.V);
}

// The row is cut into NCHUNK chunks of csize ids; inside a chunk thread t owns the CONTIGUOUS ids g0 + i, i < per <= ITEMS, so that id order == (thread, item)
// order.  Stage 1 loads its slice by this; the whole-vocabulary draw of stage 2 reads slices again by the same assignment.
struct Slice {
    int g0, per, c1;
    __device__ __forceinline__ bool has(int i) const { return i < per && g0 + i < c1; }
};
struct Slices {
    int V, csize, per;
    __device__ __forceinline__ explicit Slices(int V_) : V(V_), csize((V_ + NCHUNK - 1) / NCHUNK), per((csize + NT - 1) / NT) {}
    __device__ __forceinline__ Slice of(int chunk) const {
        const int c0 = chunk * csize, c1 = min(V, c0 + csize);
        return Slice{c0 + (int)threadIdx.x * per, per, c1};
    }
};

// The uniform of (seed; row, step).  The step is the Philox counter and, with LP, the log-prob column.
__device__ __forceinline__ uint32_t read_step(const SampleArgs& p) { return p.step_ptr ? *p.step_ptr : p.step; }
__device__ __forceinline__ float draw_uniform(const SampleArgs& p, int row, uint32_t step) {
    const unsigned long long sd = p.seed_ptr ? *p.seed_ptr : (((unsigned long long)p.seed_hi << 32) | p.seed_lo);
    return philox_uniform((uint32_t)sd, (uint32_t)(sd >> 32), (uint32_t)row, step);
}

// The single-thread tail of stage 2: softmax over the n rank-sorted candidates in sval (weights left in w), top-p cut, inverse-CDF draw.  Returns the RANK of
// the pick.  It reads the step for itself, in thread 0, where the plain pair has always read it.  min_p (EX; 0 otherwise, where the compare folds away): a further
// cut of the same rank-ordered prefix -- w[0] is 1, so "w[j] >= min_p" is transformers' MinPLogitsWarper relative to the most likely token; the shorter prefix wins.
__device__ __forceinline__ int topk_topp_pick(const SampleArgs& p, int row, const float* sval, float* w, int n, float min_p) {
    const float invT = 1.f / p.temperature;
    const float mx = sval[0] * invT;
    float tot = 0.f;
    for (int j = 0; j < n; ++j) { const float e = __expf(sval[j] * invT - mx); w[j] = e; tot += e; }
    // top-p on the top-k-renormalised distribution: keep j while the mass ranked before it is < top_p
    float before = 0.f, kept = 0.f;
    int nk = 0;
    for (int j = 0; j < n; ++j) {
        if (j > 0 && (before >= p.top_p * tot || (min_p > 0.f && w[j] < min_p))) break;
        kept += w[j];
        before += w[j];
        ++nk;
    }
    const float u = draw_uniform(p, row, read_step(p)) * kept;
    float cum = 0.f;
    int pick = nk - 1;
    for (int j = 0; j < nk; ++j) {
        cum += w[j];
        if (cum > u) { pick = j; break; }
    }
    return pick;
}

// ---- LP: whole-vocabulary sampling (top_k <= 0) + the log-prob of the pick ----------------------------------------------------------------------
// Both need the softmax normaliser of the WHOLE row.  Stage 1 holds its slice in registers anyway: it also reduces it to
//   (m1, s1) = (max x, sum exp((x - m1) * inv_tl))      nothing filtered or suppressed: what the loss scores (inv_tl = 1: iadr1_logprob_rows; iadr1_sample_ent_t: 1 / T)
//   (mT, sT) = (max x, sum exp((x - mT) / T))           suppressed token excluded; only for top_k <= 0
// four floats per (row, chunk) behind the candidate lists.  Stage 2 merges the NCHUNK partials with one wave (fixed shuffle trees, no atomics on floats).
// Whole vocabulary: an inclusive scan of the chunk masses in chunk order finds the chunk that holds u * total, that ONE slice is read again and an
// exclusive block scan of the per-thread sums (thread t owns contiguous ids, as in stage 1) finds the id.  Summation tree of a weight, all fixed:
// <= ITEMS serial adds in the thread, 6 shuffle levels in the wave, 3 adds over the waves (stage 1: the chunk mass; stage 2 again: the position in
// the chunk), 6 shuffle levels over the chunks: at most 2 * (20 + 6 + 3) + 6 = 64 fp32 additions deep.
// top_k <= 0 means "MAXK candidates" without LP (eff_k) and the whole vocabulary with it: every use of whole_vocab() sits behind `if constexpr (LP)`.
struct LogpArgs {
    float* part;        // scratch [B][NCHUNK][4]: m1, s1, mT, sT
    float* logp;        // optional [B, ld] log-probs, column = the step value
    long long ld;
    int cols;
    float inv_tl;       // 1 / the temperature the log-prob (and EN's entropy) is taken at: softmax(x * inv_tl).  1 everywhere but iadr1_sample_ent_t
};

__device__ __forceinline__ bool whole_vocab(const SampleArgs& p) { return p.top_k <= 0 && p.temperature > 0.f; }

// ---- EX: a repetition penalty in front of the filter and a min_p cut behind it -------------------------------------------------------------------------
// The filter sees x' (transformers' RepetitionPenaltyLogitsProcessor over the ids whose bit is set in `seen`), the log-prob keeps seeing the raw x.
// Whole vocabulary with min_p > 0: whether a token is kept depends on the maximum of the WHOLE row, which stage 1 does not have, so stage 2 forms the
// thresholded chunk masses itself (the block reads the row once more, chunk by chunk, with stage 1's thread -> id assignment and a tree no deeper than
// stage 1's); stage 1 contributes the maxima and (m1, s1).
struct ExArgs {
    float min_p, pen;
    unsigned* seen;     // [B, ld_seen] bitmap, bit id & 31 of word id >> 5
    long long ld_seen;
    int mark;
};

// one IEEE multiply or one IEEE divide; the empty asm keeps -ffp-contract from fusing the product into the subtraction that follows it
__device__ __forceinline__ float penalised(float x, float pen) {
    float r = x < 0.f ? x * pen : x / pen;
    asm volatile("" : "+v"(r));
    return r;
}
__device__ __forceinline__ bool seen_bit(const unsigned* srow, int g) { return (srow[g >> 5] >> (g & 31)) & 1u; }
__device__ __forceinline__ void mark_pick(const ExArgs& e, int row, int pick) {     // one thread per row: a plain read-modify-write
    if (e.mark) e.seen[(long long)row * e.ld_seen + (pick >> 5)] |= 1u << (pick & 31);
}

// ---- GD: a per-row automaton in front of everything the filter does -----------------------------------------------------------------------------------------------
// Row b is in state[b]; the filter sees -inf wherever bit id of allow[state[b]] is clear (before the penalty: -inf stays -inf through it and through the
// temperature), the log-prob keeps seeing the raw x.  The state is read once, at entry, into a register in both stages; stage 2's thread 0 moves it along trans
// after the pick.
struct GuideArgs {
    int* state;             // [B], 0 <= state[b] < S
    const unsigned* allow;  // [S, ld_allow] bitmap, bit id & 31 of word id >> 5 (the layout of `seen`)
    const short* trans;     // [S, ld_trans]: the state behind (s, id), -1 where id is not allowed
    long long ld_allow, ld_trans;
    int S;
};
// (the clamp costs two instructions and keeps the allow row inside its table whatever the caller left in state[])
__device__ __forceinline__ int guide_state(const GuideArgs& g, int row) { return min(max(g.state[row], 0), g.S - 1); }
__device__ __forceinline__ void guide_advance(const GuideArgs& g, int row, int st, int pick) {    // one thread per row: a plain load and a plain store
    const int n = pick >= 0 ? (int)g.trans[(long long)st * g.ld_trans + pick] : -1;
    g.state[row] = (n >= 0 && n < g.S) ? n : st;   // a fallback pick (every allowed logit -inf) may be a disallowed id: the state then stays where it is, in range
}

// ---- EN: the entropy of the distribution the log-prob is taken under ---------------------------------------------------------------------------------------------------
// H = -sum p ln p with p = softmax(x * inv_tl) over the RAW row (inv_tl = 1 but for iadr1_sample_ent_t): nothing suppressed, masked, penalised or filtered -- (m1, s1)'s
// distribution.  Stage 1 adds
//   u1 = sum e_i d_i,  d_i = (x_i - m1) * inv_tl,  e_i = exp(d_i)       (x_i = -inf skipped: 0 * -inf; every term <= 0)
// as a fifth partial per (row, chunk), BEHIND the [B][NCHUNK][4] block.  Stage 2, with d_c = (m1_c - M1) * inv_tl and a_c = exp(d_c) (0 for an all--inf chunk):
//   S = sum s1_c a_c,   U = sum (u1_c + d_c s1_c) a_c,   H = ln S - U / S
// ln S >= 0 (the chunk that holds M1 has s1 >= 1) and U <= 0: two non-negative numbers, no cancellation.  Fixed trees, no float atomics.
struct EntArgs {
    float* part;        // scratch [B][NCHUNK]: u1
    float* ent;         // [B, ld] entropies, column = the step value (logp's rule)
    long long ld;
    int cols;
};

// inclusive scan over the lanes of a wave
__device__ __forceinline__ float wave_incscan(float v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(v, o, WAVE);
        if (lane >= o) v += t;
    }
    return v;
}

template <bool LP, bool EX, bool GD, bool EN = false>     // EX, GD and EN build on LP: the six combinations of the header are the ones that exist
__device__ __forceinline__ void stage1(const SampleArgs& p, const LogpArgs& q, const ExArgs& e, const GuideArgs& gd, const EntArgs& en = EntArgs{}) {
    __shared__ int hist[2048];
    __shared__ int sh_i[8];
    __shared__ float sh_f[16];
    __shared__ float oval[MAXK];
    __shared__ int oidx[MAXK];
    const int row = blockIdx.y, chunk = blockIdx.x, t = threadIdx.x;
    float val[ITEMS];
    int idx[ITEMS];
    const float* x = p.logits + (long long)row * p.ld;
    const Slice sl = Slices(p.V).of(chunk);
    float xs = -INFINITY;   // the suppressed token's own logit, if this thread holds it: it counts at temperature 1
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const int g = sl.g0 + i;
        const bool ok = sl.has(i);
        idx[i] = ok ? g : -1;
        const float v = ok ? x[g] : -INFINITY;
        const bool sup = ok && g == p.suppress;
        if (sup) xs = v;
        val[i] = sup ? -INFINITY : v;
    }
    if constexpr (LP) {
        const bool wv = whole_vocab(p);
        float mT = -INFINITY;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) mT = fmaxf(mT, val[i]);
        const float m1 = block_max<NT>(fmaxf(mT, xs), sh_f);
        float s1 = 0.f, sT = 0.f;
        if (m1 > -INFINITY) {
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) s1 += expf((val[i] - m1) * q.inv_tl);      // (padding and the suppressed slot hold -inf: they add 0)
            if (xs > -INFINITY) s1 += expf((xs - m1) * q.inv_tl);
        }
        float u1 = 0.f;
        if constexpr (EN) {
            // val still holds the raw slice (the suppressed slot apart: xs carries that one)
            if (m1 > -INFINITY) {
#pragma unroll
                for (int i = 0; i < ITEMS; ++i) {
                    const float d = (val[i] - m1) * q.inv_tl;
                    if (val[i] > -INFINITY) u1 += expf(d) * d;
                }
                if (xs > -INFINITY) { const float d = (xs - m1) * q.inv_tl; u1 += expf(d) * d; }
            }
        }
        if constexpr (GD) {
            // (m1, s1) above are the raw row's; the automaton's mask comes first of all the filter does
            const unsigned* arow = gd.allow + (long long)guide_state(gd, row) * gd.ld_allow;
            mT = -INFINITY;
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                if (idx[i] >= 0 && !seen_bit(arow, idx[i])) val[i] = -INFINITY;
                mT = fmaxf(mT, val[i]);
            }
        }
        if constexpr (EX) {
            // (m1, s1) above are the raw row's; from here on val holds x' (-inf stays -inf: the suppressed slot and the padding need no test)
            if (e.pen != 1.f) {
                const unsigned* srow = e.seen + (long long)row * e.ld_seen;
                mT = -INFINITY;
#pragma unroll
                for (int i = 0; i < ITEMS; ++i) {
                    if (idx[i] >= 0 && seen_bit(srow, idx[i])) val[i] = penalised(val[i], e.pen);
                    mT = fmaxf(mT, val[i]);
                }
            }
        }
        mT = block_max<NT>(mT, sh_f + 4);
        const float invT = wv ? 1.f / p.temperature : 0.f;
        if (wv && mT > -INFINITY) {
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) sT += expf((val[i] - mT) * invT);
        }
        s1 = block_sum<NT>(s1, sh_f + 8);
        sT = block_sum<NT>(sT, sh_f + 12);
        if constexpr (EN) {
            __shared__ float sh_u[4];       // (sh_f is used up by the four reductions above)
            u1 = block_sum<NT>(u1, sh_u);
        }
        if (t == 0) {
            float* o = q.part + ((long long)row * NCHUNK + chunk) * 4;
            o[0] = m1; o[1] = s1; o[2] = mT; o[3] = sT;
            if constexpr (EN) en.part[(long long)row * NCHUNK + chunk] = u1;
        }
        if (wv) return;     // no candidate lists: stage 2 draws from the chunk masses
    }
    const int n = block_topk<ITEMS>(val, idx, eff_k(p), hist, sh_i, oval, oidx);
    float* cv = p.cand_val + ((long long)row * NCHUNK + chunk) * MAXK;
    int* ci = p.cand_idx + ((long long)row * NCHUNK + chunk) * MAXK;
    if (t < MAXK) {
        cv[t] = t < n ? oval[t] : -INFINITY;
        ci[t] = t < n ? oidx[t] : -1;
    }
}

template <bool LP, bool EX, bool GD, bool EN = false>
__device__ __forceinline__ void commit_pick(const SampleArgs& p, const ExArgs& e, const GuideArgs& gd, int row, int st, int pick, float* lp, const float* raw, float lse,
                                            float inv_tl, float* hp = nullptr, float H = 0.f) {
    p.out[row] = pick;
    if constexpr (LP) { if (lp) *lp = *raw * inv_tl - lse; }
    if constexpr (EN) { if (hp) *hp = H; }
    if constexpr (EX) mark_pick(e, row, pick);
    if constexpr (GD) guide_advance(gd, row, st, pick);
}

template <bool LP, bool EX, bool GD, bool EN = false>
__device__ __forceinline__ void stage2(const SampleArgs& p, const LogpArgs& q, const ExArgs& e, const GuideArgs& gd, const EntArgs& en = EntArgs{}) {
    __shared__ int hist[2048];
    __shared__ int sh_i[8];
    __shared__ float sh_f[8];
    __shared__ float cval[MAXK];
    __shared__ int cidx[MAXK];
    __shared__ float sval[MAXK];
    __shared__ int sidx[MAXK];
    __shared__ float sraw[MAXK];
    constexpr int NI = NCHUNK * MAXK / NT;  // 8 candidates per thread
    const int row = blockIdx.x, t = threadIdx.x, lane = t & 63;
    const float* x = p.logits + (long long)row * p.ld;     // read with LP only: the log-prob's raw logit and the whole-vocabulary draw
    const uint32_t step = read_step(p);     // read once, at entry: the Philox counter of the whole-vocabulary draw and the log-prob column
    float* lp = (LP && q.logp != nullptr && step < (uint32_t)q.cols) ? q.logp + (long long)row * q.ld + step : nullptr;
    float lse = 0.f;    // the raw row's log-sum-exp at the log-prob temperature, 1 / q.inv_tl (LP)
    float* hp = nullptr;    // where the row's entropy goes (EN): logp's column rule
    float H = 0.f;
    if constexpr (EN) { if (en.ent != nullptr && step < (uint32_t)en.cols) hp = en.ent + (long long)row * en.ld + step; }
    int st = 0;                         // the row's automaton state, read once: thread 0 overwrites it behind the __syncthreads() that precede every pick
    const unsigned* arow = nullptr;
    if constexpr (GD) {
        st = guide_state(gd, row);
        arow = gd.allow + (long long)st * gd.ld_allow;
    }
    if constexpr (LP) {
        // every wave merges the NCHUNK partials for itself (lane = chunk; the same instructions on the same data: the same bits in all four waves)
        const bool have = lane < NCHUNK;
        const float* pr = q.part + ((long long)row * NCHUNK + (have ? lane : 0)) * 4;
        const float m1 = have ? pr[0] : -INFINITY, s1 = have ? pr[1] : 0.f;
        const float M1 = wave_max(m1);
        const float dm = (m1 - M1) * q.inv_tl;      // (NaN for an all--inf chunk or row: every use sits behind m1 > -inf)
        const float S = wave_sum(m1 > -INFINITY ? s1 * expf(dm) : 0.f);
        lse = M1 * q.inv_tl + logf(S);
        if constexpr (EN) {
            const float u1 = have ? en.part[(long long)row * NCHUNK + lane] : 0.f;
            const float U = wave_sum(m1 > -INFINITY ? (u1 + dm * s1) * expf(dm) : 0.f);
            H = S > 0.f ? logf(S) - U / S : 0.f;    // (S == 0: a row of -inf only has no distribution)
        }
        if (whole_vocab(p)) {
            const float invT = 1.f / p.temperature;
            const float mT = have ? pr[2] : -INFINITY, sT = have ? pr[3] : 0.f;
            const float MT = wave_max(mT);
            float mass = mT > -INFINITY ? sT * expf((mT - MT) * invT) : 0.f;
            const Slices slices(p.V);
            const unsigned* srow = nullptr;
            float min_p = 0.f;
            // what the filter leaves of token g.  The order is the contract with transformers' processors: the automaton's mask, the penalty, the temperature,
            // then the min_p cut relative to the row maximum (its weight is 1)
            auto weight = [&](int g) {
                float v = x[g];
                if constexpr (GD) { if (!seen_bit(arow, g)) v = -INFINITY; }
                if constexpr (EX) { if (srow != nullptr && seen_bit(srow, g)) v = penalised(v, e.pen); }
                const float w = expf((v - MT) * invT);
                return (!EX || w >= min_p) ? w : 0.f;
            };
            if constexpr (EX) {
                if (e.pen != 1.f) srow = e.seen + (long long)row * e.ld_seen;
                min_p = e.min_p;
                if (min_p > 0.f) {
                    // the kept set hangs on MT: the chunk masses over the tokens with exp((x' - MT) / T) >= min_p, formed here.  Per chunk: <= ITEMS serial adds in
                    // the thread, 6 shuffle levels, 3 adds over the waves -- stage 1's depth; lane c of every wave ends up with chunk c's mass, the same bits in all four.
                    __shared__ float cm[NCHUNK][NT / WAVE];
                    for (int c = 0; c < NCHUNK; ++c) {
                        const Slice sl = slices.of(c);
                        float ts = 0.f;
#pragma unroll
                        for (int i = 0; i < ITEMS; ++i) {
                            const int g = sl.g0 + i;
                            if (sl.has(i) && g != p.suppress) ts += weight(g);
                        }
                        ts = wave_sum(ts);
                        if (lane == 0) cm[c][t >> 6] = ts;
                    }
                    __syncthreads();
                    mass = have ? ((cm[lane][0] + cm[lane][1]) + cm[lane][2]) + cm[lane][3] : 0.f;
                }
            }
            const float inc = wave_incscan(mass);
            const float total = __shfl(inc, NCHUNK - 1, WAVE);
            const float target = draw_uniform(p, row, step) * total;
            // first chunk whose inclusive mass exceeds the target; rounding may leave none: then the last chunk that has any mass
            const unsigned long long hit = __ballot(have && inc > target), any = __ballot(have && mass > 0.f);
            const int chunk = hit ? (int)__builtin_ctzll(hit) : (any ? 63 - (int)__builtin_clzll(any) : 0);
            const float rest = target - (__shfl(inc, chunk, WAVE) - __shfl(mass, chunk, WAVE));     // what is left of the target inside the chunk
            const Slice sl = slices.of(chunk);
            float w[ITEMS];
            float ts = 0.f;
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                const int g = sl.g0 + i;
                w[i] = 0.f;
                if (sl.has(i) && g != p.suppress) w[i] = weight(g);     // (g < c1 <= V: the re-read stays inside the row)
                ts += w[i];
            }
            // exclusive block scan of the thread sums, in id order
            const float winc = wave_incscan(ts);
            if (t == 0) { sh_i[0] = 0x7fffffff; sh_i[1] = -1; }
            if (lane == 63) sh_f[t >> 6] = winc;
            __syncthreads();
            float cum = winc - ts;
            for (int i = 0; i < (t >> 6); ++i) cum += sh_f[i];
            int first = 0x7fffffff, last = -1;      // first id whose inclusive weight exceeds `rest`; last id of the chunk with any weight (rounding fallback)
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) {
                cum += w[i];
                if (w[i] > 0.f) {
                    const int g = sl.g0 + i;
                    last = g;
                    if (cum > rest && first == 0x7fffffff) first = g;
                }
            }
            if (first != 0x7fffffff) atomicMin(&sh_i[0], first);
            if (last >= 0) atomicMax(&sh_i[1], last);
            __syncthreads();
            if (t == 0) {
                const int pick = sh_i[0] != 0x7fffffff ? sh_i[0] : max(sh_i[1], 0);
                commit_pick<LP, EX, GD, EN>(p, e, gd, row, st, pick, lp, &x[pick], lse, q.inv_tl, hp, H);
            }
            return;
        }
    }
    const float* cv = p.cand_val + (long long)row * NCHUNK * MAXK;
    const int* ci = p.cand_idx + (long long)row * NCHUNK * MAXK;
    float val[NI];
    int idx[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        idx[i] = ci[t * NI + i];
        val[i] = cv[t * NI + i];
    }
    const int n = block_topk<NI>(val, idx, eff_k(p), hist, sh_i, cval, cidx);
    if (p.temperature <= 0.f) {
        if (t == 0) {
            const int pick = n > 0 ? cidx[0] : 0;
            commit_pick<LP, EX, GD, EN>(p, e, gd, row, st, pick, lp, &x[pick], lse, q.inv_tl, hp, H);
        }
        return;
    }
    if (t < n) {
        const float v = cval[t];
        const int id = cidx[t];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (cval[j] > v) || (cval[j] == v && cidx[j] < id);
        sval[rank] = v;
        sidx[rank] = id;
        if constexpr (LP) sraw[rank] = x[id];     // every candidate's own logit, fetched by its thread: the serial tail below reads LDS only
    }
    __syncthreads();
    if (t == 0) {
        const int pick = topk_topp_pick(p, row, sval, cval, n, EX ? e.min_p : 0.f);
        commit_pick<LP, EX, GD, EN>(p, e, gd, row, st, sidx[pick], lp, &sraw[pick], lse, q.inv_tl, hp, H);
    }
}

__global__ __launch_bounds__(NT) void sample_stage1(SampleArgs p) { stage1<false, false, false>(p, LogpArgs{}, ExArgs{}, GuideArgs{}); }
__global__ __launch_bounds__(NT) void sample_stage2(SampleArgs p) { stage2<false, false, false>(p, LogpArgs{}, ExArgs{}, GuideArgs{}); }
__global__ __launch_bounds__(NT) void sample_logp_stage1(SampleArgs p, LogpArgs q) { stage1<true, false, false>(p, q, ExArgs{}, GuideArgs{}); }
__global__ __launch_bounds__(NT) void sample_logp_stage2(SampleArgs p, LogpArgs q) { stage2<true, false, false>(p, q, ExArgs{}, GuideArgs{}); }
__global__ __launch_bounds__(NT) void sample_ex_stage1(SampleArgs p, LogpArgs q, ExArgs e) { stage1<true, true, false>(p, q, e, GuideArgs{}); }
__global__ __launch_bounds__(NT) void sample_ex_stage2(SampleArgs p, LogpArgs q, ExArgs e) { stage2<true, true, false>(p, q, e, GuideArgs{}); }
__global__ __launch_bounds__(NT) void sample_guided_stage1(SampleArgs p, LogpArgs q, ExArgs e, GuideArgs g) { stage1<true, true, true>(p, q, e, g); }
__global__ __launch_bounds__(NT) void sample_guided_stage2(SampleArgs p, LogpArgs q, ExArgs e, GuideArgs g) { stage2<true, true, true>(p, q, e, g); }
__global__ __launch_bounds__(NT) void sample_ent_stage1(SampleArgs p, LogpArgs q, ExArgs e, EntArgs n) { stage1<true, true, false, true>(p, q, e, GuideArgs{}, n); }
__global__ __launch_bounds__(NT) void sample_ent_stage2(SampleArgs p, LogpArgs q, ExArgs e, EntArgs n) { stage2<true, true, false, true>(p, q, e, GuideArgs{}, n); }
__global__ __launch_bounds__(NT) void sample_ent_guided_stage1(SampleArgs p, LogpArgs q, ExArgs e, GuideArgs g, EntArgs n) { stage1<true, true, true, true>(p, q, e, g, n); }
__global__ __launch_bounds__(NT) void sample_ent_guided_stage2(SampleArgs p, LogpArgs q, ExArgs e, GuideArgs g, EntArgs n) { stage2<true, true, true, true>(p, q, e, g, n); }

// iadr1_seen_init: one block per sequence zeroes its bitmap row, then ORs in the live tokens of its prompt (left-padded: columns [S - len, S)).
__global__ __launch_bounds__(NT) void seen_init_kernel(const long long* ids, int S, const int* lengths, int G, int V, unsigned* seen, long long ld_seen) {
    const int r = blockIdx.x, t = threadIdx.x;
    unsigned* srow = seen + (long long)r * ld_seen;
    for (long long i = t; i < ld_seen; i += NT) srow[i] = 0u;
    __syncthreads();        // (the zeroes and the ORs below are this block's own: block-level ordering is enough)
    const int b = r / G;
    const int len = max(0, min(lengths[b], S));
    const long long* prow = ids + (long long)b * S + (S - len);
    for (int j = t; j < len; j += NT) {
        const long long id = prow[j];
        if (id >= 0 && id < V) atomicOr(&srow[id >> 5], 1u << (id & 31));
    }
}

enum SamplerPair { PAIR_PLAIN, PAIR_LOGP, PAIR_EX, PAIR_GUIDED, PAIR_ENT, PAIR_ENT_GUIDED };

template <class... A>
void launch_pair(void (*s1)(A...), void (*s2)(A...), int B, hipStream_t stream, A... a) {
    hipLaunchKernelGGL(s1, dim3(NCHUNK, B), dim3(NT), 0, stream, a...);
    hipLaunchKernelGGL(s2, dim3(B), dim3(NT), 0, stream, a...);
}

// The six entry points: the checks, the workspace carve-up, the argument structs and the launch, once.  `name` is the entry point's ("sample_ex": the prefix of
// its refusals and the middle of its workspace function's name), `pair` the kernels it launches; under the defaults of what an entry point lacks its checks pass.
int sample_launch(const char* name, SamplerPair pair, hipStream_t stream, const float* logits, long long ld, long long* out, void* workspace, int B, int V, float temperature,
                  int top_k, float top_p, int suppress_token, unsigned long long seed, unsigned step, const unsigned* step_ptr, const unsigned long long* seed_ptr,
                  float* logp_out = nullptr, long long ld_logp = 0, int logp_cols = 0, float min_p = 0.f, float repetition_penalty = 1.f, unsigned* seen = nullptr,
                  long long ld_seen = 0, int mark_seen = 0, int* state = nullptr, const unsigned* allow = nullptr, long long ld_allow = 0, const short* trans = nullptr,
                  long long ld_trans = 0, int S = 0, float* ent_out = nullptr, long long ld_ent = 0, int ent_cols = 0, float logp_temperature = 1.f) {
    IADR1_REQUIRE(logp_temperature > 0.f && logp_temperature <= 3.402823466e38f, "%s: logp_temperature must be finite and > 0 (got %g)", name, (double)logp_temperature);
    IADR1_REQUIRE(ent_out == nullptr || ent_cols > 0, "%s: ent_out needs ent_cols > 0 (got %d)", name, ent_cols);
    IADR1_REQUIRE(ent_out == nullptr || ld_ent >= ent_cols, "%s: ld_ent=%lld is less than ent_cols = %d", name, ld_ent, ent_cols);
    IADR1_REQUIRE(allow == nullptr || (state != nullptr && trans != nullptr), "%s: allow needs state [B] and trans [S, ld_trans] beside it (got state %s, trans %s)", name,
                  state ? "a buffer" : "NULL", trans ? "a buffer" : "NULL");
    IADR1_REQUIRE(allow != nullptr || (state == nullptr && trans == nullptr), "%s: state and trans must be NULL when allow is NULL: without the mask there is no automaton to advance", name);
    if (allow != nullptr) {
        IADR1_REQUIRE(S >= 1 && S <= 32767, "%s: S=%d states, outside 1..32767 (trans holds int16)", name, S);
        IADR1_REQUIRE(ld_allow >= ((long long)V + 31) / 32, "%s: ld_allow=%lld is less than ceil(V / 32) = %lld", name, ld_allow, ((long long)V + 31) / 32);
        IADR1_REQUIRE(ld_trans >= (long long)V, "%s: ld_trans=%lld is less than V = %d", name, ld_trans, V);
    }
    IADR1_REQUIRE(min_p >= 0.f && min_p < 1.f, "%s: min_p must be in [0,1) (got %g)", name, (double)min_p);
    IADR1_REQUIRE(repetition_penalty > 0.f && repetition_penalty <= 3.402823466e38f, "%s: repetition_penalty must be finite and > 0 (got %g)", name, (double)repetition_penalty);
    IADR1_REQUIRE((repetition_penalty == 1.f && !mark_seen) || (seen != nullptr && ld_seen >= ((long long)V + 31) / 32),
                  "%s: repetition_penalty != 1 and mark_seen need a seen bitmap [B, ld_seen] with ld_seen >= ceil(V / 32) (got %s, ld_seen %lld, V %d)", name,
                  seen ? "a buffer" : "NULL", ld_seen, V);
    IADR1_REQUIRE(top_p > 0.f && top_p <= 1.f, "%s: top_p must be in (0,1]", name);
    // (the plain pair has no whole-vocabulary path: top_k <= 0 means MAXK candidates there, under any top_p)
    IADR1_REQUIRE(pair == PAIR_PLAIN || top_k > 0 || top_p == 1.f, "%s: top_k <= 0 samples the whole vocabulary and takes top_p = 1 only (got %g): a nucleus over all V tokens is not built", name, (double)top_p);
    IADR1_REQUIRE(B > 0 && V > 0 && workspace != nullptr, "%s: empty problem or missing workspace (iadr1_%s_workspace_bytes)", name,
                  strcmp(name, "sample_ent_t") ? name : "sample_ent");     // (iadr1_sample_ent_t takes iadr1_sample_ent's workspace)
    IADR1_REQUIRE(V <= NCHUNK * NT * ITEMS, "%s: V=%d exceeds the built maximum %d", name, V, NCHUNK * NT * ITEMS);
    IADR1_REQUIRE(top_k <= MAXK, "%s: top_k=%d exceeds the built maximum %d", name, top_k, MAXK);
    IADR1_REQUIRE(logp_out == nullptr || (logp_cols > 0 && ld_logp >= logp_cols), "%s: logp_out needs logp_cols > 0 and ld_logp >= logp_cols", name);
    float* cv = (float*)workspace;
    int* ci = (int*)(cv + (long long)B * NCHUNK * MAXK);
    float* part = (float*)(ci + (long long)B * NCHUNK * MAXK);      // (the plain pair's workspace ends here; it has no LogpArgs)
    SampleArgs p{logits, ld, out, cv, ci, B, V, temperature, top_p, top_k, suppress_token, (uint32_t)seed, (uint32_t)(seed >> 32), step, step_ptr, seed_ptr};
    LogpArgs q{part, logp_out, ld_logp, logp_cols, 1.0f / logp_temperature};
    ExArgs e{min_p, repetition_penalty, seen, ld_seen, mark_seen != 0};
    GuideArgs g{state, allow, trans, ld_allow, ld_trans, S};
    EntArgs n{part + (long long)B * NCHUNK * 4, ent_out, ld_ent, ent_cols};     // (behind the [B][NCHUNK][4] block: only iadr1_sample_ent's workspace reaches that far)
    switch (pair) {
        case PAIR_PLAIN: launch_pair(sample_stage1, sample_stage2, B, stream, p); break;
        case PAIR_LOGP: launch_pair(sample_logp_stage1, sample_logp_stage2, B, stream, p, q); break;
        case PAIR_EX: launch_pair(sample_ex_stage1, sample_ex_stage2, B, stream, p, q, e); break;
        case PAIR_GUIDED: launch_pair(sample_guided_stage1, sample_guided_stage2, B, stream, p, q, e, g); break;
        case PAIR_ENT: launch_pair(sample_ent_stage1, sample_ent_stage2, B, stream, p, q, e, n); break;
        case PAIR_ENT_GUIDED: launch_pair(sample_ent_guided_stage1, sample_ent_guided_stage2, B, stream, p, q, e, g, n); break;
    }
    return iadr1_check_launch(pair == PAIR_PLAIN ? "sample_topk_topp" : name);
}

}  // namespace

extern "C" long long iadr1_sample_workspace_bytes(int B) { return (long long)B * NCHUNK * MAXK * 8; }
extern "C" long long iadr1_sample_logp_workspace_bytes(int B) { return (long long)B * NCHUNK * (MAXK * 8 + 16); }
extern "C" long long iadr1_sample_ex_workspace_bytes(int B) { return iadr1_sample_logp_workspace_bytes(B); }
extern "C" long long iadr1_sample_guided_workspace_bytes(int B) { return iadr1_sample_ex_workspace_bytes(B); }
extern "C" long long iadr1_sample_ent_workspace_bytes(int B) { return iadr1_sample_guided_workspace_bytes(B) + (long long)B * NCHUNK * 4; }

extern "C" int iadr1_sample_topk_topp(const float* logits, long long ld, long long* out, void* workspace, int B, int V, float temperature,
                                      int top_k, float top_p, int suppress_token, unsigned long long seed, unsigned step,
                                      const unsigned* step_ptr, const unsigned long long* seed_ptr, hipStream_t stream) {
    return sample_launch("sample", PAIR_PLAIN, stream, logits, ld, out, workspace, B, V, temperature, top_k, top_p, suppress_token, seed, step, step_ptr, seed_ptr);
}

extern "C" int iadr1_sample_logp(const float* logits, long long ld, long long* out, float* logp_out, long long ld_logp, int logp_cols, void* workspace, int B,
                                 int V, float temperature, int top_k, float top_p, int suppress_token, unsigned long long seed, unsigned step,
                                 const unsigned* step_ptr, const unsigned long long* seed_ptr, hipStream_t stream) {
    return sample_launch("sample_logp", PAIR_LOGP, stream, logits, ld, out, workspace, B, V, temperature, top_k, top_p, suppress_token, seed, step, step_ptr, seed_ptr, logp_out,
                         ld_logp, logp_cols);
}

extern "C" int iadr1_sample_ex(const float* logits, long long ld, long long* out, float* logp_out, long long ld_logp, int logp_cols, void* workspace, int B,
                               int V, float temperature, int top_k, float top_p, float min_p, float repetition_penalty, unsigned* seen, long long ld_seen,
                               int mark_seen, int suppress_token, unsigned long long seed, unsigned step, const unsigned* step_ptr,
                               const unsigned long long* seed_ptr, hipStream_t stream) {
    return sample_launch("sample_ex", PAIR_EX, stream, logits, ld, out, workspace, B, V, temperature, top_k, top_p, suppress_token, seed, step, step_ptr, seed_ptr, logp_out,
                         ld_logp, logp_cols, min_p, repetition_penalty, seen, ld_seen, mark_seen);
}

extern "C" int iadr1_sample_guided(const float* logits, long long ld, long long* out, float* logp_out, long long ld_logp, int logp_cols, void* workspace, int B,
                                   int V, float temperature, int top_k, float top_p, float min_p, float repetition_penalty, unsigned* seen, long long ld_seen,
                                   int mark_seen, int suppress_token, unsigned long long seed, unsigned step, const unsigned* step_ptr,
                                   const unsigned long long* seed_ptr, int* state, const unsigned* allow, long long ld_allow, const short* trans,
                                   long long ld_trans, int S, hipStream_t stream) {
    // no guide: iadr1_sample_ex's own kernels, the same device code and the same bits
    return sample_launch("sample_guided", allow != nullptr ? PAIR_GUIDED : PAIR_EX, stream, logits, ld, out, workspace, B, V, temperature, top_k, top_p, suppress_token, seed, step,
                         step_ptr, seed_ptr, logp_out, ld_logp, logp_cols, min_p, repetition_penalty, seen, ld_seen, mark_seen, state, allow, ld_allow, trans, ld_trans, S);
}

extern "C" int iadr1_sample_ent(const float* logits, long long ld, long long* out, float* logp_out, long long ld_logp, int logp_cols, void* workspace, int B,
                                int V, float temperature, int top_k, float top_p, float min_p, float repetition_penalty, unsigned* seen, long long ld_seen,
                                int mark_seen, int suppress_token, unsigned long long seed, unsigned step, const unsigned* step_ptr,
                                const unsigned long long* seed_ptr, int* state, const unsigned* allow, long long ld_allow, const short* trans,
                                long long ld_trans, int S, float* ent_out, long long ld_ent, int ent_cols, hipStream_t stream) {
    // no ent_out: iadr1_sample_guided's own launch (and through it, without a guide, iadr1_sample_ex's), the same device code and the same bits
    const SamplerPair pair = ent_out != nullptr ? (allow != nullptr ? PAIR_ENT_GUIDED : PAIR_ENT) : (allow != nullptr ? PAIR_GUIDED : PAIR_EX);
    return sample_launch("sample_ent", pair, stream, logits, ld, out, workspace, B, V, temperature, top_k, top_p, suppress_token, seed, step, step_ptr, seed_ptr, logp_out,
                         ld_logp, logp_cols, min_p, repetition_penalty, seen, ld_seen, mark_seen, state, allow, ld_allow, trans, ld_trans, S, ent_out, ld_ent, ent_cols);
}

// iadr1_sample_ent with logp_out and ent_out taken under softmax(x / logp_temperature) (REF:trl/trl/trainer/grpo_trainer.py:818-821); which token is picked, the filter,
// the draw, `seen` and the automaton read what they read there.  The same kernels: stage 1 forms (s1, u1) on (x - m1) * inv_tl, stage 2 merges them on the same scale.
extern "C" int iadr1_sample_ent_t(const float* logits, long long ld, long long* out, float* logp_out, long long ld_logp, int logp_cols, void* workspace, int B,
                                  int V, float temperature, int top_k, float top_p, float min_p, float repetition_penalty, unsigned* seen, long long ld_seen,
                                  int mark_seen, int suppress_token, unsigned long long seed, unsigned step, const unsigned* step_ptr,
                                  const unsigned long long* seed_ptr, int* state, const unsigned* allow, long long ld_allow, const short* trans,
                                  long long ld_trans, int S, float* ent_out, long long ld_ent, int ent_cols, float logp_temperature, hipStream_t stream) {
    // neither output: iadr1_sample_ent's launch (nothing reads the scale)
    const SamplerPair pair = ent_out != nullptr ? (allow != nullptr ? PAIR_ENT_GUIDED : PAIR_ENT) : (allow != nullptr ? PAIR_GUIDED : PAIR_EX);
    return sample_launch("sample_ent_t", pair, stream, logits, ld, out, workspace, B, V, temperature, top_k, top_p, suppress_token, seed, step, step_ptr, seed_ptr, logp_out,
                         ld_logp, logp_cols, min_p, repetition_penalty, seen, ld_seen, mark_seen, state, allow, ld_allow, trans, ld_trans, S, ent_out, ld_ent, ent_cols,
                         logp_temperature);
}

extern "C" int iadr1_seen_init(const long long* ids, int S, const int* lengths, int Bp, int G, int V, unsigned* seen, long long ld_seen, hipStream_t stream) {
    IADR1_REQUIRE(ids != nullptr && lengths != nullptr && seen != nullptr, "seen_init: ids, lengths and seen are required");
    IADR1_REQUIRE(S > 0 && Bp > 0 && G > 0 && V > 0, "seen_init: empty problem (S=%d, Bp=%d, G=%d, V=%d)", S, Bp, G, V);
    IADR1_REQUIRE(ld_seen >= ((long long)V + 31) / 32, "seen_init: ld_seen=%lld is less than ceil(V / 32) = %lld", ld_seen, ((long long)V + 31) / 32);
    hipLaunchKernelGGL(seen_init_kernel, dim3(Bp * G), dim3(NT), 0, stream, ids, S, lengths, G, V, seen, ld_seen);
    return iadr1_check_launch("seen_init");
}
