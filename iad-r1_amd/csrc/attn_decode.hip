// Paged-KV decode attention and the cache writers (rollout).  One query token per sequence.
//   K cache page: [Hkv][PAGE=32][D] in MFMA A-fragment order (kpk_off, common.h);  V cache page: [Hkv][D][PAGE] (keys contiguous) so that both
//   MFMA A operands are 16-byte contiguous global loads; a page is exactly one 32-key MFMA k-step.
//   Everything is computed transposed as in attn.hip (S^T = K . Q^T, O^T += V^T . P^T): a lane owns one query column, the `group` q heads of a
//   kv head (or the rows of a whole prompt group) are the MFMA N dimension.
//   Sequences of one GRPO group share their prompt pages through the block table (prefill once per prompt).
// Three things exist once here and are used by every kernel that needs them: the page step (PageFrags::load + page_update), the cross-wave
// combine of online-softmax states (WaveRed) and the output address (out_off); the two cache writers share put_v.
#include "attn_common.h"

namespace {

constexpr int PAGE = 32;

struct DecodeArgs {
    const bf16_t* q;          // [B, Hq*D] (row stride ldq)
    const bf16_t* kcache;     // [npages][Hkv][32 x D in kpk_off order]
    const bf16_t* vcache;     // [npages][Hkv][D][32]
    const int* block_table;   // [B][max_pages]
    const int* ctx_len;       // [B] number of valid keys (including the current token)
    bf16_t* o;                // [B, Hq*D]
    long long ldq, ldo;
    int B, Hq, Hkv, max_pages;
    float scale;
    int gseq;                 // > 1: sequences [g * gseq, (g + 1) * gseq) share their prompt pages (group rollout) -> XCD-aware block order, see the kernel
};

// element (sequence b, dim d of the q head whose columns start at col0) of the output: row-major, or decode-packed when ldo == 0
template <int D>
__device__ __forceinline__ long long out_off(const DecodeArgs& p, int b, int col0, int d) { return p.ldo ? (long long)b * p.ldo + col0 + d : xpk_off(b, col0 + d, p.Hq * D); }

// ---- the page step -------------------------------------------------------------------------------------------------------------------------------
// All K and V fragments of one (page, kv head) for lane l = (li, g): requested up front, one memory latency per page, not two
template <int D>
struct PageFrags {
    bf16x8_t k[D / 32][2], v[D / 16];
    __device__ __forceinline__ void load(const DecodeArgs& p, int phys, int kvh, int l, int li, int g) {
        const bf16_t* kp = p.kcache + ((long long)phys * p.Hkv + kvh) * PAGE * D;
        const bf16_t* vp = p.vcache + ((long long)phys * p.Hkv + kvh) * D * PAGE;
#pragma unroll
        for (int ks = 0; ks < D / 32; ++ks)
#pragma unroll
            for (int t = 0; t < 2; ++t) k[ks][t] = ld_frag_g(kp + ((ks * 2 + t) * 64 + l) * 8, true);  // keys perm_row(li) + 4t (kpk_off)
#pragma unroll
        for (int dt = 0; dt < D / 16; ++dt) v[dt] = ld_frag_g(vp + (dt * 16 + li) * PAGE + g * 8, true);
    }
};

// One page into the online-softmax state (m, lsum in the log2 domain, acc = O^T) of 16 query columns whose Q fragments qfrag(ks) yields.
// Lane (g, e) of score tile t holds key key0 + g*8 + t*4 + e.  MASKED: keys >= n are dropped and an all-masked history (m = -inf) is guarded;
// !MASKED (full prompt pages): neither -- m = -inf on the first page gives alpha = exp2(-inf) = 0.
template <int D, bool MASKED, typename QF>
__device__ __forceinline__ void page_update(const PageFrags<D>& fr, QF qfrag, int key0, int n, int g, float c, float& m, float& lsum, f32x4_t (&acc)[D / 16]) {
    f32x4_t s[2] = {(f32x4_t){0.f, 0.f, 0.f, 0.f}, (f32x4_t){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks)
#pragma unroll
        for (int t = 0; t < 2; ++t) s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr.k[ks][t], qfrag(ks), s[t], 0, 0, 0);
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (MASKED) s[t][e] = key0 + g * 8 + t * 4 + e < n ? s[t][e] * c : -INFINITY;
            else s[t][e] *= c;
            mx = fmaxf(mx, s[t][e]);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 16, WAVE));
    mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));
    const float mn = fmaxf(m, mx);
    const float alpha = (MASKED && mn == -INFINITY) ? 1.f : fast_exp2(m - mn);
    const float mref = (MASKED && mn == -INFINITY) ? 0.f : mn;
    float ps = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) { s[t][e] = fast_exp2(s[t][e] - mref); ps += s[t][e]; }
    lsum = lsum * alpha + ps;
    m = mn;
    const bf16x8_t pf = pack_frag(s[0], s[1]);
#pragma unroll
    for (int dt = 0; dt < D / 16; ++dt) {
        acc[dt] *= alpha;
        acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr.v[dt], pf, acc[dt], 0, 0, 0);
    }
}

// weight of a partial state with running max m in a merge whose max is M (an empty state has m = -inf and weighs nothing)
__device__ __forceinline__ float merge_w(float m, float M) { return (m == -INFINITY) ? 0.f : fast_exp2(m - M); }

// ---- cross-wave combine ----------------------------------------------------------------------------------------------------------------------------
// The WAVES partial states of one 16-column tile in dynamic LDS: m[WAVES][16], l[WAVES][16], o[WAVES][D][gs] (gs = columns kept per d, + 1 pad).
template <int D, int WAVES>
struct WaveRed {
    static constexpr int floats(int gs) { return 2 * WAVES * 16 + WAVES * D * gs; }
    float *m, *l, *o;
    int gs;
    __device__ __forceinline__ WaveRed(float* base, int gs_) : m(base), l(base + WAVES * 16), o(base + 2 * WAVES * 16), gs(gs_) {}
    // wave w's state (lsum still spread over the four 16-lane groups; columns >= gs - 1 are not kept)
    __device__ __forceinline__ void put(int w, int li, int g, float mw, float lsum, const f32x4_t (&acc)[D / 16]) const {
        lsum += __shfl_xor(lsum, 16, WAVE);
        lsum += __shfl_xor(lsum, 32, WAVE);
        if (g == 0) { m[w * 16 + li] = mw; l[w * 16 + li] = lsum; }
        if (li < gs - 1) {
#pragma unroll
            for (int dt = 0; dt < D / 16; ++dt)
#pragma unroll
                for (int e = 0; e < 4; ++e) o[(w * D + dt * 16 + g * 4 + e) * gs + li] = acc[dt][e];
        }
    }
    // merged max, numerator of dim d and denominator of column j (fixed summation order: wave 0 .. WAVES - 1)
    __device__ __forceinline__ void get(int j, int d, float& M, float& num, float& den) const {
        M = m[j];
#pragma unroll
        for (int ww = 1; ww < WAVES; ++ww) M = fmaxf(M, m[ww * 16 + j]);
        num = 0.f; den = 0.f;
#pragma unroll
        for (int ww = 0; ww < WAVES; ++ww) {
            const float f = merge_w(m[ww * 16 + j], M);
            num += f * o[(ww * D + d) * gs + j];
            den += f * l[ww * 16 + j];
        }
    }
};

// =====================================================================================================
// Per-sequence form.  Block = (sequence, kv head); the `group` q heads of that kv head are the MFMA N dimension (<=16).
// The waves take pages round-robin, each keeps an online-softmax state; combined through LDS at the end.
// =====================================================================================================
constexpr int decode_gs(int group) { return group <= 8 ? 9 : 17; }      // q-head columns kept per d (+1 pad): only `group` of the 16 MFMA columns are real
template <int D, int WAVES>
constexpr int decode_lds(int group) { return WaveRed<D, WAVES>::floats(decode_gs(group)) * 4; }

template <int D, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void attn_decode_kernel(DecodeArgs p, SideOut so) {
    constexpr int KS = D / 32, DT = D / 16;
    extern __shared__ float dsm[];
    const int group = p.Hq / p.Hkv;
    const WaveRed<D, WAVES> red(dsm, decode_gs(group));
    // Block -> (sequence, kv head).  Plain: grid (B, Hkv).  Group rollout (gseq > 1, 1-D grid): workgroup ids go round-robin over the 8 XCDs, each with its own
    // L2, so the plain order scatters the gseq sequences that share a prompt's K/V pages over all XCDs and every copy is an L2 miss.  Here XCD x takes the prompt
    // groups x, x + 8, ... and ALL blocks of a group (its sequences x kv heads) run on that one XCD: the pages come from HBM once and from L2 gseq - 1 times.
    int b = blockIdx.x, kvh = blockIdx.y;
    if (p.gseq > 1) {
        const int id = blockIdx.x, npg = p.gseq * p.Hkv, k = id >> 3;
        const int gi = (id & 7) + 8 * (k / npg), mem = k - (k / npg) * npg;
        if (gi * p.gseq >= p.B) return;
        kvh = mem / p.gseq;
        b = gi * p.gseq + (mem - kvh * p.gseq);
    }
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, li = l & 15, g = l >> 4;
    const long long sb = side_base(so);
    STAMP(0);
    const int n = p.ctx_len[b];
    const int npage = (n + PAGE - 1) / PAGE;

    bf16x8_t qf[KS];
    {
        const bool ok = li < group;
        const bf16_t* src = p.q + (long long)b * p.ldq + (kvh * group + li) * D;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = ld_frag_g(src + ks * 32 + g * 8, ok);
    }
    float m = -INFINITY, lsum = 0.f;
    f32x4_t acc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    const float c = p.scale * LOG2E;

    for (int pg = w; pg < npage; pg += WAVES) {
        PageFrags<D> fr;
        fr.load(p, p.block_table[(long long)b * p.max_pages + pg], kvh, l, li, g);
        page_update<D, true>(fr, [&](int ks) { return qf[ks]; }, pg * PAGE, n, g, c, m, lsum, acc);
    }
    STAMP(1);
    red.put(w, li, g, m, lsum, acc);
    __syncthreads();
    STAMP(2);
    // combine the partial states: thread -> (q head j, d)
    for (int idx = threadIdx.x; idx < group * D; idx += WAVES * 64) {
        const int j = idx / D, d = idx - j * D;
        float M, num, den;
        red.get(j, d, M, num, den);
        const bf16_t ov = f2bf(den > 0.f ? num / den : 0.f);
        p.o[out_off<D>(p, b, (kvh * group + j) * D, d)] = ov;
        if (sb >= 0) {      // the row the attention backward of the policy reads, and its log-sum-exp (natural log, as attn_fwd stores it)
            const long long r = sb + (long long)b * so.seq_stride;
            ((bf16_t*)so.p0)[r * so.ld0 + (kvh * group + j) * D + d] = ov;
            if (d == 0) ((float*)so.p1)[(long long)(kvh * group + j) * so.ld1 + r] = den > 0.f ? (M + log2f(den)) * LN2 : -INFINITY;
        }
    }
    STAMP(3);
}

// Group-shared form of the decode attention for LONG shared prompts (LLaVA families: 3000-4000 prompt tokens; MHA decoders): the G sequences of a prompt group
// share their full prompt pages through the block table, so ONE block per (group, kv head) reads those pages once for all G * (Hq / Hkv) query rows (up to NT
// MFMA column tiles of 16) instead of every (sequence, kv head) block reading its own copy -- G times less K/V traffic for the prompt part, which is nearly all
// of it (15 GB of 29 GB per decode step at LLaVA-OneVision-7B shapes).  Phase 1: the 8 waves walk the shared pages; their partial softmax states are combined
// through LDS into one state per query row.  Phase 2: wave s takes sequence s of the group: its private pages (prompt remainder + completion), then the merge
// with the shared state of its rows and the output / side-output stores.  No cross-block exchange; grid = (groups, Hkv).
struct DecodeGroupArgs {
    DecodeArgs a;
    const int* shared_pages;  // [B / G]: leading block-table entries (full prompt pages) shared by the G sequences of a group
    int G;
    // Few (group, kv head) pairs and very long prompts (LLaVA-OneVision-7B: 8 x 4 blocks for 3900 shared tokens): the shared pages are split over `chunks` blocks
    // (grid.z) in a first launch (mode 1) that leaves one partial state per (group, kv head, chunk, row) in `ws`; a second launch (mode 2, grid (groups, Hkv))
    // merges them and runs phase 2.  mode 0: both phases in one launch.
    int mode, chunks;
    float* ws;                // [groups][Hkv][chunks][RMAX][D + 2]: o[D], m, l per row
};

// dynamic LDS of the group kernel, in floats from its base: the reduction scratch, the state of the shared part per query row (log2 domain), the Q fragments
template <int D, int NT>
struct GroupLds {
    static constexpr int WAVES = 8, RMAX = 16 * NT, GS = 17;
    static constexpr int SH_M = WaveRed<D, WAVES>::floats(GS);      // [RMAX]
    static constexpr int SH_L = SH_M + RMAX;                        // [RMAX]
    static constexpr int SH_O = SH_L + RMAX;                        // [RMAX][D]
    static constexpr int QS = SH_O + RMAX * D;                      // bf16 [NT][D / 32][64 lanes][8]
    static constexpr int BYTES = QS * 4 + NT * (D / 32) * 64 * 8 * 2;
};

template <int D, int NT>
__global__ __launch_bounds__(512) void attn_decode_group_kernel(DecodeGroupArgs gp, SideOut so) {
    using L = GroupLds<D, NT>;
    constexpr int KS = D / 32, DT = D / 16, WAVES = L::WAVES, RMAX = L::RMAX;
    const DecodeArgs& p = gp.a;
    extern __shared__ float dsm[];
    const WaveRed<D, WAVES> red(dsm, L::GS);
    float* sh_m = dsm + L::SH_M;
    float* sh_l = dsm + L::SH_L;
    float* sh_o = dsm + L::SH_O;
    const int gi = blockIdx.x, kvh = blockIdx.y, group = p.Hq / p.Hkv, G = gp.G;
    const int rows = G * group;                         // <= RMAX (host checks)
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, li = l & 15, g = l >> 4;
    const long long sb = side_base(so);
    const int b0 = gi * G;
    const int ns = gp.shared_pages[gi];
    const float c = p.scale * LOG2E;

    // ---- phase 1: shared pages, all query rows of the group ----------------------------------------------------------------------------------
    // Q fragments of the NT column tiles live in LDS in fragment order (one conflict-free 16-byte read per fragment and page): 64 VGPRs less than keeping
    // them in registers, which with the 128 accumulator registers of NT = 4 spilled to scratch
    bf16_t* qs = (bf16_t*)(dsm + L::QS);
    for (int t = w; t < NT; t += WAVES) {
        const int r = t * 16 + li, sq = r / group, j = r - sq * group;
        const bool ok = r < rows;
        const bf16_t* src = p.q + (long long)(b0 + (ok ? sq : 0)) * p.ldq + (kvh * group + (ok ? j : 0)) * D;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) *(bf16x8_t*)(qs + ((t * KS + ks) * 64 + l) * 8) = ld_frag_g(src + ks * 32 + g * 8, ok);
    }
    __syncthreads();
    float m[NT], lsum[NT];
    f32x4_t acc[NT][DT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        m[t] = -INFINITY;
        lsum[t] = 0.f;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) acc[t][dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    }
    const int per = gp.mode == 1 ? (ns + gp.chunks - 1) / gp.chunks : ns;           // pages of this block's chunk (mode 1: blockIdx.z)
    const int pg0 = gp.mode == 1 ? (int)blockIdx.z * per : 0, pg1 = gp.mode == 2 ? 0 : min(ns, pg0 + per);
    float* wsb = gp.ws + (((long long)gi * p.Hkv + kvh) * gp.chunks) * RMAX * (D + 2);
    for (int pg = pg0 + w; pg < pg1; pg += WAVES) {
        asm volatile("" ::: "memory");      // keeps the (loop-invariant) Q fragment reads inside the loop: hoisted, they are 64 registers again
        PageFrags<D> fr;
        fr.load(p, p.block_table[(long long)b0 * p.max_pages + pg], kvh, l, li, g);
#pragma unroll
        for (int t = 0; t < NT; ++t)        // every key of a shared page is a prompt token of every sequence of the group: no masking
            page_update<D, false>(fr, [&](int ks) { return *(const bf16x8_t*)(qs + ((t * KS + ks) * 64 + l) * 8); }, 0, 0, g, c, m[t], lsum[t], acc[t]);
    }
    // combine the 8 waves' states, one column tile at a time, into the per-row shared state (LDS; mode 1: this chunk's slot of the workspace)
#pragma unroll
    for (int t = 0; t < NT && gp.mode != 2; ++t) {
        red.put(w, li, g, m[t], lsum[t], acc[t]);
        __syncthreads();
        for (int idx = threadIdx.x; idx < 16 * D; idx += WAVES * 64) {
            const int j = idx / D, d = idx - j * D;
            float M, num, den;
            red.get(j, d, M, num, den);
            if (gp.mode == 1) {
                float* dst = wsb + ((long long)blockIdx.z * RMAX + t * 16 + j) * (D + 2);
                dst[d] = num;
                if (d == 0) { dst[D] = M; dst[D + 1] = den; }
            } else {
                sh_o[(t * 16 + j) * D + d] = num;
                if (d == 0) { sh_m[t * 16 + j] = M; sh_l[t * 16 + j] = den; }
            }
        }
        __syncthreads();
    }
    if (gp.mode == 1) return;
    if (gp.mode == 2) {      // merge the chunks' partial states of the first launch (fixed order: reproducible)
        for (int idx = threadIdx.x; idx < rows * D; idx += WAVES * 64) {
            const int r = idx / D, d = idx - r * D;
            float M = -INFINITY;
            for (int cc = 0; cc < gp.chunks; ++cc) M = fmaxf(M, wsb[((long long)cc * RMAX + r) * (D + 2) + D]);
            float num = 0.f, den = 0.f;
            for (int cc = 0; cc < gp.chunks; ++cc) {
                const float* src = wsb + ((long long)cc * RMAX + r) * (D + 2);
                const float f = merge_w(src[D], M);
                num += f * src[d];
                den += f * src[D + 1];
            }
            sh_o[r * D + d] = num;
            if (d == 0) { sh_m[r] = M; sh_l[r] = den; }
        }
        __syncthreads();
    }

    // ---- phase 2: wave s <- sequence s of the group: private pages, merge with the shared state, stores ----------------------------------------
    for (int sq = w; sq < G; sq += WAVES) {
        const int b = b0 + sq;
        const int n = p.ctx_len[b];
        const int npage = (n + PAGE - 1) / PAGE;
        bf16x8_t q1[KS];
        {
            const bool ok = li < group;
            const bf16_t* src = p.q + (long long)b * p.ldq + (kvh * group + (ok ? li : 0)) * D;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) q1[ks] = ld_frag_g(src + ks * 32 + g * 8, ok);
        }
        float m1 = -INFINITY, l1 = 0.f;
        f32x4_t a1[DT];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) a1[dt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        for (int pg = ns; pg < npage; ++pg) {
            PageFrags<D> fr;
            fr.load(p, p.block_table[(long long)b * p.max_pages + pg], kvh, l, li, g);
            page_update<D, true>(fr, [&](int ks) { return q1[ks]; }, pg * PAGE, n, g, c, m1, l1, a1);
        }
        l1 += __shfl_xor(l1, 16, WAVE);
        l1 += __shfl_xor(l1, 32, WAVE);
        if (li < group) {       // lane (li = head j of the group, g): dims dt * 16 + g * 4 + e
            const int r = sq * group + li;
            const float ms = sh_m[r], lsh = sh_l[r];
            const float M = fmaxf(ms, m1);
            const float fs = merge_w(ms, M), f1 = merge_w(m1, M);
            const float den = fs * lsh + f1 * l1;
            const float inv = den > 0.f ? 1.f / den : 0.f;
            const int col0 = (kvh * group + li) * D;
            const long long rr = sb >= 0 ? sb + (long long)b * so.seq_stride : 0;
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const int d = dt * 16 + g * 4;
                const f32x4_t so4 = *(const f32x4_t*)(sh_o + (long long)r * D + d);
                const u32x2_t ov = {pack2bf((fs * so4[0] + f1 * a1[dt][0]) * inv, (fs * so4[1] + f1 * a1[dt][1]) * inv),
                                    pack2bf((fs * so4[2] + f1 * a1[dt][2]) * inv, (fs * so4[3] + f1 * a1[dt][3]) * inv)};
                *(u32x2_t*)(p.o + out_off<D>(p, b, col0, d)) = ov;
                if (sb >= 0) *(u32x2_t*)((bf16_t*)so.p0 + rr * so.ld0 + col0 + d) = ov;
            }
            if (sb >= 0 && g == 0) ((float*)so.p1)[(long long)(kvh * group + li) * so.ld1 + rr] = den > 0.f ? (M + log2f(den)) * LN2 : -INFINITY;
        }
    }
}

// ---- cache writers -----------------------------------------------------------------------------------------------------------------------------------
// 8 consecutive dims (16-byte chunk c) of one token's V head into the transposed page: element d of key `off` sits at [d][off]
template <int D>
__device__ __forceinline__ void put_v(bf16_t* vcache, long long page_head, int off, int c, const u32x4_t vv) {
    bf16_t* vd = vcache + page_head * D * PAGE + off;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        vd[(c * 8 + 2 * e) * PAGE] = (bf16_t)(vv[e] & 0xffffu);
        vd[(c * 8 + 2 * e + 1) * PAGE] = (bf16_t)(vv[e] >> 16);
    }
}

// Write K/V rows of `T` tokens into the paged cache (prefill: many tokens; decode: one per sequence).
// slot[t] = physical page * 32 + offset, or < 0 to skip (padding).
template <int D>
__global__ __launch_bounds__(256) void kv_store_kernel(const bf16_t* k, long long ldk, const bf16_t* v, long long ldv, const long long* slot,
                                                       bf16_t* kcache, bf16_t* vcache, int T, int Hkv) {
    constexpr int CPR = D / 8;
    const long long total = (long long)T * Hkv * CPR;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % CPR);
        const long long th = i / CPR;
        const int h = (int)(th % Hkv);
        const long long t = th / Hkv;
        const long long sl = slot[t];
        if (sl < 0) continue;
        const long long page = sl >> 5;
        const int off = (int)(sl & 31);
        const u32x4_t kv = *(const u32x4_t*)(k + t * ldk + h * D + c * 8);
        *(u32x4_t*)(kcache + (page * Hkv + h) * PAGE * D + kpk_off(off, c * 8)) = kv;
        put_v<D>(vcache, page * Hkv + h, off, c, *(const u32x4_t*)(v + t * ldv + h * D + c * 8));
    }
}

// Decode-step fusion: rotary on the q and k heads of each new token (in place for q; k goes straight to its
// cache row) + v into the transposed cache page.  One launch instead of rope + kv_store.
template <int D>
__global__ __launch_bounds__(256) void rope_kv_store_kernel(bf16_t* qkv, long long ld, const float* cs, const float* sn, const long long* slot,
                                                            bf16_t* kcache, bf16_t* vcache, int T, int Hq, int Hkv) {
    constexpr int HALF = D / 2, RC = HALF / 4, VC = D / 8;   // rope items (4-element pairs) and v items (8 elements) per head
    const int per_tok = (Hq + Hkv) * RC + Hkv * VC;
    const long long total = (long long)T * per_tok;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long t = i / per_tok;
        int r = (int)(i - t * per_tok);
        const long long sl = slot[t];
        const long long page = sl >> 5;
        const int off = (int)(sl & 31);
        bf16_t* row = qkv + t * ld;
        if (r < (Hq + Hkv) * RC) {
            const int h = r / RC, c = r - h * RC;
            bf16_t* p = row + h * D + c * 4;
            const u32x2_t lo = *(const u32x2_t*)p, hi = *(const u32x2_t*)(p + HALF);
            const f32x4_t cc = *(const f32x4_t*)(cs + t * HALF + c * 4), ss = *(const f32x4_t*)(sn + t * HALF + c * 4);
            const float a[4] = {lo_bf(lo[0]), hi_bf(lo[0]), lo_bf(lo[1]), hi_bf(lo[1])};
            const float b[4] = {lo_bf(hi[0]), hi_bf(hi[0]), lo_bf(hi[1]), hi_bf(hi[1])};
            float oa[4], ob[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) { oa[e] = a[e] * cc[e] - b[e] * ss[e]; ob[e] = b[e] * cc[e] + a[e] * ss[e]; }
            const u32x2_t va = {pack2bf(oa[0], oa[1]), pack2bf(oa[2], oa[3])}, vb = {pack2bf(ob[0], ob[1]), pack2bf(ob[2], ob[3])};
            if (h < Hq) {
                *(u32x2_t*)p = va;
                *(u32x2_t*)(p + HALF) = vb;
            } else if (sl >= 0) {
                bf16_t* kd = kcache + (page * Hkv + (h - Hq)) * PAGE * D;
                *(u32x2_t*)(kd + kpk_off(off, c * 4)) = va;
                *(u32x2_t*)(kd + kpk_off(off, c * 4 + HALF)) = vb;
            }
        } else if (sl >= 0) {
            r -= (Hq + Hkv) * RC;
            const int h = r / VC, c = r - h * VC;
            put_v<D>(vcache, page * Hkv + h, off, c, *(const u32x4_t*)(row + (Hq + Hkv + h) * D + c * 8));
        }
    }
}

}  // namespace

// Launcher configuration, fixed at first use: every instantiation the entry points below can launch is opted in for its dynamic LDS (the per-sequence
// kernel for its larger form, a GQA group above 8)
static void attn_decode_lds_optin() {
    static const bool done = [] {
        const struct { const void* kernel; int bytes; } list[] = {
            {(const void*)attn_decode_kernel<128, 16>, decode_lds<128, 16>(16)},
            {(const void*)attn_decode_group_kernel<128, 1>, GroupLds<128, 1>::BYTES},
            {(const void*)attn_decode_group_kernel<128, 2>, GroupLds<128, 2>::BYTES},
            {(const void*)attn_decode_group_kernel<128, 4>, GroupLds<128, 4>::BYTES},
        };
        for (const auto& e : list) (void)hipFuncSetAttribute(e.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, e.bytes);
        return true;
    }();
    (void)done;
}

extern "C" int iadr1_attn_decode(const void* q, const void* kcache, const void* vcache, const int* block_table, const int* ctx_len, void* o,
                                 int B, int Hq, int Hkv, int D, int max_pages, long long ldq, long long ldo, float scale, int seqs_per_group, const void* side, hipStream_t stream) {
    IADR1_REQUIRE(D == 128, "attn_decode: head dim %d not built (128 is)", D);
    IADR1_REQUIRE(B > 0 && Hq % Hkv == 0 && Hq / Hkv <= 16, "attn_decode: GQA group must be <= 16");
    IADR1_REQUIRE((ldq % 8) == 0, "attn_decode: ldq must be a multiple of 8");
    IADR1_REQUIRE(seqs_per_group >= 0 && (seqs_per_group <= 1 || B % seqs_per_group == 0), "attn_decode: B must be a multiple of seqs_per_group");
    const int gseq = seqs_per_group > 1 ? seqs_per_group : 0;      // the blocks of a prompt group on one XCD: its L2 dedupes the shared prompt pages
    DecodeArgs p{(const bf16_t*)q, (const bf16_t*)kcache, (const bf16_t*)vcache, block_table, ctx_len, (bf16_t*)o, ldq, ldo, B, Hq, Hkv, max_pages, scale, gseq};
    const dim3 grid = gseq ? dim3(8 * ((B / gseq + 7) / 8) * gseq * Hkv) : dim3(B, Hkv);
    SideOut so;
    if (int e = iadr1_side_arg(side, &so)) return e;
    attn_decode_lds_optin();
    // 16 waves per (sequence, kv head) block: a wave then walks ~1.5 pages instead of ~3 at ctx ~ 640 (the kernel is a chain of dependent
    // page loads on only B*Hkv = 128 CUs)
    const int lds = decode_lds<128, 16>(Hq / Hkv);
    hipLaunchKernelGGL((attn_decode_kernel<128, 16>), grid, dim3(1024), lds, stream, p, so);
    return iadr1_check_launch("attn_decode");
}

template <int NT>
static void launch_decode_group(dim3 grid, const DecodeGroupArgs& p, const SideOut& so, hipStream_t stream) {
    constexpr int lds = GroupLds<128, NT>::BYTES;
    hipLaunchKernelGGL((attn_decode_group_kernel<128, NT>), grid, dim3(512), lds, stream, p, so);
}

extern "C" int iadr1_attn_decode_group(const void* q, const void* kcache, const void* vcache, const int* block_table, const int* ctx_len, const int* shared_pages, void* o,
                                       int B, int G, int Hq, int Hkv, int D, int max_pages, long long ldq, long long ldo, float scale, int chunks, float* ws,
                                       const void* side, hipStream_t stream) {
    IADR1_REQUIRE(D == 128, "attn_decode_group: head dim %d not built (128 is)", D);
    IADR1_REQUIRE(B > 0 && G >= 1 && (B % G) == 0 && Hq % Hkv == 0 && Hq / Hkv <= 16 && G * (Hq / Hkv) <= 64 && shared_pages != nullptr,
                  "attn_decode_group: B must be a multiple of the group size and a group may hold at most 64 query rows per kv head (G=%d, heads per kv head=%d)", G, Hkv ? Hq / Hkv : 0);
    IADR1_REQUIRE((ldq % 8) == 0 && (ldo % 4) == 0, "attn_decode_group: ldq must be a multiple of 8, ldo of 4");
    IADR1_REQUIRE(chunks >= 1 && chunks <= 64 && (chunks == 1 || ws != nullptr), "attn_decode_group: 1 <= chunks <= 64, and chunks > 1 needs the workspace");
    DecodeGroupArgs p{{(const bf16_t*)q, (const bf16_t*)kcache, (const bf16_t*)vcache, block_table, ctx_len, (bf16_t*)o, ldq, ldo, B, Hq, Hkv, max_pages, scale, 0}, shared_pages, G, 0, chunks, ws};
    SideOut so, none{};
    if (int e = iadr1_side_arg(side, &so)) return e;
    attn_decode_lds_optin();
    const int rows = G * (Hq / Hkv);
    auto launch = rows <= 16 ? launch_decode_group<1> : (rows <= 32 ? launch_decode_group<2> : launch_decode_group<4>);
    if (chunks == 1) {
        launch(dim3(B / G, Hkv), p, so, stream);
    } else {
        p.mode = 1;
        launch(dim3(B / G, Hkv, chunks), p, none, stream);
        p.mode = 2;
        launch(dim3(B / G, Hkv), p, so, stream);
    }
    return iadr1_check_launch("attn_decode_group");
}

extern "C" int iadr1_kv_store(const void* k, long long ldk, const void* v, long long ldv, const long long* slot, void* kcache, void* vcache,
                              int T, int Hkv, int D, hipStream_t stream) {
    IADR1_REQUIRE(D == 128, "kv_store: head dim %d not built (128 is)", D);
    IADR1_REQUIRE(T > 0 && (ldk % 8) == 0 && (ldv % 8) == 0, "kv_store: strides must be multiples of 8");
    long long blocks = ((long long)T * Hkv * 16 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(kv_store_kernel<128>, dim3((int)blocks), dim3(256), 0, stream, (const bf16_t*)k, ldk, (const bf16_t*)v, ldv, slot, (bf16_t*)kcache, (bf16_t*)vcache, T, Hkv);
    return iadr1_check_launch("kv_store");
}

extern "C" int iadr1_rope_kv_store(void* qkv, long long ld, const float* cos_t, const float* sin_t, const long long* slot, void* kcache,
                                   void* vcache, int T, int Hq, int Hkv, int D, hipStream_t stream) {
    IADR1_REQUIRE(D == 128, "rope_kv_store: head dim %d not built (128 is)", D);
    IADR1_REQUIRE(T > 0 && (ld % 8) == 0, "rope_kv_store: ld must be a multiple of 8");
    const long long total = (long long)T * ((Hq + Hkv) * 16 + Hkv * 16);
    long long blocks = (total + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(rope_kv_store_kernel<128>, dim3((int)blocks), dim3(256), 0, stream, (bf16_t*)qkv, ld, cos_t, sin_t, slot, (bf16_t*)kcache, (bf16_t*)vcache, T, Hq, Hkv);
    return iadr1_check_launch("rope_kv_store");
}

IADR1_STAMPS_EXPORT(attn_decode)
