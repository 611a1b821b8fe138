// iadr1 skinny GEMMs of the rollout decode step for gfx950 (CDNA4): the four kernels, the decode packers and their entry points.
#include "common.h"
#include <type_traits>

namespace {

// ------------------------------------------------------------------------------------------------------
// Skinny GEMM for the rollout decode step:  Y[M (64 per grid.y), N] = X[M,K] . W[N,K]^T (+ bias).
// HBM-bound weight stream (6.17 GB of bf16 weights per decode step for 3B), and
// for the small projections latency-bound: the whole K extent is therefore spread over MANY waves --
// a block is WAVES (8/16) waves that share 16*NB output columns and take the 64-wide K slabs round-robin
// (optionally also split over grid.z), every wave keeps U slabs in flight, W fragments go straight
// HBM->VGPR with non-temporal 16-byte loads, X fragments come from L2.  The per-wave partial 64 x 16NB tiles
// are combined through LDS and leave as bf16 (+bias), fp32 logits, or -- when K is also split over grid.z --
// as fp32 partial slabs [z][M][N] that the fused residual+RMSNorm kernel sums (no atomics, no zero-init).
// ------------------------------------------------------------------------------------------------------
struct SkinnyArgs {
    const bf16_t* X;
    const bf16_t* W;
    void* Y;
    const bf16_t* bias;
    int M, N, K;
    long long ldx, ldy;
    int out_mode;  // 0 bf16 (+bias), 1 fp32, 2 fp32 partial slabs [gridDim.z][M][ldy], 3 fused SwiGLU (wide kernel, gate/up tile pairs),
                   // 4 fused q|k|v epilogue of the decode step (narrow kernel): bias + rotary + K/V cache append
    // out_mode 4 only: weights packed by iadr1_pack_qkv_rope_bf16 (rotary partners d, d+64 share a 16-column tile)
    const float* rope_cos;     // [M][D/2]
    const float* rope_sin;
    const long long* slot;     // [M] page*32 + offset of the new token, < 0: no cache write
    bf16_t* kcache;
    bf16_t* vcache;
    int Hq, Hkv;
    SideOut so;                // out_mode 4: p0 = roped q|k|v rows; out_mode 3 (persistent kernel): p0 = gate|up rows, p1 = SwiGLU rows (common.h)
    const float* wscale;       // non-null: W is FP8 (OCP e4m3) decode-packed (iadr1_pack_weight_fp8), wscale[n] = dequantisation scale of output row n
    int xcd_order;             // persistent kernel with side outputs: XCD-aware order of the tile groups
};

// ---- the pieces the four kernels share ------------------------------------------------------------------------------------------
// dynamic LDS of a skinny kernel: the cross-wave reduction buffer red[WAVES][64][RLD] of fp32 partial sums (RLD = columns of a reduction round + 1)
constexpr int red_bytes(int waves, int rld) { return waves * 64 * rld * 4; }
// element (m, n) of the block's tile: the waves' partial sums added in wave order
template <int WAVES, int RLD>
__device__ __forceinline__ float red_sum(const float* red, int m, int n) {
    float v = 0.f;
#pragma unroll
    for (int ww = 0; ww < WAVES; ++ww) v += red[((size_t)ww * 64 + m) * RLD + n];
    return v;
}

// a lane's 16 bytes of a packed weight fragment, straight HBM -> VGPR (non-temporal)
__device__ __forceinline__ u32x4_t wload(const void* ptr) { return __builtin_nontemporal_load((const u32x4_t*)ptr); }
// eight FP8 (OCP e4m3) weights -> a bf16 MFMA fragment: v_cvt_scalef32_pk_bf16_fp8, one instruction per pair (exact: every e4m3 value is a bf16 value)
__device__ __forceinline__ bf16x8_t fp8x8_to_bf16(uint32_t lo, uint32_t hi) {
    const bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
    const bf16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
    return (bf16x8_t){a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
// MFMA fragment of a 16-byte weight load: the load itself (bf16 pack), or its half h = the k-step 2s + h of the FP8 pack widened to bf16
template <bool FP8>
__device__ __forceinline__ bf16x8_t wfrag(u32x4_t q, int h) {
    if constexpr (FP8) return fp8x8_to_bf16(q[2 * h], q[2 * h + 1]);
    else return __builtin_bit_cast(bf16x8_t, q);
}

// X fragments of the persistent kernels.  X row-major: lane (lm, lq) reads 16 B of row m_base + 16 i + lm (16 cache lines per wave-load).  X decode-packed
// (ldx == 0, common.h xpk_off): fragment (k-step, row group) is 1 KiB contiguous in lane order, rows padded to 64.
// (The wide kernel spells the same addressing out, and the narrow kernel has pointers per row group: through this struct hipcc allocates their registers differently.)
struct XFrags {
    const bf16_t* base;
    long long group, step;     // row group i is i * group after `base`, 32-deep k-step st is st * step
    int groups_ok;             // row groups i < groups_ok are real rows for this lane (the others re-read group 0)
    __device__ __forceinline__ XFrags(const SkinnyArgs& p, int m_base, int l) {
        const bool xpk = p.ldx == 0;
        const int lm = l & 15, lq = l >> 4;
        base = xpk ? p.X + (long long)blockIdx.y * p.K * 64 + l * 8 : p.X + (long long)min(m_base + lm, p.M - 1) * p.ldx + lq * 8;
        group = xpk ? 512 : 16 * p.ldx;
        step = xpk ? 2048 : 32;
        groups_ok = xpk ? 4 : (p.M - m_base - lm + 15) / 16;
    }
    __device__ __forceinline__ bf16x8_t load(int i, long long st) const {
        return __builtin_bit_cast(bf16x8_t, *(const u32x4_t*)(base + (i < groups_ok ? i * group : 0) + st * step));
    }
};

// plain epilogue: out_mode 0 bf16 (+ bias) / 1 fp32 / 2 fp32 partial slab z; FP8 weights: times the row's dequantisation scale
template <bool FP8>
__device__ __forceinline__ void store_plain(const SkinnyArgs& p, float v, int gm, int gn, int z) {
    if constexpr (FP8) v *= p.wscale[gn];
    if (p.out_mode == 0) {
        if (p.bias) v += bf2f(p.bias[gn]);
        ((bf16_t*)p.Y)[(long long)gm * p.ldy + gn] = f2bf(v);
    } else if (p.out_mode == 1) {
        ((float*)p.Y)[(long long)gm * p.ldy + gn] = v;
    } else {
        ((float*)p.Y)[((long long)z * p.M + gm) * p.ldy + gn] = v;
    }
}
// fused SwiGLU epilogue (out_mode 3): g, u = the GATE and UP projections of output column gn (iadr1_pack_gateup_bf16 interleaves their 16-row tiles):
// a = silu(bf16(gate)) * bf16(up), TF::95-96,552-554.  sb >= 0: the same values in the training layout too, gate|up row [gate | up] and the activation row
template <bool FP8>
__device__ __forceinline__ void store_swiglu(const SkinnyArgs& p, float& g, float& u, int gm, int gn, long long sb) {
    if constexpr (FP8) { g *= p.wscale[gn]; u *= p.wscale[(p.N >> 1) + gn]; }
    g = bf2f(f2bf(g));
    u = bf2f(f2bf(u));
    const float sg = bf2f(f2bf(g / (1.f + __expf(-g))));
    ((bf16_t*)p.Y)[p.ldy ? (long long)gm * p.ldy + gn : xpk_off(gm, gn, p.N >> 1)] = f2bf(sg * u);
    if (sb >= 0) {
        const long long r = sb + (long long)gm * p.so.seq_stride;
        bf16_t* gu = (bf16_t*)p.so.p0 + r * p.so.ld0;
        gu[gn] = f2bf(g);
        gu[(p.N >> 1) + gn] = f2bf(u);
        ((bf16_t*)p.so.p1)[r * p.so.ld1 + gn] = f2bf(sg * u);
    }
}

// FUSEV (out_mode 4, NB == 1 only): the blocks of the K heads also compute the V tile of the same head and 16-dim slice from the X fragments they have already
// loaded, and the grid holds the q and k tiles only.  For the 7B-class widths (28 q + 4 k + 4 v heads = 288 tiles on 256 CUs) that is ONE round of blocks
// instead of two: the second round cost 8 us of a 20 us launch (tools/narrow_ab.py), while a second 115 KB weight tile next to 458 KB of X costs a block ~25 %.
// MG = 16-row groups of X the block multiplies (4 = the 64-row decode tile).  Rollouts of <= 16 / <= 32 sequences (the reference launch scripts' B = 1 x G = 4,
// the evaluation harness) run MG = 1 / 2: a quarter / half of the X fragment loads (each 16-column block re-reads ALL X rows from L2: 41 MB per q|k|v launch at 64 rows
// against 10.5 MB of weights), of the MFMAs and of the cross-wave reduction.  Row groups are independent: a row's bits do not depend on MG.
constexpr int narrow_lds(int nb, int waves, bool fusev = false) { return red_bytes(waves, 16 * nb + 1) * (fusev ? 2 : 1); }
template <int NB, int WAVES, bool FUSEV = false, int MG = 4>
__global__ __launch_bounds__(WAVES * 64) void gemm_skinny_kernel(SkinnyArgs p) {
    constexpr int U = 2, BNC = 16 * NB, RLD = BNC + 1;
    static_assert(!FUSEV || (NB == 1 && MG == 4), "the fused V tile exists for the 16-column q|k|v kernel at the full 64-row tile");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* red = (float*)smem_raw;  // [WAVES][64][RLD] (+ a second one for the fused V tile)
    static_assert(narrow_lds(NB, WAVES, FUSEV) == (FUSEV ? 2 : 1) * WAVES * 64 * RLD * 4, "launchers size the LDS with narrow_lds");
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    const int lm = l & 15, lq = l >> 4;
    const int n0 = blockIdx.x * BNC;
    const int m_base = blockIdx.y * 64;
    const int nslab = p.K >> 6;  // full 64-wide slabs; a trailing 32-wide half slab (K % 64 == 32) is handled after the loops
    const int per_z = (nslab + gridDim.z - 1) / gridDim.z;
    const int s_begin = blockIdx.z * per_z, s_end = min(nslab, s_begin + per_z);
    STAMP(0);

    f32x4_t acc[MG][NB];
#pragma unroll
    for (int i = 0; i < MG; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    // fused V tile of a K-head block (block-uniform): tile index of the same (kv head, 16-dim slice) among the V tiles
    const bool with_v = FUSEV && (int)(blockIdx.x >> 3) >= p.Hq;
    const int vtile = FUSEV ? (int)blockIdx.x + p.Hkv * 8 : 0;
    f32x4_t accv[FUSEV ? 4 : 1];
#pragma unroll
    for (int i = 0; i < (FUSEV ? 4 : 1); ++i) accv[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    // a thread's epilogue column is the same in every round (WAVES*64 is a multiple of BNC): fetch its bias now, not in the tail
    static_assert((WAVES * 64) % BNC == 0, "epilogue column must be loop invariant");
    const float bias_pre = ((p.out_mode == 0 || p.out_mode == 4) && p.bias) ? bf2f(p.bias[min(n0 + (t % BNC), p.N - 1)]) : 0.f;
    const long long side0 = (NB == 1 && p.out_mode == 4) ? side_base(p.so) : -1;
    // out_mode 4 (one output per thread when WAVES*64 == 64*16): rotary factors and the cache slot are fetched up front as well
    float pre_cos = 1.f, pre_sin = 0.f;
    long long pre_slot = -1;
    if (NB == 1 && p.out_mode == 4) {
        const int gm0 = min(m_base + (t >> 4), p.M - 1), dd0 = (blockIdx.x & 7) * 8 + (t & 7);
        pre_slot = p.slot[gm0];
        if ((int)(blockIdx.x >> 3) < p.Hq + p.Hkv) { pre_cos = p.rope_cos[(long long)gm0 * 64 + dd0]; pre_sin = p.rope_sin[(long long)gm0 * 64 + dd0]; }
    }
    // packed weights: fragment (n-tile, 32-k step) is 1 KiB contiguous in lane order -> one fully coalesced load
    const int ksteps = p.K >> 5;
    const bf16_t* wrow[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) wrow[j] = p.W + ((long long)min(blockIdx.x * NB + j, (p.N >> 4) - 1) * ksteps) * 512 + l * 8;
    const bf16_t* wrow_v = p.W + ((long long)min(vtile, (p.N >> 4) - 1) * ksteps) * 512 + l * 8;
    const bool xpk = p.ldx == 0;  // decode-packed X (see the wide kernel)
    const long long xstep = xpk ? 2048 : 32;
    const bf16_t* xrow[MG];
#pragma unroll
    for (int i = 0; i < MG; ++i)
        xrow[i] = xpk ? p.X + (long long)blockIdx.y * p.K * 64 + i * 512 + l * 8 : p.X + (long long)min(m_base + i * 16 + lm, p.M - 1) * p.ldx + lq * 8;

    // unpredicated loads (see the wide kernel): full trips of U slabs, then single-slab tail trips
    auto trip = [&](int sb, auto u_tag, auto v_tag) {
        constexpr int UU = decltype(u_tag)::value;
        constexpr bool WV = decltype(v_tag)::value;      // this block also walks its V tile (block-uniform: chosen once, outside the loops)
        bf16x8_t wf[UU][2][NB], xf[UU][2][MG], wv[FUSEV ? UU : 1][2];
#pragma unroll
        for (int u = 0; u < UU; ++u)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int k = (sb + u * WAVES) * 64 + kk * 32;
#pragma unroll
                for (int j = 0; j < NB; ++j)
                    wf[u][kk][j] = wfrag<false>(wload(wrow[j] + (long long)(k >> 5) * 512), 0);
                if constexpr (WV) wv[u][kk] = wfrag<false>(wload(wrow_v + (long long)(k >> 5) * 512), 0);
#pragma unroll
                for (int i = 0; i < MG; ++i) xf[u][kk][i] = __builtin_bit_cast(bf16x8_t, *(const u32x4_t*)(xrow[i] + (long long)(k >> 5) * xstep));
            }
#pragma unroll
        for (int u = 0; u < UU; ++u)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int i = 0; i < MG; ++i) {
#pragma unroll
                    for (int j = 0; j < NB; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[u][kk][j], xf[u][kk][i], acc[i][j], 0, 0, 0);
                    if constexpr (WV) accv[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv[u][kk], xf[u][kk][i], accv[i], 0, 0, 0);
                }
    };
    int sb = s_begin + w;
    if (FUSEV && with_v) {
        for (; sb + (U - 1) * WAVES < s_end; sb += WAVES * U) trip(sb, std::integral_constant<int, U>{}, std::integral_constant<bool, FUSEV>{});
        for (; sb < s_end; sb += WAVES) trip(sb, std::integral_constant<int, 1>{}, std::integral_constant<bool, FUSEV>{});
    } else {
        for (; sb + (U - 1) * WAVES < s_end; sb += WAVES * U) trip(sb, std::integral_constant<int, U>{}, std::false_type{});
        for (; sb < s_end; sb += WAVES) trip(sb, std::integral_constant<int, 1>{}, std::false_type{});
    }
    if ((p.K & 32) && w == 0 && blockIdx.z == gridDim.z - 1) {  // wave-uniform: the odd 32-wide tail of K
        const int k = nslab * 64;
        bf16x8_t wt[NB], xt[MG];
#pragma unroll
        for (int j = 0; j < NB; ++j) wt[j] = wfrag<false>(wload(wrow[j] + (long long)(k >> 5) * 512), 0);
#pragma unroll
        for (int i = 0; i < MG; ++i) xt[i] = __builtin_bit_cast(bf16x8_t, *(const u32x4_t*)(xrow[i] + (long long)(k >> 5) * xstep));
#pragma unroll
        for (int i = 0; i < MG; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[j], xt[i], acc[i][j], 0, 0, 0);
    }
    // lane owns rows n = j*16 + lq*4 + e of column m = i*16 + lm  (swapped-operand C layout)
    STAMP(1);
    float* mine = red + (size_t)w * 64 * RLD;
#pragma unroll
    for (int i = 0; i < MG; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) mine[(i * 16 + lm) * RLD + j * 16 + lq * 4 + e] = acc[i][j][e];
    float* redv = red + (size_t)WAVES * 64 * RLD;
    if constexpr (FUSEV) {
        if (with_v) {
            float* minev = redv + (size_t)w * 64 * RLD;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) minev[(i * 16 + lm) * RLD + lq * 4 + e] = accv[i][e];
        }
    }
    __syncthreads();
    STAMP(2);
    if (NB == 1 && p.out_mode == 4) {
        // Decode-step q|k|v epilogue (replaces the separate rope + kv-store launch): this block owns one 16-column tile = 8
        // rotary pairs (d, d+64) of one head (q/k heads) or 16 plain dims (v heads).  Same rounding points as the unfused path:
        // bf16(x.W + b), rotary in fp32 on those bf16 values (TF:153-171), bf16 result.
        constexpr int D = 128, HALF = 64;
        const int head = blockIdx.x >> 3, j = blockIdx.x & 7;
        for (int idx = t; idx < MG * 16 * 16; idx += WAVES * 64) {
            const int m = idx >> 4, n = idx & 15, gm = m_base + m;
            if (gm >= p.M) continue;
            const float vs = bf2f(f2bf(red_sum<WAVES, RLD>(red, m, n) + bias_pre));
            // the rotary partner (column n ^ 8 of the same row) is finished by lane ^ 8 of this wave: take its value instead of summing it again
            const float vp = __shfl_xor(vs, 8, WAVE);
            const bool first = idx == t && WAVES * 64 == 64 * 16;   // the prefetched values belong to this (m, n)
            const long long sl = first ? pre_slot : p.slot[gm];
            const long long page = sl >> 5;
            const int off = (int)(sl & 31);
            if (head < p.Hq + p.Hkv) {
                const int dd = j * 8 + (n & 7);
                const float cc = first ? pre_cos : p.rope_cos[(long long)gm * HALF + dd], ss = first ? pre_sin : p.rope_sin[(long long)gm * HALF + dd];
                const float a = n < 8 ? vs : vp, b = n < 8 ? vp : vs;
                const float r = n < 8 ? a * cc - b * ss : b * cc + a * ss;
                const int dim = n < 8 ? dd : HALF + dd;
                if (head < p.Hq) ((bf16_t*)p.Y)[(long long)gm * p.ldy + head * D + dim] = f2bf(r);
                else if (sl >= 0) p.kcache[(page * p.Hkv + (head - p.Hq)) * 32 * D + kpk_off(off, dim)] = f2bf(r);
                if (side0 >= 0) ((bf16_t*)p.so.p0)[(side0 + (long long)gm * p.so.seq_stride) * p.so.ld0 + head * D + dim] = f2bf(r);   // training layout: [q heads | k heads | v heads]
            } else {
                if (sl >= 0) p.vcache[(page * p.Hkv + (head - p.Hq - p.Hkv)) * (long long)D * 32 + (j * 16 + n) * 32 + off] = f2bf(vs);
                if (side0 >= 0) ((bf16_t*)p.so.p0)[(side0 + (long long)gm * p.so.seq_stride) * p.so.ld0 + head * D + j * 16 + n] = f2bf(vs);
            }
            if constexpr (FUSEV) {
                if (with_v) {      // the V tile of the same kv head and 16-dim slice: bias, cache append, training row -- what the V head's own block does above
                    const float vv = bf2f(f2bf(red_sum<WAVES, RLD>(redv, m, n) + (p.bias ? bf2f(p.bias[vtile * 16 + n]) : 0.f)));
                    const int hv = head + p.Hkv;
                    if (sl >= 0) p.vcache[(page * p.Hkv + (hv - p.Hq - p.Hkv)) * (long long)D * 32 + (j * 16 + n) * 32 + off] = f2bf(vv);
                    if (side0 >= 0) ((bf16_t*)p.so.p0)[(side0 + (long long)gm * p.so.seq_stride) * p.so.ld0 + hv * D + j * 16 + n] = f2bf(vv);
                }
            }
        }
        STAMP(3);
        return;
    }
    for (int idx = t; idx < MG * 16 * BNC; idx += WAVES * 64) {
        const int m = idx / BNC, n = idx - m * BNC;
        const int gm = m_base + m, gn = n0 + n;
        if (gm >= p.M || gn >= p.N) continue;
        float v = red_sum<WAVES, RLD>(red, m, n);
        if (p.out_mode == 0) {      // (not store_plain: this kernel has fetched its bias before the loops)
            v += bias_pre;
            ((bf16_t*)p.Y)[(long long)gm * p.ldy + gn] = f2bf(v);
        } else if (p.out_mode == 1) {
            ((float*)p.Y)[(long long)gm * p.ldy + gn] = v;
        } else {
            ((float*)p.Y)[((long long)blockIdx.z * p.M + gm) * p.ldy + gn] = v;
        }
    }
}

// Wide variant (MLP up/down projections, lm_head): one wave owns 16*NB (64/128) columns for its K slabs, so an
// X fragment fetched from L2 feeds NB MFMA column tiles (vector-memory traffic per weight byte drops from 3-5x
// to 1.5-2x: the X re-read through L2, not HBM, limited the narrow kernel), and the 32-deep half-slabs are
// software pipelined: the loads of step j+1 are in flight while the MFMAs of step j run.  K may also be split
// over grid.z (narrow-N, long-K down projection) -> fp32 partial slabs for the fused residual+RMSNorm.
// FP8 = true: the weights are FP8 decode-packed -- Wp8[n/16][k/64][lane][16 B], bytes 0-7 = the lane's 8 weights of k-step 2s, bytes 8-15 = of k-step 2s+1
// (iadr1_pack_weight_fp8) -- so ONE 16-byte load feeds two 32-deep MFMA steps and the weight stream is half as long; the fragments are widened to bf16
// in registers and the output columns are multiplied by the per-row dequantisation scale in the epilogue.  A "step" of the loops is then 64 deep.
constexpr int wide_lds(int waves) { return red_bytes(waves, 32 + 1); }
template <int NB, int WAVES, bool FP8 = false>
__global__ __launch_bounds__(WAVES * 64) void gemm_skinny_wide_kernel(SkinnyArgs p) {
    constexpr int RC = 32, RLD = RC + 1;  // columns per reduction round
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* red = (float*)smem_raw;  // [WAVES][64][RLD]
    static_assert(wide_lds(WAVES) == WAVES * 64 * RLD * 4, "launchers size the LDS with wide_lds");
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    const int lm = l & 15, lq = l >> 4;
    const int n0 = blockIdx.x * 16 * NB;
    const int m_base = blockIdx.y * 64;
    const int nstep = FP8 ? p.K >> 6 : p.K >> 5;
    const int per_z = (nstep + gridDim.z - 1) / gridDim.z;
    const int st_begin = blockIdx.z * per_z, st_end = min(nstep, st_begin + per_z);

    f32x4_t acc[4][NB];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    // addressing kept in a few registers: tile j of this block starts j*tile_stride after tile 0 (wide kernel requires
    // N % (16*NB) == 0), X row group i is i*16 rows further down (XFrags, spelled out)
    const int ksteps = p.K >> 5;
    const long long tile_stride = (long long)ksteps * 512;      // elements of one 16-row weight tile (= bytes in the FP8 form)
    const bf16_t* wbase = p.W + (long long)blockIdx.x * NB * tile_stride + l * 8;
    const char* wbase8 = (const char*)p.W + (long long)blockIdx.x * NB * tile_stride + l * 16;
    const bool xpk = p.ldx == 0;
    const int xr0 = min(m_base + lm, p.M - 1);
    const bf16_t* xbase = xpk ? p.X + (long long)blockIdx.y * p.K * 64 + l * 8 : p.X + (long long)xr0 * p.ldx + lq * 8;
    const long long xgroup = xpk ? 512 : 16 * p.ldx;
    const long long xstep = xpk ? 2048 : 32;
    const int xgroups_ok = xpk ? 4 : (p.M - m_base - lm + 15) / 16;  // row groups i < xgroups_ok are real rows for this lane

    // K is walked in 32-deep steps; wave w takes steps s_begin*2 + w, + WAVES, ... and keeps DEPTH steps in flight
    // (all their loads are issued before the first MFMA of the trip).  Measured against slab-wise software pipelining
    // (tools/stream_probe.py): 4.2 vs 3.0 TB/s on the gate|up stream.
    // No load in these loops is predicated: a per-load `if (ok)` makes hipcc branch around every load and wait for
    // each one (24 branches + waits per trip measured: 43 us instead of 21 us on the gate|up stream).  K % 32 == 0 is
    // guaranteed by the packed layout; the ragged end of a wave's step list runs in the DEPTH=1 tail loop.
    constexpr int DEPTH = 2;
    auto trip = [&](int s0, auto depth_tag) {
        constexpr int DD = decltype(depth_tag)::value;
        if constexpr (FP8) {
            u32x4_t wq[DD][NB];
            bf16x8_t xq[DD][2][4];
#pragma unroll
            for (int d = 0; d < DD; ++d) {
                const long long st = s0 + d * WAVES;
#pragma unroll
                for (int jj = 0; jj < NB; ++jj) wq[d][jj] = __builtin_nontemporal_load((const u32x4_t*)(wbase8 + jj * tile_stride + st * 1024));
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        xq[d][h][i] = __builtin_bit_cast(bf16x8_t, *(const u32x4_t*)(xbase + (i < xgroups_ok ? i * xgroup : 0) + (2 * st + h) * xstep));
            }
#pragma unroll
            for (int d = 0; d < DD; ++d)
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int jj = 0; jj < NB; ++jj) {
                        const bf16x8_t wfr = fp8x8_to_bf16(wq[d][jj][2 * h], wq[d][jj][2 * h + 1]);
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr, xq[d][h][i], acc[i][jj], 0, 0, 0);
                    }
            return;
        }
        bf16x8_t wf[DD][NB], xf[DD][4];
#pragma unroll
        for (int d = 0; d < DD; ++d) {
            const long long st = s0 + d * WAVES;
#pragma unroll
            for (int jj = 0; jj < NB; ++jj)
                wf[d][jj] = __builtin_bit_cast(bf16x8_t, __builtin_nontemporal_load((const u32x4_t*)(wbase + jj * tile_stride + st * 512)));
#pragma unroll
            for (int i = 0; i < 4; ++i)
                xf[d][i] = __builtin_bit_cast(bf16x8_t, *(const u32x4_t*)(xbase + (i < xgroups_ok ? i * xgroup : 0) + st * xstep));
        }
#pragma unroll
        for (int d = 0; d < DD; ++d)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int jj = 0; jj < NB; ++jj) acc[i][jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[d][jj], xf[d][i], acc[i][jj], 0, 0, 0);
    };
    int s0 = st_begin + w;
    for (; s0 + (DEPTH - 1) * WAVES < st_end; s0 += WAVES * DEPTH) trip(s0, std::integral_constant<int, DEPTH>{});
    for (; s0 < st_end; s0 += WAVES) trip(s0, std::integral_constant<int, 1>{});
    float* mine = red + (size_t)w * 64 * RLD;
#pragma unroll
    for (int r = 0; r < NB / 2; ++r) {
        if (r) __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int e = 0; e < 4; ++e) mine[(i * 16 + lm) * RLD + jj * 16 + lq * 4 + e] = acc[i][2 * r + jj][e];
        __syncthreads();
        if (p.out_mode == 3) {
            // tiles (2r, 2r+1) of this round are the gate and up projections of the same 16 output columns
            for (int idx = t; idx < 64 * 16; idx += WAVES * 64) {
                const int m = idx >> 4, n = idx & 15;
                const int gm = m_base + m, gn = (n0 >> 1) + r * 16 + n;
                if (gm >= p.M || gn >= (p.N >> 1)) continue;
                float g = red_sum<WAVES, RLD>(red, m, n), u = red_sum<WAVES, RLD>(red, m, 16 + n);
                store_swiglu<FP8>(p, g, u, gm, gn, -1);
            }
            continue;
        }
        for (int idx = t; idx < 64 * RC; idx += WAVES * 64) {
            const int m = idx / RC, n = idx - m * RC;
            const int gm = m_base + m, gn = n0 + r * RC + n;
            if (gm >= p.M || gn >= p.N) continue;
            store_plain<FP8>(p, red_sum<WAVES, RLD>(red, m, n), gm, gn, blockIdx.z);
        }
    }
}

// Persistent variant for the big decode streams (gate|up, down, lm_head): ONE block per CU stays resident, keeps the X fragments of
// its waves' k-steps in VGPRs for the whole launch (X is read once per CU instead of once per 64-column block: the X re-read was
// 3 us of the 24.6 us gate|up call) and walks groups of two column tiles; the W loads of the next group are issued BEFORE the LDS
// reduction of the current one, so the weight stream does not stop during epilogues (with one-shot blocks every block of the grid
// streams, then every block reduces).  tools/decode_stream.py on weights that really come from HBM: 19.8 vs 24.9 us on the 90 MB
// gate|up stream (4.55 TB/s; a plain read of the same bytes runs at 5.4).  grid.x = nz * bps blocks: slice z = blockIdx.x / bps of K
// (split-K partial slabs, out_mode 2), block b = blockIdx.x % bps takes tile groups b, b + bps, ...
// FP8 = true: the weights are the FP8 decode pack (see gemm_skinny_wide_kernel): a lane's 16-byte load holds its fragments of k-steps 2s and 2s + 1, so a
// wave owns the DOUBLE steps w + j * WAVES (j < KSW / 2) and keeps the X fragments of both halves; the fragments are widened to bf16 in registers and the
// output columns multiplied by the per-row scale in the epilogue.  Half the weight bytes per tile, the same MFMA count.
constexpr int pers_lds(int waves) { return red_bytes(waves, 16 * 2 + 1); }
template <int WAVES, int KSW, bool FP8 = false>
__global__ __launch_bounds__(WAVES * 64) void gemm_skinny_pers_kernel(SkinnyArgs p) {
    constexpr int TPI = 2, RLD = 16 * TPI + 1;
    static_assert(!FP8 || KSW % 2 == 0, "FP8 packs pair the k-steps");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* red = (float*)smem_raw;  // [WAVES][64][RLD]
    static_assert(pers_lds(WAVES) == WAVES * 64 * RLD * 4, "launchers size the LDS with pers_lds");
    const int t = threadIdx.x, w = t >> 6, l = t & 63, lm = l & 15, lq = l >> 4;
    const int b = blockIdx.x, bps = gridDim.x;
    const int m_base = blockIdx.y * 64;
    const long long sb = p.out_mode == 3 ? side_base(p.so) : -1;
    STAMP(4);
    constexpr int XS = FP8 ? 2 : 1;      // k-steps per 16-byte weight load
    constexpr long long tile_bytes = (long long)WAVES * KSW * (FP8 ? 512 : 1024);   // K == 32 * WAVES * KSW exactly (host checks)
    const XFrags x(p, m_base, l);
    const char* wlane = (const char*)p.W + (long long)w * 1024 + l * 16;
    const int ngroups = p.N / (16 * TPI);
    u32x4_t wq[KSW / XS][TPI];
    auto loadw = [&](int g, int j) {      // 16-byte load j of tile group g: this wave's k-step w + j * WAVES (FP8: the double step)
#pragma unroll
        for (int tt = 0; tt < TPI; ++tt) wq[j][tt] = wload(wlane + (g * TPI + tt) * tile_bytes + j * (WAVES * 1024));
    };
    auto loadw_all = [&](int g) {
#pragma unroll
        for (int j = 0; j < KSW / XS; ++j) loadw(g, j);
    };
    // Order of the tile groups.  Plain: block b takes b, b + bps, ...  With side outputs (rows of the row-major training arena: 32 bytes of a row per
    // group and array) the four groups that share a 128-byte line of a row go, in the SAME iteration, to four blocks of ONE XCD (blockIdx.x % 8 is
    // the XCD a block lands on), so that the partial-line stores merge in that XCD's L2 instead of leaving four L2s as four masked writes:
    // XCD x owns the groups g with (g / 4) % 8 == x; its bps / 8 blocks take them round-robin.
    const bool xcd_order = sb >= 0 && (bps & 7) == 0 && p.xcd_order;
    const int gq0 = xcd_order ? (b >> 3) : b, gstep = xcd_order ? (bps >> 3) : bps;
    auto group_of = [&](int q) { return xcd_order ? (((q >> 2) * 8 + (b & 7)) * 4 + (q & 3)) : q; };
    int gq = gq0;
    int g = group_of(gq);
    // the first group's weights are requested BEFORE the X fragments: they come from HBM (the longer latency) and do not depend on anything, the
    // X fragments are 256 KB per CU out of L2 -- measured with in-kernel stamps (profiles/r02_decode_stamps.txt): 6.4 us from entry to the first
    // group's MFMAs with X first
    if (g < ngroups) loadw_all(g);
    bf16x8_t xf[KSW][4];      // X fragments of this wave's k-steps w + j*WAVES (FP8: 2 (w + (j/2) WAVES) + (j & 1)): loaded once, resident for the whole launch
#pragma unroll
    for (int j = 0; j < KSW; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            xf[j][i] = x.load(i, FP8 ? 2 * (w + (j >> 1) * WAVES) + (j & 1) : w + j * WAVES);
    float* mine = red + (size_t)w * 64 * RLD;
    for (; g < ngroups; gq += gstep, g = group_of(gq)) {
        const int g_next = group_of(gq + gstep);
        f32x4_t acc[4][TPI];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int tt = 0; tt < TPI; ++tt) acc[i][tt] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
        // bf16 (round 6): the weight registers of k-step j are re-loaded for the NEXT group as soon as this group's MFMAs of k-step j have been issued -- no second
        // register set, and the stream does not pause for the MFMA phase (before: the whole next group was requested after the last MFMA).  Same arithmetic, same
        // bits; gate|up 21.2 -> 20.6 us, lm_head 113.0 -> 111.7 us on rotating weights, decode step -0.01 ... -0.03 ms (profiles/r06_skinny_reissue_ab.txt)
        const bool reissue = !FP8 && g_next < ngroups;
        auto mfmas = [&](auto reissue_tag) {
#pragma unroll
            for (int j = 0; j < KSW; ++j) {
                if constexpr (FP8) {
#pragma unroll
                    for (int tt = 0; tt < TPI; ++tt) {
                        const bf16x8_t wfr = wfrag<true>(wq[j >> 1][tt], j & 1);
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[i][tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr, xf[j][i], acc[i][tt], 0, 0, 0);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int tt = 0; tt < TPI; ++tt) acc[i][tt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfrag<false>(wq[j][tt], 0), xf[j][i], acc[i][tt], 0, 0, 0);
                    if constexpr (decltype(reissue_tag)::value) loadw(g_next, j);
                }
            }
        };
        if (reissue) mfmas(std::true_type{});
        else mfmas(std::false_type{});
        if (gq == gq0) STAMP(5);
        if (FP8 && g_next < ngroups) loadw_all(g_next);     // (FP8 pack: the whole next group at once, in flight during the reduction below)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int tt = 0; tt < TPI; ++tt)
#pragma unroll
                for (int e = 0; e < 4; ++e) mine[(i * 16 + lm) * RLD + tt * 16 + lq * 4 + e] = acc[i][tt][e];
        __syncthreads();
        const int n0 = g * 16 * TPI;
        if (p.out_mode == 3) {
            // tiles (2g, 2g+1) are the gate and up projections of the same 16 output columns
            for (int idx = t; idx < 64 * 16; idx += WAVES * 64) {
                const int m = idx >> 4, n = idx & 15, gm = m_base + m;
                if (gm >= p.M) continue;
                float gsum = red_sum<WAVES, RLD>(red, m, n), usum = red_sum<WAVES, RLD>(red, m, 16 + n);
                store_swiglu<FP8>(p, gsum, usum, gm, g * 16 + n, sb);
            }
        } else {
            for (int idx = t; idx < 64 * 16 * TPI; idx += WAVES * 64) {
                const int m = idx / (16 * TPI), n = idx - m * (16 * TPI), gm = m_base + m;
                if (gm >= p.M) continue;
                store_plain<FP8>(p, red_sum<WAVES, RLD>(red, m, n), gm, n0 + n, 0);      // (out_mode 2 here has a single K slice)
            }
        }
        __syncthreads();
    }
    STAMP(6);
}

// Split-K form of the persistent kernel for the long-K narrow-N down projection (out_mode 2, fp32 partial slabs): grid.x = nz * bps,
// slice z = blockIdx.x / bps owns k-steps [z*per_z, ...), its bps blocks walk 16-column tiles b, b + bps, ... (one tile per iteration so
// that a block has >= 4 iterations to pipeline: with two-tile groups it had 2 and ran slower than the one-shot kernel).  A wave's steps
// past the end of the slice get a zero X fragment and a clamped (valid, redundant) W address: no predicated loads in the loop.
// FP8 = true: K is walked in 64-deep DOUBLE steps of the FP8 decode pack (KSW of them per wave), see gemm_skinny_pers_kernel.
constexpr int split_lds(int waves) { return red_bytes(waves, 16 + 1); }
template <int WAVES, int KSW, bool FP8 = false>
__global__ __launch_bounds__(WAVES * 64) void gemm_skinny_pers_split_kernel(SkinnyArgs p, int nz, int bps) {
    constexpr int RLD = 16 + 1, XS = FP8 ? 2 : 1;      // X fragments per step of the weight walk
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* red = (float*)smem_raw;  // [WAVES][64][RLD]
    static_assert(split_lds(WAVES) == WAVES * 64 * RLD * 4, "launchers size the LDS with split_lds");
    const int t = threadIdx.x, w = t >> 6, l = t & 63, lm = l & 15, lq = l >> 4;
    const int z = blockIdx.x / bps, b = blockIdx.x - z * bps;
    const int m_base = blockIdx.y * 64;
    const int ksteps = FP8 ? p.K >> 6 : p.K >> 5;        // steps of the weight walk: 32 deep (bf16), 64 deep (FP8: one 16-byte load = two MFMA k-steps)
    const int per_z = (ksteps + nz - 1) / nz;
    const int st_begin = z * per_z, st_end = min(ksteps, st_begin + per_z);
    const XFrags x(p, m_base, l);
    bf16x8_t xf[KSW * XS][4];
    int woff[KSW];      // byte offsets inside a 16-row weight tile (ksteps KiB in either pack)
#pragma unroll
    for (int j = 0; j < KSW; ++j) woff[j] = min(st_begin + w + j * WAVES, st_end - 1) * 1024 + l * 16;
    const int ntiles = p.N >> 4;
    u32x4_t wf[KSW];
    auto loadw = [&](int g) {
        const char* wb = (const char*)p.W + (long long)g * ksteps * 1024;
#pragma unroll
        for (int j = 0; j < KSW; ++j) wf[j] = wload(wb + woff[j]);
    };
    int g = b;
#pragma unroll
    for (int j = 0; j < KSW; ++j) {
        const int st = st_begin + w + j * WAVES;
        const bool ok = st < st_end;
#pragma unroll
        for (int h = 0; h < XS; ++h)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                xf[j * XS + h][i] = __builtin_bit_cast(bf16x8_t, (u32x4_t){0, 0, 0, 0});
                if (ok) xf[j * XS + h][i] = x.load(i, st * XS + h);
            }
    }
    if (g < ntiles) loadw(g);          // after the X fragments here: measured 12.2 vs 12.8 us with the weights first (the opposite of the un-split kernel)
    float* mine = red + (size_t)w * 64 * RLD;
    for (; g < ntiles; g += bps) {
        f32x4_t acc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < KSW; ++j) {
#pragma unroll
            for (int h = 0; h < XS; ++h) {
                const bf16x8_t wfr = wfrag<FP8>(wf[j], h);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr, xf[j * XS + h][i], acc[i], 0, 0, 0);
            }
        }
        if (g + bps < ntiles) loadw(g + bps);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) mine[(i * 16 + lm) * RLD + lq * 4 + e] = acc[i][e];
        __syncthreads();
        for (int idx = t; idx < 64 * 16; idx += WAVES * 64) {
            const int m = idx >> 4, n = idx & 15, gm = m_base + m;
            if (gm >= p.M) continue;
            float v = red_sum<WAVES, RLD>(red, m, n);
            if constexpr (FP8) v *= p.wscale[g * 16 + n];          // the per-row dequantisation scale distributes over the K slices
            ((float*)p.Y)[((long long)z * p.M + gm) * p.ldy + g * 16 + n] = v;
        }
        __syncthreads();
    }
}

// Decode-packing of a fused gate|up matrix W[2I, K] for the SwiGLU-fused skinny GEMM: packed 16-row tile 2q holds
// gate rows [16q, 16q+16), tile 2q+1 the matching up rows [I+16q, ...), so one block owns both halves of its columns.
__global__ __launch_bounds__(256) void pack_gateup_kernel(const bf16_t* W, long long ldw, bf16_t* Wp, int I, int K) {
    const int ksteps = K >> 5;
    const long long total = (long long)(2 * I >> 4) * ksteps * 64;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int lane = (int)(i & 63);
        const long long ts = i >> 6;
        const int ks = (int)(ts % ksteps);
        const long long tile = ts / ksteps;
        const long long n = (tile & 1 ? I : 0) + (tile >> 1) * 16 + (lane & 15);
        const int k = ks * 32 + (lane >> 4) * 8;
        *(u32x4_t*)(Wp + i * 8) = *(const u32x4_t*)(W + n * ldw + k);
    }
}

// Repack W[N,K] (row-major) into MFMA-fragment order for the decode stream:
//   Wp[n/16][k/32][lane = (n%16) + 16*((k%32)/8)][k%8]
__global__ __launch_bounds__(256) void pack_weight_kernel(const bf16_t* W, long long ldw, bf16_t* Wp, int N, int K) {
    const int ksteps = K >> 5;
    const long long total = (long long)(N >> 4) * ksteps * 64;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int lane = (int)(i & 63);
        const long long ts = i >> 6;
        const int ks = (int)(ts % ksteps);
        const long long tile = ts / ksteps;
        const long long n = tile * 16 + (lane & 15);
        const int k = ks * 32 + (lane >> 4) * 8;
        *(u32x4_t*)(Wp + i * 8) = *(const u32x4_t*)(W + n * ldw + k);
    }
}

// Decode-packing of the fused q|k|v matrix for the out_mode-4 epilogue: like pack_weight_kernel, but inside every q and k head
// the 128 rows are dealt to the 8 column tiles as [8j, 8j+8) ++ [64+8j, 64+8j+8) so a tile holds complete rotary pairs; v heads keep
// their natural order.  The bias vector is permuted the same way.
__global__ __launch_bounds__(256) void pack_qkv_rope_kernel(const bf16_t* W, long long ldw, const bf16_t* bias, bf16_t* Wp, bf16_t* bias_p, int n_rope_heads, int N, int K) {
    const int ksteps = K >> 5;
    const long long total = (long long)(N >> 4) * ksteps * 64;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int lane = (int)(i & 63);
        const long long ts = i >> 6;
        const int ks = (int)(ts % ksteps);
        const int tile = (int)(ts / ksteps), lm = lane & 15;
        const int head = tile >> 3, j = tile & 7;
        const long long n = head < n_rope_heads ? (long long)head * 128 + (lm < 8 ? 8 * j + lm : 64 + 8 * j + lm - 8) : (long long)tile * 16 + lm;
        const int k = ks * 32 + (lane >> 4) * 8;
        *(u32x4_t*)(Wp + i * 8) = *(const u32x4_t*)(W + n * ldw + k);
        if (ks == 0 && lane < 16 && bias) bias_p[tile * 16 + lm] = bias[n];
    }
}

// FP8 decode pack, pass 1: dequantisation scale of every output row, scale[n] = max_k |w[n][k]| / 448 (448 = largest finite OCP e4m3 value)
__global__ __launch_bounds__(256) void fp8_row_scale_kernel(const bf16_t* W, long long ldw, float* scale, int K) {
    __shared__ float scratch[16];
    const long long n = blockIdx.x;
    float amax = 0.f;
    for (int c = threadIdx.x; c < (K >> 3); c += 256) {
        const u32x4_t v = *(const u32x4_t*)(W + n * ldw + c * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e) amax = fmaxf(amax, fmaxf(fabsf(lo_bf(v[e])), fabsf(hi_bf(v[e]))));
    }
    amax = block_max<256>(amax, scratch);
    if (threadIdx.x == 0) scale[n] = fmaxf(amax, 1e-30f) / 448.f;
}
// pass 2: Wp8[n/16][k/64][lane][16 bytes] (see gemm_skinny_wide_kernel<.., FP8>); I > 0: gate|up matrix, 16-row tiles of gate and up interleaved like
// pack_gateup_kernel.  Round-to-nearest-even through v_cvt_pk_fp8_f32; |w / scale| <= 448 by construction.
__global__ __launch_bounds__(256) void pack_fp8_kernel(const bf16_t* W, long long ldw, const float* scale, uint32_t* Wp8, int N, int K, int I) {
    const int dsteps = K >> 6;
    const long long total = (long long)(N >> 4) * dsteps * 64;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int lane = (int)(i & 63);
        const long long ts = i >> 6;
        const int sd = (int)(ts % dsteps);
        const long long tile = ts / dsteps;
        const long long n = I > 0 ? ((tile & 1 ? I : 0) + (tile >> 1) * 16 + (lane & 15)) : tile * 16 + (lane & 15);
        const float sc = scale[n];     // true divisions below (not a reciprocal multiply): the quantised values are then the round-to-nearest e4m3 of w / scale exactly
        u32x4_t o;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = sd * 64 + h * 32 + (lane >> 4) * 8;
            const u32x4_t v = *(const u32x4_t*)(W + n * ldw + k);
            int lo = 0, hi = 0;
            lo = __builtin_amdgcn_cvt_pk_fp8_f32(lo_bf(v[0]) / sc, hi_bf(v[0]) / sc, lo, false);
            lo = __builtin_amdgcn_cvt_pk_fp8_f32(lo_bf(v[1]) / sc, hi_bf(v[1]) / sc, lo, true);
            hi = __builtin_amdgcn_cvt_pk_fp8_f32(lo_bf(v[2]) / sc, hi_bf(v[2]) / sc, hi, false);
            hi = __builtin_amdgcn_cvt_pk_fp8_f32(lo_bf(v[3]) / sc, hi_bf(v[3]) / sc, hi, true);
            o[2 * h] = (uint32_t)lo;
            o[2 * h + 1] = (uint32_t)hi;
        }
        *(u32x4_t*)(Wp8 + i * 4) = o;
    }
}

// X[M,K] row-major -> decode-packed (common.h xpk_off); pad rows (M..roundup64) are zero-filled
__global__ __launch_bounds__(256) void pack_act_kernel(const bf16_t* X, long long ldx, bf16_t* Xp, int M, int K) {
    const int Mp = (M + 63) & ~63;
    const long long total = (long long)Mp * (K >> 3);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int m = (int)(i / (K >> 3)), c = (int)(i % (K >> 3));
        const u32x4_t v = m < M ? *(const u32x4_t*)(X + (long long)m * ldx + c * 8) : (u32x4_t){0, 0, 0, 0};
        *(u32x4_t*)(Xp + xpk_off(m, c * 8, K)) = v;
    }
}

}  // namespace

// Launcher configuration, fixed at first use: every instantiation the entry points below can launch is opted in for its dynamic LDS
static void skinny_lds_optin() {
    static const bool done = [] {
        const struct { const void* kernel; int bytes; } list[] = {
            {(const void*)gemm_skinny_kernel<1, 16>, narrow_lds(1, 16)},
            {(const void*)gemm_skinny_kernel<1, 16, false, 1>, narrow_lds(1, 16)},
            {(const void*)gemm_skinny_kernel<1, 16, false, 2>, narrow_lds(1, 16)},
            {(const void*)gemm_skinny_kernel<2, 8>, narrow_lds(2, 8)},
            {(const void*)gemm_skinny_kernel<1, 16, true>, narrow_lds(1, 16, true)},
            {(const void*)gemm_skinny_wide_kernel<8, 8>, wide_lds(8)},
            {(const void*)gemm_skinny_wide_kernel<4, 8>, wide_lds(8)},
            {(const void*)gemm_skinny_wide_kernel<4, 8, true>, wide_lds(8)},
            {(const void*)gemm_skinny_pers_kernel<8, 8>, pers_lds(8)},
            {(const void*)gemm_skinny_pers_kernel<8, 6>, pers_lds(8)},
            {(const void*)gemm_skinny_pers_kernel<8, 4>, pers_lds(8)},
            {(const void*)gemm_skinny_pers_kernel<8, 8, true>, pers_lds(8)},
            {(const void*)gemm_skinny_pers_kernel<8, 6, true>, pers_lds(8)},
            {(const void*)gemm_skinny_pers_kernel<8, 4, true>, pers_lds(8)},
            {(const void*)gemm_skinny_pers_split_kernel<8, 6>, split_lds(8)},
            {(const void*)gemm_skinny_pers_split_kernel<8, 10>, split_lds(8)},
            {(const void*)gemm_skinny_pers_split_kernel<8, 3, true>, split_lds(8)},
        };
        for (const auto& e : list) (void)hipFuncSetAttribute(e.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, e.bytes);
        return true;
    }();
    (void)done;
}

// Argument checks and kernel arguments the bf16 and the FP8 entry point share (`what`: the entry point's name in the error texts)
static int skinny_args(const char* what, bool fp8, SkinnyArgs* p, const void* X, const void* W, const float* wscale, void* Y, const void* bias, int M, int N, int K,
                       long long ldx, long long ldy, int out_mode, int ksplit) {
    const int kmul = fp8 ? 64 : 32, nmul = fp8 ? 64 : 16;
    IADR1_REQUIRE(M > 0 && N > 0 && K > 0 && (!fp8 || wscale != nullptr), "%s: empty problem%s", what, fp8 ? " / no scales" : "");
    IADR1_REQUIRE((K % kmul) == 0 && (N % nmul) == 0 && (ldx % 8) == 0, "%s: %spacked weights need K %% %d == 0 and N %% %d == 0 (K=%d N=%d)", what, fp8 ? "FP8-" : "", kmul, nmul, K, N);
    IADR1_REQUIRE(ldy != 0 || (out_mode == 3 && (N % 64) == 0), "%s: a decode-packed output (ldy == 0) exists for the fused-SwiGLU mode only", what);
    IADR1_REQUIRE((((uintptr_t)X) & 15) == 0 && (((uintptr_t)W) & 15) == 0, "%s: X/W must be 16-byte aligned", what);
    IADR1_REQUIRE(out_mode >= 0 && out_mode <= 3 && ksplit >= 1 && (ksplit == 1 || out_mode == 2), "%s: out_mode 0-3; ksplit > 1 needs out_mode 2 (partial slabs)", what);
    IADR1_REQUIRE(out_mode != 3 || (N % 128) == 0, "%s: fused SwiGLU needs N (= 2*I) to be a multiple of 128, got %d", what, N);
    p->X = (const bf16_t*)X; p->W = (const bf16_t*)W; p->wscale = wscale; p->Y = Y; p->bias = (const bf16_t*)bias; p->M = M; p->N = N; p->K = K;
    p->ldx = ldx; p->ldy = ldy; p->out_mode = out_mode;
    return 0;
}

// The persistent X-resident form that takes a shape, tried before the one-shot kernels; `ncu` = the CUs the decode stream owns (runtime.hip): one block per such CU.
//   bps > 0: split-K slabs for the long-K narrow-N down projection (gemm_skinny_pers_split_kernel): ksplit slices of per_z steps of the weight walk (`depth` deep:
//            32 bf16, 64 FP8 pack), of which a wave keeps <= max_per_z / 8 resident; bps blocks per slice with >= 4 tiles each; no empty slice
//   ksw > 0: the big un-split streams, gate|up and lm_head (gemm_skinny_pers_kernel): K = 32 * 8 waves * ksw exactly, >= 2 tile groups per CU.  Not for the split-K
//            down projection (2 groups per block: two exposed memory latencies, 18.9 vs 14.2 us measured)
struct PersForm { int bps, per_z, ksw; };
static PersForm pers_form(int N, int K, int out_mode, int ksplit, int ncu, int depth, int max_per_z) {
    const int steps = K / depth, per_z = (steps + ksplit - 1) / ksplit, bps = ncu / ksplit, ksw = K / 256;
    if (ksplit > 1 && out_mode == 2 && per_z <= max_per_z && bps >= 1 && (N >> 4) >= 4 * bps && (steps % ksplit == 0 || (ksplit - 1) * per_z < steps)) return {bps, per_z, 0};
    if (ksplit == 1 && (N % 32) == 0 && (K % 256) == 0 && (ksw == 8 || ksw == 6 || ksw == 4) && (N / 32) >= 2 * ncu) return {0, 0, ksw};
    return {0, 0, 0};
}

extern "C" int iadr1_gemm_skinny_bf16(const void* X, const void* W, void* Y, const void* bias, int M, int N, int K, long long ldx,
                                      long long /*ldw: packed weights have none*/, long long ldy, int out_mode, int ksplit, const void* side, hipStream_t stream) {
    SkinnyArgs p{};
    if (int e = skinny_args("gemm_skinny", false, &p, X, W, nullptr, Y, bias, M, N, K, ldx, ldy, out_mode, ksplit)) return e;
    p.xcd_order = 1;      // (decode step with side outputs 2.886 -> 2.834 ms: profiles/EXPERIMENTS.md round 2)
    skinny_lds_optin();
    const int mz = (M + 63) / 64, ncu = iadr1_decode_cus();
    const PersForm f = pers_form(N, K, out_mode, ksplit, ncu, 32, 80);
    if (f.bps) {
        IADR1_REQUIRE(side == nullptr, "gemm_skinny: no side outputs in the split-K slab form");
        // <= 48 k-steps per slice: 6 resident X steps per wave (3B widths: 344 / 8 = 43); <= 80: 10 (7B widths: 592 / 8 = 74; 160 VGPRs of X fragments)
        if (f.per_z <= 48) hipLaunchKernelGGL((gemm_skinny_pers_split_kernel<8, 6>), dim3(f.bps * ksplit, mz, 1), dim3(512), split_lds(8), stream, p, ksplit, f.bps);
        else hipLaunchKernelGGL((gemm_skinny_pers_split_kernel<8, 10>), dim3(f.bps * ksplit, mz, 1), dim3(512), split_lds(8), stream, p, ksplit, f.bps);
        return iadr1_check_launch("gemm_skinny_bf16");
    }
    if (int e = iadr1_side_arg(side, &p.so)) return e;
    IADR1_REQUIRE(!p.so.step || (out_mode == 3 && f.ksw),
                  "gemm_skinny: side outputs exist for the fused-SwiGLU projection in the persistent kernel only (mode %d N=%d K=%d)", out_mode, N, K);
    if (f.ksw) {
        const dim3 grid(ncu, mz, 1), block(512);
        if (f.ksw == 8) hipLaunchKernelGGL((gemm_skinny_pers_kernel<8, 8>), grid, block, pers_lds(8), stream, p);
        else if (f.ksw == 6) hipLaunchKernelGGL((gemm_skinny_pers_kernel<8, 6>), grid, block, pers_lds(8), stream, p);
        else hipLaunchKernelGGL((gemm_skinny_pers_kernel<8, 4>), grid, block, pers_lds(8), stream, p);
        return iadr1_check_launch("gemm_skinny_bf16");
    }
    // one-shot kernels.  Wide: NB=8 (128 columns / block) for the big-N streams (gate|up, lm_head); NB=4 with K split over grid.z for the long-K narrow-N
    // down projection; the narrow kernel for the small projections (latency-bound).
    // with decode-packed X the X fragments are cheap coalesced L2 reads, and 64-column blocks (two co-resident per CU, 344
    // blocks on the 3B gate|up) beat 128-column ones: 24.6 vs 33.7 us on the 90 MB gate|up stream (tools/decode_stream.py)
    const bool big = (N >= 8192 && ksplit == 1) || out_mode == 3;
    const int nb = ldx == 0 ? 4 : 8;      // 64-column blocks with packed X, 128-column ones with row-major X
    if (big && nb == 4 && (N % 64) == 0) hipLaunchKernelGGL((gemm_skinny_wide_kernel<4, 8>), dim3(N / 64, mz, 1), dim3(512), wide_lds(8), stream, p);
    else if (big && (N % 128) == 0) hipLaunchKernelGGL((gemm_skinny_wide_kernel<8, 8>), dim3((N + 127) / 128, mz, 1), dim3(512), wide_lds(8), stream, p);
    else if (ksplit > 1 && (N % 64) == 0 && (N / 64) * ksplit >= 192) hipLaunchKernelGGL((gemm_skinny_wide_kernel<4, 8>), dim3((N + 63) / 64, mz, ksplit), dim3(512), wide_lds(8), stream, p);
    else if (N >= 8192) hipLaunchKernelGGL((gemm_skinny_kernel<2, 8>), dim3((N + 31) / 32, mz, ksplit), dim3(512), narrow_lds(2, 8), stream, p);
    else if (M <= 16) hipLaunchKernelGGL((gemm_skinny_kernel<1, 16, false, 1>), dim3((N + 15) / 16, mz, ksplit), dim3(1024), narrow_lds(1, 16), stream, p);      // (see MG at the kernel)
    else if (M <= 32) hipLaunchKernelGGL((gemm_skinny_kernel<1, 16, false, 2>), dim3((N + 15) / 16, mz, ksplit), dim3(1024), narrow_lds(1, 16), stream, p);
    else hipLaunchKernelGGL((gemm_skinny_kernel<1, 16>), dim3((N + 15) / 16, mz, ksplit), dim3(1024), narrow_lds(1, 16), stream, p);
    return iadr1_check_launch("gemm_skinny_bf16");
}

extern "C" int iadr1_pack_weight_bf16(const void* W, long long ldw, void* Wp, int N, int K, hipStream_t stream) {
    IADR1_REQUIRE(N > 0 && K > 0 && (N % 16) == 0 && (K % 32) == 0 && (ldw % 8) == 0, "pack_weight: need N %% 16 == 0, K %% 32 == 0 (N=%d K=%d)", N, K);
    long long blocks = ((long long)N * K / 8 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(pack_weight_kernel, dim3((int)blocks), dim3(256), 0, stream, (const bf16_t*)W, ldw, (bf16_t*)Wp, N, K);
    return iadr1_check_launch("pack_weight_bf16");
}

extern "C" int iadr1_gemm_qkv_rope_kv_bf16(const void* X, const void* Wp, const void* bias_p, void* q_out, const float* rope_cos, const float* rope_sin,
                                           const long long* slot, void* kcache, void* vcache, int M, int Hq, int Hkv, int D, int K, long long ldx,
                                           long long ldq, const void* side, hipStream_t stream) {
    IADR1_REQUIRE(D == 128, "gemm_qkv_rope_kv: head dim %d not built (128 is)", D);
    IADR1_REQUIRE(M > 0 && Hq > 0 && Hkv > 0 && (K % 32) == 0 && (ldx % 8) == 0, "gemm_qkv_rope_kv: need K %% 32 == 0 (K=%d)", K);
    IADR1_REQUIRE((((uintptr_t)X) & 15) == 0 && (((uintptr_t)Wp) & 15) == 0, "gemm_qkv_rope_kv: X/W must be 16-byte aligned");
    SkinnyArgs p{};
    p.X = (const bf16_t*)X; p.W = (const bf16_t*)Wp; p.Y = q_out; p.bias = (const bf16_t*)bias_p; p.M = M; p.N = (Hq + 2 * Hkv) * D; p.K = K;
p.ldx = ldx; p.ldy = ldq; p.out_mode = 4;
    p.rope_cos = rope_cos; p.rope_sin = rope_sin; p.slot = slot; p.kcache = (bf16_t*)kcache; p.vcache = (bf16_t*)vcache; p.Hq = Hq; p.Hkv = Hkv;
    if (int e = iadr1_side_arg(side, &p.so)) return e;
    skinny_lds_optin();
    const int ncu = iadr1_decode_cus();      // the CUs the decode stream owns (runtime.hip)
    // more tiles than CUs, but the q and k tiles alone fit: the K-head blocks take their V tile along (one round of blocks instead of two)
    const int tiles = p.N / 16, rope_tiles = (Hq + Hkv) * (D / 16);
    if (tiles > ncu && rope_tiles <= ncu && (K % 64) == 0) {
        hipLaunchKernelGGL((gemm_skinny_kernel<1, 16, true>), dim3(rope_tiles, (M + 63) / 64, 1), dim3(1024), narrow_lds(1, 16, true), stream, p);
        return iadr1_check_launch("gemm_qkv_rope_kv_bf16");
    }
    if (M <= 16) hipLaunchKernelGGL((gemm_skinny_kernel<1, 16, false, 1>), dim3(p.N / 16, 1, 1), dim3(1024), narrow_lds(1, 16), stream, p);
    else if (M <= 32) hipLaunchKernelGGL((gemm_skinny_kernel<1, 16, false, 2>), dim3(p.N / 16, 1, 1), dim3(1024), narrow_lds(1, 16), stream, p);
    else hipLaunchKernelGGL((gemm_skinny_kernel<1, 16>), dim3(p.N / 16, (M + 63) / 64, 1), dim3(1024), narrow_lds(1, 16), stream, p);
    return iadr1_check_launch("gemm_qkv_rope_kv_bf16");
}

extern "C" int iadr1_pack_qkv_rope_bf16(const void* W, long long ldw, const void* bias, void* Wp, void* bias_p, int Hq, int Hkv, int D, int K, hipStream_t stream) {
    IADR1_REQUIRE(D == 128 && K > 0 && (K % 32) == 0 && (ldw % 8) == 0, "pack_qkv_rope: need D == 128, K %% 32 == 0 (D=%d K=%d)", D, K);
    const int N = (Hq + 2 * Hkv) * D;
    long long blocks = ((long long)N * K / 8 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(pack_qkv_rope_kernel, dim3((int)blocks), dim3(256), 0, stream, (const bf16_t*)W, ldw, (const bf16_t*)bias, (bf16_t*)Wp, (bf16_t*)bias_p, Hq + Hkv, N, K);
    return iadr1_check_launch("pack_qkv_rope_bf16");
}

extern "C" int iadr1_pack_act_bf16(const void* X, long long ldx, void* Xp, int M, int K, hipStream_t stream) {
    IADR1_REQUIRE(M > 0 && K > 0 && (K % 32) == 0 && (ldx % 8) == 0, "pack_act: need K %% 32 == 0 (K=%d)", K);
    long long blocks = ((long long)((M + 63) & ~63) * K / 8 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(pack_act_kernel, dim3((int)blocks), dim3(256), 0, stream, (const bf16_t*)X, ldx, (bf16_t*)Xp, M, K);
    return iadr1_check_launch("pack_act_bf16");
}

extern "C" int iadr1_pack_gateup_bf16(const void* W, long long ldw, void* Wp, int I, int K, hipStream_t stream) {
    IADR1_REQUIRE(I > 0 && K > 0 && (I % 64) == 0 && (K % 32) == 0 && (ldw % 8) == 0, "pack_gateup: need I %% 64 == 0, K %% 32 == 0 (I=%d K=%d)", I, K);
    long long blocks = ((long long)2 * I * K / 8 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(pack_gateup_kernel, dim3((int)blocks), dim3(256), 0, stream, (const bf16_t*)W, ldw, (bf16_t*)Wp, I, K);
    return iadr1_check_launch("pack_gateup_bf16");
}

// Decode-time skinny GEMM on FP8 weights (include/iadr1_hip.h).  The persistent forms follow the bf16 launcher's shape rules (one resident-step limit: 24 double
// steps per slice, 3 per wave); the one-shot wide kernel, 64 output columns per block, K slices over grid.z, takes everything else (K = 3584 of the 7B widths:
// the X fragments of a wave's k-steps no longer fit in registers).
extern "C" int iadr1_gemm_skinny_fp8w(const void* X, const void* Wp8, const float* wscale, void* Y, const void* bias, int M, int N, int K, long long ldx, long long ldy,
                                      int out_mode, int ksplit, hipStream_t stream) {
    SkinnyArgs p{};
    if (int e = skinny_args("gemm_skinny_fp8w", true, &p, X, Wp8, wscale, Y, bias, M, N, K, ldx, ldy, out_mode, ksplit)) return e;
    skinny_lds_optin();
    const int mz = (M + 63) / 64, ncu = iadr1_decode_cus();
    const PersForm f = pers_form(N, K, out_mode, ksplit, ncu, 64, 24);
    const dim3 grid(ncu, mz, 1), block(512);
    if (f.bps) hipLaunchKernelGGL((gemm_skinny_pers_split_kernel<8, 3, true>), dim3(f.bps * ksplit, mz, 1), block, split_lds(8), stream, p, ksplit, f.bps);
    else if (f.ksw == 8) hipLaunchKernelGGL((gemm_skinny_pers_kernel<8, 8, true>), grid, block, pers_lds(8), stream, p);
    else if (f.ksw == 6) hipLaunchKernelGGL((gemm_skinny_pers_kernel<8, 6, true>), grid, block, pers_lds(8), stream, p);
    else if (f.ksw == 4) hipLaunchKernelGGL((gemm_skinny_pers_kernel<8, 4, true>), grid, block, pers_lds(8), stream, p);
    else hipLaunchKernelGGL((gemm_skinny_wide_kernel<4, 8, true>), dim3(N / 64, mz, ksplit), block, wide_lds(8), stream, p);
    return iadr1_check_launch("gemm_skinny_fp8w");
}

extern "C" int iadr1_pack_weight_fp8(const void* W, long long ldw, void* Wp8, float* scale, int N, int K, int gateup_I, hipStream_t stream) {
    IADR1_REQUIRE(N > 0 && K > 0 && (N % 16) == 0 && (K % 64) == 0 && (ldw % 8) == 0, "pack_weight_fp8: need N %% 16 == 0, K %% 64 == 0 (N=%d K=%d)", N, K);
    IADR1_REQUIRE(gateup_I == 0 || (2 * gateup_I == N && (gateup_I % 64) == 0), "pack_weight_fp8: gateup_I must be N / 2 and a multiple of 64");
    IADR1_REQUIRE(scale != nullptr && (((uintptr_t)Wp8) & 15) == 0, "pack_weight_fp8: scale buffer / 16-byte aligned destination required");
    hipLaunchKernelGGL(fp8_row_scale_kernel, dim3(N), dim3(256), 0, stream, (const bf16_t*)W, ldw, scale, K);
    long long blocks = ((long long)N * K / 16 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(pack_fp8_kernel, dim3((int)blocks), dim3(256), 0, stream, (const bf16_t*)W, ldw, scale, (uint32_t*)Wp8, N, K, gateup_I);
    return iadr1_check_launch("pack_weight_fp8");
}

IADR1_STAMPS_EXPORT(skinny)
