// iadr1 GEMM family for gfx950 (CDNA4).
//
//   C[M,N] (+)= act( A[M,K] . B[N,K]^T + bias[N] )       "NT": both operands K-contiguous
//
// This is the contraction behind every Linear of the hot path (SURVEY.md section 2.3 K1,K6,K7,K8,K12,
// K14,K15; reference call sites TF:modeling_qwen2_5_vl.py:85-96,116-122,148-150,218-219,634-637,
// 552-554,1386-1387).  Forward uses W[N,K] directly; dgrad / wgrad reuse the same kernel on
// transposed copies produced by transpose.hip.
//
// Kernel gemm_nt_128: 128x128x64 block tile, 4 waves (2x2) of 64x64, v_mfma_f32_16x16x32_bf16,
// operands staged HBM->LDS with global_load_lds_dwordx4 (no VGPR round trip), 2 LDS buffers so the
// DMA of tile t+1 overlaps the MFMAs of tile t, XOR-swizzled LDS image (swizzle applied on the
// per-lane SOURCE address and on the ds_read address; the LDS destination of the DMA stays
// lane-linear as the hardware requires), XCD-aware block->tile map (8 XCDs, private L2s) with
// 8-tile-high bands so the 64 blocks resident on one XCD share A/B panels in its L2.
// MFMA operands are swapped (B-tile as the A operand) so each lane ends up with 4 consecutive
// output columns of one row: bf16 results are staged through LDS and leave as 16-byte row-contiguous
// stores; fp32 results (logit chunks, wgrad accumulation) leave as 16-byte stores/RMW per lane.
#include "common.h"
#include <stdlib.h>

namespace {

constexpr int BM = 128, BN = 128, BK = 64, NTHREADS = 256;
constexpr int TILE_BYTES = BM * BK * 2;          // 16 KiB per operand tile
constexpr int STAGE_BYTES = 2 * TILE_BYTES;      // A + B
constexpr int SMEM_BYTES = 2 * STAGE_BYTES;      // double buffered: 64 KiB
constexpr int C_LD = BN + 8;                     // bf16 epilogue row stride (elements)

struct GemmArgs {
    const bf16_t* A;
    const bf16_t* B;
    void* C;
    const bf16_t* bias;
    const void* zeros;  // >=16 zero bytes, source for out-of-range K chunks
    int M, N, K;
    long long lda, ldb, ldc;
    int act;  // 0 none, 1 exact GELU
    int band;  // tile rows per rasterisation band (gemm_nt_256)
    bf16_t* C2;      // OUT_SWIGLU: a[M, N/2] = silu(gate) * up (C = the gate|up matrix itself, or null when only `a` is wanted)
    long long ldc2;
    // OUT_LSE / OUT_DLOGITS (linear_logprob: the lm_head contraction whose logits never reach HBM)
    const long long* targets;   // [M] column of the row's target (< 0: ignored row)
    float* part;                // OUT_LSE: [M][nparts] pairs (max, sum of exp(x - max)) over each wave's 64-column slice
    float* tgt_logit;           // OUT_LSE: [M] the logit at the target column (rows with a target in range)
    const float* lse;           // OUT_DLOGITS: [M] log-sum-exp of the row
    const float* g;             // OUT_DLOGITS: [M] dLoss/dlogp of the row
    int nparts;
    // split-K (gemm_nt_256<OUT_F32>, iadr1_gemm_nt_splitk_acc_bf16): grid = ksplit x tiles; slice z = blockIdx.x / tiles contracts columns
    // [z * kslice, min(K, (z + 1) * kslice)) of A and B and stores its fp32 partial tile at C + z * zstride (a workspace the reduce kernel sums)
    int ksplit, kslice;
    long long zstride;
    // OUT_SWIGLU_ROWS (iadr1_gemm_swiglu_rows_bf16): GEMM row r is row (r >> rb_shift) * rb_stride + (r & (2^rb_shift - 1)) of A, C and C2 -- blocks of 2^rb_shift
    // consecutive rows rb_stride rows apart (the rows a chunk of decode steps produced in a sequence-major arena)
    int rb_shift;
    long long rb_stride;
    // OUT_LSE / OUT_DLOGITS at a temperature (iadr1_linear_logprob_fwd_t / _dlogits_t): both epilogues work on y = x * inv_t, inv_t = 1 / T formed once on the host
    float inv_t = 1.f;
};

enum { OUT_BF16 = 0, OUT_F32 = 1, OUT_F32_ACC = 2, OUT_SWIGLU = 3, OUT_LSE = 4, OUT_DLOGITS = 5, OUT_SWIGLU_ROWS = 6 };

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void gbl_void;

// y = x * inv_t as ONE fp32 multiply per accumulator element, in place, before an epilogue reads it; the empty asm keeps -ffp-contract from fusing the product
// into the subtraction that follows it.  Registers only: no pointer, LDS or store.  inv_t == 1: the same bits.
template <int MI>
__device__ __forceinline__ void scale_acc(f32x4_t (&acc)[MI][4], float inv_t) {
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float y = acc[i][j][e] * inv_t;
                asm volatile("" : "+v"(y));
                acc[i][j][e] = y;
            }
}

__device__ __forceinline__ void glds16(const void* g, char* lds_wave_base) {
    // LDS destination = wave-uniform base + lane*16 (hardware rule); source address is per lane.
    __builtin_amdgcn_global_load_lds((gbl_void*)g, (lds_void*)lds_wave_base, 16, 0, 0);
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f)); }

template <int OUT>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_nt_128(GemmArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l = t & 63;

    // ---- block -> tile map (XCD-aware, bijective for any grid) --------------------------------
    const int tiles_m = (p.M + BM - 1) / BM, tiles_n = (p.N + BN - 1) / BN;
    const int nwg = tiles_m * tiles_n;
    const int bid = blockIdx.x;
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    const int band = wg / (8 * tiles_n), in_band = wg - band * 8 * tiles_n;
    const int band_rows = min(8, tiles_m - band * 8);
    const int tm = band * 8 + in_band % band_rows, tn = in_band / band_rows;
    const int m0 = tm * BM, n0 = tn * BN;

    // ---- per-thread DMA sources: 4 A chunks + 4 B chunks (16 B each) per K tile --------------------
    const bf16_t* a_src[4];
    const bf16_t* b_src[4];
    int chunk_k[4];  // element offset of the (swizzled) source chunk inside the K tile
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int L = (i * 4 + w) * 64 + l;  // linear 16-B slot in the LDS tile image
        const int row = L >> 3, c = L & 7;
        const int cs = c ^ ((row >> 1) & 7);  // source chunk that must land in slot (row, c)
        chunk_k[i] = cs * 8;
        a_src[i] = p.A + (long long)min(m0 + row, p.M - 1) * p.lda + cs * 8;
        b_src[i] = p.B + (long long)min(n0 + row, p.N - 1) * p.ldb + cs * 8;
    }
    auto stage = [&](int buf, int kt) {
        char* base = smem + buf * STAGE_BYTES;
        const int k0 = kt * BK;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool ok = k0 + chunk_k[i] < p.K;
            glds16(ok ? (const void*)(a_src[i] + k0) : p.zeros, base + (i * 4 + w) * 1024);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool ok = k0 + chunk_k[i] < p.K;
            glds16(ok ? (const void*)(b_src[i] + k0) : p.zeros, base + TILE_BYTES + (i * 4 + w) * 1024);
        }
    };

    // ---- fragment read offsets (swizzled), wave tile 64x64 -------------------------------------------
    const int wm = w >> 1, wn = w & 1;
    int a_off[2], b_off[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int chunk = kk * 4 + (l >> 4);
        const int ra = wm * 64 + (l & 15), rb = wn * 64 + (l & 15);
        a_off[kk] = ra * 128 + ((chunk ^ ((ra >> 1) & 7)) << 4);
        b_off[kk] = TILE_BYTES + rb * 128 + ((chunk ^ ((rb >> 1) & 7)) << 4);
    }

    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    const int nk = (p.K + BK - 1) / BK;
    stage(0, 0);
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        __syncthreads();  // tile kt landed (vmcnt(0) + barrier); everyone is done reading buffer cur^1
        if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
        const char* sbase = smem + cur * STAGE_BYTES;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bf16x8_t af[4], bfr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) af[i] = *(const bf16x8_t*)(sbase + a_off[kk] + i * 2048);
#pragma unroll
            for (int j = 0; j < 4; ++j) bfr[j] = *(const bf16x8_t*)(sbase + b_off[kk] + j * 2048);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    // swapped operands: D[row = n][col = m] -> lane owns 4 consecutive n of one m
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i][j], 0, 0, 0);
        }
    }

    // ---- epilogue ------------------------------------------------------------------------------------
    const int lm = l & 15, lq = l >> 4;
    if constexpr (OUT == OUT_BF16) {
        __syncthreads();  // all waves finished reading the operand buffers
        bf16_t* cs = (bf16_t*)smem;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int nl = wn * 64 + j * 16 + lq * 4;
            float bv[4] = {0.f, 0.f, 0.f, 0.f};
            if (p.bias) {
#pragma unroll
                for (int e = 0; e < 4; ++e) bv[e] = (n0 + nl + e < p.N) ? bf2f(p.bias[n0 + nl + e]) : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ml = wm * 64 + i * 16 + lm;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = acc[i][j][e] + bv[e];
                    if (p.act == 1) v[e] = gelu_erf(v[e]);
                }
                u32x2_t pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
                *(u32x2_t*)(cs + ml * C_LD + nl) = pk;
            }
        }
        __syncthreads();
        bf16_t* C = (bf16_t*)p.C;
        const bool vec_ok = ((p.ldc & 7) == 0) && ((((uintptr_t)C) & 15) == 0);
        if (vec_ok && m0 + BM <= p.M && n0 + BN <= p.N) {   // interior tile: 8 slab reads, then 8 unpredicated 16-byte stores
            u32x4_t rv[8];
#pragma unroll
            for (int it = 0; it < 8; ++it) rv[it] = *(const u32x4_t*)(cs + ((it * NTHREADS + t) >> 4) * C_LD + (t & 15) * 8);
#pragma unroll
            for (int it = 0; it < 8; ++it) *(u32x4_t*)(C + (long long)(m0 + ((it * NTHREADS + t) >> 4)) * p.ldc + n0 + (t & 15) * 8) = rv[it];
            return;
        }
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = it * NTHREADS + t;
            const int row = idx >> 4, ch = idx & 15;
            const int gm = m0 + row, gn = n0 + ch * 8;
            if (gm >= p.M || gn >= p.N) continue;
            const u32x4_t v = *(const u32x4_t*)(cs + row * C_LD + ch * 8);
            bf16_t* dst = C + (long long)gm * p.ldc + gn;
            if (vec_ok && gn + 8 <= p.N) {
                *(u32x4_t*)dst = v;
            } else {
                const bf16_t* sv = cs + row * C_LD + ch * 8;  // scalar tail straight from LDS
                for (int e = 0; e < 8 && gn + e < p.N; ++e) dst[e] = sv[e];
            }
        }
    } else {
        float* C = (float*)p.C;
        const bool vec_ok = ((p.ldc & 3) == 0) && ((((uintptr_t)C) & 15) == 0);
        if (vec_ok && !p.bias && p.act == 0 && m0 + BM <= p.M && n0 + BN <= p.N) {   // interior tile, plain store / accumulate (see gemm_nt_256)
            float* base = C + (long long)(m0 + wm * 64 + lm) * p.ldc + n0 + wn * 64 + lq * 4;
#pragma unroll
            for (int i0 = 0; i0 < 4; i0 += 2) {
                f32x4_t old[2][4];
                if constexpr (OUT == OUT_F32_ACC) {
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int j = 0; j < 4; ++j) old[u][j] = *(const f32x4_t*)(base + (long long)(i0 + u) * 16 * p.ldc + j * 16);
                }
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        f32x4_t o = acc[i0 + u][j];
                        if constexpr (OUT == OUT_F32_ACC) o += old[u][j];
                        *(f32x4_t*)(base + (long long)(i0 + u) * 16 * p.ldc + j * 16) = o;
                    }
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gm = m0 + wm * 64 + i * 16 + lm;
            if (gm >= p.M) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gn = n0 + wn * 64 + j * 16 + lq * 4;
                if (gn >= p.N) continue;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = acc[i][j][e];
                    if (p.bias && gn + e < p.N) v[e] += bf2f(p.bias[gn + e]);
                    if (p.act == 1) v[e] = gelu_erf(v[e]);
                }
                float* dst = C + (long long)gm * p.ldc + gn;
                if (vec_ok && gn + 4 <= p.N) {
                    f32x4_t o = {v[0], v[1], v[2], v[3]};
                    if constexpr (OUT == OUT_F32_ACC) {
                        const f32x4_t old = *(const f32x4_t*)dst;
                        o += old;
                    }
                    *(f32x4_t*)dst = o;
                } else {
                    for (int e = 0; e < 4 && gn + e < p.N; ++e) {
                        if constexpr (OUT == OUT_F32_ACC) dst[e] += v[e];
                        else dst[e] = v[e];
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------
// gemm_nt_256: 256x256x64 block tile, 8 waves (2 x 4) of 128x64, deep software pipeline ("8 phases per two K
// tiles"): every K tile is consumed in 4 phases of 16 MFMAs (one 64x32 quadrant of the wave tile x K=64);
// each phase ds_reads only the operand half it newly needs (A half: 8 x b128, B half: 4 x b128), issues the
// LDS-DMA of ONE half-tile of the NEXT K tile into the other LDS buffer, and waits with a COUNTED vmcnt so two
// half-tiles stay in flight across the s_barrier -- the DMA queue is never drained inside the main loop.
// LDS: 2 buffers x (A 32 KiB + B 32 KiB) = 128 KiB, XOR-swizzled like gemm_nt_128 (source address + read side).
// Half-tiles are cut so that a phase needs the same half for every wave: A half h = rows {wm*128 + h*64 + 0..63},
// B half h = cols {wn*64 + h*32 + 0..31}.  Epilogue: each wave stages its 128x64 bf16 result in its own LDS
// slab and writes full 128-byte row segments.
// ------------------------------------------------------------------------------------------------------
constexpr int T2 = 256, NT2 = 512, HALF_BYTES = 128 * 64 * 2;          // 16 KiB per half tile
constexpr int BUF2_BYTES = 4 * HALF_BYTES;                             // A0 A1 B0 B1
constexpr int SMEM2_MAIN = 2 * BUF2_BYTES;                             // 128 KiB
constexpr int EP_LD = 64 + 8;                                          // epilogue slab row stride (elements)
constexpr int SMEM2_EPI = 8 * 128 * EP_LD * 2;                         // 147456 B
constexpr int SMEM2_BYTES = SMEM2_EPI > SMEM2_MAIN ? SMEM2_EPI : SMEM2_MAIN;

#define IADR1_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")

// TN form (template flag, OUT_F32 / OUT_F32_ACC only: the weight gradients  dW[M, N] (+)= A[K, M]^T . B[K, N],  A = dY and B = X as they lie in memory, the
// contraction running over their ROWS): the same pipeline and epilogue; a half-tile image is [64 contraction rows][128 columns] with 256-byte rows (chunk c of
// row r at chunk position c ^ 2 * tn_rho(r), the swizzle of the attention tiles), filled by the same 2 x 16-byte DMA per thread from row-major sources, and the
// MFMA fragments -- 8 consecutive contraction elements of one column per lane -- come out of LDS through the hardware transpose read (ds_read_b64_tr_b16, two
// per fragment: common.h tr_frag_ld).  No transposed copies of dY / X exist anywhere.
__device__ __forceinline__ int tn_rho(int r) { return (r & 3) | ((r >> 1) & 4); }
// One MFMA fragment of the TN form: contraction rows 32 kk + {0..3} and {4..7} (+ this lane's row) of the lane's column, two transpose reads at byte offsets
// kk * 8192 and + 1024.  Inline asm, not the builtin: the compiler orders every LDS-reading INTRINSIC behind all outstanding global_load_lds (it put s_waitcnt
// vmcnt(0) in front of each group of reads -- the DMA queue drained four times per K tile: 872 instead of 1230 TF/s); the kernel's own counted vmcnt / lgkmcnt
// waits and barriers are what orders these reads, exactly as for the plain ds_read_b128 of the NT form.
__device__ __forceinline__ bf16x8_t tr_frag_asm(const char* lds_addr, int kk) {
    s16x4_t a, b;
    const unsigned addr = (unsigned)(uintptr_t)lds_ptr(lds_addr);
    if (kk == 0) {
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(a) : "v"(addr));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:1024" : "=v"(b) : "v"(addr));
    } else {
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:8192" : "=v"(a) : "v"(addr));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:9216" : "=v"(b) : "v"(addr));
    }
    return __builtin_bit_cast(bf16x8_t, (s16x8_t)__builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7));
}

template <int OUT, bool TN = false>
__global__ __launch_bounds__(NT2, 2) void gemm_nt_256(GemmArgs p) {
    static_assert(!TN || OUT == OUT_F32 || OUT == OUT_F32_ACC, "the TN form exists for the fp32 (accumulate) outputs only");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l = t & 63;
    const int wm = w >> 2, wn = w & 3;

    const int tiles_m = (p.M + T2 - 1) / T2, tiles_n = (p.N + T2 - 1) / T2;
    const int nwg = tiles_m * tiles_n;
    int bid = blockIdx.x;
    if constexpr (OUT == OUT_F32) {
        if (p.ksplit > 1) {      // block-uniform: this block's K slice and its slab of the partial-sum workspace
            const int z = bid / nwg;
            bid -= z * nwg;
            p.A += (long long)z * p.kslice * (TN ? p.lda : 1);
            p.B += (long long)z * p.kslice * (TN ? p.ldb : 1);
            p.K = min(p.kslice, p.K - z * p.kslice);
            p.C = (float*)p.C + (long long)z * p.zstride;
        }
    }
    const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
    const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
    const int BR = p.band;
    const int band = wg / (BR * tiles_n), in_band = wg - band * BR * tiles_n;
    const int band_rows = min(BR, tiles_m - band * BR);
    const int tm = band * BR + in_band % band_rows, tn = in_band / band_rows;
    const int m0 = tm * T2, n0 = tn * T2;

    // ---- DMA sources: per half-tile 2 x 16 B per thread ----------------------------------------------------
    const bf16_t* src[4][2];  // [A0, A1, B0, B1][instr]
    int chunk_k[2];           // NT: element offset of the slot's chunk inside the K tile; TN: the slot's row inside the K tile
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int L = (i * 8 + w) * 64 + l;   // 16-B slot inside the half-tile image
        if constexpr (TN) {
            const int rl = L >> 4, cpos = L & 15;                  // row of the 64-row K tile, chunk POSITION inside its 256-byte row
            const int cl = (cpos ^ (2 * tn_rho(rl))) * 8;          // first of the 8 half-image columns this slot holds
            chunk_k[i] = rl;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int acol = m0 + (cl >> 6) * 128 + h * 64 + (cl & 63);     // A half h: output rows wm*128 + h*64 + ..  (columns of A)
                const int bcol = n0 + h * 128 + cl;      // B half h: 128 CONSECUTIVE columns of B (whole 128-byte lines per DMA row piece; wave wn owns columns
                                                         // h*128 + wn*32 + .. of the tile, see `coln` in the epilogue -- with the NT form's wn*64 + h*32 + .. a
                                                         // row piece would be 64 bytes and every line of B would be requested twice)
                src[h][i] = p.A + (long long)rl * p.lda + min(acol, p.M - 8);
                src[2 + h][i] = p.B + (long long)rl * p.ldb + min(bcol, p.N - 8);
            }
        } else {
        const int rl = L >> 3, c = L & 7;
        const int cs = c ^ ((rl >> 1) & 7);
        chunk_k[i] = cs * 8;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int arow = (rl >> 6) * 128 + h * 64 + (rl & 63);          // A half h: rows wm*128 + h*64 + ..
            const int bcol = (rl >> 5) * 64 + h * 32 + (rl & 31);           // B half h: cols wn*64 + h*32 + ..
            if constexpr (OUT == OUT_SWIGLU_ROWS) {
                const int ar = m0 + arow;       // (M % 256 == 0: no clamp)
                src[h][i] = p.A + ((long long)(ar >> p.rb_shift) * p.rb_stride + (ar & ((1 << p.rb_shift) - 1))) * p.lda + cs * 8;
            } else {
                src[h][i] = p.A + (long long)min(m0 + arow, p.M - 1) * p.lda + cs * 8;
            }
            if constexpr (OUT == OUT_SWIGLU || OUT == OUT_SWIGLU_ROWS) {
                // fused SwiGLU: B = [gate rows 0..I) | up rows I..2I).  The block's 256 columns are 128 gate + 128 up columns of the SAME 128 outputs,
                // arranged so that B half 0 of every wave is gate and half 1 is up: a lane then holds gate (n-tiles 0,1) and up (n-tiles 2,3) of the
                // same (row, column) and the activation is computed in registers.
                src[2 + h][i] = p.B + (long long)(h * (p.N >> 1) + (n0 >> 1) + (rl >> 5) * 32 + (rl & 31)) * p.ldb + cs * 8;
            } else {
                src[2 + h][i] = p.B + (long long)min(n0 + bcol, p.N - 1) * p.ldb + cs * 8;
            }
        }
        }
    }
    auto stage_half = [&](int buf, int half /*0..3 = A0 A1 B0 B1*/, int kt) {
        char* base = smem + buf * BUF2_BYTES + half * HALF_BYTES;
        const int k0 = kt * BK;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bool ok = k0 + chunk_k[i] < p.K;
            if constexpr (TN) glds16(ok ? (const void*)(src[half][i] + (long long)k0 * (half < 2 ? p.lda : p.ldb)) : p.zeros, base + (i * 8 + w) * 1024);
            else glds16(ok ? (const void*)(src[half][i] + k0) : p.zeros, base + (i * 8 + w) * 1024);
        }
    };

    // ---- fragment read offsets inside a half-tile image -------------------------------------------------------
    int a_off[2], b_off[2];  // per k-step; add mi*2048 / ni*2048
    int ta_off[4], tb_off[2];  // TN: per m-tile / n-tile; add kk*8192 (+1024 for the second four contraction rows)
    if constexpr (TN) {
        // lane (lg = l & 15, g = l >> 4) addresses row 8g + (lg >> 2) [+ 32 kk, + 4] and the 8-byte half (lg & 1) of chunk  2 * tile16 + ((lg & 3) >> 1)  of the
        // half image; tn_rho of that row is ((lg >> 2) & 3) | ((g & 1) << 2) for every kk and both halves of a fragment, so the swizzle is a per-lane constant
        const int lg = l & 15, g = l >> 4;
        const int x = 2 * (((lg >> 2) & 3) | ((g & 1) << 2));
        const int rowpart = (8 * g + (lg >> 2)) * 256 + (lg & 1) * 8, cb = (lg & 3) >> 1;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) ta_off[mi] = rowpart + (((wm * 8 + mi * 2 + cb) ^ x) << 4);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) tb_off[ni] = rowpart + (((wn * 4 + ni * 2 + cb) ^ x) << 4);
    } else {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const int chunk = kk * 4 + (l >> 4);
        const int ra = wm * 64 + (l & 15), rb = wn * 32 + (l & 15);
        a_off[kk] = ra * 128 + ((chunk ^ ((ra >> 1) & 7)) << 4);
        b_off[kk] = rb * 128 + ((chunk ^ ((rb >> 1) & 7)) << 4);
    }
    }

    f32x4_t acc[8][4];  // [m-tile][n-tile] of the 128x64 wave tile
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    bf16x8_t af[4][2], bfr[2][2];  // current A half (4 m-tiles x 2 k-steps), current B half (2 n-tiles x 2 k-steps)
    bf16x8_t bfr1[TN ? 2 : 1][2];  // TN: B half 1 in registers of its own, so that B half 0 survives phases 2 - 3 and phase 4 reads nothing (transpose reads are the
                                   // form's bottleneck: 48 instead of 56 per K tile)
    auto read_a = [&](int buf, int h) {
        const char* base = smem + buf * BUF2_BYTES + h * HALF_BYTES;
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                if constexpr (TN) af[mi][kk] = tr_frag_asm(base + ta_off[mi], kk);
                else af[mi][kk] = *(const bf16x8_t*)(base + a_off[kk] + mi * 2048);
            }
    };
    auto read_b = [&](int buf, int h) {
        const char* base = smem + buf * BUF2_BYTES + (2 + h) * HALF_BYTES;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                if constexpr (TN) {
                    if (h == 0) bfr[ni][kk] = tr_frag_asm(base + tb_off[ni], kk);
                    else bfr1[ni][kk] = tr_frag_asm(base + tb_off[ni], kk);
                } else {
                    bfr[ni][kk] = *(const bf16x8_t*)(base + b_off[kk] + ni * 2048);
                }
            }
    };
#define IADR1_QUAD_B(MH, NH, BF)                                                                                             \
    do {                                                                                                                     \
        __builtin_amdgcn_s_setprio(1);                                                                                       \
        _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                                                                     \
        _Pragma("unroll") for (int mi = 0; mi < 4; ++mi)                                                                     \
        _Pragma("unroll") for (int ni = 0; ni < 2; ++ni)                                                                     \
            acc[(MH) * 4 + mi][(NH) * 2 + ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(BF[ni][kk], af[mi][kk], acc[(MH) * 4 + mi][(NH) * 2 + ni], 0, 0, 0); \
        __builtin_amdgcn_s_setprio(0);                                                                                       \
    } while (0)
    // Why not v_mfma_f32_32x32x16_bf16 (4 x 2 accumulators of 32 x 32 per wave tile): one A half against BOTH B halves per phase gives four independent
    // accumulators, the same one coming round every fourth MFMA (128 cycles apart) -- with two accumulators per phase, 64 apart, the dependent MFMAs stalled:
    // 1125 instead of 1270 TF/s.  Even the four-accumulator form was 9 % slower on six of the seven hot shapes (profiles/EXPERIMENTS.md round 6 #2; code last in 70639a8).
#define IADR1_QUAD(MH, NH)                                                                                                   \
    do {                                                                                                                     \
        if constexpr (TN) { if ((NH) == 0) IADR1_QUAD_B(MH, NH, bfr); else IADR1_QUAD_B(MH, NH, bfr1); }                     \
        else IADR1_QUAD_B(MH, NH, bfr);                                                                                      \
    } while (0)

    const int nk = (p.K + BK - 1) / BK;
    // Schedule (u = K tile, buffer u&1).  A half-tile region is re-filled ONE phase after the phase that read it;
    // that is safe because every phase retires its ds_reads (lgkmcnt(0)) BEFORE its barrier:
    //   phase 1: read A0,B0(u)  | DMA B0(u+1) -> other buffer   | barrier | quadrant (0,0)
    //   phase 2: read B1(u)     | DMA A0(u+2) -> this buffer    | barrier | quadrant (0,1)
    //   phase 3: read A1(u)     | DMA B1(u+2) -> this buffer    | barrier | quadrant (1,1)
    //   phase 4: read B0(u)     | DMA A1(u+2) -> this buffer    | vmcnt(6): all of tile u+1 landed, three
    //                                                              half-tiles of u+2 stay in flight | barrier | (1,0)
    // prologue: tile 0 complete + A0,B1,A1 of tile 1 in flight.
    stage_half(0, 0, 0);
    stage_half(0, 2, 0);
    stage_half(0, 3, 0);
    stage_half(0, 1, 0);
    if (nk > 1) {
        stage_half(1, 0, 1);
        stage_half(1, 3, 1);
        stage_half(1, 1, 1);
        IADR1_VMCNT(6);
    } else {
        IADR1_VMCNT(0);
    }
    __builtin_amdgcn_s_barrier();

#define IADR1_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
    // Role split: the two waves of every SIMD (wm = 0 / 1) run half a phase apart -- while one issues its MFMAs the
    // other does its ds_reads / DMA issue -- by giving the wm=1 half ONE extra barrier here (and the wm=0 half one at
    // the end).  Each phase therefore has two barriers: [reads, DMA, lgkmcnt(0)] | barrier | [16 MFMA] | barrier.
    // The region re-fill / landing rules above still hold: a reader always passes one more barrier than the wait or
    // the last read it depends on.
    if (wm == 1) __builtin_amdgcn_s_barrier();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1, nxt = cur ^ 1;
        const bool more1 = kt + 1 < nk, more2 = kt + 2 < nk;
        read_a(cur, 0);
        read_b(cur, 0);
        if (more1) stage_half(nxt, 2, kt + 1);
        IADR1_LGKM0();
        __builtin_amdgcn_s_barrier();
        IADR1_QUAD(0, 0);
        __builtin_amdgcn_s_barrier();

        read_b(cur, 1);
        if (more2) stage_half(cur, 0, kt + 2);
        IADR1_LGKM0();
        __builtin_amdgcn_s_barrier();
        IADR1_QUAD(0, 1);
        __builtin_amdgcn_s_barrier();

        read_a(cur, 1);
        if (more2) stage_half(cur, 3, kt + 2);
        IADR1_LGKM0();
        __builtin_amdgcn_s_barrier();
        IADR1_QUAD(1, 1);
        __builtin_amdgcn_s_barrier();

        if constexpr (!TN) read_b(cur, 0);
        if (more2) { stage_half(cur, 1, kt + 2); IADR1_VMCNT(6); } else if (more1) { IADR1_VMCNT(0); }
        IADR1_LGKM0();
        __builtin_amdgcn_s_barrier();
        IADR1_QUAD(1, 0);
        __builtin_amdgcn_s_barrier();
    }
    if (wm == 0) __builtin_amdgcn_s_barrier();
#undef IADR1_LGKM0
#undef IADR1_QUAD
#undef IADR1_QUAD_B

    // ---- epilogue ------------------------------------------------------------------------------------------------
    const int lm = l & 15, lq = l >> 4;
    if constexpr (OUT == OUT_SWIGLU || OUT == OUT_SWIGLU_ROWS) {
        // interior tiles only (the launcher guarantees M % 256 == 0, N % 256 == 0, 16-byte aligned outputs)
        __syncthreads();  // every wave is done with the operand buffers
        bf16_t* slab = (bf16_t*)smem + (size_t)w * 128 * EP_LD;
        const int I = p.N >> 1;
        const long long row0 = m0 + wm * 128;
        const int ca = (n0 >> 1) + wn * 32;           // first of this wave's 32 output columns
        // row of the output matrices that GEMM row r lands in (the identity but for the row-blocked form)
        auto orow = [&](long long r) -> long long {
            if constexpr (OUT == OUT_SWIGLU_ROWS) return (r >> p.rb_shift) * p.rb_stride + (r & ((1 << p.rb_shift) - 1));
            else return r;
        };
        if (p.C) {   // the gate|up matrix itself (backward needs it): slab columns 0..31 = gate, 32..63 = up
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    *(u32x2_t*)(slab + (i * 16 + lm) * EP_LD + j * 16 + lq * 4) = (u32x2_t){pack2bf(acc[i][j][0], acc[i][j][1]), pack2bf(acc[i][j][2], acc[i][j][3])};
            bf16_t* C = (bf16_t*)p.C;
            const int ch = l & 7;
            bf16_t* dstc = C + (ch < 4 ? ca + ch * 8 : I + ca + (ch - 4) * 8);
            bf16_t* dst0 = dstc + (row0 + (l >> 3)) * p.ldc;
            const bf16_t* src0 = slab + (l >> 3) * EP_LD + ch * 8;
            u32x4_t rv[16];
#pragma unroll
            for (int it = 0; it < 16; ++it) rv[it] = *(const u32x4_t*)(src0 + it * 8 * EP_LD);
#pragma unroll
            for (int it = 0; it < 16; ++it) {
                if constexpr (OUT == OUT_SWIGLU_ROWS) *(u32x4_t*)(dstc + orow(row0 + (l >> 3) + it * 8) * p.ldc) = rv[it];
                else *(u32x4_t*)(dst0 + (long long)it * 8 * p.ldc) = rv[it];
            }
        }
        // a = bf16(silu(bf16 gate)) * bf16 up, the arithmetic of swiglu_fwd_kernel on the rounded gate|up values
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float av[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float gq = bf2f(f2bf(acc[i][j][e])), uq = bf2f(f2bf(acc[i][j + 2][e]));
                    av[e] = bf2f(f2bf(gq / (1.f + __expf(-gq)))) * uq;
                }
                *(u32x2_t*)(slab + (i * 16 + lm) * EP_LD + j * 16 + lq * 4) = (u32x2_t){pack2bf(av[0], av[1]), pack2bf(av[2], av[3])};
            }
        {
            bf16_t* dstc = p.C2 + ca + (l & 3) * 8;      // 4 lanes per 64-byte row segment, 16 rows per instruction
            bf16_t* dst0 = dstc + (row0 + (l >> 2)) * p.ldc2;
            const bf16_t* src0 = slab + (l >> 2) * EP_LD + (l & 3) * 8;
            u32x4_t rv[8];
#pragma unroll
            for (int it = 0; it < 8; ++it) rv[it] = *(const u32x4_t*)(src0 + it * 16 * EP_LD);
#pragma unroll
            for (int it = 0; it < 8; ++it) {
                if constexpr (OUT == OUT_SWIGLU_ROWS) *(u32x4_t*)(dstc + orow(row0 + (l >> 2) + it * 16) * p.ldc2) = rv[it];
                else *(u32x4_t*)(dst0 + (long long)it * 16 * p.ldc2) = rv[it];
            }
        }
    } else if constexpr (OUT == OUT_LSE) {
        // linear_logprob forward: per row and 64-column wave slice the pair (max, sum exp(x - max)) and the logit at the row's target column; the
        // logits themselves are never stored.  Lane (lm, lq) holds columns j*16 + lq*4 + e of rows i*16 + lm: in-lane over (j, e), then over lq.
        scale_acc(acc, p.inv_t);    // from here on acc holds y = x / T (REF:trl/trl/trainer/grpo_trainer.py:818-821)
        const int cbase = n0 + wn * 64;
        const bool full = cbase + 64 <= p.N;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = m0 + wm * 128 + i * 16 + lm;
            float mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (full || cbase + j * 16 + lq * 4 + e < p.N) mx = fmaxf(mx, acc[i][j][e]);
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            float sm = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (full || cbase + j * 16 + lq * 4 + e < p.N) sm += __expf(acc[i][j][e] - mx);
            sm += __shfl_xor(sm, 16);
            sm += __shfl_xor(sm, 32);
            if (row < p.M) {
                if (lq == 0) *(f32x2_t*)(p.part + ((long long)row * p.nparts + tn * 4 + wn) * 2) = (f32x2_t){mx, sm};
                const long long tg = p.targets[row];
                if (tg >= cbase && tg < cbase + 64) {
                    const int d = (int)(tg - cbase) - lq * 4;     // this lane holds d = j*16 + e, e in 0..3
                    float tv = 0.f;
                    bool hit = false;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (d == j * 16 + e) { tv = acc[i][j][e]; hit = true; }
                    if (hit) p.tgt_logit[row] = tv;
                }
            }
        }
    } else if constexpr (OUT == OUT_BF16 || OUT == OUT_DLOGITS) {
        __syncthreads();  // every wave is done with the operand buffers
        bf16_t* slab = (bf16_t*)smem + (size_t)w * 128 * EP_LD;
        if constexpr (OUT == OUT_DLOGITS) {
            // linear_logprob backward: the recomputed logits leave as dlogits = g * (onehot(target) - exp(x - lse)) in bf16 (iadr1_dlogits_rows's arithmetic);
            // at a temperature on y = x / T, with the chain rule's 1 / T on g
            scale_acc(acc, p.inv_t);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int row = min(m0 + wm * 128 + i * 16 + lm, p.M - 1);
                const float rl = p.lse[row], rg = p.g[row] * p.inv_t;
                const long long tg = p.targets[row];
                const int d = (tg >= 0 && tg < p.N) ? (int)tg - (n0 + wn * 64) - lq * 4 : -1;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = -rg * __expf(acc[i][j][e] - rl) + (d == j * 16 + e ? rg : 0.f);
                    *(u32x2_t*)(slab + (i * 16 + lm) * EP_LD + j * 16 + lq * 4) = (u32x2_t){pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (OUT == OUT_DLOGITS) break;
            const int nl = j * 16 + lq * 4;
            const int gn = n0 + wn * 64 + nl;
            float bv[4] = {0.f, 0.f, 0.f, 0.f};
            if (p.bias) {
#pragma unroll
                for (int e = 0; e < 4; ++e) bv[e] = (gn + e < p.N) ? bf2f(p.bias[gn + e]) : 0.f;
            }
            if (p.act == 1) {       // one uniform branch per column group, not one per element
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = gelu_erf(acc[i][j][e] + bv[e]);
                    *(u32x2_t*)(slab + (i * 16 + lm) * EP_LD + nl) = (u32x2_t){pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
                }
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[i][j][e] + bv[e];
                    *(u32x2_t*)(slab + (i * 16 + lm) * EP_LD + nl) = (u32x2_t){pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
                }
            }
        }
        // same wave wrote and reads its slab: only its own LDS ops need to retire (compiler inserts lgkmcnt)
        bf16_t* C = (bf16_t*)p.C;
        const bool vec_ok = ((p.ldc & 7) == 0) && ((((uintptr_t)C) & 15) == 0);
        if (vec_ok && m0 + wm * 128 + 128 <= p.M && n0 + wn * 64 + 64 <= p.N) {
            // interior sub-tile (all of them on the hot shapes): 16 slab reads, then 16 row-contiguous 16-byte stores, no per-store predicate
            // (a predicated store is a branch; 16 of them serialise the slab reads behind the stores)
            bf16_t* dst0 = C + (long long)(m0 + wm * 128 + (l >> 3)) * p.ldc + n0 + wn * 64 + (l & 7) * 8;
            const bf16_t* src0 = slab + (l >> 3) * EP_LD + (l & 7) * 8;
            u32x4_t rv[16];
#pragma unroll
            for (int it = 0; it < 16; ++it) rv[it] = *(const u32x4_t*)(src0 + it * 8 * EP_LD);
#pragma unroll
            for (int it = 0; it < 16; ++it) *(u32x4_t*)(dst0 + (long long)it * 8 * p.ldc) = rv[it];
            return;
        }
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int row = it * 8 + (l >> 3), ch = l & 7;
            const int gm = m0 + wm * 128 + row, gn = n0 + wn * 64 + ch * 8;
            if (gm >= p.M || gn >= p.N) continue;
            bf16_t* dst = C + (long long)gm * p.ldc + gn;
            if (vec_ok && gn + 8 <= p.N) {
                *(u32x4_t*)dst = *(const u32x4_t*)(slab + row * EP_LD + ch * 8);
            } else {
                const bf16_t* sv = slab + row * EP_LD + ch * 8;
                for (int e = 0; e < 8 && gn + e < p.N; ++e) dst[e] = sv[e];
            }
        }
    } else {
        float* C = (float*)p.C;
        const bool vec_ok = ((p.ldc & 3) == 0) && ((((uintptr_t)C) & 15) == 0);
        // first output column of n-tile j of this lane (TN: the wave's 64 columns are two 32-column runs 128 apart, see the B half images)
        auto coln = [&](int j) -> int {
            if constexpr (TN) return n0 + (j >> 1) * 128 + wn * 32 + (j & 1) * 16 + lq * 4;
            else return n0 + wn * 64 + j * 16 + lq * 4;
        };
        if (vec_ok && !p.bias && p.act == 0 && m0 + wm * 128 + 128 <= p.M && (TN ? n0 + T2 <= p.N : n0 + wn * 64 + 64 <= p.N)) {
            // interior sub-tile, plain store / accumulate (every wgrad and the lm_head): no predicates, and for the accumulate form the 8 loads
            // of two row groups are in flight together instead of one load -> add -> store round trip per 16 bytes
            float* base = C + (long long)(m0 + wm * 128 + lm) * p.ldc;
#pragma unroll
            for (int i0 = 0; i0 < 8; i0 += 2) {
                f32x4_t old[2][4];
                if constexpr (OUT == OUT_F32_ACC) {
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int j = 0; j < 4; ++j) old[u][j] = *(const f32x4_t*)(base + (long long)(i0 + u) * 16 * p.ldc + coln(j));
                }
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        f32x4_t o = acc[i0 + u][j];
                        if constexpr (OUT == OUT_F32_ACC) o += old[u][j];
                        *(f32x4_t*)(base + (long long)(i0 + u) * 16 * p.ldc + coln(j)) = o;
                    }
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int gm = m0 + wm * 128 + i * 16 + lm;
            if (gm >= p.M) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gn = coln(j);
                if (gn >= p.N) continue;
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = acc[i][j][e];
                    if (p.bias && gn + e < p.N) v[e] += bf2f(p.bias[gn + e]);
                    if (p.act == 1) v[e] = gelu_erf(v[e]);
                }
                float* dst = C + (long long)gm * p.ldc + gn;
                if (vec_ok && gn + 4 <= p.N) {
                    f32x4_t o = {v[0], v[1], v[2], v[3]};
                    if constexpr (OUT == OUT_F32_ACC) o += *(const f32x4_t*)dst;
                    *(f32x4_t*)dst = o;
                } else {
                    for (int e = 0; e < 4 && gn + e < p.N; ++e) {
                        if constexpr (OUT == OUT_F32_ACC) dst[e] += v[e];
                        else dst[e] = v[e];
                    }
                }
            }
        }
    }
}

// linear_logprob, second launch: one wave per row merges the row's (max, sum) pairs in a fixed order -> lse, logp = logit[target] - lse (0 for ignored rows).
__global__ __launch_bounds__(256) void lse_combine_kernel(const float* part, const float* tgt_logit, const long long* targets, float* logp, float* lse_out, int R, int V,
                                                          int nparts) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (row >= R) return;
    const f32x2_t* pp = (const f32x2_t*)part + (long long)row * nparts;
    float m = -INFINITY, s = 0.f;
    for (int i = l; i < nparts; i += 64) {
        const f32x2_t v = pp[i];
        if (v[0] > m) { s *= __expf(m - v[0]); m = v[0]; }
        if (v[0] != -INFINITY) s += v[1] * __expf(v[0] - m);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
        const float mm = fmaxf(m, m2);
        s = (m == -INFINITY ? 0.f : s * __expf(m - mm)) + (m2 == -INFINITY ? 0.f : s2 * __expf(m2 - mm));
        m = mm;
    }
    if (l == 0) {
        const float lse = m + logf(s);
        if (lse_out) lse_out[row] = lse;
        const long long tg = targets[row];
        logp[row] = (tg >= 0 && tg < V) ? tgt_logit[row] - lse : 0.f;
    }
}

// C[m][n] += sum_z ws[z][m][n], z in slice order (fixed: the sum does not depend on which block finished first); 4 floats per thread
__global__ __launch_bounds__(256) void splitk_reduce_acc_kernel(const float* ws, float* C, long long ldc, int M, int N, int ks, long long zstride) {
    const int nq = N >> 2;
    const long long total = (long long)M * nq;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int m = (int)(i / nq), c = (int)(i - (long long)m * nq) * 4;
        const float* src = ws + (long long)m * N + c;
        f32x4_t a = *(const f32x4_t*)src;
        for (int z = 1; z < ks; ++z) a += *(const f32x4_t*)(src + z * zstride);
        float* dst = C + (long long)m * ldc + c;
        *(f32x4_t*)dst = *(const f32x4_t*)dst + a;
    }
}

__device__ char g_zero16[64] __attribute__((aligned(64)));

}  // namespace

static const void* zeros_ptr() {
    static void* z = nullptr;
    if (!z) (void)hipGetSymbolAddress(&z, HIP_SYMBOL(g_zero16));
    return z;
}

extern "C" int iadr1_gemm_nt_bf16(const void* A, const void* B, void* C, const void* bias, int M, int N, int K,
                                  long long lda, long long ldb, long long ldc, int out_mode, int act, hipStream_t stream) {
    IADR1_REQUIRE(M > 0 && N > 0 && K > 0, "gemm_nt: empty problem M=%d N=%d K=%d", M, N, K);
    IADR1_REQUIRE((K % 8) == 0 && (lda % 8) == 0 && (ldb % 8) == 0, "gemm_nt: K, lda, ldb must be multiples of 8 (16-byte chunks); K=%d lda=%lld ldb=%lld", K, lda, ldb);
    IADR1_REQUIRE((((uintptr_t)A) & 15) == 0 && (((uintptr_t)B) & 15) == 0, "gemm_nt: A/B must be 16-byte aligned");
    IADR1_REQUIRE(out_mode >= 0 && out_mode <= 2, "gemm_nt: bad out_mode %d", out_mode);
    constexpr int band_rows = 4;      // tile rows per rasterisation band: 1 / 2 / 4 / 8 measured within 4 % on the hot shapes, 4 best (profiles/r05_gemm_band.txt)
    GemmArgs p{(const bf16_t*)A, (const bf16_t*)B, C, (const bf16_t*)bias, zeros_ptr(), M, N, K, lda, ldb, ldc, act, band_rows, nullptr, 0};
    static const bool attr_done = [] {
        (void)hipFuncSetAttribute((const void*)gemm_nt_128<OUT_BF16>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_BYTES);
        (void)hipFuncSetAttribute((const void*)gemm_nt_128<OUT_F32>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_BYTES);
        (void)hipFuncSetAttribute((const void*)gemm_nt_128<OUT_F32_ACC>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM_BYTES);
        (void)hipFuncSetAttribute((const void*)gemm_nt_256<OUT_BF16>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM2_BYTES);
        (void)hipFuncSetAttribute((const void*)gemm_nt_256<OUT_F32>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM2_BYTES);
        (void)hipFuncSetAttribute((const void*)gemm_nt_256<OUT_F32_ACC>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM2_BYTES);
        return true;
    }();
    (void)attr_done;
    // 256^2 deep-pipeline kernel when the grid fills the chip with big tiles; 128^2 kernel for small / ragged problems
    const long long tiles256 = (long long)((M + T2 - 1) / T2) * ((N + T2 - 1) / T2);
    const bool big = M >= 512 && N >= 512 && tiles256 >= 192;
    if (big) {
        const int grid = (int)tiles256;
        if (out_mode == 0) hipLaunchKernelGGL(gemm_nt_256<OUT_BF16>, dim3(grid), dim3(NT2), SMEM2_BYTES, stream, p);
        else if (out_mode == 1) hipLaunchKernelGGL(gemm_nt_256<OUT_F32>, dim3(grid), dim3(NT2), SMEM2_BYTES, stream, p);
        else hipLaunchKernelGGL(gemm_nt_256<OUT_F32_ACC>, dim3(grid), dim3(NT2), SMEM2_BYTES, stream, p);
        return iadr1_check_launch("gemm_nt_bf16");
    }
    const int grid = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
    if (out_mode == 0) hipLaunchKernelGGL(gemm_nt_128<OUT_BF16>, dim3(grid), dim3(NTHREADS), SMEM_BYTES, stream, p);
    else if (out_mode == 1) hipLaunchKernelGGL(gemm_nt_128<OUT_F32>, dim3(grid), dim3(NTHREADS), SMEM_BYTES, stream, p);
    else hipLaunchKernelGGL(gemm_nt_128<OUT_F32_ACC>, dim3(grid), dim3(NTHREADS), SMEM_BYTES, stream, p);
    return iadr1_check_launch("gemm_nt_bf16");
}

// Split-K form of the accumulate mode for contractions with FEW output tiles and a long K -- the weight gradients of the narrow projections
// (dW_o [2048 x 2048], dW_qkv [2560 x 2048] over K = 20480 token rows: 64 / 80 tiles of 256^2 on 256 CUs ran at 310 / 612 TFLOP/s), the down projection's
// (344 tiles: 1.3 rounds) and the vision tower's: ksplit K slices per tile fill the chip, fp32 partial tiles go to a workspace, a second launch adds them
// to C in slice order (no atomics: bit-reproducible, and equal to the un-split kernel up to fp32 summation order).
extern "C" long long iadr1_gemm_nt_splitk_workspace_bytes(int M, int N, int ksplit) {
    return (M <= 0 || N <= 0 || ksplit <= 1) ? 0 : (long long)ksplit * M * N * 4;
}

extern "C" int iadr1_gemm_nt_splitk_acc_bf16(const void* A, const void* B, float* C, void* workspace, int M, int N, int K, long long lda, long long ldb, long long ldc,
                                             int ksplit, hipStream_t stream) {
    IADR1_REQUIRE(M > 0 && N > 0 && K > 0 && ksplit >= 2, "gemm_nt_splitk: empty problem / ksplit < 2 (M=%d N=%d K=%d ksplit=%d)", M, N, K, ksplit);
    IADR1_REQUIRE((K % 8) == 0 && (lda % 8) == 0 && (ldb % 8) == 0 && (N % 4) == 0 && (ldc % 4) == 0, "gemm_nt_splitk: K, lda, ldb multiples of 8, N, ldc multiples of 4");
    IADR1_REQUIRE((((uintptr_t)A) & 15) == 0 && (((uintptr_t)B) & 15) == 0 && (((uintptr_t)C) & 15) == 0 && workspace && (((uintptr_t)workspace) & 15) == 0,
                  "gemm_nt_splitk: A, B, C and the workspace must be 16-byte aligned");
    const int kslice = ((K + ksplit - 1) / ksplit + BK - 1) / BK * BK;      // whole 64-deep K tiles per slice
    IADR1_REQUIRE((long long)(ksplit - 1) * kslice < K, "gemm_nt_splitk: ksplit %d leaves an empty slice for K = %d", ksplit, K);
    constexpr int band_rows = 4;      // tile rows per rasterisation band: 1 / 2 / 4 / 8 measured within 4 % on the hot shapes, 4 best (profiles/r05_gemm_band.txt)
    GemmArgs p{(const bf16_t*)A, (const bf16_t*)B, workspace, nullptr, zeros_ptr(), M, N, K, lda, ldb, (long long)N, 0, band_rows, nullptr, 0};
    p.ksplit = ksplit; p.kslice = kslice; p.zstride = (long long)M * N;
    static const bool attr_done = [] { (void)hipFuncSetAttribute((const void*)gemm_nt_256<OUT_F32>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM2_BYTES); return true; }();
    (void)attr_done;
    const int tiles = ((M + T2 - 1) / T2) * ((N + T2 - 1) / T2);
    hipLaunchKernelGGL(gemm_nt_256<OUT_F32>, dim3(tiles * ksplit), dim3(NT2), SMEM2_BYTES, stream, p);
    if (int rc = iadr1_check_launch("gemm_nt_splitk (partials)")) return rc;
    long long blocks = ((long long)M * (N / 4) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(splitk_reduce_acc_kernel, dim3((int)blocks), dim3(256), 0, stream, (const float*)workspace, C, ldc, M, N, ksplit, (long long)M * N);
    return iadr1_check_launch("gemm_nt_splitk (reduce)");
}

// Weight gradients without transposed copies:  C[M, N] (fp32) += A[K, M]^T . B[K, N]  with A (= dY) and B (= X) row-major as the backward holds them, the contraction
// over their K rows (gemm_nt_256<.., TN = true>).  ksplit >= 2: the split form above (K slices of whole 64-row tiles, fp32 partial tiles in `workspace` --
// iadr1_gemm_nt_splitk_workspace_bytes(M, N, ksplit) -- added to C in slice order); ksplit <= 1: one accumulating launch.  Bit-equal to iadr1_gemm_nt_bf16 /
// iadr1_gemm_nt_splitk_acc_bf16 on transposed copies (same tiles, same order of the contraction).
extern "C" int iadr1_gemm_tn_acc_bf16(const void* A, const void* B, float* C, void* workspace, int M, int N, int K, long long lda, long long ldb, long long ldc,
                                      int ksplit, hipStream_t stream) {
    IADR1_REQUIRE(M >= 256 && N >= 256 && K > 0, "gemm_tn: needs M >= 256, N >= 256, K > 0 (M=%d N=%d K=%d)", M, N, K);
    IADR1_REQUIRE((M % 8) == 0 && (N % 8) == 0 && (lda % 8) == 0 && (ldb % 8) == 0 && (N % 4) == 0 && (ldc % 4) == 0, "gemm_tn: M, N, lda, ldb multiples of 8, ldc a multiple of 4");
    IADR1_REQUIRE((((uintptr_t)A) & 15) == 0 && (((uintptr_t)B) & 15) == 0 && (((uintptr_t)C) & 15) == 0, "gemm_tn: A, B, C must be 16-byte aligned");
    constexpr int band_rows = 4;      // tile rows per rasterisation band: 1 / 2 / 4 / 8 measured within 4 % on the hot shapes, 4 best (profiles/r05_gemm_band.txt)
    static const bool attr_done = [] {
        (void)hipFuncSetAttribute((const void*)gemm_nt_256<OUT_F32, true>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM2_BYTES);
        (void)hipFuncSetAttribute((const void*)gemm_nt_256<OUT_F32_ACC, true>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM2_BYTES);
        return true;
    }();
    (void)attr_done;
    const int tiles = ((M + T2 - 1) / T2) * ((N + T2 - 1) / T2);
    if (ksplit <= 1) {
        GemmArgs p{(const bf16_t*)A, (const bf16_t*)B, C, nullptr, zeros_ptr(), M, N, K, lda, ldb, ldc, 0, band_rows, nullptr, 0};
        hipLaunchKernelGGL((gemm_nt_256<OUT_F32_ACC, true>), dim3(tiles), dim3(NT2), SMEM2_BYTES, stream, p);
        return iadr1_check_launch("gemm_tn_acc_bf16");
    }
    IADR1_REQUIRE(workspace && (((uintptr_t)workspace) & 15) == 0, "gemm_tn: the split form needs a 16-byte aligned workspace");
    const int kslice = ((K + ksplit - 1) / ksplit + BK - 1) / BK * BK;      // whole 64-row K tiles per slice
    IADR1_REQUIRE((long long)(ksplit - 1) * kslice < K, "gemm_tn: ksplit %d leaves an empty slice for K = %d", ksplit, K);
    GemmArgs p{(const bf16_t*)A, (const bf16_t*)B, workspace, nullptr, zeros_ptr(), M, N, K, lda, ldb, (long long)N, 0, band_rows, nullptr, 0};
    p.ksplit = ksplit; p.kslice = kslice; p.zstride = (long long)M * N;
    hipLaunchKernelGGL((gemm_nt_256<OUT_F32, true>), dim3(tiles * ksplit), dim3(NT2), SMEM2_BYTES, stream, p);
    if (int rc = iadr1_check_launch("gemm_tn (partials)")) return rc;
    long long blocks = ((long long)M * (N / 4) + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(splitk_reduce_acc_kernel, dim3((int)blocks), dim3(256), 0, stream, (const float*)workspace, C, ldc, M, N, ksplit, (long long)M * N);
    return iadr1_check_launch("gemm_tn (reduce)");
}

// linear_logprob: logp[r] = log_softmax(H[r] . W^T)[targets[r]] and lse[r] without the [M, V] logits ever reaching HBM (gemm_nt_256 with the OUT_LSE
// epilogue + lse_combine_kernel), and its backward's first half: dlogits (bf16) from the recomputed logits (OUT_DLOGITS epilogue).
extern "C" long long iadr1_linear_logprob_workspace_bytes(int M, int V) {
    if (M <= 0 || V <= 0) return 0;
    const long long nparts = (long long)((V + T2 - 1) / T2) * 4;
    return (long long)M * nparts * 8 + (long long)M * 4;
}

static int linear_logprob_args(const char* what, const void* H, const void* W, int M, int V, int K, long long ldh, long long ldw) {
    IADR1_REQUIRE(M > 0 && V > 0 && K > 0, "%s: empty problem M=%d V=%d K=%d", what, M, V, K);
    IADR1_REQUIRE((K % 8) == 0 && (ldh % 8) == 0 && (ldw % 8) == 0, "%s: K, ldh, ldw must be multiples of 8 (16-byte chunks); K=%d ldh=%lld ldw=%lld", what, K, ldh, ldw);
    IADR1_REQUIRE((((uintptr_t)H) & 15) == 0 && (((uintptr_t)W) & 15) == 0, "%s: H/W must be 16-byte aligned", what);
    return 0;
}

// The two forms of each entry point are one function: `what` is the entry point's name (the prefix of its refusals), temperature 1 the plain form's.
static int linear_logprob_temperature(const char* what, float temperature) {
    IADR1_REQUIRE(temperature > 0.f && temperature <= 3.402823466e38f, "%s: temperature must be finite and > 0 (got %g)", what, (double)temperature);
    return 0;
}

static int linear_logprob_fwd(const char* what, const char* what_combine, const void* H, const void* W, const long long* targets, float* logp, float* lse, void* workspace, int M, int V, int K,
                              long long ldh, long long ldw, float temperature, hipStream_t stream) {
    if (int rc = linear_logprob_temperature(what, temperature)) return rc;
    if (int rc = linear_logprob_args(what, H, W, M, V, K, ldh, ldw)) return rc;
    IADR1_REQUIRE(targets && logp && workspace && (((uintptr_t)workspace) & 7) == 0, "%s: targets, logp and an 8-byte aligned workspace are required", what);
    constexpr int band_rows = 4;      // tile rows per rasterisation band: 1 / 2 / 4 / 8 measured within 4 % on the hot shapes, 4 best (profiles/r05_gemm_band.txt)
    const int tiles_n = (V + T2 - 1) / T2, nparts = tiles_n * 4;
    float* part = (float*)workspace;
    float* tgt_logit = part + (long long)M * nparts * 2;
    GemmArgs p{(const bf16_t*)H, (const bf16_t*)W, nullptr, nullptr, zeros_ptr(), M, V, K, ldh, ldw, 0, 0, band_rows, nullptr, 0, targets, part, tgt_logit, nullptr, nullptr, nparts};
    p.inv_t = 1.0f / temperature;
    static const bool attr_done = [] { (void)hipFuncSetAttribute((const void*)gemm_nt_256<OUT_LSE>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM2_BYTES); return true; }();
    (void)attr_done;
    hipLaunchKernelGGL(gemm_nt_256<OUT_LSE>, dim3(((M + T2 - 1) / T2) * tiles_n), dim3(NT2), SMEM2_BYTES, stream, p);
    if (int rc = iadr1_check_launch(what)) return rc;
    hipLaunchKernelGGL(lse_combine_kernel, dim3((M + 3) / 4), dim3(256), 0, stream, part, tgt_logit, targets, logp, lse, M, V, nparts);
    return iadr1_check_launch(what_combine);
}

static int linear_logprob_dlogits(const char* what, const void* H, const void* W, const long long* targets, const float* lse, const float* g, void* dl, long long ldd, int M,
                                  int V, int K, long long ldh, long long ldw, float temperature, hipStream_t stream) {
    if (int rc = linear_logprob_temperature(what, temperature)) return rc;
    if (int rc = linear_logprob_args(what, H, W, M, V, K, ldh, ldw)) return rc;
    IADR1_REQUIRE(targets && lse && g && dl, "%s: targets, lse, g and dl are required", what);
    constexpr int band_rows = 4;      // tile rows per rasterisation band: 1 / 2 / 4 / 8 measured within 4 % on the hot shapes, 4 best (profiles/r05_gemm_band.txt)
    GemmArgs p{(const bf16_t*)H, (const bf16_t*)W, dl, nullptr, zeros_ptr(), M, V, K, ldh, ldw, ldd, 0, band_rows, nullptr, 0, targets, nullptr, nullptr, lse, g, 0};
    p.inv_t = 1.0f / temperature;
    static const bool attr_done = [] { (void)hipFuncSetAttribute((const void*)gemm_nt_256<OUT_DLOGITS>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM2_BYTES); return true; }();
    (void)attr_done;
    hipLaunchKernelGGL(gemm_nt_256<OUT_DLOGITS>, dim3(((M + T2 - 1) / T2) * ((V + T2 - 1) / T2)), dim3(NT2), SMEM2_BYTES, stream, p);
    return iadr1_check_launch(what);
}

extern "C" int iadr1_linear_logprob_fwd(const void* H, const void* W, const long long* targets, float* logp, float* lse, void* workspace, int M, int V, int K,
                                        long long ldh, long long ldw, hipStream_t stream) {
    return linear_logprob_fwd("linear_logprob_fwd", "linear_logprob_fwd (combine)", H, W, targets, logp, lse, workspace, M, V, K, ldh, ldw, 1.f, stream);
}

extern "C" int iadr1_linear_logprob_dlogits(const void* H, const void* W, const long long* targets, const float* lse, const float* g, void* dl, long long ldd, int M, int V,
                                            int K, long long ldh, long long ldw, hipStream_t stream) {
    return linear_logprob_dlogits("linear_logprob_dlogits", H, W, targets, lse, g, dl, ldd, M, V, K, ldh, ldw, 1.f, stream);
}

// The same pair on y = x / temperature (REF:trl/trl/trainer/grpo_trainer.py:818-821: trl scores the policy, the old policy and the reference on logits / temperature):
// lse = logsumexp(y), logp = y[target] - lse, dl = (g / T) * (onehot - exp(y - lse)).  The same two kernels; temperature 1 gives the plain pair's bits.
extern "C" int iadr1_linear_logprob_fwd_t(const void* H, const void* W, const long long* targets, float* logp, float* lse, void* workspace, int M, int V, int K,
                                          long long ldh, long long ldw, float temperature, hipStream_t stream) {
    return linear_logprob_fwd("linear_logprob_fwd_t", "linear_logprob_fwd_t (combine)", H, W, targets, logp, lse, workspace, M, V, K, ldh, ldw, temperature, stream);
}

extern "C" int iadr1_linear_logprob_dlogits_t(const void* H, const void* W, const long long* targets, const float* lse, const float* g, void* dl, long long ldd, int M,
                                              int V, int K, long long ldh, long long ldw, float temperature, hipStream_t stream) {
    return linear_logprob_dlogits("linear_logprob_dlogits_t", H, W, targets, lse, g, dl, ldd, M, V, K, ldh, ldw, temperature, stream);
}

// gate|up projection with the SwiGLU fused into the epilogue of gemm_nt_256 (training / prefill shapes): GU[M, 2I] = A . W^T (stored when GU != null:
// the backward pass needs it) and Aout[M, I] = bf16(silu(GU[:, :I])) * GU[:, I:], bit-identical to iadr1_gemm_nt_bf16 + iadr1_swiglu_fwd.
extern "C" int iadr1_gemm_swiglu_bf16(const void* A, const void* W, void* GU, void* Aout, int M, int I, int K, long long lda, long long ldw,
                                      long long ldgu, long long ldaout, hipStream_t stream) {
    IADR1_REQUIRE(M > 0 && I > 0 && K > 0 && Aout != nullptr, "gemm_swiglu: empty problem");
    IADR1_REQUIRE((M % 256) == 0 && (I % 128) == 0 && (K % 8) == 0 && (lda % 8) == 0 && (ldw % 8) == 0 && (ldaout % 8) == 0 && (GU == nullptr || (ldgu % 8) == 0),
                  "gemm_swiglu: needs M %% 256 == 0, I %% 128 == 0 and 16-byte row strides (M=%d I=%d K=%d); use gemm_nt + swiglu_fwd otherwise", M, I, K);
    IADR1_REQUIRE((((uintptr_t)A) & 15) == 0 && (((uintptr_t)W) & 15) == 0 && (((uintptr_t)GU) & 15) == 0 && (((uintptr_t)Aout) & 15) == 0, "gemm_swiglu: operands must be 16-byte aligned");
    constexpr int band_rows = 4;      // tile rows per rasterisation band: 1 / 2 / 4 / 8 measured within 4 % on the hot shapes, 4 best (profiles/r05_gemm_band.txt)
    GemmArgs p{(const bf16_t*)A, (const bf16_t*)W, GU, nullptr, zeros_ptr(), M, 2 * I, K, lda, ldw, ldgu, 0, band_rows, (bf16_t*)Aout, ldaout};
    static const bool attr_done = [] { (void)hipFuncSetAttribute((const void*)gemm_nt_256<OUT_SWIGLU>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM2_BYTES); return true; }();
    (void)attr_done;
    hipLaunchKernelGGL(gemm_nt_256<OUT_SWIGLU>, dim3((M / 256) * (I / 128)), dim3(NT2), SMEM2_BYTES, stream, p);
    return iadr1_check_launch("gemm_swiglu_bf16");
}

// The same contraction over ROW BLOCKS of a larger matrix: GEMM row r (0 <= r < M) is row (r / block) * block_stride + r % block of A, GU and Aout (block a power
// of two >= 16, all three matrices addressed from the given base pointers).  Per row the arithmetic is iadr1_gemm_swiglu_bf16's, bit for bit.
extern "C" int iadr1_gemm_swiglu_rows_bf16(const void* A, const void* W, void* GU, void* Aout, int M, int I, int K, long long lda, long long ldw,
                                           long long ldgu, long long ldaout, int block, long long block_stride, hipStream_t stream) {
    IADR1_REQUIRE(M > 0 && I > 0 && K > 0 && Aout != nullptr, "gemm_swiglu_rows: empty problem");
    IADR1_REQUIRE((M % 256) == 0 && (I % 128) == 0 && (K % 8) == 0 && (lda % 8) == 0 && (ldw % 8) == 0 && (ldaout % 8) == 0 && (GU == nullptr || (ldgu % 8) == 0),
                  "gemm_swiglu_rows: needs M %% 256 == 0, I %% 128 == 0 and 16-byte row strides (M=%d I=%d K=%d)", M, I, K);
    IADR1_REQUIRE(block >= 16 && (block & (block - 1)) == 0 && (M % block) == 0 && block_stride >= block, "gemm_swiglu_rows: block must be a power of two >= 16 dividing M, block_stride >= block (block=%d)", block);
    IADR1_REQUIRE((((uintptr_t)A) & 15) == 0 && (((uintptr_t)W) & 15) == 0 && (((uintptr_t)GU) & 15) == 0 && (((uintptr_t)Aout) & 15) == 0, "gemm_swiglu_rows: operands must be 16-byte aligned");
    constexpr int band_rows = 4;      // tile rows per rasterisation band: 1 / 2 / 4 / 8 measured within 4 % on the hot shapes, 4 best (profiles/r05_gemm_band.txt)
    GemmArgs p{(const bf16_t*)A, (const bf16_t*)W, GU, nullptr, zeros_ptr(), M, 2 * I, K, lda, ldw, ldgu, 0, band_rows, (bf16_t*)Aout, ldaout};
    p.rb_shift = __builtin_ctz((unsigned)block);
    p.rb_stride = block_stride;
    static const bool attr_done = [] { (void)hipFuncSetAttribute((const void*)gemm_nt_256<OUT_SWIGLU_ROWS>, hipFuncAttributeMaxDynamicSharedMemorySize, SMEM2_BYTES); return true; }();
    (void)attr_done;
    hipLaunchKernelGGL(gemm_nt_256<OUT_SWIGLU_ROWS>, dim3((M / 256) * (I / 128)), dim3(NT2), SMEM2_BYTES, stream, p);
    return iadr1_check_launch("gemm_swiglu_rows_bf16");
}
