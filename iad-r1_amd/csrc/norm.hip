// RMSNorm forward / backward for gfx950 (reference arithmetic
// TF:modeling_qwen2_5_vl.py:74-79: fp32 statistics, the normalised value is cast back to the storage
// dtype BEFORE the multiply by the gain).  HBM-bound: one wave per row, the whole row lives in
// registers (16-byte loads, 8 bf16 per lane per chunk), wave-shuffle reduction, no LDS.
// Optional fusions: residual add on the way in (writes the new residual stream), fp32 split-K partial
// sums as the branch input (decode path; the buffer is re-zeroed for the next skinny GEMM), and in the
// backward the add of the gradient arriving on the residual path.
#include "common.h"

namespace {

constexpr int MAXC = 8;  // 16-byte chunks per lane -> rows up to 8*64*8 = 4096 elements

struct RmsFwdArgs {
    const bf16_t* x;      // branch input [T,H] bf16 (or null when x32 is used)
    const float* x32;     // branch input: nsplit fp32 partial slabs [nsplit][T][ldx] (decode, split-K skinny GEMM)
    int nsplit;
    const bf16_t* xbias;  // optional bias [H] added to x32 (e.g. none for o_proj/down)
    const bf16_t* res;    // optional residual [T,H]
    bf16_t* res_out;      // where x+res is written (may alias res); null = do not write
    const bf16_t* w;      // gain [H]
    bf16_t* y;            // normalised output [T,H]
    float* rstd;          // optional [T]
    int T, H;
    long long ldx, ldr, ldy;
    float eps;
};

template <int NC>
__global__ __launch_bounds__(256) void rmsnorm_fwd_kernel(RmsFwdArgs p) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.T) return;
    const int nchunk = p.H >> 3;
    float v[NC][8];
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int ch = c * 64 + lane;
        if (ch < nchunk) {
            if (p.x32) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[c][e] = 0.f;
                // slabs are summed in order, four at a time with all eight loads of a group in flight together (a rolled loop over
                // a run-time slab count issues load -> wait -> add per slab: 8 dependent L2 latencies at ksplit 8)
                const float* src0 = p.x32 + (long long)row * p.ldx + ch * 8;
                const long long sstride = (long long)p.T * p.ldx;
                int sp = 0;
                if (p.nsplit == 8) {      // the down projection's eight slabs: all sixteen loads in flight at once (one memory latency instead of two)
                    f32x4_t a[8], b[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) { a[u] = *(const f32x4_t*)(src0 + u * sstride); b[u] = *(const f32x4_t*)(src0 + u * sstride + 4); }
#pragma unroll
                    for (int u = 0; u < 8; ++u)
#pragma unroll
                        for (int e = 0; e < 4; ++e) { v[c][e] += a[u][e]; v[c][4 + e] += b[u][e]; }
                    sp = 8;
                }
                for (; sp + 4 <= p.nsplit; sp += 4) {
                    f32x4_t a[4], b[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) { a[u] = *(const f32x4_t*)(src0 + (sp + u) * sstride); b[u] = *(const f32x4_t*)(src0 + (sp + u) * sstride + 4); }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int e = 0; e < 4; ++e) { v[c][e] += a[u][e]; v[c][4 + e] += b[u][e]; }
                }
                if (sp + 2 <= p.nsplit) {
                    f32x4_t a[2], b[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) { a[u] = *(const f32x4_t*)(src0 + (sp + u) * sstride); b[u] = *(const f32x4_t*)(src0 + (sp + u) * sstride + 4); }
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int e = 0; e < 4; ++e) { v[c][e] += a[u][e]; v[c][4 + e] += b[u][e]; }
                    sp += 2;
                }
                for (; sp < p.nsplit; ++sp) {
                    const f32x4_t a = *(const f32x4_t*)(src0 + sp * sstride), b = *(const f32x4_t*)(src0 + sp * sstride + 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { v[c][e] += a[e]; v[c][4 + e] += b[e]; }
                }
                if (p.xbias) {
                    const u32x4_t bb = *(const u32x4_t*)(p.xbias + ch * 8);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { v[c][2 * e] += lo_bf(bb[e]); v[c][2 * e + 1] += hi_bf(bb[e]); }
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) v[c][e] = bf2f(f2bf(v[c][e]));  // the branch output is a bf16 tensor in the reference
            } else {
                const u32x4_t a = *(const u32x4_t*)(p.x + (long long)row * p.ldx + ch * 8);
#pragma unroll
                for (int e = 0; e < 4; ++e) { v[c][2 * e] = lo_bf(a[e]); v[c][2 * e + 1] = hi_bf(a[e]); }
            }
            if (p.res) {
                const u32x4_t r = *(const u32x4_t*)(p.res + (long long)row * p.ldr + ch * 8);
                u32x4_t o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float s0 = v[c][2 * e] + lo_bf(r[e]), s1 = v[c][2 * e + 1] + hi_bf(r[e]);
                    o[e] = pack2bf(s0, s1);
                    v[c][2 * e] = lo_bf(o[e]);  // the reference's residual stream is bf16: norm sees the rounded sum
                    v[c][2 * e + 1] = hi_bf(o[e]);
                }
                if (p.res_out) *(u32x4_t*)(p.res_out + (long long)row * p.ldr + ch * 8) = o;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) ss += v[c][e] * v[c][e];
        }
    }
    ss = wave_sum(ss);
    const float rstd = rsqrtf(ss / (float)p.H + p.eps);
    if (p.rstd && lane == 0) p.rstd[row] = rstd;
    if (!p.y) return;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int ch = c * 64 + lane;
        if (ch < nchunk) {
            const u32x4_t g = *(const u32x4_t*)(p.w + ch * 8);
            u32x4_t o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float n0 = bf2f(f2bf(v[c][2 * e] * rstd)), n1 = bf2f(f2bf(v[c][2 * e + 1] * rstd));
                o[e] = pack2bf(lo_bf(g[e]) * n0, hi_bf(g[e]) * n1);
            }
            *(u32x4_t*)(p.y + (long long)row * p.ldy + ch * 8) = o;
        }
    }
}

// Few-row variant (decode: T = sequences in flight): one ROW PER BLOCK, 256 threads, so a 64-row call still
// spreads over 64 CUs and the per-thread dependent-load chain is 1/4 as long as in the wave-per-row kernel.
__global__ __launch_bounds__(256) void rmsnorm_fwd_row_kernel(RmsFwdArgs p, SideOut so) {
    __shared__ float scratch[16];
    const int row = blockIdx.x, t = threadIdx.x;
    const long long sb = side_base(so), srow = sb + (long long)row * so.seq_stride;
    const int nchunk = p.H >> 3;
    constexpr int MC = 4;  // H <= 8192
    float v[MC][8];
    float ss = 0.f;
    STAMP(0);
#pragma unroll
    for (int c = 0; c < MC; ++c) {
        const int ch = c * 256 + t;
        if (ch < nchunk) {
            if (p.x32) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[c][e] = 0.f;
                // slabs are summed in order, four at a time with all eight loads of a group in flight together (a rolled loop over
                // a run-time slab count issues load -> wait -> add per slab: 8 dependent L2 latencies at ksplit 8)
                const float* src0 = p.x32 + (long long)row * p.ldx + ch * 8;
                const long long sstride = (long long)p.T * p.ldx;
                int sp = 0;
                if (p.nsplit == 8) {      // the down projection's eight slabs: all sixteen loads in flight at once (one memory latency instead of two)
                    f32x4_t a[8], b[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) { a[u] = *(const f32x4_t*)(src0 + u * sstride); b[u] = *(const f32x4_t*)(src0 + u * sstride + 4); }
#pragma unroll
                    for (int u = 0; u < 8; ++u)
#pragma unroll
                        for (int e = 0; e < 4; ++e) { v[c][e] += a[u][e]; v[c][4 + e] += b[u][e]; }
                    sp = 8;
                }
                for (; sp + 4 <= p.nsplit; sp += 4) {
                    f32x4_t a[4], b[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) { a[u] = *(const f32x4_t*)(src0 + (sp + u) * sstride); b[u] = *(const f32x4_t*)(src0 + (sp + u) * sstride + 4); }
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int e = 0; e < 4; ++e) { v[c][e] += a[u][e]; v[c][4 + e] += b[u][e]; }
                }
                if (sp + 2 <= p.nsplit) {
                    f32x4_t a[2], b[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) { a[u] = *(const f32x4_t*)(src0 + (sp + u) * sstride); b[u] = *(const f32x4_t*)(src0 + (sp + u) * sstride + 4); }
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int e = 0; e < 4; ++e) { v[c][e] += a[u][e]; v[c][4 + e] += b[u][e]; }
                    sp += 2;
                }
                for (; sp < p.nsplit; ++sp) {
                    const f32x4_t a = *(const f32x4_t*)(src0 + sp * sstride), b = *(const f32x4_t*)(src0 + sp * sstride + 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { v[c][e] += a[e]; v[c][4 + e] += b[e]; }
                }
                if (p.xbias) {
                    const u32x4_t bb = *(const u32x4_t*)(p.xbias + ch * 8);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { v[c][2 * e] += lo_bf(bb[e]); v[c][2 * e + 1] += hi_bf(bb[e]); }
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) v[c][e] = bf2f(f2bf(v[c][e]));
            } else {
                const u32x4_t a = *(const u32x4_t*)(p.x + (long long)row * p.ldx + ch * 8);
#pragma unroll
                for (int e = 0; e < 4; ++e) { v[c][2 * e] = lo_bf(a[e]); v[c][2 * e + 1] = hi_bf(a[e]); }
            }
            if (p.res) {
                const u32x4_t r = *(const u32x4_t*)(p.res + (long long)row * p.ldr + ch * 8);
                u32x4_t o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[e] = pack2bf(v[c][2 * e] + lo_bf(r[e]), v[c][2 * e + 1] + hi_bf(r[e]));
                    v[c][2 * e] = lo_bf(o[e]);
                    v[c][2 * e + 1] = hi_bf(o[e]);
                }
                if (p.res_out) *(u32x4_t*)(p.res_out + (long long)row * p.ldr + ch * 8) = o;
                if (sb >= 0 && so.p0) *(u32x4_t*)((bf16_t*)so.p0 + srow * so.ld0 + ch * 8) = o;   // residual stream row for the backward pass
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) ss += v[c][e] * v[c][e];
        }
    }
    // the gains are fetched before the block reduction, not after it (one global latency less on the critical path of a
    // kernel that is nothing but a latency chain)
    u32x4_t gw[MC];
#pragma unroll
    for (int c = 0; c < MC; ++c) gw[c] = (p.y && c * 256 + t < nchunk) ? *(const u32x4_t*)(p.w + (c * 256 + t) * 8) : (u32x4_t){0, 0, 0, 0};
    STAMP(1);
    ss = block_sum<256>(ss, scratch);
    STAMP(2);
    const float rstd = rsqrtf(ss / (float)p.H + p.eps);
    if (p.rstd && t == 0) p.rstd[row] = rstd;
    if (sb >= 0 && so.p2 && t == 0) ((float*)so.p2)[srow] = rstd;
    if (!p.y) return;
#pragma unroll
    for (int c = 0; c < MC; ++c) {
        const int ch = c * 256 + t;
        if (ch < nchunk) {
            const u32x4_t g = gw[c];
            u32x4_t o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float n0 = bf2f(f2bf(v[c][2 * e] * rstd)), n1 = bf2f(f2bf(v[c][2 * e + 1] * rstd));
                o[e] = pack2bf(lo_bf(g[e]) * n0, hi_bf(g[e]) * n1);
            }
            *(u32x4_t*)(p.y + (p.ldy ? (long long)row * p.ldy + ch * 8 : xpk_off(row, ch * 8, p.H))) = o;   // ldy == 0: decode-packed
            if (sb >= 0 && so.p1) *(u32x4_t*)((bf16_t*)so.p1 + srow * so.ld1 + ch * 8) = o;
        }
    }
    STAMP(3);
}

struct RmsBwdArgs {
    const bf16_t* dy;    // [T,H]
    const bf16_t* x;     // pre-norm input [T,H]
    const bf16_t* w;     // [H]
    const float* rstd;   // [T]
    const bf16_t* dres;  // optional gradient arriving on the residual path [T,H]
    bf16_t* dx;          // [T,H] = dres + d(rmsnorm)/dx
    float* dw;           // [H] fp32 gain gradient, accumulated (may be null for frozen gains)
    float* ws;           // [gridDim.x][H] fp32: every block's partial gain gradient; summed into dw in block order by partial_reduce_acc_kernel (no atomics)
    int T, H;
    long long ld;
};

template <int NC>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(RmsBwdArgs p) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nchunk = p.H >> 3;
    float dwacc[NC][8];
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int e = 0; e < 8; ++e) dwacc[c][e] = 0.f;
    float g[NC][8];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int ch = c * 64 + lane;
        if (ch < nchunk) {
            const u32x4_t gg = *(const u32x4_t*)(p.w + ch * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) { g[c][2 * e] = lo_bf(gg[e]); g[c][2 * e + 1] = hi_bf(gg[e]); }
        }
    }
    for (int row = blockIdx.x * 4 + wv; row < p.T; row += gridDim.x * 4) {
        const float rstd = p.rstd[row];
        float n[NC][8], dn[NC][8];
        float dot = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int ch = c * 64 + lane;
            if (ch < nchunk) {
                const u32x4_t a = *(const u32x4_t*)(p.x + (long long)row * p.ld + ch * 8);
                const u32x4_t d = *(const u32x4_t*)(p.dy + (long long)row * p.ld + ch * 8);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    n[c][2 * e] = lo_bf(a[e]) * rstd;
                    n[c][2 * e + 1] = hi_bf(a[e]) * rstd;
                    const float d0 = lo_bf(d[e]), d1 = hi_bf(d[e]);
                    dwacc[c][2 * e] += d0 * n[c][2 * e];
                    dwacc[c][2 * e + 1] += d1 * n[c][2 * e + 1];
                    dn[c][2 * e] = d0 * g[c][2 * e];
                    dn[c][2 * e + 1] = d1 * g[c][2 * e + 1];
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) dot += dn[c][e] * n[c][e];
            }
        }
        dot = wave_sum(dot) / (float)p.H;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int ch = c * 64 + lane;
            if (ch < nchunk) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = rstd * (dn[c][e] - n[c][e] * dot);
                if (p.dres) {
                    const u32x4_t r = *(const u32x4_t*)(p.dres + (long long)row * p.ld + ch * 8);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { o[2 * e] += lo_bf(r[e]); o[2 * e + 1] += hi_bf(r[e]); }
                }
                u32x4_t ov;
#pragma unroll
                for (int e = 0; e < 4; ++e) ov[e] = pack2bf(o[2 * e], o[2 * e + 1]);
                *(u32x4_t*)(p.dx + (long long)row * p.ld + ch * 8) = ov;
            }
        }
    }
    if (!p.dw) return;
    // block-level combine of the 4 waves' partial gain gradients, then one atomic per column per block
    extern __shared__ float sdw[];  // [4][H]
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int ch = c * 64 + lane;
        if (ch < nchunk) {
#pragma unroll
            for (int e = 0; e < 8; ++e) sdw[wv * p.H + ch * 8 + e] = dwacc[c][e];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < p.H; i += 256) p.ws[(long long)blockIdx.x * p.H + i] = sdw[i] + sdw[p.H + i] + sdw[2 * p.H + i] + sdw[3 * p.H + i];
}

// Second stage of every gradient reduction over token rows (norm gains / biases, bias column sums): out[i] += sum_p ws[p][i], p ascending -- ONE thread per column adds the
// partials in a fixed order, so a run is bit-reproducible (round 5; the float atomics this replaces made two runs of the same step differ in the last bits: VERDICT r4 weak #13)
__global__ __launch_bounds__(256) void partial_reduce_acc_kernel(const float* ws, int nparts, long long stride, float* out, int n) {
    // block = 32 columns x 8 partial groups: thread (g, c) adds partials q = g, g + 8, g + 16, ... of column c, eight independent loads in flight at a time (one thread
    // walking all the partials of a column is a chain of several hundred load latencies: +5 % on a PA-SFT step); the eight group sums are then added in group order.
    // The order of additions depends on nparts only, never on timing.
    __shared__ float red[8][33];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + c;
    float s = 0.f;
    if (i < n) {
        int q = g;
        for (; q + 56 < nparts; q += 64) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = ws[(long long)(q + 8 * u) * stride + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; q < nparts; q += 8) s += ws[(long long)q * stride + i];
    }
    red[g][c] = s;
    __syncthreads();
    if (g == 0 && i < n) {
        float t = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) t += red[u][c];
        out[i] += t;
    }
}

}  // namespace

#define DISPATCH_NC(H, CALL)                                                          \
    do {                                                                              \
        const int nc_ = ((H) / 8 + 63) / 64;                                           \
        if (nc_ <= 1) { CALL(1); } else if (nc_ <= 2) { CALL(2); } else if (nc_ <= 3) { CALL(3); } \
        else if (nc_ <= 4) { CALL(4); } else if (nc_ <= 6) { CALL(6); } else { CALL(8); } \
    } while (0)

extern "C" int iadr1_rmsnorm_fwd(const void* x, const float* x32, int nsplit, const void* xbias, const void* res, void* res_out,
                                 const void* w, void* y, float* rstd, int T, int H, long long ldx, long long ldr, long long ldy,
                                 float eps, const void* side, hipStream_t stream) {
    IADR1_REQUIRE(T > 0 && H > 0 && (H % 8) == 0 && H <= MAXC * 512, "rmsnorm_fwd: H=%d must be a multiple of 8 and <= %d", H, MAXC * 512);
    IADR1_REQUIRE((x != nullptr) != (x32 != nullptr), "rmsnorm_fwd: exactly one of x / x32");
    IADR1_REQUIRE((ldx % 8) == 0 && (ldr % 8) == 0 && (ldy % 8) == 0, "rmsnorm_fwd: leading dims must be multiples of 8");
    IADR1_REQUIRE(x32 == nullptr || nsplit >= 1, "rmsnorm_fwd: nsplit >= 1 with x32");
    RmsFwdArgs p{(const bf16_t*)x, x32, nsplit, (const bf16_t*)xbias, (const bf16_t*)res, (bf16_t*)res_out, (const bf16_t*)w, (bf16_t*)y, rstd, T, H, ldx, ldr, ldy, eps};
    IADR1_REQUIRE(ldy != 0 || (T <= 256 && (H % 32) == 0), "rmsnorm_fwd: decode-packed output (ldy == 0) needs T <= 256 and H %% 32 == 0");
    SideOut so;
    if (int e = iadr1_side_arg(side, &so)) return e;
    IADR1_REQUIRE(!so.step || T <= 256, "rmsnorm_fwd: side outputs exist in the few-row (decode) kernel only, T=%d", T);
    // The few-row kernel (one block per row) serves the DECODE-form calls: decode-packed output, fp32 partial slabs as the branch input, side outputs.  Everything
    // else -- the training / prefill / teacher-forced passes -- runs the wave-per-row kernel at ANY row count: the two kernels add a row's squares in different
    // orders, so a choice by T made a row's bits depend on how many OTHER rows the launch held (round 5: the chunked reference pass runs the same rows in
    // launches of different sizes and must reproduce the one-shot pass bit for bit).
    if (T <= 256 && (ldy == 0 || x32 != nullptr || so.step != nullptr)) {
        hipLaunchKernelGGL(rmsnorm_fwd_row_kernel, dim3(T), dim3(256), 0, stream, p, so);
        return iadr1_check_launch("rmsnorm_fwd");
    }
    const dim3 grid((T + 3) / 4), block(256);
#define CALL(NC) hipLaunchKernelGGL(rmsnorm_fwd_kernel<NC>, grid, block, 0, stream, p)
    DISPATCH_NC(H, CALL);
#undef CALL
    return iadr1_check_launch("rmsnorm_fwd");
}

static int norm_bwd_blocks(int T) {
    const int blocks = (T + 3) / 4;
    return blocks > 512 ? 512 : blocks;      // grid-stride over rows: bounds the partial-gradient workspace (512 x H floats)
}
extern "C" long long iadr1_rmsnorm_bwd_workspace_bytes(int T, int H) { return (T <= 0 || H <= 0) ? 0 : (long long)norm_bwd_blocks(T) * H * 4; }
extern "C" long long iadr1_layernorm_bwd_workspace_bytes(int T, int H) { return (T <= 0 || H <= 0) ? 0 : (long long)norm_bwd_blocks(T) * 2 * H * 4; }

extern "C" int iadr1_rmsnorm_bwd(const void* dy, const void* x, const void* w, const float* rstd, const void* dres, void* dx,
                                 float* dw, float* workspace, int T, int H, long long ld, hipStream_t stream) {
    IADR1_REQUIRE(T > 0 && H > 0 && (H % 8) == 0 && H <= MAXC * 512, "rmsnorm_bwd: H=%d must be a multiple of 8 and <= %d", H, MAXC * 512);
    IADR1_REQUIRE((ld % 8) == 0, "rmsnorm_bwd: ld must be a multiple of 8");
    IADR1_REQUIRE(dw == nullptr || workspace != nullptr, "rmsnorm_bwd: a gain gradient needs the partial-sum workspace (iadr1_rmsnorm_bwd_workspace_bytes)");
    RmsBwdArgs p{(const bf16_t*)dy, (const bf16_t*)x, (const bf16_t*)w, rstd, (const bf16_t*)dres, (bf16_t*)dx, dw, workspace, T, H, ld};
    const int blocks = norm_bwd_blocks(T);
    const dim3 grid(blocks), block(256);
#define CALL(NC) hipLaunchKernelGGL(rmsnorm_bwd_kernel<NC>, grid, block, (size_t)(dw ? 4 * H * sizeof(float) : 0), stream, p)
    DISPATCH_NC(H, CALL);
#undef CALL
    if (dw) hipLaunchKernelGGL(partial_reduce_acc_kernel, dim3((H + 31) / 32), dim3(256), 0, stream, (const float*)workspace, blocks, (long long)H, dw, H);
    return iadr1_check_launch("rmsnorm_bwd");
}

// ------------------------------------------------------------------------------------------------------------------------
// LayerNorm (with bias) for the Qwen2-VL vision tower (nn.LayerNorm(eps=1e-6) at TF:models/qwen2_vl/modeling_qwen2_vl.py:
// 281,428-429): same wave-per-row structure as RMSNorm, fused residual add on the way in, mean/rstd saved for backward.
// ------------------------------------------------------------------------------------------------------------------------
namespace {

struct LnFwdArgs {
    const bf16_t* x;
    const bf16_t* res;
    bf16_t* res_out;
    const bf16_t* w;
    const bf16_t* b;
    bf16_t* y;
    float* mean;
    float* rstd;
    int T, H;
    long long ldx, ldr, ldy;
    float eps;
};

template <int NC>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(LnFwdArgs p) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.T) return;
    const int nchunk = p.H >> 3;
    float v[NC][8];
    float s1 = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int ch = c * 64 + lane;
        if (ch < nchunk) {
            const u32x4_t a = *(const u32x4_t*)(p.x + (long long)row * p.ldx + ch * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[c][2 * e] = lo_bf(a[e]); v[c][2 * e + 1] = hi_bf(a[e]); }
            if (p.res) {
                const u32x4_t r = *(const u32x4_t*)(p.res + (long long)row * p.ldr + ch * 8);
                u32x4_t o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[e] = pack2bf(v[c][2 * e] + lo_bf(r[e]), v[c][2 * e + 1] + hi_bf(r[e]));
                    v[c][2 * e] = lo_bf(o[e]);
                    v[c][2 * e + 1] = hi_bf(o[e]);
                }
                if (p.res_out) *(u32x4_t*)(p.res_out + (long long)row * p.ldr + ch * 8) = o;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) s1 += v[c][e];
        }
    }
    const float mean = wave_sum(s1) / (float)p.H;
    float s2 = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int ch = c * 64 + lane;
        if (ch < nchunk) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[c][e] - mean; s2 += d * d; }
        }
    }
    const float rstd = rsqrtf(wave_sum(s2) / (float)p.H + p.eps);
    if (lane == 0) {
        if (p.mean) p.mean[row] = mean;
        if (p.rstd) p.rstd[row] = rstd;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int ch = c * 64 + lane;
        if (ch < nchunk) {
            const u32x4_t g = *(const u32x4_t*)(p.w + ch * 8), bb = *(const u32x4_t*)(p.b + ch * 8);
            u32x4_t o;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                o[e] = pack2bf((v[c][2 * e] - mean) * rstd * lo_bf(g[e]) + lo_bf(bb[e]), (v[c][2 * e + 1] - mean) * rstd * hi_bf(g[e]) + hi_bf(bb[e]));
            *(u32x4_t*)(p.y + (long long)row * p.ldy + ch * 8) = o;
        }
    }
}

struct LnBwdArgs {
    const bf16_t* dy;
    const bf16_t* x;
    const bf16_t* w;
    const float* mean;
    const float* rstd;
    const bf16_t* dres;
    bf16_t* dx;
    float* dw;
    float* db;
    float* ws;           // [gridDim.x][2][H] partial (dw, db) of every block, summed in block order by partial_reduce_acc_kernel
    int T, H;
    long long ld;
};

template <int NC>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(LnBwdArgs p) {
    extern __shared__ float sred[];  // [2][4][H]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int nchunk = p.H >> 3;
    float dwacc[NC][8], dbacc[NC][8], g[NC][8];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int ch = c * 64 + lane;
#pragma unroll
        for (int e = 0; e < 8; ++e) { dwacc[c][e] = 0.f; dbacc[c][e] = 0.f; g[c][e] = 0.f; }
        if (ch < nchunk) {
            const u32x4_t gg = *(const u32x4_t*)(p.w + ch * 8);
#pragma unroll
            for (int e = 0; e < 4; ++e) { g[c][2 * e] = lo_bf(gg[e]); g[c][2 * e + 1] = hi_bf(gg[e]); }
        }
    }
    for (int row = blockIdx.x * 4 + wv; row < p.T; row += gridDim.x * 4) {
        const float mean = p.mean[row], rstd = p.rstd[row];
        float n[NC][8], dn[NC][8];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int ch = c * 64 + lane;
            if (ch < nchunk) {
                const u32x4_t a = *(const u32x4_t*)(p.x + (long long)row * p.ld + ch * 8);
                const u32x4_t d = *(const u32x4_t*)(p.dy + (long long)row * p.ld + ch * 8);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    n[c][2 * e] = (lo_bf(a[e]) - mean) * rstd;
                    n[c][2 * e + 1] = (hi_bf(a[e]) - mean) * rstd;
                    const float d0 = lo_bf(d[e]), d1 = hi_bf(d[e]);
                    dwacc[c][2 * e] += d0 * n[c][2 * e];
                    dwacc[c][2 * e + 1] += d1 * n[c][2 * e + 1];
                    dbacc[c][2 * e] += d0;
                    dbacc[c][2 * e + 1] += d1;
                    dn[c][2 * e] = d0 * g[c][2 * e];
                    dn[c][2 * e + 1] = d1 * g[c][2 * e + 1];
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) { s1 += dn[c][e]; s2 += dn[c][e] * n[c][e]; }
            }
        }
        s1 = wave_sum(s1) / (float)p.H;
        s2 = wave_sum(s2) / (float)p.H;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int ch = c * 64 + lane;
            if (ch < nchunk) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = rstd * (dn[c][e] - s1 - n[c][e] * s2);
                if (p.dres) {
                    const u32x4_t r = *(const u32x4_t*)(p.dres + (long long)row * p.ld + ch * 8);
#pragma unroll
                    for (int e = 0; e < 4; ++e) { o[2 * e] += lo_bf(r[e]); o[2 * e + 1] += hi_bf(r[e]); }
                }
                u32x4_t ov;
#pragma unroll
                for (int e = 0; e < 4; ++e) ov[e] = pack2bf(o[2 * e], o[2 * e + 1]);
                *(u32x4_t*)(p.dx + (long long)row * p.ld + ch * 8) = ov;
            }
        }
    }
    if (!p.dw) return;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int ch = c * 64 + lane;
        if (ch < nchunk) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                sred[wv * p.H + ch * 8 + e] = dwacc[c][e];
                sred[(4 + wv) * p.H + ch * 8 + e] = dbacc[c][e];
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < p.H; i += 256) {
        p.ws[((long long)blockIdx.x * 2) * p.H + i] = sred[i] + sred[p.H + i] + sred[2 * p.H + i] + sred[3 * p.H + i];
        p.ws[((long long)blockIdx.x * 2 + 1) * p.H + i] = sred[4 * p.H + i] + sred[5 * p.H + i] + sred[6 * p.H + i] + sred[7 * p.H + i];
    }
}

}  // namespace

extern "C" int iadr1_layernorm_fwd(const void* x, const void* res, void* res_out, const void* w, const void* b, void* y, float* mean,
                                   float* rstd, int T, int H, long long ldx, long long ldr, long long ldy, float eps, hipStream_t stream) {
    IADR1_REQUIRE(T > 0 && H > 0 && (H % 8) == 0 && H <= MAXC * 512, "layernorm_fwd: H=%d must be a multiple of 8 and <= %d", H, MAXC * 512);
    IADR1_REQUIRE((ldx % 8) == 0 && (ldr % 8) == 0 && (ldy % 8) == 0, "layernorm_fwd: leading dims must be multiples of 8");
    LnFwdArgs p{(const bf16_t*)x, (const bf16_t*)res, (bf16_t*)res_out, (const bf16_t*)w, (const bf16_t*)b, (bf16_t*)y, mean, rstd, T, H, ldx, ldr, ldy, eps};
    const dim3 grid((T + 3) / 4), block(256);
#define CALL(NC) hipLaunchKernelGGL(layernorm_fwd_kernel<NC>, grid, block, 0, stream, p)
    DISPATCH_NC(H, CALL);
#undef CALL
    return iadr1_check_launch("layernorm_fwd");
}

extern "C" int iadr1_layernorm_bwd(const void* dy, const void* x, const void* w, const float* mean, const float* rstd, const void* dres,
                                   void* dx, float* dw, float* db, float* workspace, int T, int H, long long ld, hipStream_t stream) {
    IADR1_REQUIRE(T > 0 && H > 0 && (H % 8) == 0 && H <= MAXC * 512, "layernorm_bwd: H=%d must be a multiple of 8 and <= %d", H, MAXC * 512);
    IADR1_REQUIRE((ld % 8) == 0 && ((dw == nullptr) == (db == nullptr)), "layernorm_bwd: ld multiple of 8; dw and db together");
    IADR1_REQUIRE(dw == nullptr || workspace != nullptr, "layernorm_bwd: parameter gradients need the partial-sum workspace (iadr1_layernorm_bwd_workspace_bytes)");
    LnBwdArgs p{(const bf16_t*)dy, (const bf16_t*)x, (const bf16_t*)w, mean, rstd, (const bf16_t*)dres, (bf16_t*)dx, dw, db, workspace, T, H, ld};
    const int blocks = norm_bwd_blocks(T);
    const dim3 grid(blocks), block(256);
#define CALL(NC) hipLaunchKernelGGL(layernorm_bwd_kernel<NC>, grid, block, (size_t)(dw ? 8 * H * sizeof(float) : 0), stream, p)
    DISPATCH_NC(H, CALL);
#undef CALL
    if (dw) {
        hipLaunchKernelGGL(partial_reduce_acc_kernel, dim3((H + 31) / 32), dim3(256), 0, stream, (const float*)workspace, blocks, (long long)2 * H, dw, H);
        hipLaunchKernelGGL(partial_reduce_acc_kernel, dim3((H + 31) / 32), dim3(256), 0, stream, (const float*)workspace + H, blocks, (long long)2 * H, db, H);
    }
    return iadr1_check_launch("layernorm_bwd");
}

IADR1_STAMPS_EXPORT(norm)
