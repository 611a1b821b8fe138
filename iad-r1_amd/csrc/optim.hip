// Fused flat AdamW + global grad-norm (gfx950, HBM-bound; SURVEY.md section 2.3 K19: HF Trainer's default
// torch.optim.AdamW, betas (0.9, 0.999), eps 1e-8, decoupled weight decay, max_grad_norm clipping).
// All parameters live in ONE flat buffer per dtype, so a step is two launches, not thousands:
//   sumsq:  norm2 += sum(g^2)                       (clip coefficient computed on device, no host sync)
//   adamw:  m,v,master (fp32) updated from fp32 grads; bf16 shadow parameter re-materialised; grad zeroed.
#include "common.h"

namespace {

// Deterministic two-stage reduction (no float atomics): data-parallel replicas must compute a BIT-IDENTICAL clip
// coefficient from their identical all-reduced gradients, or they drift apart.
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* g, long long n, float* partial) {
    __shared__ float scratch[16];
    float s = 0.f;
    const long long n4 = n >> 2;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4_t v = *(const f32x4_t*)(g + i * 4);
        s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    for (long long i = n4 * 4 + (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) s += g[i] * g[i];
    s = block_sum<256>(s, scratch);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void sumsq_final_kernel(const float* partial, int nblocks, float* out) {
    __shared__ float scratch[16];
    float s = 0.f;
    for (int i = threadIdx.x; i < nblocks; i += 256) s += partial[i];
    s = block_sum<256>(s, scratch);
    if (threadIdx.x == 0) out[0] = s;
}

struct AdamArgs {
    float* master;
    float* m;
    float* v;
    float* grad;
    bf16_t* param;
    long long n;
    float lr, b1, b2, eps, wd, bc1, bc2;  // bc = 1 - beta^t
    float grad_scale;                     // e.g. 1/world_size or 1/accum
    const float* norm2;                   // optional: sum of squares of the (unscaled) grads
    float max_norm;                       // <=0: no clipping
};

__global__ __launch_bounds__(256) void adamw_kernel(AdamArgs p) {
    float scale = p.grad_scale;
    if (p.norm2 && p.max_norm > 0.f) {
        const float nrm = sqrtf(*p.norm2) * p.grad_scale;
        const float coef = p.max_norm / (nrm + 1e-6f);  // torch.nn.utils.clip_grad_norm_
        if (coef < 1.f) scale *= coef;
    }
    const float step = p.lr / p.bc1;
    const float isq = rsqrtf(p.bc2);
    for (long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4; i < p.n; i += (long long)gridDim.x * 256 * 4) {
        if (i + 4 <= p.n) {
            f32x4_t g = *(const f32x4_t*)(p.grad + i), m = *(const f32x4_t*)(p.m + i), v = *(const f32x4_t*)(p.v + i), w = *(const f32x4_t*)(p.master + i);
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ge = g[e] * scale;
                w[e] *= (1.f - p.lr * p.wd);
                m[e] = p.b1 * m[e] + (1.f - p.b1) * ge;
                v[e] = p.b2 * v[e] + (1.f - p.b2) * ge * ge;
                w[e] -= step * m[e] / (sqrtf(v[e]) * isq + p.eps);
                o[e] = w[e];
            }
            *(f32x4_t*)(p.m + i) = m;
            *(f32x4_t*)(p.v + i) = v;
            *(f32x4_t*)(p.master + i) = w;
            *(f32x4_t*)(p.grad + i) = (f32x4_t){0.f, 0.f, 0.f, 0.f};
            *(u32x2_t*)(p.param + i) = (u32x2_t){pack2bf(o[0], o[1]), pack2bf(o[2], o[3])};
        } else {
            for (long long j = i; j < p.n; ++j) {
                const float ge = p.grad[j] * scale;
                float w = p.master[j] * (1.f - p.lr * p.wd);
                const float m = p.b1 * p.m[j] + (1.f - p.b1) * ge;
                const float v = p.b2 * p.v[j] + (1.f - p.b2) * ge * ge;
                w -= step * m / (sqrtf(v) * isq + p.eps);
                p.m[j] = m; p.v[j] = v; p.master[j] = w; p.grad[j] = 0.f; p.param[j] = f2bf(w);
            }
        }
    }
}

// TR-DPO reference update (trl's SyncRefModelCallback, REF:trl/trl/trainer/callbacks.py:107-109: ref.mul_(1 - alpha).add_(policy, alpha = alpha)) over the flat
// bf16 parameter buffer: one HBM-bound pass (2 B read + 2 B read + 2 B written per parameter) instead of a loop over ~450 tensors.  A sibling of adamw_kernel.
//   out = bf16_rn( fl(c * ref) + fl(a * pol) ),  a = (float)alpha,  c = (float)(1.0 - (double)alpha), both formed on the host; two fp32 products and one fp32 sum,
//   never contracted into an fma (this file is built with -ffp-contract=fast: ref_mix_one keeps the three operations apart), ONE rounding to bf16.
// This restates the formula, not one backend's rounding of it.  trl's literal in-place arithmetic on bf16 tensors rounds twice and differs between devices: on
// a CPU it is bit for bit bf16(bf16(ref * f32(1 - alpha)) + bf16(alpha) * pol) -- alpha itself rounded to bf16 (0.6 -> 0.6015625); checked on 2^20 elements at
// alpha = 0.6, 0.1 and 0.999.
// Fixed point: an element whose ref and pol hold the same BITS keeps them, by a select in front of the arithmetic.  Mathematically c x + a x = x, but for alpha
// below about 0.5 the rounded sum need not give x back; the select keeps zero padding, padded head dims and every tensor the optimizer never moved bit-identical
// for the whole run.  alpha == 1 is a copy of pol through the same select (0 * ref + 1 * pol is exact on finite inputs except that it loses the sign of a -0).
// DIST: the same pass also reduces sum (pol - ref)^2 and sum ref^2 over the reference BEFORE it is overwritten, the two-stage deterministic way of sumsq above:
// per-block partials {d2, r2} at partial[2 b], partial[2 b + 1], then ref_mix_final_kernel; no float atomics.  Depth of the summation tree, for n elements on
// B = min(ceil(n / 2048), 4096) blocks, T = ceil(n / (2048 B)) trips of the grid-stride loop:
//   D = 8 T + ceil(B / 256) + 23
// = 8 T serial adds per thread, 6 shuffle levels + 4 adds over the waves in each of the two stages (20), ceil(B / 256) serial adds per thread of the final block,
// and 3 for a term's own roundings (the difference, the square, its entry into the chain).  All terms are non-negative: relative error <= D * 2^-24.
// Under -ffp-contract=fast the backend fuses any multiply that feeds an add, whatever the source says: `#pragma clang fp contract(off)` around these three operations
// still came out of the library build as v_pk_mul + v_pk_fma (838 of 2^23 + 8 outputs one bf16 ulp off the restatement).  So each product goes through an empty asm
// that makes it an opaque register to the instruction selector: no instruction is emitted for it, and the add cannot see a multiply to fuse with.
__device__ __forceinline__ float ref_mix_one(float c, float r, float a, float p) {
    float x = c * r, y = a * p;
    asm volatile("" : "+v"(x));
    asm volatile("" : "+v"(y));
    return x + y;
}
template <bool DIST>
__global__ __launch_bounds__(256) void ref_mix_kernel(bf16_t* ref, const bf16_t* pol, long long n8, float c, float a, int copy, float* partial) {
    __shared__ float scratch[16];
    float d2 = 0.f, r2 = 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
        const u32x4_t r = *(const u32x4_t*)(ref + i * 8), p = *(const u32x4_t*)(pol + i * 8);
        u32x4_t o;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float r0 = lo_bf(r[w]), r1 = hi_bf(r[w]), p0 = lo_bf(p[w]), p1 = hi_bf(p[w]);
            if constexpr (DIST) {
                const float e0 = p0 - r0, e1 = p1 - r1;
                d2 = __builtin_fmaf(e0, e0, d2);
                d2 = __builtin_fmaf(e1, e1, d2);
                r2 = __builtin_fmaf(r0, r0, r2);
                r2 = __builtin_fmaf(r1, r1, r2);
            }
            const uint32_t mixed = pack2bf(ref_mix_one(c, r0, a, p0), ref_mix_one(c, r1, a, p1));
            const uint32_t x = r[w] ^ p[w];
            const uint32_t keep = ((copy || (x & 0x0000ffffu) == 0) ? 0x0000ffffu : 0u) | ((copy || (x & 0xffff0000u) == 0) ? 0xffff0000u : 0u);
            o[w] = (p[w] & keep) | (mixed & ~keep);
        }
        *(u32x4_t*)(ref + i * 8) = o;
    }
    if constexpr (DIST) {
        d2 = block_sum<256>(d2, scratch);
        r2 = block_sum<256>(r2, scratch);
        if (threadIdx.x == 0) {
            partial[2 * blockIdx.x] = d2;
            partial[2 * blockIdx.x + 1] = r2;
        }
    }
}
__global__ __launch_bounds__(256) void ref_mix_final_kernel(const float* partial, int nblocks, float* out) {
    __shared__ float scratch[16];
    float d2 = 0.f, r2 = 0.f;
    for (int i = threadIdx.x; i < nblocks; i += 256) {
        d2 += partial[2 * i];
        r2 += partial[2 * i + 1];
    }
    d2 = block_sum<256>(d2, scratch);
    r2 = block_sum<256>(r2, scratch);
    if (threadIdx.x == 0) {
        out[0] = d2;
        out[1] = r2;
    }
}

}  // namespace

extern "C" int iadr1_sumsq(const float* g, long long n, float* partials2048, float* out, hipStream_t stream) {
    IADR1_REQUIRE(n > 0 && partials2048 != nullptr, "sumsq: empty input or missing 2048-float scratch");
    long long blocks = (n / 4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3((int)blocks), dim3(256), 0, stream, g, n, partials2048);
    hipLaunchKernelGGL(sumsq_final_kernel, dim3(1), dim3(256), 0, stream, (const float*)partials2048, (int)blocks, out);
    return iadr1_check_launch("sumsq");
}

extern "C" int iadr1_adamw_flat(float* master, float* m, float* v, float* grad, void* param_bf16, long long n, float lr, float beta1,
                                float beta2, float eps, float weight_decay, int step, float grad_scale, const float* norm2, float max_norm,
                                hipStream_t stream) {
    IADR1_REQUIRE(n > 0 && step >= 1, "adamw: n>0 and step>=1 required");
    IADR1_REQUIRE((((uintptr_t)master | (uintptr_t)m | (uintptr_t)v | (uintptr_t)grad) & 15) == 0 && (((uintptr_t)param_bf16) & 7) == 0, "adamw: buffers must be 16-byte aligned");
    AdamArgs p{master, m, v, grad, (bf16_t*)param_bf16, n, lr, beta1, beta2, eps, weight_decay, 1.f - powf(beta1, (float)step), 1.f - powf(beta2, (float)step), grad_scale, norm2, max_norm};
    long long blocks = (n / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(adamw_kernel, dim3((int)blocks), dim3(256), 0, stream, p);
    return iadr1_check_launch("adamw_flat");
}

#define IADR1_REF_MIX_MAX_BLOCKS 4096      // the cap of adamw_flat's grid

extern "C" int iadr1_ref_mix_partials(void) { return 2 * IADR1_REF_MIX_MAX_BLOCKS; }

extern "C" int iadr1_ref_mix(void* ref_bf16, const void* pol_bf16, long long n, float alpha, float* partials, float* dist2, hipStream_t stream) {
    IADR1_REQUIRE(n > 0, "ref_mix: n must be > 0 (got n = %lld)", n);
    IADR1_REQUIRE(n % 8 == 0, "ref_mix: n must be a multiple of 8, the 16-byte unit of the pass (got n = %lld): the parameter store's offsets are multiples of 64", n);
    IADR1_REQUIRE(ref_bf16 != nullptr && pol_bf16 != nullptr, "ref_mix: ref and pol must be given (got ref = %p, pol = %p)", ref_bf16, pol_bf16);
    IADR1_REQUIRE((((uintptr_t)ref_bf16 | (uintptr_t)pol_bf16) & 15) == 0, "ref_mix: ref and pol must be 16-byte aligned (got ref = %p, pol = %p)", ref_bf16, pol_bf16);
    IADR1_REQUIRE(alpha > 0.f && alpha <= 1.f, "ref_mix: alpha must be finite and in (0, 1] (got alpha = %g)", (double)alpha);      // (a NaN fails both compares)
    IADR1_REQUIRE(dist2 == nullptr || partials != nullptr, "ref_mix: dist2 needs the partials scratch of iadr1_ref_mix_partials() floats (got partials = NULL)");
    const float a = alpha, c = (float)(1.0 - (double)alpha);
    const long long n8 = n / 8;
    long long blocks = (n8 + 255) / 256;
    if (blocks > IADR1_REF_MIX_MAX_BLOCKS) blocks = IADR1_REF_MIX_MAX_BLOCKS;
    const int copy = alpha == 1.f ? 1 : 0;
    if (dist2 != nullptr) {
        hipLaunchKernelGGL(ref_mix_kernel<true>, dim3((int)blocks), dim3(256), 0, stream, (bf16_t*)ref_bf16, (const bf16_t*)pol_bf16, n8, c, a, copy, partials);
        hipLaunchKernelGGL(ref_mix_final_kernel, dim3(1), dim3(256), 0, stream, (const float*)partials, (int)blocks, dist2);
    } else {
        hipLaunchKernelGGL(ref_mix_kernel<false>, dim3((int)blocks), dim3(256), 0, stream, (bf16_t*)ref_bf16, (const bf16_t*)pol_bf16, n8, c, a, copy, (float*)nullptr);
    }
    return iadr1_check_launch("ref_mix");
}
