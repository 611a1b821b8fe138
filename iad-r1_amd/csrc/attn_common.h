// What the training attention (attn.hip) and the paged decode attention (attn_decode.hip) share: MFMA fragment helpers and the softmax constants.
#pragma once
#include "common.h"

__device__ __forceinline__ bf16x8_t ld_frag_g(const bf16_t* p, bool ok) {
    u32x4_t v = {0, 0, 0, 0};
    if (ok) v = *(const u32x4_t*)p;
    return __builtin_bit_cast(bf16x8_t, v);
}

// v_exp_f32 directly: exp2f() wraps it in a denormal-range rescale (~5 extra VALU instructions per call); softmax terms that small are zero anyway
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ bf16x8_t pack_frag(const f32x4_t a, const f32x4_t b) {
    u32x4_t v = {pack2bf(a[0], a[1]), pack2bf(a[2], a[3]), pack2bf(b[0], b[1]), pack2bf(b[2], b[3])};
    return __builtin_bit_cast(bf16x8_t, v);
}

constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
