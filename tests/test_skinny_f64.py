"""The decode skinny GEMMs of csrc/skinny.hip and their packers against float64: iadr1_gemm_skinny_bf16 (out_mode 0 - 3, ksplit, side), iadr1_gemm_skinny_fp8w,
iadr1_gemm_qkv_rope_kv_bf16, iadr1_pack_weight_bf16, iadr1_pack_gateup_bf16, iadr1_pack_qkv_rope_bf16, iadr1_pack_act_bf16, iadr1_pack_weight_fp8.  The structure and
the helpers are those of test_tokenwise_f64.py (Guard, call_guarded, refused, frac, ...) and test_gemm_f64.py (b_x, gcheck, excess).  Every call goes to the C ABI.

THE BOUND.  Every output element is held to   |got - ref64| <= 2^-8 c |ref64| + 2^-24 (f0 E + fn n E) + 1e-30   (no element is exempt), f0 = 4, fn = 2 (test_gemm_f64.b_x).
ref64 is the operation in float64 on the bf16-rounded inputs with NO intermediate rounding, E = sum_k |x| |w| (+ |bias|), n = K + 16 + ksplit: the additions inside and across
the MFMAs, the wave-order sum through LDS (<= 16 waves) and the slab sum.  Inputs are zero or in the normal bf16 range (asserted).
  f32, slab  c 0: fp32 stores and each partial slab.  A slab is checked against the float64 sum over ITS OWN k range (E over that range), and the float64 sum of the slabs
             against the whole contraction (key `slabsum`): the sum alone would hide a step that moved from one slice to its neighbour.
  bf16       c 2 (+ bias in E).
  swiglu.gu  the gate|up rows stored through `side`: the bf16 bound.  swiglu.a there: the token-wise entry (c 3, F_EXP, E = |ref|) against float64 SwiGLU of the kernel's OWN
             stored rows, and bit-equal to iadr1_swiglu_fwd on them.
  swiglu.a   where gate|up is not stored (wide kernels, side == NULL): the token-wise term on the float64 a, plus |silu'(g)| |u| b_g + |silu(g)| b_u, b_g, b_u the bf16 bounds
             of the two pre-activations.
  qkv.v      V cache and V side rows: the bf16 bound.  qkv.rot (q, the K cache, the rotary side rows): |cos| b_a + |sin| b_b + c 2 on the result + 4 x 2^-24 (|a cos| + |b sin|),
             b_a, b_b the bf16 bounds of the two rotary partners; the four roundings are the two products, the add and a possible contraction.
  fp8.*      the reference is float64 of (x . q) scale with q and scale what the packer wrote (proven by the bit equalities below); one more fp32 rounding (f0 + 2).
No bound above was changed after the first GPU run.

EQUALITIES, bit for bit.  (1) One-hot rows: some rows of X are v e_k (v = 1, then -2), some rows of W are e_k (FP8: 0.875 e_k = 448 x 2^-9, an exact e4m3 multiple of a
power-of-two scale), k over the first and last element of every 8-chunk of the first and the last 32-step and the first and last element of every split slice (hot_ks).
The output row / column is the other operand's column after the IEEE-fixed scale multiply, bias add and bf16 store; in split-K it sits in the slab of k's slice and the other
slabs hold zeros (the sign of a zero apart).  In mode 3 the one-hot rows' gate|up values are known bf16 numbers: the side rows must be those, and a the one correct bit
pattern where swiglu_exact() says there is only one.  q|k|v: the one-hot X rows carry the exact tables below.  (2) Rotary rows with (cos, sin) = (1, 0) give q / K / side
equal to the bf16 projection (a mode 0 launch of the plain kernel on the naturally packed weights, and the known values on one-hot rows), rows with (0, 1) the partner, negated
in the first half.  (3) Every packer against an index formula written from the layout comments, ldw / ldx = K + 16 / K + 8 with poison in the padding; pack_act's pad rows are
zero; pack_weight_fp8's scale is max(amax, 1e-30f) / 448 in fp32 and every byte torch.float8_e4m3fn of the fp32 quotient (an all-zero row, a row of e4m3 subnormal quotients,
rows of exact e4m3 multiples, the gate|up interleave; each row's largest element quantises to +-448, asserted on the CPU).  (4) Sentinels: lead / trail rows of Y, columns
N .. ldy, pad rows of a decode-packed Y, side rows other than base + s seq_stride + *step, cache slots of slot < 0 and every slot not named; inputs unchanged.  (5) Two different
finite fills of X's padding (pad rows of the packed X, columns K .. ldx, rows past M) give the same bits -- every case runs twice, so run-to-run bits too.  (6) side p1 row ==
main Y row; side == NULL gives the same Y; a row's bits do not depend on MG (M 5, 20, 70; narrow and q|k|v).  (7) Empty split-K slices give exact zeros.

INPUTS.  X N(0,1), W 0.5 N(0,1), bias 2 N(0,1), all in Guards; ldx = K + 8 (row-major X), ldy = N + 8; one case per output type has ldy = N + 3.  Cache slots: pages permuted,
offsets 0 and 31 present, slot < 0 in the middle and in the last row, page counts M + 3 (row-major X) and 2 M + 5 (packed X).

WHICH CASE REACHES WHICH BRANCH.  A case is (M, N, K, out_mode, ksplit, decode_cus, X packed); route() below mirrors pers_form and the launchers' if chains, and
test_cpu_route_table asserts the kernel named for every case and that all 17 instantiations of skinny_lds_optin() are reached.
  narrow<1,16,MG>  cus 1024: (5,48,32,0,1) MG 1, only the 32-wide tail; (5,48,96,1,1) a slab + tail; (16,48,1056,0,1) 16 slabs on 16 waves, tail by wave 0;
             (17,80,2144,0,1), (32,80,2144,1,1,pk) MG 2: 33 slabs = a U = 2 trip, a single-slab trip of wave 0, the tail; (33,80,2144,0,1), (70,80,1056,0,1,pk) MG 4, two row
             tiles; (70,48,2144,2,3) slices of 11 slabs, tail in the last; (5,48,96,2,4): slices 1 and 2 empty, slice 3 holds ONLY the tail (the launcher gives the tail to
             the last slice; the issue's table counted three empty ones).
  narrow<2,8>      (9,8208,96,0,1) + bias, (70,8208,160,1,1,pk), (9,8208,1120,2,2): 257 blocks, the last one's second tile is the clamped duplicate of tile 512.
  wide<8,8>/<4,8>  (70,8192,96,0,1) <8,8> 3 steps on 8 waves; (70,8192,608,1,1,pk) <4,8> 19 steps: a depth-2 trip + a depth-1 trip of waves 0 - 2; (70,8256,96,0,1,pk) 129 blocks;
             mode 3 (9,256,608,3,1) <8,8>, (70,384,608,3,1,pk) <4,8>, Y row-major and decode-packed; (70,1536,640,2,8) 20 steps, per_z 3, slice 6 of 2, slice 7 EMPTY;
             (9,1536,96,2,8,pk) five empty slices.
  pers<8,4/6/8>    (70,160,1024,0,1,cus 2) + bias: 5 groups on 2 blocks; (9,160,1536,1,1,cus 2,pk); (70,160,2048,2,1,cus 2) slab 0 of a one-slice mode 2; mode 3 with side and
             with side == NULL: (70,640,1024,3,1,cus 8,pk) the XCD order, 20 groups, blocks 5 - 7 idle; (70,384,1024,3,1,cus 3) the plain order.
  split<8,6>/<8,10>  (70,256,416,2,2,cus 8) 13 steps, slices 7 + 6; (9,272,672,2,2,cus 8,pk) per_z 11, 17 tiles on 4 blocks; (70,64,3200,2,8,cus 8) bps 1, last slice 9;
             (70,256,3200,2,2,cus 8) per_z 50 and (9,80,5120,2,2,cus 2,pk) per_z 80: <8,10>.
  FP8        wide<4,8,fp8> cus 1024: (70,128,64,0,1) + bias, (9,192,448,1,1,pk) 7 double steps, (70,128,448,2,3), (70,128,192,3,1); (70,256,3200,2,2,cus 8) per_z 25 > 24: one-shot;
             pers<8,4/6/8,fp8>: (70,192,1024,0,1,cus 2), (9,256,1536,3,1,cus 2,pk), (70,192,2048,1,1,cus 3); split<8,3,fp8>: (70,256,832,2,2,cus 8), (9,64,3072,2,2,cus 2,pk) per_z 24.
  q|k|v      D 128, M 5 / 20 / 70: (Hq 2, Hkv 1) K 96 and K 256 at cus 1024 -> MG 1 / 2 / 4; cus 24, K 256 -> the fused-V kernel (32 tiles, 24 rotary); cus 24, K 96 -> the plain
             kernel (K % 64); (Hq 1, Hkv 1, K 256, cus 16) fused V.  Each with and without side, X row-major and packed.

THE CPU PART proves the sensitivity of the GPU part.  A torch emulation of the kernels' arithmetic -- each 32-deep step summed in float64 and rounded to fp32, each wave's chain
in the kernel's step order (plan()), the waves added in wave order, slices kept apart, bf16 at the kernel's rounding points -- stays inside every bound on every input set of the
GPU part.  It is not claimed bit-equal to the hardware.  Every fault model of FAULT_MODELS, applied to the float64 reference on the same inputs, leaves its bound by >=
FAULT_FACTOR at its designated elements, or changes bits where an equality is the check (marked inf).

USED FRACTIONS of the GPU run on an MI355X (largest |got - ref64| / bound per output key, printed by test_gpu_used_fractions_record); the first GPU run passed every bound:
  bf16 0.4972   f32 0.0039   slab 0.0060   slabsum 0.0026   swiglu.a 0.4212   swiglu.gu 0.4267   swiglu.a_of_gu 0.6163   qkv.rot 0.4654   qkv.v 0.4972
  fp8.bf16 0.4974   fp8.f32 0.0028   fp8.slab 0.0026   fp8.slabsum 0.0026   fp8.swiglu.a 0.4836
(bf16 outputs sit at half of c = 2: the store's own rounding; the fp32 ones use < 1 % of the worst-case n E term, which is why the equalities and the slab-wise check carry
the sensitivity there -- see the excesses test_cpu_every_fault_model_was_exercised_and_emulation_record prints.)"""
import collections
import contextlib
import ctypes
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iadr1_amd  # noqa: E402,F401
from iadr1_amd import hip  # noqa: E402
from iadr1_amd.ops import SideOut  # noqa: E402
from test_gemm_f64 import b_x, excess, gcheck, normal_range, ratio  # noqa: E402
from test_tokenwise_f64 import (BF, DEV, F32, F64, F_EXP, FAULT_FACTOR, INF, TINY, U8, U24, Guard, bfr, bits, call_guarded, d, frac, gen, refused,  # noqa: E402
                                same_bits, swiglu_exact, swiglu_math, vec, workspace)

assert F_EXP == 256
U8T = torch.uint8
SENT = -700.0              # what a never-written output element holds in the CPU images of the fault models (the Guards' sentinel is -700 .. -728)
POISON = 700.0
USED = {"emu": {}, "gpu": {}}
FAULT_SEEN = {}
FAULT_MODELS = ["ktail_dropped", "ktail_every_slice", "last_single_trip_skipped", "slice_boundary_off_by_one", "last_slice_per_z", "empty_slice_sentinel",
                "wave_past_end_clamped_w", "duplicate_tile_stored", "rows_ge_M_from_row0", "gate_up_swapped", "up_from_tile_2r", "fp8_upscale_wscale_gn",
                "bias_unpermuted", "fusedv_bias_from_k_tile", "rope_partner_d32", "rope_sign_flipped", "rope_row_gm0", "kcache_row_major", "vcache_written_slot_neg",
                "fp8_halves_swapped", "fp8_scale_row_xor_1", "side_row_without_step", "xcd_order_bps_not_8"]


def check(side, key, got, ref, bound, what):
    mx = gcheck(side, "skinny." + key, got, ref, bound, what)
    USED[side][key] = max(USED[side].get(key, 0.0), mx)
    return mx


def fexcess(fault, bad, ref, bound, rows=None, cols=None):
    ex = excess("skinny." + fault, bad, ref, bound, rows, cols)
    FAULT_SEEN[fault] = min(FAULT_SEEN.get(fault, INF), ex)


def fbits(fault, bad, ref):
    """an equality is the check: the fault must change bits"""
    assert bad.shape == ref.shape and int((bits(bad) != bits(ref)).sum()) > 0, f"fault '{fault}' changes no bit of what an equality checks"
    FAULT_SEEN.setdefault(fault, INF)


def ceil_div(a, b):
    return (a + b - 1) // b


def roundup(n, q):
    return ceil_div(n, q) * q


# ======================================================================================================================================================
# the launchers' routing, mirrored
# ======================================================================================================================================================

N1, N2, N4, N28, NFV = "narrow<1,16,MG1>", "narrow<1,16,MG2>", "narrow<1,16,MG4>", "narrow<2,8>", "narrow<1,16,fusedV>"
W8, W4, W4F = "wide<8,8>", "wide<4,8>", "wide<4,8,fp8>"
P4, P6, P8, P4F, P6F, P8F = "pers<8,4>", "pers<8,6>", "pers<8,8>", "pers<8,4,fp8>", "pers<8,6,fp8>", "pers<8,8,fp8>"
S6, S10, S3F = "split<8,6>", "split<8,10>", "split<8,3,fp8>"
INSTANTIATIONS = [N4, N1, N2, N28, NFV, W8, W4, W4F, P8, P6, P4, P8F, P6F, P4F, S6, S10, S3F]          # the list of skinny_lds_optin(), in its order


class Refusal(Exception):
    pass


def pers_form(N, K, out_mode, ksplit, ncu, depth, max_per_z):
    """(bps, per_z, ksw) of csrc/skinny.hip pers_form"""
    steps = K // depth
    per_z, bps, ksw = ceil_div(steps, ksplit), ncu // ksplit, K // 256
    if ksplit > 1 and out_mode == 2 and per_z <= max_per_z and bps >= 1 and (N >> 4) >= 4 * bps and (steps % ksplit == 0 or (ksplit - 1) * per_z < steps):
        return bps, per_z, 0
    if ksplit == 1 and N % 32 == 0 and K % 256 == 0 and ksw in (8, 6, 4) and N // 32 >= 2 * ncu:
        return 0, 0, ksw
    return 0, 0, 0


def route(M, N, K, out_mode, ksplit, ncu, packed, fp8=False, side=False, ldy=1, wscale=True):
    """the kernel instantiation iadr1_gemm_skinny_bf16 / _fp8w launches (skinny_args + the if chain), or Refusal"""
    kmul, nmul = (64, 64) if fp8 else (32, 16)
    if not (M > 0 and N > 0 and K > 0 and (not fp8 or wscale)):
        raise Refusal("empty / no scales")
    if K % kmul or N % nmul:
        raise Refusal("K / N multiple")
    if ldy == 0 and not (out_mode == 3 and N % 64 == 0):
        raise Refusal("ldy == 0 outside mode 3")
    if not (0 <= out_mode <= 3 and ksplit >= 1 and (ksplit == 1 or out_mode == 2)):
        raise Refusal("out_mode / ksplit")
    if out_mode == 3 and N % 128:
        raise Refusal("mode 3 N % 128")
    if fp8:
        bps, per_z, ksw = pers_form(N, K, out_mode, ksplit, ncu, 64, 24)
        return S3F if bps else {8: P8F, 6: P6F, 4: P4F}.get(ksw, W4F)
    bps, per_z, ksw = pers_form(N, K, out_mode, ksplit, ncu, 32, 80)
    if bps:
        if side:
            raise Refusal("side on the split form")
        return S6 if per_z <= 48 else S10
    if side and not (out_mode == 3 and ksw):
        raise Refusal("side outside the persistent mode 3")
    if ksw:
        return {8: P8, 6: P6, 4: P4}[ksw]
    big = (N >= 8192 and ksplit == 1) or out_mode == 3
    nb = 4 if packed else 8
    if big and nb == 4 and N % 64 == 0:
        return W4
    if big and N % 128 == 0:
        return W8
    if ksplit > 1 and N % 64 == 0 and (N // 64) * ksplit >= 192:
        return W4
    if N >= 8192:
        return N28
    return N1 if M <= 16 else (N2 if M <= 32 else N4)


def route_qkv(M, Hq, Hkv, K, ncu):
    tiles, rope_tiles = (Hq + 2 * Hkv) * 8, (Hq + Hkv) * 8
    if K % 32:
        raise Refusal("K % 32")
    if tiles > ncu and rope_tiles <= ncu and K % 64 == 0:
        return NFV
    return N1 if M <= 16 else (N2 if M <= 32 else N4)


Case = collections.namedtuple("Case", "M N K mode ks cus packed fp8 kern")


def C(M, N, K, mode, ks, cus, kern, pk=False, fp8=False):
    return Case(M, N, K, mode, ks, cus, pk, fp8, kern)


def cid(c):
    return f"{c.M}-{c.N}-{c.K}-m{c.mode}-ks{c.ks}-cus{c.cus}-{'pk' if c.packed else 'rm'}" + ("-fp8" if c.fp8 else "")


BF16_CASES = [
    C(5, 48, 32, 0, 1, 1024, N1), C(5, 48, 96, 1, 1, 1024, N1), C(16, 48, 1056, 0, 1, 1024, N1), C(17, 80, 2144, 0, 1, 1024, N2), C(32, 80, 2144, 1, 1, 1024, N2, pk=True),
    C(33, 80, 2144, 0, 1, 1024, N4), C(70, 80, 1056, 0, 1, 1024, N4, pk=True), C(70, 48, 2144, 2, 3, 1024, N4), C(5, 48, 96, 2, 4, 1024, N1),
    C(9, 8208, 96, 0, 1, 1024, N28), C(70, 8208, 160, 1, 1, 1024, N28, pk=True), C(9, 8208, 1120, 2, 2, 1024, N28),
    C(70, 8192, 96, 0, 1, 1024, W8), C(70, 8192, 608, 1, 1, 1024, W4, pk=True), C(70, 8256, 96, 0, 1, 1024, W4, pk=True), C(9, 256, 608, 3, 1, 1024, W8),
    C(70, 384, 608, 3, 1, 1024, W4, pk=True), C(70, 1536, 640, 2, 8, 1024, W4), C(9, 1536, 96, 2, 8, 1024, W4, pk=True),
    C(70, 160, 1024, 0, 1, 2, P4), C(9, 160, 1536, 1, 1, 2, P6, pk=True), C(70, 160, 2048, 2, 1, 2, P8), C(70, 640, 1024, 3, 1, 8, P4, pk=True), C(70, 384, 1024, 3, 1, 3, P4),
    C(70, 256, 416, 2, 2, 8, S6), C(9, 272, 672, 2, 2, 8, S6, pk=True), C(70, 64, 3200, 2, 8, 8, S6), C(70, 256, 3200, 2, 2, 8, S10), C(9, 80, 5120, 2, 2, 2, S10, pk=True),
]
FP8_CASES = [
    C(70, 128, 64, 0, 1, 1024, W4F, fp8=True), C(9, 192, 448, 1, 1, 1024, W4F, pk=True, fp8=True), C(70, 128, 448, 2, 3, 1024, W4F, fp8=True), C(70, 128, 192, 3, 1, 1024, W4F, fp8=True),
    C(70, 256, 3200, 2, 2, 8, W4F, fp8=True), C(70, 192, 1024, 0, 1, 2, P4F, fp8=True), C(9, 256, 1536, 3, 1, 2, P6F, pk=True, fp8=True), C(70, 192, 2048, 1, 1, 3, P8F, fp8=True),
    C(70, 256, 832, 2, 2, 8, S3F, fp8=True), C(9, 64, 3072, 2, 2, 2, S3F, pk=True, fp8=True),
]
ODD_LDY = {(5, 48, 96, 1), (70, 80, 1056, 0), (70, 48, 2144, 2), (9, 256, 608, 3)}          # (M, N, K, mode): ldy = N + 3 (mode 3: I + 3), no multiple of 8
SIDE_CASES = {(70, 640, 1024), (70, 384, 1024)}
QCase = collections.namedtuple("QCase", "M Hq Hkv K cus kern")
QKV_CASES = [QCase(M, Hq, Hkv, K, cus, kern if kern else (N1, N2, N4)[i]) for i, M in enumerate((5, 20, 70))
             for Hq, Hkv, K, cus, kern in ((2, 1, 96, 1024, None), (2, 1, 256, 1024, None), (2, 1, 256, 24, NFV), (2, 1, 96, 24, None), (1, 1, 256, 16, NFV))]


def qid(q):
    return f"{q.M}-Hq{q.Hq}-Hkv{q.Hkv}-{q.K}-cus{q.cus}"


def has_bias(c):
    return c.mode == 0 and c.M not in (16, 33)


@functools.lru_cache(maxsize=None)
def plan(c):
    """[slice][wave] -> the 32-deep k-steps in the order the wave's accumulator takes them (the kernels' loops, written out)"""
    K, ks, k = c.K, c.ks, c.kern
    if k.startswith("narrow"):
        WV, nslab = (8 if k == N28 else 16), K // 64
        per_z, out = ceil_div(nslab, ks), []
        for z in range(ks):
            waves = [[t for s in range(z * per_z + w, min(nslab, (z + 1) * per_z), WV) for t in (2 * s, 2 * s + 1)] for w in range(WV)]
            if K & 32 and z == ks - 1:
                waves[0] = waves[0] + [2 * nslab]
            out.append(waves)
        return out
    dd = 2 if c.fp8 else 1
    nstep = K // (32 * dd)
    if k.startswith("wide") or k.startswith("split"):
        per_z = ceil_div(nstep, ks)
        return [[[dd * s + h for s in range(z * per_z + w, min(nstep, (z + 1) * per_z), 8) for h in range(dd)] for w in range(8)] for z in range(ks)]
    ksw = int(k[7])
    assert K == 256 * ksw and ks == 1
    if c.fp8:
        return [[[2 * (w + (j >> 1) * 8) + (j & 1) for j in range(ksw)] for w in range(8)]]
    return [[[w + j * 8 for j in range(ksw)] for w in range(8)]]


def unit_of(c):
    """32-steps per trip unit: a 64-wide slab (narrow), a double step (FP8), a step"""
    return 2 if (c.kern.startswith("narrow") or c.fp8) else 1


def slice_steps(c, z):
    return sorted(t for w in plan(c)[z] for t in w)


def cols_of(steps):
    return torch.tensor([32 * t + i for t in steps for i in range(32)], dtype=torch.long)


def test_cpu_route_table():
    """every case of the table reaches the kernel it names, the 17 instantiations are all reached, every k-step is taken exactly once"""
    reached = set()
    for c in BF16_CASES + FP8_CASES:
        got = route(c.M, c.N, c.K, c.mode, c.ks, c.cus, c.packed, c.fp8)
        assert got == c.kern, f"{cid(c)}: the launcher's rules give {got}, the table says {c.kern}"
        reached.add(got)
        steps = sorted(t for z in range(c.ks) for t in slice_steps(c, z))
        assert steps == list(range(c.K // 32)), cid(c)
        if c.kern.startswith("split"):
            assert all(slice_steps(c, z) for z in range(c.ks)), "pers_form admits no empty slice"
    for q in QKV_CASES:
        got = route_qkv(q.M, q.Hq, q.Hkv, q.K, q.cus)
        assert got == q.kern, f"{qid(q)}: {got} != {q.kern}"
        reached.add(got)
    assert len(INSTANTIATIONS) == 17 and reached == set(INSTANTIATIONS), f"not reached: {sorted(set(INSTANTIATIONS) - reached)}"
    # the shapes the table describes in words
    c = BF16_CASES[3]
    assert [len(w) // 2 for w in plan(c)[0]][:2] == [3, 2] and plan(c)[0][0][-1] == 66          # wave 0: slabs 0, 16, 32 and the tail step 66
    assert [bool(slice_steps(BF16_CASES[8], z)) for z in range(4)] == [True, False, False, True] and slice_steps(BF16_CASES[8], 3) == [2]
    assert [len(slice_steps(BF16_CASES[17], z)) for z in range(8)] == [3] * 6 + [2, 0]
    assert [len(slice_steps(BF16_CASES[18], z)) for z in range(8)] == [1, 1, 1, 0, 0, 0, 0, 0]
    assert [len(w) for w in plan(BF16_CASES[13])[0]] == [3, 3, 3, 2, 2, 2, 2, 2]
    assert [len(slice_steps(BF16_CASES[24], z)) for z in range(2)] == [7, 6] and len(slice_steps(BF16_CASES[26], 7)) == 9
    for args in ((5, 48, 40, 0, 1), (5, 40, 64, 0, 1), (5, 48, 64, 0, 2), (5, 192, 64, 3, 1)):
        with pytest.raises(Refusal):
            route(*args, 1024, False)
    with pytest.raises(Refusal):
        route(70, 256, 416, 2, 2, 8, False, side=True)
    with pytest.raises(Refusal):
        route(9, 256, 608, 3, 1, 1024, False, side=True)


# ======================================================================================================================================================
# layouts, written from the comments of csrc/skinny.hip and csrc/common.h
# ======================================================================================================================================================

def pack_w_formula(W):
    """Wp[n/16][k/32][lane = n%16 + 16 ((k%32)/8)][k%8]"""
    N, K = W.shape
    return W.reshape(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).reshape(-1)


def gateup_rows(I):
    """packed 16-row tile 2q = gate rows [16q, 16q+16), tile 2q+1 = the up rows [I+16q, ...)"""
    t = torch.arange(2 * I // 16)
    return (((t & 1) * I + (t >> 1) * 16)[:, None] + torch.arange(16)[None, :]).reshape(-1)


def qkv_rows(Hq, Hkv):
    """inside every q and k head the 128 rows go to the 8 tiles as [8j, 8j+8) ++ [64+8j, 64+8j+8); v heads keep their order"""
    rows = []
    for head in range(Hq + 2 * Hkv):
        for j in range(8):
            for lm in range(16):
                rows.append(head * 128 + ((8 * j + lm if lm < 8 else 64 + 8 * j + lm - 8) if head < Hq + Hkv else j * 16 + lm))
    return torch.tensor(rows, dtype=torch.long)


def pack_x_formula(X, fill=0.0):
    """Xp[m/64][k/32][(m%64)/16][lane = m%16 + 16 ((k%32)/8)][k%8], rows padded to 64 (with `fill`)"""
    M, K = X.shape
    Mp = roundup(M, 64)
    Xf = torch.full((Mp, K), fill, dtype=X.dtype, device=X.device)
    Xf[:M] = X
    return Xf.reshape(Mp // 64, 4, 16, K // 32, 4, 8).permute(0, 3, 1, 4, 2, 5).reshape(-1)


def unpack_x(flat, Mp, K):
    return flat.reshape(Mp // 64, K // 32, 4, 4, 16, 8).permute(0, 2, 4, 1, 3, 5).reshape(Mp, K)


def pack_fp8_formula(q8):
    """Wp8[n/16][k/64][lane][16 bytes]: bytes 0-7 the lane's 8 weights of k-step 2s, bytes 8-15 of k-step 2s+1"""
    N, K = q8.shape
    return q8.reshape(N // 16, 16, K // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).reshape(-1)


def fp8_quant(W):
    """(scale fp32 [N], q float8_e4m3fn [N, K]) as the header states them: max(amax, 1e-30f) / 448 and round-to-nearest-even of the fp32 quotient"""
    amax = W.float().abs().amax(1)
    scale = torch.maximum(amax, torch.tensor(1e-30, dtype=F32)) / torch.tensor(448.0, dtype=F32)
    return scale, (W.float() / scale[:, None]).to(torch.float8_e4m3fn)


def kpk_index():
    """[32 keys, 128 dims] -> offset inside a (page, kv head) block of the K cache (common.h kpk_off)"""
    r, dd = torch.arange(32)[:, None], torch.arange(128)[None, :]
    li, t = (r >> 3) * 4 + (r & 3), (r >> 2) & 1
    return ((((dd >> 5) * 2 + t) * 64) + ((dd >> 3) & 3) * 16 + li) * 8 + (dd & 7)


def test_cpu_layout_formulas_are_permutations():
    W = torch.arange(48 * 96, dtype=F32).reshape(48, 96)
    p = pack_w_formula(W)
    assert sorted(p.tolist()) == list(range(48 * 96)) and float(p[(1 * 3 + 2) * 512 + (5 + 16 * 3) * 8 + 6]) == float(W[16 + 5, 64 + 24 + 6])
    X = torch.arange(70 * 64, dtype=F32).reshape(70, 64) + 1
    xp = pack_x_formula(X)
    assert torch.equal(unpack_x(xp, 128, 64)[:70], X) and float(unpack_x(xp, 128, 64)[70:].abs().max()) == 0
    m, k = 69, 43          # common.h xpk_off
    off = (m >> 6) * 64 * 64 + ((k >> 5) * 4 + ((m & 63) >> 4)) * 512 + ((m & 15) + 16 * ((k >> 3) & 3)) * 8 + (k & 7)
    assert float(xp[off]) == float(X[m, k])
    assert sorted(gateup_rows(64).tolist()) == list(range(128)) and gateup_rows(64)[16:32].tolist() == list(range(64, 80))
    r = qkv_rows(2, 1)
    assert sorted(r.tolist()) == list(range(512)) and r[16:32].tolist() == list(range(8, 16)) + list(range(72, 80)) and r[384:].tolist() == list(range(384, 512))
    assert sorted(kpk_index().reshape(-1).tolist()) == list(range(4096))
    q = torch.arange(16 * 128, dtype=torch.int32).reshape(16, 128)
    pq = pack_fp8_formula(q)
    assert int(pq[(1 * 64 + 5 + 16 * 2) * 16 + 8 + 3]) == int(q[5, 64 + 32 + 16 + 3])


# ======================================================================================================================================================
# inputs, float64 references, bounds, emulation
# ======================================================================================================================================================

def hot_ks(K, ranges):
    ks = set()
    for t0 in (0, K - 32):
        ks.update(k for k in range(t0, t0 + 32) if k % 8 in (0, 7))
    for k0, k1 in ranges:
        ks.update((k0, k0 + 31, k1 - 32, k1 - 1))
    return sorted(ks, reverse=True)


def slice_ranges(c):
    out = []
    for z in range(c.ks):
        st = slice_steps(c, z)
        if st:
            assert st == list(range(st[0], st[-1] + 1))
            out.append((32 * st[0], 32 * st[-1] + 32))
    return out


def place_onehots(g, X, W, ks, wv, wrows_from=0):
    """one-hot rows into X (v e_k; never the last row) and W (wv e_k; rows >= wrows_from); returns their bookkeeping"""
    M, N = X.shape[0], W.shape[0]
    na, nb = min(2 * len(ks), M // 2), min(len(ks), (N - wrows_from) // 2)
    arows = torch.randperm(M - 1, generator=g)[:na].tolist()
    brows = (torch.randperm(N - wrows_from, generator=g)[:nb] + wrows_from).tolist()
    ak, av = [ks[i % len(ks)] for i in range(na)], [1.0 if i < len(ks) else -2.0 for i in range(na)]
    bk = [ks[i % len(ks)] for i in range(nb)]
    for r, k, v in zip(arows, ak, av):
        X[r] = 0
        X[r, k] = v
    for r, k in zip(brows, bk):
        W[r] = 0
        W[r, k] = wv
    bg = torch.ones(M, dtype=torch.bool)
    bg[arows] = False
    return {"arows": arows, "ak": ak, "av": av, "brows": brows, "bk": bk, "bg": bg.nonzero()[:, 0]}


E4M3_GRID = torch.arange(256, dtype=torch.int32).to(U8T).view(torch.float8_e4m3fn).float()
E4M3_GRID = E4M3_GRID[torch.isfinite(E4M3_GRID)]


@functools.lru_cache(maxsize=None)
def sk_inputs(c):
    """X [M, K], W [N, K] (mode 3: [gate; up] rows), bias [N]; FP8: rows 0 - 3 of W are all zero / e4m3-subnormal quotients / exact e4m3 multiples of 2^-3 / of 2^-11"""
    M, N, K = c.M, c.N, c.K
    g = gen(M * 7919 + N * 31 + K + 1000003 * c.mode + 17 * c.ks + (5 if c.fp8 else 0))
    X, W = torch.randn(M, K, generator=g), 0.5 * torch.randn(N, K, generator=g)
    if c.fp8:
        W[0] = 0
        W[1] = 2e-5 * torch.randn(K, generator=g).sign() * (0.25 + torch.rand(K, generator=g))
        W[1, K // 2] = 1.0
        for r, s in ((2, -3), (3, -11)):
            W[r] = E4M3_GRID[torch.randint(0, len(E4M3_GRID), (K,), generator=g)] * 2.0 ** s
            W[r, 5] = -448.0 * 2.0 ** s
    X, W = X.to(BF), W.to(BF)
    oh = place_onehots(g, X, W, hot_ks(K, slice_ranges(c)), 0.875 if c.fp8 else 1.0, 4 if c.fp8 else 0)
    bias = (2 * torch.randn(N, generator=g)).to(BF)
    assert normal_range(X) and normal_range(W) and normal_range(bias)
    I = {"c": c, "X": X, "W": W, "bias": bias, **oh}
    if c.fp8:
        scale, q = fp8_quant(W)
        qf = q.float()
        assert bool((qf.abs().amax(1)[1:] == 448).all()) and float(qf[0].abs().max()) == 0, "every non-zero row's largest element quantises to +-448"
        assert bool((qf[1].abs() < 2.0 ** -6).sum() > K // 2) and bool((qf[1] != 0).sum() > K // 4), "row 1: quotients in the e4m3 subnormal range"
        assert torch.equal(qf[2:4] * scale[2:4, None], W[2:4].float()) and float(scale[2]) == 2.0 ** -3 and float(scale[3]) == 2.0 ** -11, "rows 2, 3 are exact"
        assert all(float(scale[r]) == 2.0 ** -9 and float(qf[r, k]) == 448 for r, k in zip(oh["brows"], oh["bk"]))
        I.update(scale=scale, q=q, Wd=qf)
    else:
        I.update(scale=None, Wd=W.float())
    return I


def nK(c):
    return c.K + 16 + c.ks


def bxc(E, c):
    """the contraction's bound: 2^-24 (4 + 2 n) E, FP8 one rounding more"""
    return b_x(E, nK(c)) + (U24 * 2 * E if c.fp8 else 0)


def refs(c, I, dev="cpu"):
    """float64: the contraction x [M, N] with E, per slice xs [ks, M, N] with Es"""
    X, Wd = I["X"].to(dev).double(), I["Wd"].to(dev).double()
    sc = I["scale"].to(dev).double()[None, :] if c.fp8 else 1.0
    xs, Es = [], []
    for z in range(c.ks):
        st = slice_steps(c, z)
        if not st:
            xs.append(torch.zeros(c.M, c.N, dtype=F64, device=dev))
            Es.append(torch.zeros(c.M, c.N, dtype=F64, device=dev))
            continue
        cols = cols_of(st).to(dev)
        xs.append((X[:, cols] @ Wd[:, cols].t()) * sc)
        Es.append((X[:, cols].abs() @ Wd[:, cols].abs().t()) * sc)
    xs, Es = torch.stack(xs), torch.stack(Es)
    return {"x": xs.sum(0), "E": Es.sum(0), "xs": xs, "Es": Es}


def silu64(g):
    return g / (1 + torch.exp(-g))


def swiglu_unstored(xg, xu, bg_, bu_):
    """(ref, bound) of a where gate|up is not stored"""
    s = 1 / (1 + torch.exp(-xg))
    a = xg * s * xu
    dsilu = s * (1 + xg * (1 - s))
    return a, U8 * 3 * a.abs() + U24 * F_EXP * a.abs() + dsilu.abs() * xu.abs() * bg_ + (xg * s).abs() * bu_ + TINY


def bf16_bound(ref, E, c):
    return U8 * 2 * ref.abs() + bxc(E, c) + TINY


def outputs64(c, I, R, dev="cpu"):
    """[(key, ref, bound)] of the case's main output: mode 0 / 1 one [M, N]; mode 2 the slabs [ks M, N] and their sum; mode 3 a [M, I] (gate|up not stored)"""
    pre = "fp8." if c.fp8 else ""
    if c.mode == 0:
        b = I["bias"].to(dev).double() if has_bias(c) else torch.zeros(c.N, dtype=F64, device=dev)
        ref = R["x"] + b
        return [(pre + "bf16", ref, bf16_bound(ref, R["E"] + b.abs(), c))]
    if c.mode == 1:
        return [(pre + "f32", R["x"], bxc(R["E"], c) + TINY)]
    if c.mode == 2:
        return [(pre + "slab", R["xs"].reshape(-1, c.N), bxc(R["Es"], c).reshape(-1, c.N) + TINY), (pre + "slabsum", R["x"], bxc(R["E"], c) + TINY)]
    Ih = c.N // 2
    xg, xu, Eg, Eu = R["x"][:, :Ih], R["x"][:, Ih:], R["E"][:, :Ih], R["E"][:, Ih:]
    a, bound = swiglu_unstored(xg, xu, bf16_bound(xg, Eg, c), bf16_bound(xu, Eu, c))
    return [(pre + "swiglu.a", a, bound)]


def emu_slices(c, I):
    """fp32 [ks, M, N]: per slice the waves' chains in step order, added in wave order; FP8: times the row scale"""
    X, Wd = I["X"].double(), I["Wd"].double()
    out = []
    for waves in plan(c):
        tot = torch.zeros(c.M, c.N, dtype=F32)
        for steps in waves:
            acc = torch.zeros(c.M, c.N, dtype=F32)
            for t in steps:
                acc = acc + (X[:, 32 * t: 32 * t + 32] @ Wd[:, 32 * t: 32 * t + 32].t()).to(F32)
            tot = tot + acc
        out.append(tot * I["scale"][None, :] if c.fp8 else tot)
    return torch.stack(out)


def emu_swiglu(g, u):
    """store_swiglu: (gate|up bf16, a bf16)"""
    g, u = bfr(g), bfr(u)
    sg = bfr(g / (1 + torch.exp(-g)))
    return torch.cat([g, u], 1).to(BF), (sg * u).to(BF)


def emu_outputs(c, I):
    """the emulated main output in the layout of outputs64 (+ the emulated gate|up of mode 3)"""
    s = emu_slices(c, I)
    if c.mode == 0:
        return [(s[0] + I["bias"].float() if has_bias(c) else s[0]).to(BF)], None
    if c.mode == 1:
        return [s[0]], None
    if c.mode == 2:
        return [s.reshape(-1, c.N), s.double().sum(0)], None
    gu, a = emu_swiglu(s[0][:, : c.N // 2], s[0][:, c.N // 2:])
    return [a], gu


def z_of_k(c):
    z = torch.zeros(c.K, dtype=torch.long)
    for zz in range(c.ks):
        st = slice_steps(c, zz)
        if st:
            z[cols_of(st)] = zz
    return z


def onehot_expected(c, I, dev):
    """[(index into the main output, expected values)] of the one-hot rows of X and of W, as IEEE fixes them; mode 3: the expected gate|up rows of X's one-hot rows"""
    X, Wd, bias = I["X"].to(dev).float(), I["Wd"].to(dev).float(), I["bias"].to(dev).float()
    sc = I["scale"].to(dev) if c.fp8 else torch.ones(c.N, device=dev)
    ar, br = torch.tensor(I["arows"], dtype=torch.long, device=dev), torch.tensor(I["brows"], dtype=torch.long, device=dev)
    xr = (torch.tensor(I["av"], device=dev)[:, None] * Wd[:, I["ak"]].t()) * sc[None, :]          # [na, N]: the first product is exact, the scale multiply one fp32 rounding
    xc = (X[:, I["bk"]] * Wd[br, I["bk"]][None, :]) * sc[br][None, :]                            # [M, nb]
    if c.mode == 0:
        return [((ar, slice(None)), (xr + bias[None, :] if has_bias(c) else xr).to(BF)), ((slice(None), br), (xc + bias[None, br] if has_bias(c) else xc).to(BF))]
    if c.mode == 1:
        return [((ar, slice(None)), xr), ((slice(None), br), xc)]
    if c.mode == 2:
        zk = z_of_k(c).to(dev)
        sel = torch.arange(c.ks, device=dev)[:, None, None]
        er = torch.where(zk[I["ak"]][None, :, None] == sel, xr[None], torch.zeros_like(xr)[None])          # [ks, na, N]
        ec = torch.where(zk[I["bk"]][None, None, :] == sel, xc[None], torch.zeros_like(xc)[None])          # [ks, M, nb]
        return [((slice(None), ar, slice(None)), er), ((slice(None), slice(None), br), ec)]
    return [((ar, slice(None)), xr.to(BF))]


def check_onehots(c, I, got, what):
    """got: the main output ([ks, M, N] in mode 2); values compared (0 == -0), dtypes too"""
    for idx, want in onehot_expected(c, I, got.device):
        g = got[idx]
        assert g.dtype == want.dtype and g.shape == want.shape and torch.equal(g, want), f"{what}: the output of a one-hot operand row is not the other operand's column, bit for bit"


def check_swiglu_onehot_a(c, I, a, what):
    """mode 3: a of X's one-hot rows is the one correct bit pattern where there is only one"""
    (idx, gu), = onehot_expected(c, I, "cpu")
    want, ok = swiglu_exact(gu)
    assert int(ok.sum()) > ok.numel() // 8, what
    assert torch.equal(a.cpu()[idx[0]].float()[ok], want.float()[ok]), f"{what}: a of a one-hot row differs from bf16(bf16(silu(gate)) up) (the sign of a zero apart)"


def check_stored_swiglu(side, pre, a, gu, what):
    """a against float64 SwiGLU of the stored bf16 gate|up rows (the token-wise swiglu.a entry)"""
    gu, a = gu.cpu(), a.cpu()
    m = swiglu_math(gu, torch.zeros(gu.shape[0], gu.shape[1] // 2), False)
    mx = float(frac("swiglu.a", a, m["a"], m["E_a"]).max())
    USED[side][pre + "swiglu.a_of_gu"] = max(USED[side].get(pre + "swiglu.a_of_gu", 0.0), mx)
    assert mx <= 1.0, f"{what}: a at {mx:.3g} x the token-wise bound on the stored gate|up"
    want, ok = swiglu_exact(gu)
    assert torch.equal(bits(a)[ok], bits(want)[ok]), f"{what}: a differs from bf16(bf16(silu(gate)) up) where that is one value"


# ---- fault models of the plain entry points ----

def drop_steps(c, R, I, z, steps):
    """slab z of the float64 reference without the given 32-steps"""
    X, Wd = I["X"].double(), I["Wd"].double()
    sc = I["scale"].double()[None, :] if c.fp8 else 1.0
    cols = cols_of(steps)
    return R["xs"][z] - (X[:, cols] @ Wd[:, cols].t()) * sc


def main_from_slabs(c, I, xs):
    """the float64 main output (layout of outputs64, first entry) from faulty float64 slabs; mode 3: a"""
    if c.mode == 0:
        return xs.sum(0) + (I["bias"].double() if has_bias(c) else 0)
    if c.mode == 1:
        return xs.sum(0)
    if c.mode == 2:
        return xs.reshape(-1, c.N)
    x = xs.sum(0)
    return silu64(x[:, : c.N // 2]) * x[:, c.N // 2:]


def slab_rows(c, z, rows):
    return [z * c.M + int(r) for r in rows] if c.mode == 2 else rows


def cpu_plain_faults(c, I, R, outs):
    key, ref, bound = outs[0]
    bg, M, N, K = I["bg"], c.M, c.N, c.K
    narrow, last = c.kern.startswith("narrow"), c.ks - 1
    unit = unit_of(c)

    def faulty(z, xz):
        xs = R["xs"].clone()
        xs[z] = xz
        return main_from_slabs(c, I, xs)

    if narrow and K & 32:
        fexcess("ktail_dropped", faulty(last, drop_steps(c, R, I, last, [K // 32 - 1])), ref, bound, rows=slab_rows(c, last, bg))
        if c.ks > 1 and slice_steps(c, 0):
            tail = R["xs"][last] - drop_steps(c, R, I, last, [K // 32 - 1])
            fexcess("ktail_every_slice", faulty(0, R["xs"][0] + tail), ref, bound, rows=slab_rows(c, 0, bg))
    if c.kern.startswith(("narrow", "wide")):
        for z in range(c.ks):
            dropped = []
            for wi, w in enumerate(plan(c)[z]):
                body = w[:-1] if (narrow and K & 32 and z == last and wi == 0) else w          # (without the tail step)
                if (len(body) // unit) % 2:          # an odd number of units: the wave's last trip is a single one
                    dropped += body[-unit:]
            if dropped:
                fexcess("last_single_trip_skipped", faulty(z, drop_steps(c, R, I, z, dropped)), ref, bound, rows=slab_rows(c, z, bg))
                break
    if c.ks > 1:
        st0 = slice_steps(c, 0)
        nxt = next((z for z in range(1, c.ks) if slice_steps(c, z)), None)
        if st0 and nxt is not None and len(slice_steps(c, nxt)) >= unit:
            moved = slice_steps(c, nxt)[:unit]
            xs = R["xs"].clone()
            part = R["xs"][nxt] - drop_steps(c, R, I, nxt, moved)
            xs[0], xs[nxt] = xs[0] + part, xs[nxt] - part
            fexcess("slice_boundary_off_by_one", main_from_slabs(c, I, xs), ref, bound, rows=slab_rows(c, 0, bg))
            assert float((xs.sum(0) - R["x"]).abs().max()) <= 1e-9 * float(R["E"].max()), "the slab sum does not see this fault"
        if not narrow:
            per_z = ceil_div(K // (32 * unit), c.ks)
            zl = max(z for z in range(c.ks) if slice_steps(c, z))
            if len(slice_steps(c, zl)) < per_z * unit and not c.packed:          # the steps past K: X reads the poison of the columns K .. ldx, W the next tile
                past = POISON * I["Wd"].double()[:, :8].abs().sum(-1)[None, :].expand(M, N)
                fexcess("last_slice_per_z", faulty(zl, R["xs"][zl] + past + 1.0), ref, bound, rows=slab_rows(c, zl, bg))
        empty = [z for z in range(c.ks) if not slice_steps(c, z)]
        if empty:
            fexcess("empty_slice_sentinel", faulty(empty[0], torch.full((M, N), SENT, dtype=F64)), ref, bound, rows=slab_rows(c, empty[0], range(M)))
    if c.kern.startswith("split"):
        ksw = {S6: 6, S10: 10, S3F: 3}[c.kern]
        nstep = K // (32 * unit)
        per_z = ceil_div(nstep, c.ks)
        st_end = min(nstep, per_z)
        extra = [(st, st_end - 1) for w in range(8) for j in range(ksw) for st in [w + j * 8] if st_end <= st < nstep]
        if extra:          # slice 0: X of the step past the end (not zeroed) times the clamped W step
            X, Wd = I["X"].double(), I["Wd"].double()
            sc = I["scale"].double()[None, :] if c.fp8 else 1.0
            add = sum(X[:, cols_of(range(unit * sx, unit * sx + unit))] @ Wd[:, cols_of(range(unit * sw, unit * sw + unit))].t() for sx, sw in extra) * sc
            fexcess("wave_past_end_clamped_w", faulty(0, R["xs"][0] + add), ref, bound, rows=slab_rows(c, 0, bg))
    if c.kern == N28 and c.mode != 2:
        ldy = N + 8          # the duplicate of tile 512 stored at columns N .. N + 16: 8 sentinel columns, then the next row's first 8
        img = torch.full((M, ldy), SENT, dtype=F64)
        img[:, :N] = ref
        good = img.clone()
        flat = img.reshape(-1)
        for m in range(M - 1):
            flat[m * ldy + N: m * ldy + N + 16] = ref[m, N - 16:]
        fexcess("duplicate_tile_stored", img[:, :N], ref, bound, rows=list(range(1, M)), cols=slice(0, 8))
        fbits("duplicate_tile_stored", img[:, N:].contiguous(), good[:, N:].contiguous())
    if (M - 1) % 64 >= 16 and c.mode in (0, 1):
        bad = ref.clone()
        bad[M - 1] = ref[(M - 1) // 64 * 64 + (M - 1) % 16]
        fexcess("rows_ge_M_from_row0", bad, ref, bound, rows=[M - 1])
    if c.mode == 3:
        Ih = N // 2
        xg, xu = R["x"][:, :Ih], R["x"][:, Ih:]
        fexcess("gate_up_swapped", silu64(xu) * xg, ref, bound, rows=bg)
        fexcess("up_from_tile_2r", silu64(xg) * xg, ref, bound, rows=bg)
        if c.fp8:
            sc = I["scale"].double()
            ok = ((sc[:Ih] / sc[Ih:] - 1).abs() > 0.05).nonzero()[:, 0]
            fexcess("fp8_upscale_wscale_gn", silu64(xg) * (xu * (sc[:Ih] / sc[Ih:])[None, :]), ref, bound, rows=bg, cols=ok)
        if c.kern.startswith("pers") and (M, N, K) in SIDE_CASES:
            base, ss, step, rows_total = SIDE_GEOM[0], SIDE_GEOM[1], SIDE_GEOM[2], SIDE_GEOM[0] + (M - 1) * SIDE_GEOM[1] + SIDE_GEOM[2] + 1
            img = torch.full((rows_total, Ih), SENT, dtype=F64)
            img[base + torch.arange(M) * ss] = ref
            fexcess("side_row_without_step", img[base + torch.arange(M) * ss + step], ref, bound, rows=list(range(M - 1)))
            if c.cus % 8:          # the XCD order with gstep = bps >> 3 = 0: a block would not get past its first group b * 4 (the others keep the sentinel)
                done = torch.zeros(Ih, dtype=torch.bool)
                for b in range(c.cus):
                    done[(b * 4) * 16: (b * 4) * 16 + 16] = True
                bad = torch.where(done[None, :], ref, torch.full_like(ref, SENT))
                fexcess("xcd_order_bps_not_8", bad, ref, bound, rows=list(range(M)), cols=(~done).nonzero()[:, 0])
    if c.fp8 and c.mode in (0, 1):
        X, q, sc = I["X"].double(), I["Wd"].double(), I["scale"].double()
        qs = q.reshape(N, K // 64, 2, 32).flip(2).reshape(N, K)
        b = I["bias"].double() if has_bias(c) else 0
        fexcess("fp8_halves_swapped", (X @ qs.t()) * sc[None, :] + b, ref, bound, rows=bg)
        sx = sc[torch.arange(N) ^ 1]
        cols = [n for n in range(4, N) if abs(float(sx[n] / sc[n]) - 1) > 0.05]
        fexcess("fp8_scale_row_xor_1", (X @ q.t()) * sx[None, :] + b, ref, bound, rows=bg, cols=cols)


SIDE_GEOM = (2, 3, 1)          # base, seq_stride, *step of the side arenas


@pytest.mark.parametrize("c", BF16_CASES + FP8_CASES, ids=cid)
def test_cpu_skinny_emulation_inside_and_faults_outside(c):
    I = sk_inputs(c)
    R = refs(c, I)
    outs = outputs64(c, I, R)
    emu, gu = emu_outputs(c, I)
    what = cid(c)
    for (key, ref, bound), e in zip(outs, emu):
        check("emu", key, e, ref, bound, what + " (emulation)")
    s = emu_slices(c, I) if c.mode == 2 else None
    if c.mode == 2:
        check_onehots(c, I, s, what + " (emulation)")
        for z in range(c.ks):
            if not slice_steps(c, z):
                assert float(s[z].abs().max()) == 0
    elif c.mode == 3:
        pre = "fp8." if c.fp8 else ""
        check("emu", pre + "swiglu.gu", gu, R["x"], bf16_bound(R["x"], R["E"], c), what + " (emulation)")
        check_stored_swiglu("emu", pre, emu[0], gu, what + " (emulation)")
        check_onehots(c, I, gu, what + " (emulation)")
        check_swiglu_onehot_a(c, I, emu[0], what + " (emulation)")
    else:
        check_onehots(c, I, emu[0], what + " (emulation)")
    cpu_plain_faults(c, I, R, outs)


# ======================================================================================================================================================
# q|k|v: inputs, float64 reference, emulation, fault models
# ======================================================================================================================================================

@functools.lru_cache(maxsize=None)
def qkv_base(Hq, Hkv, K):
    """70 rows; a case of M rows takes the first M.  Rows 0 / 1 (and 17 / 18): tables (1, 0) / (0, 1); rows 2, 3: one-hot with those tables; W has one-hot rows"""
    N = (Hq + 2 * Hkv) * 128
    g = gen(Hq * 131 + Hkv * 17 + K)
    X, W = torch.randn(70, K, generator=g), 0.5 * torch.randn(N, K, generator=g)
    ks = hot_ks(K, [])
    X, W = X.to(BF), W.to(BF)
    X[2], X[3] = 0, 0
    X[2, ks[0]], X[3, ks[-1]] = 1.0, -2.0
    brows = torch.randperm(N, generator=g)[: len(ks)].tolist()
    for r, k in zip(brows, ks):
        W[r] = 0
        W[r, k] = 1.0
    bias = (2 * torch.randn(N, generator=g)).to(BF)
    ang = torch.rand(70, 64, generator=g, dtype=F64) * 6.283
    cos, sin = ang.cos().to(F32), ang.sin().to(F32)
    for r, (cc, ss) in {0: (1, 0), 1: (0, 1), 2: (1, 0), 3: (0, 1), 17: (1, 0), 18: (0, 1)}.items():
        cos[r], sin[r] = cc, ss
    assert normal_range(X) and normal_range(W) and normal_range(bias)
    return {"X": X, "W": W, "bias": bias, "cos": cos, "sin": sin, "brows": brows, "bk": ks[: len(brows)], "N": N}


def qkv_slots(M, P):
    g = gen(M * 13 + P)
    pages = torch.randperm(P, generator=g)[:M]
    off = torch.randint(0, 32, (M,), generator=g)
    off[0], off[min(4, M - 1)] = 0, 31
    slot = pages * 32 + off
    slot[M // 2], slot[M - 1] = -1, -5
    return slot.to(torch.int64)


def qkv_inputs(q, packed):
    B = qkv_base(q.Hq, q.Hkv, q.K)
    P = 2 * q.M + 5 if packed else q.M + 3
    I = {k: (v[: q.M] if k in ("X", "cos", "sin") else v) for k, v in B.items()}
    I.update(P=P, slot=qkv_slots(q.M, P))
    return I


def rot64(proj, cos, sin, Hrope, partner=64, sign=1.0):
    """float64 rotary of the first Hrope heads of proj [M, heads 128]; returns (out, a cos, b sin terms' absolute sum, index of the partner)"""
    M = proj.shape[0]
    p = proj.reshape(M, -1, 128).clone()
    a, b = p[:, :Hrope, :64], p[:, :Hrope, 64:]
    if partner != 64:          # the fault model: dim d pairs with d + 32 inside each half
        b = torch.cat([p[:, :Hrope, 32:64], p[:, :Hrope, :32]], -1)
    cc, ss = cos.double()[:, None, :], sin.double()[:, None, :]
    out = p.clone()
    out[:, :Hrope, :64] = a * cc - sign * b * ss
    out[:, :Hrope, 64:] = p[:, :Hrope, 64:] * cc + sign * (a if partner == 64 else torch.cat([p[:, :Hrope, 96:], p[:, :Hrope, 64:96]], -1)) * ss
    return out.reshape(M, -1)


def qkv_refs(q, I, dev="cpu"):
    """float64 [M, N] in the training layout [q heads | k heads | v heads] with its bound"""
    X, W, b = I["X"].to(dev).double(), I["W"].to(dev).double(), I["bias"].to(dev).double()
    cos, sin = I["cos"].to(dev), I["sin"].to(dev)
    Hr, M = q.Hq + q.Hkv, q.M
    c = Case(M, I["N"], q.K, 0, 1, q.cus, False, False, q.kern)
    proj, E = X @ W.t() + b, X.abs() @ W.abs().t() + b.abs()
    bp = bf16_bound(proj, E, c)
    ref = rot64(proj, cos, sin, Hr)
    p3, b3 = proj.reshape(M, -1, 128), bp.reshape(M, -1, 128)
    cc, ss = cos.double().abs()[:, None, :], sin.double().abs()[:, None, :]
    bound = bp.clone().reshape(M, -1, 128)
    lo, hi = slice(0, 64), slice(64, 128)
    for me, other in ((lo, hi), (hi, lo)):
        bound[:, :Hr, me] = cc * b3[:, :Hr, me] + ss * b3[:, :Hr, other] + 4 * U24 * (p3[:, :Hr, me].abs() * cc + p3[:, :Hr, other].abs() * ss)
    bound = bound.reshape(M, -1)
    rot_cols = torch.arange(I["N"], device=dev) < Hr * 128
    bound = torch.where(rot_cols[None, :], bound + U8 * 2 * ref.abs() + TINY, bound)
    return {"proj": proj, "ref": ref, "bound": bound, "Hr": Hr, "case": c}


def emu_qkv(q, I):
    c = Case(q.M, I["N"], q.K, 0, 1, q.cus, False, False, N4 if q.kern == NFV else q.kern)
    J = {"X": I["X"], "Wd": I["W"].float(), "scale": None}
    vs = bfr(emu_slices(c, J)[0] + I["bias"].float())
    Hr, M = q.Hq + q.Hkv, q.M
    p = vs.reshape(M, -1, 128)
    a, b, cc, ss = p[:, :Hr, :64], p[:, :Hr, 64:], I["cos"][:, None, :], I["sin"][:, None, :]
    out = p.clone()
    out[:, :Hr, :64] = a * cc - b * ss
    out[:, :Hr, 64:] = b * cc + a * ss
    return out.reshape(M, -1).to(BF), vs.to(BF)


def exact_rows_expected(q, I, proj_bf):
    """{row: expected [N] bf16} for the rows with exact tables, from the bf16 projection: (1, 0) -> itself, (0, 1) -> the partner, negated in the first half"""
    Hr, out = q.Hq + q.Hkv, {}
    for r in range(q.M):
        cs = (float(I["cos"][r].min()), float(I["cos"][r].max()), float(I["sin"][r].min()), float(I["sin"][r].max()))
        if cs not in ((1, 1, 0, 0), (0, 0, 1, 1)):
            continue
        p = proj_bf[r].float().reshape(-1, 128).clone()
        if cs == (0, 0, 1, 1):
            p[:Hr] = torch.cat([-p[:Hr, 64:], p[:Hr, :64]], -1)
        out[r] = p.reshape(-1).to(BF)
    return out


def values_equal(a, b):
    """equal as numbers (0 == -0), same dtype"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu().float(), b.cpu().float())


@pytest.mark.parametrize("q", QKV_CASES, ids=qid)
def test_cpu_qkv_emulation_inside_and_faults_outside(q):
    I = qkv_inputs(q, False)
    R = qkv_refs(q, I)
    ref, bound, Hr, M, N = R["ref"], R["bound"], R["Hr"], q.M, I["N"]
    out, vs = emu_qkv(q, I)
    rot, vcols = slice(0, Hr * 128), slice(Hr * 128, N)
    check("emu", "qkv.rot", out[:, rot], ref[:, rot], bound[:, rot], qid(q) + " (emulation)")
    check("emu", "qkv.v", out[:, vcols], ref[:, vcols], bound[:, vcols], qid(q) + " (emulation)")
    for r, want in exact_rows_expected(q, I, vs).items():
        assert values_equal(out[r], want), f"{qid(q)}: exact-table row {r} (emulation)"
    bgr = [r for r in range(M) if r not in (0, 1, 2, 3, 17, 18)]
    proj, b = R["proj"], I["bias"].double()
    perm = qkv_rows(q.Hq, q.Hkv)
    # the packer's bias left in natural order: packed tile column c gets bias[c] instead of bias[perm[c]]
    nat = torch.empty(N, dtype=F64)
    nat[perm] = b          # what output row perm[c] then receives
    fexcess("bias_unpermuted", rot64(proj - b + nat, I["cos"], I["sin"], Hr)[:, rot], ref[:, rot], bound[:, rot], rows=bgr)
    if q.kern == NFV:          # the fused V tile's bias taken from the K tile of the same head and slice
        bad = ref.clone()
        kb = b[q.Hq * 128:(q.Hq + q.Hkv) * 128][perm[q.Hq * 128:(q.Hq + q.Hkv) * 128] - q.Hq * 128]          # bias_p of the K tiles, in tile order
        bad[:, vcols] = ref[:, vcols] - b[vcols] + kb
        fexcess("fusedv_bias_from_k_tile", bad[:, vcols], ref[:, vcols], bound[:, vcols], rows=bgr)
    fexcess("rope_partner_d32", rot64(proj, I["cos"], I["sin"], Hr, partner=32)[:, rot], ref[:, rot], bound[:, rot], rows=bgr)
    fexcess("rope_sign_flipped", rot64(proj, I["cos"], I["sin"], Hr, sign=-1.0)[:, rot], ref[:, rot], bound[:, rot], rows=bgr)
    if M > 16:
        idx = torch.arange(M) // 64 * 64 + torch.arange(M) % 16
        rows = [r for r in bgr if int(idx[r]) != r]
        fexcess("rope_row_gm0", rot64(proj, I["cos"][idx], I["sin"][idx], Hr)[:, rot], ref[:, rot], bound[:, rot], rows=rows)
    # caches: images of one (page, head) block per row
    kcols = slice(q.Hq * 128, q.Hq * 128 + 128)
    kidx = kpk_index()
    off = (I["slot"] & 31).clamp(min=0)
    img = torch.full((M, 4096), SENT, dtype=F64)
    img[torch.arange(M)[:, None], off[:, None] * 128 + torch.arange(128)[None, :]] = ref[:, kcols]
    got = img[torch.arange(M)[:, None], kidx[off]]
    fexcess("kcache_row_major", got, ref[:, kcols], bound[:, kcols], rows=[r for r in bgr if int(off[r]) > 0])
    lead = torch.full((2 * q.Hkv, 4096), SENT, dtype=F64)
    bad = lead.clone()
    neg = [r for r in range(M) if int(I["slot"][r]) < 0]
    assert len(neg) == 2 and M // 2 in neg and M - 1 in neg
    for r in neg:          # page = slot >> 5 = -1, offset = slot & 31: the write lands in the sentinel rows in front of the cache
        sl = int(I["slot"][r])
        bad[((sl >> 5) + 2) * q.Hkv, torch.arange(128) * 32 + (sl & 31)] = ref[r, vcols][:128]
    fbits("vcache_written_slot_neg", bad, lead)


def test_cpu_every_fault_model_was_exercised_and_emulation_record():
    """Every fault model of FAULT_MODELS was applied somewhere above (run the whole CPU part: this test reads what the others recorded)."""
    missing = [f for f in FAULT_MODELS if f not in FAULT_SEEN]
    assert not missing, f"fault models never exercised: {missing}"
    for f in FAULT_MODELS:
        print(f"[skinny_f64 cpu] fault {f}: smallest excess at its designated elements {FAULT_SEEN[f]:.3g} x bound")
    _print_used("emu")
    assert all(v <= 1.0 for v in USED["emu"].values())


def _print_used(side):
    for key, v in sorted(USED[side].items()):
        print(f"[skinny_f64 {side}] {key}: largest used fraction of the bound {v:.4f}")


# ======================================================================================================================================================
# GPU part
# ======================================================================================================================================================

@contextlib.contextmanager
def decode_cus(n):
    """thread-local launcher state other tests rely on: always reset"""
    hip.set_decode_cus(n)
    try:
        yield
    finally:
        hip.set_decode_cus(0)


def filled_guard(rows, cols, dtype, ld, init, fill):
    """a Guard whose padding holds `fill` (finite) instead of the sentinel pattern"""
    g_ = Guard(rows, cols, dtype, ld, init)
    if fill is not None:
        g_.buf.fill_(fill)
        g_.view.copy_(init.to(DEV))
        g_.saved = g_.buf.clone()
    return g_


def x_operand(X, packed, fill):
    """(Guard, ldx): row-major with ldx = K + 8, or decode-packed by the index formula with `fill` (finite) in the pad rows"""
    M, K = X.shape
    if packed:
        flat = pack_x_formula(X, -704.0 if fill is None else fill)
        return filled_guard(1, flat.numel(), BF, None, flat[None, :], fill), 0
    return filled_guard(M, K, BF, K + 8, X, fill), K + 8


def pack_weight_gpu(W, kind, what, Hq=0, Hkv=0, bias=None):
    """runs the packer on a row-major W (ldw = K + 16, poison in the padding), checks it against the index formula bit for bit, returns the packed Guard(s)"""
    N, K = W.shape
    Wg = Guard(N, K, BF, K + 16, W)
    Wp = Guard(1, N * K, BF)
    if kind == "plain":
        call_guarded("pack_weight_bf16", (Wg, K + 16, Wp, N, K), (Wp,), what)
        want = pack_w_formula(W)
    elif kind == "gateup":
        call_guarded("pack_gateup_bf16", (Wg, K + 16, Wp, N // 2, K), (Wp,), what)
        want = pack_w_formula(W[gateup_rows(N // 2)])
    else:
        bp, bg_ = vec(N, BF), vec(N, BF, bias)
        call_guarded("pack_qkv_rope_bf16", (Wg, K + 16, bg_, Wp, bp, Hq, Hkv, 128, K), (Wp, bp), what)
        bg_.untouched("bias")
        perm = qkv_rows(Hq, Hkv)
        want = pack_w_formula(W[perm])
        assert same_bits(bp.view[0], bias[perm].to(DEV)), f"{what}: the permuted bias"
        bp.saved = bp.buf.clone()
    assert same_bits(Wp.view[0], want.to(DEV)), f"{what}: pack ({kind}) differs from the layout formula"
    Wg.untouched("W")
    Wp.saved = Wp.buf.clone()          # from here on an input that must not change
    return (Wp, bp) if kind == "qkv" else Wp


def pack_fp8_gpu(I, gateup, what):
    c, W = I["c"], I["W"]
    N, K = W.shape
    Wg = Guard(N, K, BF, K + 16, W)
    Wp, sc = Guard(1, N * K, U8T), vec(N, F32)
    call_guarded("pack_weight_fp8", (Wg, K + 16, Wp, sc, N, K, N // 2 if gateup else 0), (Wp, sc), what)
    assert same_bits(sc.view[0], I["scale"].to(DEV)), f"{what}: scale[n] != max(amax, 1e-30f) / 448 in fp32"
    q8 = I["q"].view(U8T)
    want = pack_fp8_formula(q8[gateup_rows(N // 2)] if gateup else q8)
    assert torch.equal(Wp.view[0].cpu(), want), f"{what}: an FP8 byte differs from torch.float8_e4m3fn of the fp32 quotient"
    Wg.untouched("W")
    Wp.saved = Wp.buf.clone()          # from here on an input that must not change
    return Wp, sc


def make_side(M, N):
    base, ss, step = SIDE_GEOM
    R = base + (M - 1) * ss + step + 2
    p0, p1 = Guard(R, N, BF, N + 8), Guard(R, N // 2, BF, N // 2 + 8)
    stp = torch.tensor([step], dtype=torch.int32, device=DEV)
    rows = base + torch.arange(M, device=DEV) * ss + step
    return p0, p1, stp, rows


def side_struct(p0, p1, stp):
    base, ss, _ = SIDE_GEOM
    return SideOut.make(stp, base, ss, p0=p0.view if p0 is not None else None, p1=p1.view if p1 is not None else None)


def other_rows_intact(g_, rows, what):
    R, cols, ld = g_.view.shape[0], g_.view.shape[1], g_.view.stride(0)
    keep = torch.ones(R, dtype=torch.bool, device=DEV)
    keep[rows] = False
    saved = g_.saved.view(-1, ld)[2: 2 + R, :cols]
    assert same_bits(g_.view[keep], saved[keep]), f"{what}: a side-arena row other than base + s seq_stride + *step was written"


def launch_plain(c, I, Wp, sc, fill, ldy_kind="rowmajor", side=None):
    """one launch of the case; returns the main output as a tensor in the layout of outputs64 (mode 2: [ks, M, N]; mode 3: a [M, I]) and the Y guard"""
    M, N, K = c.M, c.N, c.K
    Xg, ldx = x_operand(I["X"], c.packed, fill)
    odd = (M, N, K, c.mode) in ODD_LDY
    what = cid(c) + f" fill={fill} Y={ldy_kind}" + (" side" if side else "")
    bias = vec(N, BF, I["bias"]) if has_bias(c) else None
    cols = N // 2 if c.mode == 3 else N
    dtype = BF if c.mode in (0, 3) else F32
    if ldy_kind == "packed":
        Yg, ldy = Guard(1, roundup(M, 64) * cols, BF), 0
    else:
        ldy = cols + (3 if odd else 8)
        Yg = Guard(M * c.ks, cols, dtype, ldy)
    guards = (Yg,) + ((side[0], side[1]) if side else ())
    sptr = None
    if side:
        so = side_struct(side[0], side[1], side[2])
        sptr = ctypes.addressof(so)
    with decode_cus(c.cus):
        if c.fp8:
            call_guarded("gemm_skinny_fp8w", (Xg, Wp, sc.view, Yg, bias, M, N, K, ldx, ldy, c.mode, c.ks), guards, what)
        else:
            call_guarded("gemm_skinny_bf16", (Xg, Wp, Yg, bias, M, N, K, ldx, K, ldy, c.mode, c.ks, sptr), guards, what)
    Xg.untouched("X")
    Wp.untouched("packed W")
    if bias is not None:
        bias.untouched("bias")
    if ldy_kind == "packed":
        Mp = roundup(M, 64)
        y, y0 = unpack_x(Yg.view[0], Mp, cols), unpack_x(Yg.saved[2 * Yg.view.shape[1]: 3 * Yg.view.shape[1]], Mp, cols)
        assert same_bits(y[M:], y0[M:]), f"{what}: a pad row of the decode-packed Y was written"
        return y[:M].clone(), Yg
    out = Yg.view.clone()
    return (out.reshape(c.ks, M, N) if c.mode == 2 else out), Yg


def gpu_plain_case(c):
    I = sk_inputs(c)
    R = refs(c, I, DEV)
    outs = outputs64(c, I, R, DEV)
    what, pre = cid(c), ("fp8." if c.fp8 else "")
    if c.fp8:
        Wp, sc = pack_fp8_gpu(I, c.mode == 3, what)
    else:
        Wp, sc = pack_weight_gpu(I["W"], "gateup" if c.mode == 3 else "plain", what), None
    y1, _ = launch_plain(c, I, Wp, sc, None)
    y2, _ = launch_plain(c, I, Wp, sc, 3.0)
    assert same_bits(y1, y2), f"{what}: the result depends on what X's padding holds (or differs from run to run)"
    if c.mode == 2:
        check("gpu", outs[0][0], y1.reshape(-1, c.N), outs[0][1], outs[0][2], what)
        check("gpu", outs[1][0], y1.double().sum(0), outs[1][1], outs[1][2], what)
        check_onehots(c, I, y1, what)
        for z in range(c.ks):
            if not slice_steps(c, z):
                assert float(y1[z].abs().max()) == 0, f"{what}: the slab of the empty slice {z} is not zero"
        return
    check("gpu", outs[0][0], y1, outs[0][1], outs[0][2], what)
    if c.mode != 3:
        check_onehots(c, I, y1, what)
        return
    check_swiglu_onehot_a(c, I, y1, what)
    yp, _ = launch_plain(c, I, Wp, sc, None, ldy_kind="packed")
    assert same_bits(yp, y1), f"{what}: the decode-packed Y differs from the row-major one"
    if (c.M, c.N, c.K) in SIDE_CASES and not c.fp8:
        p0, p1, stp, rows = make_side(c.M, c.N)
        ys, _ = launch_plain(c, I, Wp, sc, None, side=(p0, p1, stp))
        assert same_bits(ys, y1), f"{what}: Y with side outputs differs from Y with side == NULL"
        other_rows_intact(p0, rows, what)
        other_rows_intact(p1, rows, what)
        gu, a = p0.view[rows], p1.view[rows]
        assert same_bits(a, y1), f"{what}: the side activation row differs from the main Y row"
        check("gpu", "swiglu.gu", gu, R["x"], bf16_bound(R["x"], R["E"], c), what)
        check_onehots(c, I, gu, what)
        for n, k in zip(I["brows"], I["bk"]):
            assert values_equal(gu[:, n], I["X"][:, k]), f"{what}: gate|up column {n} of a one-hot W row"
        check_stored_swiglu("gpu", "", a, gu, what)
        Ih = c.N // 2
        gg, a2 = Guard(c.M, c.N, BF, c.N + 8, gu), Guard(c.M, Ih, BF, Ih + 8)
        call_guarded("swiglu_fwd", (gg, c.N + 8, a2, Ih + 8, c.M, Ih), (a2,), what)
        assert same_bits(a2.view, a), f"{what}: a differs from swiglu_fwd on the stored gate|up rows"


@pytest.mark.gpu
@pytest.mark.parametrize("c", BF16_CASES, ids=cid)
def test_gpu_gemm_skinny_bf16(c):
    """every bf16 instantiation against float64, slab by slab; packers against the layout formula; one-hot rows, sentinels, poison, side rows bit for bit"""
    gpu_plain_case(c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", FP8_CASES, ids=cid)
def test_gpu_gemm_skinny_fp8w(c):
    """the FP8 pack bit for bit against torch.float8_e4m3fn, then every FP8 instantiation against float64 of (x . q) scale"""
    gpu_plain_case(c)


@pytest.mark.gpu
def test_gpu_pack_act():
    """pack_act against the index formula, ldx = K + 8 with poison in the padding; the pad rows M .. roundup64 are zero"""
    for M, K in ((5, 32), (70, 96), (64, 160), (129, 64)):
        X = torch.randn(M, K, generator=gen(M + K)).to(BF)
        Xg, Xp = Guard(M, K, BF, K + 8, X), Guard(1, roundup(M, 64) * K, BF)
        call_guarded("pack_act_bf16", (Xg, K + 8, Xp, M, K), (Xp,), f"pack_act M={M} K={K}")
        assert same_bits(Xp.view[0], pack_x_formula(X, 0.0).to(DEV)), f"pack_act M={M} K={K}: differs from the layout formula (pad rows zero)"
        Xg.untouched("X")


@pytest.mark.gpu
def test_gpu_narrow_row_bits_do_not_depend_on_MG():
    """the same X rows at M = 5, 20, 70 through MG 1, 2, 4 of the narrow kernel give the same output rows"""
    N, K = 80, 2144
    g = gen(77)
    X, W, bias = torch.randn(70, K, generator=g).to(BF), (0.5 * torch.randn(N, K, generator=g)).to(BF), (2 * torch.randn(N, generator=g)).to(BF)
    Wp = pack_weight_gpu(W, "plain", "MG rows")
    ys = []
    for M in (5, 20, 70):
        Xg, Yg = Guard(M, K, BF, K + 8, X[:M]), Guard(M, N, BF, N + 8)
        with decode_cus(1024):
            call_guarded("gemm_skinny_bf16", (Xg, Wp, Yg, vec(N, BF, bias), M, N, K, K + 8, K, N + 8, 0, 1, None), (Yg,), f"MG rows M={M}")
        ys.append(Yg.view.clone())
    assert same_bits(ys[0], ys[2][:5]) and same_bits(ys[1], ys[2][:20]), "a row's bits depend on MG"


def launch_qkv(q, I, Wp, bp, packed, fill, with_side):
    M, K, N, P, Hkv = q.M, q.K, I["N"], I["P"], q.Hkv
    Xg, ldx = x_operand(I["X"], packed, fill)
    ldq = q.Hq * 128 + 8
    Qg, Kc, Vc = Guard(M, q.Hq * 128, BF, ldq), Guard(P * Hkv, 4096, BF), Guard(P * Hkv, 4096, BF)
    base, ss, step = SIDE_GEOM
    Sg = Guard(base + (M - 1) * ss + step + 2, N, BF, N + 8) if with_side else None
    stp = torch.tensor([step], dtype=torch.int32, device=DEV)
    Cg, Sn, Sl = Guard(M, 64, F32, 64, I["cos"]), Guard(M, 64, F32, 64, I["sin"]), vec(M, torch.int64, I["slot"])
    sptr = None
    if with_side:
        so = side_struct(Sg, None, stp)
        sptr = ctypes.addressof(so)
    what = qid(q) + f" packed={packed} fill={fill} side={with_side}"
    with decode_cus(q.cus):
        call_guarded("gemm_qkv_rope_kv_bf16", (Xg, Wp, bp, Qg, Cg, Sn, Sl, Kc, Vc, M, q.Hq, Hkv, 128, K, ldx, ldq, sptr),
                     (Qg, Kc, Vc) + ((Sg,) if with_side else ()), what)
    for g_, nm in ((Xg, "X"), (Wp, "packed W"), (bp, "packed bias"), (Cg, "cos"), (Sn, "sin"), (Sl, "slot")):
        g_.untouched(nm)
    # gather what was written, and assert that nothing else was
    slot = I["slot"]
    ok = (slot >= 0).nonzero()[:, 0]
    page, off = (slot[ok] >> 5), (slot[ok] & 31)
    kidx = kpk_index()
    full = torch.zeros(M, N, dtype=BF, device=DEV)
    full[:, : q.Hq * 128] = Qg.view
    valid = torch.zeros(M, N, dtype=torch.bool)
    valid[:, : q.Hq * 128] = True
    kmask, vmask = torch.zeros(P * Hkv, 4096, dtype=torch.bool, device=DEV), torch.zeros(P * Hkv, 4096, dtype=torch.bool, device=DEV)
    for h in range(Hkv):
        rows = d(page * Hkv + h)[:, None]
        kcol, vcol = d(kidx[off]), d(torch.arange(128)[None, :] * 32 + off[:, None])
        c0 = (q.Hq + h) * 128
        full[d(ok), c0: c0 + 128] = Kc.view[rows, kcol]
        full[d(ok), c0 + Hkv * 128: c0 + Hkv * 128 + 128] = Vc.view[rows, vcol]
        valid[ok, c0: c0 + 128] = True
        valid[ok, c0 + Hkv * 128: c0 + Hkv * 128 + 128] = True
        kmask[rows, kcol] = True
        vmask[rows, vcol] = True
    for g_, m_, nm in ((Kc, kmask, "K"), (Vc, vmask, "V")):
        saved = g_.saved.view(-1, 4096)[2: 2 + P * Hkv]
        assert same_bits(g_.view[~m_], saved[~m_]), f"{what}: a {nm}-cache element outside the named slots was written (slot < 0 rows included)"
    srows = None
    if with_side:
        rows = base + torch.arange(M, device=DEV) * ss + step
        other_rows_intact(Sg, rows, what)
        srows = Sg.view[rows].clone()
    return full, valid, srows


@pytest.mark.gpu
@pytest.mark.parametrize("q", QKV_CASES, ids=qid)
def test_gpu_gemm_qkv_rope_kv(q):
    """the fused q|k|v projection against float64 (q, both caches, side rows); exact tables and one-hot rows bit for bit; sentinels around every slot; with and
    without side, X row-major and packed, two fills of X's padding"""
    B = qkv_base(q.Hq, q.Hkv, q.K)
    Wp, bp = pack_weight_gpu(B["W"], "qkv", qid(q), q.Hq, q.Hkv, B["bias"])
    # the bf16 projection through the plain narrow kernel on the naturally packed weights: what the exact-table rows must reproduce
    Wn = pack_weight_gpu(B["W"], "plain", qid(q))
    N, K, M = B["N"], q.K, q.M
    Xg, Yg = Guard(M, K, BF, K + 8, B["X"][:M]), Guard(M, N, BF, N + 8)
    with decode_cus(1024):
        call_guarded("gemm_skinny_bf16", (Xg, Wn, Yg, vec(N, BF, B["bias"]), M, N, K, K + 8, K, N + 8, 0, 1, None), (Yg,), qid(q) + " projection")
    proj_bf = Yg.view.cpu()
    first = None
    for packed in (False, True):
        I = qkv_inputs(q, packed)
        R = qkv_refs(q, I, DEV)
        Hr = R["Hr"]
        rot, vcols = slice(0, Hr * 128), slice(Hr * 128, N)
        want_rows = exact_rows_expected(q, I, proj_bf)
        runs = []
        for fill, with_side in ((None, True), (3.0, False)):
            full, valid, srows = launch_qkv(q, I, Wp, bp, packed, fill, with_side)
            what = qid(q) + f" packed={packed} side={with_side}"
            vd = d(valid)
            ratio_ok = torch.where(vd, ratio(full, R["ref"], R["bound"]), torch.zeros_like(R["ref"]))
            check("gpu", "qkv.rot", torch.where(vd, full.double(), R["ref"])[:, rot], R["ref"][:, rot], R["bound"][:, rot], what)
            check("gpu", "qkv.v", torch.where(vd, full.double(), R["ref"])[:, vcols], R["ref"][:, vcols], R["bound"][:, vcols], what)
            assert float(ratio_ok.max()) <= 1.0
            for r, want in want_rows.items():
                m_ = valid[r]
                assert values_equal(full[r].cpu()[m_], want[m_]), f"{what}: exact-table row {r} is not the bf16 projection / its partner"
            assert same_bits(full[:, vcols].cpu()[valid[:, vcols]], proj_bf[:, vcols][valid[:, vcols]]), f"{what}: V differs from the plain projection"
            for n, k in zip(B["brows"], B["bk"]):          # one-hot W rows, at the rows with the (1, 0) table: bf16(x_k + bias_n)
                for r in (0, 2, 17):
                    if r < M and bool(valid[r, n]):
                        want = (I["X"][r, k].float() + B["bias"][n].float()).to(BF)
                        assert float(full[r, n]) == float(want), f"{what}: column {n} of a one-hot W row at row {r}"
            if with_side:
                check("gpu", "qkv.rot", srows[:, rot], R["ref"][:, rot], R["bound"][:, rot], what + " side rows")
                check("gpu", "qkv.v", srows[:, vcols], R["ref"][:, vcols], R["bound"][:, vcols], what + " side rows")
                assert same_bits(srows.cpu()[valid], full.cpu()[valid]), f"{what}: a side row differs from q / the caches"
                for r, want in want_rows.items():
                    assert values_equal(srows[r].cpu(), want), f"{what}: side row {r} with an exact table"
            runs.append((full.cpu(), valid))
        assert same_bits(runs[0][0][runs[0][1]], runs[1][0][runs[1][1]]), f"{qid(q)} packed={packed}: side == NULL / another fill of X's padding changes the output"
        if first is None:
            first = runs[0][0][:, : q.Hq * 128]
        else:
            assert same_bits(first, runs[0][0][:, : q.Hq * 128]), f"{qid(q)}: q differs between row-major and packed X"
    # one-hot X rows 2 (v 1, table (1, 0)) and 3 (v -2, table (0, 1)): IEEE fixes bf16(v W[:, k] + bias), the table then copies / swaps it
    ks = hot_ks(K, [])
    if M > 3:
        for r, k, v in ((2, ks[0], 1.0), (3, ks[-1], -2.0)):
            p = (v * B["W"][:, k].float() + B["bias"].float()).to(BF)
            want = exact_rows_expected(q, qkv_inputs(q, True), p[None, :].expand(M, -1))[r]
            assert values_equal(first[r], want[: q.Hq * 128]), f"{qid(q)}: q of the one-hot row {r}"


@pytest.mark.gpu
def test_gpu_qkv_row_bits_do_not_depend_on_MG():
    """the first 5 rows of q at M = 5, 20, 70 (MG 1, 2, 4) are the same bits"""
    qs = []
    B = qkv_base(2, 1, 256)
    Wp, bp = pack_weight_gpu(B["W"], "qkv", "qkv MG", 2, 1, B["bias"])
    for q in (x for x in QKV_CASES if (x.Hq, x.K, x.cus) == (2, 256, 1024)):
        full, valid, _ = launch_qkv(q, qkv_inputs(q, False), Wp, bp, False, None, False)
        qs.append(full[:5, :256].cpu())
    assert len(qs) == 3 and same_bits(qs[0], qs[1]) and same_bits(qs[0], qs[2]), "a q row's bits depend on MG"


@pytest.mark.gpu
def test_gpu_skinny_host_side_refusals():
    """Shapes the launchers refuse on the host: an error through the binding, no launch, outputs untouched"""
    M, N, K = 70, 256, 416
    g = gen(5)
    X, W = torch.randn(M, K, generator=g).to(BF), torch.randn(N, K, generator=g).to(BF)
    Xg, Wg, Yg, Y32 = Guard(M, K, BF, K + 8, X), Guard(1, N * K, BF, None, W.reshape(1, -1)), Guard(M, N, BF, N + 8), Guard(2 * M, N, F32, N + 8)
    outs = (Yg, Y32)
    sk = lambda Xa, Wa, Y, M_, N_, K_, ldx, ldy, mode, ks, side=None: ("gemm_skinny_bf16", (Xa, Wa, Y, None, M_, N_, K_, ldx, K_, ldy, mode, ks, side))
    with decode_cus(1024):
        refused(*sk(Xg, Wg, Yg, M, N, 408, K + 8, N + 8, 0, 1), outs, "K % 32")
        refused(*sk(Xg, Wg, Yg, M, 248, K, K + 8, N + 8, 0, 1), outs, "N % 16")
        refused(*sk(Xg, Wg, Yg, M, N, K, K + 8, 0, 0, 1), outs, "ldy == 0 outside mode 3")
        refused(*sk(Xg, Wg, Yg, M, 192, K, K + 8, N + 8, 3, 1), outs, "mode 3 with N % 128")
        refused(*sk(Xg, Wg, Y32, M, N, K, K + 8, N + 8, 1, 2), outs, "ksplit > 1 outside mode 2")
        refused(*sk(Xg.view.data_ptr() + 2, Wg, Yg, M, N, K, K + 8, N + 8, 0, 1), outs, "misaligned X")
        refused(*sk(Xg, Wg.view.data_ptr() + 2, Yg, M, N, K, K + 8, N + 8, 0, 1), outs, "misaligned W")
        p0, p1, stp, _ = make_side(M, N)
        so = side_struct(p0, p1, stp)
        refused(*sk(Xg, Wg, Yg, M, N, K, K + 8, N // 2 + 8, 3, 1, ctypes.addressof(so)), outs + (p0, p1), "side where no persistent form takes the shape")
    with decode_cus(8):
        refused(*sk(Xg, Wg, Y32, M, N, K, K + 8, N + 8, 2, 2, ctypes.addressof(so)), outs + (p0, p1), "side on the split form")
    W8g, sc = Guard(1, N * K, U8T), vec(N, F32)
    f8 = lambda N_, K_, scale: ("gemm_skinny_fp8w", (Xg, W8g, scale, Yg, None, M, N_, K_, K + 8, N + 8, 0, 1))
    with decode_cus(1024):
        refused(*f8(N, 416, sc.view), outs, "FP8 K % 64")
        refused(*f8(240, 384, sc.view), outs, "FP8 N % 64")
        refused(*f8(N, 384, None), outs, "FP8 without scales")
    Wr = Guard(N, K, BF, K + 16, W)
    refused("pack_weight_fp8", (Wr, K + 16, W8g, sc, N, 384, 64), (W8g, sc), "pack_weight_fp8 gateup_I != N / 2")
    Qg, Kc, Vc = Guard(M, 256, BF, 264), Guard(8, 4096, BF), Guard(8, 4096, BF)
    cs, slot = torch.ones(M, 64, device=DEV), torch.zeros(M, dtype=torch.int64, device=DEV)
    refused("gemm_qkv_rope_kv_bf16", (Xg, Wg, None, Qg, cs, cs, slot, Kc, Vc, M, 2, 1, 64, 384, K + 8, 264, None), (Qg, Kc, Vc), "D != 128")


@pytest.mark.gpu
def test_gpu_used_fractions_record():
    """prints the largest used fraction of every bound over the GPU tests above (run after them: it reads what they recorded)"""
    _print_used("gpu")
    assert all(v <= 1.0 for v in USED["gpu"].values())
