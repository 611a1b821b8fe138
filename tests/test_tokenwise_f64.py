"""The token-wise kernels (csrc/norm.hip, elementwise.hip, loss.hip, optim.hip and the decode bookkeeping) against float64, on every dispatch path of their launchers.

THE BOUND.  Every output element is held to   |got - ref64| <= 2^-8 c |ref64| + 2^-24 (f0 + fn n) E + 1e-30   (BOUNDS below; no element is exempt), where ref64 is the
operation in float64 on the same bf16- / fp32-rounded inputs with NO intermediate rounding, c counts the bf16 round-to-nearest points between the inputs and that output
(2^-8 relative each) plus one spare as in test_attn_f64.py (an fp32 output has c = 0), E is the same formula with the absolute value of every term (what catches
cancellation), n is the length of the fp32 sum behind the output (n 2^-24 E, the textbook bound of any summation order) and f0 covers the straight-line fp32 arithmetic
and the special functions: F_LIBM = 16 for erff / tanhf / rsqrtf / logf (the OpenCL full-profile limit; ocml is tighter) and F_EXP = 256 for a product feeding __expf
(exp2(x log2 e): the rounding of the argument is |x| 2^-24 relative in the result, twice when the argument is itself a rounded product, |x| <= 104 before the result leaves
the fp32 range).  1e-30 only guards results below the normal range.  Derivations, one line per output:
  rms.rstd   c 0, f 16 + H: sum of H squares (no cancellation: E = rstd), division, + eps, rsqrtf.
  rms.y      c 3: n = bf16(v rstd), y = bf16(w n), spare; f 16 + H from rstd; E = |y|.
  rms.dx     c 2: one rounding at the store, spare; f 16 + H: the dot product over H; E = rstd (|dn| + |n| mean|dn n|) + |dres|.
  rms.dw / ln.dw   c 0, f 8 + T: fp32 sum over the T rows of products of two rounded factors; E = |dw0| + sum_t |dy n|.       ln.db: f 4 + T, E = |db0| + sum_t |dy|.
  ln.mean    c 0, f 4 + H, E = mean|v|.       ln.rstd  c 0, f 16 + 2 H: two sums; the variance is TWO-PASS, a shift d of the mean moves it by d^2 only:
             E = rstd (1 + H 2^-24 (mean|v| rstd)^2).
  ln.y       c 2 (store, spare), f 16 + 2 H, E = (|v| + |mean|) rstd |w| + |b|.      ln.dx  c 2, f 16 + 2 H, E = rstd (|dn| + mean|dn| + |n| mean|dn n|) + |dres|.
  rope       c 2 (store, spare), f 4, E = |a cos| + |b sin|.
  gelu.fwd   c 2, f F_LIBM + 4, E = 0.5 |x| (1 + |erf|).       gelu.bwd  c 2, f F_LIBM + F_EXP, E = |da| (0.5 (1 + |erf|) + |x| pdf).
  gelu_tanh  fwd c 2, f F_LIBM + 8, E = 0.5 |x| (1 + |tanh|);   bwd c 2, f 2 F_LIBM + 16, E = |da| (0.5 (1 + |th|) + 0.5 |x| (1 + th^2) k (1 + 3 a x^2)).
  quick_gelu fwd c 2, f F_EXP, E = |ref|;   bwd c 2, f F_EXP, E = |da| (s + 1.702 |x| s (1 + s)).
  swiglu.a   c 3: bf16(silu(gate)), the store, spare; f F_EXP; E = |ref|.      swiglu.dgate c 2, f F_EXP, E = |da up| s (1 + |g| (1 + s));    swiglu.dup c 2, f F_EXP, E = |ref|.
  colsum / scatter   c 0, f 4 + n, E = |out0| + sum |terms|.        gather  c 2 (store, spare), f 4 + 2 n (product and sum), E = sum |w src|.
  bias_cast  c 2 (store, spare), f 2, E = |in| + |bias|.
  lp.lse     c 0, f 8 (|m| + |log s| + |lse| + 1) + V: lse = m + log s; the V-term sum moves log s by V 2^-24 ABSOLUTE (s >= 1); the exponents are DIFFERENCES v - m, and a term's
             argument error |v - m| 2^-24 is weighted by exp(v - m), so s is off by O(1) 2^-24 relative (= absolute in log s), not by |x| 2^-24; what scales with the operands is
             the rounding of m + log s and of the stored lse.   lp.logp  the same + 8 |x_target|.       dlogits  c 2, f F_EXP, E = |g| (onehot + p).
  grpo.kl    c 0, f 16, E = e^d + |d| + 1 (|d| <= 5).     grpo.dlogp  c 0, f 32, E = m / cnt / rows (|A| + beta (1 + e^d)).     grpo.row  c 0, f 32 + C, E = sum m (|A| + beta E_kl) / cnt.
  sumsq      c 0, f 8 + chain (32 .. 48 here): `chain` is the longest run of additions one term passes through in the fixed two-stage tree (4 per thread trip + 16 in a block sum, twice) --
             n 2^-24 with n = 2 * 10^6 would be vacuous; E = sum g^2.
  adam.m / adam.v   c 0, f 8: two products and a sum; E = |b m| + |(1 - b) g'| (g'^2 for v).     adam.master  c 0, f 64: decay, sqrtf, rsqrtf, division, the host's powf in
             the bias corrections; E = |w| + |lr_t m' / (sqrt(v') isq + eps)|.
  rope_table: |got - cos64(fl32(pos) * inv_freq)| <= (largest error of the host's fp32 cosf / sinf on the same arguments) + 2 ulp(1) for another libm.
Asserted as EQUALITIES, bit for bit: res_out == bf16(x + res); the slab sums of the x32 path (the slabs are dyadic, k 2^-8, so that every fp32 order of adding them is
exact and bf16(sum) is one value: a dropped, doubled or misplaced slab moves it by O(1)); param_bf16 == bf16(master); casts; embed; padding zeros; re-zeroed inputs;
run-to-run equality of every ordered reduction; a row of rmsnorm_fwd at T = 1 against the same row inside a T = 229 launch; decode_advance's table against rope_table.

A bound that was found mistaken: lp.lse / lp.logp were first held to 2^-24 (F_EXP (max|x| + 1) + V).  F_EXP is the allowance for a PRODUCT feeding __expf and already contains
|arg| <= 104; multiplying it by max|x| counted the operand size twice, and logprob_rows feeds __expf a difference whose error is weighted by the term itself.  That bound was 128 - 330
ulp of lse on ordinary rows (the kernel used 0.003 of it); the one above is about 12 ulp + V 2^-24.

CALLS.  The GPU part calls the C ABI through hip.call: the ops wrappers allocate contiguous outputs and cannot take the strided, sentinelled views every case here needs.  Each family
also runs its wrapper once and compares bits with the direct call; the refusals go through the binding (the wrappers only forward its error).

ONE FAULT MODEL IS CAUGHT BY AN EQUALITY, NOT BY THE BOUND: SwiGLU without the bf16 rounding of silu(gate) moves a product by at most one bf16 ulp against c = 3.  On the gate grid
the products whose two roundings are far from a tie (unchanged when silu moves by +-2^-17 relative, more than fp32 can lose for |gate| <= 16) have ONE correct bit pattern,
bf16(bf16(silu) up); the GPU output is asserted bit-equal to it there, and the fault changes bits at hundreds of those products.  Every other fault model of FAULT_MODELS exceeds
its bound >= 4 x at its designated elements.  Two of them are designated at part of the shapes only: the one-pass LayerNorm variance at H 264 and 520 (from
H = 1024 on the 2 H 2^-24 summation term of ln.rstd, the worst case of ANY order of adding H terms, is as large as what fp32 E[x^2] - mean^2 loses on bf16 data at offset 100),
and coupled weight decay at step 1 (later the two forms can cancel element by element).

INPUTS.  N(0,1) background; per family the rows its kernels can get wrong (NORM rows: 0 = one element 2^13 in the LAST 8-element chunk, 1 = all zero, 2 = scaled 2^-20,
3 = 100 + N(0, 1/16) without residual, 4 = dy aligned with the normalised row so that the backward's projection term is O(1) at every H; gains 0.5 + 2 N, biases 3 N, dres 3 N, dw0 5 N).  The unary activations run every bf16 value with 2^-10 <= |x| <= 16, 0 and +-{64, 1000, 30000}, each with
da in {1, -3, 2^-7}; SwiGLU takes that grid as the gate against up in {1, -3, 2^-7, 1000}.  sumsq runs N(0,1) at every n (every element
carries weight: the 1200 elements of the second loop trip are 5.7e-4 of the sum against a bound of 3e-6) and, as the extra case, a few 1e4 entries among 1e-4 ones.

WHICH CASE REACHES WHICH BRANCH
  rmsnorm_fwd / layernorm_fwd / *_bwd  DISPATCH_NC: H 8, 264 -> NC 1; 520, 1024 -> 2; 1280 -> 3; 2056, 3072 -> 6; 3080, 4096 -> 8 (test_gpu_norm_fwd_bwd[T-H]).
  norm backward  T 229: 58 blocks, threads g = 0, 1 of partial_reduce_acc_kernel take the 8-loads branch (q + 56 < 58); T 2051: the 512-block cap, blocks revisit rows, last wave idle.
  rmsnorm_fwd x32  test_gpu_rmsnorm_x32[...]: nsplit 8 (fast path), 4 and 9, 13 (groups of 4), 2, 3, 7 (pair, pair + 1, 4 + pair + 1), 1 (single); T 257, 300 -> the wave-per-row kernel.
  grid_for cap (2048 blocks)  rope T 1100 x 30 heads x D 128; unary n = 8 (524288 + 300); swiglu T 260 x I 16136; embed T 2049 x H 2048; casts of 8 (524288 + 300) + 3 elements.
  colsum  T 3650 -> 58 groups (8-loads branch), T 4200 -> the 64-group cap with striding.     dlogits_rows  V 131368 -> gx capped at 64, stride loop.
  sumsq n 2097152 + 1203 -> 2048-block cap;   adamw n 4194304 + 1027 -> 4096-block cap and the scalar tail;   grpo_loss C 300 -> second trip of the c += 256 loops.
  cast_f32_to_bf16  contiguous total % 8 in {0, 3} (vector + tail), R = 1 with ld != C, strided, Cpad > C, misaligned by 4 bytes (scalar kernel).

The CPU part proves the GPU part's sensitivity: a torch emulation of each kernel's arithmetic (fp32 where the kernel is fp32, bf16 at its rounding points, partial sums in
block / group order) stays inside the bounds on every input set the GPU tests use, and every fault model, applied to the float64 reference on the same inputs, is outside."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iadr1_amd  # noqa: E402,F401
from iadr1_amd import hip, ops  # noqa: E402

DEV = "cuda"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U8, U24, TINY = 2.0 ** -8, 2.0 ** -24, 1e-30
FAULT_FACTOR = 4.0
F_LIBM, F_EXP = 16, 256
EPS = 1e-6
INF = float("inf")

BOUNDS = {      # output: (c, f0, fn)    bound = 2^-8 c |ref| + 2^-24 (f0 E + fn n En) + 1e-30, En = E unless stated; derivations in the docstring
    "rms.rstd": (0, 16, 1), "rms.y": (3, 16, 1), "rms.dx": (2, 16, 1), "rms.dw": (0, 8, 1),
    "ln.mean": (0, 4, 1), "ln.rstd": (0, 16, 2), "ln.y": (2, 16, 2), "ln.dx": (2, 16, 2), "ln.dw": (0, 8, 1), "ln.db": (0, 4, 1),
    "rope": (2, 4, 0),
    "gelu.fwd": (2, F_LIBM + 4, 0), "gelu.bwd": (2, F_LIBM + F_EXP, 0), "gelu_tanh.fwd": (2, F_LIBM + 8, 0), "gelu_tanh.bwd": (2, 2 * F_LIBM + 16, 0),
    "quick_gelu.fwd": (2, F_EXP, 0), "quick_gelu.bwd": (2, F_EXP, 0),
    "swiglu.a": (3, F_EXP, 0), "swiglu.dgate": (2, F_EXP, 0), "swiglu.dup": (2, F_EXP, 0),
    "colsum": (0, 4, 1), "scatter": (0, 4, 1), "gather": (2, 4, 2), "bias_cast": (2, 2, 0),
    "lp.lse": (0, 8, 1), "lp.logp": (0, 8, 1), "dlogits": (2, F_EXP, 0),
    "grpo.kl": (0, 16, 0), "grpo.dlogp": (0, 32, 0), "grpo.row": (0, 32, 1),
    "sumsq": (0, 8, 1), "adam.m": (0, 8, 0), "adam.v": (0, 8, 0), "adam.master": (0, 64, 0),
}
FAMILY = {"rms": "norm", "ln": "norm", "rope": "rotary", "gelu": "activations", "gelu_tanh": "activations", "quick_gelu": "activations", "swiglu": "activations",
          "colsum": "reductions and maps", "scatter": "reductions and maps", "gather": "reductions and maps", "bias_cast": "casts", "lp": "loss", "dlogits": "loss",
          "grpo": "loss", "sumsq": "optimizer", "adam": "optimizer"}
FAULT_MODELS = ["sumsq_past_cap", "sumsq_tail", "stat_last_chunk", "stat_div_512nc", "drop_slab", "no_xbias", "round_after_res", "no_projection", "no_dres", "dw_rows_ge_2048", "dw_overwrite",
                "ln_onepass_var", "db_last_row", "gelu_swap", "quick_as_silu", "swiglu_no_inner_round", "dgate_no_term", "rope_bwd_sign", "rope_partner_64",
                "rope_row_t_minus_1", "partials_ge_56", "last_row_group", "weights_ignored", "entry_skipped", "lp_tail_v4", "lp_max_first_1024", "ignored_not_zeroed",
                "cnt0_div", "second_trip", "l2_decay", "bias_step_minus_1", "clip_when_coef_ge_1", "adam_tail_n4", "adam_past_cap"]
USED = {"emu": {}, "gpu": {}}       # side -> output -> largest used fraction of the bound
FAULT_SEEN = {}                     # fault model -> smallest excess (x bound) at its designated elements
ROPE_TABLE_ERR = {}


# ======================================================================================================================================================
# helpers
# ======================================================================================================================================================

def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def bfr(x):
    """round to bf16 (nearest even), back in the dtype of x"""
    return x.to(BF).to(x.dtype)


def bits(t):
    return t.contiguous().view({1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a).cpu(), bits(b).cpu())


def frac(key, got, ref, E, n=0, En=None):
    """|got - ref| in units of the bound of BOUNDS[key]; where the reference is not finite the value must be equal (else inf); NaN counts as inf"""
    c, f0, fn = BOUNDS[key]
    got, ref, E = got.detach().double().cpu(), ref.detach().double().cpu(), E.detach().double().cpu()
    ref, E = ref.expand_as(got), E.expand_as(got)
    En = E if En is None else En.detach().double().cpu().expand_as(got)          # scale of the summation term where it differs from E
    fin = torch.isfinite(ref)
    bound = U8 * c * ref.abs() + U24 * (f0 * E + fn * n * En) + TINY
    r = (got - torch.where(fin, ref, torch.zeros_like(ref))).abs() / torch.where(fin, bound, torch.ones_like(bound))
    r = torch.where(fin, r, torch.where(got == ref, torch.zeros_like(r), torch.full_like(r, INF)))
    return torch.where(torch.isnan(r), torch.full_like(r, INF), r)


def check(side, key, got, ref, E, n=0, what="", En=None):
    """Asserts the bound on every element; records the largest used fraction under USED[side][key]."""
    r = frac(key, got, ref, E, n, En)
    mx = float(r.max()) if r.numel() else 0.0
    USED[side][key] = max(USED[side].get(key, 0.0), mx)
    if mx > 1.0:
        flat = r.reshape(-1)
        worst = flat.argsort(descending=True)[:6].tolist()
        g, f = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().expand_as(r).reshape(-1)
        lines = [f"element {np.unravel_index(i, tuple(r.shape))}: got {float(g[i]):.9g} ref {float(f[i]):.9g} = {float(flat[i]):.3g} x bound" for i in worst]
        raise AssertionError(f"{what or key} [{key}]: {int((flat > 1).sum())} of {flat.numel()} elements beyond the bound\n  " + "\n  ".join(lines))
    return mx


def fault_excess(fault, key, bad, ref, E, n=0, rows=None, per_element=False, En=None):
    """Smallest excess (x bound) of the faulty reference over its designated rows (the largest element of each row) or, per_element, over every designated element."""
    r = frac(key, bad, ref, E, n, En)
    if rows is not None:
        r = r[rows]
    assert r.numel() > 0, fault
    ex = float(r.min()) if per_element else float(r.reshape(r.shape[0], -1).amax(-1).min())
    assert ex >= FAULT_FACTOR, f"fault '{fault}' moves {key} by only {ex:.3g} x the bound at its designated elements"
    FAULT_SEEN[fault] = min(FAULT_SEEN.get(fault, INF), ex)
    return ex


def fault_mismatch(fault, bad, ref):
    """For outputs held to equality: the fault must change bits."""
    n = int((bits(bad) != bits(ref)).sum())
    assert n > 0, f"fault '{fault}' changes no bit of an output asserted as an equality"
    FAULT_SEEN[fault] = min(FAULT_SEEN.get(fault, INF), INF)
    return n


def ordered_reduce8(P):
    """partial_reduce_acc_kernel / colsum_reduce_kernel: thread g adds partials g, g + 8, ... in order, the eight group sums are then added in group order (fp32)"""
    npart = P.shape[0]
    pad = (-npart) % 8
    if pad:
        P = torch.cat([P, torch.zeros(pad, *P.shape[1:], dtype=P.dtype)])
    P = P.view(-1, 8, *P.shape[1:])
    s = torch.zeros_like(P[0])
    for q in range(P.shape[0]):
        s = s + P[q]
    t = torch.zeros_like(s[0])
    for u in range(8):
        t = t + s[u]
    return t


def nc_of(H):
    nc = (H // 8 + 63) // 64
    return next(c for c in (1, 2, 3, 4, 6, 8) if nc <= c)


# ======================================================================================================================================================
# norms
# ======================================================================================================================================================

NORM_H = (8, 264, 520, 1024, 1280, 2056, 3072, 3080, 4096)
NORM_T = (1, 5, 229)
NORM_CASES = [(T, H) for T in NORM_T for H in NORM_H] + [(2051, 264), (2051, 2056)]
ROW_BIG, ROW_ZERO, ROW_TINY, ROW_OFFSET, ROW_PROJ = 0, 1, 2, 3, 4


@functools.lru_cache(maxsize=None)
def norm_inputs(T, H):
    g = gen(1000 * T + H)
    r = lambda *s: torch.randn(*s, generator=g)
    x, res = r(T, H), 2 * r(T, H)
    x[ROW_BIG, H - 3] = 8192.0
    if T >= 5:
        x[ROW_ZERO] = 0
        x[ROW_TINY] *= 2.0 ** -20
        res[ROW_ZERO], res[ROW_TINY] = 0, 0
        x[ROW_OFFSET] = 100.0 + 0.25 * x[ROW_OFFSET]        # a narrow row far from 0 (bf16 keeps steps of 0.5 there): E[x^2] - mean^2 in fp32 loses the variance
        res[ROW_OFFSET] = 0
    w, dy = (0.5 + 2 * r(H)).to(BF), r(T, H)
    if T >= 5:          # dy aligned with the normalised row: the projection term of the backward is O(1) there at every H (between independent rows it is O(1 / sqrt(H)))
        dy[ROW_PROJ] = (x[ROW_PROJ].to(BF).float() + res[ROW_PROJ].to(BF).float()) * torch.sign(w.float())
    return {"T": T, "H": H, "x": x.to(BF), "res": res.to(BF), "w": w, "b": (3 * r(H)).to(BF), "dy": dy.to(BF), "dres": (3 * r(T, H)).to(BF),
            "dw0": 5 * r(H), "db0": 5 * r(H)}


def rms_fwd_math(v_in, res, w, emu, fault=None):
    wd = F32 if emu else F64
    v, out = v_in.to(wd), {}
    if res is not None:
        out["res_out"] = (v + res.to(wd)).to(BF)         # the residual stream is a bf16 tensor: an output of its own, asserted bit for bit
        v = out["res_out"].to(wd)
    H = v.shape[1]
    vs = v[:, : H - 8] if fault == "stat_last_chunk" else v
    div = 512 * nc_of(H) if fault == "stat_div_512nc" else H
    rstd = ((vs * vs).sum(-1) / div + torch.tensor(EPS, dtype=F32).to(wd)).rsqrt()
    n = v * rstd[:, None]
    y = w.to(wd) * (bfr(n) if emu else n)
    out.update(rstd=rstd, y=bfr(y) if emu else y, v=v)
    return out


def slab_sum(slabs, xbias, emu, fault=None):
    wd = F32 if emu else F64
    s = torch.zeros_like(slabs[0], dtype=wd)
    for k in range(slabs.shape[0]):
        if not (fault == "drop_slab" and k == slabs.shape[0] // 2):
            s = s + slabs[k].to(wd)
    if xbias is not None and fault != "no_xbias":
        s = s + xbias.to(wd)
    return s


def reduce_rows(contrib, acc0, emu, fault=None, kind="norm"):
    """acc0 + sum over rows.  The emulation follows the kernels: norm backward = grid-stride rows per wave, 4 waves per block, <= 512 blocks; colsum = 8 row lanes per group,
    <= 64 groups; both end in ordered_reduce8."""
    T = contrib.shape[0]
    per, cap = (4, 512) if kind == "norm" else (8, 64)
    nblk = min((T + 3) // 4, cap) if kind == "norm" else min((T + 63) // 64, cap)
    if not emu:
        c = contrib
        rows = torch.arange(T)
        if fault == "dw_rows_ge_2048":
            c = c[:2048]
        elif fault in ("db_last_row", "entry_skipped"):
            c = c[:-1]
        elif fault == "partials_ge_56":
            c = c[(rows // per) % nblk < 56]
        elif fault == "last_row_group":
            c = c[(rows // per) % nblk < nblk - 1]
        s = c.sum(0)
        return s if fault == "dw_overwrite" else acc0.to(F64) + s
    K = -(-T // (nblk * per))
    c = torch.cat([contrib, torch.zeros(K * nblk * per - T, *contrib.shape[1:], dtype=contrib.dtype)]).view(K, nblk, per, *contrib.shape[1:])
    acc = torch.zeros_like(c[0])
    for k in range(K):
        acc = acc + c[k]
    part = torch.zeros_like(acc[:, 0])
    for u in range(per):
        part = part + acc[:, u]
    return acc0.to(F32) + ordered_reduce8(part)


def rms_bwd_math(dy, x, w, rstd32, dres, dw0, emu, fault=None):
    wd = F32 if emu else F64
    H = x.shape[1]
    r = rstd32.to(wd)[:, None]
    n, dn = x.to(wd) * r, dy.to(wd) * w.to(wd)
    dot = (dn * n).sum(-1, keepdim=True) / H
    o = r * (dn if fault == "no_projection" else dn - n * dot)
    if dres is not None and fault != "no_dres":
        o = o + dres.to(wd)
    contrib = dy.to(wd) * n
    out = {"dx": bfr(o) if emu else o, "dw": reduce_rows(contrib, dw0, emu, fault)}
    if not emu:
        out["E_dx"] = r * (dn.abs() + n.abs() * (dn * n).abs().sum(-1, keepdim=True) / H) + (dres.to(wd).abs() if dres is not None else 0)
        out["E_dw"] = dw0.abs().to(F64) + contrib.abs().sum(0)
    return out


def ln_fwd_math(v_in, res, w, b, emu, fault=None):
    wd = F32 if emu else F64
    v, out = v_in.to(wd), {}
    if res is not None:
        out["res_out"] = (v + res.to(wd)).to(BF)
        v = out["res_out"].to(wd)
    H = v.shape[1]
    mean = v.sum(-1, keepdim=True) / H
    d = v - mean
    var = (d * d).sum(-1, keepdim=True) / H
    if fault == "ln_onepass_var":          # fp32 E[x^2] - mean^2, the squares added one after the other
        v32 = v.to(F32)
        m32 = v32.sum(-1, keepdim=True) / H
        var = (torch.cumsum(v32 * v32, -1)[:, -1:] / H - m32 * m32).to(wd)
    rstd = (var + torch.tensor(EPS, dtype=F32).to(wd)).rsqrt()
    y = d * rstd * w.to(wd) + b.to(wd)
    out.update(mean=mean[:, 0], rstd=rstd[:, 0], y=bfr(y) if emu else y, v=v)
    if not emu:
        ma = v.abs().mean(-1)
        out["E_mean"] = ma
        out["E_rstd"] = rstd[:, 0] * (1 + H * U24 * (ma * rstd[:, 0]) ** 2)
        out["E_y"] = (v.abs() + mean.abs()) * rstd * w.to(wd).abs() + b.to(wd).abs()
    return out


def ln_bwd_math(dy, x, w, mean32, rstd32, dres, dw0, db0, emu, fault=None):
    wd = F32 if emu else F64
    H = x.shape[1]
    r = rstd32.to(wd)[:, None]
    n, dn = (x.to(wd) - mean32.to(wd)[:, None]) * r, dy.to(wd) * w.to(wd)
    s1, s2 = dn.sum(-1, keepdim=True) / H, (dn * n).sum(-1, keepdim=True) / H
    o = r * (dn - s1 - n * s2)
    if dres is not None:
        o = o + dres.to(wd)
    cw, cb = dy.to(wd) * n, dy.to(wd)
    out = {"dx": bfr(o) if emu else o, "dw": reduce_rows(cw, dw0, emu, None if fault == "db_last_row" else fault), "db": reduce_rows(cb, db0, emu, fault)}
    if not emu:
        out["E_dx"] = r * (dn.abs() + dn.abs().sum(-1, keepdim=True) / H + n.abs() * (dn * n).abs().sum(-1, keepdim=True) / H) + (dres.to(wd).abs() if dres is not None else 0)
        out["E_dw"], out["E_db"] = dw0.abs().to(F64) + cw.abs().sum(0), db0.abs().to(F64) + cb.abs().sum(0)
    return out


@functools.lru_cache(maxsize=4)
def norm_refs(T, H):
    """float64 references of one norm case (computed once, shared by the CPU and the GPU test)"""
    I = norm_inputs(T, H)
    rf = rms_fwd_math(I["x"], I["res"], I["w"], False)
    lf = ln_fwd_math(I["x"], I["res"], I["w"], I["b"], False)
    xin = rf["res_out"]                                                  # the backward's x is the residual stream the forward wrote
    rb = rms_bwd_math(I["dy"], xin, I["w"], rf["rstd"].to(F32), I["dres"], I["dw0"], False)
    lb = ln_bwd_math(I["dy"], xin, I["w"], lf["mean"].to(F32), lf["rstd"].to(F32), I["dres"], I["dw0"], I["db0"], False)
    return rf, lf, rb, lb


def check_norm(side, T, H, got):
    """got: dict of outputs named as below, from the emulation or the GPU"""
    rf, lf, rb, lb = norm_refs(T, H)
    w = f"T={T} H={H}"
    assert same_bits(got["rms.res_out"].cpu(), rf["res_out"]) and same_bits(got["ln.res_out"].cpu(), lf["res_out"]), f"res_out != bf16(x + res) ({w})"
    check(side, "rms.rstd", got["rms.rstd"], rf["rstd"], rf["rstd"], H, w)
    check(side, "rms.y", got["rms.y"], rf["y"], rf["y"].abs(), H, w)
    check(side, "rms.dx", got["rms.dx"], rb["dx"], rb["E_dx"], H, w)
    check(side, "rms.dw", got["rms.dw"], rb["dw"], rb["E_dw"], T, w)
    check(side, "ln.mean", got["ln.mean"], lf["mean"], lf["E_mean"], H, w)
    check(side, "ln.rstd", got["ln.rstd"], lf["rstd"], lf["E_rstd"], H, w)
    check(side, "ln.y", got["ln.y"], lf["y"], lf["E_y"], H, w)
    check(side, "ln.dx", got["ln.dx"], lb["dx"], lb["E_dx"], H, w)
    check(side, "ln.dw", got["ln.dw"], lb["dw"], lb["E_dw"], T, w)
    check(side, "ln.db", got["ln.db"], lb["db"], lb["E_db"], T, w)


# few-row rmsnorm over fp32 slabs -------------------------------------------------------------------------------------------------------------------------
X32_NSPLIT = (1, 2, 3, 4, 7, 8, 9, 13)
X32_T, X32_H = (1, 3, 64, 256), (32, 2048, 2080, 4096)
# (T, H, nsplit, xbias, res, mode): every nsplit twice, every T and H at least four times, xbias / res in all four combinations; mode "row" = strided row-major y with
# rstd, "packed" = ldy == 0 through PackedAct, "rstd_only" = y NULL, "no_res_out" = res given, res_out NULL; then the wave kernel (T > 256)
X32_CASES = [(X32_T[(i + j) % 4], X32_H[(i + 2 * j + i // 4) % 4], ns, bool((i + j) % 2), bool(j), ("packed" if (i + j) % 3 == 0 else "row"))
             for i, ns in enumerate(X32_NSPLIT) for j in range(2)]
X32_CASES += [(3, 2080, 3, True, True, "no_res_out"), (64, 2048, 8, False, False, "rstd_only"), (257, 2080, 3, True, True, "row"), (300, 2080, 8, False, True, "row"),
              (257, 32, 8, True, False, "row"), (300, 4096, 3, False, False, "row")]


@functools.lru_cache(maxsize=None)
def x32_inputs(T, H, ns, seed=0):
    g = gen(7 + 31 * T + H + 1009 * ns + seed)
    slabs = torch.round(torch.randn(ns, T, H, generator=g) * 256) / 256                # dyadic: every fp32 order of adding the slabs is exact
    slabs[0, ROW_BIG, H - 3] = 8192.0
    if T >= 3:
        slabs[:, ROW_ZERO] = 0
        slabs[:, ROW_TINY] *= 2.0 ** -20
    xbias = (torch.round(torch.randn(H, generator=g) * 1.5 * 64) / 64).clamp(-1.96875, 1.96875).to(BF)
    res = torch.round(2 * torch.randn(T, H, generator=g) * 16) / 16
    if T >= 3:
        res[ROW_ZERO], res[ROW_TINY] = 0, 0
    return {"slabs": slabs.to(F32), "xbias": xbias, "res": res.to(BF), "w": (0.5 + 2 * torch.randn(H, generator=g)).to(BF)}


def x32_math(I, use_bias, use_res, emu, fault=None):
    s = slab_sum(I["slabs"], I["xbias"] if use_bias else None, emu, fault)
    if fault == "round_after_res":
        out = rms_fwd_math(s, None, I["w"], emu)
        out["res_out"] = (s + I["res"].to(s.dtype)).to(BF)
        return out
    out = rms_fwd_math(s.to(BF), I["res"] if use_res else None, I["w"], emu)
    out["branch"] = s.to(BF)
    return out


# ======================================================================================================================================================
# rotary
# ======================================================================================================================================================

ROPE_CASES = [(7, 1, 128, 0), (7, 3, 128, 2), (5, 3, 80, 1), (5, 1, 80, 2), (6, 3, 72, 1), (1100, 30, 128, 0)]        # (T, nheads, D, untouched trailing heads)


@functools.lru_cache(maxsize=None)
def rope_inputs(T, nheads, D, extra):
    g = gen(T + 17 * nheads + D)
    x = torch.randn(T, (nheads + extra) * D, generator=g).to(BF)
    th = (torch.rand(T, D // 2, generator=g, dtype=F64) * 2 * math.pi)
    return {"x": x, "cos": torch.cos(th).to(F32), "sin": torch.sin(th).to(F32)}


def rope_math(x, cos, sin, nheads, D, backward, emu, fault=None):
    wd = F32 if emu else F64
    T, half = x.shape[0], D // 2
    X = x.to(wd)
    h = X[:, : nheads * D].reshape(T, nheads, D)
    a, b = h[..., :half], h[..., half:]
    if fault == "rope_partner_64":         # partner j + 64 whatever D: reads across the head boundary (the trailing heads keep it inside the row)
        idx = (torch.arange(nheads)[:, None] * D + torch.arange(half)[None, :] + 64)
        b = X[:, idx.reshape(-1)].reshape(T, nheads, half)
    if fault == "rope_row_t_minus_1":
        cos, sin = torch.roll(cos, 1, 0), torch.roll(sin, 1, 0)
    c, s = cos.to(wd)[:, None, :], sin.to(wd)[:, None, :]
    sg = -1.0 if (backward and fault != "rope_bwd_sign") else 1.0
    o = torch.cat([a * c - sg * b * s, b * c + sg * a * s], -1)
    E = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], -1)
    return (bfr(o) if emu else o).reshape(T, nheads * D), E.reshape(T, nheads * D)


# ======================================================================================================================================================
# activations
# ======================================================================================================================================================

@functools.lru_cache(maxsize=None)
def bf16_grid():
    """every bf16 value with 2^-10 <= |x| <= 16, then 0 and +-{64, 1000, bf16(30000)}; zero-padded to a multiple of 8"""
    e, m = np.arange(117, 131, dtype=np.uint32), np.arange(128, dtype=np.uint32)
    mag = np.concatenate([((e[:, None] << 7) | m[None, :]).reshape(-1), np.array([131 << 7], dtype=np.uint32)])
    v = ((np.concatenate([mag, mag | 0x8000]).astype(np.uint32)) << np.uint32(16)).astype(np.uint32).view(np.float32)
    v = np.concatenate([v, np.array([0, 64, -64, 1000, -1000, 29952, -29952], dtype=np.float32)])        # 29952 = bf16(30000)
    v = np.concatenate([v, np.zeros((-len(v)) % 8, dtype=np.float32)])
    t = torch.from_numpy(v.copy())
    assert torch.equal(t.to(BF).float(), t)
    return t.to(BF)


DA_VALUES = (1.0, -3.0, 2.0 ** -7)
UP_VALUES = (1.0, -3.0, 2.0 ** -7, 1000.0)
K_TANH, A_TANH = math.sqrt(2.0 / math.pi), 0.044715
UNARY = ("gelu", "gelu_tanh", "quick_gelu")
BIG_N = 8 * (524288 + 300)


@functools.lru_cache(maxsize=None)
def unary_inputs(big=False):
    if big:
        g = gen(5)
        return (3 * torch.randn(BIG_N, generator=g)).to(BF), torch.randn(BIG_N, generator=g).to(BF)
    z = bf16_grid()
    return z.repeat(len(DA_VALUES)), torch.cat([torch.full_like(z, d) for d in DA_VALUES])


def unary_math(name, z, da, emu, fault=None):
    """(fwd, E_fwd, bwd, E_bwd)"""
    wd = F32 if emu else F64
    x, d = z.to(wd), da.to(wd)
    if fault == "gelu_swap":
        name = {"gelu": "gelu_tanh", "gelu_tanh": "gelu"}[name]
    if name == "gelu":
        er = torch.erf(x * (0.70710678 if emu else math.sqrt(0.5)))
        pdf = (0.3989422804 if emu else 1 / math.sqrt(2 * math.pi)) * torch.exp(-0.5 * x * x)
        f, Ef = 0.5 * x * (1 + er), 0.5 * x.abs() * (1 + er.abs())
        b, Eb = d * (0.5 * (1 + er) + x * pdf), d.abs() * (0.5 * (1 + er.abs()) + x.abs() * pdf)
    elif name == "gelu_tanh":
        th = torch.tanh(K_TANH * (x + A_TANH * x * x * x))
        pol = K_TANH * (1 + 3 * A_TANH * x * x)
        f, Ef = 0.5 * x * (1 + th), 0.5 * x.abs() * (1 + th.abs())
        b, Eb = d * (0.5 * (1 + th) + 0.5 * x * (1 - th * th) * pol), d.abs() * (0.5 * (1 + th.abs()) + 0.5 * x.abs() * (1 + th * th) * pol)
    else:
        k = 1.0 if fault == "quick_as_silu" else 1.702
        s = 1 / (1 + torch.exp(-k * x))
        f = x * s
        Ef = f.abs()
        b, Eb = d * (s + k * x * s * (1 - s)), d.abs() * (s + k * x.abs() * s * (1 + s))
    return (bfr(f), Ef, bfr(b), Eb) if emu else (f, Ef, b, Eb)


@functools.lru_cache(maxsize=None)
def swiglu_inputs(big=False):
    """gu [T, 2 I] and da [T, I]: the gate grid against every up value (one row per up value and da value), or T 260 x I 16136 N(0, 1.5)"""
    if big:
        g = gen(9)
        return (1.5 * torch.randn(260, 2 * 16136, generator=g)).to(BF), torch.randn(260, 16136, generator=g).to(BF)
    z = bf16_grid()
    rows = [(u, d) for u in UP_VALUES for d in DA_VALUES]
    gu = torch.stack([torch.cat([z, torch.full_like(z, u)]) for u, _ in rows])
    da = torch.stack([torch.full_like(z, d) for _, d in rows])
    return gu, da


def swiglu_math(gu, da, emu, fault=None):
    wd = F32 if emu else F64
    I = gu.shape[1] // 2
    g, u, d = gu[:, :I].to(wd), gu[:, I:].to(wd), da.to(wd)
    s = 1 / (1 + torch.exp(-g))
    silu = g * s if not emu else g / (1 + torch.exp(-g))
    if fault == "swiglu_no_inner_round":
        a = silu * u
    else:
        a = (bfr(silu) if emu else silu) * u
    dgate = d * u * (s * (1 + (0 if fault == "dgate_no_term" else g * (1 - s))))
    dup = d * (g * s)
    out = {"a": bfr(a) if emu else a, "dgate": bfr(dgate) if emu else dgate, "dup": bfr(dup) if emu else dup}
    if not emu:
        out.update(E_a=a.abs(), E_dgate=(d * u).abs() * s * (1 + g.abs() * (1 + s)), E_dup=dup.abs())
    return out


def swiglu_exact(gu):
    """(expected bits of a as bf16, mask): products of the grid whose result is ONE bf16 value whatever fp32 does to silu -- bf16(bf16(silu (1 + d)) up) is the same for
    d in {0, +-2^-17} -- for |gate| <= 16"""
    I = gu.shape[1] // 2
    g, u = gu[:, :I].double(), gu[:, I:].double()
    silu = g / (1 + torch.exp(-g))
    outs = [(bfr(silu * (1 + dd)) * u).to(BF) for dd in (0.0, 2.0 ** -17, -2.0 ** -17)]
    ok = (bits(outs[0]) == bits(outs[1])) & (bits(outs[0]) == bits(outs[2])) & (g.abs() <= 16)
    return outs[0], ok


# ======================================================================================================================================================
# column sums, row maps
# ======================================================================================================================================================

COLSUM_CASES = [(T, N) for T in (1, 70, 3650, 4200) for N in (8, 264, 520)]


@functools.lru_cache(maxsize=None)
def colsum_inputs(T, N):
    g = gen(3 * T + N)
    return (torch.randn(T, N, generator=g) + 0.25).to(BF), 5 * torch.randn(N, generator=g)


MAP_H = (8, 2048, 2056)


@functools.lru_cache(maxsize=None)
def gather_inputs(H):
    """rows_gather_sum: 12 source rows, 7 output rows with lists: empty, 1, 9 (two repeated source rows), empty, 2, 1, 3"""
    g = gen(H)
    src = torch.randn(12, H, generator=g).to(BF)
    lists = [[], [4], [0, 3, 3, 7, 11, 2, 0, 9, 5], [], [11, 1], [6], [8, 8, 10]]
    ptr = np.cumsum([0] + [len(l) for l in lists]).astype(np.int32)
    idx = np.array([i for l in lists for i in l], dtype=np.int32)
    wts = (torch.randn(len(idx), generator=g) * 2 - 0.5).to(F32)
    return src, lists, torch.from_numpy(ptr), torch.from_numpy(idx), wts


def gather_math(src, lists, wts, emu, fault=None):
    wd = F32 if emu else F64
    out, E, k = [], [], 0
    for l in lists:
        v, e = torch.zeros(src.shape[1], dtype=wd), torch.zeros(src.shape[1], dtype=wd)
        for j, i in enumerate(l):
            wk = wts[k].to(wd) if (wts is not None and fault != "weights_ignored") else 1.0
            k += 1
            if fault == "entry_skipped" and len(l) >= 3 and j == len(l) - 2:
                continue
            v, e = v + wk * src[i].to(wd), e + (wk * src[i].to(wd)).abs()
        out.append(bfr(v) if emu else v)
        E.append(e)
    return torch.stack(out), torch.stack(E)


@functools.lru_cache(maxsize=None)
def scatter_inputs(H):
    """rows_scatter_acc: 40 source rows onto 6 destination rows of a [9, H] fp32 table: row 7 fed by 17 source rows, row 2 by one, the rest by a few; 3 source rows dropped"""
    g = gen(H + 1)
    src = torch.randn(40, H, generator=g).to(BF)
    dst_rows = np.full(40, -1, dtype=np.int64)
    order = torch.randperm(40, generator=g).numpy()
    for n, r in zip((17, 1, 6, 5, 4, 4), (7, 2, 0, 8, 5, 3)):
        dst_rows[order[:n]] = r
        order = order[n:]
    return src, dst_rows, 5 * torch.randn(9, H, generator=g)


def scatter_math(src, dst_rows, dst0, emu, fault=None):
    wd = F32 if emu else F64
    out, E = dst0.to(wd).clone(), dst0.to(wd).abs()
    for r in np.unique(dst_rows[dst_rows >= 0]):
        ks = np.flatnonzero(dst_rows == r)
        if fault == "entry_skipped" and len(ks) >= 3:
            ks = np.delete(ks, len(ks) // 2)
        v = torch.zeros(src.shape[1], dtype=wd)
        for k in ks:
            v = v + src[k].to(wd)
        out[r] = out[r] + v
        E[r] = E[r] + src[ks].to(wd).abs().sum(0)
    return out, E


# ======================================================================================================================================================
# loss rows
# ======================================================================================================================================================

LP_CASES = [(R, V, ld) for R in (1, 37) for V, ld in ((3, 4), (640, 640), (1289, 1292), (5003, 5004))] + [(37, 1288, 1288)]
LP_OFFSET, LP_PEAK, LP_HEAD_INF, LP_TAIL_INF, LP_IGN, LP_GE_V = 1, 2, 3, 4, 5, 6          # special rows when R = 37


@functools.lru_cache(maxsize=None)
def lp_inputs(R, V, ld):
    g = gen(R + 7 * V)
    x = 3 * torch.randn(R, V, generator=g)
    tgt = torch.randint(0, V, (R,), generator=g)
    tgt[0] = V - 1
    if R > 8:
        x[LP_OFFSET] += 3e4
        x[LP_PEAK] *= 10
        x[LP_PEAK, V - 1] = 400.0                      # the row maximum in the last id (the scalar tail when V % 4 != 0, past id 1024 when V > 1024)
        x[LP_HEAD_INF, : min(4, V - 1)] = -INF
        x[LP_TAIL_INF, max(1, V - 8):] = -INF
        tgt[LP_PEAK], tgt[LP_HEAD_INF], tgt[LP_TAIL_INF], tgt[LP_IGN], tgt[LP_GE_V], tgt[7] = V - 1, 1, 0, -100, V + 5, 0          # row LP_HEAD_INF: the target is a masked id
    buf = torch.full((R, ld), 777.0)
    buf[:, :V] = x.to(F32)
    return buf, tgt.to(torch.int64)


def lp_math(buf, V, tgt, emu, fault=None):
    wd = F32 if emu else F64
    x = buf[:, :V].to(wd)
    R = x.shape[0]
    xs = x[:, : V - V % 4] if (fault == "lp_tail_v4" and V >= 4) else x
    if fault == "lp_max_first_1024":          # fp32, like the kernel it models: exp(x - m) overflows where the true maximum lies past id 1024
        m = x[:, :1024].to(F32).amax(-1, keepdim=True)
        lse = (m + torch.log(torch.exp(x.to(F32) - m).sum(-1, keepdim=True)))[:, 0].to(wd)
    elif emu:
        m = xs.amax(-1, keepdim=True)
        lse = (m + torch.log(torch.exp(xs - m).sum(-1, keepdim=True)))[:, 0]
    else:
        lse = torch.logsumexp(xs, -1)
    ok = (tgt >= 0) & (tgt < V)
    xt = x[torch.arange(R), tgt.clamp(0, V - 1)]
    logp = torch.where(ok | (fault == "ignored_not_zeroed"), xt - lse, torch.zeros_like(lse))
    m = x.amax(-1)
    E = m.abs() + (lse - m).abs() + lse.abs() + 1           # |m| + |log s| + |lse| + 1
    return lse, logp, E, E + torch.where(ok & torch.isfinite(xt), xt.abs(), torch.zeros_like(xt))


def dlogits_math(buf, V, tgt, lse32, gvec, emu):
    wd = F32 if emu else F64
    x = buf[:, :V].to(wd)
    R = x.shape[0]
    p = torch.exp(x - lse32.to(wd)[:, None])
    oh = torch.zeros_like(p)
    ok = (tgt >= 0) & (tgt < V)
    oh[torch.arange(R)[ok], tgt[ok]] = 1
    gr = gvec.to(wd)[:, None]
    o = -gr * p + gr * oh
    return (bfr(o) if emu else o), gr.abs() * (oh + p)


DLOGITS_EXTRA = ((5, 8), (3, 131368))         # one chunk; gx capped at 64: the stride loop


@functools.lru_cache(maxsize=None)
def dlogits_extra_inputs(R, V):
    g = gen(V)
    x = (3 * torch.randn(R, V, generator=g)).to(F32)
    tgt = torch.tensor([V - 1, 0, -100, 3, V // 2][:R])
    gvec = torch.tensor([1.5, -2.0, 0.0, 0.7, 3.0][:R])
    lse32 = torch.logsumexp(x.double(), -1).to(F32)
    return x, tgt, gvec, lse32


BIAS_CAST_CASES = ((5, 24, True), (5, 24, False), (3, 7, True), (64, BIG_N // 64 + 5, True))       # the last: R C past the grid cap


@functools.lru_cache(maxsize=None)
def bias_cast_inputs(R, C):
    g = gen(R * 31 + C)
    return torch.randn(R, C, generator=g) * 3, (torch.randn(C, generator=g) * 2).to(BF)


GRPO_CASES = [(N, C) for N in (1, 8) for C in (1, 12, 300)]


@functools.lru_cache(maxsize=None)
def grpo_inputs(N, C):
    g = gen(N * 1000 + C)
    logp = -2 * torch.rand(N, C, generator=g)
    d = 10 * torch.rand(N, C, generator=g) - 5
    d.view(-1)[0], d.view(-1)[-1] = 5.0, -5.0
    mask = (torch.rand(N, C, generator=g) < 0.8).to(torch.int32)
    mask[0, C - 1] = 1
    if N > 1:
        mask[1] = 0
    rollout = logp + 0.3 * torch.randn(N, C, generator=g)
    return {"logp": logp.to(F32), "ref": (logp + d).to(F32), "adv": torch.randn(N, generator=g).to(F32) * 2, "mask": mask, "beta": 0.04, "nt": N + 3,
            "rollout": (rollout * mask).to(F32), "cap": 1.25}


def grpo_math(I, emu, fault=None, level=None):
    """grpo_loss (level None) or grpo_loss_is (0 token / 1 sequence): kl, dlogp, row_loss, row_kl and their E"""
    wd = F32 if emu else F64
    lp, rf, A, m = I["logp"].to(wd), I["ref"].to(wd), I["adv"].to(wd)[:, None], I["mask"].to(wd)
    beta, C = torch.tensor(I["beta"], dtype=F32).to(wd), lp.shape[1]
    ms = m.clone()
    if fault == "second_trip":
        ms[:, 256:] = 0
    d = rf - lp
    e = torch.exp(d)
    kl = e - d - 1
    cnt = m.sum(-1, keepdim=True)
    inv = 1 / cnt if fault == "cnt0_div" else torch.where(cnt > 0, 1 / cnt.clamp(min=1), torch.zeros_like(cnt))
    w = torch.ones_like(lp)
    if level is not None:
        dq = torch.where(m > 0, lp - I["rollout"].to(wd), torch.zeros_like(lp))
        ratio = torch.exp(dq) if level == 0 else torch.exp(dq.sum(-1, keepdim=True) * inv).expand_as(lp)
        w = ratio.clamp(max=torch.tensor(I["cap"], dtype=F32).to(wd))
    Ekl = e + d.abs() + 1
    out = {"kl": kl, "E_kl": Ekl, "row_loss": (ms * (w * -(A - beta * kl))).sum(-1) * inv[:, 0], "row_kl": (ms * kl).sum(-1) * inv[:, 0],
           "E_row_loss": (m * w * (A.abs() + beta * Ekl)).sum(-1) * inv[:, 0], "E_row_kl": (m * Ekl).sum(-1) * inv[:, 0],
           "dlogp": w * (m * inv / I["nt"] * (-A + beta * (1 - e))), "E_dlogp": w * m * inv / I["nt"] * (A.abs() + beta * (1 + e))}
    return out


# ======================================================================================================================================================
# optimizer
# ======================================================================================================================================================

SUMSQ_N = (3, 5, 10007, 2097152 + 1203)
ADAM_CAP = 4096 * 1024
# (n, step, weight_decay, grad_scale, clip): clip = None (norm2 NULL), "below" / "above" (norm a 1000th under / over max_norm 1), "off" (max_norm <= 0)
ADAM_CASES = [(1, 1, 0.1, 1.0, None), (3, 2, 0.1, 1.0, "below"), (10007, 1, 0.1, 1.0, "above"), (10007, 2, 0.1, 1.0, "below"), (10007, 1000, 0.0, 0.125, "off"),
              (10007, 1000, 0.1, 0.125, "above"), (ADAM_CAP + 1027, 2, 0.1, 1.0, None)]
LR, B1, B2, AEPS = 1e-2, 0.9, 0.999, 1e-8


SUMSQ_CAP = 2048 * 1024
SUMSQ_KINDS = ("normal", "mixed")          # N(0,1): every element carries the same weight; mixed: a few 1e4 entries among 1e-4 ones


@functools.lru_cache(maxsize=None)
def sumsq_inputs(n, kind="normal"):
    g = gen(n)
    if kind == "normal":
        return torch.randn(n, generator=g).to(F32)
    x = 1e-4 * torch.randn(n, generator=g)
    x[torch.randint(0, n, (min(n, 5),), generator=g)] = 1e4
    x[n - 1] = -2e4                                 # the tail element (n % 4 != 0) carries weight
    return x.to(F32)


def sumsq_math(x, emu, fault=None):
    """sum of squares: float64, or the kernel's two-stage fp32 tree (4 elements per thread trip, block sums, one block over the partials)"""
    n = x.numel()
    if not emu:
        x = x.double()
        if fault == "sumsq_past_cap":           # the second trip of the grid-stride loop over the float4 groups
            x = torch.cat([x[:SUMSQ_CAP], x[n - n % 4:]])
        elif fault == "sumsq_tail":
            x = x[: n - n % 4]
        return (x * x).sum()
    blocks = max(1, min(2048, (n // 4 + 255) // 256))
    x4 = x[: n - n % 4].view(-1, 4)
    q = (x4[:, 0] * x4[:, 0] + x4[:, 1] * x4[:, 1] + x4[:, 2] * x4[:, 2] + x4[:, 3] * x4[:, 3])
    K = -(-max(1, q.numel()) // (blocks * 256))
    q = torch.cat([q, torch.zeros(K * blocks * 256 - q.numel())]).view(K, blocks, 256)
    acc = torch.zeros(blocks, 256)
    for k in range(K):
        acc = acc + q[k]
    acc[0, : n % 4] += x[n - n % 4:] ** 2
    part = acc.sum(-1)
    return torch.cat([part, torch.zeros((-blocks) % 256)]).view(-1, 256).sum(0).sum()


def sumsq_chain(n):
    blocks = max(1, min(2048, (n // 4 + 255) // 256))
    return 4 * (-(-(n // 4 + 1) // (blocks * 256))) + 16 + (-(-blocks // 256)) + 16


@functools.lru_cache(maxsize=2)
def adam_inputs(n, step):
    g = gen(n + step)
    w, gr = torch.randn(n, generator=g), torch.randn(n, generator=g)
    m = 0.1 * torch.randn(n, generator=g) if step > 1 else torch.zeros(n)
    v = 0.01 * torch.rand(n, generator=g) if step > 1 else torch.zeros(n)
    if n > 100:
        gr[5], v[5], m[5] = 0, 0, 0                       # g = v = 0: the update is 0 / eps
        gr[6], v[6] = 1e-20, 0                            # g^2 underflows
    return w.to(F32), m.to(F32), v.to(F32), gr.to(F32)


def adam_math(n, step, wd_, gs, clip, emu, fault=None):
    wd = F32 if emu else F64
    w, m, v, g = (t.to(wd) for t in adam_inputs(n, step))
    f = lambda a: torch.tensor(a, dtype=F32).to(wd)
    lr, b1, b2, eps, wdec, gsc = f(LR), f(B1), f(B2), f(AEPS), f(wd_), f(gs)
    norm2, max_norm = None, 1.0
    scale = gsc
    if clip in ("below", "above"):
        # the squared norm handed in is chosen so that norm * grad_scale sits a 1000th under / over max_norm (the kernel takes it as given)
        norm2 = torch.tensor(((1 - 1e-3 if clip == "below" else 1 + 1e-3) / gs) ** 2, dtype=F32)
        nrm = norm2.to(wd).sqrt() * gsc
        coef = f(max_norm) / (nrm + f(1e-6))
        if coef < 1 or fault == "clip_when_coef_ge_1":
            scale = scale * coef
    elif clip == "off":
        norm2, max_norm = torch.tensor(4.0, dtype=F32), 0.0
    st = step - 1 if fault == "bias_step_minus_1" else step
    bc1, bc2 = 1 - b1.double() ** st, 1 - b2.double() ** st
    if emu:
        bc1, bc2 = bc1.to(F32), bc2.to(F32)
    ge = g * scale
    if fault == "l2_decay":
        ge, w2 = ge + wdec * w, w
    else:
        w2 = w * (1 - lr * wdec)
    m2 = b1 * m + (1 - b1) * ge
    v2 = b2 * v + (1 - b2) * ge * ge
    upd = (lr / bc1) * m2 / (v2.sqrt() * bc2.rsqrt() + eps)
    w3 = w2 - upd
    if fault in ("adam_tail_n4", "adam_past_cap"):
        lo = n - n % 4 if fault == "adam_tail_n4" else ADAM_CAP
        w3[lo:], m2[lo:], v2[lo:] = w[lo:], m[lo:], v[lo:]
    out = {"master": w3, "m": m2, "v": v2, "norm2": norm2, "max_norm": max_norm}
    if not emu:
        out.update(E_master=w.abs() + upd.abs(), E_m=(b1 * m).abs() + ((1 - b1) * ge).abs(), E_v=b2 * v + (1 - b2) * ge * ge)
    return out


# ======================================================================================================================================================
# decode bookkeeping
# ======================================================================================================================================================

ROPE_POS = (0, 1, 4095, 32767, 131071)


def inv_freq_of(half):
    return (1e6 ** (-np.arange(half, dtype=np.float64) / half)).astype(np.float32)


def rope_table_ref(pos, half):
    """float64 cos / sin of the fp32 product fl32(pos) * inv_freq, and the host libm's fp32 error against them (in ulp(1) = 2^-23)"""
    a32 = pos.astype(np.float32)[:, None] * inv_freq_of(half)[None, :]
    c64, s64 = np.cos(a32.astype(np.float64)), np.sin(a32.astype(np.float64))
    host = max(np.abs(np.cos(a32).astype(np.float64) - c64).max(), np.abs(np.sin(a32).astype(np.float64) - s64).max()) / 2.0 ** -23
    return c64, s64, float(host)


ADV_STEPS, ADV_C, ADV_PAGES, ADV_EOS, ADV_PAD = 40, 35, 5, 7, 3


@functools.lru_cache(maxsize=None)
def advance_inputs(B, eos):
    rs = np.random.RandomState(B)
    sampled = rs.randint(8, 1000, size=(ADV_STEPS, B)).astype(np.int64)
    eos_step = (np.arange(B) * 3 + 2) % 38
    if eos >= 0:
        sampled[eos_step, np.arange(B)] = eos
        late = eos_step + 1 < ADV_STEPS
        sampled[(eos_step + 1)[late], np.arange(B)[late]] = eos          # an EOS sampled after the end is pad, not a second end
    bt = rs.permutation(B * ADV_PAGES).astype(np.int32).reshape(B, ADV_PAGES)
    ctx = np.array([30, 31, 32, 63], dtype=np.int32)[np.arange(B) % 4]
    return sampled, bt, ctx, ctx + 11, eos_step


def advance_model(B, eos):
    """integer model of decode_advance: the state after each of the 40 steps"""
    sampled, bt, ctx, pos, _ = advance_inputs(B, eos)
    ctx, pos = ctx.copy(), pos.copy()
    fin, out, step, states = np.zeros(B, dtype=np.int32), np.full((B, ADV_C), -777, dtype=np.int64), 0, []
    for st in range(ADV_STEPS):
        tok = sampled[st].copy()
        tok[fin == 1] = ADV_PAD
        fin = np.where((fin == 0) & (eos >= 0) & (tok == eos), 1, fin).astype(np.int32)
        if st < ADV_C:
            out[:, st] = tok
        n = ctx.copy()
        pos, ctx = pos + 1, ctx + 1
        slot = bt[np.arange(B), n // 32].astype(np.int64) * 32 + n % 32
        step += 1
        states.append({"cur": tok.copy(), "out": out.copy(), "pos": pos.copy(), "ctx": ctx.copy(), "slot": slot, "fin": fin.copy(), "step": step, "all_done": int(fin.all())})
    return states


# ======================================================================================================================================================
# CPU part: the emulation is inside every bound, every fault model is outside
# ======================================================================================================================================================

@pytest.mark.parametrize("T,H", NORM_CASES)
def test_cpu_norm_emulation_inside_and_faults_outside(T, H):
    I = norm_inputs(T, H)
    rf, lf, rb, lb = norm_refs(T, H)
    er, el = rms_fwd_math(I["x"], I["res"], I["w"], True), ln_fwd_math(I["x"], I["res"], I["w"], I["b"], True)
    xin = rf["res_out"]
    eb = rms_bwd_math(I["dy"], xin, I["w"], rf["rstd"].to(F32), I["dres"], I["dw0"], True)
    elb = ln_bwd_math(I["dy"], xin, I["w"], lf["mean"].to(F32), lf["rstd"].to(F32), I["dres"], I["dw0"], I["db0"], True)
    check_norm("emu", T, H, {"rms.res_out": er["res_out"], "ln.res_out": el["res_out"], "rms.rstd": er["rstd"], "rms.y": er["y"], "rms.dx": eb["dx"], "rms.dw": eb["dw"],
                             "ln.mean": el["mean"], "ln.rstd": el["rstd"], "ln.y": el["y"], "ln.dx": elb["dx"], "ln.dw": elb["dw"], "ln.db": elb["db"]})
    big = [ROW_BIG]
    if H > 8:           # at H = 8 the last chunk is the whole row
        bad = rms_fwd_math(I["x"], I["res"], I["w"], False, "stat_last_chunk")
        fault_excess("stat_last_chunk", "rms.rstd", bad["rstd"], rf["rstd"], rf["rstd"], H, rows=big)
        fault_excess("stat_last_chunk", "rms.y", bad["y"], rf["y"], rf["y"].abs(), H, rows=big)
    if 512 * nc_of(H) != H:
        bad = rms_fwd_math(I["x"], I["res"], I["w"], False, "stat_div_512nc")
        live = [r for r in range(T) if T == 1 or r not in (ROW_ZERO, ROW_TINY)]       # where eps dominates the divisor does not matter
        fault_excess("stat_div_512nc", "rms.y", bad["y"], rf["y"], rf["y"].abs(), H, rows=live)
    args = (I["dy"], xin, I["w"], rf["rstd"].to(F32), I["dres"], I["dw0"])
    if T >= 5:
        fault_excess("no_projection", "rms.dx", rms_bwd_math(*args, False, "no_projection")["dx"], rb["dx"], rb["E_dx"], H, rows=[ROW_PROJ])
        rows = [r for r in range(T) if r not in (ROW_ZERO, ROW_TINY)]          # where eps dominates rstd is 1000: dres is below a bf16 ulp of dx there
        fault_excess("no_dres", "rms.dx", rms_bwd_math(*args, False, "no_dres")["dx"], rb["dx"], rb["E_dx"], H, rows=rows)
    fault_excess("dw_overwrite", "rms.dw", rms_bwd_math(*args, False, "dw_overwrite")["dw"][None], rb["dw"][None], rb["E_dw"][None], T)
    largs = (I["dy"], xin, I["w"], lf["mean"].to(F32), lf["rstd"].to(F32), I["dres"], I["dw0"], I["db0"])
    if T >= 5:
        fault_excess("db_last_row", "ln.db", ln_bwd_math(*largs, False, "db_last_row")["db"][None], lb["db"][None], lb["E_db"][None], T)
    if T == 229:        # 58 blocks: the partials the 8-loads branch of the reduction leaves to the tail loop
        fault_excess("partials_ge_56", "rms.dw", rms_bwd_math(*args, False, "partials_ge_56")["dw"][None], rb["dw"][None], rb["E_dw"][None], T)
    if T == 2051:
        fault_excess("dw_rows_ge_2048", "rms.dw", rms_bwd_math(*args, False, "dw_rows_ge_2048")["dw"][None], rb["dw"][None], rb["E_dw"][None], T)
    if T >= 5 and 264 <= H <= 520:     # at larger H the n 2^-24 term of the bound (the worst case of ANY order of adding H terms) is as large as this fault
        bad = ln_fwd_math(I["x"], I["res"], I["w"], I["b"], False, "ln_onepass_var")
        fault_excess("ln_onepass_var", "ln.rstd", bad["rstd"], lf["rstd"], lf["E_rstd"], H, rows=[ROW_OFFSET], per_element=True)


@pytest.mark.parametrize("case", X32_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_cpu_rmsnorm_x32_emulation_inside_and_faults_outside(case):
    T, H, ns, ub, ur, mode = case
    I = x32_inputs(T, H, ns)
    ref, emu = x32_math(I, ub, ur, False), x32_math(I, ub, ur, True)
    assert same_bits(emu["branch"], ref["branch"]), "the dyadic slabs must add exactly in fp32"
    if ur:
        assert same_bits(emu["res_out"], ref["res_out"])
    check("emu", "rms.rstd", emu["rstd"], ref["rstd"], ref["rstd"], H)
    check("emu", "rms.y", emu["y"], ref["y"], ref["y"].abs(), H)
    live = [r for r in range(T) if T < 3 or r not in (ROW_ZERO, ROW_TINY)]
    if ns >= 2:
        fault_excess("drop_slab", "rms.y", x32_math(I, ub, ur, False, "drop_slab")["y"], ref["y"], ref["y"].abs(), H, rows=live)
    if ub:
        fault_excess("no_xbias", "rms.y", x32_math(I, ub, ur, False, "no_xbias")["y"], ref["y"], ref["y"].abs(), H, rows=live)
    if ur and T * H >= 64:
        fault_mismatch("round_after_res", x32_math(I, ub, ur, False, "round_after_res")["res_out"], ref["res_out"])


@pytest.mark.parametrize("case", ROPE_CASES)
def test_cpu_rope_emulation_inside_and_faults_outside(case):
    T, nh, D, extra = case
    I = rope_inputs(*case)
    for backward in (False, True):
        ref, E = rope_math(I["x"], I["cos"], I["sin"], nh, D, backward, False)
        emu, _ = rope_math(I["x"], I["cos"], I["sin"], nh, D, backward, True)
        check("emu", "rope", emu, ref, E, 0, f"{case} backward={backward}")
        if T > 100:
            continue
        if backward:
            fault_excess("rope_bwd_sign", "rope", rope_math(I["x"], I["cos"], I["sin"], nh, D, True, False, "rope_bwd_sign")[0], ref, E)
        fault_excess("rope_row_t_minus_1", "rope", rope_math(I["x"], I["cos"], I["sin"], nh, D, backward, False, "rope_row_t_minus_1")[0], ref, E)
        if D == 80 and extra >= 1:
            fault_excess("rope_partner_64", "rope", rope_math(I["x"], I["cos"], I["sin"], nh, D, backward, False, "rope_partner_64")[0], ref, E)


@pytest.mark.parametrize("name", UNARY)
def test_cpu_unary_emulation_inside_and_faults_outside(name):
    for big in (False, True):
        z, da = unary_inputs(big)
        f, Ef, b, Eb = unary_math(name, z, da, False)
        ef, _, eb, _ = unary_math(name, z, da, True)
        check("emu", name + ".fwd", ef, f, Ef, 0, f"{name} fwd big={big}")
        check("emu", name + ".bwd", eb, b, Eb, 0, f"{name} bwd big={big}")
    z, da = unary_inputs(False)
    f, Ef, b, Eb = unary_math(name, z, da, False)
    x = z.double()
    if name in ("gelu", "gelu_tanh"):       # the two GELUs part in the negative tail, where 1 + erf cancels
        sel = ((x >= -4) & (x <= -3)).nonzero()[:, 0]
        bad = unary_math(name, z, da, False, "gelu_swap")
        fault_excess("gelu_swap", name + ".fwd", bad[0], f, Ef, 0, rows=sel, per_element=True)
        fault_excess("gelu_swap", name + ".bwd", bad[2][sel][None], b[sel][None], Eb[sel][None], 0)          # the derivatives cross inside the range: its worst element
    else:
        sel = ((x.abs() >= 0.5) & (x.abs() <= 2)).nonzero()[:, 0]           # further out both sigmoids saturate
        bad = unary_math(name, z, da, False, "quick_as_silu")
        fault_excess("quick_as_silu", name + ".fwd", bad[0], f, Ef, 0, rows=sel, per_element=True)


def test_cpu_swiglu_emulation_inside_and_faults_outside():
    for big in (False, True):
        gu, da = swiglu_inputs(big)
        ref, emu = swiglu_math(gu, da, False), swiglu_math(gu, da, True)
        for k in ("a", "dgate", "dup"):
            check("emu", "swiglu." + k, emu[k], ref[k], ref["E_" + k], 0, f"swiglu {k} big={big}")
    gu, da = swiglu_inputs(False)
    ref = swiglu_math(gu, da, False)
    g = gu[0, : gu.shape[1] // 2].double()
    sel = ((g.abs() >= 0.5) & (g.abs() <= 4)).nonzero()[:, 0]
    bad = swiglu_math(gu, da, False, "dgate_no_term")
    fault_excess("dgate_no_term", "swiglu.dgate", bad["dgate"].T, ref["dgate"].T, ref["E_dgate"].T, 0, rows=sel, per_element=True)
    # the inner rounding moves a product by one bf16 ulp, inside the bound by construction (docstring): it is caught by the equality on the products with one correct bit pattern
    want, ok = swiglu_exact(gu)
    assert int(ok.sum()) > ok.numel() // 2
    assert bool((bits(swiglu_math(gu, da, True)["a"].to(BF)) == bits(want))[ok].all()), "the fp32 emulation must give the one correct bit pattern where it is robust"
    bad = swiglu_math(gu, da, True, "swiglu_no_inner_round")["a"].to(BF)
    assert fault_mismatch("swiglu_no_inner_round", bad[ok], want[ok]) >= 100


@pytest.mark.parametrize("T,N", COLSUM_CASES)
def test_cpu_colsum_emulation_inside_and_faults_outside(T, N):
    dy, out0 = colsum_inputs(T, N)
    ref = reduce_rows(dy.double(), out0, False, kind="colsum")
    E = out0.abs().double() + dy.double().abs().sum(0)
    check("emu", "colsum", reduce_rows(dy.float(), out0, True, kind="colsum"), ref, E, T, f"T={T} N={N}")
    if T == 3650:
        fault_excess("partials_ge_56", "colsum", reduce_rows(dy.double(), out0, False, "partials_ge_56", "colsum")[None], ref[None], E[None], T)
    if T >= 70:
        fault_excess("last_row_group", "colsum", reduce_rows(dy.double(), out0, False, "last_row_group", "colsum")[None], ref[None], E[None], T)


@pytest.mark.parametrize("H", MAP_H)
def test_cpu_row_maps_emulation_inside_and_faults_outside(H):
    src, lists, ptr, idx, wts = gather_inputs(H)
    for w in (wts, None):
        ref, E = gather_math(src, lists, w, False)
        check("emu", "gather", gather_math(src, lists, w, True)[0], ref, E, 9, f"gather H={H}")
        assert bool((ref[0] == 0).all()) and bool((ref[3] == 0).all())
    ref, E = gather_math(src, lists, wts, False)
    fault_excess("weights_ignored", "gather", gather_math(src, lists, wts, False, "weights_ignored")[0], ref, E, 9, rows=[1, 2, 4, 5, 6])
    fault_excess("entry_skipped", "gather", gather_math(src, lists, wts, False, "entry_skipped")[0], ref, E, 9, rows=[2, 6])
    src, dst_rows, dst0 = scatter_inputs(H)
    ref, E = scatter_math(src, dst_rows, dst0, False)
    check("emu", "scatter", scatter_math(src, dst_rows, dst0, True)[0], ref, E, 17, f"scatter H={H}")
    bad = scatter_math(src, dst_rows, dst0, False, "entry_skipped")[0]
    fault_excess("entry_skipped", "scatter", bad, ref, E, 17, rows=[7])


@pytest.mark.parametrize("R,V,ld", LP_CASES)
def test_cpu_logprob_emulation_inside_and_faults_outside(R, V, ld):
    buf, tgt = lp_inputs(R, V, ld)
    lse, logp, El, Ep = lp_math(buf, V, tgt, False)
    assert bool(torch.isfinite(lse).all())
    el, ep, _, _ = lp_math(buf, V, tgt, True)
    one = torch.ones_like(El)
    check("emu", "lp.lse", el, lse, El, V, f"R={R} V={V}", En=one)
    check("emu", "lp.logp", ep, logp, Ep, V, f"R={R} V={V}", En=one)
    if R > 8:
        assert float(logp[LP_IGN]) == 0 and float(logp[LP_GE_V]) == 0 and float(logp[LP_TAIL_INF]) > -INF and float(logp[LP_HEAD_INF]) == -INF and float(ep[LP_HEAD_INF]) == -INF
        fault_excess("ignored_not_zeroed", "lp.logp", lp_math(buf, V, tgt, False, "ignored_not_zeroed")[1], logp, Ep, V, rows=[LP_IGN, LP_GE_V], per_element=True, En=one)
        if V % 4 and V >= 4:
            fault_excess("lp_tail_v4", "lp.lse", lp_math(buf, V, tgt, False, "lp_tail_v4")[0], lse, El, V, rows=[LP_PEAK], per_element=True, En=one)
        if V > 1024:
            fault_excess("lp_max_first_1024", "lp.lse", lp_math(buf, V, tgt, False, "lp_max_first_1024")[0], lse, El, V, rows=[LP_PEAK], per_element=True, En=one)
    if V % 8 == 0:
        gvec = torch.randn(R, generator=gen(R)).to(F32) * 2
        gvec[tgt < 0] = 0
        ref, E = dlogits_math(buf, V, tgt, lse.to(F32), gvec, False)
        check("emu", "dlogits", dlogits_math(buf, V, tgt, lse.to(F32), gvec, True)[0], ref, E, 0, f"dlogits R={R} V={V}")


@pytest.mark.parametrize("R,V", DLOGITS_EXTRA)
def test_cpu_dlogits_extra_emulation_inside(R, V):
    x, tgt, gvec, lse32 = dlogits_extra_inputs(R, V)
    ref, E = dlogits_math(x, V, tgt, lse32, gvec, False)
    check("emu", "dlogits", dlogits_math(x, V, tgt, lse32, gvec, True)[0], ref, E, 0, f"dlogits R={R} V={V}")
    assert bool((ref[tgt < 0] == 0).all())


@pytest.mark.parametrize("R,C,with_bias", BIAS_CAST_CASES)
def test_cpu_bias_cast_emulation_inside(R, C, with_bias):
    """f32_bias_to_bf16 = bf16(fl32(in + bias)); the plain casts, embed_fwd and decode_advance are exact maps: their GPU tests compare bits with torch / an integer model"""
    x, bias = bias_cast_inputs(R, C)
    b = bias if with_bias else torch.zeros_like(bias)
    check("emu", "bias_cast", (x + b.float()).to(BF), x.double() + b.double(), x.double().abs() + b.double().abs(), 0, f"R={R} C={C}")


@pytest.mark.parametrize("N,C", GRPO_CASES)
def test_cpu_grpo_emulation_inside_and_faults_outside(N, C):
    I = grpo_inputs(N, C)
    for level in (None, 0, 1):
        ref, emu = grpo_math(I, False, level=level), grpo_math(I, True, level=level)
        check("emu", "grpo.kl", emu["kl"], ref["kl"], ref["E_kl"])
        check("emu", "grpo.dlogp", emu["dlogp"], ref["dlogp"], ref["E_dlogp"])
        check("emu", "grpo.row", emu["row_loss"], ref["row_loss"], ref["E_row_loss"], C)
        check("emu", "grpo.row", emu["row_kl"], ref["row_kl"], ref["E_row_kl"], C)
    ref = grpo_math(I, False)
    if N > 1:
        assert float(ref["row_loss"][1]) == 0 and bool((ref["dlogp"][1] == 0).all())
        fault_excess("cnt0_div", "grpo.row", grpo_math(I, False, "cnt0_div")["row_loss"], ref["row_loss"], ref["E_row_loss"], C, rows=[1], per_element=True)
    if C == 300:
        rows = [r for r in range(N) if r != 1 or N == 1]
        fault_excess("second_trip", "grpo.row", grpo_math(I, False, "second_trip")["row_kl"], ref["row_kl"], ref["E_row_kl"], C, rows=rows, per_element=True)


@pytest.mark.parametrize("kind", SUMSQ_KINDS)
@pytest.mark.parametrize("n", SUMSQ_N)
def test_cpu_sumsq_emulation_inside_and_faults_outside(n, kind):
    x = sumsq_inputs(n, kind)
    ref = sumsq_math(x, False)
    check("emu", "sumsq", sumsq_math(x, True), ref, ref, sumsq_chain(n), f"n={n} {kind}")
    if n > SUMSQ_CAP and kind == "normal":          # the 1200 elements of the second trip: 5.7e-4 of the sum
        fault_excess("sumsq_past_cap", "sumsq", sumsq_math(x, False, "sumsq_past_cap").reshape(1), ref.reshape(1), ref.reshape(1), sumsq_chain(n), per_element=True)
    if n % 4 and (kind == "mixed" or n <= 10007):   # among 2 * 10^6 N(0,1) elements three are below the bound: the mixed input puts -2e4 in the tail there
        fault_excess("sumsq_tail", "sumsq", sumsq_math(x, False, "sumsq_tail").reshape(1), ref.reshape(1), ref.reshape(1), sumsq_chain(n), per_element=True)


@pytest.mark.parametrize("case", ADAM_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_cpu_adamw_emulation_inside_and_faults_outside(case):
    n, step, wd_, gs, clip = case
    ref, emu = adam_math(*case, False), adam_math(*case, True)
    for k in ("m", "v", "master"):
        check("emu", "adam." + k, emu[k], ref[k], ref["E_" + k], 0, f"adamw {k} {case}")
    bad = lambda f: adam_math(*case, False, f)
    ex = lambda f, k, rows=None: fault_excess(f, "adam." + k, bad(f)[k], ref[k], ref["E_" + k], 0, rows=rows, per_element=True)
    if wd_ > 0 and step == 1 and n > 100:      # first step: the update is lr sign(g) either way, what is left is the decay itself (later the two forms can cancel)
        ex("l2_decay", "master", rows=[i for i in range(7, 100) if abs(float(adam_inputs(n, step)[0][i])) >= 0.1])       # past the two special elements; the decay is lr wd |w|: weights that are not ~0
    if step == 2 and n < ADAM_CAP:
        ex("bias_step_minus_1", "master", rows=torch.arange(7, 100) if n > 100 else None)
    if clip == "below" and n > 100:
        ex("clip_when_coef_ge_1", "m", rows=torch.arange(7, 100))
    if n % 4 and n < ADAM_CAP:
        ex("adam_tail_n4", "m", rows=torch.arange(n - n % 4, n))
    if n > ADAM_CAP:
        ex("adam_past_cap", "m", rows=torch.arange(ADAM_CAP, n))


def test_cpu_rope_table_host_error_and_advance_model():
    for half in (64, 40):
        pos = np.array([ROPE_POS[i % 5] for i in range(37)], dtype=np.int32)
        c64, s64, host = rope_table_ref(pos, half)
        ROPE_TABLE_ERR[("host", half)] = host
        assert host <= 4.0, f"the host's own fp32 cos / sin are {host:.2f} ulp(1) off: the reference arguments are wrong"
        assert np.abs(c64 ** 2 + s64 ** 2 - 1).max() < 1e-12
    for B in (1, 37, 256):
        for eos in (ADV_EOS, -1):
            st = advance_model(B, eos)
            _, bt, ctx0, _, eos_step = advance_inputs(B, eos)
            slots = np.stack([s["slot"] for s in st])
            assert len(np.unique(slots)) == slots.size and int(st[-1]["ctx"].max()) // 32 < ADV_PAGES          # one cache slot per (sequence, step), inside the table
            done = [s["all_done"] for s in st]
            if eos >= 0:
                assert done.index(1) == int(eos_step.max()) and all(done[done.index(1):]), "all_done flips on the step the last sequence finishes"
                assert bool((st[-1]["out"][np.arange(B), np.minimum(eos_step, ADV_C - 1)] == np.where(eos_step < ADV_C, eos, st[-1]["out"][:, ADV_C - 1])).all())
            else:
                assert not any(done) and not st[-1]["fin"].any()


def test_cpu_every_fault_model_was_exercised_and_emulation_record():
    """Every fault model of FAULT_MODELS was applied somewhere above (run the whole CPU part: this test reads what the others recorded)."""
    missing = [f for f in FAULT_MODELS if f not in FAULT_SEEN]
    assert not missing, f"fault models never exercised: {missing}"
    for f in FAULT_MODELS:
        print(f"[tokenwise_f64 cpu] fault {f}: smallest excess at its designated elements {FAULT_SEEN[f]:.3g} x bound")
    _print_used("emu")


def _print_used(side):
    fam = {}
    for key, v in sorted(USED[side].items()):
        print(f"[tokenwise_f64 {side}] {key}: largest used fraction of the bound {v:.4f}")
        f = FAMILY[key.split(".")[0]]
        fam[f] = max(fam.get(f, 0.0), v)
    for f, v in sorted(fam.items()):
        print(f"[tokenwise_f64 {side}] family {f}: largest used fraction {v:.4f}")


# ======================================================================================================================================================
# GPU part
# ======================================================================================================================================================

def pattern(n, dtype):
    """the sentinel: finite, recognisable, different from element to element"""
    return (-(700 + (torch.arange(n, device=DEV) % 29))).to(dtype)


class Guard:
    """A [rows, cols] view (leading dimension ld) inside a larger sentinel-filled buffer: `lead` / `trail` rows around it, the columns cols .. ld between its rows, and
    `off` elements in front.  intact(): everything outside the view still holds the sentinel, bit for bit; untouched(): the view as well."""

    def __init__(self, rows, cols, dtype, ld=None, init=None, lead=2, trail=2, off=0):
        ld = ld or cols
        R = rows + lead + trail
        self.buf = pattern(R * ld + off, dtype)
        box = lambda t: t[off:].view(R, ld)[lead: lead + rows, :cols]
        self.view = box(self.buf)
        if init is not None:
            self.view.copy_(init.to(DEV))
        self.keep = torch.ones(R * ld + off, dtype=torch.bool, device=DEV)
        box(self.keep)[:] = False
        self.saved = self.buf.clone()

    def intact(self, what):
        assert torch.equal(bits(self.buf)[self.keep], bits(self.saved)[self.keep]), f"{what}: memory around the output was written"

    def untouched(self, what):
        assert torch.equal(bits(self.buf), bits(self.saved)), f"{what}: a buffer that must not change was written"


def vec(n, dtype, init=None):
    """a guarded vector"""
    return Guard(1, n, dtype, ld=n + (-n) % 4 + 4, init=None if init is None else init.reshape(1, -1), lead=1, trail=1)


def workspace(nbytes):
    """fp32 scratch of exactly nbytes with sentinels behind it"""
    return vec(max(1, int(nbytes) // 4), F32)


def call_guarded(name, args, guards, what):
    """hip.call(name, *args) with Guard objects standing for their views; then every guard's surroundings are checked.  Returns the guards."""
    hip.call(name, *[a.view if isinstance(a, Guard) else a for a in args])
    torch.cuda.synchronize()
    for g in guards:
        g.intact(f"{name} {what}")


def refused(name, args, outputs, what):
    """the launcher must refuse on the host (no launch) and leave the outputs alone"""
    with pytest.raises(RuntimeError):
        hip.call(name, *[a.view if isinstance(a, Guard) else a for a in args])
    torch.cuda.synchronize()
    for g in outputs:
        g.untouched(f"{name} refused ({what})")


def d(t):
    return t.to(DEV)


EPS32 = float(np.float32(EPS))


@pytest.mark.gpu
@pytest.mark.parametrize("T,H", NORM_CASES)
def test_gpu_norm_fwd_bwd(T, H):
    """rmsnorm / layernorm forward (strided x, res, y; res_out, stats) and backward (dx, accumulated dw / db, dw = NULL, run-to-run bits) against float64"""
    I = norm_inputs(T, H)
    rf, lf, rb, lb = norm_refs(T, H)
    ldx, ldr, ldy = H + 8, H + 16, H + 24
    w, b = vec(H, BF, I["w"]), vec(H, BF, I["b"])
    got = {}
    for fam in ("rms", "ln"):
        x, res = Guard(T, H, BF, ldx, I["x"]), Guard(T, H, BF, ldr, I["res"])
        ro, y, st1, st2 = Guard(T, H, BF, ldr), Guard(T, H, BF, ldy), vec(T, F32), vec(T, F32)
        if fam == "rms":
            call_guarded("rmsnorm_fwd", (x, None, 0, None, res, ro, w, y, st1, T, H, ldx, ldr, ldy, EPS32, None), (ro, y, st1), f"T={T} H={H}")
            got["rms.rstd"] = st1.view[0]
        else:
            call_guarded("layernorm_fwd", (x, res, ro, w, b, y, st1, st2, T, H, ldx, ldr, ldy, EPS32), (ro, y, st1, st2), f"T={T} H={H}")
            got["ln.mean"], got["ln.rstd"] = st1.view[0], st2.view[0]
        x.untouched(fam + " x")
        res.untouched(fam + " res")
        got[fam + ".res_out"], got[fam + ".y"] = ro.view, y.view
    ld = H + 8
    xin = rf["res_out"]
    dy, xg, dres = Guard(T, H, BF, ld, I["dy"]), Guard(T, H, BF, ld, xin), Guard(T, H, BF, ld, I["dres"])
    rstd, mean, lrstd = vec(T, F32, rf["rstd"].to(F32)), vec(T, F32, lf["mean"].to(F32)), vec(T, F32, lf["rstd"].to(F32))
    runs = {}
    for fam in ("rms", "ln"):
        for rep in ("a", "b", "nodw"):
            dx, dw, db = Guard(T, H, BF, ld), vec(H, F32, I["dw0"]), vec(H, F32, I["db0"])
            nb = hip.lib().iadr1_rmsnorm_bwd_workspace_bytes(T, H) if fam == "rms" else hip.lib().iadr1_layernorm_bwd_workspace_bytes(T, H)
            ws = workspace(nb)
            pw, pb, pws = (None, None, None) if rep == "nodw" else (dw, db, ws)
            if fam == "rms":
                call_guarded("rmsnorm_bwd", (dy, xg, w, rstd, dres, dx, pw, pws, T, H, ld), (dx, dw, ws), f"T={T} H={H} {rep}")
            else:
                call_guarded("layernorm_bwd", (dy, xg, w, mean, lrstd, dres, dx, pw, pb, pws, T, H, ld), (dx, dw, db, ws), f"T={T} H={H} {rep}")
            if rep == "nodw":
                dw.untouched("dw = NULL")
                db.untouched("db = NULL")
                ws.untouched("workspace with dw = NULL")
            runs[fam, rep] = (dx.view.clone(), dw.view[0].clone(), db.view[0].clone())
        assert all(same_bits(p, q) for p, q in zip(runs[fam, "a"], runs[fam, "b"])), f"{fam} backward: two runs differ in bits (T={T} H={H})"
        assert same_bits(runs[fam, "a"][0], runs[fam, "nodw"][0]), f"{fam} backward: dx depends on whether dw is asked for"
        got[fam + ".dx"], got[fam + ".dw"] = runs[fam, "a"][0], runs[fam, "a"][1]
    got["ln.db"] = runs["ln", "a"][2]
    for g in (dy, xg, dres, w, b, rstd, mean, lrstd):
        g.untouched("norm inputs")
    check_norm("gpu", T, H, got)


@pytest.mark.gpu
@pytest.mark.parametrize("H", NORM_H)
def test_gpu_rmsnorm_row_bits_do_not_depend_on_T(H):
    """A row of rmsnorm_fwd (bf16 x, row-major out) has the same bits launched alone as inside a T = 229 launch (the launcher's promise: the chunked passes rely on it)."""
    I = norm_inputs(229, H)
    x, w = d(I["x"]), d(I["w"])
    y, _ = ops.rmsnorm_fwd(x, w, EPS, want_rstd=True)
    for r in (0, 1, 2, 3, 100, 227, 228):
        y1, _ = ops.rmsnorm_fwd(x[r: r + 1], w, EPS, want_rstd=True)
        assert same_bits(y1[0], y[r]), f"H={H} row {r}: T = 1 and T = 229 give different bits"


@pytest.mark.gpu
@pytest.mark.parametrize("case", X32_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_gpu_rmsnorm_x32(case):
    """rmsnorm_fwd over fp32 partial slabs: every slab-summing path, xbias, res with and without res_out, y = NULL, decode-packed output, the wave kernel at T > 256"""
    T, H, ns, ub, ur, mode = case
    I = x32_inputs(T, H, ns)
    ref = x32_math(I, ub, ur, False)
    slabs = Guard(ns * T, H, F32, init=I["slabs"].reshape(ns * T, H))
    xb, w = (vec(H, BF, I["xbias"]) if ub else None), vec(H, BF, I["w"])
    ldr = H + 8
    res = Guard(T, H, BF, ldr, I["res"]) if ur else None
    ro = Guard(T, H, BF, ldr) if (ur and mode != "no_res_out") else None
    rstd = vec(T, F32)
    what = f"x32 {case}"
    if mode == "packed":
        y = ops.PackedAct(T, H, DEV)
        yg = Guard(1, y.buf.numel(), BF, init=y.buf[None])          # the packed buffer (zeros: the pad rows stay zero) inside sentinels
        y.buf = yg.view[0]
        call_guarded("rmsnorm_fwd", (None, slabs, ns, xb, res, ro, w, yg, rstd, T, H, H, ldr, 0, EPS32, None), (yg,), what)
        full = y.buf.view(-1, H // 32, 4, 4, 16, 8).permute(0, 2, 4, 1, 3, 5).reshape(-1, H)
        assert bool((full[T:] == 0).all()), f"{what}: pad rows of the packed output were written"
        ygot = y.unpack()
    elif mode == "rstd_only":
        call_guarded("rmsnorm_fwd", (None, slabs, ns, xb, res, ro, w, None, rstd, T, H, H, ldr, H, EPS32, None), (), what)       # y = NULL: rstd is the only output
        ygot = None
    else:
        y = Guard(T, H, BF, H + 16)
        call_guarded("rmsnorm_fwd", (None, slabs, ns, xb, res, ro, w, y, rstd, T, H, H, ldr, H + 16, EPS32, None), (y,), what)
        ygot = y.view
    rstd.intact(what)
    slabs.untouched(what + " slabs")
    w.untouched(what + " w")
    if ub:
        xb.untouched(what + " xbias")
    if ur:
        res.untouched(what + " res")
    if ro is not None:
        ro.intact(what)
        assert same_bits(ro.view.cpu(), ref["res_out"]), f"{what}: res_out != bf16(bf16(sum of slabs [+ bias]) + res)"
    check("gpu", "rms.rstd", rstd.view[0], ref["rstd"], ref["rstd"], H, what)
    if ygot is not None:
        check("gpu", "rms.y", ygot, ref["y"], ref["y"].abs(), H, what)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROPE_CASES)
def test_gpu_rope(case):
    """rope_inplace forward and backward against the float64 rotation and its transpose, strided rows, trailing heads untouched"""
    T, nh, D, extra = case
    I = rope_inputs(*case)
    cos, sin = d(I["cos"]), d(I["sin"])
    for backward in (0, 1):
        ref, E = rope_math(I["x"], I["cos"], I["sin"], nh, D, bool(backward), False)
        ld = (nh + extra) * D + 8
        x = Guard(T, nh * D, BF, ld, I["x"][:, : nh * D])          # the trailing heads and the row padding hold the sentinel
        call_guarded("rope_inplace", (x, ld, cos, sin, T, nh, D, backward), (x,), f"{case} backward={backward}")
        check("gpu", "rope", x.view, ref, E, 0, f"{case} backward={backward}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", UNARY)
def test_gpu_unary_activations(name):
    """every bf16 value of the grid x every da, and one call past the grid cap, forward and backward"""
    for big in (False, True):
        z, da = unary_inputs(big)
        f, Ef, b, Eb = unary_math(name, z, da, False)
        n = z.numel()
        zg, dg = Guard(1, n, BF, init=z[None]), Guard(1, n, BF, init=da[None])
        a, dz = Guard(1, n, BF), Guard(1, n, BF)
        call_guarded(name + "_fwd", (zg, a, n), (a,), f"big={big}")
        call_guarded(name + "_bwd", (dg, zg, dz, n), (dz,), f"big={big}")
        zg.untouched(name + " z")
        dg.untouched(name + " da")
        check("gpu", name + ".fwd", a.view[0], f, Ef, 0, f"{name} fwd big={big}")
        check("gpu", name + ".bwd", dz.view[0], b, Eb, 0, f"{name} bwd big={big}")
    assert same_bits(getattr(ops, name + "_fwd")(zg.view[0]), a.view[0].contiguous()) and same_bits(getattr(ops, name + "_bwd")(dg.view[0], zg.view[0]), dz.view[0].contiguous())


@pytest.mark.gpu
@pytest.mark.parametrize("big", (False, True))
def test_gpu_swiglu(big):
    """swiglu_fwd / swiglu_bwd: the gate grid against every up and da value, and T 260 x I 16136 (the grid-stride wrap falls inside a row); strided gu / a / da / dgu"""
    gu, da = swiglu_inputs(big)
    ref = swiglu_math(gu, da, False)
    T, I = da.shape
    ldg, lda, ldd, ldda = 2 * I + 8, I + 16, 2 * I + 24, I + 8
    gug, dag = Guard(T, 2 * I, BF, ldg, gu), Guard(T, I, BF, ldda, da)
    a, dgu = Guard(T, I, BF, lda), Guard(T, 2 * I, BF, ldd)
    call_guarded("swiglu_fwd", (gug, ldg, a, lda, T, I), (a,), f"big={big}")
    call_guarded("swiglu_bwd", (dag, ldda, gug, ldg, dgu, ldd, T, I), (dgu,), f"big={big}")
    gug.untouched("gu")
    dag.untouched("da")
    check("gpu", "swiglu.a", a.view, ref["a"], ref["E_a"], 0, f"big={big}")
    check("gpu", "swiglu.dgate", dgu.view[:, :I], ref["dgate"], ref["E_dgate"], 0, f"big={big}")
    check("gpu", "swiglu.dup", dgu.view[:, I:], ref["dup"], ref["E_dup"], 0, f"big={big}")
    if not big:
        assert same_bits(ops.swiglu_fwd(gug.view), a.view.contiguous())
        want, ok = swiglu_exact(gu)         # where both roundings are far from a tie there is one correct bit pattern: bf16(bf16(silu(gate)) up)
        assert bool((bits(a.view).cpu() == bits(want))[ok].all()), "swiglu_fwd: a != bf16(bf16(silu(gate)) * up) on products that have one correct value"


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", COLSUM_CASES)
def test_gpu_colsum(T, N):
    dy, out0 = colsum_inputs(T, N)
    ref = reduce_rows(dy.double(), out0, False, kind="colsum")
    E = out0.abs().double() + dy.double().abs().sum(0)
    ld = N + 8
    dyg = Guard(T, N, BF, ld, dy)
    outs = []
    for rep in range(2):
        out, ws = vec(N, F32, out0), workspace(hip.lib().iadr1_colsum_workspace_bytes(T, N))
        call_guarded("colsum_acc", (dyg, ld, out, ws, T, N), (out, ws), f"T={T} N={N}")
        outs.append(out.view[0].clone())
    dyg.untouched("dy")
    assert same_bits(outs[0], outs[1]), "colsum: two runs differ in bits"
    check("gpu", "colsum", outs[0], ref, E, T, f"T={T} N={N}")


@pytest.mark.gpu
@pytest.mark.parametrize("H", MAP_H)
def test_gpu_row_maps(H):
    """rows_gather_sum (weights and NULL, empty lists, repeated rows), rows_scatter_acc (1 and 17 source rows per destination), both twice for run-to-run bits"""
    src, lists, ptr, idx, wts = gather_inputs(H)
    sg = Guard(12, H, BF, init=src)
    T = len(lists)
    for w in (wts, None):
        ref, E = gather_math(src, lists, w, False)
        outs = []
        for rep in range(2):
            out = Guard(T, H, BF)
            call_guarded("rows_gather_sum", (sg, d(ptr), d(idx), d(w) if w is not None else None, out, T, H), (out,), f"H={H}")
            outs.append(out.view.clone())
        assert same_bits(outs[0], outs[1]), "rows_gather_sum: two runs differ in bits"
        check("gpu", "gather", outs[0], ref, E, 9, f"gather H={H} weights={w is not None}")
        assert bool((outs[0][0] == 0).all()) and bool((outs[0][3] == 0).all()), "an empty list gives zeros"
    assert same_bits(ops.rows_gather_sum(sg.view, d(ptr), d(idx), T), outs[0]), "the wrapper reaches the same kernel"
    sg.untouched("gather src")
    src, dst_rows, dst0 = scatter_inputs(H)
    ref, E = scatter_math(src, dst_rows, dst0, False)
    plan = ops.scatter_plan(dst_rows, DEV)
    sg = Guard(40, H, BF, init=src)
    outs = []
    for rep in range(2):
        dst = Guard(9, H, F32, init=dst0)
        ops.rows_scatter_acc(sg.view, plan, dst.view)
        torch.cuda.synchronize()
        dst.intact("rows_scatter_acc")
        outs.append(dst.view.clone())
    sg.untouched("scatter src")
    assert same_bits(outs[0], outs[1]), "rows_scatter_acc: two runs differ in bits"
    check("gpu", "scatter", outs[0], ref, E, 17, f"scatter H={H}")
    for r in (1, 4, 6):
        assert same_bits(outs[0][r].cpu(), dst0[r]), "a destination row no source row feeds must not change"


@pytest.mark.gpu
def test_gpu_embed_fwd():
    """embed_fwd: img_index NULL and given; T * H / 8 just above the grid cap"""
    g = gen(11)
    for T, H, with_img in ((2049, 2048, False), (2049, 2048, True), (13, 264, True), (13, 8, False)):
        E, img = torch.randn(50, H, generator=g).to(BF), torch.randn(9, H, generator=g).to(BF)
        ids = torch.randint(0, 50, (T,), generator=g)
        ii = torch.where(torch.rand(T, generator=g) < 0.3, torch.randint(0, 9, (T,), generator=g), torch.full((T,), -1)).to(torch.int32)
        Eg, ig, out = Guard(50, H, BF, init=E), Guard(9, H, BF, init=img), Guard(T, H, BF)
        call_guarded("embed_fwd", (d(ids), d(ii) if with_img else None, Eg, ig, out, T, H), (out,), f"T={T} H={H}")
        want = torch.where((ii >= 0)[:, None], img[ii.clamp(min=0).long()], E[ids]) if with_img else E[ids]
        assert same_bits(out.view.cpu(), want), f"embed_fwd T={T} H={H} img={with_img}"
        Eg.untouched("E")
        ig.untouched("img")


def cast_values(n, seed):
    """fp32 values for the casts: N(0,1) x 2^k, ties-to-even midpoints, +-0, the last fp32 values below bf16 overflow, fp32 and bf16 denormals"""
    g = gen(seed)
    x = (torch.randn(n, generator=g) * (2.0 ** torch.randint(-30, 30, (n,), generator=g).float())).numpy().view(np.uint32).copy()
    special = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0xBF818000, 0x00000000, 0x80000000, 0x7F7F7FFF, 0xFF7F7FFF, 0x7F7F0000,
                        0x00000001, 0x00008000, 0x00018000, 0x80008001, 0x007FFFFF, 0x00800000], dtype=np.uint32)
    k = min(n, len(special))
    x[np.linspace(0, n - 1, k).astype(np.int64)] = special[:k]
    return torch.from_numpy(x.view(np.float32).copy())


@pytest.mark.gpu
def test_gpu_casts():
    """cast_f32_to_bf16 (vector + scalar tail, R = 1, strided, Cpad > C, misaligned, past the grid cap), cast_bf16_to_f32 (the same), f32_bias_to_bf16"""
    for R, C, ldi, ldo, cpad, off in ((4, 64, 64, 64, 64, 0), (7, 5, 5, 5, 5, 0), (1, 43, 100, 120, 43, 0), (6, 24, 40, 56, 24, 0), (5, 19, 24, 40, 32, 0), (3, 16, 16, 16, 16, 1),
                                      (1, BIG_N + 3, BIG_N + 3, BIG_N + 3, BIG_N + 3, 0)):
        x = cast_values(R * C, R + C).view(R, C)
        xin = Guard(R, C, F32, ldi, x, lead=8, off=off)              # 8 leading rows: the view is 16-byte aligned unless `off` misaligns it
        out = Guard(R, cpad, BF, ldo, lead=8, off=2 * off)
        call_guarded("cast_f32_to_bf16", (xin, ldi, out, ldo, R, C, cpad), (out,), f"R={R} C={C} ldi={ldi} ldo={ldo} Cpad={cpad} off={off}")
        xin.untouched("cast input")
        assert same_bits(out.view[:, :C].cpu(), x.to(BF)), f"cast_f32_to_bf16 R={R} C={C} Cpad={cpad} off={off} != torch's round-to-nearest-even"
        assert bool((bits(out.view[:, C:]) == 0).all()), "padding columns must be +0"
    for n, off in ((64, 0), (67, 0), (5, 0), (24, 1), (BIG_N + 3, 0)):
        xb = cast_values(n, n).to(BF)
        xin, out = Guard(1, n, BF, init=xb[None], lead=8, off=off), Guard(1, n, F32, lead=8, off=off)
        call_guarded("cast_bf16_to_f32", (xin, out, n), (out,), f"n={n} off={off}")
        assert same_bits(out.view[0].cpu(), xb.float()), f"cast_bf16_to_f32 n={n} off={off}"
    for R2, C, with_bias in BIAS_CAST_CASES:
        x, bias = bias_cast_inputs(R2, C)
        xin, out = Guard(R2, C, F32, init=x, lead=4), Guard(R2, C, BF, lead=4)
        call_guarded("f32_bias_to_bf16", (xin, d(bias) if with_bias else None, out, R2, C), (out, xin), f"R={R2} C={C}")
        assert bool((bits(xin.view) == 0).all()), "f32_bias_to_bf16 re-zeroes its input"
        ref = x.double() + (bias.double() if with_bias else 0)
        check("gpu", "bias_cast", out.view, ref, x.double().abs() + (bias.double().abs() if with_bias else 0), 0, f"f32_bias_to_bf16 R={R2} C={C} bias={with_bias}")
        if not with_bias:
            assert same_bits(out.view.cpu(), x.to(BF))


@pytest.mark.gpu
@pytest.mark.parametrize("R,V,ld", LP_CASES)
def test_gpu_logprob_and_dlogits_rows(R, V, ld):
    """logprob_rows on N(0,3), offset, peaked and -inf-masked rows (ids 0..3 masked: the row that gave NaN before the kernel skipped dead groups); dlogits_rows where V % 8 == 0"""
    buf, tgt = lp_inputs(R, V, ld)
    lse, logp, El, Ep = lp_math(buf, V, tgt, False)
    xg = Guard(R, V, F32, ld, buf[:, :V])
    lg, sg = vec(R, F32), vec(R, F32)
    call_guarded("logprob_rows", (xg, ld, d(tgt), lg, sg, R, V), (lg, sg), f"R={R} V={V}")
    xg.untouched("logits")
    check("gpu", "lp.lse", sg.view[0], lse, El, V, f"lse R={R} V={V}", En=torch.ones_like(El))
    check("gpu", "lp.logp", lg.view[0], logp, Ep, V, f"logp R={R} V={V}", En=torch.ones_like(El))
    bad = (tgt < 0) | (tgt >= V)
    assert bool((lg.view[0].cpu()[bad] == 0).all()), "ignored rows give logp = 0"
    lo, _ = ops.logprob_rows(xg.view, d(tgt), want_lse=False)
    assert same_bits(lo, lg.view[0].contiguous()), "lse = NULL must not change logp"
    if V % 8 == 0:
        gvec = torch.randn(R, generator=gen(R)).to(F32) * 2
        gvec[tgt < 0] = 0
        ref, E = dlogits_math(buf, V, tgt, lse.to(F32), gvec, False)
        ldd = V + 8
        dl = Guard(R, V, BF, ldd)
        call_guarded("dlogits_rows", (xg, ld, d(tgt), d(lse.to(F32)), d(gvec), dl, ldd, R, V), (dl,), f"R={R} V={V}")
        check("gpu", "dlogits", dl.view, ref, E, 0, f"dlogits R={R} V={V}")
        assert bool((dl.view.cpu()[tgt < 0] == 0).all()), "g = 0 rows give zeros"


@pytest.mark.gpu
def test_gpu_dlogits_rows_small_and_stride_loop():
    """V = 8 (one chunk) and V = 131368 (gx capped at 64: the stride loop)"""
    for R, V in DLOGITS_EXTRA:
        x, tgt, gvec, lse32 = dlogits_extra_inputs(R, V)
        ref, E = dlogits_math(x, V, tgt, lse32, gvec, False)
        xg, dl = Guard(R, V, F32, init=x), Guard(R, V, BF, V + 16)
        call_guarded("dlogits_rows", (xg, V, d(tgt), d(lse32), d(gvec), dl, V + 16, R, V), (dl,), f"R={R} V={V}")
        check("gpu", "dlogits", dl.view, ref, E, 0, f"dlogits R={R} V={V}")


@pytest.mark.gpu
@pytest.mark.parametrize("N,C", GRPO_CASES)
def test_gpu_grpo_loss(N, C):
    """grpo_loss (kl and kl = NULL) and, at C = 300, grpo_loss_is at both levels; a row with an all-zero mask gives zeros, no NaN"""
    I = grpo_inputs(N, C)
    lp, rf, adv, mask = (Guard(N, C, F32, init=I["logp"]), Guard(N, C, F32, init=I["ref"]), vec(N, F32, I["adv"]), Guard(N, C, torch.int32, init=I["mask"]))
    for level in ((None, 0, 1) if C == 300 else (None,)):
        ref = grpo_math(I, False, level=level)
        for with_kl in (True, False):
            dl, kl, rl, rk = Guard(N, C, F32), Guard(N, C, F32), vec(N, F32), vec(N, F32)
            if level is None:
                call_guarded("grpo_loss", (lp, rf, adv, mask, I["beta"], I["nt"], dl, kl if with_kl else None, rl, rk, N, C), (dl, kl, rl, rk), f"N={N} C={C}")
            else:
                w, st = Guard(N, C, F32), Guard(N, 5, F32)
                call_guarded("grpo_loss_is", (lp, rf, d(I["rollout"]), adv, mask, I["beta"], I["cap"], level, I["nt"], dl, kl if with_kl else None, rl, rk, w, st, N, C),
                             (dl, kl, rl, rk, w, st), f"N={N} C={C} level={level}")
            if with_kl:
                check("gpu", "grpo.kl", kl.view, ref["kl"], ref["E_kl"], 0, f"kl N={N} C={C}")
            else:
                kl.untouched("kl = NULL")
            check("gpu", "grpo.dlogp", dl.view, ref["dlogp"], ref["E_dlogp"], 0, f"dlogp N={N} C={C} level={level}")
            check("gpu", "grpo.row", rl.view[0], ref["row_loss"], ref["E_row_loss"], C, f"row_loss N={N} C={C} level={level}")
            check("gpu", "grpo.row", rk.view[0], ref["row_kl"], ref["E_row_kl"], C, f"row_kl N={N} C={C} level={level}")
            if N > 1:
                assert float(rl.view[0][1]) == 0 and float(rk.view[0][1]) == 0 and bool((dl.view[1] == 0).all()), "all-zero mask: zeros, no NaN"
    for g in (lp, rf, adv, mask):
        g.untouched("grpo inputs")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", SUMSQ_KINDS)
@pytest.mark.parametrize("n", SUMSQ_N)
def test_gpu_sumsq(n, kind):
    """sumsq on N(0,1) (every element counts: a dropped loop trip or tail is far outside the bound) and on the mixed-magnitude gradient; twice for run-to-run bits"""
    x = sumsq_inputs(n, kind)
    ref = sumsq_math(x, False)
    xg = Guard(1, n, F32, ld=n + (-n) % 4, init=x[None])
    outs = []
    for rep in range(2):
        part, out = vec(2048, F32), vec(1, F32)
        call_guarded("sumsq", (xg, n, part, out), (part, out), f"n={n}")
        outs.append(out.view[0].clone())
    xg.untouched("g")
    assert same_bits(outs[0], outs[1]), "sumsq: two runs differ in bits"
    check("gpu", "sumsq", outs[0][0], ref, ref, sumsq_chain(n), f"n={n} {kind}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ADAM_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_gpu_adamw_flat(case):
    """adamw_flat against the float64 AdamW recurrence with the fp32-rounded hyper-parameters; param_bf16 == bf16(master) and the gradient zeroed, exactly"""
    n, step, wd_, gs, clip = case
    ref = adam_math(*case, False)
    w, m, v, g = adam_inputs(n, step)
    n4 = n + (-n) % 4
    G = lambda t, dt=F32: Guard(1, n, dt, ld=n4 if dt == F32 else n + (-n) % 8, init=t[None])
    wg, mg, vg, gg, pg = G(w), G(m), G(v), G(g), Guard(1, n, BF, ld=n + (-n) % 8)
    norm2 = d(ref["norm2"].reshape(1)) if ref["norm2"] is not None else None
    call_guarded("adamw_flat", (wg, mg, vg, gg, pg, n, LR, B1, B2, AEPS, wd_, step, gs, norm2, ref["max_norm"]), (wg, mg, vg, gg, pg), f"{case}")
    for k, gd in (("m", mg), ("v", vg), ("master", wg)):
        check("gpu", "adam." + k, gd.view[0], ref[k], ref["E_" + k], 0, f"adamw {k} {case}")
    assert same_bits(pg.view[0], wg.view[0].to(BF)), "param_bf16 != bf16(master)"
    assert bool((bits(gg.view) == 0).all()), "the gradient is zeroed after use"


@pytest.mark.gpu
def test_gpu_rope_table():
    for B in (1, 37):
        for half in (64, 40):
            pos = np.array([ROPE_POS[i % 5] for i in range(B)], dtype=np.int32)
            c64, s64, host = rope_table_ref(pos, half)
            cs, sn = Guard(B, half, F32), Guard(B, half, F32)
            call_guarded("rope_table", (torch.from_numpy(pos).to(DEV), torch.from_numpy(inv_freq_of(half)).to(DEV), cs, sn, B, half), (cs, sn), f"B={B} half={half}")
            err = max(np.abs(cs.view.cpu().numpy().astype(np.float64) - c64).max(), np.abs(sn.view.cpu().numpy().astype(np.float64) - s64).max()) / 2.0 ** -23
            ROPE_TABLE_ERR[("gpu", half)] = max(ROPE_TABLE_ERR.get(("gpu", half), 0.0), float(err))
            ROPE_TABLE_ERR[("host", half)] = max(ROPE_TABLE_ERR.get(("host", half), 0.0), host)
            print(f"[tokenwise_f64 gpu] rope_table B={B} half={half}: kernel {err:.3f} ulp(1), host libm {host:.3f} ulp(1)")
            assert err <= host + 2.0, f"rope_table B={B} half={half}: {err:.3f} ulp(1) against the host's {host:.3f} + 2"


@pytest.mark.gpu
@pytest.mark.parametrize("B", (1, 37, 256))
@pytest.mark.parametrize("eos", (ADV_EOS, -1))
def test_gpu_decode_advance(B, eos):
    """40 steps of decode_advance against the integer model: tokens, pad after EOS, positions, cache slots across page boundaries through a permuted block table,
    nothing written past column C, all_done, the step counter, and the rotary table == rope_table on the bumped positions"""
    sampled, bt, ctx0, pos0, _ = advance_inputs(B, eos)
    states = advance_model(B, eos)
    half = 40
    inv = torch.from_numpy(inv_freq_of(half)).to(DEV)
    I64, I32 = torch.int64, torch.int32
    cur, out = vec(B, I64), Guard(B, ADV_C, I64)
    pos, ctx, slot, fin = vec(B, I32, torch.from_numpy(pos0)), vec(B, I32, torch.from_numpy(ctx0)), vec(B, I64), vec(B, I32, torch.zeros(B, dtype=I32))
    step, done = vec(1, I32, torch.zeros(1, dtype=I32)), vec(1, I32, torch.full((1,), 5, dtype=I32))
    btg = Guard(B, ADV_PAGES, I32, init=torch.from_numpy(bt))
    cs, sn, cs2, sn2 = Guard(B, half, F32), Guard(B, half, F32), Guard(B, half, F32), Guard(B, half, F32)
    out_model = np.full((B, ADV_C), -777, dtype=np.int64)
    out.view.fill_(-777)
    for st in range(ADV_STEPS):
        use_table = st % 2 == 0 or st > 30
        call_guarded("decode_advance", (d(torch.from_numpy(sampled[st])), cur, out, ADV_C, pos, ctx, slot, btg, ADV_PAGES, fin, step, eos, ADV_PAD, B, done,
                                        inv if use_table else None, cs if use_table else None, sn if use_table else None, half if use_table else 0),
                     (cur, out, pos, ctx, slot, fin, step, done, cs, sn), f"B={B} step={st}")
        S = states[st]
        for name, gd, want in (("cur_tok", cur, S["cur"]), ("pos", pos, S["pos"]), ("ctx_len", ctx, S["ctx"]), ("slot", slot, S["slot"]), ("finished", fin, S["fin"])):
            assert np.array_equal(gd.view[0].cpu().numpy(), want), f"decode_advance B={B} step {st}: {name}"
        assert np.array_equal(out.view.cpu().numpy(), S["out"]), f"decode_advance B={B} step {st}: out_tokens"
        assert int(step.view[0, 0]) == S["step"] and int(done.view[0, 0]) == S["all_done"], f"decode_advance B={B} step {st}: step / all_done"
        if use_table:
            hip.call("rope_table", pos.view, inv, cs2.view, sn2.view, B, half)
            assert same_bits(cs.view, cs2.view) and same_bits(sn.view, sn2.view), f"decode_advance B={B} step {st}: rotary table != rope_table on the bumped positions"
    btg.untouched("block table")


@pytest.mark.gpu
def test_gpu_host_side_refusals():
    """Shapes the launchers refuse on the host: an error through the binding, no launch, outputs untouched"""
    T, H = 4, 64
    x, w = Guard(T, H, BF, init=torch.ones(T, H)), torch.ones(4104, dtype=BF, device=DEV)
    y, rstd, dx, dw = Guard(T, 4104, BF), vec(T, F32), Guard(T, 4104, BF), vec(4104, F32)
    x32 = torch.zeros(2, 257, H, device=DEV)
    outs = (y, rstd)
    refused("rmsnorm_fwd", (x, None, 0, None, None, None, w, y, rstd, T, 4104, 4104, 4104, 4104, EPS32, None), outs, "H = 4104")
    refused("rmsnorm_fwd", (x, None, 0, None, None, None, w, y, rstd, T, 12, 16, 16, 16, EPS32, None), outs, "H = 12")
    refused("rmsnorm_fwd", (x, None, 0, None, None, None, w, y, rstd, T, H, H + 4, H, H, EPS32, None), outs, "ldx % 8")
    refused("rmsnorm_fwd", (x, x32, 2, None, None, None, w, y, rstd, T, H, H, H, H, EPS32, None), outs, "x and x32")
    refused("rmsnorm_fwd", (None, None, 0, None, None, None, w, y, rstd, T, H, H, H, H, EPS32, None), outs, "neither x nor x32")
    refused("rmsnorm_fwd", (None, x32, 2, None, None, None, w, y, rstd, 257, H, H, H, 0, EPS32, None), outs, "ldy == 0 with T = 257")
    refused("rmsnorm_fwd", (None, x32, 0, None, None, None, w, y, rstd, T, H, H, H, H, EPS32, None), outs, "nsplit = 0")
    refused("rmsnorm_bwd", (x, x, w, rstd, None, dx, dw, None, T, H, H), (dx, dw), "dw without workspace")
    refused("rmsnorm_bwd", (x, x, w, rstd, None, dx, None, None, T, 4104, 4104), (dx,), "H = 4104")
    refused("layernorm_fwd", (x, None, None, w, w, y, rstd, rstd, T, 12, 16, 16, 16, EPS32), outs, "H = 12")
    refused("layernorm_fwd", (x, None, None, w, w, y, rstd, rstd, T, H, H, H, H + 2, EPS32), outs, "ldy % 8")
    refused("layernorm_bwd", (x, x, w, rstd, rstd, None, dx, dw, None, None, T, H, H), (dx, dw), "dw without db")
    refused("rope_inplace", (y, 66, rstd, rstd, T, 1, 60, 0), (y,), "D = 60")
    refused("rope_inplace", (y, 130, rstd, rstd, T, 1, 128, 0), (y,), "ld % 4")
    for name in ("gelu", "gelu_tanh", "quick_gelu"):
        refused(name + "_fwd", (x, y, 12), (y,), "n % 8")
        refused(name + "_bwd", (x, x, y, 12), (y,), "n % 8")
        refused(name + "_fwd", (x, y, 0), (y,), "n = 0")
    refused("swiglu_fwd", (x, H, y, 32, T, 28), (y,), "I % 8")
    refused("swiglu_fwd", (x, H + 4, y, 32, T, 32), (y,), "ldg % 8")
    refused("swiglu_bwd", (x, 32, x, H, y, 68, T, 32), (y,), "ldd % 8")
    refused("colsum_acc", (x, H, dw, None, T, H), (dw,), "no workspace")
    refused("colsum_acc", (x, H, dw, rstd, T, 60), (dw,), "N % 8")
    refused("embed_fwd", (rstd, None, x, None, y, T, 12), (y,), "H % 8")
    refused("rows_gather_sum", (x, rstd, rstd, None, y, T, 12), (y,), "H % 8")
    refused("rows_scatter_acc", (x, rstd, rstd, rstd, dw, 0, H), (dw,), "U = 0")
    refused("cast_f32_to_bf16", (dw, 8, y, 8, 2, 8, 4), (y,), "Cpad < C")
    refused("cast_bf16_to_f32", (x, dw, 0), (dw,), "n = 0")
    refused("logprob_rows", (dw, 1290, rstd, rstd, rstd, 1, 1289), (rstd,), "ld % 4")
    refused("dlogits_rows", (dw, 1292, rstd, rstd, rstd, y, 1296, 1, 1289), (y,), "V % 8")
    refused("grpo_loss", (dw, dw, rstd, rstd, 0.04, 1, dw, None, rstd, rstd, 2, 8), (dw, rstd), "n_total_rows < N")
    refused("sumsq", (dw, 0, dw, rstd), (rstd,), "n = 0")
    refused("sumsq", (dw, 8, None, rstd), (rstd,), "no scratch")
    refused("adamw_flat", (dw, dw, dw, dw, y, 8, LR, B1, B2, AEPS, 0.0, 0, 1.0, None, 0.0), (dw, y), "step = 0")
    refused("rope_table", (rstd, rstd, dw, dw, 0, 4), (dw,), "B = 0")
    refused("decode_advance", (rstd,) * 3 + (4,) + (rstd,) * 4 + (2, rstd, rstd, 1, 0, 257, None, None, None, None, 0), (rstd,), "B = 257")
    refused("decode_advance", (rstd,) * 3 + (4,) + (rstd,) * 4 + (2, rstd, rstd, 1, 0, 4, None, rstd, None, None, 0), (rstd,), "inv_freq without tables")
    with pytest.raises(AssertionError):
        ops.rmsnorm_bwd(x.view, x.view[:, :32], w[:H], rstd.view[0])
    x.untouched("x")


@pytest.mark.gpu
def test_gpu_used_fractions_record():
    """prints the largest used fraction of every bound over the GPU tests above (run after them: it reads what they recorded)"""
    _print_used("gpu")
    assert all(v <= 1.0 for v in USED["gpu"].values())
    if len(USED["gpu"]) > len(BOUNDS) // 2:         # the whole GPU part ran: every bound of the table was put to use
        assert set(USED["gpu"]) == set(BOUNDS), sorted(set(BOUNDS) - set(USED["gpu"]))
    for k, v in sorted(ROPE_TABLE_ERR.items()):
        print(f"[tokenwise_f64 gpu] rope_table error, {k[0]} half={k[1]}: {v:.3f} ulp(1)")
