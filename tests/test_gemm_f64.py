"""The training GEMMs and the fused lm_head of csrc/gemm.hip against float64: iadr1_gemm_nt_bf16 (both kernels, out_mode 0 / 1 / 2, bias, GELU), iadr1_gemm_nt_splitk_acc_bf16,
iadr1_gemm_tn_acc_bf16 (un-split and split), iadr1_gemm_swiglu_bf16 (GU stored and NULL), iadr1_gemm_swiglu_rows_bf16, iadr1_linear_logprob_fwd and iadr1_linear_logprob_dlogits.
csrc/skinny.hip (the decode GEMMs and their packers) has its own file, test_skinny_f64.py.  The structure and the helpers (Guard, frac, bfr, same_bits, ...) are those of test_tokenwise_f64.py.

THE BOUND.  Every output element is held to   |got - ref64| <= 2^-8 c |ref64| + 2^-24 (f0 E + fn n E) + 1e-30   (no element is exempt).  ref64 is the operation in float64 on the
same bf16-rounded inputs with NO intermediate rounding, E the same formula with the absolute value of every term, E = sum_k |a| |b| + |bias| + |C0|, and n = K.
  contraction (x)   Products of two bf16 values are exact in fp32.  The sum runs inside the matrix core (32 products per MFMA), then over the K tiles in the accumulator, for
             split-K over the slices and last onto the old C: K + (a few) additions.  The rounding of the MFMA's internal adder is not documented in what this project has to go by,
             so fn = 2: at most ONE fp32 ulp (2^-23 = 2 x 2^-24) per addition, any order, any rounding direction (fn = 1 would assume round-to-nearest).  f0 = 4: the bias add and
             the old-C add, two roundings of up to one ulp each.  b_x = 2^-24 (4 + 2 K) E.  Every input is zero or in the NORMAL bf16 range (asserted by the input makers):
             what the matrix core does with subnormals is likewise undocumented.
  gemm.f32   c 0: fp32 store / accumulate, bound b_x.          gemm.bf16  c 2: the store plus one spare as in the two sister files, + b_x.
  gemm.gelu  the pre-activation's b_x passes through |gelu'| <= 1.13, plus f0 = F_LIBM + 4 on E = 0.5 |x| (1 + |erf|) (the token-wise gelu.fwd entry); c 2 for bf16, c 0 for fp32.
  swiglu.gu  the stored gate|up matrix: gemm.bf16.
  swiglu.a   the token-wise entry (c 3, F_EXP, E = |ref|) against float64 SwiGLU of the kernel's OWN stored GU (bit-known inputs); also bit-equal to iadr1_swiglu_fwd on that GU, equal
             to the one correct bit pattern where swiglu_exact() says there is only one, and with GU == NULL bit-equal to the GU-storing call's a.
  lp.lse     sum_j p_j b_x(j), the softmax-weighted bound of the row's logits (d lse / d x_j = p_j), plus the token-wise lp.lse term 2^-24 (8 (|m| + |log s| + |lse| + 1) + V).
  lp.logp    the lse bound + b_x(target) + 8 x 2^-24 |x_target|; an ignored row (target < 0 or >= V) must give exactly 0.
  lp.dlogits c 2, f0 = F_EXP on E = |g| (onehot + p), plus |g| p_j (b_x(j) + b_lse): the logit's and the lse's error pass through exp.  Its lse input is the float64 lse rounded to fp32.
No bound above was changed after the first GPU run.

EQUALITIES, bit for bit.  (1) One-hot rows: some rows of A are v e_k (v = 1, then v = -2) and some rows of B are e_k, k over the first and last element of every 8-element chunk
of the first and the last K tile and over the whole ragged tail (hot_ks).  Whatever the matrix core's adder does, a sum with ONE nonzero product is that product: output row m must
be v x column k of B and output column n column k of A -- after the fp32 bias / old-C add and the bf16 store, which IEEE fixes -- in fp32 and in bf16.  This pins every swizzled
16-byte chunk and every transpose-read lane to its source without a tolerance (the sign of a zero apart: 0 + -0 depends on the adder's rounding direction; not asserted under GELU:
erff is not bit-specified).  (2) Everything around every output holds its
sentinel: lead and trail rows, the columns N .. ldc, for the rows form the arena rows between the blocks; inputs are unchanged.  (3) Run-to-run bits of split-K and
linear_logprob_fwd.  (4) The split-K result does not depend on what the workspace held (sentinels, then 2^12).  (5) logp == 0.0 on ignored rows; dlogits rows with g == 0 are zero.
(6) TN == NT on transposed copies (K padded to 8 with zeros: exact), swiglu_rows == the plain launch on the gathered rows.

INPUTS.  A is N(0,1), B 0.5 N(0,1), bias 2 N(0,1), the old C 5 N(0,1).  Every input lies in a Guard: the columns K .. lda (lda = K + 8 for A, K + 16 for B), the rows around the
operand (for TN: the rows past K of dY and X) and the arena rows between row blocks hold a finite poison (the sentinel, -700 .. -728; 2^12 in the arena gaps); a chunk, row or column read
from there moves the result by >= 10^5 bounds.  One case per output type has C misaligned by one element with an ldc that is no multiple of 8 (bf16) / 4 (fp32): the scalar
stores of both kernels.  linear_logprob: the last vocabulary row is 0.6 x the h of the `needle` rows, so its softmax weight there is >= 0.02 (asserted) and a clamped duplicate of it
counted in the ragged slice moves lse; `flat` rows (h 2^-6 N(0,1)) have lse ~ log V, where an exp(0) from an empty slice shows; on `hot` rows one 64-column slice lies about 40
above every other one (slice 65 at V = 4360: the SECOND part of lane 1 of the combine kernel has the larger maximum); targets sit at column 0, V - 1, the first and last column
of a wave slice and in the ragged slice; -100 and V are the ignored ones; some rows of H are one-hot (their E, and so their bound, is one product).

WHICH CASE REACHES WHICH BRANCH
  gemm_nt, 128^2 kernel (M < 512 or N < 512 or < 192 tiles of 256^2)   test_gpu_gemm_nt_128[M-N-K]: (1, 8) one block, every row and column clamped; (130, 136) and (257, 264) interior
             tiles (vector stores; the fp32 interior fast path with its two-row-group accumulate) + ragged tiles whose 8- / 4-column groups are whole; (100, 131) N odd: the scalar
             tails of the bf16 and the fp32 epilogues (and, with ldc = 132 + 4, vec_ok on the groups before them).  K 8 / 64 -> nk 1 (one chunk / a full tile), 72 -> nk 2 with a
             one-chunk tail, 136 -> nk 3 (odd: both buffers, last tile in buffer 0).  Variants: out_mode 0, 1, 2; bf16 + bias; bf16 + bias + GELU; fp32 + bias + GELU at (130, 136, 8).
             test_gpu_gemm_nt_misaligned: C + 1 element, ldc = N + 3 -> vec_ok false in both kernels, every store scalar (bf16, fp32, fp32 accumulate).
  gemm_nt, 256^2 kernel   test_gpu_gemm_nt_256[M-N-K]: (2824, 3912) 12 x 16 tiles, last tile row 8 rows, last tile column: wave 0 interior, wave 1 8 columns, waves 2 and 3 empty;
             (3072, 3846) N % 8 = 6: scalar tails (bf16 8-groups, fp32 4-groups).  K 8 -> nk 1 (the vmcnt(0) prologue), 72 -> nk 2 (more1 only), 136 -> nk 3 (more2 once, odd),
             264 -> nk 5 (steady state, odd; nk even is the split-K slice of 128 below).  bias, bias + GELU (bf16 and fp32) at K 72.
  split-K    test_gpu_gemm_nt_splitk[M-N-K-ks]: (264, 264), (520, 260) x (136, 2) kslice 128, last slice ONE chunk; (200, 2) last slice 72; (264, 3) last slice one chunk, slices of
             nk 2 (even); (1032, 4) kslice 320 (nk 5), last slice 72.  Ragged partial tiles in the workspace (ldc = N), the reduce kernel, old C.  Refusals: (200, 3), (264, 4) empty slice;
             ksplit 1; N % 4.
  TN         test_gpu_gemm_tn[M-N-K-ks]: (256, 256) one interior tile; (264, 520), (520, 264): the min(col, M - 8) / (col, N - 8) clamps, the 8-row / 8-column last tiles, the two 32-column
             runs per wave (coln).  K 1, 7 (a tile of 1 / 7 rows: chunk_k is a ROW here), 64, 65, 129 (nk 2, 3 with a one-row last tile), 200 un-split (the accumulate form);
             (136, 2), (264, 3) split (the OUT_F32 form into the workspace + reduce).  Refusals: M < 256, M % 8.
  SwiGLU     test_gpu_gemm_swiglu[M-I-K]: (256, 128) one block, (512, 384) 2 x 3 blocks (the h * I + n0 / 2 gate / up row map across tiles); K 8, 72, 136 -> nk 1, 2, 3; GU stored (ldgu = 2 I + 8)
             and NULL.  test_gpu_gemm_swiglu_rows: M 256 (16, 40), (64, 64); M 512 (256, 300).  Refusals: M % 256, I % 128, block 24.
  linear_logprob   test_gpu_linear_logprob[M-V-K]: (5, 258, 72) two tiles, in the last one wave 0 is ragged (2 columns) and waves 1 - 3 are EMPTY (max -inf, sum 0); (261, 1001, 136) two row
             tiles, ragged slice of 41; (130, 4360, 64) 72 parts per row: the combine kernel's second loop trip, the ragged slice of 8 and three empty ones; (1, 8, 8); (300, 4096, 264)
             every slice `full`, 64 parts.  dlogits on the same shapes with ldd = roundup(V, 8) (16-byte stores + the ragged 8-group's scalar tail) and, at V = 1001, ldd = V odd (every
             store scalar: the launcher takes any ldd >= V, which is what the header now says).

THE CPU PART proves the sensitivity of the GPU part.  A torch emulation of the kernels' arithmetic -- each 32-deep k-step summed exactly (float64) and rounded to fp32, fp32
accumulation over the k-steps in kernel order, split-K slices summed in slice order and then onto C, bf16 at the stores, the per-slice (max, sum) merged in the combine kernel's order --
stays inside every bound on every input set the GPU part uses (the two 256^2 shapes at K = 72 only).  It is not claimed bit-equal to the hardware.  Every fault model of FAULT_MODELS,
applied to the float64 reference on the same inputs, leaves its bound by >= FAULT_FACTOR at its designated elements (the largest element of each designated row; background rows
unless stated), except `swiglu_unrounded`, which an equality catches as in the token-wise file.  Designated at part of the cases only: gelu_tanh at K = 8 (tanh and erf GELU differ
by <= 5e-4, which b_x reaches from K ~ 64 on); lse_empty_slice_exp0 at V = 258 and V = 8 (at V = 4360 three extra exp(0) are 7e-4 of s, within the V 2^-24 summation term)."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iadr1_amd  # noqa: E402,F401
from iadr1_amd import hip  # noqa: E402
from test_tokenwise_f64 import (BF, DEV, F32, F64, F_EXP, F_LIBM, FAULT_FACTOR, INF, TINY, U8, U24, Guard, bfr, bits, call_guarded, d, frac, gen, refused,  # noqa: E402
                                same_bits, swiglu_exact, swiglu_math, vec, workspace)

F0, FN = 4, 2
GELU_SLOPE = 1.13
POISON = 700.0            # the smallest magnitude of the sentinel that fills the padding of every operand
USED = {"emu": {}, "gpu": {}}
FAULT_SEEN = {}
FAULT_MODELS = ["ktail_dropped", "ktail_past_K", "ktile_skipped_nk2", "ktile_skipped_nk3", "swizzle_off_by_one_a", "swizzle_off_by_one_b", "row_clamp_m2", "tn_row_past_K", "tn_col_clamp", "tn_wave_colmap_nt",
                "bias_tile_local", "bias_dropped_ragged", "gelu_tanh", "acc_overwrites", "acc_twice_scalar_tail",
                "splitk_slice_dropped", "splitk_last_slice_kslice", "splitk_reduce_ignores_c",
                "swiglu_gate_up_swapped", "swiglu_unrounded", "swiglu_rows_stride_is_block",
                "lse_cols_ge_V", "lse_empty_slice_exp0", "lse_combine_stops_64", "lse_combine_no_rescale", "logp_target_minus_1", "logp_ignored_not_zeroed",
                "dlogits_onehot_tile_local", "dlogits_lse_clamped_row"]


# ======================================================================================================================================================
# bounds, checks
# ======================================================================================================================================================

def ratio(got, ref, bound):
    r = (got.double() - ref).abs() / bound
    return torch.where(torch.isnan(r), torch.full_like(r, INF), r)


def gcheck(side, key, got, ref, bound, what):
    """Asserts the bound on every element; records the largest used fraction under USED[side][key]."""
    assert tuple(got.shape) == tuple(ref.shape), (what, got.shape, ref.shape)
    r = ratio(got, ref, bound)
    mx = float(r.max())
    USED[side][key] = max(USED[side].get(key, 0.0), mx)
    if mx > 1.0:
        flat = r.reshape(-1)
        top = torch.topk(flat, min(6, flat.numel())).indices.tolist()
        g, f = got.double().reshape(-1), ref.reshape(-1)
        cols = r.shape[-1]
        lines = [f"element ({i // cols}, {i % cols}): got {float(g[i]):.9g} ref {float(f[i]):.9g} = {float(flat[i]):.3g} x bound" for i in top]
        raise AssertionError(f"{what} [{key}]: {int((flat > 1).sum())} of {flat.numel()} elements beyond the bound\n  " + "\n  ".join(lines))
    return mx


def excess(fault, bad, ref, bound, rows=None, cols=None):
    """Smallest excess (x bound) of the faulty reference over its designated rows (the largest element of each, over the designated columns)."""
    r = ratio(bad, ref, bound)
    if r.dim() == 1:
        r = r[:, None]
    if cols is not None:
        r = r[:, cols]
    if rows is not None:
        r = r[rows]
    assert r.numel() > 0, fault
    ex = float(r.reshape(r.shape[0], -1).amax(-1).min())
    assert ex >= FAULT_FACTOR, f"fault '{fault}' moves the output by only {ex:.3g} x the bound at its designated elements"
    FAULT_SEEN[fault] = min(FAULT_SEEN.get(fault, INF), ex)
    return ex


def gelu64(x, tanh=False):
    if tanh:
        return 0.5 * x * (1 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1 + torch.erf(x * 0.7071067811865476))


def b_x(Ex, K):
    return U24 * (F0 + FN * K) * Ex


def normal_range(t):
    a = t.float().abs()
    return bool(((a == 0) | ((a >= 2.0 ** -126) & (a < 2.0 ** 127))).all())


# ======================================================================================================================================================
# dense contractions: inputs, float64 reference, emulation, fault models
# ======================================================================================================================================================

def hot_ks(K):
    """first and last element of every 8-element chunk of the first and the last K tile, and the whole ragged tail; the tail first"""
    nk = (K + 63) // 64
    ks = set(range((K // 64) * 64, K))
    for t0 in (0, (nk - 1) * 64):
        ks.update(k for k in range(t0, min(t0 + 64, K)) if k % 8 in (0, 7))
    return sorted(ks, reverse=True)


@functools.lru_cache(maxsize=None)
def mm_inputs(M, N, K):
    """logical A [M, K], B [N, K] (TN stores their transposes), bias [N], old C [M, N]; the one-hot rows of A (never the last two: the clamp model's) and of B"""
    g = gen(M * 7919 + N * 31 + K)
    A, B = torch.randn(M, K, generator=g).to(BF), (0.5 * torch.randn(N, K, generator=g)).to(BF)
    ks = hot_ks(K)
    na, nb = min(2 * len(ks), M // 2), min(len(ks), N // 2)
    arows, brows = torch.randperm(max(M - 2, 0), generator=g)[:na].tolist(), torch.randperm(max(N - 2, 0), generator=g)[:nb].tolist()
    ak, av = [ks[i % len(ks)] for i in range(na)], [1.0 if i < len(ks) else -2.0 for i in range(na)]
    bk = [ks[i % len(ks)] for i in range(nb)]
    for r, k, v in zip(arows, ak, av):
        A[r] = 0
        A[r, k] = v
    for r, k in zip(brows, bk):
        B[r] = 0
        B[r, k] = 1
    bias, C0 = (2 * torch.randn(N, generator=g)).to(BF), (5 * torch.randn(M, N, generator=g)).to(F32)
    assert normal_range(A) and normal_range(B) and normal_range(bias) and normal_range(C0)
    bg = torch.ones(M, dtype=torch.bool)
    bg[arows] = False
    return {"M": M, "N": N, "K": K, "A": A, "B": B, "bias": bias, "C0": C0, "arows": arows, "ak": ak, "av": av, "brows": brows, "bk": bk, "bg": bg.nonzero()[:, 0]}


def contract64(A, B):
    return A.double() @ B.double().t()


def mm_ref(I, dev="cpu"):
    """(x, Ex): the float64 contraction and its absolute-value form"""
    A, B = I["A"].to(dev).double(), I["B"].to(dev).double()
    return A @ B.t(), A.abs() @ B.abs().t()


def epilogue64(x, I, mode, use_bias, act, dev="cpu", fault=None, T=128):
    """float64 output of gemm_nt's epilogue from the float64 contraction x (faults: the epilogue models)"""
    N = x.shape[1]
    pre = x
    if use_bias:
        b = I["bias"].to(dev).double()
        if fault == "bias_tile_local":
            b = b[torch.arange(N, device=b.device) % T]
        elif fault == "bias_dropped_ragged":
            b = b.clone()
            b[(N // T) * T:] = 0
        pre = pre + b
    if act:
        pre = gelu64(pre, tanh=(fault == "gelu_tanh"))
    if mode == 2:
        C0 = I["C0"].to(dev).double()
        if fault in ("acc_overwrites", "splitk_reduce_ignores_c"):
            return pre
        out = pre + C0
        if fault == "acc_twice_scalar_tail":
            out[:, N - N % 4:] += pre[:, N - N % 4:]
        return out
    return pre


def out_bound(x, Ex, I, mode, use_bias, act, dev="cpu"):
    """(ref64, bound) of one gemm_nt variant"""
    K = I["K"]
    E = Ex + (I["bias"].to(dev).double().abs() if use_bias else 0) + (I["C0"].to(dev).double().abs() if mode == 2 else 0)
    ref = epilogue64(x, I, mode, use_bias, act, dev)
    b = b_x(E, K)
    if act:
        pre = x + (I["bias"].to(dev).double() if use_bias else 0)
        b = GELU_SLOPE * b + U24 * (F_LIBM + 4) * 0.5 * pre.abs() * (1 + torch.erf(pre * 0.7071067811865476).abs())
    if mode == 0:
        b = b + U8 * 2 * ref.abs()
    return ref, b + TINY


def out_key(mode, act):
    return "gemm.gelu" if act else ("gemm.bf16" if mode == 0 else "gemm.f32")


def emu_contract(A, B, k0=0, k1=None):
    """fp32 accumulator of the kernels: every 32-deep k-step (one MFMA) summed exactly and rounded to fp32, the steps added in k order"""
    k1 = A.shape[1] if k1 is None else k1
    acc = torch.zeros(A.shape[0], B.shape[0], dtype=F32, device=A.device)
    for s in range(k0, k1, 32):
        e = min(s + 32, k1)
        acc = acc + (A[:, s:e].double() @ B[:, s:e].double().t()).to(F32)
    return acc


def emu_splitk(A, B, ksplit):
    K = A.shape[1]
    kslice = ((K + ksplit - 1) // ksplit + 63) // 64 * 64
    a = None
    for z in range(ksplit):
        p = emu_contract(A, B, z * kslice, min(K, (z + 1) * kslice))
        a = p if a is None else a + p
    return a


def emu_epilogue(acc, I, mode, use_bias, act):
    v = acc
    if use_bias:
        v = v + I["bias"].to(F32)
    if act:
        v = 0.5 * v * (1 + torch.erf(v * 0.70710678118654752440))
    if mode == 2:
        v = I["C0"] + v
    return v.to(BF) if mode == 0 else v


def operand_fault(name, I, x):
    """float64 contraction under an operand-read fault model (None: the model does not apply to this K)"""
    A, B, K = I["A"].double(), I["B"].double(), I["K"]
    nk = (K + 63) // 64
    if name == "ktail_dropped":
        A = A.clone()
        A[:, K - 8:] = 0
    elif name == "ktail_past_K":
        return x + 8 * POISON * POISON
    elif name in ("ktile_skipped_nk2", "ktile_skipped_nk3"):
        if nk != int(name[-1]):
            return None
        A = A.clone()
        A[:, 64:128] = 0
    elif name in ("swizzle_off_by_one_a", "swizzle_off_by_one_b"):          # slot c of every K tile of A (of B) holds chunk c + 1 (mod 8); chunks at or past K read the zeros
        S = A if name[-1] == "a" else B
        Sp = torch.zeros(S.shape[0], nk * 64, dtype=F64)
        Sp[:, :K] = S
        Sp = Sp.view(-1, nk, 8, 8).roll(-1, 2).reshape(-1, nk * 64)[:, :K]
        A, B = (Sp, B) if name[-1] == "a" else (A, Sp)
    elif name == "row_clamp_m2":
        if I["M"] < 2:
            return None
        x = x.clone()
        x[-1] = x[-2]
        return x
    return A @ B.t()


def onehot_expected(I, mode, use_bias, dev):
    """[(index, expected)]: the output rows of A's one-hot rows and the output columns of B's, as IEEE fixes them (fp32 bias / old-C add, bf16 store)"""
    A, B, bias, C0 = I["A"].to(dev).float(), I["B"].to(dev).float(), I["bias"].to(dev).float(), I["C0"].to(dev)
    ar, br = torch.tensor(I["arows"], dtype=torch.long, device=dev), torch.tensor(I["brows"], dtype=torch.long, device=dev)
    out = []
    if len(ar):
        xr = torch.tensor(I["av"], device=dev)[:, None] * B[:, I["ak"]].t()          # [na, N]
        out.append(((ar, slice(None)), xr, bias[None, :], C0[ar]))
    if len(br):
        xc = A[:, I["bk"]]                                                           # [M, nb]
        out.append(((slice(None), br), xc, bias[None, br], C0[:, br]))
    res = []
    for idx, x, b, c0 in out:
        v = x + b if use_bias else x
        if mode == 2:
            v = c0 + v
        res.append((idx, v.to(BF) if mode == 0 else v))
    return res


def check_onehots(I, got, mode, use_bias, what):
    for idx, want in onehot_expected(I, mode, use_bias, got.device):
        assert got.dtype == want.dtype and torch.equal(got[idx], want), f"{what}: an output row / column of a one-hot operand row is not the other operand's column, bit for bit"


NT128_CASES = [(M, N, K) for (M, N) in ((1, 8), (130, 136), (100, 131), (257, 264)) for K in (8, 64, 72, 136)]
NT256_CASES = [(M, N, K) for (M, N) in ((2824, 3912), (3072, 3846)) for K in (8, 72, 136, 264)]
VARIANTS = [(0, False, 0), (1, False, 0), (2, False, 0), (0, True, 0), (0, True, 1)]          # (out_mode, bias, act)
GELU32_CASE = (130, 136, 8)
SPLITK_CASES = [(M, N, K, ks) for (M, N) in ((264, 264), (520, 260)) for (K, ks) in ((136, 2), (200, 2), (264, 3), (1032, 4))]
TN_CASES = [(M, N, K, 1) for (M, N) in ((256, 256), (264, 520), (520, 264)) for K in (1, 7, 64, 65, 129, 200)] + \
           [(M, N, K, ks) for (M, N) in ((256, 256), (264, 520), (520, 264)) for (K, ks) in ((136, 2), (264, 3))]
SWIGLU_CASES = [(M, I, K) for (M, I) in ((256, 128), (512, 384)) for K in (8, 72, 136)]
SWIGLU_ROWS = [(256, 16, 40), (256, 64, 64), (512, 256, 300)]          # (M, block, block_stride), at I = 128, K = 72


def variants_of(M, N, K, big):
    v = list(VARIANTS) if (not big or K == 72) else VARIANTS[:3]
    if (M, N, K) == GELU32_CASE or (big and K == 72):
        v.append((1, True, 1))
    return v


def cpu_nt_case(M, N, K, T):
    I = mm_inputs(M, N, K)
    x, Ex = mm_ref(I)
    acc = emu_contract(I["A"], I["B"])
    bg, N4 = I["bg"], N - N % 4
    for mode, use_bias, act in variants_of(M, N, K, T == 256):
        what = f"M={M} N={N} K={K} mode={mode} bias={use_bias} act={act}"
        ref, bound = out_bound(x, Ex, I, mode, use_bias, act)
        emu = emu_epilogue(acc, I, mode, use_bias, act)
        gcheck("emu", out_key(mode, act), emu, ref, bound, what)
        if not act:
            check_onehots(I, emu, mode, use_bias, what + " (emulation)")
        if not use_bias:          # operand-read models on the three plain variants
            for f in ("ktail_dropped", "ktail_past_K", "ktile_skipped_nk2", "ktile_skipped_nk3", "swizzle_off_by_one_a", "swizzle_off_by_one_b", "row_clamp_m2"):
                if T == 256 and f not in ("ktile_skipped_nk2", "row_clamp_m2"):
                    continue          # the big shapes run on the CPU at K = 72 only: the models that depend on the tile
                xf = operand_fault(f, I, x)
                if xf is not None:
                    excess(f, epilogue64(xf, I, mode, False, 0), ref, bound, rows=[M - 1] if f == "row_clamp_m2" else bg)
        if use_bias and not act:
            if N > T:
                excess("bias_tile_local", epilogue64(x, I, mode, True, 0, fault="bias_tile_local", T=T), ref, bound, rows=bg, cols=slice(T, None))
            if N % T:
                excess("bias_dropped_ragged", epilogue64(x, I, mode, True, 0, fault="bias_dropped_ragged", T=T), ref, bound, rows=bg, cols=slice((N // T) * T, None))
        if act and mode == 1 and K == 8:
            excess("gelu_tanh", epilogue64(x, I, mode, use_bias, 1, fault="gelu_tanh"), ref, bound, rows=bg)
        if mode == 2:
            excess("acc_overwrites", epilogue64(x, I, 2, False, 0, fault="acc_overwrites"), ref, bound, rows=bg)
            if N % 4:
                excess("acc_twice_scalar_tail", epilogue64(x, I, 2, False, 0, fault="acc_twice_scalar_tail"), ref, bound, rows=bg, cols=slice(N4, None))


@pytest.mark.parametrize("M,N,K", NT128_CASES)
def test_cpu_gemm_nt_128_emulation_inside_and_faults_outside(M, N, K):
    cpu_nt_case(M, N, K, 128)


@pytest.mark.parametrize("M,N", [(2824, 3912), (3072, 3846)])
def test_cpu_gemm_nt_256_emulation_inside_and_faults_outside(M, N):
    cpu_nt_case(M, N, 72, 256)


@pytest.mark.parametrize("M,N,K,ks", SPLITK_CASES)
def test_cpu_splitk_emulation_inside_and_faults_outside(M, N, K, ks):
    I = mm_inputs(M, N, K)
    x, Ex = mm_ref(I)
    ref, bound = out_bound(x, Ex, I, 2, False, 0)
    emu = I["C0"] + emu_splitk(I["A"], I["B"], ks)
    gcheck("emu", "gemm.f32", emu, ref, bound, f"split-K M={M} N={N} K={K} ks={ks}")
    check_onehots(I, emu, 2, False, "split-K (emulation)")
    kslice = ((K + ks - 1) // ks + 63) // 64 * 64
    A, B, bg = I["A"].double(), I["B"].double(), I["bg"]
    z = ks // 2
    dropped = x - A[:, z * kslice: (z + 1) * kslice] @ B[:, z * kslice: (z + 1) * kslice].t()
    excess("splitk_slice_dropped", dropped + I["C0"].double(), ref, bound, rows=bg)
    assert ks * kslice > K
    npast = min(ks * kslice - K, 8)          # lda = K + 8: at least the first chunk past K is poison
    excess("splitk_last_slice_kslice", ref + npast * POISON * POISON, ref, bound, rows=bg)
    excess("splitk_reduce_ignores_c", epilogue64(x, I, 2, False, 0, fault="splitk_reduce_ignores_c"), ref, bound, rows=bg)


def tn_colmap_nt(ref):
    """the TN kernel's accumulators stored at the NT form's wave columns: within every 256-column tile, tile column wn * 64 + j * 16 + t receives what belongs at
    (j >> 1) * 128 + wn * 32 + (j & 1) * 16 + t"""
    N = ref.shape[1]
    bad = ref.clone()
    for n0 in range(0, N, 256):
        for wn in range(4):
            for j in range(4):
                dst, src = n0 + wn * 64 + j * 16, n0 + (j >> 1) * 128 + wn * 32 + (j & 1) * 16
                w = min(16, N - dst, N - src)
                if w > 0:
                    bad[:, dst: dst + w] = ref[:, src: src + w]
    return bad


@pytest.mark.parametrize("M,N,K,ks", TN_CASES)
def test_cpu_gemm_tn_emulation_inside_and_faults_outside(M, N, K, ks):
    I = mm_inputs(M, N, K)
    x, Ex = mm_ref(I)
    ref, bound = out_bound(x, Ex, I, 2, False, 0)
    emu = I["C0"] + (emu_splitk(I["A"], I["B"], ks) if ks > 1 else emu_contract(I["A"], I["B"]))
    gcheck("emu", "gemm.f32", emu, ref, bound, f"TN M={M} N={N} K={K} ks={ks}")
    check_onehots(I, emu, 2, False, "TN (emulation)")
    bg = I["bg"]
    excess("tn_row_past_K", ref + POISON * POISON, ref, bound, rows=bg)
    bad = ref.clone()
    bad[M - 8:] = ref[M - 16: M - 8]          # the last 8-column chunk of dY read 8 columns early
    excess("tn_col_clamp", bad, ref, bound, rows=list(range(M - 8, M)))
    excess("tn_wave_colmap_nt", tn_colmap_nt(ref), ref, bound, rows=bg)


# ======================================================================================================================================================
# fused SwiGLU
# ======================================================================================================================================================

def swiglu_rows_index(M, block, stride):
    r = torch.arange(M)
    return (r // block) * stride + r % block


def check_swiglu_a(side, a, gu, what):
    """a against float64 SwiGLU of the given (stored) bf16 GU, and against the one correct bit pattern where there is only one"""
    gu, a = gu.cpu(), a.cpu().to(BF)
    m = swiglu_math(gu, torch.zeros(gu.shape[0], gu.shape[1] // 2), False)
    r = frac("swiglu.a", a, m["a"], m["E_a"])
    mx = float(r.max())
    USED[side]["swiglu.a"] = max(USED[side].get("swiglu.a", 0.0), mx)
    assert mx <= 1.0, f"{what}: swiglu.a at {mx:.3g} x its bound"
    want, ok = swiglu_exact(gu)
    assert int(ok.sum()) > ok.numel() // 4 and torch.equal(bits(a)[ok], bits(want)[ok]), f"{what}: a differs from bf16(bf16(silu(gate)) up) where that is one value"


@pytest.mark.parametrize("M,I_,K", SWIGLU_CASES)
def test_cpu_swiglu_emulation_inside_and_faults_outside(M, I_, K):
    I = mm_inputs(M, 2 * I_, K)
    x, Ex = mm_ref(I)
    ref, bound = out_bound(x, Ex, I, 0, False, 0)
    gu = emu_contract(I["A"], I["B"]).to(BF)
    gcheck("emu", "swiglu.gu", gu, ref, bound, f"SwiGLU GU M={M} I={I_} K={K}")
    check_onehots(I, gu, 0, False, "SwiGLU GU (emulation)")
    a = swiglu_math(gu, torch.zeros(M, I_), True)["a"]
    check_swiglu_a("emu", a, gu, f"SwiGLU a M={M} I={I_} K={K}")
    m = swiglu_math(gu, torch.zeros(M, I_), False)
    swapped = swiglu_math(torch.cat([gu[:, I_:], gu[:, :I_]], 1), torch.zeros(M, I_), False)["a"]
    r = frac("swiglu.a", swapped, m["a"], m["E_a"])[I["bg"]]
    ex = float(r.amax(-1).min())
    assert ex >= FAULT_FACTOR, ex
    FAULT_SEEN["swiglu_gate_up_swapped"] = min(FAULT_SEEN.get("swiglu_gate_up_swapped", INF), ex)
    # a from the UNROUNDED gate|up: inside the bound (one bf16 ulp against c = 3), caught by the equality
    want, ok = swiglu_exact(gu)
    g64, u64 = x[:, :I_], x[:, I_:]
    unr = (bfr(g64 / (1 + torch.exp(-g64))) * u64).to(BF)
    n = int((bits(unr)[ok] != bits(want)[ok]).sum())
    assert n > 0, "fault 'swiglu_unrounded' changes no bit where a is one value"
    FAULT_SEEN["swiglu_unrounded"] = INF


@pytest.mark.parametrize("M,block,stride", SWIGLU_ROWS)
def test_cpu_swiglu_rows_emulation_inside_and_fault_outside(M, block, stride):
    """the rows form with block_stride taken as block reads (and writes) rows r instead of (r / block) stride + r % block: from the second block on, the gaps' poison or other rows"""
    I = mm_inputs(M, 256, 72)
    x, Ex = mm_ref(I)
    ref, bound = out_bound(x, Ex, I, 0, False, 0)
    gu = emu_contract(I["A"], I["B"]).to(BF)          # per row the arithmetic of the plain launch
    gcheck("emu", "swiglu.gu", gu, ref, bound, f"SwiGLU rows GU M={M}")
    check_swiglu_a("emu", swiglu_math(gu, torch.zeros(M, 128), True)["a"], gu, f"SwiGLU rows a M={M}")
    idx = swiglu_rows_index(M, block, stride)
    arena = torch.full((int(idx[-1]) + 1, 72), 4096.0, dtype=F64)
    arena[idx] = I["A"].double()
    if stride == block:
        return
    bad = arena[:M] @ I["B"].double().t()
    excess("swiglu_rows_stride_is_block", bad, ref, bound, rows=[int(r) for r in I["bg"] if r >= block])


# ======================================================================================================================================================
# linear_logprob
# ======================================================================================================================================================

LP_CASES = [(5, 258, 72), (261, 1001, 136), (130, 4360, 64), (1, 8, 8), (300, 4096, 264)]


@functools.lru_cache(maxsize=None)
def lp_inputs(M, V, K):
    g = gen(M + 7 * V + 1009 * K)
    H, W = torch.randn(M, K, generator=g), 0.5 * torch.randn(V, K, generator=g)
    tgt = torch.randint(0, V, (M,), generator=g)
    hs = {4360: 65, 4096: 62}.get(V, 1)          # the hot slice
    ragged = (V // 64) * 64 if V % 64 else V - 2
    roles = [(0, "needle", V - 1)]
    if M >= 5:
        roles += [(1, "flat", 0), (2, "hot", hs * 64), (3, "ign", -100), (4, "normal", ragged)]
    if M > 5:
        roles += [(5, "ign", V), (6, "needle", min(63, V - 1)), (7, "flat", min(64, V - 1)), (8, "hot", hs * 64 + 63), (9, "normal", max(ragged, V - 3))]
    if M > 258:
        roles += [(256, "needle", V - 1), (257, "flat", V - 1), (258, "hot", hs * 64 + 1)]
    rows = {"needle": [], "flat": [], "hot": [], "ign": [], "normal": []}
    for r, role, t in roles:
        rows[role if (role != "hot" or V >= 128) else "normal"].append(r)
        tgt[r] = t
    hn, gv = torch.randn(K, generator=g).to(BF).float(), torch.randn(K, generator=g)
    for i, r in enumerate(rows["needle"]):
        H[r] = hn * (1.0, 0.75, 0.5)[i % 3]
    for r in rows["flat"]:
        H[r] *= 2.0 ** -6
    for r in rows["hot"]:
        H[r] = gv + 0.25 * torch.randn(K, generator=g)
    if rows["hot"]:
        W[hs * 64: hs * 64 + 64] += (40.0 / float(gv @ gv)) * gv
    W[V - 1] = 0.6 * hn
    if M >= 130:          # one-hot rows of H: their logits are single products of W
        for i, k in enumerate(hot_ks(K)):
            H[10 + i] = 0
            H[10 + i, k] = 1.0
    gvec = 2 * torch.randn(M, generator=g)
    gvec[rows["ign"]] = 0
    H, W = H.to(BF), W.to(BF)
    assert normal_range(H) and normal_range(W)
    return {"M": M, "V": V, "K": K, "H": H, "W": W, "tgt": tgt.to(torch.int64), "g": gvec.to(F32), "rows": rows, "hs": hs}


def lp_ref(I, dev="cpu"):
    """float64 references and bounds of lse, logp and dlogits"""
    M, V, K = I["M"], I["V"], I["K"]
    H, W, tgt, gv = I["H"].to(dev).double(), I["W"].to(dev).double(), I["tgt"].to(dev), I["g"].to(dev).double()
    x, bx = H @ W.t(), b_x(H.abs() @ W.abs().t(), K)
    lse, m = torch.logsumexp(x, -1), x.amax(-1)
    p = torch.exp(x - lse[:, None])
    b_lse = (p * bx).sum(-1) + U24 * (8 * (m.abs() + (lse - m).abs() + lse.abs() + 1) + V) + TINY
    ar = torch.arange(M, device=x.device)
    ok = (tgt >= 0) & (tgt < V)
    tc = tgt.clamp(0, V - 1)
    xt = x[ar, tc]
    logp = torch.where(ok, xt - lse, torch.zeros_like(lse))
    b_logp = torch.where(ok, b_lse + bx[ar, tc] + 8 * U24 * xt.abs(), torch.zeros_like(lse)) + TINY
    lse32 = lse.to(F32)
    p32 = torch.exp(x - lse32.double()[:, None])
    oh = torch.zeros_like(x)
    oh[ar[ok], tgt[ok]] = 1
    dl = gv[:, None] * (oh - p32)
    b_dl = U8 * 2 * dl.abs() + U24 * F_EXP * gv.abs()[:, None] * (oh + p32) + gv.abs()[:, None] * p32 * (bx + b_lse[:, None]) + TINY
    return {"x": x, "lse": lse, "b_lse": b_lse, "logp": logp, "b_logp": b_logp, "lse32": lse32, "dl": dl, "b_dl": b_dl, "p": p, "ok": ok, "oh": oh}


def lp_parts64(x, V):
    """float64 (max, sum exp(x - max)) of every 64-column slice of the 256-column tiles, empty slices (-inf, 0)"""
    nparts = (V + 255) // 256 * 4
    xp = torch.full((x.shape[0], nparts * 64), -INF, dtype=x.dtype)
    xp[:, :V] = x
    xp = xp.view(-1, nparts, 64)
    pm = xp.amax(-1)
    ps = torch.exp(xp - torch.where(torch.isfinite(pm), pm, torch.zeros_like(pm))[..., None]).sum(-1)
    return pm, ps


def emu_combine(pm, ps):
    """lse_combine_kernel: lane l merges parts l, l + 64, ... in order, then the 64 lanes merge in a butterfly (fp32)"""
    M, nparts = pm.shape
    m, s = torch.full((M, 64), -INF, dtype=F32), torch.zeros(M, 64, dtype=F32)
    for t0 in range(0, nparts, 64):
        v0, v1 = torch.full((M, 64), -INF, dtype=F32), torch.zeros(M, 64, dtype=F32)
        w = min(64, nparts - t0)
        v0[:, :w], v1[:, :w] = pm[:, t0: t0 + w], ps[:, t0: t0 + w]
        up = v0 > m
        s = torch.where(up, s * torch.exp(m - v0), s)
        m = torch.where(up, v0, m)
        s = torch.where(v0 != -INF, s + v1 * torch.exp(v0 - m), s)
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        m2, s2 = m[:, lane ^ o], s[:, lane ^ o]
        mm = torch.maximum(m, m2)
        z = torch.zeros_like(s)
        s = torch.where(m == -INF, z, s * torch.exp(m - mm)) + torch.where(m2 == -INF, z, s2 * torch.exp(m2 - mm))
        m = mm
    return m[:, 0] + torch.log(s[:, 0])


@pytest.mark.parametrize("M,V,K", LP_CASES)
def test_cpu_linear_logprob_emulation_inside_and_faults_outside(M, V, K):
    I = lp_inputs(M, V, K)
    R = lp_ref(I)
    x, tgt, rows, ok, gv = R["x"], I["tgt"], I["rows"], R["ok"], I["g"].double()
    what = f"M={M} V={V} K={K}"
    assert bool((R["p"][rows["needle"], V - 1] >= 0.02).all()), "the needle's softmax weight at its rows"
    # emulation
    x32 = emu_contract(I["H"], I["W"])
    pm, ps = lp_parts64(x32, V)
    lse_e = emu_combine(pm.to(F32), ps.to(F32))
    ar = torch.arange(M)
    logp_e = torch.where(ok, x32[ar, tgt.clamp(0, V - 1)] - lse_e, torch.zeros_like(lse_e))
    gcheck("emu", "lp.lse", lse_e, R["lse"], R["b_lse"], what)
    gcheck("emu", "lp.logp", logp_e, R["logp"], R["b_logp"], what)
    dl_e = (-I["g"][:, None] * torch.exp(x32 - R["lse32"][:, None]) + I["g"][:, None] * R["oh"].to(F32)).to(BF)
    gcheck("emu", "lp.dlogits", dl_e, R["dl"], R["b_dl"], what)
    # fault models on the float64 reference
    needle, flat, hot = rows["needle"], rows["flat"], rows["hot"]
    nparts = (V + 255) // 256 * 4
    if V % 64:
        ndup = 64 - V % 64
        bad = torch.logaddexp(R["lse"], x[:, V - 1] + torch.log(torch.tensor(float(ndup), dtype=F64)))
        excess("lse_cols_ge_V", bad, R["lse"], R["b_lse"], rows=needle)
    n_empty = nparts - (V + 63) // 64
    if n_empty and V in (258, 8):
        bad = torch.logaddexp(R["lse"], torch.log(torch.tensor(float(n_empty), dtype=F64)))
        excess("lse_empty_slice_exp0", bad, R["lse"], R["b_lse"], rows=flat or [0])
    if nparts > 64:
        excess("lse_combine_stops_64", torch.logsumexp(x[:, :4096], -1), R["lse"], R["b_lse"], rows=flat + [r for r in needle if int(tgt[r]) == V - 1])
        pm64, ps64 = lp_parts64(x, V)
        lm, ls = pm64[:, :64].clone(), ps64[:, :64].clone()          # per lane: part l, then part l + 64 without the rescale where it has the larger maximum
        for l in range(nparts - 64):
            m1, s1 = pm64[:, 64 + l], ps64[:, 64 + l]
            later = m1 > lm[:, l]
            mm = torch.maximum(lm[:, l], m1)
            good = ls[:, l] * torch.exp(lm[:, l] - mm) + torch.where(m1 == -INF, torch.zeros_like(s1), s1 * torch.exp(m1 - mm))
            ls[:, l] = torch.where(later, ls[:, l] + s1, good)
            lm[:, l] = mm
        bad = torch.logsumexp(lm + torch.log(ls), -1)
        excess("lse_combine_no_rescale", bad, R["lse"], R["b_lse"], rows=hot)
    t1 = [r for r in needle if int(tgt[r]) == V - 1]
    bad = R["logp"].clone()
    bad[t1] = x[t1, V - 2] - R["lse"][t1]
    excess("logp_target_minus_1", bad, R["logp"], R["b_logp"], rows=t1)
    if rows["ign"]:
        bad = x[ar, tgt.clamp(0, V - 1)] - R["lse"]
        excess("logp_ignored_not_zeroed", bad, R["logp"], R["b_logp"], rows=rows["ign"])
    far = [r for r in range(M) if ok[r] and int(tgt[r]) >= 256 and float(gv[r]) != 0]
    if far:
        oh = torch.zeros_like(x)
        oh[far, [int(tgt[r]) % 256 for r in far]] = 1
        bad = R["dl"].clone()
        bad[far] = gv[far, None] * (oh[far] - torch.exp(x[far] - R["lse32"].double()[far, None]))
        excess("dlogits_onehot_tile_local", bad, R["dl"], R["b_dl"], rows=far)
    if M > 1:
        bad = gv[:, None] * (R["oh"] - torch.exp(x - R["lse32"].double()[M - 1]))
        excess("dlogits_lse_clamped_row", bad, R["dl"], R["b_dl"], rows=needle + flat + hot)


def _print_used(side):
    for key, v in sorted(USED[side].items()):
        print(f"[gemm_f64 {side}] {key}: largest used fraction of the bound {v:.4f}")


def test_cpu_every_fault_model_was_exercised_and_emulation_record():
    """Every fault model of FAULT_MODELS was applied somewhere above (run the whole CPU part: this test reads what the others recorded)."""
    missing = [f for f in FAULT_MODELS if f not in FAULT_SEEN]
    assert not missing, f"fault models never exercised: {missing}"
    for f in FAULT_MODELS:
        print(f"[gemm_f64 cpu] fault {f}: smallest excess at its designated elements {FAULT_SEEN[f]:.3g} x bound")
    _print_used("emu")
    assert all(v <= 1.0 for v in USED["emu"].values())


# ======================================================================================================================================================
# GPU part
# ======================================================================================================================================================

def roundup(n, q):
    return (n + q - 1) // q * q


def operands(I, transposed=False):
    """A and B in Guards: poison in the columns past K (NT; lda = K + 8, ldb = K + 16) or in the rows past K (TN: [K, M] and [K, N], ld = M + 8 / N + 16) and around them"""
    M, N, K = I["M"], I["N"], I["K"]
    if transposed:
        return Guard(K, M, BF, M + 8, I["A"].t()), Guard(K, N, BF, N + 16, I["B"].t())
    return Guard(M, K, BF, K + 8, I["A"]), Guard(N, K, BF, K + 16, I["B"])


def out_guard(I, mode, misaligned=False):
    M, N = I["M"], I["N"]
    dtype, q = (BF, 8) if mode == 0 else (F32, 4)
    ldc = N + 3 if misaligned else roundup(N, q) + q
    assert not misaligned or ldc % q
    return Guard(M, N, dtype, ldc, I["C0"] if mode == 2 else None, off=1 if misaligned else 0), ldc


def gpu_nt_case(M, N, K, big, misaligned=False, variants=None):
    I = mm_inputs(M, N, K)
    x, Ex = mm_ref(I, DEV)
    Ag, Bg = operands(I)
    bias = d(I["bias"])
    for mode, use_bias, act in variants or variants_of(M, N, K, big):
        what = f"gemm_nt M={M} N={N} K={K} mode={mode} bias={use_bias} act={act}" + (" misaligned" if misaligned else "")
        ref, bound = out_bound(x, Ex, I, mode, use_bias, act, DEV)
        Cg, ldc = out_guard(I, mode, misaligned)
        call_guarded("gemm_nt_bf16", (Ag, Bg, Cg, bias if use_bias else None, M, N, K, K + 8, K + 16, ldc, mode, act), (Cg,), what)
        gcheck("gpu", out_key(mode, act), Cg.view, ref, bound, what)
        if not act:
            check_onehots(I, Cg.view, mode, use_bias, what)
    Ag.untouched("A")
    Bg.untouched("B")


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", NT128_CASES)
def test_gpu_gemm_nt_128(M, N, K):
    """the 128 x 128 kernel: out_mode 0 / 1 / 2, bf16 + bias, bf16 + bias + GELU (fp32 + bias + GELU once) against float64; one-hot rows bit for bit"""
    gpu_nt_case(M, N, K, False)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", NT256_CASES)
def test_gpu_gemm_nt_256(M, N, K):
    """the 256 x 256 kernel at nk 1, 2, 3, 5 on ragged tile rows / columns, empty waves and scalar tails"""
    gpu_nt_case(M, N, K, True)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(100, 131, 72), (257, 264, 136), (2824, 3912, 8), (3072, 3846, 8)])
def test_gpu_gemm_nt_misaligned(M, N, K):
    """C misaligned by one element, ldc no multiple of 8 / 4: the scalar store paths of both kernels, for every output type"""
    gpu_nt_case(M, N, K, M >= 512, misaligned=True, variants=VARIANTS[:3])


def splitk_ws(M, N, ks):
    return workspace(hip.lib().iadr1_gemm_nt_splitk_workspace_bytes(M, N, ks))


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,ks", SPLITK_CASES)
def test_gpu_gemm_nt_splitk(M, N, K, ks):
    """split-K accumulate against float64; run-to-run bits; the workspace's old contents do not matter"""
    I = mm_inputs(M, N, K)
    x, Ex = mm_ref(I, DEV)
    ref, bound = out_bound(x, Ex, I, 2, False, 0, DEV)
    Ag, Bg = operands(I)
    what = f"split-K M={M} N={N} K={K} ks={ks}"
    outs = []
    for fill in (None, None, 4096.0):
        Cg, ldc = out_guard(I, 2)
        ws = splitk_ws(M, N, ks)
        if fill is not None:
            ws.view.fill_(fill)
        call_guarded("gemm_nt_splitk_acc_bf16", (Ag, Bg, Cg, ws, M, N, K, K + 8, K + 16, ldc, ks), (Cg, ws), what)
        outs.append(Cg.view.clone())
    gcheck("gpu", "gemm.f32", outs[0], ref, bound, what)
    check_onehots(I, outs[0], 2, False, what)
    assert same_bits(outs[0], outs[1]), f"{what}: two runs differ"
    assert same_bits(outs[0], outs[2]), f"{what}: the result depends on what the workspace held"
    Ag.untouched("A")
    Bg.untouched("B")


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,ks", TN_CASES)
def test_gpu_gemm_tn(M, N, K, ks):
    """C += A[K, M]^T . B[K, N] (transpose reads out of LDS), un-split and split, against float64; bit-equal to the NT kernels on transposed copies"""
    I = mm_inputs(M, N, K)
    x, Ex = mm_ref(I, DEV)
    ref, bound = out_bound(x, Ex, I, 2, False, 0, DEV)
    Ag, Bg = operands(I, transposed=True)
    what = f"gemm_tn M={M} N={N} K={K} ks={ks}"
    Cg, ldc = out_guard(I, 2)
    ws = splitk_ws(M, N, ks) if ks > 1 else None
    call_guarded("gemm_tn_acc_bf16", (Ag, Bg, Cg, ws, M, N, K, M + 8, N + 16, ldc, ks), (Cg,) + ((ws,) if ws else ()), what)
    gcheck("gpu", "gemm.f32", Cg.view, ref, bound, what)
    check_onehots(I, Cg.view, 2, False, what)
    Ag.untouched("dY")
    Bg.untouched("X")
    Kp = roundup(K, 8)          # the NT form on transposed copies, K padded to 8 with zeros (exact)
    At, Bt = torch.zeros(M, Kp, dtype=BF, device=DEV), torch.zeros(N, Kp, dtype=BF, device=DEV)
    At[:, :K], Bt[:, :K] = d(I["A"]), d(I["B"])
    Cn, ldn = out_guard(I, 2)
    if ks > 1:
        call_guarded("gemm_nt_splitk_acc_bf16", (At, Bt, Cn, splitk_ws(M, N, ks), M, N, Kp, Kp, Kp, ldn, ks), (Cn,), what + " (NT)")
    else:
        call_guarded("gemm_nt_bf16", (At, Bt, Cn, None, M, N, Kp, Kp, Kp, ldn, 2, 0), (Cn,), what + " (NT)")
    assert same_bits(Cg.view, Cn.view), f"{what}: TN differs from NT on transposed copies"


def run_swiglu(I, M, I_, K, store_gu, rows=None):
    """(GU guard or None, a guard) of one launch; rows = (block, stride, index): the rows form over arenas whose gap rows hold 2^12 (A) / the sentinel (outputs)"""
    Ag, Wg = operands(I)
    R = M if rows is None else int(rows[2][-1]) + 1
    if rows is not None:
        arena = torch.full((R, K), 4096.0, dtype=BF)
        arena[rows[2]] = I["A"]
        Ag = Guard(R, K, BF, K + 8, arena)
    GUg, ag = (Guard(R, 2 * I_, BF, 2 * I_ + 8) if store_gu else None), Guard(R, I_, BF, I_ + 8)
    outs = (ag,) + ((GUg,) if store_gu else ())
    what = f"gemm_swiglu M={M} I={I_} K={K} GU={'stored' if store_gu else 'NULL'} rows={rows[:2] if rows else None}"
    if rows is None:
        call_guarded("gemm_swiglu_bf16", (Ag, Wg, GUg, ag, M, I_, K, K + 8, K + 16, 2 * I_ + 8 if store_gu else 0, I_ + 8), outs, what)
    else:
        call_guarded("gemm_swiglu_rows_bf16", (Ag, Wg, GUg, ag, M, I_, K, K + 8, K + 16, 2 * I_ + 8 if store_gu else 0, I_ + 8, rows[0], rows[1]), outs, what)
        gap = torch.ones(R, dtype=torch.bool, device=DEV)
        gap[d(rows[2])] = False
        for g_ in outs:
            cols, ld = g_.view.shape[1], g_.view.stride(0)
            saved = g_.saved.view(-1, ld)[2: 2 + R, :cols]
            assert same_bits(g_.view[gap], saved[gap]), f"{what}: an arena row between the blocks was written"
    Ag.untouched("A")
    Wg.untouched("W")
    return GUg, ag


@pytest.mark.gpu
@pytest.mark.parametrize("M,I_,K", SWIGLU_CASES)
def test_gpu_gemm_swiglu(M, I_, K):
    """GU against float64 (+ one-hot rows); a against float64 SwiGLU of the stored GU, bit-equal to swiglu_fwd on it; GU = NULL gives the same a"""
    I = mm_inputs(M, 2 * I_, K)
    x, Ex = mm_ref(I, DEV)
    ref, bound = out_bound(x, Ex, I, 0, False, 0, DEV)
    what = f"gemm_swiglu M={M} I={I_} K={K}"
    GUg, ag = run_swiglu(I, M, I_, K, True)
    gcheck("gpu", "swiglu.gu", GUg.view, ref, bound, what)
    check_onehots(I, GUg.view, 0, False, what)
    check_swiglu_a("gpu", ag.view, GUg.view, what)
    a2 = Guard(M, I_, BF, I_ + 8)
    call_guarded("swiglu_fwd", (GUg, 2 * I_ + 8, a2, I_ + 8, M, I_), (a2,), what)
    assert same_bits(ag.view, a2.view), f"{what}: a differs from swiglu_fwd on the stored GU"
    _, a3 = run_swiglu(I, M, I_, K, False)
    assert same_bits(ag.view, a3.view), f"{what}: a with GU = NULL differs"


@pytest.mark.gpu
@pytest.mark.parametrize("M,block,stride", SWIGLU_ROWS)
def test_gpu_gemm_swiglu_rows(M, block, stride):
    """the rows form equals the plain launch on the gathered rows, bit for bit; the arena rows between the blocks keep their sentinel"""
    I_, K = 128, 72
    I = mm_inputs(M, 2 * I_, K)
    idx = swiglu_rows_index(M, block, stride)
    GUp, ap = run_swiglu(I, M, I_, K, True)
    for store in (True, False):
        GUr, ar_ = run_swiglu(I, M, I_, K, store, rows=(block, stride, idx))
        assert same_bits(ar_.view[d(idx)], ap.view), f"rows form ({block}, {stride}) GU stored={store}: a differs from the plain launch"
        if store:
            assert same_bits(GUr.view[d(idx)], GUp.view), f"rows form ({block}, {stride}): GU differs from the plain launch"


@pytest.mark.gpu
@pytest.mark.parametrize("M,V,K", LP_CASES)
def test_gpu_linear_logprob(M, V, K):
    """lse, logp and dlogits of the fused lm_head against float64; run-to-run bits; ignored rows; ldd = roundup(V, 8) and, at V = 1001, ldd = V odd"""
    I = lp_inputs(M, V, K)
    R = lp_ref(I, DEV)
    what = f"linear_logprob M={M} V={V} K={K}"
    Hg, Wg, tgt = Guard(M, K, BF, K + 8, I["H"]), Guard(V, K, BF, K + 16, I["W"]), d(I["tgt"])
    runs = []
    for _ in range(2):
        lg, sg, ws = vec(M, F32), vec(M, F32), workspace(hip.lib().iadr1_linear_logprob_workspace_bytes(M, V))
        call_guarded("linear_logprob_fwd", (Hg, Wg, tgt, lg, sg, ws, M, V, K, K + 8, K + 16), (lg, sg, ws), what)
        runs.append((lg.view[0].clone(), sg.view[0].clone()))
    gcheck("gpu", "lp.lse", runs[0][1], R["lse"], R["b_lse"], what)
    gcheck("gpu", "lp.logp", runs[0][0], R["logp"], R["b_logp"], what)
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1]), f"{what}: two runs differ"
    assert bool((runs[0][0][~R["ok"]] == 0).all()), "ignored rows give logp = 0"
    gv, zero = d(I["g"]), d(I["g"]) == 0
    for ldd in [roundup(V, 8)] + ([V] if V == 1001 else []):
        dl = Guard(M, V, BF, ldd)
        call_guarded("linear_logprob_dlogits", (Hg, Wg, tgt, d(R["lse32"]), gv, dl, ldd, M, V, K, K + 8, K + 16), (dl,), what + f" ldd={ldd}")
        gcheck("gpu", "lp.dlogits", dl.view, R["dl"], R["b_dl"], what + f" ldd={ldd}")
        assert bool((dl.view[zero] == 0).all()), "g = 0 rows give zeros"
    Hg.untouched("H")
    Wg.untouched("W")


@pytest.mark.gpu
def test_gpu_gemm_host_side_refusals():
    """Shapes the launchers refuse on the host: an error through the binding, no launch, outputs untouched"""
    I = mm_inputs(264, 264, 264)
    Ag, Bg = operands(I)
    Cg, ldc = out_guard(I, 2)
    ws = splitk_ws(264, 264, 4)
    refused("gemm_nt_splitk_acc_bf16", (Ag, Bg, Cg, ws, 264, 264, 200, 272, 280, ldc, 3), (Cg, ws), "K = 200 ksplit 3: empty slice")
    refused("gemm_nt_splitk_acc_bf16", (Ag, Bg, Cg, ws, 264, 264, 264, 272, 280, ldc, 4), (Cg, ws), "K = 264 ksplit 4: empty slice")
    refused("gemm_nt_splitk_acc_bf16", (Ag, Bg, Cg, ws, 264, 264, 264, 272, 280, ldc, 1), (Cg, ws), "ksplit 1")
    refused("gemm_nt_splitk_acc_bf16", (Ag, Bg, Cg, ws, 264, 262, 264, 272, 280, ldc, 2), (Cg, ws), "N % 4")
    # TN reads the same buffers as [K, M] = [264, 264] with ld 272 / 280
    refused("gemm_tn_acc_bf16", (Ag, Bg, Cg, ws, 128, 264, 264, 272, 280, ldc, 1), (Cg, ws), "M < 256")
    refused("gemm_tn_acc_bf16", (Ag, Bg, Cg, ws, 260, 264, 264, 272, 280, ldc, 1), (Cg, ws), "M % 8")
    refused("gemm_tn_acc_bf16", (Ag, Bg, Cg, ws, 264, 264, 264, 272, 280, ldc, 4), (Cg, ws), "TN ksplit 4: empty slice")
    S = mm_inputs(256, 256, 72)
    Sg, Wg = operands(S)
    GUg, ag = Guard(256, 256, BF, 264), Guard(256, 128, BF, 136)
    refused("gemm_swiglu_bf16", (Sg, Wg, GUg, ag, 128, 128, 72, 80, 88, 264, 136), (GUg, ag), "M % 256")
    refused("gemm_swiglu_bf16", (Sg, Wg, GUg, ag, 256, 64, 72, 80, 88, 264, 136), (GUg, ag), "I % 128")
    refused("gemm_swiglu_rows_bf16", (Sg, Wg, GUg, ag, 256, 128, 72, 80, 88, 264, 136, 24, 24), (GUg, ag), "block 24")
    refused("gemm_swiglu_rows_bf16", (Sg, Wg, GUg, ag, 128, 128, 72, 80, 88, 264, 136, 16, 16), (GUg, ag), "rows: M % 256")
    refused("gemm_swiglu_rows_bf16", (Sg, Wg, GUg, ag, 256, 64, 72, 80, 88, 264, 136, 16, 16), (GUg, ag), "rows: I % 128")


@pytest.mark.gpu
def test_gpu_gemm_used_fractions_record():
    """prints the largest used fraction of every bound over the GPU tests above (run after them: it reads what they recorded)"""
    _print_used("gpu")
    assert all(v <= 1.0 for v in USED["gpu"].values())
