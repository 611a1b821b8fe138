"""Log-probs and entropies at a temperature (GRPOArgs.logps_at_temperature): iadr1_linear_logprob_fwd_t / iadr1_linear_logprob_dlogits_t (the OUT_LSE / OUT_DLOGITS
epilogues of gemm_nt_256 on y = x * inv_t) and iadr1_sample_ent_t (LogpArgs.inv_tl in the sampler's two stages), through the library and through ops.

Three kinds of check.  Against float64: lp_ref's formulas of test_gemm_f64 on y = x / T, with its contraction bound bx replaced by (bx + 2 * 2^-24 |x|) / T -- the
contraction's bound scaled, one rounding of inv_t = 1.0f / T and one of the product x * inv_t, each <= 2^-24 relative -- and g replaced by g / T in dlogits; the
sampler's two outputs against numpy at the project's rtol = atol = 1e-5.  T is the float32 value the kernel is handed.  Exact: a temperature of 0.5 is a doubling,
which is exact in bf16 and in fp32, so the run at T = 0.5 equals the plain run on doubled weights / doubled logits bit for bit.  Neutral: temperature 1 through the new
entry points gives the old entry points' bits.  What the GPU cases rely on (a result at the wrong temperature, or a dlogits without the chain rule's 1 / T, cannot
pass) is asserted on the float64 side without a GPU."""
import functools
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iadr1_amd  # noqa: E402,F401
import test_sample_ent as tse  # noqa: E402  (inputs, entropy64, tables, device_args, CASES)
from iadr1_amd import hip, ops  # noqa: E402
from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine  # noqa: E402
from test_gemm_f64 import LP_CASES, U24, b_x, gcheck, lp_inputs, lp_ref, roundup  # noqa: E402
from test_tokenwise_f64 import BF, DEV, F32, F_EXP, FAULT_FACTOR, TINY, U8, Guard, call_guarded, d, same_bits, vec, workspace  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEMPS = (0.9, 0.6, 1.5)
NAN, INF = float("nan"), float("inf")
BAD_TEMPS = (0.0, -1.0, NAN, INF, -INF)


def t32(T):
    """the float32 value of T: what the entry points receive"""
    return float(np.float32(T))


# ---- without a GPU ----------------------------------------------------------------------------------------------------------------------------------------

def test_abi_has_the_three_entry_points():
    L = hip.lib()
    assert hip.version() >= 118
    for name in ("iadr1_linear_logprob_fwd_t", "iadr1_linear_logprob_dlogits_t", "iadr1_sample_ent_t"):
        assert name in hip.PROTOS and hasattr(L, name)
    for new, old, arg in (("iadr1_linear_logprob_fwd_t", "iadr1_linear_logprob_fwd", "temperature"), ("iadr1_linear_logprob_dlogits_t", "iadr1_linear_logprob_dlogits", "temperature"),
                          ("iadr1_sample_ent_t", "iadr1_sample_ent", "logp_temperature")):
        a, b = hip.PROTOS[new][1], hip.PROTOS[old][1]
        assert a[:-2] == b[:-1] and a[-2] == ("float", arg) and a[-1] == b[-1], f"{new}: {old}'s arguments, {arg} in front of stream"


def _fwd_t(L, T, M=4, V=64, K=8, ldh=8, ldw=8, H=None, W=None, tgt=None, logp=None, ws=None):
    rc = L.iadr1_linear_logprob_fwd_t(H, W, tgt, logp, None, ws, M, V, K, ldh, ldw, T, None)
    return rc, L.iadr1_last_error()


def _dl_t(L, T, M=4, V=64, K=8, ldh=8, ldw=8, H=None, W=None, tgt=None, lse=None, g=None, dl=None):
    rc = L.iadr1_linear_logprob_dlogits_t(H, W, tgt, lse, g, dl, V, M, V, K, ldh, ldw, T, None)
    return rc, L.iadr1_last_error()


@pytest.mark.parametrize("call,prefix", [(_fwd_t, b"linear_logprob_fwd_t:"), (_dl_t, b"linear_logprob_dlogits_t:")])
def test_fused_lm_head_refusals_without_a_gpu(call, prefix):
    """Every refusal happens on the host, before any launch (the buffers are NULL or made-up addresses that nothing may read), with the entry point's prefix."""
    L = hip.lib()
    some = 0x1000
    for T in BAD_TEMPS:
        for ptrs in ({}, dict(H=some, W=some, tgt=some)):
            rc, m = call(L, T, **ptrs)
            assert rc < 0 and m.startswith(prefix) and b"temperature must be finite and > 0" in m, (T, m)
    # everything the plain pair refuses, at a good temperature
    for kw, word in ((dict(M=0), b"empty problem"), (dict(V=0), b"empty problem"), (dict(K=0), b"empty problem"), (dict(K=12), b"multiples of 8"), (dict(ldh=12), b"multiples of 8"),
                     (dict(ldw=9), b"multiples of 8"), (dict(H=some + 2, W=some), b"16-byte aligned"), (dict(H=some, W=some + 8), b"16-byte aligned"),
                     (dict(H=some, W=some), b"required")):
        rc, m = call(L, 0.9, **kw)
        assert rc < 0 and m.startswith(prefix) and word in m, (kw, m)
    if call is _fwd_t:
        rc, m = call(L, 0.9, H=some, W=some, tgt=some, logp=some, ws=some + 4)
        assert rc < 0 and m.startswith(prefix) and b"8-byte aligned workspace" in m, m


def _ent_t(L, lt, *, B_=1, V=64, T_=0.9, k=50, p=0.9, min_p=0.0, pen=1.0, seen=None, ld_seen=0, mark=0, state=None, allow=None, ld_allow=0, trans=None, ld_trans=0, S_=0,
           ent=None, ld_ent=0, cols=0, lp=None, ld_lp=0, lp_cols=0, ws=None):
    rc = L.iadr1_sample_ent_t(None, 0, None, lp, ld_lp, lp_cols, ws, B_, V, T_, k, p, min_p, pen, seen, ld_seen, mark, -1, 0, 0, None, None, state, allow, ld_allow, trans,
                              ld_trans, S_, ent, ld_ent, cols, lt, None)
    return rc, L.iadr1_last_error()


def test_sampler_refusals_without_a_gpu():
    """logp_temperature not finite or <= 0, and everything iadr1_sample_ent refuses (test_sample_ent's list), all with the prefix sample_ent_t: and before any launch."""
    L = hip.lib()
    some = 0x1000
    guide = dict(state=some, allow=some, ld_allow=2, trans=some, ld_trans=64, S_=3)
    ent = dict(ent=some, ld_ent=4, cols=4)
    for lt in BAD_TEMPS:
        for extra in ({}, ent, dict(lp=some, ld_lp=4, lp_cols=4)):
            rc, m = _ent_t(L, lt, **extra)
            assert rc < 0 and m.startswith(b"sample_ent_t:") and b"logp_temperature must be finite and > 0" in m, (lt, m)
    msgs = set()

    def refused(word, **kw):
        rc, m = _ent_t(L, 0.6, **kw)
        assert rc < 0 and m.startswith(b"sample_ent_t:") and word in m, (kw, m)
        msgs.add(m)

    refused(b"ent_out needs ent_cols > 0", **dict(ent, cols=0))
    refused(b"ld_ent=3 is less than ent_cols = 4", **dict(ent, ld_ent=3))
    refused(b"logp_out needs logp_cols > 0", lp=some, ld_lp=4, lp_cols=0, ws=some)          # (the last check of all: it sits behind the workspace's)
    for extra in (ent, {}):
        refused(b"allow needs state", **dict(guide, state=None), **extra)
        refused(b"must be NULL when allow is NULL", state=some, **extra)
        refused(b"outside 1..32767", **dict(guide, S_=0), **extra)
        refused(b"ld_allow=1 is less than ceil(V / 32) = 2", **dict(guide, ld_allow=1), **extra)
        refused(b"ld_trans=63 is less than V = 64", **dict(guide, ld_trans=63), **extra)
        refused(b"min_p must be in", min_p=1.0, **extra)
        refused(b"repetition_penalty must be finite", pen=INF, **extra)
        refused(b"seen bitmap", pen=1.3, **extra)
        refused(b"nucleus", k=0, p=0.9, **extra)          # the whole-vocabulary nucleus stays refused
        refused(b"top_p must be in", p=0.0, **extra)
        refused(b"empty problem or missing workspace (iadr1_sample_ent_workspace_bytes)", **extra)     # neither output is legal: every check passed but the workspace
    assert len(msgs) == 3 + 11


def _grpo_ad():
    spec = importlib.util.spec_from_file_location("grpo_ad_logp_temperature_flag", os.path.join(ROOT, "train", "stage_rl", "grpo_ad.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_default_flag_and_config_file(tmp_path):
    from iadr1_amd.trainer import GRPOConfig
    assert GRPOArgs().logps_at_temperature is False and GRPOConfig().logps_at_temperature is False
    assert GRPOArgs().logp_temperature == 1.0 and GRPOArgs(temperature=0.7).logp_temperature == 1.0 and GRPOArgs(temperature=0.7, logps_at_temperature=True).logp_temperature == 0.7
    mod = _grpo_ad()
    base = ["--model_name_or_path", "/m", "--output_dir", "o", "--dataset_name", "d.json"]
    assert mod.build_parser().parse_args(base).logps_at_temperature is False
    assert mod.build_parser().parse_args(base + ["--logps_at_temperature"]).logps_at_temperature is True
    a = mod.build_parser().parse_args(base + ["--logps_at_temperature", "true", "--temperature", "0.7"])
    assert a.logps_at_temperature is True and a.temperature == 0.7
    assert mod.build_parser().parse_args(base + ["--logps_at_temperature", "false"]).logps_at_temperature is False
    y = tmp_path / "run.yaml"
    y.write_text("model_name_or_path: /m\noutput_dir: o\ndataset_name: d.json\nlogps_at_temperature: true\ntemperature: 0.8\n")
    a = mod.parse_args_and_config(mod.build_parser(), ["--config", str(y)])
    assert a.logps_at_temperature is True and a.temperature == 0.8
    a = mod.parse_args_and_config(mod.build_parser(), ["--config", str(y), "--logps_at_temperature", "false"])
    assert a.logps_at_temperature is False
    assert "logps_at_temperature" in GRPOConfig.__dataclass_fields__          # grpo_ad.main copies every parsed flag that is a GRPOConfig field


@pytest.mark.parametrize("T", [0.0, -0.5, NAN, INF])
def test_the_engine_refuses_the_option_without_a_temperature_to_score_at(T):
    with pytest.raises(ValueError, match="logps_at_temperature"):
        SCGRPOEngine(None, None, None, GRPOArgs(logps_at_temperature=True, temperature=T))


# ---- the fused lm_head against float64 -------------------------------------------------------------------------------------------------------------------------

def lp_ref_t(I, T, dev="cpu"):
    """lp_ref's formulas (test_gemm_f64) on y = x / T: bx -> (bx + 2 U24 |x|) / T, g -> g / T."""
    M, V, K = I["M"], I["V"], I["K"]
    H, W, tgt = I["H"].to(dev).double(), I["W"].to(dev).double(), I["tgt"].to(dev)
    gv = I["g"].to(dev).double() / T
    x0 = H @ W.t()
    x, bx = x0 / T, (b_x(H.abs() @ W.abs().t(), K) + 2 * U24 * x0.abs()) / T
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
    return {"x": x, "lse": lse, "b_lse": b_lse, "logp": logp, "b_logp": b_logp, "lse32": lse32, "dl": dl, "b_dl": b_dl, "p32": p32, "ok": ok, "oh": oh}


def test_the_restatement_at_temperature_one_is_lp_ref():
    I = lp_inputs(*LP_CASES[1])
    A, B_ = lp_ref_t(I, 1.0), lp_ref(I)
    for k in ("lse", "logp", "dl"):
        assert torch.equal(A[k], B_[k]), k
    for k in ("b_lse", "b_logp", "b_dl"):
        assert bool((A[k] >= B_[k]).all()) and bool((A[k] <= B_[k] * 1.5 + 1e-6).all()), k          # (the same bounds plus the two roundings of the scale)


@pytest.mark.parametrize("T", TEMPS)
@pytest.mark.parametrize("M,V,K", LP_CASES)
def test_cpu_fault_models_of_the_fused_lm_head(M, V, K, T):
    """Conditions of the GPU cases: lse at temperature 1 lies beyond the bound of the reference at T on every needle row, logp on those whose target is another token; a dlogits without the 1 / T on g
    lies beyond it in every row with g != 0 and a target that is not the row's needle."""
    I = lp_inputs(M, V, K)
    T = t32(T)
    R, R1 = lp_ref_t(I, T), lp_ref(I)
    needle = I["rows"]["needle"]
    # (a needle row whose target IS the needle has logp = -0 at every temperature -- the needle's weight is 1 to float64 -- so logp is held to it on the others)
    for key, rows in (("lse", needle), ("logp", [r for r in needle if int(I["tgt"][r]) != V - 1])):
        if not rows:
            continue
        ex = ((R1[key] - R[key]).abs() / R["b_" + key])[rows]
        print(f"[logp_temperature cpu] M={M} V={V} K={K} T={T:.3g}: {key} at temperature 1 is {float(ex.min()):.3g} x the bound off at the needle rows {rows}")
        assert float(ex.min()) >= FAULT_FACTOR
    g = I["g"].double()
    bad = g[:, None] * (R["oh"] - R["p32"])          # the chain rule's 1 / T forgotten
    ex = ((bad - R["dl"]).abs() / R["b_dl"]).amax(-1)
    live = (g != 0) & R["ok"]
    live[[r for r in needle if int(I["tgt"][r]) == V - 1]] = False          # (onehot - p is 0 to float64 in a row whose target is its needle: dl is 0 whatever g is)
    if bool(live.any()):          # (M = 1: the only row's target is its needle)
        print(f"[logp_temperature cpu] M={M} V={V} K={K} T={T:.3g}: dlogits without 1 / T is >= {float(ex[live].min()):.3g} x the bound off in every row with g != 0")
    assert bool(live.any()) or M == 1
    assert bool((ex[live] >= FAULT_FACTOR).all()) and bool((ex[~(g != 0)] == 0).all())


def fused_fwd(name, Hg, Wg, tgt, M, V, K, what, *tail):
    lg, sg, ws = vec(M, F32), vec(M, F32), workspace(hip.lib().iadr1_linear_logprob_workspace_bytes(M, V))
    call_guarded(name, (Hg, Wg, tgt, lg, sg, ws, M, V, K, K + 8, K + 16, *tail), (lg, sg, ws), what)
    return lg.view[0].clone(), sg.view[0].clone()


def fused_dl(name, Hg, Wg, tgt, lse, gv, M, V, K, ldd, what, *tail):
    dl = Guard(M, V, BF, ldd)
    call_guarded(name, (Hg, Wg, tgt, lse, gv, dl, ldd, M, V, K, K + 8, K + 16, *tail), (dl,), what)
    return dl.view.clone()


@pytest.mark.gpu
@pytest.mark.parametrize("T", TEMPS)
@pytest.mark.parametrize("M,V,K", LP_CASES)
def test_gpu_fused_lm_head_at_a_temperature_against_float64(M, V, K, T):
    """lse, logp and dlogits of the _t pair against float64 inside the derived bounds; ignored rows; g = 0 rows; operands and surroundings untouched"""
    I = lp_inputs(M, V, K)
    T = t32(T)
    R = lp_ref_t(I, T, DEV)
    what = f"linear_logprob_t M={M} V={V} K={K} T={T:.3g}"
    Hg, Wg, tgt = Guard(M, K, BF, K + 8, I["H"]), Guard(V, K, BF, K + 16, I["W"]), d(I["tgt"])
    logp, lse = fused_fwd("linear_logprob_fwd_t", Hg, Wg, tgt, M, V, K, what, T)
    u = [gcheck("gpu", "lpt.lse", lse, R["lse"], R["b_lse"], what), gcheck("gpu", "lpt.logp", logp, R["logp"], R["b_logp"], what)]
    assert bool((logp[~R["ok"]] == 0).all()), "ignored rows give logp = 0"
    gv, zero = d(I["g"]), d(I["g"]) == 0
    for ldd in [roundup(V, 8)] + ([V] if V == 1001 else []):
        dl = fused_dl("linear_logprob_dlogits_t", Hg, Wg, tgt, d(R["lse32"]), gv, M, V, K, ldd, what + f" ldd={ldd}", T)
        u.append(gcheck("gpu", "lpt.dlogits", dl, R["dl"], R["b_dl"], what + f" ldd={ldd}"))
        assert bool((dl[zero] == 0).all()), "g = 0 rows give zeros"
    print(f"[logp_temperature gpu] {what}: worst err / bound lse {u[0]:.4f} logp {u[1]:.4f} dlogits {max(u[2:]):.4f}")
    Hg.untouched("H")
    Wg.untouched("W")


@pytest.mark.gpu
@pytest.mark.parametrize("M,V,K", LP_CASES)
def test_gpu_fused_lm_head_half_temperature_is_the_plain_pair_on_doubled_weights(M, V, K):
    """T = 0.5 through ops: logp and lse equal the plain call's on 2 W bit for bit, dlogits equals twice the plain call's given the doubled run's lse (doubling is
    exact in bf16 and fp32 above the underflow range).  Temperature 1 through the _t entry points of the library equals the plain entry points bit for bit."""
    I = lp_inputs(M, V, K)
    what = f"linear_logprob M={M} V={V} K={K}"
    H, W, tgt, gv = d(I["H"]), d(I["W"]), d(I["tgt"]), d(I["g"])
    W2 = (W.float() * 2).to(BF)
    assert torch.equal(W2.float(), W.float() * 2)
    lp_t, lse_t = ops.linear_logprob(H, W, tgt, temperature=0.5)
    lp_2, lse_2 = ops.linear_logprob(H, W2, tgt)
    assert same_bits(lp_t, lp_2) and same_bits(lse_t, lse_2), what
    lp_1, lse_1 = ops.linear_logprob(H, W, tgt)
    ok = d(I["tgt"] >= 0) & d(I["tgt"] < V)
    assert not torch.equal(lp_t[ok], lp_1[ok]), "the temperature reached the kernel"
    dl_t = ops.linear_logprob_dlogits(H, W, tgt, lse_2, gv, temperature=0.5)
    dl_2 = ops.linear_logprob_dlogits(H, W2, tgt, lse_2, gv)
    # (a doubling is exact only off the underflow range: the needle rows hold softmax weights down to e^-100, subnormal or flushed in fp32 and bf16 alike; there both are ~0)
    twice, tiny = (dl_2.float() * 2).to(BF), 2.0 ** -120
    big = (dl_t.float().abs() >= tiny) | (twice.float().abs() >= tiny)
    bad = big & (dl_t.view(torch.int16) != twice.view(torch.int16))
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {int(big.sum())} normal elements are not twice the doubled run's; largest {float(dl_t[bad].float().abs().max()):.3e}"
    assert int(big.sum()) > 0
    # temperature 1 through the new entry points, called directly (ops takes the old ones at 1.0)
    Hg, Wg = Guard(M, K, BF, K + 8, I["H"]), Guard(V, K, BF, K + 16, I["W"])
    a, b = fused_fwd("linear_logprob_fwd_t", Hg, Wg, tgt, M, V, K, what, 1.0), fused_fwd("linear_logprob_fwd", Hg, Wg, tgt, M, V, K, what)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and same_bits(a[0], lp_1) and same_bits(a[1], lse_1), what
    ldd = roundup(V, 8)
    da = fused_dl("linear_logprob_dlogits_t", Hg, Wg, tgt, lse_1, gv, M, V, K, ldd, what, 1.0)
    db = fused_dl("linear_logprob_dlogits", Hg, Wg, tgt, lse_1, gv, M, V, K, ldd, what)
    assert same_bits(da, db), what


# ---- the sampler -------------------------------------------------------------------------------------------------------------------------------------------------

B = tse.B
SENT = tse.SENT
RTOL, ATOL = tse.RTOL, tse.ATOL
SAMPLER_TEMPS = (0.6, 1.5)


@functools.lru_cache(maxsize=None)
def scaled64(V, T):
    """float64: (log_softmax(x / T) [B, V], entropy64(x / T) [B]) of test_sample_ent's rows, computed once per (V, T)"""
    y = tse.inputs(V).astype(np.float64) / T
    m = y.max(-1, keepdims=True)
    ls = y - (m + np.log(np.exp(y - m).sum(-1, keepdims=True)))
    return ls, tse.entropy64(y)


@pytest.mark.parametrize("V", tse.SIZES)
def test_cpu_fault_model_of_the_sampler_inputs(V):
    """On the gaussian-type rows the entropy and the log-prob of the argmax at T differ from those at temperature 1 by more than 100 x the tolerance: outputs at the
    wrong temperature cannot pass."""
    x = tse.inputs(V)
    ls1, H1 = scaled64(V, 1.0)
    for T in SAMPLER_TEMPS:
        ls, H = scaled64(V, t32(T))
        am = x.argmax(1)
        a, b = ls[np.arange(B), am], ls1[np.arange(B), am]
        rh, rl = np.abs(H - H1) / (ATOL + RTOL * np.abs(H)), np.abs(a - b) / (ATOL + RTOL * np.abs(a))
        for r in tse.RANDN_ROWS:
            assert rh[r] > 100 and rl[r] > 100, (T, r, rh[r], rl[r])


def framed(cols=3, ld=5, lead=8):
    """[B, cols] fp32 with row stride ld inside a larger allocation of sentinels"""
    whole = torch.full((2 * lead + B * ld,), SENT, dtype=F32, device=DEV)
    return whole, whole[lead: lead + B * ld].view(B, ld)[:, :cols]


def only_column(whole, col, cols=3, ld=5, lead=8):
    """the framed buffer holds sentinels everywhere but column `col`; returns that column"""
    got = whole.cpu().numpy()
    box = got[lead: lead + B * ld].reshape(B, ld)
    out = box[:, col].copy()
    exp = np.full_like(got, SENT)
    exp[lead: lead + B * ld].reshape(B, ld)[:, col] = out
    assert np.array_equal(got, exp), "something was written outside the step's column"
    return out


def close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.isfinite(ref).all(), what
    err = np.abs(got - ref)
    tol = ATOL + RTOL * np.abs(ref)
    print(f"[logp_temperature gpu] {what}: max |err| {err.max():.3e}, max err / tol {(err / tol).max():.3f}")
    assert (err <= tol).all(), f"{what}: rows {np.flatnonzero(err > tol).tolist()} out of tolerance, max |err| {err.max():.4g}, ref {ref.tolist()}, got {got.tolist()}"


def run_ent(lg, V, case, lt, step=1, seed=77):
    """one framed ops.sample_ent call -> ids, logp column, entropy column, the written seen / state"""
    args, kw = tse.device_args(V, case)
    wl, lp = framed()
    we, en = framed()
    extra = {} if lt is None else {"logp_temperature": lt}
    ids, lp2, en2 = ops.sample_ent(lg, *args, seed=seed, step=step, logp_out=lp, ent_out=en, **kw, **extra)
    assert lp2 is lp and en2 is en
    return ids, only_column(wl, step), only_column(we, step), {k: kw[k] for k in ("seen", "state") if k in kw}


@pytest.mark.gpu
@pytest.mark.parametrize("lt", SAMPLER_TEMPS)
@pytest.mark.parametrize("V", tse.SIZES)
@pytest.mark.parametrize("case", tse.CASES, ids=[c[0] for c in tse.CASES])
def test_gpu_sampler_outputs_at_a_temperature(V, case, lt):
    """ids, seen and state bit-equal to the call without logp_temperature; logp_out = log_softmax(x / T) at the pick and ent_out = entropy64(x / T) at rtol = atol =
    1e-5; nothing written outside the step's column; the logits untouched."""
    x = tse.inputs(V)
    lg = torch.from_numpy(x).to(DEV)
    ids0, lp0, en0, st0 = run_ent(lg, V, case, None)
    ids, lp, en, st = run_ent(lg, V, case, lt)
    assert torch.equal(ids, ids0), "which token is sampled does not depend on logp_temperature"
    for name in st0:
        assert torch.equal(st[name], st0[name]), name
    ls, H = scaled64(V, t32(lt))
    what = f"V={V} {case[0]} logp_temperature={lt}"
    close(lp, ls[np.arange(B), ids.cpu().numpy()], what + " logp")
    close(en, H, what + " entropy")
    assert not np.array_equal(lp, lp0) and not np.array_equal(en, en0)
    assert torch.equal(lg, torch.from_numpy(x).to(DEV)), "the logits were written"


def raw_ent(name, lg, V, case, tail=(), seed=77):
    """iadr1_sample_ent / iadr1_sample_ent_t through hip.call (not the ops shortcut) -> ids, logp, ent, seen / state"""
    (Ts, k, p), kw = tse.device_args(V, case)
    ids = torch.empty(B, dtype=torch.int64, device=DEV)
    lp, en = torch.full((B, 1), SENT, dtype=F32, device=DEV), torch.full((B, 1), SENT, dtype=F32, device=DEV)
    ws = torch.empty(hip.lib().iadr1_sample_ent_workspace_bytes(B), dtype=torch.uint8, device=DEV)
    seen, state, allow, trans = kw.get("seen"), kw.get("state"), kw.get("allow"), kw.get("trans")
    hip.call(name, lg, lg.stride(0), ids, lp, 1, 1, ws, B, V, float(Ts), int(k), float(p), float(kw["min_p"]), float(kw["repetition_penalty"]), seen,
             seen.stride(0) if seen is not None else 0, int(bool(kw.get("mark_seen"))), -1, seed, 0, None, None, state, allow, allow.stride(0) if allow is not None else 0, trans,
             trans.stride(0) if trans is not None else 0, allow.shape[0] if allow is not None else 0, en, 1, 1, *tail)
    torch.cuda.synchronize()
    return ids, lp, en, seen, state


@pytest.mark.gpu
@pytest.mark.parametrize("V", tse.SIZES)
@pytest.mark.parametrize("case", tse.CASES, ids=[c[0] for c in tse.CASES])
def test_gpu_sampler_temperature_one_is_sample_ent(V, case):
    lg = torch.from_numpy(tse.inputs(V)).to(DEV)
    a, b = raw_ent("sample_ent_t", lg, V, case, (1.0,)), raw_ent("sample_ent", lg, V, case)
    for u, v, name in zip(a, b, ("ids", "logp_out", "ent_out", "seen", "state")):
        assert (u is None and v is None) or same_bits(u, v), name


@pytest.mark.gpu
@pytest.mark.parametrize("V", tse.SIZES)
@pytest.mark.parametrize("case", tse.CASES, ids=[c[0] for c in tse.CASES])
def test_gpu_sampler_half_temperature_is_sample_ent_on_doubled_logits(V, case):
    """logp_temperature = 0.5 on x at sampling temperature Ts equals sample_ent on 2 x at 2 Ts in ids, logp_out and ent_out, bit for bit (every product by 2 is exact)."""
    x = tse.inputs(V)
    lg, lg2 = torch.from_numpy(x).to(DEV), torch.from_numpy(x * np.float32(2)).to(DEV)
    (Ts, k, p), kw = tse.device_args(V, case)
    (_, _, _), kw2 = tse.device_args(V, case)
    ids, lp, en = ops.sample_ent(lg, Ts, k, p, seed=77, step=0, logp_temperature=0.5, **kw)
    ids2, lp2, en2 = ops.sample_ent(lg2, 2 * Ts, k, p, seed=77, step=0, **kw2)
    assert torch.equal(ids, ids2), case[0]
    assert same_bits(lp, lp2) and same_bits(en, en2), case[0]


@pytest.mark.gpu
def test_gpu_sampler_without_outputs_is_legal_and_is_sample_ent():
    V = tse.SIZES[1]
    lg = torch.from_numpy(tse.inputs(V)).to(DEV)
    for case in (tse.CASES[0], tse.CASES[4], tse.CASES[5]):
        args, kw = tse.device_args(V, case)
        args2, kw2 = tse.device_args(V, case)
        ids, lp, en = ops.sample_ent(lg, *args, seed=5, step=0, want_logp=False, want_ent=False, logp_temperature=0.6, **kw)
        ids2, _, _ = ops.sample_ent(lg, *args2, seed=5, step=0, want_logp=False, want_ent=False, **kw2)
        assert lp is None and en is None and torch.equal(ids, ids2)
        for name in ("seen", "state"):
            if name in kw:
                assert torch.equal(kw[name], kw2[name]), name
