"""Truncated importance weights for the rollout / trainer log-prob mismatch: iadr1_grpo_loss_is (csrc/loss.hip), ops.grpo_loss_is, GRPOArgs.rollout_is_cap /
rollout_is_level through SCGRPOEngine and SCGRPOTrainer, and the two flags of train/stage_rl/grpo_ad.py.  The ABI / argument tests need no GPU."""
import ctypes
import dataclasses
import importlib.util
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixture_util as fx  # noqa: E402
import iadr1_amd  # noqa: E402,F401
from iadr1_amd import hip, ops  # noqa: E402
from iadr1_amd.params import ParamStore, VLMConfig  # noqa: E402
from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine  # noqa: E402

DEV = "cuda"
F32 = torch.float32
CFG = VLMConfig.from_dict(fx.TINY)
BETA = 0.04
NEW_KEYS = ("rollout/is_weight_mean", "rollout/is_clipped_frac")
OLD_KEYS = ("rollout/logp_abs_diff_mean", "rollout/logp_abs_diff_max", "rollout/kl")
_WIDE = {}      # weights and loss of the sequential 3B-width step, compared by the co-scheduled case that follows it


# ---- without a GPU -----------------------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_entry_point():
    assert "iadr1_grpo_loss_is" in hip.PROTOS and hasattr(hip.lib(), "iadr1_grpo_loss_is") and hip.version() >= 112
    names = [n for _, n in hip.PROTOS["iadr1_grpo_loss_is"][1]]
    assert names[:5] == ["logp", "ref_logp", "rollout_logp", "adv", "mask"] and {"cap", "level", "w_out", "row_stats"} <= set(names)


def _raw_call(N=2, C=4, rollout=True, cap=2.0, level=0):
    """The entry point on host buffers: every case here must be refused before anything is launched."""
    L = hip.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    rc = L.iadr1_grpo_loss_is(p, p, p if rollout else None, p, p, BETA, cap, level, max(N, 1), p, p, p, p, p, p, N, C, None)
    return rc, L.iadr1_last_error().decode()


@pytest.mark.parametrize("kw,word", [({"N": 0}, "N"), ({"N": -3}, "N"), ({"rollout": False}, "rollout_logp"), ({"cap": 0.5}, "cap"), ({"cap": 0.0}, "cap"),
                                     ({"cap": float("inf")}, "cap"), ({"cap": float("nan")}, "cap"), ({"level": 2}, "level"), ({"level": -1}, "level")])
def test_bad_arguments_are_refused_on_the_host(kw, word):
    rc, msg = _raw_call(**kw)
    assert rc < 0 and "grpo_loss_is" in msg and word in msg, (rc, msg)


def test_grpo_args_refuse_a_bad_cap_or_level_when_the_engine_is_built():
    with pytest.raises(ValueError, match="rollout_is_cap"):
        SCGRPOEngine(None, None, None, GRPOArgs(rollout_is_cap=0.5))
    with pytest.raises(ValueError, match="rollout_is_cap"):
        SCGRPOEngine(None, None, None, GRPOArgs(rollout_is_cap=float("inf")))
    with pytest.raises(ValueError, match="rollout_is_level"):
        SCGRPOEngine(None, None, None, GRPOArgs(rollout_is_level="x"))
    with pytest.raises(ValueError, match="rollout_is_level"):
        SCGRPOEngine(None, None, None, GRPOArgs(rollout_is_cap=2.0, rollout_is_level="x"))
    with pytest.raises(ValueError, match="llava_rotate_right_padded_rows"):
        SCGRPOEngine(types.SimpleNamespace(is_llava=True), None, None, GRPOArgs(rollout_is_cap=2.0))
    assert GRPOArgs().rollout_is_cap == 0.0 and GRPOArgs().rollout_is_level == "token" and not GRPOArgs().wants_rollout_logps
    assert GRPOArgs(rollout_is_cap=1.0).wants_rollout_logps and GRPOArgs(rollout_logps=True).wants_rollout_logps


def test_entry_point_flags_and_config_fields():
    from iadr1_amd.trainer import GRPOConfig
    spec = importlib.util.spec_from_file_location("grpo_ad_is_flags", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "train", "stage_rl", "grpo_ad.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["--model_name_or_path", "/m", "--output_dir", "o", "--dataset_name", "d.json"]
    d = mod.build_parser().parse_args(base)
    assert d.rollout_is_cap == 0.0 and d.rollout_is_level == "token"
    a = mod.build_parser().parse_args(base + ["--rollout_is_cap", "2.5", "--rollout_is_level", "sequence"])
    assert a.rollout_is_cap == 2.5 and a.rollout_is_level == "sequence"
    with pytest.raises(SystemExit):
        mod.build_parser().parse_args(base + ["--rollout_is_level", "x"])
    c = GRPOConfig()
    assert c.rollout_is_cap == 0.0 and c.rollout_is_level == "token"
    assert {"rollout_is_cap", "rollout_is_level"} <= set(GRPOConfig.__dataclass_fields__)     # grpo_ad.main copies every parsed flag that is a GRPOConfig field


# ---- GPU, kernel level ---------------------------------------------------------------------------------------------------------------------------------

def close(got, ref, rtol, atol, what=""):
    got, ref = got.double().cpu(), ref.double().cpu()
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    assert bool((err <= tol).all()), f"{what}: max |err| {err.max().item():.4g}, worst excess {(err - tol).max().item():.4g}, max |ref| {ref.abs().max().item():.4g}"


def kernel_inputs(C, N=8, seed=0):
    """p, r, q with |p - q| up to 1.5 on the mask and q = 0 off it (the rollout's contract); prefix masks: row 0 empty, row 1 full, the others ragged."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(N, C, generator=g) * 0.3 - 2.0
    r = p + torch.randn(N, C, generator=g) * 0.1
    d = (torch.rand(N, C, generator=g) * 2 - 1) * 1.5
    adv = torch.randn(N, generator=g)
    lens = torch.randint(1, C, (N,), generator=g)
    lens[0], lens[1] = 0, C
    mask = (torch.arange(C)[None, :] < lens[:, None]).int()
    q = torch.where(mask.bool(), p - d, torch.zeros(()))
    return [t.to(DEV).contiguous() for t in (p.to(F32), r.to(F32), q.to(F32), adv.to(F32), mask)]


def restate(p, r, q, adv, mask, cap, level, n_total):
    """The definitions in float64, with autograd for d loss / d logp.  Reads the float32 inputs exactly."""
    p = p.double().cpu().requires_grad_(True)
    r, q, adv, live = r.double().cpu(), q.double().cpu(), adv.double().cpu(), mask.bool().cpu()
    m = live.double()
    cnt = m.sum(1)
    inv = torch.where(cnt > 0, 1.0 / cnt.clamp(min=1), torch.zeros(()).double())
    d = torch.where(live, p.detach() - q, torch.zeros(()).double())
    tok_ratio = torch.exp(d)
    ratio = tok_ratio if level == "token" else torch.exp((d * m).sum(1) * inv)[:, None].expand_as(d)
    w = ratio.clamp(max=cap)
    kl = torch.exp(r - p) - (r - p) - 1
    ptl = w * (-(torch.exp(p - p.detach()) * adv[:, None] - BETA * kl))
    row_loss = (ptl * m).sum(1) * inv
    (row_loss.sum() / n_total).backward()
    stats = torch.stack([(w * m).sum(1), torch.zeros_like(cnt), (d.abs() * m).sum(1), (d.abs() * m).max(1).values, ((tok_ratio - d - 1) * m).sum(1)], 1)
    lo = ((ratio > cap * (1 + 1e-4)) & live).sum(1)
    hi = ((ratio > cap * (1 - 1e-4)) & live).sum(1)
    return {"dlogp": p.grad, "kl": kl.detach(), "w": (w * m).detach(), "row_loss": row_loss.detach(), "row_kl": ((kl * m).sum(1) * inv).detach(), "stats": stats,
            "clip_lo": lo, "clip_hi": hi, "cnt": cnt}


@pytest.mark.gpu
@pytest.mark.parametrize("C", [16, 256, 300])
@pytest.mark.parametrize("level", ["token", "sequence"])
@pytest.mark.parametrize("cap", [1.0, 2.0, 1e30])
def test_kernel_against_a_float64_autograd_restatement(C, level, cap):
    """(1) dlogp, kl, w within (rtol 1e-4, atol 1e-7), the loss (batch mean and every row) within (1e-5, 1e-7): the tolerances test_hip_kernels holds iadr1_grpo_loss
    to.  The clipped count between the counts of ratio > cap (1 + 1e-4) and ratio > cap (1 - 1e-4).  The other per-row partials: sums of positive terms (sum m w,
    sum m |d|) within rtol 1e-5; max m |d| is one correctly rounded fp32 subtraction, rtol 1e-6; sum m (exp(d) - d - 1) cancels inside every term, so its bound is
    absolute per token: 4 ulp of the ratio (<= 4.5 here) plus one of d, 4e-6 x the row's live tokens, plus rtol 1e-5 for the fp32 accumulation."""
    p, r, q, adv, mask = kernel_inputs(C, seed=C)
    N = p.shape[0]
    want = restate(p, r, q, adv, mask, cap, level, N)
    dlogp, kl, row_loss, row_kl, w, stats = ops.grpo_loss_is(p, r, q, adv, mask, BETA, cap, level)
    torch.cuda.synchronize()
    print(f"[grpo_loss_is kernel] C={C} {level} cap={cap:g}: max |dlogp err| {(dlogp.double().cpu() - want['dlogp']).abs().max().item():.3e}, "
          f"max |w err| {(w.double().cpu() - want['w']).abs().max().item():.3e}, loss {row_loss.mean().item():.6e} vs {want['row_loss'].mean().item():.6e}, "
          f"clipped {int(stats[:, 1].sum().item())} in [{int(want['clip_lo'].sum())}, {int(want['clip_hi'].sum())}]")
    close(dlogp, want["dlogp"], 1e-4, 1e-7, "dlogp")
    close(kl, want["kl"], 1e-4, 1e-7, "kl")
    close(w, want["w"], 1e-4, 1e-7, "w_out")
    assert bool((w[mask == 0] == 0).all()) and bool((dlogp[mask == 0] == 0).all())
    close(row_loss.mean(), want["row_loss"].mean(), 1e-5, 1e-7, "loss")
    close(row_loss, want["row_loss"], 1e-5, 1e-7, "row loss")
    close(row_kl.mean(), want["row_kl"].mean(), 1e-5, 1e-7, "mean kl")
    st = stats.double().cpu()
    close(st[:, 0], want["stats"][:, 0], 1e-5, 0.0, "sum m w")
    close(st[:, 2], want["stats"][:, 2], 1e-5, 0.0, "sum m |d|")
    close(st[:, 3], want["stats"][:, 3], 1e-6, 0.0, "max m |d|")
    err = (st[:, 4] - want["stats"][:, 4]).abs()
    assert bool((err <= 4e-6 * want["cnt"] + 1e-5 * want["stats"][:, 4].abs()).all()), ("sum m (exp(d) - d - 1)", err.max().item())
    assert bool((st[:, 1] >= want["clip_lo"]).all()) and bool((st[:, 1] <= want["clip_hi"]).all()), (st[:, 1], want["clip_lo"], want["clip_hi"])
    assert st[0].abs().sum() == 0 and row_loss[0] == 0         # the empty row
    # a micro-batch of a larger step: the batch mean runs over n_total_rows (a power-of-two factor here, so the scale is exact)
    assert torch.equal(ops.grpo_loss_is(p, r, q, adv, mask, BETA, cap, level, n_total_rows=2 * N)[0] * 2, dlogp)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [16, 300])
@pytest.mark.parametrize("level", ["token", "sequence"])
@pytest.mark.parametrize("cap", [1.0, 2.0, 1e30])
def test_on_policy_rows_reproduce_grpo_loss_bit_for_bit(C, level, cap):
    """(2) rollout_logp == logp bitwise: exp(0) = 1 and 1 * x is exact, so the four shared outputs are torch.equal to iadr1_grpo_loss's, w is 1.0 on the mask (0 off
    it) and nothing is clipped."""
    p, r, _, adv, mask = kernel_inputs(C, seed=C + 1)
    base = ops.grpo_loss(p, r, adv, mask, BETA)
    dlogp, kl, row_loss, row_kl, w, stats = ops.grpo_loss_is(p, r, p.clone(), adv, mask, BETA, cap, level)
    for name, a, b in zip(("dlogp", "kl", "row_loss", "row_kl"), base, (dlogp, kl, row_loss, row_kl)):
        assert torch.equal(a, b), name
    assert torch.equal(w, mask.to(F32))
    cnt = mask.sum(1).to(F32)
    assert torch.equal(stats[:, 0], cnt) and bool((stats[:, 1:] == 0).all())
    # w_out is optional in the ABI: the same call without it writes the same other outputs
    out = [torch.empty_like(t) for t in (dlogp, kl, row_loss, row_kl, stats)]
    hip.call("grpo_loss_is", p, r, p.clone(), adv, mask, BETA, cap, ops.IS_LEVELS[level], p.shape[0], *out[:4], None, out[4], *p.shape)
    assert all(torch.equal(a, b) for a, b in zip(out, (dlogp, kl, row_loss, row_kl, stats)))


@pytest.mark.gpu
@pytest.mark.parametrize("level", ["token", "sequence"])
def test_two_runs_are_bit_equal(level):
    """(3) fixed-order block reductions, no float atomics."""
    p, r, q, adv, mask = kernel_inputs(300, N=64, seed=9)
    a = ops.grpo_loss_is(p, r, q, adv, mask, BETA, 2.0, level)
    b = ops.grpo_loss_is(p, r, q, adv, mask, BETA, 2.0, level)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- GPU, engine level ---------------------------------------------------------------------------------------------------------------------------------

def stores(kind=None):
    w = fx.make_weights(fx.TINY, 0)
    pol, ref = ParamStore(CFG, DEV, trainable=True, decode_weights=kind), ParamStore(CFG, DEV, trainable=False)
    pol.load_named(fx.perturb_weights(w, 1, scale=0.25))       # away from the reference: the KL term of the loss is live
    ref.load_named(w)
    return pol, ref


def tiny_batch():
    grids = [(1, 16, 12), (1, 8, 8)]
    rows = [fx.synth_prompt(gr, n, fx.TINY, 77 + i) for i, (gr, n) in enumerate(zip(grids, [5, 17]))]
    ids, mask = fx.left_pad(rows, fx.TINY["pad_token_id"])
    return {"input_ids": ids, "attention_mask": mask, "pixel_values": fx.synth_pixel_values(grids, fx.TINY, seed=77), "image_grid_thw": grids}


def reward_fn(comp):
    return np.stack([(np.asarray(comp)[:, 0] % 5).astype(np.float32), (np.asarray(comp)[:, 1] % 3).astype(np.float32)], 1)


def tiny_engine(kind=None, **kw):
    pol, ref = stores(kind)
    return SCGRPOEngine(CFG, pol, ref, GRPOArgs(num_generations=4, max_prompt_length=4096, max_completion_length=16, seed=5, **kw)), pol


def _scored(comp, **kw):
    """loss_and_grads over given completions on a fresh engine: (result, gradient buffer)."""
    eng, pol = tiny_engine(**{k: v for k, v in kw.items() if k != "rollout_logps"})
    out = eng.loss_and_grads(tiny_batch(), comp, reward_fn(comp), rollout_logps=kw.get("rollout_logps"))
    torch.cuda.synchronize()
    return out, pol.grad.clone()


@pytest.fixture(scope="module")
def tiny_base():
    """The step with the cap off: one sampled rollout of the TINY batch, then the loss and the gradients over its completions."""
    eng, pol = tiny_engine()
    comp = eng.rollout(tiny_batch())
    comp[3, 6] = CFG.eos_token_id          # one row ends early: its tail is masked
    out, grad = _scored(comp)
    assert int(out["completion_mask"].sum()) == comp.size - 9 and float(grad.abs().max()) > 0
    return comp, out, grad


@pytest.mark.gpu
def test_engine_on_policy_weights_leave_the_step_unchanged(tiny_base):
    """(4) rollout_logps = the scored log-probs themselves, cap 2: loss, kl and the gradient buffer bit-equal to the run with the cap off; mean weight 1, nothing
    clipped.  Completions without their rollout log-probs are refused."""
    comp, o0, g0 = tiny_base
    o1, g1 = _scored(comp, rollout_is_cap=2.0, rollout_logps=o0["logps"])
    m = o1["metrics"]
    assert m["loss"] == o0["metrics"]["loss"] and m["kl"] == o0["metrics"]["kl"] and torch.equal(o1["kl"], o0["kl"]) and torch.equal(o1["logps"], o0["logps"])
    assert torch.equal(g0, g1)
    assert m["rollout/is_weight_mean"] == 1.0 and m["rollout/is_clipped_frac"] == 0.0
    assert m["rollout/logp_abs_diff_mean"] == 0.0 and m["rollout/logp_abs_diff_max"] == 0.0 and m["rollout/kl"] == 0.0
    assert torch.equal(o1["rollout_is_weights"].cpu(), torch.from_numpy(o0["completion_mask"]).to(F32))
    assert not any(k in o0["metrics"] for k in NEW_KEYS + OLD_KEYS) and "rollout_is_weights" not in o0
    o2, g2 = _scored(comp, rollout_is_cap=2.0, rollout_is_level="sequence", rollout_logps=o0["logps"], micro_batch_seqs=4)
    assert torch.equal(o2["rollout_is_weights"], o1["rollout_is_weights"]) and o2["metrics"]["rollout/is_weight_mean"] == 1.0
    eng, _ = tiny_engine(rollout_is_cap=2.0)
    with pytest.raises(ValueError, match="rollout log-probs"):
        eng.loss_and_grads(tiny_batch(), comp, reward_fn(comp))
    with pytest.raises(ValueError, match="rollout log-probs"):
        eng.step(tiny_batch(), reward_fn, do_optimizer_step=False, completions=comp)


@pytest.mark.gpu
def test_engine_weight_two_doubles_the_gradient_buffer(tiny_base):
    """(5) rollout_logps = logps - ln 4, cap 2: every live ratio is 4, every live weight exactly 2.0, and a power-of-two scale commutes with every rounding
    downstream, so the gradient buffer is torch.equal to 2 x the base buffer (and the loss to 2 x the base loss)."""
    comp, o0, g0 = tiny_base
    o1, g1 = _scored(comp, rollout_is_cap=2.0, rollout_logps=o0["logps"] - math.log(4.0))
    live = torch.from_numpy(o0["completion_mask"]).bool()
    w = o1["rollout_is_weights"].cpu()
    assert bool((w[live] == 2.0).all()) and bool((w[~live] == 0).all())
    m = o1["metrics"]
    assert m["rollout/is_weight_mean"] == 2.0 and m["rollout/is_clipped_frac"] == 1.0 and abs(m["rollout/logp_abs_diff_mean"] - math.log(4.0)) < 1e-5
    assert m["loss"] == 2 * o0["metrics"]["loss"] and m["kl"] == o0["metrics"]["kl"]
    diff = (g1 != 2 * g0)
    assert not bool(diff.any()), f"{int(diff.sum())} of {g0.numel()} gradient elements are not 2 x the base; smallest base magnitude among them {g0[diff].abs().min().item():.3e}"


def _full_step(kind, **kw):
    eng, pol = tiny_engine(kind, **kw)
    out = eng.step(tiny_batch(), reward_fn, do_optimizer_step=False, return_outputs=True)
    torch.cuda.synchronize()
    return out, pol.grad.clone()


def _check_weights_against_float64(out, cap, what):
    live = torch.from_numpy(np.asarray(out["completion_mask"])).bool()
    ratio = torch.exp(out["logps"].double().cpu() - out["rollout_logps"].double().cpu())
    want = ratio.clamp(max=cap)
    w = out["rollout_is_weights"].double().cpu()
    assert bool(((w - want).abs()[live] <= 1e-4 * want[live]).all()) and bool((w[~live] == 0).all())
    m = out["metrics"]
    n = int(live.sum())
    assert abs(m["rollout/is_weight_mean"] - float(want[live].mean())) <= 1e-4 * float(want[live].mean())
    lo, hi = int((ratio[live] > cap * (1 + 1e-4)).sum()), int((ratio[live] > cap * (1 - 1e-4)).sum())
    assert lo - 0.5 <= m["rollout/is_clipped_frac"] * n <= hi + 0.5, (m["rollout/is_clipped_frac"] * n, lo, hi)
    print(f"[rollout is] {what}, cap {cap:g}: is_weight_mean {m['rollout/is_weight_mean']:.6f} is_clipped_frac {m['rollout/is_clipped_frac']:.4f} "
          f"({ {k: m[k] for k in OLD_KEYS} }; {n} live tokens)")


@pytest.mark.gpu
def test_full_step_with_fp8_decode_weights(tiny_base):
    """(6) SCGRPOEngine.step on ParamStore(decode_weights="fp8") with cap 1.0: the returned weights against min(exp(logps - rollout_logps), 1) in float64 (rtol 1e-4),
    the two metrics against the same recomputation, and gradients that differ from the same step with the cap off.  Also prints the records at cap 2 for both
    kinds of decode weights (no bound attached)."""
    o0, g0 = _full_step("fp8")
    o1, g1 = _full_step("fp8", rollout_is_cap=1.0)
    assert np.array_equal(o0["completion_ids"], o1["completion_ids"]) and torch.equal(o0["logps"], o1["logps"])
    _check_weights_against_float64(o1, 1.0, "TINY fp8")
    assert not torch.equal(g0, g1) and o1["metrics"]["rollout/is_weight_mean"] < 1.0
    assert all(np.isfinite(o1["metrics"][k]) for k in NEW_KEYS + OLD_KEYS)
    for kind in ("bf16", "fp8"):
        for level in ("token", "sequence"):
            o, _ = _full_step(kind, rollout_is_cap=2.0, rollout_is_level=level)
            if level == "token":
                _check_weights_against_float64(o, 2.0, f"TINY {kind} token")
            else:
                print(f"[rollout is] TINY {kind} sequence, cap 2: { {k: o['metrics'][k] for k in NEW_KEYS} }")
            assert all(np.isfinite(o["metrics"][k]) for k in NEW_KEYS)


def _wide_step(monkeypatch, overlap_cus, kind=None, cap=2.0):
    """The 2-layer model at Qwen2.5-VL-3B widths of test_rollout_logps_against_float64_from_the_stored_final_norm_rows, with the cap on."""
    import test_hip_model as thm
    monkeypatch.setenv("IADR1_OVERLAP_CUS", overlap_cus)
    monkeypatch.setenv("IADR1_DECODE_KS", "1,8")       # the same split of the o projection's K whatever the CU count (see that test)
    cfg = dataclasses.replace(VLMConfig.qwen25vl_3b(), num_hidden_layers=2, v_depth=2, v_fullatt=(1,))
    ref = ParamStore(cfg, DEV, trainable=False)
    ref.init_random(seed=0)
    pol = ParamStore(cfg, DEV, trainable=True, decode_weights=kind)
    pol.load_named(fx.perturb_weights({k: v.float().numpy() for k, v in ref.export_named().items()}, 1, scale=0.25))
    G, C, Bp = 8, 16, 2
    cd = thm._oracle_cfg_dict(cfg)
    grids = [(1, 16, 16), (1, 16, 12)]
    ids, mask = fx.left_pad([fx.synth_prompt(grids[0], 37, cd, 5), fx.synth_prompt(grids[1], 21, cd, 6)], cfg.pad_token_id)
    batch = {"input_ids": ids, "attention_mask": mask, "pixel_values": fx.synth_pixel_values(grids, cd, seed=5), "image_grid_thw": grids}
    eng = SCGRPOEngine(cfg, pol, ref, GRPOArgs(num_generations=G, max_prompt_length=4096, max_completion_length=C, micro_batch_seqs=Bp * G, seed=11, rollout_is_cap=cap))
    try:
        out = eng.step(batch, reward_fn, do_optimizer_step=False, return_outputs=True)
        torch.cuda.synchronize()
    except RuntimeError as exc:
        if overlap_cus != "0" and "no stream pair" in str(exc):
            pytest.skip(f"co-scheduled case NOT RUN on this box: {exc}")
        raise
    return eng, out


@pytest.mark.gpu
@pytest.mark.parametrize("overlap_cus", ["0", "64"])
def test_sequential_and_co_scheduled_steps_give_bit_equal_weights(monkeypatch, overlap_cus):
    """(7) The decode steps fill the training arena (reuse_decode) and, co-scheduled, the side stream scores the policy's rows: weights and loss bit-equal either way."""
    eng, out = _wide_step(monkeypatch, overlap_cus)
    assert eng.last_step_traced and eng.last_step_shadowed == (overlap_cus != "0")
    _check_weights_against_float64(out, 2.0, f"3B widths bf16, IADR1_OVERLAP_CUS={overlap_cus}")
    got = (out["rollout_is_weights"].cpu().numpy(), out["metrics"]["loss"])
    _WIDE[overlap_cus] = got
    if overlap_cus != "0" and "0" in _WIDE:
        assert np.array_equal(_WIDE["0"][0], got[0]) and _WIDE["0"][1] == got[1], "sequential and co-scheduled steps returned different weights or losses"


@pytest.mark.gpu
def test_wide_step_with_fp8_decode_weights(monkeypatch):
    """The same 3B-width step sampling from FP8 weights (the policy's forward then runs after the rollout, on its bf16 weights): weights against float64; records."""
    eng, out = _wide_step(monkeypatch, "0", kind="fp8")
    assert not eng.last_step_traced
    _check_weights_against_float64(out, 2.0, "3B widths fp8")
    assert out["metrics"]["rollout/logp_abs_diff_mean"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("batched", [True, False])
def test_trainer_logs_the_two_metrics(tmp_path, batched):
    """(8) GRPOConfig.rollout_is_cap through SCGRPOTrainer.training_step, three micro-batches, one rollout for all of them or one per micro-batch: every micro-batch
    logs both new metrics (and the three existing ones), finite; with the cap at 0 none is logged."""
    from iadr1_amd import rewards, rollout as ro
    from iadr1_amd.trainer import GRPOConfig, SCGRPOTrainer
    w = fx.make_weights(fx.TINY, 0)
    grids = [(1, 16, 12), (1, 8, 8), (1, 12, 12)]
    parts = []
    for i, (gr, n) in enumerate(zip(grids, [5, 17, 9])):
        ids, mask = fx.left_pad([fx.synth_prompt(gr, n, fx.TINY, 177 + i)], fx.TINY["pad_token_id"])
        parts.append({"input_ids": ids, "attention_mask": mask, "pixel_values": torch.from_numpy(fx.synth_pixel_values([gr], fx.TINY, seed=177 + i)), "image_grid_thw": [gr]})

    class Proc:
        def apply_chat_template(self, conv, add_generation_prompt=True, tokenize=False):
            return "P"

        def __call__(self, text=None, images=None, **kw):
            return parts[images[0][1]]

        def batch_decode(self, ids, skip_special_tokens=True):
            return ["<think>a</think><location>top left</location><type>scratch</type><answer>yes</answer>"] * len(ids)
    chat = [{"role": "user", "content": [{"type": "image"}, {"type": "text", "text": "?"}]}]
    rows = lambda k: [{"prompt": chat, "image": [("synthetic", k)], "solution": "<think>gt</think><location>top left</location><type>scratch</type><answer>yes</answer>"}]
    for cap, level in ((2.0, "token"), (2.0, "sequence"), (0.0, "token")):
        tr = SCGRPOTrainer((CFG, w), [rewards.accuracy_reward, rewards.consistency_reward], processing_class=Proc(), train_dataset=None,
                           args=GRPOConfig(output_dir=str(tmp_path / "out"), num_generations=4, max_completion_length=12, max_prompt_length=4096,
                                           per_device_train_batch_size=1, gradient_accumulation_steps=3, save_steps=0, batch_rollouts=batched, rollout_is_cap=cap,
                                           rollout_is_level=level))
        n0 = ro.STATS["rollouts"]
        losses = tr.training_step([rows(0), rows(1), rows(2)])
        assert ro.STATS["rollouts"] - n0 == (1 if batched else 3) and len(losses) == 3 and all(np.isfinite(l) for l in losses)
        if cap > 0:
            assert all(len(tr._metrics[k]) == 3 and all(np.isfinite(v) and v >= 0 for v in tr._metrics[k]) for k in NEW_KEYS + OLD_KEYS), dict(tr._metrics)
            assert all(0 < v <= cap for v in tr._metrics["rollout/is_weight_mean"]) and all(v <= 1 for v in tr._metrics["rollout/is_clipped_frac"])
            tr.log({"loss": float(np.mean(losses))})
            assert all(k in tr.log_history[-1] for k in NEW_KEYS + OLD_KEYS)
        else:
            assert not any(k in tr._metrics for k in NEW_KEYS + OLD_KEYS)
