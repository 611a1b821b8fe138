"""Reusing a rollout for num_iterations optimizer steps under the clipped GRPO surrogate: iadr1_grpo_loss_clip (csrc/loss.hip), ops.grpo_loss_clip,
GRPOArgs.num_iterations / epsilon / epsilon_high through SCGRPOEngine (old_logps / is_weights) and SCGRPOTrainer (training_step, train), and the three flags of
train/stage_rl/grpo_ad.py.  The ABI / argument tests need no GPU."""
import ctypes
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixture_util as fx  # noqa: E402
import iadr1_amd  # noqa: E402,F401
import test_rollout_is as tri  # noqa: E402  (kernel_inputs, close, tiny_engine, tiny_batch, reward_fn: the fixtures of the neighbouring loss kernel's tests)
from iadr1_amd import hip, ops  # noqa: E402
from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine  # noqa: E402

DEV = "cuda"
F32 = torch.float32
CFG = tri.CFG
BETA = tri.BETA
CLIP_KEYS = ("clip_ratio/low_mean", "clip_ratio/high_mean", "clip_ratio/region_mean", "policy/ratio_mean", "policy/logp_abs_diff_max")
EPS = [(0.2, 0.2), (0.2, 0.28)]
close = tri.close


# ---- without a GPU -----------------------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_entry_point():
    """(1)"""
    assert "iadr1_grpo_loss_clip" in hip.PROTOS and hasattr(hip.lib(), "iadr1_grpo_loss_clip") and hip.version() >= 113
    names = [n for _, n in hip.PROTOS["iadr1_grpo_loss_clip"][1]]
    assert names[:6] == ["logp", "old_logp", "ref_logp", "adv", "mask", "w"] and {"eps_low", "eps_high", "n_total_rows", "row_stats"} <= set(names)


def _raw_call(N=2, C=4, old=True, stats=True, eps_low=0.2, eps_high=0.2, n_total=None):
    """The entry point on host buffers: every case here must be refused before anything is launched."""
    L = hip.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    rc = L.iadr1_grpo_loss_clip(p, p if old else None, p, p, p, None, BETA, eps_low, eps_high, max(N, 1) if n_total is None else n_total, p, p, p, p, p if stats else None, N, C,
                                None)
    return rc, L.iadr1_last_error().decode()


@pytest.mark.parametrize("kw,word", [({"N": 0}, "N"), ({"N": -3}, "N"), ({"old": False}, "old_logp"), ({"stats": False}, "row_stats"),
                                     ({"eps_low": -0.1}, "eps_low"), ({"eps_low": 1.0}, "eps_low"), ({"eps_low": float("nan")}, "eps_low"), ({"eps_low": float("inf")}, "eps_low"),
                                     ({"eps_high": -0.1}, "eps_high"), ({"eps_high": float("inf")}, "eps_high"), ({"eps_high": float("nan")}, "eps_high"),
                                     ({"C": 0}, "C"), ({"C": -1}, "C"), ({"N": 4, "n_total": 3}, "n_total_rows")])
def test_bad_arguments_are_refused_on_the_host(kw, word):
    """(2)"""
    rc, msg = _raw_call(**kw)
    assert rc < 0 and "grpo_loss_clip" in msg and word in msg, (rc, msg)


def test_args_config_and_flags():
    """(3)"""
    from iadr1_amd.trainer import GRPOConfig, SCGRPOTrainer
    for cls in (GRPOArgs, GRPOConfig):
        d = cls()
        assert d.num_iterations == 1 and d.epsilon == 0.2 and d.epsilon_high is None
    bad = [("num_iterations", 0), ("num_iterations", -2), ("epsilon", -0.1), ("epsilon", 1.0), ("epsilon", float("nan")), ("epsilon", float("inf")),
           ("epsilon_high", -0.1), ("epsilon_high", float("inf")), ("epsilon_high", float("nan"))]
    for field, value in bad:
        with pytest.raises(ValueError, match=field):
            SCGRPOEngine(None, None, None, GRPOArgs(**{field: value}))
        with pytest.raises(ValueError, match=field):
            SCGRPOTrainer((CFG, None), [], processing_class=object(), args=GRPOConfig(**{field: value}))
    with pytest.raises(ValueError, match="save_steps"):
        SCGRPOTrainer((CFG, None), [], processing_class=object(), args=GRPOConfig(save_steps=3, num_iterations=2))
    spec = importlib.util.spec_from_file_location("grpo_ad_clip_flags", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "train", "stage_rl", "grpo_ad.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    base = ["--model_name_or_path", "/m", "--output_dir", "o", "--dataset_name", "d.json"]
    d = mod.build_parser().parse_args(base)
    assert d.num_iterations == 1 and d.epsilon == 0.2 and d.epsilon_high is None
    a = mod.build_parser().parse_args(base + ["--num_iterations", "4", "--epsilon", "0.1", "--epsilon_high", "0.28"])
    assert a.num_iterations == 4 and a.epsilon == 0.1 and a.epsilon_high == 0.28
    assert {"num_iterations", "epsilon", "epsilon_high"} <= set(GRPOConfig.__dataclass_fields__)      # grpo_ad.main copies every parsed flag that is a GRPOConfig field


# ---- GPU, kernel level ---------------------------------------------------------------------------------------------------------------------------------

def clip_inputs(C, N=8, seed=0):
    """p, r, adv, mask of kernel_inputs; old = p - d with d uniform in +-0.5 (ratios 0.6 .. 1.65), everywhere (the mask decides what is read)."""
    p, r, _, adv, mask = tri.kernel_inputs(C, N=N, seed=seed)
    g = torch.Generator().manual_seed(seed + 1000)
    d = (torch.rand(N, C, generator=g) - 0.5).to(F32)
    w = (0.5 + 1.5 * torch.rand(N, C, generator=g)).to(F32)
    return p, (p.cpu() - d).to(DEV).contiguous(), r, adv, mask, w.to(DEV).contiguous()


def _near_a_bound(p, old, mask, el, eh):
    ratio = torch.exp(p.double().cpu() - old.double().cpu())
    return mask.bool().cpu() & (((ratio / (1 - el) - 1).abs() < 1e-3) | ((ratio / (1 + eh) - 1).abs() < 1e-3))


def off_the_bounds(p, old, mask, el, eh):
    """No live token within 1e-3 (relative) of a clip bound: such a token's old log-prob moves by 0.01 until none is left, so the float32 kernel and the float64
    restatement agree on every token's side and the clipped counts compare exactly.  Returns (old, tokens moved)."""
    old, moved = old.clone(), 0
    for _ in range(100):
        near = _near_a_bound(p, old, mask, el, eh)
        if not bool(near.any()):
            break
        moved += int(near.sum())
        old[near.to(old.device)] -= 0.01
    assert not bool(_near_a_bound(p, old, mask, el, eh).any())
    return old, moved


def restate(p, old, r, adv, mask, w, el, eh, n_total):
    """The clipped surrogate of trl's GRPOTrainer (loss_type "grpo") in float64, with autograd for d loss / d logp.  Reads the float32 inputs exactly."""
    p = p.double().cpu().requires_grad_(True)
    live = mask.bool().cpu()
    m = live.double()
    old, r, A = torch.where(live, old.double().cpu(), p.detach()), r.double().cpu(), adv.double().cpu()[:, None]
    cnt = m.sum(1)
    ratio = torch.exp(p - old)
    clamped = torch.clamp(ratio, 1 - el, 1 + eh)
    kl = torch.exp(r - p) - (r - p) - 1
    ptl = -torch.min(ratio * A, clamped * A) + BETA * kl
    if w is not None:
        ptl = w.double().cpu() * ptl
    row_loss = (ptl * m).sum(1) / cnt.clamp(min=1.0)
    (row_loss.sum() / n_total).backward()
    rt, d = ratio.detach(), (p.detach() - old).abs()
    low, high = (rt < 1 - el) & (A < 0) & live, (rt > 1 + eh) & (A > 0) & live
    stats = torch.stack([low.sum(1).double(), high.sum(1).double(), (rt * m).sum(1), (d * m).max(1).values], 1)
    return {"dlogp": p.grad, "kl": kl.detach(), "row_loss": row_loss.detach(), "row_kl": ((kl.detach() * m).sum(1) / cnt.clamp(min=1.0)), "stats": stats, "cnt": cnt}


def check_against(want, got, mask, what):
    dlogp, kl, row_loss, row_kl, stats = got
    close(dlogp, want["dlogp"], 1e-4, 1e-7, f"{what}: dlogp")
    close(kl, want["kl"], 1e-4, 1e-7, f"{what}: kl")
    close(row_loss, want["row_loss"], 1e-5, 1e-7, f"{what}: row loss")
    close(row_loss.mean(), want["row_loss"].mean(), 1e-5, 1e-7, f"{what}: loss")
    close(row_kl, want["row_kl"], 1e-5, 1e-7, f"{what}: row kl")
    st = stats.double().cpu()
    assert torch.equal(st[:, :2], want["stats"][:, :2]), (what, st[:, :2], want["stats"][:, :2])
    close(st[:, 2], want["stats"][:, 2], 1e-5, 0.0, f"{what}: sum m r")
    close(st[:, 3], want["stats"][:, 3], 1e-6, 0.0, f"{what}: max m |d|")
    assert bool((dlogp[mask == 0] == 0).all())
    assert st[0].abs().sum() == 0 and row_loss[0] == 0 and row_kl[0] == 0         # the empty row


@pytest.mark.gpu
@pytest.mark.parametrize("C", [16, 256, 300])
@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("weighted", [False, True])
def test_kernel_against_a_float64_autograd_restatement(C, eps, weighted):
    """(4) dlogp, kl within (rtol 1e-4, atol 1e-7); row and batch loss, row_kl within (1e-5, 1e-7): the tolerances iadr1_grpo_loss and iadr1_grpo_loss_is are held
    to.  Clipped counts equal (no live token sits within 1e-3 of a bound), sum m r within rtol 1e-5 (positive terms), max m |d| within 1e-6 (one fp32 subtraction)."""
    el, eh = eps
    p, old, r, adv, mask, w = clip_inputs(C, seed=C)
    old, moved = off_the_bounds(p, old, mask, el, eh)
    w = w if weighted else None
    N = p.shape[0]
    want = restate(p, old, r, adv, mask, w, el, eh, N)
    got = ops.grpo_loss_clip(p, old, r, adv, mask, BETA, el, eh, w=w)
    torch.cuda.synchronize()
    n_low, n_high = int(want["stats"][:, 0].sum()), int(want["stats"][:, 1].sum())
    print(f"[grpo_loss_clip kernel] C={C} eps=({el}, {eh}) w={'yes' if weighted else 'NULL'}: {moved} tokens moved off a bound, low {n_low} high {n_high} of {int(want['cnt'].sum())}; "
          f"max |dlogp err| {(got[0].double().cpu() - want['dlogp']).abs().max().item():.3e}, loss {got[2].mean().item():.6e} vs {want['row_loss'].mean().item():.6e}")
    assert n_low > 0 and n_high > 0
    check_against(want, got, mask, "clip")
    # a micro-batch of a larger step: the batch mean runs over n_total_rows (a power-of-two factor here, so the scale is exact)
    assert torch.equal(ops.grpo_loss_clip(p, old, r, adv, mask, BETA, el, eh, w=w, n_total_rows=2 * N)[0] * 2, got[0])


@pytest.mark.gpu
@pytest.mark.parametrize("C", [16, 300])
def test_old_logp_off_the_mask_is_never_read_into_a_sum(C):
    """(5) NaN at every masked position of old_logp: the outputs are torch.equal to the clean call's."""
    p, old, r, adv, mask, w = clip_inputs(C, seed=C + 2)
    clean = ops.grpo_loss_clip(p, old, r, adv, mask, BETA, 0.2, 0.28, w=w)
    dirty = torch.where(mask.bool(), old, torch.full_like(old, float("nan")))
    assert bool(torch.isnan(dirty).any())
    got = ops.grpo_loss_clip(p, dirty, r, adv, mask, BETA, 0.2, 0.28, w=w)
    for name, a, b in zip(("dlogp", "kl", "row_loss", "row_kl", "row_stats"), clean, got):
        assert torch.equal(a, b), name


@pytest.mark.gpu
@pytest.mark.parametrize("C", [16, 300])
@pytest.mark.parametrize("eps", [(0.2, 0.2), (0.0, 0.0)])
def test_on_policy_rows_reproduce_grpo_loss_bit_for_bit(C, eps):
    """(6) old_logp == logp bitwise: exp(0) = 1, clamp(1) = 1 and 1 * x is exact, so the four shared outputs are torch.equal to iadr1_grpo_loss's and, with the
    w_out of an iadr1_grpo_loss_is call as w, to that call's.  Nothing is clipped (the inequalities are strict), sum m r is the live count, max m |d| is 0."""
    p, r, q, adv, mask = tri.kernel_inputs(C, seed=C + 1)
    cnt = mask.sum(1).to(F32)
    base = ops.grpo_loss(p, r, adv, mask, BETA)
    got = ops.grpo_loss_clip(p, p.clone(), r, adv, mask, BETA, *eps)
    for name, a, b in zip(("dlogp", "kl", "row_loss", "row_kl"), base, got):
        assert torch.equal(a, b), name
    st = got[4]
    assert bool((st[:, :2] == 0).all()) and torch.equal(st[:, 2], cnt) and bool((st[:, 3] == 0).all())
    for level in ("token", "sequence"):
        weighted = ops.grpo_loss_is(p, r, q, adv, mask, BETA, 2.0, level)
        got = ops.grpo_loss_clip(p, p.clone(), r, adv, mask, BETA, *eps, w=weighted[4])
        for name, a, b in zip(("dlogp", "kl", "row_loss", "row_kl"), weighted, got):
            assert torch.equal(a, b), (level, name)
        assert bool((got[4][:, :2] == 0).all()) and torch.equal(got[4][:, 2], cnt) and bool((got[4][:, 3] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("C", [16, 300])
@pytest.mark.parametrize("side", ["high", "low"])
def test_saturated_rows_keep_only_the_kl_gradient(C, side):
    """(7) ratio 2 with positive advantages (0.5 with negative ones): every live token is clipped on that side, the advantage term has no gradient and dlogp is
    the beta-only gradient m / cnt / N * beta (1 - exp(ref - logp)), in float64 at the tolerances of (4)."""
    p, _, r, adv, mask, _ = clip_inputs(C, seed=C + 3)
    sign = 1.0 if side == "high" else -1.0
    adv = sign * (adv.abs() + 0.1)
    old = p - sign * math.log(2.0)
    N = p.shape[0]
    want = restate(p, old, r, adv, mask, None, 0.2, 0.2, N)
    got = ops.grpo_loss_clip(p, old, r, adv, mask, BETA, 0.2, 0.2)
    check_against(want, got, mask, side)
    cnt = mask.sum(1).to(F32)
    col = 1 if side == "high" else 0
    assert torch.equal(got[4][:, col], cnt) and bool((got[4][:, 1 - col] == 0).all())
    m = mask.double().cpu()
    kl_only = m / m.sum(1).clamp(min=1.0)[:, None] / N * BETA * (1 - torch.exp(r.double().cpu() - p.double().cpu()))
    close(got[0], kl_only, 1e-4, 1e-7, "beta-only gradient")


@pytest.mark.gpu
def test_two_runs_are_bit_equal():
    """(8) fixed-order block reductions, no float atomics."""
    p, old, r, adv, mask, w = clip_inputs(300, N=64, seed=9)
    a = ops.grpo_loss_clip(p, old, r, adv, mask, BETA, 0.2, 0.28, w=w)
    b = ops.grpo_loss_clip(p, old, r, adv, mask, BETA, 0.2, 0.28, w=w)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- GPU, engine level ---------------------------------------------------------------------------------------------------------------------------------

def _stepped(comp, **kw):
    """SCGRPOEngine.step over given completions on a fresh engine (same weights every time): (result, gradient buffer, engine).  Keyword arguments that step
    knows are handed to it, the others build the GRPOArgs."""
    call = {k: kw.pop(k) for k in ("rollout_logps", "ref_logps", "old_logps", "is_weights") if k in kw}
    eng, pol = tri.tiny_engine(**kw)
    out = eng.step(tri.tiny_batch(), tri.reward_fn, do_optimizer_step=False, return_outputs=True, completions=comp, **call)
    torch.cuda.synchronize()
    return out, pol.grad.clone(), eng


def _scored(comp, patch=None, **kw):
    """loss_and_grads over given completions on a fresh engine: (result, gradient buffer)."""
    call = {k: kw.pop(k) for k in ("ref_logps", "old_logps", "is_weights") if k in kw}
    eng, pol = tri.tiny_engine(**kw)
    if patch is not None:
        patch(eng)
    out = eng.loss_and_grads(tri.tiny_batch(), comp, tri.reward_fn(comp), **call)
    torch.cuda.synchronize()
    return out, pol.grad.clone()


@pytest.fixture(scope="module")
def tiny_base():
    """One sampled rollout of the TINY batch, then the loss and the gradients over its completions (today's loss, no reuse)."""
    eng, _ = tri.tiny_engine()
    comp = eng.rollout(tri.tiny_batch())
    comp[3, 6] = CFG.eos_token_id          # one row ends early: its tail is masked
    out, grad = _scored(comp)
    assert int(out["completion_mask"].sum()) == comp.size - 9 and float(grad.abs().max()) > 0
    return comp, out, grad


@pytest.mark.gpu
def test_iteration_zero_is_todays_step():
    """(9) num_iterations only changes what the caller does with the step's outputs: one full step (rollout included) of an engine built with 2 and of one built
    with 1 gives the same completions and torch.equal log-probs, loss, kl and gradient buffer."""
    res = []
    for mu in (1, 2):
        eng, pol = tri.tiny_engine(num_iterations=mu)
        out = eng.step(tri.tiny_batch(), tri.reward_fn, do_optimizer_step=False, return_outputs=True)
        torch.cuda.synchronize()
        res.append((out, pol.grad.clone()))
    (o1, g1), (o2, g2) = res
    assert np.array_equal(o1["completion_ids"], o2["completion_ids"]) and torch.equal(o1["logps"], o2["logps"]) and torch.equal(o1["kl"], o2["kl"])
    assert o1["metrics"]["loss"] == o2["metrics"]["loss"] and o1["metrics"]["kl"] == o2["metrics"]["kl"] and torch.equal(g1, g2)
    assert not any(k in o2["metrics"] for k in CLIP_KEYS) and "old_logps" not in o2


def _no_reference_forward(eng):
    def refuse(*a, **k):
        raise AssertionError("the reference forward ran in a reuse call")
    eng.ref.text_forward = refuse
    eng.ref.vision_forward = refuse


@pytest.mark.gpu
@pytest.mark.parametrize("mbs", [16, 4])
def test_reuse_at_unchanged_weights_is_the_base_step(tiny_base, mbs):
    """(10) old_logps = the log-probs the base step scored, ref_logps = its reference log-probs, the reference forward patched to raise: loss, kl and the gradient
    buffer torch.equal to the base step's; nothing clipped, mean ratio exactly 1."""
    comp, o0, g0 = tiny_base
    if mbs != 16:
        o0, g0 = _scored(comp, micro_batch_seqs=mbs)
    o1, g1 = _scored(comp, patch=_no_reference_forward, micro_batch_seqs=mbs, old_logps=o0["logps"], ref_logps=o0["ref_logps"])
    m = o1["metrics"]
    assert m["loss"] == o0["metrics"]["loss"] and m["kl"] == o0["metrics"]["kl"] and torch.equal(o1["kl"], o0["kl"]) and torch.equal(o1["logps"], o0["logps"])
    assert torch.equal(g0, g1)
    assert m["clip_ratio/low_mean"] == 0.0 and m["clip_ratio/high_mean"] == 0.0 and m["clip_ratio/region_mean"] == 0.0
    assert m["policy/ratio_mean"] == 1.0 and m["policy/logp_abs_diff_max"] == 0.0
    assert torch.equal(o1["old_logps"], o0["logps"]) and not any(k.startswith("rollout/") for k in m)


@pytest.mark.gpu
def test_shifted_old_logps_clip_the_rows_with_positive_advantage(tiny_base):
    """(11) old_logps = logps - ln 2, epsilon 0.2: every ratio is 2, so the high-clipped tokens are the live tokens of the rows with a positive advantage and no
    token is low-clipped; the three clip metrics equal the float64 recomputation from the returned tensors (to the rounding of one fp32 division), and the
    gradient buffer differs from the base step's."""
    comp, o0, g0 = tiny_base
    o1, g1 = _scored(comp, old_logps=o0["logps"] - math.log(2.0), ref_logps=o0["ref_logps"])
    live = torch.from_numpy(np.asarray(o1["completion_mask"])).bool()
    ratio = torch.exp(o1["logps"].double().cpu() - o1["old_logps"].double().cpu())
    A = o1["advantages"].double().cpu()[:, None]
    n = float(live.sum())
    low, high = float(((ratio < 0.8) & (A < 0) & live).sum()) / n, float(((ratio > 1.2) & (A > 0) & live).sum()) / n
    m = o1["metrics"]
    print(f"[grpo clip engine] ratio 2: low {m['clip_ratio/low_mean']:.6f} high {m['clip_ratio/high_mean']:.6f} region {m['clip_ratio/region_mean']:.6f} "
          f"(float64: {low:.6f} {high:.6f}); ratio_mean {m['policy/ratio_mean']:.6f} logp_abs_diff_max {m['policy/logp_abs_diff_max']:.6f}")
    assert low == 0.0 and high == float((live & (A > 0)).sum()) / n and 0 < high < 1
    assert m["clip_ratio/low_mean"] == 0.0 and abs(m["clip_ratio/high_mean"] - high) <= 1e-6 and abs(m["clip_ratio/region_mean"] - high) <= 1e-6
    assert abs(m["policy/ratio_mean"] - 2.0) <= 1e-5 and abs(m["policy/logp_abs_diff_max"] - math.log(2.0)) <= 1e-5
    assert not torch.equal(g0, g1)


@pytest.mark.gpu
def test_reuse_takes_the_cached_importance_weights(tiny_base):
    """(12) rollout_is_cap 2, num_iterations 2: the step that sampled weights its loss by min(exp(scored - sampled), 2); the reuse call is handed those weights
    (not the rollout log-probs) and, at unchanged weights, gives torch.equal loss, kl and gradient buffer.  Without is_weights it is refused."""
    comp, o0, _ = tiny_base
    g = torch.Generator().manual_seed(3)
    sampled = o0["logps"] + (2 * torch.rand(o0["logps"].shape, generator=g) - 1).to(DEV)       # ratios 0.37 .. 2.7: some weights are capped
    o1, g1, _ = _stepped(comp, rollout_is_cap=2.0, num_iterations=2, rollout_logps=sampled)
    w = o1["rollout_is_weights"]
    live = torch.from_numpy(np.asarray(o1["completion_mask"])).bool()
    assert float(w.cpu()[live].max()) == 2.0 and float(w.cpu()[live].min()) < 1.0
    o2, g2, eng = _stepped(comp, rollout_is_cap=2.0, num_iterations=2, old_logps=o1["logps"], ref_logps=o1["ref_logps"], is_weights=w)
    assert o2["metrics"]["loss"] == o1["metrics"]["loss"] and o2["metrics"]["kl"] == o1["metrics"]["kl"] and torch.equal(g1, g2)
    assert o2["metrics"]["clip_ratio/region_mean"] == 0.0 and o2["metrics"]["policy/ratio_mean"] == 1.0 and not any(k.startswith("rollout/") for k in o2["metrics"])
    with pytest.raises(ValueError, match="is_weights"):
        eng.step(tri.tiny_batch(), tri.reward_fn, do_optimizer_step=False, completions=comp, old_logps=o1["logps"], ref_logps=o1["ref_logps"])
    with pytest.raises(ValueError, match="is_weights"):
        eng.loss_and_grads(tri.tiny_batch(), comp, tri.reward_fn(comp), old_logps=o1["logps"], ref_logps=o1["ref_logps"])


# ---- GPU, trainer level --------------------------------------------------------------------------------------------------------------------------------

GRIDS = [(1, 16, 12), (1, 8, 8), (1, 12, 12)]
CHAT = [{"role": "user", "content": [{"type": "image"}, {"type": "text", "text": "?"}]}]


def _row(k):
    return {"prompt": CHAT, "image": [("synthetic", k)], "solution": "<think>gt</think><location>top left</location><type>scratch</type><answer>yes</answer>"}


def _trainer(tmp_path, calls, **cfg):
    """SCGRPOTrainer on the TINY model with a stub processor (three synthetic prompts) and two reward functions that count their calls (one of the
    reference's plug-ins, one that tells the rows of a group apart)."""
    from iadr1_amd import rewards
    from iadr1_amd.trainer import GRPOConfig, SCGRPOTrainer
    parts = []
    for i, (gr, n) in enumerate(zip(GRIDS, [5, 17, 9])):
        ids, mask = fx.left_pad([fx.synth_prompt(gr, n, fx.TINY, 177 + i)], fx.TINY["pad_token_id"])
        parts.append({"input_ids": ids, "attention_mask": mask, "pixel_values": torch.from_numpy(fx.synth_pixel_values([gr], fx.TINY, seed=177 + i)), "image_grid_thw": [gr]})

    class Proc:
        def apply_chat_template(self, conv, add_generation_prompt=True, tokenize=False):
            return "P"

        def __call__(self, text=None, images=None, **kw):
            return parts[images[0][1]]

        def batch_decode(self, ids, skip_special_tokens=True):
            return ["<think>a</think><location>top left</location><type>scratch</type><answer>yes</answer>"] * len(ids)

    def accuracy(**kw):
        calls["rewards"] += 1
        return rewards.accuracy_reward(**kw)

    def spread(completions, **kw):
        """0, 1, 2, 3 within every group: the stub decodes every completion to the same text, and with equal rewards (zero advantages) on a policy that still equals
        its reference (zero KL) the gradient would be exactly zero and no step would move the weights."""
        calls["rewards"] += 1
        return [float(i % 4) for i in range(len(completions))]
    # learning rate 1e-3: one AdamW step must move the bf16 weights (at the default 1e-6 an update is far below half a bf16 ulp of these weights)
    args = dict(output_dir=str(tmp_path / "out"), num_generations=4, max_completion_length=12, max_prompt_length=4096, per_device_train_batch_size=1, save_steps=0,
                learning_rate=1e-3)
    args.update(cfg)
    tr = SCGRPOTrainer((CFG, fx.make_weights(fx.TINY, 0)), [accuracy, spread], processing_class=Proc(), train_dataset=args.pop("train_dataset", None), args=GRPOConfig(**args))
    fwd = tr.engine.ref.text_forward

    def counted(*a, **k):
        calls["ref_forward"] += 1
        return fwd(*a, **k)
    tr.engine.ref.text_forward = counted
    return tr


@pytest.mark.gpu
@pytest.mark.parametrize("batched", [True, False])
def test_trainer_reuses_the_rollout_every_second_step(tmp_path, batched):
    """(13) num_iterations 2, three micro-batches: step 0 rolls out (once, or once per micro-batch), step 1 runs no rollout, no reward function and no reference
    forward and logs kl and the five new keys per micro-batch (nothing under reward), step 2 rolls out again.  With num_iterations 1 no new key appears."""
    from iadr1_amd import rollout as ro
    calls = {"rewards": 0, "ref_forward": 0}
    tr = _trainer(tmp_path, calls, num_iterations=2, gradient_accumulation_steps=3, batch_rollouts=batched)
    micro = [[_row(0)], [_row(1)], [_row(2)]]
    n0 = ro.STATS["rollouts"]
    losses = tr.training_step(micro)
    assert ro.STATS["rollouts"] - n0 == (1 if batched else 3) and len(losses) == 3 and all(np.isfinite(l) for l in losses)
    assert calls["rewards"] == 6 and len(tr._metrics["reward"]) == 3 and len(tr._metrics["kl"]) == 3 and not any(k in tr._metrics for k in CLIP_KEYS)
    assert all(isinstance(g[k], torch.Tensor) and g[k].is_cuda for g in tr._generation for k in ("old_logps", "ref_logps"))
    n1, before = ro.STATS["rollouts"], dict(calls)
    losses = tr.training_step(micro)
    assert ro.STATS["rollouts"] == n1 and calls == before and len(losses) == 3 and all(np.isfinite(l) for l in losses)
    assert tr.state.global_step == 2 and len(tr._metrics["reward"]) == 3 and len(tr._metrics["completion_length"]) == 3 and len(tr._metrics["kl"]) == 6
    assert all(len(tr._metrics[k]) == 3 and all(np.isfinite(v) for v in tr._metrics[k]) for k in CLIP_KEYS), dict(tr._metrics)
    assert all(0.0 <= v <= 1.0 for k in CLIP_KEYS[:3] for v in tr._metrics[k]) and all(v > 0 for v in tr._metrics["policy/logp_abs_diff_max"])
    print(f"[grpo clip trainer] batched={batched}: " + ", ".join(f"{k} {np.mean(tr._metrics[k]):.4g}" for k in CLIP_KEYS))
    tr.log({"loss": float(np.mean(losses))})
    assert all(k in tr.log_history[-1] for k in CLIP_KEYS)
    tr.training_step(micro)
    assert ro.STATS["rollouts"] - n1 == (1 if batched else 3) and calls["rewards"] == 12 and len(tr._metrics["reward"]) == 3
    tr1 = _trainer(tmp_path, calls, num_iterations=1, gradient_accumulation_steps=3, batch_rollouts=batched)
    n2 = ro.STATS["rollouts"]
    tr1.training_step(micro)
    tr1.training_step(micro)
    assert ro.STATS["rollouts"] - n2 == (2 if batched else 6) and not any(k in tr1._metrics for k in CLIP_KEYS) and not tr1._generation


@pytest.mark.gpu
def test_train_takes_num_iterations_steps_per_generation(tmp_path):
    """(14) two rows, batch 1, no accumulation, one epoch, num_iterations 2: four optimizer steps over two rollouts, a log line each; a checkpoint written at an odd
    step cannot be resumed from."""
    from iadr1_amd import rollout as ro
    from iadr1_amd.trainer import save_training_state
    calls = {"rewards": 0, "ref_forward": 0}
    tr = _trainer(tmp_path, calls, num_iterations=2, gradient_accumulation_steps=1, num_train_epochs=1, logging_steps=1, train_dataset=[_row(0), _row(1)])
    n0 = ro.STATS["rollouts"]
    hist = tr.train()
    assert tr.state.global_step == 4 and ro.STATS["rollouts"] - n0 == 2 and len(hist) == 4 and calls["rewards"] == 4
    assert [h["step"] for h in hist] == [1, 2, 3, 4] and [h["epoch"] for h in hist] == [0.25, 0.5, 0.75, 1.0]
    assert all(("reward" in h) == (i % 2 == 0) and ("clip_ratio/region_mean" in h) == (i % 2 == 1) and "kl" in h for i, h in enumerate(hist))
    ck = str(tmp_path / "checkpoint-3")
    save_training_state(tr.policy, ck, tr.engine.opt_step, 3)
    with pytest.raises(ValueError, match="num_iterations"):
        tr.train(resume_from_checkpoint=ck)
