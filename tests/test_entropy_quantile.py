"""top_entropy_quantile (trl's name): the advantage term of the loss trained on the highest-entropy share of the live completion tokens only --
sc_grpo.entropy_keep_mask, iadr1_grpo_loss_sel (csrc/loss.hip: the SEL parameter of the three loss kernels), ops.grpo_loss_ex(sel=...), GRPOArgs / SCGRPOEngine,
GRPOConfig / SCGRPOTrainer and the two flags of train/stage_rl/grpo_ad.py.  The float64 restatement of the gated objective lives here; inputs, forms, row scales
and tolerances are those tests/test_grpo_objective.py holds iadr1_grpo_loss_ex to."""
import os
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iadr1_amd  # noqa: E402,F401
import test_grpo_objective as tgo  # noqa: E402  (kernel_inputs, form_args, scales, trl_loss, close, the constants; through it test_rollout_is's TINY engine helpers)
from iadr1_amd import ops  # noqa: E402
from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine, check_entropy_args, entropy_keep_mask  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
F32 = torch.float32
BETA, CAP, EL, EH = tgo.BETA, tgo.CAP, tgo.EL, tgo.EH
close = tgo.close
tri = tgo.tri


# ---- without a GPU -------------------------------------------------------------------------------------------------------------------------------------------

def numpy_keep(ent, live, rho):
    """trl's get_high_entropy_mask in numpy: threshold = the (1 - rho) quantile (linear interpolation) of the live entropies as float32, ties kept."""
    e = ent.astype(np.float32)[live]
    if e.size == 0:
        return np.zeros_like(live), np.inf
    tau = np.quantile(e, np.float32(1.0 - rho), method="linear")
    return live & (ent.astype(np.float32) >= np.float32(tau)), float(tau)


def mask_inputs(kind):
    g = torch.Generator().manual_seed(3)
    N, C = 6, 11
    ent = (torch.rand(N, C, generator=g) * 3).to(F32)
    lens = torch.tensor([0, 11, 4, 7, 1, 9])
    live = torch.arange(C)[None, :] < lens[:, None]
    if kind == "ties":                     # a quarter of the live tokens share one value, and that value is where several of the thresholds fall
        ent = (ent * 2).round() / 2
    elif kind == "dead":
        live = torch.zeros_like(live)
    elif kind == "one":
        live = torch.zeros_like(live)
        live[3, 2] = True
    ent = torch.where(live, ent, torch.full_like(ent, 99.0))       # what sits at a dead position (here: larger than every live entropy) must not matter
    return ent, live


@pytest.mark.parametrize("kind", ["plain", "ties", "dead", "one"])
@pytest.mark.parametrize("rho", [0.0, 0.2, 0.5, 1.0])
def test_keep_mask_against_numpy(kind, rho):
    ent, live = mask_inputs(kind)
    keep, tau = entropy_keep_mask(ent, live, rho)
    want, wtau = numpy_keep(ent.numpy(), live.numpy(), rho)
    assert keep.dtype == torch.bool and tuple(keep.shape) == tuple(ent.shape) and np.array_equal(keep.numpy(), want), (kind, rho, float(tau), wtau)
    assert not bool((keep & ~live).any())
    n_live, n_keep = int(live.sum()), int(keep.sum())
    if kind == "dead":
        assert n_keep == 0 and float(tau) == float("inf")
        return
    assert abs(float(tau) - wtau) <= 1e-6 * max(1.0, abs(wtau))
    ties = int(((ent == float(np.float32(wtau))) & live).sum())
    assert n_keep >= max(1, int(np.floor(rho * n_live))) and n_keep <= int(np.ceil(rho * n_live)) + max(ties, 1), (n_keep, n_live, ties)
    if rho == 1.0:
        assert torch.equal(keep, live)
    if rho == 0.0:
        assert torch.equal(keep, live & (ent >= ent[live].max()))
    if kind == "ties" and rho in (0.2, 0.5):
        assert ties > 1 and bool(keep[(ent == float(np.float32(wtau))) & live].all()), "ties at the threshold are kept"
    # a host-resident mask (what the engine hands in) gives the same result
    k2, t2 = entropy_keep_mask(ent, live.numpy(), rho)
    assert torch.equal(k2, keep) and float(t2) == float(tau)
    with pytest.raises(ValueError, match="rho"):
        entropy_keep_mask(ent, live, 1.5)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def rank_inputs(rank):
    """Rank 0 draws its entropies from [0, 1), rank 1 from [2, 3): each rank's own quantile is far from the quantile of both together."""
    g = torch.Generator().manual_seed(40 + rank)
    N, C = 4, 9
    ent = (torch.rand(N, C, generator=g) + 2.0 * rank).to(F32)
    live = torch.arange(C)[None, :] < torch.tensor([9, 3, 0, 6] if rank == 0 else [5, 9, 8, 1])[:, None]
    return ent, live


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import iadr1_amd  # noqa: F401
    from iadr1_amd.sc_grpo import entropy_keep_mask as ekm
    ent, live = rank_inputs(rank)
    out = []
    for rho in (0.2, 0.5):
        keep, tau = ekm(ent, live, rho, group=dist.group.WORLD)
        _, own = ekm(ent, live, rho)
        out.append((rho, keep.numpy(), float(tau), float(own)))
    q.put((rank, out))
    dist.destroy_process_group()


def test_two_ranks_share_the_threshold_of_all_live_tokens():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=180) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ins = [rank_inputs(r) for r in range(world)]
    ent_all, live_all = torch.cat([e for e, _ in ins]).numpy(), torch.cat([l for _, l in ins]).numpy()
    for i, rho in enumerate((0.2, 0.5)):
        want, wtau = numpy_keep(ent_all, live_all, rho)
        for r in range(world):
            rho_r, keep, tau, own = res[r][i]
            assert rho_r == rho and abs(tau - wtau) <= 1e-6 * max(1.0, abs(wtau)), (r, rho, tau, wtau)
            assert abs(own - wtau) > 0.1, f"rank {r}'s own quantile {own} is too close to the global one {wtau} for the case to show anything"
            assert np.array_equal(keep, want[r * 4: (r + 1) * 4]), (r, rho)


def test_args_config_and_cli_refusals_by_name(tmp_path):
    from iadr1_amd.trainer import GRPOConfig, SCGRPOTrainer
    for bad in (-0.1, 1.5, float("nan"), float("inf"), None, "0.5", True):
        with pytest.raises(ValueError, match="GRPOArgs.top_entropy_quantile"):
            SCGRPOEngine(None, None, None, GRPOArgs(top_entropy_quantile=bad))
        with pytest.raises(ValueError, match="GRPOConfig.top_entropy_quantile"):
            SCGRPOTrainer((tgo.CFG, None), [], processing_class=object(), args=GRPOConfig(top_entropy_quantile=bad))
        with pytest.raises(ValueError, match="X.top_entropy_quantile"):
            check_entropy_args("X", bad)
    for ok in (0, 0.0, 0.2, 1, 1.0):
        check_entropy_args("X", ok)
    with pytest.raises(ValueError, match="top_entropy_quantile with llava_rotate_right_padded_rows"):
        SCGRPOEngine(types.SimpleNamespace(is_llava=True), None, None, GRPOArgs(top_entropy_quantile=0.5))
    check_entropy_args("X", 1.0, llava_rotated=True)       # off: nothing to refuse
    d = GRPOArgs()
    assert d.rollout_entropy is False and d.top_entropy_quantile == 1.0 and not d.wants_rollout_entropy
    assert GRPOArgs(rollout_entropy=True).wants_rollout_entropy and GRPOArgs(top_entropy_quantile=0.2).wants_rollout_entropy
    c = GRPOConfig()
    assert c.rollout_entropy is False and c.top_entropy_quantile == 1.0
    mod = tgo._grpo_ad()
    base = ["--model_name_or_path", "/m", "--output_dir", "o", "--dataset_name", "d.json"]
    a = mod.build_parser().parse_args(base)
    assert a.rollout_entropy is False and a.top_entropy_quantile == 1.0
    a = mod.build_parser().parse_args(base + ["--rollout_entropy", "--top_entropy_quantile", "0.2"])
    assert a.rollout_entropy is True and a.top_entropy_quantile == 0.2
    a = mod.build_parser().parse_args(base + ["--rollout_entropy", "false"])
    assert a.rollout_entropy is False
    with pytest.raises(SystemExit):
        mod.build_parser().parse_args(base + ["--top_entropy_quantile", "most"])
    y = tmp_path / "c.yaml"
    y.write_text("model_name_or_path: /m\noutput_dir: o\ndataset_name: d.json\nrollout_entropy: true\ntop_entropy_quantile: 0.3\n")
    a = mod.parse_args_and_config(mod.build_parser(), ["--config", str(y)])
    assert a.rollout_entropy is True and a.top_entropy_quantile == 0.3
    a = mod.parse_args_and_config(mod.build_parser(), ["--config", str(y), "--top_entropy_quantile", "0.6"])
    assert a.top_entropy_quantile == 0.6
    assert {"rollout_entropy", "top_entropy_quantile"} <= set(GRPOConfig.__dataclass_fields__)     # grpo_ad.main copies every parsed flag that is a GRPOConfig field


# ---- GPU, kernel level ------------------------------------------------------------------------------------------------------------------------------------------

FORMS = tgo.FORMS
SHAPES = [(1, 1), (1, 37), (1, 300), (5, 1), (5, 37), (5, 300)]     # one thread, a partial pass, more than one 256-pass


def inputs(N, C, seed):
    """tests/test_grpo_objective.py's kernel inputs (C = 1: one live token per row; the generator there needs C >= 2) plus a selector that keeps about half of the tokens,
    dead ones included (what sits in sel off the mask must not matter)."""
    if C == 1:
        t = tgo.kernel_inputs(N, C, None, seed, lens=[1] * N)
    else:
        t = tgo.kernel_inputs(N, C, "mixed" if N > 1 else "ragged", seed)
    g = torch.Generator().manual_seed(seed + 1)
    t["sel"] = (torch.rand(N, C, generator=g) < 0.5).to(torch.int32).to(DEV).contiguous()
    return t


def restate_sel(t, form, loss_type, beta, use_ref, mcl):
    """The written-out objective in float64 with autograd: per token  w (-(q s - beta kl)),  s = exp(p - sg p) A (plain, IS) or min(r A, rc A) (clip); q gates the
    advantage term only; the weight is a constant under differentiation.  Reads the float32 inputs exactly."""
    p = t["p"].double().cpu().requires_grad_(True)
    live = t["mask"].bool().cpu()
    m = live.double()
    q = (t["sel"].cpu() != 0).double()
    N = p.shape[0]
    A = t["adv"].double().cpu()[:, None]
    cnt = m.sum(1)
    inv = torch.where(cnt > 0, 1.0 / cnt.clamp(min=1), torch.zeros(()).double())
    r = t["r"].double().cpu()
    kl = (torch.exp(r - p) - (r - p) - 1) if use_ref else torch.zeros_like(p)
    if form.startswith("clip"):
        old = torch.where(live, t["old"].double().cpu(), p.detach())
        ratio = torch.exp(p - old)
        s = torch.min(ratio * A, torch.clamp(ratio, 1 - EL, 1 + EH) * A)
    else:
        s = torch.exp(p - p.detach()) * A
    ptl = -(q * s - beta * kl)
    if form.startswith("is_"):
        d = torch.where(live, p.detach() - t["q"].double().cpu(), torch.zeros(()).double())
        ratio = torch.exp(d) if form == "is_token" else torch.exp((d * m).sum(1) * inv)[:, None].expand_as(d)
        ptl = ratio.clamp(max=CAP) * ptl
    elif form == "clip_w":
        ptl = t["w"].double().cpu() * ptl
    loss = tgo.trl_loss(ptl, m, loss_type, N, mcl)
    loss.backward()
    sc = {"grpo": inv, "bnpo": N / m.sum().clamp(min=1.0), "dr_grpo": torch.tensor(1.0 / mcl).double()}[loss_type]
    return dict(dlogp=p.grad, kl=kl.detach(), loss=loss.detach(), row_loss=((ptl * m).sum(1) * sc).detach(), row_kl=((kl * m).sum(1) * inv).detach())


@pytest.mark.gpu
@pytest.mark.parametrize("N,C", SHAPES)
def test_kernel_against_float64_autograd_of_the_gated_objective(N, C):
    """row_loss, row_kl, kl and dlogp; every form x loss_type x {reference given, NULL with beta 0}; the tolerances of test_grpo_objective.check_against."""
    t = inputs(N, C, seed=5000 * N + C)
    sc = tgo.scales(t, C)
    worst = 0.0
    for form in FORMS:
        for lt in tgo.LOSS_TYPES:
            for use_ref in (True, False):
                beta = BETA if use_ref else 0.0
                want = restate_sel(t, form, lt, beta, use_ref, C)
                got = ops.grpo_loss_ex(t["p"], t["adv"], t["mask"], beta, ref_logp=t["r"] if use_ref else None, row_scale=sc[lt], sel=t["sel"], **tgo.form_args(t, form))
                what = f"N={N} C={C} {form} {lt} ref={'given' if use_ref else 'NULL'}"
                worst = max(worst, float((got[0].double().cpu() - want["dlogp"]).abs().max()))
                close(got[0], want["dlogp"], 1e-4, 1e-7, f"{what}: dlogp")
                close(got[1], want["kl"], 1e-4, 1e-7, f"{what}: kl")
                close(got[2], want["row_loss"], 1e-5, 1e-7, f"{what}: row loss")
                close(got[2].mean(), want["loss"], 1e-5, 1e-7, f"{what}: loss")
                close(got[3], want["row_kl"], 1e-5, 1e-7, f"{what}: row kl")
                assert bool((got[0][t["mask"] == 0] == 0).all()), what
    print(f"[grpo_loss_sel kernel] N={N} C={C}: max |dlogp err| {worst:.3e}; {int((t['sel'].bool() & t['mask'].bool()).sum())} of {int(t['mask'].sum())} live tokens selected")


@pytest.mark.gpu
@pytest.mark.parametrize("N,C", SHAPES)
def test_all_ones_and_none_are_grpo_loss_ex_bit_for_bit(N, C):
    t = inputs(N, C, seed=6000 * N + C)
    ones = torch.ones(N, C, dtype=torch.int32, device=DEV)
    n_calls = 0
    for form in FORMS:
        for lt, sc in tgo.scales(t, C).items():
            for use_ref in (True, False):
                kw = dict(ref_logp=t["r"] if use_ref else None, row_scale=sc, **tgo.form_args(t, form))
                beta = BETA if use_ref else 0.0
                ex = ops.grpo_loss_ex(t["p"], t["adv"], t["mask"], beta, **kw)
                for sel in (ones, None):
                    got = ops.grpo_loss_ex(t["p"], t["adv"], t["mask"], beta, sel=sel, **kw)
                    assert len(got) == len(ex)
                    for k, (a, b) in enumerate(zip(ex, got)):
                        assert torch.equal(a, b), (N, C, form, lt, use_ref, "ones" if sel is not None else "None", k, float((a - b).abs().max()))
                    n_calls += 1
    assert n_calls == len(FORMS) * 3 * 2 * 2
    # the raw entry point with sel == NULL
    dl, kl, rl, rk = (torch.empty(N, C, dtype=F32, device=DEV), torch.empty(N, C, dtype=F32, device=DEV), torch.empty(N, dtype=F32, device=DEV), torch.empty(N, dtype=F32, device=DEV))
    ops.hip.call("grpo_loss_sel", t["p"], t["r"], None, None, None, t["adv"], t["mask"], BETA, 0.0, 0, 0.0, 0.0, 0.0, N, dl, kl, rl, rk, None, None, N, C, None)
    ex = ops.grpo_loss_ex(t["p"], t["adv"], t["mask"], BETA, ref_logp=t["r"])
    assert all(torch.equal(a, b) for a, b in zip(ex, (dl, kl, rl, rk)))


@pytest.mark.gpu
@pytest.mark.parametrize("N,C", SHAPES)
def test_all_zeros_at_beta_zero_leave_nothing(N, C):
    t = inputs(N, C, seed=7000 * N + C)
    zeros = torch.zeros(N, C, dtype=torch.int32, device=DEV)
    for form in FORMS:
        for lt, sc in tgo.scales(t, C).items():
            for ref in (t["r"], None):
                got = ops.grpo_loss_ex(t["p"], t["adv"], t["mask"], 0.0, ref_logp=ref, row_scale=sc, sel=zeros, **tgo.form_args(t, form))
                assert bool((got[0] == 0).all()) and bool((got[2] == 0).all()), (N, C, form, lt, ref is None)
                # the statistics keep running over the live tokens
                ex = ops.grpo_loss_ex(t["p"], t["adv"], t["mask"], 0.0, ref_logp=ref, row_scale=sc, **tgo.form_args(t, form))
                assert all(torch.equal(a, b) for a, b in zip(ex[4:], got[4:])) and torch.equal(ex[1], got[1]) and torch.equal(ex[3], got[3])


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_a_zero_clears_that_tokens_advantage_gradient_and_keeps_its_kl_gradient(form):
    """One live token gets sel = 0: its dlogp is the dlogp of the same call with every advantage at 0 (the KL gradient alone, bit for bit: -0 + x == x), every other
    token's dlogp, kl, row_kl and the partials keep the bits of the all-ones call; that row's row_loss moves, the others do not."""
    N, C = 5, 37
    t = inputs(N, C, seed=8000)
    kw = dict(ref_logp=t["r"], **tgo.form_args(t, form))
    ones = torch.ones(N, C, dtype=torch.int32, device=DEV)
    full = ops.grpo_loss_ex(t["p"], t["adv"], t["mask"], BETA, sel=ones, **kw)
    klonly = ops.grpo_loss_ex(t["p"], torch.zeros_like(t["adv"]), t["mask"], BETA, sel=ones, **kw)
    row = 1         # fully live in the "mixed" inputs
    # a token whose advantage term has a gradient (in the clipped form a clipped token has none to clear)
    col = int(torch.nonzero(full[0][row] != klonly[0][row])[C // 2])
    assert int(t["mask"][row, col]) == 1 and float(t["adv"][row]) != 0
    sel = ones.clone()
    sel[row, col] = 0
    got = ops.grpo_loss_ex(t["p"], t["adv"], t["mask"], BETA, sel=sel, **kw)
    other = torch.ones(N, C, dtype=torch.bool, device=DEV)
    other[row, col] = False
    assert torch.equal(got[0][other], full[0][other])
    assert float(got[0][row, col]) == float(klonly[0][row, col]) != float(full[0][row, col]) and float(klonly[0][row, col]) != 0
    assert torch.equal(got[1], full[1]) and torch.equal(got[3], full[3]) and all(torch.equal(a, b) for a, b in zip(got[4:], full[4:]))
    rows = torch.arange(N, device=DEV) != row
    assert torch.equal(got[2][rows], full[2][rows]) and float(got[2][row]) != float(full[2][row])


# ---- GPU, engine level ------------------------------------------------------------------------------------------------------------------------------------------

def _engine_step(**kw):
    import test_rollout_logps as trl_
    pol, ref = trl_.stores()
    eng = SCGRPOEngine(tgo.CFG, pol, ref, GRPOArgs(num_generations=4, max_prompt_length=4096, max_completion_length=16, seed=5, **kw))
    out = eng.step(trl_.tiny_batch(), trl_.reward_fn, do_optimizer_step=False, return_outputs=True)
    torch.cuda.synchronize()
    return out, pol.grad.clone(), eng


@pytest.mark.gpu
def test_engine_step_with_top_entropy_quantile():
    """An engine step on TINY with top_entropy_quantile = 0.2 against the ungated step with rollout_entropy: same rollout, same entropies; the mask is the numpy
    restatement's; the loss differs, kl and the log-probs do not; gradients finite; the mask does not depend on micro_batch_seqs; the refusals of the call.
    kept_frac: with n live tokens and no tie the threshold sits at position 0.8 (n - 1) of the sorted entropies, so n - ceil(0.8 (n - 1)) tokens are kept, which is
    k + 1 for every n in 5 k + 1 .. 5 k + 5: a share in [0.2, 0.2 + 0.8 / n].  The upper bound asserted is therefore 0.2 + max(ties, 1) / n -- one token of slack where
    the threshold is interpolated between two entropies and no token sits on it (with ties / n alone, 0 ties would ask for exactly 0.2, which only n = 5 k + 5 can
    give)."""
    base, g0, _ = _engine_step(rollout_entropy=True)
    out, g1, eng = _engine_step(top_entropy_quantile=0.2)
    m = out["metrics"]
    assert np.array_equal(base["completion_ids"], out["completion_ids"]) and torch.equal(base["rollout_entropy"], out["rollout_entropy"])
    assert set(m) == set(base["metrics"]) | {"entropy/threshold", "entropy/kept_frac"} and m["entropy"] == base["metrics"]["entropy"]
    live = torch.from_numpy(np.asarray(out["completion_mask"]).astype(bool)).to(DEV)
    ent, keep = out["rollout_entropy"], out["entropy_mask"]
    n_live = int(live.sum())
    ties = int(((ent == float(np.float32(m["entropy/threshold"]))) & live).sum())
    print(f"[top_entropy_quantile] TINY: entropy {m['entropy']:.4f}, threshold {m['entropy/threshold']:.4f}, kept {int(keep.sum())} of {n_live} live tokens ({ties} at the threshold); "
          f"loss {m['loss']:.6f} against {base['metrics']['loss']:.6f} ungated")
    assert keep.dtype == torch.bool and not bool((keep & ~live).any()) and int(keep.sum()) == round(m["entropy/kept_frac"] * n_live)
    assert 0.2 - 1e-6 <= m["entropy/kept_frac"] <= 0.2 + max(ties, 1) / n_live + 1e-6
    want, _ = numpy_keep(ent.cpu().numpy(), live.cpu().numpy(), 0.2)
    assert np.array_equal(keep.cpu().numpy(), want)
    assert m["loss"] != base["metrics"]["loss"] and m["kl"] == base["metrics"]["kl"] and torch.equal(out["kl"], base["kl"]) and torch.equal(out["logps"], base["logps"])
    assert bool(torch.isfinite(g1).all()) and not torch.equal(g0, g1) and float(g1.abs().max()) > 0
    # the mask does not depend on the micro-batch
    half, g2, _ = _engine_step(top_entropy_quantile=0.2, micro_batch_seqs=4)
    assert torch.equal(half["entropy_mask"], keep) and half["metrics"]["entropy/kept_frac"] == m["entropy/kept_frac"]
    # completions handed in without their entropies, and a reuse step without the cached mask, are refused by name
    import test_rollout_logps as trl_
    comp = out["completion_ids"]
    with pytest.raises(ValueError, match="top_entropy_quantile < 1: completions were handed in without their rollout entropies"):
        eng.step(trl_.tiny_batch(), trl_.reward_fn, do_optimizer_step=False, completions=comp)
    with pytest.raises(ValueError, match="top_entropy_quantile < 1: a reuse iteration .* needs the entropy_mask"):
        eng.step(trl_.tiny_batch(), trl_.reward_fn, do_optimizer_step=False, completions=comp, old_logps=out["logps"], ref_logps=out["ref_logps"])
    with pytest.raises(ValueError, match="top_entropy_quantile < 1 needs the rollout entropies"):
        eng.loss_and_grads(trl_.tiny_batch(), comp, trl_.reward_fn(comp), backward=False)
