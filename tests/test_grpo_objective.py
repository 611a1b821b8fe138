"""trl's remaining objective options on the SC-GRPO step: loss_type (grpo | bnpo | dr_grpo), scale_rewards, mask_truncated_completions and beta == 0 without a
reference model -- iadr1_grpo_loss_ex (csrc/loss.hip), ops.grpo_loss_ex, GRPOArgs / SCGRPOEngine, GRPOConfig / SCGRPOTrainer and the three flags of
train/stage_rl/grpo_ad.py.  The float64 restatements of trl/trl/trainer/grpo_trainer.py:1192-1217 live here.  The ABI / argument / mask tests need no GPU."""
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
import test_grpo_clip as tgc  # noqa: E402  (off_the_bounds: the construction that keeps live tokens away from a clip bound)
import test_rollout_is as tri  # noqa: E402  (close, stores, tiny_batch, reward_fn)
from iadr1_amd import hip, ops, sc_grpo  # noqa: E402
from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine, eos_completion_mask, group_advantages, loss_row_scale, truncation_loss_mask  # noqa: E402

DEV = "cuda"
F32 = torch.float32
CFG = tri.CFG
BETA = tri.BETA
EOS = CFG.eos_token_id
LOSS_TYPES = ("grpo", "bnpo", "dr_grpo")
EL, EH, CAP = 0.2, 0.28, 2.0
ULP2 = 2 * 2.0 ** -24
close = tri.close
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- without a GPU -----------------------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_entry_point():
    assert "iadr1_grpo_loss_ex" in hip.PROTOS and hasattr(hip.lib(), "iadr1_grpo_loss_ex") and hip.version() >= 114
    names = [n for _, n in hip.PROTOS["iadr1_grpo_loss_ex"][1]]
    assert names[:7] == ["logp", "ref_logp", "old_logp", "rollout_logp", "w", "adv", "mask"]
    assert names[7:14] == ["beta", "cap", "level", "eps_low", "eps_high", "row_scale", "n_total_rows"] and names[-5:] == ["w_out", "row_stats", "N", "C", "stream"]


def _raw_call(N=2, C=4, ref=True, old=False, ro=False, w=False, stats=True, beta=BETA, cap=CAP, level=0, eps_low=EL, eps_high=EH, row_scale=0.0, n_total=None):
    """The entry point on host buffers: every case here must be refused before anything is launched."""
    L = hip.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    rc = L.iadr1_grpo_loss_ex(p, p if ref else None, p if old else None, p if ro else None, p if w else None, p, p, beta, cap, level, eps_low, eps_high, row_scale,
                              max(N, 1) if n_total is None else n_total, p, p, p, p, p, p if stats else None, N, C, None)
    return rc, L.iadr1_last_error().decode()


@pytest.mark.parametrize("kw,word", [({"ref": False}, "beta"), ({"ref": False, "beta": -0.5}, "ref_logp"), ({"ref": False, "beta": float("nan")}, "beta"),
                                     ({"row_scale": -1.0}, "row_scale"), ({"row_scale": float("nan")}, "row_scale"), ({"row_scale": float("inf")}, "row_scale"),
                                     ({"old": True, "ro": True}, "rollout_logp"), ({"w": True}, "without old_logp"), ({"w": True, "ro": True}, "without old_logp"),
                                     ({"old": True, "stats": False}, "row_stats"), ({"ro": True, "stats": False}, "row_stats"),
                                     ({"ro": True, "cap": 0.5}, "cap"), ({"ro": True, "cap": float("nan")}, "cap"), ({"ro": True, "cap": float("inf")}, "cap"),
                                     ({"ro": True, "level": 2}, "level"), ({"old": True, "eps_low": 1.0}, "eps_low"), ({"old": True, "eps_low": float("nan")}, "eps_low"),
                                     ({"old": True, "eps_high": -0.1}, "eps_high"), ({"old": True, "eps_high": float("inf")}, "eps_high"),
                                     ({"N": 0}, "N must be > 0"), ({"N": -3}, "N must be > 0"), ({"C": 0}, "C must be > 0"), ({"N": 4, "n_total": 3}, "n_total_rows (3) is smaller than N (4)")])
def test_bad_arguments_are_refused_on_the_host(kw, word):
    rc, msg = _raw_call(**kw)
    assert rc < 0 and "grpo_loss_ex" in msg and word in msg, (rc, msg)


@pytest.mark.parametrize("name", ["grpo_loss", "grpo_loss_is", "grpo_loss_clip"])
def test_the_older_entry_points_refuse_a_null_reference_with_a_kl_term(name):
    """ref_logp NULL with beta != 0 on otherwise valid host buffers: refused before anything is launched, with iadr1_grpo_loss_ex's rule and the entry point's prefix."""
    L = hip.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    if name == "grpo_loss":
        rc = L.iadr1_grpo_loss(p, None, p, p, BETA, 2, p, p, p, p, 2, 4, None)
    elif name == "grpo_loss_is":
        rc = L.iadr1_grpo_loss_is(p, None, p, p, p, BETA, CAP, 0, 2, p, p, p, p, p, p, 2, 4, None)
    else:
        rc = L.iadr1_grpo_loss_clip(p, p, None, p, p, None, BETA, EL, EH, 2, p, p, p, p, p, 2, 4, None)
    msg = L.iadr1_last_error().decode()
    assert rc < 0 and msg.startswith(name + ":") and "ref_logp" in msg, (rc, msg)


def _grpo_ad():
    spec = importlib.util.spec_from_file_location("grpo_ad_objective_flags", os.path.join(ROOT, "train", "stage_rl", "grpo_ad.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_defaults_flags_and_config_file(tmp_path):
    from iadr1_amd.trainer import GRPOConfig
    for cls in (GRPOArgs, GRPOConfig):
        d = cls()
        assert d.loss_type == "grpo" and d.scale_rewards is True and d.mask_truncated_completions is False
    mod = _grpo_ad()
    base = ["--model_name_or_path", "/m", "--output_dir", "o", "--dataset_name", "d.json"]
    d = mod.build_parser().parse_args(base)
    assert d.loss_type == "grpo" and d.scale_rewards is True and d.mask_truncated_completions is False
    a = mod.build_parser().parse_args(base + ["--loss_type", "dr_grpo", "--scale_rewards", "false", "--mask_truncated_completions", "true", "--beta", "0"])
    assert a.loss_type == "dr_grpo" and a.scale_rewards is False and a.mask_truncated_completions is True and a.beta == 0.0
    a = mod.build_parser().parse_args(base + ["--loss_type", "bnpo", "--scale_rewards", "--mask_truncated_completions"])
    assert a.loss_type == "bnpo" and a.scale_rewards is True and a.mask_truncated_completions is True
    with pytest.raises(SystemExit):
        mod.build_parser().parse_args(base + ["--loss_type", "ppo"])
    y = tmp_path / "run.yaml"
    y.write_text("model_name_or_path: /m\noutput_dir: o\ndataset_name: d.json\nloss_type: dr_grpo\nscale_rewards: false\nmask_truncated_completions: true\nbeta: 0.0\n")
    a = mod.parse_args_and_config(mod.build_parser(), ["--config", str(y)])
    assert a.loss_type == "dr_grpo" and a.scale_rewards is False and a.mask_truncated_completions is True and a.beta == 0.0
    a = mod.parse_args_and_config(mod.build_parser(), ["--config", str(y), "--loss_type", "bnpo"])
    assert a.loss_type == "bnpo" and a.scale_rewards is False
    assert {"loss_type", "scale_rewards", "mask_truncated_completions"} <= set(GRPOConfig.__dataclass_fields__)     # grpo_ad.main copies every parsed flag that is a GRPOConfig field


def test_refused_combinations(monkeypatch):
    from iadr1_amd.trainer import GRPOConfig, SCGRPOTrainer
    with pytest.raises(ValueError, match="loss_type"):
        SCGRPOEngine(None, None, None, GRPOArgs(loss_type="ppo"))
    with pytest.raises(ValueError, match="loss_type"):
        SCGRPOTrainer((CFG, None), [], processing_class=object(), args=GRPOConfig(loss_type="ppo"))
    with pytest.raises(ValueError, match="beta"):
        SCGRPOEngine(CFG, None, None, GRPOArgs())
    with pytest.raises(ValueError, match="suppress_eos"):
        SCGRPOEngine(CFG, None, None, GRPOArgs(mask_truncated_completions=True, suppress_eos=True))
    for forced in ("64", "-1", "half"):         # a CU share, the ordinary second stream, and no number at all: the same explained refusal
        monkeypatch.setenv("IADR1_OVERLAP_CUS", forced)
        with pytest.raises(ValueError, match="IADR1_OVERLAP_CUS=.* with GRPOArgs.beta == 0"):
            SCGRPOEngine(CFG, None, None, GRPOArgs(beta=0.0))


def test_unscaled_advantages_are_reward_minus_group_mean():
    g = torch.Generator().manual_seed(0)
    r = (torch.randn(12, generator=g) * 3).to(F32)
    adv, std = group_advantages(r, 4, scale=False)
    assert torch.equal(adv, r - r.view(-1, 4).mean(1).repeat_interleave(4))
    scaled, std1 = group_advantages(r, 4)
    assert torch.equal(std, std1) and torch.equal(scaled, group_advantages(r, 4, scale=True)[0]) and torch.equal(scaled, adv / (std + 1e-4))


def _rows(*rows):
    return np.asarray(rows, dtype=np.int64)


HAND = _rows([EOS, 7, 7, 7, 7],        # EOS at column 0
             [7, 8, 9, 7, EOS],        # EOS in the last column: a finished row of full length
             [7, 8, 9, 7, 8],          # no EOS: truncated
             [7, 8, EOS, 0, 0])
HAND_EOS_MASK = np.asarray([[1, 0, 0, 0, 0], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [1, 1, 1, 0, 0]], dtype=np.int32)


def test_loss_mask_on_hand_written_rows():
    cm = eos_completion_mask(HAND, EOS)
    assert np.array_equal(cm, HAND_EOS_MASK)
    lm = truncation_loss_mask(cm, HAND, EOS)
    want = HAND_EOS_MASK.copy()
    want[2] = 0
    assert np.array_equal(lm, want) and lm.dtype == cm.dtype
    every = _rows([7, 8, 9, 7, 8], [9, 9, 9, 9, 9])
    cm2 = eos_completion_mask(every, EOS)
    assert int(cm2.sum()) == 10 and int(truncation_loss_mask(cm2, every, EOS).sum()) == 0


@pytest.mark.parametrize("mcl", [5, 12, 256])
def test_row_scale_is_the_float64_value_rounded_once(mcl):
    cm = eos_completion_mask(HAND, EOS)
    every = _rows([7, 8, 9, 7, 8], [9, 9, 9, 9, 9])
    masks = [cm, truncation_loss_mask(cm, HAND, EOS), truncation_loss_mask(eos_completion_mask(every, EOS), every, EOS)]
    for m in masks:
        n, live = m.shape[0], int(m.sum())
        assert loss_row_scale("grpo", m, mcl) == 0.0
        assert loss_row_scale("bnpo", m, mcl) == float(np.float32(np.float64(n) / np.float64(max(live, 1))))
        assert loss_row_scale("dr_grpo", m, mcl) == float(np.float32(np.float64(1.0) / np.float64(mcl)))
    assert loss_row_scale("bnpo", masks[0], mcl) == float(np.float32(4 / 14)) and loss_row_scale("bnpo", masks[1], mcl) == float(np.float32(4 / 9))
    assert loss_row_scale("bnpo", masks[2], mcl) == 2.0         # every row truncated: the clamp at 1 live token
    with pytest.raises(ValueError, match="loss_type"):
        loss_row_scale("ppo", cm, mcl)


# ---- GPU, kernel level ---------------------------------------------------------------------------------------------------------------------------------

FORMS = ("plain", "is_token", "is_sequence", "clip", "clip_w")
SHAPES = [(1, 7), (1, 256), (1, 300), (5, 7), (5, 256), (5, 300)]


def mask_kinds(N):
    """N = 5: row 0 has no live token, row 1 is fully live, the others are ragged.  One row cannot be all three, so N = 1 runs once per kind."""
    return ("mixed",) if N > 1 else ("empty", "full", "ragged")


def kernel_inputs(N, C, kind, seed, lens=None):
    """Policy, reference, rollout (0 off the mask: the rollout's contract), old log-probs, weights, advantages and a prefix mask."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(N, C, generator=g) * 0.3 - 2.0
    r = p + torch.randn(N, C, generator=g) * 0.1
    dq = (torch.rand(N, C, generator=g) * 2 - 1) * 1.5
    do = torch.rand(N, C, generator=g) - 0.5
    w = 0.5 + 1.5 * torch.rand(N, C, generator=g)
    adv = torch.randn(N, generator=g)
    if lens is None:
        lens = torch.randint(1, C, (N,), generator=g)
        if kind == "mixed":
            lens[0], lens[1] = 0, C
        else:
            lens[0] = {"empty": 0, "full": C, "ragged": C // 2 + 1}[kind]
    mask = (torch.arange(C)[None, :] < torch.as_tensor(lens)[:, None]).int()
    q = torch.where(mask.bool(), p - dq, torch.zeros(()))
    t = {k: v.to(F32).to(DEV).contiguous() for k, v in dict(p=p, r=r, q=q, old=p - do, w=w, adv=adv).items()}
    t["mask"] = mask.to(DEV).contiguous()
    t["old"], t["moved"] = tgc.off_the_bounds(t["p"], t["old"], t["mask"], EL, EH)
    return t


def form_args(t, form):
    if form == "plain":
        return {}
    if form.startswith("is_"):
        return dict(rollout_logp=t["q"], cap=CAP, level=form[3:])
    return dict(old_logp=t["old"], eps_low=EL, eps_high=EH, w=t["w"] if form == "clip_w" else None)


def scales(t, C):
    """row_scale for the three loss types on these rows: 0, rows / live tokens, 1 / C (max_completion_length = C)."""
    m = t["mask"].cpu().numpy()
    return {lt: loss_row_scale(lt, m, C) for lt in LOSS_TYPES}


def trl_loss(ptl, m, loss_type, n_rows, mcl):
    """trl/trl/trainer/grpo_trainer.py:1212-1217 on float64 per-token losses."""
    if loss_type == "grpo":
        return ((ptl * m).sum(-1) / m.sum(-1).clamp(min=1.0)).sum() / n_rows
    if loss_type == "bnpo":
        return (ptl * m).sum() / m.sum().clamp(min=1.0)
    return (ptl * m).sum() / (n_rows * mcl)


def restate(t, form, loss_type, beta, use_ref, mcl):
    """trl:1192-1217 in float64 with autograd for d loss / d logp; the weight (truncated importance weight or handed-in w) is a constant under differentiation.
    Reads the float32 inputs exactly."""
    p = t["p"].double().cpu().requires_grad_(True)
    live = t["mask"].bool().cpu()
    m = live.double()
    N = p.shape[0]
    A = t["adv"].double().cpu()[:, None]
    cnt = m.sum(1)
    inv = torch.where(cnt > 0, 1.0 / cnt.clamp(min=1), torch.zeros(()).double())
    r = t["r"].double().cpu()
    kl = (torch.exp(r - p) - (r - p) - 1) if use_ref else torch.zeros_like(p)
    out = {}
    if form.startswith("clip"):
        old = torch.where(live, t["old"].double().cpu(), p.detach())
        ratio = torch.exp(p - old)
        ptl = -torch.min(ratio * A, torch.clamp(ratio, 1 - EL, 1 + EH) * A)
        rt, d = ratio.detach(), (p.detach() - old).abs()
        out["stats"] = torch.stack([((rt < 1 - EL) & (A < 0) & live).sum(1).double(), ((rt > 1 + EH) & (A > 0) & live).sum(1).double(), (rt * m).sum(1), (d * m).max(1).values], 1)
    else:
        ptl = -(torch.exp(p - p.detach()) * A)
    if use_ref:
        ptl = ptl + beta * kl
    if form.startswith("is_"):
        d = torch.where(live, p.detach() - t["q"].double().cpu(), torch.zeros(()).double())
        tok = torch.exp(d)
        ratio = tok if form == "is_token" else torch.exp((d * m).sum(1) * inv)[:, None].expand_as(d)
        w = ratio.clamp(max=CAP)
        out["w"] = w * m
        out["stats"] = torch.stack([(w * m).sum(1), torch.zeros_like(cnt), (d.abs() * m).sum(1), (d.abs() * m).max(1).values, ((tok - d - 1) * m).sum(1)], 1)
        out["clip_lo"], out["clip_hi"] = ((ratio > CAP * (1 + 1e-4)) & live).sum(1), ((ratio > CAP * (1 - 1e-4)) & live).sum(1)
        ptl = w * ptl
    elif form == "clip_w":
        ptl = t["w"].double().cpu() * ptl
    loss = trl_loss(ptl, m, loss_type, N, mcl)
    loss.backward()
    s = {"grpo": inv, "bnpo": N / m.sum().clamp(min=1.0), "dr_grpo": torch.tensor(1.0 / mcl).double()}[loss_type]
    out.update(dlogp=p.grad, kl=kl.detach(), loss=loss.detach(), row_loss=((ptl * m).sum(1) * s).detach(), row_kl=((kl * m).sum(1) * inv).detach(), cnt=cnt)
    return out


def check_against(want, got, t, form, what):
    """dlogp, kl (rtol 1e-4, atol 1e-7); row and batch loss, row_kl (1e-5, 1e-7); clipped counts exact; the other partials as test_grpo_clip / test_rollout_is hold them."""
    dlogp, kl, row_loss, row_kl = got[:4]
    mask = t["mask"]
    close(dlogp, want["dlogp"], 1e-4, 1e-7, f"{what}: dlogp")
    close(kl, want["kl"], 1e-4, 1e-7, f"{what}: kl")
    close(row_loss, want["row_loss"], 1e-5, 1e-7, f"{what}: row loss")
    close(row_loss.mean(), want["loss"], 1e-5, 1e-7, f"{what}: loss")
    close(row_kl, want["row_kl"], 1e-5, 1e-7, f"{what}: row kl")
    assert bool((dlogp[mask == 0] == 0).all()), what
    empty = want["cnt"] == 0
    if form.startswith("clip"):
        st = got[4].double().cpu()
        assert torch.equal(st[:, :2], want["stats"][:, :2]), (what, st[:, :2], want["stats"][:, :2])
        close(st[:, 2], want["stats"][:, 2], 1e-5, 0.0, f"{what}: sum m r")
        close(st[:, 3], want["stats"][:, 3], 1e-6, 0.0, f"{what}: max m |d|")
    elif form.startswith("is_"):
        w, st = got[4], got[5].double().cpu()
        close(w, want["w"], 1e-4, 1e-7, f"{what}: w_out")
        assert bool((w[mask == 0] == 0).all())
        close(st[:, 0], want["stats"][:, 0], 1e-5, 0.0, f"{what}: sum m w")
        close(st[:, 2], want["stats"][:, 2], 1e-5, 0.0, f"{what}: sum m |d|")
        close(st[:, 3], want["stats"][:, 3], 1e-6, 0.0, f"{what}: max m |d|")
        err = (st[:, 4] - want["stats"][:, 4]).abs()
        assert bool((err <= 4e-6 * want["cnt"] + 1e-5 * want["stats"][:, 4].abs()).all()), (what, "sum m (exp(d) - d - 1)", err.max().item())
        assert bool((st[:, 1] >= want["clip_lo"]).all()) and bool((st[:, 1] <= want["clip_hi"]).all()), (what, st[:, 1], want["clip_lo"], want["clip_hi"])
    else:
        st = None
    assert bool((row_loss.cpu()[empty] == 0).all()) and bool((row_kl.cpu()[empty] == 0).all()) and (st is None or float(st[empty].abs().sum()) == 0), what


@pytest.mark.gpu
@pytest.mark.parametrize("N,C", SHAPES)
def test_kernel_against_a_float64_restatement_of_trl(N, C):
    """(1) every form x row_scale in {0, the bnpo value, 1 / C} x {reference given, NULL with beta 0}."""
    worst, clipped = 0.0, [0, 0]
    for kind in mask_kinds(N):
        t = kernel_inputs(N, C, kind, seed=1000 * N + C)
        sc = scales(t, C)
        for form in FORMS:
            for lt in LOSS_TYPES:
                for use_ref in (True, False):
                    beta = BETA if use_ref else 0.0
                    want = restate(t, form, lt, beta, use_ref, C)
                    got = ops.grpo_loss_ex(t["p"], t["adv"], t["mask"], beta, ref_logp=t["r"] if use_ref else None, row_scale=sc[lt], **form_args(t, form))
                    torch.cuda.synchronize()
                    worst = max(worst, float((got[0].double().cpu() - want["dlogp"]).abs().max()))
                    if form == "clip":
                        clipped = [max(clipped[0], int(want["stats"][:, 0].sum())), max(clipped[1], int(want["stats"][:, 1].sum()))]
                    check_against(want, got, t, form, f"N={N} C={C} {kind} {form} {lt} ref={'given' if use_ref else 'NULL'}")
                    if not use_ref:
                        assert bool((got[1] == 0).all()) and bool((got[3] == 0).all())
    print(f"[grpo_loss_ex kernel] N={N} C={C}: max |dlogp err| {worst:.3e}; clip form: up to {clipped[0]} low- and {clipped[1]} high-clipped tokens, {t['moved']} moved off a bound")
    assert C < 256 or N == 1 or (clipped[0] > 0 and clipped[1] > 0)        # the larger cases do clip on both sides


@pytest.mark.gpu
@pytest.mark.parametrize("N,C", SHAPES)
def test_reference_given_and_row_scale_zero_is_the_old_entry_point_bit_for_bit(N, C):
    """(2) torch.equal to iadr1_grpo_loss / _is / _clip on every output, and two runs are bit-equal."""
    for kind in mask_kinds(N):
        t = kernel_inputs(N, C, kind, seed=2000 * N + C)
        p, r, adv, mask = t["p"], t["r"], t["adv"], t["mask"]
        for form in FORMS:
            if form == "plain":
                old = ops.grpo_loss(p, r, adv, mask, BETA)
            elif form.startswith("is_"):
                old = ops.grpo_loss_is(p, r, t["q"], adv, mask, BETA, CAP, form[3:])
            else:
                old = ops.grpo_loss_clip(p, t["old"], r, adv, mask, BETA, EL, EH, w=t["w"] if form == "clip_w" else None)
            new = ops.grpo_loss_ex(p, adv, mask, BETA, ref_logp=r, row_scale=0.0, **form_args(t, form))
            again = ops.grpo_loss_ex(p, adv, mask, BETA, ref_logp=r, row_scale=0.0, **form_args(t, form))
            assert len(old) == len(new)
            for k, (a, b, c) in enumerate(zip(old, new, again)):
                assert torch.equal(a, b) and torch.equal(b, c), (N, C, kind, form, k)
        sc = scales(t, C)["bnpo"]
        a = ops.grpo_loss_ex(p, adv, mask, 0.0, rollout_logp=t["q"], cap=CAP, level="sequence", row_scale=sc)
        b = ops.grpo_loss_ex(p, adv, mask, 0.0, rollout_logp=t["q"], cap=CAP, level="sequence", row_scale=sc)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("N,C", SHAPES)
def test_null_reference_equals_a_given_one_at_beta_zero(N, C):
    """(3) finite inputs: dlogp and row_loss torch.equal between the two calls; kl and row_kl exactly 0 without a reference."""
    for kind in mask_kinds(N):
        t = kernel_inputs(N, C, kind, seed=3000 * N + C)
        for form in FORMS:
            for lt, sc in scales(t, C).items():
                given = ops.grpo_loss_ex(t["p"], t["adv"], t["mask"], 0.0, ref_logp=t["r"], row_scale=sc, **form_args(t, form))
                null = ops.grpo_loss_ex(t["p"], t["adv"], t["mask"], 0.0, ref_logp=None, row_scale=sc, **form_args(t, form))
                what = (N, C, kind, form, lt)
                assert bool(torch.isfinite(given[0]).all()) and torch.equal(given[0], null[0]) and torch.equal(given[2], null[2]), what
                assert bool((null[1] == 0).all()) and bool((null[3] == 0).all()), what
                assert all(torch.equal(a, b) for a, b in zip(given[4:], null[4:])), what        # the weights and the partials do not involve the reference


@pytest.mark.gpu
def test_the_older_entry_points_run_without_a_reference_at_beta_zero():
    """N = 3, C = 300 (the second trip of the 256-wide loops), row 0 without a live token, row 1 partly live, row 2 full: iadr1_grpo_loss / _is / _clip with
    ref_logp NULL and beta 0 give every output torch.equal to grpo_loss_ex(ref_logp=None) of the same form, no NaN, and zeros on the empty row."""
    t = kernel_inputs(3, 300, "mixed", seed=77, lens=[0, 131, 300])
    p, adv, mask = t["p"], t["adv"], t["mask"]
    for form in FORMS:
        if form == "plain":
            old = ops.grpo_loss(p, None, adv, mask, 0.0)
        elif form.startswith("is_"):
            old = ops.grpo_loss_is(p, None, t["q"], adv, mask, 0.0, CAP, form[3:])
        else:
            old = ops.grpo_loss_clip(p, t["old"], None, adv, mask, 0.0, EL, EH, w=t["w"] if form == "clip_w" else None)
        new = ops.grpo_loss_ex(p, adv, mask, 0.0, ref_logp=None, **form_args(t, form))
        assert len(old) == len(new)
        for k, (a, b) in enumerate(zip(old, new)):
            assert torch.equal(a, b) and not bool(torch.isnan(a).any()), (form, k)
            assert bool((a[0] == 0).all()), (form, k, a[0])


@pytest.mark.gpu
@pytest.mark.parametrize("N,C", SHAPES)
def test_row_scale_is_a_plain_factor(N, C):
    """(4) every row with c live tokens: row_scale = 1 / c is the row_scale = 0 call within (1e-6, 0); doubling it doubles row_loss and dlogp exactly; row_kl does
    not move."""
    c = C // 2 + 1
    t = kernel_inputs(N, C, None, seed=4000 * N + C, lens=[c] * N)
    s = float(np.float32(1.0 / c))
    for form in FORMS:
        kw = form_args(t, form)
        zero = ops.grpo_loss_ex(t["p"], t["adv"], t["mask"], BETA, ref_logp=t["r"], row_scale=0.0, **kw)
        one = ops.grpo_loss_ex(t["p"], t["adv"], t["mask"], BETA, ref_logp=t["r"], row_scale=s, **kw)
        two = ops.grpo_loss_ex(t["p"], t["adv"], t["mask"], BETA, ref_logp=t["r"], row_scale=2 * s, **kw)
        close(one[2], zero[2], 1e-6, 0.0, f"{form}: row loss")
        close(one[0], zero[0], 1e-6, 0.0, f"{form}: dlogp")
        assert torch.equal(two[2], 2 * one[2]) and torch.equal(two[0], 2 * one[0]), form
        assert torch.equal(one[3], zero[3]) and torch.equal(two[3], zero[3]) and torch.equal(one[1], zero[1]), form


# ---- GPU, engine and trainer level ---------------------------------------------------------------------------------------------------------------------

G, C_ENG = 4, 16
RAGGED = {0: 5, 2: 15, 3: 0, 5: 9, 6: 12}       # row -> EOS column; rows 1, 4 and 7 hold no EOS (truncated), row 2 ends in the last column, row 3 in the first
TRUNCATED = [1, 4, 7]


def completions(eos_rows):
    return sc_grpo.right_pad(fx.synth_completions(2 * G, C_ENG, fx.TINY, 321, eos_rows), CFG.pad_token_id)


def engine(ref=True, **kw):
    pol, rf = tri.stores()
    return SCGRPOEngine(CFG, pol, rf if ref else None, GRPOArgs(num_generations=G, max_prompt_length=4096, max_completion_length=C_ENG, seed=5, **kw)), pol


def scored(comp, ref=True, **kw):
    call = {k: kw.pop(k) for k in ("ref_logps", "old_logps", "is_weights", "rollout_logps") if k in kw}
    eng, pol = engine(ref, **kw)
    out = eng.loss_and_grads(tri.tiny_batch(), comp, tri.reward_fn(comp), **call)
    torch.cuda.synchronize()
    return out, pol.grad.clone()


def formula(out, loss_type, beta):
    """The float64 trl loss (on-policy form: exp(p - sg p) = 1) on the step's own tensors."""
    p = out["logps"].double().cpu()
    m = torch.from_numpy(np.asarray(out["completion_mask"])).double()
    A = out["advantages"].double().cpu()[:, None]
    ptl = -A.expand_as(p)
    if beta != 0:
        r = out["ref_logps"].double().cpu()
        ptl = ptl + beta * (torch.exp(r - p) - (r - p) - 1)
    return float(trl_loss(ptl, m, loss_type, p.shape[0], C_ENG))


def cosine(a, b):
    a, b = a.double(), b.double()
    return float((a * b).sum() / (a.norm() * b.norm()))


@pytest.mark.gpu
def test_loss_types_match_the_trl_formulas_and_do_not_depend_on_the_micro_batch():
    """(5) ragged completions: metrics["loss"] is the float64 formula within (1e-5, 1e-7) for each loss type; one group per micro-batch against the whole batch:
    the gradient at the tolerance of test_hip_model's micro-batch test (relative norm of the difference < 2e-2) and the loss at the same relative 2e-2, nothing
    added (the advantage part of the on-policy loss does not depend on the log-probs at all, so only the KL part can move)."""
    comp = completions(RAGGED)
    for lt in LOSS_TYPES:
        whole, g_whole = scored(comp, loss_type=lt)
        want = formula(whole, lt, BETA)
        print(f"[grpo objective] {lt}: loss {whole['metrics']['loss']:.9e} float64 {want:.9e}")
        close(torch.tensor(whole["metrics"]["loss"]), torch.tensor(want), 1e-5, 1e-7, f"{lt}: loss")
        part, g_part = scored(comp, loss_type=lt, micro_batch_seqs=G)
        close(torch.tensor(part["metrics"]["loss"]), torch.tensor(formula(part, lt, BETA)), 1e-5, 1e-7, f"{lt}: loss, one group per micro-batch")
        d_loss = abs(part["metrics"]["loss"] - whole["metrics"]["loss"]) / abs(whole["metrics"]["loss"])
        d_grad = float((g_part.double() - g_whole.double()).norm() / g_whole.double().norm())
        print(f"[grpo objective] {lt}: one group per micro-batch against the whole batch: loss differs by {d_loss:.3e} relative, gradient by {d_grad:.3e}")
        assert d_loss <= 2e-2 and d_grad < 2e-2, (lt, d_loss, d_grad)


@pytest.mark.gpu
def test_loss_types_agree_on_completions_of_full_length():
    """(5) every row max_completion_length long: the three normalisers are the same number, so the losses agree within 1e-6 relative and the gradient buffers of
    bnpo / dr_grpo have cosine > 0.999999 with grpo's."""
    comp = completions(None)
    res = {lt: scored(comp, loss_type=lt) for lt in LOSS_TYPES}
    base, g0 = res["grpo"]
    assert int(np.asarray(base["completion_mask"]).sum()) == comp.size and float(g0.abs().max()) > 0
    for lt in ("bnpo", "dr_grpo"):
        out, g = res[lt]
        assert abs(out["metrics"]["loss"] - base["metrics"]["loss"]) <= 1e-6 * abs(base["metrics"]["loss"]), lt
        assert cosine(g, g0) > 0.999999, lt


@pytest.mark.gpu
def test_truncated_completions_leave_the_loss():
    """(6)"""
    comp = completions(RAGGED)
    out, grad = scored(comp, beta=0.0, mask_truncated_completions=True)
    lm = np.asarray(out["completion_mask"])
    em = eos_completion_mask(comp, EOS)
    assert not lm[TRUNCATED].any() and np.array_equal(np.delete(lm, TRUNCATED, 0), np.delete(em, TRUNCATED, 0)) and em[TRUNCATED].all()
    assert out["metrics"]["completions/clipped_ratio"] == 3 / 8 and out["metrics"]["completion_length"] == float(em.sum(1).mean())
    plain, _ = scored(comp, beta=0.0)
    assert "completions/clipped_ratio" not in plain["metrics"] and np.array_equal(np.asarray(plain["completion_mask"]), em)
    # the same step on the remaining rows' loss terms: the EOS mask, the truncated rows' advantages zeroed, the same denominators
    keep = torch.ones(2 * G)
    keep[TRUNCATED] = 0
    adv0 = (out["advantages"] * keep).to(DEV)
    for lt in LOSS_TYPES:
        s = loss_row_scale(lt, lm, C_ENG)
        a = ops.grpo_loss_ex(out["logps"], out["advantages"].to(DEV), torch.from_numpy(lm).to(DEV), 0.0, row_scale=s)
        b = ops.grpo_loss_ex(out["logps"], adv0, torch.from_numpy(em).to(DEV), 0.0, row_scale=s)
        assert torch.equal(a[0], b[0]) and float(a[0].abs().max()) > 0, lt
    real = sc_grpo.group_advantages
    try:
        sc_grpo.group_advantages = lambda rewards, G_, scale=True: (real(rewards, G_, scale)[0] * keep, real(rewards, G_, scale)[1])
        _, grad0 = scored(comp, beta=0.0)
    finally:
        sc_grpo.group_advantages = real
    assert torch.equal(grad, grad0) and float(grad.abs().max()) > 0
    # a reuse step sees the same mask (and its metric denominators: the mean ratio over the loss mask's tokens is exactly 1 at unchanged weights)
    first, _ = scored(comp, mask_truncated_completions=True, num_iterations=2)
    again, _ = scored(comp, mask_truncated_completions=True, num_iterations=2, old_logps=first["logps"], ref_logps=first["ref_logps"])
    assert np.array_equal(np.asarray(again["completion_mask"]), lm) and again["metrics"]["policy/ratio_mean"] == 1.0 and again["metrics"]["loss"] == first["metrics"]["loss"]


@pytest.mark.gpu
@pytest.mark.parametrize("lt,beta", [("grpo", 0.0), ("bnpo", BETA), ("dr_grpo", BETA)])
def test_importance_weights_and_reuse_steps_compose_with_the_loss_types(lt, beta):
    """The engine's iadr1_grpo_loss_ex branch in its IS and clip forms (grpo reaches it with beta 0 only).  On-policy rollout log-probs under cap 2 and an
    on-policy reuse step are the plain step bit for bit (weights and ratios are exactly 1); rollout log-probs ln 4 below the scored ones make every live weight
    exactly 2, a power of two that commutes with every rounding downstream, and a reuse step handed those weights doubles the same way."""
    comp = completions(RAGGED)
    kw = dict(ref=beta != 0, beta=beta, loss_type=lt, num_iterations=2)
    base, g0 = scored(comp, **kw)
    loss0 = base["metrics"]["loss"]
    live = torch.from_numpy(np.asarray(base["completion_mask"])).to(F32)
    close(torch.tensor(loss0), torch.tensor(formula(base, lt, beta)), 1e-5, 1e-7, f"{lt}: loss")
    assert float(g0.abs().max()) > 0
    on, g1 = scored(comp, rollout_is_cap=CAP, rollout_logps=base["logps"], **kw)
    m = on["metrics"]
    assert m["loss"] == loss0 and torch.equal(g1, g0) and m.get("kl") == base["metrics"].get("kl")
    # (the logged means are float32 sums times the float32 reciprocal of the live count: the weights are exact, their mean within two roundings, 2 x 2^-24 relative)
    assert torch.equal(on["rollout_is_weights"].cpu(), live)
    assert abs(m["rollout/is_weight_mean"] - 1.0) <= ULP2 and m["rollout/is_clipped_frac"] == 0.0 and m["rollout/logp_abs_diff_max"] == 0.0
    two, g2 = scored(comp, rollout_is_cap=CAP, rollout_logps=base["logps"] - math.log(4.0), **kw)
    m = two["metrics"]
    assert torch.equal(two["rollout_is_weights"].cpu(), 2 * live) and abs(m["rollout/is_weight_mean"] - 2.0) <= 2 * ULP2 and abs(m["rollout/is_clipped_frac"] - 1.0) <= ULP2
    assert m["loss"] == 2 * loss0 and m.get("kl") == base["metrics"].get("kl") and torch.equal(g2, 2 * g0)
    again, g3 = scored(comp, old_logps=base["logps"], ref_logps=base["ref_logps"], **kw)
    m = again["metrics"]
    assert m["loss"] == loss0 and torch.equal(g3, g0) and abs(m["policy/ratio_mean"] - 1.0) <= ULP2 and m["clip_ratio/region_mean"] == 0.0 and m["policy/logp_abs_diff_max"] == 0.0
    assert np.array_equal(np.asarray(again["completion_mask"]), np.asarray(base["completion_mask"])) and (again["ref_logps"] is None) == (beta == 0)
    weighted, g4 = scored(comp, rollout_is_cap=CAP, old_logps=base["logps"], ref_logps=base["ref_logps"], is_weights=two["rollout_is_weights"], **kw)
    assert weighted["metrics"]["loss"] == 2 * loss0 and torch.equal(g4, g2) and abs(weighted["metrics"]["policy/ratio_mean"] - 1.0) <= ULP2


@pytest.mark.gpu
def test_unscaled_rewards_reach_the_step():
    """(7)"""
    comp = completions(RAGGED)
    out, _ = scored(comp, scale_rewards=False)
    r = out["rewards_per_func"].sum(1)
    assert torch.equal(out["advantages"], r - r.view(-1, G).mean(1).repeat_interleave(G)) and float(out["advantages"].abs().max()) > 0
    assert out["metrics"]["reward_std"] == float(r.view(-1, G).std(1).mean())


@pytest.mark.gpu
def test_a_step_without_a_reference_model(monkeypatch):
    """(8) engine level: built with ref=None, a full step with its rollout, no kl anywhere, the sequential structure, the advantage-only loss, and weights that move."""
    monkeypatch.delenv("IADR1_OVERLAP_CUS", raising=False)
    eng, pol = engine(ref=False, beta=0.0, learning_rate=1e-3)
    assert eng.ref is None
    before = pol.flat.clone()
    out = eng.step(tri.tiny_batch(), tri.reward_fn, do_optimizer_step=True, return_outputs=True)
    torch.cuda.synchronize()
    m = out["metrics"]
    assert "kl" not in m and out["ref_logps"] is None and out["kl"] is None and eng.last_step_shadowed is False and eng.shadow_logps is None
    want = formula(out, "grpo", 0.0)
    print(f"[grpo objective] beta 0: loss {m['loss']:.9e} float64 {want:.9e}")
    close(torch.tensor(m["loss"]), torch.tensor(want), 1e-5, 1e-7, "advantage-only loss")
    assert float(out["advantages"].abs().max()) > 0 and not torch.equal(before, pol.flat)
    monkeypatch.setenv("IADR1_OVERLAP_CUS", "64")
    with pytest.raises(ValueError, match="IADR1_OVERLAP_CUS"):
        eng.step(tri.tiny_batch(), tri.reward_fn, do_optimizer_step=False)
    monkeypatch.delenv("IADR1_OVERLAP_CUS")
    # given completions, every loss type, against the float64 advantage-only formula; a reference store that is handed in is not run either
    comp = completions(RAGGED)
    for lt in LOSS_TYPES:
        o, g = scored(comp, ref=False, beta=0.0, loss_type=lt)
        close(torch.tensor(o["metrics"]["loss"]), torch.tensor(formula(o, lt, 0.0)), 1e-5, 1e-7, f"{lt}: advantage-only loss")
        assert float(g.abs().max()) > 0 and "kl" not in o["metrics"]
    o2, g2 = scored(comp, ref=True, beta=0.0, loss_type="dr_grpo")
    assert o2["ref_logps"] is None and torch.equal(g2, g) and o2["metrics"]["loss"] == o["metrics"]["loss"]


@pytest.mark.gpu
def test_trainer_without_a_reference_model(tmp_path):
    """(8) trainer level: beta 0 builds no reference store; the two optimizer steps of one generation (num_iterations 2) log no kl and cache no reference
    log-probs; completions/clipped_ratio is a metric of the generation, logged once."""
    from iadr1_amd.trainer import GRPOConfig, SCGRPOTrainer
    gr = (1, 16, 12)
    ids, mask = fx.left_pad([fx.synth_prompt(gr, 5, fx.TINY, 177)], fx.TINY["pad_token_id"])
    part = {"input_ids": ids, "attention_mask": mask, "pixel_values": torch.from_numpy(fx.synth_pixel_values([gr], fx.TINY, seed=177)), "image_grid_thw": [gr]}

    class Proc:
        def apply_chat_template(self, conv, add_generation_prompt=True, tokenize=False):
            return "P"

        def __call__(self, text=None, images=None, **kw):
            return part

        def batch_decode(self, ids, skip_special_tokens=True):
            return ["x"] * len(ids)

    def spread(completions, **kw):
        return [float(i % 4) for i in range(len(completions))]

    tr = SCGRPOTrainer((CFG, fx.make_weights(fx.TINY, 0)), [spread], processing_class=Proc(),
                       args=GRPOConfig(output_dir=str(tmp_path / "out"), num_generations=4, max_completion_length=12, max_prompt_length=4096, per_device_train_batch_size=1,
                                       save_steps=0, learning_rate=1e-3, beta=0.0, loss_type="dr_grpo", mask_truncated_completions=True, num_iterations=2))
    assert tr.ref is None and tr.engine.ref is None and tr.engine.args.loss_type == "dr_grpo" and tr.engine.args.mask_truncated_completions is True
    # a random-init model samples next to no EOS in 12 tokens, which would mask every row: the generation's completions are the test's, handed to the engine's step
    # the way a batched rollout's are (completions=); row 1 holds no EOS, the others have 6, 12 and 1 live tokens
    comp = sc_grpo.right_pad(fx.synth_completions(4, 12, fx.TINY, 99, {0: 5, 2: 11, 3: 0}), CFG.pad_token_id)
    real = tr.engine.step

    def step(batch, reward_fn, **kw):
        if kw.get("completions") is None:
            kw["completions"] = comp
        return real(batch, reward_fn, **kw)

    tr.engine.step = step
    micro = [[{"prompt": tgc.CHAT, "image": [("synthetic", 0)], "solution": "s"}]]
    before = tr.policy.flat.clone()
    losses = tr.training_step(micro)
    moved = not torch.equal(before, tr.policy.flat)
    losses = losses + tr.training_step(micro)
    assert tr.state.global_step == 2 and all(np.isfinite(l) for l in losses) and moved
    assert "kl" not in tr._metrics and len(tr._metrics["reward"]) == 1 and len(tr._metrics["policy/ratio_mean"]) == 1
    gen = tr._generation[0]
    assert gen["ref_logps"] is None and np.array_equal(gen["completions"], comp) and tr._metrics["completions/clipped_ratio"] == [0.25]
    # the first step's loss is trl's dr_grpo on the loss mask (beta 0, on policy: the per-token loss is -A): -sum_n A_n live_n / (rows x max_completion_length)
    adv = group_advantages(gen["rewards_per_func"].sum(1), 4)[0].double()
    want = float(-(adv * torch.tensor([6.0, 0.0, 12.0, 1.0]).double()).sum() / (4 * 12))
    print(f"[grpo objective] trainer, dr_grpo with the truncation mask: loss {losses[0]:.9e} float64 {want:.9e}; reuse step {losses[1]:.9e}")
    assert abs(want) > 1e-2
    close(torch.tensor(losses[0]), torch.tensor(want), 1e-5, 1e-7, "trainer: dr_grpo loss")
    tr.log({"loss": float(np.mean(losses))})
    assert "kl" not in tr.log_history[-1] and "reward" in tr.log_history[-1]
