"""SC-GRPO micro-step on the HIP engine: the arithmetic of `SCGRPOTrainer.compute_loss`
(/root/reference/train/stage_rl/trainer/sc_grpo_trainer.py:586-819) + backward + optimizer, re-scheduled for
one MI355X per rank:

  rollout (in-process, shared weights, hipGraph decode)  ->  rewards (CPU plugin functions)  ->
  advantages (per-prompt groups, rank-local)  ->  frozen-ref log-probs  ->  policy log-probs + backward  ->
  bucketed gradient all-reduce over RCCL (overlapped with the tail of backward)  ->  fused AdamW.

With GRPOArgs.num_iterations > 1 the caller reuses a rollout for that many optimizer steps: the steps after the first hand the completions back with the
log-probs the first one scored (old_logps), and the loss is trl's clipped surrogate (iadr1_grpo_loss_clip; REF trl/trl/trainer/grpo_trainer.py:1203-1213).

Ordering: sequences are laid out prompt-major (p0 x G, p1 x G, ...) everywhere, i.e. the interleaved order the
reference's reward / advantage code assumes (REF:754,775-792); its tensor tiling (REF:625-628) coincides with
this at per_device_train_batch_size=1, the only setting its scripts use.
"""
from __future__ import annotations

import math
import os
import sys

from dataclasses import dataclass

import numpy as np
import torch

from . import hip, ops
from .overlap import ChunkedRefPass
from .params import ParamStore, VLMConfig
from .rollout import Rollout
from .vlm import Engine

BF16, F32 = torch.bfloat16, torch.float32


@dataclass
class GRPOArgs:
    """The subset of trl.GRPOConfig / TrainingArguments the reference's SC-GRPO path actually reads
    (SURVEY.md section 2.1 #12 and section 5), with the same defaults."""
    num_generations: int = 8
    max_prompt_length: int | None = 512
    max_completion_length: int = 256
    beta: float = 0.04
    temperature: float = 0.9
    top_k: int = 50            # hard-coded in the reference (REF:353-358); <= 0: the whole vocabulary (needs top_p == 1.0, checked when the engine is built)
    top_p: float = 0.9
    # trl.GRPOConfig's names (REF trl/trl/trainer/grpo_config.py).  Both are filters of the rollout's sampler (iadr1_sample_ex), applied in transformers' order --
    # repetition penalty, temperature, top-k, top-p, min_p -- and both are off by default: the rollout then issues the launches it always has.  The loss does not
    # change; the rollout's log-probs (rollout_logps, rollout_is_cap) stay temperature-1, unpenalised and unfiltered.
    # min_p in [0, 1) (None: 0): a token stays iff its probability is >= min_p x the most likely token's; the one truncation top_k <= 0 can be combined with.
    # repetition_penalty (finite, > 0; 1 = off): logits of the tokens a sequence has already seen (prompt, image placeholders included, and its completion so
    # far) are divided by it when positive and multiplied when negative (transformers' RepetitionPenaltyLogitsProcessor).  Greedy rollouts keep it and drop min_p.
    min_p: float | None = 0.0
    repetition_penalty: float = 1.0
    # a guide.TokenGuide (trl's vllm_guided_decoding_regex, compiled by SCGRPOTrainer) or None: the rollout samples only tokens that keep the completion a prefix
    # of a match of the pattern, EOS only where it matches (iadr1_sample_guided).  Only which ids get sampled changes: the loss, the rollout's log-probs (raw row,
    # no mask) and the training arena are what they are without it.  Not with suppress_eos.
    guide: object | None = None
    # the rollout also returns the log-prob of every token it sampled (unfiltered, at the temperature the loss scores at -- 1 unless logps_at_temperature: the
    # quantity the loss scores); the step's metrics gain
    # rollout/logp_abs_diff_mean, rollout/logp_abs_diff_max and rollout/kl against the policy log-probs of the loss.  Nothing in the loss or the gradients changes.
    rollout_logps: bool = False
    # truncated importance weight against the rollout's log-probs (0 = off: the loss does not read them).  cap >= 1: every per-token loss term is multiplied by
    # w = min(exp(scored - sampled), cap), per token ("token") or with the row's mean log-ratio ("sequence"); w is a constant under differentiation
    # (iadr1_grpo_loss_is).  Implies what rollout_logps asks of the rollout; the rollout/* metrics then come from the kernel's partials, plus rollout/is_weight_mean
    # and rollout/is_clipped_frac.  Corrects the sampler-engine / trainer mismatch only (both sides unfiltered and at the same temperature: 1, or `temperature` with
    # logps_at_temperature), not top-k / top-p nor, by default, the sampler's temperature.
    rollout_is_cap: float = 0.0
    rollout_is_level: str = "token"
    # the rollout also returns the entropy of the distribution every token was sampled from (iadr1_sample_ent: softmax of the raw logits row at temperature 1 -- at `temperature` with logps_at_temperature --, the
    # distribution rollout_logps is taken under); the step's metrics gain `entropy` (trl's key), its mean over the live completion tokens.  An APPROXIMATION of
    # trl's number: these are the decode engine's logits under the policy that sampled, not a second forward, and they are fixed per generation where trl
    # recomputes them on every reuse step.  Nothing in the loss or the gradients changes.
    rollout_entropy: bool = False
    # trl.GRPOConfig's name: the advantage term of the loss is trained only on the share rho of the live completion tokens (of all ranks) with the highest
    # rollout entropy -- keep = entropy >= quantile(1 - rho), ties kept; the KL term stays on every live token (iadr1_grpo_loss_sel).  In [0, 1], 1 = off.  A
    # value below 1 implies what rollout_entropy asks of the rollout; metrics entropy/threshold and entropy/kept_frac.
    top_entropy_quantile: float = 1.0
    # trl.GRPOConfig's names and defaults (REF trl/trl/trainer/grpo_config.py; the reference's SC-GRPO path never sets them, so reuse is off by default).
    # num_iterations (mu) > 1: the caller (SCGRPOTrainer.training_step) uses every rollout for mu consecutive optimizer steps; steps 1 .. mu-1 hand the log-probs
    # iteration 0 scored back as old_logps, and the loss is the clipped surrogate -min(r A, clamp(r, 1 - epsilon, 1 + epsilon_high) A) + beta kl with
    # r = exp(logp - old_logp) (iadr1_grpo_loss_clip; REF trl/trl/trainer/grpo_trainer.py:1203-1210).  epsilon_high None: epsilon.
    num_iterations: int = 1
    epsilon: float = 0.2
    epsilon_high: float | None = None
    # how a step's per-token terms are normalised (REF trl/trl/trainer/grpo_trainer.py:1212-1219): "grpo" = every row a mean over its own live tokens, then the mean
    # over rows; "bnpo" = the sum over the step's rows divided by their live tokens; "dr_grpo" = divided by rows x max_completion_length.  The default is "grpo", not
    # trl's "bnpo": that is what the reference's trainer computes (sc_grpo_trainer.py:796-798).  Anything but "grpo" is a row_scale > 0 of iadr1_grpo_loss_ex (loss_row_scale).
    loss_type: str = "grpo"
    # False: advantages = reward - group mean, not divided by the group's std + 1e-4 (REF ...grpo_trainer.py:1080-1082); reward_std is logged either way
    scale_rewards: bool = True
    # a completion that reached max_completion_length without an EOS drops out of the loss: its row of the loss mask is zeroed (REF ...grpo_trainer.py:983-986), and
    # the step logs completions/clipped_ratio, the share of such rows (REF ...grpo_trainer.py:1105)
    mask_truncated_completions: bool = False
    # trl's definition of every log-prob (REF trl/trl/trainer/grpo_trainer.py:818-821: logits / temperature before the log-softmax, for the policy, the old policy and
    # the reference alike).  False: temperature 1, what the reference's trainer computes (sc_grpo_trainer.py:505-513).  True: with T = `temperature`, the policy's and
    # the reference's log-probs, the cached old_logps, the rollout's log-probs and entropies are all taken under softmax(x / T) (iadr1_linear_logprob_fwd_t /
    # _dlogits_t, iadr1_sample_ent_t), and with them everything derived: the KL term and metric, the clip ratios, rollout/*, the IS weights, `entropy` and the
    # top_entropy_quantile threshold.  Which tokens get sampled does not change.  T is `temperature` also on a greedy rollout (the sampler's 0 is its own).
    logps_at_temperature: bool = False
    # trl.GRPOConfig's names and defaults (REF trl/trl/trainer/grpo_config.py:369-390; SyncRefModelCallback, REF trl/trl/trainer/callbacks.py:93-131): the TR-DPO
    # reference update.  After every ref_model_sync_steps-th optimizer step (optimizer_step: the step counter after its increment, every step of a reused rollout
    # counts) the reference's flat buffer becomes ref_model_mixup_alpha * policy + (1 - alpha) * reference in one launch (ParamStore.mix_from, iadr1_ref_mix); that
    # step's metrics gain ref/policy_dist, the relative L2 distance |policy - reference| / |reference| before the mix, and ref/syncs, the number of syncs so far.
    # Reference log-probs a generation cached (num_iterations > 1) stay what they were scored as, as in trl.  Off: the step issues the launches it always has; the
    # other two fields are then accepted and ignored, as in trl.  Refused with beta == 0 (there is no reference to move; trl silently does nothing).
    sync_ref_model: bool = False
    ref_model_mixup_alpha: float = 0.6
    ref_model_sync_steps: int = 512
    learning_rate: float = 1e-6
    weight_decay: float = 0.0
    adam_beta1: float = 0.9
    adam_beta2: float = 0.999
    adam_epsilon: float = 1e-8
    max_grad_norm: float = 1.0
    gradient_accumulation_steps: int = 1
    micro_batch_seqs: int = 16  # sequences per forward/backward pass (activation memory knob; results do not depend on it)
    seed: int = 42
    suppress_eos: bool = False  # benchmark mode: fixed-length completions
    use_hip_graph: bool = True
    # compute every prompt once per group in the reference / policy passes (shared-prefix attention; same math as the
    # reference's G-fold repeated rows).  Off: IADR1_SHARE_PREFIX=0 or share_prefix=False.
    share_prefix: bool = os.environ.get("IADR1_SHARE_PREFIX", "1") != "0"
    # let the rollout's prefill double as the prompt part of the policy's training forward (needs share_prefix and one whole-batch micro-batch)
    reuse_prefill: bool = os.environ.get("IADR1_REUSE_PREFILL", "1") != "0"
    # the rollout's decode steps also write the completion rows of the policy's activation arena, so the policy forward over the completions is not
    # run before backward (needs reuse_prefill's conditions and the fused decode kernels)
    reuse_decode: bool = os.environ.get("IADR1_REUSE_DECODE", "1") != "0"
    # LLaVA branches only: reproduce the reference's `_ensure_left_padding_data` (REF:502-504,516-567) -- a row whose completion ended early (right
    # padding, no left padding) is rotated before the model runs while the log-probs are still sliced / masked at the un-rotated columns, so its
    # loss terms are the log-probs of the tokens `C - len` positions EARLIER (the end of the prompt, then the start of the completion).  False
    # scores the completion tokens themselves, as the Qwen branches do.
    llava_rotate_right_padded_rows: bool = True
    # `--gradient_checkpointing` (REF scripts/train/SC_GRPO/*.sh:56): "off" | "auto" | "on" -- vlm.Engine.recompute_wanted.  With recomputation the policy's
    # forward is run after the rollout (the rollout's own activations are not kept either)
    recompute: str = "off"

    @property
    def logp_temperature(self) -> float:
        """The temperature every log-prob and entropy of the step is taken at."""
        return float(self.temperature) if self.logps_at_temperature else 1.0

    @property
    def wants_rollout_logps(self) -> bool:
        return self.rollout_logps or self.rollout_is_cap > 0

    @property
    def wants_rollout_entropy(self) -> bool:
        return self.rollout_entropy or self.top_entropy_quantile < 1.0


def check_reuse_args(who: str, num_iterations, epsilon, epsilon_high):
    """num_iterations / epsilon / epsilon_high of GRPOArgs and GRPOConfig (`who` names the class in the message)."""
    if not (isinstance(num_iterations, int) and num_iterations >= 1):
        raise ValueError(f"{who}.num_iterations must be an integer >= 1 (got {num_iterations!r})")
    if not (math.isfinite(epsilon) and 0.0 <= epsilon < 1.0):
        raise ValueError(f"{who}.epsilon must be finite and in [0, 1) (got {epsilon}): the lower clip bound 1 - epsilon of a probability ratio must stay positive")
    if epsilon_high is not None and not (math.isfinite(epsilon_high) and epsilon_high >= 0.0):
        raise ValueError(f"{who}.epsilon_high must be None (= epsilon) or finite and >= 0 (got {epsilon_high})")


def check_sampler_args(who: str, min_p, repetition_penalty):
    """min_p / repetition_penalty of GRPOArgs and GRPOConfig (`who` names the class in the message): the ranges iadr1_sample_ex accepts.  Returns min_p with
    trl's None read as 0."""
    mp = 0.0 if min_p is None else float(min_p)
    if not (0.0 <= mp < 1.0):       # (a NaN fails both compares)
        raise ValueError(f"{who}.min_p must be in [0, 1) or None (got {min_p}): it is a fraction of the most likely token's probability, and 1 would keep that token only")
    if not (math.isfinite(repetition_penalty) and repetition_penalty > 0.0):
        raise ValueError(f"{who}.repetition_penalty must be finite and > 0 (got {repetition_penalty}); 1 switches it off")
    return mp


def check_entropy_args(who: str, top_entropy_quantile, llava_rotated: bool = False):
    """top_entropy_quantile of GRPOArgs and GRPOConfig (`who` names the class in the message).  llava_rotated: the engine scores the rotated window of
    llava_rotate_right_padded_rows, whose columns are not the rollout's."""
    q = top_entropy_quantile
    if isinstance(q, bool) or not isinstance(q, (int, float)) or not (0.0 <= float(q) <= 1.0):      # (a NaN fails both compares)
        raise ValueError(f"{who}.top_entropy_quantile must be in [0, 1] (got {q!r}): it is the share of the live completion tokens whose advantage term is trained; 1 = off")
    if q < 1.0 and llava_rotated:
        raise ValueError(f"{who}.top_entropy_quantile with llava_rotate_right_padded_rows: that path scores a rotated window, whose columns do not line up with the "
                         "rollout's entropies; set llava_rotate_right_padded_rows=False to select among the completion tokens themselves")


def entropy_keep_mask(ent, live, rho: float, group=None):
    """trl's get_high_entropy_mask.  ent [N, C] float, live [N, C] bool (a tensor on any device, or a host array): returns (keep [N, C] bool on ent's device, tau),
    tau = torch.quantile(live entropies of ALL ranks as float32, 1 - rho) with linear interpolation and keep = live & (ent >= tau): ties at the threshold are
    kept.  No live token anywhere: keep is all False and tau is +inf.  group: a torch.distributed process group -- the [N, C] entropies are all-gathered with the
    dead positions at -1 (an entropy is >= 0), N and C equal on every rank.
    Without a group the live indices are taken from `live` on the HOST (a host-resident mask costs nothing; a device one is read back), so that forming the
    live entropies waits for nothing on the device; with one, the other ranks' masks are only known from the gathered values (one read-back of their count)."""
    rho = float(rho)
    if not (0.0 <= rho <= 1.0):
        raise ValueError(f"entropy_keep_mask: rho must be in [0, 1] (got {rho})")
    live_h = live.detach().cpu().numpy().astype(bool) if isinstance(live, torch.Tensor) else np.asarray(live).astype(bool)
    assert tuple(ent.shape) == live_h.shape and ent.dim() == 2, f"entropy_keep_mask: ent {tuple(ent.shape)} and live {live_h.shape} must be the same [N, C]"
    dev = ent.device
    ent32 = ent.detach().to(F32)
    if dev.type == "cuda":
        live_d = ops.h2d(live_h, dev)
        idx = ops.h2d(np.flatnonzero(live_h).astype(np.int64), dev)
    else:
        live_d, idx = torch.from_numpy(live_h), torch.from_numpy(np.flatnonzero(live_h).astype(np.int64))
    if group is None:
        e_live = ent32.reshape(-1).index_select(0, idx)
    else:
        import torch.distributed as dist
        mine = torch.where(live_d, ent32, torch.full_like(ent32, -1.0)).contiguous()
        if dev.type == "cuda" and dist.get_backend(group) == "gloo":
            mine = mine.cpu()
        parts = [torch.empty_like(mine) for _ in range(dist.get_world_size(group))]
        dist.all_gather(parts, mine, group=group)
        every = torch.cat([t.reshape(-1) for t in parts]).to(dev)
        e_live = every[every >= 0]
    if e_live.numel() == 0:
        return torch.zeros_like(live_d), torch.full((), float("inf"), dtype=F32, device=dev)
    tau = torch.quantile(e_live, 1.0 - rho, interpolation="linear")
    return live_d & (ent32 >= tau), tau


def check_sync_ref_args(who: str, sync_ref_model, ref_model_mixup_alpha, ref_model_sync_steps, beta):
    """sync_ref_model / ref_model_mixup_alpha / ref_model_sync_steps of GRPOArgs and GRPOConfig (`who` names the class in the message).  With sync_ref_model off the
    other two are not looked at (trl ignores them too)."""
    if not sync_ref_model:
        return
    if beta == 0:
        raise ValueError(f"{who}.sync_ref_model with beta == 0: there is no reference model to move (no KL term, no frozen copy is built); trl silently does nothing "
                         "here -- drop sync_ref_model or set beta > 0")
    al = ref_model_mixup_alpha
    if isinstance(al, bool) or not isinstance(al, (int, float)) or not (math.isfinite(al) and 0.0 < al <= 1.0):
        raise ValueError(f"{who}.ref_model_mixup_alpha must be finite and in (0, 1] (got {al!r}): the share of the policy in the new reference; 1 copies the policy")
    n = ref_model_sync_steps
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"{who}.ref_model_sync_steps must be an integer >= 1 (got {n!r}): the reference moves after every n-th optimizer step")


def ref_sync_due(opt_step: int, ref_model_sync_steps: int) -> bool:
    """trl's on_step_end rule (REF trl/trl/trainer/callbacks.py:127): the reference is mixed at the end of optimizer step number `opt_step` (1-based: the counter
    after its increment) iff it is a multiple of ref_model_sync_steps."""
    return opt_step % ref_model_sync_steps == 0


LOSS_TYPES = ("grpo", "bnpo", "dr_grpo")


def check_objective_args(who: str, loss_type, mask_truncated_completions=False, suppress_eos=False):
    """loss_type / mask_truncated_completions of GRPOArgs and GRPOConfig (`who` names the class in the message)."""
    if loss_type not in LOSS_TYPES:
        raise ValueError(f"{who}.loss_type must be one of {list(LOSS_TYPES)} (got {loss_type!r})")
    if mask_truncated_completions and suppress_eos:
        raise ValueError(f"{who}.mask_truncated_completions with suppress_eos: no completion can end in an EOS, so every row would be masked and the step would have no loss")


def eos_completion_mask(completion_ids: np.ndarray, eos_token_id: int) -> np.ndarray:
    """REF:722-726 -- keep tokens up to and including the first EOS."""
    is_eos = completion_ids == eos_token_id
    n, c = is_eos.shape
    eos_idx = np.where(is_eos.any(1), is_eos.argmax(1), c)
    return (np.arange(c)[None, :] <= eos_idx[:, None]).astype(np.int32)


def truncation_loss_mask(cmask: np.ndarray, completion_ids: np.ndarray, eos_token_id: int) -> np.ndarray:
    """REF trl/trl/trainer/grpo_trainer.py:983-986 -- the EOS mask with the rows that hold no EOS zeroed."""
    has_eos = (np.asarray(completion_ids) == eos_token_id).any(1)
    return cmask * has_eos[:, None].astype(cmask.dtype)


def loss_row_scale(loss_type: str, loss_mask: np.ndarray, max_completion_length: int) -> float:
    """The row_scale of iadr1_grpo_loss_ex for one step's [N, C] loss mask, so that the mean of its row_loss over the N rows is trl's loss (REF
    trl/trl/trainer/grpo_trainer.py:1213 / 1215 / 1217): 0 for "grpo" (the kernel divides every row by its own live tokens), N / max(live tokens, 1) for "bnpo",
    1 / max_completion_length for "dr_grpo".  Computed in float64 and rounded once to the float32 the kernel takes."""
    if loss_type == "grpo":
        return 0.0
    if loss_type == "bnpo":
        return float(np.float32(np.float64(loss_mask.shape[0]) / np.float64(max(int(np.asarray(loss_mask, dtype=np.int64).sum()), 1))))
    if loss_type == "dr_grpo":
        return float(np.float32(np.float64(1.0) / np.float64(max_completion_length)))
    raise ValueError(f"loss_type must be one of {list(LOSS_TYPES)} (got {loss_type!r})")


def pad(rows, padding_value=0, padding_side: str = "right", pad_to_multiple_of: int | None = None) -> np.ndarray:
    """trl `pad` (REF trl/trl/trainer/utils.py:418-478): stack arrays of possibly different shape into one, every dimension grown to the
    largest (dimension 0 rounded up to `pad_to_multiple_of`), the data of each row at the start ("right" padding) or the end ("left") of
    dimension 0, `padding_value` elsewhere."""
    arrs = [np.asarray(r) for r in rows]
    if not arrs:
        return np.zeros((0, 0), dtype=np.int64)
    shape = list(np.max([a.shape for a in arrs], 0))
    if pad_to_multiple_of is not None:
        shape[0] += (-shape[0]) % pad_to_multiple_of
    out = np.full((len(arrs), *shape), padding_value, dtype=arrs[0].dtype)
    for i, a in enumerate(arrs):
        if padding_side == "left":
            first = slice(shape[0] - a.shape[0], shape[0])
        elif padding_side == "right":
            first = slice(0, a.shape[0])
        else:
            raise ValueError("padding_side must be 'left' or 'right'")
        out[(i, first, *[slice(0, n) for n in a.shape[1:]])] = a
    return out


def right_pad(rows, pad_value: int) -> np.ndarray:
    """The call at REF:682: completion id lists, right-padded with the pad token."""
    return pad([np.asarray(r, dtype=np.int64) for r in rows], pad_value, "right").astype(np.int64).reshape(len(rows), -1)


def right_padding_shift(row_ids: np.ndarray, pad_token_id: int) -> int:
    """The trigger of the reference's `_ensure_left_padding_data` (REF:534-541), on the ids alone: the first pad token of the [prompt | completion] row
    starts an all-pad suffix -> that many columns are rotated to the front (returned); otherwise (no pad, left padding, a pad inside the text) the row is
    left alone (0).  Derived from the ids like the reference, not from the EOS mask: a supplied completion that is shorter than C without an EOS is
    rotated too, and with pad == EOS the EOS itself moves into the padding."""
    pads = np.flatnonzero(row_ids == pad_token_id)
    if pads.size == 0:
        return 0
    first = int(pads[0])
    return int(len(row_ids) - first) if bool((row_ids[first:] == pad_token_id).all()) else 0


def group_advantages(rewards: torch.Tensor, G: int, scale: bool = True):
    """REF:787-793: group mean, UNBIASED std, eps 1e-4.  scale False (REF trl/trl/trainer/grpo_trainer.py:1080-1082 with scale_rewards off): rewards - group mean;
    the std is returned either way."""
    r = rewards.view(-1, G)
    mean = r.mean(1).repeat_interleave(G)
    std = r.std(1).repeat_interleave(G) if G > 1 else torch.zeros_like(mean)
    if not scale:
        return rewards - mean, std
    return (rewards - mean) / (std + 1e-4), std


class GradReducer:
    """Data-parallel gradient exchange: the ONLY collective of the data path.  The flat fp32 gradient buffer is
    all-reduced in contiguous buckets of at most `bucket_bytes` on the wire (256 MB: large enough to run at link rate, small enough that the
    first bucket leaves while backward is still producing the next) on a side stream; decoder-layer ranges are launched as soon as the last
    micro-batch's backward has left that layer, so the exchange overlaps the rest of backward.

    Wire type: bf16 by default -- what the reference moves (DeepSpeed ZeRO-3 reduce-scatters the bf16 gradients of a bf16 model,
    scripts/train/zero3.json + `--bf16`) and half the bytes over xGMI (7.5 GB instead of 15 GB for the 3B model): each bucket is cast into a bf16
    staging buffer, summed there by RCCL, and cast back into the fp32 gradient buffer, all stream-ordered on the side stream.
    IADR1_REDUCE_DTYPE=fp32 (or wire="fp32") sums the fp32 buffer in place.  Ring / tree all-reduce leaves bit-identical sums on every rank
    either way, so the replicas' parameters stay bit-identical.  The bucket sequence depends on the parameter layout only, never on a rank's
    data.  Works on CPU / gloo too (tests)."""

    RING = 3        # bf16 staging buffers of one bucket each: one being cast into, one on the wire, one being cast back

    def __init__(self, store: ParamStore, group=None, bucket_bytes: int = 256 << 20, wire: str | None = None):
        import torch.distributed as dist
        self.dist, self.store, self.group = dist, store, group
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        self.cuda = store.grad.is_cuda
        # IADR1_FORCE_REDUCE=1: run the exchange even in a one-rank group (exercises the side-stream / bucket / RCCL path on a single GPU)
        self.active = self.world > 1 or (bool(os.environ.get("IADR1_FORCE_REDUCE")) and dist.is_available() and dist.is_initialized())
        self.stream = torch.cuda.Stream() if (self.cuda and self.active) else None
        self.wire = (wire or os.environ.get("IADR1_REDUCE_DTYPE", "bf16")).lower()
        if self.wire not in ("bf16", "fp32"):
            raise ValueError("IADR1_REDUCE_DTYPE must be bf16 or fp32")
        # collective per bucket: "all_reduce" (the library picks ring / tree), or "rs_ag": reduce_scatter_tensor + all_gather_into_tensor -- the two halves of an
        # all-reduce issued explicitly, which on the fully connected xGMI mesh of one node can run as direct exchanges (every rank sends 1/N of the bucket to every
        # peer at once: SURVEY section 5 estimates ~12 ms against ~86 ms for a ring over 7.5 GB).  Bit-identical sums on every rank either way (each shard is reduced
        # on ONE rank, then copied).  Needs a backend with reduce_scatter_tensor (RCCL); on others (gloo, the CPU tests) the request falls back to all_reduce.
        self.algo = os.environ.get("IADR1_REDUCE_ALGO", "all_reduce").lower()
        if self.algo not in ("all_reduce", "rs_ag"):
            raise ValueError("IADR1_REDUCE_ALGO must be all_reduce or rs_ag")
        if self.algo == "rs_ag" and not (self.active and self.cuda and dist.get_backend(group) == "nccl"):
            self.algo = "all_reduce"
        pad = 8 * self.world                    # rs_ag: equal 16-byte aligned shards
        self.bucket_elems = max(1, min(int(bucket_bytes) // (2 if self.wire == "bf16" else 4), store.n_total))
        if self.algo == "rs_ag":
            self.bucket_elems = (self.bucket_elems + pad - 1) // pad * pad
        # staging: a RING of bucket-sized bf16 buffers (<= 768 MB), not a second copy of the model (16.6 GB at 7B, which the 7B / LLaVA-OneVision
        # configurations do not have to spare next to 245 GB of training state).  A buffer is reused only after its previous bucket has been cast
        # back into the fp32 gradient buffer -- stream order on the side stream guarantees it (the cast-back is enqueued before the next cast-in)
        self.ring = [torch.empty(self.bucket_elems, dtype=BF16, device=store.grad.device) for _ in range(self.RING)] if (self.active and self.wire == "bf16") else None
        if self.active and self.algo == "rs_ag" and self.ring is None:        # fp32 wire: the padded bucket is staged too (the gradient buffer's tail is not a multiple of the shard)
            self.ring = [torch.empty(self.bucket_elems, dtype=F32, device=store.grad.device) for _ in range(self.RING)]
        self.pending = [None] * self.RING
        self.slot = 0
        self.bytes_on_wire = 0          # per step, for the bench line
        self.n_buckets = 0
        c = store.cfg
        s = store.slots
        self.layer_range = []
        for i in range(c.num_hidden_layers):
            lo = s[f"layers.{i}.qkv.w"].offset
            hi = s[f"layers.{i + 1}.qkv.w"].offset if i + 1 < c.num_hidden_layers else (s["lm_head"].offset if "lm_head" in s else store.n_decay)
            self.layer_range.append((lo, hi))
        self.first_layer_off = s["layers.0.qkv.w"].offset
        self.reset()

    def exposed_ms(self) -> float | None:
        """Milliseconds of the LAST finish() that the compute stream waited for the exchange (synchronises on the second event); None without an exchange."""
        ev = self.__dict__.get("_exposed_events")
        if ev is None:
            return None
        ev[1].synchronize()
        return float(ev[0].elapsed_time(ev[1]))

    def staging_bytes(self) -> int:
        """Device memory the exchange adds to the training state."""
        return 0 if self.ring is None else sum(r.numel() * r.element_size() for r in self.ring)

    def reset(self):
        self.done = []

    def _complete(self, k):
        """Bucket in ring slot k: wait for its collective (stream-ordered on RCCL: the side stream waits, the host does not), cast the sum back."""
        p = self.pending[k]
        if p is None:
            return
        work, st, lo, hi = p
        work.wait()
        g = self.store.grad[lo:hi]
        if st.dtype == F32:
            g.copy_(st[: hi - lo])
        elif self.cuda:
            hip.call("cast_bf16_to_f32", st, g, hi - lo)
        else:
            g.copy_(st[: hi - lo])
        self.pending[k] = None

    def _bucket(self, lo, hi):
        g = self.store.grad[lo:hi]
        if self.ring is None:
            self.dist.all_reduce(g, group=self.group)
            return
        k = self.slot
        self.slot = (k + 1) % self.RING
        self._complete(k)                  # the slot's previous bucket (RING buckets ago) leaves the buffer first
        n = hi - lo
        st = self.ring[k][:n]
        if st.dtype == F32:
            st.copy_(g)
        elif self.cuda:   # fp32 -> bf16 (round to nearest even) and back through the library's cast kernels
            hip.call("cast_f32_to_bf16", g, n, st, n, 1, n, n)
        else:
            st.copy_(g)
        if self.algo == "rs_ag":
            # the bucket padded to world equal shards (the pad is zeroed: it is summed and gathered like data, nobody reads it back)
            npad = (n + 8 * self.world - 1) // (8 * self.world) * (8 * self.world)
            full = self.ring[k][:npad]
            if npad > n:
                full[n:].zero_()
            shard = full.view(self.world, -1)[self.dist.get_rank(self.group)]
            self.dist.reduce_scatter_tensor(shard, full, group=self.group, async_op=True)       # in place: rank r's shard of `full` receives the sum (NCCL's in-place form)
            work = self.dist.all_gather_into_tensor(full, shard, group=self.group, async_op=True)   # same communicator, same stream: ordered behind the reduce-scatter
            self.pending[k] = (work, st, lo, hi)
            return
        self.pending[k] = (self.dist.all_reduce(st, group=self.group, async_op=True), st, lo, hi)

    def _drain(self):
        for i in range(self.RING):         # oldest first
            self._complete((self.slot + i) % self.RING)

    def _reduce(self, lo, hi, drain=False):
        if not self.active or (hi <= lo and not drain):
            return
        if self.stream is not None:
            self.stream.wait_stream(torch.cuda.current_stream())
        ctx = torch.cuda.stream(self.stream) if self.stream is not None else _nullcontext()
        with ctx:
            for b0 in range(lo, hi, self.bucket_elems):
                b1 = min(hi, b0 + self.bucket_elems)
                self._bucket(b0, b1)      # on RCCL the collective is enqueued behind this stream's work: no host block
                self.bytes_on_wire += (b1 - b0) * (2 if self.wire == "bf16" else 4)
                self.n_buckets += 1
            if drain:
                self._drain()
        if hi > lo:
            self.done.append((lo, hi))

    def layer_ready(self, i):
        self._reduce(*self.layer_range[i])

    def all_layers_ready(self):
        """The decoder-layer ranges in backward order -- for a last micro-batch that ran no backward on this rank (nothing supervised in it): the
        bucket sequence must be the same on every rank whatever the rank-local data was."""
        sent = set(self.done)
        for i in reversed(range(len(self.layer_range))):
            if self.layer_range[i] not in sent:
                self.layer_ready(i)

    def finish(self):
        """Reduce whatever has not been sent yet (vision tower, embedding, lm_head, norm gains / biases) and join.
        `exposed_ms()` afterwards: GPU time the compute stream spent waiting here for the exchange -- the part of the collective that did NOT hide under backward
        (two events on the compute stream: at entry = end of backward in stream order, and behind the join)."""
        ev = None
        if self.stream is not None and self.active:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        self.all_layers_ready()
        covered = sorted(self.done)
        cur = 0
        for lo, hi in covered + [(self.store.n_total, self.store.n_total)]:
            if lo > cur:
                self._reduce(cur, lo)
            cur = max(cur, hi)
        self._reduce(0, 0, drain=True)      # the buckets still in the ring: wait + cast back
        if self.stream is not None:
            torch.cuda.current_stream().wait_stream(self.stream)
        if ev is not None:
            ev[1].record()
            self._exposed_events = ev
        self.last_bytes_on_wire, self.last_n_buckets = self.bytes_on_wire, self.n_buckets
        self.bytes_on_wire = self.n_buckets = 0
        self.reset()


class _nullcontext:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


class SCGRPOEngine:
    def __init__(self, cfg: VLMConfig, policy: ParamStore, ref: ParamStore | None, args: GRPOArgs, group=None):
        """ref: the frozen reference's store, or None with args.beta == 0 (REF trl/trl/trainer/grpo_trainer.py:407): the step then has no KL term, runs no reference
        pass of any kind (also when a store is given) and takes the sequential structure -- see _shadow_cus."""
        if args.logps_at_temperature and not (math.isfinite(args.temperature) and args.temperature > 0):
            raise ValueError(f"GRPOArgs.logps_at_temperature needs a finite temperature > 0 to score at (got temperature = {args.temperature})")
        if args.top_k <= 0 and args.top_p != 1.0:
            raise ValueError(f"GRPOArgs.top_k <= 0 samples the whole vocabulary and needs top_p == 1.0 (got top_p = {args.top_p}): a nucleus over all tokens is not built")
        if args.rollout_is_cap != 0 and not (math.isfinite(args.rollout_is_cap) and args.rollout_is_cap >= 1.0):
            raise ValueError(f"GRPOArgs.rollout_is_cap must be 0 (off) or a finite value >= 1 (got {args.rollout_is_cap}): a cap below 1 would down-weight on-policy tokens")
        if args.rollout_is_level not in ops.IS_LEVELS:
            raise ValueError(f"GRPOArgs.rollout_is_level must be one of {sorted(ops.IS_LEVELS)} (got {args.rollout_is_level!r})")
        if args.rollout_is_cap > 0 and cfg.is_llava and args.llava_rotate_right_padded_rows:
            raise ValueError("GRPOArgs.rollout_is_cap with llava_rotate_right_padded_rows: that path scores a rotated window, whose columns do not line up with the "
                             "rollout's log-probs; set llava_rotate_right_padded_rows=False to weight the completion tokens themselves")
        check_sampler_args("GRPOArgs", args.min_p, args.repetition_penalty)
        check_entropy_args("GRPOArgs", args.top_entropy_quantile, llava_rotated=bool(getattr(cfg, "is_llava", False)) and args.llava_rotate_right_padded_rows)
        if args.guide is not None and args.suppress_eos:
            raise ValueError("GRPOArgs.guide with suppress_eos: the guide's automaton decides where EOS may appear; drop one of the two")
        check_reuse_args("GRPOArgs", args.num_iterations, args.epsilon, args.epsilon_high)
        check_objective_args("GRPOArgs", args.loss_type, args.mask_truncated_completions, args.suppress_eos)
        check_sync_ref_args("GRPOArgs", args.sync_ref_model, args.ref_model_mixup_alpha, args.ref_model_sync_steps, args.beta)
        if ref is None and args.beta != 0:
            raise ValueError(f"GRPOArgs.beta = {args.beta} needs the frozen reference's ParamStore (ref=None is legal only with beta == 0: the KL term reads its log-probs)")
        self.cfg, self.args = cfg, args
        if args.beta == 0:
            self._shadow_cus(0)         # a forced IADR1_OVERLAP_CUS is refused here already, not at the first rollout
        self.last_rollout_logps = None      # [N, C] device tensor of the last rollout when args.wants_rollout_logps
        self.last_rollout_entropy = None    # [N, C] device tensor of the last rollout when args.wants_rollout_entropy
        self.pol, self.ref = Engine(policy), (Engine(ref) if ref is not None else None)
        for e in (self.pol, self.ref):      # policy, reference and (through the policy) the cached old_logps score at the same temperature
            if e is not None:
                e.logp_temperature = args.logp_temperature
        self.dev = policy.device
        self.reducer = GradReducer(policy, group)
        self.pol.resident_extra = (ref.resident_bytes() if ref is not None else 0) + self.reducer.staging_bytes()       # static inputs of Engine.recompute_wanted("auto")
        self.opt_step = 0
        self.accum = 0
        self._rollout = None
        self.shadow_logps, self.shadow_policy_head, self.last_step_shadowed = None, None, False
        self._shadow = None         # overlap.ChunkedRefPass: the frozen reference's pass over the sampled tokens runs under the rollout (step())
        self.norm2 = torch.zeros(1, dtype=F32, device=self.dev)
        self.norm_scratch = torch.zeros(2048, dtype=F32, device=self.dev)
        self.ref_syncs = 0          # sync_ref_model: how often the reference has been mixed so far (checkpointed as trainer_state.json's ref_syncs)
        self._ref_sync = None       # the last sync's record for the step's deferred metrics: (opt_step, pinned [2] host copy of dist2, event behind the copy, ref_syncs)
        if args.sync_ref_model:
            self.ref_dist2 = torch.zeros(2, dtype=F32, device=self.dev)
            self._ref_dist2_host = torch.zeros(2, dtype=F32).pin_memory() if self.dev.type == "cuda" else torch.zeros(2, dtype=F32)

    # ---- vision: once per unique image ---------------------------------------------------------------------
    def _vision(self, batch, want_policy_ctx: bool):
        return self.pol.vision_inputs(batch)

    def _per_row_images(self, batch, grids, rows):
        ipp = batch.get("images_per_prompt") or [1] * len(batch["input_ids"])
        gpr, off, k = [], [], 0
        for n in ipp:
            gpr.append(grids[k: k + n])
            off.append([int(rows[j]) for j in range(k, k + n)])
            k += n
        return gpr, off

    # ---- rollout -------------------------------------------------------------------------------------------------
    def vision_policy(self, batch, save: bool):
        """Policy vision tower once per step: its output feeds both the rollout prefill and the training forward."""
        grids, plan_v, px, rows = self._vision(batch, save)
        img, vctx = self.pol.vision_forward(px, plan_v, save=save)
        return {"grids": grids, "plan": plan_v, "px": px, "rows": rows, "img": img, "ctx": vctx}

    def rollout(self, batch, vis=None, greedy=False, train_carry=None, shadow_ref: bool = False) -> np.ndarray:
        """Completion ids [Bp*G, <=C] (numpy, right-padded with pad after EOS like REF:680-683).
        shadow_ref: also run the frozen reference's teacher-forced pass over the tokens as they are produced, on a second stream under the decode replays
        (overlap.ChunkedRefPass); afterwards self.shadow_logps is the [N, C] reference log-prob tensor (None when the pass does not apply) and the consumer
        must `self._shadow.join()` before reading it."""
        a = self.args
        ids, mask = np.asarray(batch["input_ids"]), np.asarray(batch["attention_mask"])
        if a.max_prompt_length is not None:
            ids, mask = ids[:, -a.max_prompt_length:], mask[:, -a.max_prompt_length:]
        vis = vis or self.vision_policy(batch, save=False)
        grids, rows, img_pol = vis["grids"], vis["rows"], vis["img"]
        gpr, off = self._per_row_images(batch, grids, rows)
        plan = self.pol.text_plan(ids, mask, gpr, off)
        Bp = ids.shape[0]
        N = Bp * a.num_generations
        # the KV pool, the block table and the captured graph are sized for a prompt length: a longer padded prompt than any seen so far rebuilds them (grow only;
        # prompt lengths vary from batch to batch with the image sizes of the any-resolution families)
        if self._rollout is None or self._rollout.N != N or self._rollout.max_new < a.max_completion_length or self._rollout.max_prompt < ids.shape[1]:
            grow = max(ids.shape[1], self._rollout.max_prompt if self._rollout is not None else 0)
            self._rollout = None        # release the old pool before the new one is allocated
            split = self._cu_split(N)      # (the launcher configuration that goes with it is set by Rollout.generate for the duration of each call)
            self._rollout = Rollout(self.pol, N, grow, a.max_completion_length, max_prompts=Bp, use_graph=a.use_hip_graph, **split)
        c, st = self.cfg, self.pol.p
        # decode steps that also fill the training arena (no policy forward over the completions afterwards): needs the fused decode kernels that carry
        # the side outputs (q|k|v + rotary + cache append, persistent fused-SwiGLU gate|up GEMM)
        # (not with the opt-in FP8 weight stream: the policy's training activations must come from its bf16 weights, so its forward runs after the rollout)
        trace = (train_carry is not None and a.reuse_decode and st.qkv_rope_packed and not st.decode_fp8 and self._rollout_fuses_swiglu(N))
        shadow = None
        self.shadow_logps, self.shadow_policy_head = None, None
        if shadow_ref and self.dev.type == "cuda" and ChunkedRefPass.applicable(c, N, a.max_completion_length) and (self._rollout.decode_stream is not None or ChunkedRefPass.unmasked()):
            if self._shadow is None or self._shadow.stream is not (self.__dict__.get("_shadow_stream") or self._shadow.stream):
                self._shadow = ChunkedRefPass(self.ref, stream=self.__dict__.get("_shadow_stream"))
            shadow = self._shadow
            shadow.vision = (vis["px"], vis["plan"])
        if os.environ.get("IADR1_QUIET") != "1" and self.__dict__.get("_path_logged") != (shadow is not None):
            self._path_logged = shadow is not None      # once per change: WHICH step structure runs (the two differ in the last bf16 bit of the policy's mlp rows)
            if shadow is not None:
                rb = trace and shadow.rebuilds_policy_mlp(c, N)
                print(f"[iadr1] co-scheduled step: the frozen reference's pass{', the policy mlp rows (REBUILT by the training GEMM)' if rb else ''} and the lm_head log-probs run on "
                      f"{torch.cuda.get_device_properties(self.dev).multi_processor_count - self._rollout.decode_cus if self._rollout.decode_cus else 'all'} CUs under the rollout (IADR1_OVERLAP_CUS=0: sequential step; IADR1_OVERLAP_GU=0: rows stored by the decode step)",
                      file=sys.stderr, flush=True)
            elif shadow_ref:
                print("[iadr1] sequential step: the frozen reference's pass runs after the rollout, on the whole device", file=sys.stderr, flush=True)
        toks = self._rollout.generate(plan, img_pol, a.num_generations, a.max_completion_length, temperature=0.0 if greedy else a.temperature,
                                      top_k=a.top_k, top_p=a.top_p, seed=a.seed + 1000003 * self.opt_step + 7919 * self.accum, suppress_eos=a.suppress_eos,
                                      train_carry=train_carry, train_trace=trace, shadow=shadow, return_logps=a.wants_rollout_logps,
                                      min_p=0.0 if greedy else (a.min_p or 0.0), repetition_penalty=a.repetition_penalty, **({"guide": a.guide} if a.guide is not None else {}),
                                      **({"return_entropy": True} if a.wants_rollout_entropy else {}),
                                      **({"logp_temperature": a.logp_temperature} if a.logp_temperature != 1.0 else {}))
        self.last_rollout_logps, self.last_rollout_entropy = None, None
        if a.wants_rollout_entropy:     # (the rollout's tuple ends in the entropies)
            *toks, self.last_rollout_entropy = toks
            toks = tuple(toks) if a.wants_rollout_logps else toks[0]
        if a.wants_rollout_logps:
            toks, self.last_rollout_logps = toks
        if shadow is not None:
            self.shadow_logps = shadow.logp
            self.shadow_policy_head = (shadow.pol_logp, shadow.pol_lse) if shadow.pol_logp is not None else None
        if trace:
            train_carry["traced"] = True
        return self._rollout.tokens_host()      # (the host copy left before the side pass's tail was enqueued: 1230.0 -> 1223.4 ms, EXPERIMENTS round 5)

    def _cu_split(self, N: int) -> dict:
        """Co-scheduling with a CU split (IADR1_OVERLAP_CUS = auto for this shape, or n > 0): the shadow pass is confined to n CUs and the decode replays to the
        others -- two CU-masked streams (include/iadr1_hip.h iadr1_stream_create_cu_mask) on different dispatch pipes (overlap.cu_split, one pair per process); the
        decode launchers size their persistent grids for the smaller device (iadr1_set_decode_cus).  Masked streams are BLOCKING streams: `step` moves off the null
        stream while they are in use."""
        from .overlap import cu_split
        n = self._shadow_cus(N)
        self._shadow_stream = None
        if n <= 0 or self.dev.type != "cuda" or not ChunkedRefPass.applicable(self.cfg, N, self.args.max_completion_length):
            return {}
        sp = cu_split(self.dev, n, self.ref.p.w("layers.0.gu.w"))
        # one decision for the whole data-parallel job, taken once (the first rollout of a run, the same call on every rank: N and the completion length are the
        # launch configuration's, identical across ranks): a rank without a clean stream pair switches co-scheduling off for all of them
        agreed = self.__dict__.setdefault("_co_sched_agreed", {})
        if n not in agreed:
            from .overlap import agree_across_ranks
            agreed[n] = agree_across_ranks(sp is not None, self.reducer.group, self.dev)
            if sp is not None and not agreed[n] and os.environ.get("IADR1_QUIET") != "1":
                print("[iadr1] co-scheduling off on this rank too: another rank of the process group found no clean stream pair", file=sys.stderr, flush=True)
        if sp is None or not agreed[n]:       # no candidate on another dispatch pipe (here or on some rank): no co-scheduling at all (the one-shot reference pass after the rollout)
            if sp is None and os.environ.get("IADR1_OVERLAP_CUS", "auto").strip().lower() not in ("", "auto") and os.environ.get("IADR1_OVERLAP_STRICT", "1") != "0":
                # a FORCED split that cannot be had is an error, not a silent change of the step's structure (the rebuilt policy rows differ from the stored ones in the
                # last bf16 bit: ADVICE r5 -- a run that asked for one path must not get the other)
                raise RuntimeError(f"IADR1_OVERLAP_CUS={n}: no stream pair on separate dispatch pipes was found; unset it (auto: sequential fallback) or set IADR1_OVERLAP_STRICT=0")
            return {}
        self._shadow_stream = sp[1]
        return {"decode_cus": sp[2], "decode_stream": sp[0]}

    def _shadow_cus(self, N: int) -> int:
        """overlap.shadow_cus for this engine.  With beta == 0 there is no reference pass to put under the rollout, so the step is the sequential one and the decode
        grids keep the whole device: `auto` resolves to 0, and a forced split is refused (a run that asked for one step structure must not silently get the other)."""
        from .overlap import shadow_cus
        if self.args.beta != 0:
            return shadow_cus(self.cfg, N, self.args.max_completion_length)
        v = os.environ.get("IADR1_OVERLAP_CUS", "auto").strip().lower()
        if v not in ("", "auto", "0"):      # every forced side stream, -1 (the ordinary second stream) included, and anything that is not a number
            raise ValueError(f"IADR1_OVERLAP_CUS={v} with GRPOArgs.beta == 0: the co-scheduled step puts the frozen reference's pass under the rollout (n > 0: on a CU share, "
                             "-1: on an ordinary second stream), and a step without a KL term runs no reference pass; unset it (auto: the sequential step, decode on the whole "
                             "device) or set it to 0")
        return 0

    def _rollout_fuses_swiglu(self, N) -> bool:
        """True when the decode gate|up projection runs on the persistent fused-SwiGLU kernel (the one with side outputs): include/iadr1_hip.h."""
        c = self.cfg
        ncu = torch.cuda.get_device_properties(self.dev).multi_processor_count
        K, N2 = c.hidden_size, 2 * c.intermediate_size
        return (self._rollout.fuse_swiglu and K % 256 == 0 and K // 256 in (4, 6, 8)
                and N2 % 128 == 0 and N2 // 32 >= 2 * ncu and N <= 256)

    # ---- loss + gradients for given completions ------------------------------------------------------------------
    def loss_and_grads(self, batch, completions, rewards_per_func, backward: bool = True, last_micro_step: bool = True, vis=None, train_carry=None, defer_metrics: bool = False,
                       ref_logps=None, policy_head=None, rollout_logps=None, old_logps=None, is_weights=None, rollout_entropy=None, entropy_mask=None):
        """completions: list of Bp*G id lists (prompt-major) or an [N,C] array already padded;
        rewards_per_func: [N, n_funcs] float tensor/array.  Accumulates gradients into policy.grad.
        ref_logps: [N, C] reference log-probs already computed for exactly these completions by the rollout's shadow pass (rollout(shadow_ref=True)): the
        reference forward is then not run here; the shadow stream is joined right before the loss kernel reads them.
        rollout_logps: [N, >= C] log-probs the rollout's sampler returned for exactly these completions (rollout with args.rollout_logps): compared with the policy
        log-probs computed here over the completion mask (metrics rollout/*, result "rollout_logps").  The loss reads them only with args.rollout_is_cap > 0: every
        per-token term is then weighted by min(exp(scored - sampled), cap) (iadr1_grpo_loss_is; result "rollout_is_weights", metrics rollout/is_weight_mean and
        rollout/is_clipped_frac), and completions without their rollout log-probs are refused.
        old_logps: [N, C] policy log-probs an earlier call returned as "logps" for exactly these completions (a reuse iteration of GRPOArgs.num_iterations > 1): the
        loss is then the clipped surrogate against them (iadr1_grpo_loss_clip with args.epsilon / epsilon_high), the rollout/* metrics are not produced, and the
        metrics gain clip_ratio/low_mean, clip_ratio/high_mean, clip_ratio/region_mean (shares of this call's live tokens), policy/ratio_mean and
        policy/logp_abs_diff_max; result "old_logps".  With args.rollout_is_cap > 0 it needs is_weights, the "rollout_is_weights" of that earlier call: the weight of
        the sampling engine against the policy that sampled does not change while its rollout is reused.
        args.beta == 0: no reference pass runs and ref_logps is not read; results "ref_logps" and "kl" are None and the metrics have no "kl".  args.loss_type other
        than "grpo" changes the row normaliser (loss_row_scale); args.mask_truncated_completions zeroes the loss-mask rows without an EOS (result "completion_mask",
        metric completions/clipped_ratio).  Whatever the options, the loss is one iadr1_grpo_loss_ex call per micro-batch (iadr1_grpo_loss_sel with a selector).
        rollout_entropy: [N, >= C] entropies the rollout's sampler returned for exactly these completions (rollout with args.wants_rollout_entropy): metric
        `entropy`, their mean over the EOS mask, and result "rollout_entropy".  With args.top_entropy_quantile < 1 they also select, once per call and from all N
        rows of the loss mask (entropy_keep_mask, over all ranks), the tokens whose advantage term is trained (iadr1_grpo_loss_sel): metrics entropy/threshold and
        entropy/kept_frac, result "entropy_mask" ([N, C] bool); completions without their entropies are then refused.
        entropy_mask: a reuse iteration (old_logps=...) with args.top_entropy_quantile < 1 applies the "entropy_mask" of the call that sampled instead, and logs
        none of the entropy metrics again."""
        a, c = self.args, self.cfg
        use_clip = old_logps is not None
        use_is = a.rollout_is_cap > 0 and not use_clip
        use_sel = a.top_entropy_quantile < 1.0
        G = a.num_generations
        ids_p, mask_p = np.asarray(batch["input_ids"]), np.asarray(batch["attention_mask"])
        if a.max_prompt_length is not None:
            ids_p, mask_p = ids_p[:, -a.max_prompt_length:], mask_p[:, -a.max_prompt_length:]
        Bp, P = ids_p.shape
        N = Bp * G
        comp = completions if isinstance(completions, np.ndarray) else right_pad(completions, c.pad_token_id)
        assert comp.shape[0] == N
        C = comp.shape[1]
        if use_is and (rollout_logps is None or rollout_logps.shape[0] != N or rollout_logps.shape[1] < C):
            raise ValueError(f"GRPOArgs.rollout_is_cap > 0 needs the rollout log-probs of these [{N}, {C}] completions (rollout_logps=...): "
                             f"got {None if rollout_logps is None else tuple(rollout_logps.shape)}")
        if use_clip:
            if tuple(old_logps.shape) != (N, C):
                raise ValueError(f"old_logps must be the [{N}, {C}] log-probs scored for these completions, got {tuple(old_logps.shape)}")
            w_clip = None
            if a.rollout_is_cap > 0:
                if is_weights is None or tuple(is_weights.shape) != (N, C):
                    raise ValueError(f"GRPOArgs.rollout_is_cap > 0: a reuse iteration (old_logps=...) needs is_weights, the [{N}, {C}] rollout_is_weights of the step that "
                                     f"sampled these completions: got {None if is_weights is None else tuple(is_weights.shape)}")
                w_clip = is_weights.to(F32)
        if use_sel and use_clip and (entropy_mask is None or tuple(entropy_mask.shape) != (N, C)):
            raise ValueError(f"GRPOArgs.top_entropy_quantile < 1: a reuse iteration (old_logps=...) needs entropy_mask, the [{N}, {C}] entropy_mask of the step that "
                             f"sampled these completions: got {None if entropy_mask is None else tuple(entropy_mask.shape)}")
        if use_sel and not use_clip and (rollout_entropy is None or rollout_entropy.shape[0] != N or rollout_entropy.shape[1] < C):
            raise ValueError(f"GRPOArgs.top_entropy_quantile < 1 needs the rollout entropies of these [{N}, {C}] completions (rollout_entropy=...): "
                             f"got {None if rollout_entropy is None else tuple(rollout_entropy.shape)}")
        cmask = eos_completion_mask(comp, c.eos_token_id)
        # the loss mask: what the loss kernel, the row_scale and clip / IS metric denominators and the returned "completion_mask" see.  The text plans, the llava
        # rotation and completion_length keep the EOS mask (trl also zeroes the attention mask of a dropped row; the live rows do not attend to it either way)
        lmask = truncation_loss_mask(cmask, comp, c.eos_token_id) if a.mask_truncated_completions else cmask
        no_ref = a.beta == 0            # no KL term: no reference pass, nothing read through a reference pointer
        # one value per call, from all N rows of the host-resident mask (not per micro-batch: results keep not depending on micro_batch_seqs)
        row_scale = loss_row_scale(a.loss_type, lmask, a.max_completion_length)
        ids = np.concatenate([np.repeat(ids_p, G, 0), comp], 1)
        mask = np.concatenate([np.repeat(mask_p, G, 0), cmask.astype(mask_p.dtype)], 1)
        S = P + C
        cmask_d = ops.h2d(lmask, self.dev)
        ent_all = rollout_entropy[:, :C].to(F32) if (rollout_entropy is not None and not use_clip) else None
        keep, tau, sel_d = None, None, None
        if use_sel:
            # one mask per call, from all N rows (not per micro-batch: results keep not depending on micro_batch_seqs) and the live tokens of all ranks
            red = self.reducer      # (a job without an explicit group reduces over the default one)
            grp = None if red.world <= 1 else (red.group if red.group is not None else red.dist.group.WORLD)
            keep, tau = (entropy_mask.to(self.dev).bool(), None) if use_clip else entropy_keep_mask(ent_all, lmask.astype(bool), a.top_entropy_quantile, group=grp)
            sel_d = keep.to(torch.int32).contiguous()
        state = {}

        def advantages():
            """Rewards may be handed over as a callable: it is evaluated here, after the reference and policy forwards of the first
            micro-batch have been enqueued, so the host-side reward functions (regex, ~9 ms for 64 samples) run while the GPU works."""
            if not state:
                rpf = rewards_per_func() if callable(rewards_per_func) else rewards_per_func
                rpf = torch.as_tensor(np.asarray(rpf), dtype=F32)
                adv, std = group_advantages(rpf.sum(1), G, a.scale_rewards)
                # pinned + non-blocking: a pageable host-to-device copy synchronises the stream, i.e. would make the host wait here for the reference and policy
                # forwards it has just enqueued (and leave the GPU idle for the ~1 ms the host then needs to launch the loss kernel)
                state.update(rpf=rpf, rewards=rpf.sum(1), adv=adv, std=std, adv_d=ops.h2d(adv, self.dev))
            return state

        if vis is None or (backward and vis["ctx"] is None):
            vis = self.vision_policy(batch, save=backward)
        grids, plan_v, px, rows, img_pol, vctx = vis["grids"], vis["plan"], vis["px"], vis["rows"], vis["img"], vis["ctx"]
        have_ref = not no_ref and ref_logps is not None and tuple(ref_logps.shape) == (N, C)
        shadowed = have_ref and ref_logps is self.shadow_logps      # this step's rollout ran the shadow pass that wrote them (else: handed in by the caller, nothing to join)
        img_ref = None if (have_ref or no_ref) else self.ref.vision_forward(px, plan_v, save=False)[0]
        gpr, off = self._per_row_images(batch, grids, rows)
        dimg32 = torch.zeros(img_pol.shape, dtype=F32, device=self.dev) if backward else None

        logp_all = torch.empty(N, C, dtype=F32, device=self.dev)
        ref_all = None if no_ref else torch.empty(N, C, dtype=F32, device=self.dev)
        kl_all = None if no_ref else torch.empty(N, C, dtype=F32, device=self.dev)
        row_loss = torch.empty(N, dtype=F32, device=self.dev)
        row_kl = torch.empty(N, dtype=F32, device=self.dev)
        if use_is:
            ro_all = rollout_logps[:, :C].to(F32)
            w_all = torch.empty(N, C, dtype=F32, device=self.dev)
            is_stats = torch.empty(N, 5, dtype=F32, device=self.dev)
        if use_clip:
            old_all = old_logps.to(F32)
            eps_high = a.epsilon if a.epsilon_high is None else a.epsilon_high
            clip_stats = torch.empty(N, 4, dtype=F32, device=self.dev)
        mb = max(1, min(a.micro_batch_seqs, N))
        # shared-prefix layout (vlm.Engine.text_plan_shared): every prompt runs through the layers once per group instead of
        # G times -- needs micro-batches made of whole groups.  IADR1_SHARE_PREFIX=0 keeps the reference's [n, P+C] rows.
        share = a.share_prefix and G > 1 and mb % G == 0
        starts = list(range(0, N, mb))
        col = np.arange(C)
        for si, r0 in enumerate(starts):
            r1 = min(N, r0 + mb)
            n = r1 - r0
            if share:
                b0, b1 = r0 // G, r1 // G
                plan = self.pol.text_plan_shared(ids_p[b0:b1], mask_p[b0:b1], comp[r0:r1], cmask[r0:r1], G, gpr[b0:b1], off[b0:b1])
                sel = self.pol.shared_logit_rows(b1 - b0, P, n, C, G)[0]
            else:
                rows_b = [r // G for r in range(r0, r1)]
                plan = self.pol.text_plan(ids[r0:r1], mask[r0:r1], [gpr[b] for b in rows_b], [off[b] for b in rows_b])
                sel = (np.arange(n)[:, None] * S + (P - 1) + col[None, :]).reshape(-1)        # logits rows P-1 .. S-2
            tgt = ids[r0:r1, P:].astype(np.int64).copy()
            if c.is_llava and a.llava_rotate_right_padded_rows:
                sel = sel.reshape(n, C).copy()
                for r in range(r0, r1):
                    pl = right_padding_shift(ids[r], c.pad_token_id)
                    if pl == 0:
                        continue                       # no right padding / left padding present: the reference leaves the row alone
                    ln = int(cmask[r].sum())           # the loss mask stays the un-rotated completion mask (REF:722-728)
                    if P - pl - 1 < 0:
                        # the window would start inside the rotated row's padding: the reference then scores pad tokens predicted from masked positions
                        # (its values depend on how the attention backend treats fully masked queries) -- not a defined target
                        raise ValueError(f"llava left-padding fix-up: row {r} ends in {pl} pad columns but its prompt has only {P} positions; "
                                         "the reference's rotated window would read masked positions (prompt shorter than the padding of an early-ended completion)")
                    # the row is shifted right by pl columns: window column t holds original token P - pl + t
                    for t_ in range(ln):
                        qi = P - pl + t_               # predicted token (original column), read from the hidden state of column qi - 1
                        hi = qi - 1
                        if share:
                            sel[r - r0, t_] = (r // G - b0) * P + hi if hi < P else (b1 - b0) * P + (r - r0) * C + (hi - P)
                        else:
                            sel[r - r0, t_] = (r - r0) * S + hi
                        tgt[r - r0, t_] = ids[r, qi]
                sel = sel.reshape(-1)
            rows_d = ops.h2d(sel.astype(np.int64), self.dev)
            tgt_d = ops.h2d(tgt.reshape(-1), self.dev)
            rl = None
            if not have_ref and not no_ref:
                hf, _ = self.ref.text_forward(plan, img_ref, save=False)
                rl, _ = self.ref.logprobs(hf, rows_d, tgt_d, save=False)
                del hf
            if train_carry is not None and "x0" in train_carry and share and backward and n == N and C == a.max_completion_length and vis is not None and vis["ctx"] is not None:
                # the rollout's prefill already ran (and saved) the prompt rows of this batch: only the completion rows go through the layers
                T_all = plan.ids.numel()
                train_carry["full_plan"] = plan
                if train_carry.get("traced"):      # ... and its decode steps wrote the completion rows: nothing to run at all
                    hf, ctx = self.pol.text_context_from_trace(plan.tail, ((b1 - b0) * P, T_all, T_all), train_carry)
                else:
                    hf, ctx = self.pol.text_forward(plan.tail, None, save=True, rows=((b1 - b0) * P, T_all, T_all), carry=train_carry)
            else:
                hf, ctx = self.pol.text_forward(plan, img_pol, save=backward, recompute=backward and self.pol.recompute_wanted(plan.ids.numel(), a.recompute))
            pre = None
            if have_ref and policy_head is not None and share and n == N and train_carry is not None and train_carry.get("traced") and not (c.is_llava and a.llava_rotate_right_padded_rows):
                pre = (policy_head[0].reshape(-1), policy_head[1].reshape(-1))       # the shadow pass scored the policy's rows too (same rows, same targets, same launch)
            lp, lctx = self.pol.logprobs(hf, rows_d, tgt_d, save=backward, rows_host=sel, precomputed=pre)
            if pre is not None and si == 0:
                self._shadow.join()
            adv_d = advantages()["adv_d"]
            if have_ref:
                if si == 0 and shadowed:
                    self._shadow.join()          # the tail chunk of the shadow pass ran next to the policy's lm_head; everything after this reads its log-probs
                rl = ref_logps[r0:r1].contiguous()
            # one call whatever the options: the form follows from old_logp / rollout_logp, and with a reference, row_scale 0 ("grpo") and no sel it is the
            # form's own entry point, argument for argument
            form = {}
            if use_clip:
                form = dict(old_logp=old_all[r0:r1].contiguous(), w=None if w_clip is None else w_clip[r0:r1].contiguous(), eps_low=a.epsilon, eps_high=eps_high)
            elif use_is:
                form = dict(rollout_logp=ro_all[r0:r1].contiguous(), cap=a.rollout_is_cap, level=a.rollout_is_level)
            res = ops.grpo_loss_ex(lp.view(n, C), adv_d[r0:r1].contiguous(), cmask_d[r0:r1].contiguous(), a.beta, ref_logp=None if no_ref else rl.view(n, C),
                                   row_scale=row_scale, n_total_rows=N, sel=None if sel_d is None else sel_d[r0:r1].contiguous(), **form)
            dlogp, kl, rloss, rkl = res[:4]
            if use_clip:
                clip_stats[r0:r1] = res[4]
            elif use_is:
                w_all[r0:r1], is_stats[r0:r1] = res[4], res[5]
            logp_all[r0:r1] = lp.view(n, C)
            if not no_ref:
                ref_all[r0:r1], kl_all[r0:r1] = rl.view(n, C), kl
            row_loss[r0:r1], row_kl[r0:r1] = rloss, rkl
            if backward:
                dhf = self.pol.logprobs_backward(dlogp.view(-1), lctx)
                del hf, lctx
                hook = self.reducer.layer_ready if (last_micro_step and si == len(starts) - 1) else None
                self.pol.text_backward(dhf, ctx, dimg32, layer_done=hook)
                del ctx, dhf
        if backward:
            dimg = ops.f32_bias_to_bf16(dimg32, None)
            self.pol.vision_backward(dimg, vctx)
            self.accum += 1
        st = advantages()
        metrics = {"completion_length": float(cmask.sum(1).mean()), "reward": float(st["rewards"].mean()), "reward_std": float(st["std"].mean())}
        if a.mask_truncated_completions:
            metrics["completions/clipped_ratio"] = 1.0 - float((comp == c.eos_token_id).any(1).mean())        # REF trl/trl/trainer/grpo_trainer.py:1103-1106
        means = [row_loss.mean(), row_kl.mean()]
        ro_lp = None
        if use_clip:
            # clipped shares, mean ratio and largest |logp - old_logp| over this call's live tokens, from the loss kernel's per-row partials
            cnt = float(max(1, int(lmask.sum())))
            sums = clip_stats.sum(0) / cnt
            means += [sums[0], sums[1], sums[2], clip_stats[:, 3].max()]
        elif use_is:
            # the same three rollout/* means from the loss kernel's per-row partials (columns: include/iadr1_hip.h), plus the mean weight and the clipped share
            ro_lp = ro_all
            cnt = float(max(1, int(lmask.sum())))
            sums = is_stats.sum(0) / cnt
            means += [sums[2], is_stats[:, 3].max(), sums[4], sums[0], sums[1]]
        elif rollout_logps is not None and not use_clip:
            # sampled (the rollout's logits) vs scored (the policy forward of the loss) log-probs of the same tokens, over the completion mask; k3 estimator of
            # KL(sampled || scored) in the form iadr1_grpo_loss uses for policy vs reference: exp(d) - d - 1 with d = scored - sampled
            ro_lp = rollout_logps[:, :C].to(F32)
            m_ = (cmask_d if lmask is cmask else ops.h2d(cmask, self.dev)).to(F32)      # a diagnostic of the rollout, not of the loss: the EOS mask
            d_ = (logp_all - ro_lp) * m_
            cnt = m_.sum().clamp(min=1.0)
            means += [d_.abs().sum() / cnt, d_.abs().max(), ((torch.exp(d_) - d_ - 1.0) * m_).sum() / cnt]
        ent_at = None
        if ent_all is not None:
            # the rollout's entropies over the live completion tokens (a diagnostic of the rollout: the EOS mask), and what the quantile kept of the loss mask
            ent_at = len(means)
            m_ = (cmask_d if lmask is cmask else ops.h2d(cmask, self.dev)).to(F32)
            means.append((ent_all * m_).sum() / m_.sum().clamp(min=1.0))
            if tau is not None:
                means += [tau.to(F32), keep.sum().to(F32) / float(max(1, int(lmask.sum())))]
        dev_means = torch.stack(means)       # one device -> host read for all of them
        closes_step = self.opt_step + 1      # the optimizer step this call's gradients go into; with deferred metrics it has run by the time they are read

        def finalize():
            lk = dev_means.tolist()
            metrics.update(loss=lk[0])
            if a.sync_ref_model and last_micro_step:
                metrics.update(self.ref_sync_metrics(closes_step))
            if not no_ref:          # as in trl (REF trl/trl/trainer/grpo_trainer.py:1224): no kl key without a KL term
                metrics.update(kl=lk[1])
            if use_clip:
                metrics.update({"clip_ratio/low_mean": lk[2], "clip_ratio/high_mean": lk[3], "clip_ratio/region_mean": lk[2] + lk[3], "policy/ratio_mean": lk[4],
                                "policy/logp_abs_diff_max": lk[5]})
            if ro_lp is not None:
                metrics.update({"rollout/logp_abs_diff_mean": lk[2], "rollout/logp_abs_diff_max": lk[3], "rollout/kl": lk[4]})
            if use_is:
                metrics.update({"rollout/is_weight_mean": lk[5], "rollout/is_clipped_frac": lk[6]})
            if ent_at is not None:
                metrics.update(entropy=lk[ent_at])
                if tau is not None:
                    metrics.update({"entropy/threshold": lk[ent_at + 1], "entropy/kept_frac": lk[ent_at + 2]})
            return metrics
        if defer_metrics:      # the caller enqueues more work (the optimizer) before it reads the two device-side means: no idle GPU while the host comes back from the sync
            metrics["finalize"] = finalize
        else:
            finalize()
        out = {"metrics": metrics, "logps": logp_all, "ref_logps": ref_all, "kl": kl_all, "advantages": st["adv"], "completion_mask": lmask,
               "rewards_per_func": st["rpf"], "ids": ids, "mask": mask}
        if ro_lp is not None:
            out["rollout_logps"] = ro_lp
        if use_is:
            out["rollout_is_weights"] = w_all
        if use_clip:
            out["old_logps"] = old_all
        if ent_all is not None:
            out["rollout_entropy"] = ent_all
        if keep is not None:
            out["entropy_mask"] = keep
        return out

    # ---- optimizer -------------------------------------------------------------------------------------------------
    def optimizer_step(self):
        a, st = self.args, self.pol.p
        if self._shadow is not None:
            self._shadow.check_timed_out()      # a co-scheduled pass that ran on unfinished rows must not reach the weights
        self.reducer.finish()
        self.opt_step += 1
        scale = 1.0 / (self.reducer.world * max(1, self.accum))
        hip.call("sumsq", st.grad, st.n_total, self.norm_scratch, self.norm2)
        self.grad_scale = scale          # grad_norm() = sqrt(norm2) * scale: the norm of the averaged gradient, before clipping (HF's `grad_norm` log key)
        for lo, hi, wd in ((0, st.n_decay, a.weight_decay), (st.n_decay, st.n_total, 0.0)):
            if hi > lo:
                hip.call("adamw_flat", st.master[lo:hi], st.m[lo:hi], st.v[lo:hi], st.grad[lo:hi], st.flat[lo:hi], hi - lo, a.learning_rate,
                         a.adam_beta1, a.adam_beta2, a.adam_epsilon, wd, self.opt_step, scale, self.norm2, a.max_grad_norm)
        st.refresh_shadows()
        if a.sync_ref_model and ref_sync_due(self.opt_step, a.ref_model_sync_steps):
            self._sync_ref()
        self.accum = 0
        if self.pol.check_ddp_headroom(a.recompute, group=self.reducer.group):
            # the rollout's captured graph and its training-arena views keep the freed arena's blocks alive: drop them too, THEN hand the memory back to the device
            self._rollout = None
            torch.cuda.empty_cache()

    def _sync_ref(self):
        """reference <- alpha * policy + (1 - alpha) * reference (GRPOArgs.sync_ref_model), enqueued on the optimizer's stream right behind the AdamW launches.
        Ordering, with no event of its own and no device synchronisation:
          * behind the AdamW write of pol.flat: the same stream, later in program order;
          * behind every read of the reference by the step that just ended: the sequential pass ran on this stream; the co-scheduled pass's side stream was joined
            into it by ChunkedRefPass.finish (`cur.wait_stream(side)`, and the tail ran on `cur`), and step() orders the caller's stream behind `_main_stream`;
          * ahead of every read by the next step: the sequential pass and the prefill run on this stream (or on `_main_stream`, which step() makes wait for it);
            the side stream's first work of a rollout, ChunkedRefPass.prompt_phase, waits for the `gate` event Rollout.generate records on the step's stream behind
            the prefill, and every chunk (gated on the device step counter) is behind prompt_phase in the side stream's own order; the CU-masked decode stream does
            `wait_stream` on the step's stream before its first replay.  All of those sit behind the mix in the step's stream.
        Nothing derived from the reference's weights outlives a step: overlap.cu_split reads `ref.p.w("layers.0.gu.w")` once, as the B operand of a timing GEMM
        whose values do not matter; ChunkedRefPass keeps activations only (the q|k|v rows in `store`, `_img_ref`), rebuilt by every rollout's begin / prompt_phase;
        Engine caches index plans and buffers, never weights.  The reference log-probs a generation caches (num_iterations > 1) are kept on purpose, as in trl."""
        a = self.args
        self.ref.p.mix_from(self.pol.p, a.ref_model_mixup_alpha, self.ref_dist2)
        self.ref_syncs += 1
        self._ref_dist2_host.copy_(self.ref_dist2, non_blocking=True)      # read by the step's deferred metrics (loss_and_grads' finalize), behind their own read
        ev = None
        if self.dev.type == "cuda":
            ev = torch.cuda.Event()
            ev.record()
        self._ref_sync = (self.opt_step, self._ref_dist2_host, ev, self.ref_syncs)

    def ref_sync_metrics(self, opt_step: int) -> dict:
        """{"ref/policy_dist", "ref/syncs"} when the optimizer step numbered `opt_step` (1-based) mixed the reference, else {}.  Called where the step's other
        deferred metrics are read: their device -> host read has already drained the stream the copy of dist2 was enqueued on, so the event is complete."""
        rec = self._ref_sync
        if rec is None or rec[0] != opt_step:
            return {}
        _, host, ev, count = rec
        if ev is not None:
            ev.synchronize()
        d2, r2 = float(host[0]), float(host[1])
        return {"ref/policy_dist": math.sqrt(d2 / r2) if r2 > 0 else float("nan"), "ref/syncs": float(count)}

    def grad_norm(self) -> float:
        """Global L2 norm of the last optimizer step's (averaged, unclipped) gradient; synchronises the device."""
        return float(self.norm2.sqrt().item()) * getattr(self, "grad_scale", 1.0)

    # ---- the whole micro-step ----------------------------------------------------------------------------------------
    def step(self, *args, **kw):
        """`_step` on a stream of the engine's own when the caller is on the NULL stream and the CU split is in use: the two CU-masked streams are blocking
        streams (hipExtStreamCreateWithCUMask has no non-blocking form), i.e. every operation on the null stream waits for both of them and holds back what they
        enqueue afterwards -- measured: each chunk of the shadow pass then started exactly one chunk period late.  The caller's stream is ordered before and
        after the step as usual."""
        if self.dev.type == "cuda" and torch.cuda.current_stream(self.dev).cuda_stream == 0 and self._splits_cus(args[0] if args else kw.get("batch")):
            if "_main_stream" not in self.__dict__:
                self._main_stream = torch.cuda.Stream(self.dev)
            outer = torch.cuda.current_stream(self.dev)
            self._main_stream.wait_stream(outer)
            with torch.cuda.stream(self._main_stream):
                out = self._step(*args, **kw)
            outer.wait_stream(self._main_stream)
            return out
        return self._step(*args, **kw)

    def _splits_cus(self, batch) -> bool:
        try:
            n_seq = len(batch["input_ids"]) * self.args.num_generations
        except Exception:
            return False
        return self._shadow_cus(n_seq) > 0

    def _step(self, batch, reward_fn, do_optimizer_step=True, last_micro_step=None, return_outputs=False, defer_metrics=False, completions=None, rollout_logps=None,
              ref_logps=None, old_logps=None, is_weights=None, rollout_entropy=None, entropy_mask=None):
        """One SC-GRPO micro-step: vision tower -> group rollout -> rewards -> reference / policy passes + backward (-> optimizer).  This is the path
        `SCGRPOTrainer.compute_loss` (the reference's API, REF:586) runs and the one bench.py times.
        reward_fn(completion_ids: np.ndarray [N,C]) -> [N, n_funcs] rewards (decode + plugin functions live with the caller, which owns the tokenizer).
        last_micro_step (default: do_optimizer_step): the data-parallel gradient buckets leave from this call's backward.
        completions: [N, C] ids already rolled out for these prompts (SCGRPOTrainer.training_step rolls all micro-batches of an optimizer step out at once): no
        rollout here, the policy forward runs over the completions.
        rollout_logps: with `completions`, the log-probs their rollout returned for these rows (args.rollout_logps; SCGRPOTrainer.training_step's batched rollouts);
        required with args.rollout_is_cap > 0.
        old_logps (with `completions`): a reuse iteration of args.num_iterations > 1 -- the "logps" the step that rolled these completions out returned, with its
        "ref_logps" (no reference forward here) and, with args.rollout_is_cap > 0, its "rollout_is_weights" as is_weights in place of the rollout log-probs;
        loss_and_grads then takes the clipped surrogate.
        rollout_entropy: with `completions`, the entropies their rollout returned for these rows (args.rollout_entropy; the batched rollouts again); required with
        args.top_entropy_quantile < 1.  entropy_mask (with old_logps): the "entropy_mask" of the step that sampled, required there on a reuse iteration.
        return_outputs: the whole loss_and_grads dict (log-probs, advantages, masks, ids, metrics) plus "completion_ids" instead of the metrics alone."""
        import time
        timing = os.environ.get("IADR1_TIMING") == "1"

        def mark():
            if timing:
                torch.cuda.synchronize()
            return time.perf_counter()

        if completions is None and (old_logps is not None or ref_logps is not None or is_weights is not None):
            raise ValueError("old_logps / ref_logps / is_weights belong to completions that were rolled out earlier: hand those in too (completions=...)")
        if completions is not None and old_logps is not None and is_weights is None and self.args.rollout_is_cap > 0:
            raise ValueError("GRPOArgs.rollout_is_cap > 0: a reuse iteration (old_logps=...) needs the rollout_is_weights of the step that sampled (is_weights=...)")
        if completions is not None and old_logps is None and rollout_logps is None and self.args.rollout_is_cap > 0:
            raise ValueError("GRPOArgs.rollout_is_cap > 0: completions were handed in without their rollout log-probs (rollout_logps=...)")
        if completions is None and (rollout_entropy is not None or entropy_mask is not None):
            raise ValueError("rollout_entropy / entropy_mask belong to completions that were rolled out earlier: hand those in too (completions=...)")
        if completions is not None and old_logps is not None and entropy_mask is None and self.args.top_entropy_quantile < 1:
            raise ValueError("GRPOArgs.top_entropy_quantile < 1: a reuse iteration (old_logps=...) needs the entropy_mask of the step that sampled (entropy_mask=...)")
        if completions is not None and old_logps is None and rollout_entropy is None and self.args.top_entropy_quantile < 1:
            raise ValueError("GRPOArgs.top_entropy_quantile < 1: completions were handed in without their rollout entropies (rollout_entropy=...)")
        t0 = mark()
        vis = self.vision_policy(batch, save=True)
        t1 = mark()
        # two-phase policy forward: with one whole-batch micro-batch in the shared-prefix layout the rollout's prefill IS the prompt part of
        # the training forward (saved in the training arena), so the policy forward after the rollout only runs the completion rows
        a = self.args
        N = len(batch["input_ids"]) * a.num_generations
        carry = {} if (completions is None and a.share_prefix and a.reuse_prefill and a.num_generations > 1 and a.micro_batch_seqs >= N and N % a.num_generations == 0) else None
        if carry is not None and a.recompute != "off":
            P_ = np.asarray(batch["input_ids"]).shape[1] if a.max_prompt_length is None else min(np.asarray(batch["input_ids"]).shape[1], a.max_prompt_length)
            if self.pol.recompute_wanted(len(batch["input_ids"]) * P_ + N * a.max_completion_length, a.recompute):
                carry = None       # gradient checkpointing: nothing of the rollout is kept, the policy forward runs (checkpointed) before backward
        comp = self.rollout(batch, vis=vis, train_carry=carry, shadow_ref=a.beta != 0) if completions is None else np.asarray(completions)
        ref_lp = self.shadow_logps if completions is None else ref_logps
        pol_head = self.shadow_policy_head if completions is None else None
        ro_lp = (self.last_rollout_logps if completions is None else rollout_logps) if self.args.wants_rollout_logps else None
        ro_ent = (self.last_rollout_entropy if completions is None else rollout_entropy) if self.args.wants_rollout_entropy else None
        t2 = mark()
        # rewards are computed on the host inside loss_and_grads, after the first forward passes are in the GPU queue (in the
        # phase-timing mode they are evaluated here so that they get their own column)
        rewards = reward_fn(comp) if timing else (lambda: reward_fn(comp))
        t3 = mark()
        self.last_step_traced = bool(carry and carry.get("traced"))     # the decode steps filled the completion rows of the training arena
        last = do_optimizer_step if last_micro_step is None else last_micro_step
        out = self.loss_and_grads(batch, comp, rewards, backward=True, last_micro_step=last, vis=vis, train_carry=carry, defer_metrics=defer_metrics or do_optimizer_step,
                                  ref_logps=ref_lp, policy_head=pol_head, rollout_logps=ro_lp, old_logps=old_logps, is_weights=is_weights,
                                  rollout_entropy=ro_ent, entropy_mask=entropy_mask)
        self.last_step_shadowed = ref_lp is not None and completions is None
        t4 = mark()
        if do_optimizer_step:
            self.optimizer_step()
        if not defer_metrics and "finalize" in out["metrics"]:
            out["metrics"].pop("finalize")()
        t5 = mark()
        if timing:
            print(f"[iadr1 timing] vision {1e3*(t1-t0):.1f} ms | rollout {1e3*(t2-t1):.1f} | rewards {1e3*(t3-t2):.1f} | ref+policy fwd/bwd {1e3*(t4-t3):.1f} | optimizer {1e3*(t5-t4):.1f}", flush=True)
        if return_outputs:
            out["completion_ids"] = comp
            return out
        return out["metrics"]
