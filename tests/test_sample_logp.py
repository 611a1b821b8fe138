"""iadr1_sample_logp (csrc/sample.hip): the sampler's second entry point -- token ids bit-equal to iadr1_sample_topk_topp for top_k in 1..64, whole-vocabulary
sampling for top_k <= 0, and the temperature-1 unfiltered log-prob of every pick.  CPU expectations are numpy float64, written here; the oracle contributes its
Philox uniforms only.  The two tests at the end need no GPU."""
import math

import numpy as np
import pytest
import torch

import iadr1_amd  # noqa: F401
from iadr1_amd import hip, ops

DEV = "cuda"
F32 = torch.float32
VOCABS = [640, 5000, 151936]


def rnd(*shape, scale=1.0, seed=0, dtype=F32):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def close(got, ref, rtol, atol, what=""):
    got, ref = got.double().cpu(), ref.double().cpu()
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    assert not bool((err > tol).any()), f"{what}: {int((err > tol).sum())}/{ref.numel()} out of tol, max|err| {err.max().item():.4g}"


def ref_logp(lg, ids):
    return torch.log_softmax(lg.double(), -1).gather(1, ids.view(-1, 1)).squeeze(1)


@pytest.mark.gpu
@pytest.mark.parametrize("V", VOCABS)
def test_ids_are_bit_equal_to_the_old_entry_point(V):
    """(1) top_k = 50, top_p = 0.9, T = 0.9 and greedy: the ids of ops.sample, over 20 steps (3 at the large V), with suppress_token, step_ptr and seed_ptr."""
    B = 16
    lg = rnd(B, V, seed=1, scale=2.5)
    lg[2, 17] = lg[2, V - 100] = 50.0
    sup = int(lg[5].argmax())
    for T in (0.9, 0.0):
        for step in range(20 if V < 100000 else 3):
            a = ops.sample(lg, T, 50, 0.9, seed=1234567890123, step=step)
            b, lp = ops.sample_logp(lg, T, 50, 0.9, seed=1234567890123, step=step, logp_out=torch.zeros(B, 32, device=DEV))
            assert torch.equal(a, b), (T, step)
            close(lp[:, step], ref_logp(lg, b), 1e-5, 1e-5, f"logp T={T} step={step}")
        assert torch.equal(ops.sample(lg, T, 50, 0.9, seed=7, step=2, suppress_token=sup), ops.sample_logp(lg, T, 50, 0.9, seed=7, step=2, suppress_token=sup, want_logp=False)[0])
        sp = torch.tensor([7], dtype=torch.int32, device=DEV)
        sd = torch.tensor([1234567890123], dtype=torch.int64, device=DEV)
        assert torch.equal(ops.sample(lg, T, 50, 0.9, seed=5, step=0, step_ptr=sp), ops.sample_logp(lg, T, 50, 0.9, seed=5, step=0, step_ptr=sp, want_logp=False)[0])
        assert torch.equal(ops.sample(lg, T, 50, 0.9, seed=0, step=3, seed_ptr=sd), ops.sample_logp(lg, T, 50, 0.9, seed=0, step=3, seed_ptr=sd, want_logp=False)[0])
    assert ops.sample_logp(lg, 0.0, 50, 0.9, seed=1, step=0)[0][2].item() == 17          # tie: lowest index


@pytest.mark.gpu
@pytest.mark.parametrize("V", VOCABS)
def test_logp_is_the_full_row_log_softmax_of_the_pick(V):
    """(2) logp_out against float64 log_softmax gathered at the returned ids at the tolerance test_logprob_dlogits_grpo holds iadr1_logprob_rows to (1e-5, 1e-5):
    sampled with top-k/top-p, with a suppressed token (it still counts in the normaliser), greedy, whole vocabulary; step_ptr selects the column; a column
    outside the buffer leaves it untouched."""
    B = 16
    lg = rnd(B, V, seed=1, scale=2.5)
    sup = int(lg[5].argmax())
    for T, k, p, s in ((0.9, 50, 0.9, -1), (0.9, 50, 0.9, sup), (0.0, 50, 0.9, -1), (0.0, 50, 0.9, sup), (0.9, 0, 1.0, -1), (0.9, 0, 1.0, sup), (0.0, 0, 1.0, -1)):
        ids, lp = ops.sample_logp(lg, T, k, p, seed=99, step=0, suppress_token=s)
        assert lp.shape == (B, 1) and (s < 0 or ids[5].item() != sup)
        close(lp[:, 0], ref_logp(lg, ids), 1e-5, 1e-5, f"logp T={T} k={k} suppress={s}")
    buf = torch.full((B, 6), 7.0, device=DEV)
    sp = torch.tensor([4], dtype=torch.int32, device=DEV)
    ids, _ = ops.sample_logp(lg, 0.9, 0, 1.0, seed=3, step=0, step_ptr=sp, logp_out=buf)
    close(buf[:, 4], ref_logp(lg, ids), 1e-5, 1e-5, "column from step_ptr")
    keep = torch.ones(6, dtype=torch.bool)
    keep[4] = False
    assert bool((buf[:, keep.to(DEV)] == 7.0).all())
    wide = torch.full((B, 8), 7.0, device=DEV)
    view = wide[:, :6]                                # ld 8, 6 columns: step 6 and 7 are outside
    for st in (6, 7, 1000):
        ops.sample_logp(lg, 0.9, 50, 0.9, seed=3, step=st, logp_out=view)
    assert bool((wide == 7.0).all())


def _cdf(x64, T, sup):
    w = np.exp((x64 - x64[np.arange(x64.size) != sup].max() if sup >= 0 else x64 - x64.max()) / T)
    if sup >= 0:
        w[sup] = 0.0
    return np.cumsum(w)


@pytest.mark.gpu
@pytest.mark.parametrize("V", VOCABS)
def test_whole_vocabulary_draw_is_the_inverse_cdf_in_id_order(V):
    """(3) top_k = 0, T = 0.9: EVERY draw is checked against the float64 cumulative weights in id order: cdf[t-1] - tol <= u * cdf[-1] <= cdf[t] + tol with
    tol = 1e-4 * cdf[-1], the existing sampler test's margin for summation order.  The kernel's tree is at most 2 * (20 + 6 + 3) + 6 = 64 fp32 additions deep (20 serial
    adds per thread, 6 shuffle levels, 3 adds over the waves, once in stage 1 and once in stage 2, 6 shuffle levels over the 32 chunks): a few 1e-6 relative.  A pick
    from the wrong chunk or in another order fails at once.  The suppressed id is never drawn; scalar and device-resident step / seed give the same ids; two runs
    are identical."""
    from oracle import sampler as osamp
    B, T, seed = 16, 0.9, 1234567890123
    lg = rnd(B, V, seed=1, scale=2.5)
    x = lg.cpu().numpy().astype(np.float64)
    sup = int(lg[5].argmax())
    steps = 20 if V < 100000 else 3
    for s in (-1, sup):
        cdfs = [_cdf(x[b], T, s) for b in range(B)]
        for step in range(steps):
            got = ops.sample_logp(lg, T, 0, 1.0, seed=seed, step=step, suppress_token=s, want_logp=False)[0]
            assert torch.equal(got, ops.sample_logp(lg, T, 0, 1.0, seed=seed, step=step, suppress_token=s, want_logp=False)[0])
            for b, t in enumerate(got.tolist()):
                cdf = cdfs[b]
                tol = 1e-4 * cdf[-1]
                u = osamp.philox_uniform(seed, b, step) * cdf[-1]
                assert 0 <= t < V and t != s
                lo = cdf[t - 1] if t > 0 else 0.0
                assert lo - tol <= u <= cdf[t] + tol, (V, s, step, b, t, lo / cdf[-1], u / cdf[-1], cdf[t] / cdf[-1])
    sp = torch.tensor([7], dtype=torch.int32, device=DEV)
    sd = torch.tensor([seed], dtype=torch.int64, device=DEV)
    want = ops.sample_logp(lg, T, 0, 1.0, seed=seed, step=7, want_logp=False)[0]
    assert torch.equal(ops.sample_logp(lg, T, 0, 1.0, seed=seed, step=0, step_ptr=sp, want_logp=False)[0], want)
    assert torch.equal(ops.sample_logp(lg, T, 0, 1.0, seed=0, step=7, seed_ptr=sd, want_logp=False)[0], want)


@pytest.mark.gpu
def test_whole_vocabulary_frequencies():
    """(4) In the form of test_sampler_against_transformers_warpers: one row of V = 640 logits (torch.randn, CPU generator seeded 11, times 2.5) over 64 rows x 160
    steps = 10 240 draws at T = 0.9 against float64 softmax(x / T).  Over the tokens with expected count >= 5: every one drawn, |count - N p| < 4 sigma (that test's
    bound when more than 20 tokens are tested at once), chi-square < (n - 1) + 4.5 sqrt(2 (n - 1)) + 4.  An exact float64 inverse-CDF sampler on the same Philox
    uniforms gives, for sampler seed 979, max 2.97 sigma and chi-square 148 against 226 (146 tokens)."""
    g = torch.Generator(device="cpu").manual_seed(11)
    row = (torch.randn(640, generator=g) * 2.5).to(F32)
    B, STEPS, T = 64, 160, 0.9
    N = B * STEPS
    lg = row.to(DEV).repeat(B, 1).contiguous()
    pr = torch.softmax(row.double() / T, -1).numpy()
    draws = torch.stack([ops.sample_logp(lg, T, 0, 1.0, seed=979, step=s, want_logp=False)[0] for s in range(STEPS)]).flatten().cpu().numpy()
    cnt = np.bincount(draws, minlength=640).astype(np.float64)
    sel = N * pr >= 5
    n = int(sel.sum())
    assert n > 20
    z = np.abs(cnt - N * pr)[sel] / np.sqrt(N * pr * (1 - pr))[sel]
    print(f"[whole-vocabulary frequencies] {n} tokens tested, max {z.max():.2f} sigma")
    assert (cnt[sel] > 0).all(), "a token with expected count >= 5 is never drawn"
    assert z.max() < 4.0, f"frequency off by {z.max():.2f} sigma"
    chi2 = float((((cnt - N * pr) ** 2) / (N * pr))[sel].sum())
    print(f"[whole-vocabulary frequencies] chi2 {chi2:.1f} for {n - 1} dof")
    assert chi2 < (n - 1) + 4.5 * math.sqrt(2 * (n - 1)) + 4, f"chi2 {chi2:.1f} for {n - 1} dof"


@pytest.mark.gpu
@pytest.mark.parametrize("V", [33, 8200, 20011])
def test_slice_geometries_between_the_tested_vocabularies(V):
    """(4b) The slice geometries VOCABS does not reach (csize = ceil(V / 32) ids per chunk, per = ceil(csize / 256) ids per thread): V = 33: csize 2, per 1, chunks
    17..31 empty and top_k = 50 clamped to 33; V = 8200: csize 257, per 2, last chunk 233 of 257; V = 20011: csize 626, per 3, last chunk 605 of 626.  20 steps each.
    (a) greedy: sample, sample_logp and neutral sample_ex give argmax.  (b) T 0.9, top-k 50, top-p 0.9: the four entry points give the same ids, every id is in the
    oracle's candidate set and equals the oracle's pick wherever its margin exceeds 1e-4 (test_sampler_greedy_and_topk_topp's rule); at most 4 of the 320 draws may
    be skipped that way (the oracle alone skips 2 of 320 at each V).  (c) whole vocabulary, with and without a suppressed token: every draw inside the inverse-CDF
    bracket of (3) at tol = 1e-4 * cdf[-1], none skipped, and logp_out against float64 log_softmax at (1e-5, 1e-5)."""
    from oracle import sampler as osamp
    B, T, seed, STEPS = 16, 0.9, 1234567890123, 20
    lg = rnd(B, V, seed=1, scale=2.5)
    lgc = lg.cpu().numpy()
    x = lgc.astype(np.float64)
    sup = int(lg[5].argmax())
    amax = lg.argmax(-1)
    assert torch.equal(ops.sample(lg, 0.0, 50, 0.9, seed=seed, step=0), amax)
    assert torch.equal(ops.sample_logp(lg, 0.0, 50, 0.9, seed=seed, step=0, want_logp=False)[0], amax)
    assert torch.equal(ops.sample_ex(lg, 0.0, 50, 0.9, seed=seed, step=0, want_logp=False)[0], amax)
    cand = [set(osamp.candidates(lgc[b], T, 50, 0.9)[0].tolist()) for b in range(B)]
    skipped = 0
    for step in range(STEPS):
        got = ops.sample(lg, T, 50, 0.9, seed=seed, step=step)
        assert torch.equal(got, ops.sample_logp(lg, T, 50, 0.9, seed=seed, step=step, want_logp=False)[0]), step
        assert torch.equal(got, ops.sample_ex(lg, T, 50, 0.9, seed=seed, step=step, want_logp=False)[0]), step
        assert torch.equal(got, ops.sample_guided(lg, T, 50, 0.9, seed=seed, step=step, want_logp=False)[0]), step
        for b, t in enumerate(got.tolist()):
            assert t in cand[b], "sampled token outside the top-k/top-p candidate set"
            ref, margin = osamp.sample_row(lgc[b], T, 50, 0.9, seed, b, step)
            if margin > 1e-4:
                assert t == ref, (V, step, b, t, ref, margin)
            else:
                skipped += 1
    print(f"[slice geometries] V={V}: {skipped} of {B * STEPS} top-k/top-p draws within 1e-4 of a CDF edge")
    assert skipped <= 4
    for s in (-1, sup):
        cdfs = [_cdf(x[b], T, s) for b in range(B)]
        lp = torch.zeros(B, STEPS, device=DEV)
        for step in range(STEPS):
            got = ops.sample_logp(lg, T, 0, 1.0, seed=seed, step=step, suppress_token=s, logp_out=lp)[0]
            close(lp[:, step], ref_logp(lg, got), 1e-5, 1e-5, f"logp V={V} suppress={s} step={step}")
            for b, t in enumerate(got.tolist()):
                cdf = cdfs[b]
                tol = 1e-4 * cdf[-1]
                u = osamp.philox_uniform(seed, b, step) * cdf[-1]
                assert 0 <= t < V and t != s
                lo = cdf[t - 1] if t > 0 else 0.0
                assert lo - tol <= u <= cdf[t] + tol, (V, s, step, b, t, lo / cdf[-1], u / cdf[-1], cdf[t] / cdf[-1])


def test_a_nucleus_over_the_whole_vocabulary_is_refused_without_a_gpu():
    """(5) top_p < 1 with top_k <= 0: rc < 0 and a message through iadr1_last_error, detected on the host."""
    L = hip.lib()
    assert hip.version() >= 111 and L.iadr1_sample_logp_workspace_bytes(64) > L.iadr1_sample_workspace_bytes(64)
    for k in (0, -1):
        rc = L.iadr1_sample_logp(None, 0, None, None, 0, 0, None, 1, 8, 0.9, k, 0.9, -1, 0, 0, None, None, None)
        assert rc < 0 and b"sample" in L.iadr1_last_error() and b"top_p" in L.iadr1_last_error()
    rc = L.iadr1_sample_logp(None, 0, None, None, 0, 0, None, 0, 8, 0.9, 0, 1.0, -1, 0, 0, None, None, None)
    assert rc < 0 and b"sample" in L.iadr1_last_error()


def test_grpo_args_refuse_a_nucleus_over_the_whole_vocabulary_when_the_engine_is_built():
    from iadr1_amd.sc_grpo import GRPOArgs, SCGRPOEngine
    with pytest.raises(ValueError, match="top_p"):
        SCGRPOEngine(None, None, None, GRPOArgs(top_k=0, top_p=0.9))
    m = __import__("importlib").util
    import os
    spec = m.spec_from_file_location("grpo_ad_flags", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "train", "stage_rl", "grpo_ad.py"))
    mod = m.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.build_parser().parse_args(["--model_name_or_path", "/m", "--output_dir", "o", "--dataset_name", "d.json", "--top_k", "0", "--top_p", "1.0", "--rollout_logps"])
    assert a.top_k == 0 and a.top_p == 1.0 and a.rollout_logps is True
    d = mod.build_parser().parse_args(["--model_name_or_path", "/m", "--output_dir", "o", "--dataset_name", "d.json"])
    assert d.top_k == 50 and d.top_p == 0.9 and d.rollout_logps is False
