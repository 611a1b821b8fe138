"""iadr1_ref_mix (csrc/optim.hip): reference <- alpha * policy + (1 - alpha) * reference over a flat bf16 buffer, the kernel under GRPOArgs.sync_ref_model.
The reference of every GPU test is a restatement written here: fp32 torch ops on the CPU as separate mul / add tensors (which cannot contract), one .bfloat16(),
and the same-bits select.  The argument tests need no GPU."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import iadr1_amd  # noqa: F401
from iadr1_amd import hip

DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
MAX_BLOCKS = 4096                       # the grid cap the header states (iadr1_adamw_flat's)
G = MAX_BLOCKS * 256 * 8                # elements one trip of the capped grid covers
ALPHAS = [0.6, 0.1, 0.999, 2.0 ** -8, 1.0]
SIZES = [8, 2040, 2048, 2056, G + 8]    # one lane; one block less a lane, exactly, plus a lane; a second trip of the grid-stride loop
PAD = 64                                # sentinel elements in front of and behind each buffer (128 bytes: the views stay 16-byte aligned)
SENTINEL = 0x7FC1                       # a NaN pattern no arithmetic here produces

# bf16 bit patterns written into BOTH buffers at the same positions (equal bits: the select must hand them back untouched): +-0, the largest and the smallest
# normal of either sign, subnormals (the smallest, the largest, one in between)
SAME = [0x0000, 0x8000, 0x7F7F, 0xFF7F, 0x0080, 0x8080, 0x0001, 0x807F, 0x0040]
# (ref, pol) pairs that DIFFER and go through the arithmetic: zeros of opposite sign, two subnormals, a subnormal against the smallest normal, the two largest
# normals (c * x + a * y stays finite: a + c <= 1 + 2^-24 and the smaller operand pulls the sum below the largest bf16's rounding boundary)
DIFFER = [(0x0000, 0x8000), (0x8000, 0x0000), (0x0001, 0x0003), (0x8040, 0x0040), (0x0080, 0x007F), (0x7F7F, 0x7F7E), (0xFF7E, 0xFF7F)]


def coefficients(alpha):
    """(a, c) as the entry point forms them: a = (float)alpha, c = (float)(1.0 - (double)a)."""
    a = np.float32(alpha)
    return a, np.float32(np.float64(1.0) - np.float64(a))


def bits(t):
    return t.view(torch.int16)


def from_bits(words):
    return torch.tensor(words, dtype=torch.int32).to(torch.int16).view(BF16) if len(words) else torch.empty(0, dtype=BF16)


def special_positions(n):
    """{"same": [(position, word)], "differ": [(position, ref word, pol word)], "stripe": (lo, hi)} for a buffer of n elements.  n = 8 holds four equal specials, a
    two-element stripe and two random elements; larger buffers hold every special three times -- near the front, in the last 2048 elements (the last block, and for
    n > G the second trip of the loop) and around the middle -- and a 16-element stripe."""
    if n == 8:
        return {"same": [(i, w) for i, w in enumerate(SAME[:4])], "differ": [], "stripe": (4, 6)}
    same, differ = [], []
    for base, step in ((3, 7), (n - 8 - 7 * (len(SAME) + len(DIFFER)), 7), (n // 2 + 32, 5)):
        for k, w in enumerate(SAME):
            same.append((base + step * k, w))
        for k, (r, p) in enumerate(DIFFER):
            differ.append((base + step * (len(SAME) + k), r, p))
    if n > G:       # the few elements of the second trip hold some too
        same += [(G + k, w) for k, w in enumerate(SAME[:4])]
        differ += [(G + 4 + k, r, p) for k, (r, p) in enumerate(DIFFER[:n - G - 4])]
    return {"same": same, "differ": differ, "stripe": (n // 2, n // 2 + 16)}


def make_inputs(n, seed, specials=True):
    """ref ~ 0.02 N(0, 1) in bf16, pol = ref + 1e-3 N(0, 1) in bf16; with `specials` the overwrites of special_positions."""
    g = torch.Generator().manual_seed(seed)
    ref32 = 0.02 * torch.randn(n, generator=g, dtype=F32)
    ref = ref32.to(BF16)
    pol = (ref.float() + 1e-3 * torch.randn(n, generator=g, dtype=F32)).to(BF16)
    sp = special_positions(n)
    lo, hi = sp["stripe"]
    pol[lo:hi] = ref[lo:hi]
    if specials:
        for pos, w in sp["same"]:
            ref[pos] = pol[pos] = from_bits([w])[0]
        for pos, r, p in sp["differ"]:
            ref[pos], pol[pos] = from_bits([r])[0], from_bits([p])[0]
    return ref, pol


def restate(ref, pol, alpha):
    """The contract, on the CPU: out = bf16_rn(fl(c * ref) + fl(a * pol)) with the products and the sum separate fp32 tensors, elements with equal bits kept,
    alpha == 1 a copy of pol."""
    if alpha == 1.0:
        return pol.clone()
    a, c = coefficients(alpha)
    x = ref.float() * torch.tensor(c, dtype=F32)
    y = pol.float() * torch.tensor(a, dtype=F32)
    out = (x + y).to(BF16)
    return torch.where(bits(ref) == bits(pol), ref, out)


def depth(n):
    """D of the kernel comment / header for n elements: 8 T + ceil(B / 256) + 23."""
    B = min((n + 2047) // 2048, MAX_BLOCKS)
    T = (n + 2048 * B - 1) // (2048 * B)
    return 8 * T + (B + 255) // 256 + 23


def call(ref_buf, pol_buf, n, alpha, dist2):
    L = hip.lib()
    partials = torch.full((L.iadr1_ref_mix_partials(),), float("nan"), dtype=F32, device=DEV) if dist2 is not None else None
    hip.call("ref_mix", ref_buf[PAD: PAD + n], pol_buf[PAD: PAD + n], n, float(alpha), partials, dist2)


def padded(t):
    buf = torch.full((t.numel() + 2 * PAD,), SENTINEL, dtype=torch.int32).to(torch.int16).view(BF16)
    buf[PAD: PAD + t.numel()] = t
    return buf.to(DEV)


@functools.lru_cache(maxsize=None)
def run(alpha, n, specials=True):
    """One call with dist2 and one without on the same inputs (and, for the run-to-run check, a second call with): everything comes back to the host once and is
    shared by the tests below."""
    ref, pol = make_inputs(n, seed=1000 + n % 997, specials=specials)
    first, same_bits, clean, dists = None, [], [], []
    for with_dist in (True, True, False):
        rb, pb = padded(ref), padded(pol)
        d = torch.full((2,), float("nan"), dtype=F32, device=DEV) if with_dist else None
        call(rb, pb, n, alpha, d)
        torch.cuda.synchronize()
        rb, pb = rb.cpu(), pb.cpu()
        words = [bits(b).to(torch.int32) & 0xFFFF for b in (rb, pb)]
        clean.append(all(bool((w[:PAD] == SENTINEL).all()) and bool((w[PAD + n:] == SENTINEL).all()) for w in words) and torch.equal(bits(pb[PAD: PAD + n]), bits(pol)))
        if first is None:
            first = rb[PAD: PAD + n].clone()
        same_bits.append(torch.equal(bits(rb[PAD: PAD + n]), bits(first)))
        dists.append(None if d is None else d.cpu())
    return {"ref": ref, "pol": pol, "out": first, "same_bits": same_bits, "clean": clean, "dist2": dists}


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------------------------------

def test_library_exports_the_entry_points():
    assert hip.version() >= 119
    assert "iadr1_ref_mix" in hip.PROTOS and "iadr1_ref_mix_partials" in hip.PROTOS
    assert [n for _, n in hip.PROTOS["iadr1_ref_mix"][1]] == ["ref_bf16", "pol_bf16", "n", "alpha", "partials", "dist2", "stream"]
    assert hip.lib().iadr1_ref_mix_partials() == 2 * MAX_BLOCKS
    assert "callbacks.py:107-109" in open(hip.HEADER).read()


def _raw_call(n=64, ref_off=0, pol_off=0, alpha=0.6, dist=False, partials=False):
    """The entry point on host addresses: every case here must be refused before anything is launched (nothing is ever read through them)."""
    L = hip.lib()
    buf = (ctypes.c_float * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    ptr = lambda off: None if off is None else base + off
    rc = L.iadr1_ref_mix(ptr(ref_off), ptr(pol_off), n, alpha, ptr(64) if partials else None, ptr(128) if dist else None, None)
    return rc, L.iadr1_last_error().decode()


@pytest.mark.parametrize("kw,words", [({"n": 0}, ("n", "0")), ({"n": -8}, ("n", "-8")), ({"n": 12}, ("multiple of 8", "12")), ({"n": 2047}, ("multiple of 8", "2047")),
                                      ({"ref_off": None}, ("ref", "must be given")), ({"pol_off": None}, ("pol", "must be given")),
                                      ({"ref_off": 2}, ("ref", "16-byte aligned")), ({"pol_off": 8}, ("pol", "16-byte aligned")),
                                      ({"alpha": 0.0}, ("alpha", "0")), ({"alpha": -0.25}, ("alpha", "-0.25")), ({"alpha": 1.5}, ("alpha", "1.5")),
                                      ({"alpha": float("nan")}, ("alpha", "nan")), ({"alpha": float("inf")}, ("alpha", "inf")),
                                      ({"dist": True}, ("dist2", "partials"))])
def test_arguments_outside_the_contract_are_refused_without_a_gpu(kw, words):
    rc, msg = _raw_call(**kw)
    assert rc < 0 and "ref_mix" in msg and all(w in msg for w in words), (rc, msg)


def test_the_restatement_itself():
    """The reference of the GPU tests on values that can be checked by hand: equal bits stay, alpha = 1 copies, 0.5 / 0.5 of 1 and 3 is 2, and one rounding
    (1 + 2^-7 and 1 mixed half and half is 1 + 2^-8, a tie that rounds to the even 1.0)."""
    ref = torch.tensor([1.0, 1.0, 0.3, 1.0 + 2.0 ** -7], dtype=F32).to(BF16)
    pol = torch.tensor([3.0, 1.0, 0.3, 1.0], dtype=F32).to(BF16)
    out = restate(ref, pol, 0.5)
    assert out.float().tolist() == [2.0, 1.0, float(ref[2]), 1.0]
    assert torch.equal(bits(restate(ref, pol, 1.0)), bits(pol))
    assert depth(8) == 8 + 1 + 23 and depth(G + 8) == 16 + 16 + 23 and depth(G) == 8 + 16 + 23


# ---- GPU, kernel level -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_bits_against_the_restatement(alpha, n):
    """(1) ref after the call equals the restatement bit for bit; the identical-bit stripe and the equal specials come back unchanged; alpha = 1 gives pol."""
    r = run(alpha, n)
    ref, pol = r["ref"], r["pol"]
    want = restate(ref, pol, alpha)
    got = r["out"]
    diff = bits(got) != bits(want)
    assert not bool(diff.any()), (f"{int(diff.sum())} of {n} elements differ from the restatement; first at {int(diff.nonzero()[0])}: "
                                  f"ref {ref[diff][0].item()!r} pol {pol[diff][0].item()!r} got {got[diff][0].item()!r} want {want[diff][0].item()!r}")
    sp = special_positions(n)
    lo, hi = sp["stripe"]
    assert torch.equal(bits(got[lo:hi]), bits(ref[lo:hi]))
    for pos, w in sp["same"]:
        assert int(bits(got)[pos]) & 0xFFFF == w, (pos, hex(w))
    if alpha == 1.0:
        assert torch.equal(bits(got), bits(pol))
    if n > 8 and alpha != 1.0:      # the inputs really exercise the arithmetic: most elements move, the rest are fixed points of the rounding or of the select
        assert int((bits(got) != bits(ref)).sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_nothing_outside_the_buffers_is_written_and_pol_is_only_read(alpha, n):
    """(2) the sentinels in front of and behind both buffers are untouched; pol is unchanged bit for bit; with and without dist2."""
    assert run(alpha, n)["clean"] == [True, True, True]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_against_float64(alpha, n):
    """(3) every output is within half a bf16 ulp of a * pol + c * ref taken in float64 from the fp32 a and c, plus 3 * 2^-24 * (|c ref| + |a pol|) for the three
    fp32 roundings.  The ulp is that of the larger of the result and the exact value (they may sit on either side of a power of two), 2^-133 below the normals."""
    r = run(alpha, n)
    a, c = coefficients(alpha)
    ref, pol = r["ref"].to(F64), r["pol"].to(F64)
    got = r["out"].to(F64)
    ta, tc = float(a) * pol, float(c) * ref
    exact = ta + tc
    mag = torch.maximum(exact.abs(), got.abs()).clamp(min=2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    bound = 0.5 * ulp + 3 * 2.0 ** -24 * (tc.abs() + ta.abs())
    err = (got - exact).abs()
    worst = int((err - bound).argmax())
    print(f"[ref_mix f64] alpha {alpha:g} n {n}: max err / bound = {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()), (worst, float(err[worst]), float(bound[worst]), float(ref[worst]), float(pol[worst]))


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [0.6, 0.1, 0.999])
def test_record_the_distance_from_torch_in_place_arithmetic(alpha):
    """(4) torch's own in-place mul_().add_(alpha=) on the CPU copies (bf16 tensors: two roundings, alpha rounded to bf16) against the kernel: the number of differing
    elements and the largest distance in bf16 ulps are printed, not asserted (profiles/EXPERIMENTS.md has the record)."""
    n = G + 8
    r = run(alpha, n)
    t = r["ref"].clone()
    t.mul_(1.0 - alpha).add_(r["pol"], alpha=alpha)
    got = r["out"]

    def ordered(x):     # bf16 bits -> integers in value order
        w = bits(x).to(torch.int32)
        return torch.where(w < 0, -(w & 0x7FFF), w)
    d = (ordered(got) - ordered(t)).abs()
    # (the distance counts representable values in between, so a pair of tiny results on either side of zero is thousands of ulps apart)
    print(f"[ref_mix vs torch in-place] alpha {alpha:g}, {n} elements: {int((d != 0).sum())} differ ({int((d > 1).sum())} by more than one ulp), largest distance {int(d.max())} bf16 ulps")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_distance_sums_against_float64(n):
    """(5) dist2 = {sum (pol - ref)^2, sum ref^2} over the inputs against float64 at relative D * 2^-23, D the documented depth of the summation tree for this n;
    two calls give the same bits; without dist2 the reference gets the same bits.  Inputs: the Gaussian buffers with the stripe, without the special values -- the
    square of the largest normal is not an fp32 number (the special values' own bits are test 1's business; their dist2 is checked below to be the same twice)."""
    r = run(0.6, n, False)
    ref, pol = r["ref"].to(F64), r["pol"].to(F64)
    want = torch.stack([((pol - ref) ** 2).sum(), (ref ** 2).sum()])
    got = r["dist2"][0].to(F64)
    D = depth(n)
    rel = ((got - want).abs() / want)
    print(f"[ref_mix dist2] n {n}: D {D}, relative errors {rel.tolist()} against {D * 2.0 ** -23:.3e}; relative distance {math.sqrt(float(got[0] / got[1])):.5f}")
    assert bool((want > 0).all()) and bool((rel <= D * 2.0 ** -23).all()), (got.tolist(), want.tolist())
    for rr in (r, run(0.6, n)):
        assert torch.equal(rr["dist2"][0].view(torch.int32), rr["dist2"][1].view(torch.int32))
        assert rr["same_bits"] == [True, True, True]
