#!/usr/bin/env python3
"""A/B of the paged decode attention kernels between two builds of the library (IADR1_HIP_LIB selects one; a fresh process per library).
    python tools/attn_decode_ab.py bits OUT.pt   every output of attn_decode / attn_decode_group / kv_store / rope_kv_store / the fused q|k|v epilogue's cache
                                                 pages on the inputs of the kernel tests (tests/test_hip_kernels.py), saved for a byte comparison
    python tools/attn_decode_ab.py cmp A.pt B.pt compares two such files with torch.equal (no GPU)
    python tools/attn_decode_ab.py time          us per launch: attn_decode at the 3B decode shape, attn_decode_group at the LLaVA-OneVision-7B shape, rope_kv_store"""
import os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
mode = sys.argv[1]
if mode == "cmp":
    a, b = torch.load(sys.argv[2]), torch.load(sys.argv[3])
    bad = [k for k in a if not (a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)))]
    print(f"{len(a)} arrays, {len(a) - len(bad)} byte-equal" + ("".join(f"\n  DIFFERS: {k}" for k in bad)))
    sys.exit(1 if bad or a.keys() != b.keys() else 0)
import iadr1_amd  # noqa
from iadr1_amd import ops
dev, BF, F32, D, PAGE = "cuda", torch.bfloat16, torch.float32, 128, 32
rnd = lambda *shape, seed=0, scale=1.0: (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF).to(dev)


def group_case(Hq, Hkv, G, prompts, extra, fill):
    """The rollout's page layout: full prompt pages shared by the G sequences of a group, private pages for the prompt remainder + completion."""
    Bp, B = len(prompts), len(prompts) * G
    ctx = [prompts[b // G] + extra[b % G] + 1 for b in range(B)]
    n_shared = [p // PAGE for p in prompts]
    bt = torch.zeros(B, max((c + PAGE - 1) // PAGE for c in ctx) + 1, dtype=torch.int32)
    nxt = 1 + sum(n_shared)
    first = [1 + sum(n_shared[:b]) for b in range(Bp)]
    for r in range(B):
        ns, priv = n_shared[r // G], (ctx[r] + PAGE - 1) // PAGE - n_shared[r // G]
        bt[r, :ns] = torch.arange(first[r // G], first[r // G] + ns)
        bt[r, ns:ns + priv] = torch.arange(nxt, nxt + priv)
        nxt += priv
    kc, vc = torch.zeros(nxt + 1, Hkv, 32, D, dtype=BF, device=dev), torch.zeros(nxt + 1, Hkv, D, 32, dtype=BF, device=dev)
    if fill == "random":        # timing: the values do not matter
        kc, vc = rnd(*kc.shape, seed=1), rnd(*vc.shape, seed=2)
    else:
        for b in range(Bp):
            pk, pv = rnd(prompts[b], Hkv * D, seed=100 + b), rnd(prompts[b], Hkv * D, seed=200 + b)
            for r in range(b * G, b * G + G):
                pos = torch.arange(ctx[r])
                slot = (bt[r][pos // PAGE].long() * PAGE + pos % PAGE).to(dev)
                ops.kv_store(torch.cat([pk, rnd(ctx[r] - prompts[b], Hkv * D, seed=300 + r)]), torch.cat([pv, rnd(ctx[r] - prompts[b], Hkv * D, seed=400 + r)]), slot, kc, vc, Hkv, D)
    return rnd(B, Hq * D, seed=5), kc, vc, bt.to(dev), torch.tensor(ctx, dtype=torch.int32, device=dev), torch.tensor(n_shared, dtype=torch.int32, device=dev)


def side(B, Hq):
    T = B * 8 + 10
    o, l = torch.zeros(T, Hq * D, dtype=BF, device=dev), torch.zeros(Hq, T, dtype=F32, device=dev)
    return ops.SideOut.make(torch.tensor([3], dtype=torch.int32, device=dev), 2, 8, p0=o, p1=l, ld1=T), o, l


if mode == "bits":
    out = {}
    for ci, (Hq, Hkv, lens) in enumerate([(16, 2, [1, 33, 64, 517, 767]), (2, 1, [7, 32, 100]), (28, 4, [300, 31])]):       # test_decode_attention_and_kv_store
        B, maxp = len(lens), (max(lens) + 31) // 32
        npages = B * maxp + 3
        kc, vc = torch.zeros(npages, Hkv, 32, D, dtype=BF, device=dev), torch.zeros(npages, Hkv, D, 32, dtype=BF, device=dev)
        perm = torch.randperm(npages, generator=torch.Generator().manual_seed(0))[: B * maxp].view(B, maxp).to(torch.int32)
        slot = torch.cat([perm[b, torch.arange(n) // 32].long() * 32 + torch.arange(n) % 32 for b, n in enumerate(lens)] + [torch.tensor([-1])]).to(dev)
        ops.kv_store(torch.cat([rnd(n, Hkv * D, seed=10 + b) for b, n in enumerate(lens)] + [rnd(1, Hkv * D, seed=99)]),
                     torch.cat([rnd(n, Hkv * D, seed=20 + b) for b, n in enumerate(lens)] + [rnd(1, Hkv * D, seed=98)]), slot, kc, vc, Hkv, D)
        q, ctx = rnd(B, Hq * D, seed=5), torch.tensor(lens, dtype=torch.int32, device=dev)
        so, so_o, so_l = side(B, Hq)
        out[f"seq{ci}.kc"], out[f"seq{ci}.vc"] = kc, vc
        out[f"seq{ci}.o"] = ops.attn_decode(q, kc, vc, perm.to(dev), ctx, Hq, Hkv, D, D ** -0.5, side=so)
        out[f"seq{ci}.side_o"], out[f"seq{ci}.side_lse"] = so_o, so_l
        out[f"seq{ci}.o_packed"] = ops.attn_decode(q, kc, vc, perm.to(dev), ctx, Hq, Hkv, D, D ** -0.5, out=ops.PackedAct(B, Hq * D, dev)).buf
        qkv = rnd(B, (Hq + 2 * Hkv) * D, seed=7)
        ang = torch.rand(B, D // 2, generator=torch.Generator().manual_seed(3)) * 6.28
        new_slot = torch.stack([perm[b, lens[b] // 32].long() * 32 + lens[b] % 32 for b in range(B)]).to(dev)
        kc2, vc2 = kc.clone(), vc.clone()
        ops.rope_kv_store(qkv, ang.cos().to(dev), ang.sin().to(dev), new_slot, kc2, vc2, Hq, Hkv, D)
        out[f"seq{ci}.rope_qkv"], out[f"seq{ci}.rope_kc"], out[f"seq{ci}.rope_vc"] = qkv, kc2, vc2
    cases = [(16, 2, 8, [512, 777], [0, 5, 130, 31, 64, 1, 255, 200]), (32, 32, 8, [832], [3, 60, 0, 128, 7, 33, 90, 255]), (32, 8, 8, [3184, 40], [1, 2, 3, 4, 5, 6, 7, 8]),
             (28, 4, 8, [100], [9, 19, 29, 39, 49, 59, 69, 79]), (2, 1, 4, [7, 64, 31], [0, 1, 32, 40]), (16, 16, 3, [300], [5, 6, 7])]
    for ci, (Hq, Hkv, G, prompts, extra) in enumerate(cases):                                                               # test_decode_attention_group_equals_per_sequence
        q, kc, vc, bt, ctx, sp = group_case(Hq, Hkv, G, prompts, extra, "kv_store")
        B = q.shape[0]
        out[f"grp{ci}.kc"], out[f"grp{ci}.vc"] = kc, vc
        out[f"grp{ci}.o_seq"] = ops.attn_decode(q, kc, vc, bt, ctx, Hq, Hkv, D, D ** -0.5, seqs_per_group=G)
        for chunks in (1, 2, 5):
            so, so_o, so_l = side(B, Hq)
            out[f"grp{ci}.c{chunks}.o"] = ops.attn_decode_group(q, kc, vc, bt, ctx, sp, G, Hq, Hkv, D, D ** -0.5, chunks=chunks)
            out[f"grp{ci}.c{chunks}.o_side"] = ops.attn_decode_group(q, kc, vc, bt, ctx, sp, G, Hq, Hkv, D, D ** -0.5, chunks=chunks, side=so)
            out[f"grp{ci}.c{chunks}.side_o"], out[f"grp{ci}.c{chunks}.side_lse"] = so_o, so_l
            out[f"grp{ci}.c{chunks}.o_packed"] = ops.attn_decode_group(q, kc, vc, bt, ctx, sp, G, Hq, Hkv, D, D ** -0.5, chunks=chunks, out=ops.PackedAct(B, Hq * D, dev)).buf
    for ci, (Hq, Hkv, M) in enumerate([(16, 2, 64), (2, 1, 5), (28, 4, 33)]):                                               # test_fused_qkv_rope_kv_equals_gemm_then_rope_kv_store
        N, K = (Hq + 2 * Hkv) * D, 256
        x, w, bias = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.3), rnd(N, seed=3)
        ang = torch.rand(M, D // 2, generator=torch.Generator().manual_seed(3)) * 6.28
        slot = (torch.arange(M) * 32 + (torch.arange(M) * 7) % 32 + 32).to(dev)
        slot[M // 2] = -1
        kc1, vc1, kc2, vc2 = rnd(M + 2, Hkv, 32, D, seed=4), rnd(M + 2, Hkv, D, 32, seed=5), rnd(M + 2, Hkv, 32, D, seed=4), rnd(M + 2, Hkv, D, 32, seed=5)
        qkv = ops.gemm_skinny(x, ops.pack_weight(w), N, bias=bias)
        ops.rope_kv_store(qkv, ang.cos().to(dev), ang.sin().to(dev), slot, kc1, vc1, Hq, Hkv, D)
        wp, bp = ops.pack_qkv_rope(w, bias, Hq, Hkv, D)
        q2 = torch.zeros(M, N, dtype=BF, device=dev)
        ops.gemm_qkv_rope_kv(ops.pack_act(x), wp, bp, q2, ang.cos().to(dev), ang.sin().to(dev), slot, kc2, vc2, Hq, Hkv, D)
        for k_, t in (("qkv", qkv), ("kc", kc1), ("vc", vc1), ("fused_q", q2), ("fused_kc", kc2), ("fused_vc", vc2)):
            out[f"qkv{ci}.{k_}"] = t
    torch.cuda.synchronize()
    torch.save({k: v.cpu() for k, v in out.items()}, sys.argv[2])
    print(f"{len(out)} arrays -> {sys.argv[2]}")
    sys.exit(0)


def timeit(fn, n, reps=20):
    for i in range(n): fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for r in range(reps):
        for i in range(n): fn(i)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (reps * n) * 1e3


# 3B decode shape (tools/kernel_stamps.py): 64 sequences, 16 / 2 heads, context 640, four rotating caches
M, Hq, Hkv = 64, 16, 2
npages = 64 * 26 + 8
bt = (torch.arange(26, dtype=torch.int32)[None] + torch.arange(M, dtype=torch.int32)[:, None] * 26 + 1).to(dev)
ctx = torch.full((M,), 640, dtype=torch.int32, device=dev)
kcs = [rnd(npages, Hkv, 32, D, seed=i) for i in range(4)]
vcs = [rnd(npages, Hkv, D, 32, seed=10 + i) for i in range(4)]
q, o = rnd(M, Hq * D, seed=5), ops.PackedAct(M, Hq * D, dev)
print(f"attn_decode 3B ctx 640        {timeit(lambda i: ops.attn_decode(q, kcs[i % 4], vcs[i % 4], bt, ctx, Hq, Hkv, D, D ** -0.5, out=o), 4):7.2f} us", flush=True)
qkv = rnd(M, (Hq + 2 * Hkv) * D, seed=7)
cos, sin = torch.ones(M, D // 2, device=dev), torch.zeros(M, D // 2, device=dev)
slot = ((torch.arange(M, dtype=torch.int64) * 26 + 20) * 32 + 5).to(dev)
print(f"rope_kv_store 64 tokens       {timeit(lambda i: ops.rope_kv_store(qkv, cos, sin, slot, kcs[i % 4], vcs[i % 4], Hq, Hkv, D), 4):7.2f} us", flush=True)
del kcs, vcs
# LLaVA-OneVision-7B: 8 groups x 8 sequences, 28 / 4 heads, 3900 shared prompt tokens, the rollout's 8 chunks
Hq, Hkv, G = 28, 4, 8
q, kc, vc, bt, ctx, sp = group_case(Hq, Hkv, G, [3900] * 8, [100 + 17 * s for s in range(8)], "random")
ws, o = ops.attn_decode_group_ws(64, G, Hq, Hkv, D, 8, dev), ops.PackedAct(64, Hq * D, dev)
print(f"attn_decode_group LLaVA-OV-7B {timeit(lambda i: ops.attn_decode_group(q, kc, vc, bt, ctx, sp, G, Hq, Hkv, D, D ** -0.5, out=o, chunks=8, ws=ws), 1):7.2f} us", flush=True)
