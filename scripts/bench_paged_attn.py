"""Micro-bench decode attention at bench-like shapes: the fused op
(ops.paged_attention_rope, one launch when S <= 8) against the three-launch
sequence rope_kv_append + paged_attention (attention + reduce), with the
achieved KV bandwidth vs the ~6.3 TB/s practical HBM3E roofline.

Same process, alternating, median of ROUNDS rounds. Each variant is a
captured graph (as in serving) of one call per cache copy; the copies
rotate so that every call streams KV the LLC no longer holds (enough
copies to overflow a 256 MB LLC twice). Prints one JSON line per shape.

  python scripts/bench_paged_attn.py [--kv-dtype fp8] [--batches 64,8,...]

--shared-prefix measures the op behind session fork instead, by the same
method: 64 sessions on one shared prefix, ops.paged_attention_rope_shared
against ops.paged_attention_rope on the same caches.

  python scripts/bench_paged_attn.py --shared-prefix [--kv-dtype fp8]
"""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
import kukeon_amd.ops as ops  # noqa: E402

DEV = "cuda:0"
Hq, Hk, D, BS = 32, 8, 128, 16
LLC_BYTES = 256 << 20
ROUNDS = 7
MAXPOS = 4096


def engine_splits(B):
    """LLMEngine._decode_splits for Hk kv heads."""
    want = (16 * 256 + B * Hk - 1) // (B * Hk)
    return max(4, min(32, ((want + 3) // 4) * 4))


def make_graph(fn, n):
    for i in range(n):          # warm up outside capture
        fn(i)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(n):
            fn(i)
    return g


def time_graph(g, n, reps):
    """us per call of one replay train."""
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * n)


def bench_shape(B, ctx_lo, ctx_hi, fp8, splits=None):
    gen = torch.Generator().manual_seed(B * 7919 + ctx_lo)
    ctxs = torch.randint(ctx_lo, ctx_hi + 1, (B,), generator=gen).tolist()
    nb = [(c + BS - 1) // BS for c in ctxs]
    NB = sum(nb) + 8
    esz = 1 if fp8 else 2
    kv_bytes = sum(ctxs) * Hk * D * esz * 2
    copies = max(2, -(-2 * LLC_BYTES // kv_bytes) + 1)

    def cache():
        x = torch.randn(NB, Hk, BS, D, dtype=torch.bfloat16, device=DEV)
        if fp8:
            x = x.float().to(torch.float8_e4m3fn).view(torch.uint8)
        return x

    kcs = [cache() for _ in range(copies)]
    vcs = [cache() for _ in range(copies)]
    bt = torch.zeros(B, max(nb), dtype=torch.int32, device=DEV)
    nxt = 0
    for b in range(B):
        bt[b, : nb[b]] = torch.arange(nxt, nxt + nb[b], dtype=torch.int32)
        nxt += nb[b]
    seq_lens = torch.tensor(ctxs, dtype=torch.int32, device=DEV)
    pos = seq_lens - 1
    slots = torch.zeros(B, dtype=torch.int32, device=DEV)
    inv = 1.0 / (500000.0 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.outer(torch.arange(MAXPOS).float(), inv)
    cos_sin = torch.cat([fr.cos(), fr.sin()], dim=1).to(DEV)
    qkv = torch.randn(B, (Hq + 2 * Hk) * D, dtype=torch.bfloat16, device=DEV)
    qkv_seq = qkv.clone()   # the sequence rotates its qkv in place
    out = torch.empty(B, Hq * D, dtype=torch.bfloat16, device=DEV)
    scale = D ** -0.5
    S = splits or engine_splits(B)
    tmp_out = torch.zeros(B, Hq, S, D, dtype=torch.float32, device=DEV)
    tmp_ml = torch.zeros(B, Hq, S, 2, dtype=torch.float32, device=DEV)

    def fused(i):
        ops.paged_attention_rope(out, qkv, kcs[i], vcs[i], cos_sin, pos, bt,
                                 seq_lens, Hq, Hk, S, scale, tmp_out, tmp_ml)

    def sequence(i):
        ops.rope_kv_append(qkv_seq, kcs[i], vcs[i], cos_sin, pos, slots, Hq,
                           Hk, D, block_table=bt)
        ops.paged_attention(out, qkv_seq, kcs[i], vcs[i], bt, seq_lens, 0, S,
                            scale, tmp_out, tmp_ml)

    graphs = {"fused": make_graph(fused, copies),
              "sequence": make_graph(sequence, copies)}
    reps = max(2, 200 // copies)
    times = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():     # alternating
            times[k].append(time_graph(g, copies, reps))
    res = {"B": B, "ctx": [ctx_lo, ctx_hi], "kv": "fp8" if fp8 else "bf16",
           "splits": S, "kv_mb": round(kv_bytes / 1e6, 1), "copies": copies}
    for k, ts in times.items():
        med = statistics.median(ts)
        res[k + "_us"] = round(med, 2)
        res[k + "_spread_us"] = round(max(ts) - min(ts), 2)
        res[k + "_tbps"] = round(kv_bytes / (med * 1e-6) / 1e12, 2)
    res["sequence_over_fused"] = round(res["sequence_us"] / res["fused_us"], 3)
    print(json.dumps(res), flush=True)
    return res


def engine_prefix_splits(B, hq):
    """LLMEngine._prefix_splits for Hk kv heads and hq q heads."""
    tiles = max(1, B // (16 // (hq // Hk)))
    want = (4 * 256 + tiles * Hk - 1) // (tiles * Hk)
    return max(8, min(32, ((want + 3) // 4) * 4))


def bench_shared(B, prefix, fp8, hq, prefix_splits=None):
    """B sessions forked from one `prefix`-token context (a multiple of the
    block size), each with 64-384 tokens of its own: the shared-prefix op
    against the unshared one on the same caches. bf16 compares the fused
    ops, fp8 the sequences the engine runs for an fp8 cache
    (rope_kv_append + paged_attention[_shared])."""
    assert prefix % BS == 0
    G = hq // Hk
    W = 16 // G
    P = prefix // BS
    gen = torch.Generator().manual_seed(B * 7919 + prefix)
    ctxs = [prefix + s for s in
            torch.randint(64, 385, (B,), generator=gen).tolist()]
    own = [(c + BS - 1) // BS - P for c in ctxs]
    NB = P + sum(own) + 8
    esz = 1 if fp8 else 2
    # what the unshared op streams; the distinct bytes are far fewer
    kv_bytes = sum(ctxs) * Hk * D * esz * 2
    distinct = (prefix + sum(c - prefix for c in ctxs)) * Hk * D * esz * 2
    copies = max(2, -(-2 * LLC_BYTES // distinct) + 1)

    def cache():
        x = torch.randn(NB, Hk, BS, D, dtype=torch.bfloat16, device=DEV)
        if fp8:
            x = x.float().to(torch.float8_e4m3fn).view(torch.uint8)
        return x

    kcs = [cache() for _ in range(copies)]
    vcs = [cache() for _ in range(copies)]
    bt = torch.zeros(B, P + max(own), dtype=torch.int32, device=DEV)
    nxt = P
    for b in range(B):
        bt[b, :P] = torch.arange(P, dtype=torch.int32)
        bt[b, P:P + own[b]] = torch.arange(nxt, nxt + own[b],
                                           dtype=torch.int32)
        nxt += own[b]
    seq_lens = torch.tensor(ctxs, dtype=torch.int32, device=DEV)
    pos = seq_lens - 1
    slots = torch.zeros(B, dtype=torch.int32, device=DEV)
    inv = 1.0 / (500000.0 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.outer(torch.arange(MAXPOS).float(), inv)
    cos_sin = torch.cat([fr.cos(), fr.sin()], dim=1).to(DEV)
    qkv = torch.randn(B, (hq + 2 * Hk) * D, dtype=torch.bfloat16, device=DEV)
    qkv_seq = qkv.clone()
    outs = {k: torch.empty(B, hq * D, dtype=torch.bfloat16, device=DEV)
            for k in ("unshared", "shared")}
    scale = D ** -0.5
    S = engine_splits(B)
    PS = prefix_splits or engine_prefix_splits(B, hq)
    tmp_out = torch.zeros(B, hq, S + PS, D, dtype=torch.float32, device=DEV)
    tmp_ml = torch.zeros(B, hq, S + PS, 2, dtype=torch.float32, device=DEV)
    tiles_h = torch.zeros(max(1, B // 2), 2 + 16, dtype=torch.int32)
    for t, r0 in enumerate(range(0, B, W)):
        rows = list(range(r0, min(B, r0 + W)))
        tiles_h[t, :2 + len(rows)] = torch.tensor([len(rows), P] + rows,
                                                  dtype=torch.int32)
    ops.check_prefix_tiles(tiles_h, G)
    tiles = tiles_h.to(DEV)
    prefix_blocks = torch.full((B,), P, dtype=torch.int32, device=DEV)

    def unshared(i):
        o = outs["unshared"]
        if fp8:
            ops.rope_kv_append(qkv_seq, kcs[i], vcs[i], cos_sin, pos, slots,
                               hq, Hk, D, block_table=bt)
            ops.paged_attention(o, qkv_seq, kcs[i], vcs[i], bt, seq_lens, 0,
                                S, scale, tmp_out, tmp_ml)
        else:
            ops.paged_attention_rope(o, qkv, kcs[i], vcs[i], cos_sin, pos,
                                     bt, seq_lens, hq, Hk, S, scale, tmp_out,
                                     tmp_ml)

    def shared(i):
        o = outs["shared"]
        if fp8:
            ops.rope_kv_append(qkv_seq, kcs[i], vcs[i], cos_sin, pos, slots,
                               hq, Hk, D, block_table=bt)
            ops.paged_attention_shared(o, qkv_seq, kcs[i], vcs[i], bt,
                                       seq_lens, 0, S, scale, tmp_out,
                                       tmp_ml, prefix_blocks, tiles, PS)
        else:
            ops.paged_attention_rope_shared(
                o, qkv, kcs[i], vcs[i], cos_sin, pos, bt, seq_lens, hq, Hk,
                S, scale, tmp_out, tmp_ml, prefix_blocks, tiles, PS)

    graphs = {"unshared": make_graph(unshared, copies),
              "shared": make_graph(shared, copies)}
    # same inputs, same answer up to summation order (bf16; the fp8
    # sequences rotate qkv_seq in place call after call, so only the
    # fused pair is comparable here)
    max_diff = None
    if not fp8:
        max_diff = float((outs["shared"].float() -
                          outs["unshared"].float()).abs().max())
    reps = max(2, 200 // copies)
    times = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():     # alternating
            times[k].append(time_graph(g, copies, reps))
    res = {"mode": "shared-prefix", "B": B, "Hq": hq, "Hk": Hk,
           "prefix": prefix, "suffix": [64, 384],
           "kv": "fp8" if fp8 else "bf16", "splits": S, "prefix_splits": PS,
           "tiles": -(-B // W), "kv_mb_unshared": round(kv_bytes / 1e6, 1),
           "kv_mb_distinct": round(distinct / 1e6, 1), "copies": copies,
           "max_abs_diff": max_diff}
    for k, ts in times.items():
        res[k + "_us"] = round(statistics.median(ts), 2)
        res[k + "_spread_us"] = round(max(ts) - min(ts), 2)
    res["unshared_over_shared"] = round(res["unshared_us"] /
                                        res["shared_us"], 3)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kv-dtype", default="bf16", choices=("bf16", "fp8"))
    ap.add_argument("--batches", default="64,8,16,32,128,256")
    ap.add_argument("--shared-prefix", action="store_true",
                    help="forked sessions: ops.paged_attention_rope_shared "
                         "against the unshared op at B = 64, prefix 512 / "
                         "1024 / 3072, GQA group 4 and 8")
    ap.add_argument("--prefixes", default="512,1024,3072")
    ap.add_argument("--prefix-splits", type=int, default=None,
                    help="override the engine's rule (--shared-prefix)")
    args = ap.parse_args()
    fp8 = args.kv_dtype == "fp8"
    if args.shared_prefix:
        for hq in (32, 64):
            for prefix in (int(p) for p in args.prefixes.split(",")):
                bench_shared(64, prefix, fp8, hq, args.prefix_splits)
        return
    for B in (int(b) for b in args.batches.split(",")):
        # the serving mix, and at the headline batch also uniform contexts
        shapes = [(512, 3584)]
        if B == 64:
            shapes += [(1500, 1500), (3584, 3584)]
        for lo, hi in shapes:
            bench_shape(B, lo, hi, fp8)


if __name__ == "__main__":
    main()
