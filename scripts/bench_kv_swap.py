"""The host KV tier against today's eviction: what an idle session's next
turn costs after the engine took its KV away, and the pack / unpack
kernels alone.

Workload: one session prefills `--context-len` tokens and goes idle, the
engine evicts it (LLMEngine._evict_idle_kv, called directly: it is the only
idle session), and a follow-up turn of `--followup-len` tokens is submitted.
Mode "swap" runs the engine with its host tier (kv_host_blocks > 0): the
eviction copies the blocks to pinned host memory and the follow-up copies
them back and prefills only its new tokens. Mode "drop" runs the same
engine with the tier detached, which takes the code paths of the engine
with kv_host_blocks=0 (it is not a build without the feature, and the
pinned pool and staging buffer stay allocated meanwhile): the eviction
drops the blocks and the follow-up prefills the whole history
again. Both modes run in one process, alternating, after one untimed round
of each.

Per round: seconds the eviction took, seconds from submitting the follow-up
to its first token (both from a host clock around work that ends in a
device synchronise), and in mode swap one more swap-out and swap-in of the
idle session, timed alone, with the link rate their bytes imply. Then the
kernels alone: device events around batches of kv_pack_blocks and
kv_unpack_blocks calls on a full staging buffer. --pin-gib G also times the
allocation of a pinned host pool of G GiB (a cold start pays that once).
Prints one JSON line.

    python scripts/bench_kv_swap.py               # 8B bf16, 3584 tokens
    python scripts/bench_kv_swap.py --model tiny-llama --device cpu \
        --context-len 40 --followup-len 3 --kv-blocks 64 --host-blocks 16 \
        --staging-blocks 2    # host-logic rehearsal, times mean nothing
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kukeon_amd import ops  # noqa: E402
from kukeon_amd.engine.config import (EngineConfig, MODEL_PRESETS,  # noqa: E402
                                      SamplingParams)
from kukeon_amd.engine.engine import LLMEngine  # noqa: E402
from kukeon_amd.engine.kv_cache import SequenceKV  # noqa: E402
from kukeon_amd.models.llama import LlamaModel  # noqa: E402


def spread(xs):
    return {"median": round(statistics.median(xs), 5),
            "min": round(min(xs), 5), "max": round(max(xs), 5), "n": len(xs)}


def run_round(engine, tier, mode, context, followup, sync):
    engine.host_kv = tier if mode == "swap" else None
    alloc = engine.kv.allocator
    kv = SequenceKV(engine.ecfg.block_size)
    sp = SamplingParams(temperature=0.7, top_k=50, top_p=0.9,
                        max_new_tokens=2)
    engine.add_request(kv, context, sp)
    while engine.has_work():
        engine.step()
    held = len(kv.blocks)
    sync()
    t0 = time.perf_counter()
    assert engine._evict_idle_kv()
    sync()
    evict_s = time.perf_counter() - t0
    assert alloc.num_free == alloc.num_blocks
    assert bool(kv.host_blocks) == (mode == "swap")
    moved = len(kv.host_blocks)
    t0 = time.perf_counter()
    rid = engine.add_request(kv, followup, sp)
    first = None
    while engine.has_work():
        for o in engine.step():
            if first is None and o.req_id == rid and o.new_tokens:
                sync()
                first = time.perf_counter() - t0
    out = {"evict_s": evict_s, "first_token_s": first, "blocks_held": held,
           "blocks_to_host": moved}
    if mode == "swap":
        # the same session once more, the two copies timed alone
        sync()
        t0 = time.perf_counter()
        assert engine._swap_out(kv)
        sync()
        out["swap_out_s"] = time.perf_counter() - t0
        n = len(kv.host_blocks)
        t0 = time.perf_counter()
        engine._swap_in(kv)
        sync()
        out["swap_in_s"] = time.perf_counter() - t0
        out["swap_bytes"] = n * tier.record_bytes
    engine.free_sequence(kv)
    assert alloc.num_free == alloc.num_blocks
    assert tier.allocator.num_free == tier.allocator.num_blocks
    return out


def bench_kernels(engine, tier, batches=5, calls=20):
    """Device-event time of one kv_pack_blocks / kv_unpack_blocks call that
    fills the staging buffer, on the engine's cache."""
    k, v = engine.kv.k, engine.kv.v
    n = tier.staging_blocks
    nb = k.shape[1]
    assert nb >= 2 * n
    # scattered sources, as a session's block list is after some churn
    ids = random.Random(7).sample(range(nb), n)
    blocks = torch.tensor(ids, dtype=torch.int32, device=k.device)

    def pack():
        ops.kv_pack_blocks(k, v, blocks, tier.staging)

    def unpack():
        ops.kv_unpack_blocks(tier.staging, k, v, blocks)

    out = {"blocks_per_call": n, "bytes_per_call": n * tier.record_bytes}
    for name, fn in (("kv_pack_blocks", pack), ("kv_unpack_blocks", unpack)):
        for _ in range(3):
            fn()
        per_call = []
        for _ in range(batches):
            a = torch.cuda.Event(enable_timing=True)
            b = torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            per_call.append(a.elapsed_time(b) * 1000 / calls)
        out[name + "_us"] = spread(per_call)
        # bytes copied (each is read once and written once) per second
        out[name + "_gb_per_s"] = round(
            n * tier.record_bytes / (statistics.median(per_call) * 1e-6) / 1e9,
            1)
    return out


def main():
    ap = argparse.ArgumentParser("bench_kv_swap")
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--context-len", type=int, default=3584)
    ap.add_argument("--followup-len", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kv-blocks", type=int, default=2048)
    ap.add_argument("--host-blocks", type=int, default=512)
    ap.add_argument("--staging-blocks", type=int, default=64)
    ap.add_argument("--kv-dtype", choices=["bf16", "fp8"], default="bf16")
    ap.add_argument("--pin-gib", type=float, default=0.0,
                    help="also time allocating a pinned host pool this large")
    args = ap.parse_args()
    on_gpu = args.device != "cpu"
    if on_gpu and not torch.cuda.is_available():
        sys.exit("bench_kv_swap: no GPU; nothing here may be reported as "
                 "measured (use --device cpu only to rehearse host logic)")

    cfg = MODEL_PRESETS[args.model]()
    ecfg = EngineConfig(max_model_len=max(4096, args.context_len + 256),
                        max_sessions=8, num_kv_blocks=args.kv_blocks,
                        use_graphs=False, kv_dtype=args.kv_dtype,
                        kv_host_blocks=args.host_blocks,
                        kv_swap_staging_blocks=args.staging_blocks)
    torch.manual_seed(0)
    model = LlamaModel(cfg, device=args.device)

    def sync():
        if on_gpu:
            torch.cuda.synchronize()

    sync()
    t0 = time.perf_counter()
    engine = LLMEngine(model, cfg, ecfg, device=args.device)
    sync()
    init_s = time.perf_counter() - t0
    tier = engine.host_kv

    rng = random.Random(1234)
    context = [rng.randrange(cfg.vocab_size) for _ in range(args.context_len)]
    followup = [rng.randrange(cfg.vocab_size)
                for _ in range(args.followup_len)]
    modes = ("swap", "drop")
    for m in modes:                      # warm every shape the modes use
        run_round(engine, tier, m, context, followup, sync)
    rounds = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            rounds[m].append(run_round(engine, tier, m, context, followup,
                                       sync))
    engine.host_kv = tier
    out = {"device": (torch.cuda.get_device_name(0) if on_gpu else "cpu"),
           "model": args.model, "context_len": args.context_len,
           "followup_len": args.followup_len, "kv_dtype": args.kv_dtype,
           "host_blocks": args.host_blocks,
           "staging_blocks": tier.staging_blocks,
           "record_bytes": tier.record_bytes,
           "host_pool_pinned": tier.pool.is_pinned(),
           "engine_init_s": round(init_s, 3)}
    for m in modes:
        rs = rounds[m]
        out[m] = {"evict_s": spread([r["evict_s"] for r in rs]),
                  "first_token_s": spread([r["first_token_s"] for r in rs]),
                  "blocks_held": sorted({r["blocks_held"] for r in rs}),
                  "blocks_to_host": sorted({r["blocks_to_host"] for r in rs})}
    rs = rounds["swap"]
    nbytes = rs[0]["swap_bytes"]
    for key in ("swap_out_s", "swap_in_s"):
        xs = [r[key] for r in rs]
        out["swap"][key] = spread(xs)
        out["swap"][key[:-2] + "_gb_per_s"] = round(
            nbytes / statistics.median(xs) / 1e9, 2)
    out["swap"]["swap_bytes"] = nbytes
    out["first_token_drop_over_swap"] = round(
        out["drop"]["first_token_s"]["median"] /
        out["swap"]["first_token_s"]["median"], 2)
    out["kernels"] = (bench_kernels(engine, tier) if on_gpu
                      else "not measured (no GPU)")
    if args.pin_gib > 0 and on_gpu:
        n = int(args.pin_gib * (1 << 30))
        t0 = time.perf_counter()
        big = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        out["pin"] = {"gib": args.pin_gib,
                      "alloc_s": round(time.perf_counter() - t0, 3)}
        del big
    else:
        out["pin"] = "not measured"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
