"""Session fork against per-session prefill of a shared prefix, and the
tail-block copy kernel against torch indexing.

Workload: `--sessions` sessions share a `--prefix-len` prompt, each adds a
`--suffix-len` prompt of its own and decodes `--decode-len` tokens. Mode
"fork" prefills the prefix once into a template session (prefill-only) and
forks the sessions from it; mode "prefill" (the behaviour without fork) has
every session prefill prefix + suffix itself. Both modes run in one
process, alternating, after one untimed round of each.

Per round: seconds until every session has its first token, seconds for
the whole round (both from a host clock around work that ends in a device
synchronise), their difference (the decode part), and the KV blocks in use
when the last prefill finished. --shared-prefix-min-tokens N adds mode
"fork_shared": fork with decode attention reading the shared prefix once
per tile of sessions (EngineConfig.shared_prefix_min_tokens = N), in the
same process and alternating with the others.
Prints one JSON line.

    python scripts/bench_fork.py                  # 8B, 3072 + 256 + 128
    python scripts/bench_fork.py --model tiny-llama --device cpu \
        --prefix-len 40 --suffix-len 9 --decode-len 4 --sessions 3 \
        --kv-blocks 64          # host-logic rehearsal, times mean nothing
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
    return {"median": round(statistics.median(xs), 4),
            "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def run_round(engine, mode, prefix, suffixes, decode_len, sync,
              shared_min_tokens=0):
    alloc = engine.kv.allocator
    bs = engine.ecfg.block_size
    sp = SamplingParams(temperature=0.7, top_k=50, top_p=0.9,
                        max_new_tokens=decode_len)
    n = len(suffixes)
    sync()
    t0 = time.perf_counter()
    # "fork_shared" is "fork" with the shared-prefix decode path on
    engine.ecfg.shared_prefix_min_tokens = (
        shared_min_tokens if mode == "fork_shared" else 0)
    steps0 = engine.shared_prefix_steps
    if mode in ("fork", "fork_shared"):
        template = SequenceKV(bs)
        engine.add_request(template, prefix,
                           SamplingParams(max_new_tokens=0))
        while engine.has_work():
            engine.step()
        kvs = engine.fork_sequence(template, n)
        work = list(zip(kvs, suffixes))
        owners = [template] + kvs
    else:
        owners = kvs = [SequenceKV(bs) for _ in range(n)]
        work = [(kv, prefix + s) for kv, s in zip(kvs, suffixes)]
    rids = {engine.add_request(kv, p, sp) for kv, p in work}
    first = set()
    t_first = used = None
    while engine.has_work():
        for o in engine.step():
            if o.new_tokens:
                first.add(o.req_id)
        if t_first is None and first == rids:
            sync()
            t_first = time.perf_counter() - t0
            used = alloc.num_blocks - alloc.num_free
    sync()
    total = time.perf_counter() - t0
    shared = alloc.num_shared
    for kv in owners:
        engine.free_sequence(kv)
    assert alloc.num_free == alloc.num_blocks and alloc.num_shared == 0
    return {"first_token_s": t_first, "round_s": total,
            "decode_s": total - t_first,
            "shared_prefix_steps": engine.shared_prefix_steps - steps0,
            "blocks_used_after_prefill": used, "blocks_shared": shared}


def bench_copy(engine, n_dst, batches=5, calls=20):
    """Device-event time of one kv_copy_blocks call for n_dst destinations
    on the engine's cache, against the torch indexing that does the same."""
    k, v = engine.kv.k, engine.kv.v
    nb = k.shape[1]
    assert nb > 2 * n_dst + 1
    dev = k.device
    src = torch.full((n_dst,), 0, dtype=torch.int32, device=dev)
    dst = torch.arange(nb - n_dst, nb, dtype=torch.int32, device=dev)
    src_l, dst_l = src.long(), dst.long()

    def hip():
        ops.kv_copy_blocks(k, v, src, dst)

    def indexing():
        k[:, dst_l] = k[:, src_l]
        v[:, dst_l] = v[:, src_l]

    out = {}
    for name, fn in (("kv_copy_blocks", hip), ("torch_indexing", indexing)):
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
    moved = 2 * k.shape[0] * n_dst * k[0, 0].numel() * k.element_size()
    out["bytes_written_per_call"] = moved
    return out


def main():
    ap = argparse.ArgumentParser("bench_fork")
    ap.add_argument("--model", default="llama-3-8b")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--sessions", type=int, default=64)
    ap.add_argument("--prefix-len", type=int, default=3072)
    ap.add_argument("--suffix-len", type=int, default=256)
    ap.add_argument("--decode-len", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kv-blocks", type=int, default=20000)
    ap.add_argument("--kv-dtype", choices=["bf16", "fp8"], default="bf16")
    ap.add_argument("--no-graphs", action="store_true")
    ap.add_argument("--shared-prefix-min-tokens", type=int, default=0,
                    help="also run mode fork_shared: fork with "
                         "EngineConfig.shared_prefix_min_tokens set to this, "
                         "alternating with the other modes")
    args = ap.parse_args()
    on_gpu = args.device != "cpu"
    if on_gpu and not torch.cuda.is_available():
        sys.exit("bench_fork: no GPU; nothing here may be reported as "
                 "measured (use --device cpu only to rehearse host logic)")

    cfg = MODEL_PRESETS[args.model]()
    total = args.prefix_len + args.suffix_len + args.decode_len
    ecfg = EngineConfig(max_model_len=max(4096, total),
                        max_sessions=max(args.sessions, 8),
                        num_kv_blocks=args.kv_blocks,
                        use_graphs=on_gpu and not args.no_graphs,
                        decode_microbatch=64, kv_dtype=args.kv_dtype)
    torch.manual_seed(0)
    engine = LLMEngine(LlamaModel(cfg, device=args.device), cfg, ecfg,
                       device=args.device)
    engine.capture_all()

    def sync():
        if on_gpu:
            torch.cuda.synchronize()

    rng = random.Random(1234)
    prefix = [rng.randrange(cfg.vocab_size) for _ in range(args.prefix_len)]
    suffixes = [[rng.randrange(cfg.vocab_size)
                 for _ in range(args.suffix_len)]
                for _ in range(args.sessions)]
    modes = ("fork", "prefill")
    if args.shared_prefix_min_tokens > 0:
        modes = ("fork", "fork_shared", "prefill")
    for m in modes:                      # warm every shape the modes use
        run_round(engine, m, prefix, suffixes, args.decode_len, sync,
                  args.shared_prefix_min_tokens)
    rounds = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            rounds[m].append(run_round(engine, m, prefix, suffixes,
                                       args.decode_len, sync,
                                       args.shared_prefix_min_tokens))
    out = {"device": (torch.cuda.get_device_name(0) if on_gpu else "cpu"),
           "model": args.model, "sessions": args.sessions,
           "prefix_len": args.prefix_len, "suffix_len": args.suffix_len,
           "decode_len": args.decode_len, "kv_dtype": args.kv_dtype,
           "kv_blocks_total": engine.kv.num_blocks}
    for m in modes:
        rs = rounds[m]
        out[m] = {
            "first_token_s": spread([r["first_token_s"] for r in rs]),
            "round_s": spread([r["round_s"] for r in rs]),
            "decode_s": spread([r["decode_s"] for r in rs]),
            "shared_prefix_steps":
                sorted({r["shared_prefix_steps"] for r in rs}),
            "blocks_used_after_prefill":
                sorted({r["blocks_used_after_prefill"] for r in rs}),
            "blocks_shared": sorted({r["blocks_shared"] for r in rs}),
        }
    bs = ecfg.block_size
    out["blocks_saved_expected"] = (args.sessions - 1) * (args.prefix_len
                                                          // bs)
    out["blocks_saved_measured"] = (
        out["prefill"]["blocks_used_after_prefill"][-1] -
        out["fork"]["blocks_used_after_prefill"][-1])
    out["copy"] = (bench_copy(engine, args.sessions) if on_gpu
                   else "not measured (no GPU)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
