"""Grouped-GEMM MoE route vs the per-expert hipBLASLt loop on one
Mixtral-8x7B MoE layer (E=8, K=2, H=4096, I=14336, TP=1).

Times MixtralMoE._forward_grouped against _forward_sparse in the same
process, alternating the two per round, with device events around a batch
of calls; also times the two grouped-GEMM launches alone and reports the
weight-streaming rate they reach (all 2.8 GB of expert weights over the
summed GEMM time). Prints one JSON line per T; the table in docs/perf.md
and the default of KUKEON_MOE_GROUPED_MAX_T come from this script.

    python scripts/sweep_moe_grouped.py [--out FILE] [--ts 192,256,...]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kukeon_amd import ops  # noqa: E402
from kukeon_amd.engine.config import mixtral_8x7b  # noqa: E402
from kukeon_amd.models.mixtral import MixtralMoE  # noqa: E402


def timed(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--ts", default="192,256,512,1024,2048,4096")
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the sweep needs the GPU"
    dev = "cuda:0"
    torch.manual_seed(0)
    cfg = mixtral_8x7b()
    moe = MixtralMoE(cfg, dev)
    wbytes = (moe.gate_up_w.numel() + moe.down_w.numel()) * 2
    lines = []
    for T in [int(t) for t in args.ts.split(",")]:
        x = torch.randn(T, cfg.hidden_size, dtype=torch.bfloat16, device=dev)
        g = moe._forward_grouped(x)
        s = moe._forward_sparse(x)
        torch.cuda.synchronize()
        err = (g.float() - s.float()).abs().max().item()
        scale = s.float().abs().max().item()

        # the two grouped-GEMM launches alone, on this T's real routing
        logits = torch.nn.functional.linear(x, moe.router_w)
        topk_w = torch.empty(T, moe.K, dtype=torch.float32, device=dev)
        row_map = torch.empty(T * moe.K, dtype=torch.int32, device=dev)
        inv_map = torch.empty(T, moe.K, dtype=torch.int32, device=dev)
        offsets = torch.empty(moe.E + 1, dtype=torch.int32, device=dev)
        ops.moe_route_sort(topk_w, row_map, inv_map, offsets, logits, moe.K)
        gu = torch.empty(T * moe.K, 2 * moe.inter, dtype=x.dtype, device=dev)
        act = torch.empty(T * moe.K, moe.inter, dtype=x.dtype, device=dev)
        y = torch.empty(T * moe.K, cfg.hidden_size, dtype=x.dtype, device=dev)
        ops.silu_mul(act, gu)

        def gemm_up():
            ops.moe_grouped_gemm(gu, x, row_map, moe.gate_up_w, offsets)

        def gemm_down():
            ops.moe_grouped_gemm(y, act, None, moe.down_w, offsets)

        iters = max(3, min(20, 4096 // T))
        for fn in (gemm_up, gemm_down):
            fn()
        tg, ts_, tu, td = [], [], [], []
        for _ in range(args.rounds):
            tg.append(timed(lambda: moe._forward_grouped(x), iters))
            ts_.append(timed(lambda: moe._forward_sparse(x), iters))
            tu.append(timed(gemm_up, iters))
            td.append(timed(gemm_down, iters))
        med = statistics.median
        rec = {
            "T": T, "iters": iters, "rounds": args.rounds,
            "grouped_us": round(med(tg), 1), "sparse_us": round(med(ts_), 1),
            "grouped_us_minmax": [round(min(tg), 1), round(max(tg), 1)],
            "sparse_us_minmax": [round(min(ts_), 1), round(max(ts_), 1)],
            "gemm_gate_up_us": round(med(tu), 1),
            "gemm_down_us": round(med(td), 1),
            "gemm_weight_TBps": round(
                wbytes / ((med(tu) + med(td)) * 1e-6) / 1e12, 3),
            "layer_weight_TBps": round(wbytes / (med(tg) * 1e-6) / 1e12, 3),
            "max_abs_diff_vs_sparse": err, "max_abs_sparse": scale,
        }
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
