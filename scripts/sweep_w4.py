"""W4A16 skinny decode GEMM vs the W8A16 and bf16 routes on the Llama
decode shapes.

The method of scripts/sweep_w8.py with a third route: for each of the five
Llama-3-8B decode GEMMs and the 70B o / down shapes, at M = 16 and 64,
times three routes in the same process, alternating them per round, with
device events around a batch of calls and a median and spread over rounds:

  * w4:   ops.linear(x, Mxfp4Weight)  (the W4A16 kernel + its reduce pass),
  * w8:   ops.linear(x, Fp8Weight)    (the W8A16 kernel + its reduce pass),
  * bf16: ops.linear(x, w) on the bf16 weight of the same shape (whatever
          the dispatch picks: a skinny kernel or hipBLASLt).

Cold-LLC convention of scripts/sweep_cold.py: every call streams the next
of enough weight copies to overflow the 256 MB LLC twice, so no weight is
ever re-read from cache. Weight bytes per second come from the true byte
counts (N*K/2 + N*K/32 for mxfp4, N*K + 4N for fp8, 2*N*K for bf16).
Prints one JSON line per (shape, M); the MXFP4 table in docs/perf.md comes
from this script.

    python scripts/sweep_w4.py [--out FILE] [--rounds 7] [--only qkv,o]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from kukeon_amd import ops  # noqa: E402

LLC = 256 * (1 << 20)

SHAPES = [(6144, 4096, "qkv"), (4096, 4096, "o"), (28672, 4096, "gate_up"),
          (4096, 14336, "down"), (128256, 4096, "lm_head"),
          (8192, 8192, "70b-o"), (8192, 28672, "70b-down")]


def timed(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(i)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / iters   # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sweep_w4: needs the GPU")
    if not ops.native_available():
        raise SystemExit("sweep_w4: the HIP extension is not built")
    dev = torch.device("cuda:0")
    only = set(filter(None, args.only.split(",")))
    lines = []
    for (N, K, tag) in SHAPES:
        if only and tag not in only:
            continue
        nbytes = {"w4": N * K // 2 + N * K // 32, "w8": N * K + 4 * N,
                  "bf16": N * K * 2}
        # enough copies of EACH format to overflow the LLC twice
        ncopies = {r: max(2, -(-2 * LLC // b)) for r, b in nbytes.items()}
        torch.manual_seed(13)

        def fresh():
            return torch.randn(N, K, dtype=torch.bfloat16, device=dev) * 0.05

        w16 = [fresh() for _ in range(ncopies["bf16"])]

        def source(i):
            return w16[i] if i < len(w16) else fresh()

        weights = {
            "bf16": w16,
            "w8": [ops.quantize_weight(source(i))
                   for i in range(ncopies["w8"])],
            "w4": [ops.quantize_weight(source(i), fmt="mxfp4")
                   for i in range(ncopies["w4"])],
        }
        iters = max(ncopies["w4"], 20)
        for M in (16, 64):
            x = torch.randn(M, K, dtype=torch.bfloat16, device=dev) * 0.3

            def runner(route):
                ws, n = weights[route], ncopies[route]
                return lambda i: ops.linear(x, ws[i % n])

            runs = {r: runner(r) for r in ("w4", "w8", "bf16")}
            kind16 = ops._skinny_kind(x, w16[0], fused=False) or "blas"
            for fn in runs.values():
                for i in range(3):
                    fn(i)
            t = {r: [] for r in runs}
            for _ in range(args.rounds):
                for r, fn in runs.items():
                    t[r].append(timed(fn, iters))
            med = {r: statistics.median(v) for r, v in t.items()}
            rec = {"shape": tag, "N": N, "K": K, "M": M, "iters": iters,
                   "rounds": args.rounds,
                   "copies": [ncopies[r] for r in runs],
                   "bf16_route": kind16}
            for r in runs:
                rec[f"{r}_us"] = round(med[r], 1)
                rec[f"{r}_us_minmax"] = [round(min(t[r]), 1),
                                         round(max(t[r]), 1)]
                rec[f"{r}_weight_TBps"] = round(
                    nbytes[r] / (med[r] * 1e-6) / 1e12, 3)
            rec["w8_over_w4"] = round(med["w8"] / med["w4"], 3)
            rec["bf16_over_w4"] = round(med["bf16"] / med["w4"], 3)
            rec["w4_splitk"] = ops._native().skinny_splitk("w4", N, K)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
        del w16, weights, runs
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
