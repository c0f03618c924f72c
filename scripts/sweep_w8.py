"""W8A16 skinny decode GEMM vs the bf16 route on the Llama decode shapes.

For each of the five Llama-3-8B decode GEMMs and the 70B o / down shapes,
at M = 16 and 64, times two routes in the same process, alternating them
per round, with device events around a batch of calls and a median over
rounds:

  * w8:   ops.linear(x, Fp8Weight)  (the W8A16 kernel + its reduce pass),
  * bf16: ops.linear(x, w) on the bf16 weight of the same shape (whatever
          the dispatch picks: a skinny kernel or hipBLASLt).

Cold-LLC convention of scripts/sweep_cold.py: every call streams the next
of enough weight copies to overflow the 256 MB LLC twice, so no weight is
ever re-read from cache. Weight bytes per second are computed from the
shapes (N*K for fp8 plus 4N of scales, 2*N*K for bf16). Prints one JSON
line per (shape, M); the fp8 table in docs/perf.md comes from this script.

    python scripts/sweep_w8.py [--out FILE] [--rounds 7] [--only qkv,o]
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
        raise SystemExit("sweep_w8: needs the GPU")
    if not ops.native_available():
        raise SystemExit("sweep_w8: the HIP extension is not built")
    dev = torch.device("cuda:0")
    only = set(filter(None, args.only.split(",")))
    lines = []
    for (N, K, tag) in SHAPES:
        if only and tag not in only:
            continue
        b16 = N * K * 2
        b8 = N * K + 4 * N
        # enough copies of EACH format to overflow the LLC twice
        n16 = max(2, -(-2 * LLC // b16))
        n8 = max(2, -(-2 * LLC // b8))
        torch.manual_seed(13)
        w16 = [torch.randn(N, K, dtype=torch.bfloat16, device=dev) * 0.05
               for _ in range(n16)]
        w8 = [ops.quantize_weight(w16[i % n16] if i < n16 else
                                  torch.randn(N, K, dtype=torch.bfloat16,
                                              device=dev) * 0.05)
              for i in range(n8)]
        iters = max(n8, 20)
        for M in (16, 64):
            x = torch.randn(M, K, dtype=torch.bfloat16, device=dev) * 0.3

            def run8(i):
                ops.linear(x, w8[i % n8])

            def run16(i):
                ops.linear(x, w16[i % n16])

            kind16 = ops._skinny_kind(x, w16[0], fused=False) or "blas"
            for fn in (run8, run16):
                for i in range(3):
                    fn(i)
            t8, t16 = [], []
            for _ in range(args.rounds):
                t8.append(timed(run8, iters))
                t16.append(timed(run16, iters))
            m8, m16 = statistics.median(t8), statistics.median(t16)
            rec = {
                "shape": tag, "N": N, "K": K, "M": M, "iters": iters,
                "rounds": args.rounds, "copies": [n8, n16],
                "w8_us": round(m8, 1), "bf16_us": round(m16, 1),
                "bf16_route": kind16,
                "w8_us_minmax": [round(min(t8), 1), round(max(t8), 1)],
                "bf16_us_minmax": [round(min(t16), 1), round(max(t16), 1)],
                "bf16_over_w8": round(m16 / m8, 3),
                "w8_weight_TBps": round(b8 / (m8 * 1e-6) / 1e12, 3),
                "bf16_weight_TBps": round(b16 / (m16 * 1e-6) / 1e12, 3),
                "w8_splitk": ops._native().skinny_splitk("w8", N, K),
            }
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
        del w16, w8
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
