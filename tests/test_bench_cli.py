"""bench.py command-line contract on the CPU path: --steps sets the number
of timed steps, the result line carries ms_per_step, and --dump-outputs
writes the last step's tokens reproducibly."""
import json
import runpy
import sys
from pathlib import Path

import numpy as np

from kukeon_amd.serve.sessions import TurnDriver

BENCH = Path(__file__).resolve().parent.parent / "bench.py"
SESSIONS, DECODE = 3, 5
ARGS = ["--gpus", "1", "--device", "cpu", "--model", "tiny-llama",
        "--sessions", str(SESSIONS), "--prompt-len", "8",
        "--followup-len", "4", "--decode-len", str(DECODE),
        "--ctx-cap", "64", "--max-model-len", "128"]


def run_bench(monkeypatch, capsys, extra):
    rounds = []
    orig = TurnDriver.run_round

    def counted(self):
        rounds.append(1)
        return orig(self)
    monkeypatch.setattr(TurnDriver, "run_round", counted)
    monkeypatch.setattr(sys, "argv", [str(BENCH)] + ARGS + extra)
    runpy.run_path(str(BENCH), run_name="__main__")
    lines = [ln for ln in capsys.readouterr().out.splitlines()
             if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), len(rounds)


def test_bench_steps_and_dump_outputs(monkeypatch, capsys, tmp_path):
    dumps = []
    for tag in ("a", "b"):
        d = tmp_path / tag
        res, rounds = run_bench(monkeypatch, capsys,
                                ["--steps", "2", "--warmup", "1",
                                 "--dump-outputs", str(d)])
        assert rounds == 3                      # 1 warmup + 2 timed
        assert res["steps"] == 2 and res["warmup"] == 1
        assert res["metric"] == "agent_turns_per_sec"
        assert res["unit"] == "turns/s" and res["higher_is_better"] is True
        assert res["dtype"] == "bf16"
        assert res["ms_per_step"] > 0
        # value and ms_per_step describe the same timed interval
        assert abs(res["value"] * res["ms_per_step"] / 1000 - SESSIONS) \
            < 0.05 * SESSIONS
        assert [p.name for p in d.iterdir()] == ["tokens.npy"]
        toks = np.load(d / "tokens.npy")
        assert toks.dtype == np.float32
        assert toks.shape == (SESSIONS, DECODE)
        assert (toks >= 0).all() and (toks < 512).all()
        assert (toks == np.round(toks)).all()
        dumps.append(toks)
    assert np.array_equal(dumps[0], dumps[1])


def test_bench_plain_and_full_write_nothing(monkeypatch, capsys, tmp_path):
    monkeypatch.chdir(tmp_path)
    for extra in ([], ["--full"]):
        res, rounds = run_bench(monkeypatch, capsys,
                                ["--steps", "1", "--warmup", "0"] + extra)
        assert rounds == 1 and res["steps"] == 1
        assert res["ms_per_step"] > 0
    assert list(tmp_path.iterdir()) == []
