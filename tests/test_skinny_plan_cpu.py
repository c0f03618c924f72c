"""The skinny-GEMM split-K plan, host side only: `_C.skinny_splitk` is the
plan function the launchers themselves call, and the Python dispatch sizes
its workspace from it. Expected values are worked out by hand from the
launcher formulas: ngroups = N / cols, nslices = ceil(K / slice),
splitk = min(nslices, ceil(256 / ngroups)), 1 once ngroups reaches the
variant's chip-fill count, a positive override clamped to nslices."""
import pytest
import torch

import kukeon_amd.ops as ops

if not ops.native_available():
    pytest.skip("HIP extension not built", allow_module_level=True)

_ENVS = ("KUKEON_SKINNY_SPLITK", "KUKEON_SK2_SPLITK", "KUKEON_SK5_SPLITK",
         "KUKEON_SK6_SPLITK", "KUKEON_SK5_KS", "KUKEON_SK6_KS",
         "KUKEON_SK5_NSPLIT")


@pytest.mark.parametrize("kind,N,K,env,splitk", [
    ("v1", 4096, 4096, {}, 4),           # 64 tiles, 16 slices
    ("v1", 6144, 4096, {}, 3),           # 96 tiles -> ceil(256/96)
    ("v1", 28672, 4096, {}, 1),          # 448 tiles -> ceil(256/448)
    ("v2", 6144, 4096, {}, 6),           # 48 groups of 128
    ("v2", 6144, 4096, {"KUKEON_SK2_SPLITK": "5"}, 5),
    ("v5", 4096, 14336, {}, 4),          # 64 groups, 112 slices of 128
    ("v5", 8192, 28672, {}, 2),
    ("v5", 128256, 4096, {}, 1),         # 2004 groups: split-K off
    ("v5", 4096, 14336, {"KUKEON_SK5_SPLITK": "8"}, 8),
    ("v5", 4096, 14336, {"KUKEON_SK5_SPLITK": "1000"}, 112),
    ("v5", 4096, 14336, {"KUKEON_SK5_KS": "256"}, 4),
    ("v5", 4096, 14336, {"KUKEON_SK5_NSPLIT": "2"}, 8),   # 32 groups
    # the fused launchers ignore KS: nslices stays 112, not 56
    ("v5_fused", 4096, 14336, {"KUKEON_SK5_KS": "256"}, 4),
    ("v5_fused", 4096, 14336,
     {"KUKEON_SK5_KS": "256", "KUKEON_SK5_SPLITK": "1000"}, 112),
    ("v5", 4096, 14336,
     {"KUKEON_SK5_KS": "256", "KUKEON_SK5_SPLITK": "1000"}, 56),
    ("v6", 4096, 14336, {}, 8),          # 32 groups of 128
])
def test_skinny_splitk(kind, N, K, env, splitk, monkeypatch):
    from kukeon_amd import _C
    for name in _ENVS:
        monkeypatch.delenv(name, raising=False)
    for name, val in env.items():
        monkeypatch.setenv(name, val)
    assert _C.skinny_splitk(kind, N, K) == splitk


def test_skinny_splitk_unknown_kind():
    from kukeon_amd import _C
    with pytest.raises(RuntimeError):
        _C.skinny_splitk("v4", 4096, 4096)


def test_skinny_workspace_sized_by_plan(monkeypatch):
    for name in _ENVS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(ops, "_SKINNY_WS", {})
    monkeypatch.setattr(ops, "_SKINNY_WS_RETIRED", [])
    monkeypatch.setattr(ops, "_SKINNY_SPLITK", {})
    dev = torch.device("cpu")
    ws = ops._skinny_workspace(dev, "v5", 4096, 14336)
    assert ws.dtype == torch.float32 and ws.numel() == 64 * 4096 * 4
    # grow-only: a smaller request reuses the buffer, a larger one
    # replaces it and pins the old one
    assert ops._skinny_workspace(dev, "v1", 4096, 4096) is ws
    assert ops._skinny_workspace(dev, "v5", 8192, 28672) is ws  # same size
    big = ops._skinny_workspace(dev, "v6", 4096, 14336)
    assert big.numel() == 64 * 4096 * 8
    retired = ops._SKINNY_WS_RETIRED
    assert len(retired) == 1 and retired[0] is ws
