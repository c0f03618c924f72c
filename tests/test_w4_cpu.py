"""MXFP4 weight-only quantisation without a GPU: the quantiser and linear
references, the holder, the W4 split-K plan, the tiny-llama engine on mxfp4
weights, and the server flag. The quantiser's outputs are integers fixed by
the OCP MX rule, so they are checked exactly; its error bound is read off
the e2m1 grid 0, 0.5, 1, 1.5, 2, 3, 4, 6 (spacing 0.5 below 2, 1 below 4,
2 below 6, saturation above)."""
import pytest
import torch

import kukeon_amd.ops as ops
from kukeon_amd.ops import reference

VALUES = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _weight(N, K, seed=0):
    """Rows whose magnitudes span 2^-8 .. 2^8, plus one all-zero row."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g)
    mag = torch.pow(2.0, torch.linspace(-8, 8, N))
    w = (w * mag[:, None]).bfloat16()
    w[N // 2] = 0
    return w


def _quantize(w):
    N, K = w.shape
    q = torch.empty(N, K // 2, dtype=torch.uint8)
    scale = torch.empty(N, K // 32, dtype=torch.uint8)
    reference.quantize_mxfp4_rows(q, scale, w)
    return q, scale


def _codes(q):
    """[N, K] codes: element 2j from the low nibble, 2j+1 from the high."""
    return torch.stack([q & 0xF, q >> 4], dim=2).view(q.shape[0], -1)


def _deq(q, scale):
    """The weight a (q, scale) pair stands for, in f64, by the format's
    definition (independent of reference.dequant_mxfp4_rows)."""
    c = _codes(q).long()
    v = VALUES.double()[c & 7] * torch.where((c & 8) != 0, -1.0, 1.0)
    X = torch.pow(2.0, scale.double() - 127)
    return v * X.repeat_interleave(32, dim=1)


def test_quantize_reference():
    N, K = 96, 128
    w = _weight(N, K)
    q, scale = _quantize(w)
    assert q.shape == (N, K // 2) and scale.shape == (N, K // 32)
    zero = N // 2
    amax = w.float().abs().view(N, K // 32, 32).amax(dim=2)
    live = amax > 0
    assert not bool(live[zero].any()) and bool(live[:zero].all())
    want = torch.floor(torch.log2(amax[live].double())) + 125
    assert torch.equal(scale[live].double(), want)
    assert bool((scale[~live] == 127).all()) and int(q[zero].max()) == 0
    assert int((scale == 0).sum()) == 0 and int((scale == 255).sum()) == 0
    # each block's largest element lands on 4 or 6
    top = (_codes(q) & 7).view(N, K // 32, 32).amax(dim=2)
    assert bool((top[live] >= 6).all())
    # error bound from the grid, v = |w| / X
    X = torch.pow(2.0, scale.double() - 127).repeat_interleave(32, dim=1)
    v = w.double().abs() / X
    assert bool((v < 8).all())
    bound = torch.where(v < 2, 0.25, torch.where(v < 4, 0.5, 1.0))
    bound = torch.where(v > 6, v - 6, bound) * X
    err = (_deq(q, scale) - w.double()).abs()
    assert bool((err <= bound).all())
    # signs are w's wherever the code is not zero
    c = _codes(q)
    nz = (c & 7) != 0
    assert torch.equal(((c & 8) != 0)[nz], (w.float() < 0)[nz])


def test_quantize_ties_and_saturation():
    # one block whose amax 7.9 gives X = 1 (floor(log2 7.9) - 2 = 0)
    v = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.9, -0.75, 6.0, 0.0, 0.125]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 6.0, -1.0, 6.0, 0.0, 0.0]
    w = torch.zeros(1, 32)
    w[0, :len(v)] = torch.tensor(v)
    w = w.bfloat16()
    assert torch.equal(w[0, :len(v)].float(), torch.tensor(v).bfloat16().float())
    q, scale = _quantize(w)
    assert int(scale[0, 0]) == 127
    got = _deq(q, scale)[0, :len(v)]
    assert got.tolist() == want
    # 7.9 is not a bf16 number; what was quantised is its rounding (7.90625)
    assert float(w[0, 7]) > 6
    assert int(_codes(q)[0, 8]) == 0b1010          # -1: sign | code 2
    # the same block scaled by 2^-20 and 2^20 keeps its codes
    for e in (-20, 20):
        q2, s2 = _quantize((w.float() * 2.0 ** e).bfloat16())
        assert int(s2[0, 0]) == 127 + e and torch.equal(q2, q)


def test_quantize_weight_holder_and_dequant():
    w = _weight(64, 128, seed=1)
    mw = ops.quantize_weight(w, fmt="mxfp4")
    assert isinstance(mw, ops.Mxfp4Weight)
    assert isinstance(ops.quantize_weight(w), ops.Fp8Weight)  # default stays
    assert mw.shape == (64, 128) and mw.q.shape == (64, 64)
    assert mw.q.dtype == torch.uint8 and mw.scale.dtype == torch.uint8
    assert mw.scale.shape == (64, 4)
    assert mw.nbytes == 64 * 128 // 2 + 64 * 128 // 32
    assert mw.device == w.device and not mw.is_cuda
    q, scale = _quantize(w)
    assert torch.equal(mw.q, q) and torch.equal(mw.scale, scale)
    deq = ops.dequantize_weight(mw)
    want = _deq(q, scale)
    assert deq.dtype == torch.bfloat16
    assert torch.equal(deq.double(), want)            # exact in bf16
    out = torch.empty(64, 128, dtype=torch.bfloat16)
    assert ops.dequantize_weight(mw, out=out) is out
    assert torch.equal(out, deq)
    with pytest.raises(ValueError):
        ops.quantize_weight(w[:, :48], fmt="mxfp4")
    with pytest.raises(ValueError):
        ops.quantize_weight(w, fmt="int4")


@pytest.mark.parametrize("M", [1, 17, 65])
def test_linear_mxfp4_cpu(M):
    N, K = 96, 128
    torch.manual_seed(2)
    w = _weight(N, K, seed=3)
    x = (torch.randn(M, K) * 0.5).bfloat16()
    mw = ops.quantize_weight(w, fmt="mxfp4")
    got = ops.linear(x, mw)
    deq = ops.dequantize_weight(mw)
    assert got.dtype == torch.bfloat16 and got.shape == (M, N)
    assert torch.equal(got, (x.float() @ deq.float().T).bfloat16())
    assert torch.equal(got, reference.linear_w4(x, mw.q, mw.scale))


def test_linear_add_rmsnorm_and_mlp_down_mxfp4_cpu():
    torch.manual_seed(4)
    M, N, K = 5, 64, 128
    w = (torch.randn(N, K) * 0.05).bfloat16()
    mw = ops.quantize_weight(w, fmt="mxfp4")
    x = (torch.randn(M, K) * 0.3).bfloat16()
    nw = (torch.rand(N) + 0.5).bfloat16()
    res = torch.randn(M, N).bfloat16()
    res_ref = res.clone()
    got = ops.linear_add_rmsnorm(x, mw, res, nw, 1e-5)
    h = reference.linear_w4(x, mw.q, mw.scale)
    reference.fused_add_rmsnorm(h, res_ref, nw, 1e-5)
    assert torch.equal(got, h) and torch.equal(res, res_ref)
    gu = (torch.randn(M, 2 * K) * 0.5).bfloat16()
    res2, res2_ref = res.clone(), res.clone()
    got2 = ops.mlp_down_fused(gu, mw, res2, nw, 1e-5)
    act = torch.empty(M, K, dtype=torch.bfloat16)
    reference.silu_mul(act, gu)
    h2 = reference.linear_w4(act, mw.q, mw.scale)
    reference.fused_add_rmsnorm(h2, res2_ref, nw, 1e-5)
    assert torch.equal(got2, h2) and torch.equal(res2, res2_ref)


# W4 plan: the W8 plan's parameters (64 columns per block, 256-deep slices,
# split-K sized to 256 blocks, off once 512 blocks lie along N); an
# override is clamped to the slice count.
@pytest.mark.parametrize("N,K,env,splitk", [
    (4096, 4096, None, 4),        # 64 groups, 16 slices: ceil(256/64)
    (4096, 14336, None, 4),       # 64 groups, 56 slices
    (128256, 4096, None, 1),      # 2004 groups: split-K off
    (4096, 14336, "7", 7),
    (4096, 4096, "1000", 16),     # clamped to the 16 slices
    (128256, 4096, "2", 2),
    (64, 640, "1000", 3),         # a short last slice counts as one
])
def test_w4_splitk_plan(N, K, env, splitk, monkeypatch):
    if not ops.native_available():
        pytest.skip("HIP extension not built")
    from kukeon_amd import _C
    monkeypatch.delenv("KUKEON_W4_SPLITK", raising=False)
    if env is not None:
        monkeypatch.setenv("KUKEON_W4_SPLITK", env)
    assert _C.skinny_splitk("w4", N, K) == splitk


# ---- tiny-llama on mxfp4 weights ----

def _run_turn(model, cfg, n=6):
    from kukeon_amd.engine.config import EngineConfig, SamplingParams
    from kukeon_amd.engine.engine import LLMEngine
    from kukeon_amd.engine.kv_cache import SequenceKV
    ecfg = EngineConfig(max_model_len=128, max_sessions=2, num_kv_blocks=64,
                        use_graphs=False)
    engine = LLMEngine(model, cfg, ecfg, device="cpu")
    kv = SequenceKV(ecfg.block_size)
    engine.add_request(kv, [7, 3, 99, 140, 11, 42],
                       SamplingParams(temperature=0.0, max_new_tokens=n))
    toks = []
    while engine.has_work():
        for o in engine.step():
            toks.extend(o.new_tokens)
    return toks


@pytest.fixture(scope="module")
def tiny_models():
    from kukeon_amd.engine.config import tiny_llama
    from kukeon_amd.models.llama import LlamaModel
    cfg = tiny_llama()
    return (cfg, LlamaModel(cfg, device="cpu", weight_dtype="bf16"),
            LlamaModel(cfg, device="cpu", weight_dtype="mxfp4"))


def test_tiny_llama_mxfp4_engine_turn(tiny_models):
    from kukeon_amd.models.llama import LlamaModel
    cfg, _, m4 = tiny_models
    toks = _run_turn(m4, cfg, n=6)
    assert len(toks) == 6
    again = _run_turn(LlamaModel(cfg, device="cpu", weight_dtype="mxfp4"),
                      cfg, n=6)
    assert again == toks


def test_tiny_llama_mxfp4_is_quantised_bf16_model(tiny_models):
    cfg, m16, m4 = tiny_models
    assert m16.weight_dtype == "bf16" and m4.weight_dtype == "mxfp4"
    w16 = dict(m16.gemm_weights())
    w4 = dict(m4.gemm_weights())
    assert w16.keys() == w4.keys() and len(w4) == 4 * cfg.num_layers + 1
    b16 = b4 = 0
    for name, w in w16.items():
        mw = w4[name]
        assert isinstance(mw, ops.Mxfp4Weight), name
        assert isinstance(w, torch.Tensor), name
        assert mw.shape == tuple(w.shape)
        # the decode kernel's contract holds for every tiny-llama weight
        assert w.shape[0] % 64 == 0 and w.shape[1] % 128 == 0, name
        want = ops.quantize_weight(w.data, fmt="mxfp4")
        assert torch.equal(mw.q, want.q), name
        assert torch.equal(mw.scale, want.scale), name
        assert mw.nbytes == w.numel() // 2 + w.numel() // 32
        b16 += w.numel() * w.element_size()
        b4 += mw.nbytes
    # 2 bytes per element against 0.53125
    assert b4 * 64 == b16 * 17
    # what stays bf16 is the same tensor in both models
    assert torch.equal(m16.embed, m4.embed)
    assert m4.embed.dtype == torch.bfloat16
    assert m16.resident_weight_bytes() - m4.resident_weight_bytes() == \
        b16 - b4


def test_weight_dtype_env_and_override(monkeypatch):
    from kukeon_amd.engine.config import tiny_llama
    from kukeon_amd.models.llama import LlamaModel
    cfg = tiny_llama()
    monkeypatch.setenv("KUKEON_WEIGHT_DTYPE", "mxfp4")
    m = LlamaModel(cfg, device="cpu")
    assert m.weight_dtype == "mxfp4"
    assert isinstance(m.lm_head, ops.Mxfp4Weight)
    m = LlamaModel(cfg, device="cpu", weight_dtype="bf16")
    assert m.weight_dtype == "bf16"
    assert isinstance(m.lm_head, torch.Tensor)
    monkeypatch.delenv("KUKEON_WEIGHT_DTYPE", raising=False)
    m = LlamaModel(cfg, device="cpu", weight_dtype="mxfp4")
    assert isinstance(m.layers[0].attn.qkv_w, ops.Mxfp4Weight)


def test_mixtral_mxfp4_raises(monkeypatch):
    from kukeon_amd.engine.config import tiny_mixtral
    from kukeon_amd.models.mixtral import MixtralModel
    monkeypatch.delenv("KUKEON_WEIGHT_DTYPE", raising=False)
    with pytest.raises(ValueError, match="mxfp4 expert weights"):
        MixtralModel(tiny_mixtral(), device="cpu", weight_dtype="mxfp4")
    monkeypatch.setenv("KUKEON_WEIGHT_DTYPE", "mxfp4")
    with pytest.raises(ValueError, match="expert weights"):
        MixtralModel(tiny_mixtral(), device="cpu")


def test_server_weight_dtype_flag_and_stats(tiny_models, tmp_path):
    from kukeon_amd.engine.config import EngineConfig
    from kukeon_amd.serve.server import ModelhubServer, build_parser
    ap = build_parser()
    assert ap.parse_args(["--weight-dtype", "mxfp4"]).weight_dtype == "mxfp4"
    cfg, m16, m4 = tiny_models
    ecfg = EngineConfig(max_model_len=128, max_sessions=2, num_kv_blocks=64,
                        use_graphs=False)
    stats = {}
    for m in (m16, m4):
        hub = ModelhubServer(m, cfg, ecfg, str(tmp_path / "hub.sock"),
                             device="cpu")
        stats[m.weight_dtype] = hub.handle("stats", {})
    assert stats["mxfp4"]["weight_dtype"] == "mxfp4"
    assert stats["mxfp4"]["weight_bytes"] == m4.resident_weight_bytes()
    assert stats["mxfp4"]["weight_bytes"] < stats["bf16"]["weight_bytes"]
