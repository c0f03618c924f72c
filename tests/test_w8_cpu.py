"""fp8 (e4m3) weight-only quantisation without a GPU: the quantiser and
linear references, the W8 split-K plan, the tiny-llama engine on fp8
weights, and the server flag. Every bound here is derived from the number
formats: e4m3 has 3 mantissa bits, so a normal value's half-ulp is
2^(e-3)/2 and below 2^-6 (subnormals) the spacing is 2^-9."""
import math

import pytest
import torch

import kukeon_amd.ops as ops
from kukeon_amd.ops import reference


def _weight(N, K, seed=0):
    """Rows whose magnitudes span 2^-8 .. 2^8, plus one all-zero row."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g)
    mag = torch.pow(2.0, torch.linspace(-8, 8, N))
    w = (w * mag[:, None]).bfloat16()
    w[N // 2] = 0
    return w


def half_ulp_bound(w: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """0.5 * scale * max(2^-9, 2^(floor(log2(|w|/scale)) - 3)), with one
    f32 ulp of slack for the quotient and the product."""
    v = w.float().abs() / scale[:, None]
    # frexp: v = m * 2^ex with m in [0.5, 1), so floor(log2 v) = ex - 1
    e = (torch.frexp(v.clamp_min(2.0 ** -30)).exponent - 1).float()
    ulp = torch.maximum(torch.full_like(v, 2.0 ** -9), torch.pow(2.0, e - 3))
    bound = 0.5 * scale[:, None] * ulp
    return bound * (1 + 2.0 ** -22) + 2.0 ** -23 * w.float().abs()


def test_quantize_reference():
    N, K = 96, 128
    w = _weight(N, K)
    q = torch.empty(N, K, dtype=torch.uint8)
    scale = torch.empty(N, dtype=torch.float32)
    reference.quantize_fp8_rows(q, scale, w)
    amax = w.float().abs().amax(dim=1)
    zero = N // 2
    assert scale[zero] == 1.0 and int(q[zero].max()) == 0
    live = torch.arange(N) != zero
    assert torch.equal(scale[live], (amax / 448.0)[live])
    # 0x7f / 0xff are e4m3fn's NaN encodings
    assert int(((q & 0x7F) == 0x7F).sum()) == 0
    deq = q.view(torch.float8_e4m3fn).float() * scale[:, None]
    err = (deq - w.float()).abs()
    assert bool((err <= half_ulp_bound(w, scale)).all())
    # the row maximum lands on +-448 exactly
    assert int((q[live] & 0x7F).max()) == 0x7E


def test_quantize_weight_holder_and_dequant():
    w = _weight(64, 64, seed=1)
    fw = ops.quantize_weight(w)
    assert isinstance(fw, ops.Fp8Weight)
    assert fw.shape == (64, 64) and fw.q.dtype == torch.uint8
    assert fw.scale.dtype == torch.float32 and fw.scale.shape == (64,)
    assert fw.nbytes == 64 * 64 + 4 * 64
    deq = ops.dequantize_weight(fw)
    want = (fw.q.view(torch.float8_e4m3fn).float() *
            fw.scale[:, None]).bfloat16()
    assert deq.dtype == torch.bfloat16 and torch.equal(deq, want)
    out = torch.empty(64, 64, dtype=torch.bfloat16)
    assert ops.dequantize_weight(fw, out=out) is out and torch.equal(out, want)


@pytest.mark.parametrize("M", [1, 17, 65])
def test_linear_fp8_cpu(M):
    N, K = 96, 128
    torch.manual_seed(2)
    w = _weight(N, K, seed=3)
    x = (torch.randn(M, K) * 0.5).bfloat16()
    fw = ops.quantize_weight(w)
    got = ops.linear(x, fw)
    wf = fw.q.view(torch.float8_e4m3fn).float() * fw.scale[:, None]
    assert got.dtype == torch.bfloat16
    assert torch.equal(got, (x.float() @ wf.T).bfloat16())
    # against the bf16 product: per element the quantisation error is at
    # most max(2^-4 |w|, 2^-10 scale) (half an ulp of 3 mantissa bits,
    # or half the subnormal spacing 2^-9 * scale)
    qerr = torch.maximum(2.0 ** -4 * w.float().abs(),
                         2.0 ** -10 * fw.scale[:, None].expand(N, K))
    bound = x.float().abs() @ qerr.T
    ref = x.float() @ w.float().T
    # plus the bf16 rounding of the output and f32 accumulation slack
    slack = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * (
        x.float().abs() @ w.float().abs().T)
    assert bool(((got.float() - ref).abs() <= bound + slack).all())


def test_linear_add_rmsnorm_and_mlp_down_fp8_cpu():
    torch.manual_seed(4)
    M, N, K = 5, 64, 128
    w = (torch.randn(N, K) * 0.05).bfloat16()
    fw = ops.quantize_weight(w)
    x = (torch.randn(M, K) * 0.3).bfloat16()
    nw = (torch.rand(N) + 0.5).bfloat16()
    res = torch.randn(M, N).bfloat16()
    res_ref = res.clone()
    got = ops.linear_add_rmsnorm(x, fw, res, nw, 1e-5)
    h = reference.linear_w8(x, fw.q, fw.scale)
    reference.fused_add_rmsnorm(h, res_ref, nw, 1e-5)
    assert torch.equal(got, h) and torch.equal(res, res_ref)
    gu = (torch.randn(M, 2 * K) * 0.5).bfloat16()
    res2, res2_ref = res.clone(), res.clone()
    got2 = ops.mlp_down_fused(gu, fw, res2, nw, 1e-5)
    act = torch.empty(M, K, dtype=torch.bfloat16)
    reference.silu_mul(act, gu)
    h2 = reference.linear_w8(act, fw.q, fw.scale)
    reference.fused_add_rmsnorm(h2, res2_ref, nw, 1e-5)
    assert torch.equal(got2, h2) and torch.equal(res2, res2_ref)


# W8 plan: 64 columns per block, 256-deep slices, split-K sized to 256
# blocks, off once 512 blocks lie along N; an override is clamped to the
# slice count.
@pytest.mark.parametrize("N,K,env,splitk", [
    (4096, 4096, None, 4),        # 64 groups, 16 slices: ceil(256/64)
    (4096, 14336, None, 4),       # 64 groups, 56 slices
    (128256, 4096, None, 1),      # 2004 groups: split-K off
    (4096, 14336, "7", 7),
    (4096, 4096, "1000", 16),     # clamped to the 16 slices
    (128256, 4096, "2", 2),
])
def test_w8_splitk_plan(N, K, env, splitk, monkeypatch):
    if not ops.native_available():
        pytest.skip("HIP extension not built")
    from kukeon_amd import _C
    monkeypatch.delenv("KUKEON_W8_SPLITK", raising=False)
    if env is not None:
        monkeypatch.setenv("KUKEON_W8_SPLITK", env)
    assert _C.skinny_splitk("w8", N, K) == splitk


# ---- tiny-llama on fp8 weights ----

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
            LlamaModel(cfg, device="cpu", weight_dtype="fp8"))


def test_tiny_llama_fp8_engine_turn(tiny_models):
    from kukeon_amd.models.llama import LlamaModel
    cfg, _, m8 = tiny_models
    toks = _run_turn(m8, cfg, n=6)
    assert len(toks) == 6
    again = _run_turn(LlamaModel(cfg, device="cpu", weight_dtype="fp8"), cfg,
                      n=6)
    assert again == toks


def test_tiny_llama_fp8_is_quantised_bf16_model(tiny_models):
    cfg, m16, m8 = tiny_models
    assert m16.weight_dtype == "bf16" and m8.weight_dtype == "fp8"
    w16 = dict(m16.gemm_weights())
    w8 = dict(m8.gemm_weights())
    assert w16.keys() == w8.keys() and len(w8) == 4 * cfg.num_layers + 1
    b16 = b8 = scales = 0
    for name, w in w16.items():
        fw = w8[name]
        assert isinstance(fw, ops.Fp8Weight), name
        assert not isinstance(w, ops.Fp8Weight), name
        assert fw.shape == tuple(w.shape)
        want = ops.quantize_weight(w.data)
        assert torch.equal(fw.q, want.q), name
        assert torch.equal(fw.scale, want.scale), name
        b16 += w.numel() * w.element_size()
        b8 += fw.nbytes
        scales += 4 * w.shape[0]
    assert b8 * 2 == b16 + 2 * scales
    # what stays bf16 is the same tensor in both models
    assert torch.equal(m16.embed, m8.embed)
    assert m8.embed.dtype == torch.bfloat16
    assert m16.resident_weight_bytes() - m8.resident_weight_bytes() == \
        b16 - b8


def test_weight_dtype_env_and_override(monkeypatch):
    from kukeon_amd.engine.config import tiny_llama
    from kukeon_amd.models.llama import LlamaModel
    cfg = tiny_llama()
    monkeypatch.delenv("KUKEON_WEIGHT_DTYPE", raising=False)
    assert LlamaModel(cfg, device="cpu").weight_dtype == "bf16"
    monkeypatch.setenv("KUKEON_WEIGHT_DTYPE", "fp8")
    m = LlamaModel(cfg, device="cpu")
    assert m.weight_dtype == "fp8"
    assert isinstance(m.lm_head, ops.Fp8Weight)
    m = LlamaModel(cfg, device="cpu", weight_dtype="bf16")
    assert m.weight_dtype == "bf16"
    assert isinstance(m.lm_head, torch.Tensor)
    with pytest.raises(ValueError):
        LlamaModel(cfg, device="cpu", weight_dtype="int4")


def test_mixtral_fp8_raises(monkeypatch):
    from kukeon_amd.engine.config import tiny_mixtral
    from kukeon_amd.models.mixtral import MixtralModel
    monkeypatch.delenv("KUKEON_WEIGHT_DTYPE", raising=False)
    with pytest.raises(ValueError, match="expert weights"):
        MixtralModel(tiny_mixtral(), device="cpu", weight_dtype="fp8")


def test_server_weight_dtype_flag_and_stats(tiny_models, tmp_path):
    from kukeon_amd.engine.config import EngineConfig
    from kukeon_amd.serve.server import ModelhubServer, build_parser
    ap = build_parser()
    assert ap.parse_args([]).weight_dtype is None
    assert ap.parse_args(["--weight-dtype", "fp8"]).weight_dtype == "fp8"
    assert ap.parse_args(["--weight-dtype", "bf16"]).weight_dtype == "bf16"
    with pytest.raises(SystemExit):
        ap.parse_args(["--weight-dtype", "int4"])
    cfg, m16, m8 = tiny_models
    ecfg = EngineConfig(max_model_len=128, max_sessions=2, num_kv_blocks=64,
                        use_graphs=False)
    stats = {}
    for m in (m16, m8):
        hub = ModelhubServer(m, cfg, ecfg, str(tmp_path / "hub.sock"),
                             device="cpu")
        stats[m.weight_dtype] = hub.handle("stats", {})
    assert stats["fp8"]["weight_dtype"] == "fp8"
    assert stats["bf16"]["weight_dtype"] == "bf16"
    assert stats["fp8"]["weight_bytes"] == m8.resident_weight_bytes()
    assert stats["fp8"]["weight_bytes"] < stats["bf16"]["weight_bytes"]
