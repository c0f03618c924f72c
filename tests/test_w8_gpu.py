"""fp8 (e4m3) weight-only quantisation on the GPU: the quantise and
dequantise kernels, the W8A16 skinny decode GEMM on every path of its
slice walk and both epilogues, the ops.linear dispatch, and graphed decode
on fp8 weights. S = 256 is the kernel's K-slice length."""
import functools

import pytest
import torch

import kukeon_amd.ops as ops
from kukeon_amd.ops import reference

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

DEV = "cuda:0"
S = 256
GUARD = 64


def test_native_loaded():
    assert ops.native_available()


def _weight(N, K, seed):
    """Row magnitudes vary by 2^7 across N and the columns ramp across K:
    a wrong scale index, a transposed C layout or a permuted k cannot
    pass."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * 0.05
    w = w * torch.pow(2.0, torch.linspace(-4, 3, N))[:, None]
    w = w * torch.linspace(0.25, 1.75, K)[None, :]
    return w.bfloat16()


def _half_ulp_bound(w, scale):
    """Half an e4m3 ulp of w / scale (spacing 2^-9 below the normals),
    times scale, with one f32 ulp of slack."""
    v = w.float().abs() / scale[:, None]
    e = (torch.frexp(v.clamp_min(2.0 ** -30)).exponent - 1).float()
    ulp = torch.maximum(torch.full_like(v, 2.0 ** -9), torch.pow(2.0, e - 3))
    return (0.5 * scale[:, None] * ulp * (1 + 2.0 ** -22)
            + 2.0 ** -23 * w.float().abs())


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """(x, q, scale) on the CPU, the f64 product on the exact dequantised
    weight, and |x| @ |deq|^T; computed once and only read."""
    g = torch.Generator().manual_seed(1000 * M + N + K)
    x = (torch.randn(M, K, generator=g) * 0.5).bfloat16()
    w = _weight(N, K, seed=N * 7 + K)
    q = torch.empty(N, K, dtype=torch.uint8)
    scale = torch.empty(N, dtype=torch.float32)
    reference.quantize_fp8_rows(q, scale, w)
    deq = q.view(torch.float8_e4m3fn).double() * scale.double()[:, None]
    ref = x.double() @ deq.T
    mag = x.double().abs() @ deq.abs().T
    return x, q, scale, ref, mag


def _tol(ref, mag, K):
    # one bf16 rounding of the output + f32 accumulation in any order
    return 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * mag


@pytest.mark.parametrize("N,K", [(64, 64), (192, S), (192, 2 * S + 64)])
def test_quantize_fp8_rows(N, K):
    w = _weight(N, K, seed=5)
    w[N // 3] = 0
    q_ref = torch.empty(N, K, dtype=torch.uint8)
    s_ref = torch.empty(N, dtype=torch.float32)
    reference.quantize_fp8_rows(q_ref, s_ref, w)
    fw = ops.quantize_weight(w.to(DEV))
    q, scale = fw.q.cpu(), fw.scale.cpu()
    assert torch.equal(scale, s_ref)
    assert scale[N // 3] == 1.0 and int(q[N // 3].max()) == 0
    assert int(((q & 0x7F) == 0x7F).sum()) == 0
    deq = q.view(torch.float8_e4m3fn).float() * scale[:, None]
    err = (deq - w.float()).abs()
    print("quantize: bytes differing from the reference:",
          int((q != q_ref).sum()))
    assert bool((err <= _half_ulp_bound(w, scale)).all())


@pytest.mark.parametrize("N,K", [(64, 64), (192, 2 * S + 64)])
def test_dequant_fp8_rows(N, K):
    _, q, scale, _, _ = _case(1, N, K)
    want = torch.empty(N, K, dtype=torch.bfloat16)
    reference.dequant_fp8_rows(want, q, scale)
    buf = torch.full((N * K + GUARD,), 3.0, dtype=torch.bfloat16, device=DEV)
    out = buf[:N * K].view(N, K)
    got = ops.dequantize_weight(ops.Fp8Weight(q.to(DEV), scale.to(DEV)),
                                out=out)
    assert got is out
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))
    assert bool((buf[N * K:] == 3.0).all())


@pytest.mark.parametrize("splitk", [1, 2, 1000])
@pytest.mark.parametrize("K", [64, S, 2 * S + 64])
@pytest.mark.parametrize("N", [64, 192])
@pytest.mark.parametrize("M", [1, 16, 17, 64])
def test_skinny_gemm_w8(M, N, K, splitk, monkeypatch):
    _check_w8(M, N, K, splitk, monkeypatch)


@pytest.mark.parametrize("splitk", [1, 2])
@pytest.mark.parametrize("K", [3 * S, 4 * S, 5 * S + 64, 9 * S])
@pytest.mark.parametrize("M,N", [(17, 64), (64, 192)])
def test_skinny_gemm_w8_long_walk(M, N, K, splitk, monkeypatch):
    """The kernel keeps two slices of W in flight over three rotating
    register sets: a block's last two whole slices issue nothing, the
    ones before run in turns of three with a remainder of 0, 1 or 2.
    Blocks here walk 1 to 9 whole slices, with and without a short tail:
    every remainder, and more than one whole turn."""
    _check_w8(M, N, K, splitk, monkeypatch)


def _check_w8(M, N, K, splitk, monkeypatch):
    from kukeon_amd import _C
    monkeypatch.setenv("KUKEON_W8_SPLITK", str(splitk))
    x, q, scale, ref, mag = _case(M, N, K)
    sk = min(splitk, -(-K // S))          # the plan clamps to the slices
    assert _C.skinny_splitk("w8", N, K) == sk
    obuf = torch.full((M * N + GUARD,), 3.0, dtype=torch.bfloat16,
                      device=DEV)
    wbuf = torch.full((M * N * sk + GUARD,), 7.0, dtype=torch.float32,
                      device=DEV)
    out = obuf[:M * N].view(M, N)
    _C.skinny_gemm_w8(out, x.to(DEV), q.to(DEV), scale.to(DEV),
                      wbuf[:M * N * sk])
    torch.cuda.synchronize()
    assert bool((obuf[M * N:] == 3.0).all())
    assert bool((wbuf[M * N * sk:] == 7.0).all())
    err = (out.cpu().double() - ref).abs()
    tol = _tol(ref, mag, K)
    print(f"w8 M={M} N={N} K={K} sk={sk}: max err/tol "
          f"{float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())


@pytest.mark.parametrize("M", [1, 17, 64])
def test_skinny_gemm_w8_fused_norm(M):
    """W8 GEMM + split-K reduce + residual add + RMSNorm against linear
    then fused_add_rmsnorm on the reference, at the smallest N the
    epilogue accepts; tolerances and input scale are those of
    test_skinny_gemm5_fused_norm (same epilogue)."""
    from kukeon_amd import _C
    torch.manual_seed(7)
    N, K = 2048, 2 * S
    x = (torch.randn(M, K) * 0.3).bfloat16()
    w = (torch.randn(N, K) * 0.05).bfloat16()
    resid = torch.randn(M, N).bfloat16()
    nw = (torch.rand(N) + 0.5).bfloat16()
    eps = 1e-5
    q = torch.empty(N, K, dtype=torch.uint8)
    scale = torch.empty(N, dtype=torch.float32)
    reference.quantize_fp8_rows(q, scale, w)
    h_ref = reference.linear_w8(x, q, scale)
    r_ref = resid.clone()
    reference.fused_add_rmsnorm(h_ref, r_ref, nw, eps)
    sk = _C.skinny_splitk("w8", N, K)
    assert sk == 2
    wbuf = torch.full((M * N * sk + GUARD,), 7.0, dtype=torch.float32,
                      device=DEV)
    nbuf = torch.full((M * N + GUARD,), 3.0, dtype=torch.bfloat16,
                      device=DEV)
    normed = nbuf[:M * N].view(M, N)
    resid_d = resid.to(DEV)
    _C.skinny_gemm_w8_fused_norm(normed, x.to(DEV), q.to(DEV), scale.to(DEV),
                                 wbuf[:M * N * sk], resid_d, nw.to(DEV), eps)
    torch.cuda.synchronize()
    assert bool((nbuf[M * N:] == 3.0).all())
    assert bool((wbuf[M * N * sk:] == 7.0).all())
    torch.testing.assert_close(normed.float().cpu(), h_ref.float(),
                               rtol=4e-2, atol=6e-2)
    torch.testing.assert_close(resid_d.float().cpu(), r_ref.float(),
                               rtol=3e-2, atol=5e-2)


def _fresh_buffers():
    """Retire (never free: a captured graph may still point at them) the
    cached split-K workspace and dequant scratch."""
    ops._SKINNY_WS_RETIRED.extend(ops._SKINNY_WS.values())
    ops._SKINNY_WS.clear()
    ops._W8_SCRATCH_RETIRED.extend(ops._W8_SCRATCH.values())
    ops._W8_SCRATCH.clear()


def test_linear_dispatch_fp8(monkeypatch):
    """ops.linear on an Fp8Weight: the W8 kernel up to 64 rows (same bits
    as the direct call), dequant + library GEMM above, with the workspace
    sized by the plan and the scratch by the weight.

    The 65-row route multiplies by the bf16-rounded dequantised weight (it
    is dequant_fp8_rows, then the library), so its reference is the f64
    product on reference.dequant_fp8_rows' output; against the unrounded
    weight it carries one more 2^-9 rounding per weight element, which the
    GEMM tolerance (output rounding + accumulation order) does not and
    should not cover."""
    from kukeon_amd import _C
    monkeypatch.delenv("KUKEON_W8_SPLITK", raising=False)
    monkeypatch.setattr(ops, "_SKINNY_SPLITK", {})
    N, K = 256, 4 * S                      # 4 groups, 4 slices: splitk 4
    _fresh_buffers()
    x64, q, scale, ref, mag = _case(64, N, K)
    fw = ops.Fp8Weight(q.to(DEV), scale.to(DEV))
    got = ops.linear(x64.to(DEV), fw)
    assert _C.skinny_splitk("w8", N, K) == 4
    assert ops._SKINNY_WS[0].numel() == 64 * N * 4
    assert not ops._W8_SCRATCH                 # no scratch on this route
    direct = torch.empty(64, N, dtype=torch.bfloat16, device=DEV)
    _C.skinny_gemm_w8(direct, x64.to(DEV), fw.q, fw.scale,
                      ops._SKINNY_WS[0])
    assert torch.equal(got.view(torch.int16), direct.view(torch.int16))
    assert bool(((got.cpu().double() - ref).abs()
                 <= _tol(ref, mag, K)).all())

    g = torch.Generator().manual_seed(65)
    x65 = (torch.randn(65, K, generator=g) * 0.5).bfloat16()
    got65 = ops.linear(x65.to(DEV), fw)
    assert ops._W8_SCRATCH[0].numel() == N * K
    deq = torch.empty(N, K, dtype=torch.bfloat16)
    reference.dequant_fp8_rows(deq, q, scale)
    ref65 = x65.double() @ deq.double().T
    mag65 = x65.double().abs() @ deq.double().abs().T
    err = (got65.cpu().double() - ref65).abs()
    assert got65.shape == (65, N)
    assert bool((err <= _tol(ref65, mag65, K)).all())
    # quantize_weight reserves the scratch for the largest weight it made
    _fresh_buffers()
    ops.quantize_weight(_weight(N, K, seed=1).to(DEV))
    ops.quantize_weight(_weight(64, 64, seed=2).to(DEV))
    assert ops._W8_SCRATCH[0].numel() == N * K


def test_decode_graphs_match_eager_fp8_weights():
    """test_decode_graphs_match_eager's recipe on fp8 weights."""
    from kukeon_amd.engine.config import (EngineConfig, SamplingParams,
                                          tiny_llama)
    from kukeon_amd.engine.engine import LLMEngine
    from kukeon_amd.engine.kv_cache import SequenceKV
    from kukeon_amd.models.llama import LlamaModel

    cfg = tiny_llama()
    prompt = [7, 3, 99, 140, 11, 42, 17, 23, 5, 81]
    outs = {}
    for use_graphs in (False, True):
        torch.manual_seed(0)
        ecfg = EngineConfig(max_model_len=256, max_sessions=4,
                            num_kv_blocks=128, use_graphs=use_graphs,
                            decode_microbatch=4, graph_buckets=(1, 2, 4))
        model = LlamaModel(cfg, device=DEV, weight_dtype="fp8")
        assert isinstance(model.lm_head, ops.Fp8Weight)
        engine = LLMEngine(model, cfg, ecfg, device=DEV)
        kv = SequenceKV(ecfg.block_size)
        engine.add_request(kv, prompt,
                           SamplingParams(temperature=0.0, max_new_tokens=9))
        toks = []
        while engine.has_work():
            for o in engine.step():
                toks.extend(o.new_tokens)
        outs[use_graphs] = toks
    assert outs[False] == outs[True], outs
    assert len(outs[True]) == 9
