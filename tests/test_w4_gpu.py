"""MXFP4 weight-only quantisation on the GPU: the quantise and dequantise
kernels against the CPU reference bit for bit, the W4A16 skinny decode
GEMM on every path of its slice walk and both epilogues, the ops.linear
dispatch, and graphed decode on mxfp4 weights. S = 256 is the kernel's
K-slice length; its short tail is 128."""
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
    """tests/test_w8_gpu.py's generator: row magnitudes vary by 2^7 across
    N and the columns ramp across K, so a wrong scale index, a swapped
    nibble, a transposed C layout or a permuted k cannot pass."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, K, generator=g) * 0.05
    w = w * torch.pow(2.0, torch.linspace(-4, 3, N))[:, None]
    w = w * torch.linspace(0.25, 1.75, K)[None, :]
    return w.bfloat16()


def _quantize_ref(w):
    N, K = w.shape
    q = torch.empty(N, K // 2, dtype=torch.uint8)
    scale = torch.empty(N, K // 32, dtype=torch.uint8)
    reference.quantize_mxfp4_rows(q, scale, w)
    return q, scale


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """(x, q, scale) on the CPU, the f64 product on the exact dequantised
    weight, and |x| @ |deq|^T; computed once and only read."""
    g = torch.Generator().manual_seed(1000 * M + N + K)
    x = (torch.randn(M, K, generator=g) * 0.5).bfloat16()
    q, scale = _quantize_ref(_weight(N, K, seed=N * 7 + K))
    deq = torch.empty(N, K, dtype=torch.float64)
    reference.dequant_mxfp4_rows(deq, q, scale)
    ref = x.double() @ deq.T
    mag = x.double().abs() @ deq.abs().T
    return x, q, scale, ref, mag


def _tol(ref, mag, K):
    # one bf16 rounding of the output + f32 accumulation in any order
    return 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * mag


@pytest.mark.parametrize("N,K", [(64, 128), (192, S), (192, 2 * S + 128)])
def test_quantize_mxfp4_rows(N, K):
    w = _weight(N, K, seed=5)
    w[N // 3] = 0
    # the listed ties, saturation and a negative tie, at X = 1 and X = 2^-3
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.9, -0.75])
    w[1, :32] = 0
    w[1, :9] = ties.bfloat16()
    w[2, 32:64] = 0
    w[2, 32:41] = (ties / 8).bfloat16()
    q_ref, s_ref = _quantize_ref(w)
    mw = ops.quantize_weight(w.to(DEV), fmt="mxfp4")
    assert isinstance(mw, ops.Mxfp4Weight) and mw.shape == (N, K)
    q, scale = mw.q.cpu(), mw.scale.cpu()
    print("quantize: scale bytes differing:", int((scale != s_ref).sum()),
          "code bytes differing:", int((q != q_ref).sum()))
    assert torch.equal(scale, s_ref)
    assert torch.equal(q, q_ref)
    assert bool((scale[N // 3] == 127).all()) and int(q[N // 3].max()) == 0
    assert int(scale[1, 0]) == 127 and int(scale[2, 1]) == 124
    # low nibble first: 0.25 -> 0 | 0.75 -> 1.0 (code 2) in the high nibble
    assert q[1, :5].tolist() == [0x20, 0x42, 0x64, 0x76, 0x0A]
    assert q[2, 16:21].tolist() == [0x20, 0x42, 0x64, 0x76, 0x0A]


@pytest.mark.parametrize("N,K", [(64, 128), (192, S), (192, 2 * S + 128)])
def test_dequant_mxfp4_rows(N, K):
    _, q, scale, _, _ = _case(1, N, K)
    q = q.clone()
    # every code in both nibbles of known positions, whatever the weight
    q[0, :16] = torch.arange(16, dtype=torch.uint8) * 17
    q[5, 16:32] = (torch.arange(16, dtype=torch.uint8)
                   | (15 - torch.arange(16, dtype=torch.uint8)) << 4)
    want = torch.empty(N, K, dtype=torch.bfloat16)
    reference.dequant_mxfp4_rows(want, q, scale)
    buf = torch.full((N * K + GUARD,), 3.0, dtype=torch.bfloat16, device=DEV)
    out = buf[:N * K].view(N, K)
    got = ops.dequantize_weight(ops.Mxfp4Weight(q.to(DEV), scale.to(DEV)),
                                out=out)
    assert got is out
    bad = out.cpu().view(torch.int16) != want.view(torch.int16)
    print("dequant: elements differing from the reference:", int(bad.sum()))
    assert not bool(bad.any())
    assert bool((buf[N * K:] == 3.0).all())


@pytest.mark.parametrize("splitk", [1, 2, 1000])
@pytest.mark.parametrize("K", [128, S, 2 * S + 128])
@pytest.mark.parametrize("N", [64, 192])
@pytest.mark.parametrize("M", [1, 16, 17, 64])
def test_skinny_gemm_w4(M, N, K, splitk, monkeypatch):
    _check_w4(M, N, K, splitk, monkeypatch)


@pytest.mark.parametrize("splitk", [1, 2])
@pytest.mark.parametrize("K", [3 * S, 4 * S, 5 * S + 128, 9 * S])
@pytest.mark.parametrize("M,N", [(17, 64), (64, 192)])
def test_skinny_gemm_w4_long_walk(M, N, K, splitk, monkeypatch):
    """The kernel keeps two slices of W in flight over three rotating
    register sets, as the W8 kernel does, with the same slice length 256:
    a block's last two whole slices issue nothing, the ones before run in
    turns of three with a remainder of 0, 1 or 2. Blocks here walk 1 to 9
    whole slices (K = 768, 1024, 1408, 2304 at splitk 1 and 2), with and
    without the short 128-k tail: every remainder, and more than one whole
    turn."""
    _check_w4(M, N, K, splitk, monkeypatch)


def _check_w4(M, N, K, splitk, monkeypatch):
    from kukeon_amd import _C
    monkeypatch.setenv("KUKEON_W4_SPLITK", str(splitk))
    x, q, scale, ref, mag = _case(M, N, K)
    sk = min(splitk, -(-K // S))          # the plan clamps to the slices
    assert _C.skinny_splitk("w4", N, K) == sk
    obuf = torch.full((M * N + GUARD,), 3.0, dtype=torch.bfloat16,
                      device=DEV)
    wbuf = torch.full((M * N * sk + GUARD,), 7.0, dtype=torch.float32,
                      device=DEV)
    out = obuf[:M * N].view(M, N)
    _C.skinny_gemm_w4(out, x.to(DEV), q.to(DEV), scale.to(DEV),
                      wbuf[:M * N * sk])
    torch.cuda.synchronize()
    assert bool((obuf[M * N:] == 3.0).all())
    assert bool((wbuf[M * N * sk:] == 7.0).all())
    err = (out.cpu().double() - ref).abs()
    tol = _tol(ref, mag, K)
    print(f"w4 M={M} N={N} K={K} sk={sk}: max err/tol "
          f"{float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())


@pytest.mark.parametrize("M", [1, 17, 64])
def test_skinny_gemm_w4_fused_norm(M):
    """W4 GEMM + split-K reduce + residual add + RMSNorm against linear_w4
    then fused_add_rmsnorm on the reference, at the smallest N the
    epilogue accepts; tolerances and input scale are those of
    test_skinny_gemm_w8_fused_norm (same epilogue)."""
    from kukeon_amd import _C
    torch.manual_seed(7)
    N, K = 2048, 2 * S
    x = (torch.randn(M, K) * 0.3).bfloat16()
    w = (torch.randn(N, K) * 0.05).bfloat16()
    resid = torch.randn(M, N).bfloat16()
    nw = (torch.rand(N) + 0.5).bfloat16()
    eps = 1e-5
    q, scale = _quantize_ref(w)
    h_ref = reference.linear_w4(x, q, scale)
    r_ref = resid.clone()
    reference.fused_add_rmsnorm(h_ref, r_ref, nw, eps)
    sk = _C.skinny_splitk("w4", N, K)
    assert sk == 2
    wbuf = torch.full((M * N * sk + GUARD,), 7.0, dtype=torch.float32,
                      device=DEV)
    nbuf = torch.full((M * N + GUARD,), 3.0, dtype=torch.bfloat16,
                      device=DEV)
    normed = nbuf[:M * N].view(M, N)
    resid_d = resid.to(DEV)
    _C.skinny_gemm_w4_fused_norm(normed, x.to(DEV), q.to(DEV), scale.to(DEV),
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


def test_linear_dispatch_mxfp4(monkeypatch):
    """ops.linear on an Mxfp4Weight: the W4 kernel up to 64 rows (same
    bits as the direct call), dequant + library GEMM above, with the
    workspace sized by the plan and the scratch by the weight. Both routes
    multiply by the same exact weight, so they share one reference."""
    from kukeon_amd import _C
    monkeypatch.delenv("KUKEON_W4_SPLITK", raising=False)
    monkeypatch.setattr(ops, "_SKINNY_SPLITK", {})
    N, K = 256, 4 * S                      # 4 groups, 4 slices: splitk 4
    _fresh_buffers()
    x64, q, scale, ref, mag = _case(64, N, K)
    mw = ops.Mxfp4Weight(q.to(DEV), scale.to(DEV))
    got = ops.linear(x64.to(DEV), mw)
    assert _C.skinny_splitk("w4", N, K) == 4
    assert ops._SKINNY_WS[0].numel() == 64 * N * 4
    assert not ops._W8_SCRATCH                 # no scratch on this route
    direct = torch.empty(64, N, dtype=torch.bfloat16, device=DEV)
    _C.skinny_gemm_w4(direct, x64.to(DEV), mw.q, mw.scale,
                      ops._SKINNY_WS[0])
    assert torch.equal(got.view(torch.int16), direct.view(torch.int16))
    assert bool(((got.cpu().double() - ref).abs()
                 <= _tol(ref, mag, K)).all())

    g = torch.Generator().manual_seed(65)
    x65 = (torch.randn(65, K, generator=g) * 0.5).bfloat16()
    got65 = ops.linear(x65.to(DEV), mw)
    assert ops._W8_SCRATCH[0].numel() == N * K
    deq = torch.empty(N, K, dtype=torch.float64)
    reference.dequant_mxfp4_rows(deq, q, scale)
    ref65 = x65.double() @ deq.T
    mag65 = x65.double().abs() @ deq.abs().T
    err = (got65.cpu().double() - ref65).abs()
    assert got65.shape == (65, N)
    assert bool((err <= _tol(ref65, mag65, K)).all())
    # quantize_weight reserves the scratch for the largest weight it made
    _fresh_buffers()
    ops.quantize_weight(_weight(N, K, seed=1).to(DEV), fmt="mxfp4")
    ops.quantize_weight(_weight(64, 128, seed=2).to(DEV), fmt="mxfp4")
    assert ops._W8_SCRATCH[0].numel() == N * K


def test_decode_graphs_match_eager_mxfp4_weights():
    """test_decode_graphs_match_eager's recipe on mxfp4 weights."""
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
        model = LlamaModel(cfg, device=DEV, weight_dtype="mxfp4")
        assert isinstance(model.lm_head, ops.Mxfp4Weight)
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
