"""GPU tests of the grouped-GEMM MoE route: the device-side routing/sort
kernel and the grouped GEMM vs their fp32 references, hipGraph
capturability of the Mixtral MoE layer above 128 rows, the engine serving
a graphed bucket above 128, and the route dispatch."""
import pytest
import torch

import kukeon_amd.ops as ops
from kukeon_amd.ops import reference

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

DEV = "cuda:0"
BM = 128  # moe_grouped_gemm's m-tile (GG_BM in moe_grouped.hip)


# ---------------------------------------------------------------- routing

def _route_sort(logits, K, impl):
    T, E = logits.shape
    dev = logits.device
    topk_w = torch.zeros(T, K, dtype=torch.float32, device=dev)
    row_map = torch.full((T * K,), -7, dtype=torch.int32, device=dev)
    inv_map = torch.full((T, K), -7, dtype=torch.int32, device=dev)
    offsets = torch.full((E + 1,), -7, dtype=torch.int32, device=dev)
    impl.moe_route_sort(topk_w, row_map, inv_map, offsets, logits, K)
    return topk_w, row_map, inv_map, offsets


def _check_route_sort(logits, K):
    got = _route_sort(logits.to(DEV), K, ops)
    want = _route_sort(logits.cpu(), K, reference)
    for g, w, name in zip(got[1:], want[1:],
                          ("row_map", "inv_map", "offsets")):
        assert torch.equal(g.cpu(), w), name
    torch.testing.assert_close(got[0].cpu(), want[0], rtol=1e-4, atol=1e-5)


def _logits(T, E, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    # asymmetric column scale; bf16 rounding makes genuine ties, which the
    # lowest-expert-id rule must resolve identically on both sides
    x = torch.randn(T, E, generator=g) * torch.linspace(0.5, 2.0, E)
    return x.to(dtype)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("T,E,K", [(1, 8, 2), (9, 4, 2), (160, 8, 2),
                                   (7, 16, 4)])
def test_route_sort_matches_reference(T, E, K, dtype):
    logits = _logits(T, E, dtype, 100 + T)
    logits[T // 2] = 0.25                        # all-equal row
    _check_route_sort(logits, K)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("case", ["same_k_experts", "first_empty",
                                  "last_single", "multi_chunk"])
def test_route_sort_adversarial(case, dtype):
    T, E, K = 160, 8, 2
    if case == "multi_chunk":
        T = 700                                  # three 256-token chunks
    logits = _logits(T, E, torch.float32, 7)
    if case == "same_k_experts":
        logits[:, 3] += 100.0                    # every token -> {3, 5}
        logits[:, 5] += 50.0
    elif case == "first_empty":
        logits[:, 0] -= 100.0
    elif case == "last_single":
        logits[:, E - 1] -= 100.0
        logits[T - 3, E - 1] += 300.0            # exactly one slot
    logits = logits.to(dtype)
    _check_route_sort(logits, K)
    off = _route_sort(logits.to(DEV), K, ops)[3].cpu()
    if case == "same_k_experts":
        cnt = (off[1:] - off[:-1]).tolist()
        assert cnt == [0, 0, 0, T, 0, T, 0, 0]
    elif case == "first_empty":
        assert int(off[1]) == 0
    elif case == "last_single":
        assert int(off[E]) - int(off[E - 1]) == 1


# ----------------------------------------------------------- grouped GEMM

_COUNTS = {
    # empty first and last expert; 0, 1, BM-1, BM, BM+1, 2*BM+1 all appear
    4: [[0, BM - 1, BM + 1, 0], [0, 1, BM, 0], [0, 2 * BM + 1, 1, 0],
        [0, 0, 2 * BM + 6, 0],                   # all rows in one expert
        # the kernel specialises its tile on <= 32, <= 64 and more rows
        [0, 32, 33, 0], [0, 64, 65, 0]],
    8: [[0, 1, BM - 1, BM, BM + 1, 2 * BM + 1, 0, 0]],
}


def _gemm_cases():
    for E, N, Kd in [(4, 512, 256), (4, 256, 256), (8, 1792, 4096)]:
        for ci, counts in enumerate(_COUNTS[E]):
            for gather in (False, True):
                yield pytest.param(E, N, Kd, counts, gather,
                                   id=f"E{E}-N{N}-K{Kd}-c{ci}-"
                                      f"{'gather' if gather else 'ident'}")


@pytest.mark.parametrize("E,N,Kd,counts,gather", list(_gemm_cases()))
def test_grouped_gemm(E, N, Kd, counts, gather):
    torch.manual_seed(13)
    K = 2
    R = sum(counts)
    offsets = torch.tensor([0] + counts, dtype=torch.int32).cumsum(0).to(
        torch.int32).to(DEV)
    if gather:
        # every token appears K times, shuffled over the slots
        Ta = (R + K - 1) // K
        rows = (torch.arange(R) // K)[torch.randperm(R)]
        a_rows = rows.to(torch.int32).to(DEV)
    else:
        Ta = R + 3                               # a may be longer than out
        rows = torch.arange(R)
        a_rows = None
    a = torch.randn(Ta, Kd, dtype=torch.bfloat16, device=DEV) * 0.5
    # per-column and per-expert scale: asymmetric in every axis
    w = (torch.randn(E, N, Kd, dtype=torch.bfloat16, device=DEV) * 0.05 *
         torch.linspace(0.5, 1.5, N, device=DEV)[None, :, None].bfloat16())

    G = 3                                        # guard rows on both sides
    SENT = -512.0                            # exact in bf16

    def run():
        buf = torch.full((R + 2 * G, N), SENT, dtype=torch.bfloat16,
                         device=DEV)
        ops.moe_grouped_gemm(buf[G:G + R], a, a_rows, w, offsets)
        return buf

    buf = run()
    buf2 = run()
    assert torch.equal(buf, buf2)                # bit-identical run to run
    assert bool((buf[:G] == SENT).all()) and bool((buf[G + R:] == SENT).all())

    src = a[rows.to(DEV)].float()
    ref = torch.empty(R, N, dtype=torch.float32, device=DEV)
    lo = 0
    for e, n in enumerate(counts):
        ref[lo:lo + n] = src[lo:lo + n] @ w[e].float().T
        lo += n
    torch.testing.assert_close(buf[G:G + R].float().cpu(), ref.cpu(),
                               rtol=3e-2, atol=3e-2)


def test_grouped_gemm_rejects_ineligible_shapes():
    a = torch.zeros(4, 96, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(2, 64, 96, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros(4, 64, dtype=torch.bfloat16, device=DEV)
    off = torch.tensor([0, 2, 4], dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        ops.moe_grouped_gemm(out, a, None, w, off)


# ------------------------------------------------------------ module level

@pytest.fixture(scope="module")
def tiny_model():
    from kukeon_amd.engine.config import tiny_mixtral
    from kukeon_amd.models.mixtral import MixtralModel
    torch.manual_seed(1)
    cfg = tiny_mixtral()
    return cfg, MixtralModel(cfg, device=DEV)


def test_moe_forward_captures_above_128_rows(tiny_model):
    cfg, model = tiny_model
    moe = model.layers[0].moe
    T = 160
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(T, cfg.hidden_size, generator=g).bfloat16().to(DEV),
          (torch.randn(T, cfg.hidden_size, generator=g) * 1.5
           ).bfloat16().to(DEV)]
    x_static = xs[0].clone()
    moe._forward_grouped(x_static)               # warm allocator + BLAS
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_static = moe.forward(x_static)
    routes = []
    for x in xs:
        x_static.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        got = y_static.clone()
        eager = moe._forward_grouped(x.clone())
        assert torch.equal(got, eager)
        sparse = moe._forward_sparse(x.clone())
        torch.testing.assert_close(got.float(), sparse.float(), rtol=3e-2,
                                   atol=3e-2)
        routes.append(torch.nn.functional.linear(x, moe.router_w)
                      .float().topk(cfg.top_k_experts).indices.cpu())
    assert not torch.equal(routes[0], routes[1])  # routing really differed


def test_engine_graphed_bucket_above_128(tiny_model):
    from kukeon_amd.engine.config import EngineConfig, SamplingParams
    from kukeon_amd.engine.engine import LLMEngine
    from kukeon_amd.engine.kv_cache import SequenceKV

    cfg, model = tiny_model
    B, NEW = 160, 4
    ecfg = EngineConfig(max_model_len=64, max_sessions=B, num_kv_blocks=2 * B,
                        use_graphs=True, decode_microbatch=4,
                        graph_buckets=(B,))
    engine = LLMEngine(model, cfg, ecfg, device=DEV)
    got = {}
    kvs = []
    for i in range(B):
        kv = SequenceKV(ecfg.block_size)
        kvs.append(kv)
        rid = engine.add_request(
            kv, [1 + i % 97, 2 + i % 89, 3 + i % 7],
            SamplingParams(temperature=0.0, max_new_tokens=NEW))
        got[rid] = []
    steps = 0
    while engine.has_work():
        for o in engine.step():
            got[o.req_id].extend(o.new_tokens)
        steps += 1
        assert steps < 200
    torch.cuda.synchronize()
    assert len(got) == B
    for toks in got.values():
        assert len(toks) == NEW
        assert all(0 <= t < cfg.vocab_size for t in toks)
    assert B in engine.graphs


def test_route_dispatch(tiny_model, monkeypatch):
    from kukeon_amd.models import mixtral
    cfg, model = tiny_model
    moe = model.layers[0].moe
    calls = []
    for name in ("_forward_dense", "_forward_sparse", "_forward_grouped"):
        real = getattr(moe, name)

        def spy(x, _real=real, _name=name):
            calls.append(_name)
            return _real(x)
        monkeypatch.setattr(moe, name, spy)

    def route(T):
        calls.clear()
        x = torch.randn(T, cfg.hidden_size, dtype=torch.bfloat16, device=DEV)
        moe.forward(x)
        torch.cuda.synchronize()
        return list(calls)

    monkeypatch.setattr(mixtral, "_GROUPED_MAX_T", 0)
    assert route(200) == ["_forward_sparse"]
    assert route(64) == ["_forward_dense"]
    monkeypatch.setattr(mixtral, "_GROUPED_MAX_T", 256)
    assert route(200) == ["_forward_grouped"]
    assert route(64) == ["_forward_dense"]
    assert route(300) == ["_forward_sparse"]
