"""Grouped-GEMM MoE route on the CPU reference ops: device-style routing +
stable expert sort vs the eager chain, and MixtralMoE._forward_grouped vs
the sparse route and a naive per-token loop."""
import pytest
import torch
import torch.nn.functional as F

from kukeon_amd.engine.config import tiny_mixtral
from kukeon_amd.models.mixtral import MixtralMoE
from kukeon_amd.ops import reference


def _route_sort(logits, K):
    T, E = logits.shape
    topk_w = torch.empty(T, K, dtype=torch.float32)
    row_map = torch.empty(T * K, dtype=torch.int32)
    inv_map = torch.empty(T, K, dtype=torch.int32)
    offsets = torch.empty(E + 1, dtype=torch.int32)
    reference.moe_route_sort(topk_w, row_map, inv_map, offsets, logits, K)
    return topk_w, row_map, inv_map, offsets


@pytest.mark.parametrize("T,E,K", [(1, 8, 2), (9, 4, 2), (160, 8, 2),
                                   (7, 16, 4)])
def test_route_sort_reference_matches_eager_chain(T, E, K):
    torch.manual_seed(20 + T)
    # asymmetric column scale so an expert-axis mixup cannot pass
    logits = torch.randn(T, E) * torch.linspace(0.5, 2.0, E)
    tie_row = T // 2
    logits[tie_row] = 0.25                       # all-equal row
    topk_w, row_map, inv_map, offsets = _route_sort(logits, K)

    # eager chain; the all-equal row's pick is fixed by hand because topk
    # promises no tie order
    topi = logits.topk(K, dim=-1).indices
    topi[tie_row] = torch.arange(K)
    flat = topi.reshape(-1)
    order = torch.argsort(flat, stable=True)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(order.numel())
    counts = torch.bincount(flat, minlength=E)
    want_off = torch.cat([torch.zeros(1, dtype=torch.long),
                          torch.cumsum(counts, 0)])
    assert torch.equal(row_map.long(), order // K)
    assert torch.equal(inv_map.long(), inv.reshape(T, K))
    assert torch.equal(offsets.long(), want_off)
    assert int(offsets[E]) == T * K

    # the all-equal row selects experts 0..K-1: its slots are the ones of
    # token tie_row inside experts 0..K-1, in that order
    for j in range(K):
        s = int(inv_map[tie_row, j])
        assert int(offsets[j]) <= s < int(offsets[j + 1])
        assert int(row_map[s]) == tie_row

    # softmax -> top-k -> renormalise
    probs = torch.softmax(logits, dim=-1)
    topv = probs.gather(1, topi)
    topv = topv / topv.sum(dim=-1, keepdim=True)
    torch.testing.assert_close(topk_w, topv, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("T", [11, 160])
def test_forward_grouped_cpu(T):
    torch.manual_seed(1)
    cfg = tiny_mixtral()
    moe = MixtralMoE(cfg, "cpu")
    x = torch.randn(T, cfg.hidden_size, dtype=torch.bfloat16)
    grouped = moe._forward_grouped(x.clone())
    sparse = moe._forward_sparse(x.clone())
    torch.testing.assert_close(grouped.float(), sparse.float(), rtol=3e-2,
                               atol=3e-2)

    # naive: every token through its top-k experts, weighted sum
    logits = F.linear(x, moe.router_w).float()
    probs = torch.softmax(logits, -1)
    topv, topi = probs.topk(cfg.top_k_experts, -1)
    topv = topv / topv.sum(-1, keepdim=True)
    ref = torch.zeros(x.shape, dtype=torch.float32)
    for t in range(T):
        for k in range(cfg.top_k_experts):
            e = int(topi[t, k])
            gu = F.linear(x[t:t + 1], moe.gate_up_w[e]).float()
            g, u = gu[:, :moe.inter], gu[:, moe.inter:]
            act = (F.silu(g) * u).to(torch.bfloat16)
            y = F.linear(act, moe.down_w[e]).float()
            ref[t] += float(topv[t, k]) * y[0]
    torch.testing.assert_close(grouped.float(),
                               ref.to(torch.bfloat16).float(),
                               rtol=3e-2, atol=3e-2)


def test_grouped_gemm_reference_empty_experts():
    torch.manual_seed(3)
    E, N, Kd = 4, 64, 64
    counts = [0, 3, 0, 2]
    offsets = torch.tensor([0, 0, 3, 3, 5], dtype=torch.int32)
    a = torch.randn(5, Kd).bfloat16()
    w = (torch.randn(E, N, Kd) * torch.linspace(0.5, 1.5, N)[:, None]
         ).bfloat16()
    out = torch.full((5, N), 7.0, dtype=torch.bfloat16)
    reference.moe_grouped_gemm(out, a, None, w, offsets)
    want = torch.cat([a[0:3].float() @ w[1].float().T,
                      a[3:5].float() @ w[3].float().T])
    torch.testing.assert_close(out.float(), want, rtol=1e-2, atol=1e-2)
    assert sum(counts) == 5
