"""Mixtral-8x7B decoder: Llama attention + MoE MLP with three routes.

Grouped (T > 128 under hipGraph capture, or eager up to _GROUPED_MAX_T):
routing and the expert sort in one device pass, both expert projections as
one grouped GEMM each with per-expert row ranges read from device memory —
static shapes, no host sync, no redundant flops.

Prefill (large T): softmax top-k routing, token permute into expert-sorted
order via the gfx950 HIP permute kernels, per-expert fused gate_up/down
GEMMs through hipBLASLt, weighted un-permute.

Decode (small T): dense-routed — every expert runs the whole batch as one
batched GEMM and the routing weights combine densely. Decode is
weight-bandwidth-bound (all 94 GB of expert weights stream through HBM
per step regardless of routing), so the redundant flops cost nothing while
removing the router host-sync and making the step hipGraph-capturable
(+36% measured on the 32-session config).

Experts are TP-sharded on the intermediate dim (every rank holds a slice
of all 8 experts) so routing stays rank-local and the existing all-reduce
covers the combine — the right trade for one 8-GPU xGMI node where ring
all-reduce is per-link bound.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from kukeon_amd import ops, parallel
from kukeon_amd.engine.config import ModelConfig
from kukeon_amd.models.llama import (AttnMeta, LlamaAttention, _init_weight)

# Largest eager T that takes the grouped-GEMM route (device-side routing +
# one GEMM launch for all experts). From the measured sweep in docs/perf.md:
# above it the per-expert hipBLASLt loop of the sparse route wins. Under
# hipGraph capture the grouped route runs at every T > 128 regardless — the
# sparse route's host sync cannot be captured. 0 turns the route off in
# eager mode.
_GROUPED_MAX_T = int(os.environ.get("KUKEON_MOE_GROUPED_MAX_T", "192"))


class MixtralMoE(nn.Module):
    def __init__(self, cfg: ModelConfig, device):
        super().__init__()
        tp = parallel.tp_size()
        self.ep = parallel.ep_size()
        assert cfg.intermediate_size % tp == 0
        self.E = cfg.num_experts
        self.K = cfg.top_k_experts
        self.inter = cfg.intermediate_size // tp
        self.router_w = _init_weight((self.E, cfg.hidden_size), device)
        gate_up = torch.empty(self.E, 2 * self.inter, cfg.hidden_size,
                              dtype=torch.bfloat16,
                              device=device).normal_(0, 0.02)
        down = torch.empty(self.E, cfg.hidden_size, self.inter,
                           dtype=torch.bfloat16,
                           device=device).normal_(0, 0.02)
        if self.ep > 1:
            # expert-parallel: this rank OWNS E/ep whole experts (full
            # intermediate dim); tokens travel to their experts over
            # all-to-all. Full-size init then slice keeps every rank's
            # RNG stream identical to the single-rank module, so EP is
            # numerically the same model.
            assert tp == 1 and self.E % self.ep == 0
            self.e_local = self.E // self.ep
            e0 = parallel.ep_rank() * self.e_local
            gate_up = gate_up[e0: e0 + self.e_local].contiguous()
            down = down[e0: e0 + self.e_local].contiguous()
        else:
            self.e_local = self.E
        self.gate_up_w = nn.Parameter(gate_up, requires_grad=False)
        self.down_w = nn.Parameter(down, requires_grad=False)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        T = x.shape[0]
        if self.ep > 1:
            return self._forward_ep(x)
        if x.is_cuda and T <= 128:
            return self._forward_dense(x)
        if (x.is_cuda and self._grouped_eligible(x)
                and (T <= _GROUPED_MAX_T
                     or torch.cuda.is_current_stream_capturing())):
            return self._forward_grouped(x)
        return self._forward_sparse(x)

    def _grouped_eligible(self, x: torch.Tensor) -> bool:
        # the shapes moe_route_sort / moe_grouped_gemm accept
        return (x.dtype == torch.bfloat16 and x.shape[1] % 64 == 0
                and self.inter % 64 == 0 and self.E <= 32
                and self.K <= min(4, self.E))

    def _expert_mlp(self, xs: torch.Tensor, e: int) -> torch.Tensor:
        gu = F.linear(xs, self.gate_up_w[e])
        act = torch.empty(xs.shape[0], self.inter, dtype=xs.dtype,
                          device=xs.device)
        ops.silu_mul(act, gu)
        return F.linear(act, self.down_w[e])

    def _forward_ep(self, x: torch.Tensor) -> torch.Tensor:
        """Expert-parallel MoE (BASELINE config 5: expert all-to-all over
        xGMI): route each (token, expert) pair to the rank owning that
        expert, compute there, route back, combine with the gate weights
        locally. Two all-to-alls per layer; splits are data-dependent so
        this path is eager (not hipGraph-captured).

        NOTE: the all-to-alls make every MoE forward a COLLECTIVE — all
        EP ranks must step in lockstep (the bench's TurnDriver rounds
        satisfy this: equal session counts and fixed prompt/decode
        lengths give identical step sequences). Free-running engines per
        rank would need a synchronized scheduler; that is a round-2 item
        if EP serving (rather than TP) is chosen for production MoE."""
        import torch.distributed as dist
        T, H = x.shape
        ep = self.ep
        logits = F.linear(x, self.router_w).float()
        probs = torch.softmax(logits, dim=-1)
        topv, topi = probs.topk(self.K, dim=-1)
        topv = topv / topv.sum(dim=-1, keepdim=True)
        flat_expert = topi.reshape(-1)                      # [T*K]
        dest = flat_expert // self.e_local                  # owner rank
        order = torch.argsort(dest, stable=True)
        send_rows = x[order // self.K].contiguous()
        send_eid = (flat_expert[order] % self.e_local).contiguous()
        in_splits = torch.bincount(dest, minlength=ep)
        out_splits = torch.empty_like(in_splits)
        dist.all_to_all_single(out_splits, in_splits.contiguous())
        isl = in_splits.tolist()
        osl = out_splits.tolist()
        nrecv = int(sum(osl))
        recv_rows = torch.empty(nrecv, H, dtype=x.dtype, device=x.device)
        recv_eid = torch.empty(nrecv, dtype=send_eid.dtype, device=x.device)
        dist.all_to_all_single(recv_rows, send_rows, osl, isl)
        dist.all_to_all_single(recv_eid, send_eid, osl, isl)
        # group the received tokens by local expert, run each expert once
        order2 = torch.argsort(recv_eid, stable=True)
        grouped = recv_rows[order2]
        counts = torch.bincount(recv_eid, minlength=self.e_local).tolist()
        processed = torch.empty_like(grouped)
        start = 0
        for e in range(self.e_local):
            n = counts[e]
            if n == 0:
                continue
            processed[start: start + n] = self._expert_mlp(
                grouped[start: start + n], e)
            start += n
        # un-group to the received order, send results home
        unsorted = torch.empty_like(processed)
        unsorted[order2] = processed
        back = torch.empty(T * self.K, H, dtype=x.dtype, device=x.device)
        dist.all_to_all_single(back, unsorted, isl, osl)
        # back[i] answers send slot i (= expanded slot order[i])
        expanded = torch.empty_like(back)
        expanded[order] = back
        out = (expanded.view(T, self.K, H).float() *
               topv.unsqueeze(-1)).sum(dim=1)
        return out.to(x.dtype)

    def _forward_dense(self, x: torch.Tensor) -> torch.Tensor:
        """Decode path: run EVERY expert on the whole (small) batch as one
        batched GEMM and combine with the dense routing-weight matrix.
        Decode is weight-bandwidth-bound — all 8 experts' weights stream
        through HBM regardless — so the 8x redundant flops are free, and
        this path has no router host-sync, no permute, and is
        hipGraph-capturable (the sparse path's per-expert loop is neither).
        """
        T = x.shape[0]
        logits = F.linear(x, self.router_w)                    # [T, E]
        # fused router: softmax top-K renorm scatter in ONE launch,
        # reading the bf16 logits directly — no .float() cast pass (the
        # eager chain was ~5 kernels/layer, ~6% of the Mixtral decode
        # run — profiles/r02_mixtral_stats.txt)
        wdense = torch.empty(T, self.E, dtype=torch.float32,
                             device=x.device)
        ops.moe_router_weights(wdense, logits, self.K)
        x_rep = x.unsqueeze(0).expand(self.E, T, x.shape[1])
        gu = torch.bmm(x_rep, self.gate_up_w.transpose(1, 2))  # [E,T,2I]
        act = torch.empty(self.E * T, self.inter, dtype=x.dtype,
                          device=x.device)
        ops.silu_mul(act, gu.reshape(self.E * T, 2 * self.inter))
        y = torch.bmm(act.view(self.E, T, self.inter),
                      self.down_w.transpose(1, 2))             # [E,T,H]
        # fused combine: skips zero-weight experts' rows entirely
        out = torch.empty(T, x.shape[1], dtype=x.dtype, device=x.device)
        ops.moe_dense_combine(out, y.view(self.E, T, x.shape[1]), wdense)
        return parallel.tp_all_reduce(out)

    def _forward_sparse(self, x: torch.Tensor) -> torch.Tensor:
        T = x.shape[0]
        logits = F.linear(x, self.router_w).float()           # [T, E]
        probs = torch.softmax(logits, dim=-1)
        topv, topi = probs.topk(self.K, dim=-1)               # [T, K]
        topv = topv / topv.sum(dim=-1, keepdim=True)
        flat_expert = topi.reshape(-1)                        # [T*K]
        order = torch.argsort(flat_expert, stable=True)
        inv = torch.empty_like(order)
        inv[order] = torch.arange(order.numel(), device=x.device)
        row_map = (order // self.K).to(torch.int32)           # expanded->token
        gathered = torch.empty(T * self.K, x.shape[1], dtype=x.dtype,
                               device=x.device)
        ops.moe_gather_tokens(gathered, x, row_map)
        counts = torch.bincount(flat_expert, minlength=self.E)
        counts_l = counts.tolist()                            # host sync (eager path)
        out_expanded = torch.empty_like(gathered)
        start = 0
        for e in range(self.E):
            n = counts_l[e]
            if n == 0:
                continue
            xs = gathered[start: start + n]
            gu = F.linear(xs, self.gate_up_w[e])
            act = torch.empty(n, self.inter, dtype=x.dtype, device=x.device)
            ops.silu_mul(act, gu)
            out_expanded[start: start + n] = F.linear(act, self.down_w[e])
            start += n
        out = torch.empty_like(x)
        ops.moe_scatter_tokens(out, out_expanded,
                               inv.reshape(T, self.K).to(torch.int32),
                               topv.float().contiguous(), self.K)
        return parallel.tp_all_reduce(out)

    def _grouped_mlp(self, a: torch.Tensor, a_rows, offsets: torch.Tensor,
                     rows: int) -> torch.Tensor:
        """gate_up -> SwiGLU -> down for `rows` expert-sorted slots, one
        grouped-GEMM launch per projection. Slot r reads a[a_rows[r]]
        (a[r] when a_rows is None); expert e owns the slots
        [offsets[e], offsets[e+1]), read on the device."""
        gu = torch.empty(rows, 2 * self.inter, dtype=a.dtype, device=a.device)
        ops.moe_grouped_gemm(gu, a, a_rows, self.gate_up_w, offsets)
        act = torch.empty(rows, self.inter, dtype=a.dtype, device=a.device)
        ops.silu_mul(act, gu)
        y = torch.empty(rows, self.down_w.shape[1], dtype=a.dtype,
                        device=a.device)
        ops.moe_grouped_gemm(y, act, None, self.down_w, offsets)
        return y

    def _forward_grouped(self, x: torch.Tensor) -> torch.Tensor:
        """Static-shape sparse route: routing and the expert sort stay on
        the device and both projections run as one grouped GEMM over all
        experts, so there is no host sync, every allocation is fixed by T,
        and the layer is hipGraph-capturable at any T — without the dense
        route's E/K-fold redundant flops."""
        T = x.shape[0]
        logits = F.linear(x, self.router_w)                   # [T, E] bf16
        topk_w = torch.empty(T, self.K, dtype=torch.float32, device=x.device)
        row_map = torch.empty(T * self.K, dtype=torch.int32, device=x.device)
        inv_map = torch.empty(T, self.K, dtype=torch.int32, device=x.device)
        offsets = torch.empty(self.E + 1, dtype=torch.int32, device=x.device)
        ops.moe_route_sort(topk_w, row_map, inv_map, offsets, logits, self.K)
        # the gather happens in the gate_up A-tile load: no [T*K,H] copy
        y = self._grouped_mlp(x, row_map, offsets, T * self.K)
        out = torch.empty_like(x)
        ops.moe_scatter_tokens(out, y, inv_map, topk_w, self.K)
        return parallel.tp_all_reduce(out)


class MixtralLayer(nn.Module):
    def __init__(self, cfg: ModelConfig, layer_idx: int, device):
        super().__init__()
        self.input_norm = nn.Parameter(
            torch.ones(cfg.hidden_size, dtype=torch.bfloat16, device=device),
            requires_grad=False)
        self.post_norm = nn.Parameter(
            torch.ones(cfg.hidden_size, dtype=torch.bfloat16, device=device),
            requires_grad=False)
        self.attn = LlamaAttention(cfg, layer_idx, device)
        self.moe = MixtralMoE(cfg, device)
        self.eps = cfg.rms_eps

    def forward(self, x, residual, cos_sin, kc, vc, meta):
        if residual is None:
            residual = x
            h = torch.empty_like(x)
            ops.rmsnorm(h, x, self.input_norm, self.eps)
        else:
            ops.fused_add_rmsnorm(x, residual, self.input_norm, self.eps)
            h = x
        attn_out = self.attn.forward_pre_o(h, cos_sin, kc, vc, meta)
        h = ops.linear_add_rmsnorm(attn_out, self.attn.o_w, residual,
                                   self.post_norm, self.eps)
        h = self.moe.forward(h)
        return h, residual


class MixtralModel(nn.Module):
    def __init__(self, cfg: ModelConfig, device="cuda", weight_dtype=None):
        super().__init__()
        from kukeon_amd.models.llama import LlamaModel, resolve_weight_dtype
        self.weight_dtype = resolve_weight_dtype(weight_dtype)
        if self.weight_dtype != "bf16":
            # the expert weights run through bmm and the grouped GEMM,
            # which read bf16 only; quantising them is separate work
            raise ValueError(
                "MixtralModel supports weight_dtype='bf16' only: "
                f"{self.weight_dtype} expert weights (bmm / grouped GEMM) "
                "are not implemented")
        self.cfg = cfg
        self.device_ = torch.device(device)
        torch.manual_seed(43)
        self.embed = _init_weight((cfg.vocab_size, cfg.hidden_size),
                                  self.device_)
        self.layers = nn.ModuleList(
            [MixtralLayer(cfg, i, self.device_)
             for i in range(cfg.num_layers)])
        self.final_norm = nn.Parameter(
            torch.ones(cfg.hidden_size, dtype=torch.bfloat16,
                       device=self.device_), requires_grad=False)
        self.lm_head = _init_weight((cfg.vocab_size, cfg.hidden_size),
                                    self.device_)
        # reuse the Llama RoPE table builder
        self.cos_sin = LlamaModel._build_rope_table(self).to(self.device_)

    # EP lockstep accounting: every full forward touches each MoE
    # layer's collectives exactly once, so EP ranks stay paired as long
    # as their PASS COUNTS match — a work-free rank contributes a
    # participation pass (collectives only) instead of a real forward.
    pass_count = 0

    def forward(self, input_ids, kv_k, kv_v, meta: AttnMeta) -> torch.Tensor:
        MixtralModel.pass_count += 1
        x = F.embedding(input_ids.long(), self.embed)
        residual = None
        for i, layer in enumerate(self.layers):
            x, residual = layer.forward(x, residual, self.cos_sin, kv_k[i],
                                        kv_v[i], meta)
        ops.fused_add_rmsnorm(x, residual, self.final_norm, self.cfg.rms_eps)
        return x

    def participate(self) -> None:
        """One collective-only pass: serve this rank's experts for the
        other EP ranks' tokens without any local batch (VERDICT r01
        item 9 — the cross-rank lockstep EP serving scheduler). Runs the
        same all-to-all sequence as a real forward, with zero local
        tokens."""
        MixtralModel.pass_count += 1
        empty = torch.empty(0, self.cfg.hidden_size, dtype=torch.bfloat16,
                            device=self.device_)
        for layer in self.layers:
            layer.moe.forward(empty)

    def compute_logits(self, hidden: torch.Tensor) -> torch.Tensor:
        return F.linear(hidden, self.lm_head)
