"""Plain-PyTorch fp32 reference implementations of every HIP op.

These are the numerics oracles for the GPU test suite (each HIP kernel is
compared against the fp32 reference of the same op, per the repo test
contract) and the CPU execution path for control-plane / scheduler tests on
GPU-less hosts.  They are never used on a CUDA device — `kukeon_amd.ops`
fails loudly there if the native extension is missing.
"""
from __future__ import annotations

import torch


def rmsnorm(out: torch.Tensor, input: torch.Tensor, weight: torch.Tensor,
            eps: float) -> None:
    x = input.float()
    rs = torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
    out.copy_((x * rs * weight.float()).to(out.dtype))


def fused_add_rmsnorm(input: torch.Tensor, residual: torch.Tensor,
                      weight: torch.Tensor, eps: float) -> None:
    r = (residual.float() + input.float())
    residual.copy_(r.to(residual.dtype))
    # match the kernel: it normalizes the bf16-rounded residual it wrote
    r = residual.float()
    rs = torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + eps)
    input.copy_((r * rs * weight.float()).to(input.dtype))


def silu_mul(out: torch.Tensor, gate_up: torch.Tensor) -> None:
    I = out.shape[-1]
    g = gate_up[..., :I].float()
    u = gate_up[..., I:].float()
    out.copy_((torch.nn.functional.silu(g) * u).to(out.dtype))


def _rotate(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    # NEOX half-rotation; x [T, H, D], cos/sin [T, D/2]
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    c = cos.unsqueeze(1)
    s = sin.unsqueeze(1)
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def rope_kv_append(qkv: torch.Tensor, k_cache: torch.Tensor,
                   v_cache: torch.Tensor, cos_sin: torch.Tensor,
                   positions: torch.Tensor, slot_mapping: torch.Tensor,
                   num_q_heads: int, num_kv_heads: int, head_dim: int,
                   block_table=None) -> None:
    T = qkv.shape[0]
    D = head_dim
    half = D // 2
    q = qkv[:, : num_q_heads * D].view(T, num_q_heads, D).float()
    k = qkv[:, num_q_heads * D: (num_q_heads + num_kv_heads) * D].view(
        T, num_kv_heads, D).float()
    v = qkv[:, (num_q_heads + num_kv_heads) * D:].view(T, num_kv_heads, D)
    cs = cos_sin[positions.long().clamp_min(0)]
    cos, sin = cs[:, :half], cs[:, half:]
    qr = _rotate(q, cos, sin).to(qkv.dtype)
    kr = _rotate(k, cos, sin).to(qkv.dtype)
    # inactive decode rows (pos < 0) are skipped entirely, like the kernel
    act = (positions >= 0).view(T, 1)
    qkv[:, : num_q_heads * D] = torch.where(
        act, qr.reshape(T, -1), qkv[:, : num_q_heads * D])
    qkv[:, num_q_heads * D: (num_q_heads + num_kv_heads) * D] = torch.where(
        act, kr.reshape(T, -1),
        qkv[:, num_q_heads * D: (num_q_heads + num_kv_heads) * D])
    BS = k_cache.shape[2]
    fp8 = k_cache.dtype == torch.uint8
    if fp8:
        kr = kr.float().to(torch.float8_e4m3fn).view(torch.uint8)
        v = v.float().to(torch.float8_e4m3fn).view(torch.uint8)
    table_mode = block_table is not None and block_table.dim() == 2
    for t in range(T):
        if table_mode:
            pos_t = int(positions[t])
            if pos_t < 0:
                continue
            slot = int(block_table[t, pos_t // BS]) * BS + pos_t % BS
        else:
            slot = int(slot_mapping[t])
            if slot < 0:
                continue
        blk, off = slot // BS, slot % BS
        k_cache[blk, :, off] = kr[t]
        v_cache[blk, :, off] = v[t]


def kv_copy_blocks(k_cache: torch.Tensor, v_cache: torch.Tensor,
                   src: torch.Tensor, dst: torch.Tensor) -> None:
    """cache[:, dst] = cache[:, src] on [L, NB, Hk, BS, D] caches."""
    assert k_cache.shape == v_cache.shape and src.shape == dst.shape
    if src.numel() == 0:
        return
    k_cache[:, dst.long()] = k_cache[:, src.long()]
    v_cache[:, dst.long()] = v_cache[:, src.long()]


def _check_swap_args(k_cache, v_cache, blocks, staging) -> None:
    assert k_cache.shape == v_cache.shape and k_cache.dtype == v_cache.dtype
    L, _, Hk, BS, D = k_cache.shape
    assert staging.dim() == 6 and tuple(staging.shape[1:]) == \
        (2, L, Hk, BS, D) and staging.dtype == k_cache.dtype
    assert blocks.dim() == 1 and blocks.numel() <= staging.shape[0]


def kv_pack_blocks(k_cache: torch.Tensor, v_cache: torch.Tensor,
                   blocks: torch.Tensor, staging: torch.Tensor) -> None:
    """staging[i, s, l] = cache_s[l, blocks[i]] on [L, NB, Hk, BS, D] caches
    and a [cap, 2, L, Hk, BS, D] staging buffer."""
    _check_swap_args(k_cache, v_cache, blocks, staging)
    n = blocks.numel()
    if n == 0:
        return
    idx = blocks.long()
    staging[:n, 0] = k_cache[:, idx].transpose(0, 1)
    staging[:n, 1] = v_cache[:, idx].transpose(0, 1)


def kv_unpack_blocks(staging: torch.Tensor, k_cache: torch.Tensor,
                     v_cache: torch.Tensor, blocks: torch.Tensor) -> None:
    """cache_s[l, blocks[i]] = staging[i, s, l]; the inverse of
    kv_pack_blocks for distinct blocks."""
    _check_swap_args(k_cache, v_cache, blocks, staging)
    n = blocks.numel()
    if n == 0:
        return
    idx = blocks.long()
    k_cache[:, idx] = staging[:n, 0].transpose(0, 1)
    v_cache[:, idx] = staging[:n, 1].transpose(0, 1)


def _gather_kv(cache: torch.Tensor, block_table: torch.Tensor, ctx: int,
               b: int) -> torch.Tensor:
    """-> [ctx, Hk, D] from paged cache [NB, Hk, BS, D] (bf16 or fp8)."""
    BS = cache.shape[2]
    nb = (ctx + BS - 1) // BS
    blocks = block_table[b, :nb].long()
    flat = cache[blocks]                      # [nb, Hk, BS, D]
    if flat.dtype == torch.uint8:
        flat = flat.view(torch.float8_e4m3fn).float()
    flat = flat.permute(0, 2, 1, 3).reshape(nb * BS, cache.shape[1], -1)
    return flat[:ctx]


def paged_attention(out: torch.Tensor, q: torch.Tensor, k_cache: torch.Tensor,
                    v_cache: torch.Tensor, block_table: torch.Tensor,
                    seq_lens: torch.Tensor, q_offset: int, num_splits: int,
                    scale: float, tmp_out=None, tmp_ml=None) -> None:
    B = q.shape[0]
    Hk, BS, D = k_cache.shape[1], k_cache.shape[2], k_cache.shape[3]
    Hq = out.shape[1] // D
    G = Hq // Hk
    qv = q.view(B, -1)[:, q_offset: q_offset + Hq * D].view(B, Hq, D).float()
    for b in range(B):
        ctx = int(seq_lens[b])
        if ctx <= 0:
            # inactive decode row: write zeros so downstream logits stay
            # finite (the row's sample is discarded by the advance guard,
            # but NaNs from uninitialized memory would crash the CPU
            # sampler's multinomial)
            out.view(B, -1)[b] = 0
            continue
        k = _gather_kv(k_cache, block_table, ctx, b).float()  # [ctx,Hk,D]
        v = _gather_kv(v_cache, block_table, ctx, b).float()
        for h in range(Hq):
            hk = h // G
            s = (k[:, hk] @ qv[b, h]) * scale                  # [ctx]
            p = torch.softmax(s, dim=-1)
            o = p @ v[:, hk]                                   # [D]
            out.view(B, Hq, D)[b, h] = o.to(out.dtype)


def paged_attention_rope(out: torch.Tensor, qkv: torch.Tensor,
                         k_cache: torch.Tensor, v_cache: torch.Tensor,
                         cos_sin: torch.Tensor, positions: torch.Tensor,
                         block_table: torch.Tensor, seq_lens: torch.Tensor,
                         num_q_heads: int, num_kv_heads: int,
                         num_splits: int, scale: float, tmp_out=None,
                         tmp_ml=None) -> None:
    """rope_kv_append (table mode) + paged_attention on a copy of `qkv`,
    which the fused op leaves untouched."""
    rot = qkv.clone()
    rope_kv_append(rot, k_cache, v_cache, cos_sin, positions, None,
                   num_q_heads, num_kv_heads, k_cache.shape[3],
                   block_table=block_table)
    paged_attention(out, rot, k_cache, v_cache, block_table, seq_lens, 0,
                    num_splits, scale, tmp_out, tmp_ml)


TILE_COLS = 2 + 16   # n_rows, n_prefix_blocks, up to 16 member rows


def check_prefix_tiles(tiles: torch.Tensor, group: int) -> None:
    """The part of the shared-prefix contract that needs only the tiles
    (on the host): shape, and n_rows <= 16 // group in every tile."""
    if tiles.dim() != 2 or tiles.shape[1] != TILE_COLS or \
            tiles.dtype != torch.int32:
        raise ValueError("tiles must be int32 [T, 2 + 16]")
    width = 16 // group
    for t, row in enumerate(tiles.tolist()):
        if not 0 <= row[0] <= width:
            raise ValueError(f"tile {t} has {row[0]} rows, a tile holds at "
                             f"most 16 // {group} = {width}")
        if row[0] and row[1] < 0:
            raise ValueError(f"tile {t} has a negative prefix length")


def _check_shared_prefix(block_table, seq_lens, last_pos, prefix_blocks,
                         tiles, group: int, nrows: int, block: int) -> None:
    """Everything ops.paged_attention_shared leaves to its caller, checked:
    raises ValueError at the first violation. `last_pos[b]` is the highest
    position row b attends to."""
    check_prefix_tiles(tiles, group)
    want = [0] * nrows
    seen = set()
    for t, row in enumerate(tiles.tolist()):
        n, npb, members = row[0], row[1], row[2:2 + row[0]]
        if n == 0:
            continue
        first = members[0]
        for r in members:
            if not 0 <= r < nrows:
                raise ValueError(f"tile {t}: row {r} out of range")
            if r in seen:
                raise ValueError(f"row {r} is in more than one tile")
            seen.add(r)
            if int(seq_lens[r]) <= 0:
                raise ValueError(f"tile {t}: member row {r} is not live")
            if npb * block > int(last_pos[r]):
                raise ValueError(
                    f"tile {t}: {npb} prefix blocks reach the newest token "
                    f"of row {r} (position {int(last_pos[r])})")
            if npb > block_table.shape[1] or not torch.equal(
                    block_table[r, :npb], block_table[first, :npb]):
                raise ValueError(f"tile {t}: the block table of row {r} "
                                 "does not begin with the tile's prefix")
            want[r] = npb
    got = prefix_blocks[:nrows].tolist()
    if got != want:
        raise ValueError(f"prefix_blocks {got} disagrees with the tiles, "
                         f"which give {want}")


def paged_attention_shared(out, q, k_cache, v_cache, block_table, seq_lens,
                           q_offset: int, num_splits: int, scale: float,
                           tmp_out, tmp_ml, prefix_blocks, tiles,
                           prefix_splits: int) -> None:
    """paged_attention after a strict check of the shared-prefix metadata:
    sharing only changes which kernel reads which block, so the reference
    result is the unshared one, exactly."""
    B = q.shape[0]
    G = (out.shape[1] // k_cache.shape[3]) // k_cache.shape[1]
    _check_shared_prefix(block_table, seq_lens, seq_lens[:B] - 1,
                         prefix_blocks, tiles, G, B, k_cache.shape[2])
    paged_attention(out, q, k_cache, v_cache, block_table, seq_lens, q_offset,
                    num_splits, scale, tmp_out, tmp_ml)


def paged_attention_rope_shared(out, qkv, k_cache, v_cache, cos_sin,
                                positions, block_table, seq_lens,
                                num_q_heads: int, num_kv_heads: int,
                                num_splits: int, scale: float, tmp_out,
                                tmp_ml, prefix_blocks, tiles,
                                prefix_splits: int) -> None:
    """paged_attention_rope after the same strict check; the token being
    appended (at positions[b]) must lie past the prefix."""
    B = qkv.shape[0]
    _check_shared_prefix(block_table, seq_lens, positions[:B],
                         prefix_blocks, tiles, num_q_heads // num_kv_heads,
                         B, k_cache.shape[2])
    paged_attention_rope(out, qkv, k_cache, v_cache, cos_sin, positions,
                         block_table, seq_lens, num_q_heads, num_kv_heads,
                         num_splits, scale, tmp_out, tmp_ml)


def prefill_attention(out: torch.Tensor, q: torch.Tensor,
                      k_cache: torch.Tensor, v_cache: torch.Tensor,
                      block_table: torch.Tensor, seq_lens: torch.Tensor,
                      q_starts: torch.Tensor, qb_seq=None, qb_start=None,
                      q_offset: int = 0, scale: float = 1.0) -> None:
    """Varlen causal attention where queries are the tail of each sequence.

    q: [T_total, q_stride] packed new tokens over all sequences (row i of
    sequence s is absolute position q_starts[s] + i); KV (including the new
    tokens, already appended) lives in the paged cache; seq_lens[s] is the
    total context after append. out: [T_total, Hq*D].
    """
    Hk, BS, D = k_cache.shape[1], k_cache.shape[2], k_cache.shape[3]
    Hq = out.shape[1] // D
    G = Hq // Hk
    nseq = seq_lens.shape[0]
    for s in range(nseq):
        ctx = int(seq_lens[s])
        start = int(q_starts[s, 0])
        row = int(q_starts[s, 1])
        qlen = ctx - start
        if qlen <= 0:
            continue
        k = _gather_kv(k_cache, block_table, ctx, s).float()
        v = _gather_kv(v_cache, block_table, ctx, s).float()
        qs = q[row: row + qlen, q_offset: q_offset + Hq * D].view(
            qlen, Hq, D).float()
        pos = torch.arange(start, ctx)
        kvpos = torch.arange(ctx)
        mask = kvpos[None, :] <= pos[:, None]                  # [qlen, ctx]
        for h in range(Hq):
            hk = h // G
            sc = (qs[:, h] @ k[:, hk].T) * scale               # [qlen, ctx]
            sc = sc.masked_fill(~mask, float("-inf"))
            p = torch.softmax(sc, dim=-1)
            o = p @ v[:, hk]
            out[row: row + qlen].view(qlen, Hq, D)[:, h] = o.to(out.dtype)
        pass


def sample(tokens: torch.Tensor, logits: torch.Tensor, temps: torch.Tensor,
           top_k: torch.Tensor, top_p: torch.Tensor, seed: torch.Tensor,
           workspace=None) -> None:
    """Reference sampler. Greedy rows match the kernel exactly; stochastic
    rows draw from the same masked distribution (the GPU test checks the
    distribution, not the draw)."""
    B, V = logits.shape
    lg = logits.float()
    for b in range(B):
        T = float(temps[b])
        row = lg[b]
        if T <= 0:
            tokens[b] = int(torch.argmax(row))
            continue
        k = int(top_k[b])
        p = float(top_p[b])
        probs = torch.softmax((row - row.max()) / T, dim=-1)
        keep = torch.ones(V, dtype=torch.bool)
        if 0 < k < V:
            th = torch.topk(row, k).values.min()
            keep &= row >= th
        if 0 < p < 1:
            srt, idx = torch.sort(probs, descending=True)
            cum = torch.cumsum(srt, 0)
            cut = int(torch.searchsorted(cum, p).clamp(max=V - 1))
            keep2 = torch.zeros(V, dtype=torch.bool)
            keep2[idx[: cut + 1]] = True
            keep &= keep2
        probs = probs * keep
        probs = probs / probs.sum()
        tokens[b] = int(torch.multinomial(probs, 1))
    seed += 1


def linear_add_rmsnorm(x, w, residual, norm_weight, eps: float):
    h = torch.nn.functional.linear(x, w)
    fused_add_rmsnorm(h, residual, norm_weight, eps)
    return h


E4M3_MAX = 448.0


def quantize_fp8_rows(q: torch.Tensor, scale: torch.Tensor,
                      w: torch.Tensor) -> None:
    """Per-output-row fp8 weight quantisation: scale[n] = amax_n / 448
    (1 for an all-zero row), q = rne_e4m3(w / scale) as uint8 e4m3fn."""
    wf = w.float()
    amax = wf.abs().amax(dim=1)
    s = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax))
    scale.copy_(s)
    # |w / s| <= 448 up to one rounding of the quotient; the clamp keeps
    # that rounding away from the NaN encoding, like the kernel's
    v = (wf / s[:, None]).clamp_(-E4M3_MAX, E4M3_MAX)
    q.copy_(v.to(torch.float8_e4m3fn).view(torch.uint8))


def dequant_fp8_rows(out: torch.Tensor, q: torch.Tensor,
                     scale: torch.Tensor) -> None:
    out.copy_((q.view(torch.float8_e4m3fn).float() *
               scale[:, None]).to(out.dtype))


def linear_w8(x: torch.Tensor, q: torch.Tensor,
              scale: torch.Tensor) -> torch.Tensor:
    """x @ deq(q, scale)^T in f32 on the exact (unrounded) dequantised
    weight, rounded once to x's dtype."""
    wf = q.view(torch.float8_e4m3fn).float() * scale[:, None]
    return (x.float() @ wf.T).to(x.dtype)


# ---- MXFP4 (OCP MX: e2m1 codes, one e8m0 scale per 32 along K) ----
# magnitude of e2m1 code & 7
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
MX_BLOCK = 32


def quantize_mxfp4_rows(q: torch.Tensor, scale: torch.Tensor,
                        w: torch.Tensor) -> None:
    """The project's MXFP4 quantisation rule, which the GPU kernel matches
    bit for bit. w bf16 [N, K], K % 32 == 0; q uint8 [N, K/2] (element 2j
    in the low nibble, 2j+1 in the high one), scale uint8 [N, K/32].

    Per block of 32: the scale byte is floor(log2 amax) - 2 + 127 clamped
    to [1, 254] (127 for an all-zero block), so the block's largest element
    lands on 4 or 6. floor(log2) is read off amax's exponent field: bf16
    and f32 share it, and a subnormal amax clamps to 1 either way. With
    X = 2^(byte - 127), |w| / X is exact in f32 and rounds to the nearest
    of the eight magnitudes, ties to the even code, above 6 to 6."""
    N, K = w.shape
    assert K % MX_BLOCK == 0
    wf = w.float().view(N, K // MX_BLOCK, MX_BLOCK)
    amax = wf.abs().amax(dim=2)
    ebits = (amax.contiguous().view(torch.int32) >> 23) & 0xFF
    byte = torch.where(amax > 0, (ebits - 2).clamp(1, 254),
                       torch.full_like(ebits, 127))
    scale.copy_(byte.to(torch.uint8))
    X = torch.pow(2.0, (byte - 127).double()).float()
    v = wf.abs() / X[:, :, None]
    # midpoints of the grid; a tie goes to the even code (the one whose
    # mantissa bit is clear), hence > at the odd-below and >= at the
    # even-above midpoints
    code = ((v > 0.25).int() + (v >= 0.75).int() + (v > 1.25).int()
            + (v >= 1.75).int() + (v > 2.5).int() + (v >= 3.5).int()
            + (v > 5.0).int())
    sign = (w.view(torch.int16).int() >> 12) & 8
    code = (code.view(N, K) | sign).to(torch.uint8)
    q.copy_(code[:, 0::2] | (code[:, 1::2] << 4))


def _mxfp4_values(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """The exact f32 weight [N, K] an MXFP4 (q, scale) pair stands for."""
    N, K = q.shape[0], q.shape[1] * 2
    code = torch.stack([q & 0xF, q >> 4], dim=2).view(N, K).long()
    mag = torch.tensor(E2M1_VALUES, dtype=torch.float32,
                       device=q.device)[code & 7]
    val = torch.where((code & 8) != 0, -mag, mag)
    X = torch.pow(2.0, (scale.int() - 127).double()).float()
    return (val.view(N, K // MX_BLOCK, MX_BLOCK) * X[:, :, None]).view(N, K)


def dequant_mxfp4_rows(out: torch.Tensor, q: torch.Tensor,
                       scale: torch.Tensor) -> None:
    """out[n, k] = value(code[n, k]) * 2^(scale[n, k // 32] - 127): exact
    in bf16 while the result is a normal number."""
    out.copy_(_mxfp4_values(q, scale).to(out.dtype))


def linear_w4(x: torch.Tensor, q: torch.Tensor,
              scale: torch.Tensor) -> torch.Tensor:
    """x @ deq(q, scale)^T in f32 on the exact dequantised weight, rounded
    once to x's dtype."""
    return (x.float() @ _mxfp4_values(q, scale).T).to(x.dtype)


def decode_advance(ids, pos, seq_lens, tokens, ring, counter) -> None:
    step = int(counter[0])
    B = ids.shape[0]
    for b in range(B):
        if int(seq_lens[b]) > 0:
            ids[b] = tokens[b]
            pos[b] += 1
            seq_lens[b] += 1
            ring[step * B + b] = tokens[b]
    counter[0] = step + 1


def moe_gather_tokens(out: torch.Tensor, input: torch.Tensor,
                      row_map: torch.Tensor) -> None:
    out.copy_(input[row_map.long()])


def moe_scatter_tokens(out: torch.Tensor, input: torch.Tensor,
                       inv_map: torch.Tensor, weights: torch.Tensor,
                       top_k: int) -> None:
    T = out.shape[0]
    acc = (input[inv_map.long()].float() *
           weights.unsqueeze(-1)).sum(dim=1)  # [T, H]
    out.copy_(acc.to(out.dtype))

def moe_router_weights(wdense: torch.Tensor, logits: torch.Tensor,
                       K: int) -> None:
    # accepts bf16 or fp32 logits, like the HIP kernel
    probs = torch.softmax(logits.float(), dim=-1)
    topv, topi = probs.topk(K, dim=-1)
    topv = topv / topv.sum(dim=-1, keepdim=True)
    wdense.zero_()
    wdense.scatter_(1, topi, topv)


def moe_dense_combine(out: torch.Tensor, y: torch.Tensor,
                      wdense: torch.Tensor) -> None:
    acc = (y.float() * wdense.t().unsqueeze(-1)).sum(dim=0)
    out.copy_(acc.to(out.dtype))


def moe_route_sort(topk_w: torch.Tensor, row_map: torch.Tensor,
                   inv_map: torch.Tensor, offsets: torch.Tensor,
                   logits: torch.Tensor, K: int) -> None:
    T, E = logits.shape
    # a stable descending sort keeps equal logits in expert-id order: the
    # kernel's "ties go to the lowest expert id" rule
    vals, idx = torch.sort(logits.float(), dim=-1, descending=True,
                           stable=True)
    topv, topi = vals[:, :K], idx[:, :K]
    topk_w.copy_(torch.softmax(topv, dim=-1).reshape(topk_w.shape))
    flat = topi.reshape(-1)
    order = torch.argsort(flat, stable=True)        # slots by (expert, t*K+j)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(order.numel(), device=order.device)
    row_map.copy_((order // K).to(torch.int32).reshape(row_map.shape))
    inv_map.copy_(inv.to(torch.int32).reshape(inv_map.shape))
    counts = torch.bincount(flat, minlength=E)
    offsets[0] = 0
    offsets[1:] = torch.cumsum(counts, 0).to(torch.int32)


def moe_grouped_gemm(out: torch.Tensor, a: torch.Tensor,
                     a_rows: torch.Tensor, w: torch.Tensor,
                     offsets: torch.Tensor) -> None:
    src = a if a_rows is None or a_rows.numel() == 0 else a[a_rows.long()]
    offs = offsets.tolist()
    for e in range(w.shape[0]):
        lo, hi = offs[e], offs[e + 1]
        if hi > lo:
            out[lo:hi] = (src[lo:hi].float() @ w[e].float().T).to(out.dtype)
