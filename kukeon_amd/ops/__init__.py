"""Device-op dispatch for kukeon_amd.

On a CUDA (ROCm) device every op is the hand-written gfx950 HIP kernel from
``kukeon_amd._C`` — if the extension is missing there we raise instead of
falling back, so a GPU run can never silently use an eager path.  On CPU the
fp32 reference implementations run (tests, GPU-less control-plane hosts).
"""
from __future__ import annotations

import torch

from . import reference

_C = None
_IMPORT_ERROR: Exception | None = None


def _load() -> None:
    global _C, _IMPORT_ERROR
    try:
        from kukeon_amd import _C as ext  # type: ignore
    except Exception as e:  # pragma: no cover - only on broken installs
        _IMPORT_ERROR = e
    else:
        _C, _IMPORT_ERROR = ext, None


_load()


def native_available() -> bool:
    # importing kukeon_amd.ops.build imports this package first, so in a
    # fresh tree the extension only appears after this module was loaded
    if _C is None:
        _load()
    return _C is not None


def _native():
    if _C is None:
        _load()
    if _C is None:
        raise RuntimeError(
            "kukeon_amd._C (gfx950 HIP extension) is not built but an op was "
            "called on a CUDA device. Run `python -m kukeon_amd.ops.build` "
            f"(import error: {_IMPORT_ERROR})")
    return _C


def _impl(t: torch.Tensor):
    return _native() if t.is_cuda else reference


def rmsnorm(out, input, weight, eps: float) -> None:
    _impl(input).rmsnorm(out, input, weight, eps)


def fused_add_rmsnorm(input, residual, weight, eps: float) -> None:
    _impl(input).fused_add_rmsnorm(input, residual, weight, eps)


def silu_mul(out, gate_up) -> None:
    _impl(gate_up).silu_mul(out, gate_up)


def rope_kv_append(qkv, k_cache, v_cache, cos_sin, positions, slot_mapping,
                   num_q_heads: int, num_kv_heads: int, head_dim: int,
                   block_table=None) -> None:
    if block_table is None:
        block_table = torch.empty(0, dtype=torch.int32, device=qkv.device)
    _impl(qkv).rope_kv_append(qkv, k_cache, v_cache, cos_sin, positions,
                              slot_mapping, num_q_heads, num_kv_heads,
                              head_dim, block_table)


def kv_copy_blocks(k_cache, v_cache, src, dst) -> None:
    """cache[l, dst[i]] = cache[l, src[i]] for every layer l, every pair i
    and both caches [L, NB, Hk, BS, D], as raw bytes (bf16 and fp8 caches
    alike) in one launch; an empty pair list launches nothing. `src` and
    `dst` are int32 tensors of equal length on the caches' device. A source
    may repeat; destinations must be distinct and disjoint from the
    sources, which the caller guarantees."""
    _impl(k_cache).kv_copy_blocks(k_cache, v_cache, src, dst)


def kv_pack_blocks(k_cache, v_cache, blocks, staging) -> None:
    """staging[i, s, l] = cache_s[l, blocks[i]] for every layer l, both
    sides s (0 = K, 1 = V) and every listed block i, as raw bytes (bf16 and
    fp8 caches alike) in one launch; an empty list launches nothing. The
    caches are [L, NB, Hk, BS, D]; `staging` is [cap, 2, L, Hk, BS, D] of the
    caches' dtype, so record i is one block of all layers, contiguous — the
    unit a copy to host memory moves. `blocks` is a contiguous int32 tensor
    of at most cap ids on the caches' device; records from len(blocks) on
    are left untouched."""
    _impl(k_cache).kv_pack_blocks(k_cache, v_cache, blocks, staging)


def kv_unpack_blocks(staging, k_cache, v_cache, blocks) -> None:
    """cache_s[l, blocks[i]] = staging[i, s, l]: the inverse of
    kv_pack_blocks, with the same shapes and checks. The destination blocks
    must be distinct, which the caller guarantees; no other block is
    written."""
    _impl(k_cache).kv_unpack_blocks(staging, k_cache, v_cache, blocks)


def decode_advance(ids, pos, seq_lens, tokens, ring, counter) -> None:
    _impl(ids).decode_advance(ids, pos, seq_lens, tokens, ring, counter)


def paged_attention(out, q, k_cache, v_cache, block_table, seq_lens,
                    q_offset: int, num_splits: int, scale: float,
                    tmp_out, tmp_ml) -> None:
    """Decode attention of one query token per row of `q` against the
    paged KV cache, split `num_splits` (>= 1) ways along the context.

    `tmp_out` / `tmp_ml` are float32 workspaces of at least
    B*Hq*num_splits*128 and B*Hq*num_splits*2 elements. A row with
    seq_len <= 0 leaves its `out` row untouched on the GPU (the CPU
    reference zeroes it)."""
    _impl(q).paged_attention(out, q, k_cache, v_cache, block_table, seq_lens,
                             q_offset, num_splits, scale, tmp_out, tmp_ml)


# KUKEON_DECODE_ATTN_FUSED=0 makes the models' decode path run
# rope_kv_append + paged_attention as separate launches again (A/B
# measurement, tests); the default folds both into paged_attention_rope.
DECODE_ATTN_FUSED = __import__("os").environ.get(
    "KUKEON_DECODE_ATTN_FUSED", "1") != "0"


def paged_attention_rope(out, qkv, k_cache, v_cache, cos_sin, positions,
                         block_table, seq_lens, num_q_heads: int,
                         num_kv_heads: int, num_splits: int, scale: float,
                         tmp_out, tmp_ml) -> None:
    """rope_kv_append (block-table mode) + paged_attention of one decode
    token per row of the fused `qkv` projection, in one pass: q and the new
    k are rotated on the fly, the new k/v rows are appended to the caches,
    and `out` is what the two ops would have produced, bit for bit. `qkv`
    itself is left untouched. A row with positions < 0 appends nothing;
    workspaces and seq_len <= 0 as in paged_attention (with num_splits <= 8
    the GPU kernel does not touch the workspaces at all)."""
    _impl(qkv).paged_attention_rope(out, qkv, k_cache, v_cache, cos_sin,
                                    positions, block_table, seq_lens,
                                    num_q_heads, num_kv_heads, num_splits,
                                    scale, tmp_out, tmp_ml)


def check_prefix_tiles(tiles, group: int) -> None:
    """Raise ValueError unless the host tensor `tiles` is int32 [T, 2 + 16]
    with n_rows <= 16 // group in every tile. The shared ops cannot check
    this themselves without reading device memory; whoever fills the tiles
    on the host calls this before uploading them."""
    reference.check_prefix_tiles(tiles, group)


def paged_attention_shared(out, q, k_cache, v_cache, block_table, seq_lens,
                           q_offset: int, num_splits: int, scale: float,
                           tmp_out, tmp_ml, prefix_blocks, tiles,
                           prefix_splits: int) -> None:
    """paged_attention for rows that share leading cache blocks (forked
    sessions): a tile of up to W = 16 // (Hq // Hk) sibling rows rides the
    matrix cores' N axis together, so their common prefix blocks are
    fetched and scored once per tile, not once per row.

    `prefix_blocks` int32 [B]: how many leading blocks of row b a tile
    covers, 0 for a row in no tile. `tiles` int32 [T, 2 + 16]: n_rows,
    n_prefix_blocks, then the member rows; n_rows == 0 is an empty tile.
    The prefix block ids are read from the first member's block table.
    The caller guarantees that every member's table begins with those
    n_prefix_blocks ids, that prefix_blocks[row] == n_prefix_blocks for
    every member, that n_prefix_blocks * 16 <= the row's newest position
    (the prefix is full, immutable blocks only), that a row is in at most
    one tile, that members have seq_len > 0 and that n_rows <= W
    (check_prefix_tiles). The CPU reference checks all of it; the GPU op
    reads none of it on the host and clamps what it reads on the device to
    the buffers' bounds.

    The prefix is split `prefix_splits` ways and the rest of each row
    `num_splits` ways, all merged by the reduce kernel: the workspaces hold
    at least B*Hq*(prefix_splits + num_splits) slots of 128 and 2 floats.
    `out` is paged_attention's up to summation order."""
    _impl(q).paged_attention_shared(out, q, k_cache, v_cache, block_table,
                                    seq_lens, q_offset, num_splits, scale,
                                    tmp_out, tmp_ml, prefix_blocks, tiles,
                                    prefix_splits)


def paged_attention_rope_shared(out, qkv, k_cache, v_cache, cos_sin,
                                positions, block_table, seq_lens,
                                num_q_heads: int, num_kv_heads: int,
                                num_splits: int, scale: float, tmp_out,
                                tmp_ml, prefix_blocks, tiles,
                                prefix_splits: int) -> None:
    """paged_attention_rope with the metadata and workspaces of
    paged_attention_shared. The caches come out bit-equal to
    paged_attention_rope's (the append is the suffix pass's, unchanged) and
    `qkv` is left untouched; n_prefix_blocks * 16 <= positions[row] keeps
    the token being appended out of the prefix."""
    _impl(qkv).paged_attention_rope_shared(
        out, qkv, k_cache, v_cache, cos_sin, positions, block_table,
        seq_lens, num_q_heads, num_kv_heads, num_splits, scale, tmp_out,
        tmp_ml, prefix_blocks, tiles, prefix_splits)


def prefill_attention(out, q, k_cache, v_cache, block_table, seq_lens,
                      q_starts, qb_seq, qb_start, q_offset: int,
                      scale: float) -> None:
    _impl(q).prefill_attention(out, q, k_cache, v_cache, block_table,
                               seq_lens, q_starts, qb_seq, qb_start, q_offset,
                               scale)


def sample(tokens, logits, temps, top_k, top_p, seed, workspace) -> None:
    _impl(logits).sample(tokens, logits, temps, top_k, top_p, seed, workspace)


_SKINNY_WS = {}
# replaced (outgrown) workspaces are pinned here forever: a hipGraph
# captured earlier may still hold the old tensor's device pointer, and
# letting it free would put a use-after-free inside every later replay
_SKINNY_WS_RETIRED = []
# Per-shape dispatch, from the measured sweep (profiles/r01_progress.md,
# scripts/sweep_splitk.py on MI355X): the glds-staged skinny kernel beats
# hipBLASLt on square o-projection shapes (N==K: 16.6us vs 19.3 at M=64,
# 11.9 vs 19.2 at M=16 on 4096x4096) and trails it on qkv/gate_up/down/
# lm_head, where hipBLASLt is 55-100% of the HBM floor. KUKEON_SKINNY_GEMM=1
# forces the skinny kernel for every eligible shape (benchmarking).
_USE_SKINNY = __import__("os").environ.get("KUKEON_SKINNY_GEMM", "0")
# silu-into-down-staging fusion: measured SLOWER in situ (54.2us fused vs
# 42.9 for silu_mul + gemm cold; bench 51.7 vs 53.6 turns/s same box) —
# the doubled x staging traffic outweighs the saved launch. Off by
# default; kernel + numerics test stay as the documented negative result.
_FUSE_SILU = __import__("os").environ.get("KUKEON_FUSE_SILU", "0") == "1"


def _skinny_wins(rows: int, N: int, K: int) -> bool:
    if _USE_SKINNY == "off":   # A/B: force the library everywhere
        return False
    return N == K == 4096


# v5 (full-line never-drain pipeline, KS=128/2 blocks-per-CU): beats
# hipBLASLt cold on the down-projection (32.2us vs 39.6 on 4096x14336 at
# M=64, floor 18.6 — profiles/r02_progress.md); qkv ties, gate_up and
# lm_head stay on the library. KUKEON_SKINNY_GEMM=5 forces it everywhere
# for benchmarking.
def _skinny5_wins(rows: int, N: int, K: int) -> bool:
    if _USE_SKINNY == "off":   # A/B: force the library everywhere
        return False
    # llama-3-8b down (32.2us vs blas 39.6 cold) and llama-3-70b down
    # (79.3 vs 83.1 at M=16, 92.6 vs 139.3 at M=64) — measured on
    # MI355X, profiles/r02_progress.md
    return (N, K) in ((4096, 14336), (8192, 28672))


def _skinny_kind(x: torch.Tensor, w: torch.Tensor, fused: bool):
    """Which skinny kernel runs x @ w.T: "v5", "v1", or None for the
    library. `fused` asks for the reduce + residual-add + RMSNorm epilogue,
    which exists only at TP=1 and holds a whole row per block."""
    rows = x.shape[0]
    if not (x.is_cuda and x.dim() == 2 and rows <= 64
            and x.dtype == torch.bfloat16):
        return None
    N, K = w.shape
    if fused:
        from kukeon_amd import parallel
        if not (parallel.tp_size() == 1 and N % 2048 == 0 and N <= 8192):
            return None
    if (N % 128 == 0 and K % 128 == 0
            and (_USE_SKINNY == "5" or _skinny5_wins(rows, N, K))):
        return "v5"
    if (N % 64 == 0 and K % 32 == 0
            and (_USE_SKINNY == "1" or _skinny_wins(rows, N, K))):
        return "v1"
    return None


# split-K factor per (kind, N, K), asked of the launchers' own plan once
# (so their env overrides are read at a shape's first use, like the
# switches above at import)
_SKINNY_SPLITK = {}


def _skinny_workspace(device: torch.device, kind: str, N: int,
                      K: int) -> torch.Tensor:
    """The device's split-K slab buffer, grown to the 64 * N * splitk
    floats the `kind` launcher (a skinny_splitk kind) may write."""
    splitk = _SKINNY_SPLITK.get((kind, N, K))
    if splitk is None:
        splitk = _SKINNY_SPLITK[kind, N, K] = _native().skinny_splitk(
            kind, N, K)
    need = 64 * N * splitk
    key = (device.index or 0)
    ws = _SKINNY_WS.get(key)
    if ws is None or ws.numel() < need:
        # grown only outside graph capture (engine warmup runs eager)
        if ws is not None:
            _SKINNY_WS_RETIRED.append(ws)
        ws = torch.empty(need, dtype=torch.float32, device=device)
        _SKINNY_WS[key] = ws
    return ws


class Fp8Weight:
    """A weight-only-quantised [N, K] weight: `q` uint8 [N, K] holding OCP
    e4m3fn bytes (the storage the fp8 KV cache uses) and `scale` f32 [N],
    one per output channel; the weight it stands for is
    float(q) * scale[:, None]. linear / linear_add_rmsnorm /
    mlp_down_fused take one wherever they take a bf16 weight."""

    __slots__ = ("q", "scale")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        assert q.dtype == torch.uint8 and q.dim() == 2
        assert scale.dtype == torch.float32 and scale.shape == (q.shape[0],)
        self.q = q
        self.scale = scale

    @property
    def shape(self):
        return tuple(self.q.shape)

    @property
    def device(self) -> torch.device:
        return self.q.device

    @property
    def is_cuda(self) -> bool:
        return self.q.is_cuda

    @property
    def nbytes(self) -> int:
        return self.q.numel() + 4 * self.scale.numel()


class Mxfp4Weight:
    """A weight-only-quantised [N, K] weight in OCP MXFP4: `q` uint8
    [N, K/2] holding two e2m1 codes per byte (element 2j in the low
    nibble, 2j+1 in the high one; a code is sign, two exponent bits, one
    mantissa bit: magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6) and `scale` uint8
    [N, K/32], one e8m0 byte per block of 32 along K; the weight it stands
    for is value(code[n, k]) * 2^(scale[n, k // 32] - 127). Holding one
    needs K % 32 == 0; the decode kernel N % 64 == 0 and K % 128 == 0."""

    __slots__ = ("q", "scale")

    def __init__(self, q: torch.Tensor, scale: torch.Tensor):
        assert q.dtype == torch.uint8 and q.dim() == 2
        assert q.shape[1] % 16 == 0
        assert scale.dtype == torch.uint8 and scale.shape == (
            q.shape[0], q.shape[1] // 16)
        self.q = q
        self.scale = scale

    @property
    def shape(self):
        return (self.q.shape[0], 2 * self.q.shape[1])

    @property
    def device(self) -> torch.device:
        return self.q.device

    @property
    def is_cuda(self) -> bool:
        return self.q.is_cuda

    @property
    def nbytes(self) -> int:
        return self.q.numel() + self.scale.numel()


# bf16 scratch a wide-M (prefill, > 64 rows) linear dequantises an
# Fp8Weight or Mxfp4Weight into, one per device, as large as the largest
# weight quantised there; outgrown ones are pinned like the split-K
# workspaces
_W8_SCRATCH = {}
_W8_SCRATCH_RETIRED = []


def _w8_scratch(device: torch.device, numel: int) -> torch.Tensor:
    key = (device.index or 0)
    buf = _W8_SCRATCH.get(key)
    if buf is None or buf.numel() < numel:
        # grown only outside graph capture: quantize_weight reserves the
        # size of every weight when the model is built
        if buf is not None:
            _W8_SCRATCH_RETIRED.append(buf)
        buf = torch.empty(numel, dtype=torch.bfloat16, device=device)
        _W8_SCRATCH[key] = buf
    return buf


def quantize_weight(w: torch.Tensor, fmt: str = "fp8"):
    """Quantise a bf16 [N, K] weight: fmt "fp8" to an Fp8Weight with
    per-output-channel scales (scale = amax / 448, round-to-nearest-even),
    fmt "mxfp4" to an Mxfp4Weight by the OCP MX rule
    (reference.quantize_mxfp4_rows; K % 32 == 0)."""
    w = w.detach().contiguous()
    N, K = w.shape
    if fmt == "mxfp4":
        if K % 32:
            raise ValueError(f"mxfp4 needs K % 32 == 0, got K = {K}")
        q = torch.empty(N, K // 2, dtype=torch.uint8, device=w.device)
        scale = torch.empty(N, K // 32, dtype=torch.uint8, device=w.device)
        _impl(w).quantize_mxfp4_rows(q, scale, w)
        qw = Mxfp4Weight(q, scale)
    elif fmt == "fp8":
        q = torch.empty(N, K, dtype=torch.uint8, device=w.device)
        scale = torch.empty(N, dtype=torch.float32, device=w.device)
        _impl(w).quantize_fp8_rows(q, scale, w)
        qw = Fp8Weight(q, scale)
    else:
        raise ValueError(f"quantize_weight: fmt must be 'fp8' or 'mxfp4', "
                         f"got {fmt!r}")
    if w.is_cuda:
        _w8_scratch(w.device, N * K)
    return qw


def dequantize_weight(fw, out: torch.Tensor = None) -> torch.Tensor:
    """The bf16 [N, K] weight an Fp8Weight (bf16(float(q) * scale)) or an
    Mxfp4Weight (exact) stands for; into `out` when given."""
    if out is None:
        out = torch.empty(fw.shape, dtype=torch.bfloat16, device=fw.device)
    if isinstance(fw, Mxfp4Weight):
        _impl(fw.q).dequant_mxfp4_rows(out, fw.q, fw.scale)
    else:
        _impl(fw.q).dequant_fp8_rows(out, fw.q, fw.scale)
    return out


def _w8_skinny(x: torch.Tensor, fw: Fp8Weight) -> bool:
    """Whether the W8A16 decode kernel runs x @ fw: its shape contract."""
    N, K = fw.shape
    return (x.is_cuda and x.dim() == 2 and 1 <= x.shape[0] <= 64
            and x.dtype == torch.bfloat16 and x.is_contiguous()
            and N % 64 == 0 and K % 64 == 0)


def _linear_w8(x: torch.Tensor, fw: Fp8Weight) -> torch.Tensor:
    if not x.is_cuda:
        return reference.linear_w8(x, fw.q, fw.scale)
    N, K = fw.shape
    if _w8_skinny(x, fw):
        out = torch.empty(x.shape[0], N, dtype=x.dtype, device=x.device)
        ws = _skinny_workspace(x.device, "w8", N, K)
        _native().skinny_gemm_w8(out, x, fw.q, fw.scale, ws)
        return out
    # prefill, the 96-256 row decode buckets, odd shapes: widen to bf16
    # scratch, then the library GEMM
    w = _w8_scratch(x.device, N * K)[:N * K].view(N, K)
    _native().dequant_fp8_rows(w, fw.q, fw.scale)
    return torch.nn.functional.linear(x, w)


def _w4_skinny(x: torch.Tensor, mw: Mxfp4Weight) -> bool:
    """Whether the W4A16 decode kernel runs x @ mw: its shape contract."""
    N, K = mw.shape
    return (x.is_cuda and x.dim() == 2 and 1 <= x.shape[0] <= 64
            and x.dtype == torch.bfloat16 and x.is_contiguous()
            and N % 64 == 0 and K % 128 == 0)


def _linear_w4(x: torch.Tensor, mw: Mxfp4Weight) -> torch.Tensor:
    if not x.is_cuda:
        return reference.linear_w4(x, mw.q, mw.scale)
    N, K = mw.shape
    if _w4_skinny(x, mw):
        out = torch.empty(x.shape[0], N, dtype=x.dtype, device=x.device)
        ws = _skinny_workspace(x.device, "w4", N, K)
        _native().skinny_gemm_w4(out, x, mw.q, mw.scale, ws)
        return out
    # prefill, the 96-256 row decode buckets, odd shapes: widen to bf16
    # scratch (exact), then the library GEMM
    w = _w8_scratch(x.device, N * K)[:N * K].view(N, K)
    _native().dequant_mxfp4_rows(w, mw.q, mw.scale)
    return torch.nn.functional.linear(x, w)


def linear(x: torch.Tensor, w) -> torch.Tensor:
    """F.linear with the weight-streaming skinny-GEMM kernel on the decode
    shapes where it measured faster than hipBLASLt; hipBLASLt otherwise.
    An Fp8Weight / Mxfp4Weight runs the W8A16 / W4A16 kernel at up to 64
    rows and dequantises into scratch for the library above that."""
    if isinstance(w, Fp8Weight):
        return _linear_w8(x, w)
    if isinstance(w, Mxfp4Weight):
        return _linear_w4(x, w)
    kind = _skinny_kind(x, w, fused=False)
    if kind is None:
        return torch.nn.functional.linear(x, w)
    N, K = w.shape
    out = torch.empty(x.shape[0], N, dtype=x.dtype, device=x.device)
    ws = _skinny_workspace(x.device, kind, N, K)
    if kind == "v5":
        _native().skinny_gemm5(out, x, w, ws)
    else:
        _native().skinny_gemm(out, x, w, ws)
    return out


def linear_add_rmsnorm(x: torch.Tensor, w: torch.Tensor,
                       residual: torch.Tensor, norm_weight: torch.Tensor,
                       eps: float) -> torch.Tensor:
    """out-projection + TP all-reduce + residual add + RMSNorm as one
    fused path. On the skinny decode shapes (TP=1) the split-K reduce,
    residual add and norm run in a single kernel — the separate epilogue
    pair cost two launches at the ~4.5us in-graph dispatch floor for
    <1us of work. Mutates `residual` (+= x@w.T) and returns the normed
    activations, exactly like linear() followed by fused_add_rmsnorm().
    """
    if isinstance(w, Fp8Weight):
        from kukeon_amd import parallel
        N, K = w.shape
        if (_w8_skinny(x, w) and parallel.tp_size() == 1
                and N % 2048 == 0 and N <= 8192):
            normed = torch.empty(x.shape[0], N, dtype=x.dtype,
                                 device=x.device)
            ws = _skinny_workspace(x.device, "w8", N, K)
            _native().skinny_gemm_w8_fused_norm(normed, x, w.q, w.scale, ws,
                                                residual, norm_weight, eps)
            return normed
        kind = None
    elif isinstance(w, Mxfp4Weight):
        from kukeon_amd import parallel
        N, K = w.shape
        if (_w4_skinny(x, w) and parallel.tp_size() == 1
                and N % 2048 == 0 and N <= 8192):
            normed = torch.empty(x.shape[0], N, dtype=x.dtype,
                                 device=x.device)
            ws = _skinny_workspace(x.device, "w4", N, K)
            _native().skinny_gemm_w4_fused_norm(normed, x, w.q, w.scale, ws,
                                                residual, norm_weight, eps)
            return normed
        kind = None
    else:
        kind = _skinny_kind(x, w, fused=True)
    if kind is None:
        from kukeon_amd import parallel
        h = parallel.tp_all_reduce(linear(x, w))
        fused_add_rmsnorm(h, residual, norm_weight, eps)
        return h
    N, K = w.shape
    normed = torch.empty(x.shape[0], N, dtype=x.dtype, device=x.device)
    if kind == "v5":
        ws = _skinny_workspace(x.device, "v5_fused", N, K)
        _native().skinny_gemm5_fused_norm(normed, x, w, ws, residual,
                                          norm_weight, eps)
    else:
        ws = _skinny_workspace(x.device, "v1", N, K)
        _native().skinny_gemm_fused_norm(normed, x, w, ws, residual,
                                         norm_weight, eps)
    return normed


def mlp_down_fused(gu: torch.Tensor, w: torch.Tensor,
                   residual: torch.Tensor, norm_weight: torch.Tensor,
                   eps: float) -> torch.Tensor:
    """The decode MLP tail — silu(gate)*up -> down-projection ->
    TP all-reduce -> residual add -> RMSNorm — with the activation fused
    into the down GEMM's x staging on the skinny decode shapes (the
    standalone silu_mul launch and its act-tensor HBM round trip
    disappear; profiles/r02_progress.md). `gu` is the fused gate_up GEMM
    output [rows, 2K]. Equivalent to silu_mul + linear_add_rmsnorm.
    """
    rows = gu.shape[0]
    N, K = w.shape
    # the silu-into-staging kernel reads bf16 W: a quantised weight goes
    # unfused
    if (_FUSE_SILU and not isinstance(w, (Fp8Weight, Mxfp4Weight))
            and gu.dim() == 2
            and gu.shape[1] == 2 * K
            and _skinny_kind(gu, w, fused=True) == "v5"):
        ws = _skinny_workspace(gu.device, "v5_fused", N, K)
        normed = torch.empty(rows, N, dtype=gu.dtype, device=gu.device)
        _native().skinny_gemm5_silu_fused_norm(normed, gu, w, ws,
                                               residual, norm_weight, eps)
        return normed
    act = torch.empty(rows, K, dtype=gu.dtype, device=gu.device)
    silu_mul(act, gu)
    return linear_add_rmsnorm(act, w, residual, norm_weight, eps)


def moe_router_weights(wdense, logits, k: int) -> None:
    _impl(logits).moe_router_weights(wdense, logits, k)


def moe_dense_combine(out, y, wdense) -> None:
    _impl(y).moe_dense_combine(out, y, wdense)


def moe_gather_tokens(out, input, row_map) -> None:
    _impl(input).moe_gather_tokens(out, input, row_map)


def moe_scatter_tokens(out, input, inv_map, weights, top_k: int) -> None:
    _impl(input).moe_scatter_tokens(out, input, inv_map, weights, top_k)


def moe_route_sort(topk_w, row_map, inv_map, offsets, logits, k: int) -> None:
    """Top-k routing on the raw logits (ties to the lowest expert id) and
    the stable sort of the (token, j) pairs by expert, all on the device:
    no host read, so the MoE layer's launch shapes never depend on the
    routing."""
    _impl(logits).moe_route_sort(topk_w, row_map, inv_map, offsets, logits,
                                 k)


def moe_grouped_gemm(out, a, a_rows, w, offsets) -> None:
    """out[r] = a[a_rows[r]] @ w[e].T for r in [offsets[e], offsets[e+1]),
    every expert in one launch. `a_rows` None/empty means identity."""
    if a_rows is None:
        a_rows = torch.empty(0, dtype=torch.int32, device=a.device)
    _impl(a).moe_grouped_gemm(out, a, a_rows, w, offsets)
