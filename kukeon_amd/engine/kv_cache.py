"""Paged KV cache for MI355X (288 GB HBM3E per GPU).

Layout per layer: k/v [num_blocks, Hk, BLOCK=16, D] bf16 — token-major rows
with D contiguous so the decode kernel's cooperative 16 B/lane stage is
coalesced.  One big [L, ...] allocation per side keeps the allocator trivial
and lets the engine size it against free HBM at init (kukeon capability map:
the reference has no GPU plane; this implements BASELINE.json's "paged KV
sized for 288 GB HBM").
"""
from __future__ import annotations

from typing import List

import torch

from kukeon_amd import ops


class BlockAllocator:
    """Free-list block allocator with a reference count per block.

    alloc hands a block out at count 1, share adds a holder, free drops one
    and returns the block to the free list only at zero — so sessions forked
    from a common prefix hold the same blocks. Without share it is the plain
    free list: same blocks in the same order (exact, O(1) per block)."""

    def __init__(self, num_blocks: int):
        self.num_blocks = num_blocks
        self._free: List[int] = list(range(num_blocks - 1, -1, -1))
        self._refs: List[int] = [0] * num_blocks
        self._num_shared = 0

    @property
    def num_free(self) -> int:
        return len(self._free)

    @property
    def num_shared(self) -> int:
        """Blocks held by more than one sequence."""
        return self._num_shared

    def alloc(self, n: int) -> List[int]:
        if n > len(self._free):
            raise MemoryError(
                f"KV cache exhausted: want {n} blocks, {len(self._free)} free")
        out = self._free[-n:][::-1]
        del self._free[-n:]
        for b in out:
            self._refs[b] = 1
        return out

    def share(self, blocks: List[int]) -> None:
        """Add one reference to each (allocated) block."""
        refs = self._refs
        for b in blocks:
            if refs[b] <= 0:
                raise ValueError(f"share of free KV block {b}")
        for b in blocks:
            refs[b] += 1
            if refs[b] == 2:
                self._num_shared += 1

    def free(self, blocks: List[int]) -> None:
        """Drop one reference from each block."""
        refs = self._refs
        for b in reversed(blocks):
            if refs[b] <= 0:
                raise ValueError(f"double free of KV block {b}")
            refs[b] -= 1
            if refs[b] == 0:
                self._free.append(b)
            elif refs[b] == 1:
                self._num_shared -= 1

    def num_exclusive(self, blocks: List[int]) -> int:
        """How many of `blocks` a free() of them would return to the pool."""
        refs = self._refs
        return sum(1 for b in blocks if refs[b] == 1)


class SequenceKV:
    """Per-sequence block list + logical length."""

    def __init__(self, block_size: int):
        self.block_size = block_size
        self.blocks: List[int] = []
        self.num_tokens = 0
        # last sampled token of the previous turn: sampled but never run
        # through the model, so the next turn's prefill must include it
        self.pending_token = None
        # every token whose K/V lives in the cache, in order — the replay
        # source for preemption-by-recompute
        self.history = []
        # host-tier blocks (HostKVPool ids) of a session swapped out while
        # idle: the positions after those `blocks` still covers, in order.
        # blocks_needed() then counts the device blocks a swap-in takes.
        self.host_blocks: List[int] = []

    def blocks_needed(self, new_tokens: int) -> int:
        total = self.num_tokens + new_tokens
        need = (total + self.block_size - 1) // self.block_size
        return max(0, need - len(self.blocks))

    def slots_for(self, new_tokens: int) -> List[int]:
        """Flat slot ids for the next new_tokens positions (after extend)."""
        out = []
        for i in range(new_tokens):
            p = self.num_tokens + i
            out.append(self.blocks[p // self.block_size] * self.block_size +
                       p % self.block_size)
        return out


class PagedKVCache:
    def __init__(self, num_layers: int, num_blocks: int, num_kv_heads: int,
                 block_size: int, head_dim: int, device, dtype=torch.bfloat16):
        self.num_layers = num_layers
        self.num_blocks = num_blocks
        self.block_size = block_size
        shape = (num_layers, num_blocks, num_kv_heads, block_size, head_dim)
        # zeros, NOT empty: attention masks out-of-range tail-block tokens
        # by score (-inf -> weight 0), but their V still enters the
        # accumulation as 0*value — uninitialized bytes can decode to NaN
        # bf16 and 0*NaN poisons the whole row. Zero-init guarantees every
        # slot is 0.0 or a previously written finite value.
        self.k = torch.zeros(shape, dtype=dtype, device=device)
        self.v = torch.zeros(shape, dtype=dtype, device=device)
        self.allocator = BlockAllocator(num_blocks)

    @staticmethod
    def blocks_from_bytes(free_bytes: int, num_layers: int, num_kv_heads: int,
                          block_size: int, head_dim: int,
                          dtype_bytes: int = 2) -> int:
        per_block = 2 * num_layers * num_kv_heads * block_size * head_dim * dtype_bytes
        return max(1, free_bytes // per_block)


class HostKVPool:
    """A second KV tier in host memory for sessions that idle: whole blocks
    leave the paged caches for it and come back bit for bit.

    `pool` is [host_blocks, record_bytes] uint8, pinned when the cache is on
    a GPU; a record is one block's K then V for all layers, the layout of
    the device staging buffer [staging_blocks, 2, L, Hk, BS, D]
    (ops.kv_pack_blocks). A store packs up to staging_blocks blocks into the
    staging buffer and copies each run of consecutive host ids with one
    copy_(non_blocking=True); a load is the reverse. Everything is enqueued
    on the current stream, in order. That ordering is what lets the caller
    hand the device blocks back to its allocator as soon as store returns,
    lets the staging buffer be reused chunk after chunk, and lets a host
    block be reused right after load returns. There is no copy stream and
    no overlap with compute."""

    def __init__(self, cache: PagedKVCache, host_blocks: int,
                 staging_blocks: int):
        L, _, Hk, BS, D = cache.k.shape
        dev = cache.k.device
        self.cache = cache
        self.num_blocks = host_blocks
        self.staging_blocks = max(1, staging_blocks)
        self.record_bytes = self.record_bytes_for(L, Hk, BS, D,
                                                  cache.k.element_size())
        self.pool = torch.empty(host_blocks, self.record_bytes,
                                dtype=torch.uint8,
                                pin_memory=dev.type == "cuda")
        self.allocator = BlockAllocator(host_blocks)
        self._staging_bytes = torch.zeros(self.staging_blocks,
                                          self.record_bytes,
                                          dtype=torch.uint8, device=dev)
        self.staging = self._staging_bytes.view(cache.k.dtype).view(
            self.staging_blocks, 2, L, Hk, BS, D)

    @staticmethod
    def record_bytes_for(num_layers: int, num_kv_heads: int, block_size: int,
                         head_dim: int, dtype_bytes: int = 2) -> int:
        return 2 * num_layers * num_kv_heads * block_size * head_dim * \
            dtype_bytes

    @staticmethod
    def _runs(ids: List[int]):
        """-> (offset, first id, length) of each run of consecutive ids."""
        i = 0
        while i < len(ids):
            j = i + 1
            while j < len(ids) and ids[j] == ids[j - 1] + 1:
                j += 1
            yield i, ids[i], j - i
            i = j

    def store(self, blocks: List[int]) -> List[int]:
        """Copy the device blocks to newly allocated host blocks, returned
        in the same order. MemoryError (pool cannot take them all) happens
        before anything is enqueued or allocated."""
        host = self.allocator.alloc(len(blocks))
        cap = self.staging_blocks
        dev = self.cache.k.device
        for c in range(0, len(blocks), cap):
            ids = torch.tensor(blocks[c:c + cap], dtype=torch.int32,
                               device=dev)
            ops.kv_pack_blocks(self.cache.k, self.cache.v, ids, self.staging)
            for off, h0, m in self._runs(host[c:c + cap]):
                self.pool[h0:h0 + m].copy_(self._staging_bytes[off:off + m],
                                           non_blocking=True)
        return host

    def load(self, host: List[int], blocks: List[int]) -> None:
        """Copy the host blocks into the (distinct, caller-owned) device
        blocks and free the host blocks."""
        assert len(host) == len(blocks)
        cap = self.staging_blocks
        dev = self.cache.k.device
        for c in range(0, len(host), cap):
            for off, h0, m in self._runs(host[c:c + cap]):
                self._staging_bytes[off:off + m].copy_(self.pool[h0:h0 + m],
                                                       non_blocking=True)
            ids = torch.tensor(blocks[c:c + cap], dtype=torch.int32,
                               device=dev)
            ops.kv_unpack_blocks(self.staging, self.cache.k, self.cache.v,
                                 ids)
        self.allocator.free(host)
