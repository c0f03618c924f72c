"""The MI355X serving engine: continuous batching over a paged KV cache.

Design (MI355X-first, not a port — the reference eminwux/kukeon has no
inference plane at all):

* one engine per GPU process; sessions own persistent KV (multi-turn agent
  context stays resident in the 288 GB HBM across turns); sessions forked
  from a common context share its full KV blocks by reference count,
* prefill runs as a packed varlen batch (GEMM-bound at 32k tokens),
* decode runs the whole running set each step; the full forward + logits +
  top-k/top-p sampling is captured in a hipGraph per batch-size bucket so a
  ~2.5 ms bf16 decode step is not launch-bound (~300 kernel launches/step),
* requests hold *sticky rows* in the static decode buffers, so the per-step
  host work is O(active rows) scalar updates + one slab H2D copy — no
  per-step tensor rebuilds,
* split-KV decode attention (matrix-core kernel, 4 autonomous wave-slots
  per workgroup) is split to ~4096 wave-units so the chip stays full even
  at small batch; idle sessions' KV evicts under pressure (history
  recompute, or a swap to pinned host memory when kv_host_blocks > 0) and
  running rows preempt-by-recompute on exhaustion.
"""
from __future__ import annotations

import logging
import weakref
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch

from kukeon_amd import ops
from kukeon_amd.engine.config import EngineConfig, ModelConfig, SamplingParams
from kukeon_amd.engine.kv_cache import HostKVPool, PagedKVCache, SequenceKV
from kukeon_amd.models.llama import AttnMeta

log = logging.getLogger("kukeon.engine")


@dataclass
class Request:
    req_id: int
    kv: SequenceKV                      # persistent, owned by the session
    prompt_tokens: List[int]            # new tokens to prefill this turn
    sampling: SamplingParams
    ctx_start: int = 0                  # kv.num_tokens at submission
    output_tokens: List[int] = field(default_factory=list)
    finished: bool = False
    row: int = -1                       # sticky decode row
    bt_written: int = 0                 # block-table entries already staged
    prefill_pos: int = 0                # prompt tokens already prefilled
    preempted: int = 0


@dataclass
class StepOutput:
    req_id: int
    new_tokens: List[int]
    finished: bool


class LLMEngine:
    def __init__(self, model, cfg: ModelConfig, ecfg: EngineConfig,
                 device="cuda"):
        self.model = model
        self.cfg = cfg
        self.ecfg = ecfg
        self.device = torch.device(device)
        self.is_cuda = self.device.type == "cuda"
        import kukeon_amd.parallel as parallel
        self.hk = cfg.num_kv_heads // max(1, parallel.tp_size())
        self.hq = cfg.num_q_heads // max(1, parallel.tp_size())

        kv_torch_dtype = (torch.uint8 if ecfg.kv_dtype == "fp8"
                          else torch.bfloat16)
        kv_bytes = 1 if ecfg.kv_dtype == "fp8" else 2
        nblocks = ecfg.num_kv_blocks
        if nblocks <= 0:
            if self.is_cuda:
                free, _total = torch.cuda.mem_get_info(self.device)
                # oversubscribed rehearsals (more local ranks than GPUs,
                # e.g. a world-2 torchrun on a 1-GPU box) share the HBM:
                # split the KV budget so the second rank isn't starved
                import os as _os
                lw = int(_os.environ.get("LOCAL_WORLD_SIZE", "1") or 1)
                ndev = max(1, torch.cuda.device_count())
                share = max(1, -(-lw // ndev))
                budget = int(free * ecfg.kv_mem_fraction) // share - (2 << 30)
                nblocks = PagedKVCache.blocks_from_bytes(
                    max(budget, 1 << 28), cfg.num_layers, self.hk,
                    ecfg.block_size, cfg.head_dim, dtype_bytes=kv_bytes)
                nblocks = min(nblocks, 4_000_000)
            else:
                nblocks = 512
        self.kv = PagedKVCache(cfg.num_layers, nblocks, self.hk,
                               ecfg.block_size, cfg.head_dim, self.device,
                               dtype=kv_torch_dtype)
        log.info("KV cache: %d blocks (%.1f GiB for K+V)", nblocks,
                 self.kv.k.nbytes * 2 / (1 << 30))
        # host KV tier (off by default): where _evict_idle_kv puts an idle
        # session's exclusive blocks instead of dropping them
        self.host_kv: Optional[HostKVPool] = None
        if ecfg.kv_host_blocks > 0:
            self.host_kv = HostKVPool(self.kv, ecfg.kv_host_blocks,
                                      ecfg.kv_swap_staging_blocks)
            log.info("host KV tier: %d blocks (%.1f GiB%s), %d staging",
                     ecfg.kv_host_blocks,
                     self.host_kv.pool.nbytes / (1 << 30),
                     ", pinned" if self.is_cuda else "",
                     self.host_kv.staging_blocks)
        self.swap_out_blocks = 0    # blocks copied to the host tier, ever
        self.swap_in_blocks = 0     # blocks copied back
        self.swap_fallbacks = 0     # evictions that dropped, tier being on
        # sessions that hold host blocks right now: a plain int kept where
        # host_blocks turns non-empty or empty, so other threads (the
        # server's stats) can read it
        self.swapped_sessions = 0

        self.waiting: List[Request] = []
        self._next_id = 0
        # every SequenceKV ever submitted (weak): idle-session KV is
        # evictable when admission starves on blocks (history recompute)
        self._known_kvs: "weakref.WeakValueDictionary[int, SequenceKV]" = \
            weakref.WeakValueDictionary()

        # ---- sticky-row decode state ----
        self.Bmax = ecfg.max_sessions
        self._rows: List[Optional[Request]] = [None] * self.Bmax
        self._free_rows: List[int] = list(range(self.Bmax - 1, -1, -1))
        self.num_running = 0

        mb = ecfg.max_blocks_per_seq
        d = self.device
        self.d_ids = torch.zeros(self.Bmax, dtype=torch.int32, device=d)
        self.d_pos = torch.zeros(self.Bmax, dtype=torch.int32, device=d)
        self.d_slots = torch.full((self.Bmax,), -1, dtype=torch.int32, device=d)
        self.d_bt = torch.zeros(self.Bmax, mb, dtype=torch.int32, device=d)
        self.d_seq_lens = torch.zeros(self.Bmax, dtype=torch.int32, device=d)
        self.d_temps = torch.zeros(self.Bmax, dtype=torch.float32, device=d)
        self.d_topk = torch.zeros(self.Bmax, dtype=torch.int32, device=d)
        self.d_topp = torch.ones(self.Bmax, dtype=torch.float32, device=d)
        self.d_tokens = torch.zeros(self.Bmax, dtype=torch.int32, device=d)
        self.d_seed = torch.full((1,), ecfg.seed, dtype=torch.int64, device=d)
        self.d_ws = torch.zeros(self.Bmax, 528, dtype=torch.float32,
                                device=d)  # sampling workspace rows
        # 32 split slots: small decode batches (16-session / 70B configs)
        # need B*Hk*S ~ 4096 wave-units to fill the MFMA attention kernel
        # at its 4-waves/SIMD occupancy; 16 capped them at half the chip
        self.max_splits = 32
        self.d_tmp_out = {}
        self.d_tmp_ml = {}
        # self-advancing decode: token ring + device step counter
        self.max_microbatch = 256
        self.d_ring = torch.zeros(self.max_microbatch * self.Bmax,
                                  dtype=torch.int32, device=d)
        self.d_step = torch.zeros(1, dtype=torch.int32, device=d)
        pin = self.is_cuda
        self.h_ids = torch.zeros(self.Bmax, dtype=torch.int32, pin_memory=pin)
        self.h_pos = torch.zeros(self.Bmax, dtype=torch.int32, pin_memory=pin)
        self.h_slots = torch.full((self.Bmax,), -1, dtype=torch.int32,
                                  pin_memory=pin)
        self.h_seq_lens = torch.zeros(self.Bmax, dtype=torch.int32,
                                      pin_memory=pin)
        self.h_bt = torch.zeros(self.Bmax, mb, dtype=torch.int32,
                                pin_memory=pin)
        self.h_params = torch.zeros(self.Bmax, 3, dtype=torch.float32,
                                    pin_memory=pin)
        self._params_dirty = False
        # numpy views of the pinned staging buffers: per-row scalar writes
        # through torch cost ~5-10us each; through numpy they are ~50ns,
        # and the views share the pinned memory so the H2D copies see them
        self.n_ids = self.h_ids.numpy()
        self.n_pos = self.h_pos.numpy()
        self.n_slots = self.h_slots.numpy()
        self.n_seq_lens = self.h_seq_lens.numpy()
        self.n_bt = self.h_bt.numpy()

        self.graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self._graph_pool = None

        # ---- shared-prefix decode (see _regroup) ----
        # graphs of the shared path, by bucket, apart from self.graphs
        self.shared_graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        self.tile_width = 16 // max(1, self.hq // self.hk)
        max_tiles = max(1, self.Bmax // 2)
        self.h_prefix_blocks = torch.zeros(self.Bmax, dtype=torch.int32,
                                           pin_memory=pin)
        self.h_tiles = torch.zeros(max_tiles, 2 + 16, dtype=torch.int32,
                                   pin_memory=pin)
        self.d_prefix_blocks = torch.zeros(self.Bmax, dtype=torch.int32,
                                           device=d)
        self.d_tiles = torch.zeros(max_tiles, 2 + 16, dtype=torch.int32,
                                   device=d)
        self.n_prefix_blocks = self.h_prefix_blocks.numpy()
        self.n_tiles = self.h_tiles.numpy()
        self._groups_dirty = False      # row membership changed
        self._num_tiles = 0             # tiles in use after the last regroup
        self._tile_rows = 0             # rows in them
        # decode steps that took the shared path, and the rows that were
        # in tiles at the last decode step (0 if it was an unshared one)
        self.shared_prefix_steps = 0
        self.shared_prefix_rows = 0

    # ------------------------------------------------------------------
    def add_request(self, kv: SequenceKV, prompt_tokens: List[int],
                    sampling: SamplingParams) -> int:
        evicted = kv.num_tokens == 0 and bool(kv.history)
        if (sampling.max_new_tokens == 0 and not prompt_tokens
                and kv.pending_token is None and not evicted):
            raise ValueError("prefill-only request with nothing to prefill")
        rid = self._next_id
        self._next_id += 1
        self._known_kvs[id(kv)] = kv
        prompt = list(prompt_tokens)
        if kv.pending_token is not None:
            prompt.insert(0, kv.pending_token)
            kv.pending_token = None
        if kv.num_tokens == 0 and kv.history:
            # session was evicted while idle: rebuild the whole context
            # by prefilling its history ahead of the new tokens
            prompt = list(kv.history) + prompt
            kv.history = []
        if kv.num_tokens + len(prompt) + sampling.max_new_tokens > \
                self.ecfg.max_model_len:
            raise ValueError("request exceeds max_model_len")
        self.waiting.append(Request(rid, kv, prompt, sampling,
                                    ctx_start=kv.num_tokens))
        return rid

    def _host_tier(self) -> HostKVPool:
        """The pool that a session's host blocks live in."""
        if self.host_kv is None:
            raise RuntimeError("a session holds host KV blocks but the "
                               "engine has no host tier")
        return self.host_kv

    def _free_host_blocks(self, kv: SequenceKV) -> None:
        if kv.host_blocks:
            self._host_tier().allocator.free(kv.host_blocks)
            kv.host_blocks = []
            self.swapped_sessions -= 1

    def _swap_in(self, kv: SequenceKV,
                 blocks: Optional[List[int]] = None) -> None:
        """Bring kv's host blocks back into device blocks (`blocks`, or
        newly allocated ones), behind the ones that stayed."""
        n = len(kv.host_blocks)
        assert n > 0
        tier = self._host_tier()
        if blocks is None:
            blocks = self.kv.allocator.alloc(n)
        tier.load(kv.host_blocks, blocks)
        kv.blocks.extend(blocks)
        kv.host_blocks = []
        self.swapped_sessions -= 1
        self.swap_in_blocks += n

    def free_sequence(self, kv: SequenceKV) -> None:
        self.kv.allocator.free(kv.blocks)
        self._free_host_blocks(kv)
        kv.blocks = []
        kv.num_tokens = 0
        kv.pending_token = None
        kv.history = []

    def fork_sequence(self, src: SequenceKV, n: int = 1) -> List[SequenceKV]:
        """Fork `n` children that start from `src`'s context without
        prefilling it again: they share its full blocks and each get a copy
        of its partially filled tail block (one kv_copy_blocks launch for
        the whole call, enqueued on the current stream before returning).
        `src` must have no active request — its tail is being written
        otherwise. MemoryError (pool cannot supply the tail blocks) leaves
        every reference count as it was. An evicted source forks to
        children that carry only its history and re-prefill like it; one
        swapped out to the host tier is swapped in first, and a MemoryError
        leaves it swapped out.

        Sharing is safe without copy-on-write because shared blocks are
        immutable: only blocks wholly below num_tokens are shared, that
        holds for every holder (a child starts at the parent's num_tokens
        and both only grow), and nothing in the engine writes below
        num_tokens — prefill append, the fused decode kernel and the
        stop-token rollback all act at or above it. The block a session
        appends to is therefore always its own."""
        if n < 1:
            raise ValueError("fork_sequence needs n >= 1")
        if any(r.kv is src for r in self.waiting) or \
                any(r is not None and r.kv is src for r in self._rows):
            raise ValueError("cannot fork a session with an active request")
        bs = self.ecfg.block_size
        full, tail = divmod(src.num_tokens, bs)
        alloc = self.kv.allocator
        # first, and the only step that can fail: nothing to undo. A source
        # swapped out to the host tier comes back first, its blocks taken in
        # the same all-or-nothing allocation as the tails.
        back = len(src.host_blocks)
        want = back + (n if tail else 0)
        got = alloc.alloc(want) if want else []
        tails = got[back:]
        if back:
            self._swap_in(src, got[:back])
        shared = src.blocks[:full]
        children = []
        for i in range(n):
            alloc.share(shared)
            kv = SequenceKV(bs)
            # surplus blocks src reserved beyond its context stay its own
            kv.blocks = shared + tails[i:i + 1]
            kv.num_tokens = src.num_tokens
            kv.history = list(src.history)
            kv.pending_token = src.pending_token
            self._known_kvs[id(kv)] = kv
            children.append(kv)
        if tails:
            assert src.blocks[full] not in tails
            dev = self.device
            ops.kv_copy_blocks(
                self.kv.k, self.kv.v,
                torch.tensor([src.blocks[full]] * n, dtype=torch.int32,
                             device=dev),
                torch.tensor(tails, dtype=torch.int32, device=dev))
        return children

    def has_work(self) -> bool:
        return bool(self.waiting) or self.num_running > 0

    # ------------------------------------------------------------------
    def step(self) -> List[StepOutput]:
        import kukeon_amd.parallel as parallel
        if parallel.ep_size() > 1:
            return self._step_ep_lockstep()
        return self._step_local()

    def _step_ep_lockstep(self) -> List[StepOutput]:
        """EP serving: every MoE forward is a collective, so all EP
        ranks must make the SAME number of model passes. Per lockstep
        round each rank contributes exactly ONE pass — a real step
        (decode micro-batch forced to 1) or a participation pass that
        only serves this rank's experts. The caller (modelhub engine
        loop) exchanges the has-work flag so idle ranks keep
        participating while any rank still serves."""
        from kukeon_amd.models.mixtral import MixtralModel
        self.ecfg.decode_microbatch = 1  # one pass per step, always
        before = MixtralModel.pass_count
        outs = self._step_local() if self.has_work() else []
        made = MixtralModel.pass_count - before
        assert made <= 1, f"EP lockstep violated: {made} passes in a step"
        if made == 0:
            self.model.participate()
        return outs

    def _step_local(self) -> List[StepOutput]:
        if self.waiting:
            batch, blocked = self._admit_prefill()
            # several small idle sessions may need to go before the head
            # request fits: keep evicting until admission unblocks or no
            # victims remain (single-evict crashed on spread-out
            # idle context even though capacity existed)
            while not batch and blocked and self._evict_idle_kv():
                batch, blocked = self._admit_prefill()
            if batch:
                return self._run_prefill(batch)
            if blocked and self.num_running == 0:
                # nothing running to make progress, nothing left to evict:
                # the head request alone cannot ever fit
                req = self.waiting[0]
                raise MemoryError(
                    f"request {req.req_id} cannot be admitted: needs more "
                    "KV blocks than the pool holds even with every idle "
                    "session evicted")
        if self.num_running > 0:
            return self._run_decode()
        return []

    def _evict_idle_kv(self) -> bool:
        """Evict the KV of an idle session (resident context, no active
        request) to unblock admission; its history stays so the next
        request on that session transparently re-prefills the context.
        Sessions idle in HBM are the norm for agent serving — without
        this, resident-but-idle context starves new admissions forever.
        With a host tier (kv_host_blocks > 0) the victim's exclusive blocks
        are swapped out instead (_swap_out) and its next turn copies them
        back; it is dropped as above only when that cannot be done. Every
        call that returns True shortens some session's block list."""
        active = {id(r.kv) for r in self.waiting}
        active.update(id(r.kv) for r in self._rows if r is not None)
        # rank by what the eviction returns to the pool: blocks shared with
        # a forked session only lose a reference. A session that returns
        # none stays a candidate, last — dropping its references is what
        # later makes the co-owner's blocks releasable.
        victim, gain = None, -1
        for kv in self._known_kvs.values():
            if id(kv) in active or not kv.blocks:
                continue
            g = self.kv.allocator.num_exclusive(kv.blocks)
            if g > gain:
                victim, gain = kv, g
        if victim is None:
            return False
        if self.host_kv is not None and self._swap_out(victim):
            return True
        log.info("evicting idle session KV (%d blocks, %d to the pool) to "
                 "unblock admission", len(victim.blocks), gain)
        self.swap_fallbacks += self.host_kv is not None
        self.kv.allocator.free(victim.blocks)
        self._free_host_blocks(victim)
        victim.blocks = []
        victim.num_tokens = 0
        return True

    def _swap_out(self, kv: SequenceKV) -> bool:
        """Move an idle session's exclusive blocks to the host tier instead
        of dropping them: num_tokens and history stay, kv.blocks keeps what
        stayed on the device and kv.host_blocks names the rest, in position
        order. Blocks shared with a fork are a prefix of the list (forks
        share src.blocks[:full]) and stay where they are with their
        references, so sharing and shared-prefix decode survive; what moves
        is the longest suffix of the blocks covering num_tokens that only
        this session holds. Blocks reserved beyond num_tokens are freed.
        -> False, with nothing changed, when that suffix is empty or the
        host pool cannot take it. The device blocks go back to the free
        list as soon as the copies are enqueued: whatever writes them next
        is enqueued behind those on the same stream."""
        alloc = self.kv.allocator
        bs = self.ecfg.block_size
        # device blocks that cover context; a session swapped out before
        # (its shared prefix has since become its own) has the rest on the
        # host already
        cover = (kv.num_tokens + bs - 1) // bs - len(kv.host_blocks)
        first = cover
        while first > 0 and alloc.num_exclusive(kv.blocks[first - 1:first]):
            first -= 1
        moving = kv.blocks[first:cover]
        if not moving or len(moving) > self.host_kv.allocator.num_free:
            return False
        log.info("swapping idle session KV to the host (%d of %d blocks) to "
                 "unblock admission", len(moving), len(kv.blocks))
        stored = self.host_kv.store(moving)
        self.swapped_sessions += not kv.host_blocks
        kv.host_blocks = stored + kv.host_blocks
        alloc.free(kv.blocks[first:])
        del kv.blocks[first:]
        self.swap_out_blocks += len(moving)
        return True

    # ------------------------------------------------------------------
    def _admit_prefill(self):
        """-> ([(request, chunk_len)], blocked_on_blocks); a chunk smaller
        than the remaining prompt keeps the request at the front of the
        queue (chunked prefill for prompts beyond the per-step token
        budget)."""
        batch: List[Tuple[Request, int]] = []
        blocked = False
        tokens = 0
        free = self.kv.allocator.num_free
        avail_rows = len(self._free_rows)
        budget = self.ecfg.max_prefill_tokens
        # soft tail: a request whose remainder only slightly overflows the
        # budget is admitted whole rather than leaving a tiny (<1/16
        # budget) chunk for a full extra model pass next step — at 64
        # sessions x 257 tokens vs a 16384 budget the hard cutoff cost an
        # entire 64-token full-layer sweep (~a decode step) per turn.
        slack = budget // 16
        while self.waiting and tokens < budget:
            req = self.waiting[0]
            # a prefill-only request (max_new_tokens == 0) takes no row
            wants_row = req.sampling.max_new_tokens > 0
            if wants_row and avail_rows <= 0:
                break
            remaining = len(req.prompt_tokens) - req.prefill_pos
            chunk = min(remaining, budget - tokens)
            if 0 < remaining - chunk <= slack and tokens + remaining <= \
                    budget + slack:
                chunk = remaining
            if chunk <= 0:
                break
            finishing = (req.prefill_pos + chunk) == len(req.prompt_tokens)
            reserve = chunk + (req.sampling.max_new_tokens if finishing
                               else 0)
            need = req.kv.blocks_needed(reserve)
            if need > free:
                blocked = True
                break
            free -= need
            tokens += chunk
            if finishing:
                avail_rows -= wants_row
                batch.append((self.waiting.pop(0), chunk))
            else:
                batch.append((req, chunk))
                break  # a partial chunk consumes the whole budget
        return batch, blocked

    def _alloc_for(self, req: Request, new_tokens: int) -> List[int]:
        need = req.kv.blocks_needed(new_tokens)
        if need:
            req.kv.blocks.extend(self.kv.allocator.alloc(need))
        slots = req.kv.slots_for(new_tokens)
        req.kv.num_tokens += new_tokens
        return slots

    # ------------------------------------------------------------------
    def _run_prefill(self, batch: List[Tuple[Request, int]]) -> List[StepOutput]:
        dev = self.device
        ids, pos, slots = [], [], []
        qs_pairs, qb_seq, qb_start = [], [], []
        row = 0
        for s, (req, chunk) in enumerate(batch):
            toks = req.prompt_tokens[req.prefill_pos:
                                     req.prefill_pos + chunk]
            if req.kv.host_blocks:
                # swapped out while idle: admission counted these blocks
                # (blocks_needed sees only kv.blocks), so this cannot fail;
                # the turn then continues at num_tokens like a resident one
                self._swap_in(req.kv)
            start = req.kv.num_tokens
            sl = self._alloc_for(req, chunk)
            req.kv.history.extend(toks)
            ids.extend(toks)
            pos.extend(range(start, start + chunk))
            slots.extend(sl)
            qs_pairs.append((start, row))
            for qb in range(0, chunk, 32):
                qb_seq.append(s)
                qb_start.append(qb)
            row += chunk
            req.prefill_pos += chunk
        t_ids = torch.tensor(ids, dtype=torch.int32, device=dev)
        t_pos = torch.tensor(pos, dtype=torch.int32, device=dev)
        t_slots = torch.tensor(slots, dtype=torch.int32, device=dev)
        t_seq_lens = torch.tensor([r.kv.num_tokens for r, _ in batch],
                                  dtype=torch.int32, device=dev)
        t_qs = torch.tensor(qs_pairs, dtype=torch.int32, device=dev)
        mbt = max(len(r.kv.blocks) for r, _ in batch)
        bt = torch.zeros(len(batch), mbt, dtype=torch.int32)
        for i, (r, _) in enumerate(batch):
            bt[i, : len(r.kv.blocks)] = torch.tensor(r.kv.blocks,
                                                     dtype=torch.int32)
        meta = AttnMeta(mode="prefill", positions=t_pos, slot_mapping=t_slots,
                        block_table=bt.to(dev), seq_lens=t_seq_lens,
                        q_starts=t_qs,
                        qb_seq=torch.tensor(qb_seq, dtype=torch.int32,
                                            device=dev),
                        qb_start=torch.tensor(qb_start, dtype=torch.int32,
                                              device=dev))
        hidden = self.model.forward(t_ids, self.kv.k, self.kv.v, meta)
        # sample only the requests whose prompt completed this pass; a
        # prefill-only one (max_new_tokens == 0) ends here with no token,
        # no row and nothing pending
        outs, sampled, last_rows, acc = [], [], [], 0
        for r, chunk in batch:
            acc += chunk
            if r.prefill_pos != len(r.prompt_tokens):
                continue
            if r.sampling.max_new_tokens == 0:
                r.finished = True
                outs.append(StepOutput(r.req_id, [], True))
            else:
                sampled.append(r)
                last_rows.append(acc - 1)
        if not sampled:
            return outs
        logits = self.model.compute_logits(
            hidden[torch.tensor(last_rows, dtype=torch.long, device=dev)])
        toks = self._sample_eager(sampled, logits)
        return outs + [self._append_token(r, t)
                       for r, t in zip(sampled, toks)]

    def _sample_eager(self, reqs: List[Request], logits: torch.Tensor):
        B = len(reqs)
        dev = self.device
        temps = torch.tensor([r.sampling.temperature for r in reqs],
                             dtype=torch.float32, device=dev)
        tk = torch.tensor([r.sampling.top_k for r in reqs], dtype=torch.int32,
                          device=dev)
        tp = torch.tensor([r.sampling.top_p for r in reqs],
                          dtype=torch.float32, device=dev)
        tokens = torch.zeros(B, dtype=torch.int32, device=dev)
        ops.sample(tokens, logits.contiguous(), temps, tk, tp, self.d_seed,
                   self.d_ws[:B])
        return tokens.cpu().tolist()

    # ------------------------------------------------------------------
    def _assign_row(self, req: Request) -> None:
        row = self._free_rows.pop()
        req.row = row
        req.bt_written = 0
        self._rows[row] = req
        self.num_running += 1
        self.h_params[row, 0] = req.sampling.temperature
        self.h_params[row, 1] = float(req.sampling.top_k)
        self.h_params[row, 2] = req.sampling.top_p
        self._params_dirty = True
        self._groups_dirty = True

    def _release_row(self, req: Request) -> None:
        if req.row >= 0:
            # also how _preempt and cancel take a row out of its group
            self._groups_dirty = True
            self._rows[req.row] = None
            self._free_rows.append(req.row)
            self.n_slots[req.row] = -1
            self.n_seq_lens[req.row] = 0
            req.row = -1
            self.num_running -= 1

    def cancel(self, rid: int) -> bool:
        """Abort a request at the next step boundary (client went away /
        explicit cancel verb). Must run on the engine thread (the server
        routes it through the submit queue). The session's KV keeps the
        already-computed prefix — the turn just ends early, exactly like
        a stop token at the last emitted position."""
        for i, r in enumerate(self.waiting):
            if r.req_id == rid:
                self.waiting.pop(i)
                r.finished = True
                if r.output_tokens:
                    r.kv.pending_token = r.output_tokens[-1]
                return True
        for r in self._rows:
            if r is not None and r.req_id == rid:
                r.finished = True
                if r.output_tokens:
                    r.kv.pending_token = r.output_tokens[-1]
                self._release_row(r)
                return True
        return False

    def _append_token(self, req: Request, tok: int) -> StepOutput:
        req.output_tokens.append(tok)
        if (len(req.output_tokens) >= req.sampling.max_new_tokens
                or tok in (req.sampling.stop_token_ids or ())):
            req.finished = True
            req.kv.pending_token = tok
            self._release_row(req)
        elif req.row < 0:
            self._assign_row(req)
        return StepOutput(req.req_id, [tok], req.finished)

    # ------------------------------------------------------------------
    def _bucket(self, b: int) -> int:
        for s in self.ecfg.graph_buckets:
            if b <= s:
                return min(s, self.Bmax)
        return self.Bmax

    def _decode_splits(self, bucket: int) -> int:
        # target ~4096 split slots: the decode kernel runs B*Hk*S waves,
        # one per slot, and 4096 exactly fills the chip at its
        # 4-waves/SIMD occupancy. Launch plan (paged_attn.hip): S <= 4
        # runs one 4-wave workgroup per (sequence, kv head), 5..8 one
        # 8-wave workgroup, and that workgroup merges its own splits —
        # decode attention is a single launch. S > 8 (buckets below 64
        # here) runs 4-wave workgroups into the workspaces plus the reduce
        # kernel. A multiple of 4 keeps every workgroup's waves busy.
        want = (16 * 256 + bucket * self.hk - 1) // (bucket * self.hk)
        return max(4, min(self.max_splits, ((want + 3) // 4) * 4))

    def _prefix_splits(self, bucket: int) -> int:
        # the prefix kernel runs tiles * Hk * prefix_splits waves; a bucket
        # whose rows are all grouped has bucket / tile_width tiles. Unlike
        # a suffix split, a prefix split costs every member row a
        # workspace slot that the reduce kernel reads back, so that case
        # is given a quarter of the 4096 waves of _decode_splits, but at
        # least 8 splits, as a multiple of 4 for the 4-wave workgroups
        # and capped like the suffix's: 8 at bucket 64 for both the 8B
        # (16 tiles) and the 70B shape (32 tiles), where 8 measured
        # fastest of 4 / 8 / 16 / 32 (docs/perf.md). The graph of a bucket
        # is captured once, so the count cannot follow the tiles in use.
        tiles = max(1, bucket // max(1, self.tile_width))
        want = (4 * 256 + tiles * self.hk - 1) // (tiles * self.hk)
        return max(8, min(self.max_splits, ((want + 3) // 4) * 4))

    def _regroup(self) -> None:
        """Recompute the shared-prefix tiles of the running rows into the
        host staging buffers. Rows whose block lists begin with the same
        block id form a group (forks of one context; nested forks are not
        told apart: the group shares the prefix common to ALL rows with
        that first block, and a sub-family's longer common run is read per
        row). Its prefix is the longest run of block ids common to every
        member among the blocks wholly below every member's num_tokens. A
        group is used when it has at least 2 rows and at least
        shared_prefix_min_tokens tokens of prefix; it is cut into tiles of
        tile_width = 16 // (Hq // Hk) rows, and a lone leftover row stays
        ungrouped (alone it gains nothing), so there are never more than
        rows // 2 tiles. With tile_width 1 (GQA group of 16) nothing can
        share and the path stays off.

        Block lists only grow and shared blocks are immutable (see
        fork_sequence), so a prefix stays valid until row membership
        changes: _assign_row and _release_row (hence _preempt, cancel and a
        finished request) mark the groups dirty, and the next decode step
        calls this once."""
        self._groups_dirty = False
        bs = self.ecfg.block_size
        min_tokens = self.ecfg.shared_prefix_min_tokens
        W = self.tile_width
        tiles = []
        if min_tokens > 0 and W >= 2:
            by_first: Dict[int, List[int]] = {}
            for row, r in enumerate(self._rows):
                if r is not None and r.kv.blocks:
                    by_first.setdefault(r.kv.blocks[0], []).append(row)
            for rows in by_first.values():
                if len(rows) < 2:
                    continue
                kvs = [self._rows[row].kv for row in rows]
                limit = min(kv.num_tokens // bs for kv in kvs)
                first = kvs[0].blocks
                p = 0
                while p < limit and all(kv.blocks[p] == first[p]
                                        for kv in kvs[1:]):
                    p += 1
                if p == 0 or p * bs < min_tokens:
                    continue
                for i in range(0, len(rows), W):
                    if len(rows) - i >= 2:
                        tiles.append((p, rows[i:i + W]))
        self.n_prefix_blocks[:] = 0
        self.n_tiles[:] = 0
        for t, (p, rows) in enumerate(tiles):
            self.n_tiles[t, 0] = len(rows)
            self.n_tiles[t, 1] = p
            self.n_tiles[t, 2:2 + len(rows)] = rows
            self.n_prefix_blocks[rows] = p
        self._num_tiles = len(tiles)
        self._tile_rows = sum(len(rows) for _, rows in tiles)
        if tiles:
            ops.check_prefix_tiles(self.h_tiles[:len(tiles)],
                                   max(1, self.hq // self.hk))
        self.d_prefix_blocks.copy_(self.h_prefix_blocks, non_blocking=True)
        self.d_tiles.copy_(self.h_tiles, non_blocking=True)

    def _tmp_for(self, bucket: int, splits: int):
        key = (bucket, splits)
        if key not in self.d_tmp_out:
            self.d_tmp_out[key] = torch.zeros(
                bucket, self.hq, splits, self.cfg.head_dim,
                dtype=torch.float32, device=self.device)
            self.d_tmp_ml[key] = torch.zeros(bucket, self.hq, splits, 2,
                                             dtype=torch.float32,
                                             device=self.device)
        return self.d_tmp_out[key], self.d_tmp_ml[key]

    def _preempt(self, req: Request) -> None:
        """Evict a running request: free its KV and re-queue it for full
        recompute (history + its un-processed last token become the new
        prompt; already-emitted output_tokens are preserved)."""
        log.warning("preempting request %d (KV exhausted)", req.req_id)
        # only idle sessions are swapped out, and a turn swaps in first
        assert not req.kv.host_blocks
        self._release_row(req)
        history = list(req.kv.history)
        last = req.output_tokens[-1] if req.output_tokens else None
        self.kv.allocator.free(req.kv.blocks)
        req.kv.blocks = []
        req.kv.num_tokens = 0
        req.kv.history = []
        req.kv.pending_token = None
        req.prompt_tokens = history + ([last] if last is not None else [])
        req.prefill_pos = 0
        req.preempted += 1
        self.waiting.insert(0, req)

    def _run_decode(self) -> List[StepOutput]:
        """A micro-batch of k decode steps with ONE host sync: the graph is
        self-advancing (sampled tokens feed back on device, cursors advance
        in-kernel, tokens land in a ring buffer)."""
        active0 = [r for r in self._rows if r is not None]
        k = min(min(r.sampling.max_new_tokens - len(r.output_tokens)
                    for r in active0),
                max(1, self.ecfg.decode_microbatch), self.max_microbatch)
        # ---- alloc k tokens of KV per request (preempt on exhaustion) ----
        row = 0
        while row < self.Bmax:
            r = self._rows[row]
            if r is None:
                row += 1
                continue
            need = r.kv.blocks_needed(k)
            if need:
                try:
                    r.kv.blocks.extend(self.kv.allocator.alloc(need))
                except MemoryError:
                    actives = [x for x in self._rows if x is not None]
                    victim = actives[-1] if actives[-1] is not r else r
                    self._preempt(victim)
                    if victim is r:
                        row += 1
                    continue
            row += 1
        if self.num_running == 0:
            return []
        maxrow = max(i for i, r in enumerate(self._rows) if r is not None)
        nrows = maxrow + 1
        active = []
        for row in range(nrows):
            r = self._rows[row]
            if r is None:
                self.n_seq_lens[row] = 0
                continue
            active.append((row, r))
            start = r.kv.num_tokens
            self.n_ids[row] = r.output_tokens[-1]
            self.n_pos[row] = start
            self.n_seq_lens[row] = start + 1
            n = len(r.kv.blocks)
            if n > r.bt_written:
                self.n_bt[row, r.bt_written: n] = r.kv.blocks[r.bt_written:]
                r.bt_written = n
        use_graph = self.is_cuda and self.ecfg.use_graphs
        bucket = self._bucket(nrows) if use_graph else nrows
        for row in range(nrows):
            if self._rows[row] is None:
                self.n_pos[row] = -1   # rope kernel skips the KV write
        for row in range(nrows, bucket):
            self.n_seq_lens[row] = 0
            self.n_pos[row] = -1
        nb = bucket
        self.d_ids[:nb].copy_(self.h_ids[:nb], non_blocking=True)
        self.d_pos[:nb].copy_(self.h_pos[:nb], non_blocking=True)
        self.d_seq_lens[:nb].copy_(self.h_seq_lens[:nb], non_blocking=True)
        self.d_bt[:nb].copy_(self.h_bt[:nb], non_blocking=True)
        if self._params_dirty:
            self.d_temps.copy_(self.h_params[:, 0], non_blocking=True)
            self.d_topk.copy_(self.h_params[:, 1].to(torch.int32),
                              non_blocking=True)
            self.d_topp.copy_(self.h_params[:, 2], non_blocking=True)
            self._params_dirty = False
        self.d_step.zero_()
        # the shared-prefix path: taken when at least one group qualifies;
        # tiles and prefix lengths are staged only when membership changed
        enabled = self.ecfg.shared_prefix_min_tokens > 0
        if enabled and self._groups_dirty:
            self._regroup()
        shared = enabled and self._num_tiles > 0
        graphs = self.shared_graphs if shared else self.graphs
        if use_graph and bucket not in graphs:
            # capture AFTER the staging copies: the warmup forward then runs
            # on the real current state (its KV writes land exactly where
            # the first replay re-writes the same values), never on stale
            # block tables pointing at freed blocks.
            self._capture_safely(bucket, shared)
        if use_graph:
            g = graphs[bucket]
            for _ in range(k):
                g.replay()
        else:
            for _ in range(k):
                self._decode_forward(bucket, shared)
        self.shared_prefix_steps += k if shared else 0
        self.shared_prefix_rows = self._tile_rows if shared else 0
        slab = self.d_ring[: k * bucket].view(k, bucket)[:, :nrows].cpu()
        outs = []
        for row, r in active:
            toks = [int(t) for t in slab[:, row]]
            prev = r.output_tokens[-1]
            r.kv.history.extend([prev] + toks[:-1])
            r.kv.num_tokens += k
            fin = False
            emitted = []
            for i, t in enumerate(toks):
                emitted.append(t)
                fin = self._append_token(r, t).finished
                if fin and i + 1 < k:
                    # stop token mid-microbatch: the device already
                    # advanced KV/history for the discarded tail — roll
                    # the host counters back so the next turn's context
                    # ends at the stop token (staging re-derives
                    # pos/seq_lens from kv.num_tokens)
                    extra = k - (i + 1)
                    r.kv.num_tokens -= extra
                    del r.kv.history[len(r.kv.history) - extra:]
                    break
                if fin:
                    break
            outs.append(StepOutput(r.req_id, emitted, fin))
        return outs

    def _decode_forward(self, B: int, shared: bool = False) -> None:
        splits = self._decode_splits(B)
        if shared:
            # B // 2 tiles is the most _regroup can make of B rows; the
            # workspaces grow by the prefix slots for this path only
            psplits = self._prefix_splits(B)
            tmp_out, tmp_ml = self._tmp_for(B, psplits + splits)
            meta = AttnMeta(
                mode="decode", positions=self.d_pos[:B],
                slot_mapping=self.d_slots[:B], block_table=self.d_bt[:B],
                seq_lens=self.d_seq_lens[:B], num_splits=splits,
                tmp_out=tmp_out, tmp_ml=tmp_ml,
                prefix_blocks=self.d_prefix_blocks[:B],
                prefix_tiles=self.d_tiles[:max(1, B // 2)],
                prefix_splits=psplits)
        else:
            tmp_out, tmp_ml = self._tmp_for(B, splits)
            meta = AttnMeta(
                mode="decode", positions=self.d_pos[:B],
                slot_mapping=self.d_slots[:B], block_table=self.d_bt[:B],
                seq_lens=self.d_seq_lens[:B], num_splits=splits,
                tmp_out=tmp_out, tmp_ml=tmp_ml)
        hidden = self.model.forward(self.d_ids[:B], self.kv.k, self.kv.v, meta)
        logits = self.model.compute_logits(hidden)
        ops.sample(self.d_tokens[:B], logits, self.d_temps[:B],
                   self.d_topk[:B], self.d_topp[:B], self.d_seed,
                   self.d_ws[:B])
        ops.decode_advance(self.d_ids[:B], self.d_pos[:B],
                           self.d_seq_lens[:B], self.d_tokens[:B],
                           self.d_ring, self.d_step)

    def _capture_safely(self, bucket: int, shared: bool = False) -> None:
        """Capture a bucket graph mid-serving: the warmup forward mutates
        the self-advancing cursors, so snapshot and restore them."""
        saved = (self.d_ids.clone(), self.d_pos.clone(),
                 self.d_seq_lens.clone(), self.d_step.clone())
        self._capture(bucket, shared)
        self.d_ids.copy_(saved[0])
        self.d_pos.copy_(saved[1])
        self.d_seq_lens.copy_(saved[2])
        self.d_step.copy_(saved[3])
        if self.is_cuda:
            torch.cuda.synchronize()

    def _capture(self, bucket: int, shared: bool = False) -> None:
        log.info("capturing %sdecode graph for bucket %d",
                 "shared-prefix " if shared else "", bucket)
        torch.cuda.synchronize()
        # warm up allocator + BLAS heuristics
        self._decode_forward(bucket, shared)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=self._graph_pool):
            self._decode_forward(bucket, shared)
        if self._graph_pool is None:
            self._graph_pool = g.pool()
        (self.shared_graphs if shared else self.graphs)[bucket] = g
        torch.cuda.synchronize()

    def capture_all(self) -> None:
        """Pre-capture decode buckets before serving (safe buffer state)."""
        if not (self.is_cuda and self.ecfg.use_graphs):
            return
        self.d_slots.fill_(-1)
        self.d_seq_lens.zero_()
        self.d_ids.zero_()
        self.d_pos.fill_(-1)   # rope kernel skips KV writes for pos < 0
        for b in sorted(self.ecfg.graph_buckets, reverse=True):
            b = min(b, self.Bmax)
            if b not in self.graphs:
                self._capture(b)
