"""Host KV tier on CPU (tiny model, reference ops): the pack/unpack layout,
swap instead of drop for idle sessions, the fallbacks, swaps under fork
sharing, block conservation under random traffic, and the server's flags,
stats and release."""
import random
import uuid

import pytest
import torch

from kukeon_amd import ops
from kukeon_amd.engine.config import (EngineConfig, SamplingParams,
                                      tiny_llama)
from kukeon_amd.engine.engine import LLMEngine
from kukeon_amd.engine.kv_cache import SequenceKV
from kukeon_amd.models.llama import LlamaModel
from kukeon_amd.serve.server import (ModelhubClient, ModelhubServer,
                                     build_parser, kv_host_blocks_for)

BS = 16


def make_engine(num_kv_blocks=256, max_sessions=8, max_model_len=512, **kw):
    torch.manual_seed(0)
    cfg = tiny_llama()
    ecfg = EngineConfig(max_model_len=max_model_len,
                        max_sessions=max_sessions,
                        num_kv_blocks=num_kv_blocks, use_graphs=False, **kw)
    return LLMEngine(LlamaModel(cfg, device="cpu"), cfg, ecfg, device="cpu")


def toks(n, salt):
    return [(salt * 131 + i * 29 + 7) % 512 for i in range(n)]


def run(engine, kv, prompt, n_new):
    rid = engine.add_request(kv, prompt, SamplingParams(temperature=0.0,
                                                        max_new_tokens=n_new))
    out = []
    while engine.has_work():
        for o in engine.step():
            if o.req_id == rid:
                out.extend(o.new_tokens)
    return out


def new_kv():
    return SequenceKV(BS)


def gathered(engine, kv, t=None):
    """K and V of positions [0, t) as the block table addresses them."""
    t = kv.num_tokens if t is None else t
    assert len(kv.blocks) * BS >= t
    idx = torch.tensor([kv.blocks[p // BS] for p in range(t)],
                       dtype=torch.long)
    off = torch.tensor([p % BS for p in range(t)], dtype=torch.long)
    return (engine.kv.k[:, idx, :, off].clone().view(torch.int16),
            engine.kv.v[:, idx, :, off].clone().view(torch.int16))


def assert_clean(engine):
    a = engine.kv.allocator
    assert a.num_free == a.num_blocks and a.num_shared == 0
    if engine.host_kv is not None:
        h = engine.host_kv.allocator
        assert h.num_free == h.num_blocks
    assert engine.swapped_sessions == 0


# ---- layout ------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.uint8])
def test_reference_pack_layout_and_unpack(dtype):
    g = torch.Generator().manual_seed(1)
    shape = (3, 12, 2, BS, 8)
    k = torch.randint(0, 200, shape, generator=g).to(dtype)
    v = torch.randint(0, 200, shape, generator=g).to(dtype)
    k0, v0 = k.clone(), v.clone()
    blocks = torch.tensor([7, 0, 11, 3], dtype=torch.int32)
    staging = torch.full((6, 2) + (3, 2, BS, 8), 99).to(dtype)
    ops.kv_pack_blocks(k, v, blocks, staging)
    assert torch.equal(k, k0) and torch.equal(v, v0)
    for i, b in enumerate(blocks.tolist()):
        assert torch.equal(staging[i], torch.stack([k[:, b], v[:, b]]))
    assert (staging[4:] == 99).all()          # records n..cap untouched
    # the record is one contiguous run: K of every layer, then V
    assert torch.equal(staging[0].reshape(2, -1)[0], k[:, 7].reshape(-1))
    # unpack into other blocks: those equal the sources, nothing else moves
    dst = torch.tensor([1, 2, 4, 5], dtype=torch.int32)
    ops.kv_unpack_blocks(staging, k, v, dst)
    ek, ev = k0.clone(), v0.clone()
    ek[:, dst.long()] = k0[:, blocks.long()]
    ev[:, dst.long()] = v0[:, blocks.long()]
    assert torch.equal(k, ek) and torch.equal(v, ev)
    # an empty list does nothing
    none = torch.empty(0, dtype=torch.int32)
    ops.kv_pack_blocks(k, v, none, staging)
    ops.kv_unpack_blocks(staging, k, v, none)
    assert torch.equal(k, ek) and torch.equal(v, ev)


# ---- swap instead of drop ----------------------------------------------
PROMPT = [7, 3, 9] * 14      # 42 tokens; with 6 decoded a session is 3 blocks


def test_idle_session_is_swapped_not_dropped():
    # 8 blocks = 128 tokens: three sessions of ~48 tokens cannot all stay
    engine = make_engine(num_kv_blocks=8, max_sessions=2, max_model_len=256,
                         kv_host_blocks=16, kv_swap_staging_blocks=2)
    control = make_engine(num_kv_blocks=256, max_sessions=2,
                          max_model_len=256)
    kvs = [new_kv() for _ in range(3)]
    # a prompt of its own per session: a restore from another session's
    # host blocks would show in the bits
    prompts = [toks(42, 40 + i) for i in range(3)]
    before, outs = [], []
    for kv, prompt in zip(kvs, prompts):
        outs.append(run(engine, kv, prompt, 6))
        before.append(gathered(engine, kv))   # end of its own turn
    assert not torch.equal(before[0][0], before[1][0])
    assert not torch.equal(before[1][0], before[2][0])
    assert all(len(o) == 6 for o in outs)
    swapped = [i for i, kv in enumerate(kvs) if kv.host_blocks]
    assert swapped, "at least one idle session should have been swapped out"
    assert engine.swapped_sessions == len(swapped)
    assert engine.swap_out_blocks > 0 and engine.swap_fallbacks == 0
    i = swapped[0]
    kv = kvs[i]
    n0 = kv.num_tokens
    assert n0 == 42 + 6 - 1 and kv.history == prompts[i] + outs[i][:-1]
    assert len(kv.blocks) + len(kv.host_blocks) == (n0 + BS - 1) // BS
    host_free = engine.host_kv.allocator.num_free
    assert host_free == 16 - sum(len(s.host_blocks) for s in kvs)

    # the follow-up turn swaps in and continues; same tokens as a session
    # with the same history that was never evicted
    ckv = new_kv()
    assert run(control, ckv, prompts[i], 6) == outs[i]
    got = run(engine, kv, [5, 1], 4)
    assert got == run(control, ckv, [5, 1], 4)
    assert ckv.blocks and control.kv.allocator.num_free == 256 - len(ckv.blocks)
    assert not kv.host_blocks and kv.num_tokens == n0 + 1 + 2 + 4 - 1
    assert engine.swap_in_blocks > 0 and engine.swap_out_blocks > 0
    # the restored KV has the bits the session decoded with
    k1, v1 = gathered(engine, kv, n0)
    assert torch.equal(k1, before[i][0]) and torch.equal(v1, before[i][1])
    assert before[i][0].any() and before[i][1].any()
    for s in kvs:
        engine.free_sequence(s)
    assert_clean(engine)


@pytest.mark.parametrize("host_blocks", [0, 1])
def test_tier_off_or_too_small_drops_as_before(host_blocks):
    engine = make_engine(num_kv_blocks=8, max_sessions=2, max_model_len=256,
                         kv_host_blocks=host_blocks)
    kvs = [new_kv() for _ in range(3)]
    outs = [run(engine, kv, PROMPT, 6) for kv in kvs]
    assert all(len(o) == 6 for o in outs)
    evicted = [kv for kv in kvs if not kv.blocks]
    assert evicted
    for kv in evicted:
        assert kv.num_tokens == 0 and kv.host_blocks == [] and kv.history
    assert all(kv.host_blocks == [] for kv in kvs)
    assert engine.swap_out_blocks == 0 and engine.swapped_sessions == 0
    if host_blocks:
        assert engine.swap_fallbacks == len(evicted)
        assert engine.host_kv.allocator.num_free == host_blocks
    else:
        assert engine.swap_fallbacks == 0 and engine.host_kv is None
    # the dropped session still rebuilds from its history
    kv = evicted[0]
    hist = len(kv.history)
    assert len(run(engine, kv, [5, 1], 4)) == 4
    assert kv.num_tokens == hist + 1 + 2 + 4 - 1


def test_repeated_eviction_of_swapped_sessions():
    """Evicting on until nothing is left: a swapped session whose device
    remainder is all shared is dropped whole, host blocks included; one
    whose remainder has become its own has it swapped out in front of what
    the host already holds."""
    engine = make_engine(num_kv_blocks=8, kv_host_blocks=8)
    parent = new_kv()
    run(engine, parent, toks(21, 1), 0)
    (child,) = engine.fork_sequence(parent)
    run(engine, child, toks(20, 2), 0)        # 41 tokens: shared + 2 own
    k0, v0 = gathered(engine, child)
    shared = child.blocks[0]
    assert engine._swap_out(child)
    assert child.blocks == [shared] and len(child.host_blocks) == 2
    assert not engine._swap_out(child)        # nothing exclusive is left
    # the parent's own tail is all an eviction can return to the pool now
    assert engine._evict_idle_kv()
    assert parent.blocks == [shared] and len(parent.host_blocks) == 1
    assert engine.swap_fallbacks == 0
    # neither session returns anything; the first known one is dropped
    assert engine._evict_idle_kv()
    assert parent.blocks == [] and parent.host_blocks == []
    assert parent.num_tokens == 0 and parent.history == toks(21, 1)
    assert engine.swap_fallbacks == 1
    assert engine.host_kv.allocator.num_free == 8 - 2
    # which made the shared block the child's own: it follows to the host
    assert engine._evict_idle_kv()
    assert child.blocks == [] and len(child.host_blocks) == 3
    assert child.num_tokens == 41 and engine.swap_out_blocks == 2 + 1 + 1
    assert not engine._evict_idle_kv()
    assert engine.kv.allocator.num_free == 8
    control = make_engine()
    ckv = new_kv()
    run(control, ckv, toks(21, 1), 0)
    run(control, ckv, toks(20, 2), 0)
    assert run(engine, child, toks(3, 3), 4) == run(control, ckv, toks(3, 3), 4)
    k1, v1 = gathered(engine, child, 41)
    assert torch.equal(k0, k1) and torch.equal(v0, v1)
    engine.free_sequence(parent)
    engine.free_sequence(child)
    assert_clean(engine)


# ---- forks -------------------------------------------------------------
P = toks(21, 1)              # one full block plus a tail of 5


def test_fork_child_swaps_only_its_exclusive_suffix():
    control = make_engine()
    ckv = new_kv()
    run(control, ckv, P, 0)
    want_a = run(control, ckv, toks(20, 2), 5)
    want_a2 = run(control, ckv, toks(3, 4), 4)

    # the parent holds 2 blocks and each child 2 of its own: 6 of 7
    engine = make_engine(num_kv_blocks=7, kv_host_blocks=8,
                         kv_swap_staging_blocks=2)
    parent = new_kv()
    run(engine, parent, P, 0)
    a, b = engine.fork_sequence(parent, 2)
    assert run(engine, a, toks(20, 2), 5) == want_a
    run(engine, b, toks(20, 3), 5)
    alloc = engine.kv.allocator
    assert alloc.num_shared == 1 and alloc.num_free == 1
    first = a.blocks[0]
    assert first == parent.blocks[0] == b.blocks[0]
    k0, v0 = gathered(engine, a)
    # a newcomer needs 3 blocks: a child (2 exclusive blocks against the
    # parent's 1) is the victim
    other = new_kv()
    run(engine, other, toks(30, 9), 4)
    victims = [kv for kv in (a, b) if kv.host_blocks]
    assert len(victims) == 1 and not parent.host_blocks
    vic = victims[0]
    assert vic.blocks == [first] and len(vic.host_blocks) == 2
    assert vic.num_tokens == 21 + 20 + 5 - 1
    assert alloc.num_shared == 1              # the prefix is still shared
    assert engine.swap_out_blocks == 2
    if vic is b:
        # make `a` the swapped one as well, so the control's tokens apply
        assert engine._swap_out(a)
    assert a.blocks == [first] and len(a.host_blocks) == 2
    engine.free_sequence(other)
    assert run(engine, a, toks(3, 4), 4) == want_a2
    assert a.blocks[0] == first and not a.host_blocks
    k1, v1 = gathered(engine, a, 21 + 20 + 5 - 1)
    assert torch.equal(k0, k1) and torch.equal(v0, v1)
    for kv in (parent, a, b):
        engine.free_sequence(kv)
    assert_clean(engine)


def test_fork_of_a_swapped_source():
    engine = make_engine(num_kv_blocks=16, kv_host_blocks=8,
                         kv_swap_staging_blocks=1)
    src = new_kv()
    run(engine, src, toks(37, 1), 0)          # two full blocks + tail of 5
    k0, v0 = gathered(engine, src)
    assert engine._swap_out(src)
    assert src.blocks == [] and len(src.host_blocks) == 3
    assert engine.kv.allocator.num_free == 16
    kids = engine.fork_sequence(src, 2)
    assert not src.host_blocks and len(src.blocks) == 3
    assert engine.host_kv.allocator.num_free == 8
    assert engine.swap_in_blocks == 3
    assert engine.kv.allocator.num_shared == 2
    for kv in [src] + kids:
        assert kv.num_tokens == 37
        k1, v1 = gathered(engine, kv)
        assert torch.equal(k0, k1) and torch.equal(v0, v1)
    control = make_engine()
    ckv = new_kv()
    run(control, ckv, toks(37, 1), 0)
    assert run(engine, kids[1], toks(4, 5), 5) == \
        run(control, ckv, toks(4, 5), 5)
    for kv in [src] + kids:
        engine.free_sequence(kv)
    assert_clean(engine)


def test_fork_of_a_swapped_source_without_room_changes_nothing():
    engine = make_engine(num_kv_blocks=6, kv_host_blocks=8)
    src = new_kv()
    run(engine, src, toks(37, 1), 0)
    assert engine._swap_out(src)
    hog = new_kv()
    run(engine, hog, toks(40, 2), 0)          # 3 of 6 blocks
    parent = new_kv()
    run(engine, parent, toks(16, 3), 0)
    (kid,) = engine.fork_sequence(parent)     # one shared block
    alloc, halloc = engine.kv.allocator, engine.host_kv.allocator
    state = (alloc.num_free, alloc.num_shared, halloc.num_free,
             list(src.host_blocks), list(src.blocks), src.num_tokens)
    assert state[:3] == (2, 1, 5)
    with pytest.raises(MemoryError):
        engine.fork_sequence(src, 2)          # wants 3 back + 2 tails
    assert state == (alloc.num_free, alloc.num_shared, halloc.num_free,
                     src.host_blocks, src.blocks, src.num_tokens)
    assert engine.swap_in_blocks == 0
    for kv in (src, hog, parent, kid):
        engine.free_sequence(kv)
    assert_clean(engine)


# ---- conservation ------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_traffic_conserves_blocks(seed):
    rng = random.Random(seed)
    # two requests in flight at most, of at most 5 blocks each: whatever
    # else holds blocks is idle and can be evicted, so admission never
    # starves for good
    engine = make_engine(num_kv_blocks=10, max_sessions=3, max_model_len=80,
                         kv_host_blocks=6, kv_swap_staging_blocks=2)
    sp = SamplingParams(temperature=0.0, max_new_tokens=3)
    live = []

    def idle(kv):
        return not any(r.kv is kv for r in engine.waiting) and \
            not any(r is not None and r.kv is kv for r in engine._rows)

    for _ in range(80):
        op = rng.random()
        if op < 0.45 or not live:
            kv = rng.choice(live) if live and rng.random() < 0.6 else None
            if kv is None:
                kv = new_kv()
                live.append(kv)
            ctx = kv.num_tokens or len(kv.history)
            busy = len(engine.waiting) + engine.num_running
            if idle(kv) and ctx + 30 <= 80 and busy < 2:
                engine.add_request(kv, toks(rng.randrange(12, 24),
                                            rng.randrange(99)), sp)
        elif op < 0.80:
            for _ in range(rng.randrange(1, 4)):
                if engine.has_work():
                    engine.step()
        elif op < 0.92:
            src = rng.choice(live)
            if idle(src):
                try:
                    live.extend(engine.fork_sequence(src, rng.randrange(1, 3)))
                except MemoryError:
                    pass
        else:
            kv = rng.choice(live)
            if idle(kv):
                live.remove(kv)
                engine.free_sequence(kv)
        a, h = engine.kv.allocator, engine.host_kv.allocator
        assert h.num_blocks - h.num_free == \
            sum(len(kv.host_blocks) for kv in live)
        assert engine.swapped_sessions == \
            sum(bool(kv.host_blocks) for kv in live)
        assert a.num_free <= a.num_blocks
    while engine.has_work():
        engine.step()
    assert engine.swap_out_blocks > 0, "the pool never came under pressure"
    for kv in live:
        engine.free_sequence(kv)
    assert_clean(engine)


# ---- server ------------------------------------------------------------
def test_server_flags_stats_and_release():
    args = build_parser().parse_args(["--kv-host-gib", "0.5",
                                      "--kv-swap-staging-blocks", "3"])
    assert args.kv_host_gib == 0.5 and args.kv_swap_staging_blocks == 3
    assert build_parser().parse_args([]).kv_host_gib == 0
    cfg = tiny_llama()
    # a tiny-llama record: K and V, 2 layers, 2 heads, 16 x 128 bf16
    record = 2 * 2 * 2 * 16 * 128 * 2
    assert kv_host_blocks_for(0.5, cfg, EngineConfig()) == (1 << 29) // record
    assert kv_host_blocks_for(0.5, cfg, EngineConfig(kv_dtype="fp8")) == \
        (1 << 30) // record

    sock = f"/tmp/mhs-{uuid.uuid4().hex[:10]}.sock"
    torch.manual_seed(0)
    ecfg = EngineConfig(max_model_len=256, max_sessions=2, num_kv_blocks=8,
                        use_graphs=False, kv_host_blocks=16)
    h = ModelhubServer(LlamaModel(cfg, device="cpu"), cfg, ecfg, sock,
                       device="cpu")
    h.start()
    try:
        c = ModelhubClient(sock, timeout=120)
        st = c.call("stats")
        assert st["kv_host_blocks_total"] == st["kv_host_blocks_free"] == 16
        assert (st["swap_out_blocks"], st["swap_in_blocks"],
                st["swapped_sessions"], st["swap_fallbacks"]) == (0, 0, 0, 0)
        for s in ("a", "b", "c"):
            c.generate(s, PROMPT, max_new_tokens=6, temperature=0.0)
        st = c.call("stats")
        assert st["swapped_sessions"] >= 1 and st["swap_out_blocks"] >= 3
        assert st["kv_host_blocks_free"] == 16 - st["swap_out_blocks"]
        swapped = [s for s, kv in h.sessions.items() if kv.host_blocks]
        assert st["swapped_sessions"] == len(swapped)
        # stats runs on a connection thread beside the engine thread: what
        # it reads must be a stored number, not a walk over the sessions
        assert type(vars(h.engine)["swapped_sessions"]) is int
        c.call("release", session=swapped[0])
        st2 = c.call("stats")
        assert st2["swapped_sessions"] == st["swapped_sessions"] - 1
        assert st2["kv_host_blocks_free"] > st["kv_host_blocks_free"]
        for s in list(h.sessions):
            c.call("release", session=s)
        st = c.call("stats")
        assert st["kv_host_blocks_free"] == 16 and st["swapped_sessions"] == 0
        assert st["kv_blocks_free"] == st["kv_blocks_total"]
        c.close()
    finally:
        h.stop()
