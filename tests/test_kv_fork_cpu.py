"""Session fork on CPU (tiny model, reference ops): refcounted KV blocks,
fork accounting, forked sessions against unforked controls that make the
same model passes, prefill-only requests, eviction under sharing, and the
server's fork verb."""
import queue
import random
import uuid

import pytest
import torch

from kukeon_amd import ops
from kukeon_amd.engine.config import (EngineConfig, SamplingParams,
                                      tiny_llama)
from kukeon_amd.engine.engine import LLMEngine
from kukeon_amd.engine.kv_cache import BlockAllocator, SequenceKV
from kukeon_amd.models.llama import LlamaModel
from kukeon_amd.serve.server import ModelhubClient, ModelhubServer

BS = 16


def make_engine(num_kv_blocks=256, **kw):
    torch.manual_seed(0)
    cfg = tiny_llama()
    ecfg = EngineConfig(max_model_len=512, max_sessions=8,
                        num_kv_blocks=num_kv_blocks, use_graphs=False, **kw)
    model = LlamaModel(cfg, device="cpu")
    return LLMEngine(model, cfg, ecfg, device="cpu")


def toks(n, salt):
    return [(salt * 131 + i * 29 + 7) % 512 for i in range(n)]


def run_many(engine, work, n_new, stop=()):
    """Submit [(kv, prompt)] together, in order; -> tokens per entry."""
    sp = SamplingParams(temperature=0.0, max_new_tokens=n_new,
                        stop_token_ids=tuple(stop))
    rids = [engine.add_request(kv, p, sp) for kv, p in work]
    reqs = list(engine.waiting[-len(rids):])
    got = {rid: [] for rid in rids}
    while engine.has_work():
        for o in engine.step():
            got[o.req_id].extend(o.new_tokens)
    assert all(r.preempted == 0 for r in reqs)
    return [got[rid] for rid in rids]


def run(engine, kv, prompt, n_new, stop=()):
    return run_many(engine, [(kv, prompt)], n_new, stop)[0]


def new_kv():
    return SequenceKV(BS)


def gathered(engine, kv, t):
    """K and V of positions [0, t) as the block table addresses them."""
    idx = torch.tensor([kv.blocks[p // BS] for p in range(t)],
                       dtype=torch.long)
    off = torch.tensor([p % BS for p in range(t)], dtype=torch.long)
    return (engine.kv.k[:, idx, :, off].clone(),
            engine.kv.v[:, idx, :, off].clone())


def assert_no_leak(engine):
    a = engine.kv.allocator
    assert a.num_free == a.num_blocks
    assert a.num_shared == 0


# ---- allocator ---------------------------------------------------------
def test_allocator_share_free_counting():
    a = BlockAllocator(8)
    b = a.alloc(3)
    assert a.num_free == 5 and a.num_shared == 0
    a.share(b[:2])
    a.share(b[:1])
    assert a.num_shared == 2 and a.num_free == 5
    a.free(b)                      # first holder gone: 1 block comes back
    assert a.num_free == 6 and a.num_shared == 1
    a.free(b[:2])
    assert a.num_free == 7 and a.num_shared == 0
    a.free(b[:1])
    assert a.num_free == 8 and a.num_shared == 0


def test_allocator_never_reissues_a_referenced_block():
    a = BlockAllocator(6)
    b = a.alloc(2)
    a.share(b)
    a.free(b)
    rest = a.alloc(a.num_free)
    assert not set(rest) & set(b)
    with pytest.raises(MemoryError):
        a.alloc(1)
    a.free(b)
    assert sorted(a.alloc(2)) == sorted(b)


def test_allocator_double_free_raises():
    a = BlockAllocator(4)
    b = a.alloc(2)
    a.free(b)
    with pytest.raises((AssertionError, ValueError)):
        a.free(b[:1])
    assert a.num_free == 4
    with pytest.raises((AssertionError, ValueError)):
        a.share(b[:1])             # a free block has no holder to share with


def test_allocator_without_share_is_the_plain_free_list():
    class Plain:
        def __init__(self, n):
            self.f = list(range(n - 1, -1, -1))

        def alloc(self, n):
            out = self.f[-n:][::-1]
            del self.f[-n:]
            return out

        def free(self, blocks):
            self.f.extend(reversed(blocks))

    rng = random.Random(11)
    a, m = BlockAllocator(40), Plain(40)
    held = []
    for _ in range(400):
        if held and (rng.random() < 0.45 or a.num_free < 6):
            b = held.pop(rng.randrange(len(held)))
            a.free(b)
            m.free(b)
        else:
            n = rng.randint(1, 6)
            got, want = a.alloc(n), m.alloc(n)
            assert got == want
            held.append(got)
        assert a.num_free == len(m.f) and a._free == m.f
        assert a.num_shared == 0


# ---- fork accounting ---------------------------------------------------
def _parent_with(engine, t):
    """A parent whose context holds exactly t tokens, nothing pending."""
    kv = new_kv()
    if t == 0:
        # evicted: history without resident KV
        run(engine, kv, toks(9, 3), 0)
        assert engine._evict_idle_kv()
        assert kv.num_tokens == 0 and len(kv.history) == 9 and not kv.blocks
    else:
        run(engine, kv, toks(t, 3), 0)
        assert kv.num_tokens == t
    return kv


@pytest.mark.parametrize("t", [0, 5, 16, 21, 47])
def test_fork_accounting(t):
    engine = make_engine(num_kv_blocks=32)
    a = engine.kv.allocator
    parent = _parent_with(engine, t)
    before = list(parent.blocks)
    free0 = a.num_free
    kids = engine.fork_sequence(parent, 2)
    full, tail = divmod(t, BS)
    assert parent.blocks == before
    assert a.num_free == free0 - (2 if tail else 0)
    assert a.num_shared == full
    for c in kids:
        assert len(c.blocks) == full + (1 if tail else 0)
        assert c.blocks[:full] == parent.blocks[:full]
        assert c.num_tokens == t and c.pending_token is None
        assert c.history == parent.history and c.history is not parent.history
        assert id(c) in engine._known_kvs
        if tail:
            assert c.blocks[full] not in parent.blocks
        pk, pv = gathered(engine, parent, t)
        ck, cv = gathered(engine, c, t)
        assert torch.equal(pk.view(torch.int16), ck.view(torch.int16))
        assert torch.equal(pv.view(torch.int16), cv.view(torch.int16))
    if tail:
        assert kids[0].blocks[full] != kids[1].blocks[full]
    if t == 0:
        # like the parent, a child rebuilds the context at its next request
        assert len(run(engine, kids[0], [5], 2)) == 2
        assert kids[0].num_tokens == 9 + 1 + 2 - 1
    for kv in [parent] + kids:
        engine.free_sequence(kv)
    assert_no_leak(engine)


def test_fork_leaves_surplus_blocks_and_copies_pending_token():
    engine = make_engine(num_kv_blocks=32)
    a = engine.kv.allocator
    probe = new_kv()
    greedy = run(engine, probe, toks(14, 5), 12)
    engine.free_sequence(probe)
    j = next(i for i in range(1, 12) if greedy[i] not in greedy[:i])
    parent = new_kv()
    out = run(engine, parent, toks(14, 5), 40, stop=(greedy[j],))
    assert out == greedy[:j + 1]
    t = parent.num_tokens
    assert t == 14 + j
    need = -(-t // BS)
    assert len(parent.blocks) > need, "stop mid-microbatch leaves surplus"
    free0 = a.num_free
    (child,) = engine.fork_sequence(parent)
    full, tail = divmod(t, BS)
    assert len(child.blocks) == need
    assert child.blocks[:full] == parent.blocks[:full]
    assert a.num_free == free0 - (1 if tail else 0)
    assert child.pending_token == parent.pending_token == greedy[j]
    pk, pv = gathered(engine, parent, t)
    ck, cv = gathered(engine, child, t)
    assert torch.equal(pk.view(torch.int16), ck.view(torch.int16))
    assert torch.equal(pv.view(torch.int16), cv.view(torch.int16))
    engine.free_sequence(parent)
    engine.free_sequence(child)
    assert_no_leak(engine)


def test_fork_refuses_an_active_source_and_a_short_pool():
    engine = make_engine(num_kv_blocks=4)
    a = engine.kv.allocator
    parent = new_kv()
    run(engine, parent, toks(37, 1), 0)          # 2 full blocks + tail
    refs = list(a._refs)
    with pytest.raises(MemoryError):
        engine.fork_sequence(parent, 2)          # one block left, two tails
    assert a._refs == refs and a.num_free == 1 and a.num_shared == 0
    engine.add_request(parent, [1, 2],
                       SamplingParams(temperature=0.0, max_new_tokens=3))
    with pytest.raises(ValueError):
        engine.fork_sequence(parent)             # waiting
    engine.step()
    assert engine.num_running == 1
    with pytest.raises(ValueError):
        engine.fork_sequence(parent)             # holds a row
    while engine.has_work():
        engine.step()
    (child,) = engine.fork_sequence(parent)
    engine.free_sequence(parent)
    engine.free_sequence(child)
    assert_no_leak(engine)


def test_fork_of_three_is_one_copy_launch(monkeypatch):
    engine = make_engine(num_kv_blocks=32)
    parent = _parent_with(engine, 21)
    calls = []
    real = ops.kv_copy_blocks

    def counting(k, v, src, dst):
        calls.append((src.tolist(), dst.tolist()))
        real(k, v, src, dst)

    monkeypatch.setattr(ops, "kv_copy_blocks", counting)
    kids = engine.fork_sequence(parent, 3)
    assert len(calls) == 1
    src, dst = calls[0]
    assert src == [parent.blocks[1]] * 3
    assert dst == [c.blocks[1] for c in kids] and len(set(dst)) == 3
    engine.fork_sequence(_parent_with(engine, 32), 3)   # no tail, no launch
    assert len(calls) == 1


# ---- tokens against controls that make the same passes -----------------
P = toks(21, 1)
S = [toks(7, 10 + i) for i in range(4)]
N_NEW = 9   # 21 + 7 + 9 crosses the block boundary at 32 while decoding


def _control(engine, suffix):
    kv = new_kv()
    run(engine, kv, P, 0)
    out = run(engine, kv, suffix, N_NEW)
    engine.free_sequence(kv)
    return out


def test_child_and_parent_tokens_equal_their_controls():
    engine = make_engine()
    want_child = _control(engine, S[0])
    want_parent = _control(engine, S[1])
    parent = new_kv()
    assert run(engine, parent, P, 0) == []
    (child,) = engine.fork_sequence(parent)
    assert run(engine, child, S[0], N_NEW) == want_child
    assert child.blocks[0] == parent.blocks[0]
    assert child.blocks[1] != parent.blocks[1]
    # the parent's own tail was not disturbed by the child's appends
    assert run(engine, parent, S[1], N_NEW) == want_parent
    engine.free_sequence(parent)
    engine.free_sequence(child)
    assert_no_leak(engine)


def test_parent_and_three_children_together_equal_independent_sessions():
    engine = make_engine()
    indep = [new_kv() for _ in range(4)]
    for kv in indep:
        run(engine, kv, P, 0)
    want = run_many(engine, list(zip(indep, S)), N_NEW)
    for kv in indep:
        engine.free_sequence(kv)
    parent = new_kv()
    run(engine, parent, P, 0)
    kids = engine.fork_sequence(parent, 3)
    got = run_many(engine, list(zip([parent] + kids, S)), N_NEW)
    assert got == want
    assert len({tuple(g) for g in got}) > 1, "suffixes should matter"
    assert engine.kv.allocator.num_shared == 1
    for kv in [parent] + kids:
        engine.free_sequence(kv)
    assert_no_leak(engine)


def test_child_survives_release_of_its_parent():
    engine = make_engine(num_kv_blocks=16)
    want = _control(engine, S[2])
    parent = new_kv()
    run(engine, parent, P, 0)
    (child,) = engine.fork_sequence(parent)
    shared = parent.blocks[0]
    engine.free_sequence(parent)
    a = engine.kv.allocator
    assert a.num_shared == 0 and shared not in a._free
    # take every free block, so a wrongly released one would be overwritten
    hog = new_kv()
    run(engine, hog, toks(a.num_free * BS - 40, 9), 0)
    engine.free_sequence(hog)
    assert run(engine, child, S[2], N_NEW) == want
    engine.free_sequence(child)
    assert_no_leak(engine)


def test_survivor_of_an_eviction_under_pressure_matches_its_control():
    engine = make_engine(num_kv_blocks=8)
    a = engine.kv.allocator
    p37 = toks(37, 2)
    ctl = new_kv()
    run(engine, ctl, p37, 0)
    want37 = run(engine, ctl, S[3], N_NEW)
    engine.free_sequence(ctl)
    parent = new_kv()
    run(engine, parent, p37, 0)                  # 3 blocks, 2 of them full
    (child,) = engine.fork_sequence(parent)
    assert a.num_free == 4 and a.num_shared == 2
    # 5 blocks wanted, 4 free: one holder goes, its shared blocks stay put
    big = new_kv()
    assert len(run(engine, big, toks(60, 4), 8)) == 8
    gone = [kv for kv in (parent, child) if not kv.blocks]
    assert len(gone) == 1 and a.num_shared == 0
    survivor = child if gone[0] is parent else parent
    assert not set(survivor.blocks) & set(big.blocks)
    assert not set(survivor.blocks) & set(a._free)
    assert run(engine, survivor, S[3], N_NEW) == want37
    for kv in (parent, child, big):
        engine.free_sequence(kv)
    assert_no_leak(engine)


def test_eviction_ranks_by_blocks_returned_to_the_pool():
    engine = make_engine(num_kv_blocks=16)
    parent = new_kv()
    run(engine, parent, toks(64, 1), 0)          # 4 blocks, all full
    (child,) = engine.fork_sequence(parent)      # holds the same 4
    small = new_kv()
    run(engine, small, toks(20, 2), 0)           # 2 blocks of its own
    assert engine._evict_idle_kv()
    assert not small.blocks and parent.blocks and child.blocks
    # holders that return nothing are still candidates: the first eviction
    # drops references, the second frees the blocks
    free0 = engine.kv.allocator.num_free
    assert engine._evict_idle_kv()
    assert engine.kv.allocator.num_free == free0
    assert engine._evict_idle_kv()
    assert engine.kv.allocator.num_free == free0 + 4
    assert not engine._evict_idle_kv()
    assert_no_leak(engine)


def test_capacity_three_children_fit_where_independent_sessions_do_not():
    def work(engine, kvs):
        return run_many(engine, [(kv, toks(5, 20 + i))
                                 for i, kv in enumerate(kvs)], 4)

    engine = make_engine(num_kv_blocks=12)
    parent = new_kv()
    run(engine, parent, toks(64, 1), 0)
    kids = engine.fork_sequence(parent, 3)
    outs = work(engine, kids)                    # asserts preempted == 0
    assert all(len(o) == 4 for o in outs)
    # nothing was evicted: 4 shared blocks + one block per child
    assert all(kv.blocks and kv.num_tokens for kv in [parent] + kids)
    assert engine.kv.allocator.num_free == 12 - 4 - 3
    # the same work as independent sessions: 4 + 3 * 5 blocks, over the pool
    engine2 = make_engine(num_kv_blocks=12)
    template = new_kv()
    run(engine2, template, toks(64, 1), 0)
    solo = [new_kv() for _ in range(3)]
    for kv in solo:
        run(engine2, kv, toks(64, 1), 0)
    assert not all(kv.blocks for kv in [template] + solo), \
        "four resident 64-token contexts cannot fit 12 blocks"


# ---- prefill-only requests ---------------------------------------------
def test_prefill_only_request():
    engine = make_engine()
    kv = new_kv()
    rid = engine.add_request(kv, toks(10, 1),
                             SamplingParams(temperature=0.0,
                                            max_new_tokens=0))
    outs = []
    while engine.has_work():
        outs.extend(engine.step())
        assert engine.num_running == 0
    assert [(o.req_id, o.new_tokens, o.finished) for o in outs] == \
        [(rid, [], True)]
    assert kv.pending_token is None and kv.num_tokens == 10
    assert kv.history == toks(10, 1)
    assert len(engine._free_rows) == engine.Bmax
    # a carried pending token is prefilled with the next prefill-only prompt
    t1 = run(engine, kv, toks(4, 2), 3)
    assert kv.pending_token == t1[-1]
    assert run(engine, kv, toks(2, 3), 0) == []
    assert kv.pending_token is None
    assert kv.num_tokens == 10 + 4 + 3 + 2
    assert kv.history[-3:] == [t1[-1]] + toks(2, 3)


def test_prefill_only_then_turn_matches_two_request_control():
    engine = make_engine()
    a, b = new_kv(), new_kv()
    run(engine, a, toks(10, 1), 0)
    first_a = run(engine, a, toks(6, 2), 5)
    # control: the same two prompts as two requests, the first one sampling
    # a token that is dropped again before the second
    run(engine, b, toks(10, 1), 1)
    b.pending_token = None
    first_b = run(engine, b, toks(6, 2), 5)
    assert first_a[0] == first_b[0] and first_a == first_b


def test_empty_prefill_only_request_raises():
    engine = make_engine()
    kv = new_kv()
    sp0 = SamplingParams(temperature=0.0, max_new_tokens=0)
    with pytest.raises(ValueError):
        engine.add_request(kv, [], sp0)
    assert not engine.waiting
    run(engine, kv, toks(5, 1), 0)
    with pytest.raises(ValueError):
        engine.add_request(kv, [], sp0)
    assert not engine.waiting and kv.num_tokens == 5


# ---- server ------------------------------------------------------------
@pytest.fixture
def hub():
    sock = f"/tmp/mhf-{uuid.uuid4().hex[:10]}.sock"
    torch.manual_seed(0)
    cfg = tiny_llama()
    ecfg = EngineConfig(max_model_len=256, max_sessions=8, num_kv_blocks=64,
                        use_graphs=False)
    h = ModelhubServer(LlamaModel(cfg, device="cpu"), cfg, ecfg, sock,
                       device="cpu")
    h.start()
    yield h, sock
    h.stop()


def test_server_fork_verb_stats_and_prefill_only(hub):
    h, sock = hub
    c = ModelhubClient(sock, timeout=120)
    r = c.generate("ctl", P, max_new_tokens=0)
    assert r == {"tokens": [], "context_len": 21}
    want = c.generate("ctl", S[0], max_new_tokens=N_NEW, temperature=0.0)
    c.call("release", session="ctl")
    assert c.generate("tmpl", P, max_new_tokens=0)["tokens"] == []
    assert c.call("stats")["kv_blocks_shared"] == 0
    free0 = c.call("stats")["kv_blocks_free"]
    r = c.fork("tmpl", ["a", "b"])
    assert r == {"context_len": 21, "shared_blocks": 1, "copied_blocks": 2}
    st = c.call("stats")
    assert st["kv_blocks_shared"] == 1 and st["sessions"] == 3
    assert st["kv_blocks_free"] == free0 - 2
    got = c.generate("a", S[0], max_new_tokens=N_NEW, temperature=0.0)
    assert got["tokens"] == want["tokens"]
    assert got["context_len"] == want["context_len"]
    for s in ("tmpl", "a", "b"):
        c.call("release", session=s)
    st = c.call("stats")
    assert st["kv_blocks_shared"] == 0
    assert st["kv_blocks_free"] == st["kv_blocks_total"]
    c.close()


def test_server_fork_errors_create_nothing(hub):
    h, sock = hub
    c = ModelhubClient(sock, timeout=120)
    c.generate("tmpl", P, max_new_tokens=0)
    c.generate("other", [1, 2, 3], max_new_tokens=0)
    free0 = c.call("stats")["kv_blocks_free"]
    with pytest.raises(RuntimeError, match="unknown session"):
        c.fork("nope", ["x"])
    with pytest.raises(RuntimeError, match="already present"):
        c.fork("tmpl", ["x", "other"])
    # a source with a request in flight: the engine thread takes the
    # request first (the submit queue is FIFO) and needs many steps for it
    kv = h.sessions["tmpl"]
    done = queue.Queue()
    h._submit.put(lambda: done.put(h.engine.add_request(
        kv, [4, 5], SamplingParams(temperature=0.0, max_new_tokens=200))))
    with pytest.raises(RuntimeError, match="active request"):
        c.fork("tmpl", ["y"])
    rid = done.get(timeout=60)
    h._submit.put(lambda: done.put(h.engine.cancel(rid)))
    assert done.get(timeout=60) is True
    st = c.call("stats")
    assert set(h.sessions) == {"tmpl", "other"}
    assert st["sessions"] == 2 and st["kv_blocks_shared"] == 0
    # the in-flight turn grew tmpl's context; nothing else took blocks
    held = sum(len(s.blocks) for s in h.sessions.values())
    assert st["kv_blocks_free"] == st["kv_blocks_total"] - held <= free0
    c.close()
