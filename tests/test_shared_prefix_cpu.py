"""Shared-prefix decode attention on CPU: the reference op's strict check of
the tile metadata, and the engine's grouping of forked sessions into tiles
(tiny model, reference ops, which validate every call the engine makes)."""
import pytest
import torch

from kukeon_amd import ops
from kukeon_amd.engine.config import (EngineConfig, SamplingParams,
                                      tiny_llama)
from kukeon_amd.engine.engine import LLMEngine
from kukeon_amd.engine.kv_cache import SequenceKV
from kukeon_amd.models.llama import LlamaModel
from kukeon_amd.ops import reference

BS, D, HK = 16, 128, 2


# ---- reference op ------------------------------------------------------
def _op_case(G=2):
    """Rows 0 and 2 share two prefix blocks, row 1 is on its own, row 3 is
    dead. -> (args of paged_attention_rope, prefix_blocks, tiles)."""
    Hq = G * HK
    gen = torch.Generator().manual_seed(3)
    ctxs, poss = [40, 20, 53, 0], [39, 19, 52, -1]
    bt = torch.tensor([[5, 9, 1, 0], [7, 3, 0, 0], [5, 9, 2, 4],
                       [0, 0, 0, 0]], dtype=torch.int32)
    kc = torch.randn(12, HK, BS, D, generator=gen).bfloat16()
    vc = torch.randn(12, HK, BS, D, generator=gen).bfloat16()
    qkv = torch.randn(4, (Hq + 2 * HK) * D, generator=gen).bfloat16()
    inv = 1.0 / (500000.0 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.outer(torch.arange(64).float(), inv)
    cos_sin = torch.cat([fr.cos(), fr.sin()], dim=1)
    prefix_blocks = torch.tensor([2, 0, 2, 0], dtype=torch.int32)
    tiles = torch.zeros(2, 2 + 16, dtype=torch.int32)
    tiles[1, :4] = torch.tensor([2, 2, 0, 2])       # tile 0 stays empty
    args = dict(qkv=qkv, kc=kc, vc=vc, cos_sin=cos_sin,
                pos=torch.tensor(poss, dtype=torch.int32), bt=bt,
                seq_lens=torch.tensor(ctxs, dtype=torch.int32), Hq=Hq)
    return args, prefix_blocks, tiles


def _shared(a, prefix_blocks, tiles, out=None, caches=None):
    out = torch.zeros(4, a["Hq"] * D, dtype=torch.bfloat16) \
        if out is None else out
    kc, vc = caches or (a["kc"].clone(), a["vc"].clone())
    ops.paged_attention_rope_shared(
        out, a["qkv"], kc, vc, a["cos_sin"], a["pos"], a["bt"],
        a["seq_lens"], a["Hq"], HK, 4, D ** -0.5, None, None, prefix_blocks,
        tiles, 4)
    return out, kc, vc


def test_reference_equals_unshared_exactly():
    a, pb, tiles = _op_case()
    qkv0 = a["qkv"].clone()
    out, kc, vc = _shared(a, pb, tiles)
    want = torch.zeros_like(out)
    kc_u, vc_u = a["kc"].clone(), a["vc"].clone()
    reference.paged_attention_rope(want, a["qkv"], kc_u, vc_u, a["cos_sin"],
                                   a["pos"], a["bt"], a["seq_lens"], a["Hq"],
                                   HK, 4, D ** -0.5)
    assert torch.equal(out, want) and out[:3].any()
    assert torch.equal(kc, kc_u) and torch.equal(vc, vc_u)
    assert not torch.equal(kc, a["kc"])          # something was appended
    assert torch.equal(a["qkv"], qkv0)
    # the variant without RoPE, on the appended caches
    out2 = torch.zeros_like(out)
    want2 = torch.zeros_like(out)
    ops.paged_attention_shared(out2, a["qkv"], kc, vc, a["bt"],
                               a["seq_lens"], 0, 4, D ** -0.5, None, None,
                               pb, tiles, 4)
    reference.paged_attention(want2, a["qkv"], kc, vc, a["bt"],
                              a["seq_lens"], 0, 4, D ** -0.5)
    assert torch.equal(out2, want2)


def _broken(how):
    a, pb, tiles = _op_case()
    if how == "table":            # a member's table leaves the prefix
        a["bt"][2, 1] = 8
    elif how == "prefix_blocks":  # a member's prefix length disagrees
        pb[2] = 1
    elif how == "stray":          # a row outside every tile claims a prefix
        pb[1] = 1
    elif how == "twice":          # a row in two tiles
        tiles[0, :4] = torch.tensor([2, 1, 2, 1])
    elif how == "newest":         # the prefix holds the token being appended
        a["pos"][0] = 31
        a["seq_lens"][0] = 32
    elif how == "dead":           # a member without context
        tiles[1, 3] = 3
    elif how == "wide":           # more rows than 16 // G columns hold
        tiles[1, 0] = 9
    return a, pb, tiles


@pytest.mark.parametrize("how", ["table", "prefix_blocks", "stray", "twice",
                                 "newest", "dead", "wide"])
def test_reference_rejects_bad_metadata(how):
    a, pb, tiles = _broken(how)
    with pytest.raises(ValueError):
        _shared(a, pb, tiles)


def test_check_prefix_tiles():
    tiles = torch.zeros(1, 2 + 16, dtype=torch.int32)
    tiles[0, 0] = 4
    ops.check_prefix_tiles(tiles, 4)                 # 16 // 4 rows fit
    with pytest.raises(ValueError, match="at most"):
        ops.check_prefix_tiles(tiles, 8)
    with pytest.raises(ValueError, match="int32"):
        ops.check_prefix_tiles(tiles.long(), 4)
    with pytest.raises(ValueError, match="int32"):
        ops.check_prefix_tiles(tiles[:, :17], 4)


# ---- engine: grouping --------------------------------------------------
def make_engine(min_tokens, **kw):
    torch.manual_seed(0)
    cfg = tiny_llama()
    ecfg = EngineConfig(max_model_len=512, max_sessions=8, num_kv_blocks=256,
                        use_graphs=False, decode_microbatch=1,
                        shared_prefix_min_tokens=min_tokens, **kw)
    engine = LLMEngine(LlamaModel(cfg, device="cpu"), cfg, ecfg, device="cpu")
    engine.regroups = 0
    inner = engine._regroup

    def counted():
        engine.regroups += 1
        inner()
    engine._regroup = counted
    return engine


def toks(n, salt):
    return [(salt * 131 + i * 29 + 7) % 512 for i in range(n)]


def drain(engine, got):
    while engine.has_work():
        step(engine, got)


def step(engine, got):
    for o in engine.step():
        got.setdefault(o.req_id, []).extend(o.new_tokens)


def forked(engine, n_new):
    """A 40-token template (2 shared blocks and a tail) forked into three
    children, submitted with one unrelated session. -> (kvs, rids)"""
    sp0 = SamplingParams(temperature=0.0, max_new_tokens=0)
    tmpl = SequenceKV(BS)
    engine.add_request(tmpl, toks(40, 1), sp0)
    drain(engine, {})
    kvs = engine.fork_sequence(tmpl, 3) + [SequenceKV(BS)]
    rids = [engine.add_request(
        kv, toks(5 + 2 * i, 10 + i),
        SamplingParams(temperature=0.0, max_new_tokens=n))
        for i, (kv, n) in enumerate(zip(kvs, n_new))]
    return [tmpl] + kvs, rids


def tiles_of(engine):
    return [row[:2 + row[0]] for row in engine.h_tiles.tolist() if row[0]]


def req_of(engine, kv):
    return next(r for r in engine._rows if r is not None and r.kv is kv)


def test_grouping_follows_row_membership():
    engine = make_engine(16)
    assert engine.tile_width == 16
    kvs, rids = forked(engine, [4, 12, 12, 12])
    _tmpl, k0, k1, k2, other = kvs
    got = {}
    step(engine, got)                     # prefill: rows 0..3 in this order
    assert [req_of(engine, kv).row for kv in kvs[1:]] == [0, 1, 2, 3]
    assert engine.shared_prefix_steps == 0 and engine.regroups == 0
    step(engine, got)                     # first decode step
    assert tiles_of(engine) == [[3, 2, 0, 1, 2]]
    assert engine.h_prefix_blocks.tolist()[:4] == [2, 2, 2, 0]
    assert torch.equal(engine.d_tiles, engine.h_tiles)
    assert torch.equal(engine.d_prefix_blocks, engine.h_prefix_blocks)
    assert (engine.shared_prefix_steps, engine.shared_prefix_rows) == (1, 3)
    step(engine, got)                     # same rows: nothing is recomputed
    assert engine.regroups == 1 and engine.shared_prefix_steps == 2

    # a preempted member leaves its group; it comes back with blocks of
    # its own (recompute) and stays outside
    engine._preempt(req_of(engine, k1))
    step(engine, got)                     # its prefill
    step(engine, got)
    r1 = req_of(engine, k1).row
    assert k1.blocks[0] != k0.blocks[0]
    assert tiles_of(engine) == [[2, 2, 0, 2]]
    pb = engine.h_prefix_blocks.tolist()
    assert pb[0] == pb[2] == 2 and pb[r1] == 0 and pb[3] == 0
    assert engine.shared_prefix_rows == 2 and engine.regroups == 2

    # the first child finishes: one member left, the group dissolves
    while len(got[rids[0]]) < 4:
        step(engine, got)
    before = engine.shared_prefix_steps
    step(engine, got)
    assert tiles_of(engine) == [] and not engine.h_prefix_blocks.any()
    assert engine.shared_prefix_rows == 0
    assert engine.shared_prefix_steps == before
    n = engine.regroups
    step(engine, got)
    assert engine.regroups == n
    drain(engine, got)
    assert [len(got[r]) for r in rids] == [4, 12, 12, 12]


def test_threshold_above_the_prefix_keeps_the_path_off():
    engine = make_engine(48)              # the prefix is 32 tokens
    _kvs, rids = forked(engine, [6, 6, 6, 6])
    got = {}
    drain(engine, got)
    assert engine.shared_prefix_steps == 0 and engine.shared_prefix_rows == 0
    assert tiles_of(engine) == []
    assert [len(got[r]) for r in rids] == [6, 6, 6, 6]


def test_tokens_equal_with_the_path_on_and_off():
    runs = []
    for min_tokens in (16, 0):
        engine = make_engine(min_tokens)
        kvs, rids = forked(engine, [9, 9, 9, 9])
        got = {}
        drain(engine, got)
        runs.append([got[r] for r in rids])
        assert (engine.shared_prefix_steps > 0) == (min_tokens > 0)
        for kv in kvs:
            engine.free_sequence(kv)
        a = engine.kv.allocator
        assert a.num_free == a.num_blocks and a.num_shared == 0
    assert runs[0] == runs[1]
    assert all(len(t) == 9 for t in runs[0])
