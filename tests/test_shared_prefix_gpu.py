"""Shared-prefix decode attention on the GPU: ops.paged_attention_rope_shared
/ ops.paged_attention_shared (a tile of sibling rows attends to the common
prefix blocks once; the suffix pass and the reduce kernel finish each row)
against the unshared ops and the fp32 reference, and the engine's path for
forked sessions against the same engine with the path off."""
import functools

import pytest
import torch

import kukeon_amd.ops as ops
from kukeon_amd.ops import reference

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

DEV = "cuda:0"
HK, D, BS = 2, 128, 16
OUT_SENTINEL = 7.0      # exact in bf16
TAIL_SENTINEL = -123.0
MAXPOS = 256


def _ints(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[
        t.element_size()])


def _same_bits(a, b, what):
    assert torch.equal(_ints(a), _ints(b)), what


def _cos_sin():
    inv = 1.0 / (500000.0 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.outer(torch.arange(MAXPOS).float(), inv)
    return torch.cat([fr.cos(), fr.sin()], dim=1)


def _layout(G, P):
    """Rows of one call: group A of 2 and group B of W + 1 rows (it spills
    into a second tile), interleaved so that no group's rows are
    contiguous, one ungrouped row between them and one dead row.
    -> (kinds per row, ctx per row, tiles as lists)"""
    W = 16 // G
    kinds = ["A", "B", "U", "B", "A", "dead"] + ["B"] * (W - 1)
    # the new token first in the first suffix block, mid-block, and a
    # suffix of several blocks
    suffixes = [1, 9, 40]
    ctxs, n = [], 0
    for kind in kinds:
        if kind == "dead":
            ctxs.append(0)
        elif kind == "U":
            ctxs.append(37)
        else:
            ctxs.append(P * BS + suffixes[n % 3])
            n += 1
    tiles = []
    for g in "AB":
        rows = [r for r, kind in enumerate(kinds) if kind == g]
        for i in range(0, len(rows), W):
            tiles.append([len(rows[i:i + W]), P] + rows[i:i + W])
        if g == "A":
            tiles.append([0, 0])                     # an empty tile
    return kinds, ctxs, tiles


def _build(G, fp8, P, seed=5):
    """CPU inputs. The caches hold NaN (0x7f for fp8) wherever a row may not
    read: outside every context, and in the slot the new token goes to."""
    Hq = G * HK
    kinds, ctxs, tile_rows = _layout(G, P)
    poss = [c - 1 for c in ctxs]
    B = len(kinds)
    gen = torch.Generator().manual_seed(seed)
    mb = P + 3
    own = [max(0, (c + BS - 1) // BS - (P if k in "AB" else 0))
           for k, c in zip(kinds, ctxs)]
    NB = 2 * P + sum(own) + 4
    perm = torch.randperm(NB, generator=gen).tolist()
    shared = {"A": perm[:P], "B": perm[P:2 * P]}
    nxt = 2 * P
    bt = torch.full((B, mb), perm[-1], dtype=torch.int32)
    valid = torch.zeros(NB, BS, dtype=torch.bool)
    for g in shared.values():
        valid[g] = True
    for b, (k, c, p) in enumerate(zip(kinds, ctxs, poss)):
        ids = list(shared.get(k, [])) + perm[nxt:nxt + own[b]]
        nxt += own[b]
        bt[b, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
        for t in range(len(shared.get(k, [])) * BS, c):
            valid[ids[t // BS], t % BS] = t != p
    valid = valid[:, None, :, None].expand(NB, HK, BS, D)

    def cache():
        x = torch.randn(NB, HK, BS, D, generator=gen).bfloat16()
        if fp8:
            x = x.float().to(torch.float8_e4m3fn).view(torch.uint8)
            return torch.where(valid, x, torch.tensor(0x7f, dtype=torch.uint8))
        return x.masked_fill(~valid, float("nan"))

    kc, vc = cache(), cache()
    qkv = torch.randn(B, (Hq + 2 * HK) * D, generator=gen).bfloat16()
    prefix_blocks = torch.tensor([P if k in "AB" else 0 for k in kinds],
                                 dtype=torch.int32)
    tiles = torch.zeros(len(tile_rows), 2 + 16, dtype=torch.int32)
    for t, row in enumerate(tile_rows):
        tiles[t, :len(row)] = torch.tensor(row, dtype=torch.int32)
    return dict(qkv=qkv, kc=kc, vc=vc, cos_sin=_cos_sin(),
                pos=torch.tensor(poss, dtype=torch.int32), bt=bt,
                seq_lens=torch.tensor(ctxs, dtype=torch.int32),
                prefix_blocks=prefix_blocks, tiles=tiles)


@functools.lru_cache(maxsize=None)
def _case(G, fp8, P):
    """Device inputs and the fp32 reference, built once per (G, fp8, P) and
    shared read-only by every split count. The reference op also checks
    that the metadata above keeps the op's contract."""
    cpu = _build(G, fp8, P)
    Hq = G * HK
    ref = torch.zeros(cpu["qkv"].shape[0], Hq * D, dtype=torch.bfloat16)
    reference.paged_attention_rope_shared(
        ref, cpu["qkv"], cpu["kc"].clone(), cpu["vc"].clone(),
        cpu["cos_sin"], cpu["pos"], cpu["bt"], cpu["seq_lens"], Hq, HK, 1,
        D ** -0.5, None, None, cpu["prefix_blocks"], cpu["tiles"], 1)
    case = {k: v.to(DEV) for k, v in cpu.items()}
    case["ref"] = ref.float()
    case["live"] = [b for b, c in enumerate(cpu["seq_lens"].tolist()) if c > 0]
    case["dead"] = [b for b, c in enumerate(cpu["seq_lens"].tolist())
                    if c <= 0]
    return case


def _workspaces(nrows, Hq, slots, guard=1024):
    """NaN where the kernels may write, a sentinel behind."""
    bufs = []
    for n in (nrows * Hq * slots * D, nrows * Hq * slots * 2):
        buf = torch.full((n + guard,), float("nan"), dtype=torch.float32,
                         device=DEV)
        buf[n:] = TAIL_SENTINEL
        bufs.append((buf[:n], buf[n:]))
    return bufs


def _run(c, G, S, PS=None, caches=None, rope=True):
    """One decode-attention step on private copies of qkv and the caches;
    PS None runs the unshared op. -> (out, qkv, kc, vc, workspaces)"""
    nrows, Hq = c["qkv"].shape[0], G * HK
    qkv = c["qkv"].clone()
    kc, vc = caches if caches is not None else (c["kc"].clone(),
                                                c["vc"].clone())
    out = torch.full((nrows, Hq * D), OUT_SENTINEL, dtype=torch.bfloat16,
                     device=DEV)
    ws = _workspaces(nrows, Hq, S + (PS or 0))
    scale = D ** -0.5
    if not rope:
        slots = torch.zeros(nrows, dtype=torch.int32, device=DEV)
        ops.rope_kv_append(qkv, kc, vc, c["cos_sin"], c["pos"], slots, Hq, HK,
                           D, block_table=c["bt"])
    if PS is None and rope:
        ops.paged_attention_rope(out, qkv, kc, vc, c["cos_sin"], c["pos"],
                                 c["bt"], c["seq_lens"], Hq, HK, S, scale,
                                 ws[0][0], ws[1][0])
    elif PS is None:
        ops.paged_attention(out, qkv, kc, vc, c["bt"], c["seq_lens"], 0, S,
                            scale, ws[0][0], ws[1][0])
    elif rope:
        ops.paged_attention_rope_shared(
            out, qkv, kc, vc, c["cos_sin"], c["pos"], c["bt"], c["seq_lens"],
            Hq, HK, S, scale, ws[0][0], ws[1][0], c["prefix_blocks"],
            c["tiles"], PS)
    else:
        ops.paged_attention_shared(
            out, qkv, kc, vc, c["bt"], c["seq_lens"], 0, S, scale, ws[0][0],
            ws[1][0], c["prefix_blocks"], c["tiles"], PS)
    return out, qkv, kc, vc, ws


def _check(c, fp8, shared, unshared, qkv_in):
    out_s, qkv_s, kc_s, vc_s, ws = shared
    _, _, kc_u, vc_u, _ = unshared
    _same_bits(kc_s, kc_u, "k_cache")
    _same_bits(vc_s, vc_u, "v_cache")
    _same_bits(qkv_s, qkv_in, "qkv must be left untouched")
    tol = 7e-2 if fp8 else 2e-2
    got = out_s.cpu().float()
    assert not torch.isnan(got[c["live"]]).any()
    torch.testing.assert_close(got[c["live"]], c["ref"][c["live"]], rtol=tol,
                               atol=tol)
    assert (got[c["dead"]] == OUT_SENTINEL).all()
    for _body, tail in ws:
        _same_bits(tail, torch.full_like(tail, TAIL_SENTINEL),
                   "workspace guard tail")


CONFIGS = [(G, False) for G in (1, 4, 8, 16)] + [(4, True), (16, True)]


@pytest.mark.parametrize("S", [1, 4, 8, 32])
@pytest.mark.parametrize("PS", [1, 4, 8])
@pytest.mark.parametrize("P", [1, 3, 7])
@pytest.mark.parametrize("G,fp8", CONFIGS)
def test_rope_shared_matches_unshared_and_reference(G, fp8, P, PS, S):
    """Whole caches bit-equal to paged_attention_rope's, out within the
    project's tolerance of the fp32 reference, and the op's contract. P
    against PS covers empty prefix ranges (1 and 3 blocks in 4 or 8 splits)
    and uneven ones (7 in 4)."""
    c = _case(G, fp8, P)
    unshared = _run(c, G, S)
    shared = _run(c, G, S, PS)
    _check(c, fp8, shared, unshared, c["qkv"])
    # the append is idempotent: a second call on the appended caches
    out_2, _, kc_2, vc_2, _ = _run(c, G, S, PS, caches=(shared[2], shared[3]))
    _same_bits(out_2, shared[0], "second call")
    _same_bits(kc_2, unshared[2], "k_cache after second call")
    _same_bits(vc_2, unshared[3], "v_cache after second call")


@pytest.mark.parametrize("fp8", [False, True])
def test_shared_without_rope(fp8):
    """ops.paged_attention_shared after rope_kv_append: the fp8 cache's
    decode path. The reference is the same (the fused op equals the
    sequence bit for bit)."""
    G, P = 4, 3
    c = _case(G, fp8, P)
    for PS, S in ((4, 8), (8, 32)):
        unshared = _run(c, G, S, rope=False)
        shared = _run(c, G, S, PS, rope=False)
        _check(c, fp8, shared, unshared, unshared[1])


def test_host_side_checks():
    G, P, S, PS = 4, 3, 4, 4
    c = _case(G, False, P)
    nrows, Hq = c["qkv"].shape[0], G * HK

    def call(tmp_slots=S + PS, **over):
        a = dict(c, **over)
        out = torch.zeros(nrows, Hq * D, dtype=torch.bfloat16, device=DEV)
        tmp_out = torch.zeros(nrows * Hq * tmp_slots * D, device=DEV)
        tmp_ml = torch.zeros(nrows * Hq * (S + PS) * 2, device=DEV)
        ops.paged_attention_rope_shared(
            out, a["qkv"].clone(), a["kc"].clone(), a["vc"].clone(),
            a["cos_sin"], a["pos"], a["bt"], a["seq_lens"], Hq, HK, S,
            D ** -0.5, tmp_out, tmp_ml, a["prefix_blocks"], a["tiles"], PS)

    call()
    with pytest.raises(RuntimeError, match="tmp_out"):
        call(tmp_slots=S)              # sized for the unshared op
    with pytest.raises(RuntimeError, match="tiles"):
        call(tiles=c["tiles"].long())
    with pytest.raises(RuntimeError, match="tiles"):
        call(tiles=c["tiles"][:, :17].contiguous())
    with pytest.raises(RuntimeError, match="prefix_blocks"):
        call(prefix_blocks=c["prefix_blocks"].long())
    with pytest.raises(RuntimeError, match="prefix_blocks"):
        call(prefix_blocks=c["prefix_blocks"][:2])
    with pytest.raises(RuntimeError, match="same GPU"):
        call(tiles=c["tiles"].cpu())
    # n_rows lives in device memory, which the op never reads on the host:
    # the check for it is the one callers run on their host copy
    wide = c["tiles"].cpu().clone()
    wide[0, 0] = 16 // G + 1
    with pytest.raises(ValueError, match="at most"):
        ops.check_prefix_tiles(wide, G)
    torch.cuda.synchronize()


# ---- engine level ------------------------------------------------------
def _toks(n, salt):
    return [(salt * 131 + i * 29 + 7) % 512 for i in range(n)]


def _engine(min_tokens, kv_dtype="bf16", max_splits=None):
    from kukeon_amd.engine.config import EngineConfig, tiny_llama
    from kukeon_amd.engine.engine import LLMEngine
    from kukeon_amd.models.llama import LlamaModel

    torch.manual_seed(0)
    cfg = tiny_llama()
    ecfg = EngineConfig(max_model_len=128, max_sessions=4, num_kv_blocks=128,
                        use_graphs=True, graph_buckets=(1, 2, 4),
                        decode_microbatch=4, kv_dtype=kv_dtype,
                        shared_prefix_min_tokens=min_tokens)
    engine = LLMEngine(LlamaModel(cfg, device=DEV), cfg, ecfg, device=DEV)
    if max_splits is not None:
        engine.max_splits = max_splits
    return engine


def _fork_run(engine, n_new, template=48):
    """A template of full blocks forked into 3 children with different 5-9
    token prompts. -> (tokens per child, kvs, context per child)"""
    from kukeon_amd.engine.config import SamplingParams
    from kukeon_amd.engine.kv_cache import SequenceKV
    tmpl = SequenceKV(BS)
    engine.add_request(tmpl, _toks(template, 1),
                       SamplingParams(temperature=0.0, max_new_tokens=0))
    while engine.has_work():
        engine.step()
    kids = engine.fork_sequence(tmpl, 3)
    prompts = [_toks(5 + 2 * i, 10 + i) for i in range(3)]
    sp = SamplingParams(temperature=0.0, max_new_tokens=n_new)
    rids = [engine.add_request(kv, p, sp) for kv, p in zip(kids, prompts)]
    got = {rid: [] for rid in rids}
    while engine.has_work():
        for o in engine.step():
            got[o.req_id].extend(o.new_tokens)
    return ([got[r] for r in rids], [tmpl] + kids,
            [template + len(p) for p in prompts])


@functools.lru_cache(maxsize=None)
def _one_decode_step(min_tokens, max_splits=None):
    """max_new_tokens = 2 is exactly one decode step. -> first tokens, the
    K/V rows that step appended [layer][child] and the counters."""
    engine = _engine(min_tokens, max_splits=max_splits)
    toks, kvs, ctxs = _fork_run(engine, 2)
    rows = []
    for layer in range(engine.kv.k.shape[0]):
        rows.append([torch.cat([
            cache[layer, kv.blocks[c // BS], :, c % BS].float().flatten()
            for cache in (engine.kv.k, engine.kv.v)]).cpu()
            for kv, c in zip(kvs[1:], ctxs)])
    return dict(first=[t[0] for t in toks], lens=[len(t) for t in toks],
                rows=rows, steps=engine.shared_prefix_steps,
                rows_in_tiles=engine.shared_prefix_rows,
                shared_graphs=sorted(engine.shared_graphs),
                graphs=sorted(engine.graphs))


def _layer_diffs(a, b):
    """max |a - b| / max |b| per layer over the appended K/V rows."""
    return [max(float((x - y).abs().max()) for x, y in zip(la, lb)) /
            max(float(y.abs().max()) for y in lb)
            for la, lb in zip(a["rows"], b["rows"])]


def test_engine_one_decode_step_on_and_off():
    """The same forked workload with the path on and off. The first tokens
    come from prefill; the K/V row the decode step appends is a function of
    the previous layers' attention output, so layer 0 is bit-equal and the
    later layers differ by summation order only. The yardstick printed
    beside it is the same quantity between two unshared runs at
    max_splits 8 and 32, which also differ in summation order only."""
    on, off = _one_decode_step(16), _one_decode_step(0)
    assert on["first"] == off["first"]
    assert on["lens"] == off["lens"] == [2, 2, 2]
    assert (on["steps"], on["rows_in_tiles"]) == (1, 3)
    assert (off["steps"], off["rows_in_tiles"]) == (0, 0)
    assert on["shared_graphs"] == [4] and on["graphs"] == []
    assert off["shared_graphs"] == [] and off["graphs"] == [4]
    diffs = _layer_diffs(on, off)
    yard = _layer_diffs(_one_decode_step(0, 8), _one_decode_step(0, 32))
    print(f"appended K/V rows, shared vs unshared, per layer: {diffs}; "
          f"unshared max_splits 8 vs 32: {yard}")
    assert diffs[0] == 0.0
    for x, y in zip(on["rows"][0], off["rows"][0]):
        assert torch.equal(x, y)
    assert all(d <= 2e-2 for d in diffs[1:]), diffs


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_engine_greedy_run_finishes_and_frees(kv_dtype):
    engine = _engine(16, kv_dtype)
    toks, kvs, _ = _fork_run(engine, 9)
    assert [len(t) for t in toks] == [9, 9, 9]
    assert engine.shared_prefix_steps == 8
    assert engine.shared_prefix_rows == 3 and engine.num_running == 0
    for kv in kvs:
        engine.free_sequence(kv)
    a = engine.kv.allocator
    assert a.num_free == a.num_blocks and a.num_shared == 0
