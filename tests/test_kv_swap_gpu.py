"""Host KV tier on the GPU: the kv_pack_blocks / kv_unpack_blocks kernels
against the reference (raw bits, whole buffers), their 64-bit offsets on a
cache beyond 4 GiB, the bindings' argument checks, and a session that is
swapped out to pinned host memory and comes back under graph replay (bf16
and fp8 KV) against a never-evicted control."""
import random

import pytest
import torch

import kukeon_amd.ops as ops
from kukeon_amd.ops import reference

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

DEV = "cuda:0"
BS = 16


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _filled(shape, dtype, side):
    """Small integers that differ by layer, block, side and offset."""
    L, NB = shape[0], shape[1]
    per = shape[2] * shape[3] * shape[4]
    v = (torch.arange(L, device=DEV)[:, None, None] * 37 +
         torch.arange(NB, device=DEV)[None, :, None] * 11 +
         torch.arange(per, device=DEV)[None, None, :] + side * 101)
    v = v % (256 if dtype == torch.uint8 else 251)
    return v.to(dtype).view(shape).contiguous()


def _as_t(x):
    return torch.tensor(x, dtype=torch.int32, device=DEV)


def _staging(cap, shape, dtype, fill):
    L, _, Hk, bs, D = shape
    return torch.full((cap, 2, L, Hk, bs, D), fill, device=DEV).to(dtype)


@pytest.mark.parametrize("extra", [0, 3], ids=["cap=n", "cap>n"])
@pytest.mark.parametrize("n", [0, 1, 5, 67])
@pytest.mark.parametrize("shape,dtype", [
    ((3, 160, 2, 16, 128), torch.bfloat16),
    ((3, 160, 2, 16, 128), torch.uint8),
    ((3, 160, 8, 16, 128), torch.bfloat16),
    # 1280 vectors per block: the unrolled loop, then its tail
    ((3, 160, 5, 16, 128), torch.bfloat16),
], ids=["hk2-bf16", "hk2-u8", "hk8-bf16", "hk5-bf16"])
def test_kernels_match_reference(shape, dtype, n, extra):
    k, v = _filled(shape, dtype, 0), _filled(shape, dtype, 1)
    k0, v0 = k.clone(), v.clone()
    perm = list(range(shape[1]))
    random.Random(n).shuffle(perm)
    src, dst = _as_t(perm[:n]), _as_t(perm[n:2 * n])
    cap = n + extra
    staging = _staging(cap, shape, dtype, 7)
    want = _staging(cap, shape, dtype, 7)
    reference.kv_pack_blocks(k, v, src, want)
    ops.kv_pack_blocks(k, v, src, staging)
    torch.cuda.synchronize()
    assert torch.equal(_bits(staging[:n]), _bits(want[:n]))
    for i, b in enumerate(perm[:min(n, 2)]):
        assert torch.equal(_bits(staging[i]),
                           _bits(torch.stack([k0[:, b], v0[:, b]])))
    assert (staging[n:] == 7).all()           # records n..cap untouched
    assert torch.equal(_bits(k), _bits(k0)) and torch.equal(_bits(v), _bits(v0))
    ek, ev = k0.clone(), v0.clone()
    reference.kv_unpack_blocks(want, ek, ev, dst)
    ops.kv_unpack_blocks(staging, k, v, dst)
    torch.cuda.synchronize()
    assert torch.equal(_bits(k), _bits(ek))
    assert torch.equal(_bits(v), _bits(ev))
    if n:
        assert not torch.equal(_bits(k), _bits(k0))
        assert torch.equal(_bits(k[:, dst.long()]), _bits(k0[:, src.long()]))


def test_offsets_beyond_4gib():
    free, _ = torch.cuda.mem_get_info()
    if free < (16 << 30):
        pytest.skip("needs 16 GiB of free HBM")
    shape = (2, 70000, 8, 16, 128)
    k = torch.empty(shape, dtype=torch.bfloat16, device=DEV)
    v = torch.empty(shape, dtype=torch.bfloat16, device=DEV)
    assert k[1, 69999].data_ptr() - k.data_ptr() > (1 << 32)
    srcs = [0, 69998, 12345]
    dsts = [69990, 69000, 66000]
    canaries = [69999, 1, 69997, 12346, 69989, 69991, 65999, 66001, 68999,
                69001, 12344]
    per = 8 * 16 * 128

    def pattern(layer, side, salt):
        x = torch.arange(per, device=DEV) % 199 + layer * 3 + side * 5 + salt
        return x.to(torch.bfloat16).view(8, 16, 128)

    salt = {b: i for i, b in enumerate(srcs + dsts + canaries)}
    for side, cache in enumerate((k, v)):
        for layer in range(2):
            for b in salt:
                cache[layer, b] = pattern(layer, side, salt[b])
    staging = _staging(3, shape, torch.bfloat16, 0)
    ops.kv_pack_blocks(k, v, _as_t(srcs), staging)
    torch.cuda.synchronize()
    for i, s in enumerate(srcs):
        for side in range(2):
            for layer in range(2):
                assert torch.equal(_bits(staging[i, side, layer]),
                                   _bits(pattern(layer, side, salt[s]))), \
                    (i, side, layer)
    ops.kv_unpack_blocks(staging, k, v, _as_t(dsts))
    torch.cuda.synchronize()
    for side, cache in enumerate((k, v)):
        for layer in range(2):
            for s, d in zip(srcs, dsts):
                want = _bits(pattern(layer, side, salt[s]))
                assert torch.equal(_bits(cache[layer, s]), want), (side, layer, s)
                assert torch.equal(_bits(cache[layer, d]), want), (side, layer, d)
            for b in canaries:
                assert torch.equal(_bits(cache[layer, b]),
                                   _bits(pattern(layer, side, salt[b]))), \
                    (side, layer, b)


def test_bindings_reject_bad_arguments():
    shape = (2, 8, 2, 16, 128)
    k = torch.zeros(shape, dtype=torch.bfloat16, device=DEV)
    v = torch.zeros(shape, dtype=torch.bfloat16, device=DEV)
    wide = torch.zeros((2, 16, 2, 16, 128), dtype=torch.bfloat16, device=DEV)
    st = _staging(2, shape, torch.bfloat16, 1)
    one, three = _as_t([1]), _as_t([1, 2, 3])
    bad = [
        ("contiguous", (wide[:, ::2], v, one, st)),
        ("shape", (k, wide, one, st)),
        ("dtype", (k, v.view(torch.int16), one, st)),
        ("staging", (k, v, one, _staging(2, (3, 8, 2, 16, 128),
                                         torch.bfloat16, 1))),
        ("staging", (k, v, one, st.view(torch.int16))),
        ("staging", (k, v, one, st[:, 0])),
        ("capacity", (k, v, three, st)),
        ("int32", (k, v, one.long(), st)),
    ]
    for match, (a, b, blocks, staging) in bad:
        with pytest.raises(RuntimeError, match=match):
            ops.kv_pack_blocks(a, b, blocks, staging)
        with pytest.raises(RuntimeError, match=match):
            ops.kv_unpack_blocks(staging, a, b, blocks)
    torch.cuda.synchronize()
    assert not k.any() and not v.any() and not wide.any()
    assert (st == 1).all()


# ---- engine level ------------------------------------------------------
def _engine(kv_dtype, num_kv_blocks, host_blocks=0):
    from kukeon_amd.engine.config import EngineConfig, tiny_llama
    from kukeon_amd.engine.engine import LLMEngine
    from kukeon_amd.models.llama import LlamaModel

    torch.manual_seed(0)
    cfg = tiny_llama()
    ecfg = EngineConfig(max_model_len=128, max_sessions=4,
                        num_kv_blocks=num_kv_blocks, use_graphs=True,
                        graph_buckets=(1, 2, 4), decode_microbatch=4,
                        kv_dtype=kv_dtype, kv_host_blocks=host_blocks,
                        kv_swap_staging_blocks=2)
    return LLMEngine(LlamaModel(cfg, device=DEV), cfg, ecfg, device=DEV)


def _toks(n, salt):
    return [(salt * 131 + i * 29 + 7) % 512 for i in range(n)]


def _submit(engine, kv, prompt, n_new):
    from kukeon_amd.engine.config import SamplingParams
    return engine.add_request(kv, prompt, SamplingParams(
        temperature=0.0, max_new_tokens=n_new))


def _drain(engine, got):
    while engine.has_work():
        for o in engine.step():
            got.setdefault(o.req_id, []).extend(o.new_tokens)


def _run(engine, kv, prompt, n_new):
    got = {}
    rid = _submit(engine, kv, prompt, n_new)
    _drain(engine, got)
    return got[rid]


def _new_kv():
    from kukeon_amd.engine.kv_cache import SequenceKV
    return SequenceKV(BS)


def _gathered(engine, kv, t):
    idx = torch.tensor([kv.blocks[p // BS] for p in range(t)], device=DEV)
    off = torch.tensor([p % BS for p in range(t)], device=DEV)
    return (_bits(engine.kv.k[:, idx, :, off]).clone(),
            _bits(engine.kv.v[:, idx, :, off]).clone())


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_engine_swapped_session_returns_under_graph_replay(kv_dtype):
    pa, fa = _toks(42, 1), _toks(3, 2)
    pb = _toks(40, 3)
    # control: A's two turns on a pool that never evicts, beside the same
    # neighbour so that both engines make the same model passes
    control = _engine(kv_dtype, 128)
    ca, cb = _new_kv(), _new_kv()
    want1 = _run(control, ca, pa, 6)
    got = {}
    rb = _submit(control, cb, pb, 24)
    for _ in range(2):                        # B is decoding
        for o in control.step():
            got.setdefault(o.req_id, []).extend(o.new_tokens)
    assert control.num_running == 1
    ra = _submit(control, ca, fa, 9)
    _drain(control, got)
    want2, want_b = got[ra], got[rb]
    assert control.swap_out_blocks == 0 and not ca.host_blocks

    # 8 blocks: A (3 blocks) must leave for C (3) and B (4) to be admitted
    engine = _engine(kv_dtype, 8, host_blocks=32)
    assert engine.host_kv.pool.is_pinned()
    a, b, c = _new_kv(), _new_kv(), _new_kv()
    assert _run(engine, a, pa, 6) == want1
    n0 = a.num_tokens
    k0, v0 = _gathered(engine, a, n0)
    assert k0.any() and v0.any()
    _run(engine, c, _toks(40, 4), 6)
    got = {}
    rb = _submit(engine, b, pb, 24)
    for _ in range(2):
        for o in engine.step():
            got.setdefault(o.req_id, []).extend(o.new_tokens)
    assert engine.num_running == 1 and engine.graphs
    assert len(a.host_blocks) == 3 and a.blocks == [] and a.num_tokens == n0
    assert engine.swap_out_blocks >= 3 and engine.swapped_sessions >= 1
    ra = _submit(engine, a, fa, 9)            # returns while B decodes
    _drain(engine, got)
    assert 2 in engine.graphs
    assert got[ra] == want2 and got[rb] == want_b
    assert not a.host_blocks and engine.swap_in_blocks == 3
    k1, v1 = _gathered(engine, a, n0)
    assert torch.equal(k0, k1) and torch.equal(v0, v1)
    for kv in (a, b, c):
        engine.free_sequence(kv)
    al, hl = engine.kv.allocator, engine.host_kv.allocator
    assert al.num_free == al.num_blocks and al.num_shared == 0
    assert hl.num_free == hl.num_blocks and engine.swapped_sessions == 0
