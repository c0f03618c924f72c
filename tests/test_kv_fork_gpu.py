"""Session fork on the GPU: the kv_copy_blocks kernel against torch
indexing (raw bits, whole cache), its 64-bit offsets on a cache beyond
4 GiB, the binding's argument checks, and forked sessions against unforked
controls on the graph-replay engine (bf16 and fp8 KV)."""
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


def _pairs(n, nb, seed):
    rng = random.Random(seed)
    perm = list(range(nb))
    rng.shuffle(perm)
    dst, pool = perm[:n], perm[n:]
    src = [rng.choice(pool) for _ in range(n)]
    if n >= 5:
        src[1] = src[2] = src[4]          # one source, three destinations
    as_t = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    return as_t(src), as_t(dst)


@pytest.mark.parametrize("n", [0, 1, 5, 67])
@pytest.mark.parametrize("shape,dtype", [
    ((3, 160, 2, 16, 128), torch.bfloat16),
    ((3, 160, 2, 16, 128), torch.uint8),
    ((3, 160, 8, 16, 128), torch.bfloat16),
], ids=["hk2-bf16", "hk2-u8", "hk8-bf16"])
def test_kernel_matches_torch_indexing(shape, dtype, n):
    k, v = _filled(shape, dtype, 0), _filled(shape, dtype, 1)
    src, dst = _pairs(n, shape[1], seed=n)
    ek, ev = k.clone(), v.clone()
    reference.kv_copy_blocks(ek, ev, src, dst)
    ops.kv_copy_blocks(k, v, src, dst)
    torch.cuda.synchronize()
    assert torch.equal(_bits(k), _bits(ek))
    assert torch.equal(_bits(v), _bits(ev))
    if n:
        assert not torch.equal(_bits(k), _bits(_filled(shape, dtype, 0)))


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
    canaries = [69999, 1, 69989, 69991, 65999, 66001, 68999, 69001, 12344]
    per = 8 * 16 * 128

    def pattern(layer, side, salt):
        x = torch.arange(per, device=DEV) % 199 + layer * 3 + side * 5 + salt
        return x.to(torch.bfloat16).view(8, 16, 128)

    salt = {b: i for i, b in enumerate(srcs + dsts + canaries)}
    for side, cache in enumerate((k, v)):
        for layer in range(2):
            for b in salt:
                cache[layer, b] = pattern(layer, side, salt[b])
    as_t = lambda x: torch.tensor(x, dtype=torch.int32, device=DEV)
    ops.kv_copy_blocks(k, v, as_t(srcs), as_t(dsts))
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


def test_binding_rejects_bad_arguments():
    shape = (2, 8, 2, 16, 128)
    k = torch.zeros(shape, dtype=torch.bfloat16, device=DEV)
    v = torch.zeros(shape, dtype=torch.bfloat16, device=DEV)
    one = torch.tensor([1], dtype=torch.int32, device=DEV)
    two = torch.tensor([2, 3], dtype=torch.int32, device=DEV)
    wide = torch.zeros((2, 16, 2, 16, 128), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.kv_copy_blocks(wide[:, ::2], v, one, one)
    with pytest.raises(RuntimeError, match="shape"):
        ops.kv_copy_blocks(k, wide, one, one)
    with pytest.raises(RuntimeError, match="length"):
        ops.kv_copy_blocks(k, v, one, two)
    torch.cuda.synchronize()
    assert not k.any() and not v.any()


# ---- engine level ------------------------------------------------------
def _engine(kv_dtype):
    from kukeon_amd.engine.config import EngineConfig, tiny_llama
    from kukeon_amd.engine.engine import LLMEngine
    from kukeon_amd.models.llama import LlamaModel

    torch.manual_seed(0)
    cfg = tiny_llama()
    ecfg = EngineConfig(max_model_len=128, max_sessions=4, num_kv_blocks=128,
                        use_graphs=True, graph_buckets=(1, 2, 4),
                        decode_microbatch=4, kv_dtype=kv_dtype)
    return LLMEngine(LlamaModel(cfg, device=DEV), cfg, ecfg, device=DEV)


def _toks(n, salt):
    return [(salt * 131 + i * 29 + 7) % 512 for i in range(n)]


def _run_many(engine, work, n_new):
    from kukeon_amd.engine.config import SamplingParams
    sp = SamplingParams(temperature=0.0, max_new_tokens=n_new)
    rids = [engine.add_request(kv, p, sp) for kv, p in work]
    got = {rid: [] for rid in rids}
    while engine.has_work():
        for o in engine.step():
            got[o.req_id].extend(o.new_tokens)
    return [got[rid] for rid in rids]


def _new_kv():
    from kukeon_amd.engine.kv_cache import SequenceKV
    return SequenceKV(BS)


def _gathered(engine, kv, t):
    idx = torch.tensor([kv.blocks[p // BS] for p in range(t)], device=DEV)
    off = torch.tensor([p % BS for p in range(t)], device=DEV)
    return (_bits(engine.kv.k[:, idx, :, off]),
            _bits(engine.kv.v[:, idx, :, off]))


P = _toks(21, 1)
S = [_toks(7, 10 + i) for i in range(4)]
N_NEW = 9   # decode crosses the block boundary at 32


def _assert_no_leak(engine):
    a = engine.kv.allocator
    assert a.num_free == a.num_blocks and a.num_shared == 0


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_engine_child_equals_control(kv_dtype):
    engine = _engine(kv_dtype)
    want = []
    for s in S[:2]:                 # controls: P prefill-only, then S, alone
        kv = _new_kv()
        _run_many(engine, [(kv, P)], 0)
        want.append(_run_many(engine, [(kv, s)], N_NEW)[0])
        engine.free_sequence(kv)
    parent = _new_kv()
    assert _run_many(engine, [(parent, P)], 0) == [[]]
    assert parent.pending_token is None and engine.num_running == 0
    (child,) = engine.fork_sequence(parent)
    assert child.blocks[0] == parent.blocks[0]
    assert child.blocks[1] != parent.blocks[1]
    pk, pv = _gathered(engine, parent, 21)
    ck, cv = _gathered(engine, child, 21)
    assert torch.equal(pk, ck) and torch.equal(pv, cv)
    assert pk.any() and pv.any()
    assert _run_many(engine, [(child, S[0])], N_NEW)[0] == want[0]
    assert _run_many(engine, [(parent, S[1])], N_NEW)[0] == want[1]
    engine.free_sequence(parent)
    engine.free_sequence(child)
    _assert_no_leak(engine)


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_engine_parent_and_three_children_in_one_bucket(kv_dtype):
    engine = _engine(kv_dtype)
    indep = [_new_kv() for _ in range(4)]
    for kv in indep:
        _run_many(engine, [(kv, P)], 0)
    want = _run_many(engine, list(zip(indep, S)), N_NEW)
    for kv in indep:                # four rows must suffice for the fork
        engine.free_sequence(kv)
    parent = _new_kv()
    _run_many(engine, [(parent, P)], 0)
    kids = engine.fork_sequence(parent, 3)
    assert engine.kv.allocator.num_shared == 1
    for c in kids:
        pk, pv = _gathered(engine, parent, 21)
        ck, cv = _gathered(engine, c, 21)
        assert torch.equal(pk, ck) and torch.equal(pv, cv)
    got = _run_many(engine, list(zip([parent] + kids, S)), N_NEW)
    assert 4 in engine.graphs
    assert got == want
    for kv in [parent] + kids:
        engine.free_sequence(kv)
    _assert_no_leak(engine)
