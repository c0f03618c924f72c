"""Decode attention as one launch: ops.paged_attention_rope (RoPE on q in
registers, K rotate + K/V append by the wave that reads the row, split
merge inside the workgroup when S <= 8) against the three-launch sequence
rope_kv_append + paged_attention, against the fp32 reference, and at the
engine level with KUKEON_DECODE_ATTN_FUSED at 1 and at 0."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import kukeon_amd.ops as ops
from kukeon_amd.ops import reference

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs MI355X", allow_module_level=True)

DEV = "cuda:0"
B, HK, D, BS = 6, 2, 128, 16
# ctx 1 and 17 put the new token first in a fresh block, 16 last in a block;
# the last row is dead (seq_len 0, position -1)
CTXS = [1, 16, 17, 100, 250, 0]
POS = [c - 1 for c in CTXS]
OUT_SENTINEL = 7.0      # exact in bf16
TAIL_SENTINEL = -123.0
MAXPOS = 256


def _ints(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[
        t.element_size()])


def _cos_sin():
    inv = 1.0 / (500000.0 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.outer(torch.arange(MAXPOS).float(), inv)
    return torch.cat([fr.cos(), fr.sin()], dim=1)


def _build(G, fp8, ctxs, poss, seed=5):
    """Inputs in the manner of test_ops_gpu._paged_case: seeded random
    block-table permutation, and NaN (0x7f for fp8) at every cache position
    outside the old context: the valid region of a sequence is [0, ctx)
    minus the new token's own position, so the slot the append goes to
    holds NaN until it is written."""
    Hq = G * HK
    nb_rows = len(ctxs)
    gen = torch.Generator().manual_seed(seed)
    nblk = [max((c + BS - 1) // BS, p // BS + 1 if p >= 0 else 0)
            for c, p in zip(ctxs, poss)]
    NB = sum(nblk) + 4
    perm = torch.randperm(NB, generator=gen)
    bt = torch.full((nb_rows, max(nblk)), int(perm[-1]), dtype=torch.int32)
    valid = torch.zeros(NB, BS, dtype=torch.bool)
    nxt = 0
    for b, (c, p, n) in enumerate(zip(ctxs, poss, nblk)):
        ids = perm[nxt:nxt + n]
        nxt += n
        bt[b, :n] = ids.to(torch.int32)
        v = torch.arange(n * BS) < c
        if p >= 0:
            v[p] = False
        valid[ids] = v.view(n, BS)
    valid = valid[:, None, :, None].expand(NB, HK, BS, D)

    def cache():
        x = torch.randn(NB, HK, BS, D, generator=gen).bfloat16()
        if fp8:
            x = x.float().to(torch.float8_e4m3fn).view(torch.uint8)
            return torch.where(valid, x, torch.tensor(0x7f, dtype=torch.uint8))
        return x.masked_fill(~valid, float("nan"))

    kc, vc = cache(), cache()
    qkv = torch.randn(nb_rows, (Hq + 2 * HK) * D, generator=gen).bfloat16()
    seq_lens = torch.tensor(ctxs, dtype=torch.int32)
    pos = torch.tensor(poss, dtype=torch.int32)
    return qkv, kc, vc, _cos_sin(), pos, bt, seq_lens


@functools.lru_cache(maxsize=None)
def _case(G, fp8):
    """Device inputs plus the fp32 reference (out, appended caches), built
    once per (G, fp8) and shared read-only by every split count."""
    cpu = _build(G, fp8, CTXS, POS)
    qkv, kc, vc, cos_sin, pos, bt, seq_lens = cpu
    Hq = G * HK
    ref = torch.empty(B, Hq * D, dtype=torch.bfloat16)
    reference.paged_attention_rope(ref, qkv, kc.clone(), vc.clone(), cos_sin,
                                   pos, bt, seq_lens, Hq, HK, 1, D ** -0.5)
    return tuple(t.to(DEV) for t in cpu) + (ref.float(),)


def _workspaces(nrows, Hq, splits, guard=1024):
    """NaN where the kernels may write, a sentinel behind."""
    bufs = []
    for n in (nrows * Hq * splits * D, nrows * Hq * splits * 2):
        buf = torch.full((n + guard,), float("nan"), dtype=torch.float32,
                         device=DEV)
        buf[n:] = TAIL_SENTINEL
        bufs.append((buf[:n], buf[n:]))
    return bufs


def _run(inputs, G, splits, fused, caches=None):
    """One decode-attention step on private copies of qkv and the caches.
    Returns (out, qkv, kc, vc, workspaces)."""
    qkv, kc, vc, cos_sin, pos, bt, seq_lens = inputs[:7]
    nrows, Hq = qkv.shape[0], G * HK
    qkv = qkv.clone()
    kc, vc = caches if caches is not None else (kc.clone(), vc.clone())
    out = torch.full((nrows, Hq * D), OUT_SENTINEL, dtype=torch.bfloat16,
                     device=DEV)
    ws = _workspaces(nrows, Hq, splits)
    if fused:
        ops.paged_attention_rope(out, qkv, kc, vc, cos_sin, pos, bt, seq_lens,
                                 Hq, HK, splits, D ** -0.5, ws[0][0],
                                 ws[1][0])
    else:
        slots = torch.zeros(nrows, dtype=torch.int32, device=DEV)
        ops.rope_kv_append(qkv, kc, vc, cos_sin, pos, slots, Hq, HK, D,
                           block_table=bt)
        ops.paged_attention(out, qkv, kc, vc, bt, seq_lens, 0, splits,
                            D ** -0.5, ws[0][0], ws[1][0])
    return out, qkv, kc, vc, ws


def _assert_same_bits(a, b, what):
    assert torch.equal(_ints(a), _ints(b)), what


GRID = [(G, S, fp8) for fp8 in (False, True) for G in (1, 4, 8, 16)
        for S in (1, 3, 4, 5, 8, 16, 32)
        # fp8 differs from bf16 only in the loads and the append packing:
        # one G per launch plan is enough there
        if not fp8 or G in (4, 16)]


@pytest.mark.parametrize("G,splits,fp8", GRID)
def test_fused_matches_three_launch_sequence(G, splits, fp8):
    """out and both whole caches bit-equal to rope_kv_append +
    paged_attention (whole caches: a stray write shows too), within the
    project's tolerance of the fp32 reference, and the op's contract."""
    case = _case(G, fp8)
    out_u, _, kc_u, vc_u, _ = _run(case, G, splits, fused=False)
    out_f, qkv_f, kc_f, vc_f, ws = _run(case, G, splits, fused=True)
    _assert_same_bits(out_f, out_u, "out")
    _assert_same_bits(kc_f, kc_u, "k_cache")
    _assert_same_bits(vc_f, vc_u, "v_cache")

    # ---- against the fp32 reference ----
    ref = case[-1]
    tol = 7e-2 if fp8 else 2e-2
    got = out_f.cpu().float()
    assert not torch.isnan(got).any()
    live = [b for b, c in enumerate(CTXS) if c > 0]
    dead = [b for b, c in enumerate(CTXS) if c <= 0]
    torch.testing.assert_close(got[live], ref[live], rtol=tol, atol=tol)

    # ---- contract ----
    _assert_same_bits(qkv_f, case[0], "qkv must be left untouched")
    assert (got[dead] == OUT_SENTINEL).all()
    for body, tail in ws:
        want = torch.full_like(tail, TAIL_SENTINEL)
        _assert_same_bits(tail, want, "workspace guard tail")
        if splits <= 8:
            assert torch.isnan(body).all(), "workspace written at S <= 8"
    # the append is idempotent: a second call on the appended caches
    out_2, _, kc_2, vc_2, _ = _run(case, G, splits, fused=True,
                                   caches=(kc_f, vc_f))
    _assert_same_bits(out_2, out_f, "second call")
    _assert_same_bits(kc_2, kc_u, "k_cache after second call")


@pytest.mark.parametrize("splits", [1, 8, 32])
@pytest.mark.parametrize("fp8", [False, True])
def test_append_without_a_reader(splits, fp8):
    """Rows whose new block no split slot covers are still appended, as
    rope_kv_append would: seq_len 0 with a live position, and a position
    past the context's last block. position -1 with a live context rotates
    and appends nothing."""
    G = 4
    ctxs, poss = [0, 10, 40], [5, 20, -1]
    case = tuple(t.to(DEV) for t in _build(G, fp8, ctxs, poss, seed=11))
    out_u, _, kc_u, vc_u, _ = _run(case, G, splits, fused=False)
    out_f, qkv_f, kc_f, vc_f, _ = _run(case, G, splits, fused=True)
    _assert_same_bits(out_f, out_u, "out")
    _assert_same_bits(kc_f, kc_u, "k_cache")
    _assert_same_bits(vc_f, vc_u, "v_cache")
    _assert_same_bits(qkv_f, case[0], "qkv")
    assert not _ints(kc_f).equal(_ints(case[1])), "nothing was appended"
    got = out_f.cpu().float()
    assert (got[0] == OUT_SENTINEL).all()
    assert not torch.isnan(got[1:]).any()


# ---------------------------------------------------------------------------
# engine level: the switch is read at import, so each setting is a fresh
# child process; one child runs every (kv dtype, split cap) combination
_CHILD = r"""
import json, sys, torch
from kukeon_amd.engine.config import EngineConfig, SamplingParams, tiny_llama
from kukeon_amd.engine.engine import LLMEngine
from kukeon_amd.engine.kv_cache import SequenceKV
from kukeon_amd.models.llama import LlamaModel
import kukeon_amd.ops as ops

res = {"fused": ops.DECODE_ATTN_FUSED}
cfg = tiny_llama()
# the second prompt's context crosses a block boundary while decoding
prompts = [[7, 3, 99, 140, 11, 42, 17, 23, 5, 81],
           [(13 * i + 5) % 500 for i in range(12)]]
for kv_dtype in ("bf16", "fp8"):
    for cap in (8, 32):
        torch.manual_seed(0)
        ecfg = EngineConfig(max_model_len=256, max_sessions=4,
                            num_kv_blocks=128, use_graphs=True,
                            decode_microbatch=4, graph_buckets=(1, 2, 4),
                            kv_dtype=kv_dtype)
        model = LlamaModel(cfg, device="cuda:0")
        engine = LLMEngine(model, cfg, ecfg, device="cuda:0")
        # tiny-llama's buckets all want 32 splits (the workspace + reduce
        # path); capping them at 8 takes the in-workgroup merge
        engine.max_splits = cap
        assert engine._decode_splits(2) == cap
        toks = {}
        for p in prompts:
            rid = engine.add_request(
                SequenceKV(ecfg.block_size), p,
                SamplingParams(temperature=0.0, max_new_tokens=9))
            toks[rid] = []
        order = list(toks)
        while engine.has_work():
            for o in engine.step():
                toks[o.req_id].extend(o.new_tokens)
        res[f"{kv_dtype}-{cap}"] = [toks[r] for r in order]
print("RESULT " + json.dumps(res))
"""


@functools.lru_cache(maxsize=None)
def _engine_tokens(fused: str):
    env = dict(os.environ, KUKEON_DECODE_ATTN_FUSED=fused)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    proc = subprocess.run([sys.executable, "-c", _CHILD], env=env, cwd=root,
                          capture_output=True, text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-4000:]
    line = [l for l in proc.stdout.splitlines() if l.startswith("RESULT ")]
    return json.loads(line[-1][len("RESULT "):])


@pytest.mark.parametrize("cap", [8, 32], ids=["merge", "workspace"])
@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_engine_tokens_same_fused_and_unfused(kv_dtype, cap):
    """A few graph-replayed decode micro-batches of the small model give
    identical tokens with the fused op and with the three-launch path."""
    on, off = _engine_tokens("1"), _engine_tokens("0")
    assert on["fused"] is True and off["fused"] is False
    key = f"{kv_dtype}-{cap}"
    assert on[key] == off[key], (on[key], off[key])
    assert [len(t) for t in on[key]] == [9, 9]
