"""CPU side of the fused decode-attention op: the reference
paged_attention_rope is the composition of the reference rope_kv_append
(block-table mode) and paged_attention, and leaves qkv untouched."""
import pytest
import torch

import kukeon_amd.ops as ops
from kukeon_amd.ops import reference

B, HQ, HK, D, BS = 5, 4, 2, 128, 16
CTXS = [1, 16, 17, 40, 0]
POS = [0, 15, 16, 39, -1]


def _inputs(fp8):
    gen = torch.Generator().manual_seed(3)
    nblk = [(c + BS - 1) // BS for c in CTXS]
    NB = sum(nblk) + 2
    perm = torch.randperm(NB, generator=gen)
    bt = torch.full((B, max(nblk)), int(perm[-1]), dtype=torch.int32)
    nxt = 0
    for b, n in enumerate(nblk):
        bt[b, :n] = perm[nxt:nxt + n].to(torch.int32)
        nxt += n
    kc = torch.randn(NB, HK, BS, D, generator=gen).bfloat16()
    vc = torch.randn(NB, HK, BS, D, generator=gen).bfloat16()
    if fp8:
        kc = kc.float().to(torch.float8_e4m3fn).view(torch.uint8)
        vc = vc.float().to(torch.float8_e4m3fn).view(torch.uint8)
    qkv = torch.randn(B, (HQ + 2 * HK) * D, generator=gen).bfloat16()
    inv = 1.0 / (500000.0 ** (torch.arange(0, D, 2).float() / D))
    fr = torch.outer(torch.arange(64).float(), inv)
    cos_sin = torch.cat([fr.cos(), fr.sin()], dim=1)
    return (qkv, kc, vc, cos_sin, torch.tensor(POS, dtype=torch.int32), bt,
            torch.tensor(CTXS, dtype=torch.int32))


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("via_ops", [False, True])
def test_reference_fused_equals_composition(fp8, via_ops):
    qkv, kc, vc, cos_sin, pos, bt, seq_lens = _inputs(fp8)
    scale = D ** -0.5

    qkv_c, kc_c, vc_c = qkv.clone(), kc.clone(), vc.clone()
    out_c = torch.full((B, HQ * D), 7.0, dtype=torch.bfloat16)
    reference.rope_kv_append(qkv_c, kc_c, vc_c, cos_sin, pos,
                             torch.zeros(B, dtype=torch.int32), HQ, HK, D,
                             block_table=bt)
    reference.paged_attention(out_c, qkv_c, kc_c, vc_c, bt, seq_lens, 0, 4,
                              scale)

    qkv_f, kc_f, vc_f = qkv.clone(), kc.clone(), vc.clone()
    out_f = torch.full((B, HQ * D), 7.0, dtype=torch.bfloat16)
    fn = ops.paged_attention_rope if via_ops else reference.paged_attention_rope
    fn(out_f, qkv_f, kc_f, vc_f, cos_sin, pos, bt, seq_lens, HQ, HK, 4, scale,
       None, None)

    assert torch.equal(out_f, out_c)
    assert torch.equal(kc_f, kc_c) and torch.equal(vc_f, vc_c)
    assert not torch.equal(kc_f, kc)          # something was appended
    assert torch.equal(qkv_f, qkv)            # the fused op leaves qkv alone
    assert not torch.equal(qkv_c, qkv)        # the unfused op rotates it
