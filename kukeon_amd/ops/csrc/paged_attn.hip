// Paged decode attention for gfx950 (MI355X): one query token per
// sequence against a paged KV cache, split-KV (flash-decode) on the matrix
// cores. One attention kernel; decode runs it as ONE launch whenever the
// splits of a sequence fit in one workgroup (S <= 8), else as a pair with
// the reduce kernel.
//
// paged_attn_kernel<FP8, ROPE> — grid (B, Hk, ceil(S/NW)), NW waves per
//   workgroup: NW = 4 for S <= 4 and for S > 8, NW = 8 for 5 <= S <= 8.
//   The whole GQA group (G = Hq/Hk <= 16 q-heads sharing one kv-head)
//   rides the MFMA N axis, so each K/V block is read from HBM once per
//   group — KV bandwidth is the decode cost, never multiply it by G.
//   Padding columns (heads >= G) are per-lane garbage: nothing crosses into
//   a real head and they are never written back.
//   Per 16-token cache block (one tile), lane maps as in attn_frag.h:
//     - S^T[tok, head] = K . Q^T on 16x16x32 MFMAs (K = head_dim chunks);
//       softmax is then lane-local plus two cross-lane max/sum steps.
//     - O^T[d, head] += V^T . P^T on 16x16x16 MFMAs (K = the 16 tokens).
//       In this swapped shape the C layout of the scores IS the B layout
//       of P, so P needs no cross-lane redistribution at all, just two
//       v_cvt_pk_bf16_f32.
//     - 8 KiB LDS per wave (dynamic: 32 KiB at NW = 4, 64 KiB at NW = 8,
//       so a CU holds 16 waves either way), no barriers in the tile loop.
//
// Split slots. The KV blocks of a sequence are cut into S contiguous
//   ranges ("slots") of ceil(nblocks/S) blocks; a slot past the end has an
//   empty range. Wave w of workgroup z owns slot NW*z + w and walks that
//   range alone. No workgroup ever waits for, signals or reads another:
//   there are no atomics, counters or flags anywhere in this file.
//
// ROPE (ops.paged_attention_rope; q is the fused qkv row, untouched):
//   - Q is rotated in registers. qf[st] holds dims st*32 + g4*8..+7, the
//     x half for st = 0,1 and the matching y half for st = 2,3, so the
//     NEOX rotation is lane-local; rope_rotate8 (common.h) rounds exactly
//     as rope_kv_kernel does.
//   - The new token's K row (rotated) and V row are appended to the cache
//     by the one wave whose slot range holds block pos/16 — the only wave
//     that reads that row, so no other wave depends on the write. It
//     stores, issues __threadfence_block(), and only then loads K/V, so
//     what it attends to is what the cache holds (fp8 rounding included).
//     If no slot holds the block (ctx <= 0, or pos/16 >= nblocks) slot
//     0's wave appends and nobody reads it; pos < 0 appends nothing.
//
// Merge. When S <= NW (one workgroup per (b, hk)) the waves park their
//   unnormalised O and (m, l) in the V^T buffers, which are dead by then,
//   and wave 0 computes the output rows with the loop order and
//   expressions of paged_attn_reduce_kernel (merge_weight / fmaf below),
//   bit-equal to the two-kernel path; tmp_out / tmp_ml are not touched.
//   Wave 0 keeps its own O in registers: with G = 16 the other waves' O
//   fills their 8 KiB exactly, and wave 0's buffer takes every (m, l).
//   Otherwise each wave writes its partial into tmp_out / tmp_ml at its
//   slot — every slot < S on every call (an empty range writes O = 0,
//   m = -inf, l = 0), which lets paged_attn_reduce_kernel — grid (B, Hq),
//   128 threads — read all S slots unconditionally.
//
// A row with seq_len <= 0 is skipped by both kernels: its `out` row (and
//   its workspace slots) are left untouched (ROPE still appends).
//
// Hazards this kernel is written around:
//   - Non-uniform barrier. The merge path has two __syncthreads(). The only
//     returns before them are `ctx <= 0` (b is per workgroup: uniform) and
//     the non-merge path (`merge` is a kernel argument: uniform). A wave
//     whose slot is >= S, and the padding lanes rc >= G, are NOT returned
//     early on the merge path: their block range is empty, they fall
//     through the tile loop to the barriers and write nothing. The append
//     runs before any of this and contains no barrier.
//   - NaN in the cache. Stale cache rows may hold NaN, and the new token's
//     row does until the append. The score mask (-inf) and the V-row
//     zeroing are keyed on kv_hi as before; the append precedes the first
//     K/V load of the wave that reads the row.
//   - Graph replay. positions / seq_lens / block_table are read on the
//     device at every launch; the op keeps no host state and allocates
//     nothing.
//   - Register budget. __launch_bounds__ keeps 128 VGPRs (4 waves/SIMD)
//     for bf16 and fp8 alike, spill-free; the RoPE / append prologue and
//     the merge epilogue live outside the tile loop.
//   - Bit-equal RoPE: rope_rotate8 pins the FMA contraction for both
//     kernels.
//
// Two designs were measured against this one and removed; their code is in
// the history of this file. A v_dot2 kernel (workgroup per split, K/V
// staged in LDS, packed-bf16 dot products) was issue-stall bound — ~28
// dependent VALU instructions per KV token, 3.8-4.1 TB/s against 4.9-5.4
// here. A 32-token 32x32x16 MFMA tile was LDS-residency bound — 64 KiB per
// 4-wave workgroup capped a CU at 8 waves, 25-30% behind end to end.
#include "attn_frag.h"
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

namespace kukeon {

// Weight of split s in the merge; shared by the reduce kernel and the
// in-workgroup merge so both round alike.
DEV_INLINE float merge_weight(float m_s, float M) {
  return m_s == -INFINITY ? 0.f : __expf(m_s - M);
}

constexpr int kWaveLds = 2 * 128 * 16 * 2;  // two V^T images: 8 KiB

// Trailing kernel argument of paged_attn_kernel: empty for the plain op, so
// its four instantiations keep their code; the suffix pass of the
// shared-prefix op gets the per-row prefix length and the prefix slot count.
struct NoPrefix {};
struct PrefixArgs {
  const int* prefix_blocks;  // [B] leading blocks a prefix tile covers
  int prefix_splits;         // workspace slots in front of the suffix's
};

template <bool FP8, bool ROPE, bool SHARED = false>
// 128 VGPRs (4 waves/SIMD) for both cache types. fp8 used to be bounded at
// 3 waves/SIMD for headroom but compiled to 127 registers and so ran at 4;
// with the prologue added here the looser bound let it drift to 131, which
// really is 3 waves/SIMD (one 8-wave workgroup per CU) and cost 10% of the
// fp8-KV benchmark. At this bound it builds to 128 with no spill; check the
// resource usage again after any change to the tile loop.
__global__ __launch_bounds__(512, 4) void paged_attn_kernel(
    unsigned short* __restrict__ out,     // [B, Hq*D] (merge path)
    float* __restrict__ tmp_out,          // [B, Hq, S, D] f32
    float* __restrict__ tmp_ml,           // [B, Hq, S, 2]
    const unsigned short* __restrict__ q, // [B, q_stride]; ROPE: qkv rows
    void* k_cache,                        // [NB, Hk, 16, D]; ROPE appends,
    void* v_cache,                        //   so not __restrict__
    const float* __restrict__ cos_sin,    // [max_pos, D]   (ROPE)
    const int* __restrict__ positions,    // [B]            (ROPE)
    const int* __restrict__ block_table,  // [B, max_blocks]
    const int* __restrict__ seq_lens,     // [B]
    long q_stride, int Hq, int Hk, int max_blocks, int S, int merge,
    float scale, std::conditional_t<SHARED, PrefixArgs, NoPrefix> px) {
  constexpr int D = 128;
  constexpr int BS = 16;
  const int b = blockIdx.x;
  const int hk = blockIdx.y;
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int g4 = lane >> 4;       // 0..3
  const int rc = lane & 15;
  const int G = Hq / Hk;
  const int slot = blockIdx.z * (blockDim.x / WAVE) + wid;
  const int ctx = seq_lens[b];

  const int nblocks = ctx > 0 ? (ctx + BS - 1) / BS : 0;
  // SHARED (suffix pass): blocks [0, pb) are the prefix kernel's; the S
  // slots cut [pb, nblocks) and land behind the prefix slots
  int pb = 0;
  if constexpr (SHARED) pb = min(max(px.prefix_blocks[b], 0), nblocks);
  const int per_slot = (nblocks - pb + S - 1) / S;

  const int pos = ROPE ? positions[b] : -1;
  if (ROPE && pos >= 0) {
    // ---- rotate K + append K/V: the one wave that will read the row ----
    const int pblk = pos / BS;
    int owner;
    if constexpr (SHARED)
      owner = pblk >= pb && pblk < nblocks ? (pblk - pb) / per_slot : 0;
    else
      owner = pblk < nblocks ? pblk / per_slot : 0;
    if (slot == owner && pblk < max_blocks && lane < 16) {
      const unsigned short* krow =
          q + (long)b * q_stride + (long)(Hq + hk) * D;
      const unsigned short* vrow = krow + (long)Hk * D;
      const long dst =
          (((long)block_table[(long)b * max_blocks + pblk] * Hk + hk) * BS +
           pos % BS) * D;
      auto* kdst = reinterpret_cast<kv_elem_t<FP8>*>(k_cache) + dst;
      auto* vdst = reinterpret_cast<kv_elem_t<FP8>*>(v_cache) + dst;
      if (lane < 8) {  // 8 pairs per lane
        const int d0 = lane * 8;
        const float* cs = cos_sin + (long)pos * D;
        float xo[8], yo[8];
        rope_rotate8(load_bf16x8(krow + d0), load_bf16x8(krow + D / 2 + d0),
                     cs + d0, cs + D / 2 + d0, xo, yo);
        if constexpr (FP8) {
          *reinterpret_cast<uint2*>(kdst + d0) = pack_fp8x8(xo);
          *reinterpret_cast<uint2*>(kdst + D / 2 + d0) = pack_fp8x8(yo);
        } else {
          *reinterpret_cast<uint4*>(kdst + d0) = pack_bf16x8(xo);
          *reinterpret_cast<uint4*>(kdst + D / 2 + d0) = pack_bf16x8(yo);
        }
      }
      const bf16x8 v = load_bf16x8(vrow + lane * 8);
      if constexpr (FP8) {
        float f[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = v.f(j);
        *reinterpret_cast<uint2*>(vdst + lane * 8) = pack_fp8x8(f);
      } else {
        *reinterpret_cast<uint4*>(vdst + lane * 8) = v.raw;
      }
    }
    // the appending wave is the row's only reader: order its stores
    // before its own K/V loads
    __threadfence_block();
  }
  // uniform per workgroup; a wave with slot >= S leaves only where no
  // barrier follows (on the merge path its range below is empty)
  if (ctx <= 0 || (!merge && slot >= S)) return;

  // V^T images only — K is consumed straight from HBM in fragment shape
  // (16 B/lane across 64 B-line groups; the LDS round trip was pure
  // added latency here: per-wave parked time was 67% of cycles). Two
  // V^T buffers per wave: tile bi's image is written during tile bi-1,
  // so PV never waits on fresh LDS stores.
  extern __shared__ __align__(16) unsigned short vtbuf_all[];
  unsigned short* const vtbuf0 = vtbuf_all + wid * (2 * D * BS);

  const int blk_begin = pb + slot * per_slot;
  const int blk_end = min(nblocks, blk_begin + per_slot);
  const int kv_hi = min(ctx, blk_end * BS);

  const int qh = min(rc, G - 1);  // B col = q head
  // Q fragments pinned in 16 registers (L2 re-reads in the tile loop
  // measured as 4 dependent ~250-cycle stalls per tile)
  unsigned int qf[4][4];
  {
    const unsigned short* qp =
        q + (long)b * q_stride + (long)(hk * G + qh) * D;
    bf16x8 qv[4];
#pragma unroll
    for (int st = 0; st < 4; ++st)
      qv[st] = load_bf16x8(qp + st * 32 + g4 * 8);
    if (ROPE && pos >= 0) {
      // qv[st] / qv[st + 2] are the x / y halves of the same 8 pairs
      const float* cs = cos_sin + (long)pos * D;
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const int d0 = st * 32 + g4 * 8;
        float xo[8], yo[8];
        rope_rotate8(qv[st], qv[st + 2], cs + d0, cs + D / 2 + d0, xo, yo);
        qv[st].raw = pack_bf16x8(xo);
        qv[st + 2].raw = pack_bf16x8(yo);
      }
    }
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const uint4 v = qv[st].raw;
      qf[st][0] = v.x; qf[st][1] = v.y; qf[st][2] = v.z; qf[st][3] = v.w;
    }
  }

  float m = -INFINITY, l_acc = 0.f;
  f32x4_t oacc[8] = {{}, {}, {}, {}, {}, {}, {}, {}};

  const auto* kc = reinterpret_cast<const kv_elem_t<FP8>*>(k_cache);
  const auto* vc = reinterpret_cast<const kv_elem_t<FP8>*>(v_cache);

  // K in MFMA A-fragment shape: lane (rc = token, g4 = k-group) reads
  // 16 B at tok*256B + st*64B + g4*16B — lanes sharing a token cover one
  // 64 B line, so the four per-tile loads coalesce at line granularity.
  uint4 kfr[4];
  auto kfetch = [&](int bi_f) {
    const long base =
        ((long)block_table[(long)b * max_blocks + bi_f] * Hk + hk) * BS * D;
    const long off = base + (long)rc * D + g4 * 8;
#pragma unroll
    for (int st = 0; st < 4; ++st)
      kfr[st] = load_kv8(kc + off + st * 32);
  };
  // V rows (2*kp, 2*kp+1) x 8 dims per lane, transposed into the V^T image
  // (attn_frag.h; pitch 32 B, swizzle << 3)
  const int stg_d0 = rc * 8;
  uint4 vpre[2][2];
  auto vfetch = [&](int bi_f) {
    const long base =
        ((long)block_table[(long)b * max_blocks + bi_f] * Hk + hk) * BS * D;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int kp = pass * 4 + g4;
      const long voff0 = base + (long)(2 * kp) * D + stg_d0;
      const long voff1 = base + (long)(2 * kp + 1) * D + stg_d0;
      vpre[pass][0] = load_kv8(vc + voff0);
      vpre[pass][1] = load_kv8(vc + voff1);
    }
  };
  auto vwrite = [&](unsigned short* vt, int kvbase) {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int kp = pass * 4 + g4;
      uint4 r0 = vpre[pass][0];
      uint4 r1 = vpre[pass][1];
      // zero V rows past the end: a 0*NaN in the PV mfma would poison O
      if (kvbase + 2 * kp >= kv_hi) r0 = uint4{0, 0, 0, 0};
      if (kvbase + 2 * kp + 1 >= kv_hi) r1 = uint4{0, 0, 0, 0};
      const unsigned int* a0 = reinterpret_cast<const unsigned int*>(&r0);
      const unsigned int* a1 = reinterpret_cast<const unsigned int*>(&r1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned short e0 = (a0[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
        const unsigned short e1 = (a1[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
        const unsigned int packed = (unsigned)e0 | ((unsigned)e1 << 16);
        const int d = stg_d0 + j;
        const int byte = d * 32 + ((4 * kp) ^ ((d & 3) << 3));
        *reinterpret_cast<unsigned int*>(
            reinterpret_cast<char*>(vt) + byte) = packed;
      }
    }
  };

  if (blk_begin < blk_end) {
    kfetch(blk_begin);
    vfetch(blk_begin);
    vwrite(vtbuf0 + (blk_begin & 1) * (D * BS), blk_begin * BS);
  }

  for (int bi = blk_begin; bi < blk_end; ++bi) {
    const int kvbase = bi * BS;
    const unsigned short* vt = vtbuf0 + (bi & 1) * (D * BS);

    // ---- S^T = K . Q^T from the in-flight K fragments ----
    f32x4_t sacc = {};
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          as_frag(kfr[st].x, kfr[st].y, kfr[st].z, kfr[st].w),
          as_frag(qf[st][0], qf[st][1], qf[st][2], qf[st][3]),
          sacc, 0, 0, 0);
    }
    // K registers are free again: issue the next tile's fragment loads
    // (they fly under softmax + V staging + PV + the loop turnaround)
    if (bi + 1 < blk_end) kfetch(bi + 1);

    // ---- online softmax (lane holds tokens 4*g4..+3 of its head) ----
    float sv[4];
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool valid = (kvbase + 4 * g4 + r) < kv_hi;
      sv[r] = valid ? sacc[r] * scale : -INFINITY;
      tmax = fmaxf(tmax, sv[r]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, WAVE));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, WAVE));
    const float mn = fmaxf(m, tmax);
    const float alpha = (m == -INFINITY) ? 0.f : __expf(m - mn);
    m = mn;
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sv[r] = (sv[r] == -INFINITY) ? 0.f : __expf(sv[r] - mn);
      psum += sv[r];
    }
    psum += __shfl_xor(psum, 16, WAVE);
    psum += __shfl_xor(psum, 32, WAVE);
    l_acc = l_acc * alpha + psum;
#pragma unroll
    for (int dc = 0; dc < 8; ++dc)
#pragma unroll
      for (int r = 0; r < 4; ++r) oacc[dc][r] *= alpha;

    // ---- stage NEXT tile's V^T into the other buffer ----
    if (bi + 1 < blk_end) {
      vfetch(bi + 1);
      vwrite(vtbuf0 + ((bi + 1) & 1) * (D * BS), (bi + 1) * BS);
    }

    // ---- PV: P is already a 16x16x16 B fragment ----
    const bf16x4_t pfrag = as_frag(cvtpk_bf16(sv[0], sv[1]),
                                   cvtpk_bf16(sv[2], sv[3]));
#pragma unroll
    for (int dc = 0; dc < 8; ++dc) {
      const int d = dc * 16 + rc;  // A row = output dim
      const int byte = d * 32 + ((8 * g4) ^ ((d & 3) << 3));
      const uint2 vf = *reinterpret_cast<const uint2*>(
          reinterpret_cast<const char*>(vt) + byte);
      oacc[dc] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(
          as_frag(vf.x, vf.y), pfrag, oacc[dc], 0, 0, 0);
    }
  }

  if (!merge) {
    // ---- epilogue: unnormalized O + (m, l) into this wave's slot ----
    if (rc >= G) return;
    const int head = hk * G + rc;
    long wslot = ((long)b * Hq + head) * S + slot;
    if constexpr (SHARED)
      wslot = ((long)b * Hq + head) * (px.prefix_splits + S) +
              px.prefix_splits + slot;
    float* top = tmp_out + wslot * D;
#pragma unroll
    for (int dc = 0; dc < 8; ++dc) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        top[dc * 16 + 4 * g4 + r] = oacc[dc][r];
      }
    }
    if (g4 == 0) {
      float* ml = tmp_ml + wslot * 2;
      ml[0] = m;
      ml[1] = l_acc;
    }
    return;
  }

  // ---- merge inside the workgroup (S <= waves; EVERY wave gets here) ----
  // LDS after the first barrier: wave w >= 1 parks O in its own 8 KiB as
  // [head][32 float4], the float4 index XOR-ed with the head so the 16
  // heads of a store or load spread over the banks; wave 0's 8 KiB takes
  // (m, l) of every wave as [w][head] float2.
  char* const lds = reinterpret_cast<char*>(vtbuf_all);
  __syncthreads();  // all tile loops done: the V^T images are dead
  if (rc < G && slot < S) {
    if (wid > 0) {
      float4* op = reinterpret_cast<float4*>(lds + wid * kWaveLds + rc * 512);
#pragma unroll
      for (int dc = 0; dc < 8; ++dc)
        op[(dc * 4 + g4) ^ rc] =
            float4{oacc[dc][0], oacc[dc][1], oacc[dc][2], oacc[dc][3]};
    }
    if (g4 == 0)
      reinterpret_cast<float2*>(lds)[wid * 16 + rc] = float2{m, l_acc};
  }
  __syncthreads();
  if (wid != 0 || rc >= G) return;
  // same loop order and expressions as paged_attn_reduce_kernel
  const float2* ml = reinterpret_cast<const float2*>(lds) + rc;
  float M = -INFINITY;
  for (int s = 0; s < S; ++s) M = fmaxf(M, ml[s * 16].x);
  float L = 0.f;
  for (int s = 0; s < S; ++s)
    L = __builtin_fmaf(merge_weight(ml[s * 16].x, M), ml[s * 16].y, L);
  f32x4_t acc[8];
  {
    const float w = merge_weight(ml[0].x, M);
#pragma unroll
    for (int dc = 0; dc < 8; ++dc)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        acc[dc][r] = __builtin_fmaf(w, oacc[dc][r], 0.f);
  }
  for (int s = 1; s < S; ++s) {
    const float w = merge_weight(ml[s * 16].x, M);
    const float4* op =
        reinterpret_cast<const float4*>(lds + s * kWaveLds + rc * 512);
#pragma unroll
    for (int dc = 0; dc < 8; ++dc) {
      const float4 o = op[(dc * 4 + g4) ^ rc];
      acc[dc][0] = __builtin_fmaf(w, o.x, acc[dc][0]);
      acc[dc][1] = __builtin_fmaf(w, o.y, acc[dc][1]);
      acc[dc][2] = __builtin_fmaf(w, o.z, acc[dc][2]);
      acc[dc][3] = __builtin_fmaf(w, o.w, acc[dc][3]);
    }
  }
  unsigned short* orow = out + (long)b * Hq * D + (long)(hk * G + rc) * D;
#pragma unroll
  for (int dc = 0; dc < 8; ++dc) {
    unsigned short e[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) e[r] = f2us(L > 0.f ? acc[dc][r] / L : 0.f);
    *reinterpret_cast<uint2*>(orow + dc * 16 + 4 * g4) =
        uint2{(unsigned)e[0] | ((unsigned)e[1] << 16),
              (unsigned)e[2] | ((unsigned)e[3] << 16)};
  }
}

// Shared-prefix pass of ops.paged_attention[_rope]_shared. Sessions forked
// from one context hold the same leading cache blocks; with G < 16 the
// kernel above leaves 16 - G MFMA columns as padding, and every session
// fetches those blocks again. Here a tile of up to W = 16 / G sessions
// rides the N axis together: column rc is (member rc / G, q head rc % G),
// and the tile's prefix blocks are fetched, scored and softmaxed once.
//
// paged_attn_prefix_kernel<FP8, ROPE> — grid (T, Hk, ceil(PS / 4)), 4 waves.
//   tiles[t] = {n_rows, n_prefix_blocks, member rows...} (kTileCols ints);
//   n_rows == 0 is an empty tile, so the grid can stay fixed under graph
//   replay while membership changes. The block ids come from the block
//   table of the first member. Wave `slot` walks its own contiguous range
//   of ceil(n_prefix_blocks / PS) blocks with the tile loop of the kernel
//   above and writes unnormalised O and (m, l) of column rc into prefix
//   slot `slot` of that member's row (O = 0, m = -inf, l = 0 for an empty
//   range), all PS slots of every member on every call. The suffix pass
//   (paged_attn_kernel<.., SHARED>) fills the slots behind them and the
//   reduce kernel merges both. No wave waits on another, no barrier.
//   - Q is read per column from that member's row and, with ROPE, rotated
//     at that member's position, exactly as the kernel above does.
//   - Every prefix block is full and below every member's context, so no
//     score is masked. The V-row zeroing is dead for the same reason — it
//     guards rows at or past kv_hi, and here kv_hi is the end of the range —
//     and is left out.
//   - Nothing is appended here: the new token's block is never a prefix
//     block, so this kernel only reads the caches and may overlap the
//     suffix pass.
//   - n_rows, n_prefix_blocks and the member rows are clamped to what the
//     buffers hold, so bad metadata computes nonsense but stays in bounds.
constexpr int kTileCols = 2 + 16;

template <bool FP8, bool ROPE>
__global__ __launch_bounds__(256, 4) void paged_attn_prefix_kernel(
    float* __restrict__ tmp_out,          // [B, Hq, Stot, D] f32
    float* __restrict__ tmp_ml,           // [B, Hq, Stot, 2]
    const unsigned short* __restrict__ q, // [B, q_stride]; ROPE: qkv rows
    const void* __restrict__ k_cache,     // [NB, Hk, 16, D]
    const void* __restrict__ v_cache,
    const float* __restrict__ cos_sin,    // [max_pos, D]   (ROPE)
    const int* __restrict__ positions,    // [B]            (ROPE)
    const int* __restrict__ block_table,  // [B, max_blocks]
    const int* __restrict__ tiles,        // [T, kTileCols]
    long q_stride, int B, int Hq, int Hk, int max_blocks, int PS, int Stot,
    float scale) {
  constexpr int D = 128;
  constexpr int BS = 16;
  const int hk = blockIdx.y;
  // wave-uniform, and told so: slot, the block range and the loop counter
  // then live in scalar registers
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const int lane = threadIdx.x & (WAVE - 1);
  const int g4 = lane >> 4;       // 0..3
  const int rc = lane & 15;
  const int G = Hq / Hk;
  const int slot = blockIdx.z * (blockDim.x / WAVE) + wid;
  const int* tile = tiles + (long)blockIdx.x * kTileCols;
  const int n_rows = min(tile[0], 16 / G);
  if (n_rows <= 0 || slot >= PS) return;
  const int npb = min(max(tile[1], 0), max_blocks);
  const int row0 = min(max(tile[2], 0), B - 1);
  // column -> (member, head); padding columns shadow member 0
  const bool live = rc / G < n_rows;
  const int row = live ? min(max(tile[2 + rc / G], 0), B - 1) : row0;
  const int qh = rc % G;

  extern __shared__ __align__(16) unsigned short vtbuf_all[];
  unsigned short* const vtbuf0 = vtbuf_all + wid * (2 * D * BS);

  const int per_slot = (npb + PS - 1) / PS;
  const int blk_begin = slot * per_slot;
  const int blk_end = min(npb, blk_begin + per_slot);

  unsigned int qf[4][4];
  {
    const unsigned short* qp =
        q + (long)row * q_stride + (long)(hk * G + qh) * D;
    bf16x8 qv[4];
#pragma unroll
    for (int st = 0; st < 4; ++st)
      qv[st] = load_bf16x8(qp + st * 32 + g4 * 8);
    const int pos = ROPE ? positions[row] : -1;
    if (ROPE && pos >= 0) {
      const float* cs = cos_sin + (long)pos * D;
#pragma unroll
      for (int st = 0; st < 2; ++st) {
        const int d0 = st * 32 + g4 * 8;
        float xo[8], yo[8];
        rope_rotate8(qv[st], qv[st + 2], cs + d0, cs + D / 2 + d0, xo, yo);
        qv[st].raw = pack_bf16x8(xo);
        qv[st + 2].raw = pack_bf16x8(yo);
      }
    }
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const uint4 v = qv[st].raw;
      qf[st][0] = v.x; qf[st][1] = v.y; qf[st][2] = v.z; qf[st][3] = v.w;
    }
  }

  float m = -INFINITY, l_acc = 0.f;
  f32x4_t oacc[8] = {{}, {}, {}, {}, {}, {}, {}, {}};

  const auto* kc = reinterpret_cast<const kv_elem_t<FP8>*>(k_cache);
  const auto* vc = reinterpret_cast<const kv_elem_t<FP8>*>(v_cache);
  const int* bt0 = block_table + (long)row0 * max_blocks;

  // K fragments, V staging and the V^T image as in paged_attn_kernel
  uint4 kfr[4];
  auto kfetch = [&](int bi_f) {
    const long base = ((long)bt0[bi_f] * Hk + hk) * BS * D;
    const long off = base + (long)rc * D + g4 * 8;
#pragma unroll
    for (int st = 0; st < 4; ++st)
      kfr[st] = load_kv8(kc + off + st * 32);
  };
  const int stg_d0 = rc * 8;
  uint4 vpre[2][2];
  auto vfetch = [&](int bi_f) {
    const long base = ((long)bt0[bi_f] * Hk + hk) * BS * D;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int kp = pass * 4 + g4;
      vpre[pass][0] = load_kv8(vc + base + (long)(2 * kp) * D + stg_d0);
      vpre[pass][1] = load_kv8(vc + base + (long)(2 * kp + 1) * D + stg_d0);
    }
  };
  auto vwrite = [&](unsigned short* vt) {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      const int kp = pass * 4 + g4;
      const uint4 r0 = vpre[pass][0];
      const uint4 r1 = vpre[pass][1];
      const unsigned int* a0 = reinterpret_cast<const unsigned int*>(&r0);
      const unsigned int* a1 = reinterpret_cast<const unsigned int*>(&r1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned short e0 = (a0[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
        const unsigned short e1 = (a1[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
        const unsigned int packed = (unsigned)e0 | ((unsigned)e1 << 16);
        const int d = stg_d0 + j;
        const int byte = d * 32 + ((4 * kp) ^ ((d & 3) << 3));
        *reinterpret_cast<unsigned int*>(
            reinterpret_cast<char*>(vt) + byte) = packed;
      }
    }
  };

  if (blk_begin < blk_end) {
    kfetch(blk_begin);
    vfetch(blk_begin);
    vwrite(vtbuf0 + (blk_begin & 1) * (D * BS));
  }

  for (int bi = blk_begin; bi < blk_end; ++bi) {
    const unsigned short* vt = vtbuf0 + (bi & 1) * (D * BS);

    f32x4_t sacc = {};
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      sacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          as_frag(kfr[st].x, kfr[st].y, kfr[st].z, kfr[st].w),
          as_frag(qf[st][0], qf[st][1], qf[st][2], qf[st][3]),
          sacc, 0, 0, 0);
    }
    if (bi + 1 < blk_end) kfetch(bi + 1);

    // ---- online softmax, one column = one (member, head) ----
    float sv[4];
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sv[r] = sacc[r] * scale;
      tmax = fmaxf(tmax, sv[r]);
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16, WAVE));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32, WAVE));
    const float mn = fmaxf(m, tmax);
    const float alpha = (m == -INFINITY) ? 0.f : __expf(m - mn);
    m = mn;
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      sv[r] = __expf(sv[r] - mn);
      psum += sv[r];
    }
    psum += __shfl_xor(psum, 16, WAVE);
    psum += __shfl_xor(psum, 32, WAVE);
    l_acc = l_acc * alpha + psum;
#pragma unroll
    for (int dc = 0; dc < 8; ++dc)
#pragma unroll
      for (int r = 0; r < 4; ++r) oacc[dc][r] *= alpha;

    if (bi + 1 < blk_end) {
      vfetch(bi + 1);
      vwrite(vtbuf0 + ((bi + 1) & 1) * (D * BS));
    }

    const bf16x4_t pfrag = as_frag(cvtpk_bf16(sv[0], sv[1]),
                                   cvtpk_bf16(sv[2], sv[3]));
#pragma unroll
    for (int dc = 0; dc < 8; ++dc) {
      const int d = dc * 16 + rc;
      const int byte = d * 32 + ((8 * g4) ^ ((d & 3) << 3));
      const uint2 vf = *reinterpret_cast<const uint2*>(
          reinterpret_cast<const char*>(vt) + byte);
      oacc[dc] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(
          as_frag(vf.x, vf.y), pfrag, oacc[dc], 0, 0, 0);
    }
  }

  // The epilogue derives its lane indices and the member row afresh (lane
  // id from mbcnt, the row through a volatile load the prologue's cannot be
  // merged with), so nothing of it lives across the tile loop: the fp8
  // variant spilled those registers otherwise.
  const int oln = __lane_id();
  const int om = (oln & 15) / G;
  if (om >= n_rows) return;
  const int og4 = oln >> 4;
  const int orow =
      min(max(const_cast<const volatile int*>(tile)[2 + om], 0), B - 1);
  const long wslot =
      ((long)orow * Hq + hk * G + (oln & 15) % G) * Stot + slot;
  float* top = tmp_out + wslot * D;
#pragma unroll
  for (int dc = 0; dc < 8; ++dc) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      top[dc * 16 + 4 * og4 + r] = oacc[dc][r];
    }
  }
  if (og4 == 0) {
    float* ml = tmp_ml + wslot * 2;
    ml[0] = m;
    ml[1] = l_acc;
  }
}

// Merge the S split partials of head (b, h); thread d owns output dim d.
// All S slots are read unconditionally (see the slot rule above) — no
// per-split block math, no zero-ctx division hazard.
//
// SHARED (shared-prefix op): S counts the prefix slots and the suffix slots
// behind them. The prefix kernel writes the prefix slots of tile members
// only, so a row in no tile (prefix_blocks == 0) starts at the first suffix
// slot: no slot is read that this call did not write. An empty slot weighs
// 0 in every expression below, so skipping those changes no bit.
template <int D, bool SHARED = false>
__global__ void paged_attn_reduce_kernel(
    unsigned short* __restrict__ out, const float* __restrict__ tmp_out,
    const float* __restrict__ tmp_ml, const int* __restrict__ seq_lens,
    int Hq, int S, std::conditional_t<SHARED, PrefixArgs, NoPrefix> px) {
  const int b = blockIdx.x;
  const int h = blockIdx.y;
  const int d = threadIdx.x;
  if (seq_lens[b] <= 0) return;
  int s0 = 0;
  if constexpr (SHARED) s0 = px.prefix_blocks[b] > 0 ? 0 : px.prefix_splits;
  const float* ml = tmp_ml + (((long)b * Hq + h) * S) * 2;
  float M = -INFINITY;
  for (int s = s0; s < S; ++s) M = fmaxf(M, ml[s * 2]);
  float L = 0.f;
  for (int s = s0; s < S; ++s)
    L = __builtin_fmaf(merge_weight(ml[s * 2], M), ml[s * 2 + 1], L);
  const float* top = tmp_out + (((long)b * Hq + h) * S) * D;
  float acc = 0.f;
  for (int s = s0; s < S; ++s) {
    const float w = merge_weight(ml[s * 2], M);
    acc = __builtin_fmaf(w, top[(long)s * D + d], acc);
  }
  out[(long)b * Hq * D + (long)h * D + d] = f2us(L > 0.f ? acc / L : 0.f);
}

// out[b] = attention(q[b, q_offset : q_offset + Hq*128], cache blocks of b)
// for b in [0, q.size(0)). With cos_sin / positions (both or neither) q is
// the fused qkv projection [B, (Hq+2*Hk)*128]: q and the new k are rotated
// on the fly and the new k/v rows appended to the caches; qkv itself is
// not written. All checks are on host-side metadata; nothing is allocated.
//
// With `shared` (the *_shared ops) the leading prefix_blocks[b] blocks of a
// row are attended to by the prefix kernel, a tile of sibling rows at a
// time, into workspace slots [0, prefix_splits); this kernel's suffix pass
// walks the rest into the num_splits slots behind them and the reduce
// kernel merges all of them, so the workspaces hold
// B*Hq*(prefix_splits + num_splits) slots. What the caller guarantees about
// the tiles is in ops.paged_attention_shared; none of it is read here.
struct SharedPrefix {
  torch::Tensor prefix_blocks, tiles;
  int64_t prefix_splits;
};

static void decode_attention(torch::Tensor out, torch::Tensor q,
                             torch::Tensor k_cache, torch::Tensor v_cache,
                             const torch::Tensor* cos_sin,
                             const torch::Tensor* positions,
                             torch::Tensor block_table, torch::Tensor seq_lens,
                             int64_t q_offset, int64_t num_splits,
                             double scale, torch::Tensor tmp_out,
                             torch::Tensor tmp_ml,
                             const SharedPrefix* shared = nullptr) {
  const int B = q.size(0);
  if (B == 0) return;
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(2) == 16 &&
                  k_cache.size(3) == 128,
              "kv caches must be [NB, Hk, 16, 128] (block size 16, "
              "head_dim 128)");
  TORCH_CHECK(v_cache.sizes() == k_cache.sizes() &&
                  v_cache.scalar_type() == k_cache.scalar_type() &&
                  k_cache.is_contiguous() && v_cache.is_contiguous(),
              "k_cache and v_cache must be contiguous and alike");
  const bool fp8 = k_cache.scalar_type() == torch::kUInt8;
  TORCH_CHECK(fp8 || k_cache.scalar_type() == torch::kBFloat16,
              "kv caches must be bf16 or uint8 (fp8 e4m3)");
  constexpr int D = 128;
  const int Hk = k_cache.size(1);
  TORCH_CHECK(out.dim() == 2 && out.size(0) == B && out.size(1) % D == 0 &&
                  out.scalar_type() == torch::kBFloat16 && out.is_contiguous(),
              "out must be contiguous bf16 [B, Hq*128]");
  const int Hq = out.size(1) / D;
  TORCH_CHECK(Hq >= Hk && Hq % Hk == 0 && Hq / Hk <= 16,
              "GQA group Hq/Hk must be an integer <= 16, got Hq=", Hq,
              " Hk=", Hk);
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16 && q.dim() == 2 &&
                  q.stride(1) == 1,
              "q must be bf16 [B, >= Hq*128] with unit inner stride");
  // the kernel reads Q with 16-byte loads
  TORCH_CHECK(q.stride(0) % 8 == 0 && q_offset % 8 == 0 && q_offset >= 0 &&
                  q_offset + (int64_t)Hq * D <= q.size(1),
              "q.stride(0) and q_offset must be multiples of 8 and the heads "
              "must fit in a q row, got stride ", q.stride(0), " offset ",
              q_offset);
  TORCH_CHECK(block_table.scalar_type() == torch::kInt32 &&
                  block_table.dim() == 2 && block_table.is_contiguous() &&
                  block_table.size(0) >= B,
              "block_table must be contiguous int32 [>= B, max_blocks]");
  TORCH_CHECK(seq_lens.scalar_type() == torch::kInt32 &&
                  seq_lens.is_contiguous() && seq_lens.numel() >= B,
              "seq_lens must be contiguous int32 [>= B]");
  TORCH_CHECK(num_splits >= 1, "num_splits must be >= 1");
  const int64_t PS = shared ? shared->prefix_splits : 0;
  if (shared) {
    TORCH_CHECK(PS >= 1, "prefix_splits must be >= 1");
    const auto& pb = shared->prefix_blocks;
    const auto& tl = shared->tiles;
    TORCH_CHECK(pb.scalar_type() == torch::kInt32 && pb.is_contiguous() &&
                    pb.dim() == 1 && pb.numel() >= B,
                "prefix_blocks must be contiguous int32 [>= B]");
    TORCH_CHECK(tl.scalar_type() == torch::kInt32 && tl.is_contiguous() &&
                    tl.dim() == 2 && tl.size(1) == kTileCols,
                "tiles must be contiguous int32 [T, 2 + 16]");
    TORCH_CHECK(pb.device() == q.device() && tl.device() == q.device(),
                "all tensors must be on the same GPU");
  }
  const int64_t slots = (int64_t)B * Hq * (PS + num_splits);
  TORCH_CHECK(tmp_out.scalar_type() == torch::kFloat32 &&
                  tmp_out.is_contiguous() && tmp_out.numel() >= slots * D,
              "tmp_out must be contiguous float32 with >= B*Hq*num_splits*128 "
              "elements, got ", tmp_out.numel(), " need ", slots * D);
  TORCH_CHECK(tmp_ml.scalar_type() == torch::kFloat32 &&
                  tmp_ml.is_contiguous() && tmp_ml.numel() >= slots * 2,
              "tmp_ml must be contiguous float32 with >= B*Hq*num_splits*2 "
              "elements, got ", tmp_ml.numel(), " need ", slots * 2);
  for (const auto& t : {out, k_cache, v_cache, block_table, seq_lens, tmp_out,
                        tmp_ml})
    TORCH_CHECK(t.device() == q.device() && t.is_cuda(),
                "all tensors must be on the same GPU");

  const bool rope = cos_sin != nullptr;
  const float* csp = nullptr;
  const int* posp = nullptr;
  if (rope) {
    TORCH_CHECK(q_offset == 0 && q.is_contiguous() &&
                    q.size(1) == (int64_t)(Hq + 2 * Hk) * D,
                "qkv must be contiguous bf16 [B, (Hq+2*Hk)*128]");
    TORCH_CHECK(cos_sin->scalar_type() == torch::kFloat32 &&
                    cos_sin->dim() == 2 && cos_sin->size(1) == D &&
                    cos_sin->is_contiguous(),
                "cos_sin must be contiguous float32 [max_pos, 128]");
    TORCH_CHECK(positions->scalar_type() == torch::kInt32 &&
                    positions->is_contiguous() && positions->numel() >= B,
                "positions must be contiguous int32 [>= B]");
    for (const auto* t : {cos_sin, positions})
      TORCH_CHECK(t->device() == q.device(),
                  "all tensors must be on the same GPU");
    csp = cos_sin->data_ptr<float>();
    posp = positions->data_ptr<int>();
  }

  // Launch plan: all S slots of a (sequence, kv head) in one workgroup of
  // 4 or 8 waves when they fit — that workgroup merges them itself — else
  // 4-wave workgroups into the workspaces plus the reduce kernel.
  const int S = (int)num_splits;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const unsigned short* qp =
      reinterpret_cast<const unsigned short*>(q.data_ptr()) + q_offset;
  if (shared) {
    // prefix kernel -> suffix pass -> reduce, all through the workspaces
    const int T = shared->tiles.size(0);
    const int Stot = (int)PS + S;
    const PrefixArgs px{shared->prefix_blocks.data_ptr<int>(), (int)PS};
    if (T > 0) {
      auto* prefix = fp8 ? (rope ? paged_attn_prefix_kernel<true, true>
                                 : paged_attn_prefix_kernel<true, false>)
                         : (rope ? paged_attn_prefix_kernel<false, true>
                                 : paged_attn_prefix_kernel<false, false>);
      prefix<<<dim3(T, Hk, (unsigned)((PS + 3) / 4)), 4 * WAVE, 4 * kWaveLds,
               stream>>>(
          tmp_out.data_ptr<float>(), tmp_ml.data_ptr<float>(), qp,
          k_cache.data_ptr(), v_cache.data_ptr(), csp, posp,
          block_table.data_ptr<int>(), shared->tiles.data_ptr<int>(),
          q.stride(0), B, Hq, Hk, (int)block_table.size(1), (int)PS, Stot,
          (float)scale);
      HIP_CHECK_KERNEL();
    }
    auto* suffix = fp8 ? (rope ? paged_attn_kernel<true, true, true>
                               : paged_attn_kernel<true, false, true>)
                       : (rope ? paged_attn_kernel<false, true, true>
                               : paged_attn_kernel<false, false, true>);
    suffix<<<dim3(B, Hk, (unsigned)((S + 3) / 4)), 4 * WAVE, 4 * kWaveLds,
             stream>>>(
        reinterpret_cast<unsigned short*>(out.data_ptr()),
        tmp_out.data_ptr<float>(), tmp_ml.data_ptr<float>(), qp,
        k_cache.data_ptr(), v_cache.data_ptr(), csp, posp,
        block_table.data_ptr<int>(), seq_lens.data_ptr<int>(), q.stride(0), Hq,
        Hk, (int)block_table.size(1), S, 0, (float)scale, px);
    HIP_CHECK_KERNEL();
    paged_attn_reduce_kernel<128, true><<<dim3(B, Hq), 128, 0, stream>>>(
        reinterpret_cast<unsigned short*>(out.data_ptr()),
        tmp_out.data_ptr<float>(), tmp_ml.data_ptr<float>(),
        seq_lens.data_ptr<int>(), Hq, Stot, px);
    HIP_CHECK_KERNEL();
    return;
  }
  const bool merge = S <= 8;
  const int waves = merge && S > 4 ? 8 : 4;
  auto* launch = fp8 ? (rope ? paged_attn_kernel<true, true>
                             : paged_attn_kernel<true, false>)
                     : (rope ? paged_attn_kernel<false, true>
                             : paged_attn_kernel<false, false>);
  launch<<<dim3(B, Hk, (unsigned)((S + waves - 1) / waves)), waves * WAVE,
           waves * kWaveLds, stream>>>(
      reinterpret_cast<unsigned short*>(out.data_ptr()),
      tmp_out.data_ptr<float>(), tmp_ml.data_ptr<float>(), qp,
      k_cache.data_ptr(), v_cache.data_ptr(), csp, posp,
      block_table.data_ptr<int>(), seq_lens.data_ptr<int>(), q.stride(0), Hq,
      Hk, (int)block_table.size(1), S, (int)merge, (float)scale, NoPrefix{});
  HIP_CHECK_KERNEL();
  if (merge) return;
  paged_attn_reduce_kernel<128><<<dim3(B, Hq), 128, 0, stream>>>(
      reinterpret_cast<unsigned short*>(out.data_ptr()),
      tmp_out.data_ptr<float>(), tmp_ml.data_ptr<float>(),
      seq_lens.data_ptr<int>(), Hq, S, NoPrefix{});
  HIP_CHECK_KERNEL();
}

void paged_attention(torch::Tensor out, torch::Tensor q, torch::Tensor k_cache,
                     torch::Tensor v_cache, torch::Tensor block_table,
                     torch::Tensor seq_lens, int64_t q_offset,
                     int64_t num_splits, double scale, torch::Tensor tmp_out,
                     torch::Tensor tmp_ml) {
  decode_attention(out, q, k_cache, v_cache, nullptr, nullptr, block_table,
                   seq_lens, q_offset, num_splits, scale, tmp_out, tmp_ml);
}

// rope_kv_append (table mode) + paged_attention in one pass over one decode
// token per row of the fused qkv projection; see the header comment.
void paged_attention_rope(torch::Tensor out, torch::Tensor qkv,
                          torch::Tensor k_cache, torch::Tensor v_cache,
                          torch::Tensor cos_sin, torch::Tensor positions,
                          torch::Tensor block_table, torch::Tensor seq_lens,
                          int64_t num_q_heads, int64_t num_kv_heads,
                          int64_t num_splits, double scale,
                          torch::Tensor tmp_out, torch::Tensor tmp_ml) {
  TORCH_CHECK(out.dim() == 2 && out.size(1) == num_q_heads * 128 &&
                  k_cache.dim() == 4 && k_cache.size(1) == num_kv_heads,
              "out must be [B, num_q_heads*128] and the caches "
              "[NB, num_kv_heads, 16, 128]");
  decode_attention(out, qkv, k_cache, v_cache, &cos_sin, &positions,
                   block_table, seq_lens, 0, num_splits, scale, tmp_out,
                   tmp_ml);
}

// paged_attention / paged_attention_rope with the leading blocks that
// sibling rows share attended to once per tile of rows.
void paged_attention_shared(torch::Tensor out, torch::Tensor q,
                            torch::Tensor k_cache, torch::Tensor v_cache,
                            torch::Tensor block_table, torch::Tensor seq_lens,
                            int64_t q_offset, int64_t num_splits, double scale,
                            torch::Tensor tmp_out, torch::Tensor tmp_ml,
                            torch::Tensor prefix_blocks, torch::Tensor tiles,
                            int64_t prefix_splits) {
  const SharedPrefix sp{prefix_blocks, tiles, prefix_splits};
  decode_attention(out, q, k_cache, v_cache, nullptr, nullptr, block_table,
                   seq_lens, q_offset, num_splits, scale, tmp_out, tmp_ml,
                   &sp);
}

void paged_attention_rope_shared(
    torch::Tensor out, torch::Tensor qkv, torch::Tensor k_cache,
    torch::Tensor v_cache, torch::Tensor cos_sin, torch::Tensor positions,
    torch::Tensor block_table, torch::Tensor seq_lens, int64_t num_q_heads,
    int64_t num_kv_heads, int64_t num_splits, double scale,
    torch::Tensor tmp_out, torch::Tensor tmp_ml, torch::Tensor prefix_blocks,
    torch::Tensor tiles, int64_t prefix_splits) {
  TORCH_CHECK(out.dim() == 2 && out.size(1) == num_q_heads * 128 &&
                  k_cache.dim() == 4 && k_cache.size(1) == num_kv_heads,
              "out must be [B, num_q_heads*128] and the caches "
              "[NB, num_kv_heads, 16, 128]");
  const SharedPrefix sp{prefix_blocks, tiles, prefix_splits};
  decode_attention(out, qkv, k_cache, v_cache, &cos_sin, &positions,
                   block_table, seq_lens, 0, num_splits, scale, tmp_out,
                   tmp_ml, &sp);
}

}  // namespace kukeon
