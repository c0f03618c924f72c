// Paged decode attention for gfx950 (MI355X): one query token per
// sequence against a paged KV cache, split-KV (flash-decode) on the matrix
// cores. One attention kernel plus one reduce, always run as a pair.
//
// paged_attn_kernel — grid (B, Hk, ceil(S/4)), 4 waves per workgroup.
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
//     - 8 KiB LDS per wave (32 KiB per workgroup), no barriers.
//
// Split slots. The KV blocks of a sequence are cut into S contiguous
//   ranges ("slots") of ceil(nblocks/S) blocks; a slot past the end has an
//   empty range. The 4 waves of a workgroup are fully autonomous: wave w
//   of workgroup z owns slot 4*z + w, walks that range alone and writes
//   its unnormalized O (f32) and (m, l) into tmp_out / tmp_ml at that
//   slot. Waves whose slot is >= S do nothing. Every slot < S is written
//   on every call (an empty range writes O = 0, m = -inf, l = 0), which is
//   what lets the reduce read all S slots unconditionally.
//
// paged_attn_reduce_kernel — grid (B, Hq), 128 threads: merges the S
//   partials of one head and writes the bf16 output row.
//
// A row with seq_len <= 0 is skipped by both kernels: its `out` row (and
//   its workspace slots) are left untouched.
//
// Two designs were measured against this one and removed; their code is in
// this commit's parent. A v_dot2 kernel (workgroup per split, K/V staged in
// LDS, packed-bf16 dot products) was issue-stall bound — ~28 dependent VALU
// instructions per KV token, 3.8-4.1 TB/s against 4.9-5.4 here. A 32-token
// 32x32x16 MFMA tile was LDS-residency bound — 64 KiB per workgroup caps a
// CU at 2 workgroups, 25-30% behind end to end.
#include "attn_frag.h"
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

namespace kukeon {

template <bool FP8>
// fp8 needs headroom for the cvt_pk conversions (at 4 waves/SIMD the
// 128-reg bound put a 2-VGPR spill in the hot loop)
__global__ __launch_bounds__(256, FP8 ? 3 : 4) void paged_attn_kernel(
    float* __restrict__ tmp_out,          // [B, Hq, S, D] f32
    float* __restrict__ tmp_ml,           // [B, Hq, S, 2]
    const unsigned short* __restrict__ q, // [B, q_stride]
    const void* __restrict__ k_cache,     // [NB, Hk, 16, D]
    const void* __restrict__ v_cache,
    const int* __restrict__ block_table,  // [B, max_blocks]
    const int* __restrict__ seq_lens,     // [B]
    long q_stride, int Hq, int Hk, int max_blocks, int S, float scale) {
  constexpr int D = 128;
  constexpr int BS = 16;
  const int b = blockIdx.x;
  const int hk = blockIdx.y;
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int g4 = lane >> 4;       // 0..3
  const int rc = lane & 15;
  const int G = Hq / Hk;
  const int slot = blockIdx.z * 4 + wid;
  const int ctx = seq_lens[b];
  if (ctx <= 0 || slot >= S) return;

  // V^T images only — K is consumed straight from HBM in fragment shape
  // (16 B/lane across 64 B-line groups; the LDS round trip was pure
  // added latency here: per-wave parked time was 67% of cycles). Two
  // V^T buffers per wave: tile bi's image is written during tile bi-1,
  // so PV never waits on fresh LDS stores.
  __shared__ __align__(16) unsigned short vtbuf[4][2][D * BS];

  const int nblocks = (ctx + BS - 1) / BS;
  const int per_slot = (nblocks + S - 1) / S;
  const int blk_begin = slot * per_slot;
  const int blk_end = min(nblocks, blk_begin + per_slot);
  const int kv_hi = min(ctx, blk_end * BS);

  const int qh = min(rc, G - 1);  // B col = q head
  // Q fragments pinned in 16 registers (L2 re-reads in the tile loop
  // measured as 4 dependent ~250-cycle stalls per tile)
  unsigned int qf[4][4];
  {
    const unsigned short* qp =
        q + (long)b * q_stride + (long)(hk * G + qh) * D;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const uint4 v = *reinterpret_cast<const uint4*>(qp + st * 32 + g4 * 8);
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
    vwrite(vtbuf[wid][blk_begin & 1], blk_begin * BS);
  }

  for (int bi = blk_begin; bi < blk_end; ++bi) {
    const int kvbase = bi * BS;
    const unsigned short* vt = vtbuf[wid][bi & 1];

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
      vwrite(vtbuf[wid][(bi + 1) & 1], (bi + 1) * BS);
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

  // ---- epilogue: unnormalized O + (m, l) into this wave's slot ----
  if (rc >= G) return;
  const int head = hk * G + rc;
  float* top = tmp_out + (((long)b * Hq + head) * S + slot) * D;
#pragma unroll
  for (int dc = 0; dc < 8; ++dc) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      top[dc * 16 + 4 * g4 + r] = oacc[dc][r];
    }
  }
  if (g4 == 0) {
    float* ml = tmp_ml + (((long)b * Hq + head) * S + slot) * 2;
    ml[0] = m;
    ml[1] = l_acc;
  }
}

// Merge the S split partials of head (b, h); thread d owns output dim d.
// All S slots are read unconditionally (see the slot rule above) — no
// per-split block math, no zero-ctx division hazard.
template <int D>
__global__ void paged_attn_reduce_kernel(
    unsigned short* __restrict__ out, const float* __restrict__ tmp_out,
    const float* __restrict__ tmp_ml, const int* __restrict__ seq_lens,
    int Hq, int S) {
  const int b = blockIdx.x;
  const int h = blockIdx.y;
  const int d = threadIdx.x;
  if (seq_lens[b] <= 0) return;
  const float* ml = tmp_ml + (((long)b * Hq + h) * S) * 2;
  float M = -INFINITY;
  for (int s = 0; s < S; ++s) M = fmaxf(M, ml[s * 2]);
  float L = 0.f;
  for (int s = 0; s < S; ++s)
    L += (ml[s * 2] == -INFINITY ? 0.f : __expf(ml[s * 2] - M)) *
         ml[s * 2 + 1];
  const float* top = tmp_out + (((long)b * Hq + h) * S) * D;
  float acc = 0.f;
  for (int s = 0; s < S; ++s) {
    const float w = ml[s * 2] == -INFINITY ? 0.f : __expf(ml[s * 2] - M);
    acc += w * top[(long)s * D + d];
  }
  out[(long)b * Hq * D + (long)h * D + d] = f2us(L > 0.f ? acc / L : 0.f);
}

// out[b] = attention(q[b, q_offset : q_offset + Hq*128], cache blocks of b)
// for b in [0, q.size(0)). All checks are on host-side metadata.
void paged_attention(torch::Tensor out, torch::Tensor q, torch::Tensor k_cache,
                     torch::Tensor v_cache, torch::Tensor block_table,
                     torch::Tensor seq_lens, int64_t q_offset,
                     int64_t num_splits, double scale, torch::Tensor tmp_out,
                     torch::Tensor tmp_ml) {
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
  const int64_t slots = (int64_t)B * Hq * num_splits;
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

  auto stream = c10::hip::getCurrentHIPStream().stream();
  const unsigned short* qp =
      reinterpret_cast<const unsigned short*>(q.data_ptr()) + q_offset;
  auto* launch = fp8 ? paged_attn_kernel<true> : paged_attn_kernel<false>;
  launch<<<dim3(B, Hk, (unsigned)((num_splits + 3) / 4)), 256, 0, stream>>>(
      tmp_out.data_ptr<float>(), tmp_ml.data_ptr<float>(), qp,
      k_cache.data_ptr(), v_cache.data_ptr(), block_table.data_ptr<int>(),
      seq_lens.data_ptr<int>(), q.stride(0), Hq, Hk,
      (int)block_table.size(1), (int)num_splits, (float)scale);
  HIP_CHECK_KERNEL();
  paged_attn_reduce_kernel<128><<<dim3(B, Hq), 128, 0, stream>>>(
      reinterpret_cast<unsigned short*>(out.data_ptr()),
      tmp_out.data_ptr<float>(), tmp_ml.data_ptr<float>(),
      seq_lens.data_ptr<int>(), Hq, (int)num_splits);
  HIP_CHECK_KERNEL();
}

}  // namespace kukeon
