// Skinny decode GEMM for gfx950: out[M,N] = x[M,K] @ W[N,K]^T, M <= 64.
//
// Decode is weight-bandwidth-bound (the whole W streams through HBM once
// per step). Design (ledger: profiles/r01_progress.md):
//   * x (tiny, L2-resident) is staged into per-slice LDS images by async
//     LDS-DMA (glds), double-buffered so slice s+1's stage flies under
//     slice s's W stream (XOR-swizzled, conflict-free ds_read_b128
//     B-fragments that consume no vmcnt slots),
//   * W streams with nt 16B/lane loads in 8-deep probe-shaped batches
//     (loads + consume in one iteration => hipcc emits counted vmcnt(N)),
//     batch 0 issued BEFORE the drain+barrier so the prologue overlaps,
//   * split-K over 256-deep slices, sized to ~256 blocks (chip fill);
//     partials combine through per-slice f32 slabs + a reduce pass
//     (atomicAdd measured ~35us of L2 RMW serialization), or fused
//     straight into the residual-add+RMSNorm epilogue on the decode
//     o-projection path.
// Grid: (N/64, splitk); block = 4 waves, wave w owns N rows [64b+16w, +16)
// of every slice the block walks. Dispatched per shape where it beats
// hipBLASLt cold-LLC (ops/__init__.py _skinny_kind).
//
// Layout of this file: the kernels first — v1 (above; o-projection), the
// two split-K epilogues, v2 (G-tile walk, hand-counted waits), v5
// (full-line W stream; down-projection), v6 (barrier-free), W8A16
// (fp8 weight bytes, per-row scales) and W4A16 (MXFP4 codes, per-block
// scales); v2, v6 and v5's silu path are tested negative results. The
// host side sits at the end: one split-K plan (skinny_plan, exported to Python as
// skinny_splitk so the workspace is sized by the same formula), one
// launcher skeleton (run_reduce / run_reduce_add_rmsnorm), and one short
// entry point per variant.
#include "common.h"
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <string>
#include <type_traits>

namespace kukeon {

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8_t;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4_t;
typedef __attribute__((__vector_size__(4 * sizeof(unsigned int)))) unsigned int u32x4_t;

DEV_INLINE bf16x8_t frag_of(u32x4_t v) {
  return __builtin_bit_cast(bf16x8_t, v);
}
struct uint4_s { unsigned int x[4]; };
DEV_INLINE bf16x8_t frag_of(uint4 v) {
  uint4_s u{{v.x, v.y, v.z, v.w}};
  return __builtin_bit_cast(bf16x8_t, u);
}
DEV_INLINE u32x4_t nt_load16(const void* p) {
  return __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
}

constexpr int KSLICE = 256;
constexpr int U = 8;  // W k-chunks (of 32) per batch; 1 batch per slice
// KSLICE 512 -> 256: with 512-wide slices the two x buffers took 128 KiB
// of LDS = 1 workgroup/CU = ONE wave per SIMD, and PMC showed the waves
// parked on memory 74% of their cycles with nothing to hide behind.
// 256-wide slices halve the LDS (2 workgroups/CU, 2 waves/SIMD) at the
// cost of twice the slice turnarounds.

DEV_INLINE int xswz(int row, int byte_in_row) {
  return row * (KSLICE * 2) + (byte_in_row ^ ((row & 15) << 4));
}

// ---- async global->LDS staging (gfx950 LDS-DMA) ----
// One instruction stages 64 lanes x 16 B = 1 KiB to a WAVE-UNIFORM LDS
// base + lane*16 (lane-linear dest — guide §5.4 rule 21); the swizzle
// therefore goes on the per-lane SOURCE address. Raw asm, not the
// builtin: hipcc tracks the builtin in its s_waitcnt bookkeeping and
// demotes every later counted vmcnt(N) to vmcnt(0) while one is in
// flight, which would serialize the W-stream pipeline this staging is
// meant to hide under. m0 (the LDS-DMA destination base) is saved and
// restored in the same statement (it is compiler-reserved).
DEV_INLINE void glds16(const unsigned short* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_dst)
      : "memory");
}

DEV_INLINE unsigned lds_addr_of(const void* p) {
  // LDS aperture is 2^32-aligned: the low 32 bits of a generic pointer
  // into LDS are the LDS byte address m0/LDS-DMA expects (validated by
  // glds_probe_kernel below against a read-back).
  return (unsigned)(unsigned long long)p;
}

// Stage rows [0,64) x KSLICE cols of x into the xswz LDS image with 8
// asm glds per wave (each 1 KiB instruction covers two 512-B rows) (wave w owns rows 16w..16w+15). Completion rides the
// VM counter; callers drain with s_waitcnt vmcnt + barrier. For tail
// slices (klen < KSLICE) the per-lane source byte offset is clamped
// in-bounds — the over-staged slots hold junk the consumer never reads
// (it bounds every read by klen).
DEV_INLINE void glds_stage_x(unsigned short* xbuf,
                             const unsigned short* __restrict__ x, long K,
                             long ks, int klen, int M, int wid, int lane) {
  const int cap = klen * 2 - 16;  // klen%32==0 -> 16B-aligned
  // one glds stages 1 KiB = TWO 512-B rows: lanes 0-31 cover the even
  // row, 32-63 the odd row (dest stays lane-linear)
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = wid * 16 + 2 * i + (lane >> 5);
    const int byte_in_row = min(((lane & 31) * 16) ^ ((row & 15) << 4), cap);
    const unsigned short* g =
        x + (long)min(M - 1, row) * K + ks + byte_in_row / 2;
    glds16(g, __builtin_amdgcn_readfirstlane(
                  lds_addr_of(xbuf + (row & ~1) * KSLICE)));
  }
}

// Round-trip validator for the asm path: stage via glds_stage_x, read
// back through the same xswz addresses, store linear. out must equal src.
__global__ __launch_bounds__(256) void glds_probe_kernel(
    unsigned short* __restrict__ out, const unsigned short* __restrict__ src) {
  __shared__ __align__(16) unsigned short xbuf[64 * KSLICE];
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  glds_stage_x(xbuf, src, KSLICE, 0, KSLICE, 64, wid, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const int xr = threadIdx.x >> 2;
  const int c0 = (threadIdx.x & 3) * 8;
#pragma unroll
  for (int i = 0; i < KSLICE / 32; ++i) {
    const int c = c0 + i * 32;
    const uint4 v = *reinterpret_cast<const uint4*>(
        reinterpret_cast<const char*>(xbuf) + xswz(xr, c * 2));
    *reinterpret_cast<uint4*>(out + (long)xr * KSLICE + c) = v;
  }
}

void glds_probe(torch::Tensor out, torch::Tensor src) {
  TORCH_CHECK(src.size(0) == 64 && src.size(1) == KSLICE &&
              src.is_contiguous() && out.is_contiguous());
  auto stream = c10::hip::getCurrentHIPStream().stream();
  glds_probe_kernel<<<dim3(1), 256, 0, stream>>>(
      reinterpret_cast<unsigned short*>(out.data_ptr()),
      reinterpret_cast<const unsigned short*>(src.data_ptr()));
  HIP_CHECK_KERNEL();
}

// MT = number of 16-row M subtiles (1 => M<=16, 4 => M<=64)
template <int MT, bool SPLIT>
__global__ __launch_bounds__(256) void skinny_gemm_kernel(
    unsigned short* __restrict__ out,      // [M, N] bf16 (SPLIT=false)
    float* __restrict__ ws,                // [M, N] f32  (SPLIT=true)
    const unsigned short* __restrict__ x,  // [M, K]
    const unsigned short* __restrict__ w,  // [N, K]
    int M, int N, long K) {
  // Two x buffers (128 KiB LDS, 1 block/CU): slice s+1's x is staged by
  // async LDS-DMA (glds_stage_x) issued at the END of slice s, so the
  // 64 KiB L2 read flies under slice s's tail + slice s+1's W prologue
  // instead of serializing all four waves behind a load+ds_write pass
  // between two barriers (that serial stage was ~half the kernel's time
  // on multi-slice shapes: gate_up measured 73us vs its 37us HBM floor).
  __shared__ __align__(16) unsigned short xbuf[2][64 * KSLICE];
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int n0 = blockIdx.x * 64 + wid * 16;     // this wave's 16 N rows
  const int row16 = lane & 15;                   // A row / B col
  const int kgrp = lane >> 4;                    // 0..3 -> k = 8*kgrp + j
  f32x4_t acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // a block walks slices {blockIdx.y, +gridDim.y, ...} and accumulates
  // locally, so grid.y is an occupancy choice, not forced to K/512
  const long kstride = (long)gridDim.y * KSLICE;
  const long ks0 = (long)blockIdx.y * KSLICE;
  if (ks0 < K) {
    glds_stage_x(xbuf[0], x, K, ks0, (int)min((long)KSLICE, K - ks0), M,
                 wid, lane);
  }
  int cur = 0;
  for (long ks = ks0; ks < K; ks += kstride, cur ^= 1) {
  const int klen = (int)min((long)KSLICE, K - ks);
  const unsigned short* wrow = w + (long)(n0 + row16) * K + ks + 8 * kgrp;
  const int nfull = klen / (U * 32);
  const unsigned short* xb = xbuf[cur];

  // this slice's first W batch goes in flight BEFORE the drain+barrier
  // (no LDS dependence), so its HBM latency hides under them
  u32x4_t wa0[U];
  if (nfull >= 1) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      wa0[u] = nt_load16(wrow + u * 32);
    // retire this buffer's 16 glds (older than the 8 wa0 just issued;
    // hipcc cannot count the asm DMAs, so the wait is explicit)
    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();

  // Batch 0 consumes the pre-staged wa0; later batches keep loads and
  // consume in the SAME iteration with no explicit double-buffer: hipcc
  // then emits counted vmcnt(N) per u so each load's latency hides under
  // the consumption of earlier ones (the explicit next-batch prefetch
  // variant got hoisted to the loop bottom and drained with one vmcnt(0)
  // at the top — nothing overlapped; 45us vs 13us on the
  // ingredient-identical pattern probe). No runtime condition inside the
  // unrolled body either (guide §5 ".s-level traps" (c)).
  if (nfull >= 1) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kc = u * 32 + 8 * kgrp;
      const bf16x8_t afrag = frag_of(wa0[u]);
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int xr = m * 16 + row16;
        const uint4 xv = *reinterpret_cast<const uint4*>(
            reinterpret_cast<const char*>(xb) + xswz(xr, kc * 2));
        acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            afrag, frag_of(xv), acc[m], 0, 0, 0);
      }
    }
  }
  for (int b = 1; b < nfull; ++b) {
    u32x4_t wa[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      wa[u] = nt_load16(wrow + b * U * 32 + u * 32);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kc = b * U * 32 + u * 32 + 8 * kgrp;
      const bf16x8_t afrag = frag_of(wa[u]);
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const int xr = m * 16 + row16;
        const uint4 xv = *reinterpret_cast<const uint4*>(
            reinterpret_cast<const char*>(xb) + xswz(xr, kc * 2));
        acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            afrag, frag_of(xv), acc[m], 0, 0, 0);
      }
    }
  }
  // tail chunks (klen not a multiple of U*32), one chunk at a time
  for (int kc0 = nfull * U * 32; kc0 < klen; kc0 += 32) {
    const bf16x8_t afrag = frag_of(nt_load16(wrow + kc0));
    const int kc = kc0 + 8 * kgrp;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int xr = m * 16 + row16;
      const uint4 xv = *reinterpret_cast<const uint4*>(
          reinterpret_cast<const char*>(xb) + xswz(xr, kc * 2));
      acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          afrag, frag_of(xv), acc[m], 0, 0, 0);
    }
  }
  // async-stage the NEXT slice's x into the other buffer: issued after
  // every W wait of this slice, so nothing forces these DMAs to retire
  // before the next iteration's explicit vmcnt(8) — they fly under the
  // loop turnaround and the next slice's wa0 prologue. Safe without a
  // barrier: every wave finished READING that buffer before it crossed
  // this slice's top barrier.
  {
    const long ksn = ks + kstride;
    if (ksn < K) {
      glds_stage_x(xbuf[cur ^ 1], x, K, ksn,
                   (int)min((long)KSLICE, K - ksn), M, wid, lane);
    }
  }
  }  // slice loop

  // C layout (16x16): lane -> col = lane&15 (the M index here),
  // row = 4*(lane>>4) + r (the N index). Split-K partials go to plain
  // per-slice slabs (atomicAdd here measured ~35us of L2 RMW serialization
  // on the 3M-element qkv epilogue; slabs + a reduce pass are ~4us).
  const int ncol = n0 + 4 * kgrp;
  float* slab = SPLIT ? ws + (long)blockIdx.y * M * N : nullptr;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int mrow = m * 16 + row16;
    if (mrow >= M) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long off = (long)mrow * N + ncol + r;
      if (SPLIT) {
        slab[off] = acc[m][r];
      } else {
        out[off] = f2us(acc[m][r]);
      }
    }
  }
}

// reduce the split-K slabs and cast to bf16
__global__ void skinny_reduce_kernel(unsigned short* __restrict__ out,
                                     const float* __restrict__ ws, long n,
                                     int splitk) {
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (i + 7 < n) {
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int s = 0; s < splitk; ++s) {
      const float4 a = *reinterpret_cast<const float4*>(ws + s * n + i);
      const float4 b = *reinterpret_cast<const float4*>(ws + s * n + i + 4);
      v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w;
      v[4] += b.x; v[5] += b.y; v[6] += b.z; v[7] += b.w;
    }
    *reinterpret_cast<uint4*>(out + i) = pack_bf16x8(v);
  } else {
    for (long j = i; j < n; ++j) {
      float acc = 0.f;
      for (int s = 0; s < splitk; ++s) acc += ws[s * n + j];
      out[j] = f2us(acc);
    }
  }
}

// Split-K reduce fused with residual-add + RMSNorm: the decode o-proj's
// epilogue pair (skinny_reduce 5.0us + fused_add_rmsnorm 5.4us) was two
// launches at the ~4.5us in-graph dispatch floor each for <1us of real
// work. One block per row: sum the slabs, update the residual in place,
// one block-reduce for the mean square, write the normed activations.
__global__ __launch_bounds__(256) void skinny_reduce_add_rmsnorm_kernel(
    unsigned short* __restrict__ normed,    // [M, N] bf16
    unsigned short* __restrict__ residual,  // [M, N] bf16, updated
    const float* __restrict__ ws,           // [splitk, M, N] f32
    const unsigned short* __restrict__ nw,  // [N]
    int N, long total, int splitk, float eps) {
  const int t = blockIdx.x;
  __shared__ float red[16];
  float vals[32];  // up to N = 8192 at 256 threads x 8 elems
  const int nchunk = N / (256 * 8);
  float sq = 0.f;
  for (int c = 0; c < nchunk; ++c) {
    const int n0 = (c * 256 + threadIdx.x) * 8;
    const long off = (long)t * N + n0;
    const bf16x8 r = load_bf16x8(residual + off);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = r.f(j);
    for (int s = 0; s < splitk; ++s) {
      const float4 a =
          *reinterpret_cast<const float4*>(ws + (long)s * total + off);
      const float4 b =
          *reinterpret_cast<const float4*>(ws + (long)s * total + off + 4);
      acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w;
      acc[4] += b.x; acc[5] += b.y; acc[6] += b.z; acc[7] += b.w;
    }
    *reinterpret_cast<uint4*>(residual + off) = pack_bf16x8(acc);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // norm of the bf16-rounded residual, matching the two-kernel path
      const float v = us2f(f2us(acc[j]));
      vals[c * 8 + j] = v;
      sq += v * v;
    }
  }
  sq = block_reduce(sq, red, SumOp{}, 0.f);
  const float rs = __frsqrt_rn(sq / N + eps);
  for (int c = 0; c < nchunk; ++c) {
    const int n0 = (c * 256 + threadIdx.x) * 8;
    const bf16x8 wv = load_bf16x8(nw + n0);
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = vals[c * 8 + j] * rs * wv.f(j);
    *reinterpret_cast<uint4*>(normed + (long)t * N + n0) = pack_bf16x8(o);
  }
}

// ===========================================================================
// skinny GEMM v2 — G-tile walk with hand-counted W stream (round 2).
//
// v1's duty-cycle hole (ledger): the per-slice x re-stage was issued at the
// END of slice s and drained at the TOP of slice s+1, so every slice paid
// ~1.3-1.5k cycles of LDS-DMA landing latency in the open; and the W stream
// was capped at 8 loads in flight per wave with a full drain per slice.
// v2 restructures around a constant-count VMEM pipeline (all W loads are
// inline-asm, invisible to hipcc, so its own counted waits can never
// over-wait on the staging DMAs — guide §5 ".s-level traps" (b)):
//   * each block owns G=2 N-tiles of 64 rows and walks K slices, so one
//     16-glds x stage serves 2x the W stream, and the stage for slice s+1
//     is issued at the TOP of slice s — its landing deadline is the end of
//     the slice, giving it the full 2-tile consume (~2k cycles) as cover;
//   * W chunks carry hand-counted s_waitcnt vmcnt(K) per consume with the
//     glds depth folded into the constants, so nothing ever drains early;
//   * tile0's loads for slice s+1 are issued mid-slice-s (between the two
//     consumes), keeping 8+ W loads in flight across the barrier — the
//     stream never goes dry at a slice boundary.
// Requires K%256==0, N%128==0 (all decode shapes qualify).
// ===========================================================================

DEV_INLINE void issue_w8(u32x4_t (&reg)[8], const unsigned short* p) {
  // 8 nt 16B loads at 64 B stride (one 256-k slice of one W row per lane
  // group); hipcc does not count these — waits are hand-placed.
#define SK2_LD(u, off)                                                    \
  asm volatile("global_load_dwordx4 %0, %1, off offset:" #off " nt"      \
               : "=&v"(reg[u]) : "v"(p) : "memory")
  SK2_LD(0, 0);   SK2_LD(1, 64);  SK2_LD(2, 128); SK2_LD(3, 192);
  SK2_LD(4, 256); SK2_LD(5, 320); SK2_LD(6, 384); SK2_LD(7, 448);
#undef SK2_LD
}

// consume one tile's 8 W chunks: BASE = VMEM ops younger than chunk 7 at
// its wait (so chunk u waits vmcnt(BASE + 7 - u)).
template <int MT, int BASE>
DEV_INLINE void consume8(u32x4_t (&wreg)[8], const unsigned short* xb,
                         f32x4_t (&acc)[MT], int row16, int kgrp) {
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    asm volatile("s_waitcnt vmcnt(%c1)"
                 : "+v"(wreg[u]) : "i"(BASE + 7 - u));
    const bf16x8_t af = frag_of(wreg[u]);
    const int kc = u * 32 + 8 * kgrp;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int xr = m * 16 + row16;
      const uint4 xv = *reinterpret_cast<const uint4*>(
          reinterpret_cast<const char*>(xb) + xswz(xr, kc * 2));
      acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          af, frag_of(xv), acc[m], 0, 0, 0);
    }
  }
}

template <int MT, bool SPLIT>
__global__ __launch_bounds__(256) void skinny2_kernel(
    unsigned short* __restrict__ out,      // [M, N] bf16 (SPLIT=false)
    float* __restrict__ ws,                // [splitk, M, N] f32 (SPLIT)
    const unsigned short* __restrict__ x,  // [M, K]
    const unsigned short* __restrict__ w,  // [N, K]
    int M, int N, long K) {
  __shared__ __align__(16) unsigned short xbuf[2][64 * KSLICE];
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int row16 = lane & 15;
  const int kgrp = lane >> 4;
  const int n0t0 = (blockIdx.x * 2 + 0) * 64 + wid * 16;
  const int n0t1 = (blockIdx.x * 2 + 1) * 64 + wid * 16;
  f32x4_t acc0[MT], acc1[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    acc0[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    acc1[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  const long kadv = (long)gridDim.y * KSLICE;   // strided slice walk
  const long ks0 = (long)blockIdx.y * KSLICE;
  if (ks0 >= K) return;
  u32x4_t w0[8], w1[8];
  const unsigned short* p0 = w + (long)(n0t0 + row16) * K + ks0 + 8 * kgrp;
  const unsigned short* p1 = w + (long)(n0t1 + row16) * K + ks0 + 8 * kgrp;

  // Stream discipline (v3, measured): draining the W stream to zero at
  // a slice boundary costs the full LADEN memory latency (~2-4us under
  // load) per slice — the ablation showed the consume path is entirely
  // hidden and the drain dominates. So 16 W loads stay in flight across
  // every barrier, and the only forced retirement is the x-stage DMA
  // (vmcnt(16) at the slice top). Issue order inside a slice mirrors the
  // validated v1 pattern: glds mid-slice, then the next slice's W loads
  // (crossing loads YOUNGER than the DMA — the reverse order faulted).
  // prologue order = the loop's invariant order: glds oldest, then the
  // two W tile sets — the loop-top vmcnt(16) retires exactly the glds
  // while the 16 W loads keep flying
  glds_stage_x(xbuf[0], x, K, ks0, KSLICE, M, wid, lane);
  issue_w8(w0, p0);
  issue_w8(w1, p1);
  int cur = 0;
  for (long ks = ks0; ks < K; ks += kadv, cur ^= 1) {
    // invariant on entry: glds(s) retired or retiring, w0(s)+w1(s) in
    // flight (16 loads). vmcnt(16) forces glds(s) landed (it is older
    // than the 16 W loads issued after it — except on the first
    // iteration, handled by the prologue wait above).
    asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    __syncthreads();
    const unsigned short* xb = xbuf[cur];
    const long ksn = ks + kadv;
    consume8<MT, 8>(w0, xb, acc0, row16, kgrp);      // vmcnt(15-u)
    // stage slice s+1, then its W loads (younger than the DMA)
    glds_stage_x(xbuf[cur ^ 1], x, K, (ksn < K ? ksn : 0), KSLICE, M,
                 wid, lane);
    const unsigned short* p0n = (ksn < K) ? p0 + kadv : p0;
    issue_w8(w0, p0n);
    consume8<MT, 16>(w1, xb, acc1, row16, kgrp);     // vmcnt(23-u)
    const unsigned short* p1n = (ksn < K) ? p1 + kadv : p1;
    issue_w8(w1, p1n);
    p0 = p0n;
    p1 = p1n;
  }
  // drain the cross-boundary loads (hipcc cannot see them, so it emits
  // no vmcnt(0) before s_endpgm; a load landing after the wave slot is
  // re-issued to the NEXT kernel's waves corrupts their VGPRs)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  const int ncol0 = n0t0 + 4 * kgrp;
  const int ncol1 = n0t1 + 4 * kgrp;
  float* slab = SPLIT ? ws + (long)blockIdx.y * M * N : nullptr;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int mrow = m * 16 + row16;
    if (mrow >= M) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long off0 = (long)mrow * N + ncol0 + r;
      const long off1 = (long)mrow * N + ncol1 + r;
      if (SPLIT) {
        slab[off0] = acc0[m][r];
        slab[off1] = acc1[m][r];
      } else {
        out[off0] = f2us(acc0[m][r]);
        out[off1] = f2us(acc1[m][r]);
      }
    }
  }
}

// ===========================================================================
// skinny v5 — full-line W stream through a wave-private LDS image.
//
// The request-granularity probe (scripts/pattern_probe3.hip) measured the
// fragment-shaped W read (16 rows x 64 B per instruction, half a 128-B
// line per row) at 5.7 TB/s vs 7.3 TB/s for an 8-rows x 128-B contiguous
// shape at the same geometry — the memory system is request-bound, not
// byte-bound. v5 therefore loads W contiguously (each instruction = 8
// rows x 128 B = 8 full-line requests), lands it in registers, and
// redistributes to MFMA fragment shape through a WAVE-PRIVATE LDS image
// (no barrier: only the issuing wave reads it), XOR-swizzled so the
// 16-row fragment reads are bank-conflict-free. The never-drain pipeline
// holds glds(x) + 16 W loads in flight across every slice barrier with
// every wait a constant vmcnt(16); the W image for slice s is written at
// the END of slice s-1 from loads issued a full slice earlier.
// ===========================================================================

// 8 contiguous nt loads for one tile's 16-row x 512-B slice: instruction
// (rb, u) covers rows rb..rb+7 at bytes [u*128, u*128+128). p_lo/p_hi are
// per-lane base pointers for rows (l>>3) and (8 + l>>3).
template <int NI>
DEV_INLINE void issue_wc(u32x4_t (&reg)[NI], const unsigned short* p_lo,
                         const unsigned short* p_hi) {
#define SK5_LD(i, P, off)                                                 \
  asm volatile("global_load_dwordx4 %0, %1, off offset:" #off " nt"      \
               : "=&v"(reg[i]) : "v"(P) : "memory")
  if constexpr (NI == 8) {
    SK5_LD(0, p_lo, 0); SK5_LD(1, p_lo, 128);
    SK5_LD(2, p_lo, 256); SK5_LD(3, p_lo, 384);
    SK5_LD(4, p_hi, 0); SK5_LD(5, p_hi, 128);
    SK5_LD(6, p_hi, 256); SK5_LD(7, p_hi, 384);
  } else {
    SK5_LD(0, p_lo, 0); SK5_LD(1, p_lo, 128);
    SK5_LD(2, p_hi, 0); SK5_LD(3, p_hi, 128);
  }
#undef SK5_LD
}

// same shape for the x operand but WITHOUT nt: x is L2-resident and
// re-read by every block — evict-first policy on it forces the whole x
// slice back to HBM for every block (+~50% HBM traffic on gate_up)
template <int NI>
DEV_INLINE void issue_xc(u32x4_t (&reg)[NI], const unsigned short* p_lo,
                         const unsigned short* p_hi) {
#define SK5_LDX(i, P, off)                                                \
  asm volatile("global_load_dwordx4 %0, %1, off offset:" #off            \
               : "=&v"(reg[i]) : "v"(P) : "memory")
  if constexpr (NI == 8) {
    SK5_LDX(0, p_lo, 0); SK5_LDX(1, p_lo, 128);
    SK5_LDX(2, p_lo, 256); SK5_LDX(3, p_lo, 384);
    SK5_LDX(4, p_hi, 0); SK5_LDX(5, p_hi, 128);
    SK5_LDX(6, p_hi, 256); SK5_LDX(7, p_hi, 384);
  } else {
    SK5_LDX(0, p_lo, 0); SK5_LDX(1, p_lo, 128);
    SK5_LDX(2, p_hi, 0); SK5_LDX(3, p_hi, 128);
  }
#undef SK5_LDX
}

// W-image byte offset inside one tile slot: row-major [16][KS*2 B]
// with the 16-B column slot XOR-swizzled by row (same scheme as xswz).
template <int KS>
DEV_INLINE int wimg_off(int row, int byte_in_row) {
  return row * (KS * 2) + (byte_in_row ^ ((row & 15) << 4));
}

template <int KS>
DEV_INLINE int xswz_ks(int row, int byte_in_row) {
  return row * (KS * 2) + (byte_in_row ^ ((row & 15) << 4));
}

// contiguous full-line loads for one tile slice: instruction (half, u)
// covers rows half*8+(lane>>3) at bytes [u*128, +128) — 8 whole 128-B
// lines per instruction (the request-granularity lever measured in
// scripts/pattern_probe3.hip). All loads are hipcc-VISIBLE (values in
// locals): with no LDS-DMA in this kernel the compiler's own counted
// vmcnt bookkeeping is exact, and register lifetimes are its problem —
// the invisible-asm variants corrupted under MT=4 register pressure
// (ledger: compiler reuse of in-flight asm destinations).
template <int NI, bool NT>
DEV_INLINE void load_tile(u32x4_t (&reg)[NI], const unsigned short* p_lo,
                          const unsigned short* p_hi) {
  constexpr int UPH = NI / 2;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const unsigned short* p = (i < UPH ? p_lo : p_hi) +
                              (i < UPH ? i : i - UPH) * 64;
    if constexpr (NT) {
      reg[i] = __builtin_nontemporal_load(
          reinterpret_cast<const u32x4_t*>(p));
    } else {
      reg[i] = *reinterpret_cast<const u32x4_t*>(p);
    }
  }
}

template <int MT, int KS>
DEV_INLINE void consume_img(const unsigned short* wimg,
                            const unsigned short* xb,
                            f32x4_t (&acc)[MT], int row16, int kgrp) {
#pragma unroll
  for (int u = 0; u < KS / 32; ++u) {
    const int kc = u * 32 + 8 * kgrp;
    const uint4 av = *reinterpret_cast<const uint4*>(
        reinterpret_cast<const char*>(wimg) + wimg_off<KS>(row16, kc * 2));
    const bf16x8_t af = frag_of(av);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int xr = m * 16 + row16;
      const uint4 xv = *reinterpret_cast<const uint4*>(
          reinterpret_cast<const char*>(xb) + xswz_ks<KS>(xr, kc * 2));
      acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          af, frag_of(xv), acc[m], 0, 0, 0);
    }
  }
}

// write one tile's 16-row register set into its LDS image slot
template <int KS, int NI = KS / 32>
DEV_INLINE void wimg_write(unsigned short* wimg, u32x4_t (&reg)[NI],
                           int lane) {
  const int seg16 = (lane & 7) * 16;
  constexpr int UPH = NI / 2;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int row = (i < UPH ? (lane >> 3) : 8 + (lane >> 3));
    const int u = (i < UPH) ? i : i - UPH;
    *reinterpret_cast<uint4*>(
        reinterpret_cast<char*>(wimg) +
        wimg_off<KS>(row, u * 128 + seg16)) =
        __builtin_bit_cast(uint4, reg[i]);
  }
}

// write one wave's 16 x rows into the SHARED xswz image; published to
// the other waves by the slice barrier
template <int KS, int NI = KS / 32>
DEV_INLINE void ximg_write(unsigned short* xb, u32x4_t (&reg)[NI], int wid,
                           int lane) {
  const int seg16 = (lane & 7) * 16;
  constexpr int UPH = NI / 2;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int row = wid * 16 + (i < UPH ? (lane >> 3) : 8 + (lane >> 3));
    const int u = (i < UPH) ? i : i - UPH;
    *reinterpret_cast<uint4*>(
        reinterpret_cast<char*>(xb) +
        xswz_ks<KS>(row, u * 128 + seg16)) =
        __builtin_bit_cast(uint4, reg[i]);
  }
}

// fused SwiGLU on a 16-B register fragment (8 bf16): same math as
// activation.hip silu_mul_kernel so the fused path matches the two-kernel
// path bit-for-bit through f2us round-to-nearest-even.
DEV_INLINE u32x4_t silu_mul8(u32x4_t g, u32x4_t u) {
  u32x4_t r;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const unsigned int gg = g[i], uu = u[i];
    const float g0 = us2f((unsigned short)(gg & 0xffffu));
    const float g1 = us2f((unsigned short)(gg >> 16));
    const float u0 = us2f((unsigned short)(uu & 0xffffu));
    const float u1 = us2f((unsigned short)(uu >> 16));
    const float r0 = g0 / (1.f + __expf(-g0)) * u0;
    const float r1 = g1 / (1.f + __expf(-g1)) * u1;
    r[i] = (unsigned int)f2us(r0) | ((unsigned int)f2us(r1) << 16);
  }
  return r;
}

template <int MT, bool SPLIT, int KS, bool SILU = false, int TILES = 2>
__global__ __launch_bounds__(256) void skinny5_kernel(
    unsigned short* __restrict__ out, float* __restrict__ ws,
    const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ w, int M, int N, long K) {
  // Never-drain full-line pipeline, pure HIP: slice s+1's W/x loads are
  // issued BEFORE the slice-s barrier (a full memory fence pins them
  // there) and ds_written to the images at the end of slice s, so ~3*NI
  // loads are always in flight and no wait ever sees the laden-queue
  // round trip. KS=256: 128 KiB LDS -> 1 block/CU; KS=128: 64 KiB ->
  // 2 blocks/CU (2 waves/SIMD hide the consume's dependency stalls).
  constexpr int NI = KS / 32;
  __shared__ __align__(16) unsigned short xbuf[2][64 * KS];
  __shared__ __align__(16) unsigned short wimg_all[4][TILES][16 * KS];
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int row16 = lane & 15;
  const int kgrp = lane >> 4;
  f32x4_t acc0[MT], acc1[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    acc0[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    acc1[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  const long kadv = (long)gridDim.y * KS;
  const long ks0 = (long)blockIdx.y * KS;
  if (ks0 >= K) return;
  u32x4_t w0[NI], w1[NI], xr8[NI];
  const int n0t0 = (blockIdx.x * TILES + 0) * 64 + wid * 16;
  const int n0t1 = (blockIdx.x * TILES + (TILES - 1)) * 64 + wid * 16;
  const int rlo = lane >> 3, seg = (lane & 7) * 8;  // elems
  const unsigned short* p0l = w + (long)(n0t0 + rlo) * K + ks0 + seg;
  const unsigned short* p0h = w + (long)(n0t0 + 8 + rlo) * K + ks0 + seg;
  const unsigned short* p1l = w + (long)(n0t1 + rlo) * K + ks0 + seg;
  const unsigned short* p1h = w + (long)(n0t1 + 8 + rlo) * K + ks0 + seg;
  const int xrow_l = wid * 16 + rlo;
  const int xrow_h = wid * 16 + 8 + rlo;
  // SILU: x is the fused gate_up GEMM output [M, 2K] — gate in the first
  // K columns, up in the second; the activation happens in registers on
  // the way into the LDS image and the standalone silu_mul kernel (plus
  // its act-tensor HBM round trip) disappears.
  const long xstride = SILU ? 2 * K : K;
  const unsigned short* pxl =
      x + (long)min(M - 1, xrow_l) * xstride + ks0 + seg;
  const unsigned short* pxh =
      x + (long)min(M - 1, xrow_h) * xstride + ks0 + seg;
  const unsigned short* pul = SILU ? pxl + K : nullptr;
  const unsigned short* puh = SILU ? pxh + K : nullptr;
  u32x4_t ur8[SILU ? NI : 1];
  unsigned short* img0 = wimg_all[wid][0];
  unsigned short* img1 = wimg_all[wid][TILES - 1];

  // prologue: land slice 0, build the images, put slice 1 in flight
  load_tile<NI, true>(w0, p0l, p0h);
  if constexpr (TILES == 2) load_tile<NI, true>(w1, p1l, p1h);
  load_tile<NI, false>(xr8, pxl, pxh);
  if constexpr (SILU) {
    load_tile<NI, false>(ur8, pul, puh);
#pragma unroll
    for (int i = 0; i < NI; ++i) xr8[i] = silu_mul8(xr8[i], ur8[i]);
  }
  wimg_write<KS>(img0, w0, lane);
  if constexpr (TILES == 2) wimg_write<KS>(img1, w1, lane);
  ximg_write<KS>(xbuf[0], xr8, wid, lane);
  {
    const long ks1 = ks0 + kadv;
    if (ks1 < K) {
      p0l += kadv; p0h += kadv; p1l += kadv; p1h += kadv;
      pxl += kadv; pxh += kadv;
      if constexpr (SILU) { pul += kadv; puh += kadv; }
    }
    load_tile<NI, true>(w0, p0l, p0h);
    if constexpr (TILES == 2) load_tile<NI, true>(w1, p1l, p1h);
    load_tile<NI, false>(xr8, pxl, pxh);
    if constexpr (SILU) load_tile<NI, false>(ur8, pul, puh);
  }
  int cur = 0;
  for (long ks = ks0; ks < K; ks += kadv, cur ^= 1) {
    // entry: slice s+1 loads in flight (w0/w1/xr8 values pending);
    // images(s) + xbuf[cur] ready
    __syncthreads();
    const unsigned short* xb = xbuf[cur];
    const long ksn = ks + kadv;
    const bool adv = (ksn + kadv) < K;
    consume_img<MT, KS>(img0, xb, acc0, row16, kgrp);   // LDS-only
    wimg_write<KS>(img0, w0, lane);   // first USE of w0 -> counted wait
    if (adv) { p0l += kadv; p0h += kadv; }
    load_tile<NI, true>(w0, p0l, p0h);                  // slice s+2
    if constexpr (TILES == 2) {
      consume_img<MT, KS>(img1, xb, acc1, row16, kgrp);
      wimg_write<KS>(img1, w1, lane);
      if (adv) { p1l += kadv; p1h += kadv; }
      load_tile<NI, true>(w1, p1l, p1h);
    }
    if constexpr (SILU) {
#pragma unroll
      for (int i = 0; i < NI; ++i) xr8[i] = silu_mul8(xr8[i], ur8[i]);
    }
    ximg_write<KS>(xbuf[cur ^ 1], xr8, wid, lane);
    if (adv) {
      pxl += kadv; pxh += kadv;
      if constexpr (SILU) { pul += kadv; puh += kadv; }
    }
    load_tile<NI, false>(xr8, pxl, pxh);
    if constexpr (SILU) load_tile<NI, false>(ur8, pul, puh);
    // exit: slice s+2 loads in flight — invariant restored
  }

  const int ncol0 = n0t0 + 4 * kgrp;
  const int ncol1 = n0t1 + 4 * kgrp;
  float* slab = SPLIT ? ws + (long)blockIdx.y * M * N : nullptr;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int mrow = m * 16 + row16;
    if (mrow >= M) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long off0 = (long)mrow * N + ncol0 + r;
      const long off1 = (long)mrow * N + ncol1 + r;
      if (SPLIT) {
        slab[off0] = acc0[m][r];
        if constexpr (TILES == 2) slab[off1] = acc1[m][r];
      } else {
        out[off0] = f2us(acc0[m][r]);
        if constexpr (TILES == 2) out[off1] = f2us(acc1[m][r]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// v6: barrier-free register-x pipeline.
//
// v5's residual gap (chip ~4 TB/s vs 6.1-6.75 for every ingredient probe,
// ledger profiles/r02_progress.md item 4) correlates with its one structural
// cost: the shared-LDS x image forces a per-slice __syncthreads(), and at
// ~256 blocks on 256 CUs there is ONE wave per SIMD — so every slice, all
// four waves convoy on the barrier and the slowest wave's memory jitter is
// paid by the whole block, every slice.
//
// v6 removes the barrier entirely: the MFMA x operand (B fragment) is 16
// contiguous bytes per lane at x[row][kc..kc+8], so it can be loaded
// DIRECTLY from global memory (x is L2-resident) into registers one slice
// ahead — no LDS staging, no cross-wave publication, no barrier. W keeps
// the v5 full-line nt stream + per-wave XOR-swizzled LDS image. Each wave
// is fully self-paced; the only cross-lane structure left is the wave
// itself. LDS drops to the W images (KS*256 B per block).
// ---------------------------------------------------------------------------
template <int MT, int XNI>
DEV_INLINE void load_xfrags(u32x4_t (&xr)[MT][XNI],
                            const unsigned short* const (&xq)[MT]) {
#pragma unroll
  for (int m = 0; m < MT; ++m) {
#pragma unroll
    for (int u = 0; u < XNI; ++u) {
      xr[m][u] = *reinterpret_cast<const u32x4_t*>(xq[m] + u * 32);
    }
  }
}

template <int MT, int KS>
DEV_INLINE void consume_reg(const unsigned short* wimg,
                            const u32x4_t (&xr)[MT][KS / 32],
                            f32x4_t (&acc)[MT], int row16, int kgrp) {
#pragma unroll
  for (int u = 0; u < KS / 32; ++u) {
    const int kc = u * 32 + 8 * kgrp;
    const uint4 av = *reinterpret_cast<const uint4*>(
        reinterpret_cast<const char*>(wimg) + wimg_off<KS>(row16, kc * 2));
    const bf16x8_t af = frag_of(av);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          af, frag_of(xr[m][u]), acc[m], 0, 0, 0);
    }
  }
}

template <int MT, bool SPLIT, int KS>
__global__ __launch_bounds__(256) void skinny6_kernel(
    unsigned short* __restrict__ out, float* __restrict__ ws,
    const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ w, int M, int N, long K) {
  constexpr int NI = KS / 32;
  constexpr int XNI = KS / 32;
  __shared__ __align__(16) unsigned short wimg_all[4][2][16 * KS];
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int row16 = lane & 15;
  const int kgrp = lane >> 4;
  f32x4_t acc0[MT], acc1[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    acc0[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    acc1[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
  const long kadv = (long)gridDim.y * KS;
  const long ks0 = (long)blockIdx.y * KS;
  if (ks0 >= K) return;
  u32x4_t w0[NI], w1[NI];
  u32x4_t xa[MT][XNI], xb[MT][XNI];
  const int n0t0 = (blockIdx.x * 2 + 0) * 64 + wid * 16;
  const int n0t1 = (blockIdx.x * 2 + 1) * 64 + wid * 16;
  const int rlo = lane >> 3, seg = (lane & 7) * 8;  // elems
  const unsigned short* p0l = w + (long)(n0t0 + rlo) * K + ks0 + seg;
  const unsigned short* p0h = w + (long)(n0t0 + 8 + rlo) * K + ks0 + seg;
  const unsigned short* p1l = w + (long)(n0t1 + rlo) * K + ks0 + seg;
  const unsigned short* p1h = w + (long)(n0t1 + 8 + rlo) * K + ks0 + seg;
  const unsigned short* xq[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    xq[m] = x + (long)min(M - 1, m * 16 + row16) * K + ks0 + 8 * kgrp;
  }
  unsigned short* img0 = wimg_all[wid][0];
  unsigned short* img1 = wimg_all[wid][1];

  // prologue: land slice 0, build the W images, put slice 1 in flight
  load_tile<NI, true>(w0, p0l, p0h);
  load_tile<NI, true>(w1, p1l, p1h);
  load_xfrags<MT, XNI>(xa, xq);
  wimg_write<KS>(img0, w0, lane);
  wimg_write<KS>(img1, w1, lane);
  {
    const long ks1 = ks0 + kadv;
    if (ks1 < K) {
      p0l += kadv; p0h += kadv; p1l += kadv; p1h += kadv;
#pragma unroll
      for (int m = 0; m < MT; ++m) xq[m] += kadv;
    }
    load_tile<NI, true>(w0, p0l, p0h);
    load_tile<NI, true>(w1, p1l, p1h);
    load_xfrags<MT, XNI>(xb, xq);
  }
  long ks = ks0;
  // per-slice body: consume slice `ks` from the images + xcur, keep the
  // never-drain invariant (slice ks+2's W and x loads in flight on exit).
  // No __syncthreads anywhere: images and x fragments are wave-private,
  // and a wave's LDS reads/writes to the same image are ordered by the
  // per-wave in-order LDS pipe (the same guarantee v5's consume->rewrite
  // sequence already relies on).
  auto step6 = [&](u32x4_t (&xcur)[MT][XNI]) {
    const bool adv = (ks + 2 * kadv) < K;
    consume_reg<MT, KS>(img0, xcur, acc0, row16, kgrp);
    wimg_write<KS>(img0, w0, lane);  // first USE of w0 -> counted wait
    if (adv) { p0l += kadv; p0h += kadv; }
    load_tile<NI, true>(w0, p0l, p0h);
    consume_reg<MT, KS>(img1, xcur, acc1, row16, kgrp);
    wimg_write<KS>(img1, w1, lane);
    if (adv) { p1l += kadv; p1h += kadv; }
    load_tile<NI, true>(w1, p1l, p1h);
    if (adv) {
#pragma unroll
      for (int m = 0; m < MT; ++m) xq[m] += kadv;
    }
    load_xfrags<MT, XNI>(xcur, xq);
  };
  for (;;) {
    step6(xa);
    ks += kadv;
    if (ks >= K) break;
    step6(xb);
    ks += kadv;
    if (ks >= K) break;
  }

  const int ncol0 = n0t0 + 4 * kgrp;
  const int ncol1 = n0t1 + 4 * kgrp;
  float* slab = SPLIT ? ws + (long)blockIdx.y * M * N : nullptr;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int mrow = m * 16 + row16;
    if (mrow >= M) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long off0 = (long)mrow * N + ncol0 + r;
      const long off1 = (long)mrow * N + ncol1 + r;
      if (SPLIT) {
        slab[off0] = acc0[m][r];
        slab[off1] = acc1[m][r];
      } else {
        out[off0] = f2us(acc0[m][r]);
        out[off1] = f2us(acc1[m][r]);
      }
    }
  }
}

// ===========================================================================
// W8A16: out[M,N] = (x[M,K] @ float(q[N,K])^T) * scale[N], q = OCP e4m3fn
// bytes with one f32 scale per output row (ops.Fp8Weight).
//
// v1's staging with a 1-byte W stream. e4m3 -> bf16 is exact, so the
// bytes are widened in registers and feed the same bf16 MFMA into the same
// f32 accumulators; x is not quantised. A lane's 16-B load is 16 k values
// of one row, spent on two MFMAs whose x fragments sit 8 k apart in the
// xswz image (the sum over k has no order, so A and B only have to agree
// on which k a lane holds). One load instruction covers 16 rows x 64 B and
// a slice's batch of 4 covers two whole 128-B lines per row. scale[n]
// multiplies the f32 accumulator on the way out, on the direct store and
// on the slab store alike (linear per column), so both split-K epilogues
// are shared unchanged. Requires N%64 == 0 and K%64 == 0.
// ===========================================================================
constexpr int W8_U = KSLICE / 64;  // 16-B W loads per lane per full slice

template <int MT>
DEV_INLINE void w8_consume(u32x4_t wv, const unsigned short* xb,
                           f32x4_t (&acc)[MT], int kc0, int row16) {
  const uint4 lo = fp8x8_to_bf16x8(uint2{wv[0], wv[1]});
  const uint4 hi = fp8x8_to_bf16x8(uint2{wv[2], wv[3]});
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const bf16x8_t afrag = frag_of(h == 0 ? lo : hi);
    const int kc = kc0 + 8 * h;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int xr = m * 16 + row16;
      const uint4 xv = *reinterpret_cast<const uint4*>(
          reinterpret_cast<const char*>(xb) + xswz(xr, kc * 2));
      acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          afrag, frag_of(xv), acc[m], 0, 0, 0);
    }
  }
}

template <int MT, bool SPLIT>
__global__ __launch_bounds__(256) void skinny_w8_kernel(
    unsigned short* __restrict__ out,      // [M, N] bf16 (SPLIT=false)
    float* __restrict__ ws,                // [splitk, M, N] f32 (SPLIT)
    const unsigned short* __restrict__ x,  // [M, K] bf16
    const unsigned char* __restrict__ q,   // [N, K] e4m3fn
    const float* __restrict__ scale,       // [N]
    int M, int N, long K) {
  __shared__ __align__(16) unsigned short xbuf[2][64 * KSLICE];
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int n0 = blockIdx.x * 64 + wid * 16;     // this wave's 16 N rows
  const int row16 = lane & 15;                   // A row / B col
  const int kgrp = lane >> 4;                    // 0..3 -> k = 16*kgrp + j
  f32x4_t acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // this block walks slices ks0 + i*kstride: `nfull` whole ones, then the
  // short tail slice if it falls to this block (only K's last slice can
  // be short)
  const long kstride = (long)gridDim.y * KSLICE;
  const long ks0 = (long)blockIdx.y * KSLICE;
  if (ks0 >= K) return;  // never: the plan clamps splitk to the slices
  const int nall = (int)((K - ks0 + kstride - 1) / kstride);
  const bool has_tail = ks0 + (long)(nall - 1) * kstride + KSLICE > K;
  const int nfull = nall - (has_tail ? 1 : 0);
  const unsigned char* wrow = q + (long)(n0 + row16) * K + ks0 + 16 * kgrp;

  // Three W register sets rotate so that two slices of W stay in flight
  // while a third is consumed (a drained stream pays the whole laden
  // memory latency per slice; measured 2.1 us a slice on the down shape).
  // Issue order in slice i, after its barrier: the staging DMAs of slice
  // i+1, then the W loads of slice i+2. At the top of slice i the VM
  // queue therefore holds W(i), DMA(i), W(i+1), oldest first, and the
  // one explicit wait leaves exactly the W(i+1) loads in flight: every
  // DMA is older than all the plain loads the wait counts, v1's ordering
  // (vmcnt class-ordering, profiles/r02_progress.md item 1).
  u32x4_t wa[3][W8_U];
  auto issue = [&](u32x4_t (&w)[W8_U], int i) {
#pragma unroll
    for (int u = 0; u < W8_U; ++u)
      w[u] = nt_load16(wrow + (long)i * kstride + u * 64);
  };
  auto stage = [&](int i) {
    const long ks = ks0 + (long)i * kstride;
    glds_stage_x(xbuf[i & 1], x, K, ks, (int)min((long)KSLICE, K - ks), M,
                 wid, lane);
  };
  // one whole slice: AHEAD says the W of slice i+1 is in flight behind
  // this one's (the explicit wait leaves it there), ISSUE sends slice
  // i+2's W into `nxt2`. Both are compile-time so that the steady loop
  // has no branch around a load: hipcc's own counted waits then stay
  // exact (a conditional issue made it drain to vmcnt(0) every slice).
  auto slice = [&](auto ahead, auto do_issue, u32x4_t (&cur)[W8_U],
                   u32x4_t (&nxt2)[W8_U], int i) {
    asm volatile("s_waitcnt vmcnt(%c0)" ::"i"(decltype(ahead)::value ? W8_U
                                                                      : 0)
                 : "memory");
    __syncthreads();
    // hipcc cannot count the DMAs: make it place its own wait for this
    // slice's W here, where its count is exact, not after the issues
    // below, where it would also wait out the DMAs
#pragma unroll
    for (int u = 0; u < W8_U; ++u) asm volatile("" : "+v"(cur[u]));
    // safe without a second barrier: every wave finished reading the
    // other x buffer (slice i-1) before it crossed this slice's barrier
    if (i + 1 < nall) stage(i + 1);
    if constexpr (decltype(do_issue)::value) issue(nxt2, i + 2);
#pragma unroll
    for (int u = 0; u < W8_U; ++u)
      w8_consume<MT>(cur[u], xbuf[i & 1], acc, u * 64 + 16 * kgrp, row16);
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  // the last two whole slices: nothing left to issue
  auto last2 = [&](u32x4_t (&a)[W8_U], u32x4_t (&b)[W8_U], int i) {
    slice(yes, no, a, a, i);
    slice(no, no, b, b, i + 1);
  };

  stage(0);
  if (nfull >= 2) {
    issue(wa[0], 0);
    issue(wa[1], 1);
    // whole turns of the three sets in the loop, so that each set is one
    // fixed group of registers all the way round (an exit in mid-turn
    // made hipcc rotate the sets with copies, and wait for them)
    const int nsteady = nfull - 2;  // slices with a slice i+2 to issue
    int i = 0;
    for (; i + 3 <= nsteady; i += 3) {
      slice(yes, yes, wa[0], wa[2], i);
      slice(yes, yes, wa[1], wa[0], i + 1);
      slice(yes, yes, wa[2], wa[1], i + 2);
    }
    if (nsteady - i == 0) {
      last2(wa[0], wa[1], i);
    } else if (nsteady - i == 1) {
      slice(yes, yes, wa[0], wa[2], i);
      last2(wa[1], wa[2], i + 1);
    } else {
      slice(yes, yes, wa[0], wa[2], i);
      slice(yes, yes, wa[1], wa[0], i + 1);
      last2(wa[2], wa[0], i + 2);
    }
  } else if (nfull == 1) {
    issue(wa[0], 0);
    slice(no, no, wa[0], wa[0], 0);
  }
  if (has_tail) {
    // klen in {64, 128, 192}: one 64-k chunk at a time, nothing else in
    // flight (its x was staged during the last whole slice, or above)
    const long ks = ks0 + (long)nfull * kstride;
    const int klen = (int)(K - ks);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kc0 = 0; kc0 < klen; kc0 += 64)
      w8_consume<MT>(nt_load16(wrow + (long)nfull * kstride + kc0),
                     xbuf[nfull & 1], acc, kc0 + 16 * kgrp, row16);
  }

  // C layout: lane -> M index = lane&15, N index = n0 + 4*(lane>>4) + r
  const int ncol = n0 + 4 * kgrp;
  float sc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) sc[r] = scale[ncol + r];
  float* slab = SPLIT ? ws + (long)blockIdx.y * M * N : nullptr;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int mrow = m * 16 + row16;
    if (mrow >= M) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long off = (long)mrow * N + ncol + r;
      const float v = acc[m][r] * sc[r];
      if (SPLIT) {
        slab[off] = v;
      } else {
        out[off] = f2us(v);
      }
    }
  }
}

// ===========================================================================
// W4A16: out[M,N] = x[M,K] @ deq(q, scale)^T with MXFP4 weights
// (ops.Mxfp4Weight): q[N,K/2] two e2m1 codes per byte, scale[N,K/32] one
// e8m0 byte per block of 32 along K.
//
// The W8 kernel's walk with a half-byte W stream. A lane's 16-B load is 32
// k values of one row, which is exactly one MX block: one scale byte per
// load. Four lane groups cover 128 k, so a 256-k slice is one whole 128-B
// line per row, two loads per lane. Each dword of a load is 8 consecutive
// k: v_cvt_scalef32_pk_bf16_fp4 widens it to a bf16x8 A fragment with the
// block scale already applied (exact: a 2-bit significand times a power of
// two), and the load's four fragments feed four MFMAs against x fragments
// 8 k apart in the xswz image. The accumulator is therefore stored as it
// is and both split-K epilogues are shared unchanged.
//
// Scale bytes: a slice has 8 per row and a lane needs the two at
// kgrp and 4 + kgrp. Each lane fetches all 8 itself in one 8-byte load
// (the four lane groups of a row read the same address), issued with the
// slice's W loads into the same register set, and picks its bytes out
// when it widens. That keeps every load a plain counted one (no LDS
// staging or cross-lane traffic for 2 bytes), and the 16 rows' bytes sit
// in lines that stay in L2 for the whole walk (a row of K = 4096 has 128
// scale bytes, one line). A scale row is K/32 bytes, so with K%128 == 0
// the load is dword-aligned, which is all a global dwordx2 load needs
// (8-byte-aligned only when K%256 == 0); the type below says so. Two
// dword loads instead are merged by hipcc into this same instruction,
// and the explicit wait below has to know how many loads a slice is.
// Not 1-byte loads: hipcc puts their zero-extend right behind the load,
// which made it wait for the slice just issued in the middle of the
// steady loop. Requires N%64 == 0 and K%128 == 0.
// ===========================================================================
constexpr int W4_U = KSLICE / 128;  // 16-B W loads per lane per full slice
static_assert(W4_U == 2, "a slice's scale bytes are one 8-byte load");
constexpr int W4_LOADS = W4_U + 1;  // VM ops per lane per full slice

struct __attribute__((packed, aligned(4))) W4Scales {
  unsigned int s[W4_U];  // e8m0 bytes of 128 k each, one per lane group
};

struct W4Regs {
  u32x4_t w[W4_U];
  unsigned int s[W4_U];
};

template <int MT>
DEV_INLINE void w4_consume(u32x4_t wv, unsigned int sdword, int kgrp,
                           const unsigned short* xb, f32x4_t (&acc)[MT],
                           int kc0, int row16) {
  const float s = e8m0_to_f32((sdword >> (8 * kgrp)) & 0xffu);
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const bf16x8_t afrag = frag_of(fp4x8_to_bf16x8(wv[d], s));
    const int kc = kc0 + 8 * d;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int xr = m * 16 + row16;
      const uint4 xv = *reinterpret_cast<const uint4*>(
          reinterpret_cast<const char*>(xb) + xswz(xr, kc * 2));
      acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          afrag, frag_of(xv), acc[m], 0, 0, 0);
    }
  }
}

template <int MT, bool SPLIT>
__global__ __launch_bounds__(256) void skinny_w4_kernel(
    unsigned short* __restrict__ out,         // [M, N] bf16 (SPLIT=false)
    float* __restrict__ ws,                   // [splitk, M, N] f32 (SPLIT)
    const unsigned short* __restrict__ x,     // [M, K] bf16
    const unsigned char* __restrict__ q,      // [N, K/2] e2m1 pairs
    const unsigned char* __restrict__ scale,  // [N, K/32] e8m0
    int M, int N, long K) {
  __shared__ __align__(16) unsigned short xbuf[2][64 * KSLICE];
  const int wid = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int n0 = blockIdx.x * 64 + wid * 16;     // this wave's 16 N rows
  const int row16 = lane & 15;                   // A row / B col
  const int kgrp = lane >> 4;                    // 0..3 -> k = 32*kgrp + j
  f32x4_t acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) acc[m] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // the W8 kernel's walk: `nfull` whole slices ks0 + i*kstride, then the
  // short tail slice (K % 256 == 128) if it falls to this block
  const long kstride = (long)gridDim.y * KSLICE;
  const long ks0 = (long)blockIdx.y * KSLICE;
  if (ks0 >= K) return;  // never: the plan clamps splitk to the slices
  const int nall = (int)((K - ks0 + kstride - 1) / kstride);
  const bool has_tail = ks0 + (long)(nall - 1) * kstride + KSLICE > K;
  const int nfull = nall - (has_tail ? 1 : 0);
  const unsigned char* wrow =
      q + (long)(n0 + row16) * (K / 2) + ks0 / 2 + 16 * kgrp;
  const unsigned char* srow =
      scale + (long)(n0 + row16) * (K / 32) + ks0 / 32;

  // Three register sets rotate as in the W8 kernel: two slices of W (and
  // their scale bytes) stay in flight while a third is consumed. A set is
  // W4_LOADS plain loads, so at the top of slice i the VM queue holds
  // W(i), DMA(i), W(i+1), oldest first, and the explicit wait leaves
  // exactly W(i+1)'s W4_LOADS loads in flight: every DMA is older than
  // all the plain loads the wait counts (profiles/r02_progress.md item 1).
  W4Regs wa[3];
  auto issue = [&](W4Regs& r, int i) {
#pragma unroll
    for (int u = 0; u < W4_U; ++u)
      r.w[u] = nt_load16(wrow + (long)i * (kstride / 2) + u * 64);
    const W4Scales sc = *reinterpret_cast<const W4Scales*>(
        srow + (long)i * (kstride / 32));
#pragma unroll
    for (int u = 0; u < W4_U; ++u) r.s[u] = sc.s[u];
  };
  auto stage = [&](int i) {
    const long ks = ks0 + (long)i * kstride;
    glds_stage_x(xbuf[i & 1], x, K, ks, (int)min((long)KSLICE, K - ks), M,
                 wid, lane);
  };
  // AHEAD / ISSUE are compile-time for the W8 kernel's reason: no branch
  // around a load in the steady loop, so hipcc's counted waits stay exact
  auto slice = [&](auto ahead, auto do_issue, W4Regs& cur, W4Regs& nxt2,
                   int i) {
    asm volatile("s_waitcnt vmcnt(%c0)" ::"i"(decltype(ahead)::value
                                                  ? W4_LOADS
                                                  : 0)
                 : "memory");
    __syncthreads();
    // make hipcc place its own wait for this slice's loads here, where
    // its count is exact, not after the issues below (it cannot count
    // the DMAs)
#pragma unroll
    for (int u = 0; u < W4_U; ++u)
      asm volatile("" : "+v"(cur.w[u]), "+v"(cur.s[u]));
    // safe without a second barrier: every wave finished reading the
    // other x buffer (slice i-1) before it crossed this slice's barrier
    if (i + 1 < nall) stage(i + 1);
    if constexpr (decltype(do_issue)::value) issue(nxt2, i + 2);
#pragma unroll
    for (int u = 0; u < W4_U; ++u)
      w4_consume<MT>(cur.w[u], cur.s[u], kgrp, xbuf[i & 1], acc,
                     u * 128 + 32 * kgrp, row16);
  };
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  // the last two whole slices: nothing left to issue
  auto last2 = [&](W4Regs& a, W4Regs& b, int i) {
    slice(yes, no, a, a, i);
    slice(no, no, b, b, i + 1);
  };

  stage(0);
  if (nfull >= 2) {
    issue(wa[0], 0);
    issue(wa[1], 1);
    // whole turns of the three sets in the loop, so that each set is one
    // fixed group of registers all the way round
    const int nsteady = nfull - 2;  // slices with a slice i+2 to issue
    int i = 0;
    for (; i + 3 <= nsteady; i += 3) {
      slice(yes, yes, wa[0], wa[2], i);
      slice(yes, yes, wa[1], wa[0], i + 1);
      slice(yes, yes, wa[2], wa[1], i + 2);
    }
    if (nsteady - i == 0) {
      last2(wa[0], wa[1], i);
    } else if (nsteady - i == 1) {
      slice(yes, yes, wa[0], wa[2], i);
      last2(wa[1], wa[2], i + 1);
    } else {
      slice(yes, yes, wa[0], wa[2], i);
      slice(yes, yes, wa[1], wa[0], i + 1);
      last2(wa[2], wa[0], i + 2);
    }
  } else if (nfull == 1) {
    issue(wa[0], 0);
    slice(no, no, wa[0], wa[0], 0);
  }
  if (has_tail) {
    // klen == 128: one 128-k chunk at a time, nothing else in flight (its
    // x was staged during the last whole slice, or above)
    const long ks = ks0 + (long)nfull * kstride;
    const int klen = (int)(K - ks);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kc0 = 0; kc0 < klen; kc0 += 128)
      w4_consume<MT>(
          nt_load16(wrow + (long)nfull * (kstride / 2) + kc0 / 2),
          *reinterpret_cast<const unsigned int*>(
              srow + (long)nfull * (kstride / 32) + kc0 / 32),
          kgrp,
          xbuf[nfull & 1], acc, kc0 + 32 * kgrp, row16);
  }

  // C layout: lane -> M index = lane&15, N index = n0 + 4*(lane>>4) + r
  const int ncol = n0 + 4 * kgrp;
  float* slab = SPLIT ? ws + (long)blockIdx.y * M * N : nullptr;
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int mrow = m * 16 + row16;
    if (mrow >= M) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long off = (long)mrow * N + ncol + r;
      if (SPLIT) {
        slab[off] = acc[m][r];
      } else {
        out[off] = f2us(acc[m][r]);
      }
    }
  }
}

// ===========================================================================
// Host side. Every variant is the same algorithm: split K over ~256 blocks,
// run the GEMM kernel straight to bf16 (splitk == 1) or into splitk f32
// slabs, then one of two epilogues. A variant differs only in its plan
// parameters and its kernel.
// ===========================================================================

struct SkinnyPlan {
  int M, N;
  long K;
  int ngroups;  // grid.x: blocks along N
  int nslices;  // K slices available to split over
  int splitk;   // grid.y: f32 slabs written when > 1
  int MT;       // 16-row M subtiles
};

// ~256 blocks (1x the CU count) is the sweep's knee for every shape:
// per-block latency is ~constant in N in this regime, so more split-K
// past chip fill only adds slab/reduce traffic (scripts/sweep_splitk.py).
// At `off_at` blocks or more along N the grid fills the chip by itself.
static SkinnyPlan skinny_plan(int M, int N, long K, int cols, int slice,
                              int off_at, const char* env) {
  SkinnyPlan p{M, N, K};
  p.ngroups = N / cols;
  TORCH_CHECK(p.ngroups > 0, "skinny plan: N < ", cols);
  p.nslices = (int)((K + slice - 1) / slice);
  p.splitk = p.ngroups >= off_at
                 ? 1
                 : min(p.nslices, (256 + p.ngroups - 1) / p.ngroups);
  if (const char* ov = getenv(env)) {
    const int v = atoi(ov);
    if (v > 0) p.splitk = min(p.nslices, v);
  }
  p.MT = (M + 15) / 16;
  return p;
}

// TILES=1 (default): 64 N-cols per block at the same ~256-block split-K
// budget -> HALF the slab traffic per block count, measured 3-4% faster
// on every dispatched shape (down 31.7 vs 32.6 us, 70b-down 80.2 vs 83.9
// — sweep_nsplit.py; the 512-block co-residency variant was NOT the win,
// smaller blocks at equal splitk were). KUKEON_SK5_NSPLIT=2 restores the
// two-tile geometry.
static int sk5_tiles() {
  const char* nv = getenv("KUKEON_SK5_NSPLIT");
  return (nv && atoi(nv) == 2) ? 2 : 1;
}

// KS < 128 is unsound: the XOR swizzle offsets (row&15)<<4 span 256
// bytes, a full KS=128 row — at KS=64 they cross rows (measured: garbage
// output, sweep_ks.py). 128 and 256 are the valid geometries.
static int ks_from_env(const char* env) {
  const char* ov = getenv(env);
  return (ov && atoi(ov) == 256) ? 256 : 128;
}

static SkinnyPlan plan_v1(int M, int N, long K) {
  return skinny_plan(M, N, K, 64, KSLICE, 512, "KUKEON_SKINNY_SPLITK");
}
static SkinnyPlan plan_v2(int M, int N, long K) {
  return skinny_plan(M, N, K, 128, KSLICE, 256, "KUKEON_SK2_SPLITK");
}
static SkinnyPlan plan_v5(int M, int N, long K, int tiles, int KS) {
  return skinny_plan(M, N, K, 64 * tiles, KS, 256, "KUKEON_SK5_SPLITK");
}
static SkinnyPlan plan_v6(int M, int N, long K, int KS) {
  return skinny_plan(M, N, K, 128, KS, 256, "KUKEON_SK6_SPLITK");
}
static SkinnyPlan plan_w8(int M, int N, long K) {
  return skinny_plan(M, N, K, 64, KSLICE, 512, "KUKEON_W8_SPLITK");
}
static SkinnyPlan plan_w4(int M, int N, long K) {
  return skinny_plan(M, N, K, 64, KSLICE, 512, "KUKEON_W4_SPLITK");
}

// The split-K factor a launcher will use, for sizing its workspace
// (64 * N * splitk floats cover every M). Host-only.
int64_t skinny_splitk(const std::string& kind, int64_t N, int64_t K) {
  const int n = (int)N;
  if (kind == "v1") return plan_v1(1, n, K).splitk;
  if (kind == "v2") return plan_v2(1, n, K).splitk;
  if (kind == "v5")
    return plan_v5(1, n, K, sk5_tiles(), ks_from_env("KUKEON_SK5_KS")).splitk;
  if (kind == "v5_fused") return plan_v5(1, n, K, sk5_tiles(), 128).splitk;
  if (kind == "v6")
    return plan_v6(1, n, K, ks_from_env("KUKEON_SK6_KS")).splitk;
  if (kind == "w8") return plan_w8(1, n, K).splitk;
  if (kind == "w4") return plan_w4(1, n, K).splitk;
  TORCH_CHECK(false, "skinny_splitk: unknown kind ", kind);
}

using SkinnyKernel = void (*)(unsigned short*, float*, const unsigned short*,
                              const unsigned short*, int, int, long);

// f(std::integral_constant<int, MT>) with the runtime MT as a constant
template <class F>
static void with_mt(int MT, F&& f) {
  switch (MT) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

static unsigned short* us_ptr(const torch::Tensor& t) {
  return reinterpret_cast<unsigned short*>(t.data_ptr());
}

static float* slab_ptr(const SkinnyPlan& p, torch::Tensor& ws) {
  TORCH_CHECK(ws.numel() >= (long)p.M * p.N * p.splitk,
              "skinny workspace too small");
  return ws.data_ptr<float>();
}

// What a launcher hands the two epilogues: launch(split, out, ws, grid,
// stream) starts the variant's GEMM kernel, the bf16-direct one or the
// slab one. bf16_gemm() is that for every variant whose kernel has the
// SkinnyKernel signature.
static auto bf16_gemm(const SkinnyPlan& p, SkinnyKernel direct,
                      SkinnyKernel split, const torch::Tensor& x,
                      const torch::Tensor& w) {
  return [=, &p](bool is_split, unsigned short* out, float* ws, dim3 grid,
                 hipStream_t stream) {
    (is_split ? split : direct)<<<grid, 256, 0, stream>>>(
        out, ws, us_ptr(x), us_ptr(w), p.M, p.N, p.K);
  };
}

// Plain epilogue: the direct kernel writes bf16 itself at splitk == 1;
// otherwise the split kernel fills the slabs and the reduce pass casts
// their sum to bf16.
template <class Launch>
static void run_reduce(const SkinnyPlan& p, Launch&& launch,
                       torch::Tensor& out, torch::Tensor& ws) {
  auto stream = c10::hip::getCurrentHIPStream().stream();
  const dim3 grid(p.ngroups, p.splitk);
  if (p.splitk == 1) {
    launch(false, us_ptr(out), nullptr, grid, stream);
  } else {
    float* wsp = slab_ptr(p, ws);
    const long total = (long)p.M * p.N;
    launch(true, nullptr, wsp, grid, stream);
    skinny_reduce_kernel<<<dim3((unsigned)((total / 8 + 255) / 256)), 256, 0,
                           stream>>>(us_ptr(out), wsp, total, p.splitk);
  }
  HIP_CHECK_KERNEL();
}

// Fused epilogue: always the slab kernel (also at splitk == 1), then
// split-K reduce + residual add + RMSNorm in one kernel.
template <class Launch>
static void run_reduce_add_rmsnorm(const SkinnyPlan& p, Launch&& launch,
                                   torch::Tensor& normed, torch::Tensor& ws,
                                   torch::Tensor& residual,
                                   const torch::Tensor& nw, double eps) {
  auto stream = c10::hip::getCurrentHIPStream().stream();
  float* wsp = slab_ptr(p, ws);
  launch(true, nullptr, wsp, dim3(p.ngroups, p.splitk), stream);
  HIP_CHECK_KERNEL();
  skinny_reduce_add_rmsnorm_kernel<<<dim3((unsigned)p.M), 256, 0, stream>>>(
      us_ptr(normed), us_ptr(residual), wsp, us_ptr(nw), p.N,
      (long)p.M * p.N, p.splitk, (float)eps);
  HIP_CHECK_KERNEL();
}

// shape checks shared by the plain / fused entry points (the fused
// epilogue holds one row in 32 registers per thread: N <= 8192, N%2048)
static void check_plain(const torch::Tensor& out, const torch::Tensor& x,
                        const torch::Tensor& w, int ncols, int kdiv) {
  const long M = x.size(0);
  TORCH_CHECK(M >= 1 && M <= 64, "skinny gemm: M must be in [1,64]");
  TORCH_CHECK(w.size(0) % ncols == 0 && x.size(1) % kdiv == 0,
              "skinny gemm: N%", ncols, ", K%", kdiv);
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous() && out.is_contiguous());
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16);
}
static void check_fused(const torch::Tensor& normed, const torch::Tensor& x,
                        const torch::Tensor& w, const torch::Tensor& residual,
                        long K, int kdiv) {
  const long M = x.size(0), N = w.size(0);
  TORCH_CHECK(M >= 1 && M <= 64 && N % 2048 == 0 && N <= 8192 &&
              K % kdiv == 0);
  TORCH_CHECK(x.is_contiguous() && w.is_contiguous() &&
              residual.is_contiguous() && normed.is_contiguous());
}

template <int MT, bool SPLIT, int KS, bool SILU>
static SkinnyKernel sk5_kernel(int tiles) {
  return tiles == 2 ? skinny5_kernel<MT, SPLIT, KS, SILU, 2>
                    : skinny5_kernel<MT, SPLIT, KS, SILU, 1>;
}

void skinny_gemm(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                 torch::Tensor ws) {
  check_plain(out, x, w, 64, 32);
  const SkinnyPlan p = plan_v1(x.size(0), w.size(0), x.size(1));
  SkinnyKernel direct = nullptr, split = nullptr;
  with_mt(p.MT, [&](auto mt) {
    constexpr int MT = decltype(mt)::value;
    direct = skinny_gemm_kernel<MT, false>;
    split = skinny_gemm_kernel<MT, true>;
  });
  run_reduce(p, bf16_gemm(p, direct, split, x, w), out, ws);
}

void skinny_gemm_fused_norm(torch::Tensor normed, torch::Tensor x,
                            torch::Tensor w, torch::Tensor ws,
                            torch::Tensor residual, torch::Tensor nw,
                            double eps) {
  check_fused(normed, x, w, residual, x.size(1), 32);
  const SkinnyPlan p = plan_v1(x.size(0), w.size(0), x.size(1));
  SkinnyKernel split = nullptr;
  with_mt(p.MT, [&](auto mt) {
    split = skinny_gemm_kernel<decltype(mt)::value, true>;
  });
  run_reduce_add_rmsnorm(p, bf16_gemm(p, nullptr, split, x, w), normed, ws,
                         residual, nw, eps);
}

void skinny_gemm2(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                  torch::Tensor ws) {
  check_plain(out, x, w, 128, KSLICE);
  const SkinnyPlan p = plan_v2(x.size(0), w.size(0), x.size(1));
  SkinnyKernel direct = nullptr, split = nullptr;
  with_mt(p.MT, [&](auto mt) {
    constexpr int MT = decltype(mt)::value;
    direct = skinny2_kernel<MT, false>;
    split = skinny2_kernel<MT, true>;
  });
  run_reduce(p, bf16_gemm(p, direct, split, x, w), out, ws);
}

void skinny_gemm5(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                  torch::Tensor ws) {
  const int KS = ks_from_env("KUKEON_SK5_KS");
  const int tiles = sk5_tiles();
  check_plain(out, x, w, 128, KS);
  const SkinnyPlan p = plan_v5(x.size(0), w.size(0), x.size(1), tiles, KS);
  SkinnyKernel direct = nullptr, split = nullptr;
  with_mt(p.MT, [&](auto mt) {
    constexpr int MT = decltype(mt)::value;
    if (KS == 128) {
      direct = sk5_kernel<MT, false, 128, false>(tiles);
      split = sk5_kernel<MT, true, 128, false>(tiles);
    } else {
      direct = sk5_kernel<MT, false, 256, false>(tiles);
      split = sk5_kernel<MT, true, 256, false>(tiles);
    }
  });
  run_reduce(p, bf16_gemm(p, direct, split, x, w), out, ws);
}

// skinny5 + the split-K reduce fused with residual add + RMSNorm: the
// decode down-projection epilogue in ONE kernel instead of reduce + norm
// (two ~4.5us in-graph launches).
void skinny_gemm5_fused_norm(torch::Tensor normed, torch::Tensor x,
                             torch::Tensor w, torch::Tensor ws,
                             torch::Tensor residual, torch::Tensor nw,
                             double eps) {
  check_fused(normed, x, w, residual, x.size(1), 128);
  const int tiles = sk5_tiles();
  const SkinnyPlan p = plan_v5(x.size(0), w.size(0), x.size(1), tiles, 128);
  SkinnyKernel split = nullptr;
  with_mt(p.MT, [&](auto mt) {
    split = sk5_kernel<decltype(mt)::value, true, 128, false>(tiles);
  });
  run_reduce_add_rmsnorm(p, bf16_gemm(p, nullptr, split, x, w), normed, ws,
                         residual, nw, eps);
}

// The whole decode MLP tail in two kernels: silu(gate)*up happens in
// registers inside the down-projection's x staging (SILU template path),
// and the split-K reduce fuses with the next layer's residual add +
// RMSNorm. Measured SLOWER than silu_mul + skinny_gemm5 in situ (54.2 vs
// 42.9 us cold — doubling the x-staging bytes beats the saved launch;
// ledger profiles/r02_progress.md) so dispatch is off by default
// (KUKEON_FUSE_SILU=1 re-enables); kept as the documented negative result.
void skinny_gemm5_silu_fused_norm(torch::Tensor normed, torch::Tensor gu,
                                  torch::Tensor w, torch::Tensor ws,
                                  torch::Tensor residual, torch::Tensor nw,
                                  double eps) {
  check_fused(normed, gu, w, residual, w.size(1), 128);
  TORCH_CHECK(gu.size(1) == 2 * w.size(1), "gate_up output must be [M, 2K]");
  TORCH_CHECK(gu.scalar_type() == torch::kBFloat16);
  const int tiles = sk5_tiles();
  const SkinnyPlan p = plan_v5(gu.size(0), w.size(0), w.size(1), tiles, 128);
  SkinnyKernel split = nullptr;
  with_mt(p.MT, [&](auto mt) {
    split = sk5_kernel<decltype(mt)::value, true, 128, true>(tiles);
  });
  run_reduce_add_rmsnorm(p, bf16_gemm(p, nullptr, split, gu, w), normed, ws,
                         residual, nw, eps);
}

void skinny_gemm6(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                  torch::Tensor ws) {
  const int KS = ks_from_env("KUKEON_SK6_KS");
  check_plain(out, x, w, 128, KS);
  const SkinnyPlan p = plan_v6(x.size(0), w.size(0), x.size(1), KS);
  SkinnyKernel direct = nullptr, split = nullptr;
  with_mt(p.MT, [&](auto mt) {
    constexpr int MT = decltype(mt)::value;
    if (KS == 128) {
      direct = skinny6_kernel<MT, false, 128>;
      split = skinny6_kernel<MT, true, 128>;
    } else {
      direct = skinny6_kernel<MT, false, 256>;
      split = skinny6_kernel<MT, true, 256>;
    }
  });
  run_reduce(p, bf16_gemm(p, direct, split, x, w), out, ws);
}

// ---- W8A16 entry points: fp8 weight bytes + per-row scales ----
static void check_w8(const torch::Tensor& x, const torch::Tensor& q,
                     const torch::Tensor& scale) {
  TORCH_CHECK(x.dim() == 2 && q.dim() == 2 && x.size(1) == q.size(1),
              "skinny gemm w8: x [M, K] and q [N, K]");
  TORCH_CHECK(q.size(0) % 64 == 0 && q.size(1) % 64 == 0,
              "skinny gemm w8: N%64, K%64");
  TORCH_CHECK(q.scalar_type() == torch::kUInt8 &&
              scale.scalar_type() == torch::kFloat32 &&
              x.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(scale.numel() == q.size(0) && scale.is_contiguous() &&
              q.is_contiguous());
  TORCH_CHECK(x.is_cuda() && q.is_cuda() && scale.is_cuda());
}

static auto w8_gemm(const SkinnyPlan& p, const torch::Tensor& x,
                    const torch::Tensor& q, const torch::Tensor& scale) {
  return [=, &p](bool is_split, unsigned short* out, float* ws, dim3 grid,
                 hipStream_t stream) {
    const unsigned char* qp = q.data_ptr<unsigned char>();
    const float* sp = scale.data_ptr<float>();
    with_mt(p.MT, [&](auto mt) {
      constexpr int MT = decltype(mt)::value;
      if (is_split) {
        skinny_w8_kernel<MT, true><<<grid, 256, 0, stream>>>(
            out, ws, us_ptr(x), qp, sp, p.M, p.N, p.K);
      } else {
        skinny_w8_kernel<MT, false><<<grid, 256, 0, stream>>>(
            out, ws, us_ptr(x), qp, sp, p.M, p.N, p.K);
      }
    });
  };
}

void skinny_gemm_w8(torch::Tensor out, torch::Tensor x, torch::Tensor q,
                    torch::Tensor scale, torch::Tensor ws) {
  check_w8(x, q, scale);
  check_plain(out, x, q, 64, 64);
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16 &&
              out.numel() == x.size(0) * q.size(0));
  const SkinnyPlan p = plan_w8(x.size(0), q.size(0), x.size(1));
  run_reduce(p, w8_gemm(p, x, q, scale), out, ws);
}

void skinny_gemm_w8_fused_norm(torch::Tensor normed, torch::Tensor x,
                               torch::Tensor q, torch::Tensor scale,
                               torch::Tensor ws, torch::Tensor residual,
                               torch::Tensor nw, double eps) {
  check_w8(x, q, scale);
  check_fused(normed, x, q, residual, x.size(1), 64);
  TORCH_CHECK(normed.numel() == x.size(0) * q.size(0) &&
              residual.numel() == normed.numel() &&
              nw.numel() == q.size(0));
  const SkinnyPlan p = plan_w8(x.size(0), q.size(0), x.size(1));
  run_reduce_add_rmsnorm(p, w8_gemm(p, x, q, scale), normed, ws, residual,
                         nw, eps);
}

// ---- W4A16 entry points: MXFP4 codes + per-block e8m0 scales ----
static void check_w4(const torch::Tensor& x, const torch::Tensor& q,
                     const torch::Tensor& scale) {
  TORCH_CHECK(x.dim() == 2 && q.dim() == 2 && scale.dim() == 2 &&
              x.size(1) == 2 * q.size(1) &&
              scale.size(0) == q.size(0) && x.size(1) == 32 * scale.size(1),
              "skinny gemm w4: x [M, K], q [N, K/2], scale [N, K/32]");
  TORCH_CHECK(q.size(0) % 64 == 0 && x.size(1) % 128 == 0,
              "skinny gemm w4: N%64, K%128");
  TORCH_CHECK(q.scalar_type() == torch::kUInt8 &&
              scale.scalar_type() == torch::kUInt8 &&
              x.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(scale.is_contiguous() && q.is_contiguous());
  TORCH_CHECK((uintptr_t)q.data_ptr() % 16 == 0 &&
              (uintptr_t)scale.data_ptr() % 4 == 0,
              "skinny gemm w4: q 16-byte and scale 4-byte aligned");
  TORCH_CHECK(x.is_cuda() && q.is_cuda() && scale.is_cuda());
}

static auto w4_gemm(const SkinnyPlan& p, const torch::Tensor& x,
                    const torch::Tensor& q, const torch::Tensor& scale) {
  return [=, &p](bool is_split, unsigned short* out, float* ws, dim3 grid,
                 hipStream_t stream) {
    const unsigned char* qp = q.data_ptr<unsigned char>();
    const unsigned char* sp = scale.data_ptr<unsigned char>();
    with_mt(p.MT, [&](auto mt) {
      constexpr int MT = decltype(mt)::value;
      if (is_split) {
        skinny_w4_kernel<MT, true><<<grid, 256, 0, stream>>>(
            out, ws, us_ptr(x), qp, sp, p.M, p.N, p.K);
      } else {
        skinny_w4_kernel<MT, false><<<grid, 256, 0, stream>>>(
            out, ws, us_ptr(x), qp, sp, p.M, p.N, p.K);
      }
    });
  };
}

void skinny_gemm_w4(torch::Tensor out, torch::Tensor x, torch::Tensor q,
                    torch::Tensor scale, torch::Tensor ws) {
  check_w4(x, q, scale);
  check_plain(out, x, q, 64, 128);
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16 &&
              out.numel() == x.size(0) * q.size(0));
  const SkinnyPlan p = plan_w4(x.size(0), q.size(0), x.size(1));
  run_reduce(p, w4_gemm(p, x, q, scale), out, ws);
}

void skinny_gemm_w4_fused_norm(torch::Tensor normed, torch::Tensor x,
                               torch::Tensor q, torch::Tensor scale,
                               torch::Tensor ws, torch::Tensor residual,
                               torch::Tensor nw, double eps) {
  check_w4(x, q, scale);
  check_fused(normed, x, q, residual, x.size(1), 128);
  TORCH_CHECK(normed.numel() == x.size(0) * q.size(0) &&
              residual.numel() == normed.numel() &&
              nw.numel() == q.size(0));
  const SkinnyPlan p = plan_w4(x.size(0), q.size(0), x.size(1));
  run_reduce_add_rmsnorm(p, w4_gemm(p, x, q, scale), normed, ws, residual,
                         nw, eps);
}

}  // namespace kukeon
