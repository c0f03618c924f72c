// Grouped-GEMM MoE path for gfx950: device-side routing + one GEMM launch
// for all experts (Mixtral, T > 128).
//
//   moe_route_sort   softmax top-k routing AND the stable expert sort in one
//                    single-workgroup pass — no host read, so the layer's
//                    launch shapes never depend on the routing and the whole
//                    MoE is hipGraph-capturable at any T.
//   moe_grouped_gemm out[r,:] = a[a_rows[r],:] @ w[e].T for the rows r of
//                    expert e, whose range [offsets[e], offsets[e+1]) is read
//                    from device memory. Flat work queue: a fixed grid walks
//                    (n-block, m-block) tiles with a static stride, no
//                    atomics, so results are bit-identical run to run.
#include "common.h"
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

namespace kukeon {

namespace {

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short gg_bf16x8_t;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float gg_f32x4_t;
typedef __attribute__((__vector_size__(4 * sizeof(unsigned int))))
    unsigned int gg_u32x4_t;

constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / WAVE;
constexpr int RS_MAX_E = 32;
constexpr int RS_MAX_K = 4;

}  // namespace

// One workgroup. Pass 1: each thread routes tokens tid, tid+256, ... —
// top-k by repeated max on the RAW logits (strict >, so ties go to the lowest
// expert id, independent of __expf rounding), softmax over the picked logits
// only (equals softmax-then-renormalise: the full denominator cancels). The
// picked ids are parked in inv_map and counted per expert. Pass 2 walks the
// tokens in chunks of 256 in order; a token holds each expert at most once,
// so the stable rank of pair (t, j) inside expert e is the number of earlier
// tokens that picked e: running count + earlier waves' totals + ballot
// prefix inside the wave. Pass 2 re-reads only what the same thread wrote.
__global__ __launch_bounds__(RS_THREADS) void moe_route_sort_kernel(
    float* __restrict__ topk_w,   // [T,K]
    int* __restrict__ row_map,    // [T*K]
    int* __restrict__ inv_map,    // [T,K]
    int* __restrict__ offsets,    // [E+1]
    const void* __restrict__ logits, int T, int E, int K, bool bf16_in) {
  __shared__ int cnt[RS_MAX_E];
  __shared__ int run[RS_MAX_E];
  __shared__ int wtot[RS_WAVES][RS_MAX_E];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  if (tid < RS_MAX_E) cnt[tid] = 0;
  __syncthreads();

  for (int t = tid; t < T; t += RS_THREADS) {
    float l[RS_MAX_E];
    for (int e = 0; e < E; ++e) {
      l[e] = bf16_in
          ? us2f(reinterpret_cast<const unsigned short*>(
                logits)[(long)t * E + e])
          : reinterpret_cast<const float*>(logits)[(long)t * E + e];
    }
    unsigned taken = 0u;
    float vals[RS_MAX_K];
    int ids[RS_MAX_K];
#pragma unroll
    for (int k = 0; k < RS_MAX_K; ++k) {
      if (k >= K) break;
      // start from the lowest untaken expert so a NaN row still yields
      // K distinct in-range ids
      int bi = __ffs(~taken) - 1;
      float bv = l[bi];
      for (int e = bi + 1; e < E; ++e) {
        if (!((taken >> e) & 1u) && l[e] > bv) { bv = l[e]; bi = e; }
      }
      taken |= 1u << bi;
      ids[k] = bi;
      vals[k] = bv;
    }
    float ex[RS_MAX_K];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < RS_MAX_K; ++k) {
      if (k >= K) break;
      ex[k] = __expf(vals[k] - vals[0]);   // vals[0] is the max
      sum += ex[k];
    }
#pragma unroll
    for (int k = 0; k < RS_MAX_K; ++k) {
      if (k >= K) break;
      topk_w[(long)t * K + k] = ex[k] / sum;
      inv_map[(long)t * K + k] = ids[k];
      atomicAdd(&cnt[ids[k]], 1);   // LDS; counts are order-independent
    }
  }
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int e = 0; e < E; ++e) {
      offsets[e] = acc;
      run[e] = acc;
      acc += cnt[e];
    }
    offsets[E] = acc;
  }
  __syncthreads();

  const unsigned long long below = (1ull << lane) - 1ull;
  for (int base = 0; base < T; base += RS_THREADS) {
    const int t = base + tid;
    const bool valid = t < T;
    int ids[RS_MAX_K];
    int pre[RS_MAX_K];
    unsigned sel = 0u;
#pragma unroll
    for (int k = 0; k < RS_MAX_K; ++k) {
      ids[k] = (valid && k < K) ? inv_map[(long)t * K + k] : -1;
      pre[k] = 0;
      if (ids[k] >= 0) sel |= 1u << ids[k];
    }
    for (int e = 0; e < E; ++e) {
      const unsigned long long b = __ballot((sel >> e) & 1u);
      const int p = __popcll(b & below);
#pragma unroll
      for (int k = 0; k < RS_MAX_K; ++k)
        if (ids[k] == e) pre[k] = p;
      if (lane == 0) wtot[wid][e] = __popcll(b);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < RS_MAX_K; ++k) {
      if (ids[k] < 0) continue;
      int slot = run[ids[k]] + pre[k];
      for (int w = 0; w < wid; ++w) slot += wtot[w][ids[k]];
      row_map[slot] = t;
      inv_map[(long)t * K + k] = slot;
    }
    __syncthreads();
    if (tid < E) {
      int s = 0;
#pragma unroll
      for (int w = 0; w < RS_WAVES; ++w) s += wtot[w][tid];
      run[tid] += s;
    }
    __syncthreads();
  }
}

void moe_route_sort(torch::Tensor topk_w, torch::Tensor row_map,
                    torch::Tensor inv_map, torch::Tensor offsets,
                    torch::Tensor logits, long K) {
  TORCH_CHECK(logits.dim() == 2);
  const long T = logits.size(0);
  const int E = logits.size(1);
  const bool bf16_in = logits.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(E >= 1 && E <= RS_MAX_E && K >= 1 && K <= RS_MAX_K && K <= E);
  TORCH_CHECK(bf16_in || logits.scalar_type() == torch::kFloat32);
  TORCH_CHECK(topk_w.scalar_type() == torch::kFloat32);
  TORCH_CHECK(row_map.scalar_type() == torch::kInt32 &&
              inv_map.scalar_type() == torch::kInt32 &&
              offsets.scalar_type() == torch::kInt32);
  TORCH_CHECK(topk_w.numel() == T * K && row_map.numel() == T * K &&
              inv_map.numel() == T * K && offsets.numel() == E + 1);
  TORCH_CHECK(T * K < (1L << 31));
  TORCH_CHECK(logits.is_contiguous() && topk_w.is_contiguous() &&
              row_map.is_contiguous() && inv_map.is_contiguous() &&
              offsets.is_contiguous());
  if (T == 0) return;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  moe_route_sort_kernel<<<dim3(1), RS_THREADS, 0, stream>>>(
      topk_w.data_ptr<float>(), row_map.data_ptr<int>(),
      inv_map.data_ptr<int>(), offsets.data_ptr<int>(), logits.data_ptr(),
      (int)T, E, (int)K, bf16_in);
  HIP_CHECK_KERNEL();
}

// ---------------------------------------------------------------------------
// Grouped GEMM. Tile = up to GG_BM rows of ONE expert x GG_BN output columns;
// the k loop runs in GG_BK stages. 4 waves; wave v owns W rows (output
// columns) [n0 + 16v, +16) for all tile rows (one 16x16 accumulator per 16
// rows; 16-row groups past the expert's range are skipped).
//   * W is the MFMA A operand and streams global -> registers in fragment
//     shape with nontemporal 16 B/lane loads through a ring of GG_WD
//     register sets, issued GG_WD stages ahead of their use; each W byte
//     is read once per m-block.
//   * the activation tile is gathered through a_rows on its way into a
//     double-buffered, XOR-swizzled LDS image (one barrier per stage) and
//     read back as the B operand with conflict-free 16 B reads. Rows past
//     the expert's range are never read, k past Kd is staged as zeros.
//     The activation loads run GG_AD stages ahead through registers.
//   * D[row = 4*(lane>>4)+r -> n][col = lane&15 -> m]: each lane stores 4
//     consecutive bf16 of one output row, masked to the expert's range.
// The m-blocks of all experts form one flat list (expert e contributes
// ceil(cnt_e/GG_BM)); its length is data-dependent but at most
// ceil(R/GG_BM) + E, which sizes the walk. Tile id = nb * mb_max + mbg, so
// neighbouring workgroups work on the same W column block.
// ---------------------------------------------------------------------------
constexpr int GG_BM = 128;
constexpr int GG_BN = 64;
constexpr int GG_BK = 128;
constexpr int GG_MT = GG_BM / 16;
constexpr int GG_KC = GG_BK / 32;          // 32-wide k chunks per stage
constexpr int GG_ACH = GG_BM * GG_BK / 8 / 256;  // 16-B A chunks per thread
constexpr int GG_WD = 4;                   // W register sets (ring depth)
constexpr int GG_AD = 2;                   // activation register sets

DEV_INLINE int gg_swz(int row, int byte_in_row) {
  return row * (GG_BK * 2) + (byte_in_row ^ ((row & 15) << 4));
}

// One tile's k loop + store, specialised on the number of live 16-row
// groups so the loop body is branch-free: every load is unconditional on a
// clamped (always in-bounds) address and tails are zeroed by selects at the
// point of use, which lets hipcc keep counted vmcnt waits instead of
// draining the W ring at every join. Rows past `rows` hold a clamped
// duplicate row: they only reach output rows the store masks. Stages are
// padded to a multiple of GG_WD; padded stages multiply zeros.
template <int MTU>
DEV_INLINE void gg_tile(unsigned short* __restrict__ out,
                        const unsigned short* __restrict__ a,
                        const unsigned short* __restrict__ wrow,
                        unsigned short (*abuf)[GG_BM * GG_BK],
                        const int (&asrc)[GG_ACH], int r0, int rows, int n0,
                        int N, int Kd) {
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int row16 = lane & 15;
  const int kgrp = lane >> 4;
  // A staging: chunk c = tid + 256*i -> tile row c/16, 16-B column c%16;
  // only the 16-row groups this specialisation computes are staged
  constexpr int ACH = MTU;
  const int arow0 = tid >> 4;
  const int acol = (tid & 15) * 8;   // elements
  const int nstages = ((Kd + GG_BK - 1) / GG_BK + GG_WD - 1) / GG_WD * GG_WD;

  gg_f32x4_t acc[MTU];
#pragma unroll
  for (int m = 0; m < MTU; ++m) acc[m] = gg_f32x4_t{0.f, 0.f, 0.f, 0.f};

  uint4 ar0[ACH], ar1[ACH];
  gg_u32x4_t wr0[GG_KC], wr1[GG_KC], wr2[GG_KC], wr3[GG_KC];
  auto load_a = [&](uint4 (&ar)[ACH], int s) {
    const int k = min(s * GG_BK + acol, Kd - 8);
#pragma unroll
    for (int i = 0; i < ACH; ++i)
      ar[i] = *reinterpret_cast<const uint4*>(a + (long)asrc[i] * Kd + k);
  };
  auto load_w = [&](gg_u32x4_t (&wr)[GG_KC], int s) {
#pragma unroll
    for (int u = 0; u < GG_KC; ++u) {
      const int k = min(s * GG_BK + u * 32, Kd - 32);
      wr[u] = __builtin_nontemporal_load(
          reinterpret_cast<const gg_u32x4_t*>(wrow + k));
    }
  };
  // one k stage: `wr` holds W(s) on entry and W(s + GG_WD) on exit, `ar`
  // the activations of stage s on entry and of stage s + GG_AD on exit
  auto stage = [&](gg_u32x4_t (&wr)[GG_KC], uint4 (&ar)[ACH], int s) {
    unsigned short* ab = abuf[s & 1];
    const bool a_live = s * GG_BK + acol < Kd;
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
      uint4 v = ar[i];
      if (!a_live) v = uint4{0u, 0u, 0u, 0u};
      *reinterpret_cast<uint4*>(reinterpret_cast<char*>(ab) +
                                gg_swz(arow0 + 16 * i, acol * 2)) = v;
    }
    // vmcnt retires in order: the wait for stage s+1's activations at the
    // top of the next stage covers everything issued before them, so the
    // activations run GG_AD stages ahead and W two more — only the loads
    // younger than activations(s+1) stay in flight across that wait
    load_a(ar, s + GG_AD);
    gg_bf16x8_t wf[GG_KC];
#pragma unroll
    for (int u = 0; u < GG_KC; ++u) {
      gg_u32x4_t v = wr[u];
      if (s * GG_BK + u * 32 >= Kd) v = gg_u32x4_t{0u, 0u, 0u, 0u};
      wf[u] = __builtin_bit_cast(gg_bf16x8_t, v);
    }
    load_w(wr, s + GG_WD);
    // buffer (s&1) was last read in stage s-2, which every wave left
    // before it arrived at stage s-1's barrier: one barrier per stage
    __syncthreads();
#pragma unroll
    for (int u = 0; u < GG_KC; ++u) {
      const int kb = (u * 32 + 8 * kgrp) * 2;
#pragma unroll
      for (int m = 0; m < MTU; ++m) {
        const uint4 xv = *reinterpret_cast<const uint4*>(
            reinterpret_cast<const char*>(ab) + gg_swz(m * 16 + row16, kb));
        acc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            wf[u], __builtin_bit_cast(gg_bf16x8_t, xv), acc[m], 0, 0, 0);
      }
    }
  };

  load_w(wr0, 0);
  load_w(wr1, 1);
  load_a(ar0, 0);
  load_w(wr2, 2);
  load_a(ar1, 1);
  load_w(wr3, 3);
  for (int s = 0; s < nstages; s += GG_WD) {
    stage(wr0, ar0, s);
    stage(wr1, ar1, s + 1);
    stage(wr2, ar0, s + 2);
    stage(wr3, ar1, s + 3);
  }

  const int ncol = n0 + 4 * kgrp;
#pragma unroll
  for (int m = 0; m < MTU; ++m) {
    const int tr = m * 16 + row16;
    if (tr >= rows) continue;
    uint2 v;
    v.x = (unsigned)f2us(acc[m][0]) | ((unsigned)f2us(acc[m][1]) << 16);
    v.y = (unsigned)f2us(acc[m][2]) | ((unsigned)f2us(acc[m][3]) << 16);
    *reinterpret_cast<uint2*>(out + (long)(r0 + tr) * N + ncol) = v;
  }
}

__global__ __launch_bounds__(256, 2) void moe_grouped_gemm_kernel(
    unsigned short* __restrict__ out,        // [R, N]
    const unsigned short* __restrict__ a,    // [Ta, Kd]
    const int* __restrict__ a_rows,          // [R] or nullptr (identity)
    const unsigned short* __restrict__ w,    // [E, N, Kd]
    const int* __restrict__ offsets,         // [E+1]
    int R, int Ta, int N, int Kd, int E, int mb_max, long n_tiles) {
  __shared__ __align__(16) unsigned short abuf[2][GG_BM * GG_BK];
  const int tid = threadIdx.x;
  const int wid = tid / WAVE;
  const int row16 = tid & 15;
  const int kgrp = (tid & (WAVE - 1)) >> 4;
  const int arow0 = tid >> 4;

  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int mbg = (int)(tile % mb_max);
    const int nb = (int)(tile / mb_max);
    // flat m-block index -> (expert, first row, row count)
    int e = -1, r0 = 0, rows = 0;
    {
      int seen = 0;
      for (int i = 0; i < E; ++i) {
        const int lo = max(offsets[i], 0);
        const int hi = min(offsets[i + 1], R);
        const int nblk = hi > lo ? (hi - lo + GG_BM - 1) / GG_BM : 0;
        if (e < 0 && mbg < seen + nblk) {
          e = i;
          r0 = lo + (mbg - seen) * GG_BM;
          rows = min(GG_BM, hi - r0);
        }
        seen += nblk;
      }
    }
    if (e < 0) continue;   // past the end of the data-dependent list

    const int n0 = nb * GG_BN + wid * 16;
    const unsigned short* wrow =
        w + ((long)e * N + n0 + row16) * Kd + 8 * kgrp;
    // source rows of this thread's A chunks; tile rows past the expert's
    // range re-read its last row (in bounds, never stored)
    int asrc[GG_ACH];
#pragma unroll
    for (int i = 0; i < GG_ACH; ++i) {
      const int tr = min(arow0 + 16 * i, rows - 1);
      const int src = a_rows ? a_rows[r0 + tr] : r0 + tr;
      asrc[i] = min(max(src, 0), Ta - 1);
    }

    // every wave is done reading both LDS buffers of the previous tile
    __syncthreads();
    if (rows <= 32) {
      gg_tile<2>(out, a, wrow, abuf, asrc, r0, rows, n0, N, Kd);
    } else if (rows <= 64) {
      gg_tile<4>(out, a, wrow, abuf, asrc, r0, rows, n0, N, Kd);
    } else {
      gg_tile<8>(out, a, wrow, abuf, asrc, r0, rows, n0, N, Kd);
    }
  }
}

void moe_grouped_gemm(torch::Tensor out, torch::Tensor a,
                      torch::Tensor a_rows, torch::Tensor w,
                      torch::Tensor offsets) {
  TORCH_CHECK(out.dim() == 2 && a.dim() == 2 && w.dim() == 3);
  const long R = out.size(0);
  const long N = out.size(1);
  const long Ta = a.size(0);
  const long Kd = a.size(1);
  const long E = w.size(0);
  TORCH_CHECK(w.size(1) == N && w.size(2) == Kd,
              "moe_grouped_gemm: w must be [E, N, Kd]");
  TORCH_CHECK(N % 64 == 0 && Kd % 64 == 0,
              "moe_grouped_gemm: N % 64 == 0 and Kd % 64 == 0 required");
  TORCH_CHECK(out.scalar_type() == torch::kBFloat16 &&
              a.scalar_type() == torch::kBFloat16 &&
              w.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(offsets.scalar_type() == torch::kInt32 &&
              offsets.numel() == E + 1);
  TORCH_CHECK(out.is_contiguous() && a.is_contiguous() &&
              w.is_contiguous() && offsets.is_contiguous());
  TORCH_CHECK(out.is_cuda() && a.is_cuda() && w.is_cuda() &&
              offsets.is_cuda());
  const bool gather = a_rows.defined() && a_rows.numel() > 0;
  if (gather) {
    TORCH_CHECK(a_rows.scalar_type() == torch::kInt32 &&
                a_rows.numel() == R && a_rows.is_contiguous() &&
                a_rows.is_cuda());
  } else {
    TORCH_CHECK(Ta >= R, "moe_grouped_gemm: identity rows need a >= out");
  }
  TORCH_CHECK(R < (1L << 31) && Ta < (1L << 31) && E >= 1 && E <= 1024);
  if (R == 0) return;
  TORCH_CHECK(Ta >= 1);
  const long mb_max = (R + GG_BM - 1) / GG_BM + E;
  const long n_tiles = mb_max * (N / GG_BN);
  // fixed grid from the shapes only: 8 workgroups for each of the MI355X's
  // 256 CUs (two are resident at 64 KiB LDS each); longer tile lists are walked with a static
  // stride
  const long grid = std::min(n_tiles, 256L * 8);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  moe_grouped_gemm_kernel<<<dim3((unsigned)grid), 256, 0, stream>>>(
      reinterpret_cast<unsigned short*>(out.data_ptr()),
      reinterpret_cast<const unsigned short*>(a.data_ptr()),
      gather ? a_rows.data_ptr<int>() : nullptr,
      reinterpret_cast<const unsigned short*>(w.data_ptr()),
      offsets.data_ptr<int>(), (int)R, (int)Ta, (int)N, (int)Kd, (int)E,
      (int)mb_max, n_tiles);
  HIP_CHECK_KERNEL();
}

}  // namespace kukeon
