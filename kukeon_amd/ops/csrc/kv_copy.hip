// Whole-block copies inside the paged KV caches for gfx950: the device side
// of a session fork, which gives each child its own copy of the parent's
// partially filled tail block.
//
// Caches are [L, NB, Hk, BS, D] of any element type; the kernel moves raw
// bytes, 16 per lane, so bf16 and fp8 caches share it. One launch does every
// layer, both caches and every (src, dst) pair: workgroup (i, 2*l + side)
// copies block src[i] of layer l to block dst[i]. A real cache has a layer
// stride near 4 GiB, so every byte offset is 64-bit.
//
// The same src may feed several pairs. Destinations are distinct and disjoint
// from the sources — the caller guarantees it, the kernel does not look.
#include "common.h"
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

namespace kukeon {

constexpr int KVC_THREADS = 256;

__global__ __launch_bounds__(KVC_THREADS) void kv_copy_blocks_kernel(
    unsigned char* k_cache, unsigned char* v_cache,
    const int* __restrict__ src, const int* __restrict__ dst,
    long num_blocks, long block_bytes) {
  const long s = src[blockIdx.x];
  const long d = dst[blockIdx.x];
  // a bad index must not become a wild store
  if (s < 0 || s >= num_blocks || d < 0 || d >= num_blocks) return;
  const long layer = blockIdx.y >> 1;
  unsigned char* cache = (blockIdx.y & 1) ? v_cache : k_cache;
  unsigned char* base = cache + layer * num_blocks * block_bytes;
  const uint4* from = reinterpret_cast<const uint4*>(base + s * block_bytes);
  uint4* to = reinterpret_cast<uint4*>(base + d * block_bytes);
  const int vecs = (int)(block_bytes / 16);
  constexpr int T = KVC_THREADS;
  int c = threadIdx.x;
  // four 16 B loads in flight per lane before the first store
  for (; c + 3 * T < vecs; c += 4 * T) {
    const uint4 r0 = from[c], r1 = from[c + T], r2 = from[c + 2 * T],
                r3 = from[c + 3 * T];
    to[c] = r0;
    to[c + T] = r1;
    to[c + 2 * T] = r2;
    to[c + 3 * T] = r3;
  }
  for (; c < vecs; c += T) to[c] = from[c];
}

void kv_copy_blocks(torch::Tensor k_cache, torch::Tensor v_cache,
                    torch::Tensor src, torch::Tensor dst) {
  TORCH_CHECK(k_cache.is_cuda() && v_cache.is_cuda() && src.is_cuda() &&
                  dst.is_cuda(),
              "kv_copy_blocks: tensors must be on the GPU");
  TORCH_CHECK(k_cache.dim() == 5, "kv_copy_blocks: caches are [L,NB,Hk,BS,D]");
  TORCH_CHECK(k_cache.is_contiguous() && v_cache.is_contiguous(),
              "kv_copy_blocks: caches must be contiguous");
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes() &&
                  k_cache.scalar_type() == v_cache.scalar_type(),
              "kv_copy_blocks: k_cache and v_cache differ in shape or dtype");
  TORCH_CHECK(src.scalar_type() == torch::kInt32 &&
                  dst.scalar_type() == torch::kInt32 && src.dim() == 1 &&
                  dst.dim() == 1 && src.is_contiguous() && dst.is_contiguous(),
              "kv_copy_blocks: src/dst must be contiguous 1-D int32");
  TORCH_CHECK(src.numel() == dst.numel(),
              "kv_copy_blocks: src and dst differ in length");
  const long n = src.numel();
  if (n == 0) return;
  const long L = k_cache.size(0);
  const long NB = k_cache.size(1);
  const long block_bytes = k_cache.size(2) * k_cache.size(3) *
                           k_cache.size(4) * (long)k_cache.element_size();
  TORCH_CHECK(block_bytes % 16 == 0 && block_bytes / 16 <= INT32_MAX,
              "kv_copy_blocks: block size must be a multiple of 16 bytes");
  TORCH_CHECK(2 * L <= 65535, "kv_copy_blocks: too many layers");
  auto stream = c10::hip::getCurrentHIPStream().stream();
  kv_copy_blocks_kernel<<<dim3((unsigned)n, (unsigned)(2 * L)), KVC_THREADS, 0,
                          stream>>>(
      reinterpret_cast<unsigned char*>(k_cache.data_ptr()),
      reinterpret_cast<unsigned char*>(v_cache.data_ptr()),
      src.data_ptr<int>(), dst.data_ptr<int>(), NB, block_bytes);
  HIP_CHECK_KERNEL();
}

}  // namespace kukeon
