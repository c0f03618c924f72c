// Whole-block moves between the paged KV caches and a block-major staging
// buffer for gfx950: the device side of swapping an idle session's KV to host
// memory and back. The staging buffer is what a single copy to or from the
// pinned host pool moves; these kernels gather a session's scattered blocks
// into it (pack) and scatter them back (unpack).
//
// Caches are [L, NB, Hk, BS, D] of any element type and the staging buffer is
// [cap, 2, L, Hk, BS, D]: record i holds K (side 0) then V (side 1) of one
// block for all layers, contiguously. The kernels move raw bytes, 16 per
// lane, so bf16 and fp8 caches share them. One launch does every layer, both
// sides and every listed block: workgroup (i, 2*l + side) moves block
// blocks[i] of layer l. A real cache has a layer stride near 4 GiB and a
// record is 2 MiB on the 8B model, so every byte offset is 64-bit.
//
// The unpack destinations are distinct — the caller guarantees it, the
// kernel does not look.
#include "common.h"
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

namespace kukeon {

constexpr int KVS_THREADS = 256;

// four 16 B loads in flight per lane before the first store
__device__ __forceinline__ void kvs_move_block(const uint4* __restrict__ from,
                                               uint4* __restrict__ to,
                                               int vecs) {
  constexpr int T = KVS_THREADS;
  int c = threadIdx.x;
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

// byte offset of (record i, side, layer) in the staging buffer
__device__ __forceinline__ long kvs_record_offset(long i, long side,
                                                  long layer, long num_layers,
                                                  long block_bytes) {
  return ((i * 2 + side) * num_layers + layer) * block_bytes;
}

__global__ __launch_bounds__(KVS_THREADS) void kv_pack_blocks_kernel(
    const unsigned char* __restrict__ k_cache,
    const unsigned char* __restrict__ v_cache, const int* __restrict__ blocks,
    unsigned char* __restrict__ staging, long num_layers, long num_blocks,
    long block_bytes) {
  const long b = blocks[blockIdx.x];
  // a bad index must not become a wild load: skip the record
  if (b < 0 || b >= num_blocks) return;
  const long layer = blockIdx.y >> 1;
  const long side = blockIdx.y & 1;
  const unsigned char* cache = side ? v_cache : k_cache;
  const unsigned char* from =
      cache + (layer * num_blocks + b) * block_bytes;
  unsigned char* to = staging + kvs_record_offset(blockIdx.x, side, layer,
                                                  num_layers, block_bytes);
  kvs_move_block(reinterpret_cast<const uint4*>(from),
                 reinterpret_cast<uint4*>(to), (int)(block_bytes / 16));
}

__global__ __launch_bounds__(KVS_THREADS) void kv_unpack_blocks_kernel(
    const unsigned char* __restrict__ staging, unsigned char* k_cache,
    unsigned char* v_cache, const int* __restrict__ blocks, long num_layers,
    long num_blocks, long block_bytes) {
  const long b = blocks[blockIdx.x];
  // a bad index must not become a wild store: skip the record
  if (b < 0 || b >= num_blocks) return;
  const long layer = blockIdx.y >> 1;
  const long side = blockIdx.y & 1;
  unsigned char* cache = side ? v_cache : k_cache;
  unsigned char* to = cache + (layer * num_blocks + b) * block_bytes;
  const unsigned char* from =
      staging + kvs_record_offset(blockIdx.x, side, layer, num_layers,
                                  block_bytes);
  kvs_move_block(reinterpret_cast<const uint4*>(from),
                 reinterpret_cast<uint4*>(to), (int)(block_bytes / 16));
}

// Shared argument checks; -> block bytes. `op` names the caller in messages.
static long kvs_check(const char* op, const torch::Tensor& k_cache,
                      const torch::Tensor& v_cache,
                      const torch::Tensor& blocks,
                      const torch::Tensor& staging) {
  TORCH_CHECK(k_cache.is_cuda() && v_cache.is_cuda() && blocks.is_cuda() &&
                  staging.is_cuda(),
              op, ": tensors must be on the GPU");
  TORCH_CHECK(k_cache.device() == v_cache.device() &&
                  k_cache.device() == blocks.device() &&
                  k_cache.device() == staging.device(),
              op, ": tensors must be on one device");
  TORCH_CHECK(k_cache.dim() == 5, op, ": caches are [L,NB,Hk,BS,D]");
  TORCH_CHECK(k_cache.is_contiguous() && v_cache.is_contiguous(), op,
              ": caches must be contiguous");
  TORCH_CHECK(k_cache.sizes() == v_cache.sizes() &&
                  k_cache.scalar_type() == v_cache.scalar_type(),
              op, ": k_cache and v_cache differ in shape or dtype");
  TORCH_CHECK(staging.dim() == 6 && staging.size(1) == 2 &&
                  staging.size(2) == k_cache.size(0) &&
                  staging.size(3) == k_cache.size(2) &&
                  staging.size(4) == k_cache.size(3) &&
                  staging.size(5) == k_cache.size(4) &&
                  staging.scalar_type() == k_cache.scalar_type(),
              op, ": staging must be [cap,2,L,Hk,BS,D] matching the caches");
  TORCH_CHECK(staging.is_contiguous(), op, ": staging must be contiguous");
  TORCH_CHECK(blocks.scalar_type() == torch::kInt32 && blocks.dim() == 1 &&
                  blocks.is_contiguous(),
              op, ": blocks must be contiguous 1-D int32");
  TORCH_CHECK(blocks.numel() <= staging.size(0), op, ": ", blocks.numel(),
              " blocks exceed the staging capacity of ", staging.size(0));
  const long block_bytes = k_cache.size(2) * k_cache.size(3) *
                           k_cache.size(4) * (long)k_cache.element_size();
  TORCH_CHECK(block_bytes % 16 == 0 && block_bytes / 16 <= INT32_MAX, op,
              ": block size must be a multiple of 16 bytes");
  TORCH_CHECK(2 * k_cache.size(0) <= 65535, op, ": too many layers");
  return block_bytes;
}

void kv_pack_blocks(torch::Tensor k_cache, torch::Tensor v_cache,
                    torch::Tensor blocks, torch::Tensor staging) {
  const long block_bytes =
      kvs_check("kv_pack_blocks", k_cache, v_cache, blocks, staging);
  const long n = blocks.numel();
  if (n == 0) return;
  const long L = k_cache.size(0);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  kv_pack_blocks_kernel<<<dim3((unsigned)n, (unsigned)(2 * L)), KVS_THREADS, 0,
                          stream>>>(
      reinterpret_cast<const unsigned char*>(k_cache.data_ptr()),
      reinterpret_cast<const unsigned char*>(v_cache.data_ptr()),
      blocks.data_ptr<int>(),
      reinterpret_cast<unsigned char*>(staging.data_ptr()), L,
      k_cache.size(1), block_bytes);
  HIP_CHECK_KERNEL();
}

void kv_unpack_blocks(torch::Tensor staging, torch::Tensor k_cache,
                      torch::Tensor v_cache, torch::Tensor blocks) {
  const long block_bytes =
      kvs_check("kv_unpack_blocks", k_cache, v_cache, blocks, staging);
  const long n = blocks.numel();
  if (n == 0) return;
  const long L = k_cache.size(0);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  kv_unpack_blocks_kernel<<<dim3((unsigned)n, (unsigned)(2 * L)), KVS_THREADS,
                            0, stream>>>(
      reinterpret_cast<const unsigned char*>(staging.data_ptr()),
      reinterpret_cast<unsigned char*>(k_cache.data_ptr()),
      reinterpret_cast<unsigned char*>(v_cache.data_ptr()),
      blocks.data_ptr<int>(), L, k_cache.size(1), block_bytes);
  HIP_CHECK_KERNEL();
}

}  // namespace kukeon
