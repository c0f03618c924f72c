// MXFP4 weight format (ops.Mxfp4Weight): q[N, K/2] holds two OCP e2m1
// codes per byte (element 2j in the low nibble, 2j+1 in the high one) and
// scale[N, K/32] one e8m0 byte per block of 32 along K; the weight is
// value(code) * 2^(scale - 127). quantize_mxfp4_rows runs once per weight
// at load and matches reference.quantize_mxfp4_rows bit for bit;
// dequant_mxfp4_rows feeds the wide-M path, which widens a weight to bf16
// scratch and hands it to the library GEMM. The decode path never
// dequantises to memory (skinny_gemm.hip, W4A16).
#include "common.h"
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

namespace kukeon {

// One thread per 8 elements, so the 4 neighbouring lanes of a wave hold
// one 32-element block and its amax is two xor-shuffles. Everything that
// decides a bit is integer or exact: amax is taken on the bf16 magnitude
// bits (they order like the values), the scale byte is amax's exponent
// field - 2 clamped to [1, 254] (127 for a zero block; the field never
// exceeds 255, so the byte never exceeds 253 and 2^(127 - byte) is a
// normal f32), and |w| * 2^(127 - byte) is an exact product compared
// against the grid's midpoints: > where the tie goes down to the even
// code, >= where it goes up to it.
__global__ __launch_bounds__(256) void quantize_mxfp4_rows_kernel(
    unsigned int* __restrict__ q, unsigned char* __restrict__ scale,
    const unsigned short* __restrict__ w, long groups) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  // groups % 4 == 0 and a wave starts at a multiple of 64: the 4 lanes
  // of a block are in range together, and the rest only shuffle zeros
  const bool live = g < groups;
  bf16x8 v;
  v.raw = live ? *reinterpret_cast<const uint4*>(w + g * 8)
               : uint4{0u, 0u, 0u, 0u};
  int amax = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) amax = max(amax, (int)(v.us(j) & 0x7fffu));
  amax = max(amax, __shfl_xor(amax, 1, WAVE));
  amax = max(amax, __shfl_xor(amax, 2, WAVE));
  if (!live) return;
  const int byte = amax == 0 ? 127 : min(254, max(1, (amax >> 7) - 2));
  const float inv = __builtin_bit_cast(float, (unsigned int)(254 - byte) << 23);
  unsigned int codes = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const unsigned int us = v.us(j);
    const float a = us2f((unsigned short)(us & 0x7fffu)) * inv;
    const unsigned int mag = (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) +
                             (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) +
                             (a > 5.0f);
    codes |= (mag | ((us >> 12) & 8u)) << (4 * j);
  }
  q[g] = codes;
  if ((g & 3) == 0) scale[g >> 2] = (unsigned char)byte;
}

// out[n, k] = bf16(value(code[n, k]) * 2^(scale[n, k / 32] - 127)); 8
// elements (one dword of codes) per thread. Rows are whole blocks, so
// the flat block index is the flat element index / 32.
__global__ __launch_bounds__(256) void dequant_mxfp4_rows_kernel(
    unsigned short* __restrict__ out, const unsigned int* __restrict__ q,
    const unsigned char* __restrict__ scale, long groups) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= groups) return;
  *reinterpret_cast<uint4*>(out + g * 8) =
      fp4x8_to_bf16x8(q[g], e8m0_to_f32(scale[g >> 2]));
}

static void check_mxfp4_weight(const torch::Tensor& q,
                               const torch::Tensor& scale,
                               const torch::Tensor& w) {
  TORCH_CHECK(w.dim() == 2 && q.dim() == 2 && scale.dim() == 2,
              "mxfp4 weight: q [N, K/2], scale [N, K/32], w [N, K]");
  const long N = w.size(0), K = w.size(1);
  TORCH_CHECK(N >= 1 && K >= 32 && K % 32 == 0, "mxfp4 weight: K%32");
  TORCH_CHECK(q.size(0) == N && q.size(1) == K / 2 && scale.size(0) == N &&
              scale.size(1) == K / 32,
              "mxfp4 weight: q [N, K/2], scale [N, K/32], w [N, K]");
  TORCH_CHECK(w.scalar_type() == torch::kBFloat16 &&
              q.scalar_type() == torch::kUInt8 &&
              scale.scalar_type() == torch::kUInt8);
  TORCH_CHECK(w.is_contiguous() && q.is_contiguous() &&
              scale.is_contiguous());
  TORCH_CHECK(w.is_cuda() && q.is_cuda() && scale.is_cuda());
  // the kernels move whole dwords of codes and 16-byte groups of bf16
  TORCH_CHECK((uintptr_t)q.data_ptr() % 4 == 0 &&
              (uintptr_t)w.data_ptr() % 16 == 0,
              "mxfp4 weight: q 4-byte and w 16-byte aligned");
}

void quantize_mxfp4_rows(torch::Tensor q, torch::Tensor scale,
                         torch::Tensor w) {
  check_mxfp4_weight(q, scale, w);
  const long groups = w.numel() / 8;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  quantize_mxfp4_rows_kernel<<<dim3((unsigned)((groups + 255) / 256)), 256, 0,
                               stream>>>(
      reinterpret_cast<unsigned int*>(q.data_ptr()),
      scale.data_ptr<unsigned char>(),
      reinterpret_cast<const unsigned short*>(w.data_ptr()), groups);
  HIP_CHECK_KERNEL();
}

void dequant_mxfp4_rows(torch::Tensor out, torch::Tensor q,
                        torch::Tensor scale) {
  check_mxfp4_weight(q, scale, out);
  const long groups = out.numel() / 8;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  dequant_mxfp4_rows_kernel<<<dim3((unsigned)((groups + 255) / 256)), 256, 0,
                              stream>>>(
      reinterpret_cast<unsigned short*>(out.data_ptr()),
      reinterpret_cast<const unsigned int*>(q.data_ptr()),
      scale.data_ptr<unsigned char>(), groups);
  HIP_CHECK_KERNEL();
}

}  // namespace kukeon
