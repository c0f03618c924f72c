// fp8 weight format: q[N,K] OCP e4m3fn bytes + one f32 scale per output
// row (ops.Fp8Weight). quantize_fp8_rows runs once per weight at load;
// dequant_fp8_rows feeds the wide-M path, which widens a weight to bf16
// scratch and hands it to the library GEMM. The decode path never
// dequantises to memory (skinny_gemm.hip, W8A16).
#include "common.h"
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

namespace kukeon {

constexpr float E4M3_MAX = 448.f;

// One block per row: amax in f32, scale = amax / 448 (1 for an all-zero
// row), q = rne_e4m3(w / scale) with true f32 divisions so the bytes and
// the scale match the CPU reference bit for bit. |w / scale| <= 448 up to
// one rounding of the quotient, and the clamp keeps that rounding from
// ever reaching the NaN encoding.
__global__ __launch_bounds__(256) void quantize_fp8_rows_kernel(
    unsigned char* __restrict__ q, float* __restrict__ scale,
    const unsigned short* __restrict__ w, long K) {
  __shared__ float red[16];
  const long row = blockIdx.x;
  const unsigned short* wr = w + row * K;
  float amax = 0.f;
  for (long k = (long)threadIdx.x * 8; k < K; k += 256 * 8) {
    const bf16x8 v = load_bf16x8(wr + k);
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(v.f(j)));
  }
  amax = block_reduce(amax, red, MaxOp{}, 0.f);
  const float s = amax > 0.f ? __fdiv_rn(amax, E4M3_MAX) : 1.f;
  if (threadIdx.x == 0) scale[row] = s;
  for (long k = (long)threadIdx.x * 8; k < K; k += 256 * 8) {
    const bf16x8 v = load_bf16x8(wr + k);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      f[j] = fminf(fmaxf(__fdiv_rn(v.f(j), s), -E4M3_MAX), E4M3_MAX);
    *reinterpret_cast<uint2*>(q + row * K + k) = pack_fp8x8(f);
  }
}

// out[n, k] = bf16(float(q[n, k]) * scale[n]): one f32 multiply, one
// round-to-nearest-even. 8 elements per thread.
__global__ __launch_bounds__(256) void dequant_fp8_rows_kernel(
    unsigned short* __restrict__ out, const unsigned char* __restrict__ q,
    const float* __restrict__ scale, long K, long groups) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= groups) return;
  const long e = g * 8;
  const float s = scale[e / K];
  const uint2 b = *reinterpret_cast<const uint2*>(q + e);
  const f32x2_cvt_t a0 = __builtin_amdgcn_cvt_pk_f32_fp8(b.x, false);
  const f32x2_cvt_t a1 = __builtin_amdgcn_cvt_pk_f32_fp8(b.x, true);
  const f32x2_cvt_t a2 = __builtin_amdgcn_cvt_pk_f32_fp8(b.y, false);
  const f32x2_cvt_t a3 = __builtin_amdgcn_cvt_pk_f32_fp8(b.y, true);
  const float f[8] = {a0[0] * s, a0[1] * s, a1[0] * s, a1[1] * s,
                      a2[0] * s, a2[1] * s, a3[0] * s, a3[1] * s};
  *reinterpret_cast<uint4*>(out + e) = pack_bf16x8(f);
}

static void check_fp8_weight(const torch::Tensor& q,
                             const torch::Tensor& scale,
                             const torch::Tensor& w) {
  TORCH_CHECK(w.dim() == 2 && q.dim() == 2 && q.size(0) == w.size(0) &&
              q.size(1) == w.size(1) && scale.numel() == w.size(0),
              "fp8 weight: q [N, K], scale [N], w [N, K]");
  TORCH_CHECK(w.size(0) >= 1 && w.size(1) >= 8 && w.size(1) % 8 == 0,
              "fp8 weight: K%8");
  TORCH_CHECK(w.scalar_type() == torch::kBFloat16 &&
              q.scalar_type() == torch::kUInt8 &&
              scale.scalar_type() == torch::kFloat32);
  TORCH_CHECK(w.is_contiguous() && q.is_contiguous() &&
              scale.is_contiguous());
  TORCH_CHECK(w.is_cuda() && q.is_cuda() && scale.is_cuda());
}

void quantize_fp8_rows(torch::Tensor q, torch::Tensor scale,
                       torch::Tensor w) {
  check_fp8_weight(q, scale, w);
  auto stream = c10::hip::getCurrentHIPStream().stream();
  quantize_fp8_rows_kernel<<<dim3((unsigned)w.size(0)), 256, 0, stream>>>(
      q.data_ptr<unsigned char>(), scale.data_ptr<float>(),
      reinterpret_cast<const unsigned short*>(w.data_ptr()), w.size(1));
  HIP_CHECK_KERNEL();
}

void dequant_fp8_rows(torch::Tensor out, torch::Tensor q,
                      torch::Tensor scale) {
  check_fp8_weight(q, scale, out);
  const long groups = q.numel() / 8;
  auto stream = c10::hip::getCurrentHIPStream().stream();
  dequant_fp8_rows_kernel<<<dim3((unsigned)((groups + 255) / 256)), 256, 0,
                            stream>>>(
      reinterpret_cast<unsigned short*>(out.data_ptr()),
      q.data_ptr<unsigned char>(), scale.data_ptr<float>(), q.size(1),
      groups);
  HIP_CHECK_KERNEL();
}

}  // namespace kukeon
