// MFMA fragment-layout probes: one wave computes a single C = A @ B through
// each bf16 MFMA shape the attention kernels use, loading A/B and storing C
// strictly by the lane maps documented in attn_frag.h. The GPU test suite
// compares against a plain matmul on asymmetric inputs, so a wrong map (or
// a transposed operand) cannot pass.
#include "attn_frag.h"
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

namespace kukeon {

// ---------- 32x32x16: C[32,32] = A[32,16] @ B[16,32] ----------
__global__ void mfma_probe_kernel(float* __restrict__ c,
                                  const unsigned short* __restrict__ a,
                                  const unsigned short* __restrict__ b) {
  const int lane = threadIdx.x & 63;
  const int hi = lane >> 5;
  const int rc = lane & 31;
  unsigned int areg[4], breg[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k0 = 8 * hi + 2 * i;
    areg[i] = (unsigned)a[rc * 16 + k0] | ((unsigned)a[rc * 16 + k0 + 1] << 16);
    breg[i] = (unsigned)b[k0 * 32 + rc] | ((unsigned)b[(k0 + 1) * 32 + rc] << 16);
  }
  f32x16_t acc = {};
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
      as_frag(areg[0], areg[1], areg[2], areg[3]),
      as_frag(breg[0], breg[1], breg[2], breg[3]), acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * hi;
    c[row * 32 + rc] = acc[r];
  }
}

// ---------- 16x16x32: C[16,16] = A[16,32] @ B[32,16] ----------
__global__ void mfma_probe16_kernel(float* __restrict__ c,
                                    const unsigned short* __restrict__ a,
                                    const unsigned short* __restrict__ b) {
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;     // k group
  const int rc = lane & 15;
  unsigned int areg[4], breg[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k0 = 8 * g + 2 * i;
    areg[i] = (unsigned)a[rc * 32 + k0] | ((unsigned)a[rc * 32 + k0 + 1] << 16);
    breg[i] = (unsigned)b[k0 * 16 + rc] | ((unsigned)b[(k0 + 1) * 16 + rc] << 16);
  }
  f32x4_t acc = {};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
      as_frag(areg[0], areg[1], areg[2], areg[3]),
      as_frag(breg[0], breg[1], breg[2], breg[3]), acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) c[(4 * g + r) * 16 + rc] = acc[r];
}

// ---------- 16x16x16: C[16,16] = A[16,16] @ B[16,16] ----------
__global__ void mfma_probe16k_kernel(float* __restrict__ c,
                                     const unsigned short* __restrict__ a,
                                     const unsigned short* __restrict__ b) {
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;
  const int rc = lane & 15;
  unsigned int ar[2], br[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int k0 = 4 * g + 2 * i;
    ar[i] = (unsigned)a[rc * 16 + k0] | ((unsigned)a[rc * 16 + k0 + 1] << 16);
    br[i] = (unsigned)b[k0 * 16 + rc] | ((unsigned)b[(k0 + 1) * 16 + rc] << 16);
  }
  f32x4_t acc = {};
  acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(
      as_frag(ar[0], ar[1]), as_frag(br[0], br[1]), acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) c[(4 * g + r) * 16 + rc] = acc[r];
}

// out[M,N] f32 = a[M,K] @ b[K,N], both bf16, everything contiguous
template <typename Kernel>
static void launch_probe(Kernel kernel, int M, int N, int K, torch::Tensor out,
                         torch::Tensor a, torch::Tensor b) {
  TORCH_CHECK(a.sizes() == torch::IntArrayRef({M, K}));
  TORCH_CHECK(b.sizes() == torch::IntArrayRef({K, N}));
  TORCH_CHECK(out.sizes() == torch::IntArrayRef({M, N}));
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 && a.is_contiguous());
  TORCH_CHECK(b.scalar_type() == torch::kBFloat16 && b.is_contiguous());
  TORCH_CHECK(out.scalar_type() == torch::kFloat32 && out.is_contiguous());
  auto stream = c10::hip::getCurrentHIPStream().stream();
  kernel<<<1, 64, 0, stream>>>(
      out.data_ptr<float>(),
      reinterpret_cast<const unsigned short*>(a.data_ptr()),
      reinterpret_cast<const unsigned short*>(b.data_ptr()));
  HIP_CHECK_KERNEL();
}

void mfma_probe(torch::Tensor out, torch::Tensor a, torch::Tensor b) {
  launch_probe(mfma_probe_kernel, 32, 32, 16, out, a, b);
}
void mfma_probe16(torch::Tensor out, torch::Tensor a, torch::Tensor b) {
  launch_probe(mfma_probe16_kernel, 16, 16, 32, out, a, b);
}
void mfma_probe16k(torch::Tensor out, torch::Tensor a, torch::Tensor b) {
  launch_probe(mfma_probe16k_kernel, 16, 16, 16, out, a, b);
}

}  // namespace kukeon
