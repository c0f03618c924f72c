// bf16 MFMA fragment machinery shared by the attention kernels
// (paged_attn.hip, prefill_attn.hip) and validated on the device by the
// layout probes in mfma_probe.hip. Only things that hide a format live here.
//
// gfx950 lane maps (lane l of the wave; j / r index the lane's registers):
//
//   v_mfma_f32_32x32x16_bf16     C[32,32] += A[32,16] . B[16,32]
//     A (bf16x8): row = l&31,  k = 8*(l>>5) + j
//     B (bf16x8): col = l&31,  k = 8*(l>>5) + j
//     C (f32x16): col = l&31,  row = (r&3) + 8*(r>>2) + 4*(l>>5)
//
//   v_mfma_f32_16x16x32_bf16     C[16,16] += A[16,32] . B[32,16]
//     A (bf16x8): row = l&15,  k = 8*(l>>4) + j
//     B (bf16x8): col = l&15,  k = 8*(l>>4) + j
//     C (f32x4):  col = l&15,  row = 4*(l>>4) + r
//
//   v_mfma_f32_16x16x16_bf16     C[16,16] += A[16,16] . B[16,16]
//     A (bf16x4): row = l&15,  k = 4*(l>>4) + j
//     B (bf16x4): col = l&15,  k = 4*(l>>4) + j
//     C (f32x4):  col = l&15,  row = 4*(l>>4) + r
//
// The 16x16x32 C map equals the 16x16x16 B map (row -> k): scores computed
// as S^T = K.Q^T feed P^T into O^T = V^T.P^T with no cross-lane movement.
//
// V^T LDS image (the PV A operand; both attention kernels build it with the
// same interleave loop): row d holds the tile's tokens as bf16 pairs
// (tokens 2*kp, 2*kp+1 in 4 B slot kp), PITCH bytes per row, the slot byte
// offset XOR-ed with (d&3) << SWZ so the transposing stores and the
// fragment reads both spread over the banks. PITCH/SWZ is 64/4 for the
// prefill 32-token tile and 32/3 for the decode 16-token tile. The loop is
// written out in each kernel, not shared: every formulation of a common
// helper that was tried changed the generated code of one kernel or the
// other (opcode counts in prefill, instruction order in decode).
#pragma once

#include "common.h"
#include <type_traits>

namespace kukeon {

typedef __attribute__((__vector_size__(8 * sizeof(short)))) short bf16x8_t;
typedef __attribute__((__vector_size__(4 * sizeof(short)))) short bf16x4_t;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4_t;
typedef __attribute__((__vector_size__(16 * sizeof(float)))) float f32x16_t;

// Operand fragments from packed bf16 pairs (k-contiguous, low half first).
DEV_INLINE bf16x8_t as_frag(unsigned int w0, unsigned int w1, unsigned int w2,
                            unsigned int w3) {
  struct { unsigned int x[4]; } v{{w0, w1, w2, w3}};
  return __builtin_bit_cast(bf16x8_t, v);
}
DEV_INLINE bf16x4_t as_frag(unsigned int w0, unsigned int w1) {
  struct { unsigned int x[2]; } v{{w0, w1}};
  return __builtin_bit_cast(bf16x4_t, v);
}

// KV-cache element: bf16 bits, or fp8 (OCP e4m3) bytes. load_kv8 reads 8
// consecutive elements as bf16x8 — a 16 B load, or an 8 B load + convert.
// The caller does the pointer arithmetic on the typed pointer; that keeps
// the address code the compiler sees the same as a hand-written load.
template <bool FP8>
using kv_elem_t = std::conditional_t<FP8, unsigned char, unsigned short>;
DEV_INLINE uint4 load_kv8(const unsigned short* p) {
  return *reinterpret_cast<const uint4*>(p);
}
DEV_INLINE uint4 load_kv8(const unsigned char* p) {
  return fp8x8_to_bf16x8(*reinterpret_cast<const uint2*>(p));
}

}  // namespace kukeon
