// Python bindings for the kukeon_amd gfx950 kernel library.
#include <torch/extension.h>

namespace kukeon {
void rmsnorm(torch::Tensor out, torch::Tensor input, torch::Tensor weight,
             double eps);
void fused_add_rmsnorm(torch::Tensor input, torch::Tensor residual,
                       torch::Tensor weight, double eps);
void silu_mul(torch::Tensor out, torch::Tensor gate_up);
void rope_kv_append(torch::Tensor qkv, torch::Tensor k_cache,
                    torch::Tensor v_cache, torch::Tensor cos_sin,
                    torch::Tensor positions, torch::Tensor slot_mapping,
                    int64_t num_q_heads, int64_t num_kv_heads,
                    int64_t head_dim, torch::Tensor block_table);
void decode_advance(torch::Tensor ids, torch::Tensor pos,
                    torch::Tensor seq_lens, torch::Tensor tokens,
                    torch::Tensor ring, torch::Tensor counter);
void kv_copy_blocks(torch::Tensor k_cache, torch::Tensor v_cache,
                    torch::Tensor src, torch::Tensor dst);
void kv_pack_blocks(torch::Tensor k_cache, torch::Tensor v_cache,
                    torch::Tensor blocks, torch::Tensor staging);
void kv_unpack_blocks(torch::Tensor staging, torch::Tensor k_cache,
                      torch::Tensor v_cache, torch::Tensor blocks);
void paged_attention(torch::Tensor out, torch::Tensor q, torch::Tensor k_cache,
                     torch::Tensor v_cache, torch::Tensor block_table,
                     torch::Tensor seq_lens, int64_t q_offset,
                     int64_t num_splits, double scale, torch::Tensor tmp_out,
                     torch::Tensor tmp_ml);
void paged_attention_rope(torch::Tensor out, torch::Tensor qkv,
                          torch::Tensor k_cache, torch::Tensor v_cache,
                          torch::Tensor cos_sin, torch::Tensor positions,
                          torch::Tensor block_table, torch::Tensor seq_lens,
                          int64_t num_q_heads, int64_t num_kv_heads,
                          int64_t num_splits, double scale,
                          torch::Tensor tmp_out, torch::Tensor tmp_ml);
void paged_attention_shared(torch::Tensor out, torch::Tensor q,
                            torch::Tensor k_cache, torch::Tensor v_cache,
                            torch::Tensor block_table, torch::Tensor seq_lens,
                            int64_t q_offset, int64_t num_splits, double scale,
                            torch::Tensor tmp_out, torch::Tensor tmp_ml,
                            torch::Tensor prefix_blocks, torch::Tensor tiles,
                            int64_t prefix_splits);
void paged_attention_rope_shared(
    torch::Tensor out, torch::Tensor qkv, torch::Tensor k_cache,
    torch::Tensor v_cache, torch::Tensor cos_sin, torch::Tensor positions,
    torch::Tensor block_table, torch::Tensor seq_lens, int64_t num_q_heads,
    int64_t num_kv_heads, int64_t num_splits, double scale,
    torch::Tensor tmp_out, torch::Tensor tmp_ml, torch::Tensor prefix_blocks,
    torch::Tensor tiles, int64_t prefix_splits);
void prefill_attention(torch::Tensor out, torch::Tensor q,
                       torch::Tensor k_cache, torch::Tensor v_cache,
                       torch::Tensor block_table, torch::Tensor seq_lens,
                       torch::Tensor q_starts, torch::Tensor qb_seq,
                       torch::Tensor qb_start, int64_t q_offset, double scale);
void mfma_probe(torch::Tensor out, torch::Tensor a, torch::Tensor b);
void mfma_probe16(torch::Tensor out, torch::Tensor a, torch::Tensor b);
void mfma_probe16k(torch::Tensor out, torch::Tensor a, torch::Tensor b);
void skinny_gemm2(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                  torch::Tensor ws);
void skinny_gemm5(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                  torch::Tensor ws);
void skinny_gemm6(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                  torch::Tensor ws);
void skinny_gemm5_silu_fused_norm(torch::Tensor normed, torch::Tensor gu,
                                  torch::Tensor w, torch::Tensor ws,
                                  torch::Tensor residual, torch::Tensor nw,
                                  double eps);
void skinny_gemm(torch::Tensor out, torch::Tensor x, torch::Tensor w,
                 torch::Tensor ws);
void glds_probe(torch::Tensor out, torch::Tensor src);
int64_t skinny_splitk(const std::string& kind, int64_t N, int64_t K);
void skinny_gemm5_fused_norm(torch::Tensor normed, torch::Tensor x,
                             torch::Tensor w, torch::Tensor ws,
                             torch::Tensor residual, torch::Tensor nw,
                             double eps);
void skinny_gemm_fused_norm(torch::Tensor normed, torch::Tensor x,
                            torch::Tensor w, torch::Tensor ws,
                            torch::Tensor residual, torch::Tensor nw,
                            double eps);
void skinny_gemm_w8(torch::Tensor out, torch::Tensor x, torch::Tensor q,
                    torch::Tensor scale, torch::Tensor ws);
void skinny_gemm_w8_fused_norm(torch::Tensor normed, torch::Tensor x,
                               torch::Tensor q, torch::Tensor scale,
                               torch::Tensor ws, torch::Tensor residual,
                               torch::Tensor nw, double eps);
void quantize_fp8_rows(torch::Tensor q, torch::Tensor scale, torch::Tensor w);
void dequant_fp8_rows(torch::Tensor out, torch::Tensor q,
                      torch::Tensor scale);
void skinny_gemm_w4(torch::Tensor out, torch::Tensor x, torch::Tensor q,
                    torch::Tensor scale, torch::Tensor ws);
void skinny_gemm_w4_fused_norm(torch::Tensor normed, torch::Tensor x,
                               torch::Tensor q, torch::Tensor scale,
                               torch::Tensor ws, torch::Tensor residual,
                               torch::Tensor nw, double eps);
void quantize_mxfp4_rows(torch::Tensor q, torch::Tensor scale,
                         torch::Tensor w);
void dequant_mxfp4_rows(torch::Tensor out, torch::Tensor q,
                        torch::Tensor scale);
void sample(torch::Tensor tokens, torch::Tensor logits, torch::Tensor temps,
            torch::Tensor top_k, torch::Tensor top_p, torch::Tensor seed,
            torch::Tensor workspace);
void moe_router_weights(torch::Tensor wdense, torch::Tensor logits,
                        long K);
void moe_dense_combine(torch::Tensor out, torch::Tensor y,
                       torch::Tensor wdense);
void moe_gather_tokens(torch::Tensor out, torch::Tensor input,
                       torch::Tensor row_map);
void moe_scatter_tokens(torch::Tensor out, torch::Tensor input,
                        torch::Tensor row_map, torch::Tensor weights,
                        int64_t top_k);
void moe_route_sort(torch::Tensor topk_w, torch::Tensor row_map,
                    torch::Tensor inv_map, torch::Tensor offsets,
                    torch::Tensor logits, long K);
void moe_grouped_gemm(torch::Tensor out, torch::Tensor a,
                      torch::Tensor a_rows, torch::Tensor w,
                      torch::Tensor offsets);
}  // namespace kukeon

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm", &kukeon::rmsnorm, "RMSNorm (bf16, gfx950)");
  m.def("fused_add_rmsnorm", &kukeon::fused_add_rmsnorm,
        "residual += input; input = rmsnorm(residual)");
  m.def("silu_mul", &kukeon::silu_mul, "out = silu(gate)*up from fused [T,2I]");
  m.def("rope_kv_append", &kukeon::rope_kv_append,
        "in-place NEOX RoPE on fused qkv + paged KV append");
  m.def("kv_copy_blocks", &kukeon::kv_copy_blocks,
        "cache[l, dst[i]] = cache[l, src[i]] for K and V, all layers, one "
        "launch");
  m.def("kv_pack_blocks", &kukeon::kv_pack_blocks,
        "staging[i, s, l] = cache_s[l, blocks[i]] for K and V, all layers, "
        "one launch");
  m.def("kv_unpack_blocks", &kukeon::kv_unpack_blocks,
        "cache_s[l, blocks[i]] = staging[i, s, l] for K and V, all layers, "
        "one launch");
  m.def("paged_attention", &kukeon::paged_attention,
        "decode paged attention (GQA, split-KV)");
  m.def("paged_attention_rope", &kukeon::paged_attention_rope,
        "decode paged attention with RoPE + KV append folded in");
  m.def("paged_attention_shared", &kukeon::paged_attention_shared,
        "decode paged attention, shared prefix blocks read once per tile of "
        "rows");
  m.def("paged_attention_rope_shared", &kukeon::paged_attention_rope_shared,
        "paged_attention_rope, shared prefix blocks read once per tile of "
        "rows");
  m.def("prefill_attention", &kukeon::prefill_attention,
        "varlen causal paged prefill attention (MFMA)");
  m.def("mfma_probe", &kukeon::mfma_probe,
        "32x32x16 bf16 MFMA fragment-layout probe");
  m.def("mfma_probe16", &kukeon::mfma_probe16,
        "16x16x32 bf16 MFMA fragment-layout probe");
  m.def("mfma_probe16k", &kukeon::mfma_probe16k,
        "16x16x16 (K=16) bf16 MFMA fragment-layout probe");
  m.def("skinny_gemm6", &kukeon::skinny_gemm6,
        "decode GEMM v6 (barrier-free register-x pipeline)");
  m.def("skinny_gemm5_silu_fused_norm",
        &kukeon::skinny_gemm5_silu_fused_norm,
        "silu(gate)*up + down GEMM + reduce + add + RMSNorm fused");
  m.def("skinny_gemm5", &kukeon::skinny_gemm5,
        "full-line W stream via wave-private LDS image (v5)");
  m.def("skinny_gemm2", &kukeon::skinny_gemm2,
        "G-walk hand-counted weight-streaming GEMM (v2)");
  m.def("skinny_gemm", &kukeon::skinny_gemm,
        "weight-streaming decode GEMM (M<=64)");
  m.def("skinny_splitk", &kukeon::skinny_splitk,
        "split-K factor the skinny launcher of `kind` (v1, v2, v5, v5_fused, "
        "v6, w8, w4) uses for [N, K]; host-only",
        py::arg("kind"), py::arg("N"), py::arg("K"));
  m.def("glds_probe", &kukeon::glds_probe,
        "asm global_lds round-trip validator");
  m.def("skinny_gemm5_fused_norm", &kukeon::skinny_gemm5_fused_norm,
        "skinny5 + fused split-K reduce + residual add + RMSNorm");
  m.def("skinny_gemm_fused_norm", &kukeon::skinny_gemm_fused_norm,
        "skinny GEMM + split-K reduce + residual add + RMSNorm");
  m.def("skinny_gemm_w8", &kukeon::skinny_gemm_w8,
        "W8A16 decode GEMM: (x @ fp8(q)^T) * scale, M<=64");
  m.def("skinny_gemm_w8_fused_norm", &kukeon::skinny_gemm_w8_fused_norm,
        "W8A16 decode GEMM + split-K reduce + residual add + RMSNorm");
  m.def("quantize_fp8_rows", &kukeon::quantize_fp8_rows,
        "bf16 [N,K] -> e4m3fn bytes + per-row f32 scale (amax/448)");
  m.def("dequant_fp8_rows", &kukeon::dequant_fp8_rows,
        "out = bf16(fp8(q) * scale[n])");
  m.def("skinny_gemm_w4", &kukeon::skinny_gemm_w4,
        "W4A16 decode GEMM: x @ mxfp4(q, scale)^T, M<=64");
  m.def("skinny_gemm_w4_fused_norm", &kukeon::skinny_gemm_w4_fused_norm,
        "W4A16 decode GEMM + split-K reduce + residual add + RMSNorm");
  m.def("quantize_mxfp4_rows", &kukeon::quantize_mxfp4_rows,
        "bf16 [N,K] -> e2m1 pairs [N,K/2] + e8m0 scale [N,K/32] (OCP MX)");
  m.def("dequant_mxfp4_rows", &kukeon::dequant_mxfp4_rows,
        "out = bf16(e2m1(q) * 2^(scale[n, k/32] - 127))");
  m.def("sample", &kukeon::sample, "top-k/top-p/temperature sampling");
  m.def("decode_advance", &kukeon::decode_advance,
        "on-device decode cursor advance (self-advancing graph)");
  m.def("moe_gather_tokens", &kukeon::moe_gather_tokens, "MoE permute");
  m.def("moe_router_weights", &kukeon::moe_router_weights,
        "softmax top-K renorm -> dense [T,E] weights, one launch");
  m.def("moe_dense_combine", &kukeon::moe_dense_combine,
        "out = sum_e w[t,e]*y[e,t,:], zero-weight experts skipped");
  m.def("moe_scatter_tokens", &kukeon::moe_scatter_tokens,
        "MoE unpermute + weighted combine");
  m.def("moe_route_sort", &kukeon::moe_route_sort,
        "top-k routing + stable expert sort on the device, one launch");
  m.def("moe_grouped_gemm", &kukeon::moe_grouped_gemm,
        "out[r] = a[a_rows[r]] @ w[e].T, expert row ranges from device");
}
