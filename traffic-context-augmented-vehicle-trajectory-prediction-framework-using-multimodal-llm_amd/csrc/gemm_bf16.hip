// bf16 x bf16 -> fp32-accumulate contraction for gfx950 (MI355X), hand-tiled for
// 64-wide waves and v_mfma_f32_16x16x32_bf16.
//
//   C[M,N] = A[M,K] . W[N,K]^T (+ A2[M,K2] . W2[N,K2]^T)   + fused epilogue
//
// Both operands are K-contiguous (activations [tokens][features], nn.Linear
// weights [out][in]), so they are staged with the same code: 64-deep K-tiles go
// global -> LDS by 16-byte LDS-DMA (global_load_lds_dwordx4, no VGPR round trip),
// double-buffered.  An LDS row is one tile row's 128 bytes; the eight 16-byte
// chunks of a row are XOR-swizzled with (row>>1)&7 so that every ds_read_b128
// fragment read is bank-conflict free.  Because LDS-DMA writes lane-linear, the
// swizzle is applied to the per-lane SOURCE address and to the fragment READ
// address (same involution), never to the destination.
//
// The MFMA is issued "swapped": the weight rows are the A operand and the token
// rows the B operand, so each lane ends with 4 consecutive output FEATURES of
// one token in a register quad -> 8/16-byte row-contiguous epilogue accesses,
// and RoPE / SiLU*up partners are lane-local.
//
// Replaces the nn.Linear contractions listed in include/tcavt.h (reference:
// scripts/train.py:401-406,446-452,493,754-757 and HF modeling_llama.py
// :174-176,254-256,279-280).
//
// This file holds the argument validation, the dispatch between the forms and the two extern "C" entries; the kernels
// and their launchers are in the headers below, one per form, all in this one translation unit.
#include "gemm_params.hpp"
#include "gemm_epilogue.hpp"
#include "gemm_tile8.hpp"
#include "gemm_w4.hpp"
#include "gemm_skinny.hpp"
#include "gemm_splitk.hpp"

namespace tcavt {

// Launches below one wave of 256x256 tiles (tile = 128, 64 or 0 = pick).
template <int EPI, bool F16>
static int launch_small(const GemmP& p, int tile, int batch, hipStream_t stream) {
  GemmP q = p;
  q.prio = 0;
  // grids that leave CUs idle: the 4-stage loop (latency bound, one workgroup per CU is no loss);
  // fuller grids: interleaved DMA issue, 64 KiB of LDS so that two workgroups share a CU
  const long wgs = (long)((q.M + 127) / 128) * ((q.N + 127) / 128) * batch;
  static const bool no_deep = getenv("TCAVT_GEMM_NO_DEEP") != nullptr;  // A/B switches
  static const bool no_64 = getenv("TCAVT_GEMM_NO_64") != nullptr;
  if constexpr (EPI != EPI_ROPE && EPI != EPI_NORM && EPI != EPI_NORM16) {
    // very small grids (Q-Former projections, LoRA down-projection): 64x64 tiles, four times the workgroups,
    // each K-tile costing a quarter of the DMA issue and MFMA time
    // (not for EPI_NORM: the 64x64 form's waves cover 32 columns, no whole 64-column group)
    if ((tile == 64 || (tile == 0 && wgs <= 128 && !no_64)) && !no_deep) return launch<64, 64, 2, 2, EPI, F16, 2>(q, batch, stream);
  }
  if (wgs <= 256 && !no_deep) return launch<128, 128, 2, 2, EPI, F16, 2>(q, batch, stream);
  return launch<128, 128, 2, 2, EPI, F16, 1>(q, batch, stream);
}

// tile codes (tcavt_gemm_args.tile): 0 auto | 64, 128, 256 (8-wave), 257 (4-wave 256x256), 271 (4-wave 256x192),
// 272 (4-wave two-barrier form), all bit-identical in results.  Nothing else exists: tcavt_gemm_bf16 refuses every other code.
template <int EPI, bool F16>
static int dispatch_tile(const GemmP& p, int tile, int batch, hipStream_t stream) {
  GemmP q = p;
  switch (tile) {
    case 256:  // DMA pieces interleaved with the MFMAs + s_setprio(1) around MFMA clusters (fastest measured)
      q.prio = 2;
      return launch<256, 256, 2, 4, EPI, F16, 1>(q, batch, stream);
    case 271:  // 256 x 192 tiles (N % 192 == 0)
      if (batch == 1 && (q.K2 == 0 || EPI == EPI_ROPE) && q.M % 256 == 0 && q.N % 192 == 0 &&
          (EPI != EPI_ROPE || q.out_kind == (F16 ? TCAVT_F16 : TCAVT_BF16)))
        return launch_w4<EPI, F16, 192>(q, stream);
      set_error("gemm_bf16: tile 271 (4-wave kernel, 256x192) needs M %% 256 == 0, N %% 192 == 0, no batch");
      return TCAVT_ERR_ARG;
    case 257: case 272:
      if (batch == 1 && (q.K2 == 0 || EPI == EPI_ROPE) && q.M % 256 == 0 && q.N % 256 == 0 &&
          (EPI != EPI_ROPE || q.out_kind == (F16 ? TCAVT_F16 : TCAVT_BF16))) {
        if (tile == 272) {
          if constexpr (EPI != EPI_ROPE) return launch_w4<EPI, F16, 256, true>(q, stream);  // DEEP
        }
        return launch_w4<EPI, F16>(q, stream);
      }
      set_error("gemm_bf16: tile %d (4-wave kernel) needs whole 256x256 tiles, one K source, no batch", tile);
      return TCAVT_ERR_ARG;
    default: return launch_small<EPI, F16>(q, tile, batch, stream);  // 128 / 64 / 0 (auto)
  }
}

}  // namespace tcavt

using namespace tcavt;

extern "C" int tcavt_pack_weight16(const void* W, int64_t ldw, void* out, int N, int K, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(W && out && W != out && N > 0 && K > 0 && N % 16 == 0 && K % 32 == 0 && ldw >= K && ldw % 8 == 0,
                  "pack_weight16: N %% 16 == 0, K %% 32 == 0, ldw >= K, ldw %% 8 == 0, out != W");
  TCAVT_CHECK_ARG(aligned16(W) && aligned16(out), "pack_weight16: 16-byte alignment required");
  const long pieces = (long)N * K / 8;
  hipLaunchKernelGGL(pack_weight16_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(W), (long)ldw, static_cast<bf16_t*>(out), N, K);
  TCAVT_CHECK_LAUNCH("pack_weight16");
  return TCAVT_OK;
}

extern "C" size_t tcavt_pack_weight8_bytes(int N, int K) { return N > 0 && K > 0 ? (size_t)N * K + 4 * (size_t)N : 0; }

extern "C" int tcavt_pack_weight8(const void* W, int64_t ldw, int dtype16, void* out, int N, int K, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(W && out && W != out && N > 0 && K > 0 && N % 16 == 0 && K % 32 == 0 && ldw >= K && ldw % 8 == 0 && is16(dtype16),
                  "pack_weight8: N %% 16 == 0, K %% 32 == 0, ldw >= K, ldw %% 8 == 0, out != W, dtype16 = TCAVT_F16 / TCAVT_BF16");
  TCAVT_CHECK_ARG(aligned16(W) && aligned16(out), "pack_weight8: 16-byte alignment required");
  auto kfn = dtype16 == TCAVT_F16 ? pack_weight8_kernel<true> : pack_weight8_kernel<false>;
  hipLaunchKernelGGL(kfn, dim3((unsigned)(N / 16)), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(W), (long)ldw,
                     static_cast<unsigned char*>(out), N, K);
  TCAVT_CHECK_LAUNCH("pack_weight8");
  return TCAVT_OK;
}

extern "C" int tcavt_gemm_bf16(const tcavt_gemm_args* a, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(a != nullptr, "gemm_bf16: null args");
  const bool stream16 = (a->epilogue & TCAVT_EPI_NORM_OUT) && a->C == nullptr;  // 16-bit residual stream in norm_h16
  TCAVT_CHECK_ARG(a->A && a->W && (a->C || stream16), "gemm_bf16: null A/W/C");
  TCAVT_CHECK_ARG(a->M > 0 && a->N > 0 && a->K > 0, "gemm_bf16: bad M/N/K %d/%d/%d", a->M, a->N, a->K);
  TCAVT_CHECK_ARG(a->K % 64 == 0, "gemm_bf16: K=%d must be a multiple of 64", a->K);
  TCAVT_CHECK_ARG(a->K < (1 << 26), "gemm_bf16: K too large");
  TCAVT_CHECK_ARG(a->N % 16 == 0, "gemm_bf16: N=%d must be a multiple of 16", a->N);
  TCAVT_CHECK_ARG(a->lda % 8 == 0 && a->ldw % 8 == 0 && a->lda >= a->K && a->ldw >= a->K,
                  "gemm_bf16: lda/ldw must be >= K and multiples of 8");
  TCAVT_CHECK_ARG(aligned16(a->A) && aligned16(a->W) && aligned16(a->C), "gemm_bf16: A/W/C must be 16-byte aligned");
  TCAVT_CHECK_ARG(a->out_dtype == TCAVT_F32 || a->out_dtype == TCAVT_BF16 || a->out_dtype == TCAVT_F16,
                  "gemm_bf16: bad out_dtype");
  TCAVT_CHECK_ARG(a->in_dtype == 0 || a->in_dtype == TCAVT_BF16 || a->in_dtype == TCAVT_F16, "gemm_bf16: bad in_dtype");
  const bool f16 = a->in_dtype == TCAVT_F16;
  const int batch = a->batch > 1 ? a->batch : 1;
  if (batch > 1)
    TCAVT_CHECK_ARG(!(a->epilogue & (TCAVT_EPI_SILU_MUL | TCAVT_EPI_ROPE)),
                    "gemm_bf16: batching is supported by the generic epilogue only");
  if (batch > 1) {
    TCAVT_CHECK_ARG(a->batch_inner >= 1 && batch % a->batch_inner == 0, "gemm_bf16: batch must be a multiple of batch_inner");
    TCAVT_CHECK_ARG(a->sAo % 8 == 0 && a->sAi % 8 == 0 && a->sWo % 8 == 0 && a->sWi % 8 == 0 && a->sCo % 4 == 0 &&
                        a->sCi % 4 == 0 && batch <= 65535,
                    "gemm_bf16: batch strides must keep 16-byte (A/W) and 4-element (C) alignment; batch <= 65535");
  }
  const int n_out = (a->epilogue & TCAVT_EPI_SILU_MUL) ? a->N / 2 : a->N;
  TCAVT_CHECK_ARG(a->ldc >= n_out && a->ldc % 4 == 0, "gemm_bf16: ldc=%ld too small or not a multiple of 4", (long)a->ldc);
  int K2 = 0;
  const bool lp_consumer = a->lora_part && (a->epilogue & TCAVT_EPI_ROPE);  // (W2 without A2: checked with lora_part below)
  if ((a->A2 || a->W2 || a->K2) && !lp_consumer) {
    TCAVT_CHECK_ARG(a->A2 && a->W2 && a->K2 > 0 && a->K2 % 64 == 0,
                    "gemm_bf16: second K-source needs A2, W2 and K2 %% 64 == 0");
    TCAVT_CHECK_ARG(a->lda2 % 8 == 0 && a->ldw2 % 8 == 0 && a->lda2 >= a->K2 && a->ldw2 >= a->K2 &&
                        aligned16(a->A2) && aligned16(a->W2),
                    "gemm_bf16: bad lda2/ldw2/alignment");
    K2 = a->K2;
  }
  int epi = a->epilogue;
  if (epi & TCAVT_EPI_BIAS) TCAVT_CHECK_ARG(a->bias && aligned16(a->bias), "gemm_bf16: BIAS needs an aligned bias pointer");
  if (epi & TCAVT_EPI_BIAS_ROW) TCAVT_CHECK_ARG(a->bias && !(epi & TCAVT_EPI_BIAS), "gemm_bf16: BIAS_ROW needs bias and excludes BIAS");
  if ((epi & TCAVT_EPI_RESIDUAL) && !stream16)  // (stream16: the residual is norm_h16 itself)
    TCAVT_CHECK_ARG(a->residual && aligned16(a->residual) && a->ldr >= a->N && a->ldr % 4 == 0,
                    "gemm_bf16: RESIDUAL needs residual pointer and ldr >= N");
  if (epi & TCAVT_EPI_SILU_MUL)
    TCAVT_CHECK_ARG(a->N % 128 == 0 && !(epi & ~(TCAVT_EPI_SILU_MUL | TCAVT_EPI_ROWSCALE)),
                    "gemm_bf16: SILU_MUL needs N %% 128 == 0 and no other flag but ROWSCALE");
  if (epi & TCAVT_EPI_ROPE) {
    TCAVT_CHECK_ARG(a->N % 128 == 0 && !(epi & ~(TCAVT_EPI_ROPE | TCAVT_EPI_ROWSCALE)),
                    "gemm_bf16: ROPE needs N %% 128 == 0 and no other flag but ROWSCALE");
    TCAVT_CHECK_ARG(a->rope_cos && a->rope_sin && a->rope_L > 0 && a->rope_cols % 64 == 0 &&
                        aligned16(a->rope_cos) && aligned16(a->rope_sin),
                    "gemm_bf16: ROPE needs cos/sin tables, rope_L > 0, rope_cols %% 64 == 0");
  }
  TCAVT_CHECK_ARG(a->tile == 0 || a->tile == 64 || a->tile == 128 || a->tile == 256 || a->tile == 257 || a->tile == 271 || a->tile == 272,
                  "gemm_bf16: tile must be 0 (auto), 64, 128, 256, 257, 271 or 272");

  GemmP p;
  p.A = static_cast<const bf16_t*>(a->A);
  p.W = static_cast<const bf16_t*>(a->W);
  p.A2 = static_cast<const bf16_t*>(a->A2);
  p.W2 = static_cast<const bf16_t*>(a->W2);
  p.C = a->C;
  p.bias = a->bias;
  p.residual = a->residual;
  p.cosT = a->rope_cos;
  p.sinT = a->rope_sin;
  p.lda = a->lda; p.ldw = a->ldw; p.lda2 = a->lda2; p.ldw2 = a->ldw2; p.ldc = a->ldc; p.ldr = a->ldr;
  p.M = a->M; p.N = a->N; p.K = a->K; p.K2 = K2;
  p.out_kind = a->out_dtype;
  p.batch_inner = batch > 1 ? a->batch_inner : 1;
  p.w_group = a->batch_w_group > 1 ? a->batch_w_group : 1;
  p.sAo = a->sAo; p.sAi = a->sAi; p.sWo = a->sWo; p.sWi = a->sWi; p.sCo = a->sCo; p.sCi = a->sCi;
  p.flags = epi;
  p.rope_L = a->rope_L; p.rope_cols = a->rope_cols;
  p.tiles_m = p.tiles_n = 0;
  p.prio = 0;
  p.pers_tiles = 0;
  p.xcd_gx = 8;
  p.norm_h16 = nullptr;
  p.norm_part = nullptr;
  p.res16 = nullptr;
  p.res_pf = 0;
  p.lp_part = nullptr;
  p.lp_a = nullptr;
  p.lp_lda = 0;
  p.lp_np = 0;
  p.lp_scale = 1.f;
  p.w_frag = p.a_frag = p.o_frag = 0;
  if (a->act_layout != 0) {
    TCAVT_CHECK_ARG((a->act_layout & ~(TCAVT_ACT_A_FRAG16 | TCAVT_ACT_OUT_FRAG16 | TCAVT_ACT_BLOCK8)) == 0 && a->tile == 0 &&
                        skinny_shape(a->M, a->K) && batch == 1 && a->dropout_p == 0.f,
                    "gemm_bf16: act_layout (fragment-major activations) goes with the skinny form only (M <= 32, K %% 256 == 0, tile 0)");
    const int fmode = (a->act_layout & TCAVT_ACT_BLOCK8) ? 2 : 1;
    TCAVT_CHECK_ARG(fmode == 1 || a->M <= 8, "gemm_bf16: TCAVT_ACT_BLOCK8 holds at most 8 rows");
    p.a_frag = (a->act_layout & TCAVT_ACT_A_FRAG16) ? fmode : 0;
    if (a->act_layout & TCAVT_ACT_OUT_FRAG16) {
      const bool silu = (a->epilogue & ~TCAVT_EPI_ROWSCALE) == TCAVT_EPI_SILU_MUL && a->out_dtype == (f16 ? TCAVT_F16 : TCAVT_BF16) &&
                        a->N % 64 == 0;
      const bool stream = (a->epilogue & TCAVT_EPI_NORM_OUT) && stream16 && a->N % 32 == 0;
      TCAVT_CHECK_ARG(silu || stream, "gemm_bf16: TCAVT_ACT_OUT_FRAG16 needs SILU_MUL with a 16-bit output of the operand type, or "
                                      "NORM_OUT with C == NULL (the in-place 16-bit stream)");
      p.o_frag = fmode;
    }
  }
  if (a->w_layout != 0) {
    TCAVT_CHECK_ARG((a->w_layout == TCAVT_W_FRAG16 || a->w_layout == TCAVT_W_FRAG8) && a->tile == 0 && skinny_shape(a->M, a->K) && batch == 1 &&
                        a->dropout_p == 0.f && a->lda >= a->K && a->ldw == a->K && a->N % 16 == 0,
                    "gemm_bf16: w_layout = TCAVT_W_FRAG16 / TCAVT_W_FRAG8 (tcavt_pack_weight16 / tcavt_pack_weight8 copy) goes with the "
                    "skinny form only (M <= 32, K %% 256 == 0, N %% 16 == 0, tile 0, ldw == K)");
    p.w_frag = a->w_layout == TCAVT_W_FRAG8 ? 2 : 1;
  }
  if (a->lora_part) {
    // (decode step only: the skinny form; anything else is a caller error rather than a silent no-op)
    TCAVT_CHECK_ARG(a->tile == 0 && skinny_shape(a->M, a->K) && batch == 1 && a->dropout_p == 0.f && aligned16(a->lora_part),
                    "gemm_bf16: lora_part goes with the skinny form only (M <= 32, tile 0)");
    p.lp_part = static_cast<float*>(a->lora_part);
    if (epi & TCAVT_EPI_NORM_OUT) {
      TCAVT_CHECK_ARG(a->lora_part_a && a->lora_part_lda >= a->N && a->lora_part_lda % 4 == 0 && ((uintptr_t)a->lora_part_a & 7) == 0,
                      "gemm_bf16: lora_part with NORM_OUT needs lora_part_a [32, lda >= N]");
      p.lp_a = static_cast<const bf16_t*>(a->lora_part_a);
      p.lp_lda = a->lora_part_lda;
    } else {
      TCAVT_CHECK_ARG((epi & TCAVT_EPI_ROPE) && a->lora_part_np > 0 && a->W2 && !a->A2 && a->K2 == 0 && a->ldw2 >= 32 && a->ldw2 % 8 == 0 &&
                          aligned16(a->W2) && a->M * 16 <= 512,
                      "gemm_bf16: lora_part with ROPE needs lora_part_np > 0, W2 (ldw2 >= 32) and no A2");
      p.lp_np = a->lora_part_np;
      p.lp_scale = a->lora_part_scale;
      p.W2 = static_cast<const bf16_t*>(a->W2);
      p.ldw2 = a->ldw2;
    }
  }
  p.sk_msplit = 1;
  p.sk_split = 1;
  p.sk_slab = nullptr;
  p.sk_cnt = nullptr;
  p.sk_slab_bytes = 0;
  p.sk_cnt_n = 0;
  if (a->splitk_ws && a->splitk_ws_bytes >= (64 << 10)) {  // [0, 16 KiB): 4096 tickets; the rest: slabs
    TCAVT_CHECK_ARG(aligned16(a->splitk_ws), "gemm_bf16: splitk_ws must be 16-byte aligned");
    p.sk_cnt = static_cast<int*>(a->splitk_ws);
    p.sk_cnt_n = 4096;
    p.sk_slab = reinterpret_cast<float*>(static_cast<char*>(a->splitk_ws) + (16 << 10));
    p.sk_slab_bytes = a->splitk_ws_bytes - (16 << 10);
  }
  p.nf_flag = (epi & TCAVT_EPI_NORM_OUT) ? a->nonfinite_flag : nullptr;
  p.nf_tag = a->nonfinite_tag;
  p.norm_scale = 1.f;
  if (epi & TCAVT_EPI_NORM_OUT) {
    TCAVT_CHECK_ARG(a->norm_scale >= 0.f && a->norm_scale <= 1.f, "gemm_bf16: norm_scale must be in (0, 1] (0 means 1)");
    if (a->norm_scale != 0.f) p.norm_scale = a->norm_scale;
  }
  p.rs_part = nullptr;
  p.rope_pos = (epi & TCAVT_EPI_ROPE) ? a->rope_pos : nullptr;
  p.rs_npart = 0;
  p.rs_eps = p.rs_inv_h = 0.f;
  if (epi & TCAVT_EPI_NORM_OUT) {
    TCAVT_CHECK_ARG(!(epi & ~(TCAVT_EPI_NORM_OUT | TCAVT_EPI_RESIDUAL)) && a->out_dtype == TCAVT_F32 && batch == 1 && K2 == 0 &&
                        a->N % 64 == 0 && a->norm_h16 && a->norm_part && aligned16(a->norm_h16) && a->dropout_p == 0.f &&
                        (a->acc_scale == 0.f || a->acc_scale == 1.f) && a->tile != 64,
                    "gemm_bf16: NORM_OUT goes with an fp32 output (+ RESIDUAL) only, N %% 64 == 0, and needs norm_h16 / norm_part");
    TCAVT_CHECK_ARG(!stream16 || a->residual == nullptr,
                    "gemm_bf16: NORM_OUT with C == NULL keeps the residual stream in norm_h16 (updated in place): residual must be NULL");
    p.norm_h16 = static_cast<bf16_t*>(a->norm_h16);
    p.norm_part = a->norm_part;
    TCAVT_CHECK_ARG(a->norm_res16 == nullptr || (stream16 && aligned16(a->norm_res16)),
                    "gemm_bf16: norm_res16 goes with the 16-bit residual stream (NORM_OUT, C == NULL) and needs 16-byte alignment");
    p.res16 = a->norm_res16 ? static_cast<const bf16_t*>(a->norm_res16) : p.norm_h16;
  }
  if (epi & TCAVT_EPI_ROWSCALE) {
    TCAVT_CHECK_ARG((epi & (TCAVT_EPI_SILU_MUL | TCAVT_EPI_ROPE)) && a->rowscale_part && aligned16(a->rowscale_part) &&
                        a->rowscale_npart > 0 && a->rowscale_npart % 4 == 0 && a->rowscale_h > 0,
                    "gemm_bf16: ROWSCALE goes with the ROPE / SILU_MUL epilogues and needs rowscale_part, npart %% 4 == 0, h > 0");
    p.rs_part = a->rowscale_part;
    p.rs_npart = a->rowscale_npart;
    p.rs_eps = a->rowscale_eps;
    p.rs_inv_h = 1.f / (float)a->rowscale_h;
  }
  epi &= ~TCAVT_EPI_ROWSCALE;  // (carried by p.rs_part from here on)
  TCAVT_CHECK_ARG(a->dropout_p >= 0.f && a->dropout_p < 1.f, "gemm_bf16: dropout_p must be in [0, 1)");
  if (a->dropout_p > 0.f)
    TCAVT_CHECK_ARG(!(epi & (TCAVT_EPI_SILU_MUL | TCAVT_EPI_ROPE)) && batch == 1 && a->N % 4 == 0,
                    "gemm_bf16: dropout is supported by the un-batched generic epilogue only");
  p.drop = make_dropout(a->dropout_p, a->dropout_seed, a->dropout_site);
  p.acc_scale = a->acc_scale == 0.f ? 1.f : a->acc_scale;
  if (epi & (TCAVT_EPI_SILU_MUL | TCAVT_EPI_ROPE))
    TCAVT_CHECK_ARG(p.acc_scale == 1.f, "gemm_bf16: acc_scale is only supported by the generic epilogue");

  hipStream_t s = static_cast<hipStream_t>(stream);
  // ---- two-launch split K (splitk_norm16_kernel above): the in-place 16-bit residual form on a grid that leaves CUs idle
  static const bool no_splitk2 = getenv("TCAVT_GEMM_NO_SPLITK2") != nullptr;  // (A/B switch)
  if (a->tile == 0 && stream16 && !no_splitk2 && p.sk_slab && a->M > 32 && !skinny_shape(a->M, a->K) && batch == 1 && K2 == 0 &&
      a->N % 128 == 0 && a->ldc % 8 == 0 && !a->lora_part && a->dropout_p == 0.f) {
    const int S = splitk_slices(a->M, a->N, a->K);
    if (S > 1 && (long)S * a->M * a->N * 4 <= p.sk_slab_bytes) {
      GemmP q = p;
      q.C = p.sk_slab; q.ldc = a->N; q.out_kind = TCAVT_F32; q.flags = 0; q.K = a->K / S;
      q.norm_h16 = nullptr; q.norm_part = nullptr; q.res16 = nullptr; q.nf_flag = nullptr; q.residual = nullptr;
      q.batch_inner = S; q.w_group = 1;
      q.sAo = 0; q.sAi = a->K / S; q.sWo = 0; q.sWi = a->K / S; q.sCo = 0; q.sCi = (long)a->M * a->N;
      const int rc = f16 ? dispatch_tile<EPI_GENERIC, true>(q, 0, S, s) : dispatch_tile<EPI_GENERIC, false>(q, 0, S, s);
      if (rc != TCAVT_OK) return rc;
      const long threads = (long)a->M * (a->N / 8);
      auto kfn = f16 ? splitk_norm16_kernel<true> : splitk_norm16_kernel<false>;
      hipLaunchKernelGGL(kfn, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, p.sk_slab, S, (long)a->M * a->N, p.res16, p.norm_h16,
                         p.norm_part, a->M, a->N, (long)a->ldc, a->N >> 6, p.norm_scale, (epi & TCAVT_EPI_RESIDUAL) ? 1 : 0, p.nf_flag, p.nf_tag);
      TCAVT_CHECK_LAUNCH("gemm_bf16(split-K reduce)");
      return TCAVT_OK;
    }
  }
  // ---- skinny form: M <= 32 rows (decode step), auto-selected only (tile == 0); norm_out_npart() mirrors this rule
  if (a->tile == 0 && skinny_shape(a->M, a->K) && batch == 1 && a->dropout_p == 0.f && a->lda >= a->K) {
    const int e0 = a->epilogue & ~TCAVT_EPI_ROWSCALE;
    if (e0 == TCAVT_EPI_ROPE && a->N % 64 == 0 && (K2 == 0 || K2 % 32 == 0))
      return f16 ? launch_skinny<EPI_ROPE, 2, true>(p, s) : launch_skinny<EPI_ROPE, 2, false>(p, s);
    if (e0 == TCAVT_EPI_SILU_MUL && !a->silu_preact && a->N % 32 == 0)
      return f16 ? launch_skinny<EPI_SILU, 2, true>(p, s) : launch_skinny<EPI_SILU, 2, false>(p, s);
    if ((e0 & TCAVT_EPI_NORM_OUT) && a->N % 16 == 0) {
      if (stream16) return f16 ? launch_skinny<EPI_NORM16, 1, true>(p, s) : launch_skinny<EPI_NORM16, 1, false>(p, s);
      return f16 ? launch_skinny<EPI_NORM, 1, true>(p, s) : launch_skinny<EPI_NORM, 1, false>(p, s);
    }
    if (e0 == 0 && K2 == 0 && a->N % 16 == 0) {
      // (lm_head with more than 16 rows: two column blocks per workgroup share the activation fragments -- with 16 columns
      //  the 32 activation rows are twice the weight bytes of every step, and the launch is bound by the CUs' load paths)
      if (a->M > 16 && a->N % 256 == 0 && a->N >= 8192)
        return f16 ? launch_skinny<EPI_GENERIC, 2, true>(p, s) : launch_skinny<EPI_GENERIC, 2, false>(p, s);
      return f16 ? launch_skinny<EPI_GENERIC, 1, true>(p, s) : launch_skinny<EPI_GENERIC, 1, false>(p, s);
    }
  }
  TCAVT_CHECK_ARG(!p.w_frag && !p.a_frag && !p.o_frag, "gemm_bf16: w_layout / act_layout: this epilogue / shape has no skinny form");
  if (epi & TCAVT_EPI_SILU_BWD) {  // dgrad of down_proj with d(silu(gate) * up) in the epilogue: the 4-wave kernel only
    TCAVT_CHECK_ARG(epi == TCAVT_EPI_SILU_BWD && batch == 1 && K2 == 0 && a->M % 256 == 0 && a->N % 256 == 0 && a->K >= 128 &&
                        a->silu_preact && aligned16(a->silu_preact) && a->dropout_p == 0.f && p.acc_scale == 1.f &&
                        a->out_dtype == (f16 ? TCAVT_F16 : TCAVT_BF16) && (a->tile == 0 || a->tile == 257),
                    "gemm_bf16: SILU_BWD runs on whole 256x256 tiles with silu_preact, a 16-bit output of the operand type and no other flag");
    p.aux = static_cast<bf16_t*>(a->silu_preact);
    p.ldaux = a->ld_preact;
    return f16 ? launch_w4<EPI_SILUBWD, true>(p, s) : launch_w4<EPI_SILUBWD, false>(p, s);
  }
  int tile = a->tile;
  if (tile == 0) {
    // 256x256 tiles when whole waves of 256 workgroups stay >= 75 % full (the fused q|k|v projection,
    // 32 x 12 = 384 tiles = 1.5 waves, is the boundary case: 111 us on 256x256 vs 114 us on 128x128).
    const long t256 = (long)((a->M + 255) / 256) * ((a->N + 255) / 256) * batch;
    const long waves = (t256 + 255) / 256;
    tile = (t256 >= 256 && (double)t256 / (double)(waves * 256) >= 0.75) ? 256 : 0;  // 0: dispatch_tile picks 128 / 64
    // whole 256x256 tiles, one K source, bf16, no RoPE: the 4-wave kernel (gate|up 406 vs 434 us, down 204 vs 218,
    // o 57.5 vs 60 on the 8-wave kernel)
    const bool silu_ok = (!(epi & TCAVT_EPI_SILU_MUL) || (a->out_dtype == (f16 ? TCAVT_F16 : TCAVT_BF16) && a->ldc % 8 == 0)) &&
                         (!(stream16 || (epi & TCAVT_EPI_ROPE)) || a->ldc % 8 == 0);  // (16-byte epilogue accesses of the 4-wave kernel)
    if (tile == 256 && batch == 1 && a->M % 256 == 0 && a->N % 256 == 0 && silu_ok &&
        ((epi & TCAVT_EPI_ROPE) ? a->out_dtype == (f16 ? TCAVT_F16 : TCAVT_BF16) : K2 == 0)) {
      tile = 257;
      // 256 x 192 tiles where they fill whole waves of 256 CUs and 256 x 256 tiles do not (q|k|v: N = 3072)
      if (a->N % 192 == 0) {
        const long t192 = (long)(a->M / 256) * (a->N / 192);
        const double f256 = (double)t256 / (double)(waves * 256), f192 = (double)t192 / (double)((t192 + 255) / 256 * 256);
        if (f192 > f256 + 0.1) tile = 271;
      }
      // long K (down projection, K = 8192): the two-barrier form with a whole K-tile of DMA in flight (190 vs 200 us);
      // neutral to slightly worse at K = 2048
      // (TCAVT_GEMM_DEEP_MINK=<K>: A/B switch for the threshold)
      static const int deep_mink = [] { const char* e = getenv("TCAVT_GEMM_DEEP_MINK"); return e ? atoi(e) : 4096; }();
      if (tile == 257 && !(epi & TCAVT_EPI_ROPE) && a->K >= deep_mink) tile = 272;
    }
  }
  if (epi & TCAVT_EPI_SILU_MUL) {
    if (a->silu_preact) {
      TCAVT_CHECK_ARG(aligned16(a->silu_preact) && a->ld_preact >= a->N && a->ld_preact % 4 == 0,
                      "gemm_bf16: silu_preact needs 16-byte alignment and ld_preact >= N, %% 4 == 0");
      p.aux = static_cast<bf16_t*>(a->silu_preact);
      p.ldaux = a->ld_preact;
      return f16 ? dispatch_tile<EPI_SILU_SAVE, true>(p, tile, 1, s) : dispatch_tile<EPI_SILU_SAVE, false>(p, tile, 1, s);
    }
    return f16 ? dispatch_tile<EPI_SILU, true>(p, tile, 1, s) : dispatch_tile<EPI_SILU, false>(p, tile, 1, s);
  }
  if (epi & TCAVT_EPI_ROPE) return f16 ? dispatch_tile<EPI_ROPE, true>(p, tile, 1, s) : dispatch_tile<EPI_ROPE, false>(p, tile, 1, s);
  if ((epi & TCAVT_EPI_NORM_OUT) && stream16)
    return f16 ? dispatch_tile<EPI_NORM16, true>(p, tile, 1, s) : dispatch_tile<EPI_NORM16, false>(p, tile, 1, s);
  if (epi & TCAVT_EPI_NORM_OUT) return f16 ? dispatch_tile<EPI_NORM, true>(p, tile, 1, s) : dispatch_tile<EPI_NORM, false>(p, tile, 1, s);
  if (a->dropout_p > 0.f) {  // small layers only (Q-Former, polygon encoder, LTSF): one 128x128 variant
    const int t = a->tile == 64 || a->tile == 128 ? a->tile : 0;
    return f16 ? launch_small<EPI_DROP, true>(p, t, 1, s) : launch_small<EPI_DROP, false>(p, t, 1, s);
  }
  if (f16) return dispatch_tile<EPI_GENERIC, true>(p, tile, batch, s);
  return dispatch_tile<EPI_GENERIC, false>(p, tile, batch, s);
}
