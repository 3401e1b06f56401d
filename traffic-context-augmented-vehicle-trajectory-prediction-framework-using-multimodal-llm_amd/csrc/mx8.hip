// MX8 (OCP MXFP8-E4M3, one E8M0 scale per 32 elements along K; include/tcavt.h, quant.py: quantize_mx): the quantise kernel
// and the block-scaled GEMM behind the opt-in MX8 MLP of the frozen decoder.
//
//   tcavt_quant_mx8   16-bit [M][K] -> e4m3 codes [M][K] + scale bytes [M][K / 32], byte for byte quant.quantize_mx
//   tcavt_gemm_mx8    C = A8 . W8^T with both operands' block scales applied inside v_mfma_scale_f32_16x16x128_f8f6f4
//
// The GEMM is the 128 x 128 two-stage form of gemm_tile8.hpp with one change of unit: a 128-byte row of codes is one 128-deep
// K-step, so the LDS image (128-byte rows, 16-byte chunks XOR-swizzled with (row >> 1) & 7, staged by LDS-DMA with the swizzle
// on the per-lane source address), the staging code and even the fragment addresses are the 16-bit kernel's.
//
// Operand lane map of the instruction, measured with exact one-hot data (tests/test_mx8_gpu.py: test_lane_map pins it): lane l,
// row l & 15, q = l >> 4, holds k = 16 q .. 16 q + 15 in operand registers 0-3 and k = 64 + 16 q .. 64 + 16 q + 15 in registers
// 4-7 -- chunks q and 4 + q of the 128-byte row -- and the scale byte a lane passes is that of 32-block q of its row (k = 32 q ..
// 32 q + 31), which the hardware applies to those k wherever they sit: registers 0-3 of lane groups 2 b and 2 b + 1 take the
// scale of group b, registers 4-7 that of group 2 + b.  (NOT 32 consecutive k per lane with the lane's own scale.)  The scale
// bytes of a K-step are one dword per tile row: 256 rows = 1 KiB = one 4-byte LDS-DMA per thread behind the codes of the stage.
// The MFMA is issued swapped like the 16-bit kernels' (weights = A operand), the accumulator layout is shape-determined, so
// gemm_epilogue<> runs on it unchanged.
#include "gemm_params.hpp"
#include "gemm_epilogue.hpp"

namespace tcavt {

typedef __attribute__((ext_vector_type(8))) int i32x8;

// ---------------------------------------------------------------------------
// Quantise.  A thread owns 8 consecutive elements (one 16-byte load), four threads a 32-block, sixteen a 128-column group
// (K % 128 == 0: never across rows), whose four scale bytes leave as one dword.  A wave instruction reads 1 KiB and writes
// 512 B of codes, both consecutive.
// ---------------------------------------------------------------------------
template <bool F16>
__global__ __launch_bounds__(256) void quant_mx8_kernel(const bf16_t* __restrict__ X, long ldx, unsigned char* __restrict__ codes, long ldc,
                                                        unsigned char* __restrict__ scales, long lds, long pieces, int kp) {
  const long piece = (long)blockIdx.x * 256 + threadIdx.x;
  if (piece >= pieces) return;  // (pieces % 16 == 0: a 16-lane group is in or out as a whole)
  const long row = piece / kp;
  const int c8 = (int)(piece - row * kp);
  const u32x4 v = *reinterpret_cast<const u32x4*>(X + row * ldx + c8 * 8);
  float x[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    x[2 * i] = from16_lo<F16>(v[i]);
    x[2 * i + 1] = from16_hi<F16>(v[i]);
  }
  unsigned int amax_bits = 0u;  // (non-negative floats order like their bit patterns; inf / NaN end up on top)
#pragma unroll
  for (int i = 0; i < 8; ++i) amax_bits = max(amax_bits, __builtin_bit_cast(unsigned int, x[i]) & 0x7fffffffu);
  amax_bits = max(amax_bits, (unsigned int)__shfl_xor((int)amax_bits, 1, 64));
  amax_bits = max(amax_bits, (unsigned int)__shfl_xor((int)amax_bits, 2, 64));
  const bool bad = amax_bits >= 0x7f800000u;
  int k = 0;
  if (!bad && amax_bits != 0u) {
    // (a magnitude below the smallest fp32 normal -- bf16 subnormals -- is below the clamp whatever its exponent)
    k = amax_bits < 0x00800000u ? -127 : max(-127, min(127, e4m3_row_exp(__builtin_bit_cast(float, amax_bits))));
  }
  u32x2 o = {0u, 0u};
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i >> 2] |= e4m3_code(ldexpf(x[i], -k)) << (8 * (i & 3));
  if (bad) o = u32x2{0x7f7f7f7fu, 0x7f7f7f7fu};
  *reinterpret_cast<u32x2*>(codes + row * ldc + c8 * 8) = o;
  unsigned int sb = (unsigned int)(k + 127);
  sb |= (unsigned int)__shfl_down((int)sb, 4, 64) << 8;
  sb |= (unsigned int)__shfl_down((int)sb, 8, 64) << 16;
  if ((threadIdx.x & 15) == 0) *reinterpret_cast<unsigned int*>(scales + row * lds + (c8 >> 4) * 4) = sb;
}

// ---------------------------------------------------------------------------
// GEMM: 128 x 128 output tile, 4 waves (2 x 2), each 64 x 64 = 4 x 4 MFMA tiles of 16 x 16; two LDS stages of
// 256 rows x 128 B of codes + 256 dwords of scale bytes; the DMA of K-step t + 1 is in flight under the MFMAs of K-step t,
// one drain + barrier per K-step.  (p.A / p.W point at bytes; p.lda / p.ldw are in bytes.)
// ---------------------------------------------------------------------------
constexpr int MX8_BM = 128, MX8_BN = 128, MX8_ROWS = MX8_BM + MX8_BN;
constexpr int MX8_CODE_BYTES = MX8_ROWS * 128, MX8_STAGE_BYTES = MX8_CODE_BYTES + MX8_ROWS * 4;

__device__ __forceinline__ void glds4(const void* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 4, 0, 0);
}

template <int EPI, bool F16>
__global__ __launch_bounds__(256) void gemm_mx8_kernel(GemmP p, const unsigned char* __restrict__ sa, long ldsa,
                                                       const unsigned char* __restrict__ sw, long ldsw) {
  constexpr int NW = 4, WTM = 64, WTN = 64, TM = 4, TN = 4;
  constexpr int ROUNDS = MX8_ROWS / (8 * NW);
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  int tile_m, tile_n;
  block_to_tile(p, tile_m, tile_n);
  const int m0 = tile_m * MX8_BM, n0 = tile_n * MX8_BN;

  // ---- per-lane staging sources: ROUNDS 16-byte pieces of codes and one dword of scale bytes per K-step
  const char* src[ROUNDS];
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int g = r * NW + wave;
    const int row = g * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((row >> 1) & 7);
    if (g * 8 < MX8_BM) src[r] = reinterpret_cast<const char*>(p.A) + (long)min(m0 + row, p.M - 1) * p.lda + c * 16;
    else src[r] = reinterpret_cast<const char*>(p.W) + (long)min(n0 + row - MX8_BM, p.N - 1) * p.ldw + c * 16;
  }
  const unsigned char* ssrc;  // tile row 64 wave + lane: waves 0, 1 the token rows, waves 2, 3 the weight rows
  if (wave < 2) ssrc = sa + (long)min(m0 + wave * 64 + lane, p.M - 1) * ldsa;
  else ssrc = sw + (long)min(n0 + (wave - 2) * 64 + lane, p.N - 1) * ldsw;
  const int nt = p.K >> 7;

  auto stage = [&](int buf, int t) {
    char* base = smem + buf * MX8_STAGE_BYTES;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) glds16(reinterpret_cast<const bf16_t*>(src[r] + t * 128), base + (r * NW + wave) * 1024);
    glds4(ssrc + t * 4, base + MX8_CODE_BYTES + wave * 256);
  };

  // ---- fragment read addressing: row 16 j + (lane & 15), chunks q and 4 + q (swizzled), scale byte q of the row's dword
  const int q = lane >> 4;
  const int fsw = (lane >> 1) & 7;  // == (row >> 1) & 7
  const int off0 = (q ^ fsw) * 16, off1 = ((4 + q) ^ fsw) * 16;
  const int xrow = wm * WTM + (lane & 15), wrow = MX8_BM + wn * WTN + (lane & 15);

  f32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  auto frag = [&](const char* base, int row, i32x8& f, int& s) {
    const u32x4 lo = *reinterpret_cast<const u32x4*>(base + row * 128 + off0);
    const u32x4 hi = *reinterpret_cast<const u32x4*>(base + row * 128 + off1);
    f = i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
    const unsigned int d = *reinterpret_cast<const unsigned int*>(base + MX8_CODE_BYTES + row * 4);
    s = (int)((d >> (8 * q)) & 0xffu);
  };

  auto compute = [&](int buf) {
    const char* base = smem + buf * MX8_STAGE_BYTES;
    i32x8 wf[TN], xf[TM];
    int ws[TN], xs[TM];
#pragma unroll
    for (int i = 0; i < TN; ++i) frag(base, wrow + i * 16, wf[i], ws[i]);
#pragma unroll
    for (int j = 0; j < TM; ++j) frag(base, xrow + j * 16, xf[j], xs[j]);
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[i], xf[j], acc[i][j], 0, 0, 0, ws[i], 0, xs[j]);
  };

  stage(0, 0);
  for (int t = 0; t < nt; ++t) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // K-step t is in LDS for everyone, and everyone is done with the stage K-step t + 1 goes to
    if (t + 1 < nt) stage((t + 1) & 1, t + 1);
    compute(t & 1);
  }
  gemm_epilogue<TM, TN, EPI, false, F16>(p, acc, m0 + wm * WTM, n0 + wn * WTN, lane);
}

template <int EPI, bool F16>
static int launch_mx8(const GemmP& p0, const tcavt_gemm_mx8_args* a, hipStream_t stream) {
  GemmP p = p0;
  p.tiles_m = (p.M + MX8_BM - 1) / MX8_BM;
  p.tiles_n = p.N / MX8_BN;
  p.xcd_gx = choose_xcd_partition(p);
  constexpr int lds = 2 * MX8_STAGE_BYTES;
  auto kfn = gemm_mx8_kernel<EPI, F16>;
  static bool attr_set = false;  // per instantiation
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) {
      set_error("gemm_mx8: hipFuncSetAttribute(%d B LDS) failed: %s", lds, hipGetErrorString(e));
      return TCAVT_ERR_HIP;
    }
    attr_set = true;
  }
  hipLaunchKernelGGL(kfn, dim3(p.tiles_m * p.tiles_n), dim3(256), lds, stream, p, static_cast<const unsigned char*>(a->A_scale),
                     (long)a->ldsa, static_cast<const unsigned char*>(a->W_scale), (long)a->ldsw);
  TCAVT_CHECK_LAUNCH("gemm_mx8");
  return TCAVT_OK;
}

}  // namespace tcavt

using namespace tcavt;

extern "C" int tcavt_quant_mx8(const void* X, int64_t ldx, int dtype16, void* codes, int64_t ldc, void* scales, int64_t lds, int M, int K,
                               tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(X && codes && scales && M > 0 && K > 0, "quant_mx8: null pointer or bad M / K");
  TCAVT_CHECK_ARG(K % 128 == 0, "quant_mx8: K=%d must be a multiple of 128", K);
  TCAVT_CHECK_ARG(is16(dtype16), "quant_mx8: dtype16 must be TCAVT_F16 or TCAVT_BF16");
  TCAVT_CHECK_ARG(ldx >= K && ldx % 8 == 0 && ldc >= K && ldc % 16 == 0 && lds >= K / 32 && lds % 4 == 0,
                  "quant_mx8: ldx >= K, %% 8 == 0; ldc >= K, %% 16 == 0; lds >= K / 32, %% 4 == 0");
  TCAVT_CHECK_ARG(aligned16(X) && aligned16(codes) && aligned16(scales), "quant_mx8: 16-byte alignment required");
  const long pieces = (long)M * (K / 8);
  auto kfn = dtype16 == TCAVT_F16 ? quant_mx8_kernel<true> : quant_mx8_kernel<false>;
  hipLaunchKernelGGL(kfn, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(X), (long)ldx, static_cast<unsigned char*>(codes), (long)ldc,
                     static_cast<unsigned char*>(scales), (long)lds, pieces, K / 8);
  TCAVT_CHECK_LAUNCH("quant_mx8");
  return TCAVT_OK;
}

extern "C" int tcavt_gemm_mx8(const tcavt_gemm_mx8_args* a, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(a != nullptr, "gemm_mx8: null args");
  const int epi = a->epilogue;
  const bool norm = (epi & ~TCAVT_EPI_RESIDUAL) == TCAVT_EPI_NORM_OUT;
  const bool silu = epi == (TCAVT_EPI_SILU_MUL | TCAVT_EPI_ROWSCALE);
  TCAVT_CHECK_ARG(epi == 0 || silu || norm,
                  "gemm_mx8: unsupported epilogue %d (0, SILU_MUL | ROWSCALE, or NORM_OUT with or without RESIDUAL)", epi);
  const bool stream16 = norm && a->C == nullptr;
  TCAVT_CHECK_ARG(a->A8 && a->A_scale && a->W8 && a->W_scale && (a->C || stream16), "gemm_mx8: null A8 / A_scale / W8 / W_scale / C");
  TCAVT_CHECK_ARG(a->M > 0 && a->N > 0 && a->K > 0 && a->K < (1 << 26), "gemm_mx8: bad M/N/K %d/%d/%d", a->M, a->N, a->K);
  TCAVT_CHECK_ARG(a->K % 128 == 0, "gemm_mx8: K=%d must be a multiple of 128", a->K);
  TCAVT_CHECK_ARG(a->N % 128 == 0, "gemm_mx8: N=%d must be a multiple of 128", a->N);
  TCAVT_CHECK_ARG(a->tile == 0 || a->tile == 128, "gemm_mx8: tile must be 0 (auto) or 128");
  TCAVT_CHECK_ARG(a->lda >= a->K && a->ldw >= a->K && a->lda % 16 == 0 && a->ldw % 16 == 0 && aligned16(a->A8) && aligned16(a->W8),
                  "gemm_mx8: lda / ldw must be >= K and multiples of 16, A8 / W8 16-byte aligned");
  TCAVT_CHECK_ARG(a->ldsa >= a->K / 32 && a->ldsw >= a->K / 32 && a->ldsa % 4 == 0 && a->ldsw % 4 == 0 &&
                      ((uintptr_t)a->A_scale & 3) == 0 && ((uintptr_t)a->W_scale & 3) == 0,
                  "gemm_mx8: ldsa / ldsw must be >= K / 32 and multiples of 4, the scale arrays 4-byte aligned");
  TCAVT_CHECK_ARG(a->out_dtype == TCAVT_F32 || is16(a->out_dtype), "gemm_mx8: bad out_dtype");
  TCAVT_CHECK_ARG(is16(a->dtype16), "gemm_mx8: dtype16 must be TCAVT_F16 or TCAVT_BF16");
  TCAVT_CHECK_ARG(a->out_dtype == TCAVT_F32 || a->out_dtype == a->dtype16, "gemm_mx8: a 16-bit output is of type dtype16");
  const int n_out = silu ? a->N / 2 : a->N;
  TCAVT_CHECK_ARG(a->ldc >= n_out && a->ldc % 4 == 0 && aligned16(a->C), "gemm_mx8: ldc=%ld too small or not a multiple of 4, or C not 16-byte aligned",
                  (long)a->ldc);

  GemmP p{};
  p.A = static_cast<const bf16_t*>(a->A8);
  p.W = static_cast<const bf16_t*>(a->W8);
  p.lda = a->lda; p.ldw = a->ldw; p.ldc = a->ldc; p.ldr = a->ldr;
  p.C = a->C;
  p.M = a->M; p.N = a->N; p.K = a->K;
  p.out_kind = a->out_dtype;
  p.flags = epi & ~TCAVT_EPI_ROWSCALE;
  p.acc_scale = 1.f;
  p.batch_inner = 1; p.w_group = 1;
  p.xcd_gx = 8;
  p.lp_scale = 1.f;
  p.sk_msplit = 1; p.sk_split = 1;
  p.norm_scale = 1.f;
  p.drop = make_dropout(0.f, 0, 0);
  if (silu) {
    TCAVT_CHECK_ARG(is16(a->out_dtype), "gemm_mx8: SILU_MUL writes a 16-bit output");
    TCAVT_CHECK_ARG(a->rowscale_part && aligned16(a->rowscale_part) && a->rowscale_npart > 0 && a->rowscale_npart % 4 == 0 && a->rowscale_h > 0,
                    "gemm_mx8: ROWSCALE needs rowscale_part, npart %% 4 == 0, h > 0");
    p.rs_part = a->rowscale_part;
    p.rs_npart = a->rowscale_npart;
    p.rs_eps = a->rowscale_eps;
    p.rs_inv_h = 1.f / (float)a->rowscale_h;
  }
  if (norm) {
    TCAVT_CHECK_ARG(a->out_dtype == TCAVT_F32 && a->norm_h16 && a->norm_part && aligned16(a->norm_h16),
                    "gemm_mx8: NORM_OUT goes with out_dtype = TCAVT_F32 and needs norm_h16 / norm_part");
    TCAVT_CHECK_ARG(a->norm_scale >= 0.f && a->norm_scale <= 1.f, "gemm_mx8: norm_scale must be in (0, 1] (0 means 1)");
    if (a->norm_scale != 0.f) p.norm_scale = a->norm_scale;
    if (stream16) {
      TCAVT_CHECK_ARG(a->residual == nullptr, "gemm_mx8: NORM_OUT with C == NULL keeps the residual stream in norm_h16: residual must be NULL");
      TCAVT_CHECK_ARG(a->norm_res16 == nullptr || aligned16(a->norm_res16), "gemm_mx8: norm_res16 needs 16-byte alignment");
    } else {
      TCAVT_CHECK_ARG(a->norm_res16 == nullptr, "gemm_mx8: norm_res16 goes with the 16-bit residual stream (NORM_OUT, C == NULL)");
      if (epi & TCAVT_EPI_RESIDUAL)
        TCAVT_CHECK_ARG(a->residual && aligned16(a->residual) && a->ldr >= a->N && a->ldr % 4 == 0,
                        "gemm_mx8: RESIDUAL needs residual pointer and ldr >= N");
      p.residual = a->residual;
    }
    p.norm_h16 = static_cast<bf16_t*>(a->norm_h16);
    p.norm_part = a->norm_part;
    p.res16 = a->norm_res16 ? static_cast<const bf16_t*>(a->norm_res16) : p.norm_h16;
    p.nf_flag = a->nonfinite_flag;
    p.nf_tag = a->nonfinite_tag;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool f16 = a->dtype16 == TCAVT_F16;
  if (silu) return f16 ? launch_mx8<EPI_SILU, true>(p, a, s) : launch_mx8<EPI_SILU, false>(p, a, s);
  if (stream16) return f16 ? launch_mx8<EPI_NORM16, true>(p, a, s) : launch_mx8<EPI_NORM16, false>(p, a, s);
  if (norm) return f16 ? launch_mx8<EPI_NORM, true>(p, a, s) : launch_mx8<EPI_NORM, false>(p, a, s);
  return f16 ? launch_mx8<EPI_GENERIC, true>(p, a, s) : launch_mx8<EPI_GENERIC, false>(p, a, s);
}
