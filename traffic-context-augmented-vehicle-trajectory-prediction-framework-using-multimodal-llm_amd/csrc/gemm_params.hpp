// What every form of the 16-bit GEMM (gemm_bf16.hip) shares: the kernel parameter block, the epilogue codes, the fused-RMSNorm
// row scale, the LDS-DMA primitive and the workgroup -> output tile map with its host-side XCD partition rule.
#pragma once
#include "common.hpp"
#include "philox.hpp"
#include <stdlib.h>

namespace tcavt {

struct GemmP {
  const bf16_t* A;
  const bf16_t* W;
  const bf16_t* A2;
  const bf16_t* W2;
  void* C;
  const float* bias;
  const float* residual;
  const float* cosT;
  const float* sinT;
  long lda, ldw, lda2, ldw2, ldc, ldr;
  int M, N, K, K2;
  int out_kind, flags, rope_L, rope_cols;  // out_kind: TCAVT_F32 / TCAVT_BF16 / TCAVT_F16
  int tiles_m, tiles_n;
  float acc_scale;
  int batch_inner;
  bf16_t* aux;  // EPI_SILU_SAVE: gate|up pre-activations [M, N] bf16
  long ldaux;
  int w_group;  // >= 1: the inner batch index is divided by this for W (grouped-query heads share one W)
  long sAo, sAi, sWo, sWi, sCo, sCi;
  int xcd_gx;  // XCD partition of the tile grid (block_to_tile)
  DropoutP drop;  // epilogue dropout (generic epilogue only)
  int pers_tiles;  // > 0: persistent launch of the 4-wave kernel, workgroup w runs tiles w, w + gridDim.x, ... < pers_tiles
  int prio;  // wave priority in the 8-wave kernel: 0 none, 2 s_setprio(1) around the MFMA clusters (tile code 256).  1 (static priority
             // for the upper half of the waves, measured and rejected) is set by no dispatch path; the kernel keeps its test because
             // the register allocation of 26 instantiations depends on it (profiles/gemm_source_split.txt)
  // ---- RMSNorm fused into the GEMMs around it (TCAVT_EPI_NORM_OUT / TCAVT_EPI_ROWSCALE, include/tcavt.h)
  bf16_t* norm_h16;       // NORM_OUT: 16-bit copy of the fp32 output rows (leading dimension ldc)
  float* norm_part;       // NORM_OUT: [M][N / 64] sums of squares of the fp32 output, one per 64-column group
  const float* rs_part;   // ROWSCALE: [M][rs_npart] sums of squares of the row the A operand was rounded from
  int rs_npart;
  float rs_eps, rs_inv_h;
  const int* rope_pos;    // ROPE: position of row m (decode step: one row per sample); NULL: m % rope_L
  const bf16_t* res16;    // NORM16: where the 16-bit residual is read from (norm_h16 itself unless the caller keeps every layer's stream)
  // skinny form, split K across workgroups (decode step): S = sk_split workgroups share one block of output columns, each
  // over K / S; partial sums meet in sk_slab, the last arriver (ticket in sk_cnt) adds them in slice order and finishes
  // skinny form (decode step): the NEXT layer's LoRA down-projection folded into this layer's residual GEMM and q|k|v GEMM.
  // Producer (NORM_OUT forms, lp_a != nullptr): every workgroup also writes t_part[blk][m][16] = its 16 output columns of the
  // rounded stream times the 16 adapter rows (A_q rows 0..7, A_v rows LORA_V..LORA_V+7 of a_cat).  Consumer (RoPE form,
  // lp_np > 0): t = round16(lp_scale * sum over the lp_np partials, in index order) replaces the A2 operand (K2 = 32).
  float* lp_part;
  const bf16_t* lp_a;
  long lp_lda;
  int lp_np;
  float lp_scale;
  // skinny form, M > 16: the two 16-token blocks of a column block go to TWO workgroups (sk_msplit = 2) instead of one that
  // loads both blocks' activation rows for every weight fragment (twice the weight bytes through the CU's load path)
  int sk_msplit;
  int a_frag, o_frag;  // skinny form: A / the 16-bit result in fragment-major order (tcavt_gemm_args.act_layout): 0, 1 = blocks of 16
                       // tokens, 2 = one block of 8 (common.hpp frag_off)
  int w_frag;  // skinny form: W is the fragment-major copy of tcavt_pack_weight16 (1) or the FP8 copy of tcavt_pack_weight8 (2)
               // (tcavt_gemm_args.w_layout)
  int sk_split;
  float* sk_slab;
  int* sk_cnt;
  long sk_slab_bytes;
  int sk_cnt_n;
  int* nf_flag;           // NORM_OUT: receives nf_tag (CAS from 0) when a partial sum / rounded element is not finite
  int nf_tag;
  float norm_scale;       // NORM_OUT: the 16-bit image of the stream (and its partial sums) holds norm_scale * x (tcavt_gemm_args.norm_scale)
  int res_pf;             // NORM16 + RESIDUAL in the 4-wave kernel: the residual tile arrives by LDS-DMA in the look-ahead slots past a
                          // workgroup's last K-tile (set by launch_w4 at every launch; TCAVT_GEMM_NO_RES_PREFETCH=1 clears it)
};

// a * s + b, one rounding (s = 1: exactly a + b, so the default scale leaves every result bit for bit as it was)
__device__ __forceinline__ f32x4 fma4(const f32x4& a, float s, const f32x4& b) {
  return __builtin_elementwise_fma(a, f32x4{s, s, s, s}, b);
}

// a non-finite partial sum of squares (inf: a rounded element overflowed; NaN: inf / NaN came in from upstream)
__device__ __forceinline__ void flag_nonfinite(const GemmP& p, float ss) {
  if (p.nf_flag && !(ss <= 3.0e38f)) atomicCAS(p.nf_flag, 0, p.nf_tag);
}

// 1 / rms of row m from its partial sums of squares, added in index order (bit-reproducible; rs_npart % 4 == 0)
__device__ __forceinline__ float row_rscale(const GemmP& p, long m) {
  const f32x4* q = reinterpret_cast<const f32x4*>(p.rs_part + m * p.rs_npart);
  float ss = 0.f;
  const int nq = p.rs_npart >> 2;
  // eight quads (H = 2048: all of them) in flight together -- one load per step, each waited for, was eight dependent
  // L2 round trips per output tile of the persistent kernel
  for (int i0 = 0; i0 < nq; i0 += 8) {
    f32x4 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = q[min(i0 + i, nq - 1)];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (i0 + i < nq) {
        ss += v[i][0];
        ss += v[i][1];
        ss += v[i][2];
        ss += v[i][3];
      }
    }
  }
  return rsqrtf(ss * p.rs_inv_h + p.rs_eps);
}

// EPI_DROP = EPI_GENERIC + Philox dropout.  A separate instantiation: with the mask code inside the generic
// epilogue the 256x256 kernel spilled its accumulators (528 B/lane of scratch, 3x slower).
// EPI_SILU_SAVE = EPI_SILU + a bf16 copy of the gate|up pre-activations (LoRA-trainable variant: the backward of
// silu(gate)*up needs them); its own instantiation so that the production SiLU kernel keeps its register allocation.
// EPI_NORM = TCAVT_EPI_NORM_OUT (fp32 residual output + 16-bit copy + per-row partial sums of squares): its own
// instantiation as well -- inside EPI_GENERIC it pushed the 4-wave kernel's generic form into 460 bytes of scratch.
// EPI_NORM16 = the same with C == NULL (16-bit residual stream, updated in place): again its own instantiation (both bodies in
// one kernel spilled 150-500 bytes per lane in the 4-wave kernel).
// EPI_SILUBWD = TCAVT_EPI_SILU_BWD (4-wave kernel only).
enum { EPI_GENERIC = 0, EPI_SILU = 1, EPI_ROPE = 2, EPI_DROP = 3, EPI_SILU_SAVE = 4, EPI_NORM = 5, EPI_NORM16 = 6, EPI_SILUBWD = 7 };

__device__ __forceinline__ void glds16(const bf16_t* src, char* lds_wave_base) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)src,
      (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// ---------------------------------------------------------------------------
// Workgroup -> output tile.  Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8 labels the
// XCD, each with a private 4 MiB L2), so the grid is cut into gx x gy rectangles of tiles, one per XCD
// (gx * gy = 8): an XCD then streams 1/gx of the activation rows and 1/gy of the weight rows, and the
// fabric / Infinity-Cache traffic of the launch is  gy * |A| + gx * |W|.  The host picks (gx, gy) that
// minimises it (p.xcd_gx; 8 = row bands, the right choice whenever |A| >= |W|).  Inside its rectangle an
// XCD walks 4-tile-tall super rows so that its 32 CUs work on a 4 x 8 patch at any time.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void block_to_tile(const GemmP& p, int& tile_m, int& tile_n, int bid, int nwg) {
  constexpr int GM = 4;
  const int gx = p.xcd_gx;
  if (gx != 8) {  // 2-D partition; the host guarantees tiles_m % gx == 0 and tiles_n % (8 / gx) == 0
    const int gy = 8 / gx;
    const int xcd = bid & 7, local = bid >> 3;
    const int xi = xcd / gy, xj = xcd - xi * gy;
    const int sm = p.tiles_m / gx, sn = p.tiles_n / gy;
    const int per_group = GM * sn;
    const int g = local / per_group, in_g = local - g * per_group;
    const int gsz = min(GM, sm - g * GM);
    tile_m = xi * sm + g * GM + in_g % gsz;
    tile_n = xj * sn + in_g / gsz;
    return;
  }
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  const int wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  const int per_group = GM * p.tiles_n;
  const int g = wgid / per_group, in_g = wgid - g * per_group;
  const int gsz = min(GM, p.tiles_m - g * GM);
  tile_m = g * GM + in_g % gsz;
  tile_n = in_g / gsz;
}

__device__ __forceinline__ void block_to_tile(const GemmP& p, int& tile_m, int& tile_n) {
  block_to_tile(p, tile_m, tile_n, blockIdx.x, gridDim.x);
}

// (gx, gy) minimising gy * |A| + gx * |W| -- the bytes the eight XCDs pull over the fabric -- among the partitions the
// tile grid divides evenly into whole super rows; ties go to the larger gx (row bands).  Round 1 weighted W three times
// (HBM-cold weights vs activations served from the Infinity Cache); re-measured in the model in round 2 with the fused-norm
// epilogues (forward pass, one box, us per launch for gx = 1 / 2 / 4 / 8):
//     q|k|v 116.2 / 113.4 / 112.5 / 118.1    o 104.4 / 97.2 / 96.1 / 89.5    gate|up 448.7 / 441.0 / 439.9 / 440.0
//     down 249.4 / 245.9 / 245.6 / 243.8
// which the unweighted byte count reproduces (q|k|v -> 4, o -> 8, gate|up -> 2, down -> 8).
// TCAVT_GEMM_XCD_GX=<1|2|4|8> forces a partition (A/B runs).
static int choose_xcd_partition(const GemmP& p) {
  static const int forced = [] {
    const char* e = getenv("TCAVT_GEMM_XCD_GX");
    return e ? atoi(e) : 0;
  }();
  const double a_bytes = (double)p.M * p.K, w_bytes = (double)p.N * p.K;
  int best = 8;
  double best_cost = 1.0 * a_bytes + 8.0 * w_bytes;
  for (int gx = 4; gx >= 1; gx /= 2) {
    const int gy = 8 / gx;
    if (p.tiles_m % gx || p.tiles_n % gy || (p.tiles_m / gx) % 4 || (long)p.tiles_m * p.tiles_n % 8) continue;
    if (forced == gx) return gx;
    const double cost = gy * a_bytes + gx * w_bytes;
    if (cost < best_cost) {
      best_cost = cost;
      best = gx;
    }
  }
  return forced == 8 ? 8 : best;
}

}  // namespace tcavt
