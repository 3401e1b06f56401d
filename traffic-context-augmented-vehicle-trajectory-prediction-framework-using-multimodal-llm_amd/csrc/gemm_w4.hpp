// The 4-wave GEMM kernel on whole 256-row tiles: tile codes 257 (256 x 256), 271 (256 x 192) and 272 (256 x 256, DEEP).
#pragma once
#include "gemm_epilogue.hpp"

namespace tcavt {

// ===========================================================================
// Main-loop variant 3 ("w4", 256x256 tile, whole tiles only): FOUR waves, one per SIMD, each owning a
// 128x128 quadrant (8x8 MFMA tiles = 256 accumulator registers, which the unified 512-entry file holds as
// AGPRs when a SIMD runs a single wave).  Compared with the 2x4-wave kernel above this reads a third less
// LDS per MFMA (16 fragment loads per 64 MFMAs instead of 12 per 32) and software-pipelines the fragment
// loads inside the wave: the fragments of the next 32-deep K-step are loaded into a second register set
// while the 64 MFMAs of the current one run, across the tile barrier as well -- the barrier sits 16 MFMAs
// before the end of a K-tile, and those 16 cover the first fragment loads of the next tile:
//
//   phase A : 64 MFMA on F0(t)  | ds_read F1(t)   | DMA pieces 4..15 of tile t+1 (one per 5 MFMAs)
//   phase B1: 48 MFMA on F1(t)
//   vmcnt(0) + barrier           (tile t+1 landed for everyone; everyone is done reading tile t)
//   phase B2: 16 MFMA on F1(t)  | ds_read F0(t+1) | DMA pieces 0..3 of tile t+2
//
// Same LDS image as the kernel above (128-byte rows, XOR-swizzled 16-byte chunks, two 64 KiB buffers).
//
// Residual prefetch (EPI_NORM16 with TCAVT_EPI_RESIDUAL, p.res_pf): the look-ahead of a workgroup's LAST output tile has no
// operands left to fetch -- "K-tiles" nt and nt + 1 of that tile carry the tile's 16-bit residual instead (256 x 256 x 2 bytes
// = the two 64 KiB buffers), and the epilogue reads it from LDS.  Image: K-tile nt + h holds columns [128 wn + 64 h, + 64) of
// every wave's 128 x 128 quadrant; piece r of wave w is rows 8 r .. 8 r + 7 of w's quadrant, 128 bytes of each (whole lines,
// as for the operands), and inside the piece lane i sits where the epilogue's lane with (lane & 7) = i & 7, lane >> 4 =
// (i >> 3) & 3 reads the 16 bytes of its tile pair (i >> 5): see locate_res below and gemm_epilogue.  Every wave fetches its own rows.
// ===========================================================================
// MFMA with the accumulator pinned to AGPRs and tied in place.  Written as inline asm because the compiler's
// VGPR/AGPR rewriting turned the 256-register accumulator of the 4-wave kernel into ~350 v_accvgpr copies per K-tile.
template <bool F16>
__device__ __forceinline__ void mfma_agpr(f32x4& c, const bf16x8& a, const bf16x8& b) {
  if constexpr (F16) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
  else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}

// Template parameters of the kernel and of launch_w4, in this order:
//   EPI   the epilogue.
//   F16   the operands' 16-bit type (fp16 / bf16).
//   BN    256: 2 x 2 waves of 128 x 128.  192: 4 x 1 waves of 64 x 192 (4 x 12 MFMA tiles, 192 accumulator registers) for
//         N = 3072 (fused q|k|v): 512 tiles = two full waves of 256 CUs instead of 384 = one and a half.
//   DEEP  the two-barrier deep-prefetch form of the main loop (tile code 272, long K: the down projection); see below.
//   B2R   rows of MFMA tiles (of the wave's TN) issued behind the end-of-tile barrier (phase B2): 2 for BN = 256, 4 for BN = 192.
// Instantiations that may run persistently (one workgroup per CU walking its tiles as one K-tile stream): not RoPE (falls
// apart into 1.7 KB of scratch with it); not the generic epilogue in the DEEP form (924 bytes of scratch with it -- the
// backward's long-K dgrad GEMMs are one tile per CU anyway).
constexpr bool w4_pers_ok(int epi, bool deep) {
  return epi != EPI_ROPE && !(deep && epi == EPI_GENERIC);
}

template <int EPI, bool F16, int BN = 256, bool DEEP = false, int B2R = (BN == 256 ? 2 : 4)>
__global__ __launch_bounds__(256) void gemm_bf16_w4_kernel(GemmP p) {
  constexpr int BM = 256, NW = 4;
  constexpr int WN_ = BN == 256 ? 2 : 1, WM_ = NW / WN_;
  constexpr int TM = BM / WM_ / 16, TN = BN / WN_ / 16;
  static_assert(TM + TN == 16, "the fragment pipeline assumes 16 fragment loads per 32-deep K-step");
  constexpr int TILE_BYTES = (BM + BN) * 128;
  constexpr int NP = (BM + BN) / 32;  // DMA pieces (8 rows x 128 B per wave-instruction) per thread and K-tile
  constexpr int NB2 = B2R * TM;     // MFMAs after the barrier (phase B2)
  // DEEP: a second barrier in the middle of phase A, where every wave holds all
  // fragments of tile t in registers, frees tile t's LDS buffer a whole K-tile earlier; the 16 pieces of tile t+2 are
  // issued behind it (one per 4 MFMAs over the rest of phase A and phase B1) and stay in flight ACROSS the end-of-B1
  // barrier, which waits with a counted vmcnt(NP) for the older tile t+1 only.  Every piece gets >= one full K-tile
  // (2048 MFMA cycles) to land instead of 0.4-1.2.
  static_assert(!DEEP || (TM == 8 && TN == 8), "DEEP is laid out for the 2x2-wave form");
  constexpr int EARLY = NB2 / 4;             // pieces of tile t+2 issued in phase B2 of tile t
  constexpr int SPREAD = (TM * TN) / (NP - EARLY);  // phase A: one DMA piece per SPREAD MFMAs
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave / WN_, wn = wave % WN_;
  // fused RMSNorm (TCAVT_EPI_ROWSCALE): the 256 row scales of the output tile, behind the two tile buffers
  constexpr bool RS = EPI == EPI_SILU || EPI == EPI_SILU_SAVE || EPI == EPI_ROPE;
  // (two sets, used alternately by consecutive output tiles of the persistent form: the next tile's scales are written
  // BEFORE this tile's epilogue, so that nothing has to be loaded, waited for or published behind the epilogue's stores)
  float* const rs_base = reinterpret_cast<float*>(smem + 2 * TILE_BYTES);
  int rs_sel = 0;  // (uniform) the set the current output tile reads
  // Persistent form (p.pers_tiles > 0): this workgroup walks tiles vb = blockIdx.x, + gridDim.x, ... as ONE stream of
  // K-tiles -- the look-ahead of the pipeline (fragments of the next K-tile, DMA of the next two) simply continues into
  // the next output tile, so its first operands arrive while this tile's epilogue runs (no per-tile prologue).
  // (round 4: the two-barrier DEEP form walks its tiles as one K-tile stream as well -- it used to start every output tile with a
  //  burst prologue, which is what it lost to the one-barrier form at K = 2048, 8 tiles per CU)
  constexpr bool PERS_OK = w4_pers_ok(EPI, DEEP);
  const bool pers = PERS_OK && p.pers_tiles > 0;
  const int total_tiles = pers ? p.pers_tiles : (int)gridDim.x;
  int vb = blockIdx.x;
  int tile_m, tile_n;
  block_to_tile(p, tile_m, tile_n, vb, total_tiles);
  int m0 = tile_m * BM, n0 = tile_n * BN;

  // DMA sources: piece r of a K-tile is the 8-row group g = 4 r + wave (r < 8: activation rows, r >= 8:
  // weight rows).  The swizzle term of a lane does not depend on r (32-row steps), so one base per operand.
  const int rl = lane >> 3;
  const int csw = (lane & 7) ^ (((wave & 1) * 4 + (rl >> 1)) & 7);
  const bf16_t* srcA = p.A + (long)(m0 + wave * 8 + rl) * p.lda + csw * 8;
  const bf16_t* srcW = p.W + (long)(n0 + wave * 8 + rl) * p.ldw + csw * 8;
  const long stepA = 32 * p.lda, stepW = 32 * p.ldw;
  // next output tile of this workgroup (persistent form): where the look-ahead continues
  bool has_next = pers && vb + (int)gridDim.x < total_tiles;
  int nm0 = m0, nn0 = n0;
  const bf16_t* nxtA = srcA;
  const bf16_t* nxtW = srcW;
  auto locate_next = [&]() {
    if (has_next) {
      int tm, tn;
      block_to_tile(p, tm, tn, vb + (int)gridDim.x, total_tiles);
      nm0 = tm * BM;
      nn0 = tn * BN;
      nxtA = p.A + (long)(nm0 + wave * 8 + rl) * p.lda + csw * 8;
      nxtW = p.W + (long)(nn0 + wave * 8 + rl) * p.ldw + csw * 8;
    }
  };
  locate_next();
  // second K source (LoRA: A2 = x.A_cat^T, W2 = B_ext): its 64-deep tiles follow the main ones
  constexpr bool HASK2 = EPI == EPI_ROPE;  // only the fused q|k|v projection uses it
  const bf16_t* srcA2 = nullptr;
  const bf16_t* srcW2 = nullptr;
  long stepA2 = 0, stepW2 = 0;
  // residual prefetch: this lane's source in the residual tile of (m0, n0) (rows 8 r + (lane & 7) of the wave's quadrant for piece
  // r; the tile pair (lane >> 5) of a 64-column half; the 16 bytes pair16_off() gives the epilogue lane (lane >> 3) & 3 rows of 16 on)
  constexpr bool RPF = EPI == EPI_NORM16 && BN == 256;
  const bool rpf = RPF && p.res_pf;
  bool tail_res = false;  // (uniform) no next output tile: the look-ahead past the last K-tile carries this tile's residual
  long nstepA = 0, nstepW = 0;  // piece strides of the look-ahead source past the last K-tile (next tile's operands / residual rows)
  auto locate_res = [&]() {
    if constexpr (RPF) {
      tail_res = rpf && !has_next;
      nstepA = stepA;
      nstepW = stepW;
      if (tail_res) {
        nxtA = p.res16 + (long)(m0 + wm * 128 + (lane & 7)) * p.ldc + n0 + wn * 128 + (lane >> 5) * 32 + pair16_off(((lane >> 3) & 3) << 4);
        nxtW = nxtA + 64 * p.ldc;
        nstepA = nstepW = 8 * p.ldc;
      }
    }
  };
  const int nt1 = p.K >> 6;
  int nt = nt1;
  auto locate_k2 = [&]() {
    if constexpr (HASK2) {
      if (p.K2 > 0) {
        srcA2 = p.A2 + (long)(m0 + wave * 8 + rl) * p.lda2 + csw * 8;
        srcW2 = p.W2 + (long)(n0 + wave * 8 + rl) * p.ldw2 + csw * 8;
      }
    }
  };
  if constexpr (HASK2) {
    if (p.K2 > 0) {
      stepA2 = 32 * p.lda2;
      stepW2 = 32 * p.ldw2;
      nt += p.K2 >> 6;
    }
  }
  locate_k2();
  locate_res();

  struct Src {
    const bf16_t* a;
    const bf16_t* w;
    long sa, sw;
  };
  auto tsrc = [&](int t) -> Src {
    if constexpr (PERS_OK) {
      if constexpr (RPF) {  // ... or the two halves of this tile's residual
        if (t >= nt && (has_next || tail_res)) return Src{nxtA + (t - nt) * 64, nxtW + (t - nt) * 64, nstepA, nstepW};
      } else {
        if (t >= nt && has_next) return Src{nxtA + (t - nt) * 64, nxtW + (t - nt) * 64, stepA, stepW};  // next tile's first K-tiles
      }
    }
    t = min(t, nt - 1);  // the last two K-tiles re-fetch the last tile into a free buffer (keeps the loop body uniform)
    if constexpr (HASK2) {
      if (t >= nt1) return Src{srcA2 + (t - nt1) * 64, srcW2 + (t - nt1) * 64, stepA2, stepW2};
    }
    return Src{srcA + t * 64, srcW + t * 64, stepA, stepW};
  };
  auto piece = [&](int buf, const Src& s, int r) {
    char* dst = smem + buf * TILE_BYTES + (r * NW + wave) * 1024;
    if (r < 8)
      glds16(s.a + r * s.sa, dst);
    else
      glds16(s.w + (r - 8) * s.sw, dst);
  };

  const int fsw = (lane >> 1) & 7;
  const int off0 = ((lane >> 4) ^ fsw) * 16;
  const int off1 = ((4 + (lane >> 4)) ^ fsw) * 16;
  const int xrow = (wm * TM * 16 + (lane & 15)) * 128;
  const int wrow = (BM + wn * TN * 16 + (lane & 15)) * 128;

  f32x4 acc[TN][TM];
#pragma unroll
  for (int i = 0; i < TN; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  bf16x8 w0[TN], x0[TM], w1[TN], x1[TM];
  auto ldx = [&](const char* base, int off, int j) { return *reinterpret_cast<const bf16x8*>(base + xrow + j * 2048 + off); };
  auto ldw = [&](const char* base, int off, int i) { return *reinterpret_cast<const bf16x8*>(base + wrow + i * 2048 + off); };

  // ---- prologue: tile 0 (burst), publish, first pieces of tile 1, fragments F0(0)
  if constexpr (RS) {  // (the partial-sum loads are in flight together with tile 0's DMA; written before the barrier below)
    if (p.rs_part) rs_base[threadIdx.x] = row_rscale(p, m0 + threadIdx.x);
  }
  {
    const Src s0 = tsrc(0);
#pragma unroll
    for (int r = 0; r < NP; ++r) piece(0, s0, r);
  }
  __syncthreads();
  Src sn1 = tsrc(1);  // source of tile t+1, carried from iteration to iteration (sn1(t+1) = sn2(t))
  if constexpr (DEEP) {
#pragma unroll
    for (int r = 0; r < NP; ++r) piece(1, sn1, r);  // all of tile 1 (tsrc clamps when there is none: harmless re-fetch)
  } else if (nt > 1 || (RPF && tail_res)) {
#pragma unroll
    for (int r = 0; r < EARLY; ++r) piece(1, sn1, r);
  }
#pragma unroll
  for (int j = 0; j < TM; ++j) x0[j] = ldx(smem, off0, j);
#pragma unroll
  for (int i = 0; i < TN; ++i) w0[i] = ldw(smem, off0, i);

  // One K-tile.  The loop body is one branch-free scheduling region for every tile: the last two K-tiles of a launch issue
  // their look-ahead like any other (tsrc clamps it to a harmless re-fetch of the last tile into a free buffer).
  int cur = 0;
  auto ktile = [&](int t) {
    const char* base = smem + cur * TILE_BYTES;
    const char* nbase = smem + (cur ^ 1) * TILE_BYTES;
    Src sn2;  // source of tile t+2, put together step by step in the shadow of the bare MFMAs of phase B1
    int koff2 = 0;
    bool second2 = false, into_next2 = false;
    // ---- phase A: MFMAs on F0 | load F1 (second 32-deep half of tile t) | rest of the DMA for tile t+1
#pragma unroll
    for (int i = 0; i < TN; ++i) {
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        mfma_agpr<F16>(acc[i][j], w0[i], x0[j]);
        const int idx = i * TM + j;
        if (idx < 32 && (idx & 1) == 0) {  // 16 fragment loads, one per 2 MFMAs
          const int f = idx >> 1;
          if (f < TM) x1[f] = ldx(base, off1, f);
          else w1[f - TM] = ldw(base, off1, f - TM);
        }
        if constexpr (DEEP) {
          if (idx == 0) {
            into_next2 = PERS_OK && (has_next || (RPF && tail_res)) && t + 2 >= nt;   // the look-ahead crosses into the next output tile (or the residual)
            const int tt = into_next2 ? t + 2 - nt : min(t + 2, nt - 1);  // clamp: see tsrc
            second2 = HASK2 && !into_next2 && tt >= nt1;
            koff2 = (second2 ? tt - nt1 : tt) * 64;
          }
          if (idx == 3) sn2.a = (into_next2 ? nxtA : second2 ? srcA2 : srcA) + koff2;
          if (idx == 6) sn2.w = (into_next2 ? nxtW : second2 ? srcW2 : srcW) + koff2;
          if (idx == 9) {
            sn2.sa = second2 ? stepA2 : (RPF && into_next2) ? nstepA : stepA;
            sn2.sw = second2 ? stepW2 : (RPF && into_next2) ? nstepW : stepW;
          }
          if (idx == 39) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // tile t is in registers everywhere
          if (idx >= 43 && (idx & 3) == 3) piece(cur, sn2, (idx - 43) / 4);  // pieces 0..5 of tile t+2
        } else {
          if (idx % SPREAD == SPREAD - 1 && EARLY + idx / SPREAD < NP) piece(cur ^ 1, sn1, EARLY + idx / SPREAD);
        }
      }
    }
    // ---- phase B1: first 48 MFMAs on F1
#pragma unroll
    for (int i = 0; i < TN - B2R; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        mfma_agpr<F16>(acc[i][j], w1[i], x1[j]);
        const int idx = i * TM + j;
        if constexpr (DEEP) {
          if ((idx & 3) == 3 && 6 + idx / 4 < NP) piece(cur, sn2, 6 + idx / 4);  // pieces 6..15 of tile t+2
          continue;
        }
        if (idx == 0) {
          into_next2 = PERS_OK && (has_next || (RPF && tail_res)) && t + 2 >= nt;   // the look-ahead crosses into the next output tile (or the residual)
          const int tt = into_next2 ? t + 2 - nt : min(t + 2, nt - 1);  // clamp: see tsrc
          second2 = HASK2 && !into_next2 && tt >= nt1;
          koff2 = (second2 ? tt - nt1 : tt) * 64;
        }
        if (idx == 3) sn2.a = (into_next2 ? nxtA : second2 ? srcA2 : srcA) + koff2;
        if (idx == 6) sn2.w = (into_next2 ? nxtW : second2 ? srcW2 : srcW) + koff2;
        if (idx == 9) {
          sn2.sa = second2 ? stepA2 : (RPF && into_next2) ? nstepA : stepA;
          sn2.sw = second2 ? stepW2 : (RPF && into_next2) ? nstepW : stepW;
        }
      }
    if (DEEP) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(NP) : "memory");  // tile t+1 landed; t+2 in flight
    else __syncthreads();  // tile t+1 has landed for everyone; nobody reads tile t any more
    // ---- phase B2: last 16 MFMAs on F1 | load F0 of tile t+1 | first DMA pieces of tile t+2
#pragma unroll
    for (int i = TN - B2R; i < TN; ++i) {
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        mfma_agpr<F16>(acc[i][j], w1[i], x1[j]);
        const int idx = (i - (TN - B2R)) * TM + j;  // 0..NB2-1
        if (TM == TN && idx < TM) {  // the 16 fragment loads go first, two per MFMA
          x0[idx] = ldx(nbase, off0, idx);
          w0[idx] = ldw(nbase, off0, idx);
        }
        if (TM != TN && idx < 16) {  // unequal fragment counts: one per MFMA
          if (idx < TM) x0[idx] = ldx(nbase, off0, idx);
          else w0[idx - TM] = ldw(nbase, off0, idx - TM);
        }
        if (!DEEP && (idx & 3) == 3 && (idx >> 2) < EARLY) piece(cur, sn2, idx >> 2);
      }
    }
    // Last K-tile of an output tile: the accumulators are read next (the epilogue's v_accvgpr_read, but also AGPR-to-AGPR
    // copies the register allocator may place on the loop-exit edge, BEFORE any statement that follows the loop).  The
    // compiler cannot see the MFMA write latency behind the inline asm, so the wait states sit here, inside the loop
    // body, where nothing can be scheduled between them and the last MFMA (one scalar compare + branch per K-tile).
    if (t == nt - 1) asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    cur ^= 1;
    sn1 = sn2;
  };
  for (;;) {
    for (int t = 0; t < nt; ++t) ktile(t);
    // residual prefetch, one-barrier form: only the EARLY pieces of the second half fitted behind the last end-of-tile barrier
    // (phase B2); the rest goes out here, into the buffer of the last K-tile (nobody reads it any more).  The DEEP form has
    // issued both halves inside the loop.
    const bool from_lds = RPF && tail_res;  // (uniform) this output tile's residual is in LDS / on its way there
    if constexpr (RPF && !DEEP) {
      if (from_lds) {
#pragma unroll
        for (int r = EARLY; r < NP; ++r) piece(cur ^ 1, sn1, r);
      }
    }
    // the accumulators are read by VALU next: cover the MFMA write latency the compiler cannot see behind the asm
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    // ... and pin every accumulator read behind those nops: an empty volatile asm that redefines the register is
    // ordered after the s_nop asm, and the epilogue's v_accvgpr_read depends on it (without this the scheduler is
    // free to hoist the reads above the nops -- one instantiation did, and read stale values)
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j) asm volatile("" : "+a"(acc[i][j]));
    // ---- everything of the NEXT output tile that reads memory comes BEFORE this tile's stores: vmcnt counts loads and
    // stores in one queue, so a load waited for after the epilogue (the next tile's row scales; any register the allocator
    // chose to spill around the K loop) would first wait for the whole store tail to drain -- per output tile.
    const int em0 = m0, en0 = n0;
    const bool cont = PERS_OK && has_next;  // (uniform) non-persistent launches leave after the epilogue
    if (cont) {  // F0 already holds the next tile's first fragments, its second K-tile is in flight
      vb += gridDim.x;
      if constexpr (RS) {
        // the next tile's row scales, into the set this tile does not read (last read in the previous tile's epilogue:
        // K-tile barriers have passed since; published by the next tile's K-tile barriers)
        if (p.rs_part) rs_base[(rs_sel ^ 1) * 256 + threadIdx.x] = row_rscale(p, nm0 + threadIdx.x);
      }
      m0 = nm0;
      n0 = nn0;
      srcA = nxtA;
      srcW = nxtW;
      locate_k2();
      has_next = vb + (int)gridDim.x < total_tiles;
      locate_next();
      locate_res();
    }
    __builtin_amdgcn_sched_barrier(0);
    const char* res_lds = nullptr;
    if constexpr (RPF) {
      if (from_lds) {
        // Both halves have landed for every wave before the first store of the epilogue (no load is ever queued behind stores),
        // and no LDS-DMA outlives the workgroup.  In place (norm_h16 == res16) a tile's residual region is written by its own
        // workgroup only, and only behind this barrier: every byte of it is in LDS by then.  Out of place the source is only read.
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        // half h is in the buffer of K-tile nt + h: cur / cur ^ 1; this lane's 16 bytes of piece r = 2 j + (ml >> 3)
        res_lds = smem + cur * TILE_BYTES + (((lane >> 3) & 1) * NW + wave) * 1024 + ((lane >> 4) * 8 + (lane & 7)) * 16;
      }
    }
    gemm_epilogue<TM, TN, EPI, true, F16>(p, acc, em0 + wm * TM * 16, en0 + wn * TN * 16, lane,
                                          (RS && p.rs_part) ? rs_base + rs_sel * 256 + wm * TM * 16 : nullptr, res_lds,
                                          (cur ^ 1) * TILE_BYTES - cur * TILE_BYTES);
    if (!cont) {
      if constexpr (DEEP) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no LDS-DMA (the clamped re-fetches) may outlive the workgroup
      break;
    }
    rs_sel ^= 1;
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
      for (int j = 0; j < TM; ++j) {
        acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        asm volatile("" : "+a"(acc[i][j]));  // the zeroing stays in front of ...
      }
    asm volatile("s_nop 7" ::: "memory");    // ... the wait states a VALU write needs before an MFMA reads it as SrcC
  }
}

// the forms of the SiLU*up epilogue the 4-wave kernel is built for (16-byte stores of the 16-bit operand type)
template <bool F16>
static bool silu16_ok(const GemmP& p) {
  return p.out_kind == (F16 ? TCAVT_F16 : TCAVT_BF16) && (p.ldc & 7) == 0;
}

template <int EPI, bool F16, int BN = 256, bool DEEP = false>
static int launch_w4(const GemmP& p0, hipStream_t stream) {
  if constexpr (EPI == EPI_SILU || EPI == EPI_SILU_SAVE) {
    if (!silu16_ok<F16>(p0)) {
      set_error("gemm_bf16(w4): the SiLU epilogue of the 4-wave kernel writes the 16-bit operand type with ldc %% 8 == 0");
      return TCAVT_ERR_ARG;
    }
  }
  if constexpr (EPI == EPI_SILUBWD) {
    if (p0.out_kind != (F16 ? TCAVT_F16 : TCAVT_BF16) || (p0.ldc & 7) || (p0.ldaux & 7) || p0.aux == nullptr || p0.ldc < 2 * p0.N ||
        p0.ldaux < 2 * p0.N) {
      set_error("gemm_bf16(w4): SILU_BWD needs silu_preact, 16-bit output of the operand type, ldc / ld_preact %% 8 == 0 and >= 2 N");
      return TCAVT_ERR_ARG;
    }
  }
  if constexpr (EPI == EPI_ROPE) {
    if (p0.ldc & 7) {
      set_error("gemm_bf16(w4): the RoPE epilogue of the 4-wave kernel needs ldc %% 8 == 0");
      return TCAVT_ERR_ARG;
    }
  }
  if constexpr (EPI == EPI_NORM16) {
    if (p0.ldc & 7) {
      set_error("gemm_bf16(w4): the in-place 16-bit residual epilogue of the 4-wave kernel needs ldc %% 8 == 0");
      return TCAVT_ERR_ARG;
    }
  }
  GemmP p = p0;
  p.tiles_m = p.M / 256;
  p.tiles_n = p.N / BN;
  p.xcd_gx = choose_xcd_partition(p);
  constexpr int lds = 2 * (256 + BN) * 128 + 2048;  // two tile buffers + two sets of 256 row scales (TCAVT_EPI_ROWSCALE)
  auto kfn = gemm_bf16_w4_kernel<EPI, F16, BN, DEEP>;
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kfn),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) {
      set_error("gemm_bf16(w4): hipFuncSetAttribute(%d B LDS) failed: %s", lds, hipGetErrorString(e));
      return TCAVT_ERR_HIP;
    }
    attr_set = true;
  }
  // more tiles than CUs: one persistent workgroup per CU walking its tiles as one K-tile stream (multiple of 8 so that
  // tile ids keep their XCD); TCAVT_GEMM_NO_PERSIST=1 launches one workgroup per tile (A/B)
  const int tiles = p.tiles_m * p.tiles_n;
  static const bool no_pers = getenv("TCAVT_GEMM_NO_PERSIST") != nullptr;
  static const int n_cu = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) n = 256;
    return n / 8 * 8;
  }();
  int wgs = tiles;
  p.pers_tiles = 0;
  // (the two-K-tile look-ahead may reach into the NEXT output tile only: at least two K-tiles per tile)
  if (w4_pers_ok(EPI, DEEP) && !no_pers && n_cu >= 8 && tiles > n_cu && p.K + p.K2 >= 128) {
    p.pers_tiles = tiles;
    wgs = n_cu;
  }
  // residual prefetch of the 16-bit stream epilogue (see the kernel); TCAVT_GEMM_NO_RES_PREFETCH=1: the epilogue loads the
  // residual from global memory itself.  Read at every launch, so that one process can interleave both forms (A/B).
  p.res_pf = 0;
  if constexpr (EPI == EPI_NORM16 && BN == 256) {
    const char* e = getenv("TCAVT_GEMM_NO_RES_PREFETCH");
    p.res_pf = (p.flags & TCAVT_EPI_RESIDUAL) && !(e && e[0] && e[0] != '0');
  }
  dim3 grid(wgs), block(256);
  hipLaunchKernelGGL(kfn, grid, block, lds, stream, p);
  TCAVT_CHECK_LAUNCH("gemm_bf16(w4)");
  return TCAVT_OK;
}

}  // namespace tcavt
