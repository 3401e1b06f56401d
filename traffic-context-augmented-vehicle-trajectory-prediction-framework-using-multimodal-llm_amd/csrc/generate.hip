// Autoregressive text generation on the decoder stack (reference: LlamaMultiModal.generate_batch,
// scripts/train.py:577-654, and scripts/check_generation.py:152-222).
//
// The reference hands HF `generate` a prefix of image tokens + prompt embeddings through a patched embedding layer and
// samples with temperature 0.9, top-k 40, top-p 0.9, repetition penalty 1.2 and no-repeat-3-grams (train.py:628-642).
// Here the prefix is a first-class argument: the PREFILL is the ordinary batched forward (tcavt_llama_stack_forward
// with k_cache / v_cache set), and every following token is ONE call of tcavt_llama_decode_step:
//
//   embed (table[id] + text modality embedding)  ->  16 x [ LoRA down | q|k|v + RoPE at the sample's own position |
//   attention of the one query over the cached keys (which also appends the new k, v) | o_proj | gate|up | down ]  ->
//   final RMSNorm  ->  lm_head (tied embedding table)  ->  logits processors + token selection (tcavt_sample_logits)
//
// All per-step state (positions, current tokens, token history, step counter, finished flags) lives on the device and
// is advanced by the selection kernel, so the launch sequence of a step never changes: it is captured in a hipGraph
// once and replayed per token (BASELINE.json configs[4] "hipGraph-captured decode").
// The projections reuse the MFMA GEMM (M = batch rows: weight-streaming, HBM-bound); RMSNorm is fused exactly as in the
// prefill (csrc/stack.hip).
#include "common.hpp"
#include "philox.hpp"

namespace tcavt {

// One query per (sample, query head) over the cached keys 0 .. pos[b] (the new token's own key included).
// One workgroup per (sample, query head) -- B * nq workgroups, so a batch of 8 already covers the 256 CUs; the heads of a
// GQA group re-read their kv head's rows through L2 -- with KS waves that split the keys in chunks of whole 64-key rounds.
// A round is read COALESCED: lane = (key g = lane / 8 of an 8-key row group, 16-byte column c = lane % 8), so one load
// instruction covers eight whole 128-byte rows and all eight loads of a round are in flight together (the first version gave
// a lane a whole key row -- 64 cache lines per load instruction -- and walked the values one key at a time: 26 us per layer,
// latency bound).  Scores: 8-feature partial dot products, added over the 8 lanes of a key; the KS (max, sum) pairs meet in
// LDS; the probabilities are normalised with the head's global sum and carried in fp16 as in the prefill kernel; output:
// 8 features per lane over the lane's keys, added over the 8 key groups by shuffles and over the KS waves in split order.
// The new token's own key / value (row b of qkv, position pos[b]) are read from qkv and written to the cache by the
// workgroup of the kv head's first query head: no separate append launch, and nothing written here is read back here.
// PFV: the first round of value rows is requested before the softmax statistics meet (its latency passes under the reductions
// and the barrier).  Costs 32 registers, i.e. resident waves: a gain when the grid is one workgroup per CU (B = 8: 1.138 ->
// 1.129 ms per step), a loss when several workgroups per CU hide each other's latencies anyway (B = 32: 1.45 -> 1.56).
template <bool F16, bool PFV>
__global__ __launch_bounds__(1024) void attn_decode_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kc,
                                                           bf16_t* __restrict__ vc, const int* __restrict__ pos,
                                                           bf16_t* __restrict__ out, int lmax, int nq, int nkv, float scale,
                                                           int KS, int out_frag) {
  extern __shared__ float sc[];  // [lmax] scores | [KS][2] (max, sum) | [KS][64] partial outputs
  const int group = nq / nkv;
  const int b = blockIdx.x / nq, head = blockIdx.x % nq, kvh = head / group;
  const int lane = threadIdx.x & 63, ks = threadIdx.x >> 6;
  const int g = lane >> 3, c = lane & 7;
  const int n = min(pos[b] + 1, lmax);
  const int ld = (nq + 2 * nkv) * 64, w = nkv * 64;
  const bf16_t* kb = kc + (long)b * lmax * w + kvh * 64;
  const bf16_t* vb = vc + (long)b * lmax * w + kvh * 64;
  const int jn = n - 1;  // the new token's position
  const bf16_t* knew = qkv + (long)b * ld + (nq + kvh) * 64;
  const bf16_t* vnew = qkv + (long)b * ld + (nq + nkv + kvh) * 64;
  if (head % group == 0 && ks == 0 && lane < 16) {  // append: 8 lanes x 16 bytes of k, 8 of v
    const int cc = (lane & 7) * 8;
    if (lane < 8) *reinterpret_cast<u32x4*>(kc + ((long)b * lmax + jn) * w + kvh * 64 + cc) = *reinterpret_cast<const u32x4*>(knew + cc);
    else *reinterpret_cast<u32x4*>(vc + ((long)b * lmax + jn) * w + kvh * 64 + cc) = *reinterpret_cast<const u32x4*>(vnew + cc);
  }
  float* s = sc;
  float* st = sc + lmax;
  float* po = st + KS * 2;
  const int chunk = ((n + KS - 1) / KS + 63) / 64 * 64;  // keys per split, whole 64-key rounds
  const int j0 = ks * chunk, j1 = min(j0 + chunk, n);
  float q[8];
  {
    const u32x4 t = *reinterpret_cast<const u32x4*>(qkv + (long)b * ld + head * 64 + c * 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      q[2 * e] = from16_lo<F16>(t[e]) * scale;
      q[2 * e + 1] = from16_hi<F16>(t[e]) * scale;
    }
  }
  float mx = -1e30f;
  for (int jb = j0; jb < j1; jb += 64) {
    u32x4 kr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int j = min(jb + i * 8 + g, jn);
      kr[i] = *reinterpret_cast<const u32x4*>((j == jn ? knew : kb + (long)j * w) + c * 8);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        d = fmaf(q[2 * e], from16_lo<F16>(kr[i][e]), d);
        d = fmaf(q[2 * e + 1], from16_hi<F16>(kr[i][e]), d);
      }
      d += __shfl_xor(d, 1, 64);
      d += __shfl_xor(d, 2, 64);
      d += __shfl_xor(d, 4, 64);
      const int j = jb + i * 8 + g;
      if (j < j1) {
        if (c == 0) s[j] = d;
        mx = fmaxf(mx, d);
      }
    }
  }
  u32x4 vr0[PFV ? 8 : 1];
  if constexpr (PFV) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int j = min(j0 + i * 8 + g, jn);
      vr0[i] = *reinterpret_cast<const u32x4*>((j == jn ? vnew : vb + (long)j * w) + c * 8);
    }
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = j0 + lane; j < j1; j += 64) sum += __expf(s[j] - mx);
  sum = wave_sum(sum);
  if (lane == 0) { st[ks * 2] = mx; st[ks * 2 + 1] = sum; }
  __syncthreads();
  float gm = -1e30f, gl = 0.f;
  for (int k = 0; k < KS; ++k) gm = fmaxf(gm, st[k * 2]);
  for (int k = 0; k < KS; ++k) gl += st[k * 2 + 1] * __expf(st[k * 2] - gm);
  const float inv = 1.f / gl;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  for (int jb = j0; jb < j1; jb += 64) {
    u32x4 vr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (PFV && jb == j0) {  // (uniform)
        vr[i] = vr0[PFV ? i : 0];
      } else {
        const int j = min(jb + i * 8 + g, jn);
        vr[i] = *reinterpret_cast<const u32x4*>((j == jn ? vnew : vb + (long)j * w) + c * 8);
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int j = jb + i * 8 + g;
      const float pr = j < j1 ? f16_to_f32(f32_to_f16(__expf(s[j] - gm) * inv)) : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[2 * e] = fmaf(pr, from16_lo<F16>(vr[i][e]), acc[2 * e]);
        acc[2 * e + 1] = fmaf(pr, from16_hi<F16>(vr[i][e]), acc[2 * e + 1]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    acc[e] += __shfl_xor(acc[e], 8, 64);
    acc[e] += __shfl_xor(acc[e], 16, 64);
    acc[e] += __shfl_xor(acc[e], 32, 64);
  }
  if (g == 0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) po[ks * 64 + c * 8 + e] = acc[e];
  }
  __syncthreads();
  if (ks == 0) {
    float o = po[lane];
    for (int k = 1; k < KS; ++k) o += po[k * 64 + lane];
    // (out_frag: the o projection's operand order, common.hpp frag16_off)
    out[out_frag ? frag_off(b, head * 64 + lane, nq * 64, out_frag) : (long)b * nq * 64 + head * 64 + lane] = to16<F16>(o);
  }
}

// ---------------------------------------------------------------------------
// "KV8": the opt-in FP8 KV cache (include/tcavt.h: tcavt_kv_store8 / tcavt_attn_decode8; quant.kv8_quantize is the definition).
// A cached row of one kv head is 64 e4m3fn codes + 2 E8M0 scale bytes (blocks of 32), the planes head-major:
// codes [B][nkv][lmax][64], scales [B][nkv][lmax][2].
// ---------------------------------------------------------------------------
// 2^(byte - 127) of an E8M0 scale byte (byte 0: 2^-127, a subnormal)
__device__ __forceinline__ float e8m0_value(unsigned int byte) { return __uint_as_float(byte ? byte << 23 : 0x00400000u); }

// quantize_mx of eight consecutive 16-bit elements (one 16-byte load) held by a lane; the four lanes l, l ^ 1, l ^ 2, l ^ 3 hold one
// block of 32 and all four are active.  Returns the eight codes; *sb = the block's scale byte.  (The arithmetic of quant_mx8_kernel.)
template <bool F16>
__device__ __forceinline__ u32x2 kv8_quant8(const u32x4& v, unsigned int* sb) {
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
  if (!bad && amax_bits != 0u) k = amax_bits < 0x00800000u ? -127 : max(-127, min(127, e4m3_row_exp(__builtin_bit_cast(float, amax_bits))));
  u32x2 o = {0u, 0u};
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i >> 2] |= e4m3_code(ldexpf(x[i], -k)) << (8 * (i & 3));
  if (bad) o = u32x2{0x7f7f7f7fu, 0x7f7f7f7fu};
  *sb = (unsigned int)(k + 127);
  return o;
}

// Prefill store of one layer: a thread owns 8 consecutive elements of a (row, k | v, kv head), four threads a block of 32, eight a
// cached row (64 codes = 64 consecutive bytes; its two scale bytes leave as one 16-bit store).
template <bool F16>
__global__ __launch_bounds__(256) void kv_store8_kernel(const bf16_t* __restrict__ qkv, unsigned char* __restrict__ kcod,
                                                        unsigned char* __restrict__ ksc, unsigned char* __restrict__ vcod,
                                                        unsigned char* __restrict__ vsc, long pieces, int L, int lmax, int nq, int nkv) {
  const long piece = (long)blockIdx.x * 256 + threadIdx.x;
  if (piece >= pieces) return;  // (pieces % 8 == 0: the eight lanes of a cached row are in or out as a whole)
  const int per_row = 2 * nkv * 8;
  const long row = piece / per_row;  // b * L + l
  const int r = (int)(piece - row * per_row);
  const int is_v = r / (nkv * 8), hd = (r >> 3) % nkv, c8 = r & 7;
  const int b = (int)(row / L), l = (int)(row % L);
  const u32x4 v = *reinterpret_cast<const u32x4*>(qkv + row * ((long)(nq + 2 * nkv) * 64) + nq * 64 + r * 8);
  unsigned int sb;
  const u32x2 o = kv8_quant8<F16>(v, &sb);
  const long at = ((long)b * nkv + hd) * lmax + l;  // the cached row
  *reinterpret_cast<u32x2*>((is_v ? vcod : kcod) + at * 64 + c8 * 8) = o;
  sb |= (unsigned int)__shfl_down((int)sb, 4, 64) << 8;
  if (c8 == 0) *reinterpret_cast<unsigned short*>((is_v ? vsc : ksc) + at * 2) = (unsigned short)sb;
}

// Decode attention on the FP8 cache: attn_decode_kernel's scheme -- one workgroup per (sample, query head), KS waves that split the
// CACHED keys 0 .. pos[b] - 1 in chunks of whole 64-key rounds, scores in LDS, one global (max, sum), probabilities in fp16 relative
// to the final sum, fp32 accumulation -- with its own lane map: a cached row is 64 bytes, so lane = (key g = lane / 4 of a 16-key
// group, 16-byte column c = lane % 4); one load instruction covers sixteen whole rows = 1 KiB of consecutive bytes, the four loads
// of a round are in flight together, and each lane loads the scale byte of its own 16 codes (block c / 2 of the row) with them.
// Dequantisation is v_cvt_scalef32_pk_f32_fp8 with the block's 2^k as the scale operand: code * 2^k in fp32, exact.
// The new token's key / value (row b of qkv, position pos[b]) stay 16-bit: wave 0 scores the new key (a feature per lane), carries
// it in its (max, sum) pair and adds p_new * v_new when the partial outputs meet.  The workgroup of the kv head's first query head
// writes row pos[b] of the four planes, quantised; nothing written here is read back here.
template <bool F16>
__global__ __launch_bounds__(1024) void attn_decode8_kernel(const bf16_t* __restrict__ qkv, unsigned char* __restrict__ kcod,
                                                            unsigned char* __restrict__ ksc, unsigned char* __restrict__ vcod,
                                                            unsigned char* __restrict__ vsc, const int* __restrict__ pos,
                                                            bf16_t* __restrict__ out, int lmax, int nq, int nkv, float scale, int KS,
                                                            int out_frag) {
  extern __shared__ float sc[];  // [lmax] scores | [KS][2] (max, sum) | [KS][64] partial outputs
  const int group = nq / nkv;
  const int b = blockIdx.x / nq, head = blockIdx.x % nq, kvh = head / group;
  const int lane = threadIdx.x & 63, ks = threadIdx.x >> 6;
  const int g = lane >> 2, c = lane & 3;
  const int m = min(max(pos[b], 0), lmax - 1);  // cached keys 0 .. m - 1; the new token's position is m
  const int ld = (nq + 2 * nkv) * 64;
  const long plane = ((long)b * nkv + kvh) * lmax;  // first cached row of (b, kvh)
  const unsigned char* kb = kcod + plane * 64;
  const unsigned char* vb = vcod + plane * 64;
  const unsigned char* ksb = ksc + plane * 2;
  const unsigned char* vsb = vsc + plane * 2;
  const bf16_t* qrow = qkv + (long)b * ld + head * 64;
  const bf16_t* knew = qkv + (long)b * ld + (nq + kvh) * 64;
  const bf16_t* vnew = qkv + (long)b * ld + (nq + nkv + kvh) * 64;
  if (head % group == 0 && ks == 0) {  // append (wave-uniform): lanes 0 .. 7 quantise k, 8 .. 15 v; the others repeat lane 15's work
    const int l16 = min(lane, 15), cc = l16 & 7;
    const u32x4 t = *reinterpret_cast<const u32x4*>((l16 < 8 ? knew : vnew) + cc * 8);
    unsigned int sb;
    const u32x2 o = kv8_quant8<F16>(t, &sb);
    if (lane < 16) {
      *reinterpret_cast<u32x2*>((lane < 8 ? kcod : vcod) + (plane + m) * 64 + cc * 8) = o;
      if ((cc & 3) == 0) ((lane < 8 ? ksc : vsc) + (plane + m) * 2)[cc >> 2] = (unsigned char)sb;
    }
  }
  float* s = sc;
  float* st = sc + lmax;
  float* po = st + KS * 2;
  const int chunk = ((m + KS - 1) / KS + 63) / 64 * 64;  // cached keys per split, whole 64-key rounds
  const int j0 = ks * chunk, j1 = min(j0 + chunk, m);
  float q[16];
  {
    const u32x4 t0 = *reinterpret_cast<const u32x4*>(qrow + c * 16), t1 = *reinterpret_cast<const u32x4*>(qrow + c * 16 + 8);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      q[2 * e] = from16_lo<F16>(t0[e]) * scale;
      q[2 * e + 1] = from16_hi<F16>(t0[e]) * scale;
      q[8 + 2 * e] = from16_lo<F16>(t1[e]) * scale;
      q[9 + 2 * e] = from16_hi<F16>(t1[e]) * scale;
    }
  }
  float mx = -1e30f;
  for (int jb = j0; jb < j1; jb += 64) {
    u32x4 kr[4];
    unsigned int kz[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = min(jb + i * 16 + g, m - 1);  // (j0 < j1 <= m: m >= 1 here)
      kr[i] = *reinterpret_cast<const u32x4*>(kb + (long)j * 64 + c * 16);
      kz[i] = ksb[j * 2 + (c >> 1)];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float z = e8m0_value(kz[i]);
      float d = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const auto lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(kr[i][e], z, false);
        const auto hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(kr[i][e], z, true);
        d = fmaf(q[4 * e], lo[0], d);
        d = fmaf(q[4 * e + 1], lo[1], d);
        d = fmaf(q[4 * e + 2], hi[0], d);
        d = fmaf(q[4 * e + 3], hi[1], d);
      }
      d += __shfl_xor(d, 1, 64);
      d += __shfl_xor(d, 2, 64);
      const int j = jb + i * 16 + g;
      if (j < j1) {
        if (c == 0) s[j] = d;
        mx = fmaxf(mx, d);
      }
    }
  }
  float s_new = 0.f, v_new = 0.f;
  if (ks == 0) {  // the new key, at 16-bit precision from qkv: one feature per lane
    s_new = wave_sum(from16<F16>(qrow[lane]) * scale * from16<F16>(knew[lane]));
    v_new = from16<F16>(vnew[lane]);
    mx = fmaxf(mx, s_new);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = j0 + lane; j < j1; j += 64) sum += __expf(s[j] - mx);
  sum = wave_sum(sum);
  if (ks == 0) sum += __expf(s_new - mx);
  if (lane == 0) { st[ks * 2] = mx; st[ks * 2 + 1] = sum; }
  __syncthreads();
  float gm = -1e30f, gl = 0.f;
  for (int k = 0; k < KS; ++k) gm = fmaxf(gm, st[k * 2]);
  for (int k = 0; k < KS; ++k) gl += st[k * 2 + 1] * __expf(st[k * 2] - gm);
  const float inv = 1.f / gl;
  float acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  for (int jb = j0; jb < j1; jb += 64) {
    u32x4 vr[4];
    unsigned int vz[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = min(jb + i * 16 + g, m - 1);
      vr[i] = *reinterpret_cast<const u32x4*>(vb + (long)j * 64 + c * 16);
      vz[i] = vsb[j * 2 + (c >> 1)];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = jb + i * 16 + g;
      const float pr = j < j1 ? f16_to_f32(f32_to_f16(__expf(s[j] - gm) * inv)) : 0.f;
      const float z = e8m0_value(vz[i]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const auto lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(vr[i][e], z, false);
        const auto hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(vr[i][e], z, true);
        acc[4 * e] = fmaf(pr, lo[0], acc[4 * e]);
        acc[4 * e + 1] = fmaf(pr, lo[1], acc[4 * e + 1]);
        acc[4 * e + 2] = fmaf(pr, hi[0], acc[4 * e + 2]);
        acc[4 * e + 3] = fmaf(pr, hi[1], acc[4 * e + 3]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    acc[e] += __shfl_xor(acc[e], 4, 64);
    acc[e] += __shfl_xor(acc[e], 8, 64);
    acc[e] += __shfl_xor(acc[e], 16, 64);
    acc[e] += __shfl_xor(acc[e], 32, 64);
  }
  if (g == 0) {
#pragma unroll
    for (int e = 0; e < 16; ++e) po[ks * 64 + c * 16 + e] = acc[e];
  }
  __syncthreads();
  if (ks == 0) {
    float o = po[lane];
    for (int k = 1; k < KS; ++k) o += po[k * 64 + lane];
    o = fmaf(f16_to_f32(f32_to_f16(__expf(s_new - gm) * inv)), v_new, o);
    out[out_frag ? frag_off(b, head * 64 + lane, nq * 64, out_frag) : (long)b * nq * 64 + head * 64 + lane] = to16<F16>(o);
  }
}

// out[b] = src[b * L + kv_len[b] - 1]  (the last valid position's hidden state of each sample after the prefill)
__global__ __launch_bounds__(256) void gather_last_kernel(const bf16_t* __restrict__ src, const int* __restrict__ kv_len,
                                                          bf16_t* __restrict__ out, int L, int H) {
  const int b = blockIdx.x;
  const int l = min(max(kv_len[b], 1), L) - 1;
  const bf16_t* s = src + ((long)b * L + l) * H;
  for (int c = threadIdx.x * 8; c < H; c += 256 * 8)
    *reinterpret_cast<u32x4*>(out + (long)b * H + c) = *reinterpret_cast<const u32x4*>(s + c);
}

// tcavt_slot_admit: a freshly prefilled request (a one-sample cache) moves into slot `slot` of an S-slot cache and the slot's
// bookkeeping is reset, in one launch.  Both cache forms are segments of consecutive rows on either side -- 16-bit: a layer of the
// k or v cache, rows of nkv * 128 bytes; KV8: a (layer, kv head) of a plane, rows of 64 code bytes or 2 scale bytes -- so a thread
// copies one 16-byte piece of a segment (or one row's two scale bytes), and one more workgroup behind the copying ones writes the
// slot's state.  Segment g = (layer, i < inner) starts at row g * src_lmax of the source and at row
// ((layer * S + slot) * inner + i) * kv_lmax of the destination.
struct AdmitP {
  const unsigned char* src[4];  // 16-bit: k, v; KV8: k codes, v codes, k scales, v scales
  unsigned char* dst[4];
  long pieces;   // 16-byte pieces of a segment: rows * row_bytes / 16
  long n_wide;   // threads that copy a 16-byte piece: 2 * segs * pieces; behind them (KV8) 2 * segs * rows copy a scale pair
  long n_copy;
  int segs, inner, S, slot, rows, src_lmax, kv_lmax, row_bytes;
  const long* prompt_ids;
  const int* kv_len;
  long* history;
  int *hist_len, *step, *max_new, *pos, *finished;
  long* out_row;
  long out_row_value;
  int n_ids, hist_cap, n_image, max_new_value;
};

__global__ __launch_bounds__(256) void slot_admit_kernel(AdmitP a) {
  if (blockIdx.x == gridDim.x - 1) {  // the slot's state (cur_tok is the sampler's)
    long* h = a.history + (long)a.slot * a.hist_cap;
    for (int i = threadIdx.x; i < a.n_ids; i += 256) h[i] = a.prompt_ids[i];
    if (threadIdx.x == 0) {
      const int kl = *a.kv_len;
      a.hist_len[a.slot] = kl - a.n_image;
      a.pos[a.slot] = kl;
      a.step[a.slot] = 0;
      a.finished[a.slot] = 0;
      a.max_new[a.slot] = a.max_new_value;
      a.out_row[a.slot] = a.out_row_value;
    }
    return;
  }
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_copy) return;
  const bool wide = i < a.n_wide;
  const long j = wide ? i : i - a.n_wide;
  const long per = wide ? a.pieces : (long)a.rows;  // units of a segment
  const long per_plane = a.segs * per;
  const int kv = (int)(j / per_plane);
  const long r = j - kv * per_plane;
  const long g = r / per, e = r - g * per;
  const long srow = g * a.src_lmax, drow = ((g / a.inner * a.S + a.slot) * a.inner + g % a.inner) * a.kv_lmax;
  if (wide) {
    reinterpret_cast<u32x4*>(a.dst[kv] + drow * a.row_bytes)[e] = reinterpret_cast<const u32x4*>(a.src[kv] + srow * a.row_bytes)[e];
  } else {
    reinterpret_cast<unsigned short*>(a.dst[2 + kv] + drow * 2)[e] = reinterpret_cast<const unsigned short*>(a.src[2 + kv] + srow * 2)[e];
  }
}

// tcavt_slot_admit_group: slot_admit_kernel for the G samples of a grouped prefill, blockIdx.y = the group's row.  The source is a
// G-sample cache, so segment (layer, i < inner) of row g starts at source row ((layer * G + g) * inner + i) * src_lmax; the slot, the
// kv_len, the budget and the output row of a row are read from DEVICE arrays (the launch is the same for every group: capturable).
// slot[g] < 0: a pad row, its workgroups leave at once; slot[g] >= S: nothing is written but the flag.  Every index below is
// bounded by the host-checked shape once 0 <= slot < S holds.
struct AdmitGroupP {
  const unsigned char* src[4];
  unsigned char* dst[4];
  long pieces, n_wide, n_copy;  // as AdmitP, per row of the group
  int segs, inner, S, G, rows, src_lmax, kv_lmax, row_bytes;
  const int* slot;
  const int* kv_len;
  const int* max_new_value;
  const long* out_row_value;
  const long* prompt_ids;
  int* bad_slot_flag;
  long* history;
  int *hist_len, *step, *max_new, *pos, *finished;
  long* out_row;
  int n_ids, hist_cap, n_image;
};

__global__ __launch_bounds__(256) void slot_admit_group_kernel(AdmitGroupP a) {
  const int g = blockIdx.y;
  const int slot = a.slot[g];
  if (slot < 0) return;  // pad row
  if (slot >= a.S) {
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *a.bad_slot_flag = 1;
    return;
  }
  if (blockIdx.x == gridDim.x - 1) {  // the slot's state (cur_tok is the sampler's)
    long* h = a.history + (long)slot * a.hist_cap;
    const long* ids = a.prompt_ids + (long)g * a.n_ids;
    for (int i = threadIdx.x; i < a.n_ids; i += 256) h[i] = ids[i];
    if (threadIdx.x == 0) {
      const int kl = a.kv_len[g];
      a.hist_len[slot] = kl - a.n_image;
      a.pos[slot] = kl;
      a.step[slot] = 0;
      a.finished[slot] = 0;
      a.max_new[slot] = a.max_new_value[g];
      a.out_row[slot] = a.out_row_value[g];
    }
    return;
  }
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_copy) return;
  const bool wide = i < a.n_wide;
  const long j = wide ? i : i - a.n_wide;
  const long per = wide ? a.pieces : (long)a.rows;  // units of a segment
  const long per_plane = a.segs * per;
  const int kv = (int)(j / per_plane);
  const long r = j - kv * per_plane;
  const long sg = r / per, e = r - sg * per;
  const long layer = sg / a.inner, in = sg % a.inner;
  const long srow = ((layer * a.G + g) * a.inner + in) * a.src_lmax, drow = ((layer * a.S + slot) * a.inner + in) * a.kv_lmax;
  if (wide) {
    reinterpret_cast<u32x4*>(a.dst[kv] + drow * a.row_bytes)[e] = reinterpret_cast<const u32x4*>(a.src[kv] + srow * a.row_bytes)[e];
  } else {
    reinterpret_cast<unsigned short*>(a.dst[2 + kv] + drow * 2)[e] = reinterpret_cast<const unsigned short*>(a.src[2 + kv] + srow * 2)[e];
  }
}

// tcavt_kv_fanout: a B-sample prefill becomes the state of a decode batch of B * n rows, in one launch.  The cache is cut into the
// segments of slot_admit_group_kernel -- source segment sg = (layer * B + b) * inner + i starts at source row sg * src_lmax -- and
// destination sample b * n + j of a layer is sample (layer * B + b) * n + j of the whole destination, so copy j of the segment
// starts at row (((sg / inner) * n + j) * inner + sg % inner) * kv_lmax.  A thread LOADS one 16-byte piece (or one row's two scale
// bytes, or one 16- or 4-byte piece of a logits row) once and STORES it n times from registers: consecutive lanes hold consecutive
// pieces on both sides, the n stores of a wave are n runs of up to 1 KiB.  Behind the copying workgroups, workgroup b of the last
// B writes the state of rows b * n .. b * n + n - 1 (each prompt id read once, stored n times).
struct FanoutP {
  const unsigned char* src[4];  // 16-bit: k, v; KV8: k codes, v codes, k scales, v scales
  unsigned char* dst[4];
  long pieces;   // 16-byte pieces of a segment: rows * row_bytes / 16
  long n_wide;   // threads that copy a 16-byte piece: 2 * segs * pieces; behind them (KV8) 2 * segs * rows copy a scale pair,
  long n_cache;  // and behind those B * log_per copy a piece of a logits row
  long n_copy;
  long log_per;  // pieces of a logits row: V / 4 of 16 bytes (log_wide), or V of 4 bytes
  int segs, inner, B, n, rows, src_lmax, kv_lmax, row_bytes, log_wide, V;
  const float* logits_src;
  float* logits_dst;
  const long* prompt_ids;
  const int* kv_len;
  long* history;
  int *hist_len, *pos, *finished;
  int n_ids, hist_cap, n_image;
};

// The state of prompt b's n rows, by one workgroup (cur_tok and step are the sampler's) ...
__device__ __forceinline__ void fanout_state(const FanoutP& a, int b) {
  const int n = a.n;
  const long* ids = a.prompt_ids + (long)b * a.n_ids;
  long* h = a.history + (long)b * n * a.hist_cap;
  for (int i = threadIdx.x; i < a.n_ids; i += 256) {
    const long id = ids[i];
    for (int j = 0; j < n; ++j) h[(long)j * a.hist_cap + i] = id;
  }
  const int kl = a.kv_len[b];
  for (int j = threadIdx.x; j < n; j += 256) {
    const long r = (long)b * n + j;
    a.hist_len[r] = kl - a.n_image;
    a.pos[r] = kl;
    a.finished[r] = 0;
  }
}

// ... and the first logits, one thread per piece: piece e of source row b -> rows b * n .. b * n + n - 1
__device__ __forceinline__ void fanout_logits(const FanoutP& a, long r) {
  const int n = a.n;
  const long b = r / a.log_per, e = r - b * a.log_per;
  const float* s = a.logits_src + b * a.V;
  float* d = a.logits_dst + b * n * a.V;
  if (a.log_wide) {
    const u32x4 v = reinterpret_cast<const u32x4*>(s)[e];
    for (int j = 0; j < n; ++j) reinterpret_cast<u32x4*>(d + (long)j * a.V)[e] = v;
  } else {
    const unsigned int v = reinterpret_cast<const unsigned int*>(s)[e];
    for (int j = 0; j < n; ++j) reinterpret_cast<unsigned int*>(d + (long)j * a.V)[e] = v;
  }
}

__global__ __launch_bounds__(256) void kv_fanout_kernel(FanoutP a) {
  const int n = a.n;
  const long first_state = (long)gridDim.x - a.B;
  if (blockIdx.x >= first_state) {
    fanout_state(a, (int)(blockIdx.x - first_state));
    return;
  }
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_copy) return;
  if (i >= a.n_cache) {
    fanout_logits(a, i - a.n_cache);
    return;
  }
  const bool wide = i < a.n_wide;
  const long t = wide ? i : i - a.n_wide;
  const long per = wide ? a.pieces : (long)a.rows;  // units of a segment
  const long per_plane = a.segs * per;
  const int kv = (int)(t / per_plane);
  const long r = t - kv * per_plane;
  const long sg = r / per, e = r - sg * per;
  const long sample = sg / a.inner, in = sg - sample * a.inner;  // sample = layer * B + b
  const long srow = sg * a.src_lmax;
  const long drow = (sample * n * a.inner + in) * a.kv_lmax;  // copy 0; copy j lies j * dstep rows on
  const long dstep = (long)a.inner * a.kv_lmax;
  if (wide) {
    const u32x4 v = reinterpret_cast<const u32x4*>(a.src[kv] + srow * a.row_bytes)[e];
    u32x4* d = reinterpret_cast<u32x4*>(a.dst[kv] + drow * a.row_bytes) + e;
    const long step = dstep * a.row_bytes / 16;
    for (int j = 0; j < n; ++j) d[j * step] = v;
  } else {
    const unsigned short v = reinterpret_cast<const unsigned short*>(a.src[2 + kv] + srow * 2)[e];
    unsigned short* d = reinterpret_cast<unsigned short*>(a.dst[2 + kv] + drow * 2) + e;
    for (int j = 0; j < n; ++j) d[j * dstep] = v;
  }
}

// tcavt_state_fanout: kv_fanout_kernel without a cache to copy (n_cache = 0) -- the logits pieces, and behind them the B state workgroups.
__global__ __launch_bounds__(256) void state_fanout_kernel(FanoutP a) {
  const long first_state = (long)gridDim.x - a.B;
  if (blockIdx.x >= first_state) {
    fanout_state(a, (int)(blockIdx.x - first_state));
    return;
  }
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < a.n_copy) fanout_logits(a, i);
}

// ---------------------------------------------------------------------------
// Logits processors + token selection, one workgroup per sample (HF generation: RepetitionPenaltyLogitsProcessor,
// NoRepeatNGramLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper, in that order; the warpers
// only when sampling).  `logits` is modified in place (penalty / bans).  The candidates that survive top-k are gathered
// in descending (value, then ascending index) order by k rounds of a block-wide arg-max "next after the previous one" --
// exact ties at the k-th value are all kept, as `scores < topk[-1]` keeps them.
// ---------------------------------------------------------------------------
struct SampleP {
  float temperature, top_p, rep_penalty;
  int top_k, no_repeat_ngram, do_sample;
  long eos, pad;
  unsigned int seed_lo, seed_hi;
};

// Ending rules of a request (tcavt_stop_rules; sample kernels with STOP): a stop set as a bitmap over the vocabulary, up to
// SMP_SEQS stop sequences of 1 .. SMP_SEQ_LEN ids, the ban of every ending token while step < min_new
// (MinNewTokensLengthLogitsProcessor with eos_token_id given as a list), and the record of how and when a request ended.
struct StopP {
  const unsigned int* bitmap;  // [(V + 31) / 32], bit id & 31 of word id >> 5; or NULL
  const long* seqs;            // [n_seqs][SMP_SEQ_LEN]
  const int* seq_len;          // [n_seqs]; a length outside [1, SMP_SEQ_LEN] never matches
  int* finish_reason;          // indexed like out_tokens' rows; or NULL
  int* n_generated;            // likewise
  int n_seqs, min_new;
};
constexpr int SMP_SEQS = 16, SMP_SEQ_LEN = 8;
constexpr int FIN_EOS = 1, FIN_STOP_TOKEN = 2, FIN_STOP_SEQ = 3, FIN_BUDGET = 4;

constexpr int SMP_T = 1024;   // threads
constexpr int SMP_CAP = 256;  // candidate list capacity (top_k + ties)
constexpr int SMP_BINS = 2048;  // histogram of (max - score) * 64: covers 32 units below the maximum
constexpr int SMP_LIST = 1024;  // pre-selected scores (everything down to the threshold bin)
static_assert(SMP_LIST <= SMP_T && (SMP_BINS / 64 & (SMP_BINS / 64 - 1)) == 0, "one thread per list entry; bins per lane a power of two");

__device__ __forceinline__ bool after(float v, int i, float pv, int pi) {  // (v, i) comes after (pv, pi) in (value desc, index asc) order
  return v < pv || (v == pv && i > pi);
}
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) {  // (v, i) precedes (bv, bi)
  return v > bv || (v == bv && i < bi);
}

// ---------------------------------------------------------------------------
// Two-stage form (round 4; tcavt_sample_logits with a workspace): one workgroup per sample walks 128 256 logits in three
// dependent passes -- 64 us on 8 of 256 CUs at B = 8, latency bound.  Stage 1 cuts every sample's vocabulary into SMP_G
// contiguous slices, one workgroup each (B x 16 workgroups): the slice's processors (a token's penalty / ban is applied by the
// workgroup that owns the token), then the slice's <= 8 scores per thread live in REGISTERS and the three passes (max / min,
// histogram, collection) cost no further memory traffic; out come the slice's candidates -- everything at or above the slice's
// own top-k threshold bin -- and the smallest of them, lb: at least k scores of the slice are >= lb, so the sample's k-th
// largest score is >= lb too.  Stage 2 (sample_kernel with `pre`) keeps the candidates >= max over the slices of lb (a superset
// of the global top-k and of every tie with the k-th value), and ranks / keeps / draws exactly as the one-stage form does:
// the selected token is the same.  A slice whose threshold bin overflows its list (e.g. constant logits) raises ovf[b] and the
// sample falls back to the three passes of the one-stage form (its processors are done).
// ---------------------------------------------------------------------------
// Does token t occur among the first n entries of an LDS-resident history?  Four entries per LDS read and NO early exit: written
// as "scan until found", thread i's loop is a chain of up to i dependent LDS round trips (one ~100-cycle latency per entry:
// 15 us for a 300-token history -- a quarter of the whole selection kernel); without the data-dependent exit the reads pipeline.
__device__ __forceinline__ bool occurs_before(const int* __restrict__ lds_tok, int n, int t) {
  typedef __attribute__((ext_vector_type(4))) int i32x4;
  bool dup = false;
  int j = 0;
#pragma unroll 4
  for (; j + 4 <= n; j += 4) {
    const i32x4 q = *reinterpret_cast<const i32x4*>(lds_tok + j);
    dup |= (q[0] == t) | (q[1] == t) | (q[2] == t) | (q[3] == t);
  }
  for (; j < n; ++j) dup |= lds_tok[j] == t;
  return dup;
}

constexpr int SMP_G = 16;      // slices (stage-1 workgroups) per sample
constexpr int SMP_LCAP = 512;  // candidates per slice
constexpr int SMP_E4 = 4;      // f32x4 registers per thread: slices of up to 4 * 1024 * 4 scores (V <= 262 144)

struct SliceWs {  // views into the caller's workspace (tcavt_sample_logits: layout and size)
  int* ticket;    // [1]   stage 2: workgroups that have read *step (the last one increments it); zero between calls
  int* ovf;       // [B]   a slice of the sample overflowed its list; zero between calls
  int* cand_n;    // [B][G]
  float* lb;      // [B][G]
  float* cand_v;  // [B][G][SMP_LCAP]
  int* cand_i;    // [B][G][SMP_LCAP]
};

// STOP: the ban of the ending tokens before the minimum (StopP) -- the workgroup that owns a token bans it, as with the other
// processors: the four ids of a lane's f32x4 lie in one word of the bitmap, so one load serves all four, and the banned scores go
// back to the row (the one-stage fallback of stage 2 reads them there).  The branch is uniform per row and nothing is loaded for
// the ban once the minimum is reached.  step_p: the row's step word (per_slot: step_p[sb], else *step_p).
template <bool STOP = false>
__global__ __launch_bounds__(SMP_T) void sample_slice_kernel(float* __restrict__ logits, int V, const long* __restrict__ history,
                                                             int hist_cap, const int* __restrict__ hist_len, SampleP sp, SliceWs ws,
                                                             const int* __restrict__ slot_of_row, int S, StopP sr,
                                                             const int* __restrict__ step_p, int per_slot,
                                                             const int* __restrict__ finished) {
  __shared__ int hist_bins[SMP_BINS];
  __shared__ float lv[SMP_LCAP];
  __shared__ __attribute__((aligned(16))) int li[SMP_LCAP];
  __shared__ float rv[SMP_T / 64], rm[SMP_T / 64];
  __shared__ int ri[SMP_T / 64];
  __shared__ float s_max, s_min;
  __shared__ int s_bi, list_n, thr_bin;
  const int b = blockIdx.x / SMP_G, g = blockIdx.x % SMP_G, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // (slot_of_row: logits row b belongs to slot sb of the state arrays; a row without a slot is skipped, nothing of it is written)
  const int sb = slot_of_row ? slot_of_row[b] : b;
  if (sb < 0 || sb >= S) return;  // (uniform)
  float* x = logits + (long)b * V;
  const long* hist = history + (long)sb * hist_cap;
  const int hl = min(hist_len[sb], hist_cap);
  const int V4 = V >> 2, chunk4 = (V4 + SMP_G - 1) / SMP_G;
  const int lo4 = g * chunk4, hi4 = min(lo4 + chunk4, V4);
  const long lo = 4L * lo4, hi = 4L * hi4;
  // ---- processors, for the tokens this slice owns (same arithmetic and order as the one-stage form: penalty, then ban)
  // (the history goes to LDS once when it fits, and both processors read it there: every global access the processors make is
  //  one more dependent round trip at the head of a kernel that is a handful of them long)
  const bool in_lds = hl <= SMP_LCAP;
  const int ng = sp.no_repeat_ngram;
  const bool do_rep = sp.rep_penalty != 1.f, do_ban = ng > 0 && hl + 1 >= ng;
  if (in_lds && (do_rep || do_ban)) {
    for (int i = tid; i < hl; i += SMP_T) li[i] = (int)min(max(hist[i], -1L), 0x7fffffffL);  // (ids >= 2^31 - 1 are out of range anyway)
    __syncthreads();
  }
  auto tok_at = [&](int i) -> long { return in_lds ? (long)li[i] : hist[i]; };
  if (do_rep) {
    for (int i = tid; i < hl; i += SMP_T) {
      const long t = tok_at(i);
      bool first = t >= lo && t < hi;
      if (in_lds) {
        first = first && !occurs_before(li, i, (int)t);
      } else {
        for (int j = 0; j < i && first; ++j) first = hist[j] != t;
      }
      if (first) {
        const float s_ = x[t];
        x[t] = s_ < 0.f ? s_ * sp.rep_penalty : s_ / sp.rep_penalty;
      }
    }
    __syncthreads();
  }
  if (do_ban) {
    for (int i = tid; i + ng - 1 < hl; i += SMP_T) {
      bool match = true;
      for (int k = 0; k < ng - 1 && match; ++k) {
        const int p = i + k, q = hl - (ng - 1) + k;
        const long a = tok_at(p);
        match = a == tok_at(q);
        // (the LDS copy folds every id below 0 onto -1 and every id from 2^31 - 1 up onto 2^31 - 1: two of those are equal only
        //  if the ids themselves are, as in the one-stage form)
        if (match && in_lds && (a == -1L || a == 0x7fffffffL)) match = hist[p] == hist[q];
      }
      const long t = tok_at(i + ng - 1);
      if (match && t >= lo && t < hi) x[t] = -INFINITY;
    }
    __syncthreads();
  }
  // ---- the slice, in registers (scaled by 1 / temperature when sampling: the order of the scores is what counts)
  const float sc = sp.do_sample ? 1.f / sp.temperature : 1.f;
  f32x4 v4[SMP_E4];
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
  bool min_ban = false;  // (uniform)
  if constexpr (STOP) {
    if (sr.min_new > 0) min_ban = (per_slot ? step_p[sb] : *step_p) < sr.min_new && finished[sb] == 0;
  }
#pragma unroll
  for (int e = 0; e < SMP_E4; ++e) {
    const int i4 = lo4 + tid + e * SMP_T;
    f32x4 t = i4 < hi4 ? x4[i4] : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};  // (a padding -inf never precedes a real entry: its index is larger)
    if constexpr (STOP) {
      if (min_ban && i4 < hi4) {
        unsigned int m = sr.bitmap ? (sr.bitmap[i4 >> 3] >> ((i4 & 7) * 4)) & 15u : 0u;
        if (sp.eos >= 0 && (sp.eos >> 2) == (long)i4) m |= 1u << (int)(sp.eos & 3);
        if (m) {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if ((m >> c) & 1u) t[c] = -INFINITY;
          reinterpret_cast<f32x4*>(x)[i4] = t;
        }
      }
    }
    v4[e] = t * sc;
  }
  // best (value desc, index asc) and smallest finite score of the slice
  float bv = -INFINITY, lmin = INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int e = 0; e < SMP_E4; ++e) {
    const int i4 = lo4 + tid + e * SMP_T;
    if (i4 < hi4) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float v = v4[e][c];
        const int i = 4 * i4 + c;
        if (better(v, i, bv, bi)) { bv = v; bi = i; }
        if (v > -INFINITY) lmin = fminf(lmin, v);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  lmin = -wave_max(-lmin);
  if (lane == 0) { rv[wv] = bv; ri[wv] = bi; rm[wv] = lmin; }
  __syncthreads();
  if (tid == 0) {
    float v = rv[0], m_ = rm[0];
    int i = ri[0];
    for (int k = 1; k < SMP_T / 64; ++k) {
      if (better(rv[k], ri[k], v, i)) { v = rv[k]; i = ri[k]; }
      m_ = fminf(m_, rm[k]);
    }
    s_max = v; s_bi = i; s_min = m_;
    list_n = 0;
  }
  for (int i = tid; i < SMP_BINS; i += SMP_T) hist_bins[i] = 0;
  __syncthreads();
  const long slot0 = ((long)b * SMP_G + g) * SMP_LCAP;
  if (!sp.do_sample) {  // greedy: the slice's first maximum
    if (tid == 0) {
      ws.cand_v[slot0] = s_max;
      ws.cand_i[slot0] = s_bi;
      ws.cand_n[b * SMP_G + g] = 1;
      ws.lb[b * SMP_G + g] = -INFINITY;
    }
    return;
  }
  const float gmax = s_max;
  if (!(gmax > -INFINITY)) {  // (uniform) nothing finite in this slice
    if (tid == 0) { ws.cand_n[b * SMP_G + g] = 0; ws.lb[b * SMP_G + g] = -INFINITY; }
    return;
  }
  const float bscale = (float)(SMP_BINS - 1) / fmaxf(gmax - s_min, 1e-20f);
  const int k = min(max(sp.top_k, 1), SMP_CAP);
#pragma unroll
  for (int e = 0; e < SMP_E4; ++e) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float d = (gmax - v4[e][c]) * bscale;
      if (d < (float)SMP_BINS) atomicAdd(&hist_bins[(int)d], 1);  // (-inf: d = +inf, skipped)
    }
  }
  __syncthreads();
  if (wv == 0) {  // first bin at which the running count reaches k (as in the one-stage form)
    constexpr int PER = SMP_BINS / 64;
    int loc = 0;
#pragma unroll 8
    for (int t_ = 0; t_ < PER; ++t_) loc += hist_bins[lane * PER + ((t_ + lane) & (PER - 1))];
    int pre = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(pre, o, 64);
      if (lane >= o) pre += up;
    }
    const bool hit = pre >= k && pre - loc < k;
    if (__builtin_amdgcn_ballot_w64(hit) == 0ull) {
      if (lane == 0) thr_bin = -1;  // fewer than k finite scores in the slice: all of them are candidates, no bound
    } else if (hit) {
      int cum = pre - loc, tb = lane * PER;
      for (int t_ = 0; t_ < PER; ++t_) {
        cum += hist_bins[lane * PER + t_];
        if (cum >= k) { tb = lane * PER + t_; break; }
      }
      thr_bin = cum <= SMP_LCAP ? tb : -2;  // -2: the threshold bin overflows the slice's list
    }
  }
  __syncthreads();
  const int tb = thr_bin;
  if (tb == -2) {  // (uniform)
    if (tid == 0) { atomicOr(&ws.ovf[b], 1); ws.cand_n[b * SMP_G + g] = 0; ws.lb[b * SMP_G + g] = -INFINITY; }
    return;
  }
  const float lim = tb < 0 ? (float)SMP_BINS : (float)(tb + 1);
  float mymin = INFINITY;
#pragma unroll
  for (int e = 0; e < SMP_E4; ++e) {
    const int i4 = lo4 + tid + e * SMP_T;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float v = v4[e][c];
      if ((gmax - v) * bscale < lim) {
        const int slot = atomicAdd(&list_n, 1);
        if (slot < SMP_LCAP) { lv[slot] = v; li[slot] = 4 * i4 + c; }
        mymin = fminf(mymin, v);
      }
    }
  }
  mymin = -wave_max(-mymin);
  if (lane == 0) rm[wv] = mymin;
  __syncthreads();
  const int n = min(list_n, SMP_LCAP);  // (tb >= 0: list_n = the running count at the threshold bin <= SMP_LCAP; tb < 0: < k <= SMP_CAP)
  for (int t_ = tid; t_ < n; t_ += SMP_T) {
    ws.cand_v[slot0 + t_] = lv[t_];
    ws.cand_i[slot0 + t_] = li[t_];
  }
  if (tid == 0) {
    float m_ = rm[0];
    for (int w_ = 1; w_ < SMP_T / 64; ++w_) m_ = fminf(m_, rm[w_]);
    ws.cand_n[b * SMP_G + g] = n;
    ws.lb[b * SMP_G + g] = tb >= 0 ? m_ : -INFINITY;  // (>= k scores of the slice are >= the smallest collected one)
  }
}

// `pre` (ws.cand_v != nullptr): stage 2 of the two-stage form -- the processors are done and the candidates come from the slices
// SLOTS (tcavt_sample_logits_slots): the bookkeeping is per slot -- step_p, max_new and out_row are arrays [B]; slot b chooses token
// step_p[b] of output row out_row[b] (which is also its Philox row), ends on EOS or when its budget max_new[b] is used up, and a
// finished slot is inert: cur_tok[b] = pad and nothing else of its state is written.  The selection itself is the same code.
// ROWS (tcavt_sample_logits_rows): SLOTS, with the logits row and the workspace indexed by the workgroup b and the state by the slot
// sb = slot_of_row[b] of n_state slots; a row without a slot leaves before it has written anything.
// STOP (tcavt_sample_tokens with rules): a live row -- finished == 0 -- also bans the ending tokens while step < min_new (here only
// in the one-stage form; the slices have done it otherwise), ends on a token of the stop set (the token is kept) or when its last n
// generated tokens equal a stop sequence of length n (never reaching into the prompt: step + 1 >= n), and the thread that sets
// `finished` records finish_reason (EOS 1 > stop token 2 > stop sequence 3 > budget 4) and n_generated = step + 1 at the row's
// out_tokens index.  Everything else of a row's step is as without STOP.
constexpr int SMP_BATCH = 0, SMP_SLOTS = 1, SMP_ROWS = 2;
template <int MODE, bool STOP = false>
__global__ __launch_bounds__(SMP_T) void sample_kernel(float* __restrict__ logits, int V, long* __restrict__ history,
                                                       int hist_cap, int* __restrict__ hist_len, SampleP sp,
                                                       int* __restrict__ step_p, long* __restrict__ cur_tok,
                                                       int* __restrict__ pos, int* __restrict__ finished,
                                                       long* __restrict__ out_tokens, int out_cap, int advance_pos, SliceWs ws,
                                                       int n_samples, const int* __restrict__ max_new,
                                                       const long* __restrict__ out_row, const int* __restrict__ slot_of_row,
                                                       int n_state, StopP sr) {
  constexpr bool SLOTS = MODE != SMP_BATCH;
  __shared__ float cv[SMP_CAP];
  __shared__ int ci[SMP_CAP];
  __shared__ float rv[SMP_T / 64];
  __shared__ int ri[SMP_T / 64];
  __shared__ float rm[SMP_T / 64];
  __shared__ float bestv;
  __shared__ int besti;
  __shared__ int hist_bins[SMP_BINS];
  __shared__ float list_v[SMP_LIST];
  __shared__ __attribute__((aligned(16))) int list_i[SMP_LIST];
  __shared__ int list_n, thr_bin, keep_n;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int sb = b;  // the row's entry of the state arrays
  if constexpr (MODE == SMP_ROWS) {
    sb = slot_of_row[b];
    if (sb < 0 || sb >= n_state) return;  // (uniform)
  }
  float* x = logits + (long)b * V;
  long* hist = history + (long)sb * hist_cap;
  const int hl = min(hist_len[sb], hist_cap);
  const int step = SLOTS ? step_p[sb] : *step_p;
  const bool pre = ws.cand_v != nullptr;
  __shared__ int s_ovf;
  if (pre) {
    if (tid == 0) s_ovf = ws.ovf[b];
    __syncthreads();
    if (tid == 0 && s_ovf) ws.ovf[b] = 0;  // (re-armed for the next call)
  }
  const bool pre_ok = pre && s_ovf == 0;  // (uniform) the slices' candidates are complete
  // ---- before the minimum: no ending token (-inf absorbs the penalty, so the order against the processors below does not matter)
  if constexpr (STOP) {
    if (!pre && sr.min_new > 0 && step < sr.min_new && finished[sb] == 0) {  // (uniform)
      if (sr.bitmap) {
        for (int i = tid; i < V; i += SMP_T)
          if ((sr.bitmap[i >> 5] >> (i & 31)) & 1u) x[i] = -INFINITY;
      }
      if (tid == 0 && sp.eos >= 0 && sp.eos < V) x[sp.eos] = -INFINITY;
      __syncthreads();
    }
  }
  // ---- repetition penalty: once per distinct token of the history (scatter semantics of the reference processor)
  if (!pre && sp.rep_penalty != 1.f) {
    // (the history is staged in LDS when it fits: thread i compares its token with all earlier ones)
    const bool in_lds = hl <= SMP_LIST;
    if (in_lds) {
      for (int i = tid; i < hl; i += SMP_T) list_i[i] = (int)min(max(hist[i], -1L), 0x7fffffffL);  // (ids >= 2^31 - 1 are out of range anyway)
      __syncthreads();
    }
    for (int i = tid; i < hl; i += SMP_T) {
      const long t = hist[i];
      bool first = t >= 0 && t < V;
      if (in_lds) {
        first = first && !occurs_before(list_i, i, (int)t);
      } else {
        for (int j = 0; j < i && first; ++j) first = hist[j] != t;
      }
      if (first) {
        const float s = x[t];
        x[t] = s < 0.f ? s * sp.rep_penalty : s / sp.rep_penalty;
      }
    }
    __syncthreads();
  }
  // ---- no-repeat n-gram: ban every token that would complete an n-gram already in the history
  const int ng = sp.no_repeat_ngram;
  if (!pre && ng > 0 && hl + 1 >= ng) {
    for (int i = tid; i + ng - 1 < hl; i += SMP_T) {
      bool match = true;
      for (int k = 0; k < ng - 1 && match; ++k) match = hist[i + k] == hist[hl - (ng - 1) + k];
      const long t = hist[i + ng - 1];
      if (match && t >= 0 && t < V) x[t] = -INFINITY;
    }
    __syncthreads();
  }
  // every logit of the sample, 16 bytes per lane and load when the row allows (V % 4 == 0, aligned) and several loads in flight:
  // the passes below are latency bound (one workgroup per sample), so fewer and wider loads are what shortens them
  auto walk = [&](auto&& f) {
    if ((V & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
      const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
      const int V4 = V >> 2;
#pragma unroll 4
      for (int i4 = tid; i4 < V4; i4 += SMP_T) {
        const f32x4 t = x4[i4];
        f(t[0], 4 * i4);
        f(t[1], 4 * i4 + 1);
        f(t[2], 4 * i4 + 2);
        f(t[3], 4 * i4 + 3);
      }
    } else {
#pragma unroll 4
      for (int i = tid; i < V; i += SMP_T) f(x[i], i);
    }
  };
  // block-wide arg-max of the elements that come after (pv, pi) in (value desc, index asc) order; with_min: also the
  // smallest finite value (left in rv[0] region -> minv) in the same pass
  __shared__ float minv;
  auto next_best = [&](float pv, int pi, float scale, bool with_min) {
    float bv = -INFINITY, lmin = INFINITY;
    int bi = 0x7fffffff;
    walk([&](float raw, int i) {
      const float v = raw * scale;
      if (after(v, i, pv, pi) && better(v, i, bv, bi)) { bv = v; bi = i; }
      if (with_min && v > -INFINITY) lmin = fminf(lmin, v);
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (with_min) lmin = -wave_max(-lmin);
    if (lane == 0) { rv[wv] = bv; ri[wv] = bi; rm[wv] = lmin; }
    __syncthreads();
    if (tid == 0) {
      float v = rv[0], m_ = rm[0];
      int i = ri[0];
      for (int k = 1; k < SMP_T / 64; ++k) {
        if (better(rv[k], ri[k], v, i)) { v = rv[k]; i = ri[k]; }
        m_ = fminf(m_, rm[k]);
      }
      bestv = v;
      besti = i;
      minv = m_;
    }
    __syncthreads();
  };
  long tok;
  if (!sp.do_sample && pre_ok) {  // greedy, two-stage form: the best of the slices' first maxima
    if (tid < 64) {
      float bv = -INFINITY;
      int bi = 0x7fffffff;
      if (tid < SMP_G && ws.cand_n[b * SMP_G + tid] > 0) {
        bv = ws.cand_v[((long)b * SMP_G + tid) * SMP_LCAP];
        bi = ws.cand_i[((long)b * SMP_G + tid) * SMP_LCAP];
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
      }
      if (tid == 0) besti = bi;
    }
    __syncthreads();
    tok = besti;
  } else if (!sp.do_sample) {  // greedy: arg-max of the processed scores, first maximum wins (torch.argmax)
    next_best(INFINITY, -1, 1.f, false);
    tok = besti;
  } else {
    // Candidate collection in three passes over the vocabulary instead of one pass per candidate: (1) the maximum and the
    // minimum (one pass), (2) a histogram of (max - score) in SMP_BINS bins over that range (integer counts: order-independent), from which the narrowest
    // threshold that keeps at least top_k scores follows, (3) everything at or above that threshold goes to an LDS list
    // (top_k + the rest of the threshold bin; insertion order does not matter, the selection below orders by
    // (value, index)).  The list is then ordered by top_k rounds of a wave-level arg-max over <= SMP_LIST entries.
    const float invT = 1.f / sp.temperature;
    const int k = min(max(sp.top_k, 1), SMP_CAP);
    bool have_list = false;  // (uniform)
    if (pre_ok) {
      // two-stage form: every slice's candidates at or above the largest of the slices' bounds (>= k scores of ONE slice lie at
      // or above its bound, so the sample's k-th largest score does too: nothing below it can be kept)
      if (tid == 0) { list_n = 0; keep_n = 0; }
      // (one slice per WAVE -- SMP_G == SMP_T / 64 -- and every load of a phase in flight together: written as a loop over the
      //  slices this was 2 x 16 dependent round trips to memory that another CU has just written, 40 us for a ~10 us kernel)
      static_assert(SMP_G == SMP_T / 64, "one wave per slice");
      float lmax = ws.lb[b * SMP_G + (lane & (SMP_G - 1))];
#pragma unroll
      for (int o = 1; o < SMP_G; o <<= 1) lmax = fmaxf(lmax, __shfl_xor(lmax, o, 64));
      const int n_g = ws.cand_n[b * SMP_G + wv];
      const long s0 = ((long)b * SMP_G + wv) * SMP_LCAP;
      float cvv[SMP_LCAP / 64];
      int cii[SMP_LCAP / 64];
#pragma unroll
      for (int e = 0; e < SMP_LCAP / 64; ++e) {
        const int t_ = lane + 64 * e;
        cvv[e] = t_ < n_g ? ws.cand_v[s0 + t_] : -INFINITY;
        cii[e] = t_ < n_g ? ws.cand_i[s0 + t_] : 0;
      }
      __syncthreads();
#pragma unroll
      for (int e = 0; e < SMP_LCAP / 64; ++e) {
        if (lane + 64 * e < n_g && cvv[e] >= lmax) {
          const int slot = atomicAdd(&list_n, 1);
          if (slot < SMP_LIST) { list_v[slot] = cvv[e]; list_i[slot] = cii[e]; }
        }
      }
      __syncthreads();
      have_list = list_n <= SMP_LIST;  // (more: the three passes below, over the already processed logits)
      if (tid == 0 && have_list) thr_bin = 0;
      __syncthreads();
    }
    float gmax = 0.f, bscale = 0.f;
    if (!have_list) {
    next_best(INFINITY, -1, invT, true);  // (1): the maximum and, in the same pass, the smallest finite score
    gmax = bestv;
    // bin width from the spread of the finite scores: SMP_BINS bins between the maximum and the minimum
    bscale = (float)(SMP_BINS - 1) / fmaxf(gmax - minv, 1e-20f);
    __syncthreads();
    for (int i = tid; i < SMP_BINS; i += SMP_T) hist_bins[i] = 0;
    if (tid == 0) { list_n = 0; keep_n = 0; }
    __syncthreads();
    walk([&](float raw, int) {
      const float d = (gmax - raw * invT) * bscale;
      if (d < (float)SMP_BINS) atomicAdd(&hist_bins[(int)d], 1);  // (-inf scores: d = +inf, skipped)
    });
    __syncthreads();
    if (wv == 0) {
      // first bin at which the running count reaches k: every lane adds up its SMP_BINS / 64 consecutive bins, a wave scan
      // finds the lane in whose range the count crosses k, and only that lane walks its bins (one thread walking all 2048
      // bins was a chain of up to 2048 dependent LDS reads)
      constexpr int PER = SMP_BINS / 64;
      int loc = 0;
#pragma unroll 8
      for (int t_ = 0; t_ < PER; ++t_) loc += hist_bins[lane * PER + ((t_ + lane) & (PER - 1))];  // (rotated: 2-way instead of 64-way bank conflicts)
      int pre = loc;  // inclusive prefix over the lanes
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(pre, o, 64);
        if (lane >= o) pre += up;
      }
      const bool hit = pre >= k && pre - loc < k;
      if (__builtin_amdgcn_ballot_w64(hit) == 0ull) {
        if (lane == 0) thr_bin = -1;  // fewer than k scores in range -> exact fallback
      } else if (hit) {
        int cum = pre - loc, tb = lane * PER;
        for (int t_ = 0; t_ < PER; ++t_) {
          cum += hist_bins[lane * PER + t_];
          if (cum >= k) { tb = lane * PER + t_; break; }
        }
        thr_bin = cum <= SMP_LIST ? tb : -1;  // -1: too many scores in the threshold bin -> exact fallback
      }
    }
    __syncthreads();
    }  // (!have_list)
    int n = 0;
    if (thr_bin >= 0) {
      if (!have_list) {
        const float lim = (float)(thr_bin + 1);
        walk([&](float raw, int i) {
          const float v = raw * invT;
          if ((gmax - v) * bscale < lim) {
            const int slot = atomicAdd(&list_n, 1);
            if (slot < SMP_LIST) { list_v[slot] = v; list_i[slot] = i; }
          }
        });
        __syncthreads();
      }
      const int ln = min(list_n, SMP_LIST);
      // order the list by RANK: entry t precedes rank(t) others in (value desc, index asc) order -- indices are distinct, so
      // the ranks are a permutation -- and goes to slot rank(t).  Every thread reads the same list entry at a time (LDS
      // broadcast).  Kept: the first k and every tie with the k-th value (as `scores < topk[-1]` keeps them), capped at
      // SMP_CAP.  (The first version picked the next entry by a wave-wide arg-max, one round per candidate.)
      float mv = 0.f;
      int mi = 0, rank = 0x7fffffff;
      if (tid < ln) {
        mv = list_v[tid];
        mi = list_i[tid];
        rank = 0;
        for (int j = 0; j < ln; ++j) rank += better(list_v[j], list_i[j], mv, mi) ? 1 : 0;
        if (rank < SMP_CAP) { cv[rank] = mv; ci[rank] = mi; }
      }
      __syncthreads();
      const int kk = min(k, ln);
      if (tid < ln && kk > 0 && (rank < kk || mv == cv[kk - 1])) atomicAdd(&keep_n, 1);
      __syncthreads();
      n = min(keep_n, SMP_CAP);
    } else {  // exact fallback: one pass over the vocabulary per candidate
      float pv = INFINITY;
      int pi = -1;
      for (;;) {
        next_best(pv, pi, invT, false);
        const float v = bestv;
        const int i = besti;
        if (i == 0x7fffffff || v == -INFINITY) break;        // nothing (finite) left
        if (n >= k && !(v == cv[k - 1])) break;               // beyond top-k and not a tie with the k-th value
        if (n >= SMP_CAP) break;
        if (tid == 0) { cv[n] = v; ci[n] = i; }
        ++n;
        pv = v;
        pi = i;
        __syncthreads();
      }
    }
    if (tid == 0) {
      // softmax over the kept candidates (descending), top-p: drop the low tail whose cumulative probability, counted
      // from the bottom and including the item, is <= 1 - top_p (keep at least one)
      const float m = cv[0];
      float tot = 0.f;
      for (int j = 0; j < n; ++j) tot += __expf(cv[j] - m);
      int keep = n;
      if (sp.top_p < 1.f) {
        float tail = 0.f;
        for (int j = n - 1; j >= 1; --j) {
          tail += __expf(cv[j] - m) / tot;
          if (tail <= 1.f - sp.top_p) keep = j;
          else break;
        }
      }
      float kt = 0.f;
      for (int j = 0; j < keep; ++j) kt += __expf(cv[j] - m);
      unsigned int r[4];
      philox4x32_10((unsigned int)step, SLOTS ? (unsigned int)out_row[sb] : (unsigned int)b, 0x5A3Bu, 0u, sp.seed_lo, sp.seed_hi, r);
      const float u = (float)(r[0] >> 8) * (1.0f / 16777216.0f) * kt;
      float acc = 0.f;
      int pick = keep - 1;
      for (int j = 0; j < keep; ++j) {
        acc += __expf(cv[j] - m);
        if (u < acc) { pick = j; break; }
      }
      besti = n > 0 ? ci[pick] : 0;
    }
    __syncthreads();
    tok = besti;
  }
  // ---- stop sequences: thread (q, j) compares element j from the end of sequence q with the j-th newest generated token (the new
  // token, then history elements hl - 1 ...); one predicated load each, no data-dependent trip count; a sequence matches when its
  // eight lanes agree (lanes past its length agree by definition)
  bool seq_hit = false;
  if constexpr (STOP) {
    __shared__ int s_seq[2];
    static_assert(SMP_SEQS * SMP_SEQ_LEN == 128 && SMP_SEQ_LEN == 8, "two waves, one sequence per 8 lanes");
    if (sr.n_seqs > 0) {  // (uniform)
      if (tid < SMP_SEQS * SMP_SEQ_LEN) {
        const int q = tid >> 3, j = tid & 7;
        bool ok = false;
        if (q < sr.n_seqs) {
          const int len = sr.seq_len[q];
          const bool len_ok = len >= 1 && len <= SMP_SEQ_LEN && step + 1 >= len;
          const int lc = len_ok ? len : 1;
          const bool mine = j < lc;
          const long want = sr.seqs[q * SMP_SEQ_LEN + (mine ? lc - 1 - j : 0)];
          const bool there = j == 0 || hl - j >= 0;  // (only history elements that exist)
          const long have = j == 0 ? tok : (there ? hist[hl - j] : -1L);
          ok = len_ok && (!mine || (there && have == want));
        }
        unsigned long long m = __builtin_amdgcn_ballot_w64(ok);
        m &= m >> 1; m &= m >> 2; m &= m >> 4;
        if (lane == 0) s_seq[wv] = (m & 0x0101010101010101ull) != 0ull;
      }
      __syncthreads();
      seq_hit = (s_seq[0] | s_seq[1]) != 0;
    }
  }
  // how a live row ends on `tok` (0: it does not), budget aside
  auto end_reason = [&]() -> int {
    if (sp.eos >= 0 && tok == sp.eos) return FIN_EOS;
    if (sr.bitmap && tok >= 0 && tok < V && ((sr.bitmap[tok >> 5] >> (tok & 31)) & 1u)) return FIN_STOP_TOKEN;
    return seq_hit ? FIN_STOP_SEQ : 0;
  };
  auto record = [&](long row, int reason) {
    if (sr.finish_reason) sr.finish_reason[row] = reason;
    if (sr.n_generated) sr.n_generated[row] = step + 1;
  };
  if constexpr (SLOTS) {
    if (tid == 0) {
      if (finished[sb] != 0) {  // inert: the decode step keeps running this slot on the pad token at its frozen position
        cur_tok[sb] = sp.pad;
      } else {
        if (step < out_cap) out_tokens[out_row[sb] * out_cap + step] = tok;
        cur_tok[sb] = tok;
        if (hl < hist_cap) {
          hist[hl] = tok;
          hist_len[sb] = hl + 1;
        }
        if (advance_pos) pos[sb] += 1;
        if constexpr (STOP) {
          int reason = end_reason();
          if (!reason && step + 1 == max_new[sb]) reason = FIN_BUDGET;
          if (reason) {
            finished[sb] = 1;
            record(out_row[sb], reason);
          }
        } else {
          if ((sp.eos >= 0 && tok == sp.eos) || step + 1 == max_new[sb]) finished[sb] = 1;
        }
        step_p[sb] = step + 1;  // (the slot's own word: no ticket)
      }
    }
    return;
  }
  if (tid == 0) {
    // a finished sample keeps emitting the pad token (HF generate pads finished rows)
    const bool fin = finished[b] != 0;
    const long outt = fin ? sp.pad : tok;
    if (step < out_cap) out_tokens[(long)b * out_cap + step] = outt;
    if constexpr (STOP) {
      const int reason = fin ? 0 : end_reason();
      if (reason) {
        finished[b] = 1;
        record(b, reason);
      }
    } else {
      if (!fin && sp.eos >= 0 && tok == sp.eos) finished[b] = 1;
    }
    cur_tok[b] = outt;
    if (hl < hist_cap) {
      hist[hl] = outt;
      hist_len[b] = hl + 1;
    }
    if (advance_pos) pos[b] += 1;
  }
  if (pre && tid == 0) {
    // *step is advanced here instead of by a launch of its own: every workgroup has read it by the time it takes its ticket,
    // and the one that draws the last ticket writes step + 1 and re-arms the counter
    const int t_ = __hip_atomic_fetch_add(ws.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t_ == n_samples - 1) {
      __hip_atomic_store(ws.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *step_p = step + 1;
    }
  }
}

__global__ void step_inc_kernel(int* step) { *step += 1; }

}  // namespace tcavt

using namespace tcavt;

#define TCAVT_TRY(call)              \
  do {                               \
    const int rc_ = (call);          \
    if (rc_ != TCAVT_OK) return rc_; \
  } while (0)

extern "C" int64_t tcavt_sample_workspace_bytes(int B) {
  if (B <= 0) return 0;
  return 64 + (((int64_t)B * 4 + 63) & ~(int64_t)63) + (int64_t)B * SMP_G * 8 + (int64_t)B * SMP_G * SMP_LCAP * 8;
}

// tcavt_sample_logits (max_new == out_row == NULL, one step word), tcavt_sample_logits_slots (arrays [B]) and tcavt_sample_logits_rows
// (slot_of_row: B logits rows on the state of n_state slots) share the launches
static int sample_logits_impl(const char* who, float* logits, int B, int V, const int32_t* slot_of_row, int n_state, int64_t* history,
                              int hist_cap, int32_t* hist_len, const tcavt_sample_params* sp, int32_t* step, const int32_t* max_new, const int64_t* out_row, int64_t* cur_tok,
                              int32_t* pos, int32_t* finished, int64_t* out_tokens, int out_cap, int advance_pos, void* workspace,
                              int64_t workspace_bytes, tcavt_stream_t stream, const tcavt_stop_rules* rules = nullptr) {
  const bool slots = max_new || out_row;
  // ending rules: with none set (or rules == NULL) the launches below are the instantiations without STOP, argument for argument
  StopP sr = {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
  bool stop = false;
  if (rules) {
    TCAVT_CHECK_ARG(rules->n_seqs >= 0 && rules->n_seqs <= SMP_SEQS, "%s: stop rules: n_seqs = %d outside [0, %d]", who, rules->n_seqs, SMP_SEQS);
    TCAVT_CHECK_ARG(rules->n_seqs == 0 || rules->stop_seqs, "%s: stop rules: stop_seqs is a null pointer with n_seqs = %d", who, rules->n_seqs);
    TCAVT_CHECK_ARG(rules->n_seqs == 0 || rules->stop_seq_len, "%s: stop rules: stop_seq_len is a null pointer with n_seqs = %d", who, rules->n_seqs);
    TCAVT_CHECK_ARG(rules->min_new_tokens >= 0, "%s: stop rules: min_new_tokens = %d must be >= 0", who, rules->min_new_tokens);
    TCAVT_CHECK_ARG(rules->min_new_tokens == 0 || sp->eos_token_id >= 0 || rules->stop_bitmap,
                    "%s: stop rules: min_new_tokens = %d with neither eos_token_id nor stop_bitmap (nothing to ban)", who, rules->min_new_tokens);
    TCAVT_CHECK_ARG((reinterpret_cast<uintptr_t>(rules->stop_bitmap) & 3) == 0, "%s: stop rules: stop_bitmap must be 4-byte aligned", who);
    sr.bitmap = rules->stop_bitmap;
    sr.seqs = rules->n_seqs > 0 ? reinterpret_cast<const long*>(rules->stop_seqs) : nullptr;
    sr.seq_len = rules->n_seqs > 0 ? rules->stop_seq_len : nullptr;
    sr.finish_reason = rules->finish_reason; sr.n_generated = rules->n_generated;
    sr.n_seqs = rules->n_seqs; sr.min_new = rules->min_new_tokens;
    stop = sr.bitmap || sr.n_seqs > 0 || sr.min_new > 0 || sr.finish_reason || sr.n_generated;
  }
  TCAVT_CHECK_ARG(!sp->do_sample || (sp->temperature > 0.f && sp->top_k >= 1 && sp->top_k <= SMP_CAP && sp->top_p > 0.f && sp->top_p <= 1.f),
                  "%s: sampling needs temperature > 0, 1 <= top_k <= %d, 0 < top_p <= 1", who, SMP_CAP);
  TCAVT_CHECK_ARG(sp->repetition_penalty > 0.f && sp->no_repeat_ngram_size >= 0, "%s: bad repetition_penalty / no_repeat_ngram_size", who);
  SampleP p;
  p.temperature = sp->temperature; p.top_p = sp->top_p; p.rep_penalty = sp->repetition_penalty;
  p.top_k = sp->top_k; p.no_repeat_ngram = sp->no_repeat_ngram_size; p.do_sample = sp->do_sample;
  p.eos = sp->eos_token_id; p.pad = sp->pad_token_id;
  p.seed_lo = (unsigned int)(sp->seed & 0xffffffffu); p.seed_hi = (unsigned int)(sp->seed >> 32);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // two-stage form when the caller lends a workspace and the rows can be cut into 16-byte-aligned slices that fit the registers
  SliceWs ws = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  const int64_t need = tcavt_sample_workspace_bytes(B);
  const int chunk4 = ((V >> 2) + SMP_G - 1) / SMP_G;
  if (workspace && workspace_bytes >= need && (V & 3) == 0 && aligned16(logits) && chunk4 <= SMP_E4 * SMP_T) {
    TCAVT_CHECK_ARG(aligned16(workspace), "%s: workspace must be 16-byte aligned", who);
    char* w = static_cast<char*>(workspace);
    ws.ticket = reinterpret_cast<int*>(w);
    ws.ovf = reinterpret_cast<int*>(w + 64);
    size_t off = 64 + (((size_t)B * 4 + 63) & ~(size_t)63);
    ws.cand_n = reinterpret_cast<int*>(w + off); off += (size_t)B * SMP_G * 4;
    ws.lb = reinterpret_cast<float*>(w + off); off += (size_t)B * SMP_G * 4;
    ws.cand_v = reinterpret_cast<float*>(w + off); off += (size_t)B * SMP_G * SMP_LCAP * 4;
    ws.cand_i = reinterpret_cast<int*>(w + off);
    hipLaunchKernelGGL(stop ? sample_slice_kernel<true> : sample_slice_kernel<false>, dim3(B * SMP_G), dim3(SMP_T), 0, st, logits, V,
                       reinterpret_cast<const long*>(history), hist_cap, hist_len, p, ws, slot_of_row, n_state, sr, step, slots ? 1 : 0, finished);
  }
  auto* kern = slot_of_row ? sample_kernel<SMP_ROWS> : slots ? sample_kernel<SMP_SLOTS> : sample_kernel<SMP_BATCH>;
  if (stop) kern = slot_of_row ? sample_kernel<SMP_ROWS, true> : slots ? sample_kernel<SMP_SLOTS, true> : sample_kernel<SMP_BATCH, true>;
  hipLaunchKernelGGL(kern, dim3(B), dim3(SMP_T),
                     0, st, logits, V, reinterpret_cast<long*>(history), hist_cap, hist_len, p, step, reinterpret_cast<long*>(cur_tok), pos,
                     finished, reinterpret_cast<long*>(out_tokens), out_cap, advance_pos, ws, B, max_new,
                     reinterpret_cast<const long*>(out_row), slot_of_row, n_state, sr);
  if (!ws.cand_v && !slots) hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, st, step);
  TCAVT_CHECK_LAUNCH(who);
  return TCAVT_OK;
}

extern "C" int tcavt_sample_logits(float* logits, int B, int V, int64_t* history, int hist_cap, int32_t* hist_len,
                                   const tcavt_sample_params* sp, int32_t* step, int64_t* cur_tok, int32_t* pos,
                                   int32_t* finished, int64_t* out_tokens, int out_cap, int advance_pos, void* workspace,
                                   int64_t workspace_bytes, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(logits && history && hist_len && sp && step && cur_tok && pos && finished && out_tokens && B > 0 && V > 0 &&
                      hist_cap > 0 && out_cap > 0,
                  "sample_logits: bad args");
  return sample_logits_impl("sample_logits", logits, B, V, nullptr, B, history, hist_cap, hist_len, sp, step, nullptr, nullptr, cur_tok, pos, finished,
                            out_tokens, out_cap, advance_pos, workspace, workspace_bytes, stream);
}

extern "C" int tcavt_sample_logits_slots(float* logits, int S, int V, int64_t* history, int hist_cap, int32_t* hist_len,
                                         const tcavt_sample_params* sp, int32_t* step, const int32_t* max_new, const int64_t* out_row,
                                         int64_t* cur_tok, int32_t* pos, int32_t* finished, int64_t* out_tokens, int out_cap,
                                         int advance_pos, void* workspace, int64_t workspace_bytes, tcavt_stream_t stream) {
  const struct { const void* p; const char* name; } ptrs[] = {
      {logits, "logits"}, {history, "history"}, {hist_len, "hist_len"}, {sp, "params"}, {step, "step"}, {max_new, "max_new"},
      {out_row, "out_row"}, {cur_tok, "cur_tok"}, {pos, "pos"}, {finished, "finished"}, {out_tokens, "out_tokens"}};
  for (const auto& a : ptrs) TCAVT_CHECK_ARG(a.p, "sample_logits_slots: %s is a null pointer", a.name);
  TCAVT_CHECK_ARG(S > 0, "sample_logits_slots: S = %d must be > 0", S);
  TCAVT_CHECK_ARG(V > 0, "sample_logits_slots: V = %d must be > 0", V);
  TCAVT_CHECK_ARG(hist_cap > 0, "sample_logits_slots: hist_cap = %d must be > 0", hist_cap);
  TCAVT_CHECK_ARG(out_cap > 0, "sample_logits_slots: out_cap = %d must be > 0", out_cap);
  return sample_logits_impl("sample_logits_slots", logits, S, V, nullptr, S, history, hist_cap, hist_len, sp, step, max_new, out_row, cur_tok, pos,
                            finished, out_tokens, out_cap, advance_pos, workspace, workspace_bytes, stream);
}

extern "C" int tcavt_sample_logits_rows(float* logits, int G, int V, const int32_t* slot_of_row, int S, int64_t* history, int hist_cap,
                                        int32_t* hist_len, const tcavt_sample_params* sp, int32_t* step, const int32_t* max_new,
                                        const int64_t* out_row, int64_t* cur_tok, int32_t* pos, int32_t* finished, int64_t* out_tokens,
                                        int out_cap, int advance_pos, void* workspace, int64_t workspace_bytes, tcavt_stream_t stream) {
  const struct { const void* p; const char* name; } ptrs[] = {
      {logits, "logits"}, {slot_of_row, "slot_of_row"}, {history, "history"}, {hist_len, "hist_len"}, {sp, "params"}, {step, "step"},
      {max_new, "max_new"}, {out_row, "out_row"}, {cur_tok, "cur_tok"}, {pos, "pos"}, {finished, "finished"}, {out_tokens, "out_tokens"}};
  for (const auto& a : ptrs) TCAVT_CHECK_ARG(a.p, "sample_logits_rows: %s is a null pointer", a.name);
  TCAVT_CHECK_ARG(G > 0, "sample_logits_rows: G = %d must be > 0", G);
  TCAVT_CHECK_ARG(S > 0, "sample_logits_rows: S = %d must be > 0", S);
  TCAVT_CHECK_ARG(V > 0, "sample_logits_rows: V = %d must be > 0", V);
  TCAVT_CHECK_ARG(hist_cap > 0, "sample_logits_rows: hist_cap = %d must be > 0", hist_cap);
  TCAVT_CHECK_ARG(out_cap > 0, "sample_logits_rows: out_cap = %d must be > 0", out_cap);
  return sample_logits_impl("sample_logits_rows", logits, G, V, slot_of_row, S, history, hist_cap, hist_len, sp, step, max_new, out_row,
                            cur_tok, pos, finished, out_tokens, out_cap, advance_pos, workspace, workspace_bytes, stream);
}

extern "C" int tcavt_sample_tokens(const tcavt_sample_args* a, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(a, "sample_tokens: args is a null pointer");
  const bool rows = a->slot_of_row != nullptr, slots = rows || a->max_new || a->out_row;
  const struct { const void* p; const char* name; bool need; } ptrs[] = {
      {a->logits, "logits", true}, {a->history, "history", true}, {a->hist_len, "hist_len", true}, {a->params, "params", true},
      {a->step, "step", true}, {a->max_new, "max_new", slots}, {a->out_row, "out_row", slots}, {a->cur_tok, "cur_tok", true},
      {a->pos, "pos", true}, {a->finished, "finished", true}, {a->out_tokens, "out_tokens", true}};
  for (const auto& q : ptrs) TCAVT_CHECK_ARG(q.p || !q.need, "sample_tokens: %s is a null pointer", q.name);
  TCAVT_CHECK_ARG(a->rows > 0, "sample_tokens: rows = %d must be > 0", a->rows);
  TCAVT_CHECK_ARG(a->V > 0, "sample_tokens: V = %d must be > 0", a->V);
  TCAVT_CHECK_ARG(!rows || a->n_state > 0, "sample_tokens: n_state = %d must be > 0 with slot_of_row", a->n_state);
  TCAVT_CHECK_ARG(a->hist_cap > 0, "sample_tokens: hist_cap = %d must be > 0", a->hist_cap);
  TCAVT_CHECK_ARG(a->out_cap > 0, "sample_tokens: out_cap = %d must be > 0", a->out_cap);
  return sample_logits_impl("sample_tokens", a->logits, a->rows, a->V, a->slot_of_row, rows ? a->n_state : a->rows, a->history, a->hist_cap,
                            a->hist_len, a->params, a->step, a->max_new, a->out_row, a->cur_tok, a->pos, a->finished, a->out_tokens,
                            a->out_cap, a->advance_pos, a->workspace, a->workspace_bytes, stream, a->stop);
}

extern "C" int tcavt_gather_last(const void* src16, const int32_t* kv_len, void* out16, int B, int L, int H,
                                 tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(src16 && kv_len && out16 && B > 0 && L > 0 && H > 0 && H % 8 == 0, "gather_last: bad args");
  hipLaunchKernelGGL(gather_last_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(src16), kv_len, static_cast<bf16_t*>(out16), L, H);
  TCAVT_CHECK_LAUNCH("gather_last");
  return TCAVT_OK;
}

// The decode attention's host rule: KS key splits (waves) per query head -- one 64-key round each up to 1024 keys, two beyond --
// and the LDS bytes of [kv_lmax] scores | [KS][2] (max, sum) | [KS][64] partial outputs.  false: the scores do not fit 64 KiB.
static bool attn_decode_rule(int kv_lmax, int* KS, size_t* lds) {
  *KS = std::min(16, (kv_lmax + 63) / 64);
  *lds = ((size_t)kv_lmax + (size_t)*KS * 66) * sizeof(float);
  return *lds <= 64 * 1024;
}

extern "C" int tcavt_attn_decode(const void* qkv, void* k_cache, void* v_cache, const int32_t* pos, void* out, int B, int nq, int nkv,
                                 int kv_lmax, float scale, int dtype16, int out_layout, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(qkv && k_cache && v_cache && pos && out, "attn_decode: null pointer");
  TCAVT_CHECK_ARG(is16(dtype16), "attn_decode: dtype16 must be TCAVT_F16 or TCAVT_BF16");
  TCAVT_CHECK_ARG(B > 0 && nq > 0 && nkv > 0 && nq % nkv == 0 && nq / nkv <= 8, "attn_decode: bad shape (B, nq, nkv > 0, nq %% nkv == 0, nq / nkv <= 8)");
  TCAVT_CHECK_ARG(kv_lmax >= 1, "attn_decode: kv_lmax must be >= 1");
  int KS;
  size_t lds;
  TCAVT_CHECK_ARG(attn_decode_rule(kv_lmax, &KS, &lds), "attn_decode: kv_lmax = %d too long for the score buffer", kv_lmax);
  TCAVT_CHECK_ARG(out_layout == 0 || (out_layout == 1 && B <= 32 && (nq * 64) % 256 == 0) || (out_layout == 2 && B <= 8),
                  "attn_decode: out_layout must be 0, 1 (B <= 32, nq * 64 %% 256 == 0) or 2 (B <= 8)");
  TCAVT_CHECK_ARG(aligned16(qkv) && aligned16(k_cache) && aligned16(v_cache), "attn_decode: qkv and the caches must be 16-byte aligned");
  const bool pfv = B * nq <= 512;  // (value-row prefetch: only while the grid is about one workgroup per CU)
  auto kfn = dtype16 == TCAVT_F16 ? (pfv ? attn_decode_kernel<true, true> : attn_decode_kernel<true, false>)
                                  : (pfv ? attn_decode_kernel<false, true> : attn_decode_kernel<false, false>);
  hipLaunchKernelGGL(kfn, dim3(B * nq), dim3(KS * 64), lds, static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(qkv),
                     static_cast<bf16_t*>(k_cache), static_cast<bf16_t*>(v_cache), pos, static_cast<bf16_t*>(out), kv_lmax, nq, nkv, scale,
                     KS, out_layout);
  TCAVT_CHECK_LAUNCH("attn_decode");
  return TCAVT_OK;
}

// tcavt_attn_decode8 launches by tcavt_attn_decode's rule (KS waves, the same LDS layout), applied to the CACHED keys: per sample
// pos[b] of them in chunks of ceil(ceil(pos[b] / KS) / 64) * 64.  One instantiation per 16-bit type.
extern "C" int tcavt_kv_store8(const void* qkv, int B, int L, int kv_lmax, int nq, int nkv, int dtype16, void* k_codes, void* k_scales,
                               void* v_codes, void* v_scales, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(qkv && k_codes && k_scales && v_codes && v_scales, "kv_store8: null pointer");
  TCAVT_CHECK_ARG(is16(dtype16), "kv_store8: dtype16 must be TCAVT_F16 or TCAVT_BF16");
  TCAVT_CHECK_ARG(B > 0 && L > 0 && nq > 0 && nkv > 0, "kv_store8: bad shape (B, L, nq, nkv > 0)");
  TCAVT_CHECK_ARG(kv_lmax >= L, "kv_store8: kv_lmax = %d must be >= L = %d", kv_lmax, L);
  TCAVT_CHECK_ARG(aligned16(qkv) && aligned16(k_codes) && aligned16(v_codes) && (reinterpret_cast<uintptr_t>(k_scales) & 1) == 0 &&
                      (reinterpret_cast<uintptr_t>(v_scales) & 1) == 0,
                  "kv_store8: qkv and the code planes must be 16-byte aligned, the scale planes 2-byte aligned");
  const long pieces = (long)B * L * 2 * nkv * 8;
  TCAVT_CHECK_ARG((pieces + 255) / 256 <= 0x7fffffffL, "kv_store8: too many rows");
  auto kfn = dtype16 == TCAVT_F16 ? kv_store8_kernel<true> : kv_store8_kernel<false>;
  hipLaunchKernelGGL(kfn, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     static_cast<const bf16_t*>(qkv), static_cast<unsigned char*>(k_codes), static_cast<unsigned char*>(k_scales),
                     static_cast<unsigned char*>(v_codes), static_cast<unsigned char*>(v_scales), pieces, L, kv_lmax, nq, nkv);
  TCAVT_CHECK_LAUNCH("kv_store8");
  return TCAVT_OK;
}

extern "C" int tcavt_attn_decode8(const void* qkv, void* k_codes, void* k_scales, void* v_codes, void* v_scales, const int32_t* pos,
                                  void* out, int B, int nq, int nkv, int kv_lmax, float scale, int dtype16, int out_layout,
                                  tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(qkv && k_codes && k_scales && v_codes && v_scales && pos && out, "attn_decode8: null pointer");
  TCAVT_CHECK_ARG(is16(dtype16), "attn_decode8: dtype16 must be TCAVT_F16 or TCAVT_BF16");
  TCAVT_CHECK_ARG(B > 0 && nq > 0 && nkv > 0 && nq % nkv == 0 && nq / nkv <= 8, "attn_decode8: bad shape (B, nq, nkv > 0, nq %% nkv == 0, nq / nkv <= 8)");
  TCAVT_CHECK_ARG(kv_lmax >= 1, "attn_decode8: kv_lmax must be >= 1");
  int KS;
  size_t lds;
  TCAVT_CHECK_ARG(attn_decode_rule(kv_lmax, &KS, &lds), "attn_decode8: kv_lmax = %d too long for the score buffer", kv_lmax);
  TCAVT_CHECK_ARG(out_layout == 0 || (out_layout == 1 && B <= 32 && (nq * 64) % 256 == 0) || (out_layout == 2 && B <= 8),
                  "attn_decode8: out_layout must be 0, 1 (B <= 32, nq * 64 %% 256 == 0) or 2 (B <= 8)");
  TCAVT_CHECK_ARG(aligned16(qkv) && aligned16(k_codes) && aligned16(v_codes), "attn_decode8: qkv and the code planes must be 16-byte aligned");
  auto kfn = dtype16 == TCAVT_F16 ? attn_decode8_kernel<true> : attn_decode8_kernel<false>;
  hipLaunchKernelGGL(kfn, dim3(B * nq), dim3(KS * 64), lds, static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(qkv),
                     static_cast<unsigned char*>(k_codes), static_cast<unsigned char*>(k_scales), static_cast<unsigned char*>(v_codes),
                     static_cast<unsigned char*>(v_scales), pos, static_cast<bf16_t*>(out), kv_lmax, nq, nkv, scale, KS, out_layout);
  TCAVT_CHECK_LAUNCH("attn_decode8");
  return TCAVT_OK;
}

extern "C" int tcavt_slot_admit(const tcavt_slot_admit_args* a, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(a, "slot_admit: args is a null pointer");
  const bool f16 = a->src_k || a->src_v || a->dst_k || a->dst_v;
  const bool kv8 = a->src_k_codes || a->src_k_scales || a->src_v_codes || a->src_v_scales || a->dst_k_codes || a->dst_k_scales ||
                   a->dst_v_codes || a->dst_v_scales;
  TCAVT_CHECK_ARG(!(f16 && kv8), "slot_admit: the 16-bit caches (src_k .. dst_v) and the kv8 planes exclude each other");
  TCAVT_CHECK_ARG(f16 || kv8, "slot_admit: null pointer (src_k / src_v / dst_k / dst_v, or the eight kv8 planes)");
  TCAVT_CHECK_ARG(!f16 || (a->src_k && a->src_v && a->dst_k && a->dst_v), "slot_admit: null pointer: src_k, src_v, dst_k and dst_v come together");
  TCAVT_CHECK_ARG(!kv8 || (a->src_k_codes && a->src_k_scales && a->src_v_codes && a->src_v_scales && a->dst_k_codes && a->dst_k_scales &&
                           a->dst_v_codes && a->dst_v_scales),
                  "slot_admit: null pointer: the eight kv8 planes come together");
  const struct { const void* p; const char* name; } ptrs[] = {
      {a->prompt_ids, "prompt_ids"}, {a->kv_len, "kv_len"}, {a->history, "history"}, {a->hist_len, "hist_len"}, {a->step, "step"},
      {a->max_new, "max_new"}, {a->out_row, "out_row"}, {a->pos, "pos"}, {a->finished, "finished"}, {a->cur_tok, "cur_tok"}};
  for (const auto& q : ptrs) TCAVT_CHECK_ARG(q.p, "slot_admit: %s is a null pointer", q.name);
  TCAVT_CHECK_ARG(is16(a->dtype16), "slot_admit: dtype16 must be TCAVT_F16 or TCAVT_BF16");
  TCAVT_CHECK_ARG(a->n_layers > 0 && a->S > 0 && a->nkv > 0 && a->src_lmax > 0 && a->kv_lmax > 0,
                  "slot_admit: bad shape (n_layers, S, nkv, src_lmax, kv_lmax > 0)");
  TCAVT_CHECK_ARG(a->slot >= 0 && a->slot < a->S, "slot_admit: slot = %d outside [0, S = %d)", a->slot, a->S);
  TCAVT_CHECK_ARG(a->rows >= 1 && a->rows <= std::min(a->src_lmax, a->kv_lmax), "slot_admit: rows = %d must be in [1, min(src_lmax = %d, kv_lmax = %d)]",
                  a->rows, a->src_lmax, a->kv_lmax);
  TCAVT_CHECK_ARG(a->hist_cap > 0 && a->n_ids >= 0 && a->n_ids <= a->hist_cap, "slot_admit: n_ids = %d must be in [0, hist_cap = %d]", a->n_ids,
                  a->hist_cap);
  TCAVT_CHECK_ARG(a->n_image >= 0 && a->max_new_value >= 1 && a->out_row_value >= 0,
                  "slot_admit: n_image >= 0, max_new_value >= 1 and out_row_value >= 0 required");
  AdmitP p = {};
  if (kv8) {
    TCAVT_CHECK_ARG(aligned16(a->src_k_codes) && aligned16(a->src_v_codes) && aligned16(a->dst_k_codes) && aligned16(a->dst_v_codes),
                    "slot_admit: the code planes must be 16-byte aligned");
    TCAVT_CHECK_ARG(((reinterpret_cast<uintptr_t>(a->src_k_scales) | reinterpret_cast<uintptr_t>(a->src_v_scales) |
                      reinterpret_cast<uintptr_t>(a->dst_k_scales) | reinterpret_cast<uintptr_t>(a->dst_v_scales)) & 1) == 0,
                    "slot_admit: the scale planes must be 2-byte aligned");
    const void* src[4] = {a->src_k_codes, a->src_v_codes, a->src_k_scales, a->src_v_scales};
    void* dst[4] = {a->dst_k_codes, a->dst_v_codes, a->dst_k_scales, a->dst_v_scales};
    for (int i = 0; i < 4; ++i) { p.src[i] = static_cast<const unsigned char*>(src[i]); p.dst[i] = static_cast<unsigned char*>(dst[i]); }
    p.inner = a->nkv; p.row_bytes = 64;
  } else {
    TCAVT_CHECK_ARG(aligned16(a->src_k) && aligned16(a->src_v) && aligned16(a->dst_k) && aligned16(a->dst_v),
                    "slot_admit: the caches must be 16-byte aligned");
    p.src[0] = static_cast<const unsigned char*>(a->src_k); p.src[1] = static_cast<const unsigned char*>(a->src_v);
    p.dst[0] = static_cast<unsigned char*>(a->dst_k); p.dst[1] = static_cast<unsigned char*>(a->dst_v);
    p.inner = 1; p.row_bytes = a->nkv * 128;
  }
  p.segs = a->n_layers * p.inner;
  p.S = a->S; p.slot = a->slot; p.rows = a->rows; p.src_lmax = a->src_lmax; p.kv_lmax = a->kv_lmax;
  p.pieces = (long)a->rows * (p.row_bytes / 16);
  p.n_wide = 2L * p.segs * p.pieces;
  p.n_copy = p.n_wide + (kv8 ? 2L * p.segs * a->rows : 0L);
  const long blocks = (p.n_copy + 255) / 256 + 1;
  TCAVT_CHECK_ARG(blocks <= 0x7fffffffL, "slot_admit: too many rows");
  p.prompt_ids = reinterpret_cast<const long*>(a->prompt_ids); p.kv_len = a->kv_len; p.history = reinterpret_cast<long*>(a->history);
  p.hist_len = a->hist_len; p.step = a->step; p.max_new = a->max_new; p.pos = a->pos; p.finished = a->finished;
  p.out_row = reinterpret_cast<long*>(a->out_row); p.out_row_value = a->out_row_value;
  p.n_ids = a->n_ids; p.hist_cap = a->hist_cap; p.n_image = a->n_image; p.max_new_value = a->max_new_value;
  hipLaunchKernelGGL(slot_admit_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  TCAVT_CHECK_LAUNCH("slot_admit");
  return TCAVT_OK;
}

extern "C" int tcavt_slot_admit_group(const tcavt_slot_admit_group_args* a, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(a, "slot_admit_group: args is a null pointer");
  const bool f16 = a->src_k || a->src_v || a->dst_k || a->dst_v;
  const bool kv8 = a->src_k_codes || a->src_k_scales || a->src_v_codes || a->src_v_scales || a->dst_k_codes || a->dst_k_scales ||
                   a->dst_v_codes || a->dst_v_scales;
  TCAVT_CHECK_ARG(!(f16 && kv8), "slot_admit_group: the 16-bit caches (src_k .. dst_v) and the kv8 planes exclude each other");
  TCAVT_CHECK_ARG(f16 || kv8, "slot_admit_group: null pointer (src_k / src_v / dst_k / dst_v, or the eight kv8 planes)");
  TCAVT_CHECK_ARG(!f16 || (a->src_k && a->src_v && a->dst_k && a->dst_v),
                  "slot_admit_group: null pointer: src_k, src_v, dst_k and dst_v come together");
  TCAVT_CHECK_ARG(!kv8 || (a->src_k_codes && a->src_k_scales && a->src_v_codes && a->src_v_scales && a->dst_k_codes && a->dst_k_scales &&
                           a->dst_v_codes && a->dst_v_scales),
                  "slot_admit_group: null pointer: the eight kv8 planes come together");
  const struct { const void* p; const char* name; } ptrs[] = {
      {a->slot, "slot"}, {a->kv_len, "kv_len"}, {a->max_new_value, "max_new_value"}, {a->out_row_value, "out_row_value"},
      {a->prompt_ids, "prompt_ids"}, {a->bad_slot_flag, "bad_slot_flag"}, {a->history, "history"}, {a->hist_len, "hist_len"},
      {a->step, "step"}, {a->max_new, "max_new"}, {a->out_row, "out_row"}, {a->pos, "pos"}, {a->finished, "finished"}, {a->cur_tok, "cur_tok"}};
  for (const auto& q : ptrs) TCAVT_CHECK_ARG(q.p, "slot_admit_group: %s is a null pointer", q.name);
  TCAVT_CHECK_ARG(is16(a->dtype16), "slot_admit_group: dtype16 must be TCAVT_F16 or TCAVT_BF16");
  TCAVT_CHECK_ARG(a->G >= 1, "slot_admit_group: G = %d must be >= 1", a->G);
  TCAVT_CHECK_ARG(a->G <= 65535, "slot_admit_group: G = %d must be <= 65535", a->G);
  TCAVT_CHECK_ARG(a->n_layers > 0 && a->S > 0 && a->nkv > 0 && a->src_lmax > 0 && a->kv_lmax > 0,
                  "slot_admit_group: bad shape (n_layers, S, nkv, src_lmax, kv_lmax > 0)");
  TCAVT_CHECK_ARG(a->rows >= 1 && a->rows <= std::min(a->src_lmax, a->kv_lmax),
                  "slot_admit_group: rows = %d must be in [1, min(src_lmax = %d, kv_lmax = %d)]", a->rows, a->src_lmax, a->kv_lmax);
  TCAVT_CHECK_ARG(a->hist_cap > 0 && a->n_ids >= 0 && a->n_ids <= a->hist_cap, "slot_admit_group: n_ids = %d must be in [0, hist_cap = %d]",
                  a->n_ids, a->hist_cap);
  TCAVT_CHECK_ARG(a->n_image >= 0, "slot_admit_group: n_image = %d must be >= 0", a->n_image);
  AdmitGroupP p = {};
  if (kv8) {
    TCAVT_CHECK_ARG(aligned16(a->src_k_codes) && aligned16(a->src_v_codes) && aligned16(a->dst_k_codes) && aligned16(a->dst_v_codes),
                    "slot_admit_group: the code planes must be 16-byte aligned");
    TCAVT_CHECK_ARG(((reinterpret_cast<uintptr_t>(a->src_k_scales) | reinterpret_cast<uintptr_t>(a->src_v_scales) |
                      reinterpret_cast<uintptr_t>(a->dst_k_scales) | reinterpret_cast<uintptr_t>(a->dst_v_scales)) & 1) == 0,
                    "slot_admit_group: the scale planes must be 2-byte aligned");
    const void* src[4] = {a->src_k_codes, a->src_v_codes, a->src_k_scales, a->src_v_scales};
    void* dst[4] = {a->dst_k_codes, a->dst_v_codes, a->dst_k_scales, a->dst_v_scales};
    for (int i = 0; i < 4; ++i) { p.src[i] = static_cast<const unsigned char*>(src[i]); p.dst[i] = static_cast<unsigned char*>(dst[i]); }
    p.inner = a->nkv; p.row_bytes = 64;
  } else {
    TCAVT_CHECK_ARG(aligned16(a->src_k) && aligned16(a->src_v) && aligned16(a->dst_k) && aligned16(a->dst_v),
                    "slot_admit_group: the caches must be 16-byte aligned");
    p.src[0] = static_cast<const unsigned char*>(a->src_k); p.src[1] = static_cast<const unsigned char*>(a->src_v);
    p.dst[0] = static_cast<unsigned char*>(a->dst_k); p.dst[1] = static_cast<unsigned char*>(a->dst_v);
    p.inner = 1; p.row_bytes = a->nkv * 128;
  }
  p.segs = a->n_layers * p.inner;
  p.S = a->S; p.G = a->G; p.rows = a->rows; p.src_lmax = a->src_lmax; p.kv_lmax = a->kv_lmax;
  p.pieces = (long)a->rows * (p.row_bytes / 16);
  p.n_wide = 2L * p.segs * p.pieces;
  p.n_copy = p.n_wide + (kv8 ? 2L * p.segs * a->rows : 0L);
  const long blocks = (p.n_copy + 255) / 256 + 1;
  TCAVT_CHECK_ARG(blocks <= 0x7fffffffL, "slot_admit_group: too many rows");
  p.slot = a->slot; p.kv_len = a->kv_len; p.max_new_value = a->max_new_value;
  p.out_row_value = reinterpret_cast<const long*>(a->out_row_value); p.prompt_ids = reinterpret_cast<const long*>(a->prompt_ids);
  p.bad_slot_flag = a->bad_slot_flag; p.history = reinterpret_cast<long*>(a->history);
  p.hist_len = a->hist_len; p.step = a->step; p.max_new = a->max_new; p.pos = a->pos; p.finished = a->finished;
  p.out_row = reinterpret_cast<long*>(a->out_row);
  p.n_ids = a->n_ids; p.hist_cap = a->hist_cap; p.n_image = a->n_image;
  hipLaunchKernelGGL(slot_admit_group_kernel, dim3((unsigned)blocks, (unsigned)a->G), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  TCAVT_CHECK_LAUNCH("slot_admit_group");
  return TCAVT_OK;
}

extern "C" int tcavt_kv_fanout(const tcavt_kv_fanout_args* a, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(a, "kv_fanout: args is a null pointer");
  const bool f16 = a->src_k || a->src_v || a->dst_k || a->dst_v;
  const bool kv8 = a->src_k_codes || a->src_k_scales || a->src_v_codes || a->src_v_scales || a->dst_k_codes || a->dst_k_scales ||
                   a->dst_v_codes || a->dst_v_scales;
  TCAVT_CHECK_ARG(!(f16 && kv8), "kv_fanout: the 16-bit caches (src_k .. dst_v) and the kv8 planes exclude each other");
  TCAVT_CHECK_ARG(f16 || kv8, "kv_fanout: null pointer (src_k / src_v / dst_k / dst_v, or the eight kv8 planes)");
  TCAVT_CHECK_ARG(!f16 || (a->src_k && a->src_v && a->dst_k && a->dst_v), "kv_fanout: null pointer: src_k, src_v, dst_k and dst_v come together");
  TCAVT_CHECK_ARG(!kv8 || (a->src_k_codes && a->src_k_scales && a->src_v_codes && a->src_v_scales && a->dst_k_codes && a->dst_k_scales &&
                           a->dst_v_codes && a->dst_v_scales),
                  "kv_fanout: null pointer: the eight kv8 planes come together");
  const struct { const void* p; const char* name; } ptrs[] = {
      {a->prompt_ids, "prompt_ids"}, {a->kv_len, "kv_len"}, {a->logits_src, "logits_src"}, {a->logits_dst, "logits_dst"},
      {a->history, "history"}, {a->hist_len, "hist_len"}, {a->pos, "pos"}, {a->finished, "finished"}};
  for (const auto& q : ptrs) TCAVT_CHECK_ARG(q.p, "kv_fanout: %s is a null pointer", q.name);
  TCAVT_CHECK_ARG(is16(a->dtype16), "kv_fanout: dtype16 must be TCAVT_F16 or TCAVT_BF16");
  TCAVT_CHECK_ARG(a->B >= 1, "kv_fanout: B = %d must be >= 1", a->B);
  TCAVT_CHECK_ARG(a->n >= 1, "kv_fanout: n = %d must be >= 1", a->n);
  TCAVT_CHECK_ARG((long)a->B * a->n <= 0x7fffffffL, "kv_fanout: B * n = %ld rows are too many", (long)a->B * a->n);
  TCAVT_CHECK_ARG(a->n_layers > 0 && a->nkv > 0 && a->src_lmax > 0 && a->kv_lmax > 0,
                  "kv_fanout: bad shape (n_layers, nkv, src_lmax, kv_lmax > 0)");
  TCAVT_CHECK_ARG(a->rows >= 1 && a->rows <= std::min(a->src_lmax, a->kv_lmax), "kv_fanout: rows = %d must be in [1, min(src_lmax = %d, kv_lmax = %d)]",
                  a->rows, a->src_lmax, a->kv_lmax);
  TCAVT_CHECK_ARG(a->hist_cap > 0 && a->n_ids >= 0 && a->n_ids <= a->hist_cap, "kv_fanout: n_ids = %d must be in [0, hist_cap = %d]", a->n_ids,
                  a->hist_cap);
  TCAVT_CHECK_ARG(a->n_image >= 0, "kv_fanout: n_image = %d must be >= 0", a->n_image);
  TCAVT_CHECK_ARG(a->V >= 1, "kv_fanout: V = %d must be >= 1", a->V);
  TCAVT_CHECK_ARG(aligned16(a->logits_src) && aligned16(a->logits_dst), "kv_fanout: logits_src and logits_dst must be 16-byte aligned");
  FanoutP p = {};
  if (kv8) {
    TCAVT_CHECK_ARG(aligned16(a->src_k_codes) && aligned16(a->src_v_codes) && aligned16(a->dst_k_codes) && aligned16(a->dst_v_codes),
                    "kv_fanout: the code planes must be 16-byte aligned");
    TCAVT_CHECK_ARG(((reinterpret_cast<uintptr_t>(a->src_k_scales) | reinterpret_cast<uintptr_t>(a->src_v_scales) |
                      reinterpret_cast<uintptr_t>(a->dst_k_scales) | reinterpret_cast<uintptr_t>(a->dst_v_scales)) & 1) == 0,
                    "kv_fanout: the scale planes must be 2-byte aligned");
    const void* src[4] = {a->src_k_codes, a->src_v_codes, a->src_k_scales, a->src_v_scales};
    void* dst[4] = {a->dst_k_codes, a->dst_v_codes, a->dst_k_scales, a->dst_v_scales};
    for (int i = 0; i < 4; ++i) { p.src[i] = static_cast<const unsigned char*>(src[i]); p.dst[i] = static_cast<unsigned char*>(dst[i]); }
    p.inner = a->nkv; p.row_bytes = 64;
  } else {
    TCAVT_CHECK_ARG(aligned16(a->src_k) && aligned16(a->src_v) && aligned16(a->dst_k) && aligned16(a->dst_v),
                    "kv_fanout: the caches must be 16-byte aligned");
    p.src[0] = static_cast<const unsigned char*>(a->src_k); p.src[1] = static_cast<const unsigned char*>(a->src_v);
    p.dst[0] = static_cast<unsigned char*>(a->dst_k); p.dst[1] = static_cast<unsigned char*>(a->dst_v);
    p.inner = 1; p.row_bytes = a->nkv * 128;
  }
  const long segs = (long)a->n_layers * a->B * p.inner;
  TCAVT_CHECK_ARG(segs <= 0x7fffffffL, "kv_fanout: n_layers * B * nkv is too large");
  p.segs = (int)segs;
  p.B = a->B; p.n = a->n; p.rows = a->rows; p.src_lmax = a->src_lmax; p.kv_lmax = a->kv_lmax; p.V = a->V;
  p.pieces = (long)a->rows * (p.row_bytes / 16);
  p.n_wide = 2L * p.segs * p.pieces;
  p.n_cache = p.n_wide + (kv8 ? 2L * p.segs * a->rows : 0L);
  p.log_wide = a->V % 4 == 0;  // (every logits row then starts 16-byte aligned)
  p.log_per = p.log_wide ? a->V / 4 : a->V;
  p.n_copy = p.n_cache + (long)a->B * p.log_per;
  const long blocks = (p.n_copy + 255) / 256 + a->B;
  TCAVT_CHECK_ARG(blocks <= 0x7fffffffL, "kv_fanout: too many rows");
  p.logits_src = a->logits_src; p.logits_dst = a->logits_dst;
  p.prompt_ids = reinterpret_cast<const long*>(a->prompt_ids); p.kv_len = a->kv_len; p.history = reinterpret_cast<long*>(a->history);
  p.hist_len = a->hist_len; p.pos = a->pos; p.finished = a->finished;
  p.n_ids = a->n_ids; p.hist_cap = a->hist_cap; p.n_image = a->n_image;
  hipLaunchKernelGGL(kv_fanout_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  TCAVT_CHECK_LAUNCH("kv_fanout");
  return TCAVT_OK;
}

extern "C" int tcavt_state_fanout(const tcavt_state_fanout_args* a, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(a, "state_fanout: args is a null pointer");
  const struct { const void* p; const char* name; } ptrs[] = {
      {a->prompt_ids, "prompt_ids"}, {a->kv_len, "kv_len"}, {a->logits_src, "logits_src"}, {a->logits_dst, "logits_dst"},
      {a->history, "history"}, {a->hist_len, "hist_len"}, {a->pos, "pos"}, {a->finished, "finished"}};
  for (const auto& q : ptrs) TCAVT_CHECK_ARG(q.p, "state_fanout: %s is a null pointer", q.name);
  TCAVT_CHECK_ARG(a->B >= 1, "state_fanout: B = %d must be >= 1", a->B);
  TCAVT_CHECK_ARG(a->n >= 1, "state_fanout: n = %d must be >= 1", a->n);
  TCAVT_CHECK_ARG((long)a->B * a->n <= 0x7fffffffL, "state_fanout: B * n = %ld rows are too many", (long)a->B * a->n);
  TCAVT_CHECK_ARG(a->hist_cap > 0 && a->n_ids >= 0 && a->n_ids <= a->hist_cap, "state_fanout: n_ids = %d must be in [0, hist_cap = %d]", a->n_ids,
                  a->hist_cap);
  TCAVT_CHECK_ARG(a->n_image >= 0, "state_fanout: n_image = %d must be >= 0", a->n_image);
  TCAVT_CHECK_ARG(a->V >= 1, "state_fanout: V = %d must be >= 1", a->V);
  TCAVT_CHECK_ARG(aligned16(a->logits_src) && aligned16(a->logits_dst), "state_fanout: logits_src and logits_dst must be 16-byte aligned");
  FanoutP p = {};
  p.B = a->B; p.n = a->n; p.V = a->V;
  p.log_wide = a->V % 4 == 0;  // (every logits row then starts 16-byte aligned)
  p.log_per = p.log_wide ? a->V / 4 : a->V;
  p.n_copy = (long)a->B * p.log_per;
  const long blocks = (p.n_copy + 255) / 256 + a->B;
  TCAVT_CHECK_ARG(blocks <= 0x7fffffffL, "state_fanout: too many rows");
  p.logits_src = a->logits_src; p.logits_dst = a->logits_dst;
  p.prompt_ids = reinterpret_cast<const long*>(a->prompt_ids); p.kv_len = a->kv_len; p.history = reinterpret_cast<long*>(a->history);
  p.hist_len = a->hist_len; p.pos = a->pos; p.finished = a->finished;
  p.n_ids = a->n_ids; p.hist_cap = a->hist_cap; p.n_image = a->n_image;
  hipLaunchKernelGGL(state_fanout_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  TCAVT_CHECK_LAUNCH("state_fanout");
  return TCAVT_OK;
}

// The decode step; px != NULL: the rows read their prompts' cache in place (tcavt_llama_decode_step_shared).
static int decode_step_impl(const tcavt_decode_args* a, const tcavt_kv_prefix* px, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(a && a->layers && a->gamma_final && a->rope_cos && a->rope_sin && a->table && a->txt_mod && a->cur_tok && a->pos &&
                      a->h16 && a->part && a->qkv && a->att && a->act && a->x16 && a->logits && a->bad_id_flag,
                  "llama_decode_step: null pointer");
  // the cache: the 16-bit pair, or the four FP8 planes (tcavt_attn_decode8) -- one of the two
  const bool kv8 = a->kv8_k_codes || a->kv8_k_scales || a->kv8_v_codes || a->kv8_v_scales;
  TCAVT_CHECK_ARG(!kv8 || (a->kv8_k_codes && a->kv8_k_scales && a->kv8_v_codes && a->kv8_v_scales),
                  "llama_decode_step: the four kv8 planes come together");
  TCAVT_CHECK_ARG(!kv8 || (!a->k_cache && !a->v_cache), "llama_decode_step: the kv8 planes and k_cache / v_cache exclude each other");
  TCAVT_CHECK_ARG(kv8 || (a->k_cache && a->v_cache), "llama_decode_step: null pointer (k_cache / v_cache, or the four kv8 planes)");
  // the shared prompt cache (tcavt_attn_decode_shared): k_cache / v_cache then hold the rows' suffixes only
  if (px) {
    TCAVT_CHECK_ARG(!kv8, "llama_decode_step: prefix and the kv8 planes exclude each other");
    TCAVT_CHECK_ARG(px->k && px->v && px->len, "llama_decode_step: prefix: null pointer (k, v, len)");
    TCAVT_CHECK_ARG(px->n >= 1 && px->lmax >= 1, "llama_decode_step: prefix: n = %d and lmax = %d must be >= 1", px->n, px->lmax);
    TCAVT_CHECK_ARG(a->B > 0 && a->B % px->n == 0, "llama_decode_step: prefix: B = %d must be a multiple of n = %d", a->B, px->n);
    TCAVT_CHECK_ARG((long)a->rope_L >= (long)px->lmax + a->kv_lmax, "llama_decode_step: prefix: rope_L = %d must be >= lmax + kv_lmax = %ld",
                    a->rope_L, (long)px->lmax + a->kv_lmax);
    TCAVT_CHECK_ARG(a->kv_lmax <= TCAVT_ATTN_DECODE_SHARED_MAX_SUFFIX,
                    "llama_decode_step: prefix: kv_lmax = %d exceeds TCAVT_ATTN_DECODE_SHARED_MAX_SUFFIX = %d", a->kv_lmax,
                    TCAVT_ATTN_DECODE_SHARED_MAX_SUFFIX);
  }
  TCAVT_CHECK_ARG(a->n_layers > 0 && a->B > 0 && a->H % 256 == 0 && a->I > 0 && a->nq > 0 && a->nkv > 0 && a->nq % a->nkv == 0 &&
                      a->nq / a->nkv <= 8 && a->V > 0 && a->V % 16 == 0 && a->kv_lmax > 0 && a->rope_L >= a->kv_lmax && is16(a->dtype16),
                  "llama_decode_step: bad shape (H %% 256, V %% 16, nq / nkv <= 8, rope_L >= kv_lmax)");
  const int B = a->B, H = a->H, I = a->I, nq = a->nq, nkv = a->nkv, dt = a->dtype16;
  const int nqkv = (nq + 2 * nkv) * 64;
  const int np_in = norm_out_npart(B, H, I), np_post = norm_out_npart(B, H, nq * 64);  // see csrc/stack.hip
  // scaled 16-bit image of the residual stream, as in tcavt_llama_stack_forward (the prefill that filled the cache ran at the same scale
  // or not: keys / values are true-scale either way)
  TCAVT_CHECK_ARG(a->stream_scale >= 0.f && a->stream_scale <= 1.f, "llama_decode_step: stream_scale must be in (0, 1] (0 means 1)");
  const float ss_ = a->stream_scale == 0.f ? 1.f : a->stream_scale;
  const float eps_s = a->rms_eps * ss_ * ss_;
  // fragment-major weight copies (tcavt_pack_weight16): the projections' weight streams read consecutive bytes; or their FP8
  // form (tcavt_pack_weight8): half the bytes
  const int wl = a->w_layout;
  TCAVT_CHECK_ARG(wl == 0 || ((wl == TCAVT_W_FRAG16 || wl == TCAVT_W_FRAG8) && B <= 32 && I % 256 == 0 && (nq * 64) % 256 == 0),
                  "llama_decode_step: w_layout must be 0, TCAVT_W_FRAG16 or TCAVT_W_FRAG8 (B <= 32, I %% 256 == 0, nq * 64 %% 256 == 0)");
  TCAVT_CHECK_ARG(wl != TCAVT_W_FRAG8 || a->table_packed, "llama_decode_step: TCAVT_W_FRAG8 needs table_packed (the tcavt_pack_weight8 copy of table)");
  // fragment-major activations: h16, att, act, x16 in the skinny GEMMs' operand order (16 or 32 whole rows each)
  const int al = a->act_layout;
  TCAVT_CHECK_ARG(al == 0 || ((al == 1 || al == 2) && a->h == nullptr && B <= (al == 2 ? 8 : 32) && I % 256 == 0 && (nq * 64) % 256 == 0),
                  "llama_decode_step: act_layout must be 0, 1 (B <= 32) or 2 (B <= 8) (16-bit residual stream: h == NULL; I %% 256 == 0, "
                  "nq * 64 %% 256 == 0)");
  const int blk8 = al == 2 ? TCAVT_ACT_BLOCK8 : 0;
  const int gA = al ? (TCAVT_ACT_A_FRAG16 | blk8) : 0, gAO = al ? (TCAVT_ACT_A_FRAG16 | TCAVT_ACT_OUT_FRAG16 | blk8) : 0;
  // h = table[cur_tok] + text modality embedding (generated tokens are text tokens: scripts/train.py:526-527); + the fused
  // norm's inputs
  // (a->h == NULL: the residual stream is the 16-bit h16 itself, as in tcavt_llama_stack_forward)
  TCAVT_TRY(embed_fuse_impl(a->table, a->cur_tok, a->txt_mod /* unused: Nq = 0 */, a->txt_mod, a->txt_mod, a->h, B, 0, 1, H, a->V,
                            a->bad_id_flag, dt, a->h16, a->part, np_in, ss_, al, stream));
  const size_t per_layer = (size_t)B * a->kv_lmax * nkv * 64;
  {
    int KS;
    size_t lds;
    TCAVT_CHECK_ARG(attn_decode_rule(a->kv_lmax, &KS, &lds), "llama_decode_step: kv_lmax = %d too long for the decode attention's score buffer",
                    a->kv_lmax);
  }
  for (int li = 0; li < a->n_layers; ++li) {
    const tcavt_llama_layer& w = a->layers[li];
    TCAVT_CHECK_ARG(w.w_qkv && w.w_o && w.w_gu && w.w_d && (!w.a_cat || (w.b_ext && a->t)), "llama_decode_step: layer %d: null weight", li);
    // LoRA down-projection: a launch of its own for layer 0 (and without a->lora_part); layers 1.. read the partial sums the
    // previous layer's down-projection GEMM wrote next to its residual epilogue
    // (a q|k|v workgroup reads the partial sums of its own tokens: all B for B <= 16, its 16-token block beyond)
    const bool lp_ok = a->lora_part && a->lora_rank > 0 && a->lora_rank <= 8 && B <= 32;
    const bool t_fused = lp_ok && li > 0 && w.a_cat && a->layers[li - 1].w_d;
    if (w.a_cat && !t_fused) {
      tcavt_gemm_args g = {};
      g.A = a->h16; g.lda = H; g.W = w.a_cat; g.ldw = H; g.C = a->t; g.ldc = 64; g.M = B; g.N = 64; g.K = H; g.act_layout = gA;
      g.out_dtype = dt; g.in_dtype = dt; g.acc_scale = a->lora_scale;  // (t is at the stream's scale, like the main term of the accumulator)
      g.splitk_ws = a->splitk_ws; g.splitk_ws_bytes = a->splitk_ws_bytes;
      TCAVT_TRY(tcavt_gemm_bf16(&g, stream));
    }
    {
      tcavt_gemm_args g = {};
      g.A = a->h16; g.lda = H; g.W = w.w_qkv; g.ldw = H; g.C = a->qkv; g.ldc = nqkv; g.w_layout = wl; g.act_layout = gA;
      g.M = B; g.N = nqkv; g.K = H; g.out_dtype = dt; g.in_dtype = dt;
      if (t_fused) {
        g.W2 = w.b_ext; g.ldw2 = 64; g.lora_part = a->lora_part; g.lora_part_np = H / 16; g.lora_part_scale = a->lora_scale;
      } else if (w.a_cat) { g.A2 = a->t; g.lda2 = 64; g.W2 = w.b_ext; g.ldw2 = 64; g.K2 = 64; }
      g.epilogue = TCAVT_EPI_ROPE | TCAVT_EPI_ROWSCALE;
      g.rope_cos = a->rope_cos; g.rope_sin = a->rope_sin; g.rope_L = a->rope_L; g.rope_cols = (nq + nkv) * 64;
      g.rope_pos = a->pos;
      g.rowscale_part = a->part; g.rowscale_npart = np_in; g.rowscale_h = H; g.rowscale_eps = eps_s;
      g.splitk_ws = a->splitk_ws; g.splitk_ws_bytes = a->splitk_ws_bytes;
      TCAVT_TRY(tcavt_gemm_bf16(&g, stream));
    }
    // (the new token's k / v rows are appended to the cache by the attention kernel itself)
    if (kv8) {
      const size_t rows = (size_t)li * B * nkv * a->kv_lmax;  // cached rows in front of this layer's planes
      TCAVT_TRY(tcavt_attn_decode8(a->qkv, static_cast<unsigned char*>(a->kv8_k_codes) + rows * 64, static_cast<unsigned char*>(a->kv8_k_scales) + rows * 2,
                                   static_cast<unsigned char*>(a->kv8_v_codes) + rows * 64, static_cast<unsigned char*>(a->kv8_v_scales) + rows * 2,
                                   a->pos, a->att, B, nq, nkv, a->kv_lmax, 0.125f, dt, al, stream));
    } else if (px) {
      const size_t pre_layer = (size_t)(B / px->n) * px->lmax * nkv * 64;
      TCAVT_TRY(tcavt_attn_decode_shared(a->qkv, static_cast<const bf16_t*>(px->k) + li * pre_layer, static_cast<const bf16_t*>(px->v) + li * pre_layer,
                                         px->len, static_cast<bf16_t*>(a->k_cache) + li * per_layer, static_cast<bf16_t*>(a->v_cache) + li * per_layer,
                                         a->pos, a->att, B / px->n, px->n, nq, nkv, px->lmax, a->kv_lmax, 0.125f, dt, al, stream));
    } else {
      bf16_t* kc = static_cast<bf16_t*>(a->k_cache) + li * per_layer;
      bf16_t* vc = static_cast<bf16_t*>(a->v_cache) + li * per_layer;
      TCAVT_TRY(tcavt_attn_decode(a->qkv, kc, vc, a->pos, a->att, B, nq, nkv, a->kv_lmax, 0.125f, dt, al, stream));
    }
    {
      tcavt_gemm_args g = {};
      g.A = a->att; g.lda = nq * 64; g.W = w.w_o; g.ldw = nq * 64; g.C = a->h; g.ldc = H; g.w_layout = wl; g.act_layout = gAO;
      g.M = B; g.N = H; g.K = nq * 64; g.out_dtype = TCAVT_F32; g.in_dtype = dt;
      g.residual = a->h; g.ldr = H; g.epilogue = TCAVT_EPI_RESIDUAL | TCAVT_EPI_NORM_OUT;
      g.norm_h16 = a->h16; g.norm_part = a->part; g.norm_scale = ss_;
      g.nonfinite_flag = a->nonfinite_flag; g.nonfinite_tag = 1 + 2 * li;
      g.splitk_ws = a->splitk_ws; g.splitk_ws_bytes = a->splitk_ws_bytes;
      TCAVT_TRY(tcavt_gemm_bf16(&g, stream));
    }
    {
      tcavt_gemm_args g = {};
      g.A = a->h16; g.lda = H; g.W = w.w_gu; g.ldw = H; g.C = a->act; g.ldc = I; g.w_layout = wl; g.act_layout = gAO;
      g.M = B; g.N = 2 * I; g.K = H; g.out_dtype = dt; g.in_dtype = dt;
      g.epilogue = TCAVT_EPI_SILU_MUL | TCAVT_EPI_ROWSCALE;
      g.rowscale_part = a->part; g.rowscale_npart = np_post; g.rowscale_h = H; g.rowscale_eps = eps_s;
      g.splitk_ws = a->splitk_ws; g.splitk_ws_bytes = a->splitk_ws_bytes;
      TCAVT_TRY(tcavt_gemm_bf16(&g, stream));
    }
    {
      tcavt_gemm_args g = {};
      g.A = a->act; g.lda = I; g.W = w.w_d; g.ldw = I; g.C = a->h; g.ldc = H; g.w_layout = wl; g.act_layout = gAO;
      g.M = B; g.N = H; g.K = I; g.out_dtype = TCAVT_F32; g.in_dtype = dt;
      g.residual = a->h; g.ldr = H; g.epilogue = TCAVT_EPI_RESIDUAL | TCAVT_EPI_NORM_OUT;
      g.norm_h16 = a->h16; g.norm_part = a->part; g.norm_scale = ss_;
      g.nonfinite_flag = a->nonfinite_flag; g.nonfinite_tag = 2 + 2 * li;
      if (lp_ok && li + 1 < a->n_layers && a->layers[li + 1].a_cat) {
        g.lora_part = a->lora_part; g.lora_part_a = a->layers[li + 1].a_cat; g.lora_part_lda = H;
      }
      g.splitk_ws = a->splitk_ws; g.splitk_ws_bytes = a->splitk_ws_bytes;
      TCAVT_TRY(tcavt_gemm_bf16(&g, stream));
    }
  }
  if (a->h == nullptr) TCAVT_TRY(rmsnorm16_impl(a->h16, a->gamma_final, eps_s, a->x16, nullptr, B, H, dt, al, stream));
  else TCAVT_TRY(tcavt_rmsnorm(a->h, a->gamma_final, a->rms_eps, a->x16, nullptr, B, H, nullptr, 0.f, 0, 0, dt, stream));
  // lm_head: tied to the embedding table (Llama-3.2-1B: tie_word_embeddings)
  tcavt_gemm_args g = {};
  g.A = a->x16; g.lda = H; g.W = a->table; g.ldw = H; g.C = a->logits; g.ldc = a->V;
  if (a->table_packed && B <= 32) { g.W = a->table_packed; g.w_layout = wl == TCAVT_W_FRAG8 ? TCAVT_W_FRAG8 : TCAVT_W_FRAG16; }
  g.act_layout = gA;
  g.M = B; g.N = a->V; g.K = H; g.out_dtype = TCAVT_F32; g.in_dtype = dt;
  g.splitk_ws = a->splitk_ws; g.splitk_ws_bytes = a->splitk_ws_bytes;
  return tcavt_gemm_bf16(&g, stream);
}

extern "C" int tcavt_llama_decode_step(const tcavt_decode_args* a, tcavt_stream_t stream) { return decode_step_impl(a, nullptr, stream); }

extern "C" int tcavt_llama_decode_step_shared(const tcavt_decode_args* a, const tcavt_kv_prefix* prefix, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(prefix, "llama_decode_step_shared: prefix is a null pointer");
  return decode_step_impl(a, prefix, stream);
}
