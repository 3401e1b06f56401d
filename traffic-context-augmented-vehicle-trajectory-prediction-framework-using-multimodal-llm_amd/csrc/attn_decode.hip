// Decode attention of text generation (include/tcavt.h: tcavt_attn_decode, tcavt_attn_decode_multi, tcavt_kv_store8,
// tcavt_attn_decode8): the one new query of every sample over its cached keys -- or, in the multi form, T consecutive new queries of
// every sequence --, on the 16-bit cache or on the opt-in FP8 cache ("KV8"), and the KV8 store of a prefill.  The decode step
// (csrc/generate.hip) calls these once per layer; the shared-prefix form is csrc/attn_decode_shared.hip.
#include "common.hpp"

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
// MULTI (tcavt_attn_decode_multi): T queries per sequence, row b = s * T + j of qkv on the cache of sequence s = b / T.  With
// base = pos[s * T], query j attends the cached keys 0 .. base - 1 and the new keys 0 .. j of its sequence, which it takes from the
// qkv rows s * T .. s * T + j where the plain form takes its one new key from row b; its own k | v go to cache row base + j.  The
// key count n = base + j + 1 fixes the splits, so the arithmetic of a query is the plain form's at pos = base + j, bit for bit.  A
// workgroup reads cache rows < base only and writes row base + j only: the workgroups of a launch need no order among themselves.
template <bool F16, bool PFV, bool MULTI = false>
__global__ __launch_bounds__(1024) void attn_decode_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ kc,
                                                           bf16_t* __restrict__ vc, const int* __restrict__ pos,
                                                           bf16_t* __restrict__ out, int lmax, int nq, int nkv, float scale,
                                                           int KS, int out_frag, int T) {
  extern __shared__ float sc[];  // [lmax] scores | [KS][2] (max, sum) | [KS][64] partial outputs
  const int group = nq / nkv;
  const int b = blockIdx.x / nq, head = blockIdx.x % nq, kvh = head / group;
  const int lane = threadIdx.x & 63, ks = threadIdx.x >> 6;
  const int g = lane >> 3, c = lane & 7;
  const int cb = MULTI ? b / T : b;  // whose cache
  // MULTI: the first position whose key comes from qkv (clamped into the cache: the caller keeps base + T <= lmax)
  const int base = MULTI ? min(max(pos[cb * T], 0), lmax - 1) : 0;
  const int n = MULTI ? min(base + (b - cb * T) + 1, lmax) : min(pos[b] + 1, lmax);
  const int ld = (nq + 2 * nkv) * 64, w = nkv * 64;
  const bf16_t* kb = kc + (long)cb * lmax * w + kvh * 64;
  const bf16_t* vb = vc + (long)cb * lmax * w + kvh * 64;
  const int jn = n - 1;  // the new token's position
  const bf16_t* knew = qkv + (long)b * ld + (nq + kvh) * 64;
  const bf16_t* vnew = qkv + (long)b * ld + (nq + nkv + kvh) * 64;
  if (head % group == 0 && ks == 0 && lane < 16) {  // append: 8 lanes x 16 bytes of k, 8 of v
    const int cc = (lane & 7) * 8;
    if (lane < 8) *reinterpret_cast<u32x4*>(kc + ((long)cb * lmax + jn) * w + kvh * 64 + cc) = *reinterpret_cast<const u32x4*>(knew + cc);
    else *reinterpret_cast<u32x4*>(vc + ((long)cb * lmax + jn) * w + kvh * 64 + cc) = *reinterpret_cast<const u32x4*>(vnew + cc);
  }
  // key / value row j <= jn: the plain form has one new row, MULTI the rows base .. jn of the sequence's qkv block (j - base <= b - cb * T)
  auto krow = [&](int j) -> const bf16_t* {
    if constexpr (MULTI) return j >= base ? qkv + ((long)cb * T + (j - base)) * ld + (nq + kvh) * 64 : kb + (long)j * w;
    else return j == jn ? knew : kb + (long)j * w;
  };
  auto vrow = [&](int j) -> const bf16_t* {
    if constexpr (MULTI) return j >= base ? qkv + ((long)cb * T + (j - base)) * ld + (nq + nkv + kvh) * 64 : vb + (long)j * w;
    else return j == jn ? vnew : vb + (long)j * w;
  };
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
      kr[i] = *reinterpret_cast<const u32x4*>(krow(j) + c * 8);
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
      vr0[i] = *reinterpret_cast<const u32x4*>(vrow(j) + c * 8);
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
        vr[i] = *reinterpret_cast<const u32x4*>(vrow(j) + c * 8);
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

// The decode attention's host rule: KS key splits (waves) per query head -- one 64-key round each up to 1024 keys, two beyond --
// and the LDS bytes of [kv_lmax] scores | [KS][2] (max, sum) | [KS][64] partial outputs.  false: the scores do not fit 64 KiB.
bool attn_decode_rule(int kv_lmax, int* KS, size_t* lds) {
  *KS = std::min(16, (kv_lmax + 63) / 64);
  *lds = ((size_t)kv_lmax + (size_t)*KS * 66) * sizeof(float);
  return *lds <= 64 * 1024;
}

}  // namespace tcavt

using namespace tcavt;

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
                     KS, out_layout, 1);
  TCAVT_CHECK_LAUNCH("attn_decode");
  return TCAVT_OK;
}

// T queries per sequence on one cache per sequence (the verify step of prompt-lookup decoding): the plain launch with R = S * T rows
// in the place of B; T = 1 is tcavt_attn_decode itself.
extern "C" int tcavt_attn_decode_multi(const void* qkv, void* k_cache, void* v_cache, const int32_t* pos_rows, void* out, int S, int T,
                                       int nq, int nkv, int kv_lmax, float scale, int dtype16, int out_layout, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(qkv && k_cache && v_cache && pos_rows && out, "attn_decode_multi: null pointer");
  TCAVT_CHECK_ARG(is16(dtype16), "attn_decode_multi: dtype16 must be TCAVT_F16 or TCAVT_BF16");
  TCAVT_CHECK_ARG(S > 0 && nq > 0 && nkv > 0 && nq % nkv == 0 && nq / nkv <= 8, "attn_decode_multi: bad shape (S, nq, nkv > 0, nq %% nkv == 0, nq / nkv <= 8)");
  TCAVT_CHECK_ARG(T >= 1 && T <= kv_lmax, "attn_decode_multi: T = %d must be in [1, kv_lmax = %d]", T, kv_lmax);
  TCAVT_CHECK_ARG((long)S * T * nq <= 0x7fffffffL, "attn_decode_multi: S * T * nq too large");
  TCAVT_CHECK_ARG(kv_lmax >= 1, "attn_decode_multi: kv_lmax must be >= 1");
  int KS;
  size_t lds;
  TCAVT_CHECK_ARG(attn_decode_rule(kv_lmax, &KS, &lds), "attn_decode_multi: kv_lmax = %d too long for the score buffer", kv_lmax);
  const int R = S * T;
  TCAVT_CHECK_ARG(out_layout == 0 || (out_layout == 1 && R <= 32 && (nq * 64) % 256 == 0) || (out_layout == 2 && R <= 8),
                  "attn_decode_multi: out_layout must be 0, 1 (S * T <= 32, nq * 64 %% 256 == 0) or 2 (S * T <= 8)");
  TCAVT_CHECK_ARG(aligned16(qkv) && aligned16(k_cache) && aligned16(v_cache), "attn_decode_multi: qkv and the caches must be 16-byte aligned");
  if (T == 1) return tcavt_attn_decode(qkv, k_cache, v_cache, pos_rows, out, S, nq, nkv, kv_lmax, scale, dtype16, out_layout, stream);
  const bool pfv = R * nq <= 512;  // (tcavt_attn_decode's rule)
  auto kfn = dtype16 == TCAVT_F16 ? (pfv ? attn_decode_kernel<true, true, true> : attn_decode_kernel<true, false, true>)
                                  : (pfv ? attn_decode_kernel<false, true, true> : attn_decode_kernel<false, false, true>);
  hipLaunchKernelGGL(kfn, dim3(R * nq), dim3(KS * 64), lds, static_cast<hipStream_t>(stream), static_cast<const bf16_t*>(qkv),
                     static_cast<bf16_t*>(k_cache), static_cast<bf16_t*>(v_cache), pos_rows, static_cast<bf16_t*>(out), kv_lmax, nq, nkv,
                     scale, KS, out_layout, T);
  TCAVT_CHECK_LAUNCH("attn_decode_multi");
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
