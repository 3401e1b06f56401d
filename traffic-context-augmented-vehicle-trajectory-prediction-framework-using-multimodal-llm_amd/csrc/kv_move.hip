// The cache movers of text generation (include/tcavt.h: tcavt_slot_admit, tcavt_slot_admit_group, tcavt_kv_fanout,
// tcavt_state_fanout): a prefilled cache moves into the slots or rows of a decode batch and their bookkeeping is reset, in one launch.
// The three copying kernels cut the cache the same way (CacheCut) and differ in where a segment's rows start on either side and in
// how often a piece is stored.
#include "common.hpp"

namespace tcavt {

// Both cache forms are segments of consecutive rows on either side -- 16-bit: a layer of the k or v cache, rows of nkv * 128 bytes;
// KV8: a (layer, kv head) of a plane, rows of 64 code bytes or 2 scale bytes -- so a thread copies one 16-byte piece of a segment (or
// one row's two scale bytes).  Segment sg = o * inner + i, i < inner; o is the layer (the admissions: of one sample) or
// layer * B + b (tcavt_kv_fanout); on which rows a segment starts is each kernel's own.  Filled by cache_cut below for every entry.
struct CacheCut {
  const unsigned char* src[4];  // 16-bit: k, v; KV8: k codes, v codes, k scales, v scales
  unsigned char* dst[4];
  long pieces;  // 16-byte pieces of a segment: rows * row_bytes / 16
  long n_wide;  // threads that copy a 16-byte piece: 2 * segs * pieces; behind them (KV8) 2 * segs * rows copy a scale pair
  long n_copy;
  int segs, inner, rows, src_lmax, kv_lmax, row_bytes;
};

// Copying thread i < n_copy: unit e (a 16-byte piece if wide, else a row's scale pair) of segment sg of plane kv (k or v)
struct CutAt {
  int kv;
  long sg, e;
  bool wide;
};

__device__ __forceinline__ CutAt cut_at(const CacheCut& c, long i) {
  CutAt t;
  t.wide = i < c.n_wide;
  const long j = t.wide ? i : i - c.n_wide;
  const long per = t.wide ? c.pieces : (long)c.rows;  // units of a segment
  const long per_plane = c.segs * per;
  t.kv = (int)(j / per_plane);
  const long r = j - t.kv * per_plane;
  t.sg = r / per;
  t.e = r - t.sg * per;
  return t;
}

// Unit t of a segment that starts at row srow of the source: loaded once, stored n times, at row drow of the destination and every
// dstep rows on.  Consecutive lanes hold consecutive units on both sides.
__device__ __forceinline__ void cut_copy(const CacheCut& c, const CutAt& t, long srow, long drow, int n, long dstep) {
  if (t.wide) {
    const u32x4 v = reinterpret_cast<const u32x4*>(c.src[t.kv] + srow * c.row_bytes)[t.e];
    u32x4* d = reinterpret_cast<u32x4*>(c.dst[t.kv] + drow * c.row_bytes) + t.e;
    const long step = dstep * c.row_bytes / 16;
    for (int j = 0; j < n; ++j) d[j * step] = v;
  } else {
    const unsigned short v = reinterpret_cast<const unsigned short*>(c.src[2 + t.kv] + srow * 2)[t.e];
    unsigned short* d = reinterpret_cast<unsigned short*>(c.dst[2 + t.kv] + drow * 2) + t.e;
    for (int j = 0; j < n; ++j) d[j * dstep] = v;
  }
}

// The state of a freshly admitted slot, by one workgroup (cur_tok is the sampler's), from row g of the prefill: its prompt ids and
// kv_len, and its budget and output row -- values in the launch parameters (tcavt_slot_admit) or device arrays over the rows.
__device__ __forceinline__ int of_row(int v, int) { return v; }
__device__ __forceinline__ long of_row(long v, int) { return v; }
__device__ __forceinline__ int of_row(const int* v, int g) { return v[g]; }
__device__ __forceinline__ long of_row(const long* v, int g) { return v[g]; }

template <class P>
__device__ __forceinline__ void slot_reset(const P& a, int slot, int g) {
  long* h = a.history + (long)slot * a.hist_cap;
  const long* ids = a.prompt_ids + (long)g * a.n_ids;
  for (int i = threadIdx.x; i < a.n_ids; i += 256) h[i] = ids[i];
  if (threadIdx.x == 0) {
    const int kl = a.kv_len[g];
    a.hist_len[slot] = kl - a.n_image;
    a.pos[slot] = kl;
    a.step[slot] = 0;
    a.finished[slot] = 0;
    a.max_new[slot] = of_row(a.max_new_value, g);
    a.out_row[slot] = of_row(a.out_row_value, g);
  }
}

// tcavt_slot_admit: a freshly prefilled request (a one-sample cache) moves into slot `slot` of an S-slot cache and the slot's
// bookkeeping is reset, in one launch: one more workgroup behind the copying ones writes the slot's state.  Segment sg = (layer,
// i < inner) of the cut starts at row sg * src_lmax of the source and at row ((layer * S + slot) * inner + i) * kv_lmax of the
// destination.
struct AdmitP {
  CacheCut c;
  int S, slot;
  const long* prompt_ids;
  const int* kv_len;
  long* history;
  int *hist_len, *step, *max_new, *pos, *finished;
  long* out_row;
  long out_row_value;
  int n_ids, hist_cap, n_image, max_new_value;
};

__global__ __launch_bounds__(256) void slot_admit_kernel(AdmitP a) {
  if (blockIdx.x == gridDim.x - 1) {
    slot_reset(a, a.slot, 0);
    return;
  }
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.c.n_copy) return;
  const CutAt t = cut_at(a.c, i);
  const long srow = t.sg * a.c.src_lmax, drow = ((t.sg / a.c.inner * a.S + a.slot) * a.c.inner + t.sg % a.c.inner) * a.c.kv_lmax;
  cut_copy(a.c, t, srow, drow, 1, 0);
}

// tcavt_slot_admit_group: slot_admit_kernel for the G samples of a grouped prefill, blockIdx.y = the group's row.  The source is a
// G-sample cache, so segment (layer, i < inner) of row g starts at source row ((layer * G + g) * inner + i) * src_lmax; the slot, the
// kv_len, the budget and the output row of a row are read from DEVICE arrays (the launch is the same for every group: capturable).
// slot[g] < 0: a pad row, its workgroups leave at once; slot[g] >= S: nothing is written but the flag.  Every index below is
// bounded by the host-checked shape once 0 <= slot < S holds.
struct AdmitGroupP {
  CacheCut c;  // per row of the group
  int S, G;
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
  if (blockIdx.x == gridDim.x - 1) {
    slot_reset(a, slot, g);
    return;
  }
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.c.n_copy) return;
  const CutAt t = cut_at(a.c, i);
  const long layer = t.sg / a.c.inner, in = t.sg % a.c.inner;
  const long srow = ((layer * a.G + g) * a.c.inner + in) * a.c.src_lmax, drow = ((layer * a.S + slot) * a.c.inner + in) * a.c.kv_lmax;
  cut_copy(a.c, t, srow, drow, 1, 0);
}

// tcavt_kv_fanout: a B-sample prefill becomes the state of a decode batch of B * n rows, in one launch.  Source segment
// sg = (layer * B + b) * inner + i of the cut starts at source row sg * src_lmax, and destination sample b * n + j of a layer is
// sample (layer * B + b) * n + j of the whole destination, so copy j of the segment starts at row
// (((sg / inner) * n + j) * inner + sg % inner) * kv_lmax.  A thread LOADS its piece (of the cache, or one 16- or 4-byte piece of a
// logits row) once and STORES it n times from registers: the n stores of a wave are n runs of up to 1 KiB.  Behind the copying
// workgroups, workgroup b of the last B writes the state of rows b * n .. b * n + n - 1 (each prompt id read once, stored n times).
struct FanoutP {
  CacheCut c;  // (tcavt_state_fanout: zero, no cache to copy)
  int B, n;
  long n_all;    // copying threads: c.n_copy for the cache, and behind those B * log_per copy a piece of a logits row
  long log_per;  // pieces of a logits row: V / 4 of 16 bytes (log_wide), or V of 4 bytes
  int log_wide, V;
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
  const long first_state = (long)gridDim.x - a.B;
  if (blockIdx.x >= first_state) {
    fanout_state(a, (int)(blockIdx.x - first_state));
    return;
  }
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_all) return;
  if (i >= a.c.n_copy) {
    fanout_logits(a, i - a.c.n_copy);
    return;
  }
  const CutAt t = cut_at(a.c, i);
  const long sample = t.sg / a.c.inner, in = t.sg - sample * a.c.inner;  // sample = layer * B + b
  cut_copy(a.c, t, t.sg * a.c.src_lmax, (sample * a.n * a.c.inner + in) * a.c.kv_lmax, a.n, (long)a.c.inner * a.c.kv_lmax);
}

// tcavt_state_fanout: kv_fanout_kernel without a cache to copy (c.n_copy = 0) -- the logits pieces, and behind them the B state workgroups.
__global__ __launch_bounds__(256) void state_fanout_kernel(FanoutP a) {
  const long first_state = (long)gridDim.x - a.B;
  if (blockIdx.x >= first_state) {
    fanout_state(a, (int)(blockIdx.x - first_state));
    return;
  }
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < a.n_all) fanout_logits(a, i);
}

}  // namespace tcavt

using namespace tcavt;

#define TCAVT_TRY(call)              \
  do {                               \
    const int rc_ = (call);          \
    if (rc_ != TCAVT_OK) return rc_; \
  } while (0)

// The cache form of an entry's args, first of its checks: the 16-bit pair or the eight KV8 planes, each whole, and not both.
template <class A>
static int cache_form(const char* who, const A* a, bool* is_kv8) {
  const bool f16 = a->src_k || a->src_v || a->dst_k || a->dst_v;
  const bool kv8 = a->src_k_codes || a->src_k_scales || a->src_v_codes || a->src_v_scales || a->dst_k_codes || a->dst_k_scales ||
                   a->dst_v_codes || a->dst_v_scales;
  TCAVT_CHECK_ARG(!(f16 && kv8), "%s: the 16-bit caches (src_k .. dst_v) and the kv8 planes exclude each other", who);
  TCAVT_CHECK_ARG(f16 || kv8, "%s: null pointer (src_k / src_v / dst_k / dst_v, or the eight kv8 planes)", who);
  TCAVT_CHECK_ARG(!f16 || (a->src_k && a->src_v && a->dst_k && a->dst_v), "%s: null pointer: src_k, src_v, dst_k and dst_v come together", who);
  TCAVT_CHECK_ARG(!kv8 || (a->src_k_codes && a->src_k_scales && a->src_v_codes && a->src_v_scales && a->dst_k_codes && a->dst_k_scales &&
                           a->dst_v_codes && a->dst_v_scales),
                  "%s: null pointer: the eight kv8 planes come together", who);
  *is_kv8 = kv8;
  return TCAVT_OK;
}

// ... and the cut of that form, last of its checks: `outer` segments per plane and `inner` (n_layers, times the samples of a batched
// source).  The rows and lmax of the args are checked by then; product: the entry refuses outer * inner > INT_MAX under this name.
template <class A>
static int cache_cut(const char* who, const A* a, bool kv8, long outer, const char* product, CacheCut* c) {
  if (kv8) {
    TCAVT_CHECK_ARG(aligned16(a->src_k_codes) && aligned16(a->src_v_codes) && aligned16(a->dst_k_codes) && aligned16(a->dst_v_codes),
                    "%s: the code planes must be 16-byte aligned", who);
    TCAVT_CHECK_ARG(((reinterpret_cast<uintptr_t>(a->src_k_scales) | reinterpret_cast<uintptr_t>(a->src_v_scales) |
                      reinterpret_cast<uintptr_t>(a->dst_k_scales) | reinterpret_cast<uintptr_t>(a->dst_v_scales)) & 1) == 0,
                    "%s: the scale planes must be 2-byte aligned", who);
    const void* src[4] = {a->src_k_codes, a->src_v_codes, a->src_k_scales, a->src_v_scales};
    void* dst[4] = {a->dst_k_codes, a->dst_v_codes, a->dst_k_scales, a->dst_v_scales};
    for (int i = 0; i < 4; ++i) { c->src[i] = static_cast<const unsigned char*>(src[i]); c->dst[i] = static_cast<unsigned char*>(dst[i]); }
    c->inner = a->nkv; c->row_bytes = 64;
  } else {
    TCAVT_CHECK_ARG(aligned16(a->src_k) && aligned16(a->src_v) && aligned16(a->dst_k) && aligned16(a->dst_v),
                    "%s: the caches must be 16-byte aligned", who);
    c->src[0] = static_cast<const unsigned char*>(a->src_k); c->src[1] = static_cast<const unsigned char*>(a->src_v);
    c->dst[0] = static_cast<unsigned char*>(a->dst_k); c->dst[1] = static_cast<unsigned char*>(a->dst_v);
    c->inner = 1; c->row_bytes = a->nkv * 128;
  }
  const long segs = outer * c->inner;
  TCAVT_CHECK_ARG(!product || segs <= 0x7fffffffL, "%s: %s is too large", who, product);
  c->segs = (int)segs;
  c->rows = a->rows; c->src_lmax = a->src_lmax; c->kv_lmax = a->kv_lmax;
  c->pieces = (long)a->rows * (c->row_bytes / 16);
  c->n_wide = 2L * c->segs * c->pieces;
  c->n_copy = c->n_wide + (kv8 ? 2L * c->segs * a->rows : 0L);
  return TCAVT_OK;
}

extern "C" int tcavt_slot_admit(const tcavt_slot_admit_args* a, tcavt_stream_t stream) {
  TCAVT_CHECK_ARG(a, "slot_admit: args is a null pointer");
  bool kv8;
  TCAVT_TRY(cache_form("slot_admit", a, &kv8));
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
  TCAVT_TRY(cache_cut("slot_admit", a, kv8, a->n_layers, nullptr, &p.c));
  p.S = a->S; p.slot = a->slot;
  const long blocks = (p.c.n_copy + 255) / 256 + 1;
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
  bool kv8;
  TCAVT_TRY(cache_form("slot_admit_group", a, &kv8));
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
  TCAVT_TRY(cache_cut("slot_admit_group", a, kv8, a->n_layers, nullptr, &p.c));
  p.S = a->S; p.G = a->G;
  const long blocks = (p.c.n_copy + 255) / 256 + 1;
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
  bool kv8;
  TCAVT_TRY(cache_form("kv_fanout", a, &kv8));
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
  TCAVT_TRY(cache_cut("kv_fanout", a, kv8, (long)a->n_layers * a->B, "n_layers * B * nkv", &p.c));
  p.B = a->B; p.n = a->n; p.V = a->V;
  p.log_wide = a->V % 4 == 0;  // (every logits row then starts 16-byte aligned)
  p.log_per = p.log_wide ? a->V / 4 : a->V;
  p.n_all = p.c.n_copy + (long)a->B * p.log_per;
  const long blocks = (p.n_all + 255) / 256 + a->B;
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
  p.n_all = (long)a->B * p.log_per;
  const long blocks = (p.n_all + 255) / 256 + a->B;
  TCAVT_CHECK_ARG(blocks <= 0x7fffffffL, "state_fanout: too many rows");
  p.logits_src = a->logits_src; p.logits_dst = a->logits_dst;
  p.prompt_ids = reinterpret_cast<const long*>(a->prompt_ids); p.kv_len = a->kv_len; p.history = reinterpret_cast<long*>(a->history);
  p.hist_len = a->hist_len; p.pos = a->pos; p.finished = a->finished;
  p.n_ids = a->n_ids; p.hist_cap = a->hist_cap; p.n_image = a->n_image;
  hipLaunchKernelGGL(state_fanout_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), p);
  TCAVT_CHECK_LAUNCH("state_fanout");
  return TCAVT_OK;
}
