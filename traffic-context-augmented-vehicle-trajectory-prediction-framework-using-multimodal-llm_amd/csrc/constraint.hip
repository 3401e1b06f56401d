// Token-automaton constrained decoding (tcavt_constraint_build / _mask / _advance, include/tcavt.h).
//
// A constraint is a deterministic automaton over token ids, stored by token class: token_class int32 [V] and trans int32
// [n_states][n_classes] (-1: the class is not allowed in the state).  The sampler treats a score of -inf as banned on every path,
// so the constraint is two launches around ONE call of any token-selection entry, on the same logits and state:
//
//   build    once per call of a generate entry: one workgroup per state makes the state's allowed-token bitmap (bit id & 31 of
//            word id >> 5, the bit order of the stop-set bitmap) and the number of allowed tokens.
//   mask     before the selection, rows x 16 workgroups: a live row's state is start[request] when its step word is 0, else
//            state[slot]; a state that allows every token returns after that; otherwise a thread takes groups of 4 ids -- one
//            16-byte piece of the row, whose 4 bits lie in one bitmap word -- and stores -inf over the ids that are not allowed.
//            A group that is allowed entirely is neither read nor written, one that is banned entirely is written without a
//            read.  The [V] class array is never read here: a row costs its own bytes plus V / 8 bytes of bitmap.
//            What cannot be known after the selection -- that the row was live, its slot, its state, its request -- goes to the
//            workspace.
//   advance  after the selection, one thread per row: state <- trans[state][token_class[cur_tok]] for the rows that were live;
//            a token that is not allowed leaves the state and sets bit 0 of the flag word.
//
// Nothing is sized by a device value, no host memory is read, every store is a plain vector store: all three are capturable.
#include "common.hpp"

namespace tcavt {

constexpr int CS_G = 16;          // mask workgroups per row (the slice count of the sampler and of the log-probabilities)
constexpr int CS_T = 256;         // threads per workgroup, all three kernels
constexpr int CS_META = 4;        // int32 per logits row: live, slot, state, request
constexpr int CS_MAX_STATES = 4096, CS_MAX_CLASSES = 4096;
constexpr int CS_FLAG_TOKEN = 1, CS_FLAG_REQUEST = 2, CS_FLAG_STATE = 4;

struct ConstraintP {
  const int* token_class;
  const int* trans;
  unsigned int* bitmap;
  int* count;
  float* logits;
  const int* slot_of_row;
  const int* step;
  const long* out_row;
  const int* finished;
  const long* cur_tok;
  int* state;
  const int* start;
  int* request_state;
  int* flag;
  int* meta;  // [rows][CS_META]
  int V, W, n_states, n_classes, rows, n_state, n_req;
};

// the next state of `st` on class `c`, or -1: a class or a target outside its range is "not allowed", never an address
__device__ __forceinline__ int next_state(const ConstraintP& a, int st, int c) {
  if (c < 0 || c >= a.n_classes) return -1;
  const int ns = a.trans[(long)st * a.n_classes + c];
  return (ns >= 0 && ns < a.n_states) ? ns : -1;
}

// one workgroup per state: the bitmap row and the count.  A thread makes whole words; the 32 classes of a word are eight
// 16-byte loads where the word lies inside V.
__global__ __launch_bounds__(CS_T) void constraint_build_kernel(ConstraintP a) {
  __shared__ int red[CS_T / 64];
  const int st = blockIdx.x, tid = threadIdx.x;
  unsigned int* row = a.bitmap + (long)st * a.W;
  int n = 0;
  for (int w = tid; w < a.W; w += CS_T) {
    const int base = w << 5;
    unsigned int bits = 0u;
    if (base + 32 <= a.V) {
      const int4* c4 = reinterpret_cast<const int4*>(a.token_class + base);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int4 c = c4[j];
        bits |= (next_state(a, st, c.x) >= 0 ? 1u : 0u) << (4 * j);
        bits |= (next_state(a, st, c.y) >= 0 ? 1u : 0u) << (4 * j + 1);
        bits |= (next_state(a, st, c.z) >= 0 ? 1u : 0u) << (4 * j + 2);
        bits |= (next_state(a, st, c.w) >= 0 ? 1u : 0u) << (4 * j + 3);
      }
    } else {
      for (int j = 0; j < 32 && base + j < a.V; ++j)  // the tail word: bits at or beyond V stay 0
        bits |= (next_state(a, st, a.token_class[base + j]) >= 0 ? 1u : 0u) << j;
    }
    row[w] = bits;
    n += __popc(bits);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = n;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < CS_T / 64; ++w) total += red[w];
    a.count[st] = total;
  }
}

// VEC: the row is 16-byte aligned and V a multiple of 4 -- a group of 4 ids is one 16-byte piece.  Otherwise the same ids one
// by one, bounds-checked.
template <bool VEC>
__global__ __launch_bounds__(CS_T) void constraint_mask_kernel(ConstraintP a) {
  const int r = blockIdx.x / CS_G, g = blockIdx.x % CS_G, tid = threadIdx.x;
  const bool first = g == 0 && tid == 0;
  int* meta = a.meta + (long)r * CS_META;
  const int s = a.slot_of_row ? a.slot_of_row[r] : r;
  int flag = 0, st = -1;
  long q = -1;
  bool live = s >= 0 && s < a.n_state && a.finished[s] == 0;  // (everything here is uniform over the row's workgroups)
  if (live) {
    q = a.out_row ? a.out_row[s] : (long)r;
    if (q < 0 || q >= (long)a.n_req) {
      live = false;
      flag = CS_FLAG_REQUEST;
    }
  }
  if (live) {
    const int step = a.out_row ? a.step[s] : a.step[0];
    st = step == 0 ? a.start[q] : a.state[s];
    if (st < 0 || st >= a.n_states) {
      live = false;
      flag = CS_FLAG_STATE;
    }
  }
  if (!live) {
    if (first) {
      meta[0] = 0;
      if (flag && a.flag) atomicOr(a.flag, flag);
    }
    return;
  }
  if (first) {
    meta[0] = 1;
    meta[1] = s;
    meta[2] = st;
    meta[3] = (int)q;
  }
  const int V = a.V;
  if (a.count[st] >= V) return;  // a state that allows everything: the row stays as it is
  const unsigned int* bm = a.bitmap + (long)st * a.W;
  float* x = a.logits + (long)r * V;
  const f32x4 ninf = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  if constexpr (VEC) {
    const int n4 = V >> 2, chunk4 = (n4 + CS_G - 1) / CS_G;
    const int hi4 = min((g + 1) * chunk4, n4);
    f32x4* x4 = reinterpret_cast<f32x4*>(x);
    for (int i4 = g * chunk4 + tid; i4 < hi4; i4 += CS_T) {
      const unsigned int ok = (bm[i4 >> 3] >> ((i4 & 7) << 2)) & 0xFu;
      if (ok == 0xFu) continue;
      if (ok == 0u) {
        x4[i4] = ninf;
        continue;
      }
      f32x4 v = x4[i4];
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (!((ok >> c) & 1u)) v[c] = -INFINITY;
      x4[i4] = v;
    }
  } else {
    const int chunk = (V + CS_G - 1) / CS_G;
    const int hi = min((g + 1) * chunk, V);
    for (int i = g * chunk + tid; i < hi; i += CS_T)
      if (!((bm[i >> 5] >> (i & 31)) & 1u)) x[i] = -INFINITY;
  }
}

__global__ __launch_bounds__(CS_T) void constraint_advance_kernel(ConstraintP a) {
  const int r = blockIdx.x * CS_T + threadIdx.x;
  if (r >= a.rows) return;
  const int* meta = a.meta + (long)r * CS_META;
  if (meta[0] == 0) return;  // inert, finished or skipped when the mask ran
  const int s = meta[1], st = meta[2], q = meta[3];
  if (s < 0 || s >= a.n_state || st < 0 || st >= a.n_states || q < 0 || q >= a.n_req) return;  // (the mask's own words)
  const long tok = a.cur_tok[s];
  int ns = -1;
  if (tok >= 0 && tok < (long)a.V) ns = next_state(a, st, a.token_class[tok]);
  if (ns < 0) {
    ns = st;
    if (a.flag) atomicOr(a.flag, CS_FLAG_TOKEN);
  }
  a.state[s] = ns;
  if (a.request_state) a.request_state[q] = ns;
}

static inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

static int constraint_table(const char* who, const tcavt_constraint_table* t, ConstraintP* p) {
  TCAVT_CHECK_ARG(t, "%s: table is a null pointer", who);
  const struct { const void* p; const char* name; } ptrs[] = {
      {t->token_class, "token_class"}, {t->trans, "trans"}, {t->bitmap, "bitmap"}, {t->count, "count"}};
  for (const auto& q : ptrs) TCAVT_CHECK_ARG(q.p, "%s: table: %s is a null pointer", who, q.name);
  TCAVT_CHECK_ARG(t->V > 0, "%s: table: V = %d must be > 0", who, t->V);
  TCAVT_CHECK_ARG(t->n_states >= 1 && t->n_states <= CS_MAX_STATES, "%s: table: n_states = %d outside [1, %d]", who, t->n_states,
                  CS_MAX_STATES);
  TCAVT_CHECK_ARG(t->n_classes >= 1 && t->n_classes <= CS_MAX_CLASSES, "%s: table: n_classes = %d outside [1, %d]", who, t->n_classes,
                  CS_MAX_CLASSES);
  TCAVT_CHECK_ARG(aligned16(t->token_class), "%s: table: token_class must be 16-byte aligned", who);
  TCAVT_CHECK_ARG(aligned4(t->trans) && aligned4(t->bitmap) && aligned4(t->count), "%s: table: trans, bitmap and count must be 4-byte aligned",
                  who);
  p->token_class = t->token_class; p->trans = t->trans; p->bitmap = t->bitmap; p->count = t->count;
  p->V = t->V; p->W = (t->V + 31) / 32; p->n_states = t->n_states; p->n_classes = t->n_classes;
  return TCAVT_OK;
}

static int constraint_args(const char* who, const tcavt_constraint_args* a, ConstraintP* p) {
  TCAVT_CHECK_ARG(a, "%s: args is a null pointer", who);
  const int rc = constraint_table(who, a->table, p);
  if (rc != TCAVT_OK) return rc;
  const bool rows = a->slot_of_row != nullptr;
  const struct { const void* p; const char* name; bool need; } ptrs[] = {
      {a->logits, "logits", true}, {a->step, "step", true}, {a->out_row, "out_row", rows}, {a->finished, "finished", true},
      {a->cur_tok, "cur_tok", true}, {a->state, "state", true}, {a->start, "start", true}, {a->workspace, "workspace", true}};
  for (const auto& q : ptrs) TCAVT_CHECK_ARG(q.p || !q.need, "%s: %s is a null pointer", who, q.name);
  TCAVT_CHECK_ARG(a->rows > 0, "%s: rows = %d must be > 0", who, a->rows);
  TCAVT_CHECK_ARG(!rows || a->n_state > 0, "%s: n_state = %d must be > 0 with slot_of_row", who, a->n_state);
  TCAVT_CHECK_ARG(a->n_req > 0, "%s: n_req = %d must be > 0", who, a->n_req);
  TCAVT_CHECK_ARG(a->out_row || a->n_req >= a->rows, "%s: n_req = %d for rows = %d in the batch form", who, a->n_req, a->rows);
  TCAVT_CHECK_ARG(aligned4(a->logits) && aligned4(a->state) && aligned4(a->start) && aligned4(a->request_state) && aligned4(a->flag),
                  "%s: logits, state, start, request_state and flag must be 4-byte aligned", who);
  const int64_t need = tcavt_constraint_workspace_bytes(a->rows);
  TCAVT_CHECK_ARG(a->workspace_bytes >= need, "%s: workspace_bytes = %lld, needs %lld", who, (long long)a->workspace_bytes, (long long)need);
  TCAVT_CHECK_ARG(aligned16(a->workspace), "%s: workspace must be 16-byte aligned", who);
  p->logits = a->logits; p->slot_of_row = a->slot_of_row; p->step = a->step; p->out_row = reinterpret_cast<const long*>(a->out_row);
  p->finished = a->finished; p->cur_tok = reinterpret_cast<const long*>(a->cur_tok); p->state = a->state; p->start = a->start;
  p->request_state = a->request_state; p->flag = a->flag; p->meta = static_cast<int*>(a->workspace);
  p->rows = a->rows; p->n_state = rows ? a->n_state : a->rows; p->n_req = a->n_req;
  return TCAVT_OK;
}

}  // namespace tcavt

using namespace tcavt;

extern "C" int64_t tcavt_constraint_workspace_bytes(int rows) {
  return rows <= 0 ? 0 : (int64_t)rows * CS_META * 4;
}

extern "C" int tcavt_constraint_build(const tcavt_constraint_table* t, tcavt_stream_t stream) {
  ConstraintP p = {};
  const int rc = constraint_table("constraint_build", t, &p);
  if (rc != TCAVT_OK) return rc;
  hipLaunchKernelGGL(constraint_build_kernel, dim3(p.n_states), dim3(CS_T), 0, static_cast<hipStream_t>(stream), p);
  TCAVT_CHECK_LAUNCH("constraint_build");
  return TCAVT_OK;
}

extern "C" int tcavt_constraint_mask(const tcavt_constraint_args* a, tcavt_stream_t stream) {
  ConstraintP p = {};
  const int rc = constraint_args("constraint_mask", a, &p);
  if (rc != TCAVT_OK) return rc;
  const bool vec = (p.V & 3) == 0 && aligned16(p.logits);
  hipLaunchKernelGGL(vec ? constraint_mask_kernel<true> : constraint_mask_kernel<false>, dim3(p.rows * CS_G), dim3(CS_T), 0,
                     static_cast<hipStream_t>(stream), p);
  TCAVT_CHECK_LAUNCH("constraint_mask");
  return TCAVT_OK;
}

extern "C" int tcavt_constraint_advance(const tcavt_constraint_args* a, tcavt_stream_t stream) {
  ConstraintP p = {};
  const int rc = constraint_args("constraint_advance", a, &p);
  if (rc != TCAVT_OK) return rc;
  hipLaunchKernelGGL(constraint_advance_kernel, dim3((p.rows + CS_T - 1) / CS_T), dim3(CS_T), 0, static_cast<hipStream_t>(stream), p);
  TCAVT_CHECK_LAUNCH("constraint_advance");
  return TCAVT_OK;
}
