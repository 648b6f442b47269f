// mutation.hip — the WorkflowMutation of a carry-in replay (cdr_mutation_async).
//
// CloseTransactionAsMutation (mutableStateBuilder.go:3721-3785) hands UpdateWorkflowExecution,
// per pending table, the rows to upsert and the keys to delete.  Here that is the NET
// difference of two states the device already holds: the loaded state IN (cdr_carry) and the
// replayed state OUT (cdr_out), both with every table in ascending unique key order — a keyed
// merge of two sorted row lists per entry and table, pure data movement.
//
// Shape: one wavefront (a 64-thread workgroup) takes 64 consecutive entries and one table at
// a time.  It prefix-sums the entries' row counts and deals the (entry, row) pairs out across
// its lanes, 64 at a time, so an entry with 2 rows and its neighbour with 2,000 cost what
// their rows cost, in any mix.  Each pair finds its partner row in the other state with a
// binary search by key (no merge pointer to carry between chunks, no quadratic path) and checks
// its key against its predecessor's (the order precondition, verified as it merges).  The rows
// themselves move word-wise: the chunk's 64 rows are compared against their partners, and the
// upserts copied to their compacted slots, with lane l of step t on 8-byte word 64 t + l of
// the chunk — consecutive lanes on consecutive words of consecutive rows, 512 contiguous bytes
// per instruction wherever the rows are neighbours (rows are 8-B aligned: 136 / 40 / 72 / 40 /
// 56 B).  Ranks (the compacted position of an upsert or a delete key within its entry) come
// from one ballot per chunk, segmented by entry, plus a per-entry running count in LDS.
// Every loop has a wave-uniform trip count; lanes are predicated inside.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>

#include "cdr/cdr.h"
#include "ctx.h"

#define HIPCHK(x)                                                                                     \
  do {                                                                                                \
    hipError_t _e = (x);                                                                              \
    if (_e != hipSuccess) {                                                                           \
      fprintf(stderr, "cdr: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
      return CDR_API_EDEVICE;                                                                         \
    }                                                                                                 \
  } while (0)

namespace {

constexpr uint32_t WAVE = 64;

// rows as 8-byte words: NW words per row, the key in word KW (KEY32: its low 32 bits, a handle)
static_assert(sizeof(cdr_activity_info) == 136 && offsetof(cdr_activity_info, schedule_id) == 8, "activity key");
static_assert(sizeof(cdr_timer_info) == 40 && offsetof(cdr_timer_info, timer_id) == 32, "timer key");
static_assert(sizeof(cdr_child_info) == 72 && offsetof(cdr_child_info, initiated_id) == 8, "child key");
static_assert(sizeof(cdr_cancel_info) == 40 && offsetof(cdr_cancel_info, initiated_id) == 16, "cancel key");
static_assert(sizeof(cdr_signal_info) == 56 && offsetof(cdr_signal_info, initiated_id) == 16, "signal key");

struct mut_table {
  const uint64_t* in;   // loaded rows (carry.state)
  const uint64_t* out;  // replayed rows
  uint64_t* up;         // upserts (same slices as `out`)
  int64_t* del;         // delete keys (same slices as `in`)
};

struct mut_args {
  const cdr_wf_caps* caps;    // [n_wfs] of the replayed batch
  const cdr_carry* carry;     // device copy
  const cdr_wf_result* res;   // [n_wfs] the replay's results
  cdr_wf_result* up_res;      // [n_wfs]
  cdr_mut_info* info;         // [n_wfs]
  mut_table t[5];
  uint32_t n_wfs;
};

struct wave_lds {
  uint64_t pre[WAVE + 1];             // exclusive scan of the pass's row counts
  uint64_t off_in[WAVE], off_out[WAVE];  // first row of each entry's slices
  uint32_t n_in[WAVE], n_out[WAVE];
  uint32_t cnt[WAVE];                 // upserts / deletes ranked so far
  uint32_t bad[WAVE];                 // an order violation was seen
  uint64_t src[WAVE];                 // per pair of the chunk: its row,
  int64_t par[WAVE];                  // its partner row (-1: none),
  int64_t dst[WAVE];                  // its compacted slot (-1: not written)
  uint32_t neq[WAVE];                 // and whether it differs from its partner
};

__device__ __forceinline__ uint32_t uniform32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint64_t uniform64(uint64_t x) {
  return (uint64_t)uniform32((uint32_t)x) | ((uint64_t)uniform32((uint32_t)(x >> 32)) << 32);
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t x = (uint32_t)__shfl_xor((int)v, o, WAVE);
    v = x > v ? x : v;
  }
  return uniform32(v);
}

// pre[0..64] = exclusive scan of the lanes' counts; returns the total (wave-uniform)
__device__ __forceinline__ uint64_t scan_counts(wave_lds& S, uint32_t lane, uint32_t n) {
  uint64_t v = n;
  for (int o = 1; o < (int)WAVE; o <<= 1) {
    const uint64_t x = (uint64_t)__shfl_up((unsigned long long)v, o, WAVE);
    if ((int)lane >= o) v += x;
  }
  if (lane == 0) S.pre[0] = 0;
  S.pre[lane + 1] = v;
  __syncthreads();
  return uniform64(S.pre[WAVE]);
}

// the entry (lane index) that owns pair i: the largest e with pre[e] <= i
__device__ __forceinline__ uint32_t owner(const wave_lds& S, uint64_t i) {
  uint32_t e = 0;
#pragma unroll
  for (uint32_t step = WAVE / 2; step > 0; step >>= 1)
    if (S.pre[e + step] <= i) e += step;
  return e;
}

template <bool KEY32>
__device__ __forceinline__ int64_t key_of(uint64_t word) {
  return KEY32 ? (int64_t)(uint32_t)word : (int64_t)word;
}

// One table of the wave's 64 entries.  Lane `lane` brings its entry's slices; returns its
// (upsert, delete) counts.  UPSERT pass: every OUT row looks its key up in IN, differs from
// it or not, and the ones that are new or changed are copied; DELETE pass: every IN row looks
// its key up in OUT and the missing ones' keys are written.
template <uint32_t NW, uint32_t KW, bool KEY32>
__device__ uint2 diff_table(wave_lds& S, const uint32_t lane, const mut_table& T, uint64_t off_in, uint32_t n_in,
                            uint64_t off_out, uint32_t n_out) {
  uint32_t n_up = 0, n_del = 0;
  __syncthreads();  // the previous table's reads of the per-entry arrays are done
  S.off_in[lane] = off_in;
  S.off_out[lane] = off_out;
  S.n_in[lane] = n_in;
  S.n_out[lane] = n_out;
  // search steps, wave-uniform: a 4-ary step leaves at most a quarter of the range
  const uint32_t it_in = (33u - (uint32_t)__clz((int)wave_max(n_in))) / 2;
  const uint32_t it_out = (33u - (uint32_t)__clz((int)wave_max(n_out))) / 2;

#pragma unroll 1
  for (int pass = 0; pass < 2; pass++) {  // 0: OUT rows against IN (upserts); 1: IN rows against OUT (deletes)
    const uint64_t* mine = pass == 0 ? T.out : T.in;
    const uint64_t* other = pass == 0 ? T.in : T.out;
    const uint64_t* my_off = pass == 0 ? S.off_out : S.off_in;
    const uint64_t* ot_off = pass == 0 ? S.off_in : S.off_out;
    const uint32_t* ot_n = pass == 0 ? S.n_in : S.n_out;
    const uint32_t steps = pass == 0 ? it_in : it_out;
    S.cnt[lane] = 0;
    const uint64_t total = scan_counts(S, lane, pass == 0 ? n_out : n_in);  // barrier inside
#pragma unroll 1
    for (uint64_t c0 = 0; c0 < total; c0 += WAVE) {
      const uint64_t i = c0 + lane;
      const bool active = i < total;
      uint32_t e = 0, lo = 0, hi = 0, on = 0;
      uint64_t row = 0, obase = 0, ebase = 0;
      int64_t key = 0, khi = 0;  // khi: the key at `hi` once the search has looked at it
      if (active) {
        e = owner(S, i);
        ebase = S.pre[e];
        row = my_off[e] + (i - ebase);
        key = key_of<KEY32>(mine[row * NW + KW]);
        on = ot_n[e];
        hi = on;
        obase = ot_off[e];
      }
      // the order check: the previous row's key is the neighbour lane's, except in lane 0
      int64_t prev = (int64_t)__shfl_up((unsigned long long)key, 1, WAVE);
      if (active && lane == 0 && i > ebase) prev = key_of<KEY32>(mine[(row - 1) * NW + KW]);
      if (active && i > ebase && prev >= key) S.bad[e] = 1;
      for (uint32_t s = 0; s < steps; s++) {  // lower bound of key among the partner slice's keys, 4-ary:
        if (lo < hi) {                        // three independent pivot loads per round trip
          const uint32_t len = hi - lo;
          const uint32_t m1 = lo + len / 4, m2 = lo + len / 2, m3 = lo + (len / 4) * 3 + (len % 4) * 3 / 4;
          const int64_t k1 = key_of<KEY32>(other[(obase + m1) * NW + KW]);
          const int64_t k2 = key_of<KEY32>(other[(obase + m2) * NW + KW]);
          const int64_t k3 = key_of<KEY32>(other[(obase + m3) * NW + KW]);
          if (k1 >= key) hi = m1, khi = k1;
          else if (k2 >= key) lo = m1 + 1, hi = m2, khi = k2;
          else if (k3 >= key) lo = m2 + 1, hi = m3, khi = k3;
          else lo = m3 + 1;
        }
      }
      const bool found = active && lo < on && khi == key;  // lo == hi: below `on` only if the search set it
      S.src[lane] = row;
      S.par[lane] = found && pass == 0 ? (int64_t)(obase + lo) : -1;
      S.neq[lane] = active && !found ? 1u : 0u;
      __syncthreads();
      if (pass == 0 && __ballot(found) != 0) {  // compare the rows that have a partner, word-wise
#pragma unroll 4
        for (uint32_t t = 0; t < NW; t++) {
          const uint32_t idx = t * WAVE + lane, p = idx / NW, wd = idx % NW;
          const int64_t q = S.par[p];
          if (q >= 0 && mine[S.src[p] * NW + wd] != other[(uint64_t)q * NW + wd]) S.neq[p] = 1;
        }
        __syncthreads();
      }
      // rank among the entry's flagged pairs: the chunk's flagged lanes from the entry's first
      // lane in this chunk up to this one, plus what earlier chunks counted
      const bool flag = S.neq[lane] != 0;
      const uint64_t m = __ballot(flag);
      uint32_t pos = 0;
      if (active) {
        const uint32_t first = ebase > c0 ? (uint32_t)(ebase - c0) : 0u;
        const uint64_t below = m & ((1ull << lane) - 1ull) & ~((1ull << first) - 1ull);
        pos = S.cnt[e] + (uint32_t)__popcll(below);
      }
      S.dst[lane] = flag ? (int64_t)(my_off[e] + pos) : -1;  // upserts in OUT's slice, delete keys in IN's
      __syncthreads();  // every lane has read cnt
      if (active && (lane == WAVE - 1 || i + 1 == total || i + 1 == S.pre[e + 1])) S.cnt[e] = pos + (flag ? 1u : 0u);
      if (m != 0) {
        if (pass == 0) {  // copy the upserts, word-wise, to their compacted slots
#pragma unroll 4
          for (uint32_t t = 0; t < NW; t++) {
            const uint32_t idx = t * WAVE + lane, p = idx / NW, wd = idx % NW;
            const int64_t d = S.dst[p];
            if (d >= 0) T.up[(uint64_t)d * NW + wd] = mine[S.src[p] * NW + wd];
          }
        } else if (flag) {
          T.del[S.dst[lane]] = key;
        }
      }
      __syncthreads();  // the chunk's arrays are free again; cnt is up to date
    }
    __syncthreads();
    if (pass == 0) n_up = S.cnt[lane];
    else n_del = S.cnt[lane];
    __syncthreads();
  }
  return make_uint2(n_up, n_del);
}

// an entry's slice of table TBL: its first row and its row count (never past the slice's capacity)
template <int TBL>
__device__ __forceinline__ void slice_of(const cdr_wf_caps& c, const cdr_wf_result& r, uint64_t& off, uint32_t& n) {
  if (TBL == 0) off = c.act_off, n = min(r.n_activity, c.act_cap);
  else if (TBL == 1) off = c.timer_off, n = min(r.n_timer, c.timer_cap);
  else if (TBL == 2) off = c.child_off, n = min(r.n_child, c.child_cap);
  else if (TBL == 3) off = c.cancel_off, n = min(r.n_cancel, c.cancel_cap);
  else off = c.signal_off, n = min(r.n_signal, c.signal_cap);
}

__global__ __launch_bounds__(WAVE) void k_mutation(const mut_args A) {
  __shared__ wave_lds S;
  const uint32_t lane = threadIdx.x;
  const uint32_t w = blockIdx.x * WAVE + lane;
  const bool valid = w < A.n_wfs;
  const cdr_carry& cy = *A.carry;

  int32_t rcode = -1, src = -1;
  int32_t code = CDR_MUT_NOT_OK;
  uint32_t flags = 0;
  int64_t condition = 0;
  bool ok = false, stored = false;  // the entry takes part; it has a stored predecessor to diff against
  // the entry's slices of the five tables, held in registers: reading them again table by
  // table frees registers for 7 waves per SIMD instead of 5 and measured 1.3x SLOWER (one
  // more dependent round trip per table)
  uint64_t off_in[5] = {}, off_out[5] = {};
  uint32_t n_in[5] = {}, n_out[5] = {};
  if (valid) {
    rcode = A.res[w].code;
    src = cy.src[w];
    const bool in_mem = cy.in_memory != nullptr && cy.in_memory[w] != 0;
    const bool src_ok = src < 0 || (uint32_t)src < cy.n_src;
    ok = rcode == CDR_OK && src_ok;
    if (src < 0 || in_mem) flags |= CDR_MUT_SNAPSHOT;
    if (src >= 0 && src_ok && !in_mem) {
      condition = cy.state.exec[src].next_event_id;
      if (cy.state.result[src].code != CDR_OK) ok = false;
      stored = ok;
    }
    if (stored) {
      const cdr_wf_caps& lc = cy.caps[src];
      const cdr_wf_result& lr = cy.state.result[src];
      slice_of<0>(lc, lr, off_in[0], n_in[0]), slice_of<1>(lc, lr, off_in[1], n_in[1]);
      slice_of<2>(lc, lr, off_in[2], n_in[2]), slice_of<3>(lc, lr, off_in[3], n_in[3]);
      slice_of<4>(lc, lr, off_in[4], n_in[4]);
    }
    if (ok) {
      code = CDR_MUT_OK;
      const cdr_wf_caps& c = A.caps[w];
      const cdr_wf_result& r = A.res[w];
      slice_of<0>(c, r, off_out[0], n_out[0]), slice_of<1>(c, r, off_out[1], n_out[1]);
      slice_of<2>(c, r, off_out[2], n_out[2]), slice_of<3>(c, r, off_out[3], n_out[3]);
      slice_of<4>(c, r, off_out[4], n_out[4]);
    }
  }
  S.bad[lane] = 0;
  // the loaded tables' addresses are in the device's carry record
  mut_table T = A.t[0];
  T.in = (const uint64_t*)cy.state.act;
  const uint2 c0 = diff_table<sizeof(cdr_activity_info) / 8, 1, false>(S, lane, T, off_in[0], n_in[0], off_out[0], n_out[0]);
  T = A.t[1], T.in = (const uint64_t*)cy.state.timer;
  const uint2 c1 = diff_table<sizeof(cdr_timer_info) / 8, 4, true>(S, lane, T, off_in[1], n_in[1], off_out[1], n_out[1]);
  T = A.t[2], T.in = (const uint64_t*)cy.state.child;
  const uint2 c2 = diff_table<sizeof(cdr_child_info) / 8, 1, false>(S, lane, T, off_in[2], n_in[2], off_out[2], n_out[2]);
  T = A.t[3], T.in = (const uint64_t*)cy.state.cancel;
  const uint2 c3 = diff_table<sizeof(cdr_cancel_info) / 8, 2, false>(S, lane, T, off_in[3], n_in[3], off_out[3], n_out[3]);
  T = A.t[4], T.in = (const uint64_t*)cy.state.signal;
  const uint2 c4 = diff_table<sizeof(cdr_signal_info) / 8, 2, false>(S, lane, T, off_in[4], n_in[4], off_out[4], n_out[4]);
  uint32_t n_up[5] = {c0.x, c1.x, c2.x, c3.x, c4.x}, n_del[5] = {c0.y, c1.y, c2.y, c3.y, c4.y};
  if (!valid) return;
  if (S.bad[lane]) {
    code = CDR_MUT_E_ORDER;
    for (int t = 0; t < 5; t++) n_up[t] = n_del[t] = 0;
  }
  cdr_mut_info mi;
  mi.code = code;
  mi.flags = flags;
  mi.condition = condition;
  mi.n_del_act = n_del[0], mi.n_del_timer = n_del[1], mi.n_del_child = n_del[2];
  mi.n_del_cancel = n_del[3], mi.n_del_signal = n_del[4];
  mi._pad = 0;
  A.info[w] = mi;
  cdr_wf_result r = A.res[w];
  if (rcode == CDR_OK) {  // entries that did not replay OK keep their result as it is
    r.n_activity = n_up[0], r.n_timer = n_up[1], r.n_child = n_up[2], r.n_cancel = n_up[3], r.n_signal = n_up[4];
  }
  A.up_res[w] = r;
}

bool complete(const cdr_out* out, const cdr_mutation* mut) {
  const cdr_out& u = mut->upsert;
  return out->result && out->act && out->timer && out->child && out->cancel && out->signal && u.result && u.act &&
         u.timer && u.child && u.cancel && u.signal && mut->del_act && mut->del_timer && mut->del_child &&
         mut->del_cancel && mut->del_signal && mut->info;
}

}  // namespace

extern "C" {

int cdr_mutation_async(cdr_ctx* ctx, const cdr_dev_batch* in, const cdr_out* out, const cdr_mutation* mut,
                       void* stream) {
  if (!ctx || !in || !out || !mut || !in->carry || !in->caps || !complete(out, mut)) return CDR_API_EINVAL;
  if (in->n_wfs == 0) return CDR_API_OK;
  // the carried states' table pointers live in the device copy of cdr_carry: the kernel reads
  // them there (no host read of device memory)
  mut_args A{};
  A.caps = in->caps;
  A.carry = in->carry;
  A.res = out->result;
  A.up_res = mut->upsert.result;
  A.info = mut->info;
  A.n_wfs = in->n_wfs;
  const void* outs[5] = {out->act, out->timer, out->child, out->cancel, out->signal};
  void* ups[5] = {mut->upsert.act, mut->upsert.timer, mut->upsert.child, mut->upsert.cancel, mut->upsert.signal};
  int64_t* dels[5] = {mut->del_act, mut->del_timer, mut->del_child, mut->del_cancel, mut->del_signal};
  for (int t = 0; t < 5; t++) {
    A.t[t].in = nullptr;  // the kernel takes it from the carry record
    A.t[t].out = (const uint64_t*)outs[t];
    A.t[t].up = (uint64_t*)ups[t];
    A.t[t].del = dels[t];
  }
  hipLaunchKernelGGL(k_mutation, dim3((in->n_wfs + WAVE - 1) / WAVE), dim3(WAVE), 0, (hipStream_t)stream, A);
  HIPCHK(hipGetLastError());
  return CDR_API_OK;
}

// host buffers: the loaded states, the replay's results and rows and the caller's mutation
// buffers go up into the context's workspace, the kernel runs, the mutation comes down
int cdr_mutation_batch(cdr_ctx* ctx, const cdr_batch* b, const cdr_wf_caps* caps, const cdr_totals* tot,
                       const cdr_out* out, cdr_mutation* mut, void* stream) {
  if (!ctx || !b || !caps || !tot || !out || !mut || !b->carry || !b->carry->src || !b->carry->caps ||
      !complete(out, mut))
    return CDR_API_EINVAL;
  const cdr_carry& hc = *b->carry;
  if (!hc.state.result || !hc.state.exec || !hc.state.act || !hc.state.timer || !hc.state.child ||
      !hc.state.cancel || !hc.state.signal)
    return CDR_API_EINVAL;
  if (b->n_wfs == 0) return CDR_API_OK;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  bool oom = false, dev_err = false;
  auto up = [&](int slot, const void* src, uint64_t bytes) -> void* {
    void* p = cdr_ws_get(ctx, slot, bytes ? bytes : 8);
    if (!p) {
      oom = true;
      return nullptr;
    }
    if (bytes && hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess) dev_err = true;
    return p;
  };
  const uint64_t n = b->n_wfs, ns = hc.n_src;
  const cdr_totals& ct = hc.totals;
  cdr_carry dc = hc;
  dc.state = cdr_out{};
  dc.src = (const int32_t*)up(WS_CY_SRC, hc.src, n * 4);
  dc.caps = (const cdr_wf_caps*)up(WS_CY_CAPS, hc.caps, ns * sizeof(cdr_wf_caps));
  dc.state.result = (cdr_wf_result*)up(WS_CY_RESULT, hc.state.result, ns * sizeof(cdr_wf_result));
  dc.state.exec = (cdr_exec_info*)up(WS_CY_EXEC, hc.state.exec, ns * sizeof(cdr_exec_info));
  dc.state.act = (cdr_activity_info*)up(WS_CY_ACT, hc.state.act, ct.act * sizeof(cdr_activity_info));
  dc.state.timer = (cdr_timer_info*)up(WS_CY_TIMER, hc.state.timer, ct.timer * sizeof(cdr_timer_info));
  dc.state.child = (cdr_child_info*)up(WS_CY_CHILD, hc.state.child, ct.child * sizeof(cdr_child_info));
  dc.state.cancel = (cdr_cancel_info*)up(WS_CY_CANCEL, hc.state.cancel, ct.cancel * sizeof(cdr_cancel_info));
  dc.state.signal = (cdr_signal_info*)up(WS_CY_SIGNAL, hc.state.signal, ct.signal * sizeof(cdr_signal_info));
  dc.in_memory = hc.in_memory ? (const uint8_t*)up(WS_CY_INMEM, hc.in_memory, n) : nullptr;
  cdr_dev_batch db{};
  db.n_wfs = b->n_wfs;
  db.caps = (const cdr_wf_caps*)up(WS_CAPS, caps, n * sizeof(cdr_wf_caps));
  db.carry = (const cdr_carry*)up(WS_CY_DESC, &dc, sizeof(dc));
  cdr_out dout{};
  dout.result = (cdr_wf_result*)up(WS_O_RESULT, out->result, n * sizeof(cdr_wf_result));
  dout.act = (cdr_activity_info*)up(WS_O_ACT, out->act, tot->act * sizeof(cdr_activity_info));
  dout.timer = (cdr_timer_info*)up(WS_O_TIMER, out->timer, tot->timer * sizeof(cdr_timer_info));
  dout.child = (cdr_child_info*)up(WS_O_CHILD, out->child, tot->child * sizeof(cdr_child_info));
  dout.cancel = (cdr_cancel_info*)up(WS_O_CANCEL, out->cancel, tot->cancel * sizeof(cdr_cancel_info));
  dout.signal = (cdr_signal_info*)up(WS_O_SIGNAL, out->signal, tot->signal * sizeof(cdr_signal_info));
  // the mutation's buffers keep the caller's bytes wherever the kernel writes nothing
  struct buf {
    int slot;
    void* host;
    uint64_t bytes;
    void* dev;
  } mb[12] = {
      {WS_MUT_RESULT, mut->upsert.result, n * sizeof(cdr_wf_result), nullptr},
      {WS_MUT_ACT, mut->upsert.act, tot->act * sizeof(cdr_activity_info), nullptr},
      {WS_MUT_TIMER, mut->upsert.timer, tot->timer * sizeof(cdr_timer_info), nullptr},
      {WS_MUT_CHILD, mut->upsert.child, tot->child * sizeof(cdr_child_info), nullptr},
      {WS_MUT_CANCEL, mut->upsert.cancel, tot->cancel * sizeof(cdr_cancel_info), nullptr},
      {WS_MUT_SIGNAL, mut->upsert.signal, tot->signal * sizeof(cdr_signal_info), nullptr},
      {WS_MUT_DEL_ACT, mut->del_act, ct.act * 8, nullptr},
      {WS_MUT_DEL_TIMER, mut->del_timer, ct.timer * 8, nullptr},
      {WS_MUT_DEL_CHILD, mut->del_child, ct.child * 8, nullptr},
      {WS_MUT_DEL_CANCEL, mut->del_cancel, ct.cancel * 8, nullptr},
      {WS_MUT_DEL_SIGNAL, mut->del_signal, ct.signal * 8, nullptr},
      {WS_MUT_INFO, mut->info, n * sizeof(cdr_mut_info), nullptr},
  };
  for (buf& x : mb) x.dev = up(x.slot, x.host, x.bytes);
  if (oom || dev_err) {
    (void)hipStreamSynchronize(st);  // no copy may still read the stack record
    return oom ? CDR_API_ENOMEM : CDR_API_EDEVICE;
  }
  cdr_mutation dm{};
  dm.upsert.result = (cdr_wf_result*)mb[0].dev;
  dm.upsert.act = (cdr_activity_info*)mb[1].dev;
  dm.upsert.timer = (cdr_timer_info*)mb[2].dev;
  dm.upsert.child = (cdr_child_info*)mb[3].dev;
  dm.upsert.cancel = (cdr_cancel_info*)mb[4].dev;
  dm.upsert.signal = (cdr_signal_info*)mb[5].dev;
  dm.del_act = (int64_t*)mb[6].dev;
  dm.del_timer = (int64_t*)mb[7].dev;
  dm.del_child = (int64_t*)mb[8].dev;
  dm.del_cancel = (int64_t*)mb[9].dev;
  dm.del_signal = (int64_t*)mb[10].dev;
  dm.info = (cdr_mut_info*)mb[11].dev;
  int rc = cdr_mutation_async(ctx, &db, &dout, &dm, st);
  for (buf& x : mb)
    if (rc == CDR_API_OK && x.bytes && hipMemcpyAsync(x.host, x.dev, x.bytes, hipMemcpyDeviceToHost, st) != hipSuccess)
      rc = CDR_API_EDEVICE;
  if (hipStreamSynchronize(st) != hipSuccess && rc == CDR_API_OK) rc = CDR_API_EDEVICE;
  return rc;
}

}  // extern "C"
