// sync.hip — batched historyReplicator.SyncActivity on loaded states
// (cdr_sync_activity_async / cdr_sync_activity_batch; historyReplicator.go:160-295).
//
// The standby side receives one SyncActivityRequest per activity heartbeat and per retried
// activity start.  Each is a short decision walk over the addressed state's records, an
// update of one pending-activity row (ReplicateActivityInfo, mutableStateBuilder.go:
// 1200-1231) and the activity timer pick over all of the state's rows
// (GetActivityTimerTaskIfNeeded, timerBuilder.go:211-230).  Requests of one state depend on
// one another (a heartbeat skips when the row already holds a later one), states do not.
//
// Shape: a group of G consecutive lanes (G = 4, 8, 16 or 64) takes one state and walks its
// requests in order; requests arrive grouped by state as a CSR (cdr_plan_sync).  Lane g of
// the group owns rows g, g + G, ... of the state's activity slice — a row is read and
// written by its owning lane only, so the sequence of requests needs no memory ordering
// between lanes.  The row lookup is a key compare in every lane, the pick a lexicographic
// min of (time, scheduleID, order) over the lanes' best rows; both reduce across the group
// with DPP moves inside a 16-lane row (a butterfly: pairs, quads, half-row mirror, row
// mirror — these read lanes of the group only, so groups of one wavefront may diverge from
// one another as long as the G lanes of a group stay together, which they do: every branch
// and trip count below depends on the group's state and request alone) and, for G = 64,
// two ds_bpermute steps across rows.  A lane holds the fourteen fields of a row that the walk
// and the pick read (row_regs, scalars in registers; the rest of the 136-byte row is never
// loaded).  A state with at most G rows keeps them there across its requests and stores the
// touched ones once at the end; a larger one loops over its rows and re-reads them per
// request.  Lane 0 of the group writes the request's result, or the lane that owns the timer
// pick's head row when a task is created (it holds the row's attempt).
//
// G is a template parameter; the shipped value is CDR_SYNC_GROUP (cdr.h), the others are
// reachable through cdr_set_sync_group for tools/sync_bench.py.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "cdr/cdr.h"
#include "ctx.h"
#include "group.h"
#include "internal.h"

#define HIPCHK(x)                                                                                     \
  do {                                                                                                \
    hipError_t _e = (x);                                                                              \
    if (_e != hipSuccess) {                                                                           \
      fprintf(stderr, "cdr: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
      return CDR_API_EDEVICE;                                                                         \
    }                                                                                                 \
  } while (0)

namespace {

constexpr uint32_t BLOCK = 256;

struct sync_args {
  const cdr_sync_activity* reqs;
  const uint32_t* req_off;
  const cdr_wf_caps* caps;
  const cdr_wf_result* result;
  const cdr_exec_info* exec;
  const cdr_repl_state* repl;
  const cdr_vh_item* vh;
  cdr_activity_info* act;
  cdr_sync_result* res;
  int64_t increment;
  uint32_t n_req, n_states;
};

// the group reductions and the timer pick's head record (group.h, shared with standby.hip)
using namespace cdr_group;

// what the walk and the pick read of a pending-activity row, field names as in
// cdr_activity_info (cdr_internal::act_first_timer takes either)
struct row_regs {
  int64_t version, schedule_id, scheduled_time, started_id, started_time, last_heartbeat_time, expiration_time;
  int32_t s2s, s2c, stc, hb, timer_task_status, attempt;
  uint32_t flags;
};
__device__ __forceinline__ void load_row(row_regs& r, const cdr_activity_info* p) {
  r.version = p->version;
  r.schedule_id = p->schedule_id;
  r.scheduled_time = p->scheduled_time;
  r.started_id = p->started_id;
  r.started_time = p->started_time;
  r.last_heartbeat_time = p->last_heartbeat_time;
  r.expiration_time = p->expiration_time;
  r.s2s = p->s2s;
  r.s2c = p->s2c;
  r.stc = p->stc;
  r.hb = p->hb;
  r.timer_task_status = p->timer_task_status;
  r.attempt = p->attempt;
  r.flags = p->flags;
}
// the fields ReplicateActivityInfo and the timer pick change (the rest of the row stays)
__device__ __forceinline__ void store_row(cdr_activity_info* dst, const row_regs& a) {
  dst->version = a.version;
  dst->scheduled_time = a.scheduled_time;
  dst->started_id = a.started_id;
  dst->started_time = a.started_time;
  dst->last_heartbeat_time = a.last_heartbeat_time;
  dst->timer_task_status = a.timer_task_status;
  dst->attempt = a.attempt;
  dst->flags = a.flags;
}

__device__ __forceinline__ void write_result(cdr_sync_result* dst, const cdr_sync_activity& q, int32_t action,
                                             int32_t code, uint32_t flags, int64_t next, int64_t event_time,
                                             int64_t lwv, uint32_t act_row, uint32_t task_row, bool has_task,
                                             const head& task, int32_t task_attempt) {
  cdr_sync_result r;
  r.action = action;
  r.code = code;
  r.flags = flags;
  r._pad = 0;
  r.next_event_id = next;
  r.event_time = event_time;
  r.last_write_version = lwv;
  r.act_row = act_row;
  r.task_row = task_row;
  r.tag = q.tag;
  r._pad1 = 0;
  cdr_task t{};
  if (has_task) {  // createNewTask (timerBuilder.go:391-408): ActivityTimeoutTask
    t.type = CDR_TT_ACTIVITY_TIMEOUT;
    t.timeout_type = (int32_t)((task.info >> 1) & 7u);
    t.event_id = task.sched;
    t.visibility_ts = task.t;
    t.attempt = task_attempt;
  }
  r.timer_task = t;
  *dst = r;
}

__device__ __forceinline__ void write_plain(cdr_sync_result* dst, const cdr_sync_activity& q, int32_t action,
                                            int32_t code, int64_t next, int64_t lwv) {
  head none;
  none.t = 0, none.sched = 0, none.info = 0, none.row = CDR_SYNC_NO_ROW;
  write_result(dst, q, action, code, 0, next, 0, lwv, CDR_SYNC_NO_ROW, CDR_SYNC_NO_ROW, false, none, 0);
}

// G lanes per state, BLOCK / G states per workgroup; after the states' groups, one lane per
// request of the trailing group (wf < 0 or wf >= n_states)
template <int G>
__global__ __launch_bounds__(BLOCK) void k_sync_activity(const sync_args A) {
  const uint64_t tid = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  const uint64_t grp = tid / G;
  const uint32_t g = (uint32_t)(tid % G);
  const uint64_t state_blocks = ((uint64_t)A.n_states * G + BLOCK - 1) / BLOCK;
  if (blockIdx.x >= state_blocks) {  // the trailing group
    const uint64_t first = A.req_off[A.n_states] < A.n_req ? A.req_off[A.n_states] : A.n_req;
    const uint64_t i = first + (tid - state_blocks * BLOCK);
    if (i >= A.n_req) return;
    const cdr_sync_activity q = A.reqs[i];
    write_plain(&A.res[i], q, q.wf < 0 ? CDR_SYNC_SKIP_NO_WORKFLOW : CDR_SYNC_E_STATE, CDR_OK, 0, 0);
    return;
  }
  if (grp >= A.n_states) return;
  const uint32_t s = (uint32_t)grp;
  // the state's requests, never past the arrays whatever the CSR holds
  uint32_t r1 = A.req_off[s + 1], r0 = A.req_off[s];
  if (r1 > A.n_req) r1 = A.n_req;
  if (r0 > r1) r0 = r1;
  if (r0 == r1) return;
  const cdr_wf_result wr = A.result[s];
  if (wr.code != CDR_OK) {  // nothing is read from a failed record
    for (uint32_t i = r0 + g; i < r1; i += G)
      write_plain(&A.res[i], A.reqs[i], CDR_SYNC_E_STATE, CDR_OK, 0, 0);
    return;
  }
  const cdr_wf_caps& cp = A.caps[s];
  const uint64_t act_off = cp.act_off;
  const uint32_t n_act = wr.n_activity < cp.act_cap ? wr.n_activity : cp.act_cap;
  cdr_activity_info* const act = A.act + act_off;
  const cdr_exec_info& x = A.exec[s];
  const int32_t wstate = x.state;
  const int64_t next = x.next_event_id;
  // GetLastWriteVersion (mutableStateBuilder.go:526-545)
  const cdr_repl_state& rs = A.repl[s];
  const bool is2dc = rs.present != 0;
  const bool isNdc = !is2dc && ((x.flags & CDR_XI_VH_BRANCH) != 0 || wr.n_vh != 0);
  const uint32_t n_vh = wr.n_vh < cp.vh_cap ? wr.n_vh : cp.vh_cap;
  const bool lwv_err = isNdc && n_vh == 0;
  int64_t lwv = CDR_EMPTY_VERSION;
  if (is2dc) lwv = rs.last_write_version;
  else if (isNdc && n_vh != 0) lwv = A.vh[cp.vh_off + n_vh - 1].version;

  // rows in registers when each lane has at most one
  const bool resident = n_act <= (uint32_t)G;
  const uint32_t chunks = (n_act + G - 1) / G;
  row_regs a;
  a.version = a.schedule_id = a.scheduled_time = a.started_id = a.started_time = a.last_heartbeat_time = 0;
  a.expiration_time = 0;
  a.s2s = a.s2c = a.stc = a.hb = a.timer_task_status = a.attempt = 0;
  a.flags = 0;
  bool dirty = false;
  if (resident && g < n_act) load_row(a, &act[g]);

#pragma unroll 1
  for (uint32_t i = r0; i < r1; i++) {
    const cdr_sync_activity q = A.reqs[i];
    cdr_sync_result* const out = &A.res[i];
    // ---- the exits that need no row (:198-229)
    int32_t action = -1, code = CDR_OK;
    if (wstate == CDR_STATE_COMPLETED || wstate == CDR_STATE_ZOMBIE) {
      action = CDR_SYNC_SKIP_NOT_RUNNING;
    } else if (wstate != CDR_STATE_CREATED && wstate != CDR_STATE_RUNNING) {
      action = CDR_SYNC_SKIP_NOT_RUNNING;
      code = CDR_P_UNKNOWN_WF_STATE;
    } else if (q.scheduled_id >= next) {
      if (lwv_err) {
        action = CDR_SYNC_SKIP_STALE_VERSION;
        code = CDR_E_VH_EMPTY;
      } else if (q.version < lwv) {
        action = CDR_SYNC_SKIP_STALE_VERSION;
      } else {
        action = is2dc ? CDR_SYNC_RETRY_2DC : CDR_SYNC_RETRY_NDC;
      }
    }
    if (action >= 0) {
      if (g == 0) write_plain(out, q, action, code, next, lwv);
      continue;
    }
    // ---- GetActivityInfo (:231) and the exits on the row (:238-253), in the row's lane,
    // which applies the request at once; found = row << 8 | action << 1 | reset
    uint64_t found = ~0ull;
#pragma unroll 1
    for (uint32_t c = 0; c < chunks; c++) {
      const uint32_t row = c * G + g;
      if (row >= n_act) continue;
      if (!resident) {  // only the fields the walk reads; the hit loads the rest
        a.schedule_id = act[row].schedule_id;
      }
      if (a.schedule_id != q.scheduled_id) continue;
      if (!resident) load_row(a, &act[row]);
      int32_t act_action = CDR_SYNC_APPLIED;
      if (a.version > q.version) {
        act_action = CDR_SYNC_SKIP_LOCAL_VERSION_LARGER;
      } else if (a.version == q.version) {
        // a heartbeat time that was never set is Go's zero time: before every instant
        const bool hb_set = (a.flags & (CDR_AI_STARTED_TIME_SET | CDR_AI_HEARTBEAT_TIME_SET)) != 0;
        if (a.attempt > q.attempt) act_action = CDR_SYNC_SKIP_LOCAL_ATTEMPT_LARGER;
        else if (a.attempt == q.attempt && hb_set && a.last_heartbeat_time > q.last_heartbeat_time)
          act_action = CDR_SYNC_SKIP_HEARTBEAT_OLDER;
      }
      uint32_t reset = 0;
      if (act_action == CDR_SYNC_APPLIED) {
        // IsVersionFromSameCluster (metadata.go:163-165); the difference wraps as Go's does
        const int64_t dv = (int64_t)((uint64_t)q.version - (uint64_t)a.version);
        reset = (dv % A.increment != 0 || a.attempt < q.attempt) ? 1u : 0u;
        // ReplicateActivityInfo (mutableStateBuilder.go:1200-1231)
        const bool started = q.started_id != CDR_EMPTY_EVENT_ID;
        a.version = q.version;
        a.scheduled_time = q.scheduled_time;
        a.started_id = q.started_id;
        a.last_heartbeat_time = q.last_heartbeat_time;
        a.started_time = started ? q.started_time : 0;
        a.attempt = q.attempt;
        a.flags = (a.flags & ~(uint32_t)CDR_AI_STARTED_TIME_SET) | CDR_AI_HEARTBEAT_TIME_SET |
                  (started ? CDR_AI_STARTED_TIME_SET : 0u);
        if (reset) a.timer_task_status = CDR_TIMER_TASK_STATUS_NONE;
        if (resident) dirty = true;
        else store_row(&act[row], a);
      }
      const uint64_t f = ((uint64_t)row << 8) | ((uint64_t)act_action << 1) | reset;
      found = f < found ? f : found;
    }
    found = group_min<G>(found);
    if (found == ~0ull) {
      if (g == 0) write_plain(out, q, CDR_SYNC_SKIP_NO_ACTIVITY, CDR_OK, next, lwv);
      continue;
    }
    action = (int32_t)((found >> 1) & 0x7Fu);
    if (action != CDR_SYNC_APPLIED) {
      if (g == 0) write_plain(out, q, action, CDR_OK, next, lwv);
      continue;
    }
    const uint32_t act_row = (uint32_t)(found >> 8);
    uint32_t flags = (found & 1u) ? CDR_SYNC_RESET_TIMER_STATUS : 0u;
    // ---- GetActivityTimerTaskIfNeeded (timerBuilder.go:211-230) over the state's rows
    head h;
    h.t = 0, h.sched = 0, h.info = 0, h.row = CDR_SYNC_NO_ROW;
#pragma unroll 1
    for (uint32_t c = 0; c < chunks; c++) {
      const uint32_t row = c * G + g;
      if (row >= n_act) continue;
      if (!resident) load_row(a, &act[row]);
      if (a.schedule_id == CDR_EMPTY_EVENT_ID) continue;
      const cdr_internal::act_timer ct = cdr_internal::act_first_timer(a);
      head m;
      m.t = ct.t;
      m.sched = a.schedule_id;
      const bool created = (a.timer_task_status & cdr_internal::act_timer_bit(ct.type)) != 0;
      m.info = ((uint32_t)ct.order << 4) | ((uint32_t)ct.type << 1) | (created ? 1u : 0u);
      m.row = row;
      if (before(m, h)) h = m;
    }
    group_head<G>(h);
    uint32_t task_row = CDR_SYNC_NO_ROW;
    const bool emit = h.row != CDR_SYNC_NO_ROW && !(h.info & 1u);  // firstActivityTimerTask (:384-389)
    // the head row's lane sets its bit and, holding the row's attempt, writes the result
    int32_t task_attempt = 0;
    if (emit) {
      task_row = h.row;
      flags |= CDR_SYNC_HAS_TIMER_TASK;
      if (h.row % G == g) {
        const int32_t bit = cdr_internal::act_timer_bit((int32_t)((h.info >> 1) & 7u));
        if (resident) {
          a.timer_task_status |= bit;
          dirty = true;
          task_attempt = a.attempt;
        } else {
          act[h.row].timer_task_status |= bit;
          task_attempt = act[h.row].attempt;
        }
      }
    }
    if (g == (emit ? h.row % G : 0u)) {
      int64_t et = q.scheduled_time;
      if (et < q.started_time) et = q.started_time;
      if (et < q.last_heartbeat_time) et = q.last_heartbeat_time;
      write_result(out, q, CDR_SYNC_APPLIED, CDR_OK, flags, next, et, lwv, (uint32_t)(act_off + act_row),
                   emit ? (uint32_t)(act_off + task_row) : CDR_SYNC_NO_ROW, emit, h, task_attempt);
    }
  }
  if (dirty) store_row(&act[g], a);
}

template <int G>
void launch(const sync_args& A, hipStream_t st) {
  const uint64_t state_blocks = ((uint64_t)A.n_states * G + BLOCK - 1) / BLOCK;
  // the trailing group's size lives in device memory (req_off[n_states]): one lane per request
  // covers it whatever it is, and a launch that finds nothing to do is a few empty workgroups
  const uint64_t trail_blocks = ((uint64_t)A.n_req + BLOCK - 1) / BLOCK;
  hipLaunchKernelGGL(k_sync_activity<G>, dim3((uint32_t)(state_blocks + trail_blocks)), dim3(BLOCK), 0, st, A);
}

}  // namespace

extern "C" {

int cdr_set_sync_group(cdr_ctx* ctx, int lanes) {
  if (!ctx || (lanes != 4 && lanes != 8 && lanes != 16 && lanes != 64)) return CDR_API_EINVAL;
  const int prev = ctx->sync_group;
  ctx->sync_group = lanes;
  return prev;
}

int cdr_sync_activity_async(cdr_ctx* ctx, const cdr_sync_activity* reqs, const uint32_t* req_off, uint32_t n_req,
                            uint32_t n_states, const cdr_wf_caps* state_caps, const cdr_out* state,
                            const cdr_cluster_meta* cluster, cdr_sync_result* res, void* stream) {
  if (!ctx || !reqs || !req_off || !state_caps || !state || !cluster || !res || !state->result || !state->exec ||
      !state->repl || !state->vh || !state->act || cluster->failover_version_increment <= 0)
    return CDR_API_EINVAL;
  if (n_req == 0) return CDR_API_OK;
  sync_args A{};
  A.reqs = reqs;
  A.req_off = req_off;
  A.caps = state_caps;
  A.result = state->result;
  A.exec = state->exec;
  A.repl = state->repl;
  A.vh = state->vh;
  A.act = state->act;
  A.res = res;
  A.increment = cluster->failover_version_increment;
  A.n_req = n_req;
  A.n_states = n_states;
  hipStream_t st = (hipStream_t)stream;
  switch (ctx->sync_group) {
    case 8: launch<8>(A, st); break;
    case 16: launch<16>(A, st); break;
    case 64: launch<64>(A, st); break;
    default: launch<CDR_SYNC_GROUP>(A, st); break;
  }
  HIPCHK(hipGetLastError());
  return CDR_API_OK;
}

int cdr_sync_activity_batch(cdr_ctx* ctx, const cdr_sync_activity* reqs, const uint32_t* req_off, uint32_t n_req,
                            uint32_t n_states, const cdr_wf_caps* state_caps, const cdr_totals* tot,
                            const cdr_out* state, const cdr_cluster_meta* cluster, cdr_sync_result* res,
                            void* stream) {
  if (!ctx || !reqs || !req_off || !state_caps || !tot || !state || !cluster || !res || !state->result ||
      !state->exec || !state->repl || !state->vh || !state->act || cluster->failover_version_increment <= 0)
    return CDR_API_EINVAL;
  if (n_req == 0) return CDR_API_OK;
  HIPCHK(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  bool oom = false, dev_err = false;
  auto up = [&](int slot, const void* src, uint64_t bytes) -> void* {
    void* p = cdr_ws_get(ctx, slot, bytes ? bytes : 8);
    if (!p) {
      oom = true;
      return nullptr;
    }
    if (bytes && src && hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, st) != hipSuccess) dev_err = true;
    return p;
  };
  const uint64_t ns = n_states;
  const cdr_sync_activity* d_reqs = (const cdr_sync_activity*)up(WS_SYNC_REQ, reqs, (uint64_t)n_req * sizeof(*reqs));
  const uint32_t* d_off = (const uint32_t*)up(WS_SYNC_OFF, req_off, (ns + 1) * 4);
  cdr_sync_result* d_res = (cdr_sync_result*)up(WS_SYNC_RES, nullptr, (uint64_t)n_req * sizeof(*res));
  const cdr_wf_caps* d_caps = (const cdr_wf_caps*)up(WS_CY_CAPS, state_caps, ns * sizeof(cdr_wf_caps));
  cdr_out ds{};
  ds.result = (cdr_wf_result*)up(WS_CY_RESULT, state->result, ns * sizeof(cdr_wf_result));
  ds.exec = (cdr_exec_info*)up(WS_CY_EXEC, state->exec, ns * sizeof(cdr_exec_info));
  ds.repl = (cdr_repl_state*)up(WS_CY_REPL, state->repl, ns * sizeof(cdr_repl_state));
  ds.vh = (cdr_vh_item*)up(WS_CY_VH, state->vh, tot->vh * sizeof(cdr_vh_item));
  ds.act = (cdr_activity_info*)up(WS_CY_ACT, state->act, tot->act * sizeof(cdr_activity_info));
  if (oom || dev_err) {
    (void)hipStreamSynchronize(st);
    return oom ? CDR_API_ENOMEM : CDR_API_EDEVICE;
  }
  int rc = cdr_sync_activity_async(ctx, d_reqs, d_off, n_req, n_states, d_caps, &ds, cluster, d_res, st);
  if (rc == CDR_API_OK && tot->act &&
      hipMemcpyAsync(state->act, ds.act, tot->act * sizeof(cdr_activity_info), hipMemcpyDeviceToHost, st) != hipSuccess)
    rc = CDR_API_EDEVICE;
  if (rc == CDR_API_OK &&
      hipMemcpyAsync(res, d_res, (uint64_t)n_req * sizeof(*res), hipMemcpyDeviceToHost, st) != hipSuccess)
    rc = CDR_API_EDEVICE;
  if (hipStreamSynchronize(st) != hipSuccess && rc == CDR_API_OK) rc = CDR_API_EDEVICE;
  return rc;
}

}  // extern "C"
