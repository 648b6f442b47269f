// standby.hip — batched standby task verification on loaded states
// (cdr_standby_tasks_async / cdr_standby_tasks_batch; timerQueueStandbyProcessor.go:173-626,
// transferQueueStandbyProcessor.go:137-660, xdcUtil.go:70-169).
//
// The standby cluster hands every transfer and timer task the replay emits to one of the two
// standby processors, which load the workflow's mutable state and decide: acknowledge, retry,
// re-fetch the history, push to matching, record in visibility or — the one write — regenerate
// the activity timer task.  Per task that is a short walk over the state's records, a key
// lookup in one pending table or a min over the state's timer / activity rows.  Requests of
// one state depend on one another (an UPDATED activity timeout changes timer_task_status),
// states do not.
//
// Shape: k_sync_activity's (sync.hip).  A group of G consecutive lanes takes one state and
// walks its requests in order (a CSR from cdr_plan_standby); lane g owns rows g, g + G, ... of
// whichever table the request reads.  Everything a lane gathers from its rows is one 64-bit
// scalar per pass — a row index for a lookup, an expiry or a schedule id for a min (sign bit
// flipped, so unsigned order is signed order) — reduced across the group with the DPP
// butterflies of group.h, after which every lane knows the answer; every loop around them has
// the same trip count in all lanes of a group.  The head of the activity timers (time, schedule
// id, order) is three such passes and a lookup, not a per-lane pick between whole rows.  Lane 0
// builds the result record in registers and stores it whole.  A row's timer_task_status is
// read and written by the row's owning lane only, which tells the group what it saw, so the
// sequence of requests needs no memory ordering between lanes; the fields a lane reads from
// another lane's row (version, started_id, the ScheduleToStart timeout, attempt) are never
// written here.  Of a row only the fields the walk reads are loaded: a key per row for a
// lookup, the expiry per timer row, the eleven timer fields per activity row.
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

using namespace cdr_group;

constexpr uint32_t BLOCK = 256;
constexpr uint32_t TT_ACTIVITY_RETRY_TIMER = 16 + 5;  // TaskTypeActivityRetryTimer
constexpr uint32_t TT_RESET_WORKFLOW = 7;             // TransferTaskTypeResetWorkflow

struct standby_args {
  const cdr_standby_task* reqs;
  const uint32_t* req_off;
  const cdr_wf_caps* caps;
  const cdr_wf_result* result;
  const cdr_exec_info* exec;
  const cdr_repl_state* repl;
  const cdr_vh_item* vh;
  cdr_activity_info* act;
  const cdr_timer_info* timer;
  const cdr_child_info* child;
  const cdr_cancel_info* cancel;
  const cdr_signal_info* signal;
  cdr_standby_result* res;
  int64_t now, delay;
  uint32_t n_req, n_states;
};

// what the activity timer pick reads of a row (cdr_internal::act_first_timer's fields)
struct timer_regs {
  int64_t schedule_id, scheduled_time, started_id, started_time, last_heartbeat_time, expiration_time;
  int32_t s2s, s2c, stc, hb;
  uint32_t flags;
};
__device__ __forceinline__ void load_timer_regs(timer_regs& r, const cdr_activity_info* p) {
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
  r.flags = p->flags;
}

// now.Sub(t): the difference saturates (time.Time.Sub)
__device__ __forceinline__ int64_t time_sub(int64_t now, int64_t t) {
  int64_t d;
  if (__builtin_sub_overflow(now, t, &d)) return now < t ? INT64_MIN : INT64_MAX;
  return d;
}

__device__ __forceinline__ void write_result(cdr_standby_result* dst, const cdr_standby_task& q, int32_t action,
                                             int32_t reason, int32_t code, int64_t next, int64_t lwv,
                                             uint32_t flags = 0, uint32_t act_row = CDR_SB_NO_ROW,
                                             uint32_t task_row = CDR_SB_NO_ROW, int32_t push_timeout = 0,
                                             bool has_task = false, head task = head{0, 0, 0, CDR_SYNC_NO_ROW},
                                             int32_t task_attempt = 0) {
  cdr_standby_result r;
  r.action = action;
  r.reason = reason;
  r.code = code;
  r.flags = flags;
  r.next_event_id = next;
  r.last_write_version = lwv;
  r.act_row = act_row;
  r.task_row = task_row;
  r.push_timeout_s = push_timeout;
  r.task_list = (action == CDR_SB_PUSH_ACTIVITY || action == CDR_SB_PUSH_DECISION) ? q.task.task_list : 0u;
  r.tag = q.tag;
  r._pad = 0;
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

// the types process() answers before it loads a state (timerQueueStandbyProcessor.go:184-224,
// transferQueueStandbyProcessor.go:149-203, and processDecisionTimeout's first test :384-386);
// false when the task needs the state
__device__ __forceinline__ bool stateless(const cdr_task& t, int32_t* action, int32_t* reason) {
  const uint32_t ty = t.type;
  *action = CDR_SB_DONE;
  if (ty == TT_ACTIVITY_RETRY_TIMER) *reason = CDR_SBR_RETRY_TIMER;
  else if (ty == TT_RESET_WORKFLOW) *reason = CDR_SBR_RESET_WORKFLOW;
  else if (ty == CDR_TT_DECISION_TIMEOUT && t.timeout_type == CDR_TIMEOUT_SCHEDULE_TO_START)
    *reason = CDR_SBR_DECISION_S2S;
  else if (ty == CDR_TT_DELETE_HISTORY) *action = CDR_SB_HOST, *reason = CDR_SBR_DELETE_HISTORY;
  else if (ty > CDR_TT_UPSERT_SA && ty < CDR_TT_DECISION_TIMEOUT)
    *action = CDR_SB_E_TASK_TYPE, *reason = CDR_SBR_UNKNOWN_TRANSFER;
  else if (ty > CDR_TT_WORKFLOW_BACKOFF) *action = CDR_SB_E_TASK_TYPE, *reason = CDR_SBR_UNKNOWN_TIMER;
  else return false;
  return true;
}

// GetActivityInfo / GetChildExecutionInfo / GetRequestCancelInfo / GetSignalInfo: the index of
// the row of rows[0, n) whose key is `key`, or CDR_SB_NO_ROW; the same in every lane of the group
template <int G, class Row, class KeyOf>
__device__ __forceinline__ uint32_t group_find(const Row* rows, uint32_t n, uint32_t g, int64_t key, KeyOf key_of) {
  uint64_t found = ~0ull;
  const uint32_t chunks = (n + G - 1) / G;
#pragma unroll 1
  for (uint32_t c = 0; c < chunks; c++) {
    const uint32_t row = c * G + g;
    if (row < n && key_of(rows[row]) == key && (uint64_t)row < found) found = row;
  }
  found = group_min<G>(found);
  return found == ~0ull ? CDR_SB_NO_ROW : (uint32_t)found;
}

// G lanes per state, BLOCK / G states per workgroup; after the states' groups, one lane per
// request of the trailing group (wf < 0 or wf >= n_states)
template <int G>
__global__ __launch_bounds__(BLOCK) void k_standby_tasks(const standby_args A) {
  const uint64_t tid = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  const uint64_t grp = tid / G;
  const uint32_t g = (uint32_t)(tid % G);
  const uint64_t state_blocks = ((uint64_t)A.n_states * G + BLOCK - 1) / BLOCK;
  if (blockIdx.x >= state_blocks) {  // the trailing group
    const uint64_t first = A.req_off[A.n_states] < A.n_req ? A.req_off[A.n_states] : A.n_req;
    const uint64_t i = first + (tid - state_blocks * BLOCK);
    if (i >= A.n_req) return;
    const cdr_standby_task q = A.reqs[i];
    int32_t action, reason;
    if (q.wf >= 0) action = CDR_SB_E_STATE, reason = CDR_SBR_BAD_STATE;
    else if (!stateless(q.task, &action, &reason)) action = CDR_SB_DONE, reason = CDR_SBR_NO_WORKFLOW;
    write_result(&A.res[i], q, action, reason, CDR_OK, 0, 0);
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
      write_result(&A.res[i], A.reqs[i], CDR_SB_E_STATE, CDR_SBR_BAD_STATE, CDR_OK, 0, 0);
    return;
  }
  const cdr_wf_caps& cp = A.caps[s];
  const cdr_exec_info& x = A.exec[s];
  const int32_t wstate = x.state;
  const int64_t next = x.next_event_id;
  const int64_t dec_sched = x.decision_schedule_id, dec_version = x.decision_version;
  const bool running = wstate == CDR_STATE_CREATED || wstate == CDR_STATE_RUNNING;
  const bool known = running || wstate == CDR_STATE_COMPLETED || wstate == CDR_STATE_ZOMBIE;
  // GetLastWriteVersion / GetStartVersion (mutableStateBuilder.go:504-545)
  const cdr_repl_state& rs = A.repl[s];
  const bool is2dc = rs.present != 0;
  const bool isNdc = !is2dc && ((x.flags & CDR_XI_VH_BRANCH) != 0 || wr.n_vh != 0);
  const uint32_t n_vh = wr.n_vh < cp.vh_cap ? wr.n_vh : cp.vh_cap;
  const bool ver_err = isNdc && n_vh == 0;
  int64_t lwv = CDR_EMPTY_VERSION, start_version = CDR_EMPTY_VERSION;
  if (is2dc) {
    lwv = rs.last_write_version;
    start_version = rs.start_version;
  } else if (isNdc && n_vh != 0) {
    lwv = A.vh[cp.vh_off + n_vh - 1].version;
    start_version = A.vh[cp.vh_off].version;
  }
  const uint64_t act_off = cp.act_off;
  const uint32_t n_act = wr.n_activity < cp.act_cap ? wr.n_activity : cp.act_cap;
  cdr_activity_info* const act = A.act + act_off;
  const uint32_t chunks = (n_act + G - 1) / G;

#pragma unroll 1
  for (uint32_t i = r0; i < r1; i++) {
    const cdr_standby_task q = A.reqs[i];
    cdr_standby_result* const out = &A.res[i];
    const uint32_t ty = q.task.type;
    const int64_t eid = q.task.event_id, vis = q.task.visibility_ts;
    const bool global = (q.flags & CDR_SBT_GLOBAL_DOMAIN) != 0;
    int32_t action, reason;
    if (stateless(q.task, &action, &reason)) {
      if (g == 0) write_result(out, q, action, reason, CDR_OK, 0, 0);
      continue;
    }
    // ---- the load (xdcUtil.go:95-169) and the running gate
    const bool dec_retry =
        (ty == CDR_TT_DECISION_TIMEOUT || ty == CDR_TT_DECISION) && dec_sched == eid && x.decision_attempt > 0;
    int32_t code = CDR_OK;
    action = -1;
    if (eid >= next && !dec_retry) action = CDR_SB_DONE, reason = CDR_SBR_STALE_EVENT_ID;
    else if (!known) action = CDR_SB_E_STATE, reason = CDR_SBR_E_WF_STATE, code = CDR_P_UNKNOWN_WF_STATE;
    else if (!running && ty != CDR_TT_CLOSE_EXECUTION) action = CDR_SB_DONE, reason = CDR_SBR_NOT_RUNNING;
    if (action >= 0) {
      if (g == 0) write_result(out, q, action, reason, code, next, lwv);
      continue;
    }
    // a pending entity: ErrTaskRetry, or the discardTask exit
    const bool discard = time_sub(A.now, vis) > (int64_t)(3ull * (uint64_t)A.delay);
    const int32_t pending =
        !discard ? CDR_SB_RETRY : (q.flags & CDR_SBT_LAST_ATTEMPT) ? CDR_SB_DISCARDED : CDR_SB_FETCH;
    const bool push = time_sub(A.now, vis) > A.delay;  // pushToMatching
    int32_t push_timeout = 0;
    // verifyTaskVersion against `version` (xdcUtil.go:71-91)
    auto verified = [&](int64_t version) { return !global || version == q.task.version; };
    action = CDR_SB_DONE;
    switch (ty) {
      case CDR_TT_USER_TIMER: {  // processExpiredUserTimer :227-276
        const uint32_t n = wr.n_timer < cp.timer_cap ? wr.n_timer : cp.timer_cap;
        const cdr_timer_info* rows = A.timer + cp.timer_off;
        uint64_t m = ~0ull;  // expiry with the sign bit flipped: unsigned order is signed order
        const uint32_t tchunks = (n + G - 1) / G;
        for (uint32_t c = 0; c < tchunks; c++) {
          const uint32_t row = c * G + g;
          if (row >= n) continue;
          const uint64_t e = (uint64_t)rows[row].expiry_time ^ (1ull << 63);
          m = e < m ? e : m;
        }
        m = group_min<G>(m);
        const bool expired = n != 0 && cdr_internal::unix_seconds((int64_t)(m ^ (1ull << 63))) <=
                                           cdr_internal::unix_seconds(vis);
        reason = expired ? CDR_SBR_USER_TIMER_PENDING : CDR_SBR_USER_TIMER_NONE;
        if (expired) action = pending;
        break;
      }
      case CDR_TT_ACTIVITY_TIMEOUT: {  // processActivityTimeout :278-374
        const bool is_hb = q.task.timeout_type == CDR_TIMEOUT_HEARTBEAT;
        // The head of the activity timers, smallest (time, schedule id, order), as three min
        // reductions of plain 64-bit keys (sign bit flipped: unsigned order is signed order) and
        // one lookup — the earliest expiry over the rows, the smallest schedule id among the rows
        // that expire then, that row.  A lane accumulates one scalar per pass; it never selects
        // between whole records of its rows (DESIGN, the sync section's open point).
        constexpr uint64_t SIGN = 1ull << 63;
        uint64_t any = ~0ull, tmin = ~0ull;
        for (uint32_t c = 0; c < chunks; c++) {
          const uint32_t row = c * G + g;
          if (row >= n_act) continue;
          timer_regs a;
          load_timer_regs(a, &act[row]);
          if (a.schedule_id == CDR_EMPTY_EVENT_ID) continue;
          const uint64_t t = (uint64_t)cdr_internal::act_earliest_expiry(a) ^ SIGN;
          tmin = t < tmin ? t : tmin;
          any = 0;
        }
        any = group_min<G>(any);
        tmin = group_min<G>(tmin);
        head h;
        h.t = (int64_t)(tmin ^ SIGN), h.sched = 0, h.info = 0, h.row = CDR_SYNC_NO_ROW;
        if (any == 0) {
          uint64_t smin = ~0ull;
          for (uint32_t c = 0; c < chunks; c++) {
            const uint32_t row = c * G + g;
            if (row >= n_act) continue;
            timer_regs a;
            load_timer_regs(a, &act[row]);
            if (a.schedule_id == CDR_EMPTY_EVENT_ID || cdr_internal::act_earliest_expiry(a) != h.t) continue;
            const uint64_t k = (uint64_t)a.schedule_id ^ SIGN;
            smin = k < smin ? k : smin;
          }
          smin = group_min<G>(smin);
          h.sched = (int64_t)(smin ^ SIGN);
          h.row = group_find<G>(act, n_act, g, h.sched, [](const cdr_activity_info& r) { return r.schedule_id; });
        }
        // GetActivityInfo(task.EventID) for a heartbeat task (:341-342)
        uint64_t hb_row = ~0ull;
        if (is_hb) {
          const uint32_t r = group_find<G>(act, n_act, g, eid, [](const cdr_activity_info& x) { return x.schedule_id; });
          if (r != CDR_SB_NO_ROW) hb_row = r;
        }
        if (h.row != CDR_SYNC_NO_ROW) {  // the head row's lane reads its status — whether the first timer's
                                         // task exists once :341-348 has cleared the bit — and tells the group
          uint64_t info = ~0ull;
          if (h.row % G == g) {
            timer_regs a;
            load_timer_regs(a, &act[h.row]);
            int32_t status = act[h.row].timer_task_status;
            if (hb_row == h.row) status &= ~CDR_TTS_HEARTBEAT;
            const cdr_internal::act_timer ct = cdr_internal::act_first_timer(a);
            const bool created = (status & cdr_internal::act_timer_bit(ct.type)) != 0;
            info = ((uint32_t)ct.order << 4) | ((uint32_t)ct.type << 1) | (created ? 1u : 0u);
          }
          h.info = (uint32_t)group_min<G>(info);
        }
        // the head's time is the earliest expiry of all (cdr_internal::act_earliest_expiry)
        if (h.row != CDR_SYNC_NO_ROW && cdr_internal::unix_seconds(h.t) <= cdr_internal::unix_seconds(vis)) {
          action = pending, reason = CDR_SBR_ACT_TIMER_PENDING;
          break;
        }
        if (ver_err) {  // GetLastWriteVersion :337-340
          action = CDR_SB_E_STATE, reason = CDR_SBR_E_LAST_WRITE_VERSION, code = CDR_E_VH_EMPTY;
          break;
        }
        const bool cleared = hb_row != ~0ull;
        const bool emit = h.row != CDR_SYNC_NO_ROW && !(h.info & 1u);  // firstActivityTimerTask
        if (!cleared && !emit) {
          reason = CDR_SBR_ACT_TIMER_NO_UPDATE;
          break;
        }
        // the rows' owning lanes write them: the cleared bit first, then the pick's
        if (cleared && (uint32_t)hb_row % G == g) act[hb_row].timer_task_status &= ~CDR_TTS_HEARTBEAT;
        if (emit && h.row % G == g)
          act[h.row].timer_task_status |= cdr_internal::act_timer_bit((int32_t)((h.info >> 1) & 7u));
        if (g == 0)
          write_result(out, q, CDR_SB_UPDATED, CDR_SBR_ACT_TIMER_UPDATED, CDR_OK, next, lwv,
                       (cleared ? CDR_SB_STATE_UPDATED : 0u) | (emit ? CDR_SB_HAS_TIMER_TASK : 0u),
                       cleared ? (uint32_t)(act_off + hb_row) : CDR_SB_NO_ROW,
                       emit ? (uint32_t)(act_off + h.row) : CDR_SB_NO_ROW, 0, emit, h,
                       emit ? act[h.row].attempt : 0);
        continue;
      }
      case CDR_TT_DECISION_TIMEOUT:  // processDecisionTimeout :376-427 (GetDecisionInfo,
                                     // mutableStateDecisionTaskManager.go:736-744)
        if (dec_sched != eid) reason = CDR_SBR_DECISION_GONE;
        else if (!verified(dec_version)) reason = CDR_SBR_DECISION_VERSION;
        else action = pending, reason = CDR_SBR_DECISION_PENDING;
        break;
      case CDR_TT_WORKFLOW_BACKOFF:  // processWorkflowBackoffTimer :429-473
        if (dec_sched != CDR_EMPTY_EVENT_ID || x.last_processed_event != CDR_EMPTY_EVENT_ID)
          reason = CDR_SBR_BACKOFF_DECIDED;
        else action = pending, reason = CDR_SBR_BACKOFF_PENDING;
        break;
      case CDR_TT_WORKFLOW_TIMEOUT:  // processWorkflowTimeout :475-513
        if (ver_err) action = CDR_SB_E_STATE, reason = CDR_SBR_E_START_VERSION, code = CDR_E_VH_EMPTY;
        else if (!verified(start_version)) reason = CDR_SBR_WF_TIMEOUT_VERSION;
        else action = pending, reason = CDR_SBR_WF_TIMEOUT_PENDING;
        break;
      case CDR_TT_ACTIVITY: {  // processActivityTask :206-246
        const uint32_t row =
            group_find<G>(act, n_act, g, eid, [](const cdr_activity_info& a) { return a.schedule_id; });
        if (row == CDR_SB_NO_ROW) reason = CDR_SBR_XACT_GONE;
        else if (!verified(act[row].version)) reason = CDR_SBR_XACT_VERSION;
        else if (act[row].started_id != CDR_EMPTY_EVENT_ID) reason = CDR_SBR_XACT_STARTED;
        else {
          reason = CDR_SBR_XACT_PENDING;
          action = push ? CDR_SB_PUSH_ACTIVITY : CDR_SB_RETRY;
          const int32_t s2s = act[row].s2s;
          if (push) push_timeout = s2s < CDR_MAX_TASK_TIMEOUT ? s2s : CDR_MAX_TASK_TIMEOUT;
        }
        break;
      }
      case CDR_TT_DECISION:  // processDecisionTask :248-295
        if (dec_sched != eid) reason = CDR_SBR_XDEC_GONE;
        else if (!verified(dec_version)) reason = CDR_SBR_XDEC_VERSION;
        else if (x.decision_started_id != CDR_EMPTY_EVENT_ID) reason = CDR_SBR_XDEC_STARTED;
        else {
          reason = CDR_SBR_XDEC_PENDING;
          action = push ? CDR_SB_PUSH_DECISION : CDR_SB_RETRY;
          if (push) push_timeout = x.workflow_timeout < CDR_MAX_TASK_TIMEOUT ? x.workflow_timeout : CDR_MAX_TASK_TIMEOUT;
        }
        break;
      case CDR_TT_CLOSE_EXECUTION:  // processCloseExecution :297-361
        if (running) reason = CDR_SBR_CLOSE_RUNNING;
        else if (ver_err) action = CDR_SB_E_STATE, reason = CDR_SBR_E_LAST_WRITE_VERSION, code = CDR_E_VH_EMPTY;
        else if (!verified(lwv)) reason = CDR_SBR_CLOSE_VERSION;
        else action = CDR_SB_RECORD_CLOSED, reason = CDR_SBR_CLOSE_RECORD;
        break;
      case CDR_TT_CANCEL_EXECUTION: {  // processCancelExecution :363-400
        const cdr_cancel_info* rows = A.cancel + cp.cancel_off;
        const uint32_t n = wr.n_cancel < cp.cancel_cap ? wr.n_cancel : cp.cancel_cap;
        const uint32_t row = group_find<G>(rows, n, g, eid, [](const cdr_cancel_info& r) { return r.initiated_id; });
        if (row == CDR_SB_NO_ROW) reason = CDR_SBR_CANCEL_GONE;
        else if (!verified(rows[row].version)) reason = CDR_SBR_CANCEL_VERSION;
        else action = pending, reason = CDR_SBR_CANCEL_PENDING;
        break;
      }
      case CDR_TT_SIGNAL_EXECUTION: {  // processSignalExecution :402-439
        const cdr_signal_info* rows = A.signal + cp.signal_off;
        const uint32_t n = wr.n_signal < cp.signal_cap ? wr.n_signal : cp.signal_cap;
        const uint32_t row = group_find<G>(rows, n, g, eid, [](const cdr_signal_info& r) { return r.initiated_id; });
        if (row == CDR_SB_NO_ROW) reason = CDR_SBR_SIGNAL_GONE;
        else if (!verified(rows[row].version)) reason = CDR_SBR_SIGNAL_VERSION;
        else action = pending, reason = CDR_SBR_SIGNAL_PENDING;
        break;
      }
      case CDR_TT_START_CHILD: {  // processStartChildExecution :441-482
        const cdr_child_info* rows = A.child + cp.child_off;
        const uint32_t n = wr.n_child < cp.child_cap ? wr.n_child : cp.child_cap;
        const uint32_t row = group_find<G>(rows, n, g, eid, [](const cdr_child_info& r) { return r.initiated_id; });
        if (row == CDR_SB_NO_ROW) reason = CDR_SBR_CHILD_GONE;
        else if (!verified(rows[row].version)) reason = CDR_SBR_CHILD_VERSION;
        else if (rows[row].started_id != CDR_EMPTY_EVENT_ID) reason = CDR_SBR_CHILD_STARTED;
        else action = pending, reason = CDR_SBR_CHILD_PENDING;
        break;
      }
      case CDR_TT_RECORD_STARTED:  // processRecordWorkflowStartedOrUpsertHelper :506-550
        if (ver_err) action = CDR_SB_E_STATE, reason = CDR_SBR_E_START_VERSION, code = CDR_E_VH_EMPTY;
        else if (!verified(start_version)) reason = CDR_SBR_STARTED_VERSION;
        else action = CDR_SB_RECORD_STARTED, reason = CDR_SBR_STARTED_RECORD;
        break;
      default:  // CDR_TT_UPSERT_SA: no version check (:512-513)
        action = CDR_SB_UPSERT, reason = CDR_SBR_UPSERT_RECORD;
        break;
    }
    if (g == 0)
      write_result(out, q, action, reason, code, next, lwv, 0, CDR_SB_NO_ROW, CDR_SB_NO_ROW, push_timeout);
  }
}

template <int G>
void launch(const standby_args& A, hipStream_t st) {
  const uint64_t state_blocks = ((uint64_t)A.n_states * G + BLOCK - 1) / BLOCK;
  // the trailing group's size lives in device memory (req_off[n_states]): one lane per request
  // covers it whatever it is
  const uint64_t trail_blocks = ((uint64_t)A.n_req + BLOCK - 1) / BLOCK;
  hipLaunchKernelGGL(k_standby_tasks<G>, dim3((uint32_t)(state_blocks + trail_blocks)), dim3(BLOCK), 0, st, A);
}

bool args_ok(const cdr_ctx* ctx, const void* reqs, const void* req_off, const void* caps, const cdr_out* state,
             const cdr_cluster_meta* cluster, int64_t delay, const void* res) {
  return ctx && reqs && req_off && caps && state && cluster && res && delay > 0 && state->result && state->exec &&
         state->repl && state->vh && state->act && state->timer && state->child && state->cancel && state->signal;
}

}  // namespace

extern "C" {

int cdr_set_standby_group(cdr_ctx* ctx, int lanes) {
  if (!ctx || (lanes != 4 && lanes != 8 && lanes != 16 && lanes != 64)) return CDR_API_EINVAL;
  const int prev = ctx->standby_group;
  ctx->standby_group = lanes;
  return prev;
}

int cdr_standby_tasks_async(cdr_ctx* ctx, const cdr_standby_task* reqs, const uint32_t* req_off, uint32_t n_req,
                            uint32_t n_states, const cdr_wf_caps* state_caps, const cdr_out* state,
                            const cdr_cluster_meta* cluster, int64_t now_ns, int64_t standby_delay_ns,
                            cdr_standby_result* res, void* stream) {
  if (!args_ok(ctx, reqs, req_off, state_caps, state, cluster, standby_delay_ns, res)) return CDR_API_EINVAL;
  if (n_req == 0) return CDR_API_OK;
  standby_args A{};
  A.reqs = reqs;
  A.req_off = req_off;
  A.caps = state_caps;
  A.result = state->result;
  A.exec = state->exec;
  A.repl = state->repl;
  A.vh = state->vh;
  A.act = state->act;
  A.timer = state->timer;
  A.child = state->child;
  A.cancel = state->cancel;
  A.signal = state->signal;
  A.res = res;
  A.now = now_ns;
  A.delay = standby_delay_ns;
  A.n_req = n_req;
  A.n_states = n_states;
  hipStream_t st = (hipStream_t)stream;
  switch (ctx->standby_group) {
    case 4: launch<4>(A, st); break;
    case 8: launch<8>(A, st); break;
    case 16: launch<16>(A, st); break;
    case 64: launch<64>(A, st); break;
    default: launch<CDR_STANDBY_GROUP>(A, st); break;
  }
  HIPCHK(hipGetLastError());
  return CDR_API_OK;
}

int cdr_standby_tasks_batch(cdr_ctx* ctx, const cdr_standby_task* reqs, const uint32_t* req_off, uint32_t n_req,
                            uint32_t n_states, const cdr_wf_caps* state_caps, const cdr_totals* tot,
                            const cdr_out* state, const cdr_cluster_meta* cluster, int64_t now_ns,
                            int64_t standby_delay_ns, cdr_standby_result* res, void* stream) {
  if (!tot || !args_ok(ctx, reqs, req_off, state_caps, state, cluster, standby_delay_ns, res)) return CDR_API_EINVAL;
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
  const cdr_standby_task* d_reqs = (const cdr_standby_task*)up(WS_SB_REQ, reqs, (uint64_t)n_req * sizeof(*reqs));
  const uint32_t* d_off = (const uint32_t*)up(WS_SB_OFF, req_off, (ns + 1) * 4);
  cdr_standby_result* d_res = (cdr_standby_result*)up(WS_SB_RES, nullptr, (uint64_t)n_req * sizeof(*res));
  const cdr_wf_caps* d_caps = (const cdr_wf_caps*)up(WS_CY_CAPS, state_caps, ns * sizeof(cdr_wf_caps));
  cdr_out ds{};
  ds.result = (cdr_wf_result*)up(WS_CY_RESULT, state->result, ns * sizeof(cdr_wf_result));
  ds.exec = (cdr_exec_info*)up(WS_CY_EXEC, state->exec, ns * sizeof(cdr_exec_info));
  ds.repl = (cdr_repl_state*)up(WS_CY_REPL, state->repl, ns * sizeof(cdr_repl_state));
  ds.vh = (cdr_vh_item*)up(WS_CY_VH, state->vh, tot->vh * sizeof(cdr_vh_item));
  ds.act = (cdr_activity_info*)up(WS_CY_ACT, state->act, tot->act * sizeof(cdr_activity_info));
  ds.timer = (cdr_timer_info*)up(WS_CY_TIMER, state->timer, tot->timer * sizeof(cdr_timer_info));
  ds.child = (cdr_child_info*)up(WS_CY_CHILD, state->child, tot->child * sizeof(cdr_child_info));
  ds.cancel = (cdr_cancel_info*)up(WS_CY_CANCEL, state->cancel, tot->cancel * sizeof(cdr_cancel_info));
  ds.signal = (cdr_signal_info*)up(WS_CY_SIGNAL, state->signal, tot->signal * sizeof(cdr_signal_info));
  if (oom || dev_err) {
    (void)hipStreamSynchronize(st);
    return oom ? CDR_API_ENOMEM : CDR_API_EDEVICE;
  }
  int rc = cdr_standby_tasks_async(ctx, d_reqs, d_off, n_req, n_states, d_caps, &ds, cluster, now_ns,
                                   standby_delay_ns, d_res, st);
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
