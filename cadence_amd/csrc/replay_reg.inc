// replay_reg.inc — lane-per-workflow replay with register-resident entity tables
// (included by replay.hip; semantics are k_replay's, event for event).
//
// Why a third lane kernel.  Divergent histories (SURVEY §8(d) C3-C5: timers, signals,
// children, interleaved decisions) keep a handful of pending activities and user timers
// live at every step, and every activity / timer event runs a pick over all of them
// (timerBuilder.go:171-312).  The general kernel keeps those working sets in LDS (one
// activity, four timers) or, beyond that, in a global scratch it scans per event: on
// C3 that is ~190 dependent global loads and ~2,300 VALU per step, 77% of the wave
// cycles waiting on memory (profiles/r2_c3_lanes_pmc.txt).
//
// Here the per-lane tables live in VGPRs — a slot is an unrolled register array
// element, a lookup is NA/NT compares and selects, a pick is one pass of selects — and
// everything that is only needed to build the output rows (event indices of the
// scheduling / start / cancel events, the pending children's initiating events, new
// reset points, search attributes, 2DC LastReplicationInfo) lives in LDS, lane-
// interleaved (plane p of lane L at 4-byte word p*64 + L: conflict-free).  The rows
// are written once, after the loop, from those indices (their fields are the events'
// own columns, gathered from the slab).  So the step loop touches global memory only
// for the event stream (prefetched one step ahead) and for rare events (Started,
// a new version-history item, upserts, continue-as-new), each followed by a
// vmcnt drain so the prefetch bookkeeping stays exact.
//
// Handlers are grouped; a group runs when any lane's event is in it (one ballot), and
// inside it per-lane effects are selects (wave-uniform control flow).

#ifndef CDR_WPE_REG
#define CDR_WPE_REG 1
#endif

namespace {

constexpr uint32_t RNONE = 0xFFFFFFFFu;  // "no event" index
constexpr uint32_t RA_W = 7;  // per activity slot: ts2c lo, hi, stc, hb, sched (k | (k - call first) << 20), started k, cancel k
// LDS planes (4-byte words) of the register-table kernel with NA activity, NT timer and
// NX child / request-cancel / signal slots per lane
template <int NA, int NT, int NX>
struct RegLds {
  static constexpr uint32_t A0 = 0;
  static constexpr uint32_t T0 = A0 + RA_W * NA;           // per timer slot: TimerStarted event index
  static constexpr uint32_t C0 = T0 + NT;                  // per child slot: initiated (k | dcf << 20), started k
  static constexpr uint32_t R0 = C0 + 2 * NX;              // per request-cancel slot: initiated
  static constexpr uint32_t G0 = R0 + NX;                  // per signal slot: initiated
  static constexpr uint32_t P0 = G0 + NX;                  // reset points: checksum, k | resettable << 31 (RNONE: Started row)
  static constexpr uint32_t NRP = CDR_REG_NRP_OF(NA);
  static constexpr uint32_t L0 = P0 + 2 * NRP;             // 2DC LastReplicationInfo per cluster: version, event id
  // (both < 2^31 under CDR_CAP_REG); search attributes go straight to their output rows
  // (Started / Upsert only, drained after).  LDS per wave sets this kernel's occupancy:
  // 160 KB per CU / (W x 256 B) — the <6,10,4> variant's 88 words give 7 waves per CU
  static constexpr uint32_t W = L0 + 2 * CDR_REG_NCL;
  static constexpr size_t bytes = (size_t)W * CDR_SLICE_WIDTH * 4;
};

__device__ __forceinline__ uint32_t rl(uint32_t p, uint32_t lane) {
  return ((const uint32_t*)cdr_lds)[p * CDR_SLICE_WIDTH + lane];
}
__device__ __forceinline__ void rs(uint32_t p, uint32_t lane, uint32_t v) {
  ((uint32_t*)cdr_lds)[p * CDR_SLICE_WIDTH + lane] = v;
}
__device__ __forceinline__ uint32_t bitof(int j) { return j >= 0 ? 1u << j : 0u; }
__device__ __forceinline__ void vmdrain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

}  // namespace

// per-type masks of the handler groups
#define RG_SIMPLE                                                                                         \
  (CDR_TB(CDR_EV_DT_SCHEDULED) | CDR_TB(CDR_EV_DT_STARTED) | CDR_TB(CDR_EV_WF_SIGNALED) |                 \
   CDR_TB(CDR_EV_WF_CANCEL_REQUESTED) | CDR_TB(CDR_EV_MARKER_RECORDED) | CDR_TB(CDR_EV_CANCEL_TIMER_FAILED) | \
   CDR_TB(CDR_EV_AT_REQ_CANCEL_FAILED))
#define RG_ACT                                                                                                \
  (CDR_TB(CDR_EV_AT_SCHEDULED) | CDR_TB(CDR_EV_AT_STARTED) | CDR_TB(CDR_EV_AT_COMPLETED) |                    \
   CDR_TB(CDR_EV_AT_FAILED) | CDR_TB(CDR_EV_AT_TIMED_OUT) | CDR_TB(CDR_EV_AT_CANCELED) |                      \
   CDR_TB(CDR_EV_AT_CANCEL_REQUESTED))
#define RG_ACT_CLOSE \
  (CDR_TB(CDR_EV_AT_COMPLETED) | CDR_TB(CDR_EV_AT_FAILED) | CDR_TB(CDR_EV_AT_TIMED_OUT) | CDR_TB(CDR_EV_AT_CANCELED))
#define RG_TIM (CDR_TB(CDR_EV_TIMER_STARTED) | CDR_TB(CDR_EV_TIMER_FIRED) | CDR_TB(CDR_EV_TIMER_CANCELED))
#define RG_CHILD_CLOSE                                                                                       \
  (CDR_TB(CDR_EV_CHILD_START_FAILED) | CDR_TB(CDR_EV_CHILD_COMPLETED) | CDR_TB(CDR_EV_CHILD_FAILED) |         \
   CDR_TB(CDR_EV_CHILD_CANCELED) | CDR_TB(CDR_EV_CHILD_TIMED_OUT) | CDR_TB(CDR_EV_CHILD_TERMINATED))
#define RG_EXT                                                                                                 \
  (CDR_TB(CDR_EV_CHILD_INITIATED) | CDR_TB(CDR_EV_CHILD_STARTED) | RG_CHILD_CLOSE | CDR_TB(CDR_EV_RCE_INITIATED) | \
   CDR_TB(CDR_EV_RCE_FAILED) | CDR_TB(CDR_EV_EXT_CANCEL_REQUESTED) | CDR_TB(CDR_EV_SE_INITIATED) |             \
   CDR_TB(CDR_EV_SE_FAILED) | CDR_TB(CDR_EV_EXT_SIGNALED))
#define RG_DTFAIL (CDR_TB(CDR_EV_DT_TIMED_OUT) | CDR_TB(CDR_EV_DT_FAILED))
#define RG_CLOSE                                                                                        \
  (CDR_TB(CDR_EV_WF_COMPLETED) | CDR_TB(CDR_EV_WF_FAILED) | CDR_TB(CDR_EV_WF_TIMED_OUT) |               \
   CDR_TB(CDR_EV_WF_CANCELED) | CDR_TB(CDR_EV_WF_TERMINATED))
#define RG_KNOWN ((CDR_TB(CDR_EV_NUM_TYPES) - 1ull))

// unrolled register-array access with a per-lane runtime slot (j < 0: no change)
#define RSET(arr, N, j, v)                            \
  do {                                                \
    _Pragma("unroll") for (int i_ = 0; i_ < (int)(N); i_++) arr[i_] = ((int)(j) == i_) ? (v) : arr[i_]; \
  } while (0)
#define RGET(arr, N, j, out)                          \
  do {                                                \
    out = arr[0];                                     \
    _Pragma("unroll") for (int i_ = 1; i_ < (int)(N); i_++) out = ((int)(j) == i_) ? arr[i_] : out; \
  } while (0)

// one slice (the body of k_replay_reg).  CARRY: the instantiation that also replays onto a
// loaded state (cdr_carry, mutableStateBuilder.Load mutableStateBuilder.go:272-295, then
// applyEvents, nDCHistoryReplicator.go:330-398): the loaded records fill the registers, the
// tables and the LDS planes in the prologue (a loaded row is named by its row index and a
// carried bit, re-read at emission for the fields the replay does not change).  A loaded
// state or a replay that outgrows this variant's tables (or its 31-bit id / 2DC cluster
// envelope) is handed on, whole, to the next tier: the entry's code becomes CLS_RETRY
// (the 12-activity variant next) or CLS_RETRY2 (the general kernel next) and its slice is
// listed for that tier's retry pass (KA()->olist)
template <int NA, int NT, int NX, uint32_t SFLAG, bool CARRY = false, bool TASKS = false>
__device__ __forceinline__ void reg_slice(const uint32_t s) {
  typedef RegLds<NA, NT, NX> LY;
  constexpr uint32_t RA0 = LY::A0, RT0 = LY::T0, RC0 = LY::C0, RR0 = LY::R0, RG0 = LY::G0, RP0 = LY::P0,
                     RL0 = LY::L0;
  const uint32_t lane = threadIdx.x;
  if (s >= KA()->B.ev.n_slices) return;
  if (!(__builtin_amdgcn_readfirstlane(KA()->B.ev.slice_flags[s]) & SFLAG)) return;
  const uint64_t row0_ = KA()->B.ev.slice_row0[s];
  const uint64_t row0 = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(row0_ >> 32)) << 32) |
                        __builtin_amdgcn_readfirstlane((uint32_t)row0_);
  Slice S;
  S.elems = __builtin_amdgcn_readfirstlane(KA()->B.ev.slice_len[s]) * CDR_SLICE_WIDTH;
  S.r = __builtin_amdgcn_make_buffer_rsrc((void*)(KA()->B.ev.slab + row0 * CDR_ROW_BYTES), (short)0,
                                          (int)(S.elems * CDR_EL_BYTES), 0x00020000);
  S.l4 = lane * 4u;
  const int32_t w = KA()->B.ev.lane_wf[(uint64_t)s * CDR_SLICE_WIDTH + lane];
  if (w < 0 || (KA()->B.skip && KA()->B.skip[w])) return;  // empty lane / masked entry
  if (KA()->retry && gp(KA()->O.result)[w].code != CLS_RETRY) return;  // after k_replay_cls: its leftovers only
#define B_ (KA()->B)
#define O_ (KA()->O)
#define D (gp(B_.wfs)[w])
#define CP (gp(B_.caps)[w])
#define X (gp(O_.exec) + w)
#define RS (gp(O_.repl) + w)
#define vh (gp(O_.vh) + CP.vh_off)
#define rp (gp(O_.rp) + CP.rp_off)
#define sa (gp(O_.sa) + CP.sa_off)
  const uint32_t len = (uint32_t)D.ev_len;
  const uint32_t builder = D.builder;
  const uint32_t EU = B_.empty_uuid;
  const bool isRS = builder == CDR_BUILDER_2DC;
  const bool isVH = builder == CDR_BUILDER_NDC;

  // ---- registers: workflow state (as k_replay) ...
  uint32_t x_flags = 0, cks_ok = 0;
  int64_t x_completion_batch = 0, x_next_event = CDR_FIRST_EVENT_ID, x_last_processed = CDR_EMPTY_EVENT_ID;
  int32_t x_dt_timeout_value = 0, x_state = CDR_STATE_CREATED, x_close = CDR_CLOSE_NONE, x_signals = 0;
  int64_t dv = CDR_EMPTY_VERSION, dsched = CDR_EMPTY_EVENT_ID, dstart = CDR_EMPTY_EVENT_ID, datt = 0, dst_ts = 0,
          dsc_ts = 0, dorig_ts = 0;
  uint32_t dreq = EU;
  int32_t dto = 0;
  uint32_t ld = 0;  // lastDecision bookkeeping (ld_write)
  const bool want_ld = O_.last_decision != nullptr;
  int64_t curv = D.failover_version;
  uint32_t rs_mask = 0;
  int64_t vh_last_id = 0, vh_last_ver = 0;
  uint32_t n_vh = 0, n_rp = 0, n_sa = 0;
  int64_t call_first_id = 0, prev_id = 0, prev_ver = 0;
  uint32_t call_first_k = 0, call_idx = 0;
  bool newrun_applied = false, stop_at_call_end = false;
  // the call whose continue-as-new applied the new run: a 2DC cluster panic of that call fires at
  // its first event in the reference (mutableStateBuilder.go:561-581 runs before the events),
  // so the new run was never attempted
  uint32_t nr_call = 0xFFFFFFFFu;
  // ---- transfer / timer tasks (stateBuilder.go:613-804; TASKS instantiation only, as the
  // general kernel's k_replay<LDS, true>): appended in generation order to the entry's
  // slices; a step whose lanes stored one drains before the next prefetch use
  uint32_t n_xt = 0, n_tt = 0;
  bool tstored = false, t_over = false;  // t_over: a task past its slice (capacities too small)
  // the task slices' capacities, the entry's DomainID / retention and ExecutionInfo.TaskList
  // in registers: a global load inside the step loop waits for every prefetch before it
  const uint32_t t_xcap = TASKS ? CP.xfer_cap : 0u, t_tcap = TASKS ? CP.ttask_cap : 0u;
  const uint32_t t_dom = TASKS ? D.domain_id : 0u;
  const int64_t t_ret = TASKS ? (int64_t)D.retention_days * 86400ll * NS_PER_S : 0;
  uint32_t t_tl = 0;  // TaskList as set by Started (or loaded)
  auto task_x = [&](bool c, uint32_t type, int64_t eid, uint32_t dom, uint32_t tl, uint32_t twf, uint32_t trun,
                    uint32_t fl) __attribute__((always_inline)) {
    if constexpr (TASKS) {
      t_over |= c && n_xt >= t_xcap;
      c = c && n_xt < t_xcap;
      if (c) {
        cdr_task t;
        t.type = type;
        t.timeout_type = 0;
        t.event_id = eid;
        t.visibility_ts = 0;
        t.attempt = 0;
        t.domain_id = dom;
        t.task_list = tl;
        t.target_workflow_id = twf;
        t.target_run_id = trun;
        t.flags = fl;
        t._pad = 0;
        t.version = 0;  // stateBuilder's tasks leave Version to the caller (schema.h cdr_task)
        gput(gp(O_.transfer) + CP.xfer_off + n_xt, t);
      }
      n_xt += c ? 1u : 0u;
      tstored |= c;
    }
  };
  auto task_t = [&](bool c, uint32_t type, int32_t tt, int64_t eid, int64_t vis, int64_t att)
                    __attribute__((always_inline)) {
    if constexpr (TASKS) {
      t_over |= c && n_tt >= t_tcap;
      c = c && n_tt < t_tcap;
      if (c) {
        cdr_task t;
        t.type = type;
        t.timeout_type = tt;
        t.event_id = eid;
        t.visibility_ts = vis;
        t.attempt = att;
        t.domain_id = t.task_list = t.target_workflow_id = t.target_run_id = t.flags = t._pad = 0;
        t.version = 0;
        gput(gp(O_.timer_tasks) + CP.ttask_off + n_tt, t);
      }
      n_tt += c ? 1u : 0u;
      tstored |= c;
    }
  };
  // ExecutionInfo.TaskList as of now (getTaskList, stateBuilder.go:789-794)
  auto task_list_now = [&]() -> uint32_t { return (x_flags & CDR_XI_STARTED) ? t_tl : 0u; };
  // appendTasksForFinishedExecutions (:775-787)
  auto close_tasks = [&](bool c, int64_t ts) __attribute__((always_inline)) {
    task_x(c, CDR_TT_CLOSE_EXECUTION, 0, 0, 0, 0, 0, 0);
    task_t(c, CDR_TT_DELETE_HISTORY, 0, 0, ts + t_ret, 0);
  };
  int32_t err = len == 0 ? CDR_E_HISTORY_EMPTY : CDR_OK;
  int64_t err_id = 0;
  uint32_t err_k = 0;
  // ... and the entity tables: activities (scheduleID, activityID, earliest timer
  // candidate, candidate order | its TimerTaskStatus bit << 4 | TimerTaskStatus << 8),
  // user timers (timerID, StartedID, ExpiryTime), children / request-cancels / signals
  // (initiated event id); live / byActivityID-holder / started / cancel-requested /
  // TaskID-created as bitmasks
  uint32_t a_sid[NA], a_aid[NA], a_inf[NA];
  int64_t a_t[NA];
  uint32_t t_tid[NT], t_sid[NT];
  int64_t t_exp[NT];
  uint32_t c_id[NX], r_id[NX], g_id[NX];
#pragma unroll
  for (int j = 0; j < NA; j++) {
    a_sid[j] = a_aid[j] = a_inf[j] = 0;
    a_t[j] = 0;
  }
#pragma unroll
  for (int j = 0; j < NT; j++) {
    t_tid[j] = t_sid[j] = 0;
    t_exp[j] = 0;
  }
#pragma unroll
  for (int j = 0; j < NX; j++) c_id[j] = r_id[j] = g_id[j] = 0;
  uint32_t a_live = 0, a_map = 0, a_st = 0, a_cx = 0, t_live = 0, t_cr = 0, c_live = 0, r_live = 0, g_live = 0;
  // carry-in: the slots holding loaded rows (their LDS event-index words hold the row
  // index instead), and the hand-on flag
  uint32_t a_cy = 0, t_cy = 0, c_cy = 0, r_cy = 0, g_cy = 0;
  bool cyr = false;
  const int32_t csrc = (CARRY && B_.carry) ? gp(B_.carry)->src[w] : -1;
  if (CARRY && csrc >= 0) {
    const GAS cdr_carry* CY = gp(B_.carry);
    const cdr_wf_caps cc = gget(gp(CY->caps) + csrc);
    const cdr_wf_result cr = gget(gp(CY->state.result) + csrc);
    cyr = cr.n_activity > (uint32_t)NA || cr.n_timer > (uint32_t)NT || cr.n_child > (uint32_t)NX ||
          cr.n_cancel > (uint32_t)NX || cr.n_signal > (uint32_t)NX || cr.n_reset_points > LY::NRP ||
          cr.n_search_attr > CDR_REG_NSA;
    cdr_repl_state rs0;
    if (isRS) {
      rs0 = gget(gp(CY->state.repl) + csrc);
      cyr |= (rs0.lri_mask >> CDR_REG_NCL) != 0u;  // LastReplicationInfo beyond the kept clusters
#pragma unroll
      for (uint32_t c = 0; c < CDR_REG_NCL; c++)
        cyr |= ((rs0.lri_mask >> c) & 1u) &&
               ((uint64_t)rs0.lri_version[c] >= (1ull << 31) || (uint64_t)rs0.lri_last_event_id[c] >= (1ull << 31));
    }
    auto id31 = [](int64_t v) { return (uint64_t)v < (1ull << 31); };
    if (!cyr) {
      const cdr_exec_info x = gget(gp(CY->state.exec) + csrc);
      gput(X, x);  // the Started half stays as loaded; the replay half is rewritten at the end
      x_flags = x.flags;
      if constexpr (TASKS) t_tl = x.task_list;
      x_completion_batch = x.completion_event_batch_id;
      x_next_event = x.next_event_id;
      x_last_processed = x.last_processed_event;
      x_dt_timeout_value = x.decision_timeout_value;
      x_state = x.state;
      x_close = x.close_status;
      x_signals = x.signal_count;
      dv = x.decision_version;
      dsched = x.decision_schedule_id;
      dstart = x.decision_started_id;
      datt = x.decision_attempt;
      dst_ts = x.decision_started_ts;
      dsc_ts = x.decision_scheduled_ts;
      dorig_ts = x.decision_original_scheduled_ts;
      dreq = x.decision_request_id;
      dto = x.decision_timeout;
      curv = CDR_EMPTY_VERSION;  // Load (:291); an in-memory builder keeps its own (below)
      if (isRS) {
        gput(RS, rs0);
        rs_mask = rs0.lri_mask;
#pragma unroll
        for (uint32_t c = 0; c < CDR_REG_NCL; c++)
          if ((rs_mask >> c) & 1u) {
            rs(RL0 + 2u * c, lane, (uint32_t)rs0.lri_version[c]);
            rs(RL0 + 2u * c + 1, lane, (uint32_t)rs0.lri_last_event_id[c]);
          }
      }
      // reset points (their rows as loaded; the LDS words cache the checksums), search
      // attributes, version-history items (the last one in registers).  The copy loops are
      // wave-uniform (ballot-bounded, the body predicated): a loop whose lanes leave it one
      // by one ends with exec = 0, and the ROCm 7.2 register allocator can place a live-range
      // split copy there, before exec is restored — the copy then writes no lane (it lost the
      // loaded LastReplicationInfo mask: DESIGN.md §3 "Round 6"; tools/isa_execz_lint.py
      // checks every build for such copies)
      n_rp = cr.n_reset_points;
#pragma unroll
      for (uint32_t j = 0; j < LY::NRP; j++)
        if (j < n_rp) {
          const cdr_reset_point p = gget(carry_rp(CY) + cc.rp_off + j);
          gput(rp + j, p);
          rs(RP0 + 2 * j, lane, (p.flags & CDR_RP_HAS_CHECKSUM) ? p.binary_checksum : 0u);
          rs(RP0 + 2 * j + 1, lane, RNONE);
        }
      n_sa = cr.n_search_attr;
#pragma unroll
      for (uint32_t j = 0; j < CDR_REG_NSA; j++)
        if (j < n_sa) gput(sa + j, gget(carry_sa(CY) + cc.sa_off + j));
      if (isVH && cr.n_vh > 0) {
        const uint32_t nv = cr.n_vh;
        for (uint32_t j = 0; __builtin_amdgcn_ballot_w64(j + 1 < nv); j++)
          if (j + 1 < nv) gput(vh + j, gget(carry_vh(CY) + cc.vh_off + j));
        const cdr_vh_item it = gget(carry_vh(CY) + cc.vh_off + cr.n_vh - 1);
        n_vh = cr.n_vh;
        vh_last_id = it.event_id;
        vh_last_ver = it.version;
        // cdr_carry.in_memory: the builder nDCConflictResolver.rebuild hands over never went
        // through Load (nDCConflictResolver.go:117-184): its currentVersion is the last item's
        if (CY->in_memory && CY->in_memory[w]) curv = vh_last_ver;
      }
      // children / request-cancels / signals: the initiated id in registers, the row index in LDS
#pragma unroll
      for (int j = 0; j < NX; j++) {
        if (j < (int)cr.n_child) {
          const int64_t id = gget(gp(CY->state.child) + cc.child_off + j).initiated_id;
          cyr |= !id31(id);
          c_id[j] = (uint32_t)id;
          rs(RC0 + 2 * (uint32_t)j, lane, (uint32_t)j);
          rs(RC0 + 2 * (uint32_t)j + 1, lane, RNONE);
        }
        if (j < (int)cr.n_cancel) {
          const int64_t id = gget(gp(CY->state.cancel) + cc.cancel_off + j).initiated_id;
          cyr |= !id31(id);
          r_id[j] = (uint32_t)id;
          rs(RR0 + (uint32_t)j, lane, (uint32_t)j);
        }
        if (j < (int)cr.n_signal) {
          const int64_t id = gget(gp(CY->state.signal) + cc.signal_off + j).initiated_id;
          cyr |= !id31(id);
          g_id[j] = (uint32_t)id;
          rs(RG0 + (uint32_t)j, lane, (uint32_t)j);
        }
      }
      c_live = c_cy = (1u << cr.n_child) - 1u;
      r_live = r_cy = (1u << cr.n_cancel) - 1u;
      g_live = g_cy = (1u << cr.n_signal) - 1u;
      // user timers: every field but Version in registers
#pragma unroll
      for (int j = 0; j < NT; j++)
        if (j < (int)cr.n_timer) {
          const cdr_timer_info t = gget(gp(CY->state.timer) + cc.timer_off + j);
          cyr |= !id31(t.started_id) || (uint64_t)t.task_id > CDR_TIMER_TASK_STATUS_CREATED;
          t_tid[j] = t.timer_id;
          t_sid[j] = (uint32_t)t.started_id;
          t_exp[j] = t.expiry_time;
          t_cr |= t.task_id == CDR_TIMER_TASK_STATUS_CREATED ? 1u << j : 0u;
          rs(RT0 + (uint32_t)j, lane, (uint32_t)j);
        }
      t_live = t_cy = (1u << cr.n_timer) - 1u;
      // activities: the earliest timer candidate recomputed from the loaded times
      // (loadActivityTimers, timerBuilder.go:249-312), as the general kernel's carry-in does
#pragma unroll
      for (int j = 0; j < NA; j++)
        if (j < (int)cr.n_activity) {
          const cdr_activity_info a = gget(gp(CY->state.act) + cc.act_off + j);
          cyr |= !id31(a.schedule_id);
          const bool started = a.started_id != CDR_EMPTY_EVENT_ID;
          const int64_t s2c = a.scheduled_time + (int64_t)a.s2c * NS_PER_S;
          const bool tset = (a.flags & CDR_AI_STARTED_TIME_SET) != 0;
          const int64_t st = tset ? a.started_time : 0, hb0 = tset ? a.last_heartbeat_time : 0;
          const int64_t lhb = hb0 > st ? hb0 : st;
          const int64_t t0 = a.expiration_time < s2c ? a.expiration_time : s2c;
          const int64_t ta = started ? st + (int64_t)a.stc * NS_PER_S : a.scheduled_time + (int64_t)a.s2s * NS_PER_S;
          const int64_t th = started && a.hb > 0 ? lhb + (int64_t)a.hb * NS_PER_S : T_NONE;
          const bool pa = ta < t0;  // append order breaks ties: S2C, then STC / S2S, then HB
          const int64_t t1_ = pa ? ta : t0;
          const bool ph = th < t1_;
          const uint32_t bit = ph ? CDR_TTS_HEARTBEAT
                                  : (pa ? (started ? CDR_TTS_START_TO_CLOSE : CDR_TTS_SCHEDULE_TO_START)
                                        : CDR_TTS_SCHEDULE_TO_CLOSE);
          a_sid[j] = (uint32_t)a.schedule_id;
          a_aid[j] = a.activity_id;
          a_t[j] = ph ? th : t1_;
          a_inf[j] = (ph ? 2u : (pa ? 1u : 0u)) | (bit << 4) | ((uint32_t)(a.timer_task_status & 0xFF) << 8);
          a_cx |= (a.flags & CDR_AI_CANCEL_REQUESTED) ? 1u << j : 0u;
          const uint32_t p = RA0 + RA_W * (uint32_t)j;
          rs(p, lane, (uint32_t)t0);
          rs(p + 1, lane, (uint32_t)((uint64_t)t0 >> 32));
          rs(p + 2, lane, (uint32_t)a.stc);
          rs(p + 3, lane, (uint32_t)a.hb);
          rs(p + 4, lane, (uint32_t)j);
          rs(p + 5, lane, RNONE);
          rs(p + 6, lane, RNONE);
        }
      a_live = a_cy = (1u << cr.n_activity) - 1u;
      // byActivityID: the largest scheduleID of an activityID holds it (Load's map order)
#pragma unroll
      for (int j = 0; j < NA; j++) {
        bool hold = (a_live >> j) & 1u;
#pragma unroll
        for (int i = 0; i < NA; i++)
          hold = hold && !(i != j && ((a_live >> i) & 1u) && a_aid[i] == a_aid[j] && a_sid[i] > a_sid[j]);
        a_map |= hold ? 1u << j : 0u;
      }
      vmdrain();  // the loaded rows written above are read back by upserts / Started
    }
  }

  // ---- event prefetch: operands of event k+1 and the type of event k+3 in flight
  Ev q0 = load_ops(S, el8(0, len, lane), load_tf(S, el8(0, len, lane)));
  uint32_t t1 = load_tf(S, el8(1, len, lane)), t2 = load_tf(S, el8(2, len, lane));
  const uint32_t vh_cap = CP.vh_cap;
  bool done = len == 0;

#define SEL(c, a, b) ((c) ? (a) : (b))
#define PFAIL(cond, code)               \
  do {                                  \
    const bool f_ = (cond);             \
    err = SEL(f_, (int32_t)(code), err); \
    err_id = SEL(f_, e.id, err_id);     \
    err_k = SEL(f_, k, err_k);          \
    stop_at_call_end |= f_;             \
  } while (0)
  // a table of this variant is full: the planner's bound for a fresh history (never taken);
  // with a loaded state the entry goes to the next tier
#define CAPFAIL(cond)                       \
  do {                                      \
    if constexpr (CARRY) {                  \
      cyr |= (cond);                        \
    } else {                                \
      PFAIL(cond, CDR_E_BAD_INPUT);         \
    }                                       \
  } while (0)
  // lastDecision: the record of a pending source event, before a clearing event
#define RLD_CAPTURE(mine_)                                                                               \
  do {                                                                                                     \
    const bool c_ = (mine_) && ld_pending(ld);                                                             \
    if (__builtin_amdgcn_ballot_w64(c_ && want_ld)) {                                                      \
      if (c_) ld_write(gp(O_.last_decision) + w, ld, dv, dsched, dstart, dreq, dto, datt, dsc_ts, dst_ts,  \
                       dorig_ts);                                                                          \
      vmdrain();                                                                                           \
    }                                                                                                      \
    ld |= c_ ? LD_CAPTURED : 0u;                                                                           \
  } while (0)
  const uint32_t srows = S.elems / CDR_SLICE_WIDTH;
  for (uint32_t k = 0; k < srows; k++) {
    if (__builtin_amdgcn_ballot_w64(!done) == 0) break;
    const Ev e = q0;
    const uint32_t t3 = load_tf(S, el8(k + 3, len, lane));
    q0 = load_ops(S, el8(k + 1, len, lane), t1);
    t1 = t2;
    t2 = t3;
    done |= k >= len || cyr;
    const uint32_t type = e.tf & 0xFFu;
    // ---- call boundary (stateBuilder.go:603-604; mutableStateBuilder.go:561-581)
    const bool bf = !done && ((e.tf & CDR_SEF_BATCH_FIRST) || k == 0);
    const bool end_call = bf && k > 0;
    if (__builtin_amdgcn_ballot_w64(isRS && end_call)) {
      const int src = (isRS && end_call) ? cluster_for_version(B_.cluster, prev_ver) : 0;
      const bool pan = isRS && end_call && src < 0;  // the panic fires at the call's first event
      err = SEL(pan, (int32_t)CDR_P_UNKNOWN_CLUSTER, err);
      err_id = SEL(pan, call_first_id, err_id);
      err_k = SEL(pan, call_first_k, err_k);
      newrun_applied = newrun_applied && !(pan && nr_call == call_idx);
      const bool lri = isRS && end_call && src >= 0 && src != B_.cluster.current_cluster;
      if (lri) {
        rs(RL0 + 2u * (uint32_t)src, lane, (uint32_t)prev_ver);
        rs(RL0 + 2u * (uint32_t)src + 1, lane, (uint32_t)prev_id);
      }
      rs_mask |= lri ? 1u << src : 0u;
    }
    done |= end_call && err != CDR_OK;
    const bool nxt_call = end_call && !done;
    x_next_event = SEL(nxt_call, prev_id + 1, x_next_event);
    call_idx += nxt_call ? 1u : 0u;
    const bool start_call = bf && !done;
    call_first_id = SEL(start_call, e.id, call_first_id);
    call_first_k = SEL(start_call, k, call_first_k);
    ld = SEL(start_call, 0u, ld);
    prev_id = SEL(done, prev_id, e.id);
    prev_ver = SEL(done, prev_ver, e.ver);
    bool go = !done && !stop_at_call_end;

    // ---- version prelude (stateBuilder.go:134-154)
    if (isVH) {
      const bool gv = go;
      curv = SEL(gv && (x_state == CDR_STATE_CREATED || x_state == CDR_STATE_RUNNING), e.ver, curv);
      const bool newitem = n_vh == 0 || e.ver > vh_last_ver;
      const int32_t code = (e.id < 0 || (e.ver < 0 && e.ver != CDR_EMPTY_VERSION)) ? CDR_P_VH_ITEM_INVALID
                           : (n_vh != 0 && e.ver < vh_last_ver)                     ? CDR_E_VH_LOWER_VERSION
                           : (n_vh != 0 && e.id <= vh_last_id)                      ? CDR_E_VH_LOWER_EVENT_ID
                           : (newitem && n_vh >= vh_cap)                            ? CDR_E_BAD_INPUT
                                                                                    : CDR_OK;
      const bool f = gv && code != CDR_OK;
      PFAIL(f, code);
      go = go && !f;
      const bool add = go && newitem;
      const bool close_item = add && n_vh != 0;
      if (__builtin_amdgcn_ballot_w64(close_item)) {  // a new item closes the previous one (rare)
        if (close_item) gput(vh + (n_vh - 1), cdr_vh_item{vh_last_id, vh_last_ver});
        vmdrain();
      }
      n_vh += add ? 1u : 0u;
      vh_last_ver = SEL(add, e.ver, vh_last_ver);
      vh_last_id = SEL(go, e.id, vh_last_id);
    }
    const uint64_t tb = (go && type < 64) ? (1ull << type) : 0ull;  // this lane's group bit

    // ---- register-only types (stateBuilder.go:186-213,307-322,470-481)
    if (__builtin_amdgcn_ballot_w64(tb & RG_SIMPLE)) {
      const bool ms = type == CDR_EV_DT_SCHEDULED && go;  // :186-200 -> :143-167
      dv = SEL(ms, e.ver, dv);
      dsched = SEL(ms, e.id, dsched);
      dstart = SEL(ms, CDR_EMPTY_EVENT_ID, dstart);
      dreq = SEL(ms, EU, dreq);
      dto = SEL(ms, e.n, dto);
      datt = SEL(ms, e.aux, datt);
      dsc_ts = SEL(ms, e.ts, dsc_ts);
      dst_ts = SEL(ms, (int64_t)0, dst_ts);
      dorig_ts = SEL(ms, e.ts, dorig_ts);
      ld = SEL(ms, ld_make(CDR_LD_SCHEDULED, k), ld);
      if constexpr (TASKS) task_x(ms, CDR_TT_DECISION, e.id, t_dom, task_list_now(), 0, 0, 0);  // :196-197
      const bool mt = type == CDR_EV_DT_STARTED && go;  // :202-213 -> :200-253
      const bool f = mt && e.key != dsched;
      PFAIL(f, CDR_E_DECISION_NOT_FOUND);
      const bool ok = mt && !f;
      x_state = SEL(ok && x_state == CDR_STATE_CREATED, (int32_t)CDR_STATE_RUNNING, x_state);
      dv = SEL(ok, e.ver, dv);
      dstart = SEL(ok, e.id, dstart);
      dreq = SEL(ok, e.h, dreq);
      datt = SEL(ok, (int64_t)0, datt);
      dst_ts = SEL(ok, e.ts, dst_ts);
      ld = SEL(ok, ld_make(CDR_LD_STARTED, k), ld);
      task_t(ok, CDR_TT_DECISION_TIMEOUT, CDR_TIMEOUT_START_TO_CLOSE, e.key, e.ts + (int64_t)dto * NS_PER_S, 0);
      x_signals += (go && type == CDR_EV_WF_SIGNALED) ? 1 : 0;                           // :473-476
      x_flags |= (go && type == CDR_EV_WF_CANCEL_REQUESTED) ? CDR_XI_CANCEL_REQUESTED : 0u;  // :478-481
    }
    // ---- DecisionTaskCompleted (:215-219 -> :255-262,659-674,789-800)
    if (__builtin_amdgcn_ballot_w64(tb & CDR_TB(CDR_EV_DT_COMPLETED))) {
      const bool mine = (tb & CDR_TB(CDR_EV_DT_COMPLETED)) != 0;
      RLD_CAPTURE(mine);
      dv = SEL(mine, CDR_EMPTY_VERSION, dv);
      dsched = SEL(mine, CDR_EMPTY_EVENT_ID, dsched);
      dstart = SEL(mine, CDR_EMPTY_EVENT_ID, dstart);
      dreq = SEL(mine, EU, dreq);
      dto = SEL(mine, 0, dto);
      datt = SEL(mine, (int64_t)0, datt);
      dst_ts = SEL(mine, (int64_t)0, dst_ts);
      dsc_ts = SEL(mine, (int64_t)0, dsc_ts);  // OriginalScheduledTimestamp kept
      x_last_processed = SEL(mine, e.aux, x_last_processed);
      const uint32_t cks = e.h;
      const bool chk = mine && cks != 0 && cks != cks_ok;
      if (__builtin_amdgcn_ballot_w64(chk)) {  // addBinaryCheckSumIfNotExists (mutableStateBuilder.go:1798-1842)
        bool exists = false;
#pragma unroll
        for (uint32_t q = 0; q < LY::NRP; q++) exists |= chk && q < n_rp && rl(RP0 + 2 * q, lane) == cks;
        const bool app = chk && !exists;
        // the planner's bound (CDR_CAP_REG): never taken; the entry's slice: too small a capacity
        const bool f = app && (n_rp >= LY::NRP || n_rp >= CP.rp_cap);
        CAPFAIL(f);
        const bool put = app && !f;
        if (put) {  // the row is written after the loop (its first decision-completed id is event k's)
          const bool resettable = (c_live | r_live | g_live) == 0;
          rs(RP0 + 2 * n_rp, lane, cks);
          rs(RP0 + 2 * n_rp + 1, lane, k | (resettable ? 0x80000000u : 0u));
        }
        n_rp += put ? 1u : 0u;
        x_flags |= put ? CDR_XI_HAS_RESET_POINTS : 0u;
        cks_ok = SEL(chk && !f, cks, cks_ok);
      }
    }
    // ---- DecisionTaskTimedOut / Failed: FailDecision :635-656 + transient :169-198
    if (__builtin_amdgcn_ballot_w64(tb & RG_DTFAIL)) {
      const bool mine = (tb & RG_DTFAIL) != 0;
      RLD_CAPTURE(mine);
      const bool inc = type == CDR_EV_DT_FAILED || e.n != CDR_TIMEOUT_SCHEDULE_TO_START;
      const int64_t now = B_.now_ns;
      const int64_t na = inc ? datt + 1 : 0;
      const bool tr = na != 0;
      dv = SEL(mine, tr ? (isRS ? e.ver : (isVH ? curv : CDR_EMPTY_VERSION)) : CDR_EMPTY_VERSION, dv);
      dsched = SEL(mine, tr ? x_next_event : CDR_EMPTY_EVENT_ID, dsched);
      dstart = SEL(mine, CDR_EMPTY_EVENT_ID, dstart);
      dreq = SEL(mine, EU, dreq);
      dto = SEL(mine, tr ? x_dt_timeout_value : 0, dto);
      dst_ts = SEL(mine, (int64_t)0, dst_ts);
      dorig_ts = SEL(mine, (int64_t)0, dorig_ts);
      dsc_ts = SEL(mine, (tr || inc) ? now : (int64_t)0, dsc_ts);
      datt = SEL(mine, na, datt);
      ld = SEL(mine && tr, ld_make(CDR_LD_TRANSIENT, k), ld);
      if constexpr (TASKS) task_x(mine && tr, CDR_TT_DECISION, x_next_event, t_dom, task_list_now(), 0, 0, 0);  // :235,253
    }
    // ---- activities (:259-322 -> mutableStateBuilder.go:1982-2285)
    if (__builtin_amdgcn_ballot_w64(tb & RG_ACT)) {
      const bool m_s = type == CDR_EV_AT_SCHEDULED && go, m_st = type == CDR_EV_AT_STARTED && go;
      const bool m_cl = (tb & RG_ACT_CLOSE) != 0, m_cr = type == CDR_EV_AT_CANCEL_REQUESTED && go;
      const uint32_t key32 = (uint32_t)e.key;
      const bool kfit = (uint64_t)e.key < (1ull << 31);  // a scheduleID (event ids are in [1, 2^31))
      int fs = -1, fa = -1;
#pragma unroll
      for (int j = 0; j < NA; j++) {
        const bool lv = (a_live >> j) & 1u;
        fs = (lv && kfit && a_sid[j] == key32) ? j : fs;
        fa = (lv && ((a_map >> j) & 1u) && a_aid[j] == key32) ? j : fa;
      }
      // ActivityTaskScheduled: byActivityID[aid] moves to the new activity
      uint32_t clr = 0;
#pragma unroll
      for (int j = 0; j < NA; j++)
        clr |= (m_s && ((a_live & a_map) >> j & 1u) && a_aid[j] == key32) ? 1u << j : 0u;
      a_map &= ~clr;
      const uint32_t freem = ~a_live & ((1u << NA) - 1u);
      const int ff = freem ? (int)__builtin_ctz(freem) : -1;
      const bool f_cap = m_s && ff < 0;
      CAPFAIL(f_cap);
      const bool ok_s = m_s && !f_cap;
      const int js = ok_s ? ff : -1;
      {
        const int64_t ts2c = e.ts + (int64_t)(int32_t)e.h * NS_PER_S, ts2s = e.ts + (int64_t)e.n * NS_PER_S;
        const bool pa = ts2s < ts2c;  // append order breaks ties: S2C before S2S
        RSET(a_sid, NA, js, (uint32_t)e.id);
        RSET(a_aid, NA, js, key32);
        RSET(a_t, NA, js, pa ? ts2s : ts2c);
        RSET(a_inf, NA, js, (pa ? 1u : 0u) | ((pa ? CDR_TTS_SCHEDULE_TO_START : CDR_TTS_SCHEDULE_TO_CLOSE) << 4));
        if (ok_s) {
          const uint32_t p = RA0 + RA_W * (uint32_t)js;
          rs(p, lane, (uint32_t)ts2c);
          rs(p + 1, lane, (uint32_t)((uint64_t)ts2c >> 32));
          rs(p + 2, lane, (uint32_t)((uint64_t)e.key >> 32));  // StartToClose seconds
          rs(p + 3, lane, (uint32_t)((uint64_t)e.aux >> 32));  // HeartbeatTimeout seconds
          rs(p + 4, lane, k | ((k - call_first_k) << 20));
          rs(p + 5, lane, RNONE);
          rs(p + 6, lane, RNONE);
        }
      }
      a_live |= bitof(js);
      a_map |= bitof(js);
      a_st &= ~bitof(js);
      a_cx &= ~bitof(js);
      a_cy &= ~bitof(js);
      if constexpr (TASKS) task_x(ok_s, CDR_TT_ACTIVITY, e.id, t_dom, task_list_now(), 0, 0, 0);  // :265-266
      // ActivityTaskStarted (:2083-2098): nil deref if missing
      const bool f_st = m_st && fs < 0;
      PFAIL(f_st, CDR_P_ACTIVITY_STARTED_NIL);
      const bool ok_st = m_st && !f_st;
      const int jst = ok_st ? fs : -1;
      {
        int64_t tn = 0;
        uint32_t in = 0, old = 0;
        RGET(a_inf, NA, jst, old);
        if (ok_st) {
          const uint32_t p = RA0 + RA_W * (uint32_t)jst;
          const int64_t ts2c = (int64_t)(((uint64_t)rl(p + 1, lane) << 32) | rl(p, lane));
          const int32_t stc = (int32_t)rl(p + 2, lane), hb = (int32_t)rl(p + 3, lane);
          const int64_t tstc = e.ts + (int64_t)stc * NS_PER_S, thb = hb > 0 ? e.ts + (int64_t)hb * NS_PER_S : T_NONE;
          const bool pa = tstc < ts2c;  // S2C, then StartToClose, then Heartbeat on ties
          const int64_t t1_ = pa ? tstc : ts2c;
          const bool ph = thb < t1_;
          tn = ph ? thb : t1_;
          const uint32_t bit = ph ? CDR_TTS_HEARTBEAT : (pa ? CDR_TTS_START_TO_CLOSE : CDR_TTS_SCHEDULE_TO_CLOSE);
          in = (old & 0xFF00u) | (ph ? 2u : (pa ? 1u : 0u)) | (bit << 4);
          rs(p + 5, lane, k);
        }
        RSET(a_t, NA, jst, tn);
        RSET(a_inf, NA, jst, in);
        a_st |= bitof(jst);
      }
      // closes -> DeleteActivity (:1247-1269)
      const bool f_cl = m_cl && fs < 0;
      PFAIL(f_cl, CDR_E_ACTIVITY_NOT_FOUND);
      bool ok_cl = m_cl && !f_cl;
      {
        const int jc = ok_cl ? fs : -1;
        uint32_t aid_c = 0;
        RGET(a_aid, NA, jc, aid_c);
        const bool had = jc >= 0 && ((a_map >> jc) & 1u);
        a_live &= ~bitof(jc);
        a_map &= ~bitof(jc);
        uint32_t other = 0;  // pendingActivityIDToEventID held by another activity with the same id
#pragma unroll
        for (int j = 0; j < NA; j++)
          other |= (ok_cl && !had && ((a_live & a_map) >> j & 1u) && a_aid[j] == aid_c) ? 1u << j : 0u;
        a_map &= ~other;
        const bool f2 = ok_cl && !had && other == 0;
        PFAIL(f2, CDR_E_ACTIVITY_ID_NOT_FOUND);
        ok_cl = ok_cl && !f2;
      }
      // ActivityTaskCancelRequested (:2264-2285)
      const bool f_cr = m_cr && fa < 0;
      PFAIL(f_cr, CDR_E_MISSING_ACTIVITY_INFO);
      const bool ok_cr = m_cr && !f_cr;
      if (ok_cr) rs(RA0 + RA_W * (uint32_t)fa + 6, lane, k);
      a_cx |= ok_cr ? bitof(fa) : 0u;
      // activity timer pick (timerBuilder.go:211-312): earliest (time, scheduleID, order)
      const bool on = ok_s || ok_st || ok_cl;
      if (__builtin_amdgcn_ballot_w64(on)) {
        int best = -1;
        int64_t bt = 0;
        uint32_t bs = 0, bi = 0;
#pragma unroll
        for (int j = 0; j < NA; j++) {
          const uint32_t o = a_inf[j] & 3u;
          const bool better = on && ((a_live >> j) & 1u) &&
                              (best < 0 || a_t[j] < bt || (a_t[j] == bt && (a_sid[j] < bs || (a_sid[j] == bs && o < (bi & 3u)))));
          best = better ? j : best;
          bt = better ? a_t[j] : bt;
          bs = better ? a_sid[j] : bs;
          bi = better ? a_inf[j] : bi;
        }
        const uint32_t b = (bi >> 4) & 0xFu;
        const bool made = best >= 0 && !((bi >> 8) & b);
        RSET(a_inf, NA, made ? best : -1, bi | (b << 8));
        // ActivityTimeoutTask (timerBuilder.go:391-408): TimerTaskStatus bit -> shared.TimeoutType.
        // Attempt is the row's (timerBuilder.go:263-302, 404): 0 for an activity this replay
        // scheduled, the loaded row's for a carried one — the head of a pick can be a loaded
        // activity whatever event asked for the pick (as the general kernel's act_task)
        int64_t att = 0;
        if constexpr (CARRY && TASKS) {
          if (made && ((a_cy >> best) & 1u)) {
            const GAS cdr_carry* CY = gp(B_.carry);
            att = gget(gp(CY->state.act) + gget(gp(CY->caps) + csrc).act_off +
                       rl(RA0 + RA_W * (uint32_t)best + 4, lane)).attempt;
          }
        }
        task_t(made, CDR_TT_ACTIVITY_TIMEOUT, (int32_t)__builtin_ctz(b | 16u), (int64_t)bs, bt, att);
      }
    }
    // ---- user timers (:324-350 -> :2877-2991)
    if (__builtin_amdgcn_ballot_w64(tb & RG_TIM)) {
      const bool m_ts = type == CDR_EV_TIMER_STARTED && go;
      const bool m_tf = (type == CDR_EV_TIMER_FIRED || type == CDR_EV_TIMER_CANCELED) && go;
      const uint32_t tid = (uint32_t)e.key;
      int fm = -1;
      uint32_t kill = 0;
#pragma unroll
      for (int j = 0; j < NT; j++) {
        const bool hit = ((t_live >> j) & 1u) && t_tid[j] == tid;
        fm = hit ? j : fm;
        kill |= (m_tf && hit) ? 1u << j : 0u;
      }
      t_live &= ~kill;
      const uint32_t freem = ~t_live & ((1u << NT) - 1u);
      const int slot = fm >= 0 ? fm : (freem ? (int)__builtin_ctz(freem) : -1);
      const bool f = m_ts && slot < 0;
      CAPFAIL(f);
      const bool ok = m_ts && !f;
      const int jt = ok ? slot : -1;
      RSET(t_tid, NT, jt, tid);
      RSET(t_sid, NT, jt, (uint32_t)e.id);
      RSET(t_exp, NT, jt, e.ts + e.aux * NS_PER_S);
      t_live |= bitof(jt);
      t_cr &= ~bitof(jt);  // TaskID = TimerTaskStatusNone
      t_cy &= ~bitof(jt);
      if (ok) rs(RT0 + (uint32_t)jt, lane, k);
      // user timer pick (timerBuilder.go:171-184,233-247): head by (ExpiryTime, StartedID)
      const bool on = ok || m_tf;
      int best = -1;
      int64_t be = 0;
      uint32_t bs = 0;
#pragma unroll
      for (int j = 0; j < NT; j++) {
        const bool better = on && ((t_live >> j) & 1u) && (best < 0 || t_exp[j] < be || (t_exp[j] == be && t_sid[j] < bs));
        best = better ? j : best;
        be = better ? t_exp[j] : be;
        bs = better ? t_sid[j] : bs;
      }
      // UserTimerTask when the head's TaskID was not Created yet (timerBuilder.go:171-184)
      task_t(best >= 0 && !((t_cr >> best) & 1u), CDR_TT_USER_TIMER, 0, (int64_t)bs, be, 0);
      t_cr |= bitof(best);
    }
    // ---- children, request-cancels, signals (:355-468)
    if (__builtin_amdgcn_ballot_w64(tb & RG_EXT)) {
      const uint32_t key32 = (uint32_t)e.key;
      const bool kfit = (uint64_t)e.key < (1ull << 31);
      const bool dmiss = (e.tf & CDR_SEF_DOMAIN_MISSING) != 0;
      const uint32_t init = k | ((k - call_first_k) << 20);
      // StartChildWorkflowExecutionInitiated (:3256-3280)
      {
        const bool m = type == CDR_EV_CHILD_INITIATED && go;
        const uint32_t fr = ~c_live & ((1u << NX) - 1u);
        const int j = fr ? (int)__builtin_ctz(fr) : -1;
        const bool f = m && j < 0;
        CAPFAIL(f);
        const bool ok = m && !f;
        const int jj = ok ? j : -1;
        RSET(c_id, NX, jj, (uint32_t)e.id);
        c_live |= bitof(jj);
        c_cy &= ~bitof(jj);
        if (ok) {
          rs(RC0 + 2 * (uint32_t)jj, lane, init);
          rs(RC0 + 2 * (uint32_t)jj + 1, lane, RNONE);
        }
        PFAIL(ok && dmiss, CDR_E_DOMAIN_NOT_FOUND);
        if constexpr (TASKS) {
          if (ok && !dmiss) {  // scheduleStartChildWorkflowTransferTask (:370-371)
            const cdr_attr_external xa = gget(gp((const cdr_attr_external*)(B_.ev.arena + ((uint64_t)e.key >> 32))));
            task_x(true, CDR_TT_START_CHILD, e.id, xa.target_domain_id, 0, xa.workflow_id, 0, 0);
          }
        }
      }
      // ChildWorkflowExecutionStarted (:3312-3325): nil deref if missing; closes delete
      {
        const bool ms = type == CDR_EV_CHILD_STARTED && go;
        const bool mc = (tb & RG_CHILD_CLOSE) != 0;
        int j = -1;
#pragma unroll
        for (int i = NX - 1; i >= 0; i--) j = (((c_live >> i) & 1u) && kfit && c_id[i] == key32) ? i : j;
        const bool f = ms && j < 0;
        PFAIL(f, CDR_P_CHILD_STARTED_NIL);
        if (ms && !f) rs(RC0 + 2 * (uint32_t)j + 1, lane, k);
        c_live &= ~((mc && j >= 0) ? bitof(j) : 0u);
      }
      // RequestCancelExternalWorkflowExecutionInitiated (:2577-2596) / closes (:1147-1153)
      {
        const bool m = type == CDR_EV_RCE_INITIATED && go;
        const uint32_t fr = ~r_live & ((1u << NX) - 1u);
        const int j = fr ? (int)__builtin_ctz(fr) : -1;
        const bool f = m && j < 0;
        CAPFAIL(f);
        const bool ok = m && !f;
        const int jj = ok ? j : -1;
        RSET(r_id, NX, jj, (uint32_t)e.id);
        r_live |= bitof(jj);
        r_cy &= ~bitof(jj);
        if (ok) rs(RR0 + (uint32_t)jj, lane, init);
        PFAIL(ok && dmiss, CDR_E_DOMAIN_NOT_FOUND);
        if constexpr (TASKS) {
          if (ok && !dmiss) {  // scheduleCancelExternalWorkflowTransferTask (:421-427)
            const cdr_attr_external xa = gget(gp((const cdr_attr_external*)(B_.ev.arena + ((uint64_t)e.key >> 32))));
            task_x(true, CDR_TT_CANCEL_EXECUTION, e.id, xa.target_domain_id, 0, xa.workflow_id, xa.run_id,
                   (xa.flags & CDR_XF_CHILD_ONLY) ? CDR_TF_CHILD_ONLY : 0u);
          }
        }
        const bool mc = (type == CDR_EV_RCE_FAILED || type == CDR_EV_EXT_CANCEL_REQUESTED) && go;
        int jc = -1;
#pragma unroll
        for (int i = NX - 1; i >= 0; i--) jc = (((r_live >> i) & 1u) && kfit && r_id[i] == key32) ? i : jc;
        r_live &= ~((mc && jc >= 0) ? bitof(jc) : 0u);
      }
      // SignalExternalWorkflowExecutionInitiated (:2701-2723) / closes (:1156-1162)
      {
        const bool m = type == CDR_EV_SE_INITIATED && go;
        const uint32_t fr = ~g_live & ((1u << NX) - 1u);
        const int j = fr ? (int)__builtin_ctz(fr) : -1;
        const bool f = m && j < 0;
        CAPFAIL(f);
        const bool ok = m && !f;
        const int jj = ok ? j : -1;
        RSET(g_id, NX, jj, (uint32_t)e.id);
        g_live |= bitof(jj);
        g_cy &= ~bitof(jj);
        if (ok) rs(RG0 + (uint32_t)jj, lane, init);
        PFAIL(ok && dmiss, CDR_E_DOMAIN_NOT_FOUND);
        if constexpr (TASKS) {
          if (ok && !dmiss) {  // scheduleSignalWorkflowTransferTask (:452-458)
            const cdr_attr_external xa = gget(gp((const cdr_attr_external*)(B_.ev.arena + ((uint64_t)e.key >> 32))));
            task_x(true, CDR_TT_SIGNAL_EXECUTION, e.id, xa.target_domain_id, 0, xa.workflow_id, xa.run_id,
                   (xa.flags & CDR_XF_CHILD_ONLY) ? CDR_TF_CHILD_ONLY : 0u);
          }
        }
        const bool mc = (type == CDR_EV_SE_FAILED || type == CDR_EV_EXT_SIGNALED) && go;
        int jc = -1;
#pragma unroll
        for (int i = NX - 1; i >= 0; i--) jc = (((g_live >> i) & 1u) && kfit && g_id[i] == key32) ? i : jc;
        g_live &= ~((mc && jc >= 0) ? bitof(jc) : 0u);
      }
    }
    // ---- workflow closes (:483-531 -> UpdateWorkflowStateCloseStatus)
    if (__builtin_amdgcn_ballot_w64(tb & RG_CLOSE)) {
      const bool mine = (tb & RG_CLOSE) != 0;
      const int cs = type == CDR_EV_WF_COMPLETED   ? CDR_CLOSE_COMPLETED
                     : type == CDR_EV_WF_FAILED    ? CDR_CLOSE_FAILED
                     : type == CDR_EV_WF_TIMED_OUT ? CDR_CLOSE_TIMED_OUT
                     : type == CDR_EV_WF_CANCELED  ? CDR_CLOSE_CANCELED
                                                   : CDR_CLOSE_TERMINATED;
      const bool f = mine && !transition_ok(x_state, x_close, CDR_STATE_COMPLETED, cs);
      PFAIL(f, CDR_E_INVALID_STATE_TRANSITION);
      const bool ok = mine && !f;
      x_state = SEL(ok, (int32_t)CDR_STATE_COMPLETED, x_state);
      x_close = SEL(ok, (int32_t)cs, x_close);
      x_completion_batch = SEL(ok, call_first_id, x_completion_batch);
      close_tasks(ok, e.ts);
    }
    // ---- rare types: WorkflowExecutionStarted, UpsertWorkflowSearchAttributes,
    // ContinuedAsNew, unknown types (global memory; drained after)
    if (__builtin_amdgcn_ballot_w64(go && !((tb & RG_KNOWN) &
                                           ~(CDR_TB(CDR_EV_WF_STARTED) | CDR_TB(CDR_EV_UPSERT_SA) |
                                             CDR_TB(CDR_EV_WF_CONTINUED_AS_NEW))))) {
      const bool mine_st = type == CDR_EV_WF_STARTED && go;
      RLD_CAPTURE(mine_st);  // a later Started resets the decision fields
      if (mine_st) {  // stateBuilder.go:158-184 -> mutableStateBuilder.go:1639-1716
        const GAS cdr_attr_wf_started* a = gp((const cdr_attr_wf_started*)(B_.ev.arena + (uint64_t)e.aux));
        const uint32_t af = a->flags;
        const bool f1 = (af & CDR_SF_HAS_PARENT_DOMAIN) && (af & CDR_SF_PARENT_DOMAIN_MISSING);
        const bool f2 = !f1 && !transition_ok(x_state, x_close, CDR_STATE_CREATED, CDR_CLOSE_NONE);
        PFAIL(f1, CDR_E_DOMAIN_NOT_FOUND);
        PFAIL(f2, CDR_E_INVALID_STATE_TRANSITION);
        if (!f1 && !f2) {
          const bool first = !(x_flags & CDR_XI_STARTED);
          uint32_t xf = x_flags;
          X->domain_id = D.domain_id;
          X->workflow_id = D.workflow_id;
          X->run_id = D.run_id;
          X->create_request_id = D.request_id;
          X->task_list = a->task_list;
          if constexpr (TASKS) t_tl = a->task_list;
          X->workflow_type = a->workflow_type;
          X->workflow_timeout = a->exec_timeout_s;
          X->cron_schedule = a->cron_schedule;
          X->attempt = a->attempt;
          X->initiated_id = (af & CDR_SF_HAS_PARENT_INITIATED) ? a->parent_initiated_id : CDR_EMPTY_EVENT_ID;
          if (af & CDR_SF_HAS_PARENT_DOMAIN) X->parent_domain_id = a->parent_domain_id;
          else if (first) X->parent_domain_id = 0;
          if (af & CDR_SF_HAS_PARENT_EXEC) {
            X->parent_workflow_id = a->parent_workflow_id;
            X->parent_run_id = a->parent_run_id;
          } else if (first) {
            X->parent_workflow_id = 0;
            X->parent_run_id = 0;
          }
          if (a->expiration_ts != 0) {
            X->expiration_time = a->expiration_ts;
            xf |= CDR_XI_HAS_EXPIRATION;
          } else if (first) {
            X->expiration_time = 0;
          }
          if (af & CDR_SF_HAS_RETRY) {
            xf |= CDR_XI_HAS_RETRY;
            X->backoff_coefficient = a->backoff_coefficient;
            X->expiration_seconds = a->retry_expiration_s;
            X->initial_interval = a->retry_initial_s;
            X->maximum_attempts = a->retry_max_attempts;
            X->maximum_interval = a->retry_max_interval_s;
            X->nonretriable = a->nonretriable;
          } else if (first) {
            X->backoff_coefficient = 0.0;
            X->expiration_seconds = 0;
            X->initial_interval = 0;
            X->maximum_attempts = 0;
            X->maximum_interval = 0;
            X->nonretriable = 0;
          }
          // rolloverAutoResetPointsWithExpiringTime (:3184-3205): rows written here, their
          // checksums cached for addBinaryCheckSumIfNotExists
          n_rp = 0;
          xf &= ~CDR_XI_HAS_RESET_POINTS;
          if (af & CDR_SF_HAS_RESET_POINTS) {
            xf |= CDR_XI_HAS_RESET_POINTS;
            const int64_t expiring = e.ts + (int64_t)D.retention_days * 24ll * 3600ll * NS_PER_S;
            const uint32_t crun = a->continued_run_id, off = a->reset_points_off, cnt = a->reset_points_len;
            const uint32_t cap = CP.rp_cap;
            PFAIL(cnt > cap, CDR_E_BAD_INPUT);  // the rolled-over points do not fit the slice
            if constexpr (CARRY) cyr |= (cnt < cap ? cnt : cap) > LY::NRP;
            for (uint32_t q = 0; q < cnt && q < cap && n_rp < LY::NRP; q++) {
              cdr_reset_point p = gget(gp(B_.rps) + (off + q));
              const uint32_t run = (p.flags & CDR_RP_HAS_RUN_ID) ? p.run_id : 0u;
              if (run == crun) {
                p.flags |= CDR_RP_HAS_EXPIRING;
                p.expiring_time_nano = expiring;
              }
              gput(rp + n_rp, p);
              rs(RP0 + 2 * n_rp, lane, (p.flags & CDR_RP_HAS_CHECKSUM) ? p.binary_checksum : 0u);
              rs(RP0 + 2 * n_rp + 1, lane, RNONE);
              n_rp++;
            }
          }
          if (af & CDR_SF_HAS_MEMO) {
            xf |= CDR_XI_HAS_MEMO;
            X->memo = a->memo;
          } else if (first) {
            X->memo = 0;
          }
          if (af & CDR_SF_HAS_SEARCH_ATTR) {
            n_sa = 0;
            const uint32_t off = a->search_attr_off, cnt = a->search_attr_len, cap = CP.sa_cap;
            PFAIL(cnt > cap, CDR_E_BAD_INPUT);  // the search attributes do not fit the slice
            if constexpr (CARRY) cyr |= (cnt < cap ? cnt : cap) > CDR_REG_NSA;
            for (uint32_t q = 0; q < cnt && q < cap && n_sa < CDR_REG_NSA; q++) {
              gput(sa + n_sa, gget(gp(B_.kvs) + (off + q)));
              n_sa++;
            }
            if (n_sa) xf |= CDR_XI_HAS_SEARCH_ATTR;
            else xf &= ~CDR_XI_HAS_SEARCH_ATTR;
          }
          xf |= CDR_XI_STARTED | (isVH ? CDR_XI_VH_BRANCH : CDR_XI_HAS_BRANCH);
          uint64_t lo, hi;  // SetHistoryTree (:313-339)
          cdr_uuid(B_.uuid_seed, D.wf_key, CDR_UUID_BRANCH, e.id, &lo, &hi);
          X->branch_tree_id = D.run_id;
          X->branch_id_lo = lo;
          X->branch_id_hi = hi;
          if (isRS) RS->start_version = e.ver;  // :182-184
          x_flags = xf;
          cks_ok = 0;
          x_dt_timeout_value = a->task_timeout_s;
          x_state = CDR_STATE_CREATED;
          x_close = CDR_CLOSE_NONE;
          x_last_processed = CDR_EMPTY_EVENT_ID;
          dv = CDR_EMPTY_VERSION;
          dsched = CDR_EMPTY_EVENT_ID;
          dstart = CDR_EMPTY_EVENT_ID;
          dreq = EU;
          dto = 0;
          if constexpr (TASKS) {  // scheduleWorkflowTimerTask (:706-735) + RecordWorkflowStartedTask (:614-616)
            const int64_t backoff = (int64_t)a->first_decision_backoff_s * NS_PER_S;
            task_t(backoff != 0, CDR_TT_WORKFLOW_BACKOFF, (af & CDR_SF_CRON_INITIATOR) ? 1 : 0, 0, e.ts + backoff, 0);
            task_t(true, CDR_TT_WORKFLOW_TIMEOUT, 0, 0, e.ts + (int64_t)a->exec_timeout_s * NS_PER_S + backoff, 0);
            task_x(true, CDR_TT_RECORD_STARTED, 0, 0, 0, 0, 0, 0);
          }
        }
      }
      if (type == CDR_EV_UPSERT_SA && go) {  // :533-535 -> :2746-2768 (last writer per key)
        const uint64_t off = (uint64_t)e.aux;
        const uint32_t cnt = e.h, cap = CP.sa_cap;
        for (uint32_t q = 0; q < cnt; q++) {  // the rows themselves (device-coherent reads after a drain)
          const cdr_kv kv = gget(gp(B_.kvs) + (off + q));
          bool found = false;
          for (uint32_t j = 0; j < n_sa; j++)
            if (__hip_atomic_load(&(sa + j)->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kv.key) {
              (sa + j)->value = kv.value;
              found = true;
            }
          if (!found && n_sa < cap && n_sa < CDR_REG_NSA) {
            gput(sa + n_sa, kv);
            n_sa++;
          } else if (CARRY && !found && n_sa < cap) {
            cyr = true;  // a key beyond this variant's search-attribute rows
          } else {
            PFAIL(!found && n_sa >= cap, CDR_E_BAD_INPUT);  // a new key past the slice
          }
          vmdrain();
        }
        x_flags |= CDR_XI_HAS_SEARCH_ATTR;
        task_x(true, CDR_TT_UPSERT_SA, 0, 0, 0, 0, 0, 0);  // :535
      }
      if (type == CDR_EV_WF_CONTINUED_AS_NEW && go) {  // :537-595
        const int32_t nr = D.newrun;
        const bool empty = nr < 0 || call_idx != D.newrun_call || gp(B_.wfs)[nr].ev_len == 0;
        PFAIL(empty, CDR_E_NEWRUN_HISTORY_EMPTY);
        if (!empty) {
          newrun_applied = true;  // the new run replays in its own lane; k_finalize joins
          nr_call = call_idx;
          const bool f2 = !transition_ok(x_state, x_close, CDR_STATE_COMPLETED, CDR_CLOSE_CONTINUED_AS_NEW);
          PFAIL(f2, CDR_E_INVALID_STATE_TRANSITION);
          if (!f2) {
            x_state = CDR_STATE_COMPLETED;
            x_close = CDR_CLOSE_CONTINUED_AS_NEW;
            x_completion_batch = call_first_id;
          }
          close_tasks(!f2, e.ts);  // :592
        }
      }
      PFAIL(go && !(tb & RG_KNOWN), CDR_E_UNKNOWN_EVENT_TYPE);  // :597-599
      vmdrain();
    }
    if constexpr (TASKS) {  // a task store of this step completes before the next prefetch use
      if (__builtin_amdgcn_ballot_w64(tstored)) vmdrain();
      tstored = false;
    }
  }
#undef PFAIL
#undef CAPFAIL
#undef SEL
#undef RLD_CAPTURE
  // ---- end of the last call
  if (len > 0 && (err == CDR_OK || stop_at_call_end)) {
    if (isRS) {
      const int src = cluster_for_version(B_.cluster, prev_ver);
      if (src < 0) {
        err = CDR_P_UNKNOWN_CLUSTER;
        err_id = call_first_id;
        err_k = call_first_k;
        newrun_applied = newrun_applied && nr_call != call_idx;
      } else if (src != B_.cluster.current_cluster && err == CDR_OK) {
        rs(RL0 + 2u * (uint32_t)src, lane, (uint32_t)prev_ver);
        rs(RL0 + 2u * (uint32_t)src + 1, lane, (uint32_t)prev_id);
        rs_mask |= 1u << src;
      }
    }
    if (err == CDR_OK) x_next_event = prev_id + 1;
  }
  if (err == CDR_OK && D.parent < 0 && D.expected_next_event_id != 0 && x_next_event != D.expected_next_event_id) {
    err = CDR_E_REBUILD_NEXT_EVENT_ID;  // nDCStateRebuilder.go:139-143
    err_id = prev_id;
    err_k = len;
  }
  if (TASKS && t_over && err == CDR_OK) {  // the planner's task capacities did not bound this history
    err = CDR_E_BAD_INPUT;
    err_id = prev_id;
    err_k = len;
  }
  // carry-in handed on: the next tier replays the entry from its loaded state again
  if constexpr (CARRY) err = cyr ? (NA >= (int)CDR_REG2_NA ? CLS_RETRY2 : CLS_RETRY) : err;
  const bool ok = err == CDR_OK;
  // the loaded state's row offsets (carried rows are re-read at emission)
  cdr_wf_caps ccy{};
  if constexpr (CARRY)
    if (ok && csrc >= 0) ccy = gget(gp(gp(B_.carry)->caps) + csrc);
  // event-row gathers for the rows below: (index k) -> column values of event k
  auto ev64 = [&](uint32_t kk, int c) { return bld64(S.r, el8(kk, len, lane), S.col(c)); };
  auto ev32 = [&](uint32_t kk, int c) { return bld32(S.r, el8(kk, len, lane) - S.l4, S.col(c)); };
  if constexpr (TASKS) {  // a failed workflow reports no tasks (as the general kernel)
    gp(O_.n_tasks)[2 * (uint64_t)w] = ok ? n_xt : 0u;
    gp(O_.n_tasks)[2 * (uint64_t)w + 1] = ok ? n_tt : 0u;
  }
  cdr_wf_result r;
  r.code = err;
  r.flags = (newrun_applied ? CDR_RF_NEWRUN_APPLIED : 0u) | (D.parent >= 0 ? CDR_RF_IS_NEWRUN : 0u);
  r.fail_event_id = err_id;
  r.fail_index = err_k;
  r.n_activity = r.n_timer = r.n_child = r.n_cancel = r.n_signal = 0;
  r.n_vh = ok ? n_vh : 0u;
  r.n_reset_points = ok ? n_rp : 0u;
  r.n_search_attr = ok ? n_sa : 0u;
  if (ok && want_ld && !(ld & LD_CAPTURED))
    ld_write(gp(O_.last_decision) + w, ld, dv, dsched, dstart, dreq, dto, datt, dsc_ts, dst_ts, dorig_ts);
  if (ok) {
    // ---- pending rows from the tables (k_tables orders them by key)
    uint32_t n = 0;
    GAS cdr_activity_info* act = gp(O_.act) + CP.act_off;
#pragma unroll
    for (int j = 0; j < NA; j++) {
      if (!((a_live >> j) & 1u)) continue;
      const uint32_t p = RA0 + RA_W * (uint32_t)j;
      const uint32_t sw = rl(p + 4, lane), stk = rl(p + 5, lane), cxk = rl(p + 6, lane);
      if constexpr (CARRY) {
        if ((a_cy >> j) & 1u) {  // a loaded activity: its row, with what the replay changed
          cdr_activity_info o = gget(gp(gp(B_.carry)->state.act) + ccy.act_off + sw);
          const uint32_t vk = (cxk != RNONE && (stk == RNONE || cxk > stk)) ? cxk : stk;
          if (vk != RNONE) o.version = ev64(vk, CDR_COL_VERSION);  // Started / CancelRequested (:2083-2098,2264-2285)
          if (stk != RNONE) {
            o.started_id = ev64(stk, CDR_COL_EVENT_ID);
            o.started_time = ev64(stk, CDR_COL_TIMESTAMP);
            o.last_heartbeat_time = o.started_time;
            o.request_id = ev32(stk, CDR_COL_H);
            o.flags |= CDR_AI_STARTED_TIME_SET;
          }
          if (cxk != RNONE) o.cancel_request_id = ev64(cxk, CDR_COL_EVENT_ID);
          o.timer_task_status = (int32_t)((a_inf[j] >> 8) & 0xFFu);
          o.flags = (o.flags & ~CDR_AI_CANCEL_REQUESTED) | (((a_cx >> j) & 1u) ? CDR_AI_CANCEL_REQUESTED : 0u);
          gput(act + n++, o);
          continue;
        }
      }
      const uint32_t sk = sw & 0xFFFFFu, cfk = sk - (sw >> 20);
      uint32_t vk = sk;  // Version: the last of Scheduled / Started / CancelRequested
      vk = (stk != RNONE && stk > vk) ? stk : vk;
      vk = (cxk != RNONE && cxk > vk) ? cxk : vk;
      const int64_t sched_ts = ev64(sk, CDR_COL_TIMESTAMP);
      const uint32_t arec = (uint32_t)ev64(sk, CDR_COL_AUX);
      const GAS cdr_attr_at_scheduled* a = gp((const cdr_attr_at_scheduled*)(B_.ev.arena + arec));
      const bool retry = (a->flags & CDR_AF_HAS_RETRY) != 0;
      const int32_t s2c = a->s2c_s, xs = a->retry_expiration_s;
      const bool started = stk != RNONE;
      cdr_activity_info o;
      o.version = ev64(vk, CDR_COL_VERSION);
      o.schedule_id = (int64_t)a_sid[j];
      o.scheduled_event_batch_id = ev64(cfk, CDR_COL_EVENT_ID);
      o.scheduled_time = sched_ts;
      o.started_id = started ? ev64(stk, CDR_COL_EVENT_ID) : CDR_EMPTY_EVENT_ID;
      o.started_time = started ? ev64(stk, CDR_COL_TIMESTAMP) : 0;
      o.last_heartbeat_time = o.started_time;
      o.expiration_time = sched_ts + (int64_t)((retry && xs > s2c) ? xs : s2c) * NS_PER_S;
      o.cancel_request_id = cxk != RNONE ? ev64(cxk, CDR_COL_EVENT_ID) : CDR_EMPTY_EVENT_ID;
      o.activity_id = a_aid[j];
      o.request_id = started ? ev32(stk, CDR_COL_H) : 0u;
      o.task_list = a->task_list;
      o.nonretriable = retry ? a->nonretriable : 0u;
      o.s2s = a->s2s_s;
      o.s2c = s2c;
      o.stc = a->stc_s;
      o.hb = a->hb_s;
      o.timer_task_status = (int32_t)((a_inf[j] >> 8) & 0xFFu);
      o.attempt = 0;
      o.initial_interval = retry ? a->retry_initial_s : 0;
      o.maximum_interval = retry ? a->retry_max_interval_s : 0;
      o.maximum_attempts = retry ? a->retry_max_attempts : 0;
      o.flags = (retry ? CDR_AI_HAS_RETRY : 0u) | (((a_cx >> j) & 1u) ? CDR_AI_CANCEL_REQUESTED : 0u) |
                (((a_st >> j) & 1u) ? CDR_AI_STARTED_TIME_SET : 0u);
      o.backoff_coefficient = retry ? a->backoff_coefficient : 0.0;
      gput(act + n++, o);
    }
    r.n_activity = n;
    n = 0;
    GAS cdr_timer_info* tim = gp(O_.timer) + CP.timer_off;
#pragma unroll
    for (int j = 0; j < NT; j++) {
      if (!((t_live >> j) & 1u)) continue;
      cdr_timer_info o;
      if (CARRY && ((t_cy >> j) & 1u))  // a loaded timer: its Version as loaded
        o.version = gget(gp(gp(B_.carry)->state.timer) + ccy.timer_off + rl(RT0 + (uint32_t)j, lane)).version;
      else
        o.version = ev64(rl(RT0 + (uint32_t)j, lane), CDR_COL_VERSION);
      o.started_id = (int64_t)t_sid[j];
      o.expiry_time = t_exp[j];
      o.task_id = ((t_cr >> j) & 1u) ? CDR_TIMER_TASK_STATUS_CREATED : CDR_TIMER_TASK_STATUS_NONE;
      o.timer_id = t_tid[j];
      o._pad = 0;
      gput(tim + n++, o);
    }
    r.n_timer = n;
    n = 0;
    GAS cdr_child_info* chi = gp(O_.child) + CP.child_off;
#pragma unroll
    for (int j = 0; j < NX; j++) {
      if (!((c_live >> j) & 1u)) continue;
      const uint32_t iw = rl(RC0 + 2 * (uint32_t)j, lane), stk = rl(RC0 + 2 * (uint32_t)j + 1, lane);
      const uint32_t ik = iw & 0xFFFFFu;
      if constexpr (CARRY) {
        if ((c_cy >> j) & 1u) {  // a loaded child: ChildWorkflowExecutionStarted may have started it
          cdr_child_info c = gget(gp(gp(B_.carry)->state.child) + ccy.child_off + iw);
          if (stk != RNONE) {
            c.started_id = ev64(stk, CDR_COL_EVENT_ID);
            c.started_run_id = ev32(stk, CDR_COL_H);
          }
          gput(chi + n++, c);
          continue;
        }
      }
      cdr_child_info c;
      c.version = ev64(ik, CDR_COL_VERSION);
      c.initiated_id = (int64_t)c_id[j];
      c.initiated_event_batch_id = ev64(ik - (iw >> 20), CDR_COL_EVENT_ID);
      c.started_id = stk != RNONE ? ev64(stk, CDR_COL_EVENT_ID) : CDR_EMPTY_EVENT_ID;
      uint64_t lo, hi;
      cdr_uuid(B_.uuid_seed, D.wf_key, CDR_UUID_CHILD_REQ, c.initiated_id, &lo, &hi);
      c.create_request_lo = lo;
      c.create_request_hi = hi;
      c.started_workflow_id = ev32(ik, CDR_COL_H);
      c.started_run_id = stk != RNONE ? ev32(stk, CDR_COL_H) : 0u;
      c.domain_name = (uint32_t)ev64(ik, CDR_COL_KEY);
      c.workflow_type = (uint32_t)ev64(ik, CDR_COL_AUX);
      c.parent_close_policy = (int32_t)ev32(ik, CDR_COL_N);
      c._pad = 0;
      gput(chi + n++, c);
    }
    r.n_child = n;
    n = 0;
    GAS cdr_cancel_info* can = gp(O_.cancel) + CP.cancel_off;
#pragma unroll
    for (int j = 0; j < NX; j++) {
      if (!((r_live >> j) & 1u)) continue;
      const uint32_t iw = rl(RR0 + (uint32_t)j, lane), ik = iw & 0xFFFFFu;
      if (CARRY && ((r_cy >> j) & 1u)) {  // a loaded request-cancel, unchanged
        gput(can + n++, gget(gp(gp(B_.carry)->state.cancel) + ccy.cancel_off + iw));
        continue;
      }
      cdr_cancel_info c;
      c.version = ev64(ik, CDR_COL_VERSION);
      c.initiated_event_batch_id = ev64(ik - (iw >> 20), CDR_COL_EVENT_ID);
      c.initiated_id = (int64_t)r_id[j];
      uint64_t lo, hi;
      cdr_uuid(B_.uuid_seed, D.wf_key, CDR_UUID_CANCEL_REQ, c.initiated_id, &lo, &hi);
      c.cancel_request_lo = lo;
      c.cancel_request_hi = hi;
      gput(can + n++, c);
    }
    r.n_cancel = n;
    n = 0;
    GAS cdr_signal_info* sig = gp(O_.signal) + CP.signal_off;
#pragma unroll
    for (int j = 0; j < NX; j++) {
      if (!((g_live >> j) & 1u)) continue;
      const uint32_t iw = rl(RG0 + (uint32_t)j, lane), ik = iw & 0xFFFFFu;
      if (CARRY && ((g_cy >> j) & 1u)) {  // a loaded signal, unchanged
        gput(sig + n++, gget(gp(gp(B_.carry)->state.signal) + ccy.signal_off + iw));
        continue;
      }
      cdr_signal_info c;
      c.version = ev64(ik, CDR_COL_VERSION);
      c.initiated_event_batch_id = ev64(ik - (iw >> 20), CDR_COL_EVENT_ID);
      c.initiated_id = (int64_t)g_id[j];
      uint64_t lo, hi;
      cdr_uuid(B_.uuid_seed, D.wf_key, CDR_UUID_SIGNAL_REQ, c.initiated_id, &lo, &hi);
      c.signal_request_lo = lo;
      c.signal_request_hi = hi;
      c.signal_name = ev32(ik, CDR_COL_H);
      const uint64_t aux = (uint64_t)ev64(ik, CDR_COL_AUX);
      c.input = (uint32_t)(aux >> 32);
      c.control = (uint32_t)aux;
      c._pad = 0;
      gput(sig + n++, c);
    }
    r.n_signal = n;
    // reset points added by the replay (the Started ones are written already)
    for (uint32_t q = 0; q < n_rp; q++) {
      const uint32_t kw = rl(RP0 + 2 * q + 1, lane);
      if (kw == RNONE) continue;
      cdr_reset_point p;
      p.binary_checksum = rl(RP0 + 2 * q, lane);
      p.run_id = D.run_id;
      p.first_decision_completed_id = ev64(kw & 0x7FFFFFFFu, CDR_COL_EVENT_ID);
      p.created_time_nano = B_.now_ns;
      p.expiring_time_nano = 0;
      p.flags = CDR_RP_HAS_CHECKSUM | CDR_RP_HAS_RUN_ID | CDR_RP_HAS_FIRST_DC_ID | CDR_RP_HAS_CREATED |
                CDR_RP_HAS_RESETTABLE | ((kw & 0x80000000u) ? CDR_RP_RESETTABLE : 0u);
      p._pad = 0;
      gput(rp + q, p);
    }
  }
  // the slice holds an entry to hand on: list it for the next tier's retry pass
  if constexpr (CARRY)
    if (__builtin_amdgcn_ballot_w64(cyr) && lane == __builtin_amdgcn_readfirstlane(lane) && KA()->ocount)
      KA()->olist[atomicAdd(KA()->ocount, 1u)] = s;
  gput(gp(O_.result) + w, r);
  if (!ok) return;
  if (n_vh) gput(vh + (n_vh - 1), cdr_vh_item{vh_last_id, vh_last_ver});
  // no WorkflowExecutionStarted: its fields keep their zero values (a loaded state keeps its own)
  if (!(x_flags & CDR_XI_STARTED) && csrc < 0) {
    X->domain_id = X->workflow_id = X->run_id = X->create_request_id = 0;
    X->parent_domain_id = X->parent_workflow_id = X->parent_run_id = X->task_list = 0;
    X->workflow_type = X->cron_schedule = X->memo = X->nonretriable = X->branch_tree_id = 0;
    X->initiated_id = 0;
    X->workflow_timeout = X->attempt = X->initial_interval = X->maximum_interval = X->maximum_attempts = 0;
    X->expiration_seconds = 0;
    X->backoff_coefficient = 0.0;
    X->expiration_time = 0;
    X->branch_id_lo = X->branch_id_hi = 0;
  }
  X->decision_request_id = dreq;
  X->flags = x_flags;
  X->_pad0 = 0;
  X->completion_event_batch_id = x_completion_batch;
  X->decision_timeout_value = x_dt_timeout_value;
  X->state = x_state;
  X->close_status = x_close;
  X->last_first_event_id = call_first_id;
  X->last_event_task_id = ev64(len - 1, CDR_COL_TASK_ID);
  X->next_event_id = x_next_event;
  X->last_processed_event = x_last_processed;
  X->signal_count = x_signals;
  X->decision_timeout = dto;
  X->decision_version = dv;
  X->decision_schedule_id = dsched;
  X->decision_started_id = dstart;
  X->decision_attempt = datt;
  X->decision_started_ts = dst_ts;
  X->decision_scheduled_ts = dsc_ts;
  X->decision_original_scheduled_ts = dorig_ts;
  X->_pad1 = 0;
  X->reset_points_len = n_rp;
  X->search_attr_len = n_sa;
  if (isRS) {
    RS->current_version = prev_ver;
    if (!(x_flags & CDR_XI_STARTED) && csrc < 0) RS->start_version = D.failover_version;
    RS->last_write_version = prev_ver;
    RS->last_write_event_id = prev_id;
    for (uint32_t c = 0; c < CDR_MAX_CLUSTERS; c++) {
      const bool on = c < CDR_REG_NCL && ((rs_mask >> c) & 1u);
      const uint32_t p = RL0 + 2u * (c < CDR_REG_NCL ? c : 0u);
      RS->lri_version[c] = on ? (int64_t)rl(p, lane) : 0;
      RS->lri_last_event_id[c] = on ? (int64_t)rl(p + 1, lane) : 0;
    }
    RS->lri_mask = rs_mask;
    RS->present = 1;
  }
#undef D
#undef CP
#undef X
#undef RS
#undef vh
#undef rp
#undef sa
#undef B_
#undef O_
}
// every slice of the launch (block b: slice s0 + b) — or, after k_replay_cls (retry), the
// slices it listed as holding an entry it handed on, a few workgroups walking the list: a
// launch over every slice of the class would wait for CUs with this kernel's registers and
// LDS free only to find nothing to do in almost all of them
template <int NA, int NT, int NX, uint32_t SFLAG, int WPE = CDR_WPE_REG, bool CARRY = false, bool TASKS = false>
__global__ __launch_bounds__(CDR_SLICE_WIDTH) __attribute__((amdgpu_waves_per_eu(WPE, 8))) void k_replay_reg(
    cdr_launch L) {
  (void)L;  // read through KA()
  const bool listed = KA()->retry && KA()->rcount;
  const uint32_t n = listed ? __builtin_amdgcn_readfirstlane(*KA()->rcount) : blockIdx.x + 1u;
  for (uint32_t i = blockIdx.x; i < n; i += gridDim.x)
    reg_slice<NA, NT, NX, SFLAG, CARRY, TASKS>(listed ? __builtin_amdgcn_readfirstlane(KA()->rlist[i]) : i + KA()->s0);
}
#undef RSET
#undef RGET
