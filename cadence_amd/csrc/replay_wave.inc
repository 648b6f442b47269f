// replay_wave.inc — wave-per-workflow replay kernel (included by replay.hip).
//
// For histories whose lanes would diverge in the lane-per-workflow kernels (many
// event types interleaved: timers, signals, children, cancels — SURVEY §8(d) C3-C5)
// one wavefront replays ONE workflow (a CDR_SLICE_WAVE slice): the state machine of
// stateBuilder.go:112-611 runs as wave-uniform scalar code (SGPR state, scalar
// branches, no per-type passes), and the pending-entity tables are spread over the
// lanes — slot j of every table lives in lane j (VGPR planes), so a lookup by key is
// one vector compare + ballot, an insert one lane-masked move, a timer pick one wave
// reduction.  The slice's rows hold the workflow's events 64 at a time (event k in
// row k/64, lane k%64, cdr.h), read one row per 64 events with the next row in flight.
// Semantics are k_replay's (replay.hip) event for event; entries the planner sends
// here have at most 64 live activities, timers, children, cancels and signals at any
// time (CDR_CAP_WAVE, host.cpp caps_one); reset points and search attributes past
// the 64th are looked up in their output rows.

#ifndef CDR_WVREG
#define CDR_WVREG 0 /* 1: write-mostly wave state in VGPRs (fewer SGPR spills, but 2 waves/SIMD) */
#endif
#ifndef CDR_WFAST
#define CDR_WFAST 1 /* frequent register-only event types ahead of the switch */
#endif

namespace {
// chunk of 64 events of one workflow: lane L holds event 64r+L
struct WChunk {
  uint32_t tf, h;
  int32_t n;
  int64_t id, ver, ts, key, aux;  // task_id is read once, for the last event
};
__device__ __forceinline__ WChunk wload(rsrc_t r, uint32_t row, uint32_t nrows, uint32_t lane) {
  const uint32_t o8 = (row < nrows ? row * CDR_ROW_BYTES : OOB_BIT) + lane * 8u, o4 = o8 - lane * 4u;
  WChunk c;
  c.id = bld64(r, o8, cdr_col_off(CDR_COL_EVENT_ID));
  c.ver = bld64(r, o8, cdr_col_off(CDR_COL_VERSION));
  c.ts = bld64(r, o8, cdr_col_off(CDR_COL_TIMESTAMP));
  c.key = bld64(r, o8, cdr_col_off(CDR_COL_KEY));
  c.aux = bld64(r, o8, cdr_col_off(CDR_COL_AUX));
  c.tf = bld32(r, o4, cdr_col_off(CDR_COL_TYPE_FLAGS));
  c.h = bld32(r, o4, cdr_col_off(CDR_COL_H));
  c.n = (int32_t)bld32(r, o4, cdr_col_off(CDR_COL_N));
  return c;
}
__device__ __forceinline__ uint32_t rl32(uint32_t v, uint32_t j) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)j);
}
__device__ __forceinline__ int64_t rl64(int64_t v, uint32_t j) {
  const uint64_t u = (uint64_t)v;
  return (int64_t)(((uint64_t)rl32((uint32_t)(u >> 32), j) << 32) | rl32((uint32_t)u, j));
}
__device__ __forceinline__ uint32_t u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ int64_t u64(int64_t v) { return rl64(v, 0); }
__device__ __forceinline__ uint64_t below(uint32_t n) {  // lanes [0, n)
  return n >= 64 ? ~0ull : ((1ull << n) - 1ull);
}
__device__ __forceinline__ int first_lane(uint64_t m) { return m ? (int)__builtin_ctzll(m) : -1; }
__device__ __forceinline__ int last_lane(uint64_t m) { return m ? 63 - (int)__builtin_clzll(m) : -1; }
// wave-wide minimum of an unsigned 64-bit key (every lane gets it)
__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const uint64_t o = __shfl_xor(v, m, 64);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t okey(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ull; }
// lane of the smallest (k1, k2) among lanes with `on` (-1 if none); ties on both keys
// go to the lowest lane
__device__ __forceinline__ int wave_argmin2(bool on, int64_t k1, int64_t k2) {
  const uint64_t a = on ? okey(k1) : ~0ull;
  const uint64_t m1 = wave_min(a);
  const uint64_t t1 = __builtin_amdgcn_ballot_w64(on && a == m1);
  if (!t1) return -1;
  if ((t1 & (t1 - 1)) == 0) return (int)__builtin_ctzll(t1);
  const uint64_t b = (on && a == m1) ? okey(k2) : ~0ull;
  const uint64_t m2 = wave_min(b);
  return first_lane(__builtin_amdgcn_ballot_w64(on && a == m1 && b == m2));
}
}  // namespace

#define WPUT(plane, j, v) plane = (lane == (uint32_t)(j)) ? (v) : plane
#define WGET(plane, j) rl64(plane, (uint32_t)(j))

#ifndef CDR_WPE_WAVE
#define CDR_WPE_WAVE 4
#endif
__global__ __launch_bounds__(CDR_SLICE_WIDTH) __attribute__((amdgpu_waves_per_eu(CDR_WPE_WAVE, 8))) void k_replay_wave(
    cdr_launch L) {
  (void)L;  // read through KA()
  const uint32_t s = blockIdx.x + KA()->s0;
  const uint32_t lane = threadIdx.x;
  if (s >= KA()->B.ev.n_slices) return;
  if (!(u32(KA()->B.ev.slice_flags[s]) & CDR_SLICE_WAVE)) return;
  const int32_t w = (int32_t)u32((uint32_t)KA()->B.ev.lane_wf[(uint64_t)s * CDR_SLICE_WIDTH]);
  if (w < 0 || (KA()->B.skip && KA()->B.skip[w])) return;  // empty slice / masked entry
  const uint64_t row0 = (uint64_t)u64((int64_t)KA()->B.ev.slice_row0[s]);
  const uint32_t nrows = u32(KA()->B.ev.slice_len[s]);
  const rsrc_t R = __builtin_amdgcn_make_buffer_rsrc((void*)(KA()->B.ev.slab + row0 * CDR_ROW_BYTES), (short)0,
                                                     (int)(nrows * CDR_ROW_BYTES), 0x00020000);
#define B_ (KA()->B)
#define O_ (KA()->O)
#define D (gp(B_.wfs)[w])
#define CP (gp(B_.caps)[w])
#define X (gp(O_.exec) + w)
#define RS (gp(O_.repl) + w)
#define chi (gp(O_.child) + CP.child_off)
#define can (gp(O_.cancel) + CP.cancel_off)
#define sig (gp(O_.signal) + CP.signal_off)
#define vh (gp(O_.vh) + CP.vh_off)
#define rp (gp(O_.rp) + CP.rp_off)
#define sa (gp(O_.sa) + CP.sa_off)
  const bool L0 = lane == 0;  // the lane that performs the workflow's scalar stores
  const uint32_t len = u32((uint32_t)D.ev_len);
  const uint32_t builder = u32(D.builder);
  const uint32_t EU = u32(B_.empty_uuid);
  const bool isRS = builder == CDR_BUILDER_2DC;
  const bool isVH = builder == CDR_BUILDER_NDC;
  const uint32_t vh_cap = u32(CP.vh_cap);

  // ---- pending-entity tables: slot j in lane j
  int64_t a_sid = DEAD_KEY, a_ts2c = 0, a_talt = 0, a_thb = 0, a_meta = 0, a_ver = 0, a_stid = 0, a_stime = 0,
          a_cancel = 0, a_rows = 0, a_stchb = 0, a_req = 0;
  int64_t t_sid = DEAD_KEY, t_tt = 0, t_exp = 0, t_ver = 0;
  int64_t c_key = DEAD_KEY, r_key = DEAD_KEY, g_key = DEAD_KEY;  // children, cancels, signals (initiated id)
  uint32_t ck = 0;       // binary checksum of reset point j (0: none)
  uint32_t sa_key = 0;   // search attribute j's key
  uint32_t hw_act = 0, hw_tim = 0, hw_chi = 0, hw_can = 0, hw_sig = 0;
  uint32_t live_chi = 0, live_can = 0, live_sig = 0, n_rp = 0, n_sa = 0;

  uint32_t x_flags = 0;
  int64_t x_completion_batch = 0, x_next_event = CDR_FIRST_EVENT_ID, x_last_processed = CDR_EMPTY_EVENT_ID;
  int32_t x_dt_timeout_value = 0, x_state = CDR_STATE_CREATED, x_close = CDR_CLOSE_NONE, x_signals = 0;
  int64_t dv = CDR_EMPTY_VERSION, dsched = CDR_EMPTY_EVENT_ID, dstart = CDR_EMPTY_EVENT_ID, datt = 0, dst_ts = 0,
          dsc_ts = 0, dorig_ts = 0;
  uint32_t dreq = EU;
  int32_t dto = 0;
  uint32_t ld = 0;  // lastDecision bookkeeping (ld_write)
  const bool want_ld = O_.last_decision != nullptr;
  // lastDecision: the record of a pending source event, before a clearing event
  auto ld_capture = [&]() __attribute__((always_inline)) {
    if (ld_pending(ld)) {
      if (L0 && want_ld)
        ld_write(gp(O_.last_decision) + w, ld, dv, dsched, dstart, dreq, dto, datt, dsc_ts, dst_ts, dorig_ts);
      ld |= LD_CAPTURED;
    }
  };
  int64_t curv = u64(D.failover_version);
  uint32_t rs_mask = 0;
  int64_t vh_last_id = 0, vh_last_ver = 0;
  uint32_t n_vh = 0;
  int64_t call_first_id = 0, prev_id = 0, prev_ver = 0;
  uint32_t call_first_k = 0, call_idx = 0;
  bool newrun_applied = false, stop_at_call_end = false;
  uint32_t nr_call = 0xFFFFFFFFu;  // the call that applied the new run (a cluster panic there: never attempted)
  int32_t err = len == 0 ? CDR_E_HISTORY_EMPTY : CDR_OK;
  int64_t err_id = 0;
  uint32_t err_k = 0;
  bool done = len == 0;
#if CDR_WVREG
  // write-mostly state lives in VGPRs (an opaque move makes the compiler treat it as
  // per-lane): the SGPR file keeps the hot scalars and spills less
#define VREG(x) asm volatile("" : "+v"(x))
  VREG(dv);
  VREG(dstart);
  VREG(dreq);
  VREG(dto);
  VREG(datt);
  VREG(dst_ts);
  VREG(dsc_ts);
  VREG(dorig_ts);
  VREG(x_last_processed);
  VREG(x_completion_batch);
  VREG(x_dt_timeout_value);
  VREG(x_close);
  VREG(err_id);
  VREG(err_k);
  VREG(x_signals);
#undef VREG
#endif
  // ClusterNameForFailoverVersion of the last version asked (versions change rarely)
  int64_t cv_ver = 0;
  int cv_src = -1;
  bool cv_ok = false;
  auto cluster_of = [&](int64_t v) {
    if (!cv_ok || v != cv_ver) {
      cv_ok = true;
      cv_ver = v;
      cv_src = cluster_for_version(B_.cluster, v);
    }
    return cv_src;
  };

#define FAILW(code)  \
  do {               \
    err = (code);    \
    err_id = e.id;   \
    err_k = k;       \
    stop_at_call_end = true; \
  } while (0)

  // activity timer pick (timerBuilder.go:211-312) over the live slots: a wave argmin
  // of (time, schedule id) after each lane picks its activity's earliest timer
  auto act_pick = [&]() {
    const bool on = lane < hw_act && a_sid != DEAD_KEY;
    const bool pa = a_talt < a_ts2c;
    const int64_t t1 = pa ? a_talt : a_ts2c;
    const bool ph = a_thb < t1;
    const int64_t t = ph ? a_thb : t1;
    const uint32_t bit = ph ? CDR_TTS_HEARTBEAT
                            : (pa ? (((uint64_t)a_meta & META_FLAG(AF_STARTED)) ? CDR_TTS_START_TO_CLOSE
                                                                                : CDR_TTS_SCHEDULE_TO_START)
                                  : CDR_TTS_SCHEDULE_TO_CLOSE);
    const int b = wave_argmin2(on, t, a_sid);
    if (b >= 0) {
      const uint64_t m = (uint64_t)WGET(a_meta, b);
      const uint64_t bb = (uint64_t)rl32(bit, (uint32_t)b) << META_TTS_SHIFT;
      if (!(m & bb)) WPUT(a_meta, b, (int64_t)(m | bb));
    }
  };
  // user timer pick (timerBuilder.go:171-184,233-247): head by (ExpiryTime, StartedID)
  auto tim_pick = [&]() {
    const bool on = lane < hw_tim && t_sid != DEAD_KEY;
    const int b = wave_argmin2(on, t_exp, t_sid);
    if (b >= 0) {
      const uint64_t v = (uint64_t)WGET(t_tt, b);
      if ((v >> 32) != CDR_TIMER_TASK_STATUS_CREATED)
        WPUT(t_tt, b, (int64_t)((v & 0xFFFFFFFFull) | ((uint64_t)CDR_TIMER_TASK_STATUS_CREATED << 32)));
    }
  };

  // events of one chunk (row r): false once the replay is over
  auto run_chunk = [&](const WChunk& cur, const uint32_t r) __attribute__((always_inline)) -> bool {
  for (uint32_t j = 0; j < 64u; j++) {
    const uint32_t k = r * 64u + j;
    if (k >= len) return false;
    struct {
      uint32_t tf, h;
      int32_t n;
      int64_t id, ver, ts, key, aux;
    } e;
    e.tf = rl32(cur.tf, j);
    e.id = rl64(cur.id, j);
    e.ver = rl64(cur.ver, j);
    const uint32_t type = e.tf & 0xFFu;
    // ---- call boundary (stateBuilder.go:603-604 of the previous call; 2DC replication
    // state sourced from the call's last event, mutableStateBuilder.go:561-581)
    const bool bf = (e.tf & CDR_SEF_BATCH_FIRST) || k == 0;
    const bool end_call = bf && k > 0;
    if (isRS && end_call) {
      const int src = cluster_of(prev_ver);
      if (src < 0) {
        err = CDR_P_UNKNOWN_CLUSTER;
        err_id = call_first_id;
        err_k = call_first_k;
        newrun_applied = newrun_applied && nr_call != call_idx;
      } else if (src != B_.cluster.current_cluster) {
        if (L0) {
          RS->lri_version[src] = prev_ver;
          RS->lri_last_event_id[src] = prev_id;
        }
        rs_mask |= 1u << src;
      }
    }
    if (end_call && err != CDR_OK) return false;  // a failed call ends the replay
    if (end_call) {
      x_next_event = prev_id + 1;
      call_idx++;
    }
    if (bf) {
      call_first_id = e.id;
      call_first_k = k;
      ld = 0;
    }
    prev_id = e.id;
    prev_ver = e.ver;
    if (stop_at_call_end) continue;  // rest of a failed call: only its last event matters (2DC)
    e.ts = rl64(cur.ts, j);
    e.key = rl64(cur.key, j);
    e.aux = rl64(cur.aux, j);
    e.h = rl32(cur.h, j);
    e.n = (int32_t)rl32((uint32_t)cur.n, j);
    // ---- version prelude (stateBuilder.go:134-154)
    if (isVH) {
      if (x_state == CDR_STATE_CREATED || x_state == CDR_STATE_RUNNING) curv = e.ver;
      const bool newitem = n_vh == 0 || e.ver > vh_last_ver;
      const int32_t code = (e.id < 0 || (e.ver < 0 && e.ver != CDR_EMPTY_VERSION)) ? CDR_P_VH_ITEM_INVALID
                           : (n_vh != 0 && e.ver < vh_last_ver)                     ? CDR_E_VH_LOWER_VERSION
                           : (n_vh != 0 && e.id <= vh_last_id)                      ? CDR_E_VH_LOWER_EVENT_ID
                           : (newitem && n_vh >= vh_cap)                            ? CDR_E_BAD_INPUT
                                                                                    : CDR_OK;
      if (code != CDR_OK) {
        FAILW(code);
        continue;
      }
      if (newitem) {
        if (n_vh != 0 && L0) gput(vh + (n_vh - 1), cdr_vh_item{vh_last_id, vh_last_ver});
        n_vh++;
        vh_last_ver = e.ver;
      }
      vh_last_id = e.id;
    }
#if CDR_WFAST
    // the most frequent register-only types first (a short compare chain instead of
    // the switch's search tree); semantics as in their switch cases below
    if (type == CDR_EV_WF_SIGNALED) {
      x_signals++;
      continue;
    }
    if (type == CDR_EV_DT_SCHEDULED) {
      dv = e.ver;
      dsched = e.id;
      dstart = CDR_EMPTY_EVENT_ID;
      dreq = EU;
      dto = e.n;
      datt = e.aux;
      dsc_ts = e.ts;
      dst_ts = 0;
      dorig_ts = e.ts;
      ld = ld_make(CDR_LD_SCHEDULED, k);
      continue;
    }
    if (type == CDR_EV_DT_STARTED && e.key == dsched) {
      if (x_state == CDR_STATE_CREATED) x_state = CDR_STATE_RUNNING;
      dv = e.ver;
      dstart = e.id;
      dreq = e.h;
      datt = 0;
      dst_ts = e.ts;
      ld = ld_make(CDR_LD_STARTED, k);
      continue;
    }
#endif
    // ---- dispatch (stateBuilder.go:157-600), wave-uniform
    switch (type) {
      case CDR_EV_WF_STARTED: {  // stateBuilder.go:158-184 -> mutableStateBuilder.go:1639-1716
        ld_capture();  // a later Started resets the decision fields
        const GAS cdr_attr_wf_started* a = gp((const cdr_attr_wf_started*)(B_.ev.arena + (uint64_t)e.aux));
        const uint32_t af = u32(a->flags);
        if ((af & CDR_SF_HAS_PARENT_DOMAIN) && (af & CDR_SF_PARENT_DOMAIN_MISSING)) {
          FAILW(CDR_E_DOMAIN_NOT_FOUND);
          break;
        }
        if (!transition_ok(x_state, x_close, CDR_STATE_CREATED, CDR_CLOSE_NONE)) {
          FAILW(CDR_E_INVALID_STATE_TRANSITION);
          break;
        }
        const bool first = !(x_flags & CDR_XI_STARTED);  // fields absent from a first Started stay zero
        uint32_t xf = x_flags;
        if (L0) {
          X->domain_id = D.domain_id;
          X->workflow_id = D.workflow_id;
          X->run_id = D.run_id;
          X->create_request_id = D.request_id;
          X->task_list = a->task_list;
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
          if (a->expiration_ts != 0) X->expiration_time = a->expiration_ts;
          else if (first) X->expiration_time = 0;
          if (af & CDR_SF_HAS_RETRY) {
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
          if (af & CDR_SF_HAS_MEMO) X->memo = a->memo;
          else if (first) X->memo = 0;
          uint64_t lo, hi;  // SetHistoryTree (:313-339)
          cdr_uuid(B_.uuid_seed, D.wf_key, CDR_UUID_BRANCH, e.id, &lo, &hi);
          X->branch_tree_id = D.run_id;
          X->branch_id_lo = lo;
          X->branch_id_hi = hi;
          if (isRS) RS->start_version = e.ver;  // :182-184
        }
        if (u64(a->expiration_ts) != 0) xf |= CDR_XI_HAS_EXPIRATION;
        if (af & CDR_SF_HAS_RETRY) xf |= CDR_XI_HAS_RETRY;
        if (af & CDR_SF_HAS_MEMO) xf |= CDR_XI_HAS_MEMO;
        // rolloverAutoResetPointsWithExpiringTime (:3184-3205), one reset point per lane
        xf &= ~CDR_XI_HAS_RESET_POINTS;
        n_rp = 0;
        ck = 0;
        if (af & CDR_SF_HAS_RESET_POINTS) {
          xf |= CDR_XI_HAS_RESET_POINTS;
          const int64_t expiring = e.ts + (int64_t)u32((uint32_t)D.retention_days) * 24ll * 3600ll * NS_PER_S;
          const uint32_t crun = u32(a->continued_run_id), off = u32(a->reset_points_off);
          const uint32_t cnt = u32(a->reset_points_len), cap = u32(CP.rp_cap);
          const uint32_t m = cnt < cap ? cnt : cap;
          if (cnt > cap) FAILW(CDR_E_BAD_INPUT);  // the rolled-over points do not fit the slice
          for (uint32_t q0 = 0; q0 < m; q0 += 64) {
            const uint32_t q = q0 + lane;
            if (q < m) {
              cdr_reset_point p = gget(gp(B_.rps) + (off + q));
              const uint32_t run = (p.flags & CDR_RP_HAS_RUN_ID) ? p.run_id : 0u;
              if (run == crun) {
                p.flags |= CDR_RP_HAS_EXPIRING;
                p.expiring_time_nano = expiring;
              }
              gput(rp + q, p);
              if (q0 == 0) ck = (p.flags & CDR_RP_HAS_CHECKSUM) ? p.binary_checksum : 0u;
            }
          }
          n_rp = m;
        }
        if (af & CDR_SF_HAS_SEARCH_ATTR) {
          const uint32_t off = u32(a->search_attr_off), cnt = u32(a->search_attr_len), cap = u32(CP.sa_cap);
          const uint32_t m = cnt < cap ? cnt : cap;
          if (cnt > cap) FAILW(CDR_E_BAD_INPUT);  // the search attributes do not fit the slice
          for (uint32_t q0 = 0; q0 < m; q0 += 64) {  // pairs past the lanes live in the rows only
            const uint32_t q = q0 + lane;
            if (q < m) {
              const cdr_kv kv = gget(gp(B_.kvs) + (off + q));
              gput(sa + q, kv);
              if (q0 == 0) sa_key = kv.key;
            }
          }
          n_sa = m;
          if (m) xf |= CDR_XI_HAS_SEARCH_ATTR;
          else xf &= ~CDR_XI_HAS_SEARCH_ATTR;
        }
        xf |= CDR_XI_STARTED | (isVH ? CDR_XI_VH_BRANCH : CDR_XI_HAS_BRANCH);
        x_flags = xf;
        x_dt_timeout_value = (int32_t)u32((uint32_t)a->task_timeout_s);
        x_state = CDR_STATE_CREATED;
        x_close = CDR_CLOSE_NONE;
        x_last_processed = CDR_EMPTY_EVENT_ID;
        dv = CDR_EMPTY_VERSION;
        dsched = CDR_EMPTY_EVENT_ID;
        dstart = CDR_EMPTY_EVENT_ID;
        dreq = EU;
        dto = 0;
        break;
      }
      case CDR_EV_DT_SCHEDULED:  // :186-200 -> mutableStateDecisionTaskManager.go:143-167
        dv = e.ver;
        dsched = e.id;
        dstart = CDR_EMPTY_EVENT_ID;
        dreq = EU;
        dto = e.n;
        datt = e.aux;
        dsc_ts = e.ts;
        dst_ts = 0;
        dorig_ts = e.ts;
        ld = ld_make(CDR_LD_SCHEDULED, k);
        break;
      case CDR_EV_DT_STARTED:  // :202-213 -> :200-253
        if (e.key != dsched) {
          FAILW(CDR_E_DECISION_NOT_FOUND);
          break;
        }
        if (x_state == CDR_STATE_CREATED) x_state = CDR_STATE_RUNNING;
        dv = e.ver;
        dstart = e.id;
        dreq = e.h;
        datt = 0;
        dst_ts = e.ts;
        ld = ld_make(CDR_LD_STARTED, k);
        break;
      case CDR_EV_DT_COMPLETED: {  // :215-219 -> :255-262,659-674,789-800
        ld_capture();
        dv = CDR_EMPTY_VERSION;
        dsched = CDR_EMPTY_EVENT_ID;
        dstart = CDR_EMPTY_EVENT_ID;
        dreq = EU;
        dto = 0;
        datt = 0;
        dst_ts = 0;
        dsc_ts = 0;  // OriginalScheduledTimestamp kept
        x_last_processed = e.aux;
        const uint32_t cks = e.h;
        if (cks != 0) {  // addBinaryCheckSumIfNotExists (mutableStateBuilder.go:1798-1842)
          bool exists = __builtin_amdgcn_ballot_w64(lane < n_rp && ck == cks) != 0;
          for (uint32_t q = 64; !exists && q < n_rp; q++) {  // past the lanes: the rows themselves
            const cdr_reset_point p = gget(rp + q);
            exists = u32((p.flags & CDR_RP_HAS_CHECKSUM) ? p.binary_checksum : 0u) == cks;
          }
          if (!exists) {
            if (n_rp >= u32(CP.rp_cap)) {
              FAILW(CDR_E_BAD_INPUT);
              break;
            }
            if (L0) {
              const bool resettable = live_chi == 0 && live_can == 0 && live_sig == 0;
              cdr_reset_point p;
              p.binary_checksum = cks;
              p.run_id = D.run_id;
              p.first_decision_completed_id = e.id;
              p.created_time_nano = B_.now_ns;
              p.expiring_time_nano = 0;
              p.flags = CDR_RP_HAS_CHECKSUM | CDR_RP_HAS_RUN_ID | CDR_RP_HAS_FIRST_DC_ID | CDR_RP_HAS_CREATED |
                        CDR_RP_HAS_RESETTABLE | (resettable ? CDR_RP_RESETTABLE : 0u);
              p._pad = 0;
              gput(rp + n_rp, p);
            }
            if (lane == n_rp) ck = cks;
            n_rp++;
            x_flags |= CDR_XI_HAS_RESET_POINTS;
          }
        }
        break;
      }
      case CDR_EV_DT_TIMED_OUT:  // :221-239 -> FailDecision :635-656 + transient :169-198
      case CDR_EV_DT_FAILED: {   // :241-257
        ld_capture();
        const bool inc = type == CDR_EV_DT_FAILED || e.n != CDR_TIMEOUT_SCHEDULE_TO_START;
        const int64_t now = B_.now_ns;
        const int64_t na = inc ? datt + 1 : 0;
        const bool tr = na != 0;
        if (tr) ld = ld_make(CDR_LD_TRANSIENT, k);
        dv = tr ? (isRS ? e.ver : (isVH ? curv : CDR_EMPTY_VERSION)) : CDR_EMPTY_VERSION;
        dsched = tr ? x_next_event : CDR_EMPTY_EVENT_ID;
        dstart = CDR_EMPTY_EVENT_ID;
        dreq = EU;
        dto = tr ? x_dt_timeout_value : 0;
        dst_ts = 0;
        dorig_ts = 0;
        dsc_ts = (tr || inc) ? now : (int64_t)0;
        datt = na;
        break;
      }
      case CDR_EV_AT_SCHEDULED: {  // :259-269 -> mutableStateBuilder.go:1982-2028
        const uint32_t aid = (uint32_t)e.key;
        const bool in = lane < hw_act;
        // byActivityID[aid] is overwritten: drop the mapping flag of the old holder
        if (in && a_sid != DEAD_KEY && (uint32_t)a_meta == aid && ((uint64_t)a_meta & META_FLAG(AF_AIDMAP)))
          a_meta = (int64_t)((uint64_t)a_meta & ~META_FLAG(AF_AIDMAP));
        int slot = first_lane(__builtin_amdgcn_ballot_w64(in && a_sid == DEAD_KEY));
        if (slot < 0) {
          if (hw_act >= u32(CP.act_cap) || hw_act >= 64) {
            FAILW(CDR_E_BAD_INPUT);
            break;
          }
          slot = (int)hw_act++;
        }
        const int32_t s2c = (int32_t)e.h, s2s = e.n;
        if (lane == (uint32_t)slot) {
          a_sid = e.id;
          a_ts2c = e.ts + (int64_t)s2c * NS_PER_S;
          a_talt = e.ts + (int64_t)s2s * NS_PER_S;
          a_thb = T_NONE;
          a_meta = (int64_t)(aid | META_FLAG(AF_AIDMAP));
          a_ver = e.ver;
          a_stid = CDR_EMPTY_EVENT_ID;
          a_stime = 0;
          a_cancel = CDR_EMPTY_EVENT_ID;
          a_rows = (int64_t)(k | ((uint64_t)call_first_k << 32));
          a_stchb = (int64_t)(((uint64_t)e.key >> 32) | ((uint64_t)e.aux & 0xFFFFFFFF00000000ull));
          a_req = 0;
        }
        act_pick();
        break;
      }
      case CDR_EV_AT_STARTED: {  // :271-278 -> :2083-2098
        const int slot = last_lane(__builtin_amdgcn_ballot_w64(lane < hw_act && a_sid == e.key));
        if (slot < 0) {
          FAILW(CDR_P_ACTIVITY_STARTED_NIL);  // nil deref in Go
          break;
        }
        if (lane == (uint32_t)slot) {
          const uint64_t th = (uint64_t)a_stchb;
          const int32_t stc = (int32_t)(uint32_t)th, hb = (int32_t)(uint32_t)(th >> 32);
          a_ver = e.ver;
          a_stid = e.id;
          a_req = (int64_t)e.h;
          a_stime = e.ts;  // LastHeartBeatUpdatedTime = StartedTime
          a_meta = (int64_t)((uint64_t)a_meta | META_FLAG(AF_STARTED));
          a_talt = e.ts + (int64_t)stc * NS_PER_S;
          a_thb = hb > 0 ? e.ts + (int64_t)hb * NS_PER_S : T_NONE;
        }
        act_pick();
        break;
      }
      case CDR_EV_AT_COMPLETED:  // :280-305,312-319 -> DeleteActivity :1247-1269
      case CDR_EV_AT_FAILED:
      case CDR_EV_AT_TIMED_OUT:
      case CDR_EV_AT_CANCELED: {
        const int slot = last_lane(__builtin_amdgcn_ballot_w64(lane < hw_act && a_sid == e.key));
        if (slot < 0) {
          FAILW(CDR_E_ACTIVITY_NOT_FOUND);
          break;
        }
        const uint64_t m = (uint64_t)WGET(a_meta, slot);
        const uint32_t aid = (uint32_t)m;
        if (lane == (uint32_t)slot) {
          a_sid = DEAD_KEY;
          a_meta = (int64_t)(m & ~META_FLAG(AF_AIDMAP));
        }
        bool found = (m & META_FLAG(AF_AIDMAP)) != 0;
        if (!found) {
          const bool hit = lane < hw_act && a_sid != DEAD_KEY && (uint32_t)a_meta == aid &&
                           ((uint64_t)a_meta & META_FLAG(AF_AIDMAP));
          if (hit) a_meta = (int64_t)((uint64_t)a_meta & ~META_FLAG(AF_AIDMAP));
          found = __builtin_amdgcn_ballot_w64(hit) != 0;
        }
        if (!found) {
          FAILW(CDR_E_ACTIVITY_ID_NOT_FOUND);
          break;
        }
        act_pick();
        break;
      }
      case CDR_EV_AT_CANCEL_REQUESTED: {  // :307-310 -> :2264-2285
        const uint32_t aid = (uint32_t)e.key;
        const int slot = last_lane(__builtin_amdgcn_ballot_w64(lane < hw_act && a_sid != DEAD_KEY &&
                                                              (uint32_t)a_meta == aid &&
                                                              ((uint64_t)a_meta & META_FLAG(AF_AIDMAP))));
        if (slot < 0) {
          FAILW(CDR_E_MISSING_ACTIVITY_INFO);
          break;
        }
        if (lane == (uint32_t)slot) {
          a_ver = e.ver;
          a_meta = (int64_t)((uint64_t)a_meta | META_FLAG(AF_CANCEL));
          a_cancel = e.id;
        }
        break;
      }
      case CDR_EV_TIMER_STARTED: {  // :324-332 -> :2877-2900
        const uint32_t tid = (uint32_t)e.key;
        const bool in = lane < hw_tim;
        int slot = last_lane(__builtin_amdgcn_ballot_w64(in && t_sid != DEAD_KEY && (uint32_t)t_tt == tid));
        if (slot < 0) slot = first_lane(__builtin_amdgcn_ballot_w64(in && t_sid == DEAD_KEY));
        if (slot < 0) {
          if (hw_tim >= u32(CP.timer_cap) || hw_tim >= 64) {
            FAILW(CDR_E_BAD_INPUT);
            break;
          }
          slot = (int)hw_tim++;
        }
        if (lane == (uint32_t)slot) {
          t_sid = e.id;
          t_tt = (int64_t)tid;  // TaskID = TimerTaskStatusNone
          t_exp = e.ts + e.aux * NS_PER_S;
          t_ver = e.ver;
        }
        tim_pick();
        break;
      }
      case CDR_EV_TIMER_FIRED:       // :334-341
      case CDR_EV_TIMER_CANCELED: {  // :343-350
        const uint32_t tid = (uint32_t)e.key;
        if (lane < hw_tim && t_sid != DEAD_KEY && (uint32_t)t_tt == tid) t_sid = DEAD_KEY;
        tim_pick();
        break;
      }
      case CDR_EV_CHILD_INITIATED: {  // :355-371 -> :3256-3280
        int slot = first_lane(__builtin_amdgcn_ballot_w64(lane < hw_chi && c_key == DEAD_KEY));
        if (slot < 0) {
          if (hw_chi >= u32(CP.child_cap) || hw_chi >= 64) {
            FAILW(CDR_E_BAD_INPUT);
            break;
          }
          slot = (int)hw_chi++;
        }
        if (L0) {
          cdr_child_info c;
          c.version = e.ver;
          c.initiated_id = e.id;
          c.initiated_event_batch_id = call_first_id;
          c.started_id = CDR_EMPTY_EVENT_ID;
          uint64_t lo, hi;
          cdr_uuid(B_.uuid_seed, D.wf_key, CDR_UUID_CHILD_REQ, e.id, &lo, &hi);
          c.create_request_lo = lo;
          c.create_request_hi = hi;
          c.started_workflow_id = e.h;
          c.started_run_id = 0;
          c.domain_name = (uint32_t)e.key;
          c.workflow_type = (uint32_t)e.aux;
          c.parent_close_policy = e.n;
          c._pad = 0;
          gput(chi + slot, c);
        }
        WPUT(c_key, slot, e.id);
        live_chi++;
        if (e.tf & CDR_SEF_DOMAIN_MISSING) FAILW(CDR_E_DOMAIN_NOT_FOUND);
        break;
      }
      case CDR_EV_CHILD_STARTED: {  // :378-381 -> :3312-3325
        const int slot = first_lane(__builtin_amdgcn_ballot_w64(lane < hw_chi && c_key == e.key));
        if (slot < 0) {
          FAILW(CDR_P_CHILD_STARTED_NIL);
          break;
        }
        if (L0) {
          chi[slot].started_id = e.id;
          chi[slot].started_run_id = e.h;
        }
        break;
      }
      case CDR_EV_CHILD_START_FAILED:
      case CDR_EV_CHILD_COMPLETED:
      case CDR_EV_CHILD_FAILED:
      case CDR_EV_CHILD_CANCELED:
      case CDR_EV_CHILD_TIMED_OUT:
      case CDR_EV_CHILD_TERMINATED: {  // DeletePendingChildExecution :1138-1144
        const int slot = first_lane(__builtin_amdgcn_ballot_w64(lane < hw_chi && c_key == e.key));
        if (slot >= 0) {
          if (L0) chi[slot].initiated_id = DEAD_KEY;
          WPUT(c_key, slot, DEAD_KEY);
          live_chi--;
        }
        break;
      }
      case CDR_EV_RCE_INITIATED: {  // :408-427 -> :2577-2596
        int slot = first_lane(__builtin_amdgcn_ballot_w64(lane < hw_can && r_key == DEAD_KEY));
        if (slot < 0) {
          if (hw_can >= u32(CP.cancel_cap) || hw_can >= 64) {
            FAILW(CDR_E_BAD_INPUT);
            break;
          }
          slot = (int)hw_can++;
        }
        if (L0) {
          cdr_cancel_info c;
          c.version = e.ver;
          c.initiated_event_batch_id = call_first_id;
          c.initiated_id = e.id;
          uint64_t lo, hi;
          cdr_uuid(B_.uuid_seed, D.wf_key, CDR_UUID_CANCEL_REQ, e.id, &lo, &hi);
          c.cancel_request_lo = lo;
          c.cancel_request_hi = hi;
          gput(can + slot, c);
        }
        WPUT(r_key, slot, e.id);
        live_can++;
        if (e.tf & CDR_SEF_DOMAIN_MISSING) FAILW(CDR_E_DOMAIN_NOT_FOUND);
        break;
      }
      case CDR_EV_RCE_FAILED:
      case CDR_EV_EXT_CANCEL_REQUESTED: {  // DeletePendingRequestCancel :1147-1153
        const int slot = first_lane(__builtin_amdgcn_ballot_w64(lane < hw_can && r_key == e.key));
        if (slot >= 0) {
          if (L0) can[slot].initiated_id = DEAD_KEY;
          WPUT(r_key, slot, DEAD_KEY);
          live_can--;
        }
        break;
      }
      case CDR_EV_SE_INITIATED: {  // :439-458 -> :2701-2723
        int slot = first_lane(__builtin_amdgcn_ballot_w64(lane < hw_sig && g_key == DEAD_KEY));
        if (slot < 0) {
          if (hw_sig >= u32(CP.signal_cap) || hw_sig >= 64) {
            FAILW(CDR_E_BAD_INPUT);
            break;
          }
          slot = (int)hw_sig++;
        }
        if (L0) {
          cdr_signal_info c;
          c.version = e.ver;
          c.initiated_event_batch_id = call_first_id;
          c.initiated_id = e.id;
          uint64_t lo, hi;
          cdr_uuid(B_.uuid_seed, D.wf_key, CDR_UUID_SIGNAL_REQ, e.id, &lo, &hi);
          c.signal_request_lo = lo;
          c.signal_request_hi = hi;
          c.signal_name = e.h;
          c.input = (uint32_t)((uint64_t)e.aux >> 32);
          c.control = (uint32_t)e.aux;
          c._pad = 0;
          gput(sig + slot, c);
        }
        WPUT(g_key, slot, e.id);
        live_sig++;
        if (e.tf & CDR_SEF_DOMAIN_MISSING) FAILW(CDR_E_DOMAIN_NOT_FOUND);
        break;
      }
      case CDR_EV_SE_FAILED:
      case CDR_EV_EXT_SIGNALED: {  // DeletePendingSignal :1156-1162
        const int slot = first_lane(__builtin_amdgcn_ballot_w64(lane < hw_sig && g_key == e.key));
        if (slot >= 0) {
          if (L0) sig[slot].initiated_id = DEAD_KEY;
          WPUT(g_key, slot, DEAD_KEY);
          live_sig--;
        }
        break;
      }
      case CDR_EV_AT_REQ_CANCEL_FAILED:
      case CDR_EV_CANCEL_TIMER_FAILED:
      case CDR_EV_MARKER_RECORDED:
        break;
      case CDR_EV_WF_SIGNALED:  // :473-476
        x_signals++;
        break;
      case CDR_EV_WF_CANCEL_REQUESTED:  // :478-481
        x_flags |= CDR_XI_CANCEL_REQUESTED;
        break;
      case CDR_EV_WF_COMPLETED:
      case CDR_EV_WF_FAILED:
      case CDR_EV_WF_TIMED_OUT:
      case CDR_EV_WF_CANCELED:
      case CDR_EV_WF_TERMINATED: {  // :483-531
        const int cs = type == CDR_EV_WF_COMPLETED   ? CDR_CLOSE_COMPLETED
                       : type == CDR_EV_WF_FAILED    ? CDR_CLOSE_FAILED
                       : type == CDR_EV_WF_TIMED_OUT ? CDR_CLOSE_TIMED_OUT
                       : type == CDR_EV_WF_CANCELED  ? CDR_CLOSE_CANCELED
                                                     : CDR_CLOSE_TERMINATED;
        if (!transition_ok(x_state, x_close, CDR_STATE_COMPLETED, cs)) {
          FAILW(CDR_E_INVALID_STATE_TRANSITION);
          break;
        }
        x_state = CDR_STATE_COMPLETED;
        x_close = cs;
        x_completion_batch = call_first_id;
        break;
      }
      case CDR_EV_UPSERT_SA: {  // :533-535 -> :2746-2768 (last writer per key)
        const uint64_t off = (uint64_t)e.aux;
        const uint32_t cnt = e.h, cap = u32(CP.sa_cap);
        for (uint32_t q = 0; q < cnt; q++) {
          const cdr_kv kv = gget(gp(B_.kvs) + (off + q));
          const uint32_t kk = u32(kv.key), vv = u32(kv.value);
          const bool mine = lane < n_sa && sa_key == kk;
          bool found = __builtin_amdgcn_ballot_w64(mine) != 0;
          if (mine) sa[lane].value = vv;
          for (uint32_t q0 = 64; q0 < n_sa; q0 += 64) {  // pairs past the lanes
            const uint32_t q = q0 + lane;
            const bool m2 = q < n_sa && sa[q].key == kk;
            if (m2) sa[q].value = vv;
            found = found || __builtin_amdgcn_ballot_w64(m2) != 0;
          }
          if (!found && n_sa < cap) {
            if (L0) gput(sa + n_sa, cdr_kv{kk, vv});
            if (lane == n_sa) sa_key = kk;
            n_sa++;
          } else if (!found) {
            FAILW(CDR_E_BAD_INPUT);  // a new key past the slice
          }
        }
        x_flags |= CDR_XI_HAS_SEARCH_ATTR;
        break;
      }
      case CDR_EV_WF_CONTINUED_AS_NEW: {  // :537-595
        const int32_t nr = (int32_t)u32((uint32_t)D.newrun);
        const bool empty = nr < 0 || call_idx != u32(D.newrun_call) || u32((uint32_t)gp(B_.wfs)[nr].ev_len) == 0;
        if (empty) {
          FAILW(CDR_E_NEWRUN_HISTORY_EMPTY);
          break;
        }
        newrun_applied = true;  // the new run replays as its own entry; k_finalize joins
        nr_call = call_idx;
        if (!transition_ok(x_state, x_close, CDR_STATE_COMPLETED, CDR_CLOSE_CONTINUED_AS_NEW)) {
          FAILW(CDR_E_INVALID_STATE_TRANSITION);
          break;
        }
        x_state = CDR_STATE_COMPLETED;
        x_close = CDR_CLOSE_CONTINUED_AS_NEW;
        x_completion_batch = call_first_id;
        break;
      }
      default:
        FAILW(CDR_E_UNKNOWN_EVENT_TYPE);  // :597-599
        break;
    }
  }
  return true;
  };
  // one chunk buffer: chunk r is copied out of it through opaque moves (the
  // per-event readlanes then never wait on vmcnt, which also counts the chunk in
  // flight and every store of an earlier event) and the buffer is refilled with
  // chunk r+1 at once, to land while chunk r's 64 events replay
  if (!done) {
    WChunk c0 = wload(R, 0, nrows, lane);
    auto take = [](const WChunk& b) __attribute__((always_inline)) {
      WChunk c;
      c.tf = mov32(b.tf);
      c.h = mov32(b.h);
      c.n = (int32_t)mov32((uint32_t)b.n);
      c.id = mov64(b.id);
      c.ver = mov64(b.ver);
      c.ts = mov64(b.ts);
      c.key = mov64(b.key);
      c.aux = mov64(b.aux);
      return c;
    };
    for (uint32_t r = 0;; r++) {
      const WChunk cur = take(c0);
      c0 = wload(R, r + 1, nrows, lane);
      if (!run_chunk(cur, r)) break;
    }
  }
#undef FAILW
  // ---- end of the last call
  if (len > 0 && (err == CDR_OK || stop_at_call_end)) {
    if (isRS) {
      const int src = cluster_of(prev_ver);
      if (src < 0) {
        err = CDR_P_UNKNOWN_CLUSTER;
        err_id = call_first_id;
        err_k = call_first_k;
        newrun_applied = newrun_applied && nr_call != call_idx;
      } else if (src != B_.cluster.current_cluster && err == CDR_OK) {
        if (L0) {
          RS->lri_version[src] = prev_ver;
          RS->lri_last_event_id[src] = prev_id;
        }
        rs_mask |= 1u << src;
      }
    }
    if (err == CDR_OK) x_next_event = prev_id + 1;
  }
  if (err == CDR_OK && (int32_t)u32((uint32_t)D.parent) < 0) {
    const int64_t want = u64(D.expected_next_event_id);
    if (want != 0 && x_next_event != want) {
      err = CDR_E_REBUILD_NEXT_EVENT_ID;  // nDCStateRebuilder.go:139-143
      err_id = prev_id;
      err_k = len;
    }
  }
  const bool ok = err == CDR_OK;
  // the live working slots as persisted rows, one lane per row (k_tables orders them
  // by key); fields the loop did not carry are re-read from the scheduling event
  uint32_t n_act = 0, n_tim = 0;
  if (ok) {
    const bool la = lane < hw_act && a_sid != DEAD_KEY;
    const uint64_t ma = __builtin_amdgcn_ballot_w64(la);
    n_act = (uint32_t)__builtin_popcountll(ma);
    if (la) {
      const uint32_t idx = __builtin_amdgcn_mbcnt_hi((uint32_t)(ma >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ma, 0));
      const uint64_t rows = (uint64_t)a_rows;
      const uint32_t ks = (uint32_t)rows, kb = (uint32_t)(rows >> 32);
      const uint32_t o_s = (ks >> 6) * CDR_ROW_BYTES + (ks & 63u) * 8u, o_b = (kb >> 6) * CDR_ROW_BYTES + (kb & 63u) * 8u;
      const int64_t sched_ts = bld64(R, o_s, cdr_col_off(CDR_COL_TIMESTAMP));
      const uint32_t arec = (uint32_t)bld64(R, o_s, cdr_col_off(CDR_COL_AUX));
      const GAS cdr_attr_at_scheduled* a = gp((const cdr_attr_at_scheduled*)(B_.ev.arena + arec));
      const uint64_t m = (uint64_t)a_meta;
      const bool retry = (a->flags & CDR_AF_HAS_RETRY) != 0;
      const int32_t s2c = a->s2c_s, xs = a->retry_expiration_s;
      cdr_activity_info o;
      o.version = a_ver;
      o.schedule_id = a_sid;
      o.scheduled_event_batch_id = bld64(R, o_b, cdr_col_off(CDR_COL_EVENT_ID));
      o.scheduled_time = sched_ts;
      o.started_id = a_stid;
      o.started_time = a_stime;
      o.last_heartbeat_time = a_stime;
      o.expiration_time = sched_ts + (int64_t)((retry && xs > s2c) ? xs : s2c) * NS_PER_S;
      o.cancel_request_id = a_cancel;
      o.activity_id = (uint32_t)m;
      o.request_id = (uint32_t)a_req;
      o.task_list = a->task_list;
      o.nonretriable = retry ? a->nonretriable : 0u;
      o.s2s = a->s2s_s;
      o.s2c = s2c;
      o.stc = a->stc_s;
      o.hb = a->hb_s;
      o.timer_task_status = (int32_t)((m >> META_TTS_SHIFT) & 0xFFu);
      o.attempt = 0;
      o.initial_interval = retry ? a->retry_initial_s : 0;
      o.maximum_interval = retry ? a->retry_max_interval_s : 0;
      o.maximum_attempts = retry ? a->retry_max_attempts : 0;
      o.flags = (retry ? CDR_AI_HAS_RETRY : 0u) | ((m & META_FLAG(AF_CANCEL)) ? CDR_AI_CANCEL_REQUESTED : 0u) |
                ((m & META_FLAG(AF_STARTED)) ? CDR_AI_STARTED_TIME_SET : 0u);
      o.backoff_coefficient = retry ? a->backoff_coefficient : 0.0;
      gput(gp(O_.act) + CP.act_off + idx, o);
    }
    const bool lt = lane < hw_tim && t_sid != DEAD_KEY;
    const uint64_t mt = __builtin_amdgcn_ballot_w64(lt);
    n_tim = (uint32_t)__builtin_popcountll(mt);
    if (lt) {
      const uint32_t idx = __builtin_amdgcn_mbcnt_hi((uint32_t)(mt >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mt, 0));
      cdr_timer_info o;
      o.version = t_ver;
      o.started_id = t_sid;
      o.expiry_time = t_exp;
      o.task_id = (int64_t)((uint64_t)t_tt >> 32);
      o.timer_id = (uint32_t)t_tt;
      o._pad = 0;
      gput(gp(O_.timer) + CP.timer_off + idx, o);
    }
  }
  if (L0) {
    cdr_wf_result r;
    r.code = err;
    r.flags = (newrun_applied ? CDR_RF_NEWRUN_APPLIED : 0u) | ((int32_t)D.parent >= 0 ? CDR_RF_IS_NEWRUN : 0u);
    r.fail_event_id = err_id;
    r.fail_index = err_k;
    r.n_activity = ok ? n_act : 0u;
    r.n_timer = ok ? n_tim : 0u;
    r.n_child = ok ? hw_chi : 0u;
    r.n_cancel = ok ? hw_can : 0u;
    r.n_signal = ok ? hw_sig : 0u;
    r.n_vh = ok ? n_vh : 0u;
    r.n_reset_points = ok ? n_rp : 0u;
    r.n_search_attr = ok ? n_sa : 0u;
    gput(gp(O_.result) + w, r);
  }
  if (!ok || !L0) return;
  if (want_ld && !(ld & LD_CAPTURED))
    ld_write(gp(O_.last_decision) + w, ld, dv, dsched, dstart, dreq, dto, datt, dsc_ts, dst_ts, dorig_ts);
  if (n_vh) gput(vh + (n_vh - 1), cdr_vh_item{vh_last_id, vh_last_ver});
  if (!(x_flags & CDR_XI_STARTED)) {  // no WorkflowExecutionStarted: its fields keep their zero values
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
  X->decision_timeout_value = x_dt_timeout_value;
  X->_pad0 = 0;
  X->_pad1 = 0;
  X->decision_request_id = dreq;
  X->flags = x_flags;
  X->completion_event_batch_id = x_completion_batch;
  X->state = x_state;
  X->close_status = x_close;
  X->last_first_event_id = call_first_id;  // stateBuilder.go:603 of the last call
  {  // LastEventTaskID (:155): the last applied event's (an OK replay applied all)
    const uint32_t kl = len - 1;
    const int64_t t = bld64(R, (kl >> 6) * CDR_ROW_BYTES + (kl & 63u) * 8u, cdr_col_off(CDR_COL_TASK_ID));
    X->last_event_task_id = t;
  }
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
  X->reset_points_len = n_rp;
  X->search_attr_len = n_sa;
  if (isRS) {
    RS->current_version = prev_ver;
    if (!(x_flags & CDR_XI_STARTED)) RS->start_version = D.failover_version;
    RS->last_write_version = prev_ver;
    RS->last_write_event_id = prev_id;
    for (int c = 0; c < CDR_MAX_CLUSTERS; c++)
      if (!(rs_mask & (1u << c))) {
        RS->lri_version[c] = 0;
        RS->lri_last_event_id[c] = 0;
      }
    RS->lri_mask = rs_mask;
    RS->present = 1;
  }
#undef D
#undef CP
#undef X
#undef RS
#undef chi
#undef can
#undef sig
#undef vh
#undef rp
#undef sa
#undef B_
#undef O_
}
#undef WPUT
#undef WGET
