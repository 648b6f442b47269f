// xdc_admit.h — the 2DC replicator's admission decision, compiled once for host and device.
//
// historyReplicator.ApplyEvents (service/history/historyReplicator.go:339-763, H below) up to
// the point where events are applied: ApplyOtherEventsMissingMutableState (H:451-519),
// ApplyOtherEventsVersionChecking (H:521-653) with conflictResolutionTerminateCurrentRunningIfNotSelf
// (H:925-999) and getLatestCheckpoint (H:1115-1140), then ApplyOtherEvents' event-id check
// (H:655-694) and ApplyReplicationTask's running check (H:704-707).  Everything on the active
// side that writes events — reapplyEvents, terminateWorkflow, flushEventsBuffer, ApplyResetEvent —
// is the caller's: the decision names it.
//
// Plain C++ on values: no intrinsics, no pointers into global memory.  host.cpp builds it into
// cdr_xdc_admit_host, xdc.hip into k_xdc_admit and the round's post-reset check.
#pragma once
#include "cdr/cdr.h"

namespace cdr_xdc {

// IsWorkflowExecutionRunning (mutableStateBuilder.go:1422-1434): 1 / 0, or -1 where it panics
CDR_HD int running(int32_t state) {
  if (state == CDR_STATE_CREATED || state == CDR_STATE_RUNNING) return 1;
  if (state == CDR_STATE_COMPLETED || state == CDR_STATE_ZOMBIE) return 0;
  return -1;
}

// ClusterNameForFailoverVersion (common/cluster/metadata.go:187-203): the cluster's index, -1 where it panics
CDR_HD int cluster_of(const cdr_cluster_meta& m, int64_t v) {
  if (v == CDR_EMPTY_VERSION) return m.current_cluster;
  const int64_t init = v % m.failover_version_increment;
  int r = -1;
#pragma unroll
  for (int i = 0; i < CDR_MAX_CLUSTERS; i++)
    if (i < m.n_clusters && m.initial_version[i] == init && r < 0) r = i;
  return r;
}

CDR_HD cdr_xdc_decision fail(cdr_xdc_decision d, int32_t reason, int32_t code) {
  d.action = CDR_XDC_DROP;
  d.reason = reason;
  d.code = code;
  return d;
}
CDR_HD cdr_xdc_decision done(cdr_xdc_decision d, int32_t action, int32_t reason) {
  d.action = action;
  d.reason = reason;
  return d;
}
CDR_HD cdr_xdc_decision retry(cdr_xdc_decision d, int32_t reason, uint32_t run, int64_t next_event_id) {
  d.action = CDR_XDC_RETRY;
  d.reason = reason;
  d.hint_run = run;
  d.hint_next_event_id = next_event_id;
  return d;
}

// ApplyOtherEvents (H:655-694) + ApplyReplicationTask's first check (H:704-707) against a state
// with workflow state `state` and next event id `next`; d carries `via` (and, in the round, the
// reset's fields)
CDR_HD cdr_xdc_decision apply_other(cdr_xdc_decision d, const cdr_xdc_task& t, int32_t state, int64_t next) {
  if (t.first_event_id < next) return done(d, CDR_XDC_DROP, CDR_XDR_DUPLICATE);
  const int run = running(state);
  if (run < 0) return fail(d, CDR_XDR_E_WF_STATE, CDR_P_UNKNOWN_WF_STATE);
  if (t.first_event_id > next) {
    if (!run) return done(d, CDR_XDC_DROP, CDR_XDR_CLOSED_AHEAD);
    return retry(d, CDR_XDR_BUFFER, 0, next);
  }
  if (!run) return done(d, CDR_XDC_DROP, CDR_XDR_CLOSED);
  return done(d, CDR_XDC_APPLY, CDR_XDR_APPLY);
}

// resetMutableState (H:1142-1189) up to resolver.reset: conflictResolutionTerminateCurrentRunningIfNotSelf
CDR_HD cdr_xdc_decision reset(cdr_xdc_decision d, const cdr_xdc_task& t, int32_t state, int64_t last_write_version,
                              int32_t reason, int64_t reset_event_id) {
  const int run = running(state);
  if (run < 0) return fail(d, CDR_XDR_E_WF_STATE, CDR_P_UNKNOWN_WF_STATE);
  if (!run && !(t.flags & CDR_XDC_CUR_PRESENT)) return fail(d, CDR_XDR_E_NO_CURRENT, CDR_E_BAD_INPUT);
  d.via = CDR_XDV_RESET;
  if (run) {  // H:938-947
    d.cas_prev_is_self = 1;
    d.cas_prev_last_write_version = last_write_version;
    d.cas_prev_state = state;
  } else {
    if (t.version <= t.cur_last_write_version) return done(d, CDR_XDC_DROP, CDR_XDR_RESET_ABANDONED);  // H:972-975
    d.cas_prev_is_self = (t.flags & CDR_XDC_CUR_IS_SELF) ? 1u : 0u;
    d.cas_prev_last_write_version = t.cur_last_write_version;
    if (t.cur_close_status != CDR_CLOSE_NONE) {  // H:977-982
      d.cas_prev_state = t.cur_state;
    } else {  // H:984-998
      d.terminate_current_first = 1;
      d.flags |= CDR_XDD_CAS_VERSION_FROM_TERMINATE;
      d.cas_prev_state = CDR_STATE_COMPLETED;
    }
  }
  d.reset_event_id = reset_event_id;
  return done(d, CDR_XDC_RESET_APPLY, reason);
}

// The whole decision for one task.  r / x / rs: the target run's records (not read when the
// task has CDR_XDC_NO_STATE).
CDR_HD cdr_xdc_decision admit(const cdr_xdc_task& t, const cdr_wf_result& r, const cdr_exec_info& x,
                              const cdr_repl_state& rs, const cdr_cluster_meta& m) {
  cdr_xdc_decision d{};
  if (t.n_events == 0) return done(d, CDR_XDC_DROP, CDR_XDR_EMPTY_TASK);  // H:377-381
  const bool no_state = (t.flags & CDR_XDC_NO_STATE) != 0;
  if (!no_state && (r.code != CDR_OK || !rs.present)) return fail(d, CDR_XDR_E_STATE, CDR_E_BAD_INPUT);
  if (t.first_event_type == CDR_EV_WF_STARTED) {  // H:398-410
    if (!no_state) return done(d, CDR_XDC_DROP, CDR_XDR_DUPLICATE_START);
    return done(d, CDR_XDC_APPLY_FRESH, CDR_XDR_START);
  }
  if (no_state) {  // ApplyOtherEventsMissingMutableState H:451-519
    if (!(t.flags & CDR_XDC_CUR_PRESENT)) return retry(d, CDR_XDR_MISSING_NO_CURRENT, 0, CDR_FIRST_EVENT_ID);
    const bool cur_running = (t.flags & CDR_XDC_CUR_RUNNING) != 0;
    const bool is_reset = (t.flags & CDR_XDC_RESET_WORKFLOW) != 0;
    if (t.cur_last_write_version > t.last_event_version) {
      d.reapply_to = 1;
      return done(d, CDR_XDC_REAPPLY, CDR_XDR_MISSING_STALE);
    }
    if (t.cur_last_write_version < t.last_event_version) {
      d.terminate_current_first = cur_running ? 1u : 0u;
      if (is_reset) return done(d, CDR_XDC_APPLY_RESET_EVENT, CDR_XDR_MISSING_NEWER_RESET);
      return retry(d, CDR_XDR_MISSING_NEWER, 0, CDR_FIRST_EVENT_ID);
    }
    if (cur_running) {
      if (t.last_event_task_id < t.cur_last_event_task_id) return done(d, CDR_XDC_DROP, CDR_XDR_MISSING_SAME_OLDER_TASK);
      return retry(d, CDR_XDR_MISSING_SAME_RUNNING, 1, t.cur_next_event_id);
    }
    if (is_reset) return done(d, CDR_XDC_APPLY_RESET_EVENT, CDR_XDR_MISSING_SAME_RESET);
    return retry(d, CDR_XDR_MISSING_SAME_CLOSED, 0, CDR_FIRST_EVENT_ID);
  }
  // ApplyOtherEventsVersionChecking H:521-653
  const int64_t lwv = rs.last_write_version;
  if (lwv > t.version) {  // stale task H:533-563
    const int run = running(x.state);
    if (run < 0) return fail(d, CDR_XDR_E_WF_STATE, CDR_P_UNKNOWN_WF_STATE);
    if (run) return done(d, CDR_XDC_REAPPLY, CDR_XDR_STALE_RUNNING);
    if (t.flags & CDR_XDC_CUR_IS_SELF) return done(d, CDR_XDC_REAPPLY, CDR_XDR_STALE_SELF);
    d.reapply_to = 1;
    return done(d, CDR_XDC_REAPPLY, CDR_XDR_STALE_OTHER);
  }
  if (lwv == t.version) {
    d.via = CDR_XDV_SAME_VERSION;
    return apply_other(d, t, x.state, x.next_event_id);
  }
  const int prev = cluster_of(m, lwv);  // H:576
  if (prev < 0) return fail(d, CDR_XDR_E_CLUSTER, CDR_P_UNKNOWN_CLUSTER);
  if (prev != m.current_cluster) {  // H:586-598
    if ((t.version - lwv) % m.failover_version_increment != 0) return fail(d, CDR_XDR_E_MORE_THAN_2DC, CDR_E_XDC_MORE_THAN_2DC);
    d.via = CDR_XDV_SAME_CLUSTER;
    return apply_other(d, t, x.state, x.next_event_id);
  }
  // this cluster was active before: did the remote apply its events?  ri := replicationInfo[prev]
  const bool ri_ok = ((t.ri_mask >> prev) & 1u) != 0;
  int64_t ri_version = 0, ri_last = 0;
#pragma unroll
  for (int i = 0; i < CDR_MAX_CLUSTERS; i++)
    if (i == prev) ri_version = t.ri_version[i], ri_last = t.ri_last_event_id[i];
  if (!ri_ok || lwv > ri_version) {  // rejected by remote H:603-618
    int64_t cv = CDR_EMPTY_VERSION, ce = CDR_EMPTY_EVENT_ID;  // getLatestCheckpoint, order as schema.h states
#pragma unroll
    for (int i = 0; i < CDR_MAX_CLUSTERS; i++)
      if (((t.ri_mask >> i) & 1u) && (cv == CDR_EMPTY_VERSION || t.ri_version[i] > cv))
        cv = t.ri_version[i], ce = t.ri_last_event_id[i];
#pragma unroll
    for (int i = 0; i < CDR_MAX_CLUSTERS; i++)
      if (((rs.lri_mask >> i) & 1u) && (cv == CDR_EMPTY_VERSION || rs.lri_version[i] > cv))
        cv = rs.lri_version[i], ce = rs.lri_last_event_id[i];
    if (cv == CDR_EMPTY_VERSION) return fail(d, CDR_XDR_E_MISSING_REPL_INFO, CDR_E_XDC_MISSING_REPL_INFO);
    return reset(d, t, x.state, lwv, CDR_XDR_RESET_REJECTED, ce);
  }
  if (lwv < ri_version) return fail(d, CDR_XDR_E_REMOTE_HIGHER_VERSION, CDR_E_XDC_REMOTE_HIGHER_VERSION);
  if (ri_last > rs.last_write_event_id) return fail(d, CDR_XDR_E_CORRUPTED_REPL_INFO, CDR_E_XDC_CORRUPTED_REPL_INFO);
  if (t.flags & CDR_XDC_HAS_BUFFERED) {  // flushEventsBuffer H:635-638, 1216
    const int run = running(x.state);
    if (run < 0) return fail(d, CDR_XDR_E_WF_STATE, CDR_P_UNKNOWN_WF_STATE);
    if (run) return done(d, CDR_XDC_FLUSH_BUFFER, CDR_XDR_FLUSH_BUFFER);
  }
  if (ri_last < rs.last_write_event_id) return reset(d, t, x.state, lwv, CDR_XDR_RESET_CONFLICT, ri_last);  // H:640-648
  d.via = CDR_XDV_EVENT_ID_MATCH;
  return apply_other(d, t, x.state, x.next_event_id);
}

}  // namespace cdr_xdc
