/*
 * cdr/cdr.h — C ABI of the MI355X workflow-history replay engine (libcdr.so).
 *
 * Drop-in boundary for the reference's replay hot path.  Each entry point names
 * the reference interface it replaces (paths relative to /root/reference):
 *
 *   stateBuilder.applyEvents            service/history/stateBuilder.go:38-52,112-611
 *     -> cdr_replay_batch (many workflows, each a sequence of applyEvents calls on a
 *        fresh mutable state) and cdr_replay_sliced (same, device-resident input)
 *   stateBuilderProvider / newStateBuilder
 *                                       service/history/historyReplicator.go:54,144
 *                                       service/history/nDCHistoryReplicator.go:136-141
 *     -> cdr_create / cdr_destroy (one context per goroutine-equivalent / stream)
 *   nDCStateRebuilder.rebuild batch loop service/history/nDCStateRebuilder.go:92-160
 *     -> cdr_replay_batch with cdr_wf_desc.expected_next_event_id set
 *   mutableStateTaskRefresher.refreshTasks (after nDCStateRebuilder.rebuild's replay)
 *                                       service/history/mutableStateTaskRefresher.go:66-160
 *                                       service/history/nDCStateRebuilder.go:154-157
 *     -> cdr_refresh_tasks_async (device-resident) / cdr_rebuild_batch (host buffers)
 *   sql row blobs (timerInfoToBlob, requestCancelInfoToBlob)
 *                                       common/persistence/sql/workflowStateMaps.go:239-260,504-521
 *     -> cdr_encode_rows_async
 *   sqlExecutionManager.GetWorkflowExecution
 *                                       common/persistence/sql/sqlExecutionManager.go:206-332
 *     -> cdr_load_state (stored rows -> the loaded state cdr_carry takes; cdr_load_rows: its
 *        pending tables alone)
 *   common.WorkflowIDToHistoryShard     common/util.go:249-252
 *     -> cdr_workflow_id_to_shard (farmhash Fingerprint32 % numShards)
 *
 * Conventions: plain C, caller-owned buffers, no exceptions across the boundary.
 * Every call is synchronous on the stream it is given unless named *_async.
 * Return value: 0 on success, a negative CDR_API_* code on API misuse / device
 * failure.  Per-workflow replay outcomes (the Go `error` of applyEvents) are in
 * cdr_wf_result.code, never in the return value.
 */
#ifndef CDR_CDR_H
#define CDR_CDR_H

#include <stddef.h>
#include <stdint.h>

#include "cdr/schema.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CDR_API_OK 0
#define CDR_API_EINVAL (-1)   /* bad arguments / inconsistent batch */
#define CDR_API_ENODEV (-2)   /* no HIP device or kernel image not loadable */
#define CDR_API_EDEVICE (-3)  /* HIP runtime error */
#define CDR_API_ENOMEM (-4)

#define CDR_SLICE_WIDTH 64 /* workflows per slice = one wavefront */

/* Sliced event layout ("SELL-64" rows in a slab): workflows are grouped 64 to a
 * slice (one lane each, slices sorted by length).  Slice s owns slice_len[s]
 * consecutive rows of the slab starting at row slice_row0[s]; row k of a slice holds
 * event k of its 64 lanes, column after column (cdr_col_off below), in
 * CDR_ROW_BYTES.  A wavefront that walks its 64 histories in lockstep therefore reads
 * each column of a step as one coalesced 256/512-B access and a whole step from one
 * contiguous 3.75 KB row (DRAM-page friendly), and one buffer descriptor per slice
 * addresses every column with an immediate column offset.  The kernel reads only the
 * operand columns an event's type needs (CDR_SEF_NEED_* bits of type_flags); the
 * fast-path kernel also skips a key / aux cell the event's id implies (CDR_SEF_KEY_BACK /
 * CDR_SEF_AUX_IMPL below).
 *
 * Operand columns per type (all others 0):
 *   WorkflowExecutionStarted  aux = arena word offset of cdr_attr_wf_started
 *   DecisionTaskScheduled     aux = attempt, n = StartToCloseTimeoutSeconds
 *   DecisionTaskStarted       key = scheduledEventId, h = requestId
 *   DecisionTaskCompleted     key = scheduledEventId, aux = startedEventId, h = binaryChecksum
 *   DecisionTaskTimedOut      n = timeoutType
 *   ActivityTaskScheduled     key = activityId | (u32)StartToClose << 32, h = (u32)ScheduleToClose,
 *                             n = ScheduleToStart, aux = arena word offset (< 2^32) of
 *                             cdr_attr_at_scheduled | (u32)Heartbeat << 32
 *   ActivityTask{Started,Completed,Failed,TimedOut,Canceled}  key = scheduledEventId
 *                             (Started: h = requestId)
 *   ActivityTaskCancelRequested / RequestCancelActivityTaskFailed  key = activityId
 *   Timer{Started,Fired,Canceled}, CancelTimerFailed  key = timerId (Started: aux = startToFireSeconds)
 *   StartChildWorkflowExecutionInitiated  key = domain, aux = workflowType, h = workflowId,
 *                             n = parentClosePolicy
 *   SignalExternalWorkflowExecutionInitiated  key = domain, aux = input << 32 | control, h = signalName
 *   RequestCancelExternalWorkflowExecutionInitiated  key = domain
 *                             (these three: key |= arena word offset (< 2^32) of their
 *                             cdr_attr_external << 32, read only when tasks are emitted)
 *   ChildWorkflowExecutionStarted  key = initiatedEventId, h = runId
 *   other child / external closes  key = initiatedEventId
 *   UpsertWorkflowSearchAttributes  aux = kv offset, h = kv count
 *   WorkflowExecutionContinuedAsNew  h = newExecutionRunId */
enum cdr_col {
  CDR_COL_EVENT_ID = 0, /* i64 */
  CDR_COL_VERSION,      /* i64 */
  CDR_COL_TIMESTAMP,    /* i64 */
  CDR_COL_TASK_ID,      /* i64 */
  CDR_COL_KEY,          /* i64 entity key: scheduled/initiated event id, activity/timer handle ... */
  CDR_COL_AUX,          /* i64 second operand or arena word offset (type-dependent) */
  CDR_COL_TYPE_FLAGS,   /* u32 bits 0-7 cdr_event_type, 8+ CDR_SEF_* */
  CDR_COL_H,            /* u32 string handle operand (type-dependent) */
  CDR_COL_N,            /* i32 small integer operand (type-dependent) */
  CDR_NUM_COLS
};
#define CDR_EL_BYTES 60u /* bytes of one (row, lane) element over all columns */
#define CDR_ROW_BYTES (CDR_EL_BYTES * CDR_SLICE_WIDTH) /* 3840: one event of 64 lanes */
/* element size of a column and its byte offset within a row; element (k, L) of
 * column c of a slice is at k * CDR_ROW_BYTES + cdr_col_off(c) + L * cdr_col_size(c)
 * from the slice's first row */
CDR_HD uint32_t cdr_col_size(int c) { return c < CDR_COL_TYPE_FLAGS ? 8u : 4u; }
CDR_HD uint32_t cdr_col_off(int c) {
  return CDR_SLICE_WIDTH * (c <= CDR_COL_TYPE_FLAGS ? 8u * (uint32_t)c : 48u + 4u * (uint32_t)(c - CDR_COL_TYPE_FLAGS));
}

typedef struct cdr_slices {
  uint32_t n_slices, _pad;
  uint64_t n_rows;        /* sum of slice_len */
  uint64_t arena_words;   /* 8-byte words of attribute records */
  const uint64_t* slice_row0; /* [n_slices] prefix sum of slice_len */
  const uint32_t* slice_len;  /* [n_slices] */
  const int32_t* lane_wf;     /* [n_slices*64] workflow index, -1 = empty lane */
  const uint8_t* slab;        /* n_rows * CDR_ROW_BYTES bytes of event rows */
  const uint64_t* arena; /* WorkflowExecutionStarted / ActivityTaskScheduled attribute records */
  /* working-state scratch of each slice (cdr_plan_scratch): pending activities and
   * user timers are kept lane-interleaved ("plane j*P+p, lane L") while they are live */
  const uint64_t* slice_scratch_off; /* [n_slices] 8-byte-word offset into the scratch buffer */
  const uint32_t* slice_act_slots;   /* [n_slices] activity working slots per lane */
  const uint32_t* slice_tim_slots;   /* [n_slices] user-timer working slots per lane */
  const uint32_t* slice_flags;       /* [n_slices] CDR_SLICE_* */
} cdr_slices;
#define CDR_SLICE_FAST 0x1u /* every lane's history has CDR_CAP_FAST */
/* a wave slice: ONE workflow (lane_wf[64 s]; the other lanes -1) replayed by a whole
 * wavefront (replay_wave.inc); its slice_len rows hold the workflow's events 64 at a
 * time, event k in row k/64, lane k%64 (cdr_plan_slices_ex with CDR_PLAN_WAVE) */
#define CDR_SLICE_WAVE 0x2u
/* every lane's history has CDR_CAP_REG: the slice replays in k_replay_reg
 * (replay_reg.inc: entity tables in registers, no global memory traffic in the step
 * loop beyond the event stream) */
#define CDR_SLICE_REG 0x4u
/* every lane's history has CDR_CAP_REG2 or CDR_CAP_REG: the register-table kernel's
 * variant with CDR_REG2_NA activity slots */
#define CDR_SLICE_REG2 0x8u
/* every lane's history has CDR_CAP_REG0: the register-table variant with the small tables
 * (CDR_REG0_*) at 3 waves per SIMD */
#define CDR_SLICE_REG0 0x10u
/* a lane slice of the batch's long register-table histories (cdr_plan_slices_ex with
 * CDR_PLAN_PAR; the first n_par_slices slices): replayed by k_replay_cls's four-wave
 * variant, its loops at once (replay_cls.inc), or by k_replay_reg <CDR_REG2_NA, ...> */
#define CDR_SLICE_PAR 0x20u
/* event types the fast-path kernel replays (bit = cdr_event_type) */
#define CDR_FAST_TYPES                                                                                       \
  (CDR_TB(CDR_EV_WF_STARTED) | CDR_TB(CDR_EV_WF_COMPLETED) | CDR_TB(CDR_EV_WF_FAILED) |                      \
   CDR_TB(CDR_EV_WF_TIMED_OUT) | CDR_TB(CDR_EV_DT_SCHEDULED) | CDR_TB(CDR_EV_DT_STARTED) |                   \
   CDR_TB(CDR_EV_DT_COMPLETED) | CDR_TB(CDR_EV_DT_TIMED_OUT) | CDR_TB(CDR_EV_DT_FAILED) |                    \
   CDR_TB(CDR_EV_AT_SCHEDULED) | CDR_TB(CDR_EV_AT_STARTED) | CDR_TB(CDR_EV_AT_COMPLETED) |                   \
   CDR_TB(CDR_EV_AT_FAILED) | CDR_TB(CDR_EV_AT_TIMED_OUT) | CDR_TB(CDR_EV_AT_CANCEL_REQUESTED) |             \
   CDR_TB(CDR_EV_AT_REQ_CANCEL_FAILED) | CDR_TB(CDR_EV_AT_CANCELED) | CDR_TB(CDR_EV_CANCEL_TIMER_FAILED) |   \
   CDR_TB(CDR_EV_WF_CANCEL_REQUESTED) | CDR_TB(CDR_EV_WF_CANCELED) | CDR_TB(CDR_EV_MARKER_RECORDED) |        \
   CDR_TB(CDR_EV_WF_SIGNALED) | CDR_TB(CDR_EV_WF_TERMINATED))

#define CDR_ACT_PLANES 12 /* words per activity working slot (replay.hip) */
#define CDR_TIM_PLANES 4  /* words per user-timer working slot */

#define CDR_SEF_BATCH_FIRST (1u << 8)
#define CDR_SEF_DOMAIN_MISSING (1u << 9)
/* delta bits (set by the packer for every event after an entry's first): the event's
 * event_id is the previous event's + 1 / its version equals the previous event's.  The
 * columns still hold the full values; the fast-path kernel skips loading them when
 * the bit is set (16 of the ~46 bytes a C2 event costs it) and rebuilds them from its
 * registers */
#define CDR_SEF_ID_NEXT (1u << 21)
#define CDR_SEF_VER_SAME (1u << 22)
/* operand hint fields (set by the packer from the event's own values, only when the
 * type's need bit for that column is set): the key / aux operand follows from the
 * event's id, as Cadence writes history (a DecisionTaskStarted follows its Scheduled,
 * Started and Completed are flushed together, attempt is 0 outside transient decisions).
 *   CDR_SEF_KEY_BACK  0 = none; d = 1..7: key == event_id - d
 *   CDR_SEF_AUX_IMPL  0 = none; 7: aux == 0; else d = 1..6: aux == event_id - d
 * (uint64_t arithmetic, wrapping, like the delta bits; aux == 0 takes 7 whatever the
 * id).  The columns still hold the full values; the fast-path kernel skips loading a
 * hinted column and rebuilds the operand from the event's id (replay.hip ev_hint), every
 * other reader ignores the fields. */
#define CDR_SEF_KEY_BACK_SHIFT 10
#define CDR_SEF_KEY_BACK (7u << CDR_SEF_KEY_BACK_SHIFT)
#define CDR_SEF_AUX_IMPL_SHIFT 13
#define CDR_SEF_AUX_IMPL (7u << CDR_SEF_AUX_IMPL_SHIFT)
#define CDR_SEF_AUX_ZERO 7u
/* operand columns the event's type reads (set by the packer from CDR_NEED_*) */
#define CDR_SEF_NEED_TS (1u << 16)
#define CDR_SEF_NEED_KEY (1u << 17)
#define CDR_SEF_NEED_AUX (1u << 18)
#define CDR_SEF_NEED_H (1u << 19)
#define CDR_SEF_NEED_N (1u << 20)
/* per-column sets of event types (bit = cdr_event_type) that read it; every type
 * reads type_flags, event_id and version (stateBuilder.go:134-155) */
#define CDR_TB(t) (1ull << (t))
#define CDR_NEED_TS                                                                                  \
  (CDR_TB(CDR_EV_WF_STARTED) | CDR_TB(CDR_EV_DT_SCHEDULED) | CDR_TB(CDR_EV_DT_STARTED) |              \
   CDR_TB(CDR_EV_AT_SCHEDULED) | CDR_TB(CDR_EV_AT_STARTED) | CDR_TB(CDR_EV_TIMER_STARTED) |            \
   CDR_TB(CDR_EV_WF_COMPLETED) | CDR_TB(CDR_EV_WF_FAILED) | CDR_TB(CDR_EV_WF_TIMED_OUT) |              \
   CDR_TB(CDR_EV_WF_CANCELED) | CDR_TB(CDR_EV_WF_TERMINATED) | CDR_TB(CDR_EV_WF_CONTINUED_AS_NEW))
#define CDR_NEED_KEY                                                                                 \
  (CDR_TB(CDR_EV_DT_STARTED) | CDR_TB(CDR_EV_AT_SCHEDULED) | CDR_TB(CDR_EV_AT_STARTED) |              \
   CDR_TB(CDR_EV_AT_COMPLETED) | CDR_TB(CDR_EV_AT_FAILED) | CDR_TB(CDR_EV_AT_TIMED_OUT) |              \
   CDR_TB(CDR_EV_AT_CANCELED) | CDR_TB(CDR_EV_AT_CANCEL_REQUESTED) | CDR_TB(CDR_EV_TIMER_STARTED) |    \
   CDR_TB(CDR_EV_TIMER_FIRED) | CDR_TB(CDR_EV_TIMER_CANCELED) | CDR_TB(CDR_EV_CHILD_INITIATED) |       \
   CDR_TB(CDR_EV_CHILD_STARTED) | CDR_TB(CDR_EV_CHILD_START_FAILED) | CDR_TB(CDR_EV_CHILD_COMPLETED) | \
   CDR_TB(CDR_EV_CHILD_FAILED) | CDR_TB(CDR_EV_CHILD_CANCELED) | CDR_TB(CDR_EV_CHILD_TIMED_OUT) |      \
   CDR_TB(CDR_EV_CHILD_TERMINATED) | CDR_TB(CDR_EV_RCE_FAILED) | CDR_TB(CDR_EV_EXT_CANCEL_REQUESTED) | \
   CDR_TB(CDR_EV_SE_FAILED) | CDR_TB(CDR_EV_EXT_SIGNALED) | CDR_TB(CDR_EV_RCE_INITIATED) |                 \
   CDR_TB(CDR_EV_SE_INITIATED))
#define CDR_NEED_AUX                                                                                 \
  (CDR_TB(CDR_EV_WF_STARTED) | CDR_TB(CDR_EV_DT_SCHEDULED) | CDR_TB(CDR_EV_DT_COMPLETED) |            \
   CDR_TB(CDR_EV_AT_SCHEDULED) | CDR_TB(CDR_EV_TIMER_STARTED) | CDR_TB(CDR_EV_CHILD_INITIATED) |       \
   CDR_TB(CDR_EV_SE_INITIATED) | CDR_TB(CDR_EV_UPSERT_SA))
#define CDR_NEED_H                                                                                   \
  (CDR_TB(CDR_EV_DT_STARTED) | CDR_TB(CDR_EV_DT_COMPLETED) | CDR_TB(CDR_EV_AT_SCHEDULED) |            \
   CDR_TB(CDR_EV_AT_STARTED) | CDR_TB(CDR_EV_CHILD_INITIATED) | CDR_TB(CDR_EV_CHILD_STARTED) |        \
   CDR_TB(CDR_EV_SE_INITIATED) | CDR_TB(CDR_EV_UPSERT_SA))
#define CDR_NEED_N \
  (CDR_TB(CDR_EV_DT_SCHEDULED) | CDR_TB(CDR_EV_DT_TIMED_OUT) | CDR_TB(CDR_EV_AT_SCHEDULED) | CDR_TB(CDR_EV_CHILD_INITIATED))
/* type_flags word of an event: type, flags and its column-need bits */
CDR_HD uint32_t cdr_type_flags(uint32_t type, uint32_t flags) {
  /* the type byte: a caller's type of 255 (the padding value) or past the byte (256 would alias
   * WorkflowExecutionStarted) is as unknown as any (stateBuilder.go:597-599) and travels as 254,
   * which no kernel knows and none takes for padding */
  uint32_t tf = (type >= (uint32_t)CDR_EV_PAD ? 0xFEu : type) | flags;
  if (type < 64) {
    const uint64_t b = 1ull << type;
    tf |= ((CDR_NEED_TS & b) ? CDR_SEF_NEED_TS : 0u) | ((CDR_NEED_KEY & b) ? CDR_SEF_NEED_KEY : 0u) |
          ((CDR_NEED_AUX & b) ? CDR_SEF_NEED_AUX : 0u) | ((CDR_NEED_H & b) ? CDR_SEF_NEED_H : 0u) |
          ((CDR_NEED_N & b) ? CDR_SEF_NEED_N : 0u);
  }
  return tf;
}
/* the operand hint fields of an event whose type_flags word (need bits) is tf */
CDR_HD uint32_t cdr_operand_hints(uint32_t tf, int64_t event_id, int64_t key, int64_t aux) {
  uint32_t hints = 0;
  if (tf & CDR_SEF_NEED_KEY) {
    const uint64_t d = (uint64_t)event_id - (uint64_t)key;
    if (d >= 1 && d <= 7) hints |= (uint32_t)d << CDR_SEF_KEY_BACK_SHIFT;
  }
  if (tf & CDR_SEF_NEED_AUX) {
    const uint64_t d = (uint64_t)event_id - (uint64_t)aux;
    if (aux == 0)
      hints |= CDR_SEF_AUX_ZERO << CDR_SEF_AUX_IMPL_SHIFT;
    else if (d >= 1 && d <= 6)
      hints |= (uint32_t)d << CDR_SEF_AUX_IMPL_SHIFT;
  }
  return hints;
}

/* everything the device needs for one replay launch (all pointers device memory) */
typedef struct cdr_dev_batch {
  cdr_slices ev;
  uint64_t* scratch; /* working-state buffer, cdr_plan_scratch words (device) */
  const cdr_wf_desc* wfs; /* [n_wfs] */
  const cdr_wf_caps* caps; /* [n_wfs] */
  const cdr_kv* kvs;
  const cdr_reset_point* rps;
  uint32_t n_wfs;
  uint32_t empty_uuid; /* handle of "emptyUuid" (mutableStateBuilder.go:42) */
  /* max over slices of slice_act_slots / slice_tim_slots (cdr_plan_scratch): the
   * launcher keeps up to this many working slots per lane in LDS (0 = all in scratch) */
  uint32_t max_act_slots, max_tim_slots;
  uint32_t n_fast_slices; /* slices with CDR_SLICE_FAST (cdr_plan_scratch) */
  uint32_t n_wave_slices; /* slices with CDR_SLICE_WAVE (cdr_plan_slices_ex) */
  uint32_t n_reg_slices;  /* slices with CDR_SLICE_REG (cdr_plan_scratch) */
  uint32_t n_reg2_slices; /* slices with CDR_SLICE_REG2 (cdr_plan_scratch) */
  uint32_t n_reg0_slices; /* slices with CDR_SLICE_REG0 (cdr_plan_scratch) */
  uint32_t n_par_slices;  /* slices with CDR_SLICE_PAR: slices 0 .. n_par_slices - 1 (cdr_plan_slices_ex) */
  /* slice index range [class_lo[c], class_hi[c]) holding every slice of kernel class c
   * (CDR_CLASS_*, cdr_plan_class_ranges): each replay kernel is launched over its range
   * only; all zero = unknown, every kernel is launched over every slice */
  uint32_t class_lo[6], class_hi[6];
  cdr_cluster_meta cluster;
  int64_t now_ns;
  uint64_t uuid_seed;
  /* device copy of the batch's cdr_carry (pointers into device memory), or NULL; its
   * entries replay with the general kernel (cdr_plan_caps clears CDR_CAP_FAST/WAVE) */
  const cdr_carry* carry;
  /* class-sorted copy of the register-table slices (cdr_cls_plan_async +
   * cdr_cls_pack_async), or NULL: slice s's block starts at row cls_row0[s] of cls_slab
   * (standard CDR_ROW_BYTES rows) and holds its lanes' W, activity, timer and external
   * events in four regions of cls_rows[4 s + 0..3] rows (CDR_CLS_*) */
  const uint8_t* cls_slab;
  const uint64_t* cls_row0; /* [n_slices + 1], exclusive scan of the blocks' rows */
  const uint32_t* cls_rows; /* [n_slices * 4] */
  /* [n_wfs] device, nullable: entries with skip[w] != 0 are not replayed by this launch —
   * their lanes stay idle and their output records untouched (the caller marks them,
   * e.g. result.code = CDR_NOT_RUN).  A masked launch replays without class-sorted blocks. */
  const uint8_t* skip;
  /* task-slice rows of the batch (cdr_totals.xfer + cdr_totals.ttask), used to size the class
   * kernels' task staging when the output asks for task lists; 0 = unknown: the launcher
   * reads the last entry's capacities from caps (a copy and a stream synchronisation) */
  uint64_t task_rows;
} cdr_dev_batch;

/* Class-sorted blocks (replay_cls.inc).  Every register-table slice (CDR_SLICE_REG /
 * REG2 / REG0) can carry a second copy of its events, permuted per lane into four
 * class regions aligned across the slice's 64 lanes: W (decision and workflow events),
 * activity events, user-timer events, external (child / request-cancel / signal)
 * events, each region in history order; MarkerRecorded, CancelTimerFailed and
 * RequestCancelActivityTaskFailed (no state of their own) are left out, and a lane with
 * fewer events of a class than the slice's maximum gets CDR_EV_PAD rows there.  Columns
 * are the standard ones except: the task_id column holds the annotation
 * CDR_CLS_ANN(k, k - k0, d) — k the event's index in its history, k0 the index of its
 * call's first event, d = event_id - NextEventID at its call (0xFFFFFFFF when that does
 * not fit) — and type_flags' bits 21 / 22 mean "event_id not needed" / "version not
 * needed or equal to the previous W event's".  The replay reads them instead of the
 * original rows for the entity FSMs (one class per step), and the original rows for the
 * call structure and the version bookkeeping. */
#define CDR_CLS_W 0
#define CDR_CLS_A 1
#define CDR_CLS_T 2
#define CDR_CLS_X 3
#define CDR_SEF_CLS_NO_ID (1u << 21)
#define CDR_SEF_CLS_VER_SAME (1u << 22)
#define CDR_CLS_ANN(k, dk, d) ((uint64_t)(k) | ((uint64_t)(dk) << 20) | ((uint64_t)(d) << 32))
#define CDR_CLS_DROP 4 /* cdr_cls_of: a type with no state of its own (only the P loop sees it) */
#define CDR_CLS_SLICES (CDR_SLICE_REG | CDR_SLICE_REG2 | CDR_SLICE_REG0 | CDR_SLICE_PAR) /* slices with a block */
#define CDR_CLS_A_TYPES                                                                                       \
  (CDR_TB(CDR_EV_AT_SCHEDULED) | CDR_TB(CDR_EV_AT_STARTED) | CDR_TB(CDR_EV_AT_COMPLETED) |                    \
   CDR_TB(CDR_EV_AT_FAILED) | CDR_TB(CDR_EV_AT_TIMED_OUT) | CDR_TB(CDR_EV_AT_CANCELED) |                      \
   CDR_TB(CDR_EV_AT_CANCEL_REQUESTED))
#define CDR_CLS_T_TYPES (CDR_TB(CDR_EV_TIMER_STARTED) | CDR_TB(CDR_EV_TIMER_FIRED) | CDR_TB(CDR_EV_TIMER_CANCELED))
#define CDR_CLS_X_TYPES                                                                                         \
  (CDR_TB(CDR_EV_CHILD_INITIATED) | CDR_TB(CDR_EV_CHILD_STARTED) | CDR_TB(CDR_EV_CHILD_START_FAILED) |         \
   CDR_TB(CDR_EV_CHILD_COMPLETED) | CDR_TB(CDR_EV_CHILD_FAILED) | CDR_TB(CDR_EV_CHILD_CANCELED) |              \
   CDR_TB(CDR_EV_CHILD_TIMED_OUT) | CDR_TB(CDR_EV_CHILD_TERMINATED) | CDR_TB(CDR_EV_RCE_INITIATED) |           \
   CDR_TB(CDR_EV_RCE_FAILED) | CDR_TB(CDR_EV_EXT_CANCEL_REQUESTED) | CDR_TB(CDR_EV_SE_INITIATED) |             \
   CDR_TB(CDR_EV_SE_FAILED) | CDR_TB(CDR_EV_EXT_SIGNALED))
#define CDR_CLS_DROP_TYPES \
  (CDR_TB(CDR_EV_MARKER_RECORDED) | CDR_TB(CDR_EV_CANCEL_TIMER_FAILED) | CDR_TB(CDR_EV_AT_REQ_CANCEL_FAILED))
/* class-sorted events whose event_id a class loop reads (the others get CDR_SEF_CLS_NO_ID) */
#define CDR_CLS_NEED_ID                                                                                          \
  (CDR_TB(CDR_EV_WF_STARTED) | CDR_TB(CDR_EV_DT_SCHEDULED) | CDR_TB(CDR_EV_DT_STARTED) |                         \
   CDR_TB(CDR_EV_DT_TIMED_OUT) | CDR_TB(CDR_EV_DT_FAILED) | CDR_TB(CDR_EV_AT_SCHEDULED) |                        \
   CDR_TB(CDR_EV_TIMER_STARTED) | CDR_TB(CDR_EV_CHILD_INITIATED) | CDR_TB(CDR_EV_RCE_INITIATED) |                 \
   CDR_TB(CDR_EV_SE_INITIATED))
/* class region of an event type (CDR_CLS_W / A / T / X, or CDR_CLS_DROP); unknown types
 * go to W, whose loop reports them */
CDR_HD uint32_t cdr_cls_of(uint32_t type) {
  if (type >= 64) return CDR_CLS_W;
  const uint64_t b = 1ull << type;
  return (b & CDR_CLS_A_TYPES)      ? (uint32_t)CDR_CLS_A
         : (b & CDR_CLS_T_TYPES)    ? (uint32_t)CDR_CLS_T
         : (b & CDR_CLS_X_TYPES)    ? (uint32_t)CDR_CLS_X
         : (b & CDR_CLS_DROP_TYPES) ? (uint32_t)CDR_CLS_DROP
                                    : (uint32_t)CDR_CLS_W;
}

/* ------------------------------------------------------------ host planning */

/* Per-workflow output capacities (upper bounds derived from the input: counts of
 * entity-creating events, version runs, reset points, search-attribute pairs)
 * and their prefix offsets. */
int cdr_plan_caps(const cdr_batch* b, cdr_wf_caps* caps, cdr_totals* totals);

/* Slice assignment: workflows sorted by event count (descending, stable) and
 * dealt 64 to a slice.  Outputs lane_wf[n_slices*64], slice_len[n_slices],
 * slice_row0[n_slices]; returns n_slices via *n_slices and rows via *n_rows.
 * Call with lane_wf == NULL to query sizes only. */
int cdr_plan_slices(const cdr_wf_desc* wfs, uint32_t n_wfs, int32_t* lane_wf, uint32_t* slice_len,
                    uint64_t* slice_row0, uint32_t* n_slices, uint64_t* n_rows);

/* As cdr_plan_slices, with a mode: CDR_PLAN_WAVE gives every entry whose caps carry
 * CDR_CAP_WAVE and neither register-table cap (CDR_CAP_REG / REG2) a wave slice of its
 * own (after the lane slices, longest first) and
 * marks it in slice_flags (nullable; the other slices get 0).  `caps` may be NULL
 * when mode is 0.  Returns the number of wave slices via *n_wave (nullable). */
#define CDR_PLAN_WAVE 0x1u
/* with CDR_PLAN_WAVE: also the register-table entries get wave slices (by default they
 * stay in lane slices, where they replay cheaper) */
#define CDR_PLAN_WAVE_ALL 0x2u
/* with CDR_PLAN_WAVE the planner also gives a wave slice to every CDR_CAP_WAVE entry
 * whose history is longer than T = max(CDR_LONG_MIN, CDR_LONG_FACTOR x the lane events
 * per resident lane slot, i.e. lane events / (64 x CDR_LANE_RESIDENT)) — T /
 * CDR_LONG_REG2_DIV (at least CDR_LONG_MIN / 2) for CDR_CAP_REG2 entries: such a history
 * alone would set the lane kernels' critical path.  This bit turns that rule off. */
#define CDR_PLAN_NO_LONG 0x4u
/* with CDR_PLAN_WAVE (default on): the long register-table histories the rule above would
 * give wave slices go instead to CDR_SLICE_PAR lane slices (longest first, CDR_PAR_LANES to
 * a slice, the first slices of the plan), where the class-decomposed kernel runs their
 * loops on four waves at once */
#define CDR_PLAN_PAR 0x8u
/* with CDR_PLAN_PAR: every PAR history alone in its slice, the CDR_PAR_SOLO_MAX longest at most —
 * the plan of batches with task lists, whose PAR slices replay on k_replay_reg<TASKS>: a row there
 * costs the union of the handler groups its lanes hit, so one history per slice steps one group
 * (C5 --tasks 23.6 -> 16.0 ms; the PAR class kernel emits no tasks) */
#define CDR_PLAN_PAR_SOLO 0x10u
#define CDR_PAR_SOLO_MAX 512u
#define CDR_PAR_LANES 16u /* histories per CDR_SLICE_PAR slice (lanes 0 .. 15; the rest empty) */
#define CDR_PAR_SOLO 0u   /* ... except the longest CDR_PAR_SOLO, one per slice */
#define CDR_PAR_SOLO_LEN 16384u /* ... and every PAR history at least this long, one per slice
                                   (k_replay_cls: its class loops in wave form) */
#define CDR_PAR_MAX_SLICES 128u /* at most this many PAR slices (the longest histories); the rest stay lane slices */
#define CDR_LONG_MIN 1024u
#define CDR_LONG_FACTOR 2u
#define CDR_LONG_REG2_DIV 2u
#define CDR_PAR_FACTOR 1u /* CDR_PLAN_PAR: the long threshold's factor for PAR slices */
#define CDR_LANE_RESIDENT 2048u
int cdr_plan_slices_ex(const cdr_wf_desc* wfs, const cdr_wf_caps* caps, uint32_t n_wfs, uint32_t mode,
                       int32_t* lane_wf, uint32_t* slice_len, uint64_t* slice_row0, uint32_t* slice_flags,
                       uint32_t* n_slices, uint64_t* n_rows, uint32_t* n_wave);

/* Working-state scratch layout: per slice, slots = max over its lanes of the live
 * bounds in caps, and the slice's CDR_SLICE_* flags (CDR_SLICE_WAVE, when set on input by
 * cdr_plan_slices_ex, is kept and such slices get no scratch); returns the total words via
 * *total_words and the number of CDR_SLICE_FAST slices via *n_fast (nullable).
 * Outputs sized [n_slices]; pass NULL outputs to query the totals only. */
/* Kernel classes of the slices (by their CDR_SLICE_* flags) and the index range each
 * class's slices span: lo[c] = first, hi[c] = last + 1 (0, 0 for an absent class).  The
 * planner above puts a class's slices next to each other, so a range holds only its
 * class's slices; the kernels check the flags, so any order stays correct. */
enum cdr_kernel_class {
  CDR_CLASS_FAST = 0, CDR_CLASS_REG0 = 1, CDR_CLASS_REG = 2, CDR_CLASS_REG2 = 3, CDR_CLASS_WAVE = 4,
  CDR_CLASS_GENERAL = 5
};
int cdr_plan_class_ranges(const uint32_t* slice_flags, uint32_t n_slices, uint32_t* lo, uint32_t* hi);
int cdr_plan_scratch(const cdr_wf_caps* caps, const int32_t* lane_wf, uint32_t n_slices, uint64_t* scratch_off,
                     uint32_t* act_slots, uint32_t* tim_slots, uint32_t* slice_flags, uint64_t* total_words,
                     uint32_t* n_fast);

/* Arena words needed by the batch's attribute records. */
uint64_t cdr_plan_arena_words(const cdr_batch* b);

/* Pack the natural-order batch into the sliced columns (host memory, sized by the
 * planners above).  Columns are passed through a cdr_slices whose pointers are
 * cast away from const by the packer.  `threads` host threads (<=0: hardware). */
int cdr_pack_slices(const cdr_batch* b, cdr_slices* out, int threads);

/* ------------------------------------------------------------- device entry */

typedef struct cdr_ctx cdr_ctx;
/* Context options (cdr_opts_default fills the defaults). */
typedef struct cdr_opts {
  uint32_t plan_mode;       /* CDR_PLAN_* of the host-buffer calls' planning (CDR_PLAN_WAVE) */
  int32_t fast_path;        /* CDR_SLICE_FAST / REG / REG2 slices on their kernels (1) */
  int32_t reg_path;         /* CDR_SLICE_REG / REG2 slices on k_replay_reg (1) */
  int32_t concurrent;       /* wave-kernel slices on a side stream, concurrent with the lane kernels (1) */
  uint64_t workspace_bytes; /* device bytes reserved at creation for the host-buffer calls' event slab
                             * (0: on demand; the workspace only grows) */
} cdr_opts;
void cdr_opts_default(cdr_opts* opts);
/* A context on HIP device `device` (opts NULL: defaults); NULL when the device is absent
 * or its kernel image cannot load — there is no CPU fallback. */
cdr_ctx* cdr_create(int device, const cdr_opts* opts);
void cdr_destroy(cdr_ctx* ctx);

/* Route CDR_SLICE_FAST slices to the fast-path kernel and CDR_SLICE_REG slices to the
 * register-table kernel (default 1) or replay every lane slice with the general kernel
 * (0; parity tests run both).  Returns the old value. */
int cdr_set_fast_path(cdr_ctx* ctx, int enable);
/* Route CDR_SLICE_REG slices to k_replay_reg (default 1) or to the general kernel (0);
 * returns the old value. */
int cdr_set_reg_path(cdr_ctx* ctx, int enable);
/* Replay register-table slices that carry a class-sorted block (cdr_dev_batch.cls_slab)
 * with the class-decomposed kernel k_replay_cls (entries it leaves CLS_RETRY go through
 * k_replay_reg) or with k_replay_reg alone (CDR_CLS_OFF).  Modes:
 *   CDR_CLS_OFF      k_replay_reg alone
 *   CDR_CLS_ON       (default) k_replay_cls for device-resident batches that carry blocks
 *                    (the packer emitted them: cdr_pack_cls); the host-buffer calls
 *                    (cdr_replay_batch / cdr_rebuild_batch / cdr_replay_one) build none —
 *                    a batch replayed once pays more for its block (packing + H2D of a
 *                    second copy of the slab) than k_replay_cls saves over k_replay_reg
 *   CDR_CLS_ALONE    (tests) as CDR_CLS_BUILD, with no k_replay_reg pass, so an entry it
 *                    hands on keeps the internal result code 0x7FFF
 *   CDR_CLS_BUILD    as CDR_CLS_ON, and the host-buffer calls pack blocks too (host packer)
 * Returns the old mode. */
#define CDR_CLS_OFF 0
#define CDR_CLS_ON 1
#define CDR_CLS_ALONE 2
#define CDR_CLS_BUILD 3
int cdr_set_cls_path(cdr_ctx* ctx, int mode);

/* Host packer of the class-sorted blocks (the layout above), from a packed host slab
 * (cdr_pack_slices / the synthetic generator) and the entries' descriptors (ev_len):
 * cdr_plan_cls writes cls_rows[4 s + c] (n_slices * 4: the rows of each class region of
 * every CDR_CLS_SLICES slice, 0 for the others) and cls_row0[0..n_slices] (their
 * exclusive scan; cls_row0[n_slices] = total rows); cdr_pack_cls then writes the blocks
 * into cls_slab (total * CDR_ROW_BYTES bytes; padding elements carry type_flags
 * CDR_EV_PAD | CDR_SEF_CLS_NO_ID | CDR_SEF_CLS_VER_SAME and zero columns).  Byte for byte
 * the blocks cdr_cls_plan_async / cdr_cls_pack_async build on the device (padding
 * elements' other columns aside).  `threads` host threads (<= 0: hardware). */
int cdr_plan_cls(const cdr_slices* s, const cdr_wf_desc* wfs, uint32_t* cls_rows, uint64_t* cls_row0);
int cdr_pack_cls(const cdr_slices* s, const cdr_wf_desc* wfs, const uint32_t* cls_rows, const uint64_t* cls_row0,
                 uint8_t* cls_slab, int threads);

/* Size pass of the class-sorted blocks (see cdr_dev_batch.cls_slab): cls_rows[4 s + c]
 * (device, n_slices * 4) = the rows of each class region of every register-table slice
 * (0 for the others) and cls_row0[0..n_slices] (device, n_slices + 1) their exclusive
 * scan; the caller reads the total, cls_row0[n_slices], and allocates cls_slab at
 * total * CDR_ROW_BYTES bytes.  It also keeps, in the context's workspace (16 B per slab
 * element), each event's class position, block type word and annotation for the write pass.
 * Asynchronous. */
int cdr_cls_plan_async(cdr_ctx* ctx, const cdr_dev_batch* in, uint32_t* cls_rows, uint64_t* cls_row0,
                       void* stream);
/* Write pass: the class-sorted blocks into in->cls_slab at in->cls_row0 / cls_rows (from
 * cdr_cls_plan_async on the same batch, the last plan on this context): a transposition
 * through LDS, column by column, one workgroup per slice (slices longer than its LDS budget,
 * and every slice when the plan's map is not this batch's: a per-lane scatter).
 * Asynchronous. */
int cdr_cls_pack_async(cdr_ctx* ctx, const cdr_dev_batch* in, void* stream);

/* Slicing mode of cdr_replay_batch's planning (CDR_PLAN_*; default CDR_PLAN_WAVE).
 * Returns the previous mode. */
int cdr_set_plan_mode(cdr_ctx* ctx, uint32_t mode);

/* Replay a device-resident sliced batch into device-resident outputs on `stream`
 * (a hipStream_t; NULL = default stream).  Asynchronous: enqueues the replay
 * kernel and the continue-as-new finalize kernel and returns.
 * A context's asynchronous calls all go on ONE stream, in order: the retry lists and the
 * side streams the kernel classes fork onto are the context's (per-context workspace), so
 * two calls in flight on one context from different streams would share them.  Use one
 * context per stream (per goroutine in the cgo shim).
 * Carry-in (in->carry): loaded entries replay in the register-table kernels' carry-in
 * instantiations (their slices) or the general kernel; an entry whose loaded state
 * outgrows its variant is handed on, on the device, to the 12-activity variant and then to
 * the general kernel (replay_reg.inc).  Never plan a loaded entry onto a fast or wave slice
 * (cdr_plan_caps / cdr_plan_ndc_apply never do: CDR_CAP_LOADED).
 * Task lists (out->transfer set) with class-sorted blocks (in->cls_slab): the class kernels
 * stage each entry's tasks per class in the context's workspace and merge them on the device
 * (replay_cls.inc, k_tasks_merge); the workspace is sized from the batch's task-slice total,
 * which the first launch over a batch (a new in->caps pointer or entry count) reads back with
 * one blocking 40-byte copy of in->caps[n_wfs - 1] — later launches over the same batch stay
 * fully asynchronous.  A plan with task lists must have no wave slices (CDR_API_EINVAL).
 * Capacities (in->caps): every kernel writes an entry's rows into [*_off, *_off + *_cap) of
 * the caller's tables and nowhere else.  An entry whose grow-only state slices (vh_cap,
 * rp_cap, sa_cap) or task slices (xfer_cap, ttask_cap) cannot hold what its history produces
 * ends with CDR_E_BAD_INPUT, all n_* counts and both n_tasks zero, on every kernel route, and
 * leaves every other entry of the batch unaffected (schema.h CDR_E_BAD_INPUT: the failure
 * location).  The five pending-table capacities (act_cap .. signal_cap) are outside this
 * contract: they must be the planner's values (cdr_plan_caps / cdr_plan_ndc_apply) — the lane
 * kernels size their working sets from act_live / timer_live and the CDR_CAP_* flags and never
 * read them, the wave kernel uses them as working bounds. */
int cdr_replay_sliced_async(cdr_ctx* ctx, const cdr_dev_batch* in, const cdr_out* out, void* stream);

/* Whole pipeline for host-resident data: plan + pack + H2D + replay + D2H on `stream`
 * (a hipStream_t; NULL = the default stream).  `caps` must come from cdr_plan_caps on the
 * same batch; `out` points at host buffers sized by its totals (out->last_decision, if
 * set, at n_wfs records).  Device buffers come from the context's grow-only workspace:
 * a warmed-up context allocates nothing.  Synchronous on `stream`; one call at a time
 * per context. */
int cdr_replay_batch(cdr_ctx* ctx, const cdr_batch* b, const cdr_wf_caps* caps, const cdr_totals* totals,
                     cdr_out* out, void* stream);

/* The drop-in applyEvents shim's call: the sequence of applyEvents calls
 * of ONE workflow — `b` holds its entry (0) and, when its history continues as new, the
 * new run's entry (b->n_wfs 1 or 2).  The context plans the capacities itself and
 * replays into its own host buffers: *view receives the outputs (tables at the
 * offsets in *caps, last_decision set), valid until the next call on `ctx`.  Synchronous
 * on `stream`. */
int cdr_replay_one(cdr_ctx* ctx, const cdr_batch* b, const cdr_out** view, const cdr_wf_caps** caps, void* stream);

/* refreshTasks (mutableStateTaskRefresher.go:66-160) over the rebuilt states of a
 * replay: run after cdr_replay_sliced_async on the same `in` / `out` (same stream).
 * For every entry whose result is CDR_OK it regenerates the transfer and timer tasks
 * of the rebuilt state at time `now_ns` into out->transfer / out->timer_tasks (the
 * entry's caps.xfer_off / ttask_off slices, counts in out->n_tasks — the stateBuilder
 * lists, if any, are replaced), clears every pending activity's TimerTaskStatus and
 * every user timer's TaskID and sets the ones the activity / user-timer picks created
 * (:264-342).  Events the refresher reads (WorkflowExecutionStarted, the scheduled /
 * initiated events of pending entities — the reference's events cache) are looked up
 * among the entry's own events in `in`; a miss, a Decider initiator with a first-decision
 * backoff, an unknown target domain or an overflowing task slice set the entry's
 * result.code (CDR_E_REFRESH_*, CDR_E_DOMAIN_NOT_FOUND) and leave its tables unchanged
 * with no tasks.  `flags`: CDR_REFRESH_ADVANCED_VISIBILITY adds the
 * UpsertWorkflowSearchAttributes task (:148-156); CDR_REFRESH_SNAPSHOT_PASSIVE below.
 * Asynchronous. */
#define CDR_REFRESH_ADVANCED_VISIBILITY 0x1u
/* then CloseTransactionAsSnapshot(now, transactionPolicyPassive)
 * (mutableStateBuilder.go:3787-3855): with the passive policy and no new events its only
 * effect on the outputs is setTaskInfo (historyEngine.go:2383-2397) — every task's Version
 * becomes GetCurrentVersion() (LastUpdatedTimestamp = now is the caller's: the record
 * omits it) */
#define CDR_REFRESH_SNAPSHOT_PASSIVE 0x2u
int cdr_refresh_tasks_async(cdr_ctx* ctx, const cdr_dev_batch* in, const cdr_out* out, int64_t now_ns,
                            uint32_t flags, void* stream);

/* nDCStateRebuilder.rebuild's replay + refreshTasks for host-resident data: as
 * cdr_replay_batch, then cdr_refresh_tasks_async at b->now_ns.  out->transfer,
 * timer_tasks and n_tasks are required (sized by `totals`).  Synchronous on `stream`. */
int cdr_rebuild_batch(cdr_ctx* ctx, const cdr_batch* b, const cdr_wf_caps* caps, const cdr_totals* totals,
                      cdr_out* out, uint32_t flags, void* stream);

/* Persisted-format row encoders: the SQL persistence's per-row blobs,
 * thriftrw binary protocol (common/persistence/sql/blob.go:61-73, protocol.Binary) of
 * the sqlblobs structs the row writers build (common/persistence/sql/workflowStateMaps.go):
 *   table 1  TimerInfo{Version, StartedID, ExpiryTimeNanos, TaskID}
 *            (sqlblobs.thrift:201-206, workflowStateMaps.go:242-247): CDR_BLOB_TIMER_BYTES
 *   table 3  RequestCancelInfo{Version, InitiatedEventBatchID, CancelRequestID}
 *            (sqlblobs.thrift:195-199, workflowStateMaps.go:507-511): CDR_BLOB_CANCEL_BYTES;
 *            CancelRequestID is the row's UUID in RFC 4122 text form (hi then lo, 8-4-4-4-12
 *            lowercase hex)
 * Every field is set (the row writers pass pointers), so each blob has a fixed size
 * (CDR_BLOB_*_BYTES); row r of the table (caps.*_off + j) is written to the 16-B aligned
 * slot blobs + r * CDR_BLOB_*_STRIDE (its first *_BYTES bytes are the blob, the rest
 * zero), for the rows j < result.n_* of every CDR_OK entry (other slots untouched);
 * `blobs` must be 16-B aligned.  Asynchronous. */
#define CDR_BLOB_TIMER_BYTES 45u
#define CDR_BLOB_TIMER_STRIDE 48u
#define CDR_BLOB_CANCEL_BYTES 66u
#define CDR_BLOB_CANCEL_STRIDE 80u
int cdr_encode_rows_async(cdr_ctx* ctx, int table, const cdr_dev_batch* in, const cdr_out* out, uint8_t* blobs,
                          void* stream);

/* The variable-size row blobs (encode_var.hip):
 *   table 0  ActivityInfo        (sqlblobs.thrift:136-168, workflowStateMaps.go:48-83)
 *   table 2  ChildExecutionInfo  (sqlblobs.thrift:170-184, workflowStateMaps.go:371-385)
 *   table 4  SignalInfo          (sqlblobs.thrift:186-193, workflowStateMaps.go:632-639)
 *   table 5  WorkflowExecutionInfo of the execution row (sqlblobs.thrift:73-134,
 *            buildExecutionRow sqlExecutionManagerUtil.go:1197-1308), one row per entry
 * Strings come from a device string table (handle h's bytes are bytes[off[h], off[h+1]),
 * handle 0 = "" / nil).  Its conventions: a plain string or binary field is its bytes; a
 * NonRetriableErrors handle holds the wire body of the list<string> (element type, i32
 * count, elements) and a Memo handle the wire body of the Memo struct — what
 * cdr_ingest_decode interns.  UUID-typed binaries (ParentDomainID, ParentRunID,
 * StartedRunID) are MustParseUUID of their strings; ID strings the replay generates
 * (CreateRequestID, SignalRequestID, the branch ID) are RFC 4122 text of their 128 bits.
 * Go's map iteration order is random, so the reference has no fixed byte order for the
 * map fields (LastReplicationInfo, SearchAttributes, Memo): they are written in cluster-
 * index, row and input order.  Not carried by the replay projection, and so written as a
 * fresh replay leaves them: ScheduledEvent / StartedEvent / InitiatedEvent (nil),
 * CompletionEvent (nil), the branch's ancestors ([]); the execution row's fields outside
 * the projection come from cdr_exec_persist.
 * Two calls: with blobs == NULL, a size pass and an exclusive scan write row_off[0..n_rows]
 * (device, n_rows + 1: row r's blob is bytes [row_off[r], row_off[r+1]) — zero-length for
 * rows past an entry's count and for entries that did not replay OK) and per-row
 * CDR_BLOB_* status codes into row_status (device, nullable); the caller reads
 * row_off[n_rows] (the total), allocates `blobs` and calls again to write them.  Rows are
 * the table's capacity rows (caps.*_off + j; n_rows = the table's total capacity), for
 * table 5 the entries (n_rows = n_wfs); cluster_names[i] (device) is the handle of cluster
 * i's name, the LastReplicationInfo key of 2DC entries.  Asynchronous on `stream`. */
typedef struct cdr_strtab {
  const uint8_t* bytes; /* device */
  const uint64_t* off;  /* device, n + 1 */
  uint32_t n, _pad;
} cdr_strtab;
/* per-entry inputs of buildExecutionRow outside the replay projection */
typedef struct cdr_exec_persist {
  int64_t start_version, current_version; /* buildExecutionRow's startVersion / currentVersion */
  int64_t start_time, last_updated_time;  /* UnixNano (CDR_ZERO_TIME_NANOS: Go's zero time) */
  int64_t history_size, sticky_s2s_timeout;
  uint32_t execution_context, sticky_task_list; /* handles */
  uint32_t client_library_version, client_feature_version, client_impl, _pad;
} cdr_exec_persist;
#define CDR_ZERO_TIME_NANOS (-6795364578871345152ll) /* time.Time{}.UnixNano() */
/* A handle >= strs->n is CDR_BLOB_E_HANDLE in every field that reads it, UUID-typed and Memo
 * fields included (nothing is parsed); a row with a status != 0 has unspecified bytes. */
#define CDR_BLOB_OK 0
#define CDR_BLOB_E_UUID 1   /* MustParseUUID would panic on the string */
#define CDR_BLOB_E_HANDLE 2 /* a handle past the string table */
#define CDR_BLOB_E_MEMO 3   /* the Memo handle does not hold a Memo struct body */
int cdr_encode_blobs_async(cdr_ctx* ctx, int table, const cdr_dev_batch* in, const cdr_out* out,
                           const cdr_strtab* strs, const cdr_exec_persist* persist, const uint32_t* cluster_names,
                           uint64_t n_rows, uint64_t* row_off, uint8_t* blobs, int32_t* row_status, void* stream);

/* The Cassandra persistence's form of the same rows (common/persistence/cassandra/
 * cassandraPersistenceUtil.go; CQL templates cassandraPersistence.go:114-306,439-520): per row
 * the values the statement that writes it binds, in order, each a CQL native-protocol [bytes]
 * value — big-endian int32 length (-1 = null), then the value as gocql (v0.0.0-20171220143535-
 * 56a164ee9f31, go.mod:22) marshals it for the column's CQL type: bigint / int big-endian,
 * boolean one byte, double IEEE big-endian, timestamp milliseconds since the epoch (the zero
 * time.Time: zero bytes), text / blob the bytes (a nil []byte: null), uuid the 16 bytes gocql's
 * ParseUUID reads from the string (CDR_BLOB_E_UUID where it fails), list<text> / map<text, blob>
 * an int32 count and the [bytes] elements, a UDT its fields' [bytes] in declaration order.
 *   table 0  activity_map[schedule_id] = activity_info (updateActivityInfos :1264-1337): the
 *            key, then the UDT's 33 fields
 *   table 1  timer_map[timer_id] = timer_info (updateTimerInfos :1384-1422)
 *   table 2  child_executions_map[initiated_id] = child_execution_info (:1444-1503; "" started
 *            run -> emptyRunID)
 *   table 3  request_cancel_map[initiated_id] = request_cancel_info (:1530-1568)
 *   table 4  signal_map[initiated_id] = signal_info (:1590-1631)
 *   table 5  the execution row's SET values of updateExecution (:625-890): the
 *            workflow_execution UDT's 58 fields (no parent -> emptyDomainID / "" / emptyRunID /
 *            emptyInitiatedID), then the 2DC replication_state's 5 (last_replication_info
 *            a map<text, frozen<replication_info>> keyed by cluster_names) and next_event_id,
 *            or next_event_id, version_histories and its encoding (NDC), or next_event_id
 *            (local); what the projection does not carry comes from `persist`, as for table 5
 *            of cdr_encode_blobs_async
 * The statements' WHERE / IF values (shard, row type, the execution's keys, the condition) are
 * the caller's.  Map iteration order is Go's random order in the reference; maps are written
 * in input / cluster-index order.  Two calls (sizes, then values) as cdr_encode_blobs_async. */
int cdr_encode_cql_async(cdr_ctx* ctx, int table, const cdr_dev_batch* in, const cdr_out* out,
                         const cdr_strtab* strs, const cdr_exec_persist* persist, const uint32_t* cluster_names,
                         uint64_t n_rows, uint64_t* row_off, uint8_t* values, int32_t* row_status, void* stream);

/* The WorkflowMutation of a carry-in replay (schema.h cdr_mutation; mutation.hip): run after
 * cdr_replay_sliced_async on the same `in` / `out` (same stream).  This is the step after the
 * replay in nDCHistoryReplicator.applyNonStartEventsToCurrentBranch and the 2DC
 * historyReplicator: transactionMgr.updateWorkflow -> CloseTransactionAsMutation
 * (service/history/mutableStateBuilder.go:3721-3785) -> UpdateWorkflowExecution, which writes
 * the execution row, per pending table the rows to upsert and the keys to delete, and
 * Condition = nextEventIDInDB.  The call diffs, per entry and table, the loaded rows
 * (in->carry) against the replayed rows (out) by key and writes the net mutation into `mut`:
 * upserts compacted in mut->upsert — a cdr_out the row encoders (cdr_encode_rows_async,
 * cdr_encode_blobs_async, cdr_encode_cql_async) take as it is — delete keys and the per-entry
 * cdr_mut_info.  Nothing is written for rows past an entry's counts; an entry whose replay is
 * not CDR_OK gets only its info record and a copy of its result.
 * Preconditions: both states' pending tables in ascending, unique key order (every replay
 * path writes them so); the kernel checks the order as it merges — an entry that violates it
 * gets CDR_MUT_E_ORDER and zero counts (its own upsert / delete slices are then unspecified,
 * other entries are unaffected).  Timer keys are string handles: equal timer IDs must have
 * equal handles in the loaded state and in the batch (the replay kernels need the same).
 * Capacities: the delete arrays are sized by in->carry->totals and the upsert tables by the
 * totals of in->caps; delete counts cannot exceed the loaded row counts nor upsert counts
 * OUT's, so nothing can overflow.
 * One launch, no allocation, no host round trip; asynchronous on `stream`.  CDR_API_EINVAL
 * for null arguments and for in->carry == NULL (a batch without loaded states has no
 * mutation: everything it writes is a snapshot). */
int cdr_mutation_async(cdr_ctx* ctx, const cdr_dev_batch* in, const cdr_out* out, const cdr_mutation* mut,
                       void* stream);
/* The same for host buffers (as cdr_rebuild_batch): `b->carry` (the loaded states), `caps` /
 * `totals` of the replayed batch and `out` (its replay's outputs) are uploaded into the
 * context's grow-only workspace together with the current contents of `mut`'s buffers, the
 * kernel runs, and `mut`'s buffers are downloaded (bytes the kernel leaves untouched keep the
 * caller's values).  Only b->n_wfs and b->carry are read from `b`.  Synchronous on `stream`;
 * one call at a time per context. */
int cdr_mutation_batch(cdr_ctx* ctx, const cdr_batch* b, const cdr_wf_caps* caps, const cdr_totals* totals,
                       const cdr_out* out, cdr_mutation* mut, void* stream);

/* ---------------------------------------------- SyncActivity (sync.hip) */
/* Batched historyReplicator.SyncActivity (service/history/historyReplicator.go:160-295) on
 * loaded states in cdr_out form: per request the walk of its exits (:198-253), then for a
 * request that applies resetActivityTimerTaskStatus (:261-270; IsVersionFromSameCluster,
 * common/cluster/metadata.go:163-165), ReplicateActivityInfo on the pending-activity row
 * (mutableStateBuilder.go:1200-1231) and GetActivityTimerTaskIfNeeded over the state's rows
 * (timerBuilder.go:211-230,249-312,384-408; ties by time, scheduleID, then ScheduleToClose <
 * StartToClose / ScheduleToStart < Heartbeat, as refreshTasks).  Requests of one state apply
 * in order; schema.h cdr_sync_activity / cdr_sync_result describe the records.
 *
 * cdr_plan_sync (host): groups n_req requests by state with a stable counting sort by `wf`.
 * order[i] is the index in `reqs` of the i-th request of the grouped sequence; the requests of
 * state s are [req_off[s], req_off[s + 1]); requests with wf < 0 or wf >= n_states form a
 * trailing group [req_off[n_states], req_off[n_states + 1] = n_req), so req_off has
 * n_states + 2 entries.  The caller gathers reqs through `order` before the calls below. */
int cdr_plan_sync(const cdr_sync_activity* reqs, uint32_t n_req, uint32_t n_states, uint32_t* order,
                  uint32_t* req_off);
/* Applies the grouped requests: reqs [n_req], req_off [at least n_states + 1] (requests from
 * req_off[n_states] on are the trailing group: SKIP_NO_WORKFLOW for wf < 0, else E_STATE),
 * state_caps [n_states], the arrays `state` names and res [n_req] are device memory; `state`
 * and `cluster` themselves are host structs.  Of `state` only result, exec, repl, vh and act
 * are read; state->act is updated in place (as cdr_ndc_replicate_async updates its `state`):
 * the synced row's version, scheduled_time, started_id, started_time, last_heartbeat_time,
 * attempt, flags (CDR_AI_STARTED_TIME_SET iff started, CDR_AI_HEARTBEAT_TIME_SET always) and
 * timer_task_status, and the bit the timer pick sets on its head row; every other byte of act,
 * rows of states without an applied request and rows past a state's n_activity keep their
 * values.  res[i] belongs to reqs[i].  Rows of one state must be in ascending unique
 * schedule_id order (every replay path writes them so; cdr_mutation_async relies on the same).
 * One launch, no allocation, no host round trip; asynchronous on `stream`.  CDR_API_EINVAL
 * for null arguments or cluster->failover_version_increment <= 0. */
int cdr_sync_activity_async(cdr_ctx* ctx, const cdr_sync_activity* reqs, const uint32_t* req_off, uint32_t n_req,
                            uint32_t n_states, const cdr_wf_caps* state_caps, const cdr_out* state,
                            const cdr_cluster_meta* cluster, cdr_sync_result* res, void* stream);
/* The same for host buffers (as cdr_mutation_batch): the requests, req_off and the states'
 * result, exec, repl, vh and act records (sized by state_totals) are uploaded into the
 * context's grow-only workspace, the same kernel runs, then state->act and res are downloaded.
 * Synchronous on `stream`; one call at a time per context. */
int cdr_sync_activity_batch(cdr_ctx* ctx, const cdr_sync_activity* reqs, const uint32_t* req_off, uint32_t n_req,
                            uint32_t n_states, const cdr_wf_caps* state_caps, const cdr_totals* state_totals,
                            const cdr_out* state, const cdr_cluster_meta* cluster, cdr_sync_result* res,
                            void* stream);
/* Lanes that work on one state in the sync kernel: 4, 8, 16 or 64.  The default,
 * CDR_SYNC_GROUP, is the one tools/sync_bench.py measured fastest on an MI355X (1M config-3
 * prefix states, one and four requests per workflow: profiles/sync_activity.json).  Returns
 * the previous value, or CDR_API_EINVAL for another value.  A measurement knob: every value
 * computes the same bytes. */
#define CDR_SYNC_GROUP 4
int cdr_set_sync_group(cdr_ctx* ctx, int lanes);

/* ---------------------------------------------- standby task verification (standby.hip) */
/* Batched timerQueueStandbyProcessorImpl.process / transferQueueStandbyProcessorImpl.process
 * (service/history/timerQueueStandbyProcessor.go:173-225, transferQueueStandbyProcessor.go:
 * 137-204) on loaded states in cdr_out form: the standby cluster's consumer of the tasks
 * cdr_out.transfer / timer_tasks hold.  schema.h cdr_standby_task / cdr_standby_result describe
 * the records, cdr_sb_action what the caller does, cdr_sb_reason the exit taken.  Per request:
 *
 *   load (loadMutableStateForTimerTask / ...TransferTask, xdcUtil.go:95-169): wf < 0 is DONE;
 *     event_id >= next_event_id is DONE (there is one copy of the state: the reload finds the
 *     same) unless the task is a DecisionTimeout / DecisionTask with decision_schedule_id ==
 *     event_id and decision_attempt > 0; then the IsWorkflowExecutionRunning gate of processTimer
 *     (timerQueueStandbyProcessor.go:555-558) / processTransfer (transferQueueStandbyProcessor.go:
 *     580-583; CloseExecution passes it, processTaskIfClosed).  The type switch comes first: the
 *     types it answers without a state (ActivityRetryTimer, DeleteHistoryEvent, ResetWorkflow,
 *     a ScheduleToStart DecisionTimeout, an unknown type) read no state, but a failed record or
 *     wf >= n_states is E_STATE for every type.
 *   shouldProcessTask is the caller's domain filter: it submits only tasks it would process.
 *   verifyTaskVersion (xdcUtil.go:71-91): passes without CDR_SBT_GLOBAL_DOMAIN, else compares
 *     the entity's version with task.version.
 *   discardTask (timerQueueStandbyProcessor.go:618-626, transferQueueStandbyProcessor.go:652-660):
 *     now - visibility_ts > 3 * standby_delay (the difference saturates as time.Sub does); a
 *     pending entity gives RETRY without it, FETCH with it, DISCARDED with it on the last attempt.
 *   UserTimer (:227-276): the earliest expiry_time over the state's timer rows against
 *     visibility_ts, both floored to whole seconds (IsTimerExpired, timerBuilder.go:198-203;
 *     time.Unix() floors, also below zero).  The reference looks at the head of the sorted list
 *     only and flooring is monotonic, so this is a min-reduction.
 *   ActivityTimeout (:278-374): the same over the earliest timer of every activity row
 *     (loadActivityTimers, timerBuilder.go:249-312); when none has expired, a Heartbeat task
 *     clears CDR_TTS_HEARTBEAT on its row if the row exists (:341-348), GetActivityTimerTaskIfNeeded
 *     runs as in cdr_sync_activity_async (same tie rule), and if either changed something the
 *     result is UPDATED with the rows, the task and last_write_version (:359-372).
 *   DecisionTimeout (:376-427), WorkflowBackoffTimer (:429-473; HasProcessedOrPendingDecision,
 *     mutableStateDecisionTaskManager.go:731-733), WorkflowTimeout (:475-513; GetStartVersion,
 *     mutableStateBuilder.go:504-524: repl.start_version for 2DC, the first version-history item's
 *     version for NDC, CDR_EMPTY_VERSION for a local builder).
 *   ActivityTask (transferQueueStandbyProcessor.go:206-246), DecisionTask (:248-295; the timeout
 *     is min(workflow_timeout, CDR_MAX_TASK_TIMEOUT)): pushToMatching = now - visibility_ts >
 *     standby_delay.  CloseExecution (:297-361), CancelExecution (:363-400), SignalExecution
 *     (:402-439), StartChildExecution (:441-482), RecordWorkflowStarted / UpsertWorkflowSearch
 *     Attributes (:484-550).
 *
 * Requests of one state apply in order (an UPDATED ActivityTimeout changes what the next
 * request of the state sees); states are independent.
 *
 * cdr_plan_standby (host): cdr_plan_sync's contract for cdr_standby_task (req_off has
 * n_states + 2 entries; strangers form the trailing group). */
int cdr_plan_standby(const cdr_standby_task* reqs, uint32_t n_req, uint32_t n_states, uint32_t* order,
                     uint32_t* req_off);
/* Verifies the grouped requests: the contract of cdr_sync_activity_async — reqs [n_req], req_off
 * [at least n_states + 1], state_caps [n_states], the arrays `state` names and res [n_req] are
 * device memory, `state` and `cluster` host structs; a record whose result.code != CDR_OK is not
 * touched; rows of one state are in ascending unique key order.  Of `state` result, exec, repl,
 * vh, act, timer, child, cancel and signal are read.  state->act is updated in place by UPDATED
 * requests only, and only the timer_task_status of the rows the result names; every other byte
 * of act keeps its value.  now_ns: shard.GetCurrentTime(clusterName), already delayed;
 * standby_delay_ns: StandbyClusterDelay.  res[i] belongs to reqs[i].  One launch, no
 * allocation, no host round trip; asynchronous on `stream`.  CDR_API_EINVAL for null arguments
 * or standby_delay_ns <= 0. */
int cdr_standby_tasks_async(cdr_ctx* ctx, const cdr_standby_task* reqs, const uint32_t* req_off, uint32_t n_req,
                            uint32_t n_states, const cdr_wf_caps* state_caps, const cdr_out* state,
                            const cdr_cluster_meta* cluster, int64_t now_ns, int64_t standby_delay_ns,
                            cdr_standby_result* res, void* stream);
/* The same for host buffers (as cdr_sync_activity_batch): requests, req_off and the states'
 * records (sized by state_totals) are uploaded into the context's grow-only workspace, the same
 * kernel runs, then state->act and res are downloaded.  Synchronous on `stream`; one call at a
 * time per context. */
int cdr_standby_tasks_batch(cdr_ctx* ctx, const cdr_standby_task* reqs, const uint32_t* req_off, uint32_t n_req,
                            uint32_t n_states, const cdr_wf_caps* state_caps, const cdr_totals* state_totals,
                            const cdr_out* state, const cdr_cluster_meta* cluster, int64_t now_ns,
                            int64_t standby_delay_ns, cdr_standby_result* res, void* stream);
/* Lanes that work on one state in the standby kernel: 4, 8, 16 or 64, as cdr_set_sync_group.
 * Returns the previous value, or CDR_API_EINVAL.  Every value computes the same bytes. */
#define CDR_STANDBY_GROUP 4
int cdr_set_standby_group(cdr_ctx* ctx, int lanes);

/* Stream compaction of the per-workflow pending tables into dense tables
 * (device pointers): for each table, rows [caps.off, caps.off + result.n) of every
 * workflow are copied to dense[row_base[w] ...]; row_base is an exclusive scan of
 * the counts (written to `row_base` [n_wfs+1]).  Tables: 0 activity, 1 timer,
 * 2 child, 3 cancel, 4 signal. */
int cdr_compact_async(cdr_ctx* ctx, int table, const cdr_dev_batch* in, const cdr_out* out, void* dense,
                      uint64_t* row_base, void* stream);

/* Order-independent 64-bit checksum of every OK workflow's outputs (sum over
 * workflows of a per-workflow hash) — reduced across GPUs with RCCL by the
 * multi-GPU driver.  Writes one u64 to `*dev_sum` (device memory). */
int cdr_checksum_async(cdr_ctx* ctx, const cdr_dev_batch* in, const cdr_out* out, uint64_t* dev_sum,
                       void* stream);
/* The same, plus each entry's hash in per_entry[n_wfs] (device memory, nullable): the
 * full-size parity check compares these entry by entry with the CPU restatement's
 * (oracle/digest_ref.cpp restates the hash).  Hash of entry w: a fold of cdr_mix64 over
 * (code | flags << 32), fail_event_id and, when OK, the 8-byte words of its ExecutionInfo,
 * ReplicationState (2DC builder), version-history items, pending rows, reset points and
 * search attributes — the CopyToPersistence projection (mutableStateBuilder.go:257-270). */
int cdr_entry_digests_async(cdr_ctx* ctx, const cdr_dev_batch* in, const cdr_out* out, uint64_t* per_entry,
                            uint64_t* dev_sum, void* stream);

/* ------------------------------------------------ NDC branches (ndc.hip) */
/* Conflict resolution around the replay when replication tasks fork a history
 * (SURVEY §8(d) C5).  Per workflow w (all pointers device memory):
 *
 *   cdr_ndc_branch_async: task[w] against the workflow's persisted VersionHistories
 *     vhs[w] (items in `pool`): nDCBranchMgr.prepareVersionHistory
 *     (service/history/nDCBranchMgr.go:80-249: FindLCAVersionHistoryIndexAndItem,
 *     IsLCAAppendable, verifyEventsOrder, DuplicateUntilLCAItem + createNewBranch's
 *     AddVersionHistory) then nDCConflictResolver.prepareMutableState
 *     (nDCConflictResolver.go:73-114), and for a lower-version task on a non-current
 *     branch the backfill's AddOrUpdateItem (nDCHistoryReplicator.go:437-447).  vhs[w]
 *     is updated only when dec[w].code is CDR_OK; dec[w].action says what the caller
 *     replays next (CDR_NDC_*).
 *   cdr_ndc_rebuild_verify_async: after the rebuild replay of every CDR_NDC_REBUILD
 *     workflow (entry w of `out`, NDC builder, expected_next_event_id =
 *     dec[w].rebuild_next_event_id — nDCStateRebuilder.rebuild, nDCStateRebuilder.go:92-160):
 *     SetCurrentBranchToken(dec[w].rebuild_token), the rebuilt VersionHistory must equal
 *     the branch's (else result.code = CDR_E_REBUILD_VH_MISMATCH, nDCConflictResolver.go:
 *     154-165), then vhs[w].current = the branch (SetCurrentVersionHistoryIndex, :172-174).
 *   cdr_vhs_sync_async: after a replay applied to the current branch, its VersionHistory
 *     (the replay output's items and token) becomes branch vhs[w].current (a workflow
 *     with no branch gets its first, NewVersionHistories).  Needs items_cap >= the
 *     entry's caps.vh_cap.
 * Asynchronous on `stream`. */
int cdr_ndc_branch_async(cdr_ctx* ctx, const cdr_ndc_task* tasks, const cdr_vh_item* task_items, uint32_t n,
                         cdr_vhs* vhs, cdr_vh_item* pool, cdr_ndc_decision* dec, void* stream);
int cdr_ndc_rebuild_verify_async(cdr_ctx* ctx, uint32_t n, const cdr_ndc_decision* dec, cdr_vhs* vhs,
                                 const cdr_vh_item* pool, const cdr_wf_caps* caps, const cdr_out* out, void* stream);
int cdr_vhs_sync_async(cdr_ctx* ctx, uint32_t n, cdr_vhs* vhs, cdr_vh_item* pool, const cdr_wf_caps* caps,
                       const cdr_out* out, void* stream);

/* One round of NDC replication tasks over n workflows, device-resident end to end — the
 * batch form of nDCHistoryReplicator.applyNonStartEvents (service/history/
 * nDCHistoryReplicator.go:246-470) for task w of workflow w:
 *   1. nDCBranchMgr.prepareVersionHistory + nDCConflictResolver.prepareMutableState
 *      (k_ndc_branch, as cdr_ndc_branch_async) -> dec[w];
 *   2. CDR_NDC_REBUILD: nDCStateRebuilder.rebuild (nDCStateRebuilder.go:92-160) — entry w of
 *      `rebuild` replayed on a fresh NDC builder (the other entries masked), the
 *      next-event check, SetCurrentBranchToken, refreshTasks at refresh_now (its tasks in
 *      rebuild_out) — then nDCConflictResolver.rebuild's verification and branch switch
 *      (nDCConflictResolver.go:117-184, as cdr_ndc_rebuild_verify_async);
 *   3. applyNonStartEventsToCurrentBranch (:330-398): entry w of `apply` replayed onto the
 *      REBUILT state kept in memory (cdr_carry.in_memory: no Load) or, for
 *      CDR_NDC_APPLY_CURRENT, onto the loaded current state; its VersionHistory becomes the
 *      current branch's (as cdr_vhs_sync_async);
 *   4. `state` (device records with per-entry capacities state_caps) := the applied state;
 *      a task that fails leaves its error in state->result[w] (that workflow is skipped by
 *      later rounds); skipped / backfilled tasks leave the state as it was.
 * `rebuild` / `apply` are device-resident batches (host structs holding device pointers)
 * with entry w = workflow w and no continue-as-new entries; `apply` is planned with
 * cdr_plan_ndc_apply(state_caps) and both without class-sorted blocks.  rebuild_out needs
 * transfer / timer_tasks / n_tasks (the refresher's task lists).  Entries a step does not
 * run have result.code CDR_NOT_RUN in that step's output.  No device allocation once the
 * context's workspace is warm; asynchronous on `stream`. */
typedef struct cdr_ndc_round {
  const cdr_ndc_task* tasks;     /* [n] device */
  const cdr_vh_item* task_items; /* device */
  cdr_dev_batch rebuild;
  cdr_out rebuild_out;
  cdr_dev_batch apply;
  cdr_out apply_out;
  cdr_ndc_decision* dec; /* [n] device, out */
  int64_t refresh_now;   /* nDCStateRebuilder.rebuild's `now` */
  uint32_t refresh_flags, _pad; /* CDR_REFRESH_* of the rebuild's refreshTasks */
} cdr_ndc_round;
int cdr_ndc_replicate_async(cdr_ctx* ctx, uint32_t n, const cdr_ndc_round* round, cdr_vhs* vhs, cdr_vh_item* pool,
                            const cdr_wf_caps* state_caps, const cdr_out* state, void* stream);
/* Capacities of a round's `apply` batch (cdr_plan_caps restated for carry-in entries whose
 * loaded state has at most state_caps[w] rows; every entry replays in the general kernel). */
int cdr_plan_ndc_apply(const cdr_batch* b, const cdr_wf_caps* state_caps, cdr_wf_caps* caps, cdr_totals* totals);

/* ------------------------------------------- 2DC replication rounds (xdc.hip) */
/* historyReplicator.ApplyEvents (service/history/historyReplicator.go:339-763, H below) for one
 * task per workflow: the replication path while EnableNDC is off.
 *
 *   cdr_xdc_admit_host / cdr_xdc_admit_async: task[w] against the target run's records
 *     (state->result / exec / repl [w]; not read for a task with CDR_XDC_NO_STATE) -> dec[w]:
 *     the empty-task and start-event exits (H:377-410), ApplyOtherEventsMissingMutableState
 *     (H:451-519), ApplyOtherEventsVersionChecking (H:521-653) with
 *     conflictResolutionTerminateCurrentRunningIfNotSelf (H:925-999) and getLatestCheckpoint
 *     (H:1115-1140), then, for a state that passes, ApplyOtherEvents' event-id check (H:664-686)
 *     and ApplyReplicationTask's running check (H:704-707).  One function (csrc/xdc_admit.h)
 *     compiled for both; the host form takes host records, the device form device records and
 *     runs on `stream`.  The state is not written.  Valid alone, for callers that stage their
 *     own replays: a task whose events end in ContinuedAsNew goes this way.  tasks / dec are
 *     16-byte aligned; state_caps is not read (the decision reads no table rows).
 *   What the decision only names is the caller's — everything on the active side that writes
 *     events: reapplyEvents (REAPPLY), terminateWorkflow (terminate_current_first),
 *     flushEventsBuffer (FLUSH_BUFFER), resetor.ApplyResetEvent (APPLY_RESET_EVENT), and
 *     replicateWorkflowStarted's create-workflow handling after an APPLY_FRESH. */
int cdr_xdc_admit_host(const cdr_xdc_task* tasks, uint32_t n, const cdr_wf_caps* state_caps, const cdr_out* state,
                       const cdr_cluster_meta* cluster, cdr_xdc_decision* dec);
int cdr_xdc_admit_async(cdr_ctx* ctx, const cdr_xdc_task* tasks, uint32_t n, const cdr_wf_caps* state_caps,
                        const cdr_out* state, const cdr_cluster_meta* cluster, cdr_xdc_decision* dec, void* stream);

/* One round of 2DC replication tasks over n workflows, device-resident end to end, for task
 * w of workflow w:
 *   1. admit (k_xdc_admit, as cdr_xdc_admit_async) -> dec[w]; every record of reset_out /
 *      apply_out a later step will not write gets result.code CDR_NOT_RUN;
 *   2. CDR_XDC_RESET_APPLY: conflictResolverImpl.reset (conflictResolver.go:66-184) — entry w of
 *      `reset` (the workflow's events 1 .. reset_event_id, 2DC builder; its applyEvents calls
 *      are the pages the caller read, :94-133, the last one trimmed to the reset point)
 *      replayed on a fresh builder, the other entries masked.  A replay that does not end at
 *      next_event_id == reset_event_id + 1 fails the workflow with CDR_E_BAD_INPUT (the wrong
 *      prefix).  The loaded state's BranchToken replaces the Started event's (:141-142;
 *      StartTimestamp, :144-146, is not in the records).  With reset_out.transfer /
 *      timer_tasks / n_tasks set, the replay emits the stateBuilder's task lists, which the
 *      snapshot persists (stateBuilder.go:606-608, conflictResolver.go:150-162; the extra
 *      UpsertWorkflowSearchAttributesTask of :159-162 is the caller's): `reset` is then
 *      planned without wave slices and, where it carries class-sorted blocks, with task_rows.
 *      The reset state replaces state[w] (the reference has persisted it, :166-183) and
 *      dec[w] gains CDR_XDD_RESET_RAN;
 *   3. ApplyOtherEvents (H:655-694) against the reset state — dec[w] can turn from RESET_APPLY
 *      into DROP or RETRY — then ApplyReplicationTask (H:696-763) of every workflow still to
 *      apply: entry w of `apply` replayed onto state[w] as a loaded state (in_memory = 0: the
 *      reference re-loads after a reset, conflictResolver.go:183), APPLY_FRESH entries on a
 *      fresh builder (ApplyStartEvent H:436-449);
 *   4. state[w] := the applied state.  A failed replay leaves its error in state->result[w]
 *      (a failed reset also in dec[w], reasons CDR_XDR_E_RESET_*).  DROP, REAPPLY, RETRY,
 *      FLUSH_BUFFER and APPLY_RESET_EVENT leave the state as it was, or as the reset left it.
 *      A decision error (dec[w].code) leaves the state untouched: the reference returns the
 *      error without writing.
 * `reset` / `apply` are device-resident batches with entry w = workflow w and no continue-as-new
 * entries; `apply` is planned with cdr_plan_ndc_apply(state_caps), without fast or wave slices
 * (else CDR_API_EINVAL).  The apply's own task lists are not emitted.  No device allocation
 * once the context's workspace is warm, no host round trip; asynchronous on `stream`. */
typedef struct cdr_xdc_round {
  const cdr_xdc_task* tasks; /* [n] device */
  cdr_dev_batch reset;       /* entry w: events 1 .. reset point of workflow w */
  cdr_out reset_out;
  cdr_dev_batch apply;       /* entry w: the task's events */
  cdr_out apply_out;
  cdr_xdc_decision* dec;     /* [n] device, out */
} cdr_xdc_round;
int cdr_xdc_replicate_async(cdr_ctx* ctx, uint32_t n, const cdr_xdc_round* round, const cdr_wf_caps* state_caps,
                            const cdr_out* state, const cdr_cluster_meta* cluster, void* stream);

/* ------------------------------------------- loading persisted rows (load.hip) */
/* The inverse of the row encoders above for the SQL form: the five pending tables' row
 * blobs decoded on the device, straight into the loaded-state tables cdr_carry takes — what
 * mutableStateBuilder.Load (mutableStateBuilder.go:272-295) is fed by GetWorkflowExecution's
 * getActivityInfoMap, getTimerInfoMap, getChildExecutionInfoMap, getRequestCancelInfoMap and
 * getSignalInfoMap (common/persistence/sql/workflowStateMaps.go:139-206, 297-332, 423-471,
 * 561-596, 689-727), all through thriftRWDecode (blob.go:75-84).  Tables are numbered as in
 * the encoders: 0 activity, 1 timer, 2 child, 3 request-cancel, 4 signal.
 * cdr_load_rows decodes these five tables alone (the caller supplies the exec / repl / vh / rp /
 * sa records); cdr_load_state below decodes the execution row with them.
 * The Cassandra form of the five pending tables is cdr_load_cql_rows further below.
 * OUT OF SCOPE of all three: the Cassandra form of the execution row, BufferedEvents,
 * SignalRequestedIDs and the execution row's CompletionEvent.
 *
 * Blob format.  A blob is a bare thriftrw binary-protocol struct with no 0x59 preamble
 * (blob.go:61-84).  The wire rules are those of cdr/ingest.h: fields in any order, unknown
 * fields skipped, a field of an unexpected wire type skipped (an earlier occurrence stays), a
 * repeated field keeps its last occurrence, CDR_THRIFT_MAX_DEPTH bounds the containers open at
 * once inside a skipped value (a kept list<string> included).  Bytes after the struct's stop
 * byte are ignored (protocol.Binary.Decode reads one value).  DataEncoding validation
 * (validateProto) stays with the caller.
 *
 * Field mapping: the inverse of the row writers (oracle/thrift_binary.py restates them),
 * following the get*InfoMap functions.  An absent field is Go's GetX() zero.  Fields the
 * records do not keep are parsed over and dropped: the event blobs and their encodings,
 * StartedIdentity, the Retry*Last* fields, and the Details / DomainID columns (never passed).
 *   ActivityInfo (sqlblobs.thrift:136-168): 10 version, 12 scheduled_event_batch_id, 18
 *     scheduled_time, 20 started_id, 26 StartedTimeNanos, 28 activity_id, 30 request_id, 32 s2s,
 *     34 s2c, 36 stc, 38 hb, 40 CDR_AI_CANCEL_REQUESTED, 42 cancel_request_id, 44
 *     timer_task_status, 46 attempt, 48 task_list, 52 CDR_AI_HAS_RETRY, 54 / 56 / 58 initial /
 *     maximum interval / maximum attempts, 60 expiration_time, 62 backoff_coefficient (the bits),
 *     64 nonretriable; schedule_id is the key column.
 *     Times: CDR_AI_STARTED_TIME_SET is set iff field 26's value != CDR_ZERO_TIME_NANOS and
 *     started_time is that value, else 0 — an absent field 26 decodes as set with 0,
 *     time.Unix(0, 0) as in Go.  last_heartbeat_time is the act_heartbeat column if it is !=
 *     CDR_ZERO_TIME_NANOS, else 0; CDR_AI_HEARTBEAT_TIME_SET is set iff it is non-zero and
 *     STARTED is not set: a row cdr_sync_activity_async left with both bits comes back with
 *     STARTED alone, which sync.hip and the replay read the same way.
 *   TimerInfo (:201-206): 10 version, 12 started_id, 14 expiry_time, 16 task_id; timer_id is the
 *     handle of the key column's string.
 *   ChildExecutionInfo (:170-184): 10 version, 12 initiated_event_batch_id, 14 started_id, 20
 *     started_workflow_id, 22 StartedRunID, 28 CreateRequestID, 30 domain_name, 32 workflow_type,
 *     35 parent_close_policy; initiated_id is the key column.
 *   RequestCancelInfo (:195-199): 10 version, 11 initiated_event_batch_id, 12 CancelRequestID.
 *   SignalInfo (:186-193): 10 version, 11 initiated_event_batch_id, 12 SignalRequestID, 14
 *     signal_name, 16 input, 18 control (absent or empty: handle 0).
 * Request IDs (CancelRequestID, CreateRequestID, SignalRequestID) are kept as 128 bits: exactly
 * the canonical lowercase 36-character RFC 4122 text the encoders emit is accepted (hi then lo);
 * anything else, an absent field included, is CDR_LOAD_E_UUID — the record cannot hold it.
 * Child StartedRunID follows sqldb.UUID(b).String() (:455): an absent or empty binary is handle
 * 0; 16 bytes are rendered as canonical lowercase text into gen_bytes (36 bytes at 36 * the
 * child row's index) and interned, so the handle equals that of the same run ID seen in a
 * history; any other length is CDR_LOAD_E_UUID.  RetryNonRetryableErrors: a non-empty
 * list<string> is interned by the bytes of its list body (the encoders' and the ingest's
 * convention); an empty list or another element type is handle 0.
 *
 * Interning is the ingest's: seed i keeps handle i (seed 0 = ""), every other distinct string
 * gets n_seeds + its rank by cdr_str_hash, handle 0 is "".  Timer IDs from the key column are
 * interned like any other string, so equal timer IDs in two entries, or in a later ingest
 * seeded with this table, share a handle.  Only the last occurrence of a repeated field is
 * interned, and only the rows of entries in which every row decoded (a duplicate key does not
 * take an entry's strings out).  str_ref is cdr_ingest_out's with one more source: bit 63 =
 * offset into seed_bytes, bit 62 = offset into gen_bytes, else offset into `bytes`.
 *
 * Order.  Each entry's rows are written in ascending (signed) key order — the timer key is the
 * handle as an integer — whatever order they arrive in: the order every replay path writes and
 * cdr_carry / cdr_mutation_async require.  Two rows of one entry and table with the same key
 * are both CDR_LOAD_E_DUP_KEY (checked for entries in which every row decoded).  The ranking
 * compares every row of an entry with every other row of its table, so an entry may hold at
 * most CDR_LOAD_MAX_ENTRY_ROWS rows per table (the reference's pending tables hold tens): in a
 * larger one every row of that table is CDR_LOAD_E_ENTRY_ROWS and the entry fails, which bounds
 * the kernel's time whatever the caller passes.
 *
 * Failure.  As in Go, one bad row fails the whole GetWorkflowExecution: entry_status[w] is the
 * status of the entry's first failing row (lowest table, then lowest row), state.result[w].code
 * is CDR_E_LOAD_ROWS, its n_* are 0 and its table slices are unspecified; other entries are
 * unaffected.  Row statuses are the CDR_DEC_* codes of cdr/ingest.h plus the two below.
 *
 * Inputs (device pointers): `bytes` holds every blob and every timer-ID string; table t has
 * n_rows[t] rows, row r's blob at bytes[blob_off[t][r], blob_off[t][r+1]) and entry w's rows at
 * [entry_row0[t][w], entry_row0[t][w+1]); key[t] is schedule_id (t = 0) or initiated_id (t =
 * 2..4) per row, key[1] is not read: timer row r's ID is bytes[timer_id_off[r],
 * timer_id_off[r+1]); act_heartbeat[r] is the LastHeartbeatUpdatedTime column as UnixNano
 * (CDR_ZERO_TIME_NANOS: Go's zero time); seeds as in cdr_ingest_in.  Offsets past n_bytes are
 * clamped: no byte outside [bytes, bytes + n_bytes) is read.
 *
 * Outputs live in the context's grow-only workspace (slots of their own: a later
 * cdr_ingest_decode does not touch them) and stay valid until the next cdr_load_rows or
 * cdr_load_state on the context: `state` is a cdr_out view with the five pending tables ([n_rows[t]] records) and
 * result[n_entries] filled, exec / repl / vh / rp / sa and the task pointers NULL; caps[w]
 * (device) has *_off = entry_row0[t][w], *_cap = the entry's row count and everything else 0;
 * totals = the row counts.  All-empty tables and zero entries are valid.  No allocation once
 * the workspace is warm.  Synchronous on `stream` (the string count sizes the table).
 * CDR_API_EINVAL for null arguments, n_seeds == 0, or rows without entries. */
#define CDR_LOAD_E_UUID 16    /* a request ID that is not canonical UUID text / a run ID that is not 0 or 16 bytes */
#define CDR_LOAD_E_DUP_KEY 17 /* two rows of one entry and table share a key */
#define CDR_LOAD_E_ENTRY_ROWS 18 /* more than CDR_LOAD_MAX_ENTRY_ROWS rows of one entry in one table */
#define CDR_LOAD_MAX_ENTRY_ROWS 16384u
#define CDR_LOAD_TABLES 5
typedef struct cdr_rows_in { /* device pointers */
  const uint8_t* bytes;
  uint64_t n_bytes;
  const uint64_t* blob_off[CDR_LOAD_TABLES];   /* [n_rows[t] + 1] */
  const uint32_t* entry_row0[CDR_LOAD_TABLES]; /* [n_entries + 1] */
  const int64_t* key[CDR_LOAD_TABLES];         /* [n_rows[t]]; key[1] unused */
  const uint64_t* timer_id_off;                /* [n_rows[1] + 1] */
  const int64_t* act_heartbeat;                /* [n_rows[0]] */
  const uint8_t* seed_bytes;
  const uint64_t* seed_off;                    /* [n_seeds + 1]; seed 0 must be "" */
  uint32_t n_rows[CDR_LOAD_TABLES];
  uint32_t n_entries, n_seeds, _pad;
} cdr_rows_in;
typedef struct cdr_rows_out { /* device buffers owned by the context */
  cdr_out state;
  cdr_wf_caps* caps;     /* [n_entries] */
  cdr_totals totals;
  int32_t* row_status[CDR_LOAD_TABLES]; /* [n_rows[t]] */
  int32_t* entry_status; /* [n_entries] */
  uint64_t* str_ref;     /* [n_strings] */
  uint32_t* str_len;     /* [n_strings] */
  uint8_t* gen_bytes;    /* [n_gen_bytes] = 36 * n_rows[2] */
  uint64_t n_gen_bytes;
  uint32_t n_strings, n_bad_entries;
} cdr_rows_out;
int cdr_load_rows(cdr_ctx* ctx, const cdr_rows_in* in, cdr_rows_out* out, void* stream);
/* Whole stored states: the five pending tables as cdr_load_rows decodes them and, with them,
 * the execution row of every entry — GetWorkflowExecution (common/persistence/sql/
 * sqlExecutionManager.go:206-332: workflowExecutionInfoFromBlob and the row's columns) followed
 * by DeserializeExecutionInfo / DeserializeVersionHistories (common/persistence/
 * executionStore.go:108, 746-757), DeserializeResetPoints / DeserializeVersionHistories
 * (serializer.go:127, 168) and NewVersionHistoriesFromThrift (versionHistory.go:366).  The
 * result is a loaded state cdr_carry takes as it is: nothing of an earlier replay is needed.
 * `exec` == NULL is cdr_load_rows (which is this call with exec == NULL).
 *
 * One string-interning pass serves the pending rows and the execution rows, so the handles of
 * the exec record, the reset points, the search attributes and the pending rows live in one
 * handle space (seeds first, then hash rank).  The handles of the same pending rows therefore
 * DIFFER between cdr_load_rows and cdr_load_state with exec != NULL: more strings are ranked.
 *
 * Inputs (cdr_exec_rows_in, device pointers, one row per entry of rows->n_entries): the `data`
 * column at rows->bytes[blob_off[w], blob_off[w+1]), a bare thriftrw struct as the other
 * tables' (sqlblobs.thrift:73-134); the BINARY(16) key columns domain_id and run_id, 16 bytes
 * per entry; the workflow ID at rows->bytes[workflow_id_off[w], workflow_id_off[w+1]); the
 * next_event_id and last_write_version columns; cluster_seed[i] (i < n_clusters <=
 * CDR_MAX_CLUSTERS), the seed whose bytes are cluster i's name.  Offsets are clamped to
 * rows->n_bytes as in cdr_load_rows; the fixed-size columns are read at their entry's index.
 *
 * Field mapping: the inverse of the table-5 writer of cdr_encode_blobs_async (oracle/
 * thrift_binary.py exec_info_blob restates it).  Wire rules and absent fields as for the
 * pending tables.  cdr_exec_info:
 *   domain_id / run_id  the key columns as sqldb.UUID(b).String(): canonical lowercase text
 *     written into gen_bytes and interned (as a child row's StartedRunID), so they share
 *     handles with the same IDs in histories; workflow_id the key column's string.
 *   10 parent_domain_id, 14 parent_run_id  the same rendering of their 16 bytes; 12
 *     parent_workflow_id, 16 initiated_id.  All four are read only if field 10 is present
 *     (:305); else the handles are 0 and initiated_id is EmptyEventID (-23), what every replay
 *     leaves for a workflow without a parent (the SQL read leaves Go's zero there and the
 *     Cassandra read -23; nothing reads it, and a loaded state then equals a replayed one).  An
 *     empty or absent binary is handle 0; a length other than 0 or 16 is CDR_LOAD_E_UUID.
 *   18 completion_event_batch_id if present, else EmptyEventID (-23) (:270, 320).
 *   24 task_list, 26 workflow_type, 28 workflow_timeout, 30 decision_timeout_value, 34 state, 36
 *   close_status, 50 last_first_event_id, 52 last_processed_event, 58 decision_version, 60
 *   decision_schedule_id, 62 decision_started_id, 64 decision_timeout, 66 decision_attempt, 68
 *   decision_started_ts, 69 decision_scheduled_ts, 71 decision_original_scheduled_ts, 72
 *   create_request_id and 74 decision_request_id (plain strings, as the encoder writes them), 84 /
 *   86 / 88 / 90 initial_interval / maximum_interval / maximum_attempts / expiration_seconds, 92
 *   backoff_coefficient (the double's bits), 100 cron_schedule.
 *   next_event_id is the column.  last_event_task_id is 0: the reference's SQL read never
 *     assigns it (field 48 is written at sqlExecutionManagerUtil.go:1216 and read nowhere), and
 *     every applyEvents overwrites it.
 *   82 attempt and 106 signal_count narrowed as Go's int32(): the low 32 bits.
 *   94 expiration_time: CDR_XI_HAS_EXPIRATION iff the value != CDR_ZERO_TIME_NANOS, and the value
 *     is kept, else 0 (an absent field is 0: set, time.Unix(0, 0)).
 *   96 nonretriable: the list's body; an empty list or another element type is handle 0.
 *   flags: 70 CDR_XI_CANCEL_REQUESTED, 98 CDR_XI_HAS_RETRY (the booleans' values); field 118 /
 *     120 / 104 present (as a map / map / binary) CDR_XI_HAS_SEARCH_ATTR / _HAS_MEMO /
 *     _HAS_BRANCH; CDR_XI_HAS_RESET_POINTS iff the ResetPoints struct has its Points field (a
 *     list of structs); CDR_XI_VH_BRANCH iff the VersionHistory's token is non-empty;
 *     CDR_XI_STARTED always (an execution row exists only for a started execution).
 *   120 memo: the handle of the wire body of a Memo struct, 0D 00 0A + the map's body + 00,
 *     written into gen_bytes (the bytes are not contiguous in the input) and interned from there.
 *   118 search attributes: cdr_kv rows in wire order; a key that occurs twice keeps the
 *     position of its first occurrence and the value of its last; n_search_attr (and the
 *     record's search_attr_len) counts distinct keys, sa_cap is the wire count; every pair's
 *     strings are interned, a superseded value included.  A map whose key / value types are
 *     not both string has no rows.
 *   104 / VersionHistory.BranchToken: the 0x59 preamble (else CDR_LOAD_E_ENCODING, an empty field
 *     104 included; an empty VersionHistory token is "no token"), then HistoryBranch{10 TreeID ->
 *     branch_tree_id, 20 BranchID -> branch_id_hi / lo, canonical 36-character text only as the
 *     request IDs, else CDR_LOAD_E_UUID; 30 Ancestors must be empty}.
 *   115 / 116 AutoResetPoints and 122 / 124 VersionHistories: the encoding must be "thriftrw" and
 *     the blob's first byte 0x59, else CDR_LOAD_E_ENCODING; an absent or empty 115 is nil reset
 *     points (nothing checked).  ResetPointInfo's optional fields 10 .. 60 set the CDR_RP_HAS_*
 *     bits one for one; reset_points_len = n_reset_points.  The one VersionHistory's items go
 *     to state.vh in order.  A nested blob is walked level by level: each level's wire errors
 *     (CDR_DEC_*, bytes after its stop byte ignored) come before any finding inside it.
 *   builder[w] (a cdr_wf_desc.builder value): CDR_BUILDER_2DC iff field 44 is present (:286) —
 *     then repl.present = 1, start / current version 38 / 40, last_write_event_id 44,
 *     last_write_version the column, LastReplicationInfo from field 46 {10 version, 12
 *     last_event_id} by comparing each key's bytes with the clusters' names (a key that names
 *     none: CDR_LOAD_E_CLUSTER; a repeated key: the last) — CDR_BUILDER_NDC iff field 122 is
 *     present, else CDR_BUILDER_LOCAL; state.repl of other builders is zero.
 *   persist[w] (cdr_exec_persist): 38 start_version, 40 current_version, 54 start_time, 56
 *     last_updated_time, 108 history_size, 80 sticky_s2s_timeout narrowed through int32 (:263),
 *     32 execution_context (absent or empty: handle 0), 78 sticky_task_list, 110 / 112 / 114
 *     client_library_version / client_feature_version / client_impl.
 *   Parsed over and dropped: 20 / 22 CompletionEvent and its encoding, 76 CancelRequestID, 48.
 * Statuses of an execution row (exec_status[w]): CDR_DEC_*, CDR_LOAD_E_UUID and the three below,
 * the first finding in this order: the row's own wire errors; the parent IDs' lengths; fields
 * 44 and 122 together (SHAPE); an unknown cluster; field 104's token; the reset points'
 * encoding, preamble, wire errors, count over CDR_LOAD_MAX_RESET_POINTS (SHAPE); search
 * attributes over CDR_LOAD_MAX_SEARCH_ATTR (SHAPE); the version histories' encoding, preamble,
 * wire errors, CurrentVersionHistoryIndex != 0 or not exactly one VersionHistory (SHAPE), its
 * token, field 104 and a non-empty token together (SHAPE), items over CDR_LOAD_MAX_VH_ITEMS
 * (SHAPE).  The bounds exist for the reason CDR_LOAD_MAX_ENTRY_ROWS does: one lane walks an
 * entry's items, and search-attribute keys are compared pairwise.
 * A failing execution row fails its entry exactly as a failing pending row does (CDR_E_LOAD_ROWS,
 * zero counts, none of the entry's strings interned, other entries unaffected); in the entry's
 * first-failure order the execution row is table 5, after the pending tables.
 *
 * Outputs: everything cdr_rows_out has, with state.exec / repl [n_entries] and state.vh / rp /
 * sa filled, caps[w].vh_off / rp_off / sa_off and *_cap (the wire counts), result[w].n_vh /
 * n_reset_points / n_search_attr and totals to match — state, caps and totals are a cdr_carry's
 * as they are — and persist, builder, exec_status [n_entries].  gen_bytes holds the child rows'
 * run IDs first (36 * n_rows[2] bytes), then each entry's UUID texts (36 bytes each) and Memo
 * body (its length + 4, the entry's share rounded up to 4 bytes).  Same lifetime, workspace and
 * synchronisation as cdr_load_rows, and no host round trip more.  CDR_API_EINVAL also for a
 * null column of `exec` with n_entries != 0 and n_clusters > CDR_MAX_CLUSTERS. */
#define CDR_LOAD_E_ENCODING 19 /* a nested blob's encoding is not thriftrw / its 0x59 preamble is missing */
#define CDR_LOAD_E_SHAPE 20    /* a valid row the records cannot hold */
#define CDR_LOAD_E_CLUSTER 21  /* a LastReplicationInfo key names none of the clusters */
#define CDR_LOAD_MAX_VH_ITEMS 16384u
#define CDR_LOAD_MAX_RESET_POINTS 1024u
#define CDR_LOAD_MAX_SEARCH_ATTR 256u
typedef struct cdr_exec_rows_in { /* device pointers */
  const uint64_t* blob_off;        /* [n_entries + 1] into rows->bytes */
  const uint8_t* domain_id;        /* [16 * n_entries] */
  const uint8_t* run_id;           /* [16 * n_entries] */
  const uint64_t* workflow_id_off; /* [n_entries + 1] into rows->bytes */
  const int64_t* next_event_id;    /* [n_entries] */
  const int64_t* last_write_version; /* [n_entries] */
  uint32_t cluster_seed[CDR_MAX_CLUSTERS];
  uint32_t n_clusters, _pad;
} cdr_exec_rows_in;
typedef struct cdr_state_out { /* device buffers owned by the context */
  cdr_rows_out rows;
  cdr_exec_persist* persist; /* [n_entries] */
  uint32_t* builder;         /* [n_entries] */
  int32_t* exec_status;      /* [n_entries] */
} cdr_state_out;
int cdr_load_state(cdr_ctx* ctx, const cdr_rows_in* rows, const cdr_exec_rows_in* exec, cdr_state_out* out,
                   void* stream);

/* The five pending tables from the Cassandra persistence: the map columns activity_map,
 * timer_map, child_executions_map, request_cancel_map and signal_map as GetWorkflowExecution
 * selects them (common/persistence/cassandra/cassandraPersistence.go:1228-1320, the maps at
 * :1277-1316, templateGetWorkflowExecutionQuery :408), through createActivityInfo,
 * createTimerInfo, createChildExecutionInfo, createRequestCancelInfo and createSignalInfo
 * (cassandraPersistenceUtil.go:2055-2251).  Everything after the wire is cdr_load_rows: the
 * same records, interning (seeds first, then hash rank), ascending key order,
 * CDR_LOAD_E_DUP_KEY, per-entry failure rule (lowest table, then lowest row; CDR_E_LOAD_ROWS;
 * other entries unaffected), str_ref bits 62 / 63, output lifetime and workspace.  The
 * execution row (the execution / replication_state UDTs, version_histories) is not read
 * here: cdr_load_cql_state below reads it in the same call; with this one the caller supplies
 * exec / repl / vh / rp / sa as with cdr_load_rows.
 *
 * Inputs (device pointers).  One byte buffer bytes[n_bytes]; per table t (0 activity .. 4
 * signal) col_off[t] holds n_entries + 1 non-decreasing offsets, and entry w's column value
 * BODY is bytes[col_off[t][w], col_off[t][w+1]) — without the column's own 4-byte length.
 * Offsets are clamped to n_bytes; no byte outside [bytes, bytes + n_bytes) is read, whatever
 * the counts and lengths inside say.  An empty range is a null column: an empty map.  Seeds as
 * in cdr_rows_in.
 *
 * Wire.  A body is what Cassandra returns for map<K, frozen<udt>> (CQL native protocol v4): a
 * big-endian int32 count n, then n pairs of [bytes] values (int32 length, -1 = null, then the
 * bytes), the key and then the UDT value; the UDT value's body is its fields' [bytes] in the
 * DECLARATION order of schema/cassandra/cadence/schema.cql:149-228 (not the statement order
 * cdr_encode_cql_async emits: request_cancel_info and signal_info declare
 * initiated_event_batch_id before initiated_id).  gocql is not vendored in the reference: the
 * rules below are this contract's, restated in tests/cql_rows_ref.py.
 *   The device splits the maps (the caller does not know row counts): a pre-pass, one lane per
 *   (entry, table), reads the count and delimits the pairs; one scan per table gives
 *   entry_row0[t]; one host readback of the five row totals sizes the workspace.  A row is a
 *   delimited pair; row statuses exist for rows only.
 *   Map-level findings.  A column of 1..3 bytes is CDR_DEC_TRUNCATED; a negative count is
 *   CDR_DEC_BAD_SIZE; a count above CDR_LOAD_MAX_ENTRY_ROWS is CDR_LOAD_E_ENTRY_ROWS, decided from
 *   the count word alone before any pair is walked (the column then has no rows).  A key or UDT
 *   length below -1 is CDR_DEC_BAD_SIZE, a key or UDT that runs past its column (or whose
 *   length word does) is CDR_DEC_TRUNCATED.  A map-level finding belongs to the index of the
 *   first pair that could not be delimited (0 for the three count findings): pairs before it
 *   are rows with statuses of their own, nothing after it is a row, and the finding takes part
 *   in the entry's first-failure order as a row of that index would.  Bytes after the n-th
 *   pair are ignored.  The map key is delimited and otherwise not read (keys come from the
 *   UDT's own field, as in the reference).  A null UDT value is a UDT with no fields.
 *   Fields.  A UDT value with fewer fields than declared leaves the missing trailing fields
 *   null; bytes after the last declared field, inside the UDT's length, are ignored (a later
 *   schema appends fields).  A field's length word or value that runs past its UDT is
 *   CDR_DEC_TRUNCATED; a negative length other than -1 is CDR_DEC_BAD_SIZE.
 *   Fixed-size values (bigint 8, int 4, boolean 1, double 8, uuid 16, timestamp 8 bytes): a null
 *   or zero-length value is the type's zero (0, false, sixteen zero bytes, Go's zero time);
 *   any other length that is not the type's size is CDR_LOAD_E_CQL_SIZE.  A boolean is true iff
 *   its byte is non-zero.  Null or empty text / blob is "" (handle 0).
 *   Timestamps are milliseconds: nanoseconds = ms * 1,000,000, a product outside int64 is
 *   CDR_LOAD_E_SHAPE; Go's zero time is CDR_ZERO_TIME_NANOS.
 *   list<text> (non_retriable_errors): null or empty value, or count 0: handle 0.  A value of
 *   1..3 bytes, or an element that runs past the value, is CDR_DEC_TRUNCATED; a negative count,
 *   a null element or another negative element length is CDR_DEC_BAD_SIZE.  A non-empty list is
 *   interned under the project's convention, the thrift list body 0B + count + elements: the
 *   CQL value's bytes up to the end of its last element are that body without the type byte,
 *   so the body is written into gen_bytes and interned from there.
 *   A row's status is its first finding in field order (a wrong size, an overflowing timestamp
 *   and a wire error alike); the request-cancel ID's text is checked after the walk.
 *
 * Field mapping (every field not named is parsed over and dropped: the event blobs, details,
 * started_identity, last_failure_*, last_worker_identity, event_data_encoding — the set the
 * SQL loader drops):
 *   activity_info -> cdr_activity_info one for one: version, schedule_id (the key),
 *     scheduled_event_batch_id, scheduled_time, started_id, started_time, activity_id,
 *     request_id, schedule_to_start / schedule_to_close / start_to_close / heart_beat timeouts
 *     -> s2s / s2c / stc / hb, cancel_requested, cancel_request_id (the bigint),
 *     last_hb_updated_time, timer_task_status, attempt, task_list, has_retry_policy,
 *     init_interval, backoff_coefficient (the bits), max_interval, expiration_time,
 *     max_attempts, non_retriable_errors.  From the nanosecond values on, the time and flag
 *     rules are exactly cdr_load_rows's: CDR_AI_STARTED_TIME_SET iff started_time !=
 *     CDR_ZERO_TIME_NANOS (then the value is kept, else 0); last_heartbeat_time is
 *     last_hb_updated_time if != CDR_ZERO_TIME_NANOS, else 0, and CDR_AI_HEARTBEAT_TIME_SET iff
 *     it is non-zero and STARTED is not set.  scheduled_time and expiration_time keep their
 *     nanoseconds as they are (a null one is CDR_ZERO_TIME_NANOS).
 *   timer_info: version, timer_id (text: the interned handle, and the key), started_id,
 *     expiry_time (nanoseconds as they are), task_id.
 *   child_execution_info: version, initiated_id (the key), initiated_event_batch_id, started_id,
 *     started_workflow_id, started_run_id, create_request_id (uuid: create_request_hi = its
 *     first 8 bytes, lo = its last 8), domain_name, workflow_type_name, parent_close_policy.
 *     started_run_id is rendered as canonical lowercase text into gen_bytes and interned, as in
 *     the SQL loader; sixteen zero bytes and the writer's emptyRunID
 *     (30000000-0000-f000-f000-000000000000, cassandraPersistence.go:48, written at
 *     cassandraPersistenceUtil.go:1461) both give handle 0.  The reference keeps the sentinel's
 *     text there and nothing reads it before ReplicateChildWorkflowExecutionStartedEvent
 *     overwrites it; with 0 a loaded row equals a replayed one (the decision cdr_load_state
 *     documents for initiated_id).
 *   request_cancel_info: version, initiated_event_batch_id, initiated_id (the key),
 *     cancel_request_id (text: only the canonical 36-character form, else CDR_LOAD_E_UUID).
 *   signal_info: version, initiated_event_batch_id, initiated_id (the key), signal_request_id
 *     (uuid -> hi / lo), signal_name, input, control (null or empty: handle 0).
 *
 * Outputs: a cdr_rows_out exactly as cdr_load_rows fills it, over the discovered rows —
 * n_rows[t] and entry_row0[t] (device, [n_entries + 1]) say which; row_status[t] has n_rows[t]
 * words, rows in column order.  gen_bytes holds the child rows' run-ID texts first (36 bytes
 * at 36 * the child row's index), then the activity rows' list bodies.  Synchronous on
 * `stream`; one host round trip more than cdr_load_rows (the row totals); no allocation once
 * the workspace is warm.  CDR_API_EINVAL for null arguments, n_seeds == 0, a null col_off[t]
 * with n_entries != 0, null bytes with n_bytes != 0, and n_bytes >= 2^35 (row indices are 32
 * bits and a pair takes at least 8 bytes). */
#define CDR_LOAD_E_CQL_SIZE 22 /* a fixed-size CQL value whose length is neither 0 nor its type's size */
typedef struct cdr_cql_rows_in { /* device pointers */
  const uint8_t* bytes;
  uint64_t n_bytes;
  const uint64_t* col_off[CDR_LOAD_TABLES]; /* [n_entries + 1] */
  const uint8_t* seed_bytes;
  const uint64_t* seed_off;                 /* [n_seeds + 1]; seed 0 must be "" */
  uint32_t n_entries, n_seeds;
} cdr_cql_rows_in;
typedef struct cdr_cql_rows_out { /* device buffers owned by the context */
  cdr_rows_out rows;
  uint32_t* entry_row0[CDR_LOAD_TABLES]; /* [n_entries + 1], device */
  uint32_t n_rows[CDR_LOAD_TABLES];
  uint32_t _pad;
} cdr_cql_rows_out;
int cdr_load_cql_rows(cdr_ctx* ctx, const cdr_cql_rows_in* in, cdr_cql_rows_out* out, void* stream);

/* Whole stored states from the Cassandra persistence: cdr_load_cql_rows with the execution row
 * decoded too — the `execution` UDT, the `replication_state` UDT, `version_histories` and
 * `version_histories_encoding` as GetWorkflowExecution selects them (cassandraPersistence.go:
 * 1228-1332), through createWorkflowExecutionInfo (cassandraPersistenceUtil.go:1798-1935),
 * createReplicationState (:1937-1966) and createReplicationInfo (:2472).  It relates to
 * cdr_load_cql_rows as cdr_load_state relates to cdr_load_rows: exec == NULL is cdr_load_cql_rows
 * (that call is this one with exec == NULL), and with exec the outputs are exactly
 * cdr_load_state's — state.exec / repl / vh / rp / sa, caps, result counts, totals, persist,
 * builder, exec_status — over one string table and one handle space, the pending tables filled
 * as cdr_load_cql_rows fills them.  A failing execution row is table 5 in its entry's
 * first-failure order.  No host round trip more than cdr_load_cql_rows and cdr_load_state make
 * (the per-entry counts share their scan and readback); no allocation once the workspace is warm.
 *
 * Inputs (cdr_cql_exec_in, device pointers): four more columns in in->bytes, each [n_entries + 1]
 * non-decreasing offsets clamped to n_bytes, entry w's column BODY (without its own 4-byte
 * length) at [off[w], off[w+1]): the `execution` UDT value, the `replication_state` UDT value
 * (empty: null), the `version_histories` blob (empty: null) and the
 * `version_histories_encoding` text.  cluster_seed / n_clusters as in cdr_exec_rows_in.
 *
 * Wire.  The execution body holds the 58 fields of workflow_execution as [bytes] values in the
 * DECLARATION order of schema.cql:23-82 — not the statement order cdr_encode_cql_async emits
 * (last_first_event_id is the statement's 18th field and the declaration's 50th).  The rules are
 * cdr_load_cql_rows': missing trailing fields are null, bytes after the last declared field are
 * ignored, a null or empty fixed-size value is the type's zero and another wrong size is
 * CDR_LOAD_E_CQL_SIZE (event_store_version, which is dropped, included), length errors are
 * CDR_DEC_TRUNCATED / CDR_DEC_BAD_SIZE, timestamps are milliseconds x 1,000,000 (outside int64:
 * CDR_LOAD_E_SHAPE; null: CDR_ZERO_TIME_NANOS).  Field mapping onto cdr_exec_info /
 * cdr_exec_persist; where nothing is said the SQL loader's rule applies to the decoded value:
 *   domain_id, run_id, create_request_id (uuid; null: sixteen zero bytes): canonical lowercase
 *     text written into the entry's share of gen_bytes and interned from there (the SQL form
 *     takes create_request_id as a plain string).  workflow_id: the UDT's text (the read has no
 *     key columns).
 *   parent_domain_id / parent_run_id: sixteen zero bytes and the writer's sentinels
 *     emptyDomainID / emptyRunID (cassandraPersistence.go:46-48) give handle 0 (:1818, :1825);
 *     parent_workflow_id and initiated_id as they are — but the writer's emptyInitiatedID (-7,
 *     :69, stored for a workflow without a parent) under a parent domain that is none reads as
 *     EmptyEventID (-23), what every replay leaves there, so that a loaded state equals a
 *     replayed one (cdr_load_state's decision for the same field).
 *   completion_event_batch_id, next_event_id and last_event_task_id are the UDT's values.
 *     last_event_task_id is KEPT: the Cassandra read assigns it (:1856); cdr_load_state gives 0.
 *   start_time, last_updated_time (timestamps), history_size, sticky_task_list,
 *     sticky_schedule_to_start_timeout, client_library_version / client_feature_version /
 *     client_impl and execution_context go to persist; attempt, signal_count and the sticky
 *     timeout are CQL int (nothing is narrowed).
 *   expiration_time: CDR_XI_HAS_EXPIRATION iff != CDR_ZERO_TIME_NANOS, as in the SQL form.
 *   non_retriable_errors: the activity row's list<text> rule, the body 0B + value written into
 *     gen_bytes and interned from there.
 *   completion_event, its encoding, cancel_request_id, event_store_version: parsed over, dropped.
 *   branch_token: null or empty is no token and no CDR_XI_HAS_BRANCH (gocql cannot tell them
 *     apart; the SQL form makes an empty field 104 CDR_LOAD_E_ENCODING); else as field 104.
 *   auto_reset_points + encoding: a null or empty blob is nil reset points; else as 115 / 116.
 *   search_attributes, memo (map<text, blob>): a value of 1..3 bytes or an element that runs
 *     past the value is CDR_DEC_TRUNCATED, a negative count, a null element or another negative
 *     length CDR_DEC_BAD_SIZE — found in the walk, in field order, as the list's are; bytes
 *     after the last pair are ignored; a count over CDR_LOAD_MAX_SEARCH_ATTR is CDR_LOAD_E_SHAPE
 *     (search_attributes first).  CDR_XI_HAS_SEARCH_ATTR / _HAS_MEMO iff the map holds at least
 *     one pair: Cassandra stores an empty map as null, so unlike the SQL form (where the flag is
 *     the field's presence) an empty map's flag does not come back.  Search-attribute rows as
 *     in the SQL loader (repeated keys merged).  The Memo handle is the thrift struct body 0D 00
 *     0A 0B 0B + the CQL map body (count and pairs: a [bytes] element and a thrift binary are
 *     both a big-endian int32 length and the bytes, so the pairs are copied) + 00, written into
 *     gen_bytes, hashed while written and interned from there.
 *   replication_state body, null or empty: not 2DC.  Else CDR_BUILDER_2DC, repl.present = 1 and
 *     the fields in declaration order (schema.cql:91-97): current_version, start_version (both
 *     also persist's), last_write_version, last_write_event_id, last_replication_info — a map
 *     of text -> replication_info{version, last_event_id} with the maps' wire rules (a null
 *     value is a UDT without fields), its keys matched against the clusters' names: an unknown
 *     key is CDR_LOAD_E_CLUSTER, a repeated key keeps the last.
 *   version_histories body, non-empty: CDR_BUILDER_NDC; the encoding column must be "thriftrw",
 *     the blob's rules are fields 122 / 124's.  With a non-empty replication_state too:
 *     CDR_LOAD_E_SHAPE (:1270).
 * exec_status[w] is the first finding in this order: the execution UDT's, in field order; the
 * replication state's wire findings; both set (SHAPE); an unknown cluster; the branch token; the
 * reset points; the maps' counts; the version histories — inside the nested blobs level by
 * level as in cdr_load_state.
 * gen_bytes: the child rows' run IDs (36 * n_rows[2] bytes), then each entry's share — its UUID
 * texts (up to five), the list body and the Memo body, rounded up to 4 bytes — then the
 * activity rows' list bodies.  CDR_API_EINVAL as cdr_load_cql_rows, and for a null column of
 * `exec` with n_entries != 0 and n_clusters > CDR_MAX_CLUSTERS. */
typedef struct cdr_cql_exec_in { /* device pointers, offsets into cdr_cql_rows_in.bytes */
  const uint64_t* execution_off;         /* [n_entries + 1]  body of the `execution` UDT value */
  const uint64_t* replication_state_off; /* [n_entries + 1]  body of `replication_state` (empty: null) */
  const uint64_t* version_histories_off; /* [n_entries + 1]  the blob (empty: null) */
  const uint64_t* vh_encoding_off;       /* [n_entries + 1]  version_histories_encoding text */
  uint32_t cluster_seed[CDR_MAX_CLUSTERS];
  uint32_t n_clusters, _pad;
} cdr_cql_exec_in;
typedef struct cdr_cql_state_out { /* device buffers owned by the context */
  cdr_cql_rows_out rows;
  cdr_exec_persist* persist; /* [n_entries] */
  uint32_t* builder;         /* [n_entries] */
  int32_t* exec_status;      /* [n_entries] */
} cdr_cql_state_out;
int cdr_load_cql_state(cdr_ctx* ctx, const cdr_cql_rows_in* rows, const cdr_cql_exec_in* exec,
                       cdr_cql_state_out* out, void* stream);

/* Device milliseconds of the last cdr_load_rows / cdr_load_state / cdr_load_cql_rows /
 * cdr_load_cql_state on the context (the Cassandra forms' map split counts into ms[0]), between HIP events on its
 * stream: ms[0] the count pass (with the row -> entry map), ms[1] the intern pass and the
 * string ranking (with the two host round trips that size the table and the sort), ms[2] the
 * row ranking, ms[3] the fill pass and the entry epilogue.  The call is synchronous and holds
 * host round trips between its passes, so a caller's own events around it cannot tell the
 * passes apart; like cdr_last_kernel_ms for the replay, this is how the measurement
 * (tools/load_bench.py) and a caller's monitoring read them. */
int cdr_load_pass_ms(cdr_ctx* ctx, float* ms);

/* A decoded string table (cdr_rows_out's, or cdr_ingest_out's with gen_bytes == NULL) as the
 * contiguous cdr_strtab the encoders take and cdr_ingest_in takes as seeds.  Two calls, as the
 * encoders: with out_bytes == NULL it writes off[0..n] (device; string h = [off[h], off[h+1]));
 * the caller reads off[n], allocates out_bytes and calls again with the same `off` to copy the
 * bytes.  `bytes` is the blob buffer the table was decoded from.  Asynchronous. */
int cdr_strtab_gather_async(cdr_ctx* ctx, const uint64_t* str_ref, const uint32_t* str_len, uint32_t n,
                            const uint8_t* bytes, const uint8_t* seed_bytes, const uint8_t* gen_bytes,
                            uint64_t* off, uint8_t* out_bytes, void* stream);

/* ------------------------------------------------------------------ misc */

/* farmhash Fingerprint32(workflowID) % numShards (common/util.go:249-252) */
uint32_t cdr_fingerprint32(const char* s, size_t len);
int32_t cdr_workflow_id_to_shard(const char* workflow_id, size_t len, int32_t num_shards);

/* Kernel statistics of the last replay launch on ctx: average duration (ms) of
 * the replay kernel measured with HIP events on the launch stream. */
int cdr_last_kernel_ms(cdr_ctx* ctx, float* replay_ms, float* finalize_ms);

/* Per-launch timing ring: record the replay kernel of the next max_launches launches
 * with HIP events on their stream; read back durations (ms) after the fact. */
int cdr_timing_begin(cdr_ctx* ctx, uint32_t max_launches);
int cdr_timing_read(cdr_ctx* ctx, float* ms, uint32_t* n);

const char* cdr_version(void);

/* The measurement's bandwidth ceiling: copy `bytes` (a multiple of 64) from src to dst on
 * `stream` with 16-B vector loads and stores, one per lane, one-shot grid (the MI355X guide's
 * float4 copy, ~6.3 TB/s of read + write).  bench.py times it beside the replay kernel. */
int cdr_stream_copy_async(void* dst, const void* src, uint64_t bytes, void* stream);

/* Compile-time variant flags of this build (0 = the product build): bit 0 the PAR
 * profiling variant (CDR_PAR_PROF: writes per-wave times into result fields), bit 1 any
 * tuning knob off its default (prefetch depths, wave priority, kernel variants).  bench.py
 * refuses to report a line from a library that is not 0. */
uint32_t cdr_build_flags(void);

#ifdef __cplusplus
}
#endif
#endif /* CDR_CDR_H */
