// internal.h — helpers shared by the host-side translation units of libcdr.
#pragma once
#include <cstdint>
#include <vector>

#include "cdr/cdr.h"

namespace cdr_internal {

// loadActivityTimers (timerBuilder.go:249-312) for one pending row with a schedule ID: the
// first of the row's timers by (time, order) — between rows the tie key is the schedule ID,
// so the head of the sorted list is the smallest (t, schedule_id, order) over the rows.
// Order: ScheduleToClose 0 < StartToClose / ScheduleToStart 1 < Heartbeat 2.  Shared by
// refreshTasks (refresh.hip) and SyncActivity (sync.hip).
struct act_timer {
  int64_t t;
  int32_t order, type;  // type: cdr_timeout_type
};
// (Row: cdr_activity_info, or any record with its scheduled_time, expiration_time, started_id,
// started_time, last_heartbeat_time, s2s, s2c, stc, hb and flags)
template <class Row>
CDR_HD act_timer act_first_timer(const Row& a) {
  constexpr int64_t kSec = 1000000000LL;
  act_timer best;
  int64_t s2c = a.scheduled_time + (int64_t)a.s2c * kSec;
  if (a.expiration_time < s2c) s2c = a.expiration_time;
  best.t = s2c, best.order = 0, best.type = CDR_TIMEOUT_SCHEDULE_TO_CLOSE;
  auto cand = [&](int64_t t, int order, int type) {
    if (t < best.t) best.t = t, best.order = order, best.type = type;
  };
  if (a.started_id != CDR_EMPTY_EVENT_ID) {
    const bool set = (a.flags & CDR_AI_STARTED_TIME_SET) != 0;
    const int64_t st = set ? a.started_time : 0;
    cand(st + (int64_t)a.stc * kSec, 1, CDR_TIMEOUT_START_TO_CLOSE);
    if (a.hb > 0) {
      int64_t lhb = set ? a.last_heartbeat_time : 0;
      if (lhb < st) lhb = st;
      cand(lhb + (int64_t)a.hb * kSec, 2, CDR_TIMEOUT_HEARTBEAT);
    }
  } else {
    cand(a.scheduled_time + (int64_t)a.s2s * kSec, 1, CDR_TIMEOUT_SCHEDULE_TO_START);
  }
  return best;
}
// The earliest expiry over all of a row's activity timers, created or not: what the standby
// timer processor's expiry loop meets first (timerQueueStandbyProcessor.go:308-329 looks at the
// head of the sorted list only).  It is the first timer's time, whatever its task status.
template <class Row>
CDR_HD int64_t act_earliest_expiry(const Row& a) {
  return act_first_timer(a).t;
}
// time.Time.Unix() of a nanosecond instant: whole seconds, floored (also below zero), as
// IsTimerExpired compares them (timerBuilder.go:198-203)
CDR_HD int64_t unix_seconds(int64_t ns) {
  constexpr int64_t kSec = 1000000000LL;
  const int64_t q = ns / kSec;
  return (ns % kSec) < 0 ? q - 1 : q;
}
// the timer_task_status bit of a timeout type (getActivityTimerStatus, timerBuilder.go:36-47)
CDR_HD int32_t act_timer_bit(int32_t type) {
  return type == CDR_TIMEOUT_HEARTBEAT          ? CDR_TTS_HEARTBEAT
         : type == CDR_TIMEOUT_SCHEDULE_TO_START ? CDR_TTS_SCHEDULE_TO_START
         : type == CDR_TIMEOUT_SCHEDULE_TO_CLOSE ? CDR_TTS_SCHEDULE_TO_CLOSE
                                                 : CDR_TTS_START_TO_CLOSE;
}

// arena words of the attribute record of `type` (0 if the type has none)
uint32_t arena_words_for(uint32_t type);

// Output capacities of one history (cdr_plan_caps restricted to one workflow);
// offsets are left zero.
// The live rows a loaded state (cdr_carry) starts with: counts (activities, user timers,
// children, request-cancels, signals, reset points, search-attribute keys) and, when the
// state is host-visible, the rows themselves (their keys: a history event that removes a
// loaded row removes it from the simulation too; without rows, the loaded rows count as
// rows no event removes — an upper bound).
struct loaded_rows {
  uint32_t n[7];
  const cdr_timer_info* timer;
  const cdr_child_info* child;
  const cdr_cancel_info* cancel;
  const cdr_signal_info* signal;
  const cdr_reset_point* rp;
  const cdr_kv* sa;
};
// `loaded` (nullable): the entry replays onto that state; its rows count into the peak
// live sets and the register-table envelope.
// upper bounds of the transfer / timer tasks an entry's events append (host.cpp)
void task_caps(const cdr_event* ev, uint64_t n, uint32_t* xfer, uint32_t* ttask);
void caps_one(const cdr_event* ev, uint64_t n, uint32_t builder, cdr_wf_caps* c, const cdr_kv* kvs = nullptr,
              const cdr_reset_point* rps = nullptr, const loaded_rows* loaded = nullptr);

// Pack one workflow's events into lane `lane` of a slice whose first row is row0 and
// whose length is len (rows beyond n are padding).  `apos` is the workflow's arena
// word offset; kv/rp offsets inside the events are rebased by kv_base/rp_base.
void pack_chunked(const cdr_event* ev, uint64_t n_ev, uint64_t row0, uint32_t rows, uint64_t apos,
                  const cdr_slices* o);
void pack_lane(const cdr_event* ev, uint64_t n, uint64_t row0, uint32_t len, uint32_t lane, uint64_t apos,
               const cdr_slices* o);

// cdr_plan_slices_ex in one call, its outputs in vectors sized by the plan (the host-buffer
// pipeline and the device ingest plan once per batch instead of a size query and a fill)
struct plan_vecs {
  std::vector<int32_t> lane_wf;
  std::vector<uint32_t> slice_len;
  std::vector<uint64_t> slice_row0;
  std::vector<uint32_t> slice_flags;
};
int plan_slices_vec(const cdr_wf_desc* wfs, const cdr_wf_caps* caps, uint32_t n_wfs, uint32_t mode, plan_vecs& out,
                    uint32_t* n_slices, uint64_t* n_rows, uint32_t* n_wave);

}  // namespace cdr_internal
