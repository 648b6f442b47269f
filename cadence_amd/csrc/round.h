// round.h — device helpers shared by the replication rounds (ndc.hip, xdc.hip): a round keeps
// every workflow's state in one cdr_out and moves whole states between it and the outputs of
// the replays it runs.
#pragma once
#include <hip/hip_runtime.h>

#include "cdr/cdr.h"

namespace cdr_round {

__device__ inline void zero_result(cdr_wf_result& r, int32_t code) {
  r = cdr_wf_result{};
  r.code = code;
}

// the state records of entry w := the source's (rows at the destination's capacities)
__device__ inline void copy_state(const cdr_out& S, const cdr_wf_caps& sc, const cdr_out& D, const cdr_wf_caps& dc,
                                  uint32_t w) {
  const cdr_wf_result r = S.result[w];
  D.exec[w] = S.exec[w];
  D.repl[w] = S.repl[w];
  D.result[w] = r;
  if (r.code != CDR_OK) return;
  bool ok = true;
  auto cp = [&](auto* src, auto* dst, uint64_t so, uint64_t doff, uint32_t n, uint32_t cap) {
    if (n > cap) {
      ok = false;
      return;
    }
    for (uint32_t i = 0; i < n; i++) dst[doff + i] = src[so + i];
  };
  cp(S.act, D.act, sc.act_off, dc.act_off, r.n_activity, dc.act_cap);
  cp(S.timer, D.timer, sc.timer_off, dc.timer_off, r.n_timer, dc.timer_cap);
  cp(S.child, D.child, sc.child_off, dc.child_off, r.n_child, dc.child_cap);
  cp(S.cancel, D.cancel, sc.cancel_off, dc.cancel_off, r.n_cancel, dc.cancel_cap);
  cp(S.signal, D.signal, sc.signal_off, dc.signal_off, r.n_signal, dc.signal_cap);
  cp(S.vh, D.vh, sc.vh_off, dc.vh_off, r.n_vh, dc.vh_cap);
  cp(S.rp, D.rp, sc.rp_off, dc.rp_off, r.n_reset_points, dc.rp_cap);
  cp(S.sa, D.sa, sc.sa_off, dc.sa_off, r.n_search_attr, dc.sa_cap);
  if (!ok) D.result[w].code = CDR_E_BAD_INPUT;
}

// the carry descriptor of a round's apply replay, written on the stream (no host copy)
static __global__ void k_carry_desc(cdr_carry* dst, cdr_carry c) { *dst = c; }

}  // namespace cdr_round
