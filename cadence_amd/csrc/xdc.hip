// xdc.hip — 2DC replication rounds: historyReplicator.ApplyEvents for a batch of workflows.
//
// While EnableNDC is off, Handler.ReplicateEvents -> historyReplicator.ApplyEvents
// (service/history/historyReplicator.go:339-763) decides per task whether to drop it, buffer
// it (RetryTaskError), apply it, or reset the state to the last common checkpoint
// (conflictResolverImpl.reset, conflictResolver.go:66-184) and then apply it.  k_xdc_admit
// takes that decision (xdc_admit.h, the same function cdr_xdc_admit_host runs) for one task per
// workflow, one lane each: a few dozen comparisons on three records, so the kernel is bound by
// the latency of its loads, and what matters is that it runs next to the replays it routes.
// cdr_xdc_replicate_async chains it with the reset replay, the post-reset check, the apply
// replay and the adoption of the applied states, all on the caller's stream.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

#include "cdr/cdr.h"
#include "ctx.h"
#include "round.h"
#include "xdc_admit.h"

#define HIPCHK(x)                                                                                     \
  do {                                                                                                \
    hipError_t _e = (x);                                                                              \
    if (_e != hipSuccess) {                                                                           \
      fprintf(stderr, "cdr: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
      return CDR_API_EDEVICE;                                                                         \
    }                                                                                                 \
  } while (0)

namespace {

using cdr_round::copy_state;
using cdr_round::zero_result;

// a record whose size is a multiple of 16 bytes, 16-byte aligned: whole 16-byte vectors
template <class T>
__device__ __forceinline__ T ld_rec(const T* p) {
  static_assert(sizeof(T) % 16 == 0, "record of 16-byte vectors");
  uint4 q[sizeof(T) / 16];
  const uint4* s = reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (uint32_t i = 0; i < sizeof(T) / 16; i++) q[i] = s[i];
  T v;
  __builtin_memcpy(&v, q, sizeof(T));
  return v;
}
template <class T>
__device__ __forceinline__ void st_rec(T* p, const T& v) {
  static_assert(sizeof(T) % 16 == 0, "record of 16-byte vectors");
  uint4 q[sizeof(T) / 16];
  __builtin_memcpy(q, &v, sizeof(T));
  uint4* d = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (uint32_t i = 0; i < sizeof(T) / 16; i++) d[i] = q[i];
}

__global__ __launch_bounds__(256) void k_xdc_admit(const cdr_xdc_task* tasks, uint32_t n, const cdr_wf_result* result,
                                                   const cdr_exec_info* exec, const cdr_repl_state* repl,
                                                   cdr_cluster_meta cluster, cdr_xdc_decision* dec) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  const cdr_xdc_task t = ld_rec(tasks + w);
  // the decision reads two fields of the 256-byte exec record: only they are loaded
  cdr_exec_info x{};
  x.state = exec[w].state;
  x.next_event_id = exec[w].next_event_id;
  const cdr_wf_result r = result[w];
  const cdr_repl_state rs = repl[w];
  st_rec(dec + w, cdr_xdc::admit(t, r, x, rs, cluster));
}

// which workflows the reset replays; every output record a step will not write is marked
// CDR_NOT_RUN; the apply carry's src map (ApplyStartEvent: a fresh builder)
__global__ __launch_bounds__(256) void k_xdc_round_begin(uint32_t n, const cdr_xdc_decision* dec, cdr_out RS, cdr_out AP,
                                                         uint8_t* skip_rs, int32_t* src) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  const cdr_xdc_decision d = ld_rec(dec + w);
  const bool rs = d.code == CDR_OK && d.action == CDR_XDC_RESET_APPLY;
  skip_rs[w] = rs ? 0 : 1;
  if (!rs) zero_result(RS.result[w], CDR_NOT_RUN);
  zero_result(AP.result[w], CDR_NOT_RUN);
  src[w] = d.action == CDR_XDC_APPLY_FRESH ? -1 : (int32_t)w;
}

// after the reset replay: the prefix check, conflictResolver.go:141-146's overrides, the reset
// state replaces the workflow's (the reference has persisted it, :166-183), and
// ApplyOtherEvents' checks run against it; which workflows the apply replays
__global__ __launch_bounds__(256) void k_xdc_round_adopt_reset(uint32_t n, const cdr_xdc_task* tasks,
                                                               cdr_xdc_decision* dec, const cdr_wf_caps* sc, cdr_out S,
                                                               const cdr_wf_caps* rc, cdr_out RS, uint8_t* skip_ap) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  cdr_xdc_decision d = ld_rec(dec + w);
  skip_ap[w] = 1;
  if (d.code != CDR_OK) return;  // the reference returns the error without writing
  if (d.action == CDR_XDC_APPLY || d.action == CDR_XDC_APPLY_FRESH) {
    skip_ap[w] = 0;
    return;
  }
  if (d.action != CDR_XDC_RESET_APPLY) return;
  const int32_t rcode = RS.result[w].code;
  if (rcode != CDR_OK) {  // the reset replay failed
    S.result[w] = RS.result[w];
    st_rec(dec + w, cdr_xdc::fail(d, CDR_XDR_E_RESET_REPLAY, rcode));
    return;
  }
  if (RS.exec[w].next_event_id != d.reset_event_id + 1) {  // the caller packed the wrong prefix
    zero_result(S.result[w], CDR_E_BAD_INPUT);
    st_rec(dec + w, cdr_xdc::fail(d, CDR_XDR_E_RESET_PREFIX, CDR_E_BAD_INPUT));
    return;
  }
  // the loaded state's BranchToken replaces the one the Started event set (conflictResolver.go:141-142)
  const cdr_exec_info& old = S.exec[w];
  cdr_exec_info& x = RS.exec[w];
  x.branch_tree_id = old.branch_tree_id;
  x.branch_id_lo = old.branch_id_lo;
  x.branch_id_hi = old.branch_id_hi;
  x.flags = (x.flags & ~CDR_XI_HAS_BRANCH) | (old.flags & CDR_XI_HAS_BRANCH);
  copy_state(RS, rc[w], S, sc[w], w);
  const int32_t ccode = S.result[w].code;
  if (ccode != CDR_OK) {  // the state's capacities do not hold the reset state
    st_rec(dec + w, cdr_xdc::fail(d, CDR_XDR_E_RESET_REPLAY, ccode));
    return;
  }
  d.flags |= CDR_XDD_RESET_RAN;
  d = cdr_xdc::apply_other(d, ld_rec(tasks + w), x.state, x.next_event_id);
  if (d.code == CDR_OK && d.action == CDR_XDC_APPLY) skip_ap[w] = 0;
  st_rec(dec + w, d);
}

// after the apply: the applied state is the workflow's
__global__ __launch_bounds__(256) void k_xdc_round_adopt_applied(uint32_t n, const uint8_t* skip_ap,
                                                                 const cdr_wf_caps* sc, cdr_out S,
                                                                 const cdr_wf_caps* ac, cdr_out AP) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n || skip_ap[w]) return;
  if (AP.result[w].code != CDR_OK)
    S.result[w] = AP.result[w];
  else
    copy_state(AP, ac[w], S, sc[w], w);
}

bool cluster_ok(const cdr_cluster_meta* m) {
  return m && m->failover_version_increment > 0 && m->n_clusters > 0 && m->n_clusters <= CDR_MAX_CLUSTERS &&
         m->current_cluster >= 0 && m->current_cluster < m->n_clusters;
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" {

int cdr_xdc_admit_async(cdr_ctx* ctx, const cdr_xdc_task* tasks, uint32_t n, const cdr_wf_caps* state_caps,
                        const cdr_out* state, const cdr_cluster_meta* cluster, cdr_xdc_decision* dec, void* stream) {
  (void)state_caps;  // the decision reads no table rows
  if (!ctx || !cluster_ok(cluster)) return CDR_API_EINVAL;
  if (n && (!tasks || !dec || !state || !state->result || !state->exec || !state->repl || !aligned16(tasks) ||
            !aligned16(dec)))
    return CDR_API_EINVAL;
  HIPCHK(hipSetDevice(cdr_ctx_device(ctx)));
  if (n) hipLaunchKernelGGL(k_xdc_admit, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, tasks, n,
                            state->result, state->exec, state->repl, *cluster, dec);
  HIPCHK(hipGetLastError());
  return CDR_API_OK;
}

int cdr_xdc_replicate_async(cdr_ctx* ctx, uint32_t n, const cdr_xdc_round* R, const cdr_wf_caps* state_caps,
                            const cdr_out* state, const cdr_cluster_meta* cluster, void* stream) {
  if (!ctx || !R || !state || !cluster_ok(cluster) || (n && (!R->tasks || !R->dec || !state_caps)))
    return CDR_API_EINVAL;
  if (n > R->reset.n_wfs || n > R->apply.n_wfs || R->apply.carry || R->reset.carry) return CDR_API_EINVAL;
  // every apply entry replays onto a loaded state: only the general and the register-table
  // kernels take one (cdr_plan_ndc_apply never plans fast or wave slices)
  if (R->apply.n_fast_slices || R->apply.n_wave_slices) return CDR_API_EINVAL;
  // the reset's task lists: all three arrays, a plan without wave slices, and the task rows
  // known on the host where class-sorted blocks are replayed (else the replay reads them back)
  const bool rs_tasks = R->reset_out.transfer != nullptr;
  if (rs_tasks && (!R->reset_out.timer_tasks || !R->reset_out.n_tasks || R->reset.n_wave_slices ||
                   (R->reset.cls_slab && !R->reset.task_rows)))
    return CDR_API_EINVAL;
  if (n == 0) return CDR_API_OK;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipSetDevice(cdr_ctx_device(ctx)));
  uint8_t* skip_rs = (uint8_t*)cdr_ws_get(ctx, WS_XDC_SKIP_RS, n);
  uint8_t* skip_ap = (uint8_t*)cdr_ws_get(ctx, WS_XDC_SKIP_AP, n);
  int32_t* src = (int32_t*)cdr_ws_get(ctx, WS_XDC_SRC, n * 4ull);
  cdr_carry* carry_d = (cdr_carry*)cdr_ws_get(ctx, WS_XDC_CARRY, sizeof(cdr_carry));
  if (!skip_rs || !skip_ap || !src || !carry_d) return CDR_API_ENOMEM;
  const dim3 g((n + 255) / 256), b(256);
  // 1. ApplyEvents' admission (historyReplicator.go:377-653, and :655-707 for the loaded states)
  int rc = cdr_xdc_admit_async(ctx, R->tasks, n, state_caps, state, cluster, R->dec, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(k_xdc_round_begin, g, b, 0, st, n, R->dec, R->reset_out, R->apply_out, skip_rs, src);
  HIPCHK(hipGetLastError());
  // 2. conflictResolver.reset of the RESET_APPLY workflows: events 1 .. reset point on a fresh builder
  cdr_dev_batch rs = R->reset;
  rs.skip = skip_rs;
  cdr_out rso = R->reset_out;
  if (!rs_tasks) rso.transfer = rso.timer_tasks = nullptr, rso.n_tasks = nullptr;
  if ((rc = cdr_replay_sliced_async(ctx, &rs, &rso, stream))) return rc;
  hipLaunchKernelGGL(k_xdc_round_adopt_reset, g, b, 0, st, n, R->tasks, R->dec, state_caps, *state, R->reset.caps,
                     R->reset_out, skip_ap);
  HIPCHK(hipGetLastError());
  // 3. ApplyReplicationTask: carry-in replay onto the loaded (or reset, re-loaded: in_memory = 0) state
  cdr_carry cy{};
  cy.src = src;
  cy.caps = state_caps;
  cy.n_src = n;
  cy.state = *state;
  cy.state.transfer = cy.state.timer_tasks = nullptr;
  cy.state.n_tasks = nullptr;
  cy.state.last_decision = nullptr;
  hipLaunchKernelGGL(cdr_round::k_carry_desc, dim3(1), dim3(1), 0, st, carry_d, cy);
  HIPCHK(hipGetLastError());
  cdr_dev_batch ap = R->apply;
  ap.skip = skip_ap;
  ap.carry = carry_d;
  ap.cls_slab = nullptr;
  ap.cls_row0 = nullptr;
  ap.cls_rows = nullptr;
  cdr_out apo = R->apply_out;
  apo.transfer = apo.timer_tasks = nullptr;  // the round keeps states; an apply's task lists are a replay of its own
  apo.n_tasks = nullptr;
  if ((rc = cdr_replay_sliced_async(ctx, &ap, &apo, stream))) return rc;
  // 4. the applied states become the workflows'
  hipLaunchKernelGGL(k_xdc_round_adopt_applied, g, b, 0, st, n, skip_ap, state_caps, *state, R->apply.caps,
                     R->apply_out);
  HIPCHK(hipGetLastError());
  return CDR_API_OK;
}

}  // extern "C"
