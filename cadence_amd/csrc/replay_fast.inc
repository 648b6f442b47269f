// replay_fast.inc — fast-path replay kernel (included by replay.hip after k_replay).
//
// Slices whose every workflow is a sequential-activity history (CDR_CAP_FAST, set by
// the host planner, host.cpp caps_one): WorkflowExecutionStarted first and nowhere
// else, at most one pending activity at any time, no user timers, children, external
// requests, search-attribute upserts or continue-as-new, builder NDC or local.  That
// is the shape of the canary echo and activity-chain workloads (SURVEY §8(d) C1, C2).
// The semantics are k_replay's for those event types (stateBuilder.go:112-611 and the
// Replicate* methods it calls); the state machine is smaller — one activity working
// slot at a fixed LDS address, no 2DC replication state, and an error ends the lane at
// once because only 2DC needs the rest of a failed call — so it needs fewer registers
// and runs more waves per SIMD.
#ifndef CDR_WPE_FAST
#define CDR_WPE_FAST 4 /* 4 waves per SIMD: FD prefetch slots + state fit 128 VGPRs (121, no scratch), and sixteen one-wave workgroups' LDS fits the CU (FAST_LDS_BYTES) */
#endif
#ifndef CDR_FDEPTH
#define CDR_FDEPTH 1 /* rows in flight per wave (2: 138 VGPRs, which costs the fourth wave; forced to four it spills) */
#endif
constexpr uint32_t FD = CDR_FDEPTH;
#ifndef CDR_VHBF
#define CDR_VHBF 1 /* branch-free version-history prelude */
#endif
#ifndef CDR_VHQUICK
#define CDR_VHQUICK 1 /* skip the version-history prelude on steps the delta bits prove trivial */
#endif
#ifndef CDR_FAST_TBUF
#define CDR_FAST_TBUF 5 /* TASKS: the wave's LDS task-record pool holds CDR_FAST_TBUF x 64 records (0: stored at once; 8: 1.5 waves per SIMD, +7%; 12: +17%) */
#endif
#ifndef CDR_TQ_NT
#define CDR_TQ_NT 1 /* TASKS: the task records leave with nontemporal stores */
#endif
#ifndef CDR_WPE_FAST_TBUF
#define CDR_WPE_FAST_TBUF 2 /* the buffered TASKS instantiation (140 VGPRs, no spill; at 5 x 64 records its LDS, 17.5 KB, allows 9 workgroups per CU: 2 waves per SIMD) */
#endif
#ifndef CDR_FAST_SADDR
#define CDR_FAST_SADDR 1 /* the loop's row offsets from a scalar row index clamped to the slice */
#endif
#ifndef CDR_FAST_QROW
#define CDR_FAST_QROW 1 /* the quick-row step: a wave-uniform row of delta-implied ids / versions skips the prelude */
#endif
#ifndef CDR_FAST_DELTA
#define CDR_FAST_DELTA 1 /* skip event_id / version loads the delta bits make redundant */
#endif
#ifndef CDR_FAST_HINT
#define CDR_FAST_HINT 1 /* skip key / aux loads the operand hint fields make redundant (0: load as before) */
#endif
#ifndef CDR_FAST_UNI
#define CDR_FAST_UNI 1 /* the uniform loop: groups of rows whose type_flags are the same on every lane take their gates, hints and dispatch from a scalar (0: the per-lane loop alone) */
#endif
#ifndef CDR_FAST_UNI_SKIP
#define CDR_FAST_UNI_SKIP 1 /* the uniform loop issues only the loads its row needs, scalar branches round the others (0: every load, an unneeded one through a descriptor of no records) */
#endif
// which instantiation of the step a loop runs (a tag: the step is a generic lambda)
struct fast_uni_no { static constexpr bool value = false; };
struct fast_uni_yes { static constexpr bool value = true; };
#define FAST_LOAD_OPS load_ops<CDR_FAST_DELTA, CDR_NT_FAST, CDR_FAST_HINT != 0>
// copy a landed prefetch slot out through an opaque move, so that the register
// allocator cannot merge the copy with the slot (which would move the slot's refill
// into fresh registers and copy it back, waiting on the refill, at the loop latch)
__device__ __forceinline__ int64_t mov64(int64_t x) {
  int64_t y;
  asm volatile("v_mov_b64 %0, %1" : "=v"(y) : "v"(x));
  return y;
}
__device__ __forceinline__ uint32_t mov32(uint32_t x) {
  uint32_t y;
  asm volatile("v_mov_b32 %0, %1" : "=v"(y) : "v"(x));
  return y;
}
__device__ __forceinline__ uint32_t tf_take(uint32_t t) { return mov32(t); }
__device__ __forceinline__ Ev ev_take(const Ev& q) {
  Ev e;
  e.tf = mov32(q.tf);
  e.h = mov32(q.h);
  e.n = (int32_t)mov32((uint32_t)q.n);
  e.id = mov64(q.id);
  e.ver = mov64(q.ver);
  e.ts = mov64(q.ts);
  e.key = mov64(q.key);
  e.aux = mov64(q.aux);
  return e;
}
// write-only ExecutionInfo / decision fields of the fast loop, kept in LDS
// and the loop's read-mostly per-workflow words (output offsets, run id | reset point
// capacity, the first FAST_CK reset-point binary checksums two to a word) — a global
// load inside the loop would wait on every prefetch issued before it
#ifndef FAST_CK
#define FAST_CK 8u /* reset-point checksums cached in LDS (the rest are looked up in their rows) */
#endif
// (the entry's output offsets, run id and reset-point capacity are not among them: only the
// rare steps that store a VersionHistory item or a reset point need them, and those end in a
// drain anyway, so they read them from the entry's descriptors there)
enum : uint32_t {
  ZP_DST_TS = 0, ZP_DSC_TS, ZP_DORIG_TS, ZP_LAST_PROCESSED, ZP_COMPLETION_BATCH,
  ZP_CLOSE_VER, /* NDC: CurrentVersion as the closing event froze it */
  ZP_CK0, FAST_COLD = ZP_CK0 + FAST_CK / 2
};
// the activity working slot of the fast kernel: k_replay's planes (replay.hip AP_*) without the
// two timer candidates, which only k_replay's timer pick over several activities reads back
enum : uint32_t {
  FP_SID = 0, FP_TS2C, FP_META, FP_VER, FP_STARTED_ID, FP_STARTED_TIME, FP_CANCEL_ID, FP_ROWS, FP_STC_HB, FP_REQ,
  FAST_ACT_PLANES
};
template <class O>
__device__ __forceinline__ GAS cdr_vh_item* fast_out_vh(const O& o) { return gp(o.vh); }
template <class O>
__device__ __forceinline__ GAS cdr_reset_point* fast_out_rp(const O& o) { return gp(o.rp); }
// vmcnt(0) expcnt(7) lgkmcnt(15): after a rare in-loop global store, so that no store
// stays in flight beside the prefetch loads (the waitcnt pass would otherwise count
// vmcnt as out of order and wait for zero at every prefetch use)
#define VM_DRAIN() __builtin_amdgcn_s_waitcnt(0x0F70)
#define FAST_LDS_BYTES ((FAST_ACT_PLANES + FAST_COLD) * CDR_SLICE_WIDTH * sizeof(uint64_t))
// TASKS: the wave's task-record pool, three planes of CDR_FAST_TBUF x 64 words
#define FAST_TQ_WORDS (3u * CDR_FAST_TBUF * CDR_SLICE_WIDTH)
#define FAST_TBUF_BYTES (FAST_TQ_WORDS * sizeof(uint64_t))

// TASKS: the instantiation that also appends the stateBuilder's transfer / timer tasks
// (stateBuilder.go:613-804, as k_replay<LDS, true> does) to the entry's task slices — the
// opt-in path (cdr_out.transfer set); its records wait in an LDS buffer (CDR_FAST_TBUF) and
// go out when one could overflow, so that few steps drain the prefetch ring with stores
template <bool TASKS = false>
__global__ __launch_bounds__(CDR_SLICE_WIDTH) __attribute__((amdgpu_waves_per_eu(TASKS && CDR_FAST_TBUF > 0 ? CDR_WPE_FAST_TBUF : CDR_WPE_FAST, 8))) void
k_replay_fast(cdr_launch L) {
  (void)L;  // read through KA()
  const uint32_t s = blockIdx.x + KA()->s0;
  const uint32_t lane = threadIdx.x;
  if (s >= KA()->B.ev.n_slices || !KA()->fast) return;
  const uint32_t sflags = __builtin_amdgcn_readfirstlane(KA()->B.ev.slice_flags[s]);
  if (!(sflags & CDR_SLICE_FAST)) return;
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
#define B_ (KA()->B)
#define O_ (KA()->O)
#define D (gp(B_.wfs)[w])
#define CP (gp(B_.caps)[w])
#define X (gp(O_.exec) + w)
#define vh (gp(O_.vh) + CP.vh_off)
#define rp (gp(O_.rp) + CP.rp_off)
#define sa (gp(O_.sa) + CP.sa_off)
  const uint32_t len = (uint32_t)D.ev_len;
  const bool isVH = D.builder == CDR_BUILDER_NDC;
  const uint32_t EU = B_.empty_uuid;
  // the single activity working slot: plane p at cdr_lds[p * 64 + lane]; after it, the
  // ExecutionInfo fields the loop only writes (read back once at the end), in LDS
  // rather than VGPRs so that the loop fits 128 registers (4 waves per SIMD)
  const LdsSlots<FAST_ACT_PLANES> A{lane};
  const LdsSlots<FAST_COLD> Z{FAST_ACT_PLANES * CDR_SLICE_WIDTH + lane};
  Z.st(0, ZP_DST_TS, 0);
  Z.st(0, ZP_DSC_TS, 0);
  Z.st(0, ZP_DORIG_TS, 0);
  Z.st(0, ZP_LAST_PROCESSED, CDR_EMPTY_EVENT_ID);
  Z.st(0, ZP_COMPLETION_BATCH, 0);
#pragma unroll
  for (uint32_t i = 0; i < FAST_CK / 2; i++) Z.st(0, ZP_CK0 + i, 0);
  // reset point q's checksum (0 when it has none: never a lookup key) into the cache
  auto ck_put = [&](uint32_t q, uint32_t c) {
    if (q < FAST_CK) {
      const uint64_t v = (uint64_t)Z.ld(0, ZP_CK0 + q / 2);
      Z.st(0, ZP_CK0 + q / 2,
           (int64_t)((q & 1) ? ((v & 0xFFFFFFFFull) | ((uint64_t)c << 32)) : ((v & ~0xFFFFFFFFull) | c)));
    }
  };
  auto ck_has = [&](uint32_t c) {
    bool x = false;
#pragma unroll
    for (uint32_t i = 0; i < FAST_CK / 2; i++) {
      const uint64_t v = (uint64_t)Z.ld(0, ZP_CK0 + i);
      x |= (uint32_t)v == c || (uint32_t)(v >> 32) == c;
    }
    return x;
  };
  // the entry's slices inside the loop (rare steps, each ending in a drain): the offsets from
  // the entry's descriptor there, through an opaque pointer so that no load is hoisted out
#define CP_L (late(B_.caps)[w])
#define vh_l (fast_out_vh(O_) + CP_L.vh_off)
#define rp_l (fast_out_rp(O_) + CP_L.rp_off)

  uint32_t x_flags = 0, dreq = EU, n_vh = 0, n_rp = 0, cks_ok = 0, call_first_k = 0, err_k = 0;
  int32_t x_signals = 0, dto = 0;
  // ExecutionInfo.State | CloseStatus << 8 | the activity slot was ever used << 31 (the sign: one compare)
  uint32_t xs = (uint32_t)CDR_STATE_CREATED | ((uint32_t)CDR_CLOSE_NONE << 8);
#define XS_STATE (int32_t)(xs & 0xFFu)
#define XS_CLOSE (int32_t)((xs >> 8) & 0xFFu)
#define XS_ACT ((int32_t)xs < 0)
  int64_t x_next_event = CDR_FIRST_EVENT_ID;
  int64_t dv = CDR_EMPTY_VERSION, dsched = CDR_EMPTY_EVENT_ID, dstart = CDR_EMPTY_EVENT_ID, datt = 0;
  // NDC: the last VersionHistory item is (prev_id, prev_ver) — every accepted event leaves
  // the item's event id at its own id, and the item's version at its own version (a higher one
  // opens a new item, a lower one fails the entry) — and CurrentVersion is the version of the
  // event in hand until the workflow closes (stateBuilder.go:134-154), so none of the three
  // has a register of its own
  int64_t call_first_id = 0, prev_id = 0, prev_ver = 0;
  uint32_t ld = 0;  // lastDecision bookkeeping (ld_write)
  const bool want_ld = O_.last_decision != nullptr;
  // a failure ends the lane (done) and keeps its code and row; the failed event's id is read
  // back from that row after the loop (the event_id column holds every id, implied or not)
  int32_t err = len == 0 ? CDR_E_HISTORY_EMPTY : CDR_OK;
  bool done = len == 0;
  // ---- stateBuilder tasks (TASKS): counts, and ExecutionInfo.TaskList once Started set it
  uint32_t n_xt = 0, n_tt = 0, tlist = 0;
  // the task slices' capacities and the entry's DomainID in registers: a global load inside
  // the step loop would wait for every prefetch issued before it (one vmcnt)
  const uint32_t t_xcap = TASKS ? CP.xfer_cap : 0u, t_tcap = TASKS ? CP.ttask_cap : 0u;
  const uint32_t t_dom = TASKS ? D.domain_id : 0u;
  // with CDR_FAST_TBUF: a record goes to the wave's LDS record pool (CDR_FAST_TBUF x 64 records,
  // three planes: type | timeout type << 8 | timer << 12 | destination index << 16, event id,
  // visibility time or domain | task list << 32), appended at a wave-wide prefix of the lanes
  // that emit, and flushed at a step end once the next step could overflow it (<= 2 records per
  // lane per step), so that most steps store nothing to HBM and keep the prefetch ring (a store
  // drains it: one vmcnt for loads and stores).  A record carries its own destination, so the
  // pool's order is free; one pool for the wave, not a buffer per lane, flushes when the wave's
  // records fill it rather than when its busiest lane does.
  constexpr uint32_t TQ_BASE = (FAST_ACT_PLANES + FAST_COLD) * CDR_SLICE_WIDTH;
  constexpr uint32_t TQ_CAP = CDR_FAST_TBUF * CDR_SLICE_WIDTH;
  uint32_t n_pool = 0;  // wave-uniform
  const uint64_t t_xoff = TASKS ? (uint64_t)CP.xfer_off : 0u, t_toff = TASKS ? (uint64_t)CP.ttask_off : 0u;
  // (n_pool is wave-uniform only if every task_x / task_t call runs in wave-uniform control
  // flow: a call inside a lane-divergent branch would advance it on the active lanes alone)
  auto tq_put = [&](bool c, uint32_t kind, uint32_t type, int32_t tt, uint64_t dst, int64_t eid, int64_t v)
      __attribute__((always_inline)) {
    const uint64_t m = __builtin_amdgcn_ballot_w64(c);
    const uint32_t pos = n_pool + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (c) {
      cdr_lds[TQ_BASE + pos] = (int64_t)(type | ((uint32_t)tt << 8) | (kind << 12) | (dst << 16));
      cdr_lds[TQ_BASE + TQ_CAP + pos] = eid;
      cdr_lds[TQ_BASE + 2u * TQ_CAP + pos] = v;
    }
    n_pool = __builtin_amdgcn_readfirstlane(n_pool + (uint32_t)__builtin_popcountll(m));
  };
  auto task_x = [&](bool c, uint32_t type, int64_t eid, uint32_t dom, uint32_t tl) __attribute__((always_inline)) {
    if constexpr (TASKS) {
      // n_xt counts every record, stored or not: a count past the capacity fails the entry
      // after the loop (schema.h CDR_E_BAD_INPUT)
      const bool st = c && n_xt < t_xcap;
      if constexpr (CDR_FAST_TBUF > 0) {
        tq_put(st, 0u, type, 0, t_xoff + n_xt, eid, (int64_t)(dom | ((uint64_t)tl << 32)));
      } else if (st) {
        cdr_task t;
        t.type = type;
        t.timeout_type = 0;
        t.event_id = eid;
        t.visibility_ts = 0;
        t.attempt = 0;
        t.domain_id = dom;
        t.task_list = tl;
        t.target_workflow_id = t.target_run_id = t.flags = t._pad = 0;
        t.version = 0;
        gput(gp(O_.transfer) + t_xoff + n_xt, t);
      }
      n_xt += c ? 1u : 0u;
    }
  };
  auto task_t = [&](bool c, uint32_t type, int32_t tt, int64_t eid, int64_t vis) __attribute__((always_inline)) {
    if constexpr (TASKS) {
      const bool st = c && n_tt < t_tcap;
      if constexpr (CDR_FAST_TBUF > 0) {
        tq_put(st, 1u, type, tt, t_toff + n_tt, eid, vis);
      } else if (st) {
        cdr_task t;
        t.type = type;
        t.timeout_type = tt;
        t.event_id = eid;
        t.visibility_ts = vis;
        t.attempt = 0;
        t.domain_id = t.task_list = t.target_workflow_id = t.target_run_id = t.flags = t._pad = 0;
        t.version = 0;
        gput(gp(O_.timer_tasks) + t_toff + n_tt, t);
      }
      n_tt += c ? 1u : 0u;
    }
  };
  // The pool out to the task slices, written by the wave together: a lane per 16-B quarter of a
  // 64-B record, 16 records per store instruction, each record's 64 B in one instruction.
  // Written lane by lane, 64 lanes x 16 B to 64 task slices per instruction, every quarter
  // became a 64-B write request of its own (tools/calib.hip: partial-line stores cost a
  // request each).
  auto tq_flush = [&]() __attribute__((always_inline)) {
    const uint64_t em = __builtin_amdgcn_read_exec();
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(em >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)em, 0u));
    const uint32_t na = (uint32_t)__builtin_popcountll(em);  // >= 1: this lane is active
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): every lane's records before any lane reads them
    __builtin_amdgcn_wave_barrier();
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    GAS u64x2* const xb = (GAS u64x2*)gp(O_.transfer);
    GAS u64x2* const tb = (GAS u64x2*)gp(O_.timer_tasks);
    // item i = (record i / 4, quarter i % 4): quarter 0 type | timeout_type << 32, event_id;
    // 1 visibility_ts, attempt 0; 2 domain_id | task_list << 32, target workflow / run 0;
    // 3 flags, _pad, version 0
    for (uint32_t i = rank; i < 4u * n_pool; i += na) {
      const uint32_t r = i >> 2, q = i & 3u;
      const uint64_t w0 = (uint64_t)cdr_lds[TQ_BASE + r];
      const uint64_t x = (uint64_t)cdr_lds[TQ_BASE + (q == 0 ? TQ_CAP : 2u * TQ_CAP) + r];
      const bool tim = (w0 >> 12) & 1u;
      u64x2 v2;
      v2.x = q == 0 ? ((w0 & 0xFFu) | ((w0 >> 8) & 0xFu) << 32) : (q == (tim ? 1u : 2u) ? x : 0ull);
      v2.y = q == 0 ? x : 0ull;
#if CDR_TQ_NT
      __builtin_nontemporal_store(v2, (tim ? tb : xb) + (w0 >> 16) * 4u + q);
#else
      *((tim ? tb : xb) + (w0 >> 16) * 4u + q) = v2;
#endif
    }
    __builtin_amdgcn_s_waitcnt(0xC07F);  // the pool's reads before the next records land
    __builtin_amdgcn_wave_barrier();
    n_pool = 0;
  };

#define SEL(c, a, b) ((c) ? (a) : (b))
  // lastDecision: the record of a pending source event, before a clearing event
#define FLD_CAPTURE(mine_)                                                                                   \
  do {                                                                                                       \
    const bool c_ = (mine_) && ld_pending(ld);                                                               \
    if (__builtin_amdgcn_ballot_w64(c_ && want_ld)) {                                                        \
      if (c_)                                                                                                \
        ld_write(gp(O_.last_decision) + w, ld, dv, dsched, dstart, dreq, dto, datt, Z.ld(0, ZP_DSC_TS),      \
                 Z.ld(0, ZP_DST_TS), Z.ld(0, ZP_DORIG_TS));                                                  \
      VM_DRAIN();                                                                                            \
    }                                                                                                        \
    ld |= c_ ? LD_CAPTURED : 0u;                                                                             \
  } while (0)
#define PFAIL(cond, code)                \
  do {                                   \
    const bool f_ = (cond);              \
    err = SEL(f_, (int32_t)(code), err); \
    err_k = SEL(f_, k, err_k);           \
    done |= f_;                          \
  } while (0)

  // prefetch ring: slot j holds the operands of row j (mod FD) and the type_flags word
  // FD rows further on; each slot keeps its registers for the whole loop (the loop is
  // unrolled FD times and a step copies its slot out before refilling it), so no
  // register copy ever waits on a load still in flight
  Ev Q[FD];
  uint32_t T[FD];
#pragma unroll
  for (uint32_t j = 0; j < FD; j++) T[j] = load_tf<CDR_NT_FAST>(S, el8(j, len, lane));
#pragma unroll
  for (uint32_t j = 0; j < FD; j++) Q[j] = FAST_LOAD_OPS(S, el8(j, len, lane), T[j]);
#pragma unroll
  for (uint32_t j = 0; j < FD; j++) T[j] = load_tf<CDR_NT_FAST>(S, el8(j + FD, len, lane));
  const uint32_t srows = S.elems / CDR_SLICE_WIDTH;
  {  // ---- event 0: WorkflowExecutionStarted on every lane (CDR_CAP_FAST), peeled so
     // that its temporaries do not add to the replay loop's register pressure
    const uint32_t k = 0;
    Ev e = ev_take(Q[0]);
    if (CDR_FAST_HINT) ev_hint(e);  // (an entry's first event carries no delta bit: its id was loaded)
    const uint32_t tn = tf_take(T[0]);
    Q[0] = FAST_LOAD_OPS(S, el8(FD, len, lane), tn);
    T[0] = load_tf<CDR_NT_FAST>(S, el8(2 * FD, len, lane));
    call_first_id = SEL(!done, e.id, call_first_id);
    prev_id = SEL(done, prev_id, e.id);  // (done: an empty history)
    prev_ver = SEL(done, prev_ver, e.ver);
    if (isVH) {  // version prelude of the first event (stateBuilder.go:134-154)
      const int32_t code =
          (e.id < 0 || (e.ver < 0 && e.ver != CDR_EMPTY_VERSION)) ? CDR_P_VH_ITEM_INVALID
          : (CP.vh_cap == 0)                                         ? CDR_E_BAD_INPUT
                                                                     : CDR_OK;
      PFAIL(!done && code != CDR_OK, code);
      n_vh = done ? 0u : 1u;
    }
    {
      const bool mine = !done;  // mutableStateBuilder.go:1639-1716
      const GAS cdr_attr_wf_started* a =
          gp((const cdr_attr_wf_started*)(B_.ev.arena + (uint64_t)(mine ? e.aux : 0)));
      const uint32_t af = a->flags;
      const bool f1 = mine && (af & CDR_SF_HAS_PARENT_DOMAIN) && (af & CDR_SF_PARENT_DOMAIN_MISSING);
      PFAIL(f1, CDR_E_DOMAIN_NOT_FOUND);  // (Created -> Created is always an accepted transition)
      const bool ok = mine && !f1;
      uint32_t nrp = 0, xf = CDR_XI_STARTED | (isVH ? CDR_XI_VH_BRANCH : CDR_XI_HAS_BRANCH);
      // the Started half of ExecutionInfo (bytes 0-127, every field written: absent optional
      // fields as zero) assembled in registers and written by the wave together below
      uint32_t h0[32] = {};
      if (ok) {
        const bool retry = (af & CDR_SF_HAS_RETRY) != 0;
        uint64_t lo, hi;  // SetHistoryTree (:313-339)
        cdr_uuid(B_.uuid_seed, D.wf_key, CDR_UUID_BRANCH, e.id, &lo, &hi);
        auto q64 = [&](int i, uint64_t v) {
          h0[i] = (uint32_t)v;
          h0[i + 1] = (uint32_t)(v >> 32);
        };
        h0[0] = D.domain_id;
        h0[1] = D.workflow_id;
        h0[2] = D.run_id;
        h0[3] = D.request_id;  // create_request_id
        h0[4] = (af & CDR_SF_HAS_PARENT_DOMAIN) ? a->parent_domain_id : 0u;
        h0[5] = (af & CDR_SF_HAS_PARENT_EXEC) ? a->parent_workflow_id : 0u;
        h0[6] = (af & CDR_SF_HAS_PARENT_EXEC) ? a->parent_run_id : 0u;
        h0[7] = a->task_list;
        h0[8] = a->workflow_type;
        h0[9] = a->cron_schedule;
        h0[10] = (af & CDR_SF_HAS_MEMO) ? a->memo : 0u;
        h0[11] = retry ? a->nonretriable : 0u;
        h0[12] = D.run_id;  // branch_tree_id
        h0[13] = (uint32_t)a->exec_timeout_s;  // workflow_timeout
        h0[14] = (uint32_t)a->task_timeout_s;  // decision_timeout_value
        h0[15] = (uint32_t)a->attempt;
        q64(16, (uint64_t)((af & CDR_SF_HAS_PARENT_INITIATED) ? a->parent_initiated_id : CDR_EMPTY_EVENT_ID));
        h0[18] = (uint32_t)(retry ? a->retry_initial_s : 0);  // initial_interval
        h0[19] = (uint32_t)(retry ? a->retry_max_interval_s : 0);  // maximum_interval
        q64(20, __builtin_bit_cast(uint64_t, retry ? a->backoff_coefficient : 0.0));
        h0[22] = (uint32_t)(retry ? a->retry_max_attempts : 0);  // maximum_attempts
        h0[23] = (uint32_t)(retry ? a->retry_expiration_s : 0);  // expiration_seconds
        q64(24, (uint64_t)a->expiration_ts);
        q64(26, lo);  // branch_id_lo, branch_id_hi
        q64(28, hi);
        // 30, 31: _pad0, _pad1
        xf |= a->expiration_ts != 0 ? CDR_XI_HAS_EXPIRATION : 0u;
        xf |= retry ? CDR_XI_HAS_RETRY : 0u;
      }
      {  // two 64-B rounds through the activity slot's planes (free until the first schedule):
         // 4 lanes per 64-B segment, each segment one store instruction
        constexpr uint32_t RS = 65;
        static_assert(17u * RS * 4u <= FAST_ACT_PLANES * CDR_SLICE_WIDTH * sizeof(uint64_t), "the activity planes");
        uint32_t* const L32 = (uint32_t*)cdr_lds;
        const uint64_t em = __builtin_amdgcn_read_exec();
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(em >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)em, 0u));
        const uint32_t na = (uint32_t)__builtin_popcountll(em);
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (uint32_t half = 0; half < 2; half++) {
          __builtin_amdgcn_s_waitcnt(0xC07F);
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (uint32_t j = 0; j < 16; j++) L32[j * RS + rank] = h0[16 * half + j];
          L32[16 * RS + rank] = ok ? (uint32_t)w : 0xFFFFFFFFu;
          __builtin_amdgcn_s_waitcnt(0xC07F);
          __builtin_amdgcn_wave_barrier();
          for (uint32_t i = rank; i < 4u * na; i += na) {
            const uint32_t rr = i >> 2, c = i & 3u;
            const uint32_t wr = L32[16 * RS + rr];
            if (wr != 0xFFFFFFFFu) {
              u32x4 v;
              v.x = L32[(4 * c) * RS + rr];
              v.y = L32[(4 * c + 1) * RS + rr];
              v.z = L32[(4 * c + 2) * RS + rr];
              v.w = L32[(4 * c + 3) * RS + rr];
              *((GAS u32x4*)((GAS uint8_t*)(gp(O_.exec) + wr) + 64 * half) + c) = v;
            }
          }
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
      }
      bool f_cap = false;  // the event's reset points or search attributes do not fit their slices
      if (ok) {
        if (af & CDR_SF_HAS_RESET_POINTS) {  // rolloverAutoResetPointsWithExpiringTime (:3184-3205)
          xf |= CDR_XI_HAS_RESET_POINTS;
          const int64_t expiring = e.ts + (int64_t)D.retention_days * 24ll * 3600ll * NS_PER_S;
          const uint32_t crun = a->continued_run_id, off = a->reset_points_off, cnt = a->reset_points_len;
          const uint32_t cap = CP.rp_cap;
          f_cap |= cnt > cap;
          for (uint32_t q = 0; q < cnt && q < cap; q++) {
            cdr_reset_point p = gget(gp(B_.rps) + (off + q));
            const uint32_t run = (p.flags & CDR_RP_HAS_RUN_ID) ? p.run_id : 0u;
            if (run == crun) {
              p.flags |= CDR_RP_HAS_EXPIRING;
              p.expiring_time_nano = expiring;
            }
            ck_put(nrp, (p.flags & CDR_RP_HAS_CHECKSUM) ? p.binary_checksum : 0u);
            gput(rp + nrp++, p);
          }
        }
        xf |= (af & CDR_SF_HAS_MEMO) ? CDR_XI_HAS_MEMO : 0u;
        if (af & CDR_SF_HAS_SEARCH_ATTR) {
          const uint32_t off = a->search_attr_off, cnt = a->search_attr_len, cap = CP.sa_cap;
          f_cap |= cnt > cap;
          // each row at its rank among the input keys (ascending, equal keys in input order):
          // k_tables' order, so that a launch of fast slices alone needs no k_tables pass
          const uint32_t nsa = cnt < cap ? cnt : cap;  // (the epilogue counts them again: n_sa)
          for (uint32_t q = 0; q < nsa; q++) {
            const cdr_kv kv = gget(gp(B_.kvs) + (off + q));
            uint32_t rank = 0;
            for (uint32_t j = 0; j < nsa; j++) {
              const uint32_t kj = gp(B_.kvs)[off + j].key;
              rank += (kj < kv.key || (kj == kv.key && j < q)) ? 1u : 0u;
            }
            gput(sa + rank, kv);
          }
          xf |= nsa ? CDR_XI_HAS_SEARCH_ATTR : 0u;
        }
      }
      PFAIL(f_cap, CDR_E_BAD_INPUT);
      n_rp = SEL(ok, nrp, n_rp);
      x_flags = SEL(ok, xf, x_flags);
      if constexpr (TASKS) {  // scheduleWorkflowTimerTask (stateBuilder.go:706-735) + RecordWorkflowStartedTask (:614-616)
        tlist = ok ? a->task_list : 0u;
        const int64_t backoff = ok ? (int64_t)a->first_decision_backoff_s * NS_PER_S : 0;
        task_t(ok && backoff != 0, CDR_TT_WORKFLOW_BACKOFF, (af & CDR_SF_CRON_INITIATOR) ? 1 : 0, 0, e.ts + backoff);
        task_t(ok, CDR_TT_WORKFLOW_TIMEOUT, 0, 0, e.ts + (int64_t)(ok ? a->exec_timeout_s : 0) * NS_PER_S + backoff);
        task_x(ok, CDR_TT_RECORD_STARTED, 0, 0, 0);
      }
    }
    VM_DRAIN();  // the first Started's stores, before the loop's prefetch accounting
  }
  // one replay step over row k from its prefetch slot (rows past the slice are OOB
  // loads of zero on lanes already done: the tail group needs no guard)
  const uint32_t lane8 = lane * 8u;
#if CDR_FAST_SADDR
  // the loop's row offsets: the row index clamped to the slice (a scalar), plus the lane's
  // element offset — a lane past its own history reads the slice's padding cells (type
  // CDR_EV_PAD, no operand column needed) and is `done` anyway; no per-lane bounds select
  auto el8q = [&](uint32_t kk) {
    return __builtin_amdgcn_readfirstlane((kk < srows ? kk : srows - 1u) * CDR_ROW_BYTES) + lane8;
  };
#else
  auto el8q = [&](uint32_t kk) { return el8(kk, len, lane); };
#endif
#if CDR_FAST_UNI
  // the uniform step's loads: the row in soffset (a scalar, clamped to the slice like el8q:
  // the range check does not see soffset), the lane's element of the column in a loop-invariant
  // voffset; a column the row does not need is not loaded (its field is zero, as an out-of-range
  // load leaves it) or, with CDR_FAST_UNI_SKIP 0, read through a descriptor of no records (every
  // offset out of range: zero, no memory touched).  Skipping makes the compiler's vmcnt count
  // conservative (a group waits for every load issued before it) and still measured faster
#if !CDR_FAST_UNI_SKIP
  const rsrc_t r_none = __builtin_amdgcn_make_buffer_rsrc((void*)(KA()->B.ev.slab + row0 * CDR_ROW_BYTES), (short)0, 0, 0x00020000);
  auto rs = [&](bool need) { return need ? S.r : r_none; };
#endif
  auto rowq = [&](uint32_t kk) { return __builtin_amdgcn_readfirstlane((kk < srows ? kk : srows - 1u) * CDR_ROW_BYTES); };
#endif
  // the general row of a step: delta bits, call boundary and version prelude, per lane
  auto general_row = [&](Ev& e, const uint32_t k) __attribute__((always_inline)) {
    // event_id / version the packer marked as implied by the previous event (cdr.h)
    e.id = (e.tf & CDR_SEF_ID_NEXT) ? (int64_t)((uint64_t)prev_id + 1u) : e.id;
    e.ver = (e.tf & CDR_SEF_VER_SAME) ? prev_ver : e.ver;
    done |= k >= len;
    // call boundary (stateBuilder.go:603-604 of the previous call)
    const bool bf = !done && ((e.tf & CDR_SEF_BATCH_FIRST) || k == 0);
    x_next_event = SEL(bf && k > 0, prev_id + 1, x_next_event);
    call_first_id = SEL(bf, e.id, call_first_id);
    call_first_k = SEL(bf, k, call_first_k);
    ld = SEL(bf, 0u, ld);
    // version prelude (stateBuilder.go:134-154), against the last item (prev_id, prev_ver)
    if (isVH) {
#if CDR_VHQUICK
      // the common step: the packer's delta bits say event_id = the previous event's + 1 and
      // version = the previous event's, and the last item is the previous event's id / version
      // (prev_id, prev_ver: an accepted event always leaves it so) — so the item checks
      // pass and no item is added; only a non-negative id remains to check.  When every
      // replaying lane is such a step, the full prelude below is skipped.
      const bool quick = done || (n_vh != 0 && (e.tf & CDR_SEF_ID_NEXT) && (e.tf & CDR_SEF_VER_SAME) && e.id >= 0);
      if (__builtin_amdgcn_ballot_w64(!quick) != 0)
#endif
      {
#if CDR_VHBF
      // the same decision tree as selects over non-short-circuit conditions (no branches)
      const uint32_t vh_cap = CP_L.vh_cap;
      const bool has = n_vh != 0;
      const bool newitem = !has | (e.ver > prev_ver);
      const bool b_inv = (e.id < 0) | ((e.ver < 0) & (e.ver != CDR_EMPTY_VERSION));
      const bool b_ver = has & (e.ver < prev_ver);
      const bool b_id = has & (e.id <= prev_id);
      const bool b_cap = newitem & (n_vh >= vh_cap);
      int32_t code = b_cap ? (int32_t)CDR_E_BAD_INPUT : (int32_t)CDR_OK;
      code = b_id ? (int32_t)CDR_E_VH_LOWER_EVENT_ID : code;
      code = b_ver ? (int32_t)CDR_E_VH_LOWER_VERSION : code;
      code = b_inv ? (int32_t)CDR_P_VH_ITEM_INVALID : code;
#else
      const uint32_t vh_cap = CP_L.vh_cap;
      const bool newitem = n_vh == 0 || e.ver > prev_ver;
      const int32_t code = (e.id < 0 || (e.ver < 0 && e.ver != CDR_EMPTY_VERSION)) ? CDR_P_VH_ITEM_INVALID
                           : (n_vh != 0 && e.ver < prev_ver)                        ? CDR_E_VH_LOWER_VERSION
                           : (n_vh != 0 && e.id <= prev_id)                         ? CDR_E_VH_LOWER_EVENT_ID
                           : (newitem && n_vh >= vh_cap)                            ? CDR_E_BAD_INPUT
                                                                                    : CDR_OK;
#endif
      PFAIL(!done && code != CDR_OK, code);
      const bool add = !done && newitem;
      const bool put = add && n_vh != 0;
      if (put) gput(vh_l + (n_vh - 1), cdr_vh_item{prev_id, prev_ver});
      if (__builtin_amdgcn_ballot_w64(put)) VM_DRAIN();
      n_vh += add ? 1u : 0u;
      }
    }
    // (a lane the prelude failed keeps the previous event's: nothing reads a failed lane's)
    prev_id = SEL(done, prev_id, e.id);
    prev_ver = SEL(done, prev_ver, e.ver);
  };
  // UNI: the row's type_flags word and the one that gates the next loads are the same on every
  // executing lane (stf, stn: scalars), every lane is inside its history, and k + FD - 1 < srows
  auto step = [&](auto uni_, const uint32_t k, Ev& q, uint32_t& t, const uint32_t stf, const uint32_t stn)
      __attribute__((always_inline)) {
    constexpr bool UNI = decltype(uni_)::value;
    Ev e;
    if constexpr (UNI) {
#if CDR_FAST_UNI
      e.tf = stf;
      e.h = mov32(q.h);
      e.n = (int32_t)mov32((uint32_t)q.n);
      e.id = mov64(q.id);
      e.ver = mov64(q.ver);
      e.ts = mov64(q.ts);
      e.key = mov64(q.key);
      e.aux = mov64(q.aux);
      // the type_flags word first: the loop's uniformity test reads the newest one, and only
      // this step's operand loads are then younger than it
      // the lane's two element offsets through an opaque copy: the column offset added to a
      // loop-invariant register would be hoisted out of the loop, one register per column;
      // added here it folds into the load's immediate offset
      uint32_t l8 = lane8, l4 = S.l4;
      asm volatile("" : "+v"(l8), "+v"(l4));
      t = bld32<CDR_NT_FAST>(S.r, l4 + S.col(CDR_COL_TYPE_FLAGS), rowq(k + 2 * FD));
      const uint32_t so = rowq(k + FD);
      const uint32_t kbn = CDR_FAST_HINT ? (stn & CDR_SEF_KEY_BACK) : 0u, ain = CDR_FAST_HINT ? (stn & CDR_SEF_AUX_IMPL) : 0u;
      q.tf = stn;
#if CDR_FAST_UNI_SKIP
#define UNI_LD64(need, c_) ((need) ? bld64<CDR_NT_FAST>(S.r, l8 + S.col(c_), so) : (int64_t)0)
#define UNI_LD32(need, c_) ((need) ? bld32<CDR_NT_FAST>(S.r, l4 + S.col(c_), so) : 0u)
#else
#define UNI_LD64(need, c_) bld64<CDR_NT_FAST>(rs(need), l8 + S.col(c_), so)
#define UNI_LD32(need, c_) bld32<CDR_NT_FAST>(rs(need), l4 + S.col(c_), so)
#endif
      q.id = UNI_LD64(!(CDR_FAST_DELTA && (stn & CDR_SEF_ID_NEXT)), CDR_COL_EVENT_ID);
      q.ver = UNI_LD64(!(CDR_FAST_DELTA && (stn & CDR_SEF_VER_SAME)), CDR_COL_VERSION);
      q.ts = UNI_LD64((stn & CDR_SEF_NEED_TS) != 0, CDR_COL_TIMESTAMP);
      q.key = UNI_LD64((stn & CDR_SEF_NEED_KEY) && !kbn, CDR_COL_KEY);
      q.aux = UNI_LD64((stn & CDR_SEF_NEED_AUX) && !ain, CDR_COL_AUX);
      q.h = UNI_LD32((stn & CDR_SEF_NEED_H) != 0, CDR_COL_H);
      q.n = (int32_t)UNI_LD32((stn & CDR_SEF_NEED_N) != 0, CDR_COL_N);
#undef UNI_LD64
#undef UNI_LD32
#endif
    } else {
      e = ev_take(q);
      const uint32_t tn = tf_take(t);
      q = FAST_LOAD_OPS(S, el8q(k + FD), tn);
      t = load_tf<CDR_NT_FAST>(S, el8q(k + 2 * FD));
    }
    const uint32_t type = e.tf & 0xFFu;
    if constexpr (UNI) {
      // the quick row from the scalar word: the delta bits are a scalar test and the call
      // boundary a scalar branch; what remains per lane is `done` and the version-history part
      const int64_t qid = (int64_t)((uint64_t)prev_id + 1u);
      const bool qlane = !done && (!isVH || (n_vh != 0 && qid >= 0));
      if (CDR_FAST_QROW && (stf & CDR_SEF_ID_NEXT) && (stf & CDR_SEF_VER_SAME) && __builtin_amdgcn_ballot_w64(!qlane) == 0) {
        e.id = qid;
        e.ver = prev_ver;
        if (stf & CDR_SEF_BATCH_FIRST) {  // call boundary (stateBuilder.go:603-604)
          x_next_event = qid;
          call_first_id = qid;
          call_first_k = k;
          ld = 0u;
        }
        prev_id = qid;
      } else {
        general_row(e, k);
      }
      if (CDR_FAST_HINT) {  // ev_hint with scalar distances
        const uint32_t kb = (stf & CDR_SEF_KEY_BACK) >> CDR_SEF_KEY_BACK_SHIFT;
        const uint32_t ai = (stf & CDR_SEF_AUX_IMPL) >> CDR_SEF_AUX_IMPL_SHIFT;
        if (kb) e.key = (int64_t)((uint64_t)e.id - kb);
        if (ai && ai != CDR_SEF_AUX_ZERO) e.aux = (int64_t)((uint64_t)e.id - ai);
      }
    } else {
#if CDR_FAST_QROW
    // the quick row: every lane of the wave still replaying, inside its history, and its event
    // carrying both delta bits (id = previous + 1, version = previous).  Then the version
    // prelude's checks pass and add no item (the VHQUICK argument below), CurrentVersion is
    // already this version (the previous event set it while the state was Created / Running,
    // and the state only moves forward), and nothing can end a lane before the dispatch — so
    // the step's bookkeeping is the call boundary alone, with no `done` guard on any of it
    const int64_t qid = (int64_t)((uint64_t)prev_id + 1u);
    const bool qlane = !done && k < len && (e.tf & CDR_SEF_ID_NEXT) && (e.tf & CDR_SEF_VER_SAME) &&
                       (!isVH || (n_vh != 0 && qid >= 0));
    if (__builtin_amdgcn_ballot_w64(!qlane) == 0) {
      e.id = qid;
      e.ver = prev_ver;
      const bool bf = (e.tf & CDR_SEF_BATCH_FIRST) != 0;  // call boundary (stateBuilder.go:603-604)
      x_next_event = SEL(bf, qid, x_next_event);
      call_first_id = SEL(bf, qid, call_first_id);
      call_first_k = SEL(bf, k, call_first_k);
      ld = SEL(bf, 0u, ld);
      prev_id = qid;
    } else
#endif
    {
      general_row(e, k);
    }
    if (CDR_FAST_HINT) ev_hint(e);  // key / aux the packer marked as implied by the event's id (cdr.h)
    }
    // ---- dispatch: one pass per distinct event type among the lanes still replaying
    // (UNI: the one type is a scalar already, entered once; `mine` is every lane still replaying)
    for (uint64_t pend = UNI ? 1u : __builtin_amdgcn_ballot_w64(!done); pend;) {
      uint32_t ut;
      bool mine;
      if constexpr (UNI) {
        ut = type;
        mine = !done;
        pend = 0;
      } else {
        ut = __builtin_amdgcn_readlane(type, __builtin_ctzll(pend));
        asm volatile("" : "+s"(ut));
        mine = !done && type == ut;
        pend &= ~__builtin_amdgcn_ballot_w64(mine);
      }
      switch (ut) {
        case CDR_EV_DT_SCHEDULED:  // mutableStateDecisionTaskManager.go:143-167
          dv = SEL(mine, e.ver, dv);
          dsched = SEL(mine, e.id, dsched);
          dstart = SEL(mine, CDR_EMPTY_EVENT_ID, dstart);
          dreq = SEL(mine, EU, dreq);
          dto = SEL(mine, e.n, dto);
          datt = SEL(mine, e.aux, datt);
          ld = SEL(mine, ld_make(CDR_LD_SCHEDULED, k), ld);
          if (mine) {
            Z.st(0, ZP_DSC_TS, e.ts);
            Z.st(0, ZP_DST_TS, 0);
            Z.st(0, ZP_DORIG_TS, e.ts);
          }
          task_x(mine, CDR_TT_DECISION, e.id, t_dom, tlist);  // stateBuilder.go:196-197
          break;
        case CDR_EV_DT_STARTED: {  // :200-253
          const bool f = mine && e.key != dsched;
          PFAIL(f, CDR_E_DECISION_NOT_FOUND);
          const bool ok = mine && !f;
          static_assert(CDR_STATE_CREATED == 0 && CDR_STATE_RUNNING == 1, "Created -> Running sets bit 0");
          xs |= (ok && XS_STATE == CDR_STATE_CREATED) ? 1u : 0u;
          dv = SEL(ok, e.ver, dv);
          dstart = SEL(ok, e.id, dstart);
          dreq = SEL(ok, e.h, dreq);
          datt = SEL(ok, (int64_t)0, datt);
          ld = SEL(ok, ld_make(CDR_LD_STARTED, k), ld);
          if (ok) Z.st(0, ZP_DST_TS, e.ts);
          task_t(ok, CDR_TT_DECISION_TIMEOUT, CDR_TIMEOUT_START_TO_CLOSE, e.key, e.ts + (int64_t)dto * NS_PER_S);  // :209-212
          break;
        }
        case CDR_EV_DT_COMPLETED: {  // :255-262,659-674,789-800
          FLD_CAPTURE(mine);
          dv = SEL(mine, CDR_EMPTY_VERSION, dv);
          dsched = SEL(mine, CDR_EMPTY_EVENT_ID, dsched);
          dstart = SEL(mine, CDR_EMPTY_EVENT_ID, dstart);
          dreq = SEL(mine, EU, dreq);
          dto = SEL(mine, 0, dto);
          datt = SEL(mine, (int64_t)0, datt);
          if (mine) {  // OriginalScheduledTimestamp kept
            Z.st(0, ZP_DST_TS, 0);
            Z.st(0, ZP_DSC_TS, 0);
            Z.st(0, ZP_LAST_PROCESSED, e.aux);
          }
          const uint32_t cks = e.h;
          const bool chk = mine && cks != 0 && cks != cks_ok;
          if (__builtin_amdgcn_ballot_w64(chk)) {  // addBinaryCheckSumIfNotExists (mutableStateBuilder.go:1798-1842)
            bool exists = chk && ck_has(cks);
            const bool deep = chk && !exists && n_rp > FAST_CK;
            if (__builtin_amdgcn_ballot_w64(deep)) {  // past the cache: the rows themselves
              for (uint32_t q = FAST_CK; deep && q < n_rp; q++) {
                const cdr_reset_point p = gget(rp_l + q);
                exists |= ((p.flags & CDR_RP_HAS_CHECKSUM) ? p.binary_checksum : 0u) == cks;
              }
            }
            const bool app = chk && !exists;
            const bool f = app && n_rp >= (app ? CP_L.rp_cap : 0u);
            PFAIL(f, CDR_E_BAD_INPUT);
            const bool put = app && !f;
            if (put) {  // no children / cancels / signals on the fast path: always resettable
              cdr_reset_point p;
              p.binary_checksum = cks;
              p.run_id = late(B_.wfs)[w].run_id;
              p.first_decision_completed_id = e.id;
              p.created_time_nano = B_.now_ns;
              p.expiring_time_nano = 0;
              p.flags = CDR_RP_HAS_CHECKSUM | CDR_RP_HAS_RUN_ID | CDR_RP_HAS_FIRST_DC_ID | CDR_RP_HAS_CREATED |
                        CDR_RP_HAS_RESETTABLE | CDR_RP_RESETTABLE;
              p._pad = 0;
              gput(rp_l + n_rp, p);
              ck_put(n_rp, cks);
            }
            if (__builtin_amdgcn_ballot_w64(put)) VM_DRAIN();
            n_rp += put ? 1u : 0u;
            x_flags |= put ? CDR_XI_HAS_RESET_POINTS : 0u;
            cks_ok = SEL(chk && !f, cks, cks_ok);
          }
          break;
        }
        case CDR_EV_DT_TIMED_OUT:  // FailDecision :635-656 + transient decision :169-198
        case CDR_EV_DT_FAILED: {
          FLD_CAPTURE(mine);
          const bool inc = ut == CDR_EV_DT_FAILED || e.n != CDR_TIMEOUT_SCHEDULE_TO_START;
          const int64_t now = B_.now_ns;
          const int64_t na = inc ? datt + 1 : 0;
          const bool tr = na != 0;
          // CurrentVersion: this event's, or what the closing event left (a closed workflow's stays)
          const int64_t curv = XS_STATE == CDR_STATE_COMPLETED ? Z.ld(0, ZP_CLOSE_VER) : e.ver;
          dv = SEL(mine, tr ? (isVH ? curv : CDR_EMPTY_VERSION) : CDR_EMPTY_VERSION, dv);
          dsched = SEL(mine, tr ? x_next_event : CDR_EMPTY_EVENT_ID, dsched);
          dstart = SEL(mine, CDR_EMPTY_EVENT_ID, dstart);
          dreq = SEL(mine, EU, dreq);
          int32_t dtv = 0;  // ExecutionInfo.DecisionTimeoutValue: the Started event's, from its record
          if (mine && tr)
            dtv = ((const GAS cdr_attr_wf_started*)(late(B_.ev.arena) + (uint64_t)bld64(S.r, lane8, S.col(CDR_COL_AUX))))->task_timeout_s;
          dto = SEL(mine, dtv, dto);
          if (mine) {
            Z.st(0, ZP_DST_TS, 0);
            Z.st(0, ZP_DORIG_TS, 0);
            Z.st(0, ZP_DSC_TS, (tr || inc) ? now : (int64_t)0);
          }
          task_x(mine && tr, CDR_TT_DECISION, x_next_event, t_dom, tlist);  // :235,253
          datt = SEL(mine, na, datt);
          ld = SEL(mine && tr, ld_make(CDR_LD_TRANSIENT, k), ld);
          break;
        }
        case CDR_EV_AT_SCHEDULED: {  // mutableStateBuilder.go:1982-2028
          // CDR_CAP_FAST: the slot is free (one pending activity at most); a second
          // pending one is k_replay's capacity error too (slice_act_slots == 1)
          const bool f = mine && XS_ACT && A.ld(0, FP_SID) != DEAD_KEY;
          PFAIL(f, CDR_E_BAD_INPUT);
          const bool ok = mine && !f;
          xs |= ok ? 0x80000000u : 0u;
          if (ok) {
            const uint32_t aid = (uint32_t)e.key;
            const int32_t s2c = (int32_t)e.h, s2s = e.n;
            const int64_t t_s2c = e.ts + (int64_t)s2c * NS_PER_S, t_s2s = e.ts + (int64_t)s2s * NS_PER_S;
            // the activity timer pick over this one activity (timerBuilder.go:211-312):
            // ScheduleToClose unless ScheduleToStart is strictly earlier
            const uint32_t bit = t_s2s < t_s2c ? CDR_TTS_SCHEDULE_TO_START : CDR_TTS_SCHEDULE_TO_CLOSE;
            A.st(0, FP_SID, e.id);
            A.st(0, FP_TS2C, t_s2c);
            A.st(0, FP_META, (int64_t)(aid | META_FLAG(AF_AIDMAP) | ((uint64_t)bit << META_TTS_SHIFT)));
            A.st(0, FP_VER, e.ver);
            A.st(0, FP_STARTED_ID, CDR_EMPTY_EVENT_ID);
            A.st(0, FP_STARTED_TIME, 0);
            A.st(0, FP_CANCEL_ID, CDR_EMPTY_EVENT_ID);
            A.st(0, FP_ROWS, (int64_t)(k | ((uint64_t)call_first_k << 32)));
            A.st(0, FP_STC_HB, (int64_t)(((uint64_t)e.key >> 32) | ((uint64_t)e.aux & 0xFFFFFFFF00000000ull)));
            A.st(0, FP_REQ, 0);
          }
          if constexpr (TASKS) {  // ActivityTask (:265-266), then the pick's ActivityTimeoutTask (:724-729)
            task_x(ok, CDR_TT_ACTIVITY, e.id, t_dom, tlist);
            const int64_t t_s2c = e.ts + (int64_t)(int32_t)e.h * NS_PER_S, t_s2s = e.ts + (int64_t)e.n * NS_PER_S;
            const bool s2s = t_s2s < t_s2c;
            task_t(ok, CDR_TT_ACTIVITY_TIMEOUT, s2s ? CDR_TIMEOUT_SCHEDULE_TO_START : CDR_TIMEOUT_SCHEDULE_TO_CLOSE, e.id,
                   s2s ? t_s2s : t_s2c);
          }
          break;
        }
        case CDR_EV_AT_STARTED: {  // :2083-2098
          const bool f = mine && !(XS_ACT && A.ld(0, FP_SID) == e.key);
          PFAIL(f, CDR_P_ACTIVITY_STARTED_NIL);  // nil deref in Go
          bool t_made = false;  // TASKS: the pick's timer, emitted below in uniform control flow
          int32_t t_tt = 0;
          int64_t t_vis = 0;
          if (mine && !f) {
            const uint64_t th = (uint64_t)A.ld(0, FP_STC_HB);
            const int32_t stc = (int32_t)(uint32_t)th, hb = (int32_t)(uint32_t)(th >> 32);
            const uint64_t m = (uint64_t)A.ld(0, FP_META) | META_FLAG(AF_STARTED);
            const int64_t t0 = A.ld(0, FP_TS2C);
            const int64_t ta = e.ts + (int64_t)stc * NS_PER_S;
            const int64_t tb = hb > 0 ? e.ts + (int64_t)hb * NS_PER_S : T_NONE;
            // pick: ScheduleToClose, then StartToClose, then Heartbeat on ties
            const int64_t t1 = ta < t0 ? ta : t0;
            const uint32_t bit =
                tb < t1 ? CDR_TTS_HEARTBEAT : (ta < t0 ? CDR_TTS_START_TO_CLOSE : CDR_TTS_SCHEDULE_TO_CLOSE);
            A.st(0, FP_VER, e.ver);
            A.st(0, FP_STARTED_ID, e.id);
            A.st(0, FP_REQ, (int64_t)e.h);
            A.st(0, FP_STARTED_TIME, e.ts);  // LastHeartBeatUpdatedTime = StartedTime
            A.st(0, FP_META, (int64_t)(m | ((uint64_t)bit << META_TTS_SHIFT)));
            if constexpr (TASKS) {  // the pick created a timer unless its status bit was set (timerBuilder.go:211-230)
              t_made = !(m & ((uint64_t)bit << META_TTS_SHIFT));
              t_tt = (int32_t)__builtin_ctz(bit);
              t_vis = tb < t1 ? tb : t1;
            }
          }
          task_t(t_made, CDR_TT_ACTIVITY_TIMEOUT, t_tt, e.key, t_vis);
          break;
        }
        case CDR_EV_AT_COMPLETED:  // DeleteActivity :1247-1269
        case CDR_EV_AT_FAILED:
        case CDR_EV_AT_TIMED_OUT:
        case CDR_EV_AT_CANCELED: {
          const bool live = XS_ACT && A.ld(0, FP_SID) == e.key;
          PFAIL(mine && !live, CDR_E_ACTIVITY_NOT_FOUND);
          // the only pending activity holds its own byActivityID entry (another
          // Scheduled with the same ID would need two pending)
          const bool ok = mine && live;
          PFAIL(ok && !((uint64_t)A.ld(0, FP_META) & META_FLAG(AF_AIDMAP)), CDR_E_ACTIVITY_ID_NOT_FOUND);
          if (ok) A.st(0, FP_SID, DEAD_KEY);
          break;
        }
        case CDR_EV_AT_CANCEL_REQUESTED: {  // :2264-2285
          const uint64_t m = (uint64_t)A.ld(0, FP_META);
          const bool hit = XS_ACT && A.ld(0, FP_SID) != DEAD_KEY && (uint32_t)m == (uint32_t)e.key &&
                           (m & META_FLAG(AF_AIDMAP));
          PFAIL(mine && !hit, CDR_E_MISSING_ACTIVITY_INFO);
          if (mine && hit) {
            A.st(0, FP_VER, e.ver);
            A.st(0, FP_META, (int64_t)(m | META_FLAG(AF_CANCEL)));
            A.st(0, FP_CANCEL_ID, e.id);
          }
          break;
        }
        case CDR_EV_AT_REQ_CANCEL_FAILED:
        case CDR_EV_CANCEL_TIMER_FAILED:
        case CDR_EV_MARKER_RECORDED:
          break;
        case CDR_EV_WF_SIGNALED:  // :3082-3089
          x_signals += mine ? 1 : 0;
          break;
        case CDR_EV_WF_CANCEL_REQUESTED:  // :2504-2510
          x_flags |= mine ? CDR_XI_CANCEL_REQUESTED : 0u;
          break;
        case CDR_EV_WF_COMPLETED:
        case CDR_EV_WF_FAILED:
        case CDR_EV_WF_TIMED_OUT:
        case CDR_EV_WF_CANCELED:
        case CDR_EV_WF_TERMINATED: {  // stateBuilder.go:483-531
          const int cs = ut == CDR_EV_WF_COMPLETED   ? CDR_CLOSE_COMPLETED
                         : ut == CDR_EV_WF_FAILED    ? CDR_CLOSE_FAILED
                         : ut == CDR_EV_WF_TIMED_OUT ? CDR_CLOSE_TIMED_OUT
                         : ut == CDR_EV_WF_CANCELED  ? CDR_CLOSE_CANCELED
                                                     : CDR_CLOSE_TERMINATED;
          const bool f = mine && !transition_ok(XS_STATE, XS_CLOSE, CDR_STATE_COMPLETED, cs);
          PFAIL(f, CDR_E_INVALID_STATE_TRANSITION);
          const bool ok = mine && !f;
          xs = SEL(ok, (xs & 0x80000000u) | (uint32_t)CDR_STATE_COMPLETED | ((uint32_t)cs << 8), xs);
          if (ok) {
            Z.st(0, ZP_COMPLETION_BATCH, call_first_id);
            Z.st(0, ZP_CLOSE_VER, e.ver);
          }
          // appendTasksForFinishedExecutions (:775-787)
          task_x(ok, CDR_TT_CLOSE_EXECUTION, 0, 0, 0);
          task_t(ok, CDR_TT_DELETE_HISTORY, 0, 0, e.ts + (int64_t)D.retention_days * 86400ll * NS_PER_S);
          break;
        }
        default:  // not a fast-path type: the planner never routes such a history here
          PFAIL(mine, CDR_E_BAD_INPUT);
          break;
      }
    }
    if constexpr (TASKS) {  // this step's task stores, before the next step's prefetch accounting
      if constexpr (CDR_FAST_TBUF > 0) {
        if (n_pool + 2u * CDR_SLICE_WIDTH > TQ_CAP) {  // <= 2 records per lane a step
          tq_flush();
          VM_DRAIN();
        }
      } else {
        VM_DRAIN();
      }
    }
  };
  static_assert(FD >= 1 && FD <= 3, "CDR_FDEPTH");
  // whole groups of FD steps with no exit between them: a skipped step would be a
  // path on which a slot's refill is the newest load, and the waitcnt pass would then
  // wait for everything at every slot use
  uint32_t k = 1;
#if CDR_FAST_UNI
  // The uniform loop: whole groups whose rows carry one type_flags word on every executing lane
  // (the flagship shape: every history of the slice alike).  A group qualifies when the FD words
  // its steps consume and the FD words that gate their loads each equal the first executing
  // lane's, every lane's history reaches the group's last row, and that row is inside the slice
  // (so the group's steps never see a clamped row).  The first group that does not qualify goes
  // to the loop below, at its boundary, with the ring as that loop keeps it; the uniform loop is
  // not entered again.  (A uniform step stores the scalar it gated its loads with as the slot's
  // Q[].tf, so from the second group on only the T[] half of the test can fail: a row that is not
  // uniform is seen FD rows ahead, as the word that would gate its loads, and the per-lane loop
  // takes over one group before that row.  The Q[].tf half decides the first group, whose words
  // the Started block and the prologue loaded per lane.)
  for (; k + FD <= srows; k += FD) {
    uint32_t stf[FD], stn[FD];
    bool nu = k + FD > len;
#pragma unroll
    for (uint32_t j = 0; j < FD; j++) {
      stf[j] = __builtin_amdgcn_readfirstlane(Q[(1 + j) % FD].tf);
      stn[j] = __builtin_amdgcn_readfirstlane(T[(1 + j) % FD]);
      nu |= Q[(1 + j) % FD].tf != stf[j] || T[(1 + j) % FD] != stn[j];
    }
    if (__builtin_amdgcn_ballot_w64(nu) != 0 || __builtin_amdgcn_ballot_w64(!done) == 0) break;
    step(fast_uni_yes{}, k, Q[1 % FD], T[1 % FD], stf[0], stn[0]);
    if (FD > 1) step(fast_uni_yes{}, k + 1, Q[2 % FD], T[2 % FD], stf[1 % FD], stn[1 % FD]);
    if (FD > 2) step(fast_uni_yes{}, k + 2, Q[3 % FD], T[3 % FD], stf[2 % FD], stn[2 % FD]);
  }
#endif
  for (; k < srows; k += FD) {  // slot of row k is k % FD
    if (__builtin_amdgcn_ballot_w64(!done) == 0) break;
    step(fast_uni_no{}, k, Q[1 % FD], T[1 % FD], 0u, 0u);
    if (FD > 1) step(fast_uni_no{}, k + 1, Q[2 % FD], T[2 % FD], 0u, 0u);
    if (FD > 2) step(fast_uni_no{}, k + 2, Q[3 % FD], T[3 % FD], 0u, 0u);
  }
#undef PFAIL
#undef SEL
#undef FLD_CAPTURE
  if constexpr (TASKS && CDR_FAST_TBUF > 0) tq_flush();
  // the failed event's id from its row (row 0 of an empty history is out of range: 0)
  int64_t err_id = err != CDR_OK ? bld64(S.r, el8(err_k, len, lane), S.col(CDR_COL_EVENT_ID)) : 0;
  if (len > 0 && err == CDR_OK) x_next_event = prev_id + 1;
  if (err == CDR_OK && D.parent < 0 && D.expected_next_event_id != 0 && x_next_event != D.expected_next_event_id) {
    err = CDR_E_REBUILD_NEXT_EVENT_ID;  // nDCStateRebuilder.go:139-143
    err_id = prev_id;
    err_k = len;
  }
  if (TASKS && err == CDR_OK && (n_xt > t_xcap || n_tt > t_tcap)) {  // a task list past its slice
    err = CDR_E_BAD_INPUT;
    err_id = prev_id;
    err_k = len;
  }
  const bool ok = err == CDR_OK;
  uint32_t n_sa = 0;  // the Started event's search attributes, as its block stored them
  if (ok) {
    const GAS cdr_attr_wf_started* a =
        gp((const cdr_attr_wf_started*)(B_.ev.arena + (uint64_t)bld64(S.r, lane8, S.col(CDR_COL_AUX))));
    const uint32_t cnt = a->search_attr_len, cap = CP.sa_cap;
    n_sa = (a->flags & CDR_SF_HAS_SEARCH_ATTR) ? (cnt < cap ? cnt : cap) : 0u;
  }
  const bool act_live = ok && XS_ACT && A.ld(0, FP_SID) != DEAD_KEY;
  cdr_wf_result r;
  r.code = err;
  r.flags = D.parent >= 0 ? CDR_RF_IS_NEWRUN : 0u;
  r.fail_event_id = err_id;
  r.fail_index = err_k;
  r.n_activity = act_live ? 1u : 0u;
  r.n_timer = r.n_child = r.n_cancel = r.n_signal = 0;
  r.n_vh = ok ? n_vh : 0u;
  r.n_reset_points = ok ? n_rp : 0u;
  r.n_search_attr = ok ? n_sa : 0u;
  if constexpr (TASKS) {
    gp(O_.n_tasks)[2 * (uint64_t)w] = ok ? n_xt : 0u;
    gp(O_.n_tasks)[2 * (uint64_t)w + 1] = ok ? n_tt : 0u;
  }
  // every record below is assembled in registers first (the LDS planes are read for the last
  // time here), then written by the wave together (coop_put) through those planes
  const bool ld_on = ok && want_ld && !(ld & LD_CAPTURED);
  const cdr_last_decision ldr =
      ld_rec(ld, dv, dsched, dstart, dreq, dto, datt, Z.ld(0, ZP_DSC_TS), Z.ld(0, ZP_DST_TS), Z.ld(0, ZP_DORIG_TS));
  cdr_activity_info o{};
  if (act_live) {  // the pending activity as a persisted row (as in k_replay)
    const uint64_t rows = (uint64_t)A.ld(0, FP_ROWS);
    const uint32_t o_s = el8((uint32_t)rows, len, lane), o_b = el8((uint32_t)(rows >> 32), len, lane);
    const int64_t sched_ts = bld64(S.r, o_s, S.col(CDR_COL_TIMESTAMP));
    const uint32_t arec = (uint32_t)bld64(S.r, o_s, S.col(CDR_COL_AUX));
    const GAS cdr_attr_at_scheduled* a = gp((const cdr_attr_at_scheduled*)(B_.ev.arena + arec));
    const uint64_t m = (uint64_t)A.ld(0, FP_META);
    const bool retry = (a->flags & CDR_AF_HAS_RETRY) != 0;
    const int32_t s2c = a->s2c_s, xs = a->retry_expiration_s;
    o.version = A.ld(0, FP_VER);
    o.schedule_id = A.ld(0, FP_SID);
    o.scheduled_event_batch_id = bld64(S.r, o_b, S.col(CDR_COL_EVENT_ID));
    o.scheduled_time = sched_ts;
    o.started_id = A.ld(0, FP_STARTED_ID);
    o.started_time = A.ld(0, FP_STARTED_TIME);
    o.last_heartbeat_time = A.ld(0, FP_STARTED_TIME);
    o.expiration_time = sched_ts + (int64_t)((retry && xs > s2c) ? xs : s2c) * NS_PER_S;
    o.cancel_request_id = A.ld(0, FP_CANCEL_ID);
    o.activity_id = (uint32_t)m;
    o.request_id = (uint32_t)A.ld(0, FP_REQ);
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
  }
  uint32_t hv[32] = {};  // the replay half of ExecutionInfo (bytes 128-255)
  {
    auto p64 = [&](int i, int64_t v) {
      hv[i] = (uint32_t)v;
      hv[i + 1] = (uint32_t)((uint64_t)v >> 32);
    };
    hv[0] = dreq;  // decision_request_id, flags
    hv[1] = x_flags;
    p64(2, Z.ld(0, ZP_COMPLETION_BATCH));
    hv[4] = (uint32_t)XS_STATE;
    hv[5] = (uint32_t)XS_CLOSE;
    p64(6, call_first_id);  // last_first_event_id: stateBuilder.go:603 of the last call
    p64(8, bld64(S.r, el8(len - 1, len, lane), S.col(CDR_COL_TASK_ID)));  // last_event_task_id :155
    p64(10, x_next_event);
    p64(12, Z.ld(0, ZP_LAST_PROCESSED));
    hv[14] = (uint32_t)x_signals;
    hv[15] = (uint32_t)dto;
    p64(16, dv);
    p64(18, dsched);
    p64(20, dstart);
    p64(22, datt);
    p64(24, Z.ld(0, ZP_DST_TS));
    p64(26, Z.ld(0, ZP_DSC_TS));
    p64(28, Z.ld(0, ZP_DORIG_TS));
    hv[30] = n_rp;  // reset_points_len, search_attr_len
    hv[31] = n_sa;
  }
  const bool vh_on = ok && n_vh;
  const cdr_vh_item vi{prev_id, prev_ver};
  GAS cdr_vh_item* const vh_dst = vh_on ? vh + (n_vh - 1) : nullptr;
  GAS cdr_activity_info* const act_dst = act_live ? gp(O_.act) + CP.act_off : nullptr;
  coop_put<7>(gp(O_.result) + w, r, true, 0);
  coop_put<10>(gp(O_.last_decision) + w, ldr, ld_on, 0);
  coop_put<9>(act_dst, o, act_live, 0);
  coop_put<2>(vh_dst, vi, vh_on, 0);
  // The replay half of every OK entry's ExecutionInfo record — one 128-B line at offset 128
  // (schema.h) — written by the wave together: through LDS (the activity slot and cold planes,
  // read for the last time above), 8 lanes per record, so that each line is written whole by
  // one store instruction.  Field by field from 64 lanes whose records lie 256 B+ apart, every
  // 4- or 8-B store was a write request of its own (tools/calib.hip: k_cal_wrec).
  {
    constexpr uint32_t RS = 65;  // LDS row stride (dwords): conflict-free column writes
    static_assert(33u * RS * 4u <= FAST_LDS_BYTES, "the transpose fits the planes it reuses");
    static_assert(11u * RS * 8u <= FAST_LDS_BYTES, "so does coop_put<10>'s");
    static_assert(16u * FAST_LDS_BYTES <= 160u * 1024u, "sixteen one-wave workgroups per CU: four waves per SIMD");
    uint32_t* const L32 = (uint32_t*)cdr_lds;
    const uint64_t em = __builtin_amdgcn_read_exec();
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(em >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)em, 0u));
    const uint32_t na = (uint32_t)__builtin_popcountll(em);
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): the planes' last reads have landed
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (uint32_t j = 0; j < 32; j++) L32[j * RS + rank] = hv[j];
    L32[32 * RS + rank] = ok ? (uint32_t)w : 0xFFFFFFFFu;
    __builtin_amdgcn_s_waitcnt(0xC07F);
    __builtin_amdgcn_wave_barrier();
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    for (uint32_t i = rank; i < 8u * na; i += na) {
      const uint32_t rr = i >> 3, c = i & 7u;  // record (by lane rank), 16-B chunk
      const uint32_t wr = L32[32 * RS + rr];
      if (wr != 0xFFFFFFFFu) {
        u32x4 v;
        v.x = L32[(4 * c) * RS + rr];
        v.y = L32[(4 * c + 1) * RS + rr];
        v.z = L32[(4 * c + 2) * RS + rr];
        v.w = L32[(4 * c + 3) * RS + rr];
        *((GAS u32x4*)((GAS uint8_t*)(gp(O_.exec) + wr) + 128) + c) = v;
      }
    }
  }
#undef D
#undef CP
#undef X
#undef vh
#undef rp
#undef vh_l
#undef XS_STATE
#undef XS_CLOSE
#undef XS_ACT
#undef CP_L
#undef rp_l
#undef sa
#undef B_
#undef O_
}
