// replay_cls.inc — class-decomposed lane-per-workflow replay (included by replay.hip
// after replay_reg.inc; semantics are k_replay_reg's, output for output).
//
// Why.  k_replay_reg walks its 64 histories in lockstep, one event per lane per step, so
// a step costs the union of the handler groups its lanes' events hit — on C3-C5 nearly
// every group, ~2,100 instructions for 64 events.  Yet the entity FSMs hardly touch one
// another: pending activities change only at activity events, user timers only at timer
// events, children / request-cancels / signals only at theirs, and the decision /
// workflow FSM ("W") only at the rest.  What couples them is
//   * the call structure (batch boundaries: LastFirstEventID, NextEventID, the transient
//     decision's schedule ID, the batch IDs of pending rows, lastDecision's reset),
//   * the version bookkeeping (NDC VersionHistory, 2DC ReplicationState /
//     LastReplicationInfo), which reads every event,
//   * one flag: a new reset point is Resettable only while no child / request-cancel /
//     signal is pending (mutableStateBuilder.go:1798-1842).
// So every register-table slice also gets a class-sorted block (cdr.h, built once after
// packing by k_cls_fill): per lane its W events, activity events, timer events and
// external events, each class in history order, in regions aligned across the 64
// lanes, every event annotated with its history index, its call's first index and the
// NextEventID at its call (functions of the input's batch structure only).  The kernel
// runs five loops over the slice:
//   P  the original block in history order, type_flags plus the ids / versions the delta
//      bits do not imply: call structure, NDC VersionHistory, 2DC LastReplicationInfo;
//   W  the W region: decision FSM, close FSM, Started / upserts / continue-as-new, reset
//      points (their history indices in LDS), signals — then the ExecutionInfo record;
//   A, T, X  one region each: the entity tables in registers, one handler group per
//      step, the rows written at the end of each loop; X also settles each new reset
//      point's Resettable flag at the first external event after it.
// Each loop holds only its own state, so registers and LDS are sized by the largest
// phase, not by their sum.
//
// Anything this kernel does not replay itself — any error or panic, a second
// WorkflowExecutionStarted, a continue-as-new outside the entry's last call, a
// NextEventID the annotation cannot carry — leaves the entry's result code CLS_RETRY;
// k_replay_reg then replays exactly those entries from the original block (same slice,
// launched right after on the same stream), so every output is k_replay_reg's.

#ifndef CDR_CLS_DEPTH
#define CDR_CLS_DEPTH 1 /* class-region rows in flight per wave (2: +15 VGPRs, spills at 4 waves/SIMD: +50% on C3) */
#endif
#ifndef CDR_CLS_TBUF
#define CDR_CLS_TBUF 3 /* TASKS: the wave's LDS pool of staged task records, CDR_CLS_TBUF x 64 (32 B each); C3 --tasks 2 / 3 / 4 / 6: 13.05 / 10.92 / 11.81 / 11.38 ms (round 6, profiles/r6_tbuf) */
#endif
#ifndef CDR_WPE_CLS_T
#define CDR_WPE_CLS_T 3 /* the <6,10,4> / <3,5,3> TASKS instantiations (staging adds registers and LDS) */
#endif
#define CLS_TQ_BYTES ((size_t)CDR_CLS_TBUF * CDR_SLICE_WIDTH * 32u)
#ifndef CDR_CLS_PEEL_STARTED
#define CDR_CLS_PEEL_STARTED 1 /* the W loop's first row replayed before it (Started) */
#endif
#ifndef CDR_CLS_DEPTH_W
#define CDR_CLS_DEPTH_W CDR_CLS_DEPTH /* the same for the W loop (its state is smaller than A's) */
#endif
#ifndef CDR_CLS_DEPTH_T
#define CDR_CLS_DEPTH_T CDR_CLS_DEPTH /* the T loop */
#endif
#ifndef CDR_CLS_DEPTH_X
#define CDR_CLS_DEPTH_X CDR_CLS_DEPTH /* the X loop */
#endif
#ifndef CDR_CLS_PDEPTH
#define CDR_CLS_PDEPTH 4 /* history rows (type_flags, id, version) in flight in the P loop */
#endif
#ifndef CDR_CLS_DEPTH_PAR
#define CDR_CLS_DEPTH_PAR 4 /* the same in the four-wave PAR variant (one long history's chain per wave) */
#endif
#ifndef CDR_CLS_PDEPTH_PAR
#define CDR_CLS_PDEPTH_PAR 16
#endif
#ifndef CDR_PAR_PRIO
#define CDR_PAR_PRIO 0 /* s_setprio of the PAR waves (0-3) */
#endif
#ifndef CDR_WPE_CLS
#define CDR_WPE_CLS 4 /* waves per SIMD the <6,10,4> variant is compiled for */
#endif
#ifndef CDR_WPE_CLS0
#define CDR_WPE_CLS0 4 /* <3,5,3> */
#endif
#ifndef CDR_WPE_CLS2
#define CDR_WPE_CLS2 2 /* <12,10,4> */
#endif

namespace {

// the class sets live in cdr.h (cdr_cls_of), shared with the host packer (cdr_pack_cls)
enum : uint32_t { CLS_DROP = CDR_CLS_DROP };
static_assert(CDR_CLS_A_TYPES == RG_ACT && CDR_CLS_T_TYPES == RG_TIM && CDR_CLS_X_TYPES == RG_EXT,
              "class regions = the register kernel's handler groups");
#define CLS_DROP_TYPES CDR_CLS_DROP_TYPES
#define CLS_NEED_ID CDR_CLS_NEED_ID
__device__ __forceinline__ uint32_t cls_of(uint32_t type) { return cdr_cls_of(type); }
constexpr uint32_t CLS_REG_SLICES = CDR_CLS_SLICES;
constexpr uint32_t XD_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t u = (uint32_t)__shfl_xor((int)v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}
__device__ __forceinline__ uint8_t* el_ptr(uint8_t* slab, uint64_t row, int c, uint32_t lane) {
  return slab + row * CDR_ROW_BYTES + cdr_col_off(c) + (uint64_t)lane * cdr_col_size(c);
}

// ---- The device class sort (cdr_cls_plan_async + cdr_cls_pack_async): the class-sorted
// blocks the host packer emits (cdr_pack_cls), built from the slab in HBM.
//
// k_cls_count (one wave per slice, a lane per history) walks each history once, reading the
// type word, event id and version of row k on every lane together (coalesced), and keeps per
// event what the block needs: its class and position in the class region, the block's type
// word (CLS_NO_ID / CLS_VER_SAME) and the annotation CDR_CLS_ANN(k, k - k0, d) — written in the
// slab's own row layout into a map beside it (map rows = slab rows: coalesced too), plus the
// slice's class-region sizes (the wave max of each class count).
// k_cls_gather (one 1024-thread workgroup per slice) then transposes column by column through
// LDS: the inverse map (output row r, lane L) -> source row k, then for each of the nine
// columns the slice's source column staged in LDS with 16-B loads and the output rows written
// whole (64 lanes x 4 or 8 B, one store instruction per wave and row).  Slices too long for
// the LDS budget (a column of more than CLS_G_MAXLEN rows, or more than CLS_G_MAXR block rows)
// go to k_cls_fill, the per-lane scatter (one write request per event and column).
constexpr uint32_t CLS_G_MAXLEN = 216;   // source rows of a staged 8-B column: 216 x 512 B = 108 KB
constexpr uint32_t CLS_G_MAXR = 320;     // block rows of the inverse map (u16 source rows): 320 x 128 B = 40 KB
constexpr uint32_t CLS_G_THREADS = 1024;
constexpr uint32_t CLS_MAP_NONE = 0xFFFFFFFFu;  // a dropped event / a row past the history
// per slab row: the map (u32 class << 30 | position), the block's type word (u32), the
// annotation (u64) — three planes of n_rows x 64 entries
struct ClsMap {
  uint32_t* pos;
  uint32_t* tf2;
  uint64_t* ann;
};
__device__ __forceinline__ ClsMap cls_map_planes(void* base, uint64_t n_rows) {
  uint8_t* p = (uint8_t*)base;
  const uint64_t n = n_rows * CDR_SLICE_WIDTH;
  return ClsMap{(uint32_t*)p, (uint32_t*)(p + 4 * n), (uint64_t*)(p + 8 * n)};
}

// the class-sorted block's type word and annotation of event k (the rules of cdr_pack_cls):
// state carried along the lane's history
struct ClsWalk {
  int64_t prev_id = 0, x_next = CDR_FIRST_EVENT_ID, wver = 0;
  uint32_t k0 = 0;
  bool any_w = false;
  __device__ __forceinline__ void step(uint32_t k, uint32_t tf, int64_t id, int64_t ver, uint32_t& c, uint32_t& tf2,
                                       uint64_t& ann) {
    const bool bf = (tf & CDR_SEF_BATCH_FIRST) || k == 0;
    if (bf && k > 0) x_next = prev_id + 1;  // NextEventID after the previous call (stateBuilder.go:603-604)
    if (bf) k0 = k;
    prev_id = id;
    const uint32_t type = tf & 0xFFu;
    c = cls_of(type);
    const bool need_id = type < 64 && ((1ull << type) & CLS_NEED_ID);
    const bool same_v = c != CDR_CLS_W || (any_w && ver == wver);
    if (c == CDR_CLS_W) {
      wver = ver;
      any_w = true;
    }
    tf2 = (tf & ~(CDR_SEF_ID_NEXT | CDR_SEF_VER_SAME)) | (need_id ? 0u : CDR_SEF_CLS_NO_ID) |
          (same_v ? CDR_SEF_CLS_VER_SAME : 0u);
    const uint64_t d = (uint64_t)id - (uint64_t)x_next;
    const uint32_t xd = (id >= x_next && d < XD_NONE) ? (uint32_t)d : XD_NONE;
    ann = CDR_CLS_ANN(k, (k - k0) & 0xFFFu, xd);
  }
};

// ---- size pass (+ the map when `map` is set): per register-table slice, the wave max of
// each class count
__global__ __launch_bounds__(CDR_SLICE_WIDTH) void k_cls_count(cdr_dev_batch B, uint32_t* cls_rows,
                                                               uint64_t* cls_len, void* map) {
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  if (s >= B.ev.n_slices) return;
  const bool on = (B.ev.slice_flags[s] & CLS_REG_SLICES) != 0;
  const int32_t w = on ? B.ev.lane_wf[(uint64_t)s * CDR_SLICE_WIDTH + lane] : -1;
  const uint32_t len = w >= 0 ? (uint32_t)B.wfs[w].ev_len : 0u;
  const uint64_t row0 = B.ev.slice_row0[s];
  const uint8_t* slab = B.ev.slab + row0 * CDR_ROW_BYTES;
  const uint32_t slen = on ? B.ev.slice_len[s] : 0u;
  const ClsMap M = cls_map_planes(map, B.ev.n_rows);
  auto at = [&](uint32_t k, int c, uint32_t sz) { return slab + (uint64_t)k * CDR_ROW_BYTES + cdr_col_off(c) + lane * sz; };
  uint32_t n[4] = {0, 0, 0, 0};
  ClsWalk cw;
  // (the next row's words are loaded before this row is processed: two rows in flight)
  uint32_t tf_n = 0;
  int64_t id_n = 0, ver_n = 0;
  if (0 < len) {
    tf_n = *(const uint32_t*)at(0, CDR_COL_TYPE_FLAGS, 4);
    if (map) {
      id_n = *(const int64_t*)at(0, CDR_COL_EVENT_ID, 8);
      ver_n = *(const int64_t*)at(0, CDR_COL_VERSION, 8);
    }
  }
  for (uint32_t k = 0; k < slen; k++) {
    const bool live = k < len;
    const uint32_t tf = tf_n;
    const int64_t id = id_n, ver = ver_n;
    if (k + 1 < len) {
      tf_n = *(const uint32_t*)at(k + 1, CDR_COL_TYPE_FLAGS, 4);
      if (map) {
        id_n = *(const int64_t*)at(k + 1, CDR_COL_EVENT_ID, 8);
        ver_n = *(const int64_t*)at(k + 1, CDR_COL_VERSION, 8);
      }
    }
    uint32_t c = CLS_DROP, tf2 = 0;
    uint64_t ann = 0;
    if (live) {
      if (map) cw.step(k, tf, id, ver, c, tf2, ann);
      else c = cls_of(tf & 0xFFu);
    }
    uint32_t p = CLS_MAP_NONE;
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
      p = (live && c == j) ? (j << 30) | n[j] : p;
      n[j] += (live && c == j) ? 1u : 0u;
    }
    if (map) {
      const uint64_t e = (row0 + k) * CDR_SLICE_WIDTH + lane;
      M.pos[e] = p;
      M.tf2[e] = tf2;
      M.ann[e] = ann;
    }
  }
  uint32_t tot = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) {
    n[j] = wave_max(n[j]);
    tot += n[j];
  }
  if (lane == 0) {
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) cls_rows[4ull * s + j] = n[j];
    cls_len[s] = tot;
  }
}

// exclusive scan of n values in place (one workgroup of 1024 threads; n + 1 entries,
// entry n = the total)
__global__ __launch_bounds__(1024) void k_cls_scan(uint64_t* v, uint32_t n) {
  __shared__ uint64_t part[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t chunk = (n + 1023u) / 1024u;
  const uint32_t lo = t * chunk, hi = lo + chunk < n ? lo + chunk : n;
  uint64_t sum = 0;
  for (uint32_t i = lo; i < hi; i++) sum += v[i];
  part[t] = sum;
  __syncthreads();
  for (uint32_t o = 1; o < 1024; o <<= 1) {
    const uint64_t x = t >= o ? part[t - o] : 0ull;
    __syncthreads();
    part[t] += x;
    __syncthreads();
  }
  uint64_t run = part[t] - sum;  // exclusive prefix of this chunk
  for (uint32_t i = lo; i < hi; i++) {
    const uint64_t x = v[i];
    v[i] = run;
    run += x;
  }
  if (t == 1023) v[n] = part[1023];
}

__device__ __forceinline__ bool cls_gather_fits(const cdr_dev_batch& B, uint32_t s) {
  uint32_t r = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) r += B.cls_rows[4ull * s + j];
  return B.ev.slice_len[s] <= CLS_G_MAXLEN && r <= CLS_G_MAXR;
}

// ---- write pass, LDS transposition (k_cls_count's map): one workgroup per slice
__global__ __launch_bounds__(CLS_G_THREADS) void k_cls_gather(cdr_dev_batch B, const void* map) {
  const uint32_t s = blockIdx.x, tid = threadIdx.x;
  if (s >= B.ev.n_slices || !(B.ev.slice_flags[s] & CLS_REG_SLICES) || !cls_gather_fits(B, s)) return;
  typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
  extern __shared__ __align__(16) uint8_t cls_g_lds[];
  uint32_t off[4], R = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) {
    off[j] = R;
    R += B.cls_rows[4ull * s + j];
  }
  const uint32_t len = B.ev.slice_len[s];
  const uint64_t row0 = B.ev.slice_row0[s], base = B.cls_row0[s];
  const ClsMap M = cls_map_planes((void*)map, B.ev.n_rows);
  uint16_t* const inv = (uint16_t*)cls_g_lds;                      // [R][64]: source row + 1, 0 = pad
  u32x4* const col = (u32x4*)(cls_g_lds + (size_t)CLS_G_MAXR * CDR_SLICE_WIDTH * 2);  // [len][64] x 4 / 8 B
  // the inverse map: output row off[c] + position of lane L <- source row k
  for (uint32_t i = tid; i < R * CDR_SLICE_WIDTH; i += CLS_G_THREADS) inv[i] = 0u;
  __syncthreads();
  for (uint32_t i = tid; i < len * CDR_SLICE_WIDTH; i += CLS_G_THREADS) {
    const uint32_t p = M.pos[row0 * CDR_SLICE_WIDTH + i];
    if (p != CLS_MAP_NONE)
      inv[(off[p >> 30] + (p & 0x3FFFFFFFu)) * CDR_SLICE_WIDTH + (i & 63u)] = (uint16_t)(i / CDR_SLICE_WIDTH + 1u);
  }
  __syncthreads();
  uint8_t* const dst = (uint8_t*)B.cls_slab + base * CDR_ROW_BYTES;
  // the nine columns: source (the slab's column, or the map's type word / annotation plane)
  for (uint32_t cidx = 0; cidx < 9; cidx++) {
    const int c = cidx == 0 ? CDR_COL_TYPE_FLAGS : cidx == 1 ? CDR_COL_EVENT_ID : cidx == 2 ? CDR_COL_VERSION
                : cidx == 3 ? CDR_COL_TIMESTAMP : cidx == 4 ? CDR_COL_TASK_ID : cidx == 5 ? CDR_COL_KEY
                : cidx == 6 ? CDR_COL_AUX : cidx == 7 ? CDR_COL_H : CDR_COL_N;
    const uint32_t sz = cdr_col_size(c);  // 4 or 8
    const uint32_t q_row = CDR_SLICE_WIDTH * sz / 16u;  // 16-B chunks per row segment
    // stage: source rows 0 .. len-1 of this column, 16 B per load, 8 loads in flight per thread
    const uint8_t* srcb = cidx == 0 ? (const uint8_t*)(M.tf2 + row0 * CDR_SLICE_WIDTH)
                        : cidx == 4 ? (const uint8_t*)(M.ann + row0 * CDR_SLICE_WIDTH) : nullptr;
    const uint32_t nq = len * q_row;
    for (uint32_t i0 = tid; i0 < nq; i0 += 8 * CLS_G_THREADS) {
      u32x4 v[8];
#pragma unroll
      for (uint32_t u = 0; u < 8; u++) {
        const uint32_t i = i0 + u * CLS_G_THREADS;
        if (i < nq) {
          const uint32_t k = i / q_row, q = i % q_row;
          const u32x4* p = srcb ? (const u32x4*)(srcb + (uint64_t)k * CDR_SLICE_WIDTH * sz) + q
                                : (const u32x4*)(B.ev.slab + (row0 + k) * CDR_ROW_BYTES + cdr_col_off(c)) + q;
          v[u] = *p;
        }
      }
#pragma unroll
      for (uint32_t u = 0; u < 8; u++) {
        const uint32_t i = i0 + u * CLS_G_THREADS;
        if (i < nq) col[i] = v[u];
      }
    }
    __syncthreads();
    // emit: output row r, lane L = the staged element (source row, L); a wave per row
    const uint32_t L = tid & 63u;
    for (uint32_t r = tid / CDR_SLICE_WIDTH; r < R; r += CLS_G_THREADS / CDR_SLICE_WIDTH) {
      const uint32_t kk = inv[r * CDR_SLICE_WIDTH + L];
      uint8_t* const o = dst + (uint64_t)r * CDR_ROW_BYTES + cdr_col_off(c);
      if (sz == 8) {
        const uint64_t x = kk ? ((const uint64_t*)col)[(kk - 1u) * CDR_SLICE_WIDTH + L] : 0ull;
        ((uint64_t*)o)[L] = x;
      } else {
        const uint32_t x = kk ? ((const uint32_t*)col)[(kk - 1u) * CDR_SLICE_WIDTH + L]
                              : (cidx == 0 ? (uint32_t)(CDR_EV_PAD | CDR_SEF_CLS_NO_ID | CDR_SEF_CLS_VER_SAME) : 0u);
        ((uint32_t*)o)[L] = x;
      }
    }
    __syncthreads();
  }
}
constexpr size_t CLS_G_LDS = (size_t)CLS_G_MAXR * CDR_SLICE_WIDTH * 2 + (size_t)CLS_G_MAXLEN * CDR_SLICE_WIDTH * 8;
static_assert(CLS_G_LDS <= 160 * 1024, "k_cls_gather's LDS");

// ---- write pass, per-lane scatter (the slices k_cls_gather leaves: longer than its LDS
// budget; every slice when `all`): lane L walks its history once and writes every kept event
// into its class region (row off[c] + position), then pads its regions with CDR_EV_PAD rows
__global__ __launch_bounds__(CDR_SLICE_WIDTH) void k_cls_fill(cdr_dev_batch B, int all) {
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  if (s >= B.ev.n_slices || !(B.ev.slice_flags[s] & CLS_REG_SLICES)) return;
  if (!all && cls_gather_fits(B, s)) return;
  const int32_t w = B.ev.lane_wf[(uint64_t)s * CDR_SLICE_WIDTH + lane];
  uint32_t M[4], off[4];
  uint32_t acc = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) {
    M[j] = B.cls_rows[4ull * s + j];
    off[j] = acc;
    acc += M[j];
  }
  uint8_t* dst = (uint8_t*)B.cls_slab;
  const uint64_t base = B.cls_row0[s];
  const uint8_t* src = B.ev.slab + B.ev.slice_row0[s] * CDR_ROW_BYTES;
  const uint32_t len = w >= 0 ? (uint32_t)B.wfs[w].ev_len : 0u;
  uint32_t pos[4] = {0, 0, 0, 0};
  ClsWalk cw;
  auto rd64 = [&](uint32_t k, int c) { return *(const int64_t*)(src + (uint64_t)k * CDR_ROW_BYTES + cdr_col_off(c) + lane * 8u); };
  auto rd32 = [&](uint32_t k, int c) { return *(const uint32_t*)(src + (uint64_t)k * CDR_ROW_BYTES + cdr_col_off(c) + lane * 4u); };
  for (uint32_t k = 0; k < len; k++) {
    const uint32_t tf = rd32(k, CDR_COL_TYPE_FLAGS);
    const int64_t id = rd64(k, CDR_COL_EVENT_ID), ver = rd64(k, CDR_COL_VERSION);
    uint32_t c, tf2;
    uint64_t ann;
    cw.step(k, tf, id, ver, c, tf2, ann);
    if (c == CLS_DROP) continue;
    const uint64_t row = base + off[c] + pos[c]++;
    *(uint32_t*)el_ptr(dst, row, CDR_COL_TYPE_FLAGS, lane) = tf2;
    *(int64_t*)el_ptr(dst, row, CDR_COL_EVENT_ID, lane) = id;
    *(int64_t*)el_ptr(dst, row, CDR_COL_VERSION, lane) = ver;
    *(int64_t*)el_ptr(dst, row, CDR_COL_TIMESTAMP, lane) = rd64(k, CDR_COL_TIMESTAMP);
    *(uint64_t*)el_ptr(dst, row, CDR_COL_TASK_ID, lane) = ann;
    *(int64_t*)el_ptr(dst, row, CDR_COL_KEY, lane) = rd64(k, CDR_COL_KEY);
    *(int64_t*)el_ptr(dst, row, CDR_COL_AUX, lane) = rd64(k, CDR_COL_AUX);
    *(uint32_t*)el_ptr(dst, row, CDR_COL_H, lane) = rd32(k, CDR_COL_H);
    *(uint32_t*)el_ptr(dst, row, CDR_COL_N, lane) = rd32(k, CDR_COL_N);
  }
#pragma unroll
  for (uint32_t j = 0; j < 4; j++)
    for (uint32_t p = pos[j]; p < M[j]; p++)
      *(uint32_t*)el_ptr(dst, base + off[j] + p, CDR_COL_TYPE_FLAGS, lane) =
          CDR_EV_PAD | CDR_SEF_CLS_NO_ID | CDR_SEF_CLS_VER_SAME;
}

// LDS planes (4-byte words, lane-interleaved) of k_replay_cls: the reset points live from
// the W loop to the X loop; the rest is one region each loop reuses
// (PAR: the loops run at once on four waves of one workgroup, so each gets a region of its
// own, plus the mailbox words through which they hand over results)
template <int NA, int NT, int NX, bool PAR = false>
struct ClsLds {
  static constexpr uint32_t P0 = 0;  // reset points: checksum, history index (RNONE: Started row) | resettable << 31
  static constexpr uint32_t NRP = CDR_REG_NRP_OF(NA);
  static constexpr uint32_t Q0 = 2 * NRP;
  static constexpr uint32_t L0 = Q0;  // P..W: 2DC LastReplicationInfo per cluster: version, event id
  static constexpr uint32_t A0 = PAR ? L0 + 2 * CDR_REG_NCL : Q0;  // A: per activity slot: sched (k | (k - call first) << 20), started k, cancel k
  static constexpr uint32_t T0 = PAR ? A0 + 3 * NA : Q0;  // T: per timer slot: TimerStarted index
  static constexpr uint32_t C0 = PAR ? T0 + NT : Q0;      // X: per child slot: initiated (k | dcf << 20), started k
  static constexpr uint32_t R0 = C0 + 2 * NX;  //    per request-cancel slot: initiated
  static constexpr uint32_t G0 = R0 + NX;      //    per signal slot: initiated
  // PAR mailbox: P's last call first index, call count, n_vh | retry << 31; A/T's counts |
  // retry << 31; X's counts | retry << 31; W's progress (history index below which every
  // W event is replayed; ~0 when done) and reset point count
  static constexpr uint32_t MB = G0 + NX;
  enum : uint32_t { MB_CFK = 0, MB_NCALLS, MB_P, MB_AT, MB_X, MB_WPROG, MB_WNRP, MB_T, MB_N };
  static constexpr uint32_t cmax(uint32_t a, uint32_t b) { return a > b ? a : b; }
  static constexpr uint32_t PF = MB + MB_N;  // CDR_PAR_PROF (variant builds): each wave's loop time
  static constexpr uint32_t W = PAR ? PF + 4 : Q0 + cmax(cmax(2 * CDR_REG_NCL, 3 * NA), cmax(NT, 4 * NX));
  static constexpr size_t bytes = (size_t)W * CDR_SLICE_WIDTH * 4;
};
__device__ __forceinline__ void rs_release(uint32_t p, uint32_t lane, uint32_t v) {
  __hip_atomic_store(((uint32_t*)cdr_lds) + p * CDR_SLICE_WIDTH + lane, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// the W wave's per-step progress word: its earlier LDS writes (reset points, their count)
// complete first (lgkmcnt(0); LDS executes one wave's operations in order), but the
// vector-memory loads in flight stay in flight — a release store would wait for them too
// (vmcnt(0)) and drain the prefetch ring at every step
__device__ __forceinline__ void rs_publish(uint32_t p, uint32_t lane, uint32_t v) {
  __builtin_amdgcn_s_waitcnt(0xC07F);  // vmcnt 63 (no wait), expcnt 7, lgkmcnt 0
  asm volatile("" ::: "memory");
  __hip_atomic_store(((uint32_t*)cdr_lds) + p * CDR_SLICE_WIDTH + lane, v, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ uint32_t rl_poll(uint32_t p, uint32_t lane) {
  const uint32_t v = __hip_atomic_load(((uint32_t*)cdr_lds) + p * CDR_SLICE_WIDTH + lane, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
  asm volatile("" ::: "memory");
  return v;
}
__device__ __forceinline__ uint32_t rl_acquire(uint32_t p, uint32_t lane) {
  return __hip_atomic_load(((uint32_t*)cdr_lds) + p * CDR_SLICE_WIDTH + lane, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// one workgroup barrier with LDS (and global) release / acquire around it
__device__ __forceinline__ void wg_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---- wave helpers of the PAR W scan (one history, 64 of its W events per step)
__device__ __forceinline__ uint32_t rdl(uint32_t v, uint32_t l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ int64_t rdl64(int64_t v, uint32_t l) {
  return (int64_t)(((uint64_t)rdl((uint32_t)((uint64_t)v >> 32), l) << 32) | rdl((uint32_t)v, l));
}
// index of the highest set bit (-1: none) — per lane or of a wave-uniform mask
__device__ __forceinline__ int hbit(uint64_t m) { return m ? 63 - __builtin_clzll(m) : -1; }
// lanes strictly above lane j (j < 0: every lane)
__device__ __forceinline__ uint64_t above(int j) { return j < 0 ? ~0ull : (j >= 63 ? 0ull : ~0ull << (j + 1)); }
// the value lane j holds (j < 0: `old`) — the last writer of a field before / at a lane
__device__ __forceinline__ int64_t from64(int64_t v, int j, int64_t old) {
  const int64_t x = __shfl(v, j < 0 ? 0 : j, CDR_SLICE_WIDTH);
  return j < 0 ? old : x;
}
__device__ __forceinline__ uint32_t from32(uint32_t v, int j, uint32_t old) {
  const uint32_t x = (uint32_t)__shfl((int)v, j < 0 ? 0 : j, CDR_SLICE_WIDTH);
  return j < 0 ? old : x;
}

template <class O>
__device__ __forceinline__ GAS cdr_kv* out_sa(const O& o) { return gp(o.sa); }

// DPP lane moves (gfx9 encodings): a VALU operand modifier, no LDS round trip as a
// ds_bpermute (__shfl*) takes
enum : int { DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140, DPP_WAVE_SHR1 = 0x138 };
template <int CTRL>
__device__ __forceinline__ uint64_t dpp64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, false);
  return ((uint64_t)hi << 32) | lo;
}
template <int CTRL>
__device__ __forceinline__ void min_step(uint64_t& m) {
  const uint64_t o = dpp64<CTRL>(m);
  m = o < m ? o : m;
}
// the smallest `v` over the first 16-lane row, in every lane of it (a DPP butterfly: pairs,
// quads, half-row mirror, row mirror)
__device__ __forceinline__ uint64_t row_min(uint64_t v) {
  min_step<DPP_XOR1>(v);
  min_step<DPP_XOR2>(v);
  min_step<DPP_HALF_MIRROR>(v);
  min_step<DPP_MIRROR>(v);
  return v;
}
// the wave-form tables of a solo PAR slice live in lanes 0..15: the lane of the smallest
// (k1, k2) among those with `on` (lowest lane on a full tie; -1 if none) — k1 first, k2
// only among the lanes that tie on it
__device__ __forceinline__ int row_argmin2(bool on, int64_t k1, int64_t k2) {
  const uint32_t lane = __lane_id();
  // (each reduction runs in every lane, outside any condition: a DPP move reads a lane
  // outside EXEC as zero)
  const uint64_t a = on ? okey(k1) : ~0ull;
  const uint64_t ma = row_min(a);
  const uint64_t t = __builtin_amdgcn_ballot_w64(on && a == ma) & 0xFFFFull;
  if (!(t & (t - 1))) return t ? (int)__builtin_ctzll(t) : -1;
  const bool on2 = (t >> lane) & 1u;
  const uint64_t b = on2 ? okey(k2) : ~0ull;
  const uint64_t mb = row_min(b);
  const uint64_t w = __builtin_amdgcn_ballot_w64(on2 && b == mb) & 0xFFFFull;
  return (int)__builtin_ctzll(w);
}

// a W-region chunk of one history: 64 consecutive W events (row p0 + lane, column h),
// every column loaded (the class block holds full ids and versions, so the scan needs no
// delta bits and no load waits on type_flags)
struct WScanRow {
  uint32_t tf, hh;
  int32_t n;
  int64_t id, ver, ts, key, aux;
  uint64_t ann;
};
__device__ __forceinline__ WScanRow load_wscan(const Slice& C, uint32_t p, uint32_t m, uint32_t h) {
  const uint32_t o8 = (p < m ? p * CDR_ROW_BYTES : OOB_BIT) + h * 8u, o4 = o8 - h * 4u;
  WScanRow q;
  q.tf = bld32<CDR_NT_CLS>(C.r, o4, C.col(CDR_COL_TYPE_FLAGS));
  q.hh = bld32<CDR_NT_CLS>(C.r, o4, C.col(CDR_COL_H));
  q.n = (int32_t)bld32<CDR_NT_CLS>(C.r, o4, C.col(CDR_COL_N));
  q.id = bld64<CDR_NT_CLS>(C.r, o8, C.col(CDR_COL_EVENT_ID));
  q.ver = bld64<CDR_NT_CLS>(C.r, o8, C.col(CDR_COL_VERSION));
  q.ts = bld64<CDR_NT_CLS>(C.r, o8, C.col(CDR_COL_TIMESTAMP));
  q.key = bld64<CDR_NT_CLS>(C.r, o8, C.col(CDR_COL_KEY));
  q.aux = bld64<CDR_NT_CLS>(C.r, o8, C.col(CDR_COL_AUX));
  q.ann = (uint64_t)bld64<CDR_NT_CLS>(C.r, o8, C.col(CDR_COL_TASK_ID));
  return q;
}
__device__ __forceinline__ WScanRow wscan_take(const WScanRow& q) {
  WScanRow e;
  e.tf = mov32(q.tf);
  e.hh = mov32(q.hh);
  e.n = (int32_t)mov32((uint32_t)q.n);
  e.id = mov64(q.id);
  e.ver = mov64(q.ver);
  e.ts = mov64(q.ts);
  e.key = mov64(q.key);
  e.aux = mov64(q.aux);
  e.ann = (uint64_t)mov64((int64_t)q.ann);
  return e;
}

// a class-region event: its operands and its annotation
struct EvC {
  Ev e;
  uint64_t ann;
};
__device__ __forceinline__ EvC load_cls(const Slice& C, uint32_t o8, uint32_t tf) {
  const uint32_t o4 = o8 - C.l4;
  EvC q;
  q.e.tf = tf;
  q.e.id = bld64<CDR_NT_CLS>(C.r, o8 | ((tf & CDR_SEF_CLS_NO_ID) ? OOB_BIT : 0u), C.col(CDR_COL_EVENT_ID));
  q.e.ver = bld64<CDR_NT_CLS>(C.r, o8 | ((tf & CDR_SEF_CLS_VER_SAME) ? OOB_BIT : 0u), C.col(CDR_COL_VERSION));
  q.e.ts = bld64<CDR_NT_CLS>(C.r, gate(o8, tf, CDR_SEF_NEED_TS), C.col(CDR_COL_TIMESTAMP));
  q.e.key = bld64<CDR_NT_CLS>(C.r, gate(o8, tf, CDR_SEF_NEED_KEY), C.col(CDR_COL_KEY));
  q.e.aux = bld64<CDR_NT_CLS>(C.r, gate(o8, tf, CDR_SEF_NEED_AUX), C.col(CDR_COL_AUX));
  q.e.h = bld32<CDR_NT_CLS>(C.r, gate(o4, tf, CDR_SEF_NEED_H), C.col(CDR_COL_H));
  q.e.n = (int32_t)bld32<CDR_NT_CLS>(C.r, gate(o4, tf, CDR_SEF_NEED_N), C.col(CDR_COL_N));
  q.ann = (uint64_t)bld64<CDR_NT_CLS>(C.r, o8 | (((tf & 0xFFu) == CDR_EV_PAD) ? OOB_BIT : 0u), C.col(CDR_COL_TASK_ID));
  return q;
}

}  // namespace

// unrolled register-array access with a per-lane runtime slot (j < 0: no change)
#define CSET(arr, N, j, v)                                                                             \
  do {                                                                                                 \
    _Pragma("unroll") for (int i_ = 0; i_ < (int)(N); i_++) arr[i_] = ((int)(j) == i_) ? (v) : arr[i_]; \
  } while (0)
#define CGET(arr, N, j, out)                                                                           \
  do {                                                                                                 \
    out = arr[0];                                                                                      \
    _Pragma("unroll") for (int i_ = 1; i_ < (int)(N); i_++) out = ((int)(j) == i_) ? arr[i_] : out;     \
  } while (0)
// a class loop over region [off, off + m) of the class-sorted block: a ring of DEPTH
// rows in flight (the operands of rows p .. p + DEPTH - 1 and the types of the DEPTH rows
// after them), unrolled DEPTH times with no exit inside a group, each landed slot copied
// out through opaque moves before its refill (as k_replay_fast's ring); body(event,
// valid) once per row, valid false past the region
template <int DEPTH, class F>
__device__ __forceinline__ void cls_run(const Slice& C, uint32_t off, uint32_t m, uint32_t lane, const bool& retry,
                                        F&& body) {
  auto elc = [&](uint32_t p) { return (p < m ? (off + p) * CDR_ROW_BYTES : OOB_BIT) + lane * 8u; };
  EvC Q[DEPTH];
  uint32_t T[DEPTH];
#pragma unroll
  for (int j = 0; j < DEPTH; j++) T[j] = load_tf(C, elc(j));
#pragma unroll
  for (int j = 0; j < DEPTH; j++) Q[j] = load_cls(C, elc(j), T[j]);
#pragma unroll
  for (int j = 0; j < DEPTH; j++) T[j] = load_tf(C, elc(j + DEPTH));
  for (uint32_t p = 0; p < m; p += DEPTH) {
    if (__builtin_amdgcn_ballot_w64(!retry) == 0) break;
#pragma unroll
    for (int j = 0; j < DEPTH; j++) {
      EvC q;
      q.e = ev_take(Q[j].e);
      q.ann = (uint64_t)mov64((int64_t)Q[j].ann);
      const uint32_t tn = mov32(T[j]);
      Q[j] = load_cls(C, elc(p + j + DEPTH), tn);
      T[j] = load_tf(C, elc(p + j + 2 * DEPTH));
      body(q, p + j < m);
    }
  }
}
// (SKIP: a per-lane flag that drops the row, read before the body runs)
#define CLS_LOOP_BEGIN2(OFF, M, DEPTH, SKIP)                                                          \
  cls_run<PAR ? CDR_CLS_DEPTH_PAR : (DEPTH)>(C, (OFF), (M), lane, retry, [&](const EvC& q_, bool valid_) __attribute__((always_inline)) { \
    const Ev& e = q_.e;                                                                              \
    const uint32_t type = e.tf & 0xFFu;                                                              \
    const bool act = valid_ && !retry && type != CDR_EV_PAD && !(SKIP);                                 \
    const uint32_t k = (uint32_t)q_.ann & 0xFFFFFu;                                                  \
    const uint32_t dcf = ((uint32_t)q_.ann >> 20) & 0xFFFu;                                          \
    (void)dcf;
#define CLS_LOOP_BEGIN(OFF, M, DEPTH) CLS_LOOP_BEGIN2(OFF, M, DEPTH, false)
#define CLS_LOOP_END \
  });
// rk[j] = the number of live slots whose key is below slot j's (keys are distinct): the
// position of slot j's row in key order
#define CLS_RANKS(rk, N, live, key)                                                              \
  do {                                                                                           \
    _Pragma("unroll") for (int j_ = 0; j_ < (int)(N); j_++) {                                    \
      uint32_t r_ = 0;                                                                           \
      _Pragma("unroll") for (int i_ = 0; i_ < (int)(N); i_++) r_ += (((live) >> i_) & 1u) && key[i_] < key[j_] ? 1u : 0u; \
      rk[j_] = r_;                                                                               \
    }                                                                                            \
  } while (0)

// PAR's P loop for ONE history, lane h of the slice (history order, column h of the
// original block): its events 64 at a time, one per lane — call boundaries and counts
// from ballots, NDC VersionHistory items where the version rises (each lane compares with
// its predecessor, lane 0 with the previous chunk's last event), 2DC LastReplicationInfo as
// the last call end per cluster — the same outputs as the lane loop: P's records, LRI
// planes and mailbox words of lane h.  Any error leaves the history to k_replay_reg.
template <class LY, class M>
__device__ __attribute__((noinline)) void cls_p_scan(const Slice& S, const GAS cdr_wf_desc* dh,
                                                      const GAS cdr_wf_caps* ch, GAS cdr_exec_info* xh,
                                                      GAS cdr_repl_state* rh, GAS cdr_vh_item* vh_all, const M& cl,
                                                      uint32_t h, uint32_t lane) {
  constexpr uint32_t RL0 = LY::L0, MB = LY::MB;
  const uint32_t lenh = __builtin_amdgcn_readfirstlane((uint32_t)dh->ev_len);
  const uint32_t bld = __builtin_amdgcn_readfirstlane(dh->builder);
  const bool hRS = bld == CDR_BUILDER_2DC, hVH = bld == CDR_BUILDER_NDC;
  const uint32_t vcap = __builtin_amdgcn_readfirstlane(ch->vh_cap);
  GAS cdr_vh_item* vhh = vh_all + ch->vh_off;
  bool bad = lenh == 0;
  int64_t pid = 0, pver = 0, cfid = 0;  // last event of the previous chunk; the last call's first id
  uint32_t nvh = 0, cfk = 0, ncalls = 0, rsm = 0;
  // chunk k0's columns: its events' type flags, the next event's, ids and versions — the
  // next chunk's are in flight while this one is scanned (copied out through opaque moves)
  auto pload = [&](uint32_t k0, uint32_t& tf, uint32_t& tfn, int64_t& id, int64_t& ver) {
    const uint32_t k = k0 + lane;
    const uint32_t o8 = (k < lenh ? k * CDR_ROW_BYTES : OOB_BIT) + h * 8u, o4 = o8 - h * 4u;
    const uint32_t o4n = ((k + 1 < lenh) ? (k + 1) * CDR_ROW_BYTES : OOB_BIT) + h * 4u;
    tf = bld32(S.r, o4, S.col(CDR_COL_TYPE_FLAGS));
    tfn = bld32(S.r, o4n, S.col(CDR_COL_TYPE_FLAGS));
    id = bld64(S.r, o8, S.col(CDR_COL_EVENT_ID));
    ver = bld64(S.r, o8, S.col(CDR_COL_VERSION));
  };
  uint32_t n_tf, n_tfn;
  int64_t n_id, n_ver;
  pload(0, n_tf, n_tfn, n_id, n_ver);
  for (uint32_t k0 = 0; k0 < lenh && !bad; k0 += CDR_SLICE_WIDTH) {
    const uint32_t k = k0 + lane;
    const bool on = k < lenh;
    const uint32_t tf = mov32(n_tf), tfn = mov32(n_tfn);
    const int64_t id = mov64(n_id), ver = mov64(n_ver);
    pload(k0 + CDR_SLICE_WIDTH, n_tf, n_tfn, n_id, n_ver);
    int64_t pi = (int64_t)dpp64<DPP_WAVE_SHR1>((uint64_t)id), pv = (int64_t)dpp64<DPP_WAVE_SHR1>((uint64_t)ver);
    pi = lane == 0 ? pid : pi;
    pv = lane == 0 ? pver : pv;
    const bool bf = on && ((tf & CDR_SEF_BATCH_FIRST) || k == 0);
    const bool cend = on && (k + 1 == lenh || (tfn & CDR_SEF_BATCH_FIRST));  // a call's last event
    const uint64_t bfm = __builtin_amdgcn_ballot_w64(bf);
    ncalls += (uint32_t)__builtin_popcountll(bfm);
    if (bfm) {
      const uint32_t hb = 63u - (uint32_t)__builtin_clzll(bfm);
      cfk = k0 + hb;
      cfid = rdl64(id, hb);
    }
    if (hRS) {  // ClusterNameForFailoverVersion of each call's last event; last writer per cluster
      const int src = cend ? cluster_for_version(cl, ver) : 0;
      bad |= __builtin_amdgcn_ballot_w64(cend && src < 0) != 0;
#pragma unroll
      for (int c = 0; c < (int)CDR_REG_NCL; c++) {
        const uint64_t m = __builtin_amdgcn_ballot_w64(cend && src == c && c != cl.current_cluster);
        if (m) {
          const int hb = 63 - __builtin_clzll(m);
          const int64_t lv = rdl64(ver, (uint32_t)hb), li = rdl64(id, (uint32_t)hb);
          if (lane == 0) {
            rs(RL0 + 2u * (uint32_t)c, h, (uint32_t)lv);
            rs(RL0 + 2u * (uint32_t)c + 1, h, (uint32_t)li);
          }
          rsm |= 1u << c;
        }
      }
    }
    if (hVH) {  // stateBuilder.go:134-154 over the chunk
      const bool first = k == 0;
      const bool newitem = on && (first || ver > pv);
      const bool e = on && ((id < 0) | ((ver < 0) & (ver != CDR_EMPTY_VERSION)) | (!first & (ver < pv)) |
                            (!first & (id <= pi)));
      const uint64_t nm = __builtin_amdgcn_ballot_w64(newitem);
      const uint32_t before = nvh + (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(nm >> 32),
                                                                        __builtin_amdgcn_mbcnt_lo((uint32_t)nm, 0u));
      const bool capx = newitem && before >= vcap;
      bad |= __builtin_amdgcn_ballot_w64(e || capx) != 0;
      if (newitem && !first && !capx) gput(vhh + (before - 1), cdr_vh_item{pi, pv});  // closes the open item
      nvh += (uint32_t)__builtin_popcountll(nm);
    }
    const int last = (int)((lenh - 1 - k0) < 63u ? (lenh - 1 - k0) : 63u);
    pid = rdl64(id, (uint32_t)last);
    pver = rdl64(ver, (uint32_t)last);
  }
  if (!bad) {  // end of the last call
    const int64_t x_next = pid + 1;
    if (dh->parent < 0 && dh->expected_next_event_id != 0 && x_next != dh->expected_next_event_id) bad = true;
    if (!bad && lane == 0) {
      if (nvh) gput(vhh + (nvh - 1), cdr_vh_item{pid, pver});
      xh->last_first_event_id = cfid;  // stateBuilder.go:603 of the last call
      xh->next_event_id = x_next;
      xh->last_event_task_id = bld64(S.r, (lenh - 1) * CDR_ROW_BYTES + h * 8u, S.col(CDR_COL_TASK_ID));
      if (hRS) {
        rh->current_version = pver;
        rh->last_write_version = pver;
        rh->last_write_event_id = pid;
        for (uint32_t c = 0; c < CDR_MAX_CLUSTERS; c++) {
          const bool on = c < CDR_REG_NCL && ((rsm >> c) & 1u);
          const uint32_t pw = RL0 + 2u * (c < CDR_REG_NCL ? c : 0u);
          rh->lri_version[c] = on ? (int64_t)rl(pw, h) : 0;
          rh->lri_last_event_id[c] = on ? (int64_t)rl(pw + 1, h) : 0;
        }
        rh->lri_mask = rsm;
        rh->present = 1;
      }
    }
  }
  if (lane == 0) {
    rs(MB + LY::MB_CFK, h, cfk);
    rs(MB + LY::MB_NCALLS, h, ncalls);
    rs(MB + LY::MB_P, h, nvh | (bad ? 0x80000000u : 0u));
  }
}

// PAR: one workgroup of four waves per slice (CDR_SLICE_PAR: the batch's long histories),
// the loops at once instead of one after another — wave 0 P (as scans) then T, wave 1 W
// (as scans, histories round-robin), wave 2 A, wave 3 X (which waits, lane by lane, until
// the W wave has passed the history index of its event, so that the reset points it
// settles exist) — then wave 1 assembles the ExecutionInfo record and the result from the
// mailbox.  A slice's critical path is then its longest loop, not their sum.
// TASKS (non-PAR only): the instantiation that also emits the stateBuilder's transfer / timer
// tasks (stateBuilder.go:613-804).  Each class loop stages its tasks — in history order within
// the class, keyed by the event's history index — into a list of its own per entry
// (cdr_launch.tstage: 32-B records, list c of entry w at 4 (xfer_off + ttask_off) + c (xfer_cap +
// ttask_cap)) through a wave-wide LDS pool, and the entry's header (cdr_launch.thead: the four
// counts | valid << 31, TaskList) says the lists are complete; k_tasks_merge then merges the four
// lists by history index into the entry's task slices — the order stateBuilder appends them in.
template <int NA, int NT, int NX, uint32_t SFLAG, int WPE = CDR_WPE_CLS, bool PAR = false, bool TASKS = false>
__global__ __launch_bounds__(PAR ? 4 * CDR_SLICE_WIDTH : CDR_SLICE_WIDTH)
    __attribute__((amdgpu_waves_per_eu(WPE, 8))) void k_replay_cls(cdr_launch L) {
  (void)L;  // read through KA()
  static_assert(!(PAR && TASKS), "the PAR slices' tasks come from k_replay_reg<TASKS>");
  static_assert(!TASKS || CDR_CLS_PEEL_STARTED, "TASKS: Started is the peeled first W row");
  typedef ClsLds<NA, NT, NX, PAR> LY;
  constexpr uint32_t RP0 = LY::P0, RL0 = LY::L0, RA0 = LY::A0, RT0 = LY::T0, RC0 = LY::C0, RR0 = LY::R0,
                     RG0 = LY::G0, MB = LY::MB;
  // records written by the wave together (coop_put): through the loops' shared region (free
  // between the P and A loops: the ExecutionInfo halves) or the whole layout (the result, at
  // the end); words per pass so that (words + 1) * 65 8-B words fit
  constexpr uint32_t CWX_ = (LY::W - LY::Q0) * CDR_SLICE_WIDTH / 2 / 65 - 1, CWX = CWX_ < 16 ? CWX_ : 16;
  constexpr uint32_t CWR_ = LY::W * CDR_SLICE_WIDTH / 2 / 65 - 1, CWR = CWR_ < 7 ? CWR_ : 7;
  constexpr uint32_t LWX = LY::Q0 * CDR_SLICE_WIDTH / 2;  // the shared region's first 8-B word
  static_assert(PAR || (CWX >= 2 && CWR >= 2 && LY::Q0 % 2 == 0), "coop_put room");
  const uint32_t s = blockIdx.x + KA()->s0;
  const uint32_t lane = threadIdx.x & (CDR_SLICE_WIDTH - 1);
  const uint32_t role = PAR ? __builtin_amdgcn_readfirstlane(threadIdx.x / CDR_SLICE_WIDTH) : 0u;
#if CDR_PAR_PRIO
  if constexpr (PAR) __builtin_amdgcn_s_setprio(CDR_PAR_PRIO);  // issue priority over co-resident waves
#endif
  {  // count this workgroup in (a vector atomic; the launcher's gate)
    uint32_t* ps = KA()->pstart;
    if (ps && threadIdx.x == 0) __hip_atomic_fetch_add(ps, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (s >= KA()->B.ev.n_slices) return;
  if (!(__builtin_amdgcn_readfirstlane(KA()->B.ev.slice_flags[s]) & SFLAG)) return;
  const uint64_t row0_ = KA()->B.ev.slice_row0[s];
  const uint64_t row0 = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(row0_ >> 32)) << 32) |
                        __builtin_amdgcn_readfirstlane((uint32_t)row0_);
  Slice S;  // the original block (history order)
  S.elems = __builtin_amdgcn_readfirstlane(KA()->B.ev.slice_len[s]) * CDR_SLICE_WIDTH;
  S.r = __builtin_amdgcn_make_buffer_rsrc((void*)(KA()->B.ev.slab + row0 * CDR_ROW_BYTES), (short)0,
                                          (int)(S.elems * CDR_EL_BYTES), 0x00020000);
  S.l4 = lane * 4u;
  uint32_t MR[4];
#pragma unroll
  for (uint32_t j = 0; j < 4; j++) MR[j] = __builtin_amdgcn_readfirstlane(KA()->B.cls_rows[4ull * s + j]);
  const uint32_t MW = MR[0], MA = MR[1], MT = MR[2], MX = MR[3];
  const uint64_t crow_ = KA()->B.cls_row0[s];
  const uint64_t crow = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(crow_ >> 32)) << 32) |
                        __builtin_amdgcn_readfirstlane((uint32_t)crow_);
  Slice C;  // the class-sorted block
  C.elems = (MW + MA + MT + MX) * CDR_SLICE_WIDTH;
  C.r = __builtin_amdgcn_make_buffer_rsrc((void*)(KA()->B.cls_slab + crow * CDR_ROW_BYTES), (short)0,
                                          (int)(C.elems * CDR_EL_BYTES), 0x00020000);
  C.l4 = lane * 4u;
  const int32_t wl = KA()->B.ev.lane_wf[(uint64_t)s * CDR_SLICE_WIDTH + lane];
  const int32_t w0 = (wl >= 0 && KA()->B.skip && KA()->B.skip[wl]) ? -1 : wl;  // a masked entry: an empty lane
  if (!PAR && w0 < 0) return;
  const bool nolane = w0 < 0;  // PAR: an empty lane still reaches the workgroup barrier
  const int32_t w = nolane ? 0 : w0;
  // a solo PAR slice (one history, in lane 0: the batch's histories of CDR_PAR_SOLO_LEN
  // events and more, host.cpp): its A, T and X classes replay in wave form — one event per
  // step, each pending table spread over the lanes (slot j in lane j: a lookup is a compare
  // and a ballot, a timer pick a wave argmin) — instead of one lane walking them
  const bool solo = PAR && __builtin_amdgcn_ballot_w64(w0 >= 0) == 1ull;
  static_assert(NA <= 16 && NT <= 16 && NX <= 16, "wave-form tables fit the first 16 lanes");
#define B_ (KA()->B)
#define O_ (KA()->O)
#define D (gp(B_.wfs)[w])
#define CP (gp(B_.caps)[w])
#define X (gp(O_.exec) + w)
#define RS (gp(O_.repl) + w)
#define vh (gp(O_.vh) + CP.vh_off)
#define rp (gp(O_.rp) + CP.rp_off)
#define sa (gp(O_.sa) + CP.sa_off)
#define SEL(c, a, b) ((c) ? (a) : (b))
  const uint32_t len = (uint32_t)D.ev_len;
  const uint32_t builder = D.builder;
  const uint32_t EU = B_.empty_uuid;
  const bool isRS = builder == CDR_BUILDER_2DC;
  const bool isVH = builder == CDR_BUILDER_NDC;
  const uint32_t srows = S.elems / CDR_SLICE_WIDTH;
  auto ev64 = [&](uint32_t kk, int c) { return bld64(S.r, el8(kk, len, lane), S.col(c)); };
  auto ev32 = [&](uint32_t kk, int c) { return bld32(S.r, el8(kk, len, lane) - S.l4, S.col(c)); };
  bool retry = nolane || len == 0;  // the empty history's error comes from k_replay_reg
  // ---- TASKS: staged task records (w0 = type | timeout type << 8 | timer << 12 | history index
  // << 32, w1 = event id, w2 = visibility time / arena offset of an external initiation's
  // attributes, then the staging index) appended to the wave's LDS pool at the wave-wide prefix
  // of the emitting lanes; every staging call runs in wave-uniform control flow (n_pool is
  // advanced by the wave), and the pool is flushed at a step end once the next step could
  // overflow it (<= 2 records per lane a step) — so few steps drain the prefetch ring
  constexpr uint32_t TQ_BASE = (uint32_t)(LY::bytes / 8), TQ_CAP = CDR_CLS_TBUF * CDR_SLICE_WIDTH;
  uint32_t n_pool = 0;
  uint32_t t_n[4] = {0u, 0u, 0u, 0u};
  const uint64_t t_sbase = TASKS ? 4ull * (CP.xfer_off + CP.ttask_off) : 0ull;
  const uint32_t t_scap = TASKS ? CP.xfer_cap + CP.ttask_cap : 0u;
  const uint64_t t_rows = TASKS ? KA()->trows : 0ull;
  auto stage = [&](uint32_t cl, bool c, uint32_t type, uint32_t tt, uint32_t kind, uint32_t kk, int64_t eid, int64_t v)
      __attribute__((always_inline)) {
    if constexpr (TASKS) {
      // a record past the entry's list or the staging buffer (capacities that do not bound the
      // history's tasks): the entry is handed on, and k_replay_reg<TASKS> reports it
      const bool fit = t_n[cl] < t_scap && t_sbase + (uint64_t)cl * t_scap + t_n[cl] < t_rows;
      retry = retry || (c && !fit);
      c = c && fit;
      const uint64_t m = __builtin_amdgcn_ballot_w64(c);
      const uint32_t pos = n_pool + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      if (c) {
        uint64_t* P = cdr_lds + TQ_BASE + 4u * pos;
        P[0] = (uint64_t)(type | (tt << 8) | (kind << 12)) | ((uint64_t)kk << 32);
        P[1] = (uint64_t)eid;
        P[2] = (uint64_t)v;
        P[3] = t_sbase + (uint64_t)cl * t_scap + t_n[cl];
      }
      t_n[cl] += c ? 1u : 0u;
      n_pool = __builtin_amdgcn_readfirstlane(n_pool + (uint32_t)__builtin_popcountll(m));
    }
  };
  // the pool out to the staging lists: a lane per 16-B half of a 32-B record
  auto tq_flush = [&]() __attribute__((always_inline)) {
    if constexpr (TASKS) {
      const uint64_t em = __builtin_amdgcn_read_exec();
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(em >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)em, 0u));
      const uint32_t na = (uint32_t)__builtin_popcountll(em);
      __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): every lane's records before any lane reads them
      __builtin_amdgcn_wave_barrier();
      typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
      GAS u64x2* const st = (GAS u64x2*)KA()->tstage;
      for (uint32_t i = rank; i < 2u * n_pool; i += na) {
        const uint32_t r = i >> 1, q = i & 1u;
        const uint64_t* P = cdr_lds + TQ_BASE + 4u * r;
        u64x2 v2;
        v2.x = P[2u * q];
        v2.y = P[2u * q + 1u];
        __builtin_nontemporal_store(v2, st + 2ull * P[3] + q);
      }
      __builtin_amdgcn_s_waitcnt(0xC07F);  // the pool's reads before the next records land
      __builtin_amdgcn_wave_barrier();
      n_pool = 0;
    }
  };
  // a class loop's step end: flush (and drain) when the next step could overflow the pool
  auto tq_step = [&]() __attribute__((always_inline)) {
    if constexpr (TASKS) {
      if (n_pool + 2u * CDR_SLICE_WIDTH > TQ_CAP) {
        tq_flush();
        vmdrain();
      }
    }
  };
  if constexpr (PAR) {  // the W wave's progress words start at 0 before any X wave reads them
    if (role == 1) {
      rs(MB + LY::MB_WPROG, lane, 0u);
      rs(MB + LY::MB_WNRP, lane, 0u);
    }
    wg_sync();
  }
#ifdef CDR_PAR_PROF  // profiling variant only: each wave's time to its final barrier (us)
  const uint64_t prof_t0 = __builtin_amdgcn_s_memrealtime();
  const uint32_t prof_start = (uint32_t)(prof_t0 / 100u);  // the slice's start (us, absolute)
#define PAR_PROF_MARK() \
  if (lane == 0) rs(LY::PF + role, 0, (uint32_t)((__builtin_amdgcn_s_memrealtime() - prof_t0) / 100u))
#else
#define PAR_PROF_MARK() (void)0
#endif

  // ================================================================ P: history order
  int64_t prev_id = 0, prev_ver = 0, call_first_id = 0;
  uint32_t call_first_k = 0, n_calls = 0, rs_mask = 0, n_vh = 0;
  int64_t vh_last_id = 0, vh_last_ver = 0;
  if constexpr (PAR) {
    if (role == 0) {  // the P loop as scans: one history at a time, 64 of its events per step
      for (uint32_t h = 0; h < CDR_SLICE_WIDTH; h++) {
        const int32_t wh = __builtin_amdgcn_readlane(w0, h);
        if (wh < 0) continue;
        cls_p_scan<LY>(S, gp(B_.wfs) + wh, gp(B_.caps) + wh, gp(O_.exec) + wh, gp(O_.repl) + wh, fast_out_vh(O_), B_.cluster,
                       h, lane);
      }
    }
  }
  if (!PAR) {
    const uint32_t vh_cap = CP.vh_cap;
    bool done = retry;
    // ring of PD history rows in flight: type_flags, and the id / version the delta bits
    // do not imply (as k_replay_fast's ring: whole groups, opaque copies)
    constexpr int PD = PAR ? CDR_CLS_PDEPTH_PAR : CDR_CLS_PDEPTH;
    auto pid = [&](uint32_t kk, uint32_t tf) {
      return bld64(S.r, el8(kk, len, lane) | ((tf & CDR_SEF_ID_NEXT) ? OOB_BIT : 0u), S.col(CDR_COL_EVENT_ID));
    };
    auto pver = [&](uint32_t kk, uint32_t tf) {
      return bld64(S.r, el8(kk, len, lane) | ((tf & CDR_SEF_VER_SAME) ? OOB_BIT : 0u), S.col(CDR_COL_VERSION));
    };
    uint32_t PF[PD], PT[PD];
    int64_t PI[PD], PV[PD];
    int64_t cv_ver = (int64_t)0x8000000000000000ll;  // the last version mapped to a cluster, and its cluster
    int cv_src = 0;
#pragma unroll
    for (int j = 0; j < PD; j++) PF[j] = load_tf(S, el8(j, len, lane));
#pragma unroll
    for (int j = 0; j < PD; j++) {
      PI[j] = pid(j, PF[j]);
      PV[j] = pver(j, PF[j]);
    }
#pragma unroll
    for (int j = 0; j < PD; j++) PT[j] = load_tf(S, el8(j + PD, len, lane));
    auto pstep = [&](const uint32_t k, const uint32_t tf, const int64_t li, const int64_t lv)
                     __attribute__((always_inline)) {
      done |= k >= len;
      const int64_t id = (tf & CDR_SEF_ID_NEXT) ? (int64_t)((uint64_t)prev_id + 1u) : li;
      const int64_t ver = (tf & CDR_SEF_VER_SAME) ? prev_ver : lv;
      // call boundary (stateBuilder.go:603-604; mutableStateBuilder.go:561-581)
      const bool bf = !done && ((tf & CDR_SEF_BATCH_FIRST) || k == 0);
      const bool end_call = bf && k > 0;
      if (__builtin_amdgcn_ballot_w64(isRS && end_call)) {
        // ClusterNameForFailoverVersion of the call's version: a history's versions change
        // only at failovers, so the last answer is kept (the kernarg cluster map and the
        // 64-bit modulo only for a new version)
        const bool fresh = isRS && end_call && prev_ver != cv_ver;
        if (__builtin_amdgcn_ballot_w64(fresh)) {
          const int sn = fresh ? cluster_for_version(B_.cluster, prev_ver) : 0;
          cv_src = fresh ? sn : cv_src;
          cv_ver = fresh ? prev_ver : cv_ver;
        }
        const int src = (isRS && end_call) ? cv_src : 0;
        retry |= isRS && end_call && src < 0;  // ClusterNameForFailoverVersion panic
        const bool lri = isRS && end_call && src >= 0 && src != B_.cluster.current_cluster;
        if (lri) {
          rs(RL0 + 2u * (uint32_t)src, lane, (uint32_t)prev_ver);
          rs(RL0 + 2u * (uint32_t)src + 1, lane, (uint32_t)prev_id);
        }
        rs_mask |= lri ? 1u << src : 0u;
      }
      n_calls += bf ? 1u : 0u;
      call_first_id = SEL(bf, id, call_first_id);
      call_first_k = SEL(bf, k, call_first_k);
      prev_id = SEL(done, prev_id, id);
      prev_ver = SEL(done, prev_ver, ver);
      if (isVH) {  // version prelude (stateBuilder.go:134-154), its decision tree as selects
        const bool has = n_vh != 0;
        const bool newitem = !has | (ver > vh_last_ver);
        const bool bad = (id < 0) | ((ver < 0) & (ver != CDR_EMPTY_VERSION)) | (has & (ver < vh_last_ver)) |
                         (has & (id <= vh_last_id)) | (newitem & (n_vh >= vh_cap));
        retry |= !done && bad;
        const bool go = !done && !bad;
        const bool add = go && newitem;
        const bool put = add && has;
        if (__builtin_amdgcn_ballot_w64(put)) {  // a new item closes the previous one (rare)
          if (put) gput(vh + (n_vh - 1), cdr_vh_item{vh_last_id, vh_last_ver});
          vmdrain();
        }
        n_vh += add ? 1u : 0u;
        vh_last_ver = SEL(add, ver, vh_last_ver);
        vh_last_id = SEL(go, id, vh_last_id);
      }
      done |= retry;
    };
    for (uint32_t k = 0; k < srows; k += PD) {
      if (__builtin_amdgcn_ballot_w64(!done) == 0) break;
#pragma unroll
      for (int j = 0; j < PD; j++) {
        const uint32_t tf = mov32(PF[j]);
        const int64_t li = mov64(PI[j]), lv = mov64(PV[j]);
        const uint32_t tn = mov32(PT[j]);
        PF[j] = tn;
        PI[j] = pid(k + j + PD, tn);
        PV[j] = pver(k + j + PD, tn);
        PT[j] = load_tf(S, el8(k + j + 2 * PD, len, lane));
        pstep(k + j, tf, li, lv);
      }
    }
    if (!retry) {  // end of the last call
      if (isRS) {
        const int src = cluster_for_version(B_.cluster, prev_ver);
        if (src < 0) {
          retry = true;
        } else if (src != B_.cluster.current_cluster) {
          rs(RL0 + 2u * (uint32_t)src, lane, (uint32_t)prev_ver);
          rs(RL0 + 2u * (uint32_t)src + 1, lane, (uint32_t)prev_id);
          rs_mask |= 1u << src;
        }
      }
      const int64_t x_next_event = prev_id + 1;
      // nDCStateRebuilder.go:139-143 (its error code comes from k_replay_reg)
      if (D.parent < 0 && D.expected_next_event_id != 0 && x_next_event != D.expected_next_event_id) retry = true;
      // P's share of the records (the W loop writes the rest of ExecutionInfo; an entry
      // handed on later is rewritten whole by k_replay_reg)
      if (n_vh) gput(vh + (n_vh - 1), cdr_vh_item{vh_last_id, vh_last_ver});
      X->last_first_event_id = call_first_id;  // stateBuilder.go:603 of the last call
      X->next_event_id = x_next_event;
      X->last_event_task_id = ev64(len - 1, CDR_COL_TASK_ID);  // :155
      if (isRS) {
        RS->current_version = prev_ver;
        RS->last_write_version = prev_ver;
        RS->last_write_event_id = prev_id;
        for (uint32_t c = 0; c < CDR_MAX_CLUSTERS; c++) {
          const bool on = c < CDR_REG_NCL && ((rs_mask >> c) & 1u);
          const uint32_t pw = RL0 + 2u * (c < CDR_REG_NCL ? c : 0u);
          RS->lri_version[c] = on ? (int64_t)rl(pw, lane) : 0;
          RS->lri_last_event_id[c] = on ? (int64_t)rl(pw + 1, lane) : 0;
        }
        RS->lri_mask = rs_mask;
        RS->present = 1;
      }
    }
  }

  // ================================================================ W: decisions, workflow
  uint32_t n_rp = 0, n_sa = 0;
  uint32_t wwhy = 0;  // PAR: the checks that handed the entry on (the CLS_RETRY result's fail_index)
  bool newrun_applied = false;
  uint32_t n_act = 0, n_tim = 0, n_chi = 0, n_can = 0, n_sig = 0;
  if (!PAR || role == 1) {
    uint32_t x_flags = 0, cks_ok = 0, dreq = EU, ld = 0, close_k = RNONE, can_k = RNONE, last_wk = 0;
    int64_t x_last_processed = CDR_EMPTY_EVENT_ID, dv = CDR_EMPTY_VERSION, dsched = CDR_EMPTY_EVENT_ID,
            dstart = CDR_EMPTY_EVENT_ID, datt = 0, dst_ts = 0, dsc_ts = 0, dorig_ts = 0;
    int32_t x_dt_timeout_value = 0, x_state = CDR_STATE_CREATED, x_close = CDR_CLOSE_NONE, x_signals = 0, dto = 0;
    int64_t curv = D.failover_version, wver = 0;
    bool any_w = false;
    const bool want_ld = O_.last_decision != nullptr;
    // PAR: lastDecision as the decision fields right after the history's last source event
    // (scheduled / started / transient) and that event's call (ld_cfk); it survives iff that
    // call is the entry's last (the lane loop's per-call reset, stateBuilder.go:126)
    int64_t s_dv = 0, s_dsched = 0, s_dstart = 0, s_datt = 0, s_dsc = 0, s_dst = 0, s_dorig = 0;
    uint32_t s_dreq = 0, ld_cfk = 0;
    int32_t s_dto = 0;
    // PAR, a solo slice: its search attributes live in the lanes (slot j in lane j) while the
    // W scan runs — an upsert is one gather of its rows and a ballot per row instead of a
    // global read-modify-write round trip per row; written out once after the scan
    uint32_t sa_k = 0, sa_v = 0;
    if constexpr (PAR) {
      // ---- the W loop as scans (the north star's recast, as cls_p_scan does for P): one
      // history at a time, 64 of its W events per step, one per lane.  Every field the loop
      // keeps is a last writer (decision fields, LastProcessedEvent, checksum, version), an
      // affine map (Attempt: set, or +1 at a counted DecisionTaskFailed / TimedOut), a count
      // (signals) or a rare serial step (closes, continue-as-new, upserts, new reset points),
      // so a chunk costs ballots, one gather per field read inside the chunk and readlanes
      // for the carry.  Histories are taken round-robin, one chunk each, so that every lane
      // of the X wave sees W progress; lane h keeps history h's state (the lane loop's
      // registers), read and written back with readlane / a lane select around each chunk.
      const uint64_t LT = lane ? (~0ull >> (64u - lane)) : 0ull;  // lanes below this one
      const uint64_t LE = LT | (1ull << lane);
      uint32_t wcnt = 0;  // lane h: history h's W events (its W rows before the padding)
      if (!retry) {
        uint32_t lo = 0, hi = MW;
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          const uint32_t t = bld32<CDR_NT_CLS>(C.r, mid * CDR_ROW_BYTES + lane * 4u, C.col(CDR_COL_TYPE_FLAGS)) & 0xFFu;
          if (t != CDR_EV_PAD) lo = mid + 1;
          else hi = mid;
        }
        wcnt = lo;
      }
      const int64_t now = B_.now_ns;
      // the chunk after (h, r) in the round-robin order, or h = 64 (none)
      auto wnext = [&](uint32_t h, uint32_t r, uint32_t& nh, uint32_t& nr) {
        const uint64_t m0 = __builtin_amdgcn_ballot_w64(wcnt > r * CDR_SLICE_WIDTH) & above((int)h);
        const uint64_t m1 = __builtin_amdgcn_ballot_w64(wcnt > (r + 1) * CDR_SLICE_WIDTH);
        nh = m0 ? (uint32_t)__builtin_ctzll(m0) : (m1 ? (uint32_t)__builtin_ctzll(m1) : 64u);
        nr = m0 ? r : r + 1;
      };
      uint32_t ch = 64, cr = 0;
      {
        const uint64_t m = __builtin_amdgcn_ballot_w64(wcnt > 0);
        ch = m ? (uint32_t)__builtin_ctzll(m) : 64u;
      }
      WScanRow Qn = load_wscan(C, ch < 64 ? lane : MW, MW, ch < 64 ? ch : 0u);
      while (ch < 64) {
        const WScanRow q = wscan_take(Qn);
        uint32_t nh, nr;
        wnext(ch, cr, nh, nr);
        Qn = load_wscan(C, nh < 64 ? nr * CDR_SLICE_WIDTH + lane : MW, MW, nh < 64 ? nh : 0u);
        const uint32_t h = ch, r = cr;
        ch = nh;
        cr = nr;
        const uint32_t wn = rdl(wcnt, h);
        if (wn <= r * CDR_SLICE_WIDTH) continue;  // handed on since this chunk was loaded
        const bool me = lane == h;
        const int32_t wh = (int32_t)rdl((uint32_t)w0, h);
        const GAS cdr_wf_desc* Dh = gp(B_.wfs) + wh;
        const GAS cdr_wf_caps* CPh = gp(B_.caps) + wh;
        const uint32_t bldh = __builtin_amdgcn_readfirstlane(Dh->builder);
        const bool hRS = bldh == CDR_BUILDER_2DC, hVH = bldh == CDR_BUILDER_NDC;
        // history h's carry (uniform)
        uint32_t u_flags = rdl(x_flags, h), u_cks = rdl(cks_ok, h), u_dreq = rdl(dreq, h), u_close_k = rdl(close_k, h),
                 u_can_k = rdl(can_k, h), u_last_wk = rdl(last_wk, h), u_nrp = rdl(n_rp, h), u_nsa = rdl(n_sa, h),
                 u_ld = rdl(ld, h), u_ldcfk = rdl(ld_cfk, h);
        bool u_anyw = rdl(any_w ? 1u : 0u, h) != 0, u_newrun = rdl(newrun_applied ? 1u : 0u, h) != 0;
        int32_t u_dtv = (int32_t)rdl((uint32_t)x_dt_timeout_value, h), u_state = (int32_t)rdl((uint32_t)x_state, h),
                u_close = (int32_t)rdl((uint32_t)x_close, h), u_sig = (int32_t)rdl((uint32_t)x_signals, h),
                u_dto = (int32_t)rdl((uint32_t)dto, h);
        int64_t u_lp = rdl64(x_last_processed, h), u_dv = rdl64(dv, h), u_dsched = rdl64(dsched, h),
                u_dstart = rdl64(dstart, h), u_datt = rdl64(datt, h), u_dst = rdl64(dst_ts, h), u_dsc = rdl64(dsc_ts, h),
                u_dorig = rdl64(dorig_ts, h), u_curv = rdl64(curv, h), u_wver = rdl64(wver, h);
        bool rty = false, snap = false;
        uint32_t why = 0;  // which check handed the history on (diagnostic: the result's fail_index)
        int64_t v_dv = 0, v_dsched = 0, v_dstart = 0, v_datt = 0, v_dsc = 0, v_dst = 0, v_dorig = 0;
        uint32_t v_dreq = 0;
        int32_t v_dto = 0;

        const uint32_t type = q.tf & 0xFFu;
        const bool act = r * CDR_SLICE_WIDTH + lane < wn;
        const uint64_t mAct = __builtin_amdgcn_ballot_w64(act);
        const uint64_t tb = (act && type < 64) ? (1ull << type) : 0ull;
        const uint32_t k = (uint32_t)q.ann & 0xFFFFFu, cfk = k - (((uint32_t)q.ann >> 20) & 0xFFFu);
        const uint32_t xd = (uint32_t)(q.ann >> 32);
        const int64_t ver = q.ver;
        auto M = [&](uint64_t types) { return __builtin_amdgcn_ballot_w64((tb & types) != 0); };
        const uint64_t mSCH = M(CDR_TB(CDR_EV_DT_SCHEDULED)), mDST = M(CDR_TB(CDR_EV_DT_STARTED)),
                       mDC = M(CDR_TB(CDR_EV_DT_COMPLETED)), mDF = M(RG_DTFAIL), mWS = M(CDR_TB(CDR_EV_WF_STARTED)),
                       mCL = M(RG_CLOSE), mCAN = M(CDR_TB(CDR_EV_WF_CONTINUED_AS_NEW)),
                       mUPS = M(CDR_TB(CDR_EV_UPSERT_SA));
        { const bool b_ = __builtin_amdgcn_ballot_w64(act && type >= CDR_EV_NUM_TYPES) != 0; rty |= b_; why |= b_ ? 1u : 0u; }  // stateBuilder.go:597-599
        // WorkflowExecutionStarted: replayed here as the history's first W event only (any
        // other, and a second one, go to k_replay_reg); it sets the carry the chunk starts from
        if (mWS && !rty) {
          if (mWS != 1ull || r != 0) {
            rty = true; why |= 2u;
          } else {  // stateBuilder.go:158-184 -> mutableStateBuilder.go:1639-1716
            const GAS cdr_attr_wf_started* a =
                gp((const cdr_attr_wf_started*)(B_.ev.arena + (uint64_t)rdl64(q.aux, 0)));
            const uint32_t af = a->flags;
            const bool f1 = (af & CDR_SF_HAS_PARENT_DOMAIN) && (af & CDR_SF_PARENT_DOMAIN_MISSING);
            const bool f2 = !f1 && !transition_ok(u_state, u_close, CDR_STATE_CREATED, CDR_CLOSE_NONE);
            if (f1 || f2) {
              rty = true; why |= 4u;
            } else {
              const int64_t ts0 = rdl64(q.ts, 0), id0 = rdl64(q.id, 0), ver0 = rdl64(ver, 0);
              GAS cdr_exec_info* Xh = gp(O_.exec) + wh;
              GAS cdr_reset_point* rph = fast_out_rp(O_) + CPh->rp_off;
              GAS cdr_kv* sah = out_sa(O_) + CPh->sa_off;
              uint32_t xf = u_flags;
              if (lane == 0) {
                Xh->domain_id = Dh->domain_id;
                Xh->workflow_id = Dh->workflow_id;
                Xh->run_id = Dh->run_id;
                Xh->create_request_id = Dh->request_id;
                Xh->task_list = a->task_list;
                Xh->workflow_type = a->workflow_type;
                Xh->workflow_timeout = a->exec_timeout_s;
                Xh->cron_schedule = a->cron_schedule;
                Xh->attempt = a->attempt;
                Xh->initiated_id = (af & CDR_SF_HAS_PARENT_INITIATED) ? a->parent_initiated_id : CDR_EMPTY_EVENT_ID;
                Xh->parent_domain_id = (af & CDR_SF_HAS_PARENT_DOMAIN) ? a->parent_domain_id : 0u;
                Xh->parent_workflow_id = (af & CDR_SF_HAS_PARENT_EXEC) ? a->parent_workflow_id : 0u;
                Xh->parent_run_id = (af & CDR_SF_HAS_PARENT_EXEC) ? a->parent_run_id : 0u;
                Xh->expiration_time = a->expiration_ts;
              }
              xf |= a->expiration_ts != 0 ? CDR_XI_HAS_EXPIRATION : 0u;
              const bool retry_p = (af & CDR_SF_HAS_RETRY) != 0;
              xf |= retry_p ? CDR_XI_HAS_RETRY : 0u;
              if (lane == 0) {
                Xh->backoff_coefficient = retry_p ? a->backoff_coefficient : 0.0;
                Xh->expiration_seconds = retry_p ? a->retry_expiration_s : 0;
                Xh->initial_interval = retry_p ? a->retry_initial_s : 0;
                Xh->maximum_attempts = retry_p ? a->retry_max_attempts : 0;
                Xh->maximum_interval = retry_p ? a->retry_max_interval_s : 0;
                Xh->nonretriable = retry_p ? a->nonretriable : 0u;
              }
              // rolloverAutoResetPointsWithExpiringTime (:3184-3205)
              u_nrp = 0;
              xf &= ~CDR_XI_HAS_RESET_POINTS;
              if (af & CDR_SF_HAS_RESET_POINTS) {
                xf |= CDR_XI_HAS_RESET_POINTS;
                const int64_t expiring = ts0 + (int64_t)Dh->retention_days * 24ll * 3600ll * NS_PER_S;
                const uint32_t crun = a->continued_run_id, off = a->reset_points_off, cnt = a->reset_points_len;
                const uint32_t cap = CPh->rp_cap;
                rty |= cnt > cap;  // the points do not fit the slice: k_replay_reg reports it
                for (uint32_t qq = 0; qq < cnt && qq < cap && u_nrp < LY::NRP; qq++) {
                  cdr_reset_point pr = gget(gp(B_.rps) + (off + qq));
                  const uint32_t run = (pr.flags & CDR_RP_HAS_RUN_ID) ? pr.run_id : 0u;
                  if (run == crun) {
                    pr.flags |= CDR_RP_HAS_EXPIRING;
                    pr.expiring_time_nano = expiring;
                  }
                  if (lane == 0) gput(rph + u_nrp, pr);
                  if (lane == 0) {
                    rs(RP0 + 2 * u_nrp, h, (pr.flags & CDR_RP_HAS_CHECKSUM) ? pr.binary_checksum : 0u);
                    rs(RP0 + 2 * u_nrp + 1, h, RNONE);
                  }
                  u_nrp++;
                }
              }
              xf |= (af & CDR_SF_HAS_MEMO) ? CDR_XI_HAS_MEMO : 0u;
              if (lane == 0) Xh->memo = (af & CDR_SF_HAS_MEMO) ? a->memo : 0u;
              if (af & CDR_SF_HAS_SEARCH_ATTR) {
                u_nsa = 0;
                const uint32_t off = a->search_attr_off, cnt = a->search_attr_len, cap = CPh->sa_cap;
                rty |= cnt > cap;
                for (uint32_t qq = 0; qq < cnt && qq < cap && u_nsa < CDR_REG_NSA; qq++) {
                  const cdr_kv kv = gget(gp(B_.kvs) + (off + qq));
                  if (lane == 0) gput(sah + u_nsa, kv);
                  u_nsa++;
                }
                if (u_nsa) xf |= CDR_XI_HAS_SEARCH_ATTR;
                else xf &= ~CDR_XI_HAS_SEARCH_ATTR;
              }
              xf |= CDR_XI_STARTED | (hVH ? CDR_XI_VH_BRANCH : CDR_XI_HAS_BRANCH);
              uint64_t lo, hi;  // SetHistoryTree (:313-339)
              cdr_uuid(B_.uuid_seed, Dh->wf_key, CDR_UUID_BRANCH, id0, &lo, &hi);
              if (lane == 0) {
                Xh->branch_tree_id = Dh->run_id;
                Xh->branch_id_lo = lo;
                Xh->branch_id_hi = hi;
                if (hRS) (gp(O_.repl) + wh)->start_version = ver0;  // :182-184
              }
              vmdrain();
              if (solo) {  // the lane-held table starts from the rows just written
                sa_k = lane < u_nsa ? __hip_atomic_load(&(sah + lane)->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
                sa_v = lane < u_nsa ? __hip_atomic_load(&(sah + lane)->value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
              }
              u_flags = xf;
              u_cks = 0;
              u_dtv = a->task_timeout_s;
              u_state = CDR_STATE_CREATED;
              u_close = CDR_CLOSE_NONE;
              u_lp = CDR_EMPTY_EVENT_ID;
              u_dv = CDR_EMPTY_VERSION;
              u_dsched = CDR_EMPTY_EVENT_ID;
              u_dstart = CDR_EMPTY_EVENT_ID;
              u_dreq = EU;
              u_dto = 0;
            }
          }
        }
        if (!rty) {
          // state before each lane: open (Created / Running) until the chunk's first close /
          // continue-as-new (a failing one hands the entry on); currentVersion (NDC) is the
          // version of the last W event replayed while open (stateBuilder.go:134-154)
          const uint64_t mRare = mCL | mCAN;
          const bool copen = u_state == CDR_STATE_CREATED || u_state == CDR_STATE_RUNNING;
          const int fr = mRare ? (int)__builtin_ctzll(mRare) : 64;
          const int64_t verfr = rdl64(ver, fr < 64 ? (uint32_t)fr : 0u);
          const int64_t curv_l = copen ? ((int)lane <= fr ? ver : verfr) : u_curv;
          // Attempt: set by Scheduled (its attempt), Started / Completed / an uncounted failure
          // (0), +1 at a counted DecisionTaskFailed / TimedOut (mutableStateDecisionTaskManager.go:635-656)
          const bool isDF = (tb & RG_DTFAIL) != 0, isSCH = (tb & CDR_TB(CDR_EV_DT_SCHEDULED)) != 0,
                     isDST = (tb & CDR_TB(CDR_EV_DT_STARTED)) != 0;
          const bool inc = isDF && (type == CDR_EV_DT_FAILED || q.n != CDR_TIMEOUT_SCHEDULE_TO_START);
          const uint64_t mINC = __builtin_amdgcn_ballot_w64(inc);
          const uint64_t mSETA = mSCH | mDST | mDC | (mDF & ~mINC);
          const int64_t seta = isSCH ? q.aux : 0;
          const int ja = hbit(mSETA & LT);
          // (every gather runs on all lanes: a lane outside EXEC would not provide its value)
          const int64_t apre = from64(seta, ja, u_datt) + (int64_t)__builtin_popcountll(mINC & LT & above(ja));
          const int64_t na = inc ? apre + 1 : 0;
          const bool tr = isDF && na != 0;
          const uint64_t mTR = __builtin_amdgcn_ballot_w64(tr);
          { const bool b_ = __builtin_amdgcn_ballot_w64(tr && xd == XD_NONE) != 0; rty |= b_; why |= b_ ? 8u : 0u; }
          // each decision field's value at its writers (mutableStateDecisionTaskManager.go:143-279)
          const uint64_t mD = mSCH | mDST | mDC | mDF, mDSW = mSCH | mDC | mDF, mDOR = mSCH | mDF;
          const int64_t dsch_l = isSCH ? q.id : tr ? q.id - (int64_t)xd : (int64_t)CDR_EMPTY_EVENT_ID;
          // DecisionTaskStarted: the scheduled ID must be the pending decision's
          const int64_t dpre = from64(dsch_l, hbit(mDSW & LT), u_dsched);
          { const bool b_ = __builtin_amdgcn_ballot_w64(isDST && q.key != dpre) != 0; rty |= b_; why |= b_ ? 16u : 0u; }
          const int64_t dv_l = (isSCH || isDST) ? ver
                               : tr ? (hRS ? ver : (hVH ? curv_l : (int64_t)CDR_EMPTY_VERSION))
                                    : (int64_t)CDR_EMPTY_VERSION;
          const int64_t dstart_l = isDST ? q.id : (int64_t)CDR_EMPTY_EVENT_ID;
          const uint32_t dreq_l = isDST ? q.hh : EU;
          const int32_t dto_l = isSCH ? q.n : tr ? u_dtv : 0;
          const int64_t datt_l = isSCH ? q.aux : na;
          const int64_t dst_l = isDST ? q.ts : 0;
          const int64_t dsc_l = isSCH ? q.ts : (isDF && (tr || inc)) ? now : 0;
          const int64_t dorig_l = isSCH ? q.ts : 0;
          // lastDecision: the fields right after the chunk's last source event
          const uint64_t mLD = mSCH | mDST | mTR;
          if (mLD && !rty) {
            const int L = hbit(mLD);
            const uint64_t le = ~above(L);
            auto at = [&](uint64_t m, int64_t v, int64_t old) {
              const int j = hbit(m & le);
              return j < 0 ? old : rdl64(v, (uint32_t)j);
            };
            snap = true;
            v_dv = at(mD, dv_l, u_dv);
            v_dsched = at(mDSW, dsch_l, u_dsched);
            v_dstart = at(mD, dstart_l, u_dstart);
            v_dreq = (uint32_t)at(mD, (int64_t)dreq_l, (int64_t)u_dreq);
            v_dto = (int32_t)at(mDSW, (int64_t)dto_l, (int64_t)u_dto);
            v_datt = at(mSETA | mINC, datt_l, u_datt);
            v_dst = at(mD, dst_l, u_dst);
            v_dsc = at(mDSW, dsc_l, u_dsc);
            v_dorig = at(mDOR, dorig_l, u_dorig);
            const uint32_t src = ((mSCH >> L) & 1u) ? CDR_LD_SCHEDULED : ((mDST >> L) & 1u) ? CDR_LD_STARTED : CDR_LD_TRANSIENT;
            u_ld = ld_make(src, rdl(k, (uint32_t)L));
            u_ldcfk = rdl(cfk, (uint32_t)L);
          }
          // carry-out of the decision fields: each field's last writer in the chunk
          auto lastw = [&](uint64_t m, int64_t v, int64_t old) { return m ? rdl64(v, (uint32_t)hbit(m)) : old; };
          {
            const int ha = hbit(mSETA);
            u_datt = (ha >= 0 ? rdl64(seta, (uint32_t)ha) : u_datt) +
                     (int64_t)__builtin_popcountll(mINC & above(ha));
          }
          u_dv = lastw(mD, dv_l, u_dv);
          u_dsched = lastw(mDSW, dsch_l, u_dsched);
          u_dstart = lastw(mD, dstart_l, u_dstart);
          u_dreq = (uint32_t)lastw(mD, (int64_t)dreq_l, (int64_t)u_dreq);
          u_dto = (int32_t)lastw(mDSW, (int64_t)dto_l, (int64_t)u_dto);
          u_dst = lastw(mD, dst_l, u_dst);
          u_dsc = lastw(mDSW, dsc_l, u_dsc);
          u_dorig = lastw(mDOR, dorig_l, u_dorig);
          u_lp = lastw(mDC, q.aux, u_lp);  // LastProcessedEvent (:255-262)
          // addBinaryCheckSumIfNotExists (mutableStateBuilder.go:1798-1842): a Completed whose
          // checksum differs from the last one checked appends it unless the list holds it
          const uint32_t cks = (tb & CDR_TB(CDR_EV_DT_COMPLETED)) ? q.hh : 0u;
          const uint64_t mCK = __builtin_amdgcn_ballot_w64(cks != 0);
          const uint32_t cpre = from32(cks, hbit(mCK & LT), u_cks);
          const bool chk = cks != 0 && cks != cpre;
          if (__builtin_amdgcn_ballot_w64(chk) && !rty) {
            bool inl = false;
#pragma unroll
            for (uint32_t qq = 0; qq < LY::NRP; qq++) inl |= qq < u_nrp && rl(RP0 + 2 * qq, h) == cks;
            uint64_t cand = __builtin_amdgcn_ballot_w64(chk && !inl);
            while (cand) {
              const uint32_t j = (uint32_t)__builtin_ctzll(cand);
              const uint32_t c = rdl(cks, j);
              if (u_nrp >= LY::NRP || u_nrp >= CPh->rp_cap) {  // the planner's bound (CDR_CAP_REG), or the slice
                rty = true; why |= 32u;
                break;
              }
              if (lane == 0) {
                rs(RP0 + 2 * u_nrp, h, c);
                rs(RP0 + 2 * u_nrp + 1, h, rdl(k, j));
              }
              u_nrp++;
              u_flags |= CDR_XI_HAS_RESET_POINTS;
              cand &= ~__builtin_amdgcn_ballot_w64(cks == c);
            }
          }
          u_cks = mCK ? rdl(cks, (uint32_t)hbit(mCK)) : u_cks;
          // closes / continue-as-new, in order (:483-531,537-595 -> UpdateWorkflowStateCloseStatus);
          // a DecisionTaskStarted before one takes Created to Running
          {
            int32_t st = u_state, cl = u_close;
            int prev = -1;
            for (uint64_t m = mRare; m && !rty; m &= m - 1) {
              const int j = (int)__builtin_ctzll(m);
              if (st == CDR_STATE_CREATED && (mDST & above(prev) & ~above(j - 1) & ~(1ull << j))) st = CDR_STATE_RUNNING;
              const uint32_t tj = rdl(type, (uint32_t)j), cfj = rdl(cfk, (uint32_t)j);
              if (tj == CDR_EV_WF_CONTINUED_AS_NEW) {
                const int32_t nr = Dh->newrun;
                const bool empty = nr < 0 || gp(B_.wfs)[nr].ev_len == 0 || u_can_k != RNONE;
                if (empty || !transition_ok(st, cl, CDR_STATE_COMPLETED, CDR_CLOSE_CONTINUED_AS_NEW)) {
                  rty = true; why |= 64u;
                } else {
                  u_newrun = true;
                  st = CDR_STATE_COMPLETED;
                  cl = CDR_CLOSE_CONTINUED_AS_NEW;
                  u_close_k = cfj;
                  u_can_k = cfj;
                }
              } else {
                const int cs = tj == CDR_EV_WF_COMPLETED   ? CDR_CLOSE_COMPLETED
                               : tj == CDR_EV_WF_FAILED    ? CDR_CLOSE_FAILED
                               : tj == CDR_EV_WF_TIMED_OUT ? CDR_CLOSE_TIMED_OUT
                               : tj == CDR_EV_WF_CANCELED  ? CDR_CLOSE_CANCELED
                                                           : CDR_CLOSE_TERMINATED;
                if (!transition_ok(st, cl, CDR_STATE_COMPLETED, cs)) {
                  rty = true; why |= 128u;
                } else {
                  st = CDR_STATE_COMPLETED;
                  cl = cs;
                  u_close_k = cfj;
                }
              }
              prev = j;
            }
            if (st == CDR_STATE_CREATED && (mDST & above(prev))) st = CDR_STATE_RUNNING;
            u_state = st;
            u_close = cl;
          }
          // UpsertWorkflowSearchAttributes (:533-535 -> :2746-2768): last writer per key, rows in place
          for (uint64_t m = mUPS; m && !rty; m &= m - 1) {
            const uint32_t j = (uint32_t)__builtin_ctzll(m);
            const uint64_t aoff = (uint64_t)rdl64(q.aux, j);
            const uint32_t cnt = rdl(q.hh, j), cap = CPh->sa_cap;
            if (solo) {
              for (uint32_t q0 = 0; q0 < cnt; q0 += CDR_SLICE_WIDTH) {
                const bool in = q0 + lane < cnt;
                const cdr_kv kl = in ? gget(gp(B_.kvs) + (aoff + q0 + lane)) : cdr_kv{0u, 0u};
                const uint32_t nq = cnt - q0 < CDR_SLICE_WIDTH ? cnt - q0 : CDR_SLICE_WIDTH;
                for (uint32_t qq = 0; qq < nq; qq++) {
                  const uint32_t kk = rdl(kl.key, qq), kv_ = rdl(kl.value, qq);
                  const uint64_t hit = __builtin_amdgcn_ballot_w64(lane < u_nsa && sa_k == kk);
                  if (hit) {
                    sa_v = ((hit >> lane) & 1u) ? kv_ : sa_v;
                  } else if (u_nsa < cap && u_nsa < CDR_REG_NSA) {
                    sa_k = lane == u_nsa ? kk : sa_k;
                    sa_v = lane == u_nsa ? kv_ : sa_v;
                    u_nsa++;
                  } else {
                    rty |= u_nsa >= cap;  // a new key past the slice: k_replay_reg reports it
                  }
                }
              }
              u_flags |= CDR_XI_HAS_SEARCH_ATTR;
              continue;
            }
            GAS cdr_kv* sah = out_sa(O_) + CPh->sa_off;
            for (uint32_t qq = 0; qq < cnt; qq++) {
              const cdr_kv kv = gget(gp(B_.kvs) + (aoff + qq));
              bool found = false;
              for (uint32_t jj = 0; jj < u_nsa; jj++)
                if (__hip_atomic_load(&(sah + jj)->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kv.key) {
                  if (lane == 0) (sah + jj)->value = kv.value;
                  found = true;
                }
              if (!found && u_nsa < cap && u_nsa < CDR_REG_NSA) {
                if (lane == 0) gput(sah + u_nsa, kv);
                u_nsa++;
              } else {
                rty |= !found && u_nsa >= cap;
              }
              vmdrain();
            }
            u_flags |= CDR_XI_HAS_SEARCH_ATTR;
          }
          u_sig += (int32_t)__builtin_popcountll(M(CDR_TB(CDR_EV_WF_SIGNALED)));  // :473-476
          u_flags |= M(CDR_TB(CDR_EV_WF_CANCEL_REQUESTED)) ? CDR_XI_CANCEL_REQUESTED : 0u;  // :478-481
          if (hVH && copen) u_curv = mRare ? verfr : (mAct ? rdl64(ver, (uint32_t)hbit(mAct)) : u_curv);
          if (mAct) {
            const uint32_t la = (uint32_t)hbit(mAct);
            u_anyw = true;
            u_last_wk = rdl(k, la);
            u_wver = rdl64(ver, la);
          }
        }
        // write history h's state back into lane h
        x_flags = me ? u_flags : x_flags;
        cks_ok = me ? u_cks : cks_ok;
        dreq = me ? u_dreq : dreq;
        close_k = me ? u_close_k : close_k;
        can_k = me ? u_can_k : can_k;
        last_wk = me ? u_last_wk : last_wk;
        n_rp = me ? u_nrp : n_rp;
        n_sa = me ? u_nsa : n_sa;
        ld = me ? u_ld : ld;
        ld_cfk = me ? u_ldcfk : ld_cfk;
        any_w = me ? u_anyw : any_w;
        newrun_applied = me ? u_newrun : newrun_applied;
        x_dt_timeout_value = me ? u_dtv : x_dt_timeout_value;
        x_state = me ? u_state : x_state;
        x_close = me ? u_close : x_close;
        x_signals = me ? u_sig : x_signals;
        dto = me ? u_dto : dto;
        x_last_processed = me ? u_lp : x_last_processed;
        dv = me ? u_dv : dv;
        dsched = me ? u_dsched : dsched;
        dstart = me ? u_dstart : dstart;
        datt = me ? u_datt : datt;
        dst_ts = me ? u_dst : dst_ts;
        dsc_ts = me ? u_dsc : dsc_ts;
        dorig_ts = me ? u_dorig : dorig_ts;
        curv = me ? u_curv : curv;
        wver = me ? u_wver : wver;
        if (snap) {
          s_dv = me ? v_dv : s_dv;
          s_dsched = me ? v_dsched : s_dsched;
          s_dstart = me ? v_dstart : s_dstart;
          s_dreq = me ? v_dreq : s_dreq;
          s_dto = me ? v_dto : s_dto;
          s_datt = me ? v_datt : s_datt;
          s_dst = me ? v_dst : s_dst;
          s_dsc = me ? v_dsc : s_dsc;
          s_dorig = me ? v_dorig : s_dorig;
        }
        retry |= me && rty;
        wwhy = me ? why : wwhy;
        const bool hdone = rty || (r + 1) * CDR_SLICE_WIDTH >= wn;
        if (rty) wcnt = me ? 0u : wcnt;
        // every W event below the published history index is replayed (and its reset point stored)
        if (lane == 0) rs(MB + LY::MB_WNRP, h, u_nrp);
        rs_publish(MB + LY::MB_WPROG, h, hdone ? 0xFFFFFFFFu : u_last_wk + 1u);
      }
    }
#define CLD_CAPTURE(mine_)                                                                                 \
  do {                                                                                                     \
    const bool c_ = (mine_) && ld_pending(ld);                                                             \
    if (__builtin_amdgcn_ballot_w64(c_ && want_ld)) {                                                      \
      if (c_) ld_write(gp(O_.last_decision) + w, ld, dv, dsched, dstart, dreq, dto, datt, dsc_ts, dst_ts,  \
                       dorig_ts);                                                                          \
      vmdrain();                                                                                           \
    }                                                                                                      \
    ld |= c_ ? LD_CAPTURED : 0u;                                                                           \
  } while (0)
    // WorkflowExecutionStarted (stateBuilder.go:158-184 -> mutableStateBuilder.go:1639-1716)
    // (h0: the Started half of the record into these 32 words instead of field by field, for
    // the caller to write with the wave, *h0_on set when the lane's Started applied)
    auto wf_started = [&](const Ev& e, int64_t ver, uint32_t* h0 = nullptr, bool* h0_on = nullptr)
                          __attribute__((always_inline)) {
      const GAS cdr_attr_wf_started* a = gp((const cdr_attr_wf_started*)(B_.ev.arena + (uint64_t)e.aux));
      const uint32_t af = a->flags;
      const bool f1 = (af & CDR_SF_HAS_PARENT_DOMAIN) && (af & CDR_SF_PARENT_DOMAIN_MISSING);
      const bool f2 = !f1 && !transition_ok(x_state, x_close, CDR_STATE_CREATED, CDR_CLOSE_NONE);
      retry |= f1 || f2;
      if (!f1 && !f2 && h0) {
        const bool rp_ = (af & CDR_SF_HAS_RETRY) != 0;
        uint64_t lo, hi;  // SetHistoryTree (:313-339)
        cdr_uuid(B_.uuid_seed, D.wf_key, CDR_UUID_BRANCH, e.id, &lo, &hi);
        auto q64 = [&](int i, uint64_t v) {
          h0[i] = (uint32_t)v;
          h0[i + 1] = (uint32_t)(v >> 32);
        };
        h0[0] = D.domain_id;
        h0[1] = D.workflow_id;
        h0[2] = D.run_id;
        h0[3] = D.request_id;
        h0[4] = (af & CDR_SF_HAS_PARENT_DOMAIN) ? a->parent_domain_id : 0u;
        h0[5] = (af & CDR_SF_HAS_PARENT_EXEC) ? a->parent_workflow_id : 0u;
        h0[6] = (af & CDR_SF_HAS_PARENT_EXEC) ? a->parent_run_id : 0u;
        h0[7] = a->task_list;
        h0[8] = a->workflow_type;
        h0[9] = a->cron_schedule;
        h0[10] = (af & CDR_SF_HAS_MEMO) ? a->memo : 0u;
        h0[11] = rp_ ? a->nonretriable : 0u;
        h0[12] = D.run_id;  // branch_tree_id
        h0[13] = (uint32_t)a->exec_timeout_s;
        h0[14] = (uint32_t)a->task_timeout_s;  // decision_timeout_value (the W loop never changes it)
        h0[15] = (uint32_t)a->attempt;
        q64(16, (uint64_t)((af & CDR_SF_HAS_PARENT_INITIATED) ? a->parent_initiated_id : CDR_EMPTY_EVENT_ID));
        h0[18] = (uint32_t)(rp_ ? a->retry_initial_s : 0);
        h0[19] = (uint32_t)(rp_ ? a->retry_max_interval_s : 0);
        q64(20, __builtin_bit_cast(uint64_t, rp_ ? a->backoff_coefficient : 0.0));
        h0[22] = (uint32_t)(rp_ ? a->retry_max_attempts : 0);
        h0[23] = (uint32_t)(rp_ ? a->retry_expiration_s : 0);
        q64(24, (uint64_t)a->expiration_ts);
        q64(26, lo);
        q64(28, hi);
        h0[30] = h0[31] = 0u;  // _pad0, _pad1
        *h0_on = true;
      }
      if (!f1 && !f2) {  // the first Started: absent optional fields are written as zero
        uint32_t xf = x_flags;
        if (!h0) {
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
        X->parent_domain_id = (af & CDR_SF_HAS_PARENT_DOMAIN) ? a->parent_domain_id : 0u;
        X->parent_workflow_id = (af & CDR_SF_HAS_PARENT_EXEC) ? a->parent_workflow_id : 0u;
        X->parent_run_id = (af & CDR_SF_HAS_PARENT_EXEC) ? a->parent_run_id : 0u;
        X->expiration_time = a->expiration_ts;
        xf |= a->expiration_ts != 0 ? CDR_XI_HAS_EXPIRATION : 0u;
        const bool retry_p = (af & CDR_SF_HAS_RETRY) != 0;
        xf |= retry_p ? CDR_XI_HAS_RETRY : 0u;
        X->backoff_coefficient = retry_p ? a->backoff_coefficient : 0.0;
        X->expiration_seconds = retry_p ? a->retry_expiration_s : 0;
        X->initial_interval = retry_p ? a->retry_initial_s : 0;
        X->maximum_attempts = retry_p ? a->retry_max_attempts : 0;
        X->maximum_interval = retry_p ? a->retry_max_interval_s : 0;
        X->nonretriable = retry_p ? a->nonretriable : 0u;
        } else {
        xf |= a->expiration_ts != 0 ? CDR_XI_HAS_EXPIRATION : 0u;
        xf |= (af & CDR_SF_HAS_RETRY) ? CDR_XI_HAS_RETRY : 0u;
        }
        // rolloverAutoResetPointsWithExpiringTime (:3184-3205): rows written here, their
        // checksums kept for addBinaryCheckSumIfNotExists
        n_rp = 0;
        xf &= ~CDR_XI_HAS_RESET_POINTS;
        if (af & CDR_SF_HAS_RESET_POINTS) {
          xf |= CDR_XI_HAS_RESET_POINTS;
          const int64_t expiring = e.ts + (int64_t)D.retention_days * 24ll * 3600ll * NS_PER_S;
          const uint32_t crun = a->continued_run_id, off = a->reset_points_off, cnt = a->reset_points_len;
          const uint32_t cap = CP.rp_cap;
          retry |= cnt > cap;  // the points do not fit the slice: k_replay_reg reports it
          for (uint32_t q = 0; q < cnt && q < cap && n_rp < LY::NRP; q++) {
            cdr_reset_point pr = gget(gp(B_.rps) + (off + q));
            const uint32_t run = (pr.flags & CDR_RP_HAS_RUN_ID) ? pr.run_id : 0u;
            if (run == crun) {
              pr.flags |= CDR_RP_HAS_EXPIRING;
              pr.expiring_time_nano = expiring;
            }
            gput(rp + n_rp, pr);
            rs(RP0 + 2 * n_rp, lane, (pr.flags & CDR_RP_HAS_CHECKSUM) ? pr.binary_checksum : 0u);
            rs(RP0 + 2 * n_rp + 1, lane, RNONE);
            n_rp++;
          }
        }
        xf |= (af & CDR_SF_HAS_MEMO) ? CDR_XI_HAS_MEMO : 0u;
        if (!h0) X->memo = (af & CDR_SF_HAS_MEMO) ? a->memo : 0u;
        if (af & CDR_SF_HAS_SEARCH_ATTR) {
          n_sa = 0;
          const uint32_t off = a->search_attr_off, cnt = a->search_attr_len, cap = CP.sa_cap;
          retry |= cnt > cap;
          for (uint32_t q = 0; q < cnt && q < cap && n_sa < CDR_REG_NSA; q++) {
            gput(sa + n_sa, gget(gp(B_.kvs) + (off + q)));
            n_sa++;
          }
          if (n_sa) xf |= CDR_XI_HAS_SEARCH_ATTR;
          else xf &= ~CDR_XI_HAS_SEARCH_ATTR;
        }
        xf |= CDR_XI_STARTED | (isVH ? CDR_XI_VH_BRANCH : CDR_XI_HAS_BRANCH);
        if (!h0) {
          uint64_t lo, hi;  // SetHistoryTree (:313-339)
          cdr_uuid(B_.uuid_seed, D.wf_key, CDR_UUID_BRANCH, e.id, &lo, &hi);
          X->branch_tree_id = D.run_id;
          X->branch_id_lo = lo;
          X->branch_id_hi = hi;
        }
        if (isRS) RS->start_version = ver;  // :182-184
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
      }
    };
    if constexpr (!PAR) {
    // the first W row is the history's Started in (nearly) every lane: replayed here, so
    // that the loop below keeps none of its state live (a Started anywhere else hands the
    // entry on); the loop then starts at row 1, or at row 0 with the peeled lanes skipping it
    uint32_t w_off = 0;
    bool skip0 = false;
#if CDR_CLS_PEEL_STARTED
    if (MW) {
      const uint32_t tf0 = load_tf(C, lane * 8u);
      const uint32_t t0 = tf0 & 0xFFu;
      const bool st0 = !retry && t0 == CDR_EV_WF_STARTED;
      if (__builtin_amdgcn_ballot_w64(st0)) {
        const EvC q0 = load_cls(C, lane * 8u, tf0);
        uint32_t h0[32];
        bool h0_on = false;
        int64_t st_backoff = 0, st_timeout = 0;  // TASKS: the Started's timer tasks
        uint32_t st_cron = 0;
        if (st0) {  // the loop body's prologue for a first W event, then the handler
          const int64_t ver = q0.e.ver;
          wver = ver;
          ld = 0u;
          any_w = true;
          last_wk = (uint32_t)q0.ann & 0xFFFFFu;
          if (isVH) curv = ver;  // x_state is Created
          wf_started(q0.e, ver, h0, &h0_on);
          if constexpr (TASKS) {
            if (h0_on) {
              const GAS cdr_attr_wf_started* a = gp((const cdr_attr_wf_started*)(B_.ev.arena + (uint64_t)q0.e.aux));
              st_backoff = (int64_t)a->first_decision_backoff_s * NS_PER_S;
              st_timeout = (int64_t)a->exec_timeout_s * NS_PER_S;
              st_cron = (a->flags & CDR_SF_CRON_INITIATOR) ? 1u : 0u;
              KA()->thead[8ull * (uint64_t)w + 4] = h0[7];  // ExecutionInfo.TaskList, for the merge
            }
          }
        }
        // the Started half of ExecutionInfo, written by the wave together (coop_put)
        coop_put<CWX>((GAS exec_half*)X, *reinterpret_cast<const exec_half*>(h0), h0_on, LWX);
        // scheduleWorkflowTimerTask (stateBuilder.go:706-735) + RecordWorkflowStartedTask (:614-616)
        stage(CDR_CLS_W, h0_on && st_backoff != 0, CDR_TT_WORKFLOW_BACKOFF, st_cron, 1u, 0u, 0, q0.e.ts + st_backoff);
        stage(CDR_CLS_W, h0_on, CDR_TT_WORKFLOW_TIMEOUT, 0u, 1u, 0u, 0, q0.e.ts + st_timeout + st_backoff);
        stage(CDR_CLS_W, h0_on, CDR_TT_RECORD_STARTED, 0u, 0u, 0u, 0, 0);
        tq_step();
      }
      const bool need0 = !retry && !st0 && t0 != CDR_EV_PAD;
      if (__builtin_amdgcn_ballot_w64(need0)) skip0 = st0;
      else w_off = 1;
    }
#endif
    CLS_LOOP_BEGIN2(w_off, MW - w_off, CDR_CLS_DEPTH_W, skip0)
    skip0 = false;
    const int64_t ver = (e.tf & CDR_SEF_CLS_VER_SAME) ? wver : e.ver;
    wver = act ? ver : wver;
    const uint32_t cfk = k - dcf;
    // lastDecision is a local of each applyEvents call: a call with no W event before
    // this one reset it (stateBuilder.go:126)
    ld = SEL(act && (!any_w || cfk > last_wk), 0u, ld);
    any_w |= act;
    last_wk = act ? k : last_wk;
    // currentVersion follows every event while Created / Running (stateBuilder.go:134-
    // 154); between W events the state cannot change, so at a W event it is the event's
    // own version or, once closed, the closing event's
    if (isVH) curv = SEL(act && (x_state == CDR_STATE_CREATED || x_state == CDR_STATE_RUNNING), ver, curv);
    retry |= act && type >= CDR_EV_NUM_TYPES;  // :597-599
    const uint64_t tb = (act && type < 64) ? (1ull << type) : 0ull;
    // ---- register-only types (stateBuilder.go:186-213,470-481)
    if (__builtin_amdgcn_ballot_w64(tb & RG_SIMPLE)) {
      const bool ms = type == CDR_EV_DT_SCHEDULED && act;  // :186-200 -> :143-167
      dv = SEL(ms, ver, dv);
      dsched = SEL(ms, e.id, dsched);
      dstart = SEL(ms, CDR_EMPTY_EVENT_ID, dstart);
      dreq = SEL(ms, EU, dreq);
      dto = SEL(ms, e.n, dto);
      datt = SEL(ms, e.aux, datt);
      dsc_ts = SEL(ms, e.ts, dsc_ts);
      dst_ts = SEL(ms, (int64_t)0, dst_ts);
      dorig_ts = SEL(ms, e.ts, dorig_ts);
      ld = SEL(ms, ld_make(CDR_LD_SCHEDULED, k), ld);
      stage(CDR_CLS_W, ms, CDR_TT_DECISION, 0u, 0u, k, e.id, 0);  // :196-197 (domain, TaskList: the merge)
      const bool mt = type == CDR_EV_DT_STARTED && act;  // :202-213 -> :200-253
      const bool f = mt && e.key != dsched;
      retry |= f;
      const bool ok = mt && !f;
      stage(CDR_CLS_W, ok, CDR_TT_DECISION_TIMEOUT, CDR_TIMEOUT_START_TO_CLOSE, 1u, k, e.key,
            e.ts + (int64_t)dto * NS_PER_S);  // :209-212
      x_state = SEL(ok && x_state == CDR_STATE_CREATED, (int32_t)CDR_STATE_RUNNING, x_state);
      dv = SEL(ok, ver, dv);
      dstart = SEL(ok, e.id, dstart);
      dreq = SEL(ok, e.h, dreq);
      datt = SEL(ok, (int64_t)0, datt);
      dst_ts = SEL(ok, e.ts, dst_ts);
      ld = SEL(ok, ld_make(CDR_LD_STARTED, k), ld);
      x_signals += (act && type == CDR_EV_WF_SIGNALED) ? 1 : 0;                           // :473-476
      x_flags |= (act && type == CDR_EV_WF_CANCEL_REQUESTED) ? CDR_XI_CANCEL_REQUESTED : 0u;  // :478-481
    }
    // ---- DecisionTaskCompleted (:215-219 -> :255-262,659-674,789-800)
    if (__builtin_amdgcn_ballot_w64(tb & CDR_TB(CDR_EV_DT_COMPLETED))) {
      const bool mine = (tb & CDR_TB(CDR_EV_DT_COMPLETED)) != 0;
      CLD_CAPTURE(mine);
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
        // the planner's bound (CDR_CAP_REG): never taken; the entry's slice: k_replay_reg reports it
        const bool f = app && (n_rp >= LY::NRP || n_rp >= CP.rp_cap);
        retry |= f;
        const bool put = app && !f;
        if (put) {  // Resettable is settled in the X loop; the row is written after it
          rs(RP0 + 2 * n_rp, lane, cks);
          rs(RP0 + 2 * n_rp + 1, lane, k);
        }
        n_rp += put ? 1u : 0u;
        x_flags |= put ? CDR_XI_HAS_RESET_POINTS : 0u;
        cks_ok = SEL(chk && !f, cks, cks_ok);
      }
    }
    // ---- DecisionTaskTimedOut / Failed: FailDecision :635-656 + transient :169-198
    if (__builtin_amdgcn_ballot_w64(tb & RG_DTFAIL)) {
      const bool mine = (tb & RG_DTFAIL) != 0;
      CLD_CAPTURE(mine);
      const uint32_t xd = (uint32_t)(q_.ann >> 32);
      const bool inc = type == CDR_EV_DT_FAILED || e.n != CDR_TIMEOUT_SCHEDULE_TO_START;
      const int64_t now = B_.now_ns;
      const int64_t na = inc ? datt + 1 : 0;
      const bool tr = na != 0;
      retry |= mine && tr && xd == XD_NONE;
      const int64_t xnext = e.id - (int64_t)xd;  // NextEventID at this call
      dv = SEL(mine, tr ? (isRS ? ver : (isVH ? curv : CDR_EMPTY_VERSION)) : CDR_EMPTY_VERSION, dv);
      dsched = SEL(mine, tr ? xnext : CDR_EMPTY_EVENT_ID, dsched);
      dstart = SEL(mine, CDR_EMPTY_EVENT_ID, dstart);
      dreq = SEL(mine, EU, dreq);
      dto = SEL(mine, tr ? x_dt_timeout_value : 0, dto);
      dst_ts = SEL(mine, (int64_t)0, dst_ts);
      dorig_ts = SEL(mine, (int64_t)0, dorig_ts);
      dsc_ts = SEL(mine, (tr || inc) ? now : (int64_t)0, dsc_ts);
      datt = SEL(mine, na, datt);
      ld = SEL(mine && tr, ld_make(CDR_LD_TRANSIENT, k), ld);
      stage(CDR_CLS_W, mine && tr, CDR_TT_DECISION, 0u, 0u, k, xnext, 0);  // :235,253
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
      retry |= f;
      const bool ok = mine && !f;
      x_state = SEL(ok, (int32_t)CDR_STATE_COMPLETED, x_state);
      x_close = SEL(ok, (int32_t)cs, x_close);
      close_k = SEL(ok, cfk, close_k);  // CompletionEventBatchID = the call's first event id
      // appendTasksForFinishedExecutions (:775-787): DeleteHistoryEvent at close + retention
      // (the merge adds the retention)
      stage(CDR_CLS_W, ok, CDR_TT_CLOSE_EXECUTION, 0u, 0u, k, 0, 0);
      stage(CDR_CLS_W, ok, CDR_TT_DELETE_HISTORY, 0u, 1u, k, 0, e.ts);
    }
    // ---- rare types: WorkflowExecutionStarted, UpsertWorkflowSearchAttributes,
    // ContinuedAsNew (global memory; drained after)
    if (__builtin_amdgcn_ballot_w64(tb & (CDR_TB(CDR_EV_WF_STARTED) | CDR_TB(CDR_EV_UPSERT_SA) |
                                          CDR_TB(CDR_EV_WF_CONTINUED_AS_NEW)))) {
      const bool mine_st = type == CDR_EV_WF_STARTED && act;
#if CDR_CLS_PEEL_STARTED
      retry |= mine_st;  // not the first W row (peeled above), or a second Started: k_replay_reg
#else
      retry |= mine_st && (x_flags & CDR_XI_STARTED);  // a second Started: k_replay_reg
      CLD_CAPTURE(mine_st && !retry);
      if (mine_st && !retry) wf_started(e, ver);
#endif
      if (type == CDR_EV_UPSERT_SA && act) {  // :533-535 -> :2746-2768 (last writer per key)
        const uint64_t aoff = (uint64_t)e.aux;
        const uint32_t cnt = e.h, cap = CP.sa_cap;
        for (uint32_t q = 0; q < cnt; q++) {  // the rows themselves (device-coherent reads after a drain)
          const cdr_kv kv = gget(gp(B_.kvs) + (aoff + q));
          bool found = false;
          for (uint32_t j = 0; j < n_sa; j++)
            if (__hip_atomic_load(&(sa + j)->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == kv.key) {
              (sa + j)->value = kv.value;
              found = true;
            }
          if (!found && n_sa < cap && n_sa < CDR_REG_NSA) {
            gput(sa + n_sa, kv);
            n_sa++;
          } else {
            retry |= !found && n_sa >= cap;  // a new key past the slice: k_replay_reg reports it
          }
          vmdrain();
        }
        x_flags |= CDR_XI_HAS_SEARCH_ATTR;
      }
      const bool t_ups = type == CDR_EV_UPSERT_SA && act;  // TASKS: UpsertWorkflowSearchAttributesTask (:535)
      bool t_can = false;
      if (type == CDR_EV_WF_CONTINUED_AS_NEW && act) {  // :537-595 (the call-index check after the loop)
        const int32_t nr = D.newrun;
        // only one continue-as-new, in the last call, has a new-run history: a second one
        // fails there (newRunHistory is per call) — k_replay_reg reports it
        const bool empty = nr < 0 || gp(B_.wfs)[nr].ev_len == 0 || can_k != RNONE;
        retry |= empty;
        const bool f2 = !empty && !transition_ok(x_state, x_close, CDR_STATE_COMPLETED, CDR_CLOSE_CONTINUED_AS_NEW);
        retry |= f2;
        if (!empty && !f2) {
          newrun_applied = true;  // the new run replays in its own lane; k_finalize joins
          x_state = CDR_STATE_COMPLETED;
          x_close = CDR_CLOSE_CONTINUED_AS_NEW;
          close_k = cfk;
          can_k = cfk;
          t_can = true;
        }
      }
      vmdrain();
      stage(CDR_CLS_W, t_ups, CDR_TT_UPSERT_SA, 0u, 0u, k, 0, 0);
      stage(CDR_CLS_W, t_can, CDR_TT_CLOSE_EXECUTION, 0u, 0u, k, 0, 0);  // :592
      stage(CDR_CLS_W, t_can, CDR_TT_DELETE_HISTORY, 0u, 1u, k, 0, e.ts);
    }
    tq_step();
    CLS_LOOP_END
    }
#undef CLD_CAPTURE
    if constexpr (PAR) {  // the W loop is done: the X wave waits for nothing more; P's results
      if (solo) {  // the lane-held search attributes of lane 0's history
        const uint32_t nsa0 = rdl(n_sa, 0);
        const int32_t wh0 = (int32_t)rdl((uint32_t)w0, 0);
        if (lane < nsa0) gput(out_sa(O_) + gp(B_.caps)[wh0].sa_off + lane, cdr_kv{sa_k, sa_v});
      }
      rs(MB + LY::MB_WNRP, lane, n_rp);
      rs_release(MB + LY::MB_WPROG, lane, 0xFFFFFFFFu);
      PAR_PROF_MARK();
      wg_sync();
      call_first_k = rl(MB + LY::MB_CFK, lane);
      n_calls = rl(MB + LY::MB_NCALLS, lane);
      const uint32_t pw = rl(MB + LY::MB_P, lane);
      n_vh = pw & 0x7FFFFFFFu;
      retry |= (pw >> 31) != 0;
      wwhy |= (pw >> 31) ? 0x100u : 0u;
    }
    // continue-as-new: only in the entry's last call (the reference's call index check)
    if (!retry && can_k != RNONE && !(can_k == call_first_k && n_calls - 1u == (uint32_t)D.newrun_call)) retry = true;
    if (!retry) {  // ---- the ExecutionInfo record, ReplicationState, last VH item, lastDecision
      if constexpr (PAR) {  // the source event's call is not the last: no lastDecision
        if (ld_cfk != call_first_k) ld = 0u;
        if (want_ld)
          ld_write(gp(O_.last_decision) + w, ld, s_dv, s_dsched, s_dstart, s_dreq, s_dto, s_datt, s_dsc, s_dst, s_dorig);
      } else {
        if (!any_w || call_first_k > last_wk) ld = 0u;  // the last call had no W event
        if (want_ld && !(ld & LD_CAPTURED))
          ld_write(gp(O_.last_decision) + w, ld, dv, dsched, dstart, dreq, dto, datt, dsc_ts, dst_ts, dorig_ts);
      }
      if (PAR && !(x_flags & CDR_XI_STARTED)) {  // no WorkflowExecutionStarted: its fields keep their zero values
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
      if constexpr (PAR) {
      X->decision_request_id = dreq;
      X->flags = x_flags;
      X->_pad0 = 0;
      X->completion_event_batch_id = close_k != RNONE ? ev64(close_k, CDR_COL_EVENT_ID) : 0;
      X->decision_timeout_value = x_dt_timeout_value;
      X->state = x_state;
      X->close_status = x_close;
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
      }
      if (isRS && !(x_flags & CDR_XI_STARTED)) RS->start_version = D.failover_version;
    }
    if constexpr (!PAR) {
      // the replay half of ExecutionInfo (P wrote last_first_event_id / last_event_task_id /
      // next_event_id into the record: re-read here), and the Started half of an entry without
      // WorkflowExecutionStarted (all zero), written by the wave together (coop_put).  The
      // Started half of the others went out with the Started event (decision_timeout_value in it:
      // only Started sets it); the padding words are zero
      uint32_t hv[32] = {};
      if (!retry) {
        auto p64 = [&](int i, int64_t v) {
          hv[i] = (uint32_t)v;
          hv[i + 1] = (uint32_t)((uint64_t)v >> 32);
        };
        hv[0] = dreq;
        hv[1] = x_flags;
        p64(2, close_k != RNONE ? ev64(close_k, CDR_COL_EVENT_ID) : 0);
        hv[4] = (uint32_t)x_state;
        hv[5] = (uint32_t)x_close;
        p64(6, X->last_first_event_id);
        p64(8, X->last_event_task_id);
        p64(10, X->next_event_id);
        p64(12, x_last_processed);
        hv[14] = (uint32_t)x_signals;
        hv[15] = (uint32_t)dto;
        p64(16, dv);
        p64(18, dsched);
        p64(20, dstart);
        p64(22, datt);
        p64(24, dst_ts);
        p64(26, dsc_ts);
        p64(28, dorig_ts);
        hv[30] = n_rp;
        hv[31] = n_sa;
      }
      coop_put<CWX>((GAS exec_half*)X + 1, *reinterpret_cast<const exec_half*>(hv), !retry, LWX);
      const exec_half zero{};
      coop_put<CWX>((GAS exec_half*)X, zero, !retry && !(x_flags & CDR_XI_STARTED), LWX);
    }
    if constexpr (PAR) {  // ---- the result, from the other waves' mailbox words
      const uint32_t at = rl(MB + LY::MB_AT, lane), tw = rl(MB + LY::MB_T, lane), xw = rl(MB + LY::MB_X, lane);
      retry |= ((at | tw | xw) >> 31) != 0;
      wwhy |= ((at >> 31) ? 0x200u : 0u) | ((tw >> 31) ? 0x400u : 0u) | ((xw >> 31) ? 0x800u : 0u);
      n_act = at & 0xFFu;
      n_tim = tw & 0xFFu;
      n_chi = xw & 0xFFu;
      n_can = (xw >> 8) & 0xFFu;
      n_sig = (xw >> 16) & 0xFFu;
    }
  }

  // ================================================================ A: activities
  if (!PAR || role == 2) {
    uint32_t a_sid[NA], a_aid[NA], a_inf[NA];
    int64_t a_t[NA], a_s2c[NA];
    int32_t a_stc[NA], a_hb[NA];
#pragma unroll
    for (int j = 0; j < NA; j++) {
      a_sid[j] = a_aid[j] = a_inf[j] = 0;
      a_t[j] = a_s2c[j] = 0;
      a_stc[j] = a_hb[j] = 0;
    }
    uint32_t a_live = 0, a_map = 0, a_st = 0, a_cx = 0;
    bool wform = false;
    if constexpr (PAR) {
      if (solo) {  // ---- wave form (the same handlers as the lane loop below, event for event)
        wform = true;
        uint32_t A_sid = 0, A_aid = 0, A_inf = 0, A_sw = RNONE, A_stk = RNONE, A_cxk = RNONE;
        int64_t A_t = 0, A_s2c = 0;
        int32_t A_stc = 0, A_hb = 0;
        uint64_t m_live = 0, m_map = 0, m_st = 0, m_cx = 0;
        // the pick's argmin, kept across events: its slot (-1: empty table, -2: to recompute)
        // and its (time, key); an event that neither lowers another slot below it nor
        // raises / deletes it keeps it, so most picks need no reduction over the table
        int mj = -1;
        int64_t mt = 0, mk = 0;
        auto below_min = [&](int64_t t_, int64_t k_) { return t_ < mt || (t_ == mt && k_ < mk); };
        bool wr = rdl(retry ? 1u : 0u, 0) != 0;  // uniform: lane 0's history (the other lanes are empty)
        WScanRow Qn = load_wscan(C, MW + lane, MW + MA, 0u);
        for (uint32_t p0 = 0; p0 < MA && !wr; p0 += CDR_SLICE_WIDTH) {
          const WScanRow q = wscan_take(Qn);
          Qn = load_wscan(C, MW + p0 + CDR_SLICE_WIDTH + lane, MW + MA, 0u);
          const uint32_t cnt = MA - p0 < CDR_SLICE_WIDTH ? MA - p0 : CDR_SLICE_WIDTH;
          for (uint32_t i = 0; i < cnt && !wr; i++) {
            const uint32_t type = rdl(q.tf, i) & 0xFFu;
            if (type == CDR_EV_PAD) break;
            const uint64_t ann = (uint64_t)rdl64((int64_t)q.ann, i);
            const uint32_t k = (uint32_t)ann & 0xFFFFFu, dcf = ((uint32_t)ann >> 20) & 0xFFFu;
            const int64_t key = rdl64(q.key, i), ts = rdl64(q.ts, i);
            const uint32_t key32 = (uint32_t)key;
            const bool kfit = (uint64_t)key < (1ull << 31);
            const bool lv = (m_live >> lane) & 1u;
            bool pick = false;
            if (type == CDR_EV_AT_SCHEDULED) {  // :1982-2028; byActivityID[aid] moves to it
              m_map &= ~__builtin_amdgcn_ballot_w64(lv && ((m_map >> lane) & 1u) && A_aid == key32);
              const uint64_t fr = ~m_live & below((uint32_t)NA);
              if (!fr) { wr = true; break; }
              const uint32_t j = (uint32_t)__builtin_ctzll(fr);
              const int64_t ts2c = ts + (int64_t)(int32_t)rdl(q.hh, i) * NS_PER_S;
              const int64_t ts2s = ts + (int64_t)(int32_t)rdl((uint32_t)q.n, i) * NS_PER_S;
              const bool pa = ts2s < ts2c;  // append order breaks ties: S2C before S2S
              const uint32_t sid = (uint32_t)rdl64(q.id, i);
              const int64_t tj = pa ? ts2s : ts2c, kj = ((int64_t)sid << 2) | (pa ? 1 : 0);
              if (!m_live || below_min(tj, kj)) {
                mj = (int)j;
                mt = tj;
                mk = kj;
              }
              if (lane == j) {
                A_sid = sid;
                A_aid = key32;
                A_t = tj;
                A_inf = (pa ? 1u : 0u) | ((pa ? CDR_TTS_SCHEDULE_TO_START : CDR_TTS_SCHEDULE_TO_CLOSE) << 4);
                A_s2c = ts2c;
                A_stc = (int32_t)((uint64_t)key >> 32);
                A_hb = (int32_t)((uint64_t)rdl64(q.aux, i) >> 32);
                A_sw = k | (dcf << 20);
                A_stk = A_cxk = RNONE;
              }
              m_live |= 1ull << j;
              m_map |= 1ull << j;
              m_st &= ~(1ull << j);
              m_cx &= ~(1ull << j);
              pick = true;
            } else if (type == CDR_EV_AT_CANCEL_REQUESTED) {  // :2264-2285 (by activityID)
              const uint64_t fa = __builtin_amdgcn_ballot_w64(lv && ((m_map >> lane) & 1u) && A_aid == key32);
              if (!fa) { wr = true; break; }
              const uint32_t j = 63u - (uint32_t)__builtin_clzll(fa);
              if (lane == j) A_cxk = k;
              m_cx |= 1ull << j;
            } else {
              const uint64_t fs = __builtin_amdgcn_ballot_w64(lv && kfit && A_sid == key32);
              if (!fs) { wr = true; break; }  // nil deref (Started) / not found (closes)
              const uint32_t j = 63u - (uint32_t)__builtin_clzll(fs);
              if (type == CDR_EV_AT_STARTED) {  // :2083-2098
                if (lane == j) {
                  const int64_t tstc = ts + (int64_t)A_stc * NS_PER_S, thb = A_hb > 0 ? ts + (int64_t)A_hb * NS_PER_S : T_NONE;
                  const bool pa = tstc < A_s2c;  // S2C, then StartToClose, then Heartbeat on ties
                  const int64_t t1_ = pa ? tstc : A_s2c;
                  const bool ph = thb < t1_;
                  const uint32_t bit = ph ? CDR_TTS_HEARTBEAT : (pa ? CDR_TTS_START_TO_CLOSE : CDR_TTS_SCHEDULE_TO_CLOSE);
                  A_t = ph ? thb : t1_;
                  A_inf = (A_inf & 0xFF00u) | (ph ? 2u : (pa ? 1u : 0u)) | (bit << 4);
                  A_stk = k;
                }
                m_st |= 1ull << j;
                const int64_t tn = rdl64(A_t, j), kn = ((int64_t)key32 << 2) | (rdl(A_inf, j) & 3u);
                if ((int)j == mj) {  // raised above the others' minimum: recompute
                  if (below_min(tn, kn) || (tn == mt && kn == mk)) {
                    mt = tn;
                    mk = kn;
                  } else {
                    mj = -2;
                  }
                } else if (below_min(tn, kn)) {
                  mj = (int)j;
                  mt = tn;
                  mk = kn;
                }
              } else {  // closes -> DeleteActivity (:1247-1269)
                if ((int)j == mj) mj = -2;
                const uint32_t aid_c = rdl(A_aid, j);
                const bool had = (m_map >> j) & 1u;
                m_live &= ~(1ull << j);
                m_map &= ~(1ull << j);
                if (!had) {  // pendingActivityIDToEventID held by another activity with the same id
                  const uint64_t other = __builtin_amdgcn_ballot_w64(((m_live & m_map) >> lane & 1u) && A_aid == aid_c);
                  if (!other) { wr = true; break; }
                  m_map &= ~other;
                }
              }
              pick = true;
            }
            if (!m_live) mj = -1;
            if (pick && m_live) {  // activity timer pick (timerBuilder.go:211-312): earliest (time, scheduleID, order)
              if (mj < 0) {
                mj = row_argmin2((m_live >> lane) & 1u, A_t, ((int64_t)A_sid << 2) | (A_inf & 3u));
                mt = rdl64(A_t, (uint32_t)mj);
                mk = ((int64_t)rdl(A_sid, (uint32_t)mj) << 2) | (rdl(A_inf, (uint32_t)mj) & 3u);
              }
              const int b = mj;
              const uint32_t bi = rdl(A_inf, (uint32_t)b);
              const uint32_t bit = (bi >> 4) & 0xFu;
              if (!((bi >> 8) & bit) && lane == (uint32_t)b) A_inf |= bit << 8;
            }
          }
        }
        retry = retry || wr;
        // the tables, as the lane loop leaves them in lane 0
#pragma unroll
        for (int j = 0; j < NA; j++) {
          a_sid[j] = rdl(A_sid, j);
          a_aid[j] = rdl(A_aid, j);
          a_inf[j] = rdl(A_inf, j);
          if (lane == 0) {
            rs(RA0 + 3u * (uint32_t)j, 0, rdl(A_sw, j));
            rs(RA0 + 3u * (uint32_t)j + 1, 0, rdl(A_stk, j));
            rs(RA0 + 3u * (uint32_t)j + 2, 0, rdl(A_cxk, j));
          }
        }
        a_live = (uint32_t)m_live;
        a_map = (uint32_t)m_map;
        a_st = (uint32_t)m_st;
        a_cx = (uint32_t)m_cx;
      }
    }
    if (!wform) {
    CLS_LOOP_BEGIN(MW, MA, CDR_CLS_DEPTH)
    const uint64_t tb = act ? (1ull << type) : 0ull;
    if (__builtin_amdgcn_ballot_w64(tb & RG_ACT)) {  // :259-322 -> mutableStateBuilder.go:1982-2285
      const bool m_s = type == CDR_EV_AT_SCHEDULED && act, m_st = type == CDR_EV_AT_STARTED && act;
      const bool m_cl = (tb & RG_ACT_CLOSE) != 0, m_cr = type == CDR_EV_AT_CANCEL_REQUESTED && act;
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
      retry |= f_cap;
      const bool ok_s = m_s && !f_cap;
      const int js = ok_s ? ff : -1;
      {
        const int64_t ts2c = e.ts + (int64_t)(int32_t)e.h * NS_PER_S, ts2s = e.ts + (int64_t)e.n * NS_PER_S;
        const bool pa = ts2s < ts2c;  // append order breaks ties: S2C before S2S
        CSET(a_sid, NA, js, (uint32_t)e.id);
        CSET(a_aid, NA, js, key32);
        CSET(a_t, NA, js, pa ? ts2s : ts2c);
        CSET(a_inf, NA, js, (pa ? 1u : 0u) | ((pa ? CDR_TTS_SCHEDULE_TO_START : CDR_TTS_SCHEDULE_TO_CLOSE) << 4));
        CSET(a_s2c, NA, js, ts2c);
        CSET(a_stc, NA, js, (int32_t)((uint64_t)e.key >> 32));  // StartToClose seconds
        CSET(a_hb, NA, js, (int32_t)((uint64_t)e.aux >> 32));   // HeartbeatTimeout seconds
        if (ok_s) {
          const uint32_t pw = RA0 + 3u * (uint32_t)js;
          rs(pw, lane, k | (dcf << 20));
          rs(pw + 1, lane, RNONE);
          rs(pw + 2, lane, RNONE);
        }
      }
      a_live |= bitof(js);
      a_map |= bitof(js);
      a_st &= ~bitof(js);
      a_cx &= ~bitof(js);
      stage(CDR_CLS_A, ok_s, CDR_TT_ACTIVITY, 0u, 0u, k, e.id, 0);  // :265-266 (domain, TaskList: the merge)
      // ActivityTaskStarted (:2083-2098): nil deref if missing
      const bool f_st = m_st && fs < 0;
      retry |= f_st;
      const bool ok_st = m_st && !f_st;
      const int jst = ok_st ? fs : -1;
      {
        int64_t ts2c = 0;
        int32_t stc = 0, hb = 0;
        uint32_t old = 0;
        CGET(a_inf, NA, jst, old);
        CGET(a_s2c, NA, jst, ts2c);
        CGET(a_stc, NA, jst, stc);
        CGET(a_hb, NA, jst, hb);
        const int64_t tstc = e.ts + (int64_t)stc * NS_PER_S, thb = hb > 0 ? e.ts + (int64_t)hb * NS_PER_S : T_NONE;
        const bool pa = tstc < ts2c;  // S2C, then StartToClose, then Heartbeat on ties
        const int64_t t1_ = pa ? tstc : ts2c;
        const bool ph = thb < t1_;
        const int64_t tn = ph ? thb : t1_;
        const uint32_t bit = ph ? CDR_TTS_HEARTBEAT : (pa ? CDR_TTS_START_TO_CLOSE : CDR_TTS_SCHEDULE_TO_CLOSE);
        const uint32_t in = (old & 0xFF00u) | (ph ? 2u : (pa ? 1u : 0u)) | (bit << 4);
        if (ok_st) rs(RA0 + 3u * (uint32_t)jst + 1, lane, k);
        CSET(a_t, NA, jst, tn);
        CSET(a_inf, NA, jst, in);
        a_st |= bitof(jst);
      }
      // closes -> DeleteActivity (:1247-1269)
      const bool f_cl = m_cl && fs < 0;
      retry |= f_cl;
      bool ok_cl = m_cl && !f_cl;
      {
        const int jc = ok_cl ? fs : -1;
        uint32_t aid_c = 0;
        CGET(a_aid, NA, jc, aid_c);
        const bool had = jc >= 0 && ((a_map >> jc) & 1u);
        a_live &= ~bitof(jc);
        a_map &= ~bitof(jc);
        uint32_t other = 0;  // pendingActivityIDToEventID held by another activity with the same id
#pragma unroll
        for (int j = 0; j < NA; j++)
          other |= (ok_cl && !had && ((a_live & a_map) >> j & 1u) && a_aid[j] == aid_c) ? 1u << j : 0u;
        a_map &= ~other;
        const bool f2 = ok_cl && !had && other == 0;
        retry |= f2;
        ok_cl = ok_cl && !f2;
      }
      // ActivityTaskCancelRequested (:2264-2285)
      const bool f_cr = m_cr && fa < 0;
      retry |= f_cr;
      const bool ok_cr = m_cr && !f_cr;
      if (ok_cr) rs(RA0 + 3u * (uint32_t)fa + 2, lane, k);
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
        CSET(a_inf, NA, made ? best : -1, bi | (b << 8));
        // ActivityTimeoutTask (timerBuilder.go:391-408): TimerTaskStatus bit -> shared.TimeoutType
        stage(CDR_CLS_A, made, CDR_TT_ACTIVITY_TIMEOUT, (uint32_t)__builtin_ctz(b | 16u), 1u, k, (int64_t)bs, bt);
      }
    }
    tq_step();
    CLS_LOOP_END
    }
    if (!retry) {  // ---- pending rows, each at its rank by ScheduleID (k_tables' order)
      GAS cdr_activity_info* act_rows = gp(O_.act) + CP.act_off;
      uint32_t rk[NA];
      CLS_RANKS(rk, NA, a_live, a_sid);
#pragma unroll
      for (int j = 0; j < NA; j++) {
        if (!((a_live >> j) & 1u)) continue;
        const uint32_t pw = RA0 + 3u * (uint32_t)j;
        const uint32_t sw = rl(pw, lane), stk = rl(pw + 1, lane), cxk = rl(pw + 2, lane);
        const uint32_t sk = sw & 0xFFFFFu, cfk = sk - (sw >> 20);
        uint32_t vk = sk;  // Version: the last of Scheduled / Started / CancelRequested
        vk = (stk != RNONE && stk > vk) ? stk : vk;
        vk = (cxk != RNONE && cxk > vk) ? cxk : vk;
        const int64_t sched_ts = ev64(sk, CDR_COL_TIMESTAMP);
        const uint32_t arec = (uint32_t)ev64(sk, CDR_COL_AUX);
        const GAS cdr_attr_at_scheduled* a = gp((const cdr_attr_at_scheduled*)(B_.ev.arena + arec));
        const bool rt = (a->flags & CDR_AF_HAS_RETRY) != 0;
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
        o.expiration_time = sched_ts + (int64_t)((rt && xs > s2c) ? xs : s2c) * NS_PER_S;
        o.cancel_request_id = cxk != RNONE ? ev64(cxk, CDR_COL_EVENT_ID) : CDR_EMPTY_EVENT_ID;
        o.activity_id = a_aid[j];
        o.request_id = started ? ev32(stk, CDR_COL_H) : 0u;
        o.task_list = a->task_list;
        o.nonretriable = rt ? a->nonretriable : 0u;
        o.s2s = a->s2s_s;
        o.s2c = s2c;
        o.stc = a->stc_s;
        o.hb = a->hb_s;
        o.timer_task_status = (int32_t)((a_inf[j] >> 8) & 0xFFu);
        o.attempt = 0;
        o.initial_interval = rt ? a->retry_initial_s : 0;
        o.maximum_interval = rt ? a->retry_max_interval_s : 0;
        o.maximum_attempts = rt ? a->retry_max_attempts : 0;
        o.flags = (rt ? CDR_AI_HAS_RETRY : 0u) | (((a_cx >> j) & 1u) ? CDR_AI_CANCEL_REQUESTED : 0u) |
                  (((a_st >> j) & 1u) ? CDR_AI_STARTED_TIME_SET : 0u);
        o.backoff_coefficient = rt ? a->backoff_coefficient : 0.0;
        gput(act_rows + rk[j], o);
        n_act++;
      }
    }
  }

  if constexpr (PAR) {  // the A wave is done (T runs on the P wave, after its scans)
    if (role == 2) {
      rs(MB + LY::MB_AT, lane, n_act | (retry ? 0x80000000u : 0u));
      PAR_PROF_MARK();
      wg_sync();
    }
  }
  // ================================================================ T: user timers
  if (!PAR || role == 0) {
    uint32_t t_tid[NT], t_sid[NT];
    int64_t t_exp[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) {
      t_tid[j] = t_sid[j] = 0;
      t_exp[j] = 0;
    }
    uint32_t t_live = 0, t_cr = 0;
    bool wform = false;
    if constexpr (PAR) {
      if (solo) {  // ---- wave form (the lane loop's handlers below, event for event)
        wform = true;
        uint32_t T_tid = 0, T_sid = 0, T_k = 0;
        int64_t T_exp = 0;
        uint64_t m_live = 0, m_cr = 0;
        bool wr = rdl(retry ? 1u : 0u, 0) != 0;  // uniform: lane 0's history
        const uint32_t o0 = MW + MA;
        WScanRow Qn = load_wscan(C, o0 + lane, o0 + MT, 0u);
        for (uint32_t p0 = 0; p0 < MT && !wr; p0 += CDR_SLICE_WIDTH) {
          const WScanRow q = wscan_take(Qn);
          Qn = load_wscan(C, o0 + p0 + CDR_SLICE_WIDTH + lane, o0 + MT, 0u);
          const uint32_t cnt = MT - p0 < CDR_SLICE_WIDTH ? MT - p0 : CDR_SLICE_WIDTH;
          for (uint32_t i = 0; i < cnt && !wr; i++) {
            const uint32_t type = rdl(q.tf, i) & 0xFFu;
            if (type == CDR_EV_PAD) break;
            const uint32_t k = (uint32_t)(uint64_t)rdl64((int64_t)q.ann, i) & 0xFFFFFu;
            const uint32_t tid = (uint32_t)rdl64(q.key, i);
            const uint64_t hit = __builtin_amdgcn_ballot_w64(((m_live >> lane) & 1u) && T_tid == tid);
            if (type == CDR_EV_TIMER_STARTED) {  // :2877-2900 (a started timer ID is overwritten)
              const uint64_t fr = ~m_live & below((uint32_t)NT);
              if (!hit && !fr) { wr = true; break; }
              const uint32_t j = hit ? 63u - (uint32_t)__builtin_clzll(hit) : (uint32_t)__builtin_ctzll(fr);
              if (lane == j) {
                T_tid = tid;
                T_sid = (uint32_t)rdl64(q.id, i);
                T_exp = rdl64(q.ts, i) + rdl64(q.aux, i) * NS_PER_S;
                T_k = k;
              }
              m_live |= 1ull << j;
              m_cr &= ~(1ull << j);  // TaskID = TimerTaskStatusNone
            } else {  // Fired / Canceled (:2930-2991): deleted if present
              m_live &= ~hit;
            }
            if (m_live) {  // user timer pick (timerBuilder.go:171-184,233-247): head by (ExpiryTime, StartedID)
              const int b = row_argmin2((m_live >> lane) & 1u, T_exp, (int64_t)T_sid);
              m_cr |= 1ull << b;
            }
          }
        }
        retry = retry || wr;
#pragma unroll
        for (int j = 0; j < NT; j++) {
          t_tid[j] = rdl(T_tid, j);
          t_sid[j] = rdl(T_sid, j);
          t_exp[j] = rdl64(T_exp, j);
          if (lane == 0) rs(RT0 + (uint32_t)j, 0, rdl(T_k, j));
        }
        t_live = (uint32_t)m_live;
        t_cr = (uint32_t)m_cr;
      }
    }
    if (!wform) {
    CLS_LOOP_BEGIN(MW + MA, MT, CDR_CLS_DEPTH_T)
    if (__builtin_amdgcn_ballot_w64(act)) {  // :324-350 -> :2877-2991
      const bool m_ts = type == CDR_EV_TIMER_STARTED && act;
      const bool m_tf = (type == CDR_EV_TIMER_FIRED || type == CDR_EV_TIMER_CANCELED) && act;
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
      retry |= f;
      const bool ok = m_ts && !f;
      const int jt = ok ? slot : -1;
      CSET(t_tid, NT, jt, tid);
      CSET(t_sid, NT, jt, (uint32_t)e.id);
      CSET(t_exp, NT, jt, e.ts + e.aux * NS_PER_S);
      t_live |= bitof(jt);
      t_cr &= ~bitof(jt);  // TaskID = TimerTaskStatusNone
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
      stage(CDR_CLS_T, best >= 0 && !((t_cr >> best) & 1u), CDR_TT_USER_TIMER, 0u, 1u, k, (int64_t)bs, be);
      t_cr |= bitof(best);
    }
    tq_step();
    CLS_LOOP_END
    }
    if (!retry) {
      GAS cdr_timer_info* tim = gp(O_.timer) + CP.timer_off;
      uint32_t rk[NT];
      CLS_RANKS(rk, NT, t_live, t_tid);  // by TimerID
#pragma unroll
      for (int j = 0; j < NT; j++) {
        if (!((t_live >> j) & 1u)) continue;
        cdr_timer_info o;
        o.version = ev64(rl(RT0 + (uint32_t)j, lane), CDR_COL_VERSION);
        o.started_id = (int64_t)t_sid[j];
        o.expiry_time = t_exp[j];
        o.task_id = ((t_cr >> j) & 1u) ? CDR_TIMER_TASK_STATUS_CREATED : CDR_TIMER_TASK_STATUS_NONE;
        o.timer_id = t_tid[j];
        o._pad = 0;
        gput(tim + rk[j], o);
        n_tim++;
      }
    }
  }

  if constexpr (PAR) {
    if (role == 0) {
      rs(MB + LY::MB_T, lane, n_tim | (retry ? 0x80000000u : 0u));
      PAR_PROF_MARK();
      wg_sync();
    }
  }
  // ================================================================ X: children, cancels, signals
  if (!PAR || role == 3) {
    uint32_t c_id[NX], r_id[NX], g_id[NX];
#pragma unroll
    for (int j = 0; j < NX; j++) c_id[j] = r_id[j] = g_id[j] = 0;
    uint32_t c_live = 0, r_live = 0, g_live = 0;
    uint32_t rn = 0;  // first reset point whose Resettable flag is not settled yet
    // settle the reset points created (by a DecisionTaskCompleted) before history index
    // ko: Resettable iff no child / request-cancel / signal is pending then (:1798-1842)
    auto settle = [&](bool on_, uint32_t ko) {
      uint32_t nrp = n_rp;
      if constexpr (PAR) {  // wait until the W wave has replayed every W event below ko
        for (;;) {
          const bool wait = on_ && rl_poll(MB + LY::MB_WPROG, lane) < ko;
          if (!__builtin_amdgcn_ballot_w64(wait)) break;
          __builtin_amdgcn_s_sleep(2);
        }
        nrp = rl(MB + LY::MB_WNRP, lane);
      }
      for (;;) {
        const uint32_t kw = (on_ && rn < nrp) ? rl(RP0 + 2 * rn + 1, lane) : 0u;
        const bool more = on_ && rn < nrp && (kw == RNONE || kw < ko);
        if (!__builtin_amdgcn_ballot_w64(more)) break;
        if (more && kw != RNONE && (c_live | r_live | g_live) == 0) rs(RP0 + 2 * rn + 1, lane, kw | 0x80000000u);
        rn += more ? 1u : 0u;
      }
    };
    bool wform = false;
    if constexpr (PAR) {
      if (solo) {  // ---- wave form (the lane loop's handlers below, event for event)
        wform = true;
        uint32_t C_id = 0, C_iw = 0, C_stk = RNONE, R_id = 0, R_iw = 0, G_id = 0, G_iw = 0;
        uint64_t mc = 0, mr = 0, mg = 0;
        bool wr = rdl(retry ? 1u : 0u, 0) != 0;  // uniform: lane 0's history
        // settle's wave form for lane 0's history: the W wave's progress word, then every
        // reset point created before history index ko
        // (the progress word, the reset-point count and the next reset point's index are kept
        // between events: an event the W wave is already past costs no LDS round trip)
        uint32_t wseen = 0, nrp = 0, kw_n = 0;
        bool kw_ok = false;
        auto wsettle = [&](uint32_t ko) {
          if (ko > wseen) {
            uint32_t pw;
            while ((pw = rl_poll(MB + LY::MB_WPROG, 0)) < ko) __builtin_amdgcn_s_sleep(2);
            wseen = pw;
            nrp = rl(MB + LY::MB_WNRP, 0);  // published before the progress word
          }
          while (rn < nrp) {
            if (!kw_ok) kw_n = rl(RP0 + 2 * rn + 1, 0);
            kw_ok = true;
            if (!(kw_n == RNONE || kw_n < ko)) break;
            if (kw_n != RNONE && (mc | mr | mg) == 0 && lane == 0) rs(RP0 + 2 * rn + 1, 0, kw_n | 0x80000000u);
            rn++;
            kw_ok = false;
          }
        };
        const uint32_t o0 = MW + MA + MT;
        WScanRow Qn = load_wscan(C, o0 + lane, o0 + MX, 0u);
        for (uint32_t p0 = 0; p0 < MX && !wr; p0 += CDR_SLICE_WIDTH) {
          const WScanRow q = wscan_take(Qn);
          Qn = load_wscan(C, o0 + p0 + CDR_SLICE_WIDTH + lane, o0 + MX, 0u);
          const uint32_t cnt = MX - p0 < CDR_SLICE_WIDTH ? MX - p0 : CDR_SLICE_WIDTH;
          for (uint32_t i = 0; i < cnt && !wr; i++) {
            const uint32_t tf = rdl(q.tf, i), type = tf & 0xFFu;
            if (type == CDR_EV_PAD) break;
            const uint64_t ann = (uint64_t)rdl64((int64_t)q.ann, i);
            const uint32_t k = (uint32_t)ann & 0xFFFFFu, dcf = ((uint32_t)ann >> 20) & 0xFFFu;
            wsettle(k);
            const int64_t key = rdl64(q.key, i);
            const uint32_t key32 = (uint32_t)key;
            const bool kfit = (uint64_t)key < (1ull << 31);
            const bool dmiss = (tf & CDR_SEF_DOMAIN_MISSING) != 0;
            const uint32_t init = k | (dcf << 20);
            const uint32_t id = (uint32_t)rdl64(q.id, i);
            auto lowest = [&](uint64_t m) { return (uint32_t)__builtin_ctzll(m); };
            if (type == CDR_EV_CHILD_INITIATED) {  // :3256-3280
              const uint64_t fr = ~mc & below((uint32_t)NX);
              if (!fr || dmiss) { wr = true; break; }
              const uint32_t j = lowest(fr);
              if (lane == j) {
                C_id = id;
                C_iw = init;
                C_stk = RNONE;
              }
              mc |= 1ull << j;
            } else if (type == CDR_EV_CHILD_STARTED || ((1ull << type) & RG_CHILD_CLOSE)) {  // :3312-3325 / closes
              const uint64_t hit = __builtin_amdgcn_ballot_w64(((mc >> lane) & 1u) && kfit && C_id == key32);
              if (type == CDR_EV_CHILD_STARTED) {
                if (!hit) { wr = true; break; }  // nil deref
                if (lane == lowest(hit)) C_stk = k;
              } else if (hit) {
                mc &= ~(1ull << lowest(hit));
              }
            } else if (type == CDR_EV_RCE_INITIATED || type == CDR_EV_SE_INITIATED) {  // :2577-2596 / :2701-2723
              const bool rce = type == CDR_EV_RCE_INITIATED;
              const uint64_t fr = ~(rce ? mr : mg) & below((uint32_t)NX);
              if (!fr || dmiss) { wr = true; break; }
              const uint32_t j = lowest(fr);
              if (lane == j) {
                if (rce) {
                  R_id = id;
                  R_iw = init;
                } else {
                  G_id = id;
                  G_iw = init;
                }
              }
              (rce ? mr : mg) |= 1ull << j;
            } else if (type == CDR_EV_RCE_FAILED || type == CDR_EV_EXT_CANCEL_REQUESTED) {  // :1147-1153
              const uint64_t hit = __builtin_amdgcn_ballot_w64(((mr >> lane) & 1u) && kfit && R_id == key32);
              if (hit) mr &= ~(1ull << lowest(hit));
            } else if (type == CDR_EV_SE_FAILED || type == CDR_EV_EXT_SIGNALED) {  // :1156-1162
              const uint64_t hit = __builtin_amdgcn_ballot_w64(((mg >> lane) & 1u) && kfit && G_id == key32);
              if (hit) mg &= ~(1ull << lowest(hit));
            }
          }
        }
        if (!wr) wsettle(0xFFFFFFFFu);
        retry = retry || wr;
#pragma unroll
        for (int j = 0; j < NX; j++) {
          c_id[j] = rdl(C_id, j);
          r_id[j] = rdl(R_id, j);
          g_id[j] = rdl(G_id, j);
          if (lane == 0) {
            rs(RC0 + 2 * (uint32_t)j, 0, rdl(C_iw, j));
            rs(RC0 + 2 * (uint32_t)j + 1, 0, rdl(C_stk, j));
            rs(RR0 + (uint32_t)j, 0, rdl(R_iw, j));
            rs(RG0 + (uint32_t)j, 0, rdl(G_iw, j));
          }
        }
        c_live = (uint32_t)mc;
        r_live = (uint32_t)mr;
        g_live = (uint32_t)mg;
      }
    }
    if (!wform) {
    CLS_LOOP_BEGIN(MW + MA + MT, MX, CDR_CLS_DEPTH_X)
    if (__builtin_amdgcn_ballot_w64(act)) {  // :355-468
      settle(act, k);
      const uint32_t key32 = (uint32_t)e.key;
      const bool kfit = (uint64_t)e.key < (1ull << 31);
      const bool dmiss = (e.tf & CDR_SEF_DOMAIN_MISSING) != 0;
      const uint32_t init = k | (dcf << 20);
      // StartChildWorkflowExecutionInitiated (:3256-3280)
      {
        const bool m = type == CDR_EV_CHILD_INITIATED && act;
        const uint32_t fr = ~c_live & ((1u << NX) - 1u);
        const int j = fr ? (int)__builtin_ctz(fr) : -1;
        const bool f = m && (j < 0 || dmiss);
        retry |= f;
        const bool ok = m && !f;
        const int jj = ok ? j : -1;
        CSET(c_id, NX, jj, (uint32_t)e.id);
        c_live |= bitof(jj);
        if (ok) {
          rs(RC0 + 2 * (uint32_t)jj, lane, init);
          rs(RC0 + 2 * (uint32_t)jj + 1, lane, RNONE);
        }
        // scheduleStartChildWorkflowTransferTask (:370-371): targets from the attributes (the merge)
        stage(CDR_CLS_X, ok, CDR_TT_START_CHILD, 0u, 0u, k, e.id, (int64_t)((uint64_t)e.key >> 32));
      }
      // ChildWorkflowExecutionStarted (:3312-3325): nil deref if missing; closes delete
      {
        const bool ms = type == CDR_EV_CHILD_STARTED && act;
        const bool mc = act && ((1ull << type) & RG_CHILD_CLOSE) != 0;
        int j = -1;
#pragma unroll
        for (int i = NX - 1; i >= 0; i--) j = (((c_live >> i) & 1u) && kfit && c_id[i] == key32) ? i : j;
        const bool f = ms && j < 0;
        retry |= f;
        if (ms && !f) rs(RC0 + 2 * (uint32_t)j + 1, lane, k);
        c_live &= ~((mc && j >= 0) ? bitof(j) : 0u);
      }
      // RequestCancelExternalWorkflowExecutionInitiated (:2577-2596) / closes (:1147-1153)
      {
        const bool m = type == CDR_EV_RCE_INITIATED && act;
        const uint32_t fr = ~r_live & ((1u << NX) - 1u);
        const int j = fr ? (int)__builtin_ctz(fr) : -1;
        const bool f = m && (j < 0 || dmiss);
        retry |= f;
        const bool ok = m && !f;
        const int jj = ok ? j : -1;
        CSET(r_id, NX, jj, (uint32_t)e.id);
        r_live |= bitof(jj);
        if (ok) rs(RR0 + (uint32_t)jj, lane, init);
        stage(CDR_CLS_X, ok, CDR_TT_CANCEL_EXECUTION, 0u, 0u, k, e.id, (int64_t)((uint64_t)e.key >> 32));  // :421-427
        const bool mc = (type == CDR_EV_RCE_FAILED || type == CDR_EV_EXT_CANCEL_REQUESTED) && act;
        int jc = -1;
#pragma unroll
        for (int i = NX - 1; i >= 0; i--) jc = (((r_live >> i) & 1u) && kfit && r_id[i] == key32) ? i : jc;
        r_live &= ~((mc && jc >= 0) ? bitof(jc) : 0u);
      }
      // SignalExternalWorkflowExecutionInitiated (:2701-2723) / closes (:1156-1162)
      {
        const bool m = type == CDR_EV_SE_INITIATED && act;
        const uint32_t fr = ~g_live & ((1u << NX) - 1u);
        const int j = fr ? (int)__builtin_ctz(fr) : -1;
        const bool f = m && (j < 0 || dmiss);
        retry |= f;
        const bool ok = m && !f;
        const int jj = ok ? j : -1;
        CSET(g_id, NX, jj, (uint32_t)e.id);
        g_live |= bitof(jj);
        if (ok) rs(RG0 + (uint32_t)jj, lane, init);
        stage(CDR_CLS_X, ok, CDR_TT_SIGNAL_EXECUTION, 0u, 0u, k, e.id, (int64_t)((uint64_t)e.key >> 32));  // :452-458
        const bool mc = (type == CDR_EV_SE_FAILED || type == CDR_EV_EXT_SIGNALED) && act;
        int jc = -1;
#pragma unroll
        for (int i = NX - 1; i >= 0; i--) jc = (((g_live >> i) & 1u) && kfit && g_id[i] == key32) ? i : jc;
        g_live &= ~((mc && jc >= 0) ? bitof(jc) : 0u);
      }
    }
    tq_step();
    CLS_LOOP_END
    settle(!retry, 0xFFFFFFFFu);
    }
    if constexpr (PAR) n_rp = rl(MB + LY::MB_WNRP, lane);  // final: the W loop is done (settle waited)
    if (!retry) {
      GAS cdr_child_info* chi = gp(O_.child) + CP.child_off;
      uint32_t rk_chi[NX];
      CLS_RANKS(rk_chi, NX, c_live, c_id);  // by InitiatedID
      #pragma unroll
      for (int j = 0; j < NX; j++) {
        if (!((c_live >> j) & 1u)) continue;
        const uint32_t iw = rl(RC0 + 2 * (uint32_t)j, lane), stk = rl(RC0 + 2 * (uint32_t)j + 1, lane);
        const uint32_t ik = iw & 0xFFFFFu;
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
        gput(chi + rk_chi[j], c);
        n_chi++;
      }
      GAS cdr_cancel_info* can = gp(O_.cancel) + CP.cancel_off;
      uint32_t rk_can[NX];
      CLS_RANKS(rk_can, NX, r_live, r_id);  // by InitiatedID
      #pragma unroll
      for (int j = 0; j < NX; j++) {
        if (!((r_live >> j) & 1u)) continue;
        const uint32_t iw = rl(RR0 + (uint32_t)j, lane), ik = iw & 0xFFFFFu;
        cdr_cancel_info c;
        c.version = ev64(ik, CDR_COL_VERSION);
        c.initiated_event_batch_id = ev64(ik - (iw >> 20), CDR_COL_EVENT_ID);
        c.initiated_id = (int64_t)r_id[j];
        uint64_t lo, hi;
        cdr_uuid(B_.uuid_seed, D.wf_key, CDR_UUID_CANCEL_REQ, c.initiated_id, &lo, &hi);
        c.cancel_request_lo = lo;
        c.cancel_request_hi = hi;
        gput(can + rk_can[j], c);
        n_can++;
      }
      GAS cdr_signal_info* sig = gp(O_.signal) + CP.signal_off;
      uint32_t rk_sig[NX];
      CLS_RANKS(rk_sig, NX, g_live, g_id);  // by InitiatedID
      #pragma unroll
      for (int j = 0; j < NX; j++) {
        if (!((g_live >> j) & 1u)) continue;
        const uint32_t iw = rl(RG0 + (uint32_t)j, lane), ik = iw & 0xFFFFFu;
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
        gput(sig + rk_sig[j], c);
        n_sig++;
      }
      // reset points added by the replay (the Started ones are written already)
      for (uint32_t q = 0; q < n_rp; q++) {
        const uint32_t kw = rl(RP0 + 2 * q + 1, lane);
        if (kw == RNONE) continue;
        cdr_reset_point pr;
        pr.binary_checksum = rl(RP0 + 2 * q, lane);
        pr.run_id = D.run_id;
        pr.first_decision_completed_id = ev64(kw & 0x7FFFFFFFu, CDR_COL_EVENT_ID);
        pr.created_time_nano = B_.now_ns;
        pr.expiring_time_nano = 0;
        pr.flags = CDR_RP_HAS_CHECKSUM | CDR_RP_HAS_RUN_ID | CDR_RP_HAS_FIRST_DC_ID | CDR_RP_HAS_CREATED |
                   CDR_RP_HAS_RESETTABLE | ((kw & 0x80000000u) ? CDR_RP_RESETTABLE : 0u);
        pr._pad = 0;
        gput(rp + q, pr);
      }
    }
    if constexpr (PAR) {
      rs(MB + LY::MB_X, lane, n_chi | (n_can << 8) | (n_sig << 16) | (retry ? 0x80000000u : 0u));
      PAR_PROF_MARK();
      wg_sync();
    }
  }
  if constexpr (TASKS) {  // the last staged records, then the header: the entry's lists are complete
    tq_flush();
    if (!retry) {
      typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
      u32x4 h;
      h.x = t_n[CDR_CLS_W] | 0x80000000u;
      h.y = t_n[CDR_CLS_A];
      h.z = t_n[CDR_CLS_T];
      h.w = t_n[CDR_CLS_X];
      *(GAS u32x4*)(KA()->thead + 8ull * (uint64_t)w) = h;
    }
  }
  if (PAR && (role != 1 || nolane)) return;
  cdr_wf_result r;
  r.code = retry ? CLS_RETRY : CDR_OK;
  r.flags = retry ? 0u
                  : ((newrun_applied ? CDR_RF_NEWRUN_APPLIED : 0u) | (D.parent >= 0 ? CDR_RF_IS_NEWRUN : 0u) |
                     RF_ROWS_SORTED);
  r.fail_event_id = 0;
#ifdef CDR_PAR_PROF
  if constexpr (PAR) {  // P+T, W, A, X wave times (us), 16 bits each
    r.fail_event_id = 0;
    for (uint32_t j = 0; j < 4; j++) r.fail_event_id |= (int64_t)(rl(LY::PF + j, 0) & 0xFFFFu) << (16 * j);
  }
#endif
#undef PAR_PROF_MARK
  r.fail_index = retry ? wwhy : 0u;
#ifdef CDR_PAR_PROF
  if constexpr (PAR) r.fail_index = retry ? wwhy : (int64_t)prof_start;
#endif
  r.n_activity = retry ? 0u : n_act;
  r.n_timer = retry ? 0u : n_tim;
  r.n_child = retry ? 0u : n_chi;
  r.n_cancel = retry ? 0u : n_can;
  r.n_signal = retry ? 0u : n_sig;
  r.n_vh = retry ? 0u : n_vh;
  r.n_reset_points = retry ? 0u : n_rp;
  r.n_search_attr = retry ? 0u : n_sa;
  if constexpr (PAR) gput(gp(O_.result) + w, r);
  else coop_put<CWR>(gp(O_.result) + w, r, true, 0);  // every LDS word is free again here
  // the slice holds an entry to hand on: list it for k_replay_reg's retry pass
  if (__builtin_amdgcn_ballot_w64(retry) && lane == __builtin_amdgcn_readfirstlane(lane) && KA()->rcount)
    KA()->rlist[atomicAdd(KA()->rcount, 1u)] = s;
#undef SEL
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
#undef CSET
#undef CGET
#undef CLS_LOOP_BEGIN
#undef CLS_LOOP_BEGIN2
#undef CLS_LOOP_END
#undef CLS_RANKS
