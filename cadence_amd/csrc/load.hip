// load.hip — on-device decode of the SQL persistence's row blobs into the loaded states
// cdr_carry takes (cdr.h "loading persisted rows"): the inverse of encode.hip / encode_var.hip
// for the five pending tables (cdr_load_rows) and, with them, the execution row
// (cdr_load_state; "the execution rows" below).
//
// One lane per row, one parser template per table (the pass is its parameter, so the passes
// agree on every byte); each wavefront stages its 64 consecutive rows' bytes in LDS first
// (thrift_dev.h stage_blobs).  The walk of a row only records where its kept fields are (the
// last occurrence of each); what a pass does with them comes after the walk:
//   1. COUNT   row status (wire errors, request-ID text, run-ID length) and the string fields
//              per row; a failing row lowers its entry's first-failure word (atomicMin of
//              table, row in entry, status);
//   2. INTERN  seeds, then the strings of rows whose entry has no failing row, then the
//              generated run-ID texts; the new strings are ranked by hash (hipcub radix sort);
//   3. RANK    one lane per row: its slot is entry_row0 + #{rows of the entry with a smaller
//              key}; equal keys fail the entry (a second failure word: the rank pass reads the
//              first one while it writes);
//   4. FILL    each record built in registers and stored whole at its ranked slot.
// An epilogue, one lane per entry, writes result / caps / entry_status from the failure words
// and the row ranges alone: it walks no rows.
//
// The Cassandra form of the pending tables (cdr_load_cql_rows) is a second front end of the
// same passes: a pre-pass, one lane per (entry, table), splits each map column into its pairs
// (k_cql_split: count, one scan per table, then the row offsets), and Row<TBL>::parse_cql walks
// a pair's UDT — a fixed sequence of length-prefixed values, straight-line code — into the same
// record and Spans.  Keys come from the UDT (the count pass writes them out for the ranking),
// and an activity's error list, whose bytes lack the thrift type byte, goes through gen_bytes.
// Its execution row (cdr_load_cql_state) is the same front end of k_exec: XRow<true>::parse_cql
// walks the `execution` UDT's declared fields, the replication_state and version_histories
// columns are read beside it, and everything after the walk that reads the same bytes is shared.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include <cstdio>
#include <type_traits>

#include "cdr/cdr.h"
#include "cdr/ingest.h"
#include "ctx.h"
#include "thrift_dev.h"

#define HIPCHK(x)                                                                                     \
  do {                                                                                                \
    hipError_t _e = (x);                                                                              \
    if (_e != hipSuccess) {                                                                           \
      fprintf(stderr, "cdr: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(_e), __FILE__, __LINE__); \
      return CDR_API_EDEVICE;                                                                         \
    }                                                                                                 \
  } while (0)

// bytes of row data staged in LDS per wavefront: 64 ActivityInfo rows (~250 B each) fit
#ifndef CDR_LOAD_STAGE
#define CDR_LOAD_STAGE 24576
#endif
#define CDR_LOAD_BLOCK 128 /* 2 wavefronts: 48 KiB of LDS per workgroup */

namespace {

extern __shared__ uint4 ld_lds[];

enum Pass { COUNT = 0, INTERN = 1, FILL = 2 };
constexpr uint64_t GEN_REF = 1ull << 62;
constexpr unsigned long long NO_FAIL = ~0ull;
constexpr uint32_t GEN_BYTES = 36;

struct Span {  // a string / binary value's bytes in `bytes`; n = 0: absent or empty
  uint64_t at;
  uint32_t n;
};

struct LCtx {  // per launch (one table)
  const uint8_t* bytes;
  uint64_t total;
  const uint64_t* blob_off;
  const uint64_t* tid_off;    // table 1: the timer-ID strings
  const int64_t* key;         // tables 0, 2-4
  const int64_t* hb;          // table 0: the LastHeartbeatUpdatedTime column
  const uint32_t* row_entry;  // [n_rows]
  const uint32_t* row0;       // the table's entry_row0
  unsigned long long* fail;   // [2 * n_entries]: decode failures, then duplicate keys
  STab T;
  int32_t* status;             // [n_rows]
  unsigned long long* totals;  // COUNT: string fields
  uint8_t* gen;                // table 2: GEN_BYTES per row
  const uint32_t* dest;        // FILL: [n_rows] ranked slots
  void* recs;                  // FILL: the table
  int64_t* tkey;               // table 1: INTERN writes the ID's hash, FILL reads its handle
  uint32_t n_rows, n_entries;
  // the Cassandra form only
  int64_t* key_out;            // tables 0, 2-4: COUNT writes the UDT's key field ([n_rows]; = key)
  uint64_t* gneed;             // table 0: COUNT writes the row's list-body bytes in gen_bytes
  const uint64_t* goff;        // its exclusive scan, [n_rows + 1]
  uint64_t gen_base;           // where the list bodies start in gen_bytes
};

__device__ __forceinline__ unsigned long long fail_word(uint32_t table, uint32_t row_in_entry, int32_t status) {
  return ((unsigned long long)table << 56) | ((unsigned long long)row_in_entry << 8) | (uint32_t)status;
}
__device__ __forceinline__ uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }

// ---------------------------------------------------------------- field readers
template <class F>
__device__ __forceinline__ void fields(Rd& r, F&& f) {  // f(field type, field id) consumes the value
  while (r.ok()) {
    const uint32_t ft = r.u8();
    if (!r.ok() || ft == T_STOP) return;
    const uint32_t fid = r.be16();
    if (!r.ok()) return;
    f(ft, fid);
  }
}
// (a field of another wire type is ignored: an earlier occurrence stays)
__device__ __forceinline__ void f_i64(Rd& r, uint32_t t, int64_t* v) {
  if (t == T_I64) *v = (int64_t)r.be64();
  else skip1(r, t);
}
__device__ __forceinline__ void f_i32(Rd& r, uint32_t t, int32_t* v) {
  if (t == T_I32) *v = (int32_t)r.be32();
  else skip1(r, t);
}
__device__ __forceinline__ void f_bool(Rd& r, uint32_t t, uint32_t* flags, uint32_t bit) {
  if (t == T_BOOL) *flags = (*flags & ~bit) | (r.u8() ? bit : 0u);
  else skip1(r, t);
}
__device__ __forceinline__ void f_str(Rd& r, uint32_t t, Span* s) {
  if (t != T_STRING) {
    skip1(r, t);
    return;
  }
  const uint32_t n = (uint32_t)r.size();
  if (!r.need(n)) return;
  *s = Span{r.pos, n};
  r.pos += n;
}

// the canonical lowercase RFC 4122 text (8-4-4-4-12) -> hi (first 16 digits), lo
__device__ __forceinline__ bool parse_uuid(Rd& r, Span s, uint64_t* lo, uint64_t* hi) {
  if (s.n != 36) return false;
  uint64_t h = 0, l = 0;
  bool good = true;
  uint32_t d = 0;
  for (uint32_t i = 0; i < 36; i++) {
    const uint32_t c = r.at(s.at + i);
    if (i == 8 || i == 13 || i == 18 || i == 23) {
      good = good && c == '-';
      continue;
    }
    uint32_t v;
    if (c >= '0' && c <= '9') v = c - '0';
    else if (c >= 'a' && c <= 'f') v = c - 'a' + 10;
    else {
      v = 0;
      good = false;
    }
    if (d < 16) h = (h << 4) | v;
    else l = (l << 4) | v;
    d++;
  }
  *lo = l;
  *hi = h;
  return good;
}
// character i of sqldb.UUID(b).String() of the 16 bytes at `at`
__device__ __forceinline__ uint32_t uuid_char(Rd& r, uint64_t at, uint32_t i) {
  if (i == 8 || i == 13 || i == 18 || i == 23) return '-';
  const uint32_t d = i - (i > 8 ? 1u : 0u) - (i > 13 ? 1u : 0u) - (i > 18 ? 1u : 0u) - (i > 23 ? 1u : 0u);
  const uint32_t b = r.at(at + (d >> 1));
  const uint32_t nib = (d & 1u) ? (b & 15u) : (b >> 4);
  return nib < 10 ? '0' + nib : 'a' + (nib - 10);
}
__device__ __forceinline__ uint64_t uuid_text_hash(Rd& r, uint64_t at) {  // cdr_str_hash of that text
  uint64_t h = 0xCBF29CE484222325ull;
  for (uint32_t i = 0; i < GEN_BYTES; i++) h = (h ^ uuid_char(r, at, i)) * 0x100000001B3ull;
  h = cdr_mix64(h ^ ((uint64_t)GEN_BYTES * 0x9E3779B97F4A7C15ull));
  return h ? h : 1u;
}

// ---------------------------------------------------------------- CQL values
// (cdr.h cdr_load_cql_rows) the reader stands inside a UDT value: [pos, end) are its fields
// the next field's [bytes]: false = null, absent (the UDT ended: fewer fields) or an error
__device__ __forceinline__ bool cq_val(Rd& r, Span* v) {
  *v = Span{0, 0};
  if (!r.ok() || r.pos == r.end) return false;
  const int32_t len = (int32_t)r.be32();
  if (!r.ok()) return false;
  if (len < 0) {
    if (len != -1) r.err = CDR_DEC_BAD_SIZE;
    return false;
  }
  if (!r.need((uint32_t)len)) return false;
  *v = Span{r.pos, (uint32_t)len};
  r.pos += (uint32_t)len;
  return true;
}
// a fixed-size value: false = the type's zero (null, empty, or an error)
__device__ __forceinline__ bool cq_fixed(Rd& r, uint32_t size, Span* v) {
  if (!cq_val(r, v) || v->n == 0) return false;
  if (v->n != size) {
    r.err = CDR_LOAD_E_CQL_SIZE;
    return false;
  }
  return true;
}
__device__ __forceinline__ uint64_t be64_at(Rd& r, uint64_t at) {
  uint64_t v = 0;
  for (uint32_t i = 0; i < 8; i++) v = (v << 8) | r.at(at + i);
  return v;
}
__device__ __forceinline__ uint32_t be32_at(Rd& r, uint64_t at) {
  return (r.at(at) << 24) | (r.at(at + 1) << 16) | (r.at(at + 2) << 8) | r.at(at + 3);
}
__device__ __forceinline__ int64_t cq_i64(Rd& r) {
  Span v;
  return cq_fixed(r, 8, &v) ? (int64_t)be64_at(r, v.at) : 0;
}
__device__ __forceinline__ int32_t cq_i32(Rd& r) {
  Span v;
  return cq_fixed(r, 4, &v) ? (int32_t)be32_at(r, v.at) : 0;
}
__device__ __forceinline__ uint32_t cq_bool(Rd& r, uint32_t bit) {
  Span v;
  return cq_fixed(r, 1, &v) && r.at(v.at) ? bit : 0u;
}
// a timestamp, milliseconds -> UnixNano; null or empty: Go's zero time
__device__ __forceinline__ int64_t cq_time(Rd& r) {
  Span v;
  if (!cq_fixed(r, 8, &v)) return CDR_ZERO_TIME_NANOS;
  const int64_t ms = (int64_t)be64_at(r, v.at);
  if (ms > 9223372036854ll || ms < -9223372036854ll) {  // ms * 1e6 leaves int64
    r.err = CDR_LOAD_E_SHAPE;
    return 0;
  }
  return ms * 1000000ll;
}
__device__ __forceinline__ Span cq_text(Rd& r) {  // text / blob: null is ""
  Span v;
  cq_val(r, &v);
  return v.n ? v : Span{0, 0};
}
// list<text>: the value's bytes from its count to the end of its last element (the thrift
// list<string> body without its type byte); null, empty or count 0: none
__device__ __forceinline__ Span cq_list_text(Rd& r) {
  Span v;
  if (!cq_val(r, &v) || v.n == 0) return Span{0, 0};
  uint64_t p = v.at;
  const uint64_t e = v.at + v.n;
  if (e - p < 4) {
    r.err = CDR_DEC_TRUNCATED;
    return Span{0, 0};
  }
  const int32_t cnt = (int32_t)be32_at(r, p);
  p += 4;
  if (cnt < 0) {
    r.err = CDR_DEC_BAD_SIZE;
    return Span{0, 0};
  }
  for (int32_t k = 0; k < cnt; k++) {
    if (e - p < 4) {
      r.err = CDR_DEC_TRUNCATED;
      return Span{0, 0};
    }
    const int32_t len = (int32_t)be32_at(r, p);
    p += 4;
    if (len < 0) {  // a null element included
      r.err = CDR_DEC_BAD_SIZE;
      return Span{0, 0};
    }
    if (e - p < (uint64_t)len) {
      r.err = CDR_DEC_TRUNCATED;
      return Span{0, 0};
    }
    p += (uint64_t)len;
  }
  return cnt ? Span{v.at, (uint32_t)(p - v.at)} : Span{0, 0};
}
// cdr_str_hash of 0B + the list body b; the bytes go to `out` as well when it is not null
// (inline: a call would take the reader by address and so move it to scratch for the whole row)
__device__ __forceinline__ uint64_t list_hash(Rd& r, Span b, uint8_t* out) {
  uint64_t h = 0xCBF29CE484222325ull;
  const uint64_t n = (uint64_t)b.n + 1;
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t c = i == 0 ? (uint32_t)T_STRING : r.at(b.at + (i - 1));
    h = (h ^ c) * 0x100000001B3ull;
    if (out) out[i] = (uint8_t)c;
  }
  h = cdr_mix64(h ^ (n * 0x9E3779B97F4A7C15ull));
  return h ? h : 1u;
}
// a uuid: its 16 bytes; null or empty: none
__device__ __forceinline__ Span cq_uuid(Rd& r) {
  Span v;
  return cq_fixed(r, 16, &v) ? v : Span{0, 0};
}
// a parent's ID: sixteen zero bytes and the writer's sentinel (x0000000-0000-f000-f000-000000000000,
// `hi` its first 8 bytes) are none
__device__ __forceinline__ Span cq_parent_uuid(Rd& r, uint64_t hi_none) {
  const Span v = cq_uuid(r);
  if (!v.n) return v;
  const uint64_t hi = be64_at(r, v.at), lo = be64_at(r, v.at + 8);
  const bool none = (hi == 0 && lo == 0) || (hi == hi_none && lo == 0xf000'000000000000ull);
  return none ? Span{0, 0} : v;
}
// map<text, blob>: the value's bytes from its count to the end of its last pair and the count;
// null, empty or count 0: none.  Every length is checked here, so a later walk of the pairs
// stays inside the span.
__device__ __forceinline__ Span cq_map_blob(Rd& r, uint32_t* n_pairs) {
  *n_pairs = 0;
  Span v;
  if (!cq_val(r, &v) || v.n == 0) return Span{0, 0};
  uint64_t p = v.at;
  const uint64_t e = v.at + v.n;
  if (e - p < 4) {
    r.err = CDR_DEC_TRUNCATED;
    return Span{0, 0};
  }
  const int32_t cnt = (int32_t)be32_at(r, p);
  p += 4;
  if (cnt < 0) {
    r.err = CDR_DEC_BAD_SIZE;
    return Span{0, 0};
  }
  for (int64_t k = 0; k < 2 * (int64_t)cnt; k++) {  // (each element takes 4 bytes at least: bounded by the value)
    if (e - p < 4) {
      r.err = CDR_DEC_TRUNCATED;
      return Span{0, 0};
    }
    const int32_t len = (int32_t)be32_at(r, p);
    p += 4;
    if (len < 0) {  // a null element included
      r.err = CDR_DEC_BAD_SIZE;
      return Span{0, 0};
    }
    if (e - p < (uint64_t)len) {
      r.err = CDR_DEC_TRUNCATED;
      return Span{0, 0};
    }
    p += (uint64_t)len;
  }
  *n_pairs = (uint32_t)cnt;
  return cnt ? Span{v.at, (uint32_t)(p - v.at)} : Span{0, 0};
}
// one [bytes] element of a collection the reader stands in: a missing one is truncation, a
// null one an error unless `null_ok` (then it is empty)
__device__ __forceinline__ void cq_elem(Rd& r, Span* v, bool null_ok) {
  *v = Span{0, 0};
  const int32_t len = (int32_t)r.be32();
  if (!r.ok()) return;
  if (len < 0) {
    if (len != -1 || !null_ok) r.err = CDR_DEC_BAD_SIZE;
    return;
  }
  if (!r.need((uint32_t)len)) return;
  *v = Span{r.pos, (uint32_t)len};
  r.pos += (uint32_t)len;
}
// one [bytes] of a map's pair delimited (the key, then the UDT): its length, -1 = null
__device__ __forceinline__ int32_t cq_delimit(Rd& r) {
  const int32_t len = (int32_t)r.be32();
  if (!r.ok()) return -1;
  if (len < -1) {
    r.err = CDR_DEC_BAD_SIZE;
    return -1;
  }
  if (len > 0 && r.need((uint32_t)len)) r.pos += (uint32_t)len;
  return len;
}

// ---------------------------------------------------------------- the rows
template <int TBL> struct RecOf;
template <> struct RecOf<0> { typedef cdr_activity_info type; };
template <> struct RecOf<1> { typedef cdr_timer_info type; };
template <> struct RecOf<2> { typedef cdr_child_info type; };
template <> struct RecOf<3> { typedef cdr_cancel_info type; };
template <> struct RecOf<4> { typedef cdr_signal_info type; };

// what the walk of one row leaves: the record's scalar fields, and where its strings are
template <int TBL>
struct Row {
  typename RecOf<TBL>::type rec;
  Span sp[4];         // the table's handle fields, in the order of finish()
  Span uu;            // the request-ID text (tables 2-4)
  Span run;           // table 2: StartedRunID
  int64_t started26;  // table 0: StartedTimeNanos (absent: 0)
  int64_t hb_ns;      // table 0, Cassandra form: last_hb_updated_time as UnixNano
  Span tid;           // table 1, Cassandra form: timer_id

  __device__ __forceinline__ void clear() {
    uint64_t* z = reinterpret_cast<uint64_t*>(&rec);
#pragma unroll
    for (uint32_t i = 0; i < sizeof(rec) / 8; i++) z[i] = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) sp[i] = Span{0, 0};
    uu = run = tid = Span{0, 0};
    started26 = 0;
    hb_ns = CDR_ZERO_TIME_NANOS;
  }

  // The Cassandra form: r stands at a map pair (the key's length word).  The key is stepped
  // over, the UDT's length bounds the walk, and the fields come in declaration order
  // (schema.cql:149-228), each one bounded [bytes] read; the first finding stops the walk.
  __device__ __forceinline__ void parse_cql(Rd& r) {
    clear();
    cq_delimit(r);
    {
      const int32_t len = (int32_t)r.be32();
      if (r.ok() && len < -1) r.err = CDR_DEC_BAD_SIZE;
      if (!r.ok()) return;
      if (len > 0 && !r.need((uint32_t)len)) return;
      r.end = r.pos + (len > 0 ? (uint32_t)len : 0u);
    }
    if constexpr (TBL == 0) {  // activity_info
      cdr_activity_info& a = rec;
      a.version = cq_i64(r);
      a.schedule_id = cq_i64(r);
      a.scheduled_event_batch_id = cq_i64(r);
      cq_text(r);  // scheduled_event
      a.scheduled_time = cq_time(r);
      a.started_id = cq_i64(r);
      cq_text(r);  // started_event
      started26 = cq_time(r);
      sp[0] = cq_text(r);
      sp[1] = cq_text(r);
      cq_text(r);  // details
      a.s2s = cq_i32(r);
      a.s2c = cq_i32(r);
      a.stc = cq_i32(r);
      a.hb = cq_i32(r);
      a.flags |= cq_bool(r, CDR_AI_CANCEL_REQUESTED);
      a.cancel_request_id = cq_i64(r);
      hb_ns = cq_time(r);
      a.timer_task_status = cq_i32(r);
      a.attempt = cq_i32(r);
      sp[2] = cq_text(r);
      cq_text(r);  // started_identity
      a.flags |= cq_bool(r, CDR_AI_HAS_RETRY);
      a.initial_interval = cq_i32(r);
      a.backoff_coefficient = __longlong_as_double((long long)cq_i64(r));
      a.maximum_interval = cq_i32(r);
      a.expiration_time = cq_time(r);
      a.maximum_attempts = cq_i32(r);
      sp[3] = cq_list_text(r);
      cq_text(r);  // last_failure_reason
      cq_text(r);  // last_worker_identity
      cq_text(r);  // last_failure_details
      cq_text(r);  // event_data_encoding
    } else if constexpr (TBL == 1) {  // timer_info
      cdr_timer_info& x = rec;
      x.version = cq_i64(r);
      tid = cq_text(r);
      x.started_id = cq_i64(r);
      x.expiry_time = cq_time(r);
      x.task_id = cq_i64(r);
    } else if constexpr (TBL == 2) {  // child_execution_info
      cdr_child_info& c = rec;
      c.version = cq_i64(r);
      c.initiated_id = cq_i64(r);
      c.initiated_event_batch_id = cq_i64(r);
      cq_text(r);  // initiated_event
      c.started_id = cq_i64(r);
      sp[0] = cq_text(r);
      Span u;
      if (cq_fixed(r, 16, &u)) {  // started_run_id: zero and the writer's emptyRunID are none
        const uint64_t hi = be64_at(r, u.at), lo = be64_at(r, u.at + 8);
        const bool none = (hi == 0 && lo == 0) || (hi == 0x30000000'0000'f000ull && lo == 0xf000'000000000000ull);
        run = none ? Span{0, 0} : u;
      }
      cq_text(r);  // started_event
      if (cq_fixed(r, 16, &u)) {
        c.create_request_hi = be64_at(r, u.at);
        c.create_request_lo = be64_at(r, u.at + 8);
      }
      cq_text(r);  // event_data_encoding
      sp[1] = cq_text(r);
      sp[2] = cq_text(r);
      c.parent_close_policy = cq_i32(r);
    } else if constexpr (TBL == 3) {  // request_cancel_info
      cdr_cancel_info& c = rec;
      c.version = cq_i64(r);
      c.initiated_event_batch_id = cq_i64(r);
      c.initiated_id = cq_i64(r);
      uu = cq_text(r);
    } else {  // signal_info
      cdr_signal_info& g = rec;
      g.version = cq_i64(r);
      g.initiated_event_batch_id = cq_i64(r);
      g.initiated_id = cq_i64(r);
      Span u;
      if (cq_fixed(r, 16, &u)) {
        g.signal_request_hi = be64_at(r, u.at);
        g.signal_request_lo = be64_at(r, u.at + 8);
      }
      sp[0] = cq_text(r);
      sp[1] = cq_text(r);
      sp[2] = cq_text(r);
    }
  }

  __device__ __forceinline__ void parse(Rd& r) {
    uint64_t* z = reinterpret_cast<uint64_t*>(&rec);
#pragma unroll
    for (uint32_t i = 0; i < sizeof(rec) / 8; i++) z[i] = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) sp[i] = Span{0, 0};
    uu = run = Span{0, 0};
    started26 = 0;
    if constexpr (TBL == 0) {  // sqlblobs.ActivityInfo
      cdr_activity_info& a = rec;
      fields(r, [&](uint32_t t, uint32_t id) {
        switch (id) {
          case 10: f_i64(r, t, &a.version); break;
          case 12: f_i64(r, t, &a.scheduled_event_batch_id); break;
          case 18: f_i64(r, t, &a.scheduled_time); break;
          case 20: f_i64(r, t, &a.started_id); break;
          case 26: f_i64(r, t, &started26); break;
          case 28: f_str(r, t, &sp[0]); break;
          case 30: f_str(r, t, &sp[1]); break;
          case 32: f_i32(r, t, &a.s2s); break;
          case 34: f_i32(r, t, &a.s2c); break;
          case 36: f_i32(r, t, &a.stc); break;
          case 38: f_i32(r, t, &a.hb); break;
          case 40: f_bool(r, t, &a.flags, CDR_AI_CANCEL_REQUESTED); break;
          case 42: f_i64(r, t, &a.cancel_request_id); break;
          case 44: f_i32(r, t, &a.timer_task_status); break;
          case 46: f_i32(r, t, &a.attempt); break;
          case 48: f_str(r, t, &sp[2]); break;
          case 52: f_bool(r, t, &a.flags, CDR_AI_HAS_RETRY); break;
          case 54: f_i32(r, t, &a.initial_interval); break;
          case 56: f_i32(r, t, &a.maximum_interval); break;
          case 58: f_i32(r, t, &a.maximum_attempts); break;
          case 60: f_i64(r, t, &a.expiration_time); break;
          case 62:
            if (t == T_DOUBLE) a.backoff_coefficient = __longlong_as_double((long long)r.be64());
            else skip1(r, t);
            break;
          case 64:
            if (t == T_LIST) {  // RetryNonRetryableErrors: the list's bytes; empty / not strings -> 0
              const uint64_t at = r.pos;
              const uint32_t et = r.u8();
              const int32_t cnt = r.size();
              r.pos = r.ok() ? at : r.pos;
              skip1(r, T_LIST);
              if (r.ok()) sp[3] = (et == T_STRING && cnt > 0) ? Span{at, (uint32_t)(r.pos - at)} : Span{0, 0};
            } else skip1(r, t);
            break;
          default: skip1(r, t); break;  // event blobs, encodings, identities, the Retry*Last* fields
        }
      });
    } else if constexpr (TBL == 1) {  // sqlblobs.TimerInfo
      cdr_timer_info& x = rec;
      fields(r, [&](uint32_t t, uint32_t id) {
        switch (id) {
          case 10: f_i64(r, t, &x.version); break;
          case 12: f_i64(r, t, &x.started_id); break;
          case 14: f_i64(r, t, &x.expiry_time); break;
          case 16: f_i64(r, t, &x.task_id); break;
          default: skip1(r, t); break;
        }
      });
    } else if constexpr (TBL == 2) {  // sqlblobs.ChildExecutionInfo
      cdr_child_info& c = rec;
      fields(r, [&](uint32_t t, uint32_t id) {
        switch (id) {
          case 10: f_i64(r, t, &c.version); break;
          case 12: f_i64(r, t, &c.initiated_event_batch_id); break;
          case 14: f_i64(r, t, &c.started_id); break;
          case 20: f_str(r, t, &sp[0]); break;
          case 22: f_str(r, t, &run); break;
          case 28: f_str(r, t, &uu); break;
          case 30: f_str(r, t, &sp[1]); break;
          case 32: f_str(r, t, &sp[2]); break;
          case 35: f_i32(r, t, &c.parent_close_policy); break;
          default: skip1(r, t); break;
        }
      });
    } else if constexpr (TBL == 3) {  // sqlblobs.RequestCancelInfo
      cdr_cancel_info& c = rec;
      fields(r, [&](uint32_t t, uint32_t id) {
        switch (id) {
          case 10: f_i64(r, t, &c.version); break;
          case 11: f_i64(r, t, &c.initiated_event_batch_id); break;
          case 12: f_str(r, t, &uu); break;
          default: skip1(r, t); break;
        }
      });
    } else {  // sqlblobs.SignalInfo
      cdr_signal_info& g = rec;
      fields(r, [&](uint32_t t, uint32_t id) {
        switch (id) {
          case 10: f_i64(r, t, &g.version); break;
          case 11: f_i64(r, t, &g.initiated_event_batch_id); break;
          case 12: f_str(r, t, &uu); break;
          case 14: f_str(r, t, &sp[0]); break;
          case 16: f_str(r, t, &sp[1]); break;
          case 18: f_str(r, t, &sp[2]); break;
          default: skip1(r, t); break;
        }
      });
    }
  }
};

template <int TBL, int P, bool CQL>
__global__ __launch_bounds__(CDR_LOAD_BLOCK) void k_rows(LCtx C) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  LDS3 uint4* stage = (LDS3 uint4*)ld_lds + (uint64_t)wv * (CDR_LOAD_STAGE / 16);
  uint64_t s_lo, s_n;
  stage_blobs(C.bytes, C.blob_off, C.total, CDR_LOAD_STAGE, C.n_rows, r - lane, lane, stage, &s_lo, &s_n);
  // the wave's LDS writes complete before any of its lanes reads them (one wave: in order)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  uint64_t n_str = 0;
  if (r < C.n_rows) {
    const uint32_t w = C.row_entry[r];
    // INTERN: rows whose entry can still succeed; FILL: rows whose entry succeeded
    const bool live = P == COUNT || (C.fail[w] == NO_FAIL && (P == INTERN || C.fail[C.n_entries + w] == NO_FAIL));
    if (live) {
      Rd rd;
      // (the Cassandra form: the pair's own lengths, checked by the split, bound the walk)
      const uint64_t e = CQL ? C.total : umin64(C.blob_off[r + 1], C.total), p = umin64(C.blob_off[r], e);
      rd.init(C.bytes, p, e, C.total);
      rd.sb = (const LDS3 uint8_t*)stage;
      rd.s_lo = s_lo;
      rd.s_n = s_n;
      Row<TBL> x;
      if constexpr (CQL) x.parse_cql(rd);
      else x.parse(rd);
      int32_t err = rd.err;
      if constexpr (CQL && TBL != 1) {  // the key is the UDT's own field
        if constexpr (TBL == 0) {
          if (P == COUNT) C.key_out[r] = x.rec.schedule_id;
        } else {
          if (P == COUNT) C.key_out[r] = x.rec.initiated_id;
        }
      }
      // a handle field by pass: counted, interned, or looked up
      auto H = [&](Span s) -> uint32_t {
        if (s.n == 0) return 0u;
        if (P == COUNT) {
          n_str++;
          return 0u;
        }
        const uint64_t h = rd.hash(s.at, s.n);
        if (P == INTERN) {
          tab_insert(C.T, h, s.at, s.n, UNASSIGNED);
          return 0u;
        }
        return tab_lookup(C.T, h);
      };
      if (err == CDR_DEC_OK) {
        if constexpr (TBL == 0) {
          cdr_activity_info& a = x.rec;
          if constexpr (!CQL) a.schedule_id = C.key[r];
          if (x.started26 != CDR_ZERO_TIME_NANOS) {
            a.flags |= CDR_AI_STARTED_TIME_SET;
            a.started_time = x.started26;
          }
          const int64_t hb = CQL ? x.hb_ns : C.hb[r];
          a.last_heartbeat_time = hb != CDR_ZERO_TIME_NANOS ? hb : 0;
          if (a.last_heartbeat_time != 0 && !(a.flags & CDR_AI_STARTED_TIME_SET)) a.flags |= CDR_AI_HEARTBEAT_TIME_SET;
          a.activity_id = H(x.sp[0]);
          a.request_id = H(x.sp[1]);
          a.task_list = H(x.sp[2]);
          if constexpr (CQL) {  // the list body gets its type byte in the row's share of gen_bytes
            const Span b = x.sp[3];
            if (P == COUNT) {
              n_str += b.n ? 1u : 0u;
              C.gneed[r] = b.n ? (uint64_t)b.n + 1 : 0u;
            } else if (b.n) {
              if (P == INTERN) {
                const uint64_t g = C.goff[r];
                if (g + b.n + 1 <= C.goff[r + 1]) {
                  const uint64_t h = list_hash(rd, b, C.gen + C.gen_base + g);
                  tab_insert(C.T, h, (C.gen_base + g) | GEN_REF, b.n + 1, UNASSIGNED);
                }
              } else {
                a.nonretriable = tab_lookup(C.T, list_hash(rd, b, nullptr));
              }
            }
          } else {
            a.nonretriable = H(x.sp[3]);
          }
        } else if constexpr (TBL == 1) {
          Span id = x.tid;
          if constexpr (!CQL) {
            const uint64_t e2 = umin64(C.tid_off[r + 1], C.total), p2 = umin64(C.tid_off[r], e2);
            id = Span{p2, (uint32_t)(e2 - p2)};
          }
          if (P == COUNT) n_str += id.n ? 1u : 0u;
          if (P == INTERN) {
            const uint64_t h = id.n ? rd.hash(id.at, id.n) : 0ull;
            if (id.n) tab_insert(C.T, h, id.at, id.n, UNASSIGNED);
            C.tkey[r] = (int64_t)h;
          }
          if (P == FILL) x.rec.timer_id = (uint32_t)C.tkey[r];
        } else if constexpr (TBL == 2) {
          cdr_child_info& c = x.rec;
          if constexpr (!CQL) {
            c.initiated_id = C.key[r];
            if (!parse_uuid(rd, x.uu, &c.create_request_lo, &c.create_request_hi)) err = CDR_LOAD_E_UUID;
            if (x.run.n != 0 && x.run.n != 16) err = CDR_LOAD_E_UUID;
          }
          if (err == CDR_DEC_OK) {
            c.started_workflow_id = H(x.sp[0]);
            c.domain_name = H(x.sp[1]);
            c.workflow_type = H(x.sp[2]);
            if (P == COUNT) n_str += x.run.n ? 1u : 0u;
            if (P == INTERN) {  // the run ID's text, for k_gen_intern (first byte 0: none)
              uint32_t* g = reinterpret_cast<uint32_t*>(C.gen + (uint64_t)GEN_BYTES * r);
              if (x.run.n) {
                for (uint32_t i = 0; i < GEN_BYTES; i += 4)
                  g[i >> 2] = uuid_char(rd, x.run.at, i) | (uuid_char(rd, x.run.at, i + 1) << 8) |
                              (uuid_char(rd, x.run.at, i + 2) << 16) | (uuid_char(rd, x.run.at, i + 3) << 24);
              } else {
                g[0] = 0;
              }
            }
            if (P == FILL) c.started_run_id = x.run.n ? tab_lookup(C.T, uuid_text_hash(rd, x.run.at)) : 0u;
          }
        } else if constexpr (TBL == 3) {
          cdr_cancel_info& c = x.rec;
          if constexpr (!CQL) c.initiated_id = C.key[r];
          if (!parse_uuid(rd, x.uu, &c.cancel_request_lo, &c.cancel_request_hi)) err = CDR_LOAD_E_UUID;
        } else {
          cdr_signal_info& g = x.rec;
          if constexpr (!CQL) {
            g.initiated_id = C.key[r];
            if (!parse_uuid(rd, x.uu, &g.signal_request_lo, &g.signal_request_hi)) err = CDR_LOAD_E_UUID;
          }
          if (err == CDR_DEC_OK) {
            g.signal_name = H(x.sp[0]);
            g.input = H(x.sp[1]);
            g.control = H(x.sp[2]);
          }
        }
      }
      if (P == COUNT) {
        C.status[r] = err;
        if (err != CDR_DEC_OK) atomicMin(&C.fail[w], fail_word(TBL, r - umin32(C.row0[w], r), err));
        if constexpr (CQL && TBL == 0) {
          if (err != CDR_DEC_OK) C.gneed[r] = 0;
        }
      }
      if (P == FILL) {
        const uint32_t d = C.dest[r];
        if (d < C.n_rows) {  // (unranked: a row outside its entry's range, malformed entry_row0)
          typedef typename RecOf<TBL>::type Rec;
          const uint64_t* s = reinterpret_cast<const uint64_t*>(&x.rec);
          uint64_t* o = reinterpret_cast<uint64_t*>(reinterpret_cast<Rec*>(C.recs) + d);
#pragma unroll
          for (uint32_t i = 0; i < sizeof(Rec) / 8; i++) o[i] = s[i];
        }
      }
    } else if (P == INTERN && TBL == 1) {
      C.tkey[r] = 0;
    }
  }
  if (P == COUNT) {  // the table's size: string fields, one atomic per wave
    for (int o = 32; o > 0; o >>= 1) n_str += __shfl_down(n_str, o, 64);
    if (lane == 0 && n_str) atomicAdd(C.totals, (unsigned long long)n_str);
  }
}

// ---------------------------------------------------------------- the execution rows
// One lane per entry, the same three passes (cdr.h cdr_load_state).  The walk of the row records
// its scalars and where its strings, maps and nested blobs are; every pass then derives the
// status, the builder and the item counts again from those, level by level through the nested
// blobs (a level's walk has skipped, and so checked, everything below it), and names each
// handle field in the same order: COUNT counts them and the entry's gen_bytes need, INTERN
// inserts them (UUID texts and the Memo body written into the entry's share of gen_bytes
// first), FILL looks them up and stores the records whole.
struct XCnt {  // per entry: version-history items, reset points, search-attribute rows, gen bytes
  uint64_t v[4];
};
struct XCntAdd {
  __host__ __device__ __forceinline__ XCnt operator()(const XCnt& a, const XCnt& b) const {
    return XCnt{{a.v[0] + b.v[0], a.v[1] + b.v[1], a.v[2] + b.v[2], a.v[3] + b.v[3]}};
  }
};

struct XCtx {
  const uint8_t* bytes;
  uint64_t total;
  cdr_exec_rows_in in;
  const uint8_t* seed_bytes;
  const uint64_t* seed_off;
  uint32_t n_seeds, n_entries;
  unsigned long long* fail;
  STab T;
  int32_t* status;             // [n_entries]
  unsigned long long* totals;  // COUNT: string fields
  XCnt* cnt;                   // COUNT writes
  const XCnt* off;             // its exclusive scan, [n_entries + 1]
  uint8_t* gen;                // the execution rows' part of gen_bytes, at offset gen_base
  uint64_t gen_base;
  cdr_exec_info* exec;
  cdr_repl_state* repl;
  cdr_exec_persist* persist;
  uint32_t* builder;
  cdr_vh_item* vh;
  cdr_reset_point* rp;
  cdr_kv* sa;
  uint32_t* n_sa;  // FILL: distinct search-attribute keys, for the epilogue
  // the Cassandra form only (in.blob_off: the execution column's offsets)
  const uint64_t *rs_off, *vhb_off, *vhe_off;  // replication_state, version_histories, its encoding
};

struct U16 {  // 16 bytes, big-endian
  uint64_t hi, lo;
};
__device__ __forceinline__ U16 u16_at(Rd& r, uint64_t at) {
  U16 u{0, 0};
  for (uint32_t i = 0; i < 8; i++) u.hi = (u.hi << 8) | r.at(at + i);
  for (uint32_t i = 8; i < 16; i++) u.lo = (u.lo << 8) | r.at(at + i);
  return u;
}
__device__ __forceinline__ U16 u16_col(const uint8_t* p) {
  U16 u{0, 0};
  for (uint32_t i = 0; i < 8; i++) u.hi = (u.hi << 8) | p[i];
  for (uint32_t i = 8; i < 16; i++) u.lo = (u.lo << 8) | p[i];
  return u;
}
__device__ __forceinline__ uint32_t u16_char(U16 u, uint32_t i) {  // character i of UUID(b).String()
  if (i == 8 || i == 13 || i == 18 || i == 23) return '-';
  const uint32_t d = i - (i > 8 ? 1u : 0u) - (i > 13 ? 1u : 0u) - (i > 18 ? 1u : 0u) - (i > 23 ? 1u : 0u);
  const uint32_t nib = (uint32_t)(((d < 16 ? u.hi : u.lo) >> (60u - 4u * (d & 15u))) & 15u);
  return nib < 10 ? '0' + nib : 'a' + (nib - 10);
}
__device__ __forceinline__ uint64_t u16_hash(U16 u) {  // cdr_str_hash of that text
  uint64_t h = 0xCBF29CE484222325ull;
  for (uint32_t i = 0; i < GEN_BYTES; i++) h = (h ^ u16_char(u, i)) * 0x100000001B3ull;
  h = cdr_mix64(h ^ ((uint64_t)GEN_BYTES * 0x9E3779B97F4A7C15ull));
  return h ? h : 1u;
}
// cdr_str_hash of a Memo struct's wire body around the map body m (0D 00 0A, m, 00); the
// bytes go to `out` as well when it is not null
__device__ uint64_t memo_hash(Rd& r, Span m, uint8_t* out) {
  uint64_t h = 0xCBF29CE484222325ull;
  const uint64_t n = (uint64_t)m.n + 4;
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t c = i == 0 ? 0x0Du : i == 2 ? 0x0Au : (i == 1 || i == n - 1) ? 0u : r.at(m.at + (i - 3));
    h = (h ^ c) * 0x100000001B3ull;
    if (out) out[i] = (uint8_t)c;
  }
  h = cdr_mix64(h ^ (n * 0x9E3779B97F4A7C15ull));
  return h ? h : 1u;
}

// the Cassandra form's: 0D 00 0A 0B 0B, the CQL map body m (count and pairs), 00
__device__ __forceinline__ uint64_t memo_hash_cql(Rd& r, Span m, uint8_t* out) {
  uint64_t h = 0xCBF29CE484222325ull;
  const uint64_t n = (uint64_t)m.n + 6;
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t c = i == 0                        ? 0x0Du
                       : i == 2                      ? 0x0Au
                       : (i == 3 || i == 4)          ? 0x0Bu
                       : (i == 1 || i == n - 1)      ? 0u
                                                     : r.at(m.at + (i - 5));
    h = (h ^ c) * 0x100000001B3ull;
    if (out) out[i] = (uint8_t)c;
  }
  h = cdr_mix64(h ^ (n * 0x9E3779B97F4A7C15ull));
  return h ? h : 1u;
}

__device__ __forceinline__ Rd sub_reader(const Rd& r, uint64_t at, uint64_t n) {  // over [at, at + n) of the same bytes
  Rd q = r;
  q.pos = at;
  q.end = at + n;
  q.err = CDR_DEC_OK;
  return q;
}
// a list field: element type, count and the bytes of its body (the value skipped, so checked);
// another wire type is skipped and an earlier occurrence stays
__device__ __forceinline__ void f_list(Rd& r, uint32_t t, uint32_t* et, uint32_t* cnt, Span* body) {
  if (t != T_LIST) {
    skip1(r, t);
    return;
  }
  const uint64_t at = r.pos;
  const uint32_t e = r.u8();
  const uint32_t c = (uint32_t)r.size();
  if (!r.ok()) return;
  r.pos = at;
  skip(r, T_LIST);
  if (!r.ok()) return;
  *et = e;
  *cnt = c;
  *body = Span{at, (uint32_t)(r.pos - at)};
}
__device__ __forceinline__ bool f_map(Rd& r, uint32_t t, Span* body) {
  if (t != T_MAP) {
    skip1(r, t);
    return false;
  }
  const uint64_t at = r.pos;
  skip(r, T_MAP);
  if (!r.ok()) return false;
  *body = Span{at, (uint32_t)(r.pos - at)};
  return true;
}
__device__ __forceinline__ bool is_thriftrw(Rd& r, Span s) {
  const char* k = "thriftrw";
  if (s.n != 8) return false;
  bool same = true;
  for (uint32_t i = 0; i < 8; i++) same = same && r.at(s.at + i) == (uint32_t)k[i];
  return same;
}

// a branch token: 0x59, HistoryBranch{10 TreeID, 20 BranchID, 30 Ancestors}
struct Tok {
  Span tree;
  uint64_t lo, hi;
};
__device__ int32_t parse_token(Rd& r, Span s, Tok* out) {
  if (s.n == 0 || r.at(s.at) != 0x59u) return CDR_LOAD_E_ENCODING;
  Rd q = sub_reader(r, s.at + 1, s.n - 1);
  Span tree{0, 0}, bid{0, 0}, anc{0, 0};
  uint32_t et = 0, n_anc = 0;
  fields(q, [&](uint32_t t, uint32_t id) {
    switch (id) {
      case 10: f_str(q, t, &tree); break;
      case 20: f_str(q, t, &bid); break;
      case 30: f_list(q, t, &et, &n_anc, &anc); break;
      default: skip1(q, t); break;
    }
  });
  if (q.err) return q.err;
  if (n_anc) return CDR_LOAD_E_SHAPE;
  if (!parse_uuid(r, bid, &out->lo, &out->hi)) return CDR_LOAD_E_UUID;
  out->tree = tree;
  return CDR_DEC_OK;
}

enum : uint32_t { X_PARENT = 1, X_F18 = 2, X_F44 = 4, X_TOKEN = 8, X_SA = 16, X_MEMO = 32, X_VH = 64 };

// the Cassandra form only: the IDs the SQL form has as key columns, the UDT's own event IDs,
// the maps' pair counts
struct XCqlOnly {
  Span dom, run, wid;
  int64_t next_ev, letid;
  uint32_t n_sam, n_memo;
};
struct XSqlOnly {};

template <bool CQL>
struct XRow : std::conditional<CQL, XCqlOnly, XSqlOnly>::type {  // what the walk of one execution row leaves
  cdr_exec_info x;
  cdr_exec_persist ps;
  int64_t f44, f80, f82, f94, f106;
  uint32_t has;
  Span pdom, pwf, prun, tl, wt, ctx, crq, drq, stl, nonret, cron, token, clv, cfv, cimpl;
  Span rpb, rpenc, vhb, vhenc, lri, sam, memo;

  // The Cassandra form: r stands at the first field of the `execution` UDT value and ends
  // with it.  The 58 fields in declaration order (schema.cql:23-82), one bounded [bytes]
  // read each; the first finding stops the walk (every later read gives the type's zero).
  __device__ __forceinline__ void parse_cql(Rd& r) {
    {
      uint64_t* z = reinterpret_cast<uint64_t*>(&x);
#pragma unroll
      for (uint32_t i = 0; i < sizeof(x) / 8; i++) z[i] = 0;
      z = reinterpret_cast<uint64_t*>(&ps);
#pragma unroll
      for (uint32_t i = 0; i < sizeof(ps) / 8; i++) z[i] = 0;
    }
    f44 = 0;
    lri = vhb = vhenc = Span{0, 0};
    this->dom = cq_uuid(r);
    this->wid = cq_text(r);
    this->run = cq_uuid(r);
    pdom = cq_parent_uuid(r, 0x10000000'0000'f000ull);  // emptyDomainID
    pwf = cq_text(r);
    prun = cq_parent_uuid(r, 0x30000000'0000'f000ull);  // emptyRunID
    x.initiated_id = cq_i64(r);
    x.completion_event_batch_id = cq_i64(r);
    cq_text(r);  // completion_event
    cq_text(r);  // completion_event_data_encoding
    tl = cq_text(r);
    wt = cq_text(r);
    x.workflow_timeout = cq_i32(r);
    x.decision_timeout_value = cq_i32(r);
    ctx = cq_text(r);
    x.state = cq_i32(r);
    x.close_status = cq_i32(r);
    x.last_processed_event = cq_i64(r);
    ps.start_time = cq_time(r);
    ps.last_updated_time = cq_time(r);
    crq = cq_uuid(r);
    x.decision_version = cq_i64(r);
    x.decision_schedule_id = cq_i64(r);
    x.decision_started_id = cq_i64(r);
    drq = cq_text(r);
    x.decision_timeout = cq_i32(r);
    x.decision_attempt = cq_i64(r);
    x.decision_started_ts = cq_i64(r);
    x.decision_scheduled_ts = cq_i64(r);
    x.decision_original_scheduled_ts = cq_i64(r);
    x.flags |= cq_bool(r, CDR_XI_CANCEL_REQUESTED);
    cq_text(r);  // cancel_request_id
    stl = cq_text(r);
    f80 = cq_i32(r);
    clv = cq_text(r);
    cfv = cq_text(r);
    cimpl = cq_text(r);
    f82 = cq_i32(r);
    x.flags |= cq_bool(r, CDR_XI_HAS_RETRY);
    x.initial_interval = cq_i32(r);
    x.backoff_coefficient = __longlong_as_double((long long)cq_i64(r));
    x.maximum_interval = cq_i32(r);
    f94 = cq_time(r);
    x.maximum_attempts = cq_i32(r);
    nonret = cq_list_text(r);
    cq_i32(r);  // event_store_version
    f106 = cq_i32(r);
    token = cq_text(r);
    ps.history_size = cq_i64(r);
    x.last_first_event_id = cq_i64(r);
    this->next_ev = cq_i64(r);
    cron = cq_text(r);
    x.expiration_seconds = cq_i32(r);
    this->letid = cq_i64(r);
    rpb = cq_text(r);
    rpenc = cq_text(r);
    sam = cq_map_blob(r, &this->n_sam);
    memo = cq_map_blob(r, &this->n_memo);
    // a parent that is none with the writer's emptyInitiatedID: what a replay leaves (cdr.h)
    if (!pdom.n && x.initiated_id == -7) x.initiated_id = CDR_EMPTY_EVENT_ID;
    has = X_PARENT | X_F18 | (token.n ? X_TOKEN : 0u) | (sam.n ? X_SA : 0u) | (memo.n ? X_MEMO : 0u);
  }

  __device__ __forceinline__ void parse(Rd& r) {
    {
      uint64_t* z = reinterpret_cast<uint64_t*>(&x);
#pragma unroll
      for (uint32_t i = 0; i < sizeof(x) / 8; i++) z[i] = 0;
      z = reinterpret_cast<uint64_t*>(&ps);
#pragma unroll
      for (uint32_t i = 0; i < sizeof(ps) / 8; i++) z[i] = 0;
    }
    f44 = f80 = f82 = f94 = f106 = 0;
    has = 0;
    pdom = pwf = prun = tl = wt = ctx = crq = drq = stl = nonret = cron = token = clv = cfv = cimpl = Span{0, 0};
    rpb = rpenc = vhb = vhenc = lri = sam = memo = Span{0, 0};
    auto present = [&](uint32_t t, uint32_t want, uint32_t bit) { has |= t == want ? bit : 0u; };
    fields(r, [&](uint32_t t, uint32_t id) {
      switch (id) {
        case 10: present(t, T_STRING, X_PARENT); f_str(r, t, &pdom); break;
        case 12: f_str(r, t, &pwf); break;
        case 14: f_str(r, t, &prun); break;
        case 16: f_i64(r, t, &x.initiated_id); break;
        case 18: present(t, T_I64, X_F18); f_i64(r, t, &x.completion_event_batch_id); break;
        case 24: f_str(r, t, &tl); break;
        case 26: f_str(r, t, &wt); break;
        case 28: f_i32(r, t, &x.workflow_timeout); break;
        case 30: f_i32(r, t, &x.decision_timeout_value); break;
        case 32: f_str(r, t, &ctx); break;
        case 34: f_i32(r, t, &x.state); break;
        case 36: f_i32(r, t, &x.close_status); break;
        case 38: f_i64(r, t, &ps.start_version); break;
        case 40: f_i64(r, t, &ps.current_version); break;
        case 44: present(t, T_I64, X_F44); f_i64(r, t, &f44); break;
        case 46: f_map(r, t, &lri); break;
        case 50: f_i64(r, t, &x.last_first_event_id); break;
        case 52: f_i64(r, t, &x.last_processed_event); break;
        case 54: f_i64(r, t, &ps.start_time); break;
        case 56: f_i64(r, t, &ps.last_updated_time); break;
        case 58: f_i64(r, t, &x.decision_version); break;
        case 60: f_i64(r, t, &x.decision_schedule_id); break;
        case 62: f_i64(r, t, &x.decision_started_id); break;
        case 64: f_i32(r, t, &x.decision_timeout); break;
        case 66: f_i64(r, t, &x.decision_attempt); break;
        case 68: f_i64(r, t, &x.decision_started_ts); break;
        case 69: f_i64(r, t, &x.decision_scheduled_ts); break;
        case 70: f_bool(r, t, &x.flags, CDR_XI_CANCEL_REQUESTED); break;
        case 71: f_i64(r, t, &x.decision_original_scheduled_ts); break;
        case 72: f_str(r, t, &crq); break;
        case 74: f_str(r, t, &drq); break;
        case 78: f_str(r, t, &stl); break;
        case 80: f_i64(r, t, &f80); break;
        case 82: f_i64(r, t, &f82); break;
        case 84: f_i32(r, t, &x.initial_interval); break;
        case 86: f_i32(r, t, &x.maximum_interval); break;
        case 88: f_i32(r, t, &x.maximum_attempts); break;
        case 90: f_i32(r, t, &x.expiration_seconds); break;
        case 92:
          if (t == T_DOUBLE) x.backoff_coefficient = __longlong_as_double((long long)r.be64());
          else skip1(r, t);
          break;
        case 94: f_i64(r, t, &f94); break;
        case 96: {  // RetryNonRetryableErrors: the list's bytes; empty / not strings -> 0
          uint32_t et = T_STRING, cnt = 0;
          Span body{0, 0};
          const bool lst = t == T_LIST;
          f_list(r, t, &et, &cnt, &body);
          if (lst && r.ok()) nonret = (et == T_STRING && cnt > 0) ? body : Span{0, 0};
          break;
        }
        case 98: f_bool(r, t, &x.flags, CDR_XI_HAS_RETRY); break;
        case 100: f_str(r, t, &cron); break;
        case 104: present(t, T_STRING, X_TOKEN); f_str(r, t, &token); break;
        case 106: f_i64(r, t, &f106); break;
        case 108: f_i64(r, t, &ps.history_size); break;
        case 110: f_str(r, t, &clv); break;
        case 112: f_str(r, t, &cfv); break;
        case 114: f_str(r, t, &cimpl); break;
        case 115: f_str(r, t, &rpb); break;
        case 116: f_str(r, t, &rpenc); break;
        case 118: has |= f_map(r, t, &sam) ? X_SA : 0u; break;
        case 120: has |= f_map(r, t, &memo) ? X_MEMO : 0u; break;
        case 122: present(t, T_STRING, X_VH); f_str(r, t, &vhb); break;
        case 124: f_str(r, t, &vhenc); break;
        default: skip1(r, t); break;  // CompletionEvent and its encoding, CancelRequestID, LastEventTaskID
      }
    });
  }
};

template <class T>
__device__ __forceinline__ void store_whole(T* dst, const T& v) {
  const uint64_t* s = reinterpret_cast<const uint64_t*>(&v);
  uint64_t* o = reinterpret_cast<uint64_t*>(dst);
#pragma unroll
  for (uint32_t i = 0; i < sizeof(T) / 8; i++) o[i] = s[i];
}

template <int P, bool CQL>
__global__ __launch_bounds__(CDR_LOAD_BLOCK) void k_exec(XCtx C) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  LDS3 uint4* stage = (LDS3 uint4*)ld_lds + (uint64_t)wv * (CDR_LOAD_STAGE / 16);
  uint64_t s_lo, s_n;
  stage_blobs(C.bytes, C.in.blob_off, C.total, CDR_LOAD_STAGE, C.n_entries, w - lane, lane, stage, &s_lo, &s_n);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  uint64_t n_str = 0;
  const bool live = w < C.n_entries &&
                    (P == COUNT || (C.fail[w] == NO_FAIL && (P == INTERN || C.fail[C.n_entries + w] == NO_FAIL)));
  if (live) {
    Rd rd;
    const uint64_t e = umin64(C.in.blob_off[w + 1], C.total), p = umin64(C.in.blob_off[w], e);
    rd.init(C.bytes, p, e, C.total);
    rd.sb = (const LDS3 uint8_t*)stage;
    rd.s_lo = s_lo;
    rd.s_n = s_n;
    XRow<CQL> R;
    if constexpr (CQL) {  // the other three columns are small: read through the window
      R.parse_cql(rd);
      uint64_t e2 = umin64(C.vhb_off[w + 1], C.total), p2 = umin64(C.vhb_off[w], e2);
      R.vhb = Span{p2, (uint32_t)(e2 - p2)};
      e2 = umin64(C.vhe_off[w + 1], C.total), p2 = umin64(C.vhe_off[w], e2);
      R.vhenc = Span{p2, (uint32_t)(e2 - p2)};
      e2 = umin64(C.rs_off[w + 1], C.total), p2 = umin64(C.rs_off[w], e2);
      R.lri = Span{p2, (uint32_t)(e2 - p2)};  // the replication_state body
      R.has |= (R.lri.n ? X_F44 : 0u) | (R.vhb.n ? X_VH : 0u);
    } else {
      R.parse(rd);
    }
    int32_t err = rd.err;
    // ---- the status, the builder and the item lists, derived alike in every pass
    uint32_t builder = CDR_BUILDER_LOCAL;
    cdr_repl_state rs;
    {
      uint64_t* z = reinterpret_cast<uint64_t*>(&rs);
#pragma unroll
      for (uint32_t i = 0; i < sizeof(rs) / 8; i++) z[i] = 0;
    }
    Tok tok{Span{0, 0}, 0, 0};
    uint32_t n_rp = 0, n_sa = 0, n_vh = 0;
    bool has_points = false, vh_branch = false;
    Span points{0, 0}, items{0, 0};
    if (!(R.has & X_PARENT)) {
      R.pdom = R.pwf = R.prun = Span{0, 0};
      R.x.initiated_id = CDR_EMPTY_EVENT_ID;
    }
    if (!err && ((R.pdom.n != 0 && R.pdom.n != 16) || (R.prun.n != 0 && R.prun.n != 16))) err = CDR_LOAD_E_UUID;
    bool unknown_cluster = false;
    if constexpr (CQL) {
      // replication_state: current_version, start_version, last_write_version,
      // last_write_event_id, last_replication_info (schema.cql:91-97); its wire findings
      if (!err && (R.has & X_F44)) {
        Rd q = sub_reader(rd, R.lri.at, R.lri.n);
        rs.current_version = cq_i64(q);
        rs.start_version = cq_i64(q);
        rs.last_write_version = cq_i64(q);
        rs.last_write_event_id = cq_i64(q);
        Span m;
        if (cq_val(q, &m) && m.n) {
          Rd mq = sub_reader(q, m.at, m.n);
          const int32_t cnt = (int32_t)mq.be32();
          if (mq.ok() && cnt < 0) mq.err = CDR_DEC_BAD_SIZE;
          for (int32_t k = 0; k < cnt && mq.ok(); k++) {  // (8 bytes a pair at least: bounded by the value)
            Span key, u;
            cq_elem(mq, &key, false);
            cq_elem(mq, &u, true);
            if (!mq.ok()) break;
            Rd uq = sub_reader(mq, u.at, u.n);  // replication_info{version, last_event_id}
            const int64_t ver = cq_i64(uq), last = cq_i64(uq);
            if (uq.err) {
              mq.err = uq.err;
              break;
            }
            uint32_t ci = CDR_MAX_CLUSTERS;
            for (uint32_t i = 0; i < C.in.n_clusters && ci == CDR_MAX_CLUSTERS; i++) {
              const uint32_t s = C.in.cluster_seed[i];
              if (s >= C.n_seeds) continue;
              const uint64_t a = C.seed_off[s], n = C.seed_off[s + 1] - a;
              if (n != key.n) continue;
              bool same = true;
              for (uint32_t j = 0; j < key.n && same; j++) same = rd.at(key.at + j) == C.seed_bytes[a + j];
              if (same) ci = i;
            }
            if (ci == CDR_MAX_CLUSTERS) {
              unknown_cluster = true;
            } else {
              rs.lri_mask |= 1u << ci;
              rs.lri_version[ci] = ver;
              rs.lri_last_event_id[ci] = last;
            }
          }
          if (mq.err) q.err = mq.err;
        }
        err = q.err;
      }
    }
    if (!err && (R.has & X_F44) && (R.has & X_VH)) err = CDR_LOAD_E_SHAPE;
    if (!err && (R.has & X_F44)) {
      builder = CDR_BUILDER_2DC;
      rs.present = 1;
      if constexpr (CQL) {
        R.ps.start_version = rs.start_version;
        R.ps.current_version = rs.current_version;
        if (unknown_cluster) err = CDR_LOAD_E_CLUSTER;
      } else {
        rs.start_version = R.ps.start_version;
        rs.current_version = R.ps.current_version;
        rs.last_write_version = C.in.last_write_version[w];
        rs.last_write_event_id = R.f44;
        if (R.lri.n >= 6 && rd.at(R.lri.at) == T_STRING && rd.at(R.lri.at + 1) == T_STRUCT) {
          Rd q = sub_reader(rd, R.lri.at + 2, R.lri.n - 2);
          const uint32_t cnt = (uint32_t)q.size();
          for (uint32_t k = 0; k < cnt && q.ok() && !err; k++) {
            Span key{0, 0};
            f_str(q, T_STRING, &key);
            int64_t ver = 0, last = 0;
            fields(q, [&](uint32_t t, uint32_t id) {
              switch (id) {
                case 10: f_i64(q, t, &ver); break;
                case 12: f_i64(q, t, &last); break;
                default: skip1(q, t); break;
              }
            });
            uint32_t ci = CDR_MAX_CLUSTERS;
            for (uint32_t i = 0; i < C.in.n_clusters && ci == CDR_MAX_CLUSTERS; i++) {
              const uint32_t s = C.in.cluster_seed[i];
              if (s >= C.n_seeds) continue;
              const uint64_t a = C.seed_off[s], n = C.seed_off[s + 1] - a;
              if (n != key.n) continue;
              bool same = true;
              for (uint32_t j = 0; j < key.n && same; j++) same = rd.at(key.at + j) == C.seed_bytes[a + j];
              if (same) ci = i;
            }
            if (ci == CDR_MAX_CLUSTERS) {
              err = CDR_LOAD_E_CLUSTER;
            } else {
              rs.lri_mask |= 1u << ci;
              rs.lri_version[ci] = ver;
              rs.lri_last_event_id[ci] = last;
            }
          }
        }
      }
    } else if (R.has & X_VH) {
      builder = CDR_BUILDER_NDC;
    }
    if (!err && (R.has & X_TOKEN)) err = parse_token(rd, R.token, &tok);
    if (!err && R.rpb.n) {  // ResetPoints{10 Points}
      if (!is_thriftrw(rd, R.rpenc) || rd.at(R.rpb.at) != 0x59u) {
        err = CDR_LOAD_E_ENCODING;
      } else {
        Rd q = sub_reader(rd, R.rpb.at + 1, R.rpb.n - 1);
        uint32_t et = 0, cnt = 0;
        fields(q, [&](uint32_t t, uint32_t id) {
          if (id == 10) f_list(q, t, &et, &cnt, &points);
          else skip1(q, t);
        });
        err = q.err;
        has_points = points.n != 0 && et == T_STRUCT;
        n_rp = has_points ? cnt : 0u;
        if (!err && n_rp > CDR_LOAD_MAX_RESET_POINTS) err = CDR_LOAD_E_SHAPE;
      }
    }
    if constexpr (CQL) {  // the pairs were delimited in the walk: the counts alone are left
      n_sa = R.n_sam;
      if (!err && (R.n_sam > CDR_LOAD_MAX_SEARCH_ATTR || R.n_memo > CDR_LOAD_MAX_SEARCH_ATTR)) err = CDR_LOAD_E_SHAPE;
    } else if (!err && (R.has & X_SA)) {
      if (rd.at(R.sam.at) == T_STRING && rd.at(R.sam.at + 1) == T_STRING) {
        Rd q = sub_reader(rd, R.sam.at + 2, 4);
        n_sa = (uint32_t)q.size();
      }
      if (n_sa > CDR_LOAD_MAX_SEARCH_ATTR) err = CDR_LOAD_E_SHAPE;
    }
    if (!err && (R.has & X_VH)) {  // VersionHistories{10 index, 20 [VersionHistory{10 token, 20 items}]}
      if (!is_thriftrw(rd, R.vhenc) || R.vhb.n == 0 || rd.at(R.vhb.at) != 0x59u) {
        err = CDR_LOAD_E_ENCODING;
      } else {
        Rd q = sub_reader(rd, R.vhb.at + 1, R.vhb.n - 1);
        int32_t index = 0;
        uint32_t et = 0, cnt = 0;
        Span hs{0, 0};
        fields(q, [&](uint32_t t, uint32_t id) {
          if (id == 10) f_i32(q, t, &index);
          else if (id == 20) f_list(q, t, &et, &cnt, &hs);
          else skip1(q, t);
        });
        err = q.err;
        if (!err && (index != 0 || hs.n == 0 || et != T_STRUCT || cnt != 1)) err = CDR_LOAD_E_SHAPE;
        if (!err) {
          Rd h = sub_reader(rd, hs.at + 5, hs.n - 5);
          Span vt{0, 0};
          uint32_t it = 0, ic = 0;
          fields(h, [&](uint32_t t, uint32_t id) {
            if (id == 10) f_str(h, t, &vt);
            else if (id == 20) f_list(h, t, &it, &ic, &items);
            else skip1(h, t);
          });
          if (vt.n) {
            err = parse_token(rd, vt, &tok);
            if (!err && (R.has & X_TOKEN)) err = CDR_LOAD_E_SHAPE;
            vh_branch = true;
          }
          n_vh = (items.n != 0 && it == T_STRUCT) ? ic : 0u;
          if (!err && n_vh > CDR_LOAD_MAX_VH_ITEMS) err = CDR_LOAD_E_SHAPE;
        }
      }
    }
    if (P == COUNT) {
      C.status[w] = err;
      if (err != CDR_DEC_OK) atomicMin(&C.fail[w], fail_word(CDR_LOAD_TABLES, 0, err));
    }
    XCnt need{{0, 0, 0, 0}};
    if (err == CDR_DEC_OK) {
      const XCnt o0 = P == COUNT ? XCnt{{0, 0, 0, 0}} : C.off[w];
      const XCnt o1 = P == COUNT ? XCnt{{n_vh, n_rp, n_sa, ~0ull}} : C.off[w + 1];
      uint64_t g = o0.v[3];  // the entry's share of gen_bytes: [g, o1.v[3])
      auto H = [&](Span s) -> uint32_t {  // a handle field by pass: counted, interned, or looked up
        if (s.n == 0) return 0u;
        if (P == COUNT) {
          n_str++;
          return 0u;
        }
        const uint64_t h = rd.hash(s.at, s.n);
        if (P == INTERN) {
          tab_insert(C.T, h, s.at, s.n, UNASSIGNED);
          return 0u;
        }
        return tab_lookup(C.T, h);
      };
      auto G = [&](U16 u) -> uint32_t {  // a UUID's text: generated, then as H
        if (P == COUNT) {
          n_str++;
          need.v[3] += GEN_BYTES;
          return 0u;
        }
        const uint64_t h = u16_hash(u);
        if (P == INTERN) {
          if (g + GEN_BYTES <= o1.v[3]) {
            uint32_t* t = reinterpret_cast<uint32_t*>(C.gen + g);
            for (uint32_t i = 0; i < GEN_BYTES; i += 4)
              t[i >> 2] = u16_char(u, i) | (u16_char(u, i + 1) << 8) | (u16_char(u, i + 2) << 16) |
                          (u16_char(u, i + 3) << 24);
            tab_insert(C.T, h, (C.gen_base + g) | GEN_REF, GEN_BYTES, UNASSIGNED);
          }
          g += GEN_BYTES;
          return 0u;
        }
        return tab_lookup(C.T, h);
      };
      cdr_exec_info& x = R.x;
      if constexpr (CQL) {  // (a null ID is sixteen zero bytes)
        x.domain_id = G(R.dom.n ? u16_at(rd, R.dom.at) : U16{0, 0});
        x.run_id = G(R.run.n ? u16_at(rd, R.run.at) : U16{0, 0});
        x.workflow_id = H(R.wid);
      } else {
        x.domain_id = G(u16_col(C.in.domain_id + 16ull * w));
        x.run_id = G(u16_col(C.in.run_id + 16ull * w));
        const uint64_t e2 = umin64(C.in.workflow_id_off[w + 1], C.total), p2 = umin64(C.in.workflow_id_off[w], e2);
        x.workflow_id = H(Span{p2, (uint32_t)(e2 - p2)});
      }
      x.parent_domain_id = R.pdom.n ? G(u16_at(rd, R.pdom.at)) : 0u;
      x.parent_run_id = R.prun.n ? G(u16_at(rd, R.prun.at)) : 0u;
      x.parent_workflow_id = H(R.pwf);
      if constexpr (CQL) x.create_request_id = G(R.crq.n ? u16_at(rd, R.crq.at) : U16{0, 0});
      else x.create_request_id = H(R.crq);
      x.task_list = H(R.tl);
      x.workflow_type = H(R.wt);
      x.cron_schedule = H(R.cron);
      if constexpr (CQL) {  // the list body gets its type byte in the entry's share of gen_bytes
        if (R.nonret.n) {
          const uint64_t n = (uint64_t)R.nonret.n + 1;
          if (P == COUNT) {
            n_str++;
            need.v[3] += n;
          } else if (P == INTERN) {
            if (g + n <= o1.v[3]) {
              const uint64_t h = list_hash(rd, R.nonret, C.gen + g);
              tab_insert(C.T, h, (C.gen_base + g) | GEN_REF, (uint32_t)n, UNASSIGNED);
            }
            g += n;
          } else {
            x.nonretriable = tab_lookup(C.T, list_hash(rd, R.nonret, nullptr));
          }
        }
      } else {
        x.nonretriable = H(R.nonret);
      }
      x.branch_tree_id = H(tok.tree);
      x.decision_request_id = H(R.drq);
      if (R.has & X_MEMO) {
        const uint64_t n = (uint64_t)R.memo.n + (CQL ? 6 : 4);
        if (P == COUNT) {
          n_str++;
          need.v[3] += n;
        } else if (P == INTERN) {
          if (g + n <= o1.v[3]) {
            const uint64_t h = CQL ? memo_hash_cql(rd, R.memo, C.gen + g) : memo_hash(rd, R.memo, C.gen + g);
            tab_insert(C.T, h, (C.gen_base + g) | GEN_REF, (uint32_t)n, UNASSIGNED);
          }
          g += n;
        } else {
          x.memo = tab_lookup(C.T, CQL ? memo_hash_cql(rd, R.memo, nullptr) : memo_hash(rd, R.memo, nullptr));
        }
      }
      cdr_exec_persist& ps = R.ps;
      ps.execution_context = H(R.ctx);
      ps.sticky_task_list = H(R.stl);
      ps.client_library_version = H(R.clv);
      ps.client_feature_version = H(R.cfv);
      ps.client_impl = H(R.cimpl);
      // reset points: every pass walks them for their strings
      {
        const uint64_t cap = umin64(n_rp, o1.v[1] - o0.v[1]);
        Rd q = sub_reader(rd, points.at + 5, points.n >= 5 ? points.n - 5 : 0);
        for (uint64_t k = 0; k < cap && q.ok(); k++) {
          cdr_reset_point pt;
          pt.binary_checksum = pt.run_id = 0;
          pt.first_decision_completed_id = pt.created_time_nano = pt.expiring_time_nano = 0;
          pt.flags = pt._pad = 0;
          Span cs{0, 0}, ru{0, 0};
          fields(q, [&](uint32_t t, uint32_t id) {
            const uint32_t bit = id == 10   ? CDR_RP_HAS_CHECKSUM
                                 : id == 20 ? CDR_RP_HAS_RUN_ID
                                 : id == 30 ? CDR_RP_HAS_FIRST_DC_ID
                                 : id == 40 ? CDR_RP_HAS_CREATED
                                 : id == 50 ? CDR_RP_HAS_EXPIRING
                                 : id == 60 ? CDR_RP_HAS_RESETTABLE
                                            : 0u;
            const uint32_t want = id <= 20 ? T_STRING : id == 60 ? T_BOOL : T_I64;
            if (bit && t == want) pt.flags |= bit;
            switch (id) {
              case 10: f_str(q, t, &cs); break;
              case 20: f_str(q, t, &ru); break;
              case 30: f_i64(q, t, &pt.first_decision_completed_id); break;
              case 40: f_i64(q, t, &pt.created_time_nano); break;
              case 50: f_i64(q, t, &pt.expiring_time_nano); break;
              case 60: f_bool(q, t, &pt.flags, CDR_RP_RESETTABLE); break;
              default: skip1(q, t); break;
            }
          });
          pt.binary_checksum = H(cs);
          pt.run_id = H(ru);
          if (P == FILL) store_whole(C.rp + o0.v[1] + k, pt);
        }
      }
      // search attributes, in wire order; a repeated key keeps its first slot and its last value
      uint32_t n_keys = 0;
      {
        const uint64_t cap = umin64(n_sa, o1.v[2] - o0.v[2]);
        // (past the map's header: the thrift type bytes and count, or the CQL count; a thrift
        // binary and a CQL [bytes] element are both a big-endian length and the bytes)
        constexpr uint32_t HDR = CQL ? 4 : 6;
        Rd q = sub_reader(rd, R.sam.at + HDR, R.sam.n >= HDR ? R.sam.n - HDR : 0);
        cdr_kv* o = P == FILL ? C.sa + o0.v[2] : nullptr;
        for (uint64_t k = 0; k < cap && q.ok(); k++) {
          Span ks{0, 0}, vs{0, 0};
          f_str(q, T_STRING, &ks);
          f_str(q, T_STRING, &vs);
          const uint32_t hk = H(ks), hv = H(vs);
          if (P == FILL) {
            uint32_t j = 0;
            while (j < n_keys && o[j].key != hk) j++;
            o[j] = cdr_kv{hk, hv};
            n_keys += j == n_keys ? 1u : 0u;
          }
        }
      }
      if (P == COUNT) {
        need.v[0] = n_vh;
        need.v[1] = n_rp;
        need.v[2] = n_sa;
        need.v[3] = (need.v[3] + 3) & ~3ull;
      }
      if (P == FILL) {
        const uint64_t cap = umin64(n_vh, o1.v[0] - o0.v[0]);
        Rd q = sub_reader(rd, items.at + 5, items.n >= 5 ? items.n - 5 : 0);
        for (uint64_t k = 0; k < cap && q.ok(); k++) {
          cdr_vh_item it{0, 0};
          fields(q, [&](uint32_t t, uint32_t id) {
            if (id == 10) f_i64(q, t, &it.event_id);
            else if (id == 20) f_i64(q, t, &it.version);
            else skip1(q, t);
          });
          store_whole(C.vh + o0.v[0] + k, it);
        }
        x.branch_id_lo = tok.lo;
        x.branch_id_hi = tok.hi;
        x.attempt = (int32_t)(uint32_t)(uint64_t)R.f82;
        x.signal_count = (int32_t)(uint32_t)(uint64_t)R.f106;
        if (!(R.has & X_F18)) x.completion_event_batch_id = CDR_EMPTY_EVENT_ID;
        if constexpr (CQL) {  // the UDT's own (the Cassandra read assigns both)
          x.next_event_id = R.next_ev;
          x.last_event_task_id = R.letid;
        } else {
          x.next_event_id = C.in.next_event_id[w];
          x.last_event_task_id = 0;
        }
        x.flags |= CDR_XI_STARTED | ((R.has & X_TOKEN) ? CDR_XI_HAS_BRANCH : 0u) |
                   ((R.has & X_MEMO) ? CDR_XI_HAS_MEMO : 0u) | ((R.has & X_SA) ? CDR_XI_HAS_SEARCH_ATTR : 0u) |
                   (has_points ? CDR_XI_HAS_RESET_POINTS : 0u) | (vh_branch ? CDR_XI_VH_BRANCH : 0u);
        if (R.f94 != CDR_ZERO_TIME_NANOS) {
          x.flags |= CDR_XI_HAS_EXPIRATION;
          x.expiration_time = R.f94;
        }
        x.reset_points_len = (uint32_t)umin64(n_rp, o1.v[1] - o0.v[1]);
        x.search_attr_len = n_keys;
        ps.sticky_s2s_timeout = (int64_t)(int32_t)(uint32_t)(uint64_t)R.f80;
        store_whole(C.exec + w, x);  // two 128-B halves, each whole
        store_whole(C.repl + w, rs);
        store_whole(C.persist + w, ps);
        C.builder[w] = builder;
        C.n_sa[w] = n_keys;
      }
    }
    if (P == COUNT) C.cnt[w] = need;
  }
  if (P == COUNT) {
    for (int o = 32; o > 0; o >>= 1) n_str += __shfl_down(n_str, o, 64);
    if (lane == 0 && n_str) atomicAdd(C.totals, (unsigned long long)n_str);
  }
}

// the entry of each row: the last w with entry_row0[w] <= r (empty entries share a start)
__global__ void k_row_entry(const uint32_t* row0, uint32_t n_entries, uint32_t n_rows, uint32_t* row_entry) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  uint32_t lo = 0, hi = n_entries - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (row0[mid] <= r) lo = mid;
    else hi = mid - 1;
  }
  row_entry[r] = lo;
}

// the generated run-ID texts into the string table, after every string of the rows
__global__ void k_gen_intern(STab T, const uint8_t* gen, const uint32_t* row_entry, const unsigned long long* fail,
                             uint32_t n_rows) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows || fail[row_entry[r]] != NO_FAIL) return;
  const uint8_t* g = gen + (uint64_t)GEN_BYTES * r;
  if (g[0] == 0) return;
  tab_insert(T, cdr_str_hash(g, GEN_BYTES), ((uint64_t)GEN_BYTES * r) | GEN_REF, GEN_BYTES, UNASSIGNED);
}

// timer keys: the ID's hash (INTERN) -> its handle
__global__ void k_timer_keys(STab T, int64_t* tkey, uint32_t n_rows) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const uint64_t h = (uint64_t)tkey[r];
  tkey[r] = h ? (int64_t)tab_lookup(T, h) : 0;
}

// RANK: the row's slot among its entry's rows by key; equal keys fail the entry, and so does
// a table with more than CDR_LOAD_MAX_ENTRY_ROWS rows of the entry
__global__ void k_rank_rows(const int64_t* key, const uint32_t* row_entry, const uint32_t* row0, uint32_t n_rows,
                            uint32_t n_entries, unsigned long long* fail, int32_t* status, uint32_t* dest,
                            uint32_t table) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const uint32_t w = row_entry[r];
  if (fail[w] != NO_FAIL) return;
  const uint32_t lo = umin32(row0[w], n_rows), hi = umin32(row0[w + 1], n_rows);
  if (r < lo || r >= hi) return;
  if (hi - lo > CDR_LOAD_MAX_ENTRY_ROWS) {  // every lane walks its entry's rows: bounded (cdr.h)
    status[r] = CDR_LOAD_E_ENTRY_ROWS;
    if (r == lo) atomicMin(&fail[n_entries + w], fail_word(table, 0, CDR_LOAD_E_ENTRY_ROWS));
    return;
  }
  const int64_t k = key[r];
  uint32_t below = 0, same = 0;
  for (uint32_t j = lo; j < hi; j++) {
    const int64_t kj = key[j];
    below += kj < k ? 1u : 0u;
    same += kj == k ? 1u : 0u;
  }
  dest[r] = lo + below;
  if (same > 1) {
    status[r] = CDR_LOAD_E_DUP_KEY;
    atomicMin(&fail[n_entries + w], fail_word(table, r - lo, CDR_LOAD_E_DUP_KEY));
  }
}

struct EpiIn {
  const uint32_t* row0[CDR_LOAD_TABLES];
  uint32_t n_rows[CDR_LOAD_TABLES];
};
__global__ void k_epilogue(EpiIn E, uint32_t n_entries, const unsigned long long* fail, cdr_wf_result* result,
                           cdr_wf_caps* caps, int32_t* entry_status, uint32_t* n_bad, const XCnt* xoff,
                           const uint32_t* n_sa) {
  const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n_entries) return;
  unsigned long long f = fail[w];
  if (f == NO_FAIL) f = fail[n_entries + w];
  const bool ok = f == NO_FAIL;
  uint64_t off[CDR_LOAD_TABLES];
  uint32_t cnt[CDR_LOAD_TABLES];
#pragma unroll
  for (int t = 0; t < CDR_LOAD_TABLES; t++) {
    const uint32_t a = E.row0[t] ? umin32(E.row0[t][w], E.n_rows[t]) : 0u;
    const uint32_t b = E.row0[t] ? umin32(E.row0[t][w + 1], E.n_rows[t]) : 0u;
    off[t] = a;
    cnt[t] = b > a ? b - a : 0u;
  }
  cdr_wf_result res;
  {
    uint64_t* z = reinterpret_cast<uint64_t*>(&res);
#pragma unroll
    for (uint32_t i = 0; i < sizeof(res) / 8; i++) z[i] = 0;
  }
  res.code = ok ? CDR_OK : CDR_E_LOAD_ROWS;
  res.n_activity = ok ? cnt[0] : 0u;
  res.n_timer = ok ? cnt[1] : 0u;
  res.n_child = ok ? cnt[2] : 0u;
  res.n_cancel = ok ? cnt[3] : 0u;
  res.n_signal = ok ? cnt[4] : 0u;
  cdr_wf_caps c;
  {
    uint64_t* z = reinterpret_cast<uint64_t*>(&c);
#pragma unroll
    for (uint32_t i = 0; i < sizeof(c) / 8; i++) z[i] = 0;
  }
  c.act_off = off[0], c.timer_off = off[1], c.child_off = off[2], c.cancel_off = off[3], c.signal_off = off[4];
  c.act_cap = cnt[0], c.timer_cap = cnt[1], c.child_cap = cnt[2], c.cancel_cap = cnt[3], c.signal_cap = cnt[4];
  if (xoff) {  // the execution row's item tables (cdr_load_state)
    const XCnt a = xoff[w], b = xoff[w + 1];
    c.vh_off = a.v[0], c.rp_off = a.v[1], c.sa_off = a.v[2];
    c.vh_cap = (uint32_t)(b.v[0] - a.v[0]), c.rp_cap = (uint32_t)(b.v[1] - a.v[1]);
    c.sa_cap = (uint32_t)(b.v[2] - a.v[2]);
    res.n_vh = ok ? c.vh_cap : 0u;
    res.n_reset_points = ok ? c.rp_cap : 0u;
    res.n_search_attr = ok ? n_sa[w] : 0u;
  }
  result[w] = res;
  caps[w] = c;
  entry_status[w] = ok ? CDR_DEC_OK : (int32_t)(f & 0xFFu);
  if (!ok) atomicAdd(n_bad, 1u);
}

// ---------------------------------------------------------------- string table gather
__global__ void k_gather_len(const uint32_t* str_len, uint32_t n, uint64_t* lens) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  lens[i] = i < n ? str_len[i] : 0u;
}
// one wavefront per string
__global__ __launch_bounds__(256) void k_gather_copy(const uint64_t* str_ref, const uint32_t* str_len, uint32_t n,
                                                     const uint8_t* bytes, const uint8_t* seed_bytes,
                                                     const uint8_t* gen_bytes, const uint64_t* off, uint8_t* out) {
  const uint32_t h = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (h >= n) return;
  const uint64_t ref = str_ref[h];
  const uint8_t* src = (ref & SEED_REF) ? seed_bytes : (ref & GEN_REF) ? gen_bytes : bytes;
  if (!src) return;
  src += ref & ~(SEED_REF | GEN_REF);
  uint8_t* dst = out + off[h];
  const uint32_t len = str_len[h];
  for (uint32_t i = lane; i < len; i += 64) dst[i] = src[i];
}

// ---------------------------------------------------------------- the Cassandra maps' split
// One lane per (entry, table) walks its column: the count word, then pair after pair
// delimited by the two length words alone.  The first launch counts the pairs (the rows) and
// lowers the entry's failure word at a map-level finding; after one scan per table the second
// writes each row's offset — its key's length word — at the entry's rows, and the end of the
// table's last pair at [n_rows].
struct QCtx {
  const uint8_t* bytes;
  uint64_t total;
  const uint64_t* col_off[CDR_LOAD_TABLES];
  uint32_t n_entries;
  uint32_t* cnt;               // [5][n_entries + 1], the last of each zero
  const uint32_t* row0;        // their exclusive scans
  unsigned long long* fail;    // [n_entries]
  uint64_t* off[CDR_LOAD_TABLES];  // WRITE: [n_rows[t] + 1]
  uint32_t n_rows[CDR_LOAD_TABLES];
};
template <bool WRITE>
__global__ __launch_bounds__(256) void k_cql_split(QCtx Q) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)CDR_LOAD_TABLES * Q.n_entries) return;
  const uint32_t t = (uint32_t)(i / Q.n_entries), w = (uint32_t)(i % Q.n_entries);
  const uint64_t slot = (uint64_t)t * (Q.n_entries + 1ull) + w;
  const uint64_t* co = Q.col_off[0];
#pragma unroll
  for (uint32_t k = 1; k < CDR_LOAD_TABLES; k++) co = t == k ? Q.col_off[k] : co;
  const uint64_t e = umin64(co[w + 1], Q.total), p = umin64(co[w], e);
  uint32_t rows = 0, lo = 0, cap = 0;
  uint64_t* off = nullptr;
  if (WRITE) {  // every write capped by the entry's row range
    uint32_t nr = Q.n_rows[0];
    off = Q.off[0];
#pragma unroll
    for (uint32_t k = 1; k < CDR_LOAD_TABLES; k++) {
      nr = t == k ? Q.n_rows[k] : nr;
      off = t == k ? Q.off[k] : off;
    }
    lo = umin32(Q.row0[slot], nr);
    cap = umin32(Q.row0[slot + 1], nr) - lo;
    if (cap == 0) return;
  }
  int32_t finding = CDR_DEC_OK;
  Rd r;
  r.init(Q.bytes, p, e, Q.total);
  if (e != p) {  // (an empty range: a null column, an empty map)
    const int32_t n = (int32_t)r.be32();
    if (!r.ok()) finding = r.err;
    else if (n < 0) finding = CDR_DEC_BAD_SIZE;
    else if ((uint32_t)n > CDR_LOAD_MAX_ENTRY_ROWS) finding = CDR_LOAD_E_ENTRY_ROWS;
    const uint32_t want = finding ? 0u : WRITE ? umin32((uint32_t)n, cap) : (uint32_t)n;
    while (rows < want) {
      const uint64_t at = r.pos;
      cq_delimit(r);
      cq_delimit(r);
      if (!r.ok()) {
        finding = r.err;
        break;
      }
      if (WRITE) off[lo + rows] = at;
      rows++;
    }
  }
  if (WRITE) {
    uint32_t nr = Q.n_rows[0];
#pragma unroll
    for (uint32_t k = 1; k < CDR_LOAD_TABLES; k++) nr = t == k ? Q.n_rows[k] : nr;
    if (rows == cap && lo + cap == nr) off[nr] = r.pos;  // the table's last row ends here
  } else {
    Q.cnt[slot] = rows;
    if (finding != CDR_DEC_OK) atomicMin(&Q.fail[w], fail_word(t, rows, finding));
  }
}

template <class T>
int ws(cdr_ctx* c, int slot, uint64_t n, T** p) {
  *p = (T*)cdr_ws_get(c, slot, n * sizeof(T) + 8);
  return *p ? CDR_API_OK : CDR_API_ENOMEM;
}

template <int P, bool CQL>
void launch_rows_of(int t, const LCtx& C, hipStream_t st) {
  const dim3 grid((C.n_rows + CDR_LOAD_BLOCK - 1) / CDR_LOAD_BLOCK), blk(CDR_LOAD_BLOCK);
  const size_t lds = (CDR_LOAD_BLOCK / 64) * CDR_LOAD_STAGE;
  switch (t) {
    case 0: hipLaunchKernelGGL((k_rows<0, P, CQL>), grid, blk, lds, st, C); break;
    case 1: hipLaunchKernelGGL((k_rows<1, P, CQL>), grid, blk, lds, st, C); break;
    case 2: hipLaunchKernelGGL((k_rows<2, P, CQL>), grid, blk, lds, st, C); break;
    case 3: hipLaunchKernelGGL((k_rows<3, P, CQL>), grid, blk, lds, st, C); break;
    default: hipLaunchKernelGGL((k_rows<4, P, CQL>), grid, blk, lds, st, C); break;
  }
}
template <int P>
void launch_rows(int t, const LCtx& C, hipStream_t st, bool cql) {
  if (!C.n_rows) return;
  if (cql) launch_rows_of<P, true>(t, C, st);
  else launch_rows_of<P, false>(t, C, st);
}

template <int P>
void launch_exec(const XCtx& X, hipStream_t st, bool cql) {
  if (!X.n_entries) return;
  const dim3 grid((X.n_entries + CDR_LOAD_BLOCK - 1) / CDR_LOAD_BLOCK), blk(CDR_LOAD_BLOCK);
  const size_t lds = (CDR_LOAD_BLOCK / 64) * CDR_LOAD_STAGE;
  if (cql) hipLaunchKernelGGL((k_exec<P, true>), grid, blk, lds, st, X);
  else hipLaunchKernelGGL((k_exec<P, false>), grid, blk, lds, st, X);
}

// what the Cassandra front end hands the passes besides a cdr_rows_in of generated offsets
struct CqlX {
  const unsigned long long* fail;  // [n_entries]: the split's map-level findings
  int64_t* key;                    // [all rows]: in->key[t] point into it; the count pass writes
  uint64_t *gneed, *goff;          // [n_rows[0] + 1]
  const cdr_cql_exec_in* xq;       // cdr_load_cql_state: the execution row's columns (xin holds execution_off)
};

// cdr_load_rows (xin == NULL) and cdr_load_state; cx != NULL: the passes of cdr_load_cql_rows
int load_impl(cdr_ctx* ctx, const cdr_rows_in* in, const cdr_exec_rows_in* xin, cdr_rows_out* out,
              cdr_state_out* xout, void* stream, const CqlX* cx = nullptr) {
  if (!ctx || !in || !out || !in->seed_off || in->n_seeds == 0) return CDR_API_EINVAL;
  if (xin && !cx && in->n_entries &&
      (!xin->blob_off || !xin->domain_id || !xin->run_id || !xin->workflow_id_off || !xin->next_event_id ||
       !xin->last_write_version || xin->n_clusters > CDR_MAX_CLUSTERS || (in->n_bytes && !in->bytes)))
    return CDR_API_EINVAL;
  constexpr int NT = CDR_LOAD_TABLES;
  uint64_t n_all = 0, base[NT + 1];
  for (int t = 0; t < NT; t++) {
    base[t] = n_all;
    n_all += in->n_rows[t];
    if (!in->n_rows[t]) continue;
    if (!in->blob_off[t] || !in->entry_row0[t] || (t != 1 && !in->key[t])) return CDR_API_EINVAL;
  }
  base[NT] = n_all;
  if (!cx && ((in->n_rows[1] && !in->timer_id_off) || (in->n_rows[0] && !in->act_heartbeat))) return CDR_API_EINVAL;
  if (n_all && (!in->n_entries || (in->n_bytes && !in->bytes))) return CDR_API_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipSetDevice(cdr_ctx_device(ctx)));
  const uint32_t ne = in->n_entries;
  *out = cdr_rows_out{};
  // every row belongs to an entry: entry_row0 runs from 0 to n_rows (the split's own do)
  if (!cx) {
    uint32_t ends[NT][2] = {};
    for (int t = 0; t < NT; t++) {
      if (!in->n_rows[t]) continue;
      HIPCHK(hipMemcpyAsync(&ends[t][0], in->entry_row0[t], 4, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(&ends[t][1], in->entry_row0[t] + ne, 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    for (int t = 0; t < NT; t++)
      if (in->n_rows[t] && (ends[t][0] != 0 || ends[t][1] != in->n_rows[t])) return CDR_API_EINVAL;
  }
  for (hipEvent_t& e : ctx->ld_ev)
    if (!e) HIPCHK(hipEventCreate(&e));
  if (!cx) HIPCHK(hipEventRecord(ctx->ld_ev[0], st));  // (the split is part of the first pass)
  int rc;
  uint32_t *row_entry, *dest, *misc;
  int32_t *status, *estatus;
  int64_t* tkey;
  unsigned long long* fail;
  cdr_wf_result* result;
  cdr_wf_caps* caps;
  uint8_t* gen;
  void* recs[NT];
  static const int rec_slot[NT] = {WS_LD_ACT, WS_LD_TIMER, WS_LD_CHILD, WS_LD_CANCEL, WS_LD_SIGNAL};
  static const uint64_t rec_size[NT] = {sizeof(cdr_activity_info), sizeof(cdr_timer_info), sizeof(cdr_child_info),
                                        sizeof(cdr_cancel_info), sizeof(cdr_signal_info)};
  if ((rc = ws(ctx, WS_LD_ROWENT, n_all + 1, &row_entry)) || (rc = ws(ctx, WS_LD_STATUS, n_all + 1, &status)) ||
      (rc = ws(ctx, WS_LD_DEST, n_all + 1, &dest)) || (rc = ws(ctx, WS_LD_TKEY, in->n_rows[1] + 1ull, &tkey)) ||
      (rc = ws(ctx, WS_LD_FAIL, 2ull * ne + 1, &fail)) || (rc = ws(ctx, WS_LD_ESTATUS, ne + 1ull, &estatus)) ||
      (rc = ws(ctx, WS_LD_RESULT, ne + 1ull, &result)) || (rc = ws(ctx, WS_LD_CAPS, ne + 1ull, &caps)) ||
      (rc = ws(ctx, WS_LD_MISC, 16, &misc)))
    return rc;
  XCtx X{};
  XCnt* xoff = nullptr;
  uint32_t* n_sa = nullptr;
  const bool with_exec = xin && ne;
  if (with_exec) {
    X.bytes = in->bytes;
    X.total = in->n_bytes;
    X.in = *xin;
    if (cx) {
      X.rs_off = cx->xq->replication_state_off;
      X.vhb_off = cx->xq->version_histories_off;
      X.vhe_off = cx->xq->vh_encoding_off;
    }
    X.seed_bytes = in->seed_bytes;
    X.seed_off = in->seed_off;
    X.n_seeds = in->n_seeds;
    X.n_entries = ne;
    if ((rc = ws(ctx, WS_LD_XSTATUS, ne + 1ull, &X.status)) || (rc = ws(ctx, WS_LD_XCNT, ne + 1ull, &X.cnt)) ||
        (rc = ws(ctx, WS_LD_XOFF, ne + 1ull, &xoff)) || (rc = ws(ctx, WS_LD_EXEC, ne + 1ull, &X.exec)) ||
        (rc = ws(ctx, WS_LD_REPL, ne + 1ull, &X.repl)) || (rc = ws(ctx, WS_LD_PERSIST, ne + 1ull, &X.persist)) ||
        (rc = ws(ctx, WS_LD_BUILDER, ne + 1ull, &X.builder)) || (rc = ws(ctx, WS_LD_NSA, ne + 1ull, &n_sa)))
      return rc;
    X.off = xoff;
    X.n_sa = n_sa;
    X.fail = fail;
    HIPCHK(hipMemsetAsync(X.cnt + ne, 0, sizeof(XCnt), st));
  }
  for (int t = 0; t < NT; t++) {
    recs[t] = cdr_ws_get(ctx, rec_slot[t], (in->n_rows[t] + 1ull) * rec_size[t]);
    if (!recs[t]) return CDR_API_ENOMEM;
  }
  const dim3 blk(256);
  auto grid = [](uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); };
  // misc, as u32 words: [0] table overflow, [1] new strings, [2] failed entries, [3] unused,
  // [4..5] one u64: string fields
  unsigned long long* n_fields = reinterpret_cast<unsigned long long*>(misc) + 2;
  HIPCHK(hipMemsetAsync(misc, 0, 64, st));
  HIPCHK(hipMemsetAsync(fail, 0xFF, (2ull * ne + 1) * 8, st));
  if (cx && ne) HIPCHK(hipMemcpyAsync(fail, cx->fail, 8ull * ne, hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemsetAsync(dest, 0xFF, (n_all + 1) * 4, st));
  LCtx C[NT];
  for (int t = 0; t < NT; t++) {
    LCtx& c = C[t];
    c = LCtx{};
    c.bytes = in->bytes;
    c.total = in->n_bytes;
    c.blob_off = in->blob_off[t];
    c.tid_off = in->timer_id_off;
    c.key = in->key[t];
    c.hb = in->act_heartbeat;
    c.row_entry = row_entry + base[t];
    c.row0 = in->entry_row0[t];
    c.fail = fail;
    c.status = status + base[t];
    c.totals = n_fields;
    c.dest = dest + base[t];
    c.recs = recs[t];
    c.tkey = tkey;
    c.n_rows = in->n_rows[t];
    c.n_entries = ne;
    if (cx) {
      c.key_out = cx->key + base[t];
      c.gneed = cx->gneed;
      c.goff = cx->goff;
    }
    if (c.n_rows)
      hipLaunchKernelGGL(k_row_entry, grid(c.n_rows), blk, 0, st, c.row0, ne, c.n_rows, row_entry + base[t]);
  }
  HIPCHK(hipGetLastError());
  // ---- pass 1: statuses and string-field counts
  const bool cql = cx != nullptr;
  for (int t = 0; t < NT; t++) launch_rows<COUNT>(t, C[t], st, cql);
  XCnt xtot{{0, 0, 0, 0}};
  uint64_t act_gen = 0;  // the Cassandra form's activity list bodies: after the execution rows' shares
  if (cx && in->n_rows[0]) {  // the activity rows' list bodies in gen_bytes, scanned into offsets
    const int n = (int)(in->n_rows[0] + 1);
    HIPCHK(hipMemsetAsync(cx->gneed + in->n_rows[0], 0, 8, st));
    size_t tb = 0;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cx->gneed, cx->goff, n, st));
    void* tmp = cdr_ws_get(ctx, WS_LD_CQ_GTMP, tb ? tb : 8);
    if (!tmp) return CDR_API_ENOMEM;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, cx->gneed, cx->goff, n, st));
    HIPCHK(hipMemcpyAsync(&act_gen, cx->goff + in->n_rows[0], 8, hipMemcpyDeviceToHost, st));
  }
  if (with_exec) {  // ... and the execution rows' item counts and gen_bytes need, scanned into offsets
    X.totals = n_fields;
    launch_exec<COUNT>(X, st, cql);
    size_t tb = 0;
    HIPCHK(hipcub::DeviceScan::ExclusiveScan(nullptr, tb, X.cnt, xoff, XCntAdd(), XCnt{{0, 0, 0, 0}}, (int)(ne + 1), st));
    void* tmp = cdr_ws_get(ctx, WS_LD_XTMP, tb ? tb : 8);
    if (!tmp) return CDR_API_ENOMEM;
    HIPCHK(hipcub::DeviceScan::ExclusiveScan(tmp, tb, X.cnt, xoff, XCntAdd(), XCnt{{0, 0, 0, 0}}, (int)(ne + 1), st));
    HIPCHK(hipMemcpyAsync(&xtot, xoff + ne, sizeof(XCnt), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->ld_ev[1], st));
  uint64_t n_str_fields = 0;
  HIPCHK(hipMemcpyAsync(&n_str_fields, n_fields, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const uint64_t gen_rows = (uint64_t)GEN_BYTES * in->n_rows[2];  // the child rows' part of gen_bytes
  if ((rc = ws(ctx, WS_LD_GEN, gen_rows + xtot.v[3] + act_gen + 8, &gen))) return rc;
  for (int t = 0; t < NT; t++) {
    C[t].gen = gen;
    C[t].gen_base = gen_rows + xtot.v[3];
  }
  if (with_exec) {
    X.gen = gen + gen_rows;
    X.gen_base = gen_rows;
    if ((rc = ws(ctx, WS_LD_VH, xtot.v[0] + 1, &X.vh)) || (rc = ws(ctx, WS_LD_RP, xtot.v[1] + 1, &X.rp)) ||
        (rc = ws(ctx, WS_LD_SA, xtot.v[2] + 1, &X.sa)))
      return rc;
  }
  uint64_t cap = 1024;
  while (cap < 2 * (n_str_fields + in->n_seeds)) cap <<= 1;
  STab T{};
  T.mask = cap - 1;
  if ((rc = ws(ctx, WS_LD_TABKEY, cap, (unsigned long long**)&T.key)) || (rc = ws(ctx, WS_LD_TABVAL, cap, &T.val)) ||
      (rc = ws(ctx, WS_LD_TABREF, cap, &T.ref)) || (rc = ws(ctx, WS_LD_TABLEN, cap, &T.len)))
    return rc;
  T.overflow = misc;
  HIPCHK(hipMemsetAsync(T.key, 0, cap * 8, st));
  // ---- pass 2: seeds, the rows' strings, the generated run IDs; rank the new ones by hash
  hipLaunchKernelGGL(k_seed, grid(in->n_seeds), blk, 0, st, T, in->seed_bytes, in->seed_off, in->n_seeds);
  for (int t = 0; t < NT; t++) {
    C[t].T = T;
    launch_rows<INTERN>(t, C[t], st, cql);
  }
  if (with_exec) {
    X.T = T;
    launch_exec<INTERN>(X, st, cql);
  }
  if (in->n_rows[2])
    hipLaunchKernelGGL(k_gen_intern, grid(in->n_rows[2]), blk, 0, st, T, gen, row_entry + base[2], fail,
                       in->n_rows[2]);
  HIPCHK(hipGetLastError());
  unsigned long long *k1, *k2;
  uint64_t *i1, *i2;
  uint32_t *ccount, *coffs;
  if ((rc = ws(ctx, WS_LD_SKEY, n_str_fields + 1, &k1)) || (rc = ws(ctx, WS_LD_SKEY2, n_str_fields + 1, &k2)) ||
      (rc = ws(ctx, WS_LD_SIDX, n_str_fields + 1, &i1)) || (rc = ws(ctx, WS_LD_SIDX2, n_str_fields + 1, &i2)) ||
      (rc = ws(ctx, WS_LD_STRREF, n_str_fields + in->n_seeds + 1, &out->str_ref)) ||
      (rc = ws(ctx, WS_LD_STRLEN, n_str_fields + in->n_seeds + 1, &out->str_len)) ||
      (rc = ws(ctx, WS_LD_CCOUNT, COLLECT_WG + 1ull, &ccount)) || (rc = ws(ctx, WS_LD_COFFS, COLLECT_WG + 1ull, &coffs)))
    return rc;
  {
    HIPCHK(hipMemsetAsync(ccount + COLLECT_WG, 0, 4, st));
    hipLaunchKernelGGL(k_collect_count, dim3(COLLECT_WG), blk, 0, st, T, ccount);
    size_t tb = 0;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, ccount, coffs, (int)(COLLECT_WG + 1), st));
    void* tmp = cdr_ws_get(ctx, WS_LD_CTMP, tb ? tb : 8);
    if (!tmp) return CDR_API_ENOMEM;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, ccount, coffs, (int)(COLLECT_WG + 1), st));
    hipLaunchKernelGGL(k_collect_write, dim3(COLLECT_WG), blk, 0, st, T, coffs, k1, i1);
    HIPCHK(hipMemcpyAsync(misc + 1, coffs + COLLECT_WG, 4, hipMemcpyDeviceToDevice, st));
  }
  HIPCHK(hipGetLastError());
  uint32_t hm[2];
  HIPCHK(hipMemcpyAsync(hm, misc, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (hm[0]) return CDR_API_ENOMEM;  // table overflow: cannot happen at twice the fields
  const uint32_t n_new = hm[1];
  if (n_new) {
    hipcub::DoubleBuffer<unsigned long long> kb(k1, k2);
    hipcub::DoubleBuffer<uint64_t> vb(i1, i2);
    size_t tmp_bytes = 0;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, kb, vb, (int)n_new, 0, 64, st));
    void* sort_tmp = cdr_ws_get(ctx, WS_LD_SORTTMP, tmp_bytes ? tmp_bytes : 8);
    if (!sort_tmp) return CDR_API_ENOMEM;
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(sort_tmp, tmp_bytes, kb, vb, (int)n_new, 0, 64, st));
    hipLaunchKernelGGL(k_rank, grid(n_new), blk, 0, st, T, vb.Current(), n_new, in->n_seeds, out->str_ref,
                       out->str_len);
  }
  hipLaunchKernelGGL(k_seed_refs, grid(in->n_seeds), blk, 0, st, in->seed_off, in->n_seeds, out->str_ref,
                     out->str_len);
  HIPCHK(hipGetLastError());
  out->n_strings = in->n_seeds + n_new;
  HIPCHK(hipEventRecord(ctx->ld_ev[2], st));
  // ---- pass 3: each row's slot in key order (timer keys: the handles, known now)
  if (in->n_rows[1]) hipLaunchKernelGGL(k_timer_keys, grid(in->n_rows[1]), blk, 0, st, T, tkey, in->n_rows[1]);
  for (int t = 0; t < NT; t++)
    if (in->n_rows[t])
      hipLaunchKernelGGL(k_rank_rows, grid(in->n_rows[t]), blk, 0, st, t == 1 ? (const int64_t*)tkey : in->key[t],
                         row_entry + base[t], in->entry_row0[t], in->n_rows[t], ne, fail, status + base[t],
                         dest + base[t], (uint32_t)t);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->ld_ev[3], st));
  // ---- pass 4: the records, then the entries
  for (int t = 0; t < NT; t++) launch_rows<FILL>(t, C[t], st, cql);
  EpiIn E{};
  for (int t = 0; t < NT; t++) {
    E.row0[t] = in->entry_row0[t];
    E.n_rows[t] = in->n_rows[t];
  }
  if (with_exec) launch_exec<FILL>(X, st, cql);
  if (ne)
    hipLaunchKernelGGL(k_epilogue, grid(ne), blk, 0, st, E, ne, fail, result, caps, estatus, misc + 2,
                       (const XCnt*)(with_exec ? xoff : nullptr), (const uint32_t*)n_sa);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ctx->ld_ev[4], st));
  uint32_t n_bad = 0;
  HIPCHK(hipMemcpyAsync(&n_bad, misc + 2, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int i = 0; i < 4; i++) HIPCHK(hipEventElapsedTime(&ctx->ld_ms[i], ctx->ld_ev[i], ctx->ld_ev[i + 1]));
  out->state.result = result;
  out->state.act = (cdr_activity_info*)recs[0];
  out->state.timer = (cdr_timer_info*)recs[1];
  out->state.child = (cdr_child_info*)recs[2];
  out->state.cancel = (cdr_cancel_info*)recs[3];
  out->state.signal = (cdr_signal_info*)recs[4];
  out->caps = caps;
  out->totals.act = in->n_rows[0];
  out->totals.timer = in->n_rows[1];
  out->totals.child = in->n_rows[2];
  out->totals.cancel = in->n_rows[3];
  out->totals.signal = in->n_rows[4];
  for (int t = 0; t < NT; t++) out->row_status[t] = status + base[t];
  out->entry_status = estatus;
  out->gen_bytes = gen;
  out->n_gen_bytes = gen_rows + xtot.v[3] + act_gen;
  out->n_bad_entries = n_bad;
  if (with_exec) {
    out->state.exec = X.exec;
    out->state.repl = X.repl;
    out->state.vh = X.vh;
    out->state.rp = X.rp;
    out->state.sa = X.sa;
    out->totals.vh = xtot.v[0];
    out->totals.rp = xtot.v[1];
    out->totals.sa = xtot.v[2];
    xout->persist = X.persist;
    xout->builder = X.builder;
    xout->exec_status = X.status;
  }
  return CDR_API_OK;
}

}  // namespace

extern "C" int cdr_load_rows(cdr_ctx* ctx, const cdr_rows_in* in, cdr_rows_out* out, void* stream) {
  return load_impl(ctx, in, nullptr, out, nullptr, stream);
}

extern "C" int cdr_load_state(cdr_ctx* ctx, const cdr_rows_in* rows, const cdr_exec_rows_in* exec,
                              cdr_state_out* out, void* stream) {
  if (!out) return CDR_API_EINVAL;
  *out = cdr_state_out{};
  return load_impl(ctx, rows, exec, &out->rows, out, stream);
}

namespace {
// cdr_load_cql_rows (xq == NULL) and cdr_load_cql_state
int load_cql_impl(cdr_ctx* ctx, const cdr_cql_rows_in* in, const cdr_cql_exec_in* xq, cdr_cql_rows_out* out,
                  cdr_state_out* xout, void* stream) {
  if (!ctx || !in || !out || !in->seed_off || in->n_seeds == 0) return CDR_API_EINVAL;
  if (xq && in->n_entries &&
      (!xq->execution_off || !xq->replication_state_off || !xq->version_histories_off || !xq->vh_encoding_off ||
       xq->n_clusters > CDR_MAX_CLUSTERS))
    return CDR_API_EINVAL;
  constexpr int NT = CDR_LOAD_TABLES;
  const uint32_t ne = in->n_entries;
  if ((in->n_bytes && !in->bytes) || in->n_bytes >= (1ull << 35)) return CDR_API_EINVAL;
  for (int t = 0; t < NT; t++)
    if (ne && !in->col_off[t]) return CDR_API_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipSetDevice(cdr_ctx_device(ctx)));
  *out = cdr_cql_rows_out{};
  for (hipEvent_t& e : ctx->ld_ev)
    if (!e) HIPCHK(hipEventCreate(&e));
  HIPCHK(hipEventRecord(ctx->ld_ev[0], st));
  int rc;
  QCtx Q{};
  uint32_t *cnt, *row0;
  const uint64_t per = ne + 1ull;
  if ((rc = ws(ctx, WS_LD_CQ_CNT, NT * per, &cnt)) || (rc = ws(ctx, WS_LD_CQ_ROW0, NT * per, &row0)) ||
      (rc = ws(ctx, WS_LD_CQ_FAIL, per, &Q.fail)))
    return rc;
  Q.bytes = in->bytes;
  Q.total = in->n_bytes;
  for (int t = 0; t < NT; t++) Q.col_off[t] = in->col_off[t];
  Q.n_entries = ne;
  Q.cnt = cnt;
  Q.row0 = row0;
  uint32_t n_rows[NT] = {};
  const dim3 blk(256), grid((uint32_t)((NT * (uint64_t)ne + 255) / 256));
  if (ne) {
    HIPCHK(hipMemsetAsync(cnt, 0, NT * per * 4, st));
    HIPCHK(hipMemsetAsync(Q.fail, 0xFF, per * 8, st));
    hipLaunchKernelGGL(k_cql_split<false>, grid, blk, 0, st, Q);
    HIPCHK(hipGetLastError());
    size_t tb = 0;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, cnt, row0, (int)per, st));
    void* tmp = cdr_ws_get(ctx, WS_LD_XTMP, tb ? tb : 8);
    if (!tmp) return CDR_API_ENOMEM;
    for (int t = 0; t < NT; t++) {
      HIPCHK(hipcub::DeviceScan::ExclusiveSum(tmp, tb, cnt + t * per, row0 + t * per, (int)per, st));
      HIPCHK(hipMemcpyAsync(&n_rows[t], row0 + t * per + ne, 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));  // the one readback the split adds: the five row totals
  }
  uint64_t n_all = 0, base[NT];
  for (int t = 0; t < NT; t++) {
    base[t] = n_all;
    n_all += n_rows[t];
  }
  uint64_t* off;
  CqlX cx{};
  cx.fail = Q.fail;
  if ((rc = ws(ctx, WS_LD_CQ_OFF, n_all + NT, &off)) || (rc = ws(ctx, WS_LD_CQ_KEY, n_all + 1, &cx.key)) ||
      (rc = ws(ctx, WS_LD_CQ_GNEED, n_rows[0] + 1ull, &cx.gneed)) ||
      (rc = ws(ctx, WS_LD_CQ_GOFF, n_rows[0] + 1ull, &cx.goff)))
    return rc;
  cdr_rows_in R{};
  R.bytes = in->bytes;
  R.n_bytes = in->n_bytes;
  R.seed_bytes = in->seed_bytes;
  R.seed_off = in->seed_off;
  R.n_entries = ne;
  R.n_seeds = in->n_seeds;
  for (int t = 0; t < NT; t++) {
    Q.off[t] = off + base[t] + t;
    Q.n_rows[t] = n_rows[t];
    R.blob_off[t] = Q.off[t];
    R.entry_row0[t] = row0 + t * per;
    R.key[t] = cx.key + base[t];
    R.n_rows[t] = n_rows[t];
  }
  if (n_all) {
    hipLaunchKernelGGL(k_cql_split<true>, grid, blk, 0, st, Q);
    HIPCHK(hipGetLastError());
  }
  cdr_exec_rows_in xin{};
  if (xq) {  // the execution column is the rows' blob; the other columns go by cx.xq
    xin.blob_off = xq->execution_off;
    for (uint32_t i = 0; i < CDR_MAX_CLUSTERS; i++) xin.cluster_seed[i] = xq->cluster_seed[i];
    xin.n_clusters = xq->n_clusters;
    cx.xq = xq;
  }
  if ((rc = load_impl(ctx, &R, xq ? &xin : nullptr, &out->rows, xout, stream, &cx))) return rc;
  for (int t = 0; t < NT; t++) {
    out->n_rows[t] = n_rows[t];
    out->entry_row0[t] = row0 + t * per;
  }
  return CDR_API_OK;
}
}  // namespace

extern "C" int cdr_load_cql_rows(cdr_ctx* ctx, const cdr_cql_rows_in* in, cdr_cql_rows_out* out, void* stream) {
  return load_cql_impl(ctx, in, nullptr, out, nullptr, stream);
}

extern "C" int cdr_load_cql_state(cdr_ctx* ctx, const cdr_cql_rows_in* rows, const cdr_cql_exec_in* exec,
                                  cdr_cql_state_out* out, void* stream) {
  if (!out) return CDR_API_EINVAL;
  cdr_state_out x{};
  const int rc = load_cql_impl(ctx, rows, exec, &out->rows, &x, stream);
  out->persist = x.persist;
  out->builder = x.builder;
  out->exec_status = x.exec_status;
  return rc;
}

extern "C" int cdr_load_pass_ms(cdr_ctx* ctx, float* ms) {
  if (!ctx || !ms) return CDR_API_EINVAL;
  for (int i = 0; i < 4; i++) ms[i] = ctx->ld_ms[i];
  return CDR_API_OK;
}

extern "C" int cdr_strtab_gather_async(cdr_ctx* ctx, const uint64_t* str_ref, const uint32_t* str_len, uint32_t n,
                                       const uint8_t* bytes, const uint8_t* seed_bytes, const uint8_t* gen_bytes,
                                       uint64_t* off, uint8_t* out_bytes, void* stream) {
  if (!ctx || !off || (n && (!str_ref || !str_len))) return CDR_API_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipSetDevice(cdr_ctx_device(ctx)));
  if (!out_bytes) {  // sizes: off[0 .. n] = exclusive scan of the lengths
    size_t tb = 0;
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (uint64_t*)nullptr, off, (int)(n + 1), st));
    const uint64_t lens_bytes = ((n + 1ull) * 8 + 255) & ~255ull;
    uint8_t* tmp = (uint8_t*)cdr_ws_get(ctx, WS_GATHER_TMP, lens_bytes + (tb ? tb : 8));
    if (!tmp) return CDR_API_ENOMEM;
    uint64_t* lens = (uint64_t*)tmp;
    hipLaunchKernelGGL(k_gather_len, dim3((n + 256) / 256), dim3(256), 0, st, str_len, n, lens);
    HIPCHK(hipGetLastError());
    HIPCHK(hipcub::DeviceScan::ExclusiveSum(tmp + lens_bytes, tb, lens, off, (int)(n + 1), st));
    return CDR_API_OK;
  }
  if (n)
    hipLaunchKernelGGL(k_gather_copy, dim3((n + 3) / 4), dim3(256), 0, st, str_ref, str_len, n, bytes, seed_bytes,
                       gen_bytes, off, out_bytes);
  HIPCHK(hipGetLastError());
  return CDR_API_OK;
}
