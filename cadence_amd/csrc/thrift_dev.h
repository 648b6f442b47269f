// thrift_dev.h — device code shared by the thriftrw decoders (ingest.hip: history blobs;
// load.hip: persisted pending-table rows): the open-addressing string table with its
// seed / collect / rank kernels, and the byte reader with the value skipper and the
// per-wavefront LDS staging.  Everything has internal linkage: each translation unit
// gets its own copy of the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cdr/cdr.h"
#include "cdr/ingest.h"

namespace {

enum : uint32_t {
  T_STOP = 0, T_BOOL = 2, T_BYTE = 3, T_DOUBLE = 4, T_I16 = 6, T_I32 = 8, T_I64 = 10, T_STRING = 11,
  T_STRUCT = 12, T_MAP = 13, T_SET = 14, T_LIST = 15
};
constexpr uint32_t UNASSIGNED = 0xFFFFFFFFu;
constexpr uint64_t SEED_REF = 1ull << 63;

// ---------------------------------------------------------------- string table
struct STab {
  unsigned long long* key;  // 0 = empty slot
  uint32_t* val;            // handle (UNASSIGNED until ranked)
  uint64_t* ref;            // blob-byte offset of the first occurrence (| SEED_REF: seed byte offset)
  uint32_t* len;
  uint64_t mask;
  uint32_t* overflow;
};
__device__ __forceinline__ uint64_t slot0(uint64_t h, uint64_t mask) { return cdr_mix64(h) & mask; }

__device__ void tab_insert(const STab& T, uint64_t h, uint64_t ref, uint32_t len, uint32_t handle) {
  uint64_t i = slot0(h, T.mask);
  for (uint64_t probe = 0; probe <= T.mask; probe++, i = (i + 1) & T.mask) {
    // most string fields repeat a string already in the table (task lists, types, ids):
    // a plain load finds those without an atomic on a slot every lane of the chip hits
    const unsigned long long seen = __hip_atomic_load(&T.key[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (seen == (unsigned long long)h) return;
    if (seen != 0ull) continue;
    const unsigned long long k = atomicCAS(&T.key[i], 0ull, (unsigned long long)h);
    if (k == 0ull) {  // this lane owns the slot
      T.ref[i] = ref;
      T.len[i] = len;
      T.val[i] = handle;
      return;
    }
    if (k == h) return;
  }
  atomicOr(T.overflow, 1u);  // sized at twice the string fields: never taken
}

__device__ uint32_t tab_lookup(const STab& T, uint64_t h) {
  uint64_t i = slot0(h, T.mask);
  for (uint64_t probe = 0; probe <= T.mask; probe++, i = (i + 1) & T.mask) {
    const uint64_t k = T.key[i];
    if (k == h) return T.val[i];
    if (k == 0) break;
  }
  return 0;  // not interned (cannot happen after pass 2)
}

// ---------------------------------------------------------------- reader
// Each wavefront first copies its 64 consecutive blobs — one contiguous byte range — into
// LDS with 16-byte loads (64 lanes x 16 B per instruction, coalesced), so the parse reads
// bytes from LDS; a wave whose range exceeds its share of LDS (stage_blobs' `cap`: the ingest
// passes CDR_INGEST_STAGE, the row loader its own, larger share) reads
// through a 16-byte aligned window held in registers (one global_load_dwordx4 per 16
// bytes instead of a load per byte), as does any byte outside the staged range; the last
// 16 bytes of the buffer, which an aligned window could overrun, are read byte by byte.
#ifndef CDR_INGEST_STAGE
#define CDR_INGEST_STAGE 12288 /* bytes of blob data staged in LDS per wavefront */
#endif
#define LDS3 __attribute__((address_space(3)))
struct Rd {
  const uint8_t* b;  // blob_bytes
  uint64_t pos, end;
  uint64_t total;    // bytes in blob_bytes
  uint64_t wb;       // window address (16-aligned), ~0 = empty
  uint64_t w0, w1;
  const LDS3 uint8_t* sb;  // the wave's staged bytes: addresses [s_lo, s_lo + s_n)
  uint64_t s_lo, s_n;
  int32_t err;
  __device__ __forceinline__ void init(const uint8_t* base, uint64_t p, uint64_t e, uint64_t t) {
    b = base;
    pos = p;
    end = e;
    total = t;
    wb = ~0ull;
    sb = nullptr;
    s_lo = s_n = 0;
    err = CDR_DEC_OK;
  }
  __device__ __forceinline__ uint32_t at(uint64_t p) {
    // the window is aligned in the address space (the buffer itself need not be)
    const uint64_t addr = (uint64_t)(uintptr_t)(b + p), a = addr & ~15ull;
    if (addr - s_lo < s_n) return sb[addr - s_lo];
    if (a != wb) {
      const uint64_t lo = (uint64_t)(uintptr_t)b;
      if (a < lo || a + 16 > lo + total) return b[p];
      const uint4 v = *reinterpret_cast<const uint4*>((uintptr_t)a);
      w0 = (uint64_t)v.x | ((uint64_t)v.y << 32);
      w1 = (uint64_t)v.z | ((uint64_t)v.w << 32);
      wb = a;
    }
    const uint32_t o = (uint32_t)(addr - a);
    return (uint32_t)(((o < 8) ? (w0 >> (8 * o)) : (w1 >> (8 * (o - 8)))) & 0xFFu);
  }
  __device__ __forceinline__ bool ok() const { return err == CDR_DEC_OK; }
  __device__ __forceinline__ bool need(uint64_t n) {
    if (err) return false;
    if (end - pos < n) {
      err = CDR_DEC_TRUNCATED;
      pos = end;
      return false;
    }
    return true;
  }
  __device__ __forceinline__ uint32_t u8() {
    if (!need(1)) return 0;
    return at(pos++);
  }
  __device__ __forceinline__ uint32_t be16() {
    if (!need(2)) return 0;
    const uint32_t v = (at(pos) << 8) | at(pos + 1);
    pos += 2;
    return v;
  }
  __device__ __forceinline__ uint32_t be32() {
    if (!need(4)) return 0;
    const uint32_t v = (at(pos) << 24) | (at(pos + 1) << 16) | (at(pos + 2) << 8) | at(pos + 3);
    pos += 4;
    return v;
  }
  __device__ __forceinline__ uint64_t be64() {
    const uint64_t hi = be32();
    return (hi << 32) | be32();
  }
  __device__ __forceinline__ int32_t size() {  // a length / count: negative is a decode error
    const int32_t n = (int32_t)be32();
    if (n < 0 && !err) err = CDR_DEC_BAD_SIZE;
    return n < 0 ? 0 : n;
  }
  // cdr_str_hash of bytes [p, p + n), through the window
  __device__ uint64_t hash(uint64_t p, uint64_t n) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (uint64_t i = 0; i < n; i++) h = (h ^ at(p + i)) * 0x100000001B3ull;
    h = cdr_mix64(h ^ (n * 0x9E3779B97F4A7C15ull));
    return h ? h : 1u;
  }
};

__device__ __forceinline__ uint32_t fixed_size(uint32_t t) {
  switch (t) {
    case T_BOOL: case T_BYTE: return 1;
    case T_I16: return 2;
    case T_I32: return 4;
    case T_I64: case T_DOUBLE: return 8;
    default: return 0;
  }
}

// skip one value of wire type t (iterative: an explicit stack of open containers)
__device__ __forceinline__ void skip_body(Rd& r, uint32_t t) {
  struct Fr {
    uint32_t kind, t1, t2;
    uint32_t n;  // remaining elements (maps: 2 per pair)
  };
  Fr st[CDR_THRIFT_MAX_DEPTH];
  int d = 0;
  uint32_t cur = t;
  for (;;) {
    if (!r.ok()) return;
    // ---- one value of type cur
    if (const uint32_t fs = fixed_size(cur)) {
      if (r.need(fs)) r.pos += fs;
    } else if (cur == T_STRING) {
      const uint32_t n = (uint32_t)r.size();
      if (r.need(n)) r.pos += n;
    } else if (cur == T_STRUCT || cur == T_LIST || cur == T_SET || cur == T_MAP) {
      if (d == CDR_THRIFT_MAX_DEPTH) {
        r.err = CDR_DEC_DEPTH;
        return;
      }
      Fr f{cur, 0, 0, 0};
      if (cur == T_LIST || cur == T_SET) {
        f.t1 = r.u8();
        f.n = (uint32_t)r.size();
      } else if (cur == T_MAP) {
        f.t1 = r.u8();
        f.t2 = r.u8();
        f.n = 2u * (uint32_t)r.size();
      }
      st[d++] = f;
    } else {
      r.err = CDR_DEC_BAD_TYPE;
      return;
    }
    // ---- the next value, from the innermost open container
    bool have = false;
    while (d > 0 && !have && r.ok()) {
      Fr& f = st[d - 1];
      if (f.kind == T_STRUCT) {
        const uint32_t ft = r.u8();
        if (ft == T_STOP) {
          d--;
          continue;
        }
        r.be16();
        cur = ft;
        have = true;
      } else if (f.n == 0) {
        d--;
      } else {
        cur = (f.kind == T_MAP && (f.n & 1u)) ? f.t2 : f.t1;
        f.n--;
        have = true;
      }
    }
    if (!have) return;
  }
}

// a container skipped out of line: the reader's fields go by value and the new position /
// error come back in registers, so a call site does not force the caller's reader (or any
// other parser state) into scratch memory; the walker's own stack lives in the callee's frame
struct SkipRes {
  uint64_t pos;
  int32_t err;
};
__device__ __attribute__((noinline)) SkipRes skip_v(const uint8_t* b, uint64_t pos, uint64_t end, uint64_t total,
                                                    const LDS3 uint8_t* sb, uint64_t s_lo, uint64_t s_n, uint32_t t) {
  Rd r;
  r.init(b, pos, end, total);
  r.sb = sb;
  r.s_lo = s_lo;
  r.s_n = s_n;
  skip_body(r, t);
  return SkipRes{r.pos, r.err};
}
__device__ __forceinline__ void skip(Rd& r, uint32_t t) {
  if (r.err) return;
  const SkipRes x = skip_v(r.b, r.pos, r.end, r.total, r.sb, r.s_lo, r.s_n, t);
  r.pos = x.pos;
  r.err = x.err;
}

// skip one value: a fixed-size or string value inline; a container through skip() (a call:
// its explicit stack lives in scratch, so the common field types must not pay for it)
__device__ __forceinline__ void skip1(Rd& r, uint32_t t) {
  if (const uint32_t fs = fixed_size(t)) {
    if (r.need(fs)) r.pos += fs;
  } else if (t == T_STRING) {
    const uint32_t n = (uint32_t)r.size();
    if (r.need(n)) r.pos += n;
  } else {
    skip(r, t);
  }
}

// the wave's blobs [wb0, wb0 + 64) of `bytes` (`total` of them; blob i at [blob_off[i],
// blob_off[i + 1])) into its LDS share of `cap` bytes when their bytes fit: returns the
// staged address range (lo, n; n = 0: nothing staged).  No byte outside [bytes, bytes +
// total) is read, whatever the offsets say.
__device__ void stage_blobs(const uint8_t* bytes, const uint64_t* blob_off, uint64_t total, uint32_t cap,
                            uint32_t n_blobs, uint32_t wb0, uint32_t lane, LDS3 uint4* dst, uint64_t* lo_out,
                            uint64_t* n_out) {
  *lo_out = *n_out = 0;
  if (wb0 >= n_blobs) return;
  const uint32_t wb1 = wb0 + 64 < n_blobs ? wb0 + 64 : n_blobs;
  const uint64_t base = (uint64_t)(uintptr_t)bytes;
  const uint64_t A = base + blob_off[wb0], E = base + blob_off[wb1];
  const uint64_t A16 = A & ~15ull;
  if (E <= A || E - A16 > cap) return;
  const uint64_t lim = base + total;
  for (uint64_t i = (uint64_t)lane * 16u; A16 + i < E; i += 64u * 16u) {
    const uint64_t a = A16 + i;
    uint4 v;
    if (a >= base && a + 16 <= lim) {
      v = *reinterpret_cast<const uint4*>((uintptr_t)a);
    } else {  // the buffer's first / last partial 16 bytes
      uint32_t w[4] = {0, 0, 0, 0};
      for (uint32_t j = 0; j < 16; j++)
        if (a + j >= base && a + j < lim) w[j >> 2] |= (uint32_t)bytes[a + j - base] << (8 * (j & 3));
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    LDS3 uint32_t* d4 = (LDS3 uint32_t*)dst + (i >> 2);
    d4[0] = v.x;
    d4[1] = v.y;
    d4[2] = v.z;
    d4[3] = v.w;
  }
  *lo_out = A16;
  *n_out = E - A16;
}

// ---------------------------------------------------------------- seeds, collect, rank
__global__ void k_seed(STab T, const uint8_t* bytes, const uint64_t* off, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 || i >= n) return;  // seed 0 is "" (handle 0, never in the table)
  const uint64_t a = off[i], len = off[i + 1] - a;
  if (len == 0) return;
  tab_insert(T, cdr_str_hash(bytes + a, len), a | SEED_REF, (uint32_t)len, i);
}

// seeds may collide with one another only by equal strings; the first claimant keeps its
// handle, the table's value is what lookups return

// the new strings' slots (key set, value UNASSIGNED), in two passes over the table and no
// shared counter: each of COLLECT_WG workgroups counts the new slots of its span of the
// table, the counts are scanned, and each workgroup writes its slots from its offset (one
// atomic per wavefront on a single counter took 8.9 ms: millions of new strings)
constexpr uint32_t COLLECT_WG = 2048;
__device__ __forceinline__ bool is_new(const STab& T, uint64_t i, unsigned long long* k) {
  *k = i <= T.mask ? T.key[i] : 0ull;
  return *k != 0ull && T.val[i] == UNASSIGNED;
}
__global__ __launch_bounds__(256) void k_collect_count(STab T, uint32_t* counts) {
  const uint64_t span = ((T.mask + 1 + COLLECT_WG - 1) / COLLECT_WG + 255) & ~255ull;
  const uint64_t lo = (uint64_t)blockIdx.x * span;
  uint32_t c = 0;
  for (uint64_t i = lo + threadIdx.x; i < lo + span && i <= T.mask; i += 256) {
    unsigned long long k;
    c += is_new(T, i, &k) ? 1u : 0u;
  }
  for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o, 64);
  __shared__ uint32_t part[4];
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) counts[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
__global__ __launch_bounds__(256) void k_collect_write(STab T, const uint32_t* offs, unsigned long long* keys,
                                                       uint64_t* idx) {
  const uint64_t span = ((T.mask + 1 + COLLECT_WG - 1) / COLLECT_WG + 255) & ~255ull;
  const uint64_t lo = (uint64_t)blockIdx.x * span;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  __shared__ uint32_t part[4];
  uint32_t base = offs[blockIdx.x];
  for (uint64_t c0 = lo; c0 < lo + span && c0 <= T.mask; c0 += 256) {
    const uint64_t i = c0 + threadIdx.x;
    unsigned long long k;
    const bool take = i < lo + span && is_new(T, i, &k);
    const uint64_t m = __builtin_amdgcn_ballot_w64(take);
    __syncthreads();  // the previous chunk's reads of part[] are done
    if (lane == 0) part[wv] = (uint32_t)__builtin_popcountll(m);
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t v = 0; v < 4; v++) {
      before += v < wv ? part[v] : 0u;
      total += part[v];
    }
    if (take) {
      const uint32_t j = base + before +
                         __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      keys[j] = k;
      idx[j] = i;
    }
    base += total;
  }
}

__global__ void k_rank(STab T, const uint64_t* idx_sorted, uint32_t n_new, uint32_t n_seeds, uint64_t* str_ref,
                       uint32_t* str_len) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_new) return;
  const uint64_t s = idx_sorted[j];
  const uint32_t h = n_seeds + j;
  T.val[s] = h;
  str_ref[h] = T.ref[s];
  str_len[h] = T.len[s];
}

__global__ void k_seed_refs(const uint64_t* off, uint32_t n, uint64_t* str_ref, uint32_t* str_len) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  str_ref[i] = off[i] | SEED_REF;
  str_len[i] = (uint32_t)(off[i + 1] - off[i]);
}

}  // namespace
