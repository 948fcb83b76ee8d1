// The join fast path (single integer key; the NDS hot path: fact-table joins
// on surrogate keys, BASELINE config[2]): three table layouts, a build kernel
// each, and one probe pipeline over all of them (join_probe.hpp).
//
// Why a separate design from hashtable.hip's generic (fp|row) table: the
// generic probe is a dependent chain of TWO random loads per row (slot word,
// then the build key for equality). rocprof on the v1 kernel showed it
// latency-bound at ~3% of HBM bandwidth (profiles/r01_join_v1_kernel_stats).
// Here the key is inline in the slot, so a probe is ONE random load per slot
// visited, and builds and probes are software-pipelined batches of PIPE rows
// per lane: first-slot accesses for the whole batch issue independently
// before any is resolved (memory-level parallelism instead of one dependent
// chain).
//
//   wide    16-byte {key, row+1} slots, any int64 key
//   narrow  8-byte key-kmin | row+1 | chain words, key range within 32 bits
//   dense   4-byte row+1 words addressed by key-kmin, no hashing, for a
//           duplicate-free key column of a dense range
//   ordered no table at all: build row i holds key kmin + i, so the word the
//           dense table would hold at key-kmin is key-kmin+1. One scan of the
//           build keys (join_scan_keys) finds the range and this order.
#include "i64_slots.hpp"
#include "join_probe.hpp"

namespace srj {

// ---------------------------------------------------------------------------
// wide table. Claim protocol: atomicCAS on the row word (0 = empty), winner
// writes key; no sentinel key needed, build completes before probe launches.
// ---------------------------------------------------------------------------
__global__ void join_build_i64_kernel(const long long* __restrict__ keys,
                                      const uint8_t* __restrict__ valid,
                                      int64_t nrows, Slot64* __restrict__ slots,
                                      uint64_t mask) {
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  // batch of PIPE strided rows per iteration
  for (int64_t base = tid * PIPE; base < nrows; base += nthreads * PIPE) {
    long long k[PIPE];
    uint64_t s[PIPE];
    bool act[PIPE];
    long long prev[PIPE];
#pragma unroll
    for (int b = 0; b < PIPE; ++b) {
      int64_t row = base + b;
      act[b] = row < nrows && is_valid(valid, row);
      k[b] = act[b] ? keys[row < nrows ? row : 0] : 0;
      s[b] = act[b] ? slot_of(i64_hash(k[b]), mask) : 0;
    }
    // first-slot claims issued back-to-back (independent atomics pipeline
    // with counted vmcnt); inactive lanes CAS 0->0 on slot 0, a no-op
#pragma unroll
    for (int b = 0; b < PIPE; ++b) {
      prev[b] = atomicCAS(
          reinterpret_cast<unsigned long long*>(&slots[s[b]].row1), 0ull,
          (unsigned long long)(act[b] ? base + b + 1 : 0));
    }
#pragma unroll
    for (int b = 0; b < PIPE; ++b) {
      if (!act[b]) continue;
      if (prev[b] == 0) {
        slots[s[b]].key = k[b];
        continue;
      }
      int64_t row = base + b;
      // mark the displaced-over slots so probes know the chain continues
      atomicOr(reinterpret_cast<unsigned long long*>(&slots[s[b]].row1),
               (unsigned long long)SLOT_CHAIN);
      uint64_t sl = (s[b] + 1) & mask;
      while (true) {
        long long p = atomicCAS(
            reinterpret_cast<unsigned long long*>(&slots[sl].row1), 0ull,
            (unsigned long long)(row + 1));
        if (p == 0) {
          slots[sl].key = k[b];
          break;
        }
        atomicOr(reinterpret_cast<unsigned long long*>(&slots[sl].row1),
                 (unsigned long long)SLOT_CHAIN);
        sl = (sl + 1) & mask;
      }
    }
  }
}

struct WideLayout {
  using Tag = long long;  // the key itself
  using Word = longlong2;  // {key, row1} in one load
  using Index = uint64_t;
  static constexpr bool CHAINED = true;
  // per wave and batch: at 2^28 slots of 16 bytes and 4 waves per SIMD the
  // workgroup append's barriers cost 1.3 % (docs/PERF.md)
  static constexpr bool WG_APPEND = false;
  const longlong2* slots;
  uint64_t mask;

  __device__ Index index(long long key, Tag& tag, bool& live) const {
    tag = key;
    live = true;
    return slot_of(i64_hash(key), mask);
  }
  __device__ Index reindex(Tag tag) const {
    return slot_of(i64_hash(tag), mask);
  }
  __device__ Index next(Index i) const { return (i + 1) & mask; }
  __device__ Word load(Index i) const { return slots[i]; }
  __device__ static bool empty(Word w) { return w.y == 0; }
  __device__ static bool match(Word w, Tag tag) { return w.x == tag; }
  __device__ static bool chain(Word w) { return w.y & SLOT_CHAIN; }
  // the build side is capped below 2^31 rows
  __device__ static uint32_t row1(Word w) { return (uint32_t)(w.y & SLOT_ROW); }
};

// ---------------------------------------------------------------------------
// narrow table: 8-byte slots for keys whose range fits 32 bits (INT32/DATE32
// columns, packed multi-key tuples, int64 surrogate keys of a dense range).
//   word = (key - kmin) | (row + 1) << 32 | chain << 63;   0 = empty
// One CAS 0 -> word claims the slot and publishes key and row together, so an
// insert is one memory-side transaction instead of a CAS plus a scattered
// key store, and the table is half the bytes at the same load. The slot index
// still comes from the hash of the ORIGINAL key (part_hist / part_scatter
// prefixes line up with table windows exactly as for the wide table).
// K is the key column's element type: int columns are read in place.
// ---------------------------------------------------------------------------
constexpr unsigned long long NSLOT_CHAIN = 1ull << 63;
constexpr uint32_t NSLOT_ROW = 0x7fffffffu;  // of the word's high half

template <typename K>
__global__ void join_build_n32_kernel(const K* __restrict__ keys,
                                      const uint8_t* __restrict__ valid,
                                      int64_t nrows,
                                      unsigned long long* __restrict__ slots,
                                      uint64_t mask, long long kmin) {
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  for (int64_t base = tid * PIPE; base < nrows; base += nthreads * PIPE) {
    unsigned long long w[PIPE];
    uint64_t s[PIPE];
    unsigned long long prev[PIPE];
#pragma unroll
    for (int b = 0; b < PIPE; ++b) {
      int64_t row = base + b;
      bool act = row < nrows && is_valid(valid, row);
      long long k = act ? (long long)keys[row] : 0;
      // the host guarantees key - kmin < 2^32 for every valid build row
      w[b] = act ? ((uint64_t)(uint32_t)((uint64_t)k - (uint64_t)kmin) |
                    (uint64_t)(row + 1) << 32)
                 : 0ull;
      s[b] = act ? slot_of(i64_hash(k), mask) : 0;
    }
    // first-slot claims back-to-back; inactive lanes CAS 0->0 on slot 0
#pragma unroll
    for (int b = 0; b < PIPE; ++b) prev[b] = atomicCAS(&slots[s[b]], 0ull, w[b]);
#pragma unroll
    for (int b = 0; b < PIPE; ++b) {
      if (w[b] == 0 || prev[b] == 0) continue;
      // mark the displaced-over slots so probes know the chain continues
      atomicOr(&slots[s[b]], NSLOT_CHAIN);
      uint64_t sl = (s[b] + 1) & mask;
      while (atomicCAS(&slots[sl], 0ull, w[b]) != 0) {
        atomicOr(&slots[sl], NSLOT_CHAIN);
        sl = (sl + 1) & mask;
      }
    }
  }
}

// A lane keeps only the 32-bit key offset and the fetched word per row, which
// keeps the batch state small enough for a fifth wave per SIMD.
struct NarrowLayout {
  using Tag = uint32_t;  // key - kmin
  using Word = unsigned long long;
  using Index = uint64_t;
  static constexpr bool CHAINED = true;
  static constexpr bool WG_APPEND = true;
  const unsigned long long* slots;
  uint64_t mask;
  long long kmin;

  __device__ Index index(long long key, Tag& tag, bool& live) const {
    uint64_t o = (uint64_t)key - (uint64_t)kmin;
    tag = (uint32_t)o;
    // an offset past 32 bits can never match; it must not alias
    live = !(o >> 32);
    return slot_of(i64_hash(key), mask);
  }
  __device__ Index reindex(Tag tag) const {
    return slot_of(i64_hash((long long)((uint64_t)kmin + (uint64_t)tag)), mask);
  }
  __device__ Index next(Index i) const { return (i + 1) & mask; }
  __device__ Word load(Index i) const { return slots[i]; }
  __device__ static bool empty(Word w) { return w == 0; }
  __device__ static bool match(Word w, Tag tag) { return (uint32_t)w == tag; }
  __device__ static bool chain(Word w) { return w & NSLOT_CHAIN; }
  __device__ static uint32_t row1(Word w) {
    return (uint32_t)(w >> 32) & NSLOT_ROW;
  }
};

// ---------------------------------------------------------------------------
// dense table: direct addressing for dense, duplicate-free integer build keys
// (the shape of nearly every NDS surrogate key: d_date_sk, i_item_sk, ...).
//   slots[key - kmin] = row + 1;   0 = empty;   one uint32 per key of
//   [kmin, kmin + range)
// Hashing is work such a join does not need: the table is range x 4 B (an
// eighth of the narrow table at 25 % load), a build is one CAS per row with
// no chain, and a probe is one 4-byte load per row with at most one match. A
// duplicate build key cannot be represented: the build raises a flag and the
// host falls back to the hashed tables.
// ---------------------------------------------------------------------------
constexpr int DPIPE = 8;  // build rows per lane and iteration

// Rows of a wave are interleaved (row = wave base + b * 64 + lane), not
// consecutive per lane: for sorted keys the 64 claims of one atomic
// instruction are then one contiguous 256-byte segment, the shape memory-side
// atomics run at full rate for, and the key loads are fully coalesced.
// Keys and validity bytes load unconditionally (clamped) and every lane
// issues its DPIPE claims back-to-back: a row that is null or past the end
// issues CAS 0 -> 0, a no-op on whatever slot it lands on, spread over the
// table's first 64 slots so that nulls do not pile onto one address.
// flag (one word, ordinary stores): bit 0 = duplicate key, bit 1 = a key
// outside [kmin, kmin + range), which the host rules out; such a row is
// dropped, never stored out of bounds.
template <typename K>
__global__ void join_build_d32_kernel(const K* __restrict__ keys,
                                      const uint8_t* __restrict__ valid,
                                      int64_t nrows,
                                      uint32_t* __restrict__ slots,
                                      uint64_t range, long long kmin,
                                      uint32_t* __restrict__ flag) {
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t nwaves = (int64_t)gridDim.x * blockDim.x / WAVE;
  uint32_t lane = threadIdx.x & (WAVE - 1);
  uint32_t idle = lane < range ? lane : 0u;  // slot of this lane's no-op CAS
  constexpr int64_t WROWS = (int64_t)WAVE * DPIPE;
  uint32_t bad = 0;
  for (int64_t base = (tid / WAVE) * WROWS; base < nrows;
       base += nwaves * WROWS) {
    long long k[DPIPE];
    uint32_t vb[DPIPE];
    uint32_t o[DPIPE], w[DPIPE], prev[DPIPE];
#pragma unroll
    for (int b = 0; b < DPIPE; ++b) {
      int64_t row = base + (int64_t)b * WAVE + lane;
      int64_t crow = row < nrows ? row : 0;
      k[b] = (long long)keys[crow];
      vb[b] = valid ? (uint32_t)valid[crow >> 3] : 0xffu;
    }
#pragma unroll
    for (int b = 0; b < DPIPE; ++b) {
      int64_t row = base + (int64_t)b * WAVE + lane;
      bool act = row < nrows && ((vb[b] >> (row & 7)) & 1);
      uint64_t off = (uint64_t)k[b] - (uint64_t)kmin;
      if (act && off >= range) {
        bad |= 2u;
        act = false;
      }
      o[b] = act ? (uint32_t)off : idle;
      w[b] = act ? (uint32_t)(row + 1) : 0u;
    }
#pragma unroll
    for (int b = 0; b < DPIPE; ++b) prev[b] = atomicCAS(&slots[o[b]], 0u, w[b]);
    // a failed claim of a live row is a duplicate key: no chain, no retry
#pragma unroll
    for (int b = 0; b < DPIPE; ++b)
      if (w[b] != 0 && prev[b] != 0) bad |= 1u;
  }
  if (bad) atomicOr(flag, bad);
}

// A key is live when key - kmin, compared as a full 64-bit value, is below
// range; a dead row loads slot 0, so no load leaves the table and an offset
// that wraps past 2^32 or 2^63 cannot alias.
struct DenseLayout {
  struct Tag {};  // the slot index is the whole comparison
  using Word = uint32_t;
  using Index = uint32_t;
  static constexpr bool CHAINED = false;
  static constexpr bool WG_APPEND = true;
  const uint32_t* slots;
  uint64_t range;
  long long kmin;

  __device__ Index index(long long key, Tag&, bool& live) const {
    uint64_t o = (uint64_t)key - (uint64_t)kmin;
    live = o < range;
    return live ? (uint32_t)o : 0u;
  }
  __device__ Word load(Index i) const { return slots[i]; }
  __device__ static bool empty(Word w) { return w == 0; }
  __device__ static bool match(Word, Tag) { return true; }
  __device__ static uint32_t row1(Word w) { return w; }
};

// ---------------------------------------------------------------------------
// ordered build keys: key[i] = kmin + i for every row, all rows valid. The
// dense table of such a column would hold slots[o] = o + 1, so the probe
// computes the word from the key it has already loaded and touches no table:
// it streams keys in and pairs out. The offset rules are the dense table's.
// ---------------------------------------------------------------------------
struct OrderedLayout {
  struct Tag {};
  using Word = uint32_t;
  using Index = uint32_t;  // the word itself; load() is the identity
  static constexpr bool CHAINED = false;
  static constexpr bool WG_APPEND = true;
  static constexpr bool NT_OUT = true;
  uint64_t range;  // build rows, below 2^31
  long long kmin;

  __device__ Index index(long long key, Tag&, bool& live) const {
    uint64_t o = (uint64_t)key - (uint64_t)kmin;
    live = o < range;
    return live ? (uint32_t)o + 1u : 0u;
  }
  __device__ Word load(Index i) const { return i; }
  __device__ static bool empty(Word w) { return w == 0; }
  __device__ static bool match(Word, Tag) { return true; }
  __device__ static uint32_t row1(Word w) { return w; }
};

// One pass over a single integer key column: signed min, signed max, and
// whether the column is ordered, i.e. every row i is valid and
// (uint64)key[i] - (uint64)key[0] == i (an int key is sign-extended first).
// out = {min, max, ordered}, initialised to {INT64_MAX, INT64_MIN, 1} by
// join_scan_init_kernel on the same stream; each workgroup reduces per wave,
// then through LDS, and finishes with one atomic min, one atomic max and, if
// it saw a violation, one atomic and. No workgroup waits on another.
// VEC: 16-byte loads (keys 16-byte aligned); rows past the last whole vector
// are taken one per thread by the first threads of the grid. A vector index
// past the end is clamped to the thread's first one: re-reducing a row
// changes nothing, so the SCAN_UNROLL loads of an iteration issue together
// with no branch between them. Validity is read only when a mask is given,
// one byte per vector (a vector never straddles a byte), and only bits of
// rows below n are looked at. Min and max cover null rows too, as the
// range scan they replace did.
// ---------------------------------------------------------------------------
constexpr int SCAN_UNROLL = 4;

__global__ void join_scan_init_kernel(long long* __restrict__ out) {
  out[0] = INT64_MAX;
  out[1] = INT64_MIN;
  out[2] = 1;
}

template <typename K, bool VEC>
__global__ void __launch_bounds__(DEFAULT_BLOCK)
join_scan_keys_kernel(const K* __restrict__ keys,
                      const uint8_t* __restrict__ valid, int64_t n,
                      long long* __restrict__ out) {
  constexpr int N = VEC ? 16 / (int)sizeof(K) : 1;
  struct alignas(sizeof(K) * N) Vec {
    K e[N];
  };
  constexpr int NW = DEFAULT_BLOCK / WAVE;
  __shared__ long long slo[NW], shi[NW];
  __shared__ uint32_t sbad[NW];
  const Vec* __restrict__ vk = reinterpret_cast<const Vec*>(keys);
  const int64_t nvec = n / N;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  const uint64_t k0 = (uint64_t)(long long)keys[0];  // n >= 1
  long long lo = INT64_MAX, hi = INT64_MIN;
  bool bad = false;
  auto take = [&](K key, int64_t row, uint32_t vbyte) {
    long long k = (long long)key;
    lo = k < lo ? k : lo;
    hi = k > hi ? k : hi;
    bad |= (uint64_t)k - k0 != (uint64_t)row;
    bad |= !((vbyte >> (row & 7)) & 1u);
  };
  for (int64_t v0 = tid; v0 < nvec; v0 += nthreads * SCAN_UNROLL) {
    Vec x[SCAN_UNROLL];
    uint32_t vb[SCAN_UNROLL];
#pragma unroll
    for (int u = 0; u < SCAN_UNROLL; ++u) {
      int64_t v = v0 + u * nthreads;
      v = v < nvec ? v : v0;
      x[u] = vk[v];
      vb[u] = valid ? (uint32_t)valid[(v * N) >> 3] : 0xffu;
    }
#pragma unroll
    for (int u = 0; u < SCAN_UNROLL; ++u) {
      int64_t v = v0 + u * nthreads;
      v = v < nvec ? v : v0;
#pragma unroll
      for (int j = 0; j < N; ++j) take(x[u].e[j], v * N + j, vb[u]);
    }
  }
  {
    int64_t row = nvec * N + tid;
    if (row < n)
      take(keys[row], row, valid ? (uint32_t)valid[row >> 3] : 0xffu);
  }
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    long long l = __shfl_down(lo, off, WAVE);
    long long h = __shfl_down(hi, off, WAVE);
    lo = l < lo ? l : lo;
    hi = h > hi ? h : hi;
  }
  const bool wbad = __ballot(bad) != 0;
  if (lane == 0) {
    slo[wave] = lo;
    shi[wave] = hi;
    sbad[wave] = wbad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t b = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      lo = slo[w] < lo ? slo[w] : lo;
      hi = shi[w] > hi ? shi[w] : hi;
      b |= sbad[w];
    }
    atomicMin(&out[0], lo);
    atomicMax(&out[1], hi);
    if (b) atomicAnd(reinterpret_cast<unsigned long long*>(&out[2]), 0ull);
  }
}

// Dense probe geometry, chosen by measurement (docs/PERF.md): 8 rows per lane
// keeps 8 waves per SIMD, and a 1024-thread workgroup reserves output space
// once per 8192 rows. With the workgroup append, 16 rows per lane no longer
// win at any table size.
constexpr int DENSE_PPIPE = 8;
constexpr int DENSE_BLOCK = 1024;

// What a probe launch takes besides its keys and its table; the entry points
// of a layout differ only in which of these they expose.
struct ProbeOut {
  uint64_t* counter;
  int32_t* out_build;
  int64_t* out_probe;
  int64_t out_capacity;
  uint8_t* build_matched;
  int32_t fill;
  const int32_t* idxmap;
  ProbeEmit emit;
  uint8_t* probe_hit;
  int32_t anti;
};

template <typename L, int PPIPE, int BLOCK>
static void probe_keys(const void* probe, int32_t key_i32,
                       const uint8_t* pvalid, int64_t nprobe, L l,
                       const ProbeOut& o, hipStream_t stream) {
  if (key_i32)
    launch_probe<L, int, PPIPE, BLOCK>(
        reinterpret_cast<const int*>(probe), pvalid, nprobe, l, o.counter,
        o.out_build, o.out_probe, o.out_capacity, o.build_matched, o.fill,
        o.idxmap, stream, o.emit, o.probe_hit, o.anti);
  else
    launch_probe<L, long long, PPIPE, BLOCK>(
        reinterpret_cast<const long long*>(probe), pvalid, nprobe, l,
        o.counter, o.out_build, o.out_probe, o.out_capacity, o.build_matched,
        o.fill, o.idxmap, stream, o.emit, o.probe_hit, o.anti);
}

// batch 16 measured slower for the wide table (12.5 vs 15.8 B rows/s):
// occupancy drop
static void probe_wide(const long long* probe, const uint8_t* pvalid,
                       int64_t nprobe, const void* slots, int64_t capacity,
                       const ProbeOut& o, hipStream_t stream) {
  WideLayout l{reinterpret_cast<const longlong2*>(slots),
               (uint64_t)(capacity - 1)};
  launch_probe<WideLayout, long long, PIPE, DEFAULT_BLOCK>(
      probe, pvalid, nprobe, l, o.counter, o.out_build, o.out_probe,
      o.out_capacity, o.build_matched, o.fill, o.idxmap, stream, o.emit,
      o.probe_hit, o.anti);
}

static void probe_narrow(const void* probe, int32_t key_i32,
                         const uint8_t* pvalid, int64_t nprobe,
                         const void* slots, int64_t capacity, long long kmin,
                         const ProbeOut& o, hipStream_t stream) {
  NarrowLayout l{reinterpret_cast<const unsigned long long*>(slots),
                 (uint64_t)(capacity - 1), kmin};
  probe_keys<NarrowLayout, PIPE, DEFAULT_BLOCK>(probe, key_i32, pvalid,
                                                nprobe, l, o, stream);
}

static void probe_dense(const void* probe, int32_t key_i32,
                        const uint8_t* pvalid, int64_t nprobe,
                        const void* slots, int64_t range, long long kmin,
                        const ProbeOut& o, hipStream_t stream) {
  DenseLayout l{reinterpret_cast<const uint32_t*>(slots), (uint64_t)range,
                kmin};
  probe_keys<DenseLayout, DENSE_PPIPE, DENSE_BLOCK>(probe, key_i32, pvalid,
                                                    nprobe, l, o, stream);
}

// Ordered probe geometry, chosen by measurement (docs/PERF.md, "ordered"):
// with no random load the kernel streams, and what is left to amortise is the
// reservation, two barriers and one atomic per tile. 16 rows per lane in a
// 1024-thread workgroup reserve once per 16384 rows; with nontemporal pair
// stores that is 3.30 ms per 1B rows against 3.55 at 8 rows per lane with
// plain stores, and 6.2 at 256 threads x 8 rows.
constexpr int ORD_PPIPE = 16;
constexpr int ORD_BLOCK = 1024;

static void probe_ordered(const void* probe, int32_t key_i32,
                          const uint8_t* pvalid, int64_t nprobe, int64_t range,
                          long long kmin, const ProbeOut& o,
                          hipStream_t stream) {
  OrderedLayout l{(uint64_t)range, kmin};
  probe_keys<OrderedLayout, ORD_PPIPE, ORD_BLOCK>(probe, key_i32, pvalid,
                                                  nprobe, l, o, stream);
}

}  // namespace srj

using namespace srj;

extern "C" {

// probe rows per workgroup and iteration: layout 0 wide, 1 narrow, 2 dense,
// 3 ordered
int32_t srj_join_probe_tile(int32_t layout) {
  if (layout == 3) return ORD_BLOCK * ORD_PPIPE;
  return layout == 2 ? DENSE_BLOCK * DENSE_PPIPE : DEFAULT_BLOCK * PIPE;
}

// out: three int64 words {min, max, ordered} (see the kernel); n >= 1.
void srj_join_scan_keys(const void* keys, int32_t key_i32,
                        const uint8_t* valid, int64_t n, long long* out,
                        hipStream_t stream) {
  join_scan_init_kernel<<<1, 1, 0, stream>>>(out);
  const bool vec = (reinterpret_cast<uintptr_t>(keys) & 15u) == 0;
  const int per = vec ? (key_i32 ? 4 : 2) : 1;
  int64_t g = grid_1d((n / per + SCAN_UNROLL - 1) / SCAN_UNROLL);
  auto launch = [&](auto* k, auto kernel) {
    kernel<<<g, DEFAULT_BLOCK, 0, stream>>>(k, valid, n, out);
  };
  if (key_i32) {
    auto* k = reinterpret_cast<const int*>(keys);
    if (vec) launch(k, join_scan_keys_kernel<int, true>);
    else launch(k, join_scan_keys_kernel<int, false>);
  } else {
    auto* k = reinterpret_cast<const long long*>(keys);
    if (vec) launch(k, join_scan_keys_kernel<long long, true>);
    else launch(k, join_scan_keys_kernel<long long, false>);
  }
}

void srj_join_build_i64(const long long* keys, const uint8_t* valid, int64_t nrows,
                        void* slots, int64_t capacity, hipStream_t stream) {
  int64_t nthreads_needed = (nrows + PIPE - 1) / PIPE;
  join_build_i64_kernel<<<grid_1d(nthreads_needed), DEFAULT_BLOCK, 0, stream>>>(
      keys, valid, nrows, reinterpret_cast<Slot64*>(slots),
      (uint64_t)(capacity - 1));
}

void srj_join_probe_i64(const long long* probe, const uint8_t* pvalid,
                        int64_t nprobe, const void* slots, int64_t capacity,
                        uint64_t* counter, int32_t* out_build, int64_t* out_probe,
                        int64_t out_capacity, uint8_t* build_matched, int32_t fill,
                        const int32_t* idxmap, hipStream_t stream) {
  probe_wide(probe, pvalid, nprobe, slots, capacity,
             {counter, out_build, out_probe, out_capacity, build_matched, fill,
              idxmap, ProbeEmit::INNER, nullptr, 0},
             stream);
}

// The emit modes of join_probe.hpp on the same tables. mode: 1 left outer
// (build index -1 for an unmatched probe row, counted too), 2 flags:
// probe_hit[row] = has_match ^ anti, and nothing else is written. probe_hit
// is 8-byte aligned and has (nprobe + 15) / 16 * 16 bytes: the hashed layouts
// store 8 flags as one word. The bindings pass no other mode.
void srj_join_probe_mode_i64(const long long* probe, const uint8_t* pvalid,
                             int64_t nprobe, const void* slots,
                             int64_t capacity, uint64_t* counter,
                             int32_t* out_build, int64_t* out_probe,
                             int64_t out_capacity, uint8_t* build_matched,
                             int32_t fill, int32_t mode, uint8_t* probe_hit,
                             int32_t anti, hipStream_t stream) {
  probe_wide(probe, pvalid, nprobe, slots, capacity,
             {counter, out_build, out_probe, out_capacity, build_matched, fill,
              nullptr, (ProbeEmit)mode, probe_hit, anti},
             stream);
}

// key_i32 != 0: keys are a 4-byte int column read in place, else int64
void srj_join_build_n32(const void* keys, int32_t key_i32, const uint8_t* valid,
                        int64_t nrows, void* slots, int64_t capacity,
                        long long kmin, hipStream_t stream) {
  int64_t g = grid_1d((nrows + PIPE - 1) / PIPE);
  auto* sl = reinterpret_cast<unsigned long long*>(slots);
  uint64_t mask = (uint64_t)(capacity - 1);
  if (key_i32)
    join_build_n32_kernel<int><<<g, DEFAULT_BLOCK, 0, stream>>>(
        reinterpret_cast<const int*>(keys), valid, nrows, sl, mask, kmin);
  else
    join_build_n32_kernel<long long><<<g, DEFAULT_BLOCK, 0, stream>>>(
        reinterpret_cast<const long long*>(keys), valid, nrows, sl, mask, kmin);
}

void srj_join_probe_n32(const void* probe, int32_t key_i32,
                        const uint8_t* pvalid, int64_t nprobe, const void* slots,
                        int64_t capacity, long long kmin, uint64_t* counter,
                        int32_t* out_build, int64_t* out_probe,
                        int64_t out_capacity, uint8_t* build_matched,
                        int32_t fill, const int32_t* idxmap,
                        hipStream_t stream) {
  probe_narrow(probe, key_i32, pvalid, nprobe, slots, capacity, kmin,
               {counter, out_build, out_probe, out_capacity, build_matched,
                fill, idxmap, ProbeEmit::INNER, nullptr, 0},
               stream);
}

void srj_join_probe_mode_n32(const void* probe, int32_t key_i32,
                             const uint8_t* pvalid, int64_t nprobe,
                             const void* slots, int64_t capacity,
                             long long kmin, uint64_t* counter,
                             int32_t* out_build, int64_t* out_probe,
                             int64_t out_capacity, uint8_t* build_matched,
                             int32_t fill, int32_t mode, uint8_t* probe_hit,
                             int32_t anti, hipStream_t stream) {
  probe_narrow(probe, key_i32, pvalid, nprobe, slots, capacity, kmin,
               {counter, out_build, out_probe, out_capacity, build_matched,
                fill, nullptr, (ProbeEmit)mode, probe_hit, anti},
               stream);
}

// slots: `range` zeroed words; flag: one zeroed word (see the kernel).
void srj_join_build_d32(const void* keys, int32_t key_i32,
                        const uint8_t* valid, int64_t nrows, void* slots,
                        int64_t range, long long kmin, uint32_t* flag,
                        hipStream_t stream) {
  int64_t g = grid_1d((nrows + DPIPE - 1) / DPIPE);
  auto* sl = reinterpret_cast<uint32_t*>(slots);
  if (key_i32)
    join_build_d32_kernel<int><<<g, DEFAULT_BLOCK, 0, stream>>>(
        reinterpret_cast<const int*>(keys), valid, nrows, sl, (uint64_t)range,
        kmin, flag);
  else
    join_build_d32_kernel<long long><<<g, DEFAULT_BLOCK, 0, stream>>>(
        reinterpret_cast<const long long*>(keys), valid, nrows, sl,
        (uint64_t)range, kmin, flag);
}

void srj_join_probe_d32(const void* probe, int32_t key_i32,
                        const uint8_t* pvalid, int64_t nprobe,
                        const void* slots, int64_t range, long long kmin,
                        uint64_t* counter, int32_t* out_build,
                        int64_t* out_probe, int64_t out_capacity,
                        uint8_t* build_matched, int32_t fill,
                        hipStream_t stream) {
  probe_dense(probe, key_i32, pvalid, nprobe, slots, range, kmin,
              {counter, out_build, out_probe, out_capacity, build_matched,
               fill, nullptr, ProbeEmit::INNER, nullptr, 0},
              stream);
}

void srj_join_probe_mode_d32(const void* probe, int32_t key_i32,
                             const uint8_t* pvalid, int64_t nprobe,
                             const void* slots, int64_t range, long long kmin,
                             uint64_t* counter, int32_t* out_build,
                             int64_t* out_probe, int64_t out_capacity,
                             uint8_t* build_matched, int32_t fill,
                             int32_t mode, uint8_t* probe_hit, int32_t anti,
                             hipStream_t stream) {
  probe_dense(probe, key_i32, pvalid, nprobe, slots, range, kmin,
              {counter, out_build, out_probe, out_capacity, build_matched,
               fill, nullptr, (ProbeEmit)mode, probe_hit, anti},
              stream);
}

// the _d32 entry points without a table: build rows are [kmin, kmin + range)
void srj_join_probe_ord(const void* probe, int32_t key_i32,
                        const uint8_t* pvalid, int64_t nprobe, int64_t range,
                        long long kmin, uint64_t* counter, int32_t* out_build,
                        int64_t* out_probe, int64_t out_capacity,
                        uint8_t* build_matched, int32_t fill,
                        hipStream_t stream) {
  probe_ordered(probe, key_i32, pvalid, nprobe, range, kmin,
                {counter, out_build, out_probe, out_capacity, build_matched,
                 fill, nullptr, ProbeEmit::INNER, nullptr, 0},
                stream);
}

void srj_join_probe_mode_ord(const void* probe, int32_t key_i32,
                             const uint8_t* pvalid, int64_t nprobe,
                             int64_t range, long long kmin, uint64_t* counter,
                             int32_t* out_build, int64_t* out_probe,
                             int64_t out_capacity, uint8_t* build_matched,
                             int32_t fill, int32_t mode, uint8_t* probe_hit,
                             int32_t anti, hipStream_t stream) {
  probe_ordered(probe, key_i32, pvalid, nprobe, range, kmin,
                {counter, out_build, out_probe, out_capacity, build_matched,
                 fill, nullptr, (ProbeEmit)mode, probe_hit, anti},
                stream);
}

}  // extern "C"
