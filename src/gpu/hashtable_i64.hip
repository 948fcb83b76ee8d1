// Specialized int64-key group-by over the 16-byte slots of i64_slots.hpp
// (the joins over the same slots are in join_fast.hip).
#include "i64_slots.hpp"
#include "agg_common.hpp"

namespace srj {

// ---------------------------------------------------------------------------
// specialized int64-key group-by (BASELINE config[1]: hash-aggregate over an
// int64 grouping key). Differences from the generic groupby_kernel:
//   * 16B slots {key, row1} with the key CLAIMED BY CAS (EMPTY_KEY sentinel),
//     so concurrent insert-or-find needs no representative-row re-load: one
//     random 16B load resolves the common hit case;
//   * software-pipelined batches of PIPE rows (hash + first-slot loads issued
//     back-to-back) — the same MLP structure that took the join probe from
//     1.2 to 7.5+ B rows/s;
//   * rows whose key equals the sentinel (INT64_MIN) fall through to a single
//     reserved slot at index `capacity` (aggregated with plain atomics).
// Aggregation itself is the shared agg_accumulate switch.
// ---------------------------------------------------------------------------
constexpr long long GB_EMPTY_KEY = 0x8000000000000000ll;  // INT64_MIN

// returns slot index, or -1 when the table is FULL (undersized cardinality
// hint) — the caller sets the overflow flag and the host re-runs unhinted
__device__ inline int64_t gb64_find_or_claim(Slot64* __restrict__ slots,
                                             uint64_t mask, int64_t capacity,
                                             long long k, int64_t row) {
  if (k == GB_EMPTY_KEY) {
    atomicCAS(reinterpret_cast<unsigned long long*>(&slots[capacity].row1),
              0ull, (unsigned long long)(row + 1));
    return capacity;
  }
  uint64_t sl = slot_of(i64_hash(k), mask);
  Slot64 cur = slots[sl];
  // longest linear-probe cluster at <=50% load is O(log n) (~100 at 4B
  // slots); a chain past 1024 means the table is overloaded (bad hint)
  int64_t bound = (int64_t)mask < 1024 ? (int64_t)mask : 1024;
  for (int64_t probes = 0; probes <= bound; ++probes) {
    if (cur.key == k) return (int64_t)sl;
    if (cur.key == GB_EMPTY_KEY) {
      long long prev = atomicCAS(
          reinterpret_cast<unsigned long long*>(&slots[sl].key),
          (unsigned long long)GB_EMPTY_KEY, (unsigned long long)k);
      if (prev == GB_EMPTY_KEY) {
        slots[sl].row1 = row + 1;
        return (int64_t)sl;
      }
      if (prev == k) return (int64_t)sl;
    }
    sl = (sl + 1) & mask;
    cur = slots[sl];
  }
  return -1;
}

// ---------------------------------------------------------------------------
// LDS pre-aggregated group-by for LOW-cardinality keys (planner hint):
// each workgroup keeps a 2048-slot {key, aggs} table in LDS and only merges
// per-block partials into the global table at the end — global atomic
// traffic drops from one-per-row to one-per-(block x group), fixing the
// hot-address contention that capped 100-group aggregation at 2.5 B rows/s.
// Keys overflowing the LDS table fall through to the direct global path.
// ---------------------------------------------------------------------------
constexpr int GB_LDS_CAP = 2048;   // slots (pow2)
constexpr int GB_LDS_MAX_AGGS = 3;

__global__ void groupby_i64_lds_kernel(
    const long long* __restrict__ keys, int64_t nrows,
    Slot64* __restrict__ slots, uint64_t mask,
    const AggDesc* __restrict__ aggs, int32_t naggs,
    const int64_t* __restrict__ identities,
    int32_t* __restrict__ overflow) {
  __shared__ long long lkey[GB_LDS_CAP];
  __shared__ long long lrep[GB_LDS_CAP];  // a row holding this key
  __shared__ long long lagg[GB_LDS_MAX_AGGS][GB_LDS_CAP];
  int64_t capacity = (int64_t)mask + 1;
  for (int i = threadIdx.x; i < GB_LDS_CAP; i += blockDim.x) {
    lkey[i] = GB_EMPTY_KEY;
    lrep[i] = 0;
    for (int a = 0; a < naggs; ++a) lagg[a][i] = identities[a];
  }
  __syncthreads();

  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       row < nrows; row += stride) {
    // on overflow: BREAK (not return) so every wave still reaches the
    // __syncthreads() before the flush — the host re-runs unhinted anyway
    if (*overflow) break;
    long long k = keys[row];
    int lidx = -1;
    if (k != GB_EMPTY_KEY) {
      uint32_t sl = (uint32_t)(i64_hash(k) >> 32) & (GB_LDS_CAP - 1);
      for (int probe = 0; probe < 32; ++probe) {  // bounded: full -> global
        long long cur = lkey[sl];
        if (cur == k) { lidx = (int)sl; break; }
        if (cur == GB_EMPTY_KEY) {
          long long prev = atomicCAS(
              reinterpret_cast<unsigned long long*>(&lkey[sl]),
              (unsigned long long)GB_EMPTY_KEY, (unsigned long long)k);
          if (prev == GB_EMPTY_KEY) {
            lrep[sl] = row;  // claimer records a representative row
            lidx = (int)sl;
            break;
          }
          if (prev == k) { lidx = (int)sl; break; }
        }
        sl = (sl + 1) & (GB_LDS_CAP - 1);
      }
    }
    if (lidx < 0) {
      // sentinel key or LDS table full: direct global accumulate
      int64_t gi = gb64_find_or_claim(slots, mask, capacity, k, row);
      if (gi < 0) { atomicOr(overflow, 1); continue; }
      agg_accumulate(aggs, naggs, row, gi);
      continue;
    }
    // representative row for the group: claim via global table (once per
    // block per group is fine - find_or_claim is idempotent)
    for (int32_t a = 0; a < naggs; ++a) {
      const AggDesc& g = aggs[a];
      switch (g.op) {
        case AGG_COUNT_ALL:
          atomicAdd(reinterpret_cast<unsigned long long*>(&lagg[a][lidx]),
                    1ull);
          break;
        case AGG_COUNT_VALID:
          if (is_valid(g.valid, row))
            atomicAdd(reinterpret_cast<unsigned long long*>(&lagg[a][lidx]),
                      1ull);
          break;
        case AGG_SUM_INT64:
          if (is_valid(g.valid, row))
            atomicAdd(reinterpret_cast<unsigned long long*>(&lagg[a][lidx]),
                      (unsigned long long)fetch_int64(g.data, g.in_dtype, row));
          break;
        case AGG_SUM_FLOAT64:
          if (is_valid(g.valid, row))
            atomicAdd(reinterpret_cast<double*>(&lagg[a][lidx]),
                      fetch_double(g.data, g.in_dtype, row));
          break;
        case AGG_MIN_INT64:
          if (is_valid(g.valid, row))
            atomicMin(reinterpret_cast<long long*>(&lagg[a][lidx]),
                      (long long)fetch_int64(g.data, g.in_dtype, row));
          break;
        case AGG_MAX_INT64:
          if (is_valid(g.valid, row))
            atomicMax(reinterpret_cast<long long*>(&lagg[a][lidx]),
                      (long long)fetch_int64(g.data, g.in_dtype, row));
          break;
        case AGG_MIN_FLOAT64:
          if (is_valid(g.valid, row))
            atomic_min_f64(reinterpret_cast<double*>(&lagg[a][lidx]),
                           fetch_double(g.data, g.in_dtype, row));
          break;
        case AGG_MAX_FLOAT64:
          if (is_valid(g.valid, row))
            atomic_max_f64(reinterpret_cast<double*>(&lagg[a][lidx]),
                           fetch_double(g.data, g.in_dtype, row));
          break;
      }
    }
  }
  __syncthreads();
  // flush block partials into the global table (merge semantics)
  for (int i = threadIdx.x; i < GB_LDS_CAP; i += blockDim.x) {
    long long k = lkey[i];
    if (k == GB_EMPTY_KEY) continue;
    int64_t gi = gb64_find_or_claim(slots, mask, capacity, k, lrep[i]);
    if (gi < 0) { atomicOr(overflow, 1); continue; }
    for (int32_t a = 0; a < naggs; ++a) {
      const AggDesc& g = aggs[a];
      long long part = lagg[a][i];
      if (part == identities[a]) continue;
      switch (g.op) {
        case AGG_COUNT_ALL:
        case AGG_COUNT_VALID:
        case AGG_SUM_INT64:
          atomicAdd((unsigned long long*)g.state + gi,
                    (unsigned long long)part);
          break;
        case AGG_SUM_FLOAT64: {
          double d;
          __builtin_memcpy(&d, &part, 8);
          atomicAdd(reinterpret_cast<double*>(g.state) + gi, d);
          break;
        }
        case AGG_MIN_INT64:
          atomic_min_i64(reinterpret_cast<int64_t*>(g.state) + gi, part);
          break;
        case AGG_MAX_INT64:
          atomic_max_i64(reinterpret_cast<int64_t*>(g.state) + gi, part);
          break;
        case AGG_MIN_FLOAT64: {
          double d;
          __builtin_memcpy(&d, &part, 8);
          atomic_min_f64(reinterpret_cast<double*>(g.state) + gi, d);
          break;
        }
        case AGG_MAX_FLOAT64: {
          double d;
          __builtin_memcpy(&d, &part, 8);
          atomic_max_f64(reinterpret_cast<double*>(g.state) + gi, d);
          break;
        }
      }
    }
  }
}

__global__ void groupby_i64_kernel(const long long* __restrict__ keys,
                                   int64_t nrows, Slot64* __restrict__ slots,
                                   uint64_t mask,
                                   const AggDesc* __restrict__ aggs,
                                   int32_t naggs,
                                   int32_t* __restrict__ overflow) {
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  int64_t capacity = (int64_t)mask + 1;
  for (int64_t base = tid * PIPE; base < nrows; base += nthreads * PIPE) {
    if (*overflow) return;  // undersized hint: host re-runs unhinted anyway
    long long k[PIPE];
    uint64_t s[PIPE];
    Slot64 first[PIPE];
#pragma unroll
    for (int b = 0; b < PIPE; ++b) {
      int64_t row = base + b;
      k[b] = keys[row < nrows ? row : 0];  // clamped, unconditional
      s[b] = slot_of(i64_hash(k[b]), mask);
    }
#pragma unroll
    for (int b = 0; b < PIPE; ++b) first[b] = slots[s[b]];
#pragma unroll
    for (int b = 0; b < PIPE; ++b) {
      int64_t row = base + b;
      if (row >= nrows) continue;
      int64_t idx;
      if (k[b] == GB_EMPTY_KEY) {
        // reserved overflow slot for the sentinel key value
        idx = capacity;
        atomicCAS(reinterpret_cast<unsigned long long*>(&slots[capacity].row1),
                  0ull, (unsigned long long)(row + 1));
      } else {
        idx = -1;
        Slot64 cur = first[b];
        uint64_t sl = s[b];
        int64_t bound = (int64_t)mask < 1024 ? (int64_t)mask : 1024;
        for (int64_t probes = 0; probes <= bound; ++probes) {
          if (cur.key == k[b]) { idx = (int64_t)sl; break; }
          if (cur.key == GB_EMPTY_KEY) {
            long long prev = atomicCAS(
                reinterpret_cast<unsigned long long*>(&slots[sl].key),
                (unsigned long long)GB_EMPTY_KEY, (unsigned long long)k[b]);
            if (prev == GB_EMPTY_KEY) {
              slots[sl].row1 = row + 1;  // winner records the representative
              idx = (int64_t)sl;
              break;
            }
            if (prev == k[b]) { idx = (int64_t)sl; break; }
            // lost to a different key: fall through and advance
          }
          sl = (sl + 1) & mask;
          cur = slots[sl];
        }
        if (idx < 0) {  // table FULL: undersized hint — host re-runs unhinted
          atomicOr(overflow, 1);
          continue;
        }
      }
      agg_accumulate(aggs, naggs, row, idx);
    }
  }
}

// compact the Slot64 table: same contract as groupby_compact_kernel but with
// 16B slots; scans capacity+1 entries (the reserved sentinel slot included).
// Two-pass compaction: pass 1 counts occupied slots per BLOCK (no global
// atomics), torch.cumsum turns the 2048-entry count array into exclusive
// bases, pass 2 assigns dense output indices from a per-block LDS cursor.
// The single-pass variant's wave-leader atomicAdd on ONE global counter was
// the bottleneck on large tables (512M slots -> 8M same-address atomics,
// 101 ms; two passes run at slot-scan bandwidth instead).

// Loads slot s into word and returns whether it is occupied. s may run past
// the table (a wave's tail lanes reach the ballot too): such a slot is empty.
// Normal slots are occupied iff the key is claimed; the reserved last slot
// keeps the sentinel key and is occupied iff row1 was set.
__device__ inline bool gb64_load_occupied(const Slot64* __restrict__ slots,
                                          int64_t capacity1, int64_t s,
                                          Slot64& word) {
  if (s >= capacity1) return false;
  word = slots[s];
  return s == capacity1 - 1 ? word.row1 != 0 : word.key != GB_EMPTY_KEY;
}

__global__ void groupby_compact_i64_count_kernel(
    const Slot64* __restrict__ slots, int64_t capacity1,
    int64_t* __restrict__ blk_counts) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t cnt = 0;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       s < ((capacity1 + WAVE - 1) & ~(int64_t)(WAVE - 1)); s += stride) {
    Slot64 word;
    uint64_t ballot = __ballot(gb64_load_occupied(slots, capacity1, s, word));
    if ((threadIdx.x & (WAVE - 1)) == 0) cnt += __popcll(ballot);
  }
  __shared__ int64_t red[DEFAULT_BLOCK / WAVE];
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t t = 0;
    for (int w = 0; w < (int)(blockDim.x / WAVE); ++w) t += red[w];
    blk_counts[blockIdx.x] = t;
  }
}

__global__ void groupby_compact_i64_fill_kernel(
    const Slot64* __restrict__ slots, int64_t capacity1,
    const AggDesc* __restrict__ aggs, int32_t naggs,
    const int64_t* __restrict__ blk_bases, int64_t* __restrict__ out_repr,
    int64_t* __restrict__ out_agg_base, int64_t out_capacity) {
  __shared__ unsigned long long cursor;
  if (threadIdx.x == 0) cursor = (unsigned long long)blk_bases[blockIdx.x];
  __syncthreads();
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       s < ((capacity1 + WAVE - 1) & ~(int64_t)(WAVE - 1)); s += stride) {
    Slot64 word;
    bool occ = gb64_load_occupied(slots, capacity1, s, word);
    uint64_t ballot = __ballot(occ);
    int lane = threadIdx.x & (WAVE - 1);
    int nset = __popcll(ballot);
    int leader = __ffsll((unsigned long long)ballot) - 1;
    uint64_t bs = 0;
    if (nset && lane == leader)
      bs = atomicAdd(&cursor, (unsigned long long)nset);  // LDS atomic
    bs = __shfl(bs, leader >= 0 ? leader : 0, WAVE);
    if (occ) {
      uint64_t pos = bs + __popcll(ballot & ((1ull << lane) - 1));
      if ((int64_t)pos < out_capacity) {
        out_repr[pos] = word.row1 - 1;
        for (int32_t a = 0; a < naggs; ++a) {
          out_agg_base[(int64_t)a * out_capacity + (int64_t)pos] =
              reinterpret_cast<const int64_t*>(aggs[a].state)[s];
        }
      }
    }
  }
}

}  // namespace srj

using namespace srj;

extern "C" {

void srj_groupby_i64_lds(const long long* keys, int64_t nrows, void* slots,
                         int64_t capacity, const void* aggs, int32_t naggs,
                         const int64_t* identities, int32_t* overflow,
                         hipStream_t stream) {
  groupby_i64_lds_kernel<<<grid_1d(nrows), DEFAULT_BLOCK, 0, stream>>>(
      keys, nrows, reinterpret_cast<Slot64*>(slots), (uint64_t)(capacity - 1),
      reinterpret_cast<const AggDesc*>(aggs), naggs, identities, overflow);
}

void srj_groupby_i64(const long long* keys, int64_t nrows, void* slots,
                     int64_t capacity, const void* aggs, int32_t naggs,
                     int32_t* overflow, hipStream_t stream) {
  int64_t nthreads_needed = (nrows + PIPE - 1) / PIPE;
  groupby_i64_kernel<<<grid_1d(nthreads_needed), DEFAULT_BLOCK, 0, stream>>>(
      keys, nrows, reinterpret_cast<Slot64*>(slots), (uint64_t)(capacity - 1),
      reinterpret_cast<const AggDesc*>(aggs), naggs, overflow);
}

void srj_groupby_compact_i64_count(const void* slots, int64_t capacity1,
                                   int64_t* blk_counts, hipStream_t stream) {
  groupby_compact_i64_count_kernel<<<grid_1d(capacity1), DEFAULT_BLOCK, 0,
                                     stream>>>(
      reinterpret_cast<const Slot64*>(slots), capacity1, blk_counts);
}

void srj_groupby_compact_i64_fill(const void* slots, int64_t capacity1,
                                  const void* aggs, int32_t naggs,
                                  const int64_t* blk_bases, int64_t* out_repr,
                                  int64_t* out_agg, int64_t out_capacity,
                                  hipStream_t stream) {
  groupby_compact_i64_fill_kernel<<<grid_1d(capacity1), DEFAULT_BLOCK, 0,
                                    stream>>>(
      reinterpret_cast<const Slot64*>(slots), capacity1,
      reinterpret_cast<const AggDesc*>(aggs), naggs, blk_bases, out_repr,
      out_agg, out_capacity);
}

}  // extern "C"
