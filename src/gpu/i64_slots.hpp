// The 16-byte {key, row+1} slot and its hash-to-slot mapping, shared by the
// wide join table (join_fast.hip) and the int64 group-by (hashtable_i64.hip).
#pragma once
#include "srj_common.hpp"

namespace srj {

struct Slot64 {
  long long key;
  long long row1;  // low 62 bits: row + 1 (0 = empty); bit 62: chain bit,
                   // set when some LATER insert probed through this slot —
                   // a probe may stop at the first clear chain bit instead
                   // of loading slots until it sees an empty one (cuts the
                   // common case from 2 random loads to 1)
};

constexpr long long SLOT_CHAIN = 1ll << 62;
constexpr long long SLOT_ROW = SLOT_CHAIN - 1;

constexpr int PIPE = 8;  // rows per lane and batch

__device__ inline uint64_t i64_hash(long long k) { return mix64((uint64_t)k); }

// Slot from the TOP hash bits (mask = 2^k - 1). This orders the table by
// hash prefix; a radix-partitioned probe over it was built and measured NOT
// to pay on the 10Bx1B config (docs/PERF.md) — the layout is kept because it
// is equivalent in cost to low-bit indexing and keeps that option open.
__device__ inline uint64_t slot_of(uint64_t h, uint64_t mask) {
  return h >> __builtin_clzll(mask);
}

}  // namespace srj
