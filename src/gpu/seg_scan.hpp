// The segmented scan under the window functions (window.hip) and the
// segmented reduce of the sort-based group-by (seg_reduce.hip): the function
// descriptor the bindings fill in, and the device core both kernel families
// scan with. Spark's null, NaN and overflow semantics of count / sum / min /
// max / avg live here, once.
//
// The first part has no HIP in it and is what bind_window.cpp and
// bind_seg_reduce.cpp include; Python mirrors its numeric values in
// ops/_segscan.py. The device part is compiled by hipcc only.
#pragma once
#include <cstdint>

namespace srj {

// The window functions take all eight; the segmented reduce takes
// SF_COUNT..SF_AVG.
enum SegFn : int32_t {
  SF_ROW_NUMBER = 0,
  SF_RANK = 1,
  SF_DENSE_RANK = 2,
  SF_COUNT = 3,
  SF_SUM = 4,
  SF_MIN = 5,
  SF_MAX = 6,
  SF_AVG = 7,
};

// Window frames of the five aggregates; the ranking functions and the
// segmented reduce ignore the frame.
enum SegFrame : int32_t {
  SFR_PARTITION = 0,  // the whole partition
  SFR_ROWS = 1,       // unbounded preceding .. current row
  SFR_RANGE = 2,      // unbounded preceding .. last peer of the current row
};

// Element kind of the value column; `width` is its size in bytes.
enum SegKind : int32_t {
  SK_NONE = 0,  // no value column: ranking functions and count(*)
  SK_BOOL = 1,
  SK_SINT = 2,
  SK_F32 = 3,
  SK_F64 = 4,
};

struct SegFunc {
  int32_t fn;
  int32_t frame;
  int32_t kind;
  int32_t width;
  int64_t stride;        // elements between consecutive rows of `values`
  const void* values;    // read in place as values[perm[i] * stride]
  const uint8_t* valid;  // byte per original row, zero = null; may be null
  void* out;             // out[perm[i]] (window), out[segment number] (reduce)
  uint8_t* out_valid;    // byte per output row; may be null
};

constexpr int SEG_MAX_FUNCS = 8;
constexpr int SEG_EPT = 8;
constexpr int SEG_TILE_ROWS = 256 * SEG_EPT;  // 2048
constexpr int SEG_SMALL_ROWS = SEG_TILE_ROWS;
// tile carries scanned per round of the one-workgroup carry scan
constexpr int SEG_CARRY_PER_THREAD = 4;
constexpr int SEG_CARRY_CHUNK = 256 * SEG_CARRY_PER_THREAD;  // 1024

}  // namespace srj

#ifdef __HIPCC__
#include "srj_common.hpp"

namespace srj {

constexpr int SEG_WAVES = DEFAULT_BLOCK / WAVE;  // 4

static_assert(SEG_TILE_ROWS == DEFAULT_BLOCK * SEG_EPT, "tile");
static_assert(SEG_CARRY_CHUNK == DEFAULT_BLOCK * SEG_CARRY_PER_THREAD,
              "carry chunk");

enum SegOp : int32_t {
  OP_COUNT,  // only the count
  OP_RANK,   // count of rows; acc = position of the last peer head
  OP_SUM_I,
  OP_SUM_F,
  OP_MIN_I,
  OP_MAX_I,
  OP_MIN_F,
  OP_MAX_F,
};

struct SegFuncs {
  SegFunc f[SEG_MAX_FUNCS];
  int32_t nf;
};

// Scan state: head flag, valid values so far, accumulator (int64 or the bits
// of a double, by the op).
struct SegState {
  int32_t flag;
  int64_t cnt;
  uint64_t acc;
};

__device__ inline bool seg_is_float(int32_t kind) {
  return kind == SK_F32 || kind == SK_F64;
}

__device__ inline int32_t seg_op(const SegFunc& f) {
  switch (f.fn) {
    case SF_RANK: return OP_RANK;
    case SF_SUM: return seg_is_float(f.kind) ? OP_SUM_F : OP_SUM_I;
    case SF_AVG: return OP_SUM_F;
    case SF_MIN: return seg_is_float(f.kind) ? OP_MIN_F : OP_MIN_I;
    case SF_MAX: return seg_is_float(f.kind) ? OP_MAX_F : OP_MAX_I;
    default: return OP_COUNT;
  }
}

// Accumulator of the empty state (no flag, count 0). min and max ignore the
// accumulator of a side with count 0.
__device__ inline uint64_t seg_identity(int32_t op) {
  return op == OP_RANK ? ~0ull : 0ull;  // position -1; +0.0; 0
}

__device__ inline double seg_f64(uint64_t b) {
  return __longlong_as_double((long long)b);
}
__device__ inline uint64_t seg_bits(double d) {
  return (uint64_t)__double_as_longlong(d);
}

// Spark order: NaN is greater than every value.
__device__ inline double seg_max_f(double a, double b) {
  if (a != a) return a;
  if (b != b) return b;
  return a > b ? a : b;
}
__device__ inline double seg_min_f(double a, double b) {
  if (a != a) return b;
  if (b != b) return a;
  return a < b ? a : b;
}

// Segmented combine, a to the left of b: b wins outright if it carries a
// head flag.
__device__ inline SegState seg_combine(int32_t op, const SegState& a,
                                       const SegState& b) {
  if (b.flag) return b;
  SegState r;
  r.flag = a.flag;
  r.cnt = a.cnt + b.cnt;
  switch (op) {
    case OP_COUNT:
      r.acc = 0;
      break;
    case OP_RANK:
      r.acc = (int64_t)a.acc > (int64_t)b.acc ? a.acc : b.acc;
      break;
    case OP_SUM_I:
      r.acc = a.acc + b.acc;  // wraps
      break;
    case OP_SUM_F:
      r.acc = seg_bits(seg_f64(a.acc) + seg_f64(b.acc));
      break;
    default:
      if (a.cnt == 0) {
        r.acc = b.acc;
      } else if (b.cnt == 0) {
        r.acc = a.acc;
      } else if (op == OP_MIN_I) {
        r.acc = (int64_t)a.acc < (int64_t)b.acc ? a.acc : b.acc;
      } else if (op == OP_MAX_I) {
        r.acc = (int64_t)a.acc > (int64_t)b.acc ? a.acc : b.acc;
      } else if (op == OP_MIN_F) {
        r.acc = seg_bits(seg_min_f(seg_f64(a.acc), seg_f64(b.acc)));
      } else {
        r.acc = seg_bits(seg_max_f(seg_f64(a.acc), seg_f64(b.acc)));
      }
      break;
  }
  return r;
}

__device__ inline SegState seg_shfl_up(const SegState& s, int off) {
  SegState r;
  r.flag = __shfl_up(s.flag, off, WAVE);
  r.cnt = (int64_t)__shfl_up((long long)s.cnt, off, WAVE);
  r.acc = (uint64_t)__shfl_up((long long)s.acc, off, WAVE);
  return r;
}

// Exclusive segmented prefix of `agg` over the DEFAULT_BLOCK threads in
// thread order, with `carry` combined in front of thread 0; *total is carry
// combined with every thread (the same in all threads). One barrier, between
// the write of wt and its reads; the caller owes one before the next call.
__device__ inline SegState seg_block_scan(int32_t op, const SegState& agg,
                                          const SegState& carry,
                                          SegState (&wt)[SEG_WAVES],
                                          SegState* total) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  SegState inc = agg;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const SegState o = seg_shfl_up(inc, off);
    if (lane >= off) inc = seg_combine(op, o, inc);
  }
  if (lane == WAVE - 1) wt[wave] = inc;
  __syncthreads();
  SegState pre = carry, tot = carry;
#pragma unroll
  for (int w = 0; w < SEG_WAVES; ++w) {
    const SegState t = wt[w];
    if (w < wave) pre = seg_combine(op, pre, t);
    tot = seg_combine(op, tot, t);
  }
  const SegState ex = seg_shfl_up(inc, 1);
  if (lane > 0) pre = seg_combine(op, pre, ex);
  *total = tot;
  return pre;
}

__device__ inline int64_t seg_load_int(const void* p, int64_t e, int32_t kind,
                                       int32_t width) {
  if (kind == SK_BOOL) return static_cast<const uint8_t*>(p)[e] != 0;
  switch (width) {
    case 1: return static_cast<const int8_t*>(p)[e];
    case 2: return static_cast<const int16_t*>(p)[e];
    case 4: return static_cast<const int32_t*>(p)[e];
    default: return static_cast<const int64_t*>(p)[e];
  }
}

// The scan input of the value column of aggregate f at a sorted position that
// holds row `row` (-1: no row of the column there).
__device__ inline SegState seg_value_item(const SegFunc& f, int32_t op,
                                          int64_t row, bool head) {
  SegState x;
  x.flag = head;
  x.cnt = 0;
  x.acc = seg_identity(op);
  if (row < 0) return x;
  if (f.valid != nullptr && f.valid[row] == 0) return x;
  x.cnt = 1;
  if (op == OP_COUNT) return x;
  const int64_t e = row * f.stride;
  if (op == OP_SUM_I || op == OP_MIN_I || op == OP_MAX_I) {
    x.acc = (uint64_t)seg_load_int(f.values, e, f.kind, f.width);
  } else {
    double d;
    if (f.kind == SK_F32) {
      d = static_cast<const float*>(f.values)[e];
    } else if (f.kind == SK_F64) {
      d = static_cast<const double*>(f.values)[e];
    } else {
      d = (double)seg_load_int(f.values, e, f.kind, f.width);
    }
    x.acc = seg_bits(d);
  }
  return x;
}

// out[j] and out_valid[j] of sum, avg, min or max from the closing state
// (cnt, acc) of the frame or segment.
__device__ inline void seg_store_agg(const SegFunc& f, int64_t j, int64_t cnt,
                                     uint64_t acc) {
  const bool has = cnt > 0;
  switch (f.fn) {
    case SF_SUM:
      static_cast<uint64_t*>(f.out)[j] = has ? acc : 0ull;
      break;
    case SF_AVG:
      static_cast<double*>(f.out)[j] = has ? seg_f64(acc) / (double)cnt : 0.0;
      break;
    default:  // min, max: the dtype of the input
      if (f.kind == SK_F32) {
        static_cast<float*>(f.out)[j] = has ? (float)seg_f64(acc) : 0.0f;
      } else if (f.kind == SK_F64) {
        static_cast<uint64_t*>(f.out)[j] = has ? acc : 0ull;
      } else {
        const uint64_t v = has ? acc : 0ull;
        switch (f.width) {
          case 1: static_cast<uint8_t*>(f.out)[j] = (uint8_t)v; break;
          case 2: static_cast<uint16_t*>(f.out)[j] = (uint16_t)v; break;
          case 4: static_cast<uint32_t*>(f.out)[j] = (uint32_t)v; break;
          default: static_cast<uint64_t*>(f.out)[j] = v; break;
        }
      }
      break;
  }
  if (f.out_valid != nullptr) f.out_valid[j] = has ? 1 : 0;
}

// The carry scan of one function by ONE workgroup (the structure of
// block_scan_chunked, with the segmented operator): fw holds (cnt, acc) per
// tile, the state at its last row scanned from its own first row; heads[T] is
// nonzero where tile T holds a head. Turns fw[2T], fw[2T + 1] into the
// carry-in of tile T, the state at the last row of tile T - 1, and calls
// per_tile(T, that state) just before the write. Returns the state at the
// last row of all, in every thread. Ends with a barrier, so wt is free for
// reuse on return.
template <typename PerTile>
__device__ __forceinline__ SegState seg_carry_scan(int32_t op,
                                                   const int64_t* heads,
                                                   int64_t* fw, int64_t nt,
                                                   SegState (&wt)[SEG_WAVES],
                                                   PerTile per_tile) {
  const int64_t nchunks = (nt + SEG_CARRY_CHUNK - 1) / SEG_CARRY_CHUNK;
  SegState carry;
  carry.flag = 0;
  carry.cnt = 0;
  carry.acc = seg_identity(op);
  for (int64_t c = 0; c < nchunks; ++c) {
    const int64_t t0 =
        c * SEG_CARRY_CHUNK + (int64_t)threadIdx.x * SEG_CARRY_PER_THREAD;
    SegState s[SEG_CARRY_PER_THREAD];
#pragma unroll
    for (int k = 0; k < SEG_CARRY_PER_THREAD; ++k) {
      const int64_t T = t0 + k;
      SegState x;
      x.flag = 0;
      x.cnt = 0;
      x.acc = seg_identity(op);
      if (T < nt) {
        x.flag = heads[T] != 0;
        x.cnt = fw[2 * T];
        x.acc = (uint64_t)fw[2 * T + 1];
      }
      s[k] = k == 0 ? x : seg_combine(op, s[k - 1], x);
    }
    SegState total;
    const SegState pre =
        seg_block_scan(op, s[SEG_CARRY_PER_THREAD - 1], carry, wt, &total);
#pragma unroll
    for (int k = 0; k < SEG_CARRY_PER_THREAD; ++k) {
      const int64_t T = t0 + k;
      if (T >= nt) continue;
      // the state at the last row of tile T - 1
      const SegState ex = k == 0 ? pre : seg_combine(op, pre, s[k - 1]);
      per_tile(T, ex);
      fw[2 * T] = ex.cnt;
      fw[2 * T + 1] = (int64_t)ex.acc;
    }
    carry = total;
    carry.flag = 0;
    __syncthreads();  // wt is rewritten by the next chunk
  }
  return carry;
}

}  // namespace srj
#endif  // __HIPCC__
