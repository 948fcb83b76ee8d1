// Window functions that look a fixed number of rows backwards or forwards
// over a sorted order: lag, lead and count/sum/min/max/avg over the bounded
// frame ROWS BETWEEN a PRECEDING AND b FOLLOWING.
//
// Reference parity: the rolling aggregations (grouped_rolling_window) and
// lead/lag the reference's Window exec takes from libcudf - SURVEY.md L0.
//
// A scan (window.hip) does not fit these: min and max have no inverse, float
// sums by prefix difference cancel, and the frames are short. So every output
// row folds its own frame, as cudf's rolling kernel does. Cost is
// O(m * frame width) and there is no cap on the width.
//
// Inputs are those of window.hip - the permutation `perm` that sorts the rows
// and up to SEG_MAX_FUNCS by-value function descriptors - and, per SORTED
// position i, the 1-based row number `rn` within its partition and the
// partition's row count `pcnt` (one srj_window call over the identity
// permutation gives both, once per call of the op). The partition of i is
// the positions [ps, pe] with ps = i - (rn - 1), pe = ps + pcnt - 1. Values
// are read in place as values[perm[j]] and results are written as
// out[perm[i]].
//
//  * BOUNDED AGGREGATE. The frame of i is [max(i + lo, ps), min(i + hi, pe)]
//    and may be empty. The result is the left fold, in ascending position
//    from the empty state, of seg_value_item under seg_combine, stored with
//    seg_store_agg: the state, the operator, the value load and the store of
//    seg_scan.hpp, so null skipping, NaN-greatest min/max, wrapping int64
//    sums, float64 accumulation, the zero under a null and the result dtypes
//    are those of the scan frames. The fold order is fixed by the position
//    alone, so float sums are the same bits on every run and on both paths.
//  * LAG / LEAD. The source of i is j = i + shift; the result is valid if j
//    lies in [ps, pe] and the source row is valid, and is then the source's
//    bits in the input dtype (NaN payloads and -0.0 come through); zero
//    otherwise. Every source is read once, so there is nothing to stage:
//    both kernels read it from global memory.
//  * STAGED PATH (every aggregate of the launch has |lo|, |hi| <=
//    ROLL_MAX_REACH). A workgroup owns ROLL_TILE_ROWS consecutive positions.
//    Per function it first loads the items of the positions its frames can
//    touch, [tile start + lo, tile end + hi] clipped to [0, m), into LDS: the
//    accumulator word and one validity bit per slot. Every perm[j] gather and
//    every value load happens once per tile, not once per frame member;
//    threads then fold out of LDS.
//  * DIRECT PATH (a wider reach). The same fold with every item loaded from
//    global memory.
//  * NO SPINS, NO ATOMICS, NO HOST SYNC: one launch per call of up to
//    SEG_MAX_FUNCS functions, whatever the data; a perm entry outside [0, m) is never
//    dereferenced (the position holds no row: it gets no result and counts as
//    a null source); all index arithmetic is int64 and the offsets are at
//    most ROLL_MAX_OFFSET, so i + hi and i + shift cannot wrap.
//
// MI355X notes: thread t owns positions t, t + 256, ... of its tile, so at
// every step of the fold the lanes of a wave read consecutive 8-byte LDS
// words - a half-wave covers the 64 banks exactly once, no padding - or, where
// a frame is clipped at the partition start, the same word (a broadcast). The
// validity bits of 64 consecutive slots are one __ballot word. perm, rn and
// pcnt are read coalesced.
#include "window_rolling.hpp"

#include <cstdlib>

namespace srj {

static_assert(ROLL_TILE_ROWS == DEFAULT_BLOCK * ROLL_EPT, "tile");
static_assert(ROLL_SLOTS % DEFAULT_BLOCK == 0, "the load loop is uniform");
static_assert(DEFAULT_BLOCK % WAVE == 0 && WAVE == 64, "one mask word a wave");

struct RollFuncs {
  RollFunc f[SEG_MAX_FUNCS];
  int32_t nf;
};

__device__ inline uint64_t roll_load_bits(const SegFunc& f, int64_t row) {
  const int64_t e = row * f.stride;
  switch (f.width) {
    case 1: return static_cast<const uint8_t*>(f.values)[e];
    case 2: return static_cast<const uint16_t*>(f.values)[e];
    case 4: return static_cast<const uint32_t*>(f.values)[e];
    default: return static_cast<const uint64_t*>(f.values)[e];
  }
}

__device__ inline void roll_store_bits(const SegFunc& f, int64_t row,
                                       uint64_t v) {
  switch (f.width) {
    case 1: static_cast<uint8_t*>(f.out)[row] = (uint8_t)v; break;
    case 2: static_cast<uint16_t*>(f.out)[row] = (uint16_t)v; break;
    case 4: static_cast<uint32_t*>(f.out)[row] = (uint32_t)v; break;
    default: static_cast<uint64_t*>(f.out)[row] = v; break;
  }
}

// The item of aggregate f at sorted position j (0 <= j < m).
__device__ inline SegState roll_item(const SegFunc& f, int32_t op,
                                     const int64_t* __restrict__ perm,
                                     int64_t j, int64_t m) {
  const int64_t r = perm[j];
  return seg_value_item(f, op, (r >= 0 && r < m) ? r : -1, false);
}

// The left fold of the items of positions [a, b] (empty if a > b) from the
// empty state. OP is a compile-time constant, so seg_combine's switch folds
// away in the loop; slot j - origin of the stage holds position j.
template <bool STAGED, int32_t OP>
__device__ __forceinline__ SegState roll_fold(
    const SegFunc& f, const int64_t* __restrict__ perm, int64_t m, int64_t a,
    int64_t b, int64_t origin, const uint64_t* s_acc, const uint64_t* s_ok) {
  SegState st;
  st.flag = 0;
  st.cnt = 0;
  st.acc = seg_identity(OP);
  for (int64_t j = a; j <= b; ++j) {
    SegState x;
    if (STAGED) {
      const int s = (int)(j - origin);
      x.flag = 0;
      x.cnt = (int64_t)((s_ok[s / WAVE] >> (s & (WAVE - 1))) & 1u);
      x.acc = s_acc[s];
    } else {
      x = roll_item(f, OP, perm, j, m);
    }
    st = seg_combine(OP, st, x);
  }
  return st;
}

template <bool STAGED>
__device__ __forceinline__ SegState roll_fold_op(
    int32_t op, const SegFunc& f, const int64_t* __restrict__ perm, int64_t m,
    int64_t a, int64_t b, int64_t origin, const uint64_t* s_acc,
    const uint64_t* s_ok) {
  switch (op) {
    case OP_SUM_I:
      return roll_fold<STAGED, OP_SUM_I>(f, perm, m, a, b, origin, s_acc,
                                         s_ok);
    case OP_SUM_F:
      return roll_fold<STAGED, OP_SUM_F>(f, perm, m, a, b, origin, s_acc,
                                         s_ok);
    case OP_MIN_I:
      return roll_fold<STAGED, OP_MIN_I>(f, perm, m, a, b, origin, s_acc,
                                         s_ok);
    case OP_MAX_I:
      return roll_fold<STAGED, OP_MAX_I>(f, perm, m, a, b, origin, s_acc,
                                         s_ok);
    case OP_MIN_F:
      return roll_fold<STAGED, OP_MIN_F>(f, perm, m, a, b, origin, s_acc,
                                         s_ok);
    case OP_MAX_F:
      return roll_fold<STAGED, OP_MAX_F>(f, perm, m, a, b, origin, s_acc,
                                         s_ok);
    default:
      return roll_fold<STAGED, OP_COUNT>(f, perm, m, a, b, origin, s_acc,
                                         s_ok);
  }
}

template <bool STAGED>
__global__ __launch_bounds__(DEFAULT_BLOCK) void window_rolling_kernel(
    RollFuncs fs, const int64_t* __restrict__ perm,
    const int64_t* __restrict__ rn, const int64_t* __restrict__ pcnt,
    int64_t m, int64_t nt) {
  __shared__ uint64_t s_acc[STAGED ? ROLL_SLOTS : 1];      // 16 KiB
  __shared__ uint64_t s_ok[STAGED ? ROLL_SLOTS / WAVE : 1];
  const int tid = threadIdx.x;

  for (int64_t T = blockIdx.x; T < nt; T += gridDim.x) {
    const int64_t base = T * ROLL_TILE_ROWS;

    int64_t row[ROLL_EPT], ps[ROLL_EPT], pe[ROLL_EPT];
#pragma unroll
    for (int k = 0; k < ROLL_EPT; ++k) {
      const int64_t i = base + tid + k * DEFAULT_BLOCK;
      row[k] = -1;
      ps[k] = 0;
      pe[k] = -1;
      if (i < m) {
        const int64_t r = perm[i];
        if (r >= 0 && r < m) row[k] = r;  // never touch memory off the columns
        const int64_t s = i - (rn[i] - 1);
        const int64_t e = s + pcnt[i] - 1;
        ps[k] = s > 0 ? s : 0;  // never a position off perm
        pe[k] = e < m - 1 ? e : m - 1;
      }
    }

    for (int32_t fi = 0; fi < fs.nf; ++fi) {
      const RollFunc& g = fs.f[fi];
      const SegFunc& f = g.f;

      if (f.fn == RF_SHIFT) {
#pragma unroll
        for (int k = 0; k < ROLL_EPT; ++k) {
          if (row[k] < 0) continue;
          const int64_t j = base + tid + k * DEFAULT_BLOCK + g.shift;
          uint64_t v = 0;
          bool ok = false;
          if (j >= ps[k] && j <= pe[k]) {
            const int64_t src = perm[j];
            if (src >= 0 && src < m &&
                (f.valid == nullptr || f.valid[src] != 0)) {
              ok = true;
              v = roll_load_bits(f, src);
            }
          }
          roll_store_bits(f, row[k], v);
          f.out_valid[row[k]] = ok ? 1 : 0;
        }
        continue;
      }

      const int32_t op = seg_op(f);
      // slot s of the stage holds position origin + s
      const int64_t origin = base + g.lo;
      if (STAGED) {
        // hi - lo <= 2 * ROLL_MAX_REACH (checked on the host)
        const int nslots = ROLL_TILE_ROWS + (int)(g.hi - g.lo);
        for (int s = tid; s < nslots; s += DEFAULT_BLOCK) {
          // s of lane 0 is a multiple of 64 and the lowest of its wave: it
          // is active whenever a lane of the wave is, and the ballot leaves
          // zero bits for the slots past nslots
          const int64_t j = origin + s;
          SegState x;
          x.cnt = 0;
          x.acc = seg_identity(op);
          if (j >= 0 && j < m) x = roll_item(f, op, perm, j, m);
          s_acc[s] = x.acc;
          const uint64_t word = __ballot(x.cnt != 0);
          if ((tid & (WAVE - 1)) == 0) s_ok[s / WAVE] = word;
        }
        __syncthreads();
      }

#pragma unroll
      for (int k = 0; k < ROLL_EPT; ++k) {
        if (row[k] < 0) continue;
        const int64_t i = base + tid + k * DEFAULT_BLOCK;
        const int64_t a = i + g.lo > ps[k] ? i + g.lo : ps[k];
        const int64_t b = i + g.hi < pe[k] ? i + g.hi : pe[k];
        // a >= i + lo = origin + (i - base) and b <= i + hi: the slots of
        // [a, b] lie in [0, nslots)
        const SegState st =
            roll_fold_op<STAGED>(op, f, perm, m, a, b, origin, s_acc, s_ok);
        if (f.fn == SF_COUNT) {
          static_cast<int64_t*>(f.out)[row[k]] = st.cnt;
        } else {
          seg_store_agg(f, row[k], st.cnt, st.acc);
        }
      }
      if (STAGED) __syncthreads();  // the stage is rewritten
    }
  }
}

}  // namespace srj

using namespace srj;

extern "C" {

// Whether a launch of these functions takes the staged path: every aggregate
// reaches at most ROLL_MAX_REACH rows either way, there is an aggregate to
// stage, and SRJ_WINDOW_ROLLING_DIRECT (for measuring one path against the
// other) is unset or 0.
int32_t srj_window_rolling_staged(const RollFunc* funcs, int32_t nfuncs) {
  if (const char* env = getenv("SRJ_WINDOW_ROLLING_DIRECT"))
    if (atoi(env) != 0) return 0;
  bool any = false;
  for (int32_t i = 0; i < nfuncs; ++i) {
    if (funcs[i].f.fn == RF_SHIFT) continue;
    any = true;
    if (funcs[i].lo < -ROLL_MAX_REACH || funcs[i].hi > ROLL_MAX_REACH)
      return 0;
  }
  return any;
}

// 1 <= nfuncs <= SEG_MAX_FUNCS, m > 0; rn and pcnt: see the head of the file.
void srj_window_rolling(const RollFunc* funcs, int32_t nfuncs,
                        const int64_t* perm, const int64_t* rn,
                        const int64_t* pcnt, int64_t m, hipStream_t stream) {
  RollFuncs a{};
  a.nf = nfuncs;
  for (int32_t i = 0; i < nfuncs; ++i) a.f[i] = funcs[i];
  const int64_t nt = (m + ROLL_TILE_ROWS - 1) / ROLL_TILE_ROWS;
  const int grid = (int)(nt < MAX_GRID ? nt : MAX_GRID);
  if (srj_window_rolling_staged(funcs, nfuncs)) {
    window_rolling_kernel<true><<<grid, DEFAULT_BLOCK, 0, stream>>>(
        a, perm, rn, pcnt, m, nt);
  } else {
    window_rolling_kernel<false><<<grid, DEFAULT_BLOCK, 0, stream>>>(
        a, perm, rn, pcnt, m, nt);
  }
}

}  // extern "C"
