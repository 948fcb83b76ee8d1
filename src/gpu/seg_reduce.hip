// Segmented reduce over a sorted order: count/sum/min/max/avg per segment,
// one output row per segment - the reduction half of a sort-based group-by.
//
// Reference parity: the sort-based groupby aggregations the reference's
// aggregate exec takes from libcudf (segmented reductions over a sorted
// table) - SURVEY.md L0.
//
// Inputs are the permutation `perm` that sorts the rows by the group keys
// (null: the identity, the rows are grouped already) and one byte flag per
// SORTED position, nonzero where a segment starts. Values are read in place
// as values[perm[i]]; results are written as out[g] with g the number of the
// segment, counted from 0 in sorted order.
//
// How it works:
//  * ONE SCAN PER FUNCTION, the scan of seg_scan.hpp that window.hip runs
//    too (state, operator, block scan, value load, aggregate store and carry
//    scan are shared, not copied): a forward segmented inclusive scan of a
//    (valid count, accumulator) state. The thread that
//    holds the LAST position of a segment has the segment's final state and
//    writes it to out[g]; g is the inclusive count of heads up to the
//    position, minus one, from a plain prefix sum of the head flags. The
//    thread that holds the head writes first_rows[g]; the thread that holds
//    position m - 1 writes the number of segments.
//  * SMALL PATH (m <= SEG_SMALL_ROWS). One workgroup, one launch.
//  * TILED PATH. Three launches: (1) every tile reduces itself and writes,
//    per function, the state of the segment still open at its end, and once
//    its head count (nonzero = "tile holds a head", the segmented operator's
//    flag); (2) one workgroup scans the tile carries in chunks with a running
//    carry (seg_carry_scan, the structure of block_scan_chunked) and
//    turns the head counts into their exclusive sum, the base segment number
//    of every tile; (3) every tile rescans with its carry-in and writes at
//    the segment ends inside it. A segment that runs past a tile is written
//    by the tile where it ends, so no tile looks ahead.
//  * NO SPINS, NO ATOMICS: no kernel waits on another workgroup, the launch
//    count depends on m and the number of functions only, and the combine
//    order is fixed by the position, so float sums are bit-identical run to
//    run.
//
// MI355X notes: wave64 scans by __shfl_up; a thread owns SEG_EPT consecutive
// positions, so perm is read 64 contiguous bytes per lane and the in-register
// part of the scan needs no LDS. Unlike the window kernels no state is looked
// up at another position, so LDS holds the four wave totals only.
#include "seg_scan.hpp"

namespace srj {

static_assert(SEG_EPT <= 32, "head flags of a thread are bits of a word");

// out[g] of function f from the state at the segment's last position.
__device__ inline void seg_store(const SegFunc& f, int64_t g, int64_t cnt,
                                 uint64_t acc) {
  if (f.fn == SF_COUNT) {
    static_cast<int64_t*>(f.out)[g] = cnt;
  } else {
    seg_store_agg(f, g, cnt, acc);
  }
}

// Work layout (int64 words, nt tiles, function f):
//   [0, nt)            heads in the tile, then (launch 2) heads before it
//   nt + f * 2nt + ... (cnt, acc) per tile: its carry, then its carry-in
__host__ __device__ inline int64_t seg_func_words(int64_t nt) {
  return 2 * nt;
}

// EMIT = false: launch 1 of the tiled path (tile carries and head counts).
// EMIT = true: the small path (work == nullptr, one tile) and launch 3.
// nrows: rows of the value columns (perm entries outside [0, nrows) are
// skipped). num_out: rows of the outputs.
template <bool EMIT>
__global__ __launch_bounds__(DEFAULT_BLOCK) void seg_tile_kernel(
    SegFuncs fs, const int64_t* __restrict__ perm,
    const uint8_t* __restrict__ head, int64_t m, int64_t nrows, int64_t nt,
    int64_t num_out, int64_t* __restrict__ first_rows,
    int64_t* __restrict__ count, int64_t* work) {
  __shared__ SegState wt[SEG_WAVES];
  __shared__ int64_t wh[SEG_WAVES];
  const int tid = threadIdx.x;
  const int p0 = tid * SEG_EPT;

  for (int64_t T = blockIdx.x; T < nt; T += gridDim.x) {
    const int64_t base = T * SEG_TILE_ROWS;
    const int32_t nvalid =
        m - base < SEG_TILE_ROWS ? (int32_t)(m - base) : SEG_TILE_ROWS;

    int64_t row[SEG_EPT];
    uint32_t hf = 0;  // bit k: position p0 + k starts a segment
    uint32_t in = 0;  // bit k: position p0 + k is inside the input
#pragma unroll
    for (int k = 0; k < SEG_EPT; ++k) {
      const int64_t i = base + p0 + k;
      row[k] = -1;
      if (p0 + k < nvalid) {
        const int64_t r = perm != nullptr ? perm[i] : i;
        if (r >= 0 && r < nrows) row[k] = r;  // never touch memory off the columns
        const bool h = i == 0 || head[i] != 0;
        hf |= (uint32_t)h << k;
        in |= 1u << k;
      }
    }

    // segment number of every position: heads up to it, minus one
    int64_t tile_heads;
    int64_t seg = block_scan_excl<int64_t>((int64_t)__builtin_popcount(hf), wh,
                                           &tile_heads) - 1;
    if (EMIT) {
      if (work != nullptr) seg += work[T];
    } else if (tid == 0) {
      work[T] = tile_heads;
    }
    __syncthreads();  // wh is rewritten by the next tile

    uint32_t ef = 0;  // bit k: position p0 + k ends a segment
    if (EMIT) {
      // a position ends its segment when the next one is a head or lies
      // past the input; the position after this thread's last is read from
      // memory (it may belong to the next tile)
      const int64_t nx = base + p0 + SEG_EPT;
      const bool nh = nx >= m || head[nx] != 0;
      ef = ((((hf | ~in) >> 1) & ((1u << (SEG_EPT - 1)) - 1u)) |
            ((uint32_t)nh << (SEG_EPT - 1))) & in;
      int64_t g = seg;
#pragma unroll
      for (int k = 0; k < SEG_EPT; ++k) {
        if ((hf >> k) & 1u) {
          ++g;
          if (g < num_out) first_rows[g] = perm != nullptr ? perm[base + p0 + k]
                                                           : base + p0 + k;
        }
        if (base + p0 + k == m - 1 && ((in >> k) & 1u)) count[0] = g + 1;
      }
    }

    for (int32_t fi = 0; fi < fs.nf; ++fi) {
      const SegFunc& f = fs.f[fi];
      const int32_t op = seg_op(f);
      int64_t* fw =
          work != nullptr ? work + nt + fi * seg_func_words(nt) : nullptr;
      SegState carry;
      carry.flag = 0;
      carry.cnt = 0;
      carry.acc = seg_identity(op);
      if (EMIT && fw != nullptr) {
        carry.cnt = fw[2 * T];
        carry.acc = (uint64_t)fw[2 * T + 1];
      }
      SegState s[SEG_EPT];
#pragma unroll
      for (int k = 0; k < SEG_EPT; ++k) {
        const SegState x = seg_value_item(f, op, row[k], (hf >> k) & 1u);
        s[k] = k == 0 ? x : seg_combine(op, s[k - 1], x);
      }
      SegState total;
      const SegState pre = seg_block_scan(op, s[SEG_EPT - 1], carry, wt, &total);
      if (EMIT) {
        int64_t g = seg;
#pragma unroll
        for (int k = 0; k < SEG_EPT; ++k) {
          g += (hf >> k) & 1u;
          if (((ef >> k) & 1u) && g < num_out) {
            const SegState e = seg_combine(op, pre, s[k]);
            seg_store(f, g, e.cnt, e.acc);
          }
        }
      } else if (tid == 0) {
        // positions past the input are identities: the state at the tile's
        // last row
        fw[2 * T] = total.cnt;
        fw[2 * T + 1] = (int64_t)total.acc;
      }
      __syncthreads();  // wt is rewritten by the next function
    }
  }
}

// Launch 2 of the tiled path: one workgroup. See the work layout above.
__global__ __launch_bounds__(DEFAULT_BLOCK) void seg_carry_kernel(
    SegFuncs fs, int64_t nt, int64_t* work) {
  __shared__ SegState wt[SEG_WAVES];
  __shared__ int64_t wh[SEG_WAVES];
  const int64_t* heads = work;

  for (int32_t fi = 0; fi < fs.nf; ++fi) {
    int64_t* fw = work + nt + fi * seg_func_words(nt);
    seg_carry_scan(seg_op(fs.f[fi]), heads, fw, nt, wt,
                   [](int64_t, const SegState&) {});
  }
  // last, the head counts become the base segment number of every tile (the
  // scans above read them as flags)
  block_scan_chunked<int64_t>(heads, work, nt, wh);
}

inline int64_t seg_ntiles(int64_t m) {
  return (m + SEG_TILE_ROWS - 1) / SEG_TILE_ROWS;
}

}  // namespace srj

using namespace srj;

extern "C" {

// bytes of scratch one srj_seg_reduce call of nfuncs functions needs
int64_t srj_seg_reduce_work_bytes(int64_t m, int32_t nfuncs) {
  if (m <= SEG_SMALL_ROWS) return 0;
  const int64_t nt = seg_ntiles(m);
  return 8 * (nt + (int64_t)nfuncs * seg_func_words(nt));
}

// 0 <= nfuncs <= SEG_MAX_FUNCS, m > 0, perm may be null (identity). nrows:
// rows of the value and validity columns. first_rows and every out hold
// num_out rows, count one. work: srj_seg_reduce_work_bytes(m, nfuncs) bytes,
// 8-byte aligned.
void srj_seg_reduce(const SegFunc* funcs, int32_t nfuncs, const int64_t* perm,
                    const uint8_t* head, int64_t m, int64_t nrows,
                    int64_t num_out, int64_t* first_rows, int64_t* count,
                    int64_t* work, hipStream_t stream) {
  SegFuncs a{};
  a.nf = nfuncs;
  for (int32_t i = 0; i < nfuncs; ++i) a.f[i] = funcs[i];
  if (m <= SEG_SMALL_ROWS) {
    seg_tile_kernel<true><<<1, DEFAULT_BLOCK, 0, stream>>>(
        a, perm, head, m, nrows, 1, num_out, first_rows, count, nullptr);
    return;
  }
  const int64_t nt = seg_ntiles(m);
  const int grid = (int)(nt < MAX_GRID ? nt : MAX_GRID);
  seg_tile_kernel<false><<<grid, DEFAULT_BLOCK, 0, stream>>>(
      a, perm, head, m, nrows, nt, num_out, first_rows, count, work);
  seg_carry_kernel<<<1, DEFAULT_BLOCK, 0, stream>>>(a, nt, work);
  seg_tile_kernel<true><<<grid, DEFAULT_BLOCK, 0, stream>>>(
      a, perm, head, m, nrows, nt, num_out, first_rows, count, work);
}

}  // extern "C"
