// Stream compaction: stable nonzero (boolean-mask selection), fused
// multi-column compaction by mask, and fused multi-column gather by index.
//
// Reference parity: libcudf apply_boolean_mask / copy_if / multi-column
// gather, the primitives every Filter, Join, Sort and semi-join of the
// reference funnels through.
//
// Design requirements (not tuning choices):
//  * STABLE ORDER. Kept rows come out in input order; Spark filter semantics
//    and the sort/limit determinism tests rely on it. Selection is therefore
//    two-pass (count per tile, scan the tile counts, scatter by rank) and
//    uses no atomics anywhere.
//  * NO SPINS. The tile scan is ONE workgroup walking the tile counts in
//    chunks with a running carry. There is no decoupled look-back, no
//    inter-workgroup flag and no wait on another workgroup: a kernel here
//    never depends on which other workgroups are resident.
//
// MI355X design notes:
//  * one workgroup of 256 threads per tile of COMPACT_TILE rows, grid capped
//    at MAX_GRID and grid-strided over tiles (srj_common.hpp ground rules).
//  * mask/valid are byte-per-row and are read one byte per lane, so a pointer
//    of any byte alignment (a slice of a larger buffer) needs no head/tail
//    handling; a wave still reads 64 consecutive bytes per load.
//  * rank within a wave is popcount(ballot & lanes_below) — no shuffles; the
//    4 waves x ROUNDS wave counts of a tile meet once in LDS (one barrier).
//  * column descriptors travel by value in the kernel-argument struct, so a
//    launch needs no descriptor H2D copy. The column kernel first writes the
//    tile's kept rows as a dense list in LDS (4 KiB) and copies from that
//    list: only kept rows are ever loaded, so at low selectivity only the
//    touched lines are fetched, a wave's lanes are all busy and its stores
//    contiguous at any selectivity, and no index array goes to memory.
#include "srj_common.hpp"

namespace srj {

constexpr int COMPACT_TILE = 2048;                        // rows per tile
constexpr int COMPACT_ROUNDS = COMPACT_TILE / DEFAULT_BLOCK;  // 8
constexpr int COMPACT_WAVES = DEFAULT_BLOCK / WAVE;       // 4
constexpr int COMPACT_MAX_COLS = 16;

static_assert(COMPACT_TILE % DEFAULT_BLOCK == 0, "tile is whole rounds");
static_assert(COMPACT_TILE <= 65536, "tile-local rows are uint16");

struct CompactCol {
  const void* src;
  void* dst;
  int32_t width;  // bytes per row: 1, 2, 4, 8 or 16
  int32_t pad_;
};

struct CompactCols {
  CompactCol c[COMPACT_MAX_COLS];
  int32_t ncols;
};

// 16-byte rows (DECIMAL128 pairs, complex128) are only 8-byte aligned
struct alignas(8) Bytes16 {
  uint64_t lo, hi;
};

__device__ inline bool keep_row(const uint8_t* __restrict__ mask,
                                const uint8_t* __restrict__ valid, int64_t i,
                                int64_t n) {
  if (i >= n) return false;
  bool k = mask[i] != 0;
  if (valid != nullptr) k = k && valid[i] != 0;
  return k;
}

__device__ inline uint64_t lanes_below() {
  return (1ull << (threadIdx.x & (WAVE - 1))) - 1ull;
}

// ---------------------------------------------------------------------------
// pass 1: kept rows per tile
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(DEFAULT_BLOCK) void compact_count_kernel(
    const uint8_t* __restrict__ mask, const uint8_t* __restrict__ valid,
    int64_t n, int64_t ntiles, int32_t* __restrict__ counts) {
  __shared__ int32_t wcount[COMPACT_WAVES];
  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * COMPACT_TILE;
    int32_t cnt = 0;  // wave-uniform
#pragma unroll
    for (int r = 0; r < COMPACT_ROUNDS; ++r) {
      bool keep = keep_row(mask, valid, base + r * DEFAULT_BLOCK + tid, n);
      cnt += __popcll(__ballot(keep));
    }
    if ((tid & (WAVE - 1)) == 0) wcount[wave] = cnt;
    __syncthreads();
    if (tid == 0) {
      int32_t s = 0;
#pragma unroll
      for (int w = 0; w < COMPACT_WAVES; ++w) s += wcount[w];
      counts[tile] = s;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// pass 2: exclusive scan of the tile counts. ONE workgroup, chunked with a
// running carry (see the no-spin requirement above).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(DEFAULT_BLOCK) void compact_scan_kernel(
    const int32_t* __restrict__ counts, int64_t ntiles,
    int64_t* __restrict__ offsets, int64_t* __restrict__ total) {
  __shared__ int64_t wtotal[COMPACT_WAVES];
  const int64_t kept = block_scan_chunked(counts, offsets, ntiles, wtotal);
  if (threadIdx.x == 0) *total = kept;
}

// ---------------------------------------------------------------------------
// pass 3 helper: keep bits and tile-local output ranks of this thread's
// ROUNDS rows of one tile. All 256 threads must call it (ballot + barriers).
// Returns the keep bits (bit r = round r); rank[r] is valid where bit r is
// set; *tile_count is the number of kept rows of the tile.
// ---------------------------------------------------------------------------
__device__ inline uint32_t tile_ranks(const uint8_t* __restrict__ mask,
                                      const uint8_t* __restrict__ valid,
                                      int64_t n, int64_t base,
                                      int32_t (*wcount)[COMPACT_WAVES],
                                      int32_t rank[COMPACT_ROUNDS],
                                      int32_t* tile_count) {
  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const uint64_t below = lanes_below();
  uint32_t keepbits = 0;
#pragma unroll
  for (int r = 0; r < COMPACT_ROUNDS; ++r) {
    bool keep = keep_row(mask, valid, base + r * DEFAULT_BLOCK + tid, n);
    uint64_t b = __ballot(keep);
    rank[r] = __popcll(b & below);
    keepbits |= (uint32_t)keep << r;
    if ((tid & (WAVE - 1)) == 0) wcount[r][wave] = __popcll(b);
  }
  __syncthreads();
  // rows of a tile are ordered (round, wave, lane)
  int32_t running = 0;
#pragma unroll
  for (int r = 0; r < COMPACT_ROUNDS; ++r) {
    int32_t before = running;
#pragma unroll
    for (int w = 0; w < COMPACT_WAVES; ++w) {
      int32_t c = wcount[r][w];
      if (w < wave) before += c;
      running += c;
    }
    rank[r] += before;
  }
  *tile_count = running;
  __syncthreads();  // wcount is rewritten by the next tile
  return keepbits;
}

__global__ __launch_bounds__(DEFAULT_BLOCK) void compact_nonzero_kernel(
    const uint8_t* __restrict__ mask, const uint8_t* __restrict__ valid,
    int64_t n, int64_t ntiles, const int64_t* __restrict__ offsets,
    int64_t* __restrict__ out) {
  __shared__ int32_t wcount[COMPACT_ROUNDS][COMPACT_WAVES];
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * COMPACT_TILE;
    int32_t rank[COMPACT_ROUNDS];
    int32_t cnt;
    uint32_t keepbits = tile_ranks(mask, valid, n, base, wcount, rank, &cnt);
    int64_t* __restrict__ o = out + offsets[tile];
#pragma unroll
    for (int r = 0; r < COMPACT_ROUNDS; ++r) {
      if ((keepbits >> r) & 1u)
        o[rank[r]] = base + r * DEFAULT_BLOCK + (int64_t)threadIdx.x;
    }
  }
}

// Copy the kept rows of one tile for one column. `row` holds this thread's
// share of the tile's dense kept-row list (entry r*256+tid), so the lanes of
// a wave are all busy and the stores are contiguous at any selectivity.
template <typename T>
__device__ inline void compact_copy(const void* __restrict__ src,
                                    void* __restrict__ dst, int64_t base,
                                    int64_t tile_offset, int32_t cnt,
                                    const int32_t row[COMPACT_ROUNDS]) {
  const T* __restrict__ s = static_cast<const T*>(src) + base;
  T* __restrict__ d = static_cast<T*>(dst) + tile_offset;
#pragma unroll
  for (int r = 0; r < COMPACT_ROUNDS; ++r) {
    int32_t j = r * DEFAULT_BLOCK + (int32_t)threadIdx.x;
    if (j < cnt) d[j] = s[row[r]];
  }
}

__global__ __launch_bounds__(DEFAULT_BLOCK) void compact_cols_kernel(
    const uint8_t* __restrict__ mask, const uint8_t* __restrict__ valid,
    int64_t n, int64_t ntiles, const int64_t* __restrict__ offsets,
    CompactCols cols) {
  __shared__ int32_t wcount[COMPACT_ROUNDS][COMPACT_WAVES];
  __shared__ uint16_t kept[COMPACT_TILE];  // tile-local rows, in order
  const int tid = threadIdx.x;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t base = tile * COMPACT_TILE;
    int32_t rank[COMPACT_ROUNDS];
    int32_t cnt;
    // the barriers inside tile_ranks also order the previous tile's reads
    // of kept[] before the writes below
    uint32_t keepbits = tile_ranks(mask, valid, n, base, wcount, rank, &cnt);
    if (cnt == 0) continue;  // block-uniform
#pragma unroll
    for (int r = 0; r < COMPACT_ROUNDS; ++r) {
      if ((keepbits >> r) & 1u)
        kept[rank[r]] = (uint16_t)(r * DEFAULT_BLOCK + tid);
    }
    __syncthreads();
    int32_t row[COMPACT_ROUNDS];
#pragma unroll
    for (int r = 0; r < COMPACT_ROUNDS; ++r) {
      int32_t j = r * DEFAULT_BLOCK + tid;
      row[r] = j < cnt ? kept[j] : 0;
    }
    const int64_t off = offsets[tile];
    for (int c = 0; c < cols.ncols; ++c) {
      const void* src = cols.c[c].src;
      void* dst = cols.c[c].dst;
      switch (cols.c[c].width) {
        case 1: compact_copy<uint8_t>(src, dst, base, off, cnt, row); break;
        case 2: compact_copy<uint16_t>(src, dst, base, off, cnt, row); break;
        case 4: compact_copy<uint32_t>(src, dst, base, off, cnt, row); break;
        case 8: compact_copy<uint64_t>(src, dst, base, off, cnt, row); break;
        case 16: compact_copy<Bytes16>(src, dst, base, off, cnt, row); break;
        default: break;  // widths are validated on the host
      }
    }
  }
}

// ---------------------------------------------------------------------------
// fused multi-column gather: out[j] = src[idx[j]] for every descriptor.
// An entry outside [0, src_rows) is never dereferenced; its output is zero.
// ---------------------------------------------------------------------------
template <typename T>
__device__ inline void gather_one(const void* __restrict__ src,
                                  void* __restrict__ dst, int64_t j,
                                  int64_t idx, bool ok) {
  T v = T{};
  if (ok) v = static_cast<const T*>(src)[idx];
  static_cast<T*>(dst)[j] = v;
}

__global__ __launch_bounds__(DEFAULT_BLOCK) void gather_cols_kernel(
    const int64_t* __restrict__ map, int64_t m, int64_t src_rows,
    CompactCols cols) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < m;
       j += stride) {
    const int64_t idx = map[j];
    const bool ok = idx >= 0 && idx < src_rows;
    for (int c = 0; c < cols.ncols; ++c) {
      const void* src = cols.c[c].src;
      void* dst = cols.c[c].dst;
      switch (cols.c[c].width) {
        case 1: gather_one<uint8_t>(src, dst, j, idx, ok); break;
        case 2: gather_one<uint16_t>(src, dst, j, idx, ok); break;
        case 4: gather_one<uint32_t>(src, dst, j, idx, ok); break;
        case 8: gather_one<uint64_t>(src, dst, j, idx, ok); break;
        case 16:  // two words: a zero-initialised struct temporary would
                  // be promoted to LDS
          gather_one<uint64_t>(src, dst, 2 * j, 2 * idx, ok);
          gather_one<uint64_t>(src, dst, 2 * j + 1, 2 * idx + 1, ok);
          break;
        default: break;
      }
    }
  }
}

inline int64_t compact_ntiles(int64_t n) {
  return (n + COMPACT_TILE - 1) / COMPACT_TILE;
}

inline int compact_grid(int64_t ntiles) {
  return (int)(ntiles < MAX_GRID ? (ntiles > 0 ? ntiles : 1) : MAX_GRID);
}

}  // namespace srj

using namespace srj;

extern "C" {

int32_t srj_compact_tile_rows() { return COMPACT_TILE; }
int32_t srj_compact_max_grid() { return (int32_t)MAX_GRID; }
int32_t srj_compact_scan_chunk() { return BLOCK_SCAN_CHUNK; }
int32_t srj_compact_max_cols() { return COMPACT_MAX_COLS; }

// count + scan: counts[ntiles] (int32 scratch), offsets[ntiles] exclusive
// int64 tile offsets, *total = number of kept rows. n > 0.
void srj_compact_offsets(const uint8_t* mask, const uint8_t* valid, int64_t n,
                         int32_t* counts, int64_t* offsets, int64_t* total,
                         hipStream_t stream) {
  int64_t ntiles = compact_ntiles(n);
  compact_count_kernel<<<compact_grid(ntiles), DEFAULT_BLOCK, 0, stream>>>(
      mask, valid, n, ntiles, counts);
  compact_scan_kernel<<<1, DEFAULT_BLOCK, 0, stream>>>(counts, ntiles, offsets,
                                                       total);
}

// out must hold *total int64 entries
void srj_compact_nonzero(const uint8_t* mask, const uint8_t* valid, int64_t n,
                         const int64_t* offsets, int64_t* out,
                         hipStream_t stream) {
  int64_t ntiles = compact_ntiles(n);
  compact_nonzero_kernel<<<compact_grid(ntiles), DEFAULT_BLOCK, 0, stream>>>(
      mask, valid, n, ntiles, offsets, out);
}

// every dsts[c] must hold *total rows of widths[c] bytes; ncols <= MAX_COLS
void srj_compact_cols(const uint8_t* mask, const uint8_t* valid, int64_t n,
                      const int64_t* offsets, const void* const* srcs,
                      void* const* dsts, const int32_t* widths, int32_t ncols,
                      hipStream_t stream) {
  CompactCols cols{};
  cols.ncols = ncols;
  for (int32_t c = 0; c < ncols; ++c) cols.c[c] = {srcs[c], dsts[c], widths[c], 0};
  int64_t ntiles = compact_ntiles(n);
  compact_cols_kernel<<<compact_grid(ntiles), DEFAULT_BLOCK, 0, stream>>>(
      mask, valid, n, ntiles, offsets, cols);
}

void srj_gather_cols(const int64_t* map, int64_t m, int64_t src_rows,
                     const void* const* srcs, void* const* dsts,
                     const int32_t* widths, int32_t ncols, hipStream_t stream) {
  CompactCols cols{};
  cols.ncols = ncols;
  for (int32_t c = 0; c < ncols; ++c) cols.c[c] = {srcs[c], dsts[c], widths[c], 0};
  gather_cols_kernel<<<grid_1d(m), DEFAULT_BLOCK, 0, stream>>>(map, m, src_rows,
                                                              cols);
}

}  // extern "C"
