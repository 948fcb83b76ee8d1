// Stable multi-column, null-aware sort order (cudf sorted_order) as a
// packed-key LSD radix sort, plus "key changed from the previous sorted row"
// flags.
//
// Reference parity: libcudf sorted_order / sort_by_key and the group/peer
// boundary detection the reference's Sort and Window execs take from it
// (SURVEY.md L0).
//
// How it works:
//  * KEY PACKER. Every key column contributes a value field whose unsigned
//    order is the wanted order (sign-flipped ints, order-preserving float
//    bits with NaN and zero canonicalised, inverted when descending) and,
//    when it has validity, a 1-bit null field just above it. The host lays
//    the fields out least-significant key first into 64-bit words; one sort
//    of a word is ceil(used_bits / 8) radix passes, not 8 per column.
//    Field descriptors travel by value in the kernel-argument struct.
//  * SMALL PATH (n <= SORT_TILE). One workgroup packs the word and runs all
//    its passes in LDS (keys + 32-bit row index, double-buffered), then
//    writes the int64 permutation once. A pass whose digit is the same for
//    every row is skipped. A pass ranks the whole tile at once from 16-bit
//    (round, wave, digit) counts: seven barriers, not three per round.
//  * LARGE PATH. Per word, least significant first: pack through the running
//    permutation, then per pass histogram (srj_radix_hist) -> per-digit row
//    scan -> scatter. The scatter adds the 256 digit totals up in LDS.
//  * NO SPINS (the requirement compact.hip states): the scan is one
//    workgroup per digit walking its row of block counts with a running
//    carry. No kernel waits on another workgroup; no global atomics.
//
// MI355X notes: wave64 multi-split by 8 ballots (digit_peers). The tile
// counts are written by one lane per distinct digit per wave and scanned by
// one thread per digit, lanes on consecutive digits (conflict-free), with no
// LDS atomics, so tie-heavy keys do not serialise on one counter. Key and
// index reads from LDS are lane-contiguous; the rank-ordered writes are
// data-dependent by nature.
#include "srj_common.hpp"
#include "sort_order.hpp"

namespace srj {

constexpr int SORT_RADIX_BITS = 8;
constexpr int SORT_RADIX = 256;
constexpr int SORT_EPT = 8;
constexpr int SORT_TILE = DEFAULT_BLOCK * SORT_EPT;  // 2048
constexpr int SORT_WAVES = DEFAULT_BLOCK / WAVE;     // 4
constexpr int SORT_MAX_KEYS = 16;

static_assert(SORT_RADIX == DEFAULT_BLOCK, "one thread per digit");

struct SortKeys {
  SortKey k[SORT_MAX_KEYS];
  int32_t nkeys;
};

__device__ inline uint64_t load_uint(const void* p, int64_t e, int32_t width) {
  switch (width) {
    case 1: return static_cast<const uint8_t*>(p)[e];
    case 2: return static_cast<const uint16_t*>(p)[e];
    case 4: return static_cast<const uint32_t*>(p)[e];
    default: return static_cast<const uint64_t*>(p)[e];
  }
}

// The field of one key for one row, unshifted. Equality of fields is the
// sort's equality: nulls equal each other, all NaNs are equal, -0.0 == 0.0.
__device__ inline uint64_t encode_field(const SortKey& k, int64_t row) {
  const bool valid = k.valid == nullptr || k.valid[row] != 0;
  const uint64_t nullbit = (valid == ((k.flags & SF_NULLS_FIRST) != 0)) ? 1 : 0;
  if (k.kind == SK_NULL) return nullbit;
  const uint64_t mask = k.bits >= 64 ? ~0ull : ((1ull << k.bits) - 1ull);
  uint64_t v = 0;
  if (valid) {
    const int64_t e = row * k.stride;
    switch (k.kind) {
      case SK_UINT:
        v = load_uint(k.data, e, k.width);
        break;
      case SK_SINT:
        v = load_uint(k.data, e, k.width) ^ (1ull << (8 * k.width - 1));
        break;
      case SK_BOOL:
        v = static_cast<const uint8_t*>(k.data)[e] != 0;
        break;
      case SK_F32: {
        uint32_t b =
            (uint32_t)norm_float_bits(static_cast<const float*>(k.data)[e]);
        v = (b & 0x80000000u) ? (uint32_t)~b : (b ^ 0x80000000u);
        break;
      }
      case SK_F64: {
        uint64_t b =
            (uint64_t)norm_double_bits(static_cast<const double*>(k.data)[e]);
        v = (b >> 63) ? ~b : (b ^ 0x8000000000000000ull);
        break;
      }
      default: break;
    }
    v &= mask;
    if (k.flags & SF_DESC) v = ~v & mask;
  }
  // bits < 64 whenever SF_NULL_BIT is set (checked on the host)
  if (k.flags & SF_NULL_BIT) v |= nullbit << k.bits;
  return v;
}

__device__ inline uint64_t pack_row(const SortKeys& keys, int64_t row) {
  uint64_t w = 0;
  for (int c = 0; c < keys.nkeys; ++c)
    w |= encode_field(keys.k[c], row) << keys.k[c].shift;
  return w;
}

// out[i] (|)= packed word of row perm[i] (row i without perm)
__global__ __launch_bounds__(DEFAULT_BLOCK) void sort_pack_kernel(
    SortKeys keys, const int64_t* __restrict__ perm, int64_t n,
    int32_t accumulate, uint64_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    int64_t row = perm ? perm[i] : i;
    if (row < 0 || row >= n) row = 0;  // never read outside the columns
    uint64_t w = pack_row(keys, row);
    if (accumulate) w |= out[i];
    out[i] = w;
  }
}

// out[i] = i == 0 || fields of perm[i] and perm[i-1] differ (|= if accumulate)
__global__ __launch_bounds__(DEFAULT_BLOCK) void key_change_kernel(
    SortKeys keys, const int64_t* __restrict__ perm, int64_t n, int64_t nrows,
    int32_t accumulate, uint8_t* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    bool change = i == 0;
    if (i > 0) {
      int64_t a = perm[i], b = perm[i - 1];
      if (a < 0 || a >= nrows) a = 0;  // never read outside the columns
      if (b < 0 || b >= nrows) b = 0;
      for (int c = 0; c < keys.nkeys; ++c)
        change |= encode_field(keys.k[c], a) != encode_field(keys.k[c], b);
    }
    if (accumulate) change |= out[i] != 0;
    out[i] = change ? 1 : 0;
  }
}

// Equality mask of digit d over the active lanes of the wave: 8 ballots
// (no __match_any on CDNA).
__device__ inline uint64_t digit_peers(uint32_t d, bool act) {
  uint64_t eq = __ballot(act);
#pragma unroll
  for (int bit = 0; bit < SORT_RADIX_BITS; ++bit) {
    uint64_t bal = __ballot((d >> bit) & 1);
    eq &= ((d >> bit) & 1) ? bal : ~bal;
  }
  return eq;
}

// Digit counts of one tile per (round, wave): 16 KiB. A wave-round holds at
// most 64 rows and a tile 2048, so 16 bits do.
typedef uint16_t TileCounts[SORT_WAVES][SORT_RADIX];

// Stable rank of each of this thread's rows among the tile's rows that share
// its digit; rows of a tile are ordered (round, wave, lane). d[r] is the digit
// of the row in slot r * 256 + tid, bit r of actbits says the slot holds a
// row, `rounds` (block-uniform) is the number of rounds that hold any. All
// 256 threads call it. On return rank[r] is set for the thread's rows and
// *digit_count is the number of rows whose digit is threadIdx.x. Three
// barriers for the whole tile; the caller adds one before cnt is reused.
__device__ inline void tile_digit_ranks(const uint32_t d[SORT_EPT],
                                        uint32_t actbits, int rounds,
                                        TileCounts* cnt,
                                        int32_t rank[SORT_EPT],
                                        int32_t* digit_count) {
  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const uint64_t below = (1ull << (tid & (WAVE - 1))) - 1ull;
  uint32_t* z = reinterpret_cast<uint32_t*>(cnt);
  const int nz = rounds * SORT_WAVES * SORT_RADIX / 2;
  for (int i = tid; i < nz; i += DEFAULT_BLOCK) z[i] = 0;
  __syncthreads();
  // wave multi-split: the first lane of each digit writes the wave's count
#pragma unroll
  for (int r = 0; r < SORT_EPT; ++r) {
    if (r < rounds) {  // block-uniform
      const bool act = (actbits >> r) & 1u;
      const uint64_t eq = digit_peers(d[r], act);
      rank[r] = __popcll(eq & below);
      if (act && rank[r] == 0) cnt[r][wave][d[r]] = (uint16_t)__popcll(eq);
    }
  }
  __syncthreads();
  // thread = digit: exclusive prefix of its counts along (round, wave)
  int32_t run = 0;
  for (int r = 0; r < rounds; ++r) {
#pragma unroll
    for (int w = 0; w < SORT_WAVES; ++w) {
      int32_t c = cnt[r][w][tid];
      cnt[r][w][tid] = (uint16_t)run;
      run += c;
    }
  }
  *digit_count = run;
  __syncthreads();
#pragma unroll
  for (int r = 0; r < SORT_EPT; ++r) {
    if (r < rounds && ((actbits >> r) & 1u)) rank[r] += cnt[r][wave][d[r]];
  }
}

// ---------------------------------------------------------------------------
// small path: one workgroup, n <= SORT_TILE. Rows sit in LDS in (round,
// thread) order: slot r * 256 + tid. `words` (already packed through
// in_perm) replaces the fused packing when a word has more fields than one
// descriptor struct holds. in_perm may alias out: every input is in LDS
// before the first output is written. The tile counts of a pass live in the
// key buffer the pass is about to fill, so LDS stays at 48 KiB + 1 KiB.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(DEFAULT_BLOCK) void sort_small_kernel(
    SortKeys keys, const uint64_t* __restrict__ words,
    const int64_t* in_perm, int32_t n, int32_t passes, int64_t* out) {
  __shared__ uint64_t skey[2][SORT_TILE];          // 32 KiB
  __shared__ uint32_t sidx[2][SORT_TILE];          // 16 KiB
  __shared__ int32_t digit_base[SORT_RADIX];       // exclusive digit offsets
  __shared__ int32_t wave_tot[SORT_WAVES];
  static_assert(sizeof(TileCounts) * SORT_EPT <= sizeof(skey[0]),
                "tile counts fit the idle key buffer");
  const int tid = threadIdx.x;
  const int rounds = (n + DEFAULT_BLOCK - 1) / DEFAULT_BLOCK;

  uint32_t actbits = 0;
#pragma unroll
  for (int r = 0; r < SORT_EPT; ++r) {
    int i = r * DEFAULT_BLOCK + tid;
    if (i < n) {
      actbits |= 1u << r;
      int64_t row = in_perm ? in_perm[i] : i;
      if (row < 0 || row >= n) row = 0;
      skey[0][i] = words ? words[i] : pack_row(keys, row);
      sidx[0][i] = (uint32_t)row;
    }
  }
  __syncthreads();

  int cur = 0;
  for (int p = 0; p < passes; ++p) {
    const int shift = p * SORT_RADIX_BITS;
    uint64_t k[SORT_EPT];
    uint32_t d[SORT_EPT];
    int32_t rank[SORT_EPT];
#pragma unroll
    for (int r = 0; r < SORT_EPT; ++r) {
      k[r] = ((actbits >> r) & 1u) ? skey[cur][r * DEFAULT_BLOCK + tid] : 0;
      d[r] = (uint32_t)((k[r] >> shift) & 0xff);
    }
    int32_t count;
    tile_digit_ranks(d, actbits, rounds,
                     reinterpret_cast<TileCounts*>(skey[cur ^ 1]), rank,
                     &count);
    // every row has the same digit: the order stays. The barrier also ends
    // the reads of the tile counts before skey[cur ^ 1] is written.
    if (__syncthreads_or(count == n)) continue;
    digit_base[tid] = block_scan_excl<int32_t>(count, wave_tot);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SORT_EPT; ++r) {
      if ((actbits >> r) & 1u) {
        int32_t dst = digit_base[d[r]] + rank[r];
        skey[cur ^ 1][dst] = k[r];
        sidx[cur ^ 1][dst] = sidx[cur][r * DEFAULT_BLOCK + tid];
      }
    }
    __syncthreads();
    cur ^= 1;
  }
#pragma unroll
  for (int r = 0; r < SORT_EPT; ++r) {
    int i = r * DEFAULT_BLOCK + tid;
    if (i < n) out[i] = (int64_t)sidx[cur][i];
  }
}

// ---------------------------------------------------------------------------
// large path, histogram: digit counts of every tile by LDS atomics.
// ---------------------------------------------------------------------------
__global__ void radix_hist_kernel(const uint64_t* __restrict__ keys, int64_t n,
                                  int32_t shift, int64_t nblocks,
                                  int64_t* __restrict__ hist) {
  __shared__ int lhist[SORT_RADIX];
  for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
    for (int i = threadIdx.x; i < SORT_RADIX; i += blockDim.x) lhist[i] = 0;
    __syncthreads();
    int64_t base = b * SORT_TILE;
    for (int r = 0; r < SORT_EPT; ++r) {
      int64_t e = base + r * (int64_t)blockDim.x + threadIdx.x;
      if (e < n) {
        uint32_t d = (uint32_t)((keys[e] >> shift) & (SORT_RADIX - 1));
        atomicAdd(lhist + d, 1);
      }
    }
    __syncthreads();
    // layout: hist[digit * nblocks + block], one row of block counts per digit
    for (int i = threadIdx.x; i < SORT_RADIX; i += blockDim.x) {
      hist[(int64_t)i * nblocks + b] = lhist[i];
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// large path, between histogram and scatter: workgroup d turns row d of the
// digit-major hist[256][nblocks] into exclusive offsets within the digit, in
// place, and writes the digit's total. Chunked with a running carry.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(DEFAULT_BLOCK) void sort_scan_rows_kernel(
    int64_t* __restrict__ hist, int64_t nblocks, int64_t* __restrict__ totals) {
  __shared__ int64_t wtotal[SORT_WAVES];
  for (int d = blockIdx.x; d < SORT_RADIX; d += gridDim.x) {
    int64_t* row = hist + (int64_t)d * nblocks;
    const int64_t total = block_scan_chunked(row, row, nblocks, wtotal);
    if (threadIdx.x == 0) totals[d] = total;
  }
}

// Large path, scatter: the per-(digit, block) offsets are relative to the
// digit, and every block adds the 256 digit totals up in LDS first. The
// payload is the running permutation (identity when null).
__global__ __launch_bounds__(DEFAULT_BLOCK) void sort_scatter_kernel(
    const uint64_t* __restrict__ keys, const int64_t* __restrict__ payload,
    int64_t n, int32_t shift, int64_t nblocks,
    const int64_t* __restrict__ offsets, const int64_t* __restrict__ totals,
    uint64_t* __restrict__ out_keys, int64_t* __restrict__ out_payload) {
  __shared__ TileCounts cnt[SORT_EPT];  // 16 KiB
  __shared__ int64_t digit_start[SORT_RADIX];
  __shared__ int64_t base_off[SORT_RADIX];
  __shared__ int64_t wtotal[SORT_WAVES];
  const int tid = threadIdx.x;
  digit_start[tid] = block_scan_excl<int64_t>(totals[tid], wtotal);
  for (int64_t b = blockIdx.x; b < nblocks; b += gridDim.x) {
    base_off[tid] = digit_start[tid] + offsets[(int64_t)tid * nblocks + b];
    const int64_t base = b * SORT_TILE;
    const int64_t left = n - base;
    const int rounds = left >= SORT_TILE
                           ? SORT_EPT
                           : (int)((left + DEFAULT_BLOCK - 1) / DEFAULT_BLOCK);
    uint64_t k[SORT_EPT];
    int64_t pl[SORT_EPT];
    uint32_t d[SORT_EPT];
    int32_t rank[SORT_EPT];
    uint32_t actbits = 0;
#pragma unroll
    for (int r = 0; r < SORT_EPT; ++r) {
      const int64_t e = base + r * DEFAULT_BLOCK + tid;
      const bool act = e < n;
      actbits |= (uint32_t)act << r;
      k[r] = act ? keys[e] : 0;
      pl[r] = (act && payload) ? payload[e] : e;
      d[r] = (uint32_t)((k[r] >> shift) & 0xff);
    }
    int32_t count;
    // its barriers also publish base_off
    tile_digit_ranks(d, actbits, rounds, cnt, rank, &count);
#pragma unroll
    for (int r = 0; r < SORT_EPT; ++r) {
      if ((actbits >> r) & 1u) {
        const int64_t dst = base_off[d[r]] + rank[r];
        if (dst >= 0 && dst < n) {  // a corrupt histogram must not write out
          out_keys[dst] = k[r];
          out_payload[dst] = pl[r];
        }
      }
    }
    __syncthreads();  // base_off and cnt are rewritten by the next block
  }
}

inline int64_t sort_nblocks(int64_t n) {
  return (n + SORT_TILE - 1) / SORT_TILE;
}

}  // namespace srj

using namespace srj;

extern "C" {

// int64 words of scratch one srj_sort_order call needs
int64_t srj_sort_order_work_words(int64_t n) {
  if (n <= SORT_TILE) return n;
  return 3 * n + SORT_RADIX * sort_nblocks(n) + SORT_RADIX;
}

void srj_sort_pack(const SortKey* keys, int32_t nkeys, const int64_t* perm,
                   int64_t n, int32_t accumulate, uint64_t* out,
                   hipStream_t stream) {
  for (int32_t lo = 0; lo < nkeys; lo += SORT_MAX_KEYS) {
    SortKeys a{};
    a.nkeys = nkeys - lo < SORT_MAX_KEYS ? nkeys - lo : SORT_MAX_KEYS;
    for (int32_t c = 0; c < a.nkeys; ++c) a.k[c] = keys[lo + c];
    sort_pack_kernel<<<grid_1d(n), DEFAULT_BLOCK, 0, stream>>>(
        a, perm, n, (accumulate || lo > 0) ? 1 : 0, out);
  }
}

void srj_key_change_flags(const SortKey* keys, int32_t nkeys,
                          const int64_t* perm, int64_t n, int64_t nrows,
                          uint8_t* out, hipStream_t stream) {
  for (int32_t lo = 0; lo == 0 || lo < nkeys; lo += SORT_MAX_KEYS) {
    SortKeys a{};
    a.nkeys = nkeys - lo < SORT_MAX_KEYS ? nkeys - lo : SORT_MAX_KEYS;
    for (int32_t c = 0; c < a.nkeys; ++c) a.k[c] = keys[lo + c];
    key_change_kernel<<<grid_1d(n), DEFAULT_BLOCK, 0, stream>>>(
        a, perm, n, nrows, lo > 0 ? 1 : 0, out);
  }
}

void srj_radix_hist(const uint64_t* keys, int64_t n, int32_t shift,
                    int64_t nblocks, int64_t* hist, hipStream_t stream) {
  int64_t g = nblocks < MAX_GRID ? nblocks : MAX_GRID;
  radix_hist_kernel<<<g, DEFAULT_BLOCK, 0, stream>>>(keys, n, shift, nblocks,
                                                     hist);
}

// keys: every field of every word; word w owns keys [word_begin[w],
// word_begin[w + 1]) and uses word_bits[w] bits; word 0 is least significant.
// work: srj_sort_order_work_words(n) int64 words. out: n int64. n > 0.
void srj_sort_order(const SortKey* keys, const int32_t* word_begin,
                    const int32_t* word_bits, int32_t nwords, int64_t n,
                    int64_t* work, int64_t* out, hipStream_t stream) {
  if (n <= SORT_TILE) {
    for (int32_t w = 0; w < nwords; ++w) {
      const SortKey* wk = keys + word_begin[w];
      int32_t nk = word_begin[w + 1] - word_begin[w];
      int32_t passes = (word_bits[w] + SORT_RADIX_BITS - 1) / SORT_RADIX_BITS;
      const int64_t* in_perm = w == 0 ? nullptr : out;
      SortKeys a{};
      const uint64_t* words = nullptr;
      if (nk <= SORT_MAX_KEYS) {
        a.nkeys = nk;
        for (int32_t c = 0; c < nk; ++c) a.k[c] = wk[c];
      } else {
        srj_sort_pack(wk, nk, in_perm, n, 0, (uint64_t*)work, stream);
        words = (const uint64_t*)work;
      }
      sort_small_kernel<<<1, DEFAULT_BLOCK, 0, stream>>>(
          a, words, in_perm, (int32_t)n, passes, out);
    }
    return;
  }
  const int64_t nblocks = sort_nblocks(n);
  const int grid = (int)(nblocks < MAX_GRID ? nblocks : MAX_GRID);
  uint64_t* kbuf[2] = {(uint64_t*)work, (uint64_t*)work + n};
  int64_t* ptmp = work + 2 * n;
  int64_t* hist = work + 3 * n;
  int64_t* totals = hist + SORT_RADIX * nblocks;
  int64_t total_passes = 0;
  for (int32_t w = 0; w < nwords; ++w)
    total_passes += (word_bits[w] + SORT_RADIX_BITS - 1) / SORT_RADIX_BITS;
  // the payload alternates between ptmp and out so the last pass writes out
  int64_t left = total_passes;
  const int64_t* perm = nullptr;  // identity
  for (int32_t w = 0; w < nwords; ++w) {
    srj_sort_pack(keys + word_begin[w], word_begin[w + 1] - word_begin[w], perm,
                  n, 0, kbuf[0], stream);
    int32_t passes = (word_bits[w] + SORT_RADIX_BITS - 1) / SORT_RADIX_BITS;
    int kc = 0;
    for (int32_t p = 0; p < passes; ++p) {
      const int32_t shift = p * SORT_RADIX_BITS;
      int64_t* pdst = (left % 2 == 1) ? out : ptmp;
      srj_radix_hist(kbuf[kc], n, shift, nblocks, hist, stream);
      sort_scan_rows_kernel<<<SORT_RADIX, DEFAULT_BLOCK, 0, stream>>>(
          hist, nblocks, totals);
      sort_scatter_kernel<<<grid, DEFAULT_BLOCK, 0, stream>>>(
          kbuf[kc], perm, n, shift, nblocks, hist, totals, kbuf[kc ^ 1], pdst);
      perm = pdst;
      kc ^= 1;
      --left;
    }
  }
}

}  // extern "C"
