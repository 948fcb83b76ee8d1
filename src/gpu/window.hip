// Window functions over a sorted order: row_number, rank, dense_rank and
// count/sum/min/max/avg over the partition, running (rows) and default range
// frames, as one family of segmented-scan kernels.
//
// Reference parity: the windowed aggregations and ranking scans the
// reference's Window exec takes from libcudf (grouped scans over a sorted
// table) - SURVEY.md L0.
//
// Inputs are the permutation `perm` that sorts the rows by (partition keys,
// order keys) and two byte flags per SORTED position: partition head and peer
// group head. Values are read in place as values[perm[i]] and results are
// written as out[perm[i]]: no sorted copy, no inverse permutation.
//
// How it works:
//  * ONE SCAN PER FUNCTION. Every function is a forward segmented inclusive
//    scan of a (valid count, accumulator) state, segmented by the partition
//    heads, followed by a read of the state at the frame's last position: the
//    row itself (rows), the last row of its peer group (range) or of its
//    partition (partition). row_number is the count of rows, dense_rank the
//    count of peer heads, rank the row count minus the distance to the last
//    peer head (a running maximum of head positions). The last positions
//    come from a reverse scan of the next head position. The state, the
//    operator, the block scan, the value load and the aggregate store are
//    those of seg_scan.hpp, shared with seg_reduce.hip; here are the ranking
//    cases, the frame lookup and the reverse scan.
//  * SMALL PATH (m <= SEG_SMALL_ROWS). One workgroup, one launch: the
//    states of the tile sit in LDS and the frame ends index them.
//  * TILED PATH. Three launches: (1) every tile scans itself and writes, per
//    function, its carry, the state before its first partition head and the
//    state before its first peer head; (2) one workgroup scans the tile
//    carries in chunks with a running carry (the structure of
//    block_scan_chunked, with the segmented operator) and turns the two
//    prefix states into "state at the end of the partition / peer group that
//    is open when the tile begins", and a reverse pass finds for every tile
//    the next tile that holds a head; (3) every tile rescans with its
//    carry-in, looks the frame ends up (in LDS, or the closing state of the
//    next tile with a head when the frame ends past the tile) and scatters.
//  * NO SPINS, NO ATOMICS (the requirement compact.hip and sort_order.hip
//    state): no kernel waits on another workgroup, the launch count depends
//    on m and the number of functions only, and the combine order is fixed by
//    the position, so float sums are bit-identical run to run.
//
// MI355X notes: wave64 scans by __shfl_up/__shfl_down; a thread owns
// SEG_EPT consecutive positions, so perm is read 64 contiguous bytes per
// lane and the in-register part of the scan needs no LDS. The LDS state
// arrays are padded by one slot per 8 so the 64-byte lane stride does not
// fold the lanes of a half-wave onto 8 banks.
#include "seg_scan.hpp"

namespace srj {

constexpr int32_t WIN_NONE = SEG_TILE_ROWS;  // no head later in the tile
constexpr int WIN_SLOTS = SEG_TILE_ROWS + SEG_TILE_ROWS / 8;

static_assert(SEG_EPT == 8, "lds_slot pads one slot per thread");
static_assert(SEG_TILE_ROWS < 65536, "next-head positions are 16-bit");

// Reverse exclusive minimum over the threads AFTER this one, of two values
// at once (`none` where there is no later thread); *allp / *allq are the
// minima over all threads. One barrier, as seg_block_scan.
__device__ inline void win_block_rmin2(int32_t& p, int32_t& q, int32_t none,
                                       int32_t (&wm)[2][SEG_WAVES],
                                       int32_t* allp, int32_t* allq) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  int32_t ip = p, iq = q;
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const int32_t op = __shfl_down(ip, off, WAVE);
    const int32_t oq = __shfl_down(iq, off, WAVE);
    if (lane + off < WAVE) {
      ip = op < ip ? op : ip;
      iq = oq < iq ? oq : iq;
    }
  }
  if (lane == 0) {
    wm[0][wave] = ip;
    wm[1][wave] = iq;
  }
  __syncthreads();
  int32_t ep = __shfl_down(ip, 1, WAVE);
  int32_t eq = __shfl_down(iq, 1, WAVE);
  if (lane == WAVE - 1) ep = eq = none;
  int32_t ap = none, aq = none;
#pragma unroll
  for (int w = 0; w < SEG_WAVES; ++w) {
    const int32_t a = wm[0][w], b = wm[1][w];
    if (w > wave) {
      ep = a < ep ? a : ep;
      eq = b < eq ? b : eq;
    }
    ap = a < ap ? a : ap;
    aq = b < aq ? b : aq;
  }
  p = ep;
  q = eq;
  *allp = ap;
  *allq = aq;
}

// The scan input of function f at sorted position i (row `row`, -1 when perm
// holds no row of the column there).
__device__ inline SegState win_item(const SegFunc& f, int32_t op, int64_t i,
                                    int64_t row, bool part_head,
                                    bool peer_head) {
  SegState x;
  x.flag = part_head;
  x.cnt = 0;
  x.acc = seg_identity(op);
  if (row < 0) return x;
  switch (f.fn) {
    case SF_ROW_NUMBER:
      x.cnt = 1;
      return x;
    case SF_DENSE_RANK:
      x.cnt = peer_head;
      return x;
    case SF_RANK:
      x.cnt = 1;
      if (peer_head) x.acc = (uint64_t)i;
      return x;
    default:
      return seg_value_item(f, op, row, part_head);
  }
}

// out[row] of function f from the state at the frame's last position.
__device__ inline void win_store(const SegFunc& f, int64_t i, int64_t row,
                                 int64_t cnt, uint64_t acc) {
  switch (f.fn) {
    case SF_ROW_NUMBER:
    case SF_DENSE_RANK:
    case SF_COUNT:
      static_cast<int64_t*>(f.out)[row] = cnt;
      return;
    case SF_RANK:
      static_cast<int64_t*>(f.out)[row] = cnt - i + (int64_t)acc;
      return;
    default:
      seg_store_agg(f, row, cnt, acc);
  }
}

__device__ inline int win_lds_slot(int p) { return p + (p >> 3); }

// Work layout (int64 words, nt tiles, function f):
//   [0, nt)        tile holds a partition head
//   [nt, 2nt)      tile holds a peer head
//   [2nt, 3nt)     next tile after this one that holds a partition head (nt:
//                  none)
//   [3nt, 4nt)     the same for peer heads
//   4nt + f * (6nt + 2) + ...
//     [0, 2nt)     (cnt, acc) per tile: its carry, then its carry-in
//     [2nt, 4nt)   state before the tile's first partition head, then the
//                  closing state of the partition open when the tile begins
//     [4nt, 6nt)   the same for the first peer head / open peer group
//     [6nt, 6nt+2) state at the last position of all
__host__ __device__ inline int64_t win_func_words(int64_t nt) {
  return 6 * nt + 2;
}

// EMIT = false: launch 1 of the tiled path (tile carries and prefix states).
// EMIT = true: the small path (work == nullptr, one tile) and launch 3.
template <bool EMIT>
__global__ __launch_bounds__(DEFAULT_BLOCK) void window_tile_kernel(
    SegFuncs fs, const int64_t* __restrict__ perm,
    const uint8_t* __restrict__ part, const uint8_t* __restrict__ peer,
    int64_t m, int64_t nt, int64_t* work) {
  __shared__ int64_t s_cnt[WIN_SLOTS];   // 18 KiB
  __shared__ uint64_t s_acc[WIN_SLOTS];  // 18 KiB
  __shared__ uint16_t s_np[SEG_TILE_ROWS];  // next partition head after p
  __shared__ uint16_t s_nq[SEG_TILE_ROWS];  // next peer head after p
  __shared__ SegState wt[SEG_WAVES];
  __shared__ int32_t wm[2][SEG_WAVES];
  const int tid = threadIdx.x;
  const int p0 = tid * SEG_EPT;

  for (int64_t T = blockIdx.x; T < nt; T += gridDim.x) {
    const int64_t base = T * SEG_TILE_ROWS;
    const int32_t nvalid =
        m - base < SEG_TILE_ROWS ? (int32_t)(m - base) : SEG_TILE_ROWS;
    const bool last = T == nt - 1;

    int64_t row[SEG_EPT];
    uint32_t pf = 0, qf = 0;
#pragma unroll
    for (int k = 0; k < SEG_EPT; ++k) {
      const int64_t i = base + p0 + k;
      row[k] = -1;
      if (p0 + k < nvalid) {
        const int64_t r = perm[i];
        if (r >= 0 && r < m) row[k] = r;  // never touch memory off the columns
        const bool h = i == 0 || part[i] != 0;
        const bool q = h || peer == nullptr || peer[i] != 0;
        pf |= (uint32_t)h << k;
        qf |= (uint32_t)q << k;
      }
    }

    // next head strictly after every position of the tile
    int32_t np = pf ? p0 + __builtin_ctz(pf) : WIN_NONE;
    int32_t nq = qf ? p0 + __builtin_ctz(qf) : WIN_NONE;
    int32_t firstp, firstq;  // first head of the tile
    win_block_rmin2(np, nq, WIN_NONE, wm, &firstp, &firstq);
#pragma unroll
    for (int k = SEG_EPT - 1; k >= 0; --k) {
      // the last tile ends every frame at its last row
      s_np[p0 + k] = (uint16_t)((last && np > nvalid) ? nvalid : np);
      s_nq[p0 + k] = (uint16_t)((last && nq > nvalid) ? nvalid : nq);
      if ((pf >> k) & 1u) np = p0 + k;
      if ((qf >> k) & 1u) nq = p0 + k;
    }
    int64_t nhp = nt, nhq = nt;
    if (EMIT) {
      if (work != nullptr) {
        nhp = work[2 * nt + T];
        nhq = work[3 * nt + T];
        if (nhp < 0 || nhp > nt) nhp = nt;  // never read off the work buffer
        if (nhq < 0 || nhq > nt) nhq = nt;
      }
    } else if (tid == 0) {
      work[T] = firstp != WIN_NONE;
      work[nt + T] = firstq != WIN_NONE;
    }
    __syncthreads();

    for (int32_t fi = 0; fi < fs.nf; ++fi) {
      const SegFunc& f = fs.f[fi];
      const int32_t op = seg_op(f);
      int64_t* fw =
          work != nullptr ? work + 4 * nt + fi * win_func_words(nt) : nullptr;
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
        const SegState x = win_item(f, op, base + p0 + k, row[k],
                                    (pf >> k) & 1u, (qf >> k) & 1u);
        s[k] = k == 0 ? x : seg_combine(op, s[k - 1], x);
      }
      SegState total;
      const SegState pre =
          seg_block_scan(op, s[SEG_EPT - 1], carry, wt, &total);
#pragma unroll
      for (int k = 0; k < SEG_EPT; ++k) {
        s[k] = seg_combine(op, pre, s[k]);
        const int slot = win_lds_slot(p0 + k);
        s_cnt[slot] = s[k].cnt;
        s_acc[slot] = s[k].acc;
      }
      __syncthreads();

      if (EMIT) {
        const bool ranking = f.fn <= SF_DENSE_RANK;
        const int32_t frame = ranking ? SFR_ROWS : f.frame;
        // frames that end past the tile: the closing state of the open
        // partition / peer group (the last tile has none)
        int64_t ecnt = 0;
        uint64_t eacc = 0;
        if (fw != nullptr && !last && frame != SFR_ROWS) {
          const int64_t nh = frame == SFR_PARTITION ? nhp : nhq;
          const int64_t* src =
              nh >= nt ? fw + 6 * nt
                       : fw + (frame == SFR_PARTITION ? 2 : 4) * nt + 2 * nh;
          ecnt = src[0];
          eacc = (uint64_t)src[1];
        }
#pragma unroll
        for (int k = 0; k < SEG_EPT; ++k) {
          if (row[k] < 0) continue;
          int64_t cnt = s[k].cnt;
          uint64_t acc = s[k].acc;
          if (frame != SFR_ROWS) {
            const int32_t nx =
                frame == SFR_PARTITION ? s_np[p0 + k] : s_nq[p0 + k];
            if (!last && nx >= WIN_NONE) {
              cnt = ecnt;
              acc = eacc;
            } else {
              // p0 + k < nx <= SEG_TILE_ROWS
              const int slot = win_lds_slot(nx - 1);
              cnt = s_cnt[slot];
              acc = s_acc[slot];
            }
          }
          win_store(f, base + p0 + k, row[k], cnt, acc);
        }
      } else if (tid == 0) {
        const int lslot = win_lds_slot(nvalid - 1);
        fw[2 * T] = s_cnt[lslot];
        fw[2 * T + 1] = (int64_t)s_acc[lslot];
        int64_t c = 0;
        uint64_t a = seg_identity(op);
        if (firstp > 0 && firstp < WIN_NONE) {
          c = s_cnt[win_lds_slot(firstp - 1)];
          a = s_acc[win_lds_slot(firstp - 1)];
        }
        fw[2 * nt + 2 * T] = c;
        fw[2 * nt + 2 * T + 1] = (int64_t)a;
        c = 0;
        a = seg_identity(op);
        if (firstq > 0 && firstq < WIN_NONE) {
          c = s_cnt[win_lds_slot(firstq - 1)];
          a = s_acc[win_lds_slot(firstq - 1)];
        }
        fw[4 * nt + 2 * T] = c;
        fw[4 * nt + 2 * T + 1] = (int64_t)a;
      }
      __syncthreads();  // the state arrays and wt are rewritten
    }
  }
}

// Launch 2 of the tiled path: one workgroup. See the work layout above.
__global__ __launch_bounds__(DEFAULT_BLOCK) void window_carry_kernel(
    SegFuncs fs, int64_t nt, int64_t* work) {
  __shared__ SegState wt[SEG_WAVES];
  __shared__ int32_t wm[2][SEG_WAVES];
  const int tid = threadIdx.x;
  const int64_t nchunks = (nt + SEG_CARRY_CHUNK - 1) / SEG_CARRY_CHUNK;
  const int32_t none = (int32_t)nt;  // nt < 2^31 (checked on the host)
  const int64_t* headp = work;
  const int64_t* headq = work + nt;

  // reverse: the next tile with a head, chunk by chunk from the end
  int32_t carryp = none, carryq = none;
  for (int64_t c = nchunks - 1; c >= 0; --c) {
    const int64_t t0 =
        c * SEG_CARRY_CHUNK + (int64_t)tid * SEG_CARRY_PER_THREAD;
    uint32_t hp = 0, hq = 0;
    int32_t fp = none, fq = none;
#pragma unroll
    for (int k = SEG_CARRY_PER_THREAD - 1; k >= 0; --k) {
      const int64_t T = t0 + k;
      if (T < nt && headp[T] != 0) {
        hp |= 1u << k;
        fp = (int32_t)T;
      }
      if (T < nt && headq[T] != 0) {
        hq |= 1u << k;
        fq = (int32_t)T;
      }
    }
    int32_t allp, allq;
    win_block_rmin2(fp, fq, none, wm, &allp, &allq);
    fp = carryp < fp ? carryp : fp;
    fq = carryq < fq ? carryq : fq;
#pragma unroll
    for (int k = SEG_CARRY_PER_THREAD - 1; k >= 0; --k) {
      const int64_t T = t0 + k;
      if (T < nt) {
        work[2 * nt + T] = fp;
        work[3 * nt + T] = fq;
      }
      if ((hp >> k) & 1u) fp = (int32_t)T;
      if ((hq >> k) & 1u) fq = (int32_t)T;
    }
    carryp = allp < carryp ? allp : carryp;
    carryq = allq < carryq ? allq : carryq;
    __syncthreads();  // wm is rewritten by the next chunk
  }

  for (int32_t fi = 0; fi < fs.nf; ++fi) {
    const int32_t op = seg_op(fs.f[fi]);
    int64_t* fw = work + 4 * nt + fi * win_func_words(nt);
    const SegState end = seg_carry_scan(
        op, headp, fw, nt, wt, [&](int64_t T, const SegState& ex) {
          // the two prefix states of tile T close behind its carry-in
#pragma unroll
          for (int h = 2; h <= 4; h += 2) {
            SegState px;
            px.flag = 0;
            px.cnt = fw[h * nt + 2 * T];
            px.acc = (uint64_t)fw[h * nt + 2 * T + 1];
            const SegState cl = seg_combine(op, ex, px);
            fw[h * nt + 2 * T] = cl.cnt;
            fw[h * nt + 2 * T + 1] = (int64_t)cl.acc;
          }
        });
    if (tid == 0) {
      fw[6 * nt] = end.cnt;
      fw[6 * nt + 1] = (int64_t)end.acc;
    }
  }
}

inline int64_t window_ntiles(int64_t m) {
  return (m + SEG_TILE_ROWS - 1) / SEG_TILE_ROWS;
}

}  // namespace srj

using namespace srj;

extern "C" {

// bytes of scratch one srj_window call of nfuncs functions needs
int64_t srj_window_work_bytes(int64_t m, int32_t nfuncs) {
  if (m <= SEG_SMALL_ROWS) return 0;
  const int64_t nt = window_ntiles(m);
  return 8 * (4 * nt + (int64_t)nfuncs * win_func_words(nt));
}

// 1 <= nfuncs <= SEG_MAX_FUNCS, m > 0, peer may be null (every row its own
// peer group), work: srj_window_work_bytes(m, nfuncs) bytes, 8-byte aligned.
void srj_window(const SegFunc* funcs, int32_t nfuncs, const int64_t* perm,
                const uint8_t* part, const uint8_t* peer, int64_t m,
                int64_t* work, hipStream_t stream) {
  SegFuncs a{};
  a.nf = nfuncs;
  for (int32_t i = 0; i < nfuncs; ++i) a.f[i] = funcs[i];
  if (m <= SEG_SMALL_ROWS) {
    window_tile_kernel<true><<<1, DEFAULT_BLOCK, 0, stream>>>(
        a, perm, part, peer, m, 1, nullptr);
    return;
  }
  const int64_t nt = window_ntiles(m);
  const int grid = (int)(nt < MAX_GRID ? nt : MAX_GRID);
  window_tile_kernel<false><<<grid, DEFAULT_BLOCK, 0, stream>>>(
      a, perm, part, peer, m, nt, work);
  window_carry_kernel<<<1, DEFAULT_BLOCK, 0, stream>>>(a, nt, work);
  window_tile_kernel<true><<<grid, DEFAULT_BLOCK, 0, stream>>>(
      a, perm, part, peer, m, nt, work);
}

}  // extern "C"
