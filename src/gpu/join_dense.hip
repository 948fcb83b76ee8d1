// Direct-address join table for dense, duplicate-free integer build keys (the
// shape of nearly every NDS surrogate key: d_date_sk, i_item_sk, ...).
//
//   slots[key - kmin] = row + 1;   0 = empty;   one uint32 per key of
//   [kmin, kmin + range)
//
// Hashing is work such a join does not need: the table is range x 4 B (an
// eighth of the narrow hashed table of hashtable_i64.hip at 25 % load), a
// build is one CAS per row with no chain, and a probe is one 4-byte load per
// row with at most one match. A duplicate build key cannot be represented:
// the build raises a flag and the host falls back to the hashed tables.
// K is the key column's element type: int columns are read in place.
#include "srj_common.hpp"

namespace srj {

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

// Contract of join_probe_n32_kernel minus idxmap: counter, out_build,
// out_probe, out_capacity (pairs past it are counted, not written) and
// build_matched (written even when the capacity is 0). A lane takes PPIPE
// consecutive rows (one or two validity bytes). A row is live when its
// validity bit is set and key - kmin, compared as a full 64-bit value, is
// below range; dead rows load slot 0 and are masked, so no load leaves the
// table and an offset that wraps past 2^32 or 2^63 cannot alias.
template <typename K, bool FILL, bool HAS_VALID, int PPIPE>
__global__ void join_probe_d32_kernel(
    const K* __restrict__ probe, const uint8_t* __restrict__ pvalid,
    int64_t nprobe, const uint32_t* __restrict__ slots, uint64_t range,
    long long kmin, uint64_t* __restrict__ counter,
    int32_t* __restrict__ out_build, int64_t* __restrict__ out_probe,
    int64_t out_capacity, uint8_t* __restrict__ build_matched) {
  static_assert(PPIPE == 8 || PPIPE == 16, "validity bytes per batch");
  int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  int lane = threadIdx.x & (WAVE - 1);
  uint64_t count_local = 0;
  int64_t nbatch = (nprobe + (int64_t)PPIPE - 1) / PPIPE;
  // pad so every lane of a wave runs the same iterations (wave shuffles)
  int64_t nbatch_pad = (nbatch + WAVE - 1) & ~(int64_t)(WAVE - 1);
  for (int64_t batch = tid; batch < nbatch_pad; batch += nthreads) {
    bool batch_ok = batch < nbatch;
    int64_t base = batch_ok ? batch * PPIPE : 0;
    uint32_t vbits = (1u << PPIPE) - 1u;
    if (HAS_VALID) {
      vbits = pvalid[base >> 3];
      // the second byte of a 16-row batch may lie past the mask's last byte
      if (PPIPE == 16 && base + 8 < nprobe)
        vbits |= (uint32_t)pvalid[(base >> 3) + 1] << 8;
    }
    if (base + PPIPE > nprobe) {
      int64_t tail = nprobe - base;
      vbits &= (uint32_t)((1u << (tail < 0 ? 0 : tail)) - 1u);
    }
    if (!batch_ok) vbits = 0;
    K k[PPIPE];
    if (base + PPIPE <= nprobe) {
      // whole batch in range: consecutive keys, merged into wide loads
#pragma unroll
      for (int b = 0; b < PPIPE; ++b) k[b] = probe[base + b];
    } else {
#pragma unroll
      for (int b = 0; b < PPIPE; ++b) {
        int64_t row = base + b;
        k[b] = row < nprobe ? probe[row] : (K)0;  // masked by vbits
      }
    }
    uint32_t off[PPIPE];
    uint32_t fw[PPIPE];
#pragma unroll
    for (int b = 0; b < PPIPE; ++b) {
      uint64_t o = (uint64_t)(long long)k[b] - (uint64_t)kmin;
      bool live = o < range;
      off[b] = live ? (uint32_t)o : 0u;
      if (!live) vbits &= ~(1u << b);
    }
#pragma unroll
    for (int b = 0; b < PPIPE; ++b) fw[b] = slots[off[b]];
    uint32_t mbits = 0;
#pragma unroll
    for (int b = 0; b < PPIPE; ++b)
      mbits |= (uint32_t)(fw[b] != 0) << b;
    mbits &= vbits;
    uint32_t nm = __popc(mbits);
    if (!FILL) {
      count_local += nm;
      continue;
    }
    // emit: one atomic per wave and batch, then plain stores from registers
    uint32_t incl = wave_prefix_incl(nm);
    uint32_t total = __shfl(incl, WAVE - 1, WAVE);
    uint64_t wave_base = 0;
    if (lane == WAVE - 1 && total)
      wave_base = atomicAdd((unsigned long long*)counter,
                            (unsigned long long)total);
    wave_base = __shfl(wave_base, WAVE - 1, WAVE);
    int64_t pos = (int64_t)(wave_base + incl - nm);
    if (mbits) {
#pragma unroll
      for (int b = 0; b < PPIPE; ++b) {
        if (!((mbits >> b) & 1)) continue;
        if (pos < out_capacity) {
          out_build[pos] = (int32_t)(fw[b] - 1);
          out_probe[pos] = base + b;
        }
        // matched flags are valid even when the pair output overflows
        if (build_matched) build_matched[fw[b] - 1] = 1;
        ++pos;
      }
    }
  }
  if (!FILL) {
    count_local = wave_sum(count_local);
    if (lane == 0 && count_local)
      atomicAdd((unsigned long long*)counter, (unsigned long long)count_local);
  }
}

}  // namespace srj

using namespace srj;

template <typename K, int PPIPE>
static void launch_probe_d32(const K* probe, const uint8_t* pvalid,
                             int64_t nprobe, const uint32_t* sl,
                             uint64_t range, long long kmin, uint64_t* counter,
                             int32_t* out_build, int64_t* out_probe,
                             int64_t out_capacity, uint8_t* build_matched,
                             int32_t fill, hipStream_t stream) {
  int64_t g = grid_1d((nprobe + PPIPE - 1) / PPIPE);
  if (fill) {
    if (pvalid)
      join_probe_d32_kernel<K, true, true, PPIPE>
          <<<g, DEFAULT_BLOCK, 0, stream>>>(
              probe, pvalid, nprobe, sl, range, kmin, counter, out_build,
              out_probe, out_capacity, build_matched);
    else
      join_probe_d32_kernel<K, true, false, PPIPE>
          <<<g, DEFAULT_BLOCK, 0, stream>>>(
              probe, pvalid, nprobe, sl, range, kmin, counter, out_build,
              out_probe, out_capacity, build_matched);
  } else {
    if (pvalid)
      join_probe_d32_kernel<K, false, true, PPIPE>
          <<<g, DEFAULT_BLOCK, 0, stream>>>(
              probe, pvalid, nprobe, sl, range, kmin, counter, nullptr,
              nullptr, 0, nullptr);
    else
      join_probe_d32_kernel<K, false, false, PPIPE>
          <<<g, DEFAULT_BLOCK, 0, stream>>>(
              probe, pvalid, nprobe, sl, range, kmin, counter, nullptr,
              nullptr, 0, nullptr);
  }
}

// Rows per lane and batch, chosen by measurement (docs/PERF.md): 16 while the
// table fits the 256 MiB Infinity Cache (half the wave-wide appends, 1.7x the
// probe rate at 2^20 and 2^26 slots), 8 beyond it, where the probe lives on
// waves in flight (8 per SIMD at 50 VGPRs against 5 at 88; 29.1 against 31.4
// ms per 1B rows into 1B slots).
constexpr uint64_t DENSE_PIPE16_MAX_SLOTS = 1ull << 26;

template <typename K>
static void probe_d32(const K* probe, const uint8_t* pvalid, int64_t nprobe,
                      const uint32_t* sl, uint64_t range, long long kmin,
                      uint64_t* counter, int32_t* out_build,
                      int64_t* out_probe, int64_t out_capacity,
                      uint8_t* build_matched, int32_t fill,
                      hipStream_t stream) {
  if (range <= DENSE_PIPE16_MAX_SLOTS)
    launch_probe_d32<K, 16>(probe, pvalid, nprobe, sl, range, kmin, counter,
                            out_build, out_probe, out_capacity, build_matched,
                            fill, stream);
  else
    launch_probe_d32<K, 8>(probe, pvalid, nprobe, sl, range, kmin, counter,
                           out_build, out_probe, out_capacity, build_matched,
                           fill, stream);
}

extern "C" {

// key_i32 != 0: keys are a 4-byte int column read in place, else int64.
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
  auto* sl = reinterpret_cast<const uint32_t*>(slots);
  if (key_i32)
    probe_d32(reinterpret_cast<const int*>(probe), pvalid, nprobe, sl,
              (uint64_t)range, kmin, counter, out_build, out_probe,
              out_capacity, build_matched, fill, stream);
  else
    probe_d32(reinterpret_cast<const long long*>(probe), pvalid, nprobe, sl,
              (uint64_t)range, kmin, counter, out_build, out_probe,
              out_capacity, build_matched, fill, stream);
}

}  // extern "C"
