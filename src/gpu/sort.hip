// Sort-merge join kernel.
//
// Reference parity: JoinPrimitives.sort_merge_inner_join
// (join_primitives.hpp:64-72). The build keys arrive sorted (the packed-key
// radix sort of sort_order.hip, through ops/sort.py: sort_pairs_i64); each
// probe row, sorted or not, binary-searches them (lower/upper bound) and the
// matches are emitted in two phases, count then fill, with wave-aggregated
// output cursors.
#include "srj_common.hpp"

namespace srj {

template <bool FILL>
__global__ void merge_join_kernel(const int64_t* __restrict__ build_sorted,
                                  const int64_t* __restrict__ build_rows,
                                  int64_t nbuild,
                                  const int64_t* __restrict__ probe,
                                  const uint8_t* __restrict__ pvalid,
                                  int64_t nprobe, uint64_t* __restrict__ counter,
                                  int32_t* __restrict__ out_build,
                                  int64_t* __restrict__ out_probe,
                                  int64_t out_capacity) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int lane = threadIdx.x & (WAVE - 1);
  uint64_t local = 0;
  int64_t npad = (nprobe + WAVE - 1) & ~(int64_t)(WAVE - 1);
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < npad;
       row += stride) {
    bool act = row < nprobe && is_valid(pvalid, row);
    int64_t lo = 0, hi = 0;
    if (act) {
      int64_t k = probe[row];
      int64_t a = 0, b2 = nbuild;
      while (a < b2) {  // lower bound
        int64_t mid = (a + b2) >> 1;
        if (build_sorted[mid] < k) a = mid + 1;
        else b2 = mid;
      }
      lo = a;
      b2 = nbuild;
      while (a < b2) {  // upper bound
        int64_t mid = (a + b2) >> 1;
        if (build_sorted[mid] <= k) a = mid + 1;
        else b2 = mid;
      }
      hi = a;
    }
    uint32_t nm = (uint32_t)(hi - lo);
    if (!FILL) {
      local += nm;
      continue;
    }
    uint32_t incl = wave_prefix_incl(nm);
    uint32_t total = __shfl(incl, WAVE - 1, WAVE);
    uint64_t wbase = 0;
    if (lane == WAVE - 1 && total)
      wbase = atomicAdd((unsigned long long*)counter, (unsigned long long)total);
    wbase = __shfl(wbase, WAVE - 1, WAVE);
    int64_t pos = (int64_t)(wbase + incl - nm);
    for (int64_t j = lo; j < hi; ++j) {
      if (pos < out_capacity) {
        out_build[pos] = (int32_t)build_rows[j];
        out_probe[pos] = row;
      }
      ++pos;
    }
  }
  if (!FILL) {
    local = wave_sum(local);
    if (lane == 0 && local)
      atomicAdd((unsigned long long*)counter, (unsigned long long)local);
  }
}

}  // namespace srj

using namespace srj;

extern "C" {

void srj_merge_join(const int64_t* build_sorted, const int64_t* build_rows,
                    int64_t nbuild, const int64_t* probe, const uint8_t* pvalid,
                    int64_t nprobe, uint64_t* counter, int32_t* out_build,
                    int64_t* out_probe, int64_t out_capacity, int32_t fill,
                    hipStream_t stream) {
  if (fill)
    merge_join_kernel<true><<<grid_1d(nprobe), DEFAULT_BLOCK, 0, stream>>>(
        build_sorted, build_rows, nbuild, probe, pvalid, nprobe, counter,
        out_build, out_probe, out_capacity);
  else
    merge_join_kernel<false><<<grid_1d(nprobe), DEFAULT_BLOCK, 0, stream>>>(
        build_sorted, build_rows, nbuild, probe, pvalid, nprobe, counter,
        nullptr, nullptr, 0);
}

}  // extern "C"
