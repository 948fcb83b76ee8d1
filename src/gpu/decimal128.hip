// DECIMAL128 arithmetic with 256-bit intermediates and Spark semantics.
//
// Reference parity: decimal_utils.cu (chunked256 4xu64 bignum, multiply/
// divide/add/sub/integer-divide/remainder with Spark's result scale and
// HALF_UP rounding, overflow -> null or ANSI error) + DecimalUtils.java.
//
// Values are 128-bit two's complement (2 x int64 little-endian words per
// row). The arithmetic of one row is in decimal128_core.hpp.
#include "srj_common.hpp"
#include "decimal128_core.hpp"

namespace srj {

// One thread per row. The three kernels differ only in the row function;
// this is the part they share: the grid-stride loop over whole waves, the
// input validity, the ANSI first-failing-row channel (a row that computed a
// null from non-null inputs) and the ballot-written output validity.
template <typename RowFn>
__device__ inline void dec128_rows(const __int128* __restrict__ a,
                                   const uint8_t* __restrict__ va,
                                   const __int128* __restrict__ b,
                                   const uint8_t* __restrict__ vb, int64_t n,
                                   __int128* __restrict__ out,
                                   uint8_t* __restrict__ out_valid,
                                   int64_t* __restrict__ err_row, RowFn row) {
  int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t npad = (n + WAVE - 1) & ~(int64_t)(WAVE - 1);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npad;
       i += stride) {
    bool in_range = i < n;
    bool valid = in_range && is_valid(va, i) && is_valid(vb, i);
    __int128 res = 0;
    if (valid) {
      valid = row(a[i], b[i], &res);
      if (!valid && err_row)
        atomicMin(reinterpret_cast<long long*>(err_row), (long long)i);
    }
    if (in_range) out[i] = res;
    ballot_write_validity(out_valid, i, valid);
  }
}

__global__ void dec128_mul_kernel(const __int128* __restrict__ a,
                                  const uint8_t* __restrict__ va,
                                  const __int128* __restrict__ b,
                                  const uint8_t* __restrict__ vb, int64_t n,
                                  int32_t scale_sum, int32_t out_scale,
                                  int32_t out_precision,
                                  __int128* __restrict__ out,
                                  uint8_t* __restrict__ out_valid,
                                  int64_t* __restrict__ err_row) {
  dec128_rows(a, va, b, vb, n, out, out_valid, err_row,
              [=](__int128 x, __int128 y, __int128* res) {
                return dec128_mul_row(x, y, scale_sum, out_scale,
                                      out_precision, res);
              });
}

// divide, integer divide (integer_div != 0) and remainder (remainder != 0;
// s1/s2 then carry the scale-up counts of the two sides)
__global__ void dec128_div_kernel(const __int128* __restrict__ a,
                                  const uint8_t* __restrict__ va,
                                  const __int128* __restrict__ b,
                                  const uint8_t* __restrict__ vb, int64_t n,
                                  int32_t s1, int32_t s2, int32_t out_scale,
                                  int32_t out_precision, int32_t integer_div,
                                  int32_t remainder,
                                  __int128* __restrict__ out,
                                  uint8_t* __restrict__ out_valid,
                                  int64_t* __restrict__ err_row) {
  dec128_rows(a, va, b, vb, n, out, out_valid, err_row,
              [=](__int128 x, __int128 y, __int128* res) {
                if (remainder) return dec128_rem_row(x, y, s1, s2, res);
                if (integer_div)
                  return dec128_intdiv_row(x, y, s1, s2, out_precision, res);
                return dec128_div_row(x, y, s1, s2, out_scale, out_precision,
                                      res);
              });
}

// add/sub with scale alignment (caller passes the scale-up counts)
__global__ void dec128_addsub_kernel(const __int128* __restrict__ a,
                                     const uint8_t* __restrict__ va,
                                     const __int128* __restrict__ b,
                                     const uint8_t* __restrict__ vb, int64_t n,
                                     int32_t up_a, int32_t up_b, int32_t sub,
                                     int32_t out_precision,
                                     __int128* __restrict__ out,
                                     uint8_t* __restrict__ out_valid,
                                     int64_t* __restrict__ err_row) {
  dec128_rows(a, va, b, vb, n, out, out_valid, err_row,
              [=](__int128 x, __int128 y, __int128* res) {
                return dec128_addsub_row(x, y, up_a, up_b, sub != 0,
                                         out_precision, res);
              });
}

}  // namespace srj

using namespace srj;

extern "C" {

void srj_dec128_mul(const void* a, const uint8_t* va, const void* b,
                    const uint8_t* vb, int64_t n, int32_t scale_sum,
                    int32_t out_scale, int32_t out_precision, void* out,
                    uint8_t* out_valid, int64_t* err_row, hipStream_t stream) {
  dec128_mul_kernel<<<grid_1d(n), DEFAULT_BLOCK, 0, stream>>>(
      (const __int128*)a, va, (const __int128*)b, vb, n, scale_sum, out_scale,
      out_precision, (__int128*)out, out_valid, err_row);
}

void srj_dec128_div(const void* a, const uint8_t* va, const void* b,
                    const uint8_t* vb, int64_t n, int32_t s1, int32_t s2,
                    int32_t out_scale, int32_t out_precision, int32_t integer_div,
                    int32_t remainder, void* out, uint8_t* out_valid,
                    int64_t* err_row, hipStream_t stream) {
  dec128_div_kernel<<<grid_1d(n), DEFAULT_BLOCK, 0, stream>>>(
      (const __int128*)a, va, (const __int128*)b, vb, n, s1, s2, out_scale,
      out_precision, integer_div, remainder, (__int128*)out, out_valid, err_row);
}

void srj_dec128_addsub(const void* a, const uint8_t* va, const void* b,
                       const uint8_t* vb, int64_t n, int32_t up_a, int32_t up_b,
                       int32_t sub, int32_t out_precision, void* out,
                       uint8_t* out_valid, int64_t* err_row, hipStream_t stream) {
  dec128_addsub_kernel<<<grid_1d(n), DEFAULT_BLOCK, 0, stream>>>(
      (const __int128*)a, va, (const __int128*)b, vb, n, up_a, up_b, sub,
      out_precision, (__int128*)out, out_valid, err_row);
}

}  // extern "C"
