// Per-row DECIMAL128 arithmetic: magnitudes in a 4 x u64 chunked 256-bit type
// (like the reference's chunked256), the sign carried beside them. Nothing in
// here multiplies, adds or negates a signed 128-bit value, so no result rests
// on signed overflow. Every function is __host__ __device__: the kernels in
// decimal128.hip call one of the dec128_*_row functions per row, and the same
// code compiles for the host.
//
// Domain: |unscaled value| <= 2^127 and scales in [0, 38], which is every
// DECIMAL128 column. The comments on overflow below rely on it.
#pragma once
#include <cstdint>

namespace srj {

typedef unsigned __int128 u128;

struct U256 {
  uint64_t w[4];  // little-endian
};

__host__ __device__ inline u128 u128_abs(__int128 v) {
  u128 u = (u128)v;
  return v < 0 ? (u128)0 - u : u;  // 2^127 for INT128_MIN
}

__host__ __device__ inline U256 u256_from_u128(u128 v) {
  U256 r{};
  r.w[0] = (uint64_t)v;
  r.w[1] = (uint64_t)(v >> 64);
  return r;
}

// unsigned 128x128 -> 256 multiply
__host__ __device__ inline U256 u256_mul_u128(u128 a, u128 b) {
  uint64_t a0 = (uint64_t)a, a1 = (uint64_t)(a >> 64);
  uint64_t b0 = (uint64_t)b, b1 = (uint64_t)(b >> 64);
  u128 p00 = (u128)a0 * b0;
  u128 p01 = (u128)a0 * b1;
  u128 p10 = (u128)a1 * b0;
  u128 p11 = (u128)a1 * b1;
  U256 r{};
  r.w[0] = (uint64_t)p00;
  u128 mid = (p00 >> 64) + (uint64_t)p01 + (uint64_t)p10;
  r.w[1] = (uint64_t)mid;
  u128 hi = (mid >> 64) + (p01 >> 64) + (p10 >> 64) + (uint64_t)p11;
  r.w[2] = (uint64_t)hi;
  r.w[3] = (uint64_t)((hi >> 64) + (p11 >> 64));
  return r;
}

// a * m; *ovf is set (never cleared) when the product needs more than 256 bits
__host__ __device__ inline U256 u256_mul_small(const U256& a, uint64_t m,
                                               bool* ovf) {
  U256 r{};
  u128 carry = 0;
  for (int i = 0; i < 4; ++i) {
    u128 p = (u128)a.w[i] * m + (uint64_t)carry;
    r.w[i] = (uint64_t)p;
    carry = p >> 64;
  }
  if (carry) *ovf = true;
  return r;
}

// divide a by a small u64, returning the quotient; remainder out
__host__ __device__ inline U256 u256_divmod_u64(const U256& a, uint64_t d,
                                                uint64_t* rem) {
  U256 q{};
  u128 r = 0;
  for (int i = 3; i >= 0; --i) {
    r = (r << 64) | a.w[i];
    q.w[i] = (uint64_t)(r / d);
    r = r % d;
  }
  *rem = (uint64_t)r;
  return q;
}

__host__ __device__ inline U256 u256_add(const U256& a, const U256& b) {
  U256 r;
  u128 c = 0;
  for (int i = 0; i < 4; ++i) {
    u128 s = (u128)a.w[i] + b.w[i] + (uint64_t)c;
    r.w[i] = (uint64_t)s;
    c = s >> 64;
  }
  return r;
}

// a - b modulo 2^256
__host__ __device__ inline U256 u256_sub(const U256& a, const U256& b) {
  U256 r;
  uint64_t borrow = 0;
  for (int i = 0; i < 4; ++i) {
    u128 d = (u128)a.w[i] - b.w[i] - borrow;
    r.w[i] = (uint64_t)d;
    borrow = (uint64_t)(d >> 64) & 1;
  }
  return r;
}

__host__ __device__ inline bool u256_ge(const U256& a, const U256& b) {
  for (int i = 3; i > 0; --i)
    if (a.w[i] != b.w[i]) return a.w[i] > b.w[i];
  return a.w[0] >= b.w[0];
}

__host__ __device__ inline U256 u256_inc(const U256& a) {
  U256 one{};
  one.w[0] = 1;
  return u256_add(a, one);
}

__host__ __device__ inline const uint64_t* pow10_u64_table() {
  static const uint64_t t[20] = {1ull,
                                 10ull,
                                 100ull,
                                 1000ull,
                                 10000ull,
                                 100000ull,
                                 1000000ull,
                                 10000000ull,
                                 100000000ull,
                                 1000000000ull,
                                 10000000000ull,
                                 100000000000ull,
                                 1000000000000ull,
                                 10000000000000ull,
                                 100000000000000ull,
                                 1000000000000000ull,
                                 10000000000000000ull,
                                 100000000000000000ull,
                                 1000000000000000000ull,
                                 10000000000000000000ull};
  return t;
}

// a * 10^p in chunks of 10^19; *ovf as in u256_mul_small
__host__ __device__ inline U256 u256_mul_pow10(U256 a, int p, bool* ovf) {
  const uint64_t* P = pow10_u64_table();
  while (p > 0) {
    int step = p > 19 ? 19 : p;
    a = u256_mul_small(a, P[step], ovf);
    p -= step;
  }
  return a;
}

// scale mag down by `drop` decimal digits with HALF_UP. Only the FIRST
// dropped digit decides HALF_UP, so: truncate (drop-1) digits chunked, then
// one divmod-10 with rem >= 5 rounding.
__host__ __device__ inline U256 u256_scale_down_half_up(U256 mag, int drop) {
  const uint64_t* P = pow10_u64_table();
  int trunc = drop - 1;
  while (trunc > 0) {
    int step = trunc > 19 ? 19 : trunc;
    uint64_t rem;
    mag = u256_divmod_u64(mag, P[step], &rem);
    trunc -= step;
  }
  uint64_t rem;
  U256 q = u256_divmod_u64(mag, 10, &rem);
  if (rem >= 5) q = u256_inc(q);
  return q;
}

// num / den, den != 0: shift-subtract long division, one step per bit of num
// below its leading zeros; the remainder comes out in *rem. The words of num
// are walked with constant indices so that they stay in registers.
__host__ __device__ inline U256 u256_divmod(const U256& num, const U256& den,
                                            U256* rem) {
  U256 q{}, r{};
  bool started = false;
#pragma unroll
  for (int i = 3; i >= 0; --i) {
    uint64_t w = num.w[i];
    int nbits = 64;
    if (!started) {
      if (w == 0) continue;
      int lz = __builtin_clzll(w);
      w <<= lz;
      nbits -= lz;
      started = true;
    }
    uint64_t qw = 0;
    for (int k = 0; k < nbits; ++k) {
      // r = 2r + next bit of num. r < den, so a bit shifted out at the top
      // means 2r >= 2^256 > den, and the subtraction modulo 2^256 is exact.
      uint64_t top = r.w[3] >> 63;
      r.w[3] = (r.w[3] << 1) | (r.w[2] >> 63);
      r.w[2] = (r.w[2] << 1) | (r.w[1] >> 63);
      r.w[1] = (r.w[1] << 1) | (r.w[0] >> 63);
      r.w[0] = (r.w[0] << 1) | (w >> 63);
      w <<= 1;
      qw <<= 1;
      if (top || u256_ge(r, den)) {
        r = u256_sub(r, den);
        qw |= 1;
      }
    }
    q.w[i] = qw;
  }
  *rem = r;
  return q;
}

__host__ __device__ inline u128 pow10_u128(int p) {  // p <= 38
  u128 r = 1;
  for (int i = 0; i < p; ++i) r *= 10;
  return r;
}

// |v| < 10^precision, for every int128: INT128_MIN has magnitude 2^127, which
// is above 10^38 and is taken as unsigned, never negated as a signed value.
__host__ __device__ inline bool i128_precision_ok(__int128 v, int precision) {
  if (precision >= 39) return true;
  return u128_abs(v) < pow10_u128(precision);
}

// sign and magnitude -> int128. False (null) when the magnitude needs more
// than 127 bits or `precision` digits.
__host__ __device__ inline bool dec128_finish(const U256& mag, bool neg,
                                              int precision, __int128* res) {
  if (mag.w[2] | mag.w[3] | (mag.w[1] >> 63)) return false;
  u128 m = ((u128)mag.w[1] << 64) | mag.w[0];
  __int128 v = (__int128)(neg ? (u128)0 - m : m);
  if (!i128_precision_ok(v, precision)) return false;
  *res = v;
  return true;
}

// The dec128_*_row functions return the row's validity and store its value in
// *res, which the caller has set to 0 and which stays 0 for a null.

// multiply: the product of the unscaled values rescaled from s1 + s2 to
// out_scale, HALF_UP when digits are dropped.
__host__ __device__ inline bool dec128_mul_row(__int128 x, __int128 y,
                                               int scale_sum, int out_scale,
                                               int precision, __int128* res) {
  U256 p = u256_mul_u128(u128_abs(x), u128_abs(y));
  int drop = scale_sum - out_scale;
  bool ovf = false;  // past 2^256 is past every precision
  if (drop > 0) p = u256_scale_down_half_up(p, drop);
  else if (drop < 0) p = u256_mul_pow10(p, -drop, &ovf);
  return !ovf && dec128_finish(p, (x < 0) != (y < 0), precision, res);
}

// divide: the exact HALF_UP of the true quotient at out_scale. With
// e = out_scale - s1 + s2 that is |x| * 10^e / |y| for e >= 0 and
// |x| / (|y| * 10^-e) for e < 0, rounded once from the remainder. (For e < 0
// the reference divides twice and truncates the first time, so it can differ
// in the last digit; this is the exact value.)
__host__ __device__ inline bool dec128_div_row(__int128 x, __int128 y, int s1,
                                               int s2, int out_scale,
                                               int precision, __int128* res) {
  if (y == 0) return false;
  int e = out_scale - s1 + s2;
  U256 num = u256_from_u128(u128_abs(x)), den = u256_from_u128(u128_abs(y));
  // |x| * 10^e >= 2^256 makes the quotient at least 2^256 / 2^127: null.
  // |y| * 10^38 is below 2^254, so the divisor cannot overflow.
  bool num_ovf = false, den_ovf = false;
  if (e >= 0) num = u256_mul_pow10(num, e, &num_ovf);
  else den = u256_mul_pow10(den, -e, &den_ovf);
  if (num_ovf) return false;
  U256 r;
  U256 q = u256_divmod(num, den, &r);
  if (u256_ge(r, u256_sub(den, r))) q = u256_inc(q);  // 2r >= den
  return dec128_finish(q, (x < 0) != (y < 0), precision, res);
}

// integer divide: (|x| * 10^s2) / (|y| * 10^s1) truncated, sign of the
// operands. Both sides stay below 2^254.
__host__ __device__ inline bool dec128_intdiv_row(__int128 x, __int128 y,
                                                  int s1, int s2,
                                                  int precision,
                                                  __int128* res) {
  if (y == 0) return false;
  bool ovf = false;
  U256 num = u256_mul_pow10(u256_from_u128(u128_abs(x)), s2, &ovf);
  U256 den = u256_mul_pow10(u256_from_u128(u128_abs(y)), s1, &ovf);
  U256 r;
  U256 q = u256_divmod(num, den, &r);
  return dec128_finish(q, (x < 0) != (y < 0), precision, res);
}

// remainder of the operands aligned to one scale (up_x, up_y: digits to scale
// each side up by, one of them 0), sign of x. Null only for y == 0: the
// remainder is below both aligned operands, and the one that was not scaled
// fits in 128 bits.
__host__ __device__ inline bool dec128_rem_row(__int128 x, __int128 y,
                                               int up_x, int up_y,
                                               __int128* res) {
  if (y == 0) return false;
  bool ovf = false;
  U256 num = u256_mul_pow10(u256_from_u128(u128_abs(x)), up_x, &ovf);
  U256 den = u256_mul_pow10(u256_from_u128(u128_abs(y)), up_y, &ovf);
  U256 r;
  u256_divmod(num, den, &r);
  return dec128_finish(r, x < 0, 39, res);
}

// add / subtract of the operands aligned to one scale (up_x, up_y as above).
// The aligned magnitudes stay below 2^254, so their sum fits in 256 bits.
__host__ __device__ inline bool dec128_addsub_row(__int128 x, __int128 y,
                                                  int up_x, int up_y, bool sub,
                                                  int precision,
                                                  __int128* res) {
  bool ovf = false;
  U256 mx = u256_mul_pow10(u256_from_u128(u128_abs(x)), up_x, &ovf);
  U256 my = u256_mul_pow10(u256_from_u128(u128_abs(y)), up_y, &ovf);
  bool nx = x < 0, ny = (y < 0) != sub;
  if (nx == ny) return dec128_finish(u256_add(mx, my), nx, precision, res);
  if (u256_ge(mx, my)) return dec128_finish(u256_sub(mx, my), nx, precision, res);
  return dec128_finish(u256_sub(my, mx), ny, precision, res);
}

}  // namespace srj
