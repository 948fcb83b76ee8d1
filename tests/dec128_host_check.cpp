// Host driver for the per-row DECIMAL128 arithmetic of
// src/gpu/decimal128_core.hpp, which compiles for the host as well as for the
// GPU. tests/test_decimal128_exact.py builds it with the host compiler and
// compares it with the exact oracle, so the arithmetic is checked on a
// machine without a GPU too.
//
// stdin, one row per line:  op x y p0 p1 p2 p3
//   op 0 multiply       p = scale_sum, out_scale, precision
//   op 1 divide         p = s1, s2, out_scale, precision
//   op 2 integer divide p = s1, s2, precision
//   op 3 remainder      p = up_x, up_y
//   op 4 add, 5 subtract p = up_x, up_y, precision
// stdout: the unscaled result, or "null".
#define __host__
#define __device__
#include "decimal128_core.hpp"

#include <cstdio>
#include <cstring>
#include <string>

using srj::u128;

static __int128 parse(const char* s) {
  bool neg = *s == '-';
  if (neg) ++s;
  u128 v = 0;
  for (; *s; ++s) v = v * 10 + (u128)(*s - '0');
  return (__int128)(neg ? (u128)0 - v : v);
}

static std::string format(__int128 v) {
  u128 u = srj::u128_abs(v);
  std::string s;
  do {
    s.insert(s.begin(), (char)('0' + (int)(u % 10)));
    u /= 10;
  } while (u);
  return v < 0 ? "-" + s : s;
}

int main() {
  int op, p[4];
  char xs[64], ys[64];
  while (std::scanf("%d %63s %63s %d %d %d %d", &op, xs, ys, &p[0], &p[1],
                    &p[2], &p[3]) == 7) {
    __int128 x = parse(xs), y = parse(ys), res = 0;
    bool valid = false;
    switch (op) {
      case 0: valid = srj::dec128_mul_row(x, y, p[0], p[1], p[2], &res); break;
      case 1:
        valid = srj::dec128_div_row(x, y, p[0], p[1], p[2], p[3], &res);
        break;
      case 2: valid = srj::dec128_intdiv_row(x, y, p[0], p[1], p[2], &res); break;
      case 3: valid = srj::dec128_rem_row(x, y, p[0], p[1], &res); break;
      case 4:
      case 5:
        valid = srj::dec128_addsub_row(x, y, p[0], p[1], op == 5, p[2], &res);
        break;
      default: return 2;
    }
    std::puts(valid ? format(res).c_str() : "null");
  }
  return 0;
}
