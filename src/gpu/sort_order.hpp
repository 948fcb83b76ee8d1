// Field descriptor of the sort-order key packer, shared by sort_order.hip and
// its bindings. Plain C++: no HIP types.
#pragma once
#include <cstdint>

namespace srj {

enum SortKind : int32_t {
  SK_UINT = 0,   // value as is (uint8, key_bits-hinted ints, DECIMAL128 low)
  SK_SINT = 1,   // sign bit flipped at the dtype's width
  SK_BOOL = 2,   // non-zero byte -> 1
  SK_F32 = 3,
  SK_F64 = 4,
  SK_NULL = 5,   // the null field alone (a 64-bit value leaves it no room)
};

constexpr int32_t SF_DESC = 1;         // invert the value field
constexpr int32_t SF_NULLS_FIRST = 2;  // null -> 0, valid -> 1
constexpr int32_t SF_NULL_BIT = 4;     // emit the null field above the value

struct SortKey {
  const void* data;
  const uint8_t* valid;  // byte per row, or null
  int64_t stride;        // elements between rows (2 for a DECIMAL128 half)
  int32_t kind;
  int32_t width;         // bytes per element: 1, 2, 4 or 8
  int32_t bits;          // value field bits, 1..64
  int32_t shift;         // position of the field in its word
  int32_t flags;
  int32_t pad_;
};

}  // namespace srj
