// Segmented reduce over a sorted order: descriptors shared by seg_reduce.hip
// and bind_seg_reduce.cpp. Python mirrors the numeric values in
// ops/segmented.py.
#pragma once
#include <cstdint>

namespace srj {

enum SegFn : int32_t {
  SR_COUNT = 0,
  SR_SUM = 1,
  SR_MIN = 2,
  SR_MAX = 3,
  SR_AVG = 4,
};

// Element kind of the value column; `width` is its size in bytes.
enum SegKind : int32_t {
  SRK_NONE = 0,  // no value column: count(*)
  SRK_BOOL = 1,
  SRK_SINT = 2,
  SRK_F32 = 3,
  SRK_F64 = 4,
};

struct SegFunc {
  int32_t fn;
  int32_t kind;
  int32_t width;
  int32_t pad;
  int64_t stride;        // elements between consecutive rows of `values`
  const void* values;    // read in place as values[perm[i] * stride]
  const uint8_t* valid;  // byte per original row, zero = null; may be null
  void* out;             // written as out[segment number]
  uint8_t* out_valid;    // byte per segment; may be null
};

constexpr int SEG_MAX_FUNCS = 8;
constexpr int SEG_EPT = 8;
constexpr int SEG_TILE_ROWS = 256 * SEG_EPT;  // 2048
constexpr int SEG_SMALL_ROWS = SEG_TILE_ROWS;
// tile carries scanned per round of the one-workgroup carry scan
constexpr int SEG_CARRY_PER_THREAD = 4;
constexpr int SEG_CARRY_CHUNK = 256 * SEG_CARRY_PER_THREAD;  // 1024

}  // namespace srj
