// Window functions over a sorted order: descriptors shared by window.hip and
// bind_window.cpp. Python mirrors the numeric values in ops/window.py.
#pragma once
#include <cstdint>

namespace srj {

enum WinFn : int32_t {
  WF_ROW_NUMBER = 0,
  WF_RANK = 1,
  WF_DENSE_RANK = 2,
  WF_COUNT = 3,
  WF_SUM = 4,
  WF_MIN = 5,
  WF_MAX = 6,
  WF_AVG = 7,
};

// Frames of the five aggregates; the ranking functions ignore the frame.
enum WinFrame : int32_t {
  WFR_PARTITION = 0,  // the whole partition
  WFR_ROWS = 1,       // unbounded preceding .. current row
  WFR_RANGE = 2,      // unbounded preceding .. last peer of the current row
};

// Element kind of the value column; `width` is its size in bytes.
enum WinKind : int32_t {
  WK_NONE = 0,  // no value column: ranking functions and count(*)
  WK_BOOL = 1,
  WK_SINT = 2,
  WK_F32 = 3,
  WK_F64 = 4,
};

struct WinFunc {
  int32_t fn;
  int32_t frame;
  int32_t kind;
  int32_t width;
  int64_t stride;        // elements between consecutive rows of `values`
  const void* values;    // read in place as values[perm[i] * stride]
  const uint8_t* valid;  // byte per row, zero = null; may be null
  void* out;             // written as out[perm[i]]
  uint8_t* out_valid;    // byte per row; may be null
};

constexpr int WINDOW_MAX_FUNCS = 8;
constexpr int WINDOW_EPT = 8;
constexpr int WINDOW_TILE_ROWS = 256 * WINDOW_EPT;  // 2048
constexpr int WINDOW_SMALL_ROWS = WINDOW_TILE_ROWS;
// tile carries scanned per round of the one-workgroup carry scan
constexpr int WINDOW_CARRY_PER_THREAD = 4;
constexpr int WINDOW_CARRY_CHUNK = 256 * WINDOW_CARRY_PER_THREAD;  // 1024

}  // namespace srj
