// The function descriptor and the tile constants of the rolling window
// kernel (window_rolling.hip). No HIP in here: bind_window_rolling.cpp
// includes it, and Python mirrors the constants in ops/_segscan.py.
#pragma once
#include "seg_scan.hpp"

namespace srj {

// lag and lead, one function: the value `shift` sorted positions away. The
// code follows SF_AVG; window.hip and seg_reduce.hip never see it.
constexpr int32_t RF_SHIFT = 8;

// SegFunc (its layout is window.hip's and seg_reduce.hip's, untouched) plus
// the row offsets. f.fn is SF_COUNT..SF_AVG or RF_SHIFT; f.frame is unused.
struct RollFunc {
  SegFunc f;
  int64_t lo, hi;  // aggregates: the frame is positions [i + lo, i + hi]
  int64_t shift;   // RF_SHIFT: the source is position i + shift
};

// |lo|, |hi| and |shift| are at most this, so that i + offset cannot wrap
constexpr int64_t ROLL_MAX_OFFSET = 2147483647;

// Sorted positions a workgroup owns, and the widest offset the staged path
// takes. One staged function holds ROLL_SLOTS 8-byte accumulator words and a
// validity bit per slot in LDS: 16 KiB + 256 B, so LDS admits 9 workgroups
// per CU of 160 KiB and the 32-waves-per-CU cap (8 workgroups of 4 waves) is
// what bounds occupancy, as for the scan kernels.
constexpr int ROLL_EPT = 4;
constexpr int ROLL_TILE_ROWS = 256 * ROLL_EPT;  // 1024
constexpr int ROLL_MAX_REACH = 512;
constexpr int ROLL_SLOTS = ROLL_TILE_ROWS + 2 * ROLL_MAX_REACH;  // 2048

}  // namespace srj
