// The function descriptor of seg_scan.hpp as the window and segmented-reduce
// bindings take it from Python, and its checks.
#pragma once
#include "srj_bind.hpp"
#include "seg_scan.hpp"

#include <tuple>
#include <vector>

// (fn, frame, kind, width, stride, values, valid, out, out_valid)
using SegFuncTuple = std::tuple<int32_t, int32_t, int32_t, int32_t, int64_t,
                                uintptr_t, uintptr_t, uintptr_t, uintptr_t>;

// `name` heads the messages. windowed: the ranking functions and the frames
// are accepted; otherwise SF_COUNT..SF_AVG only, and the frame is ignored.
inline srj::SegFunc to_seg_func(const SegFuncTuple& t, size_t index,
                                const char* name, bool windowed) {
  srj::SegFunc f{};
  f.fn = std::get<0>(t);
  f.frame = windowed ? std::get<1>(t) : srj::SFR_PARTITION;
  f.kind = std::get<2>(t);
  f.width = std::get<3>(t);
  f.stride = std::get<4>(t);
  f.values = as_ptr<const void>(std::get<5>(t));
  f.valid = as_ptr<const uint8_t>(std::get<6>(t));
  f.out = as_ptr<void>(std::get<7>(t));
  f.out_valid = as_ptr<uint8_t>(std::get<8>(t));
  const std::string w =
      std::string(name) + ": funcs[" + std::to_string(index) + "]";
  if (f.fn < (windowed ? srj::SF_ROW_NUMBER : srj::SF_COUNT) ||
      f.fn > srj::SF_AVG)
    throw std::invalid_argument(w + ": unknown function");
  if (f.frame < srj::SFR_PARTITION || f.frame > srj::SFR_RANGE)
    throw std::invalid_argument(w + ": unknown frame");
  if (f.kind < srj::SK_NONE || f.kind > srj::SK_F64)
    throw std::invalid_argument(w + ": unknown value kind");
  if (f.out == nullptr) throw std::invalid_argument(w + ": null output");
  if (std::get<7>(t) % 8 != 0 && (f.fn < srj::SF_MIN || f.fn > srj::SF_MAX))
    throw std::invalid_argument(w + ": output not aligned to 8 bytes");
  const bool needs_values = f.fn >= srj::SF_SUM;
  if (needs_values && f.kind == srj::SK_NONE)
    throw std::invalid_argument(w + ": function needs a value column");
  if (f.kind == srj::SK_NONE) {
    f.values = nullptr;
    f.stride = 1;
    f.width = 1;
    if (f.fn <= srj::SF_DENSE_RANK) f.valid = nullptr;
  } else {
    if (f.values == nullptr) throw std::invalid_argument(w + ": null values");
    if (f.width != 1 && f.width != 2 && f.width != 4 && f.width != 8)
      throw std::invalid_argument(w + ": width must be 1, 2, 4 or 8");
    if ((f.kind == srj::SK_F32 && f.width != 4) ||
        (f.kind == srj::SK_F64 && f.width != 8) ||
        (f.kind == srj::SK_BOOL && f.width != 1))
      throw std::invalid_argument(w + ": width does not match the kind");
    if (std::get<5>(t) % f.width != 0 || std::get<7>(t) % f.width != 0)
      throw std::invalid_argument(w + ": buffer not aligned to its element");
    if (f.stride < 1) throw std::invalid_argument(w + ": stride < 1");
  }
  return f;
}

inline std::vector<srj::SegFunc> to_seg_funcs(
    const std::vector<SegFuncTuple>& funcs, const char* name, bool windowed) {
  std::vector<srj::SegFunc> fs;
  for (size_t i = 0; i < funcs.size(); ++i)
    fs.push_back(to_seg_func(funcs[i], i, name, windowed));
  return fs;
}
