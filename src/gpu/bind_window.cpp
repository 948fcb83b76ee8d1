// Bindings for the window-function kernels.
#include "srj_bind.hpp"
#include "window.hpp"

#include <tuple>
#include <vector>

using srj::WinFunc;

extern "C" {
int64_t srj_window_work_bytes(int64_t, int32_t);
void srj_window(const WinFunc*, int32_t, const int64_t*, const uint8_t*,
                const uint8_t*, int64_t, int64_t*, hipStream_t);
}

namespace {

// (fn, frame, kind, width, stride, values, valid, out, out_valid)
using Func = std::tuple<int32_t, int32_t, int32_t, int32_t, int64_t, uintptr_t,
                        uintptr_t, uintptr_t, uintptr_t>;

WinFunc to_func(const Func& t, size_t index) {
  WinFunc f{};
  f.fn = std::get<0>(t);
  f.frame = std::get<1>(t);
  f.kind = std::get<2>(t);
  f.width = std::get<3>(t);
  f.stride = std::get<4>(t);
  f.values = as_ptr<const void>(std::get<5>(t));
  f.valid = as_ptr<const uint8_t>(std::get<6>(t));
  f.out = as_ptr<void>(std::get<7>(t));
  f.out_valid = as_ptr<uint8_t>(std::get<8>(t));
  const std::string w = "window: funcs[" + std::to_string(index) + "]";
  if (f.fn < srj::WF_ROW_NUMBER || f.fn > srj::WF_AVG)
    throw std::invalid_argument(w + ": unknown function");
  if (f.frame < srj::WFR_PARTITION || f.frame > srj::WFR_RANGE)
    throw std::invalid_argument(w + ": unknown frame");
  if (f.kind < srj::WK_NONE || f.kind > srj::WK_F64)
    throw std::invalid_argument(w + ": unknown value kind");
  if (f.out == nullptr) throw std::invalid_argument(w + ": null output");
  if (std::get<7>(t) % 8 != 0 && (f.fn < srj::WF_MIN || f.fn > srj::WF_MAX))
    throw std::invalid_argument(w + ": output not aligned to 8 bytes");
  const bool needs_values = f.fn >= srj::WF_SUM;
  if (needs_values && f.kind == srj::WK_NONE)
    throw std::invalid_argument(w + ": function needs a value column");
  if (f.kind == srj::WK_NONE) {
    f.values = nullptr;
    f.stride = 1;
    f.width = 1;
    if (f.fn <= srj::WF_DENSE_RANK) f.valid = nullptr;
  } else {
    if (f.values == nullptr) throw std::invalid_argument(w + ": null values");
    if (f.width != 1 && f.width != 2 && f.width != 4 && f.width != 8)
      throw std::invalid_argument(w + ": width must be 1, 2, 4 or 8");
    if ((f.kind == srj::WK_F32 && f.width != 4) ||
        (f.kind == srj::WK_F64 && f.width != 8) ||
        (f.kind == srj::WK_BOOL && f.width != 1))
      throw std::invalid_argument(w + ": width does not match the kind");
    if (std::get<5>(t) % f.width != 0 || std::get<7>(t) % f.width != 0)
      throw std::invalid_argument(w + ": buffer not aligned to its element");
    if (f.stride < 1) throw std::invalid_argument(w + ": stride < 1");
  }
  return f;
}

}  // namespace

void register_window(py::module_& m) {
  m.attr("WINDOW_MAX_FUNCS") = srj::WINDOW_MAX_FUNCS;
  m.attr("WINDOW_SMALL_ROWS") = srj::WINDOW_SMALL_ROWS;
  m.attr("WINDOW_TILE_ROWS") = srj::WINDOW_TILE_ROWS;
  m.attr("WINDOW_CARRY_CHUNK") = srj::WINDOW_CARRY_CHUNK;
  m.def("window_work_bytes", [](int64_t rows, int32_t nfuncs) {
    return srj_window_work_bytes(rows, nfuncs);
  });
  m.def("window",
        [](const std::vector<Func>& funcs, uintptr_t perm, uintptr_t part,
           uintptr_t peer, int64_t rows, uintptr_t work, uintptr_t stream) {
          if (rows <= 0) throw std::invalid_argument("window: rows <= 0");
          // tile indices are 32-bit in the carry scan
          if (rows > (int64_t(1) << 40))
            throw std::invalid_argument("window: more than 2^40 rows");
          if (funcs.empty() || funcs.size() > (size_t)srj::WINDOW_MAX_FUNCS)
            throw std::invalid_argument(
                "window: 1..WINDOW_MAX_FUNCS functions per call");
          if (perm == 0 || part == 0)
            throw std::invalid_argument("window: null perm or flags");
          if (perm % 8 != 0)
            throw std::invalid_argument("window: perm not aligned");
          if (srj_window_work_bytes(rows, (int32_t)funcs.size()) > 0 &&
              (work == 0 || work % 8 != 0))
            throw std::invalid_argument("window: work buffer missing");
          std::vector<WinFunc> fs;
          for (size_t i = 0; i < funcs.size(); ++i)
            fs.push_back(to_func(funcs[i], i));
          srj_window(fs.data(), (int32_t)fs.size(), as_ptr<const int64_t>(perm),
                     as_ptr<const uint8_t>(part), as_ptr<const uint8_t>(peer),
                     rows, as_ptr<int64_t>(work), as_stream(stream));
          check_hip("window");
        });
}
