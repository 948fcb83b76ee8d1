// Bindings for the window-function kernels.
#include "bind_seg_scan.hpp"

using srj::SegFunc;

extern "C" {
int64_t srj_window_work_bytes(int64_t, int32_t);
void srj_window(const SegFunc*, int32_t, const int64_t*, const uint8_t*,
                const uint8_t*, int64_t, int64_t*, hipStream_t);
}

void register_window(py::module_& m) {
  m.attr("WINDOW_MAX_FUNCS") = srj::SEG_MAX_FUNCS;
  m.attr("WINDOW_SMALL_ROWS") = srj::SEG_SMALL_ROWS;
  m.attr("WINDOW_TILE_ROWS") = srj::SEG_TILE_ROWS;
  m.attr("WINDOW_CARRY_CHUNK") = srj::SEG_CARRY_CHUNK;
  m.def("window_work_bytes", [](int64_t rows, int32_t nfuncs) {
    return srj_window_work_bytes(rows, nfuncs);
  });
  m.def("window",
        [](const std::vector<SegFuncTuple>& funcs, uintptr_t perm,
           uintptr_t part, uintptr_t peer, int64_t rows, uintptr_t work,
           uintptr_t stream) {
          if (rows <= 0) throw std::invalid_argument("window: rows <= 0");
          // tile indices are 32-bit in the carry scan
          if (rows > (int64_t(1) << 40))
            throw std::invalid_argument("window: more than 2^40 rows");
          if (funcs.empty() || funcs.size() > (size_t)srj::SEG_MAX_FUNCS)
            throw std::invalid_argument(
                "window: 1..WINDOW_MAX_FUNCS functions per call");
          if (perm == 0 || part == 0)
            throw std::invalid_argument("window: null perm or flags");
          if (perm % 8 != 0)
            throw std::invalid_argument("window: perm not aligned");
          if (srj_window_work_bytes(rows, (int32_t)funcs.size()) > 0 &&
              (work == 0 || work % 8 != 0))
            throw std::invalid_argument("window: work buffer missing");
          const std::vector<SegFunc> fs = to_seg_funcs(funcs, "window", true);
          srj_window(fs.data(), (int32_t)fs.size(), as_ptr<const int64_t>(perm),
                     as_ptr<const uint8_t>(part), as_ptr<const uint8_t>(peer),
                     rows, as_ptr<int64_t>(work), as_stream(stream));
          check_hip("window");
        });
}
