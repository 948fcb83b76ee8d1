// Bindings for the segmented-reduce kernels.
#include "bind_seg_scan.hpp"

using srj::SegFunc;

extern "C" {
int64_t srj_seg_reduce_work_bytes(int64_t, int32_t);
void srj_seg_reduce(const SegFunc*, int32_t, const int64_t*, const uint8_t*,
                    int64_t, int64_t, int64_t, int64_t*, int64_t*, int64_t*,
                    hipStream_t);
}

void register_seg_reduce(py::module_& m) {
  m.attr("SEG_MAX_FUNCS") = srj::SEG_MAX_FUNCS;
  m.attr("SEG_SMALL_ROWS") = srj::SEG_SMALL_ROWS;
  m.attr("SEG_TILE_ROWS") = srj::SEG_TILE_ROWS;
  m.attr("SEG_CARRY_CHUNK") = srj::SEG_CARRY_CHUNK;
  m.def("seg_reduce_work_bytes", [](int64_t rows, int32_t nfuncs) {
    return srj_seg_reduce_work_bytes(rows, nfuncs);
  });
  m.def("seg_reduce",
        [](const std::vector<SegFuncTuple>& funcs, uintptr_t perm,
           uintptr_t head, int64_t rows, int64_t value_rows, int64_t num_out,
           uintptr_t first_rows, uintptr_t count, uintptr_t work,
           uintptr_t stream) {
          if (rows <= 0) throw std::invalid_argument("seg_reduce: rows <= 0");
          if (rows > (int64_t(1) << 40))
            throw std::invalid_argument("seg_reduce: more than 2^40 rows");
          if (value_rows < 0 || num_out < 0)
            throw std::invalid_argument("seg_reduce: negative size");
          if (funcs.size() > (size_t)srj::SEG_MAX_FUNCS)
            throw std::invalid_argument(
                "seg_reduce: at most SEG_MAX_FUNCS functions per call");
          if (head == 0) throw std::invalid_argument("seg_reduce: null flags");
          if (count == 0 || count % 8 != 0)
            throw std::invalid_argument("seg_reduce: count missing");
          if (perm % 8 != 0 || first_rows % 8 != 0)
            throw std::invalid_argument("seg_reduce: buffer not aligned");
          if (num_out > 0 && first_rows == 0)
            throw std::invalid_argument("seg_reduce: null first_rows");
          if (srj_seg_reduce_work_bytes(rows, (int32_t)funcs.size()) > 0 &&
              (work == 0 || work % 8 != 0))
            throw std::invalid_argument("seg_reduce: work buffer missing");
          // the ranking functions are the window's alone
          const std::vector<SegFunc> fs =
              to_seg_funcs(funcs, "seg_reduce", false);
          srj_seg_reduce(fs.data(), (int32_t)fs.size(),
                         as_ptr<const int64_t>(perm),
                         as_ptr<const uint8_t>(head), rows, value_rows,
                         num_out, as_ptr<int64_t>(first_rows),
                         as_ptr<int64_t>(count), as_ptr<int64_t>(work),
                         as_stream(stream));
          check_hip("seg_reduce");
        });
}
