// Bindings for stream compaction (nonzero / fused column compaction) and the
// fused multi-column gather.
#include "srj_bind.hpp"

#include <vector>

extern "C" {
int32_t srj_compact_tile_rows();
int32_t srj_compact_max_grid();
int32_t srj_compact_scan_chunk();
int32_t srj_compact_max_cols();
void srj_compact_offsets(const uint8_t*, const uint8_t*, int64_t, int32_t*,
                         int64_t*, int64_t*, hipStream_t);
void srj_compact_nonzero(const uint8_t*, const uint8_t*, int64_t, const int64_t*,
                         int64_t*, hipStream_t);
void srj_compact_cols(const uint8_t*, const uint8_t*, int64_t, const int64_t*,
                      const void* const*, void* const*, const int32_t*, int32_t,
                      hipStream_t);
void srj_gather_cols(const int64_t*, int64_t, int64_t, const void* const*,
                     void* const*, const int32_t*, int32_t, hipStream_t);
}

namespace {

struct ColArgs {
  std::vector<const void*> srcs;
  std::vector<void*> dsts;
  std::vector<int32_t> widths;
};

// A launch carries at most compact_max_cols() descriptors by value; the
// Python layer splits wider inputs into several calls.
ColArgs col_args(const std::vector<uintptr_t>& srcs,
                 const std::vector<uintptr_t>& dsts,
                 const std::vector<int32_t>& widths, const char* what) {
  size_t nc = srcs.size();
  if (dsts.size() != nc || widths.size() != nc)
    throw std::invalid_argument(std::string(what) +
                                ": srcs/dsts/widths differ in length");
  if (nc == 0 || nc > (size_t)srj_compact_max_cols())
    throw std::invalid_argument(std::string(what) +
                                ": column count out of range");
  ColArgs a;
  for (size_t c = 0; c < nc; ++c) {
    int32_t w = widths[c];
    if (w != 1 && w != 2 && w != 4 && w != 8 && w != 16)
      throw std::invalid_argument(std::string(what) +
                                  ": width must be 1, 2, 4, 8 or 16");
    if (srcs[c] % (w == 16 ? 8 : w) != 0 || dsts[c] % (w == 16 ? 8 : w) != 0)
      throw std::invalid_argument(std::string(what) +
                                  ": buffer not aligned to its element");
    a.srcs.push_back(as_ptr<const void>(srcs[c]));
    a.dsts.push_back(as_ptr<void>(dsts[c]));
    a.widths.push_back(w);
  }
  return a;
}

}  // namespace

void register_compact(py::module_& m) {
  m.def("compact_tile_rows", [] { return srj_compact_tile_rows(); });
  m.def("compact_max_grid", [] { return srj_compact_max_grid(); });
  m.def("compact_scan_chunk", [] { return srj_compact_scan_chunk(); });
  m.def("compact_max_cols", [] { return srj_compact_max_cols(); });
  m.def("compact_offsets",
        [](uintptr_t mask, uintptr_t valid, int64_t n, uintptr_t counts,
           uintptr_t offsets, uintptr_t total, uintptr_t stream) {
          if (n <= 0) throw std::invalid_argument("compact_offsets: n <= 0");
          srj_compact_offsets(as_ptr<uint8_t>(mask), as_ptr<uint8_t>(valid), n,
                              as_ptr<int32_t>(counts), as_ptr<int64_t>(offsets),
                              as_ptr<int64_t>(total), as_stream(stream));
          check_hip("compact_offsets");
        });
  m.def("compact_nonzero",
        [](uintptr_t mask, uintptr_t valid, int64_t n, uintptr_t offsets,
           uintptr_t out, uintptr_t stream) {
          if (n <= 0) throw std::invalid_argument("compact_nonzero: n <= 0");
          srj_compact_nonzero(as_ptr<uint8_t>(mask), as_ptr<uint8_t>(valid), n,
                              as_ptr<int64_t>(offsets), as_ptr<int64_t>(out),
                              as_stream(stream));
          check_hip("compact_nonzero");
        });
  m.def("compact_cols",
        [](uintptr_t mask, uintptr_t valid, int64_t n, uintptr_t offsets,
           const std::vector<uintptr_t>& srcs,
           const std::vector<uintptr_t>& dsts,
           const std::vector<int32_t>& widths, uintptr_t stream) {
          if (n <= 0) throw std::invalid_argument("compact_cols: n <= 0");
          ColArgs a = col_args(srcs, dsts, widths, "compact_cols");
          srj_compact_cols(as_ptr<uint8_t>(mask), as_ptr<uint8_t>(valid), n,
                           as_ptr<int64_t>(offsets), a.srcs.data(),
                           a.dsts.data(), a.widths.data(),
                           (int32_t)a.widths.size(), as_stream(stream));
          check_hip("compact_cols");
        });
  m.def("gather_cols",
        [](uintptr_t map, int64_t m_rows, int64_t src_rows,
           const std::vector<uintptr_t>& srcs,
           const std::vector<uintptr_t>& dsts,
           const std::vector<int32_t>& widths, uintptr_t stream) {
          if (m_rows <= 0) throw std::invalid_argument("gather_cols: m <= 0");
          ColArgs a = col_args(srcs, dsts, widths, "gather_cols");
          srj_gather_cols(as_ptr<int64_t>(map), m_rows, src_rows, a.srcs.data(),
                          a.dsts.data(), a.widths.data(),
                          (int32_t)a.widths.size(), as_stream(stream));
          check_hip("gather_cols");
        });
}
