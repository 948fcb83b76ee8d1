// Bindings for the segmented-reduce kernels.
#include "srj_bind.hpp"
#include "seg_reduce.hpp"

#include <tuple>
#include <vector>

using srj::SegFunc;

extern "C" {
int64_t srj_seg_reduce_work_bytes(int64_t, int32_t);
void srj_seg_reduce(const SegFunc*, int32_t, const int64_t*, const uint8_t*,
                    int64_t, int64_t, int64_t, int64_t*, int64_t*, int64_t*,
                    hipStream_t);
}

namespace {

// (fn, kind, width, stride, values, valid, out, out_valid)
using Func = std::tuple<int32_t, int32_t, int32_t, int64_t, uintptr_t,
                        uintptr_t, uintptr_t, uintptr_t>;

SegFunc to_func(const Func& t, size_t index) {
  SegFunc f{};
  f.fn = std::get<0>(t);
  f.kind = std::get<1>(t);
  f.width = std::get<2>(t);
  f.stride = std::get<3>(t);
  f.values = as_ptr<const void>(std::get<4>(t));
  f.valid = as_ptr<const uint8_t>(std::get<5>(t));
  f.out = as_ptr<void>(std::get<6>(t));
  f.out_valid = as_ptr<uint8_t>(std::get<7>(t));
  const std::string w = "seg_reduce: funcs[" + std::to_string(index) + "]";
  if (f.fn < srj::SR_COUNT || f.fn > srj::SR_AVG)
    throw std::invalid_argument(w + ": unknown function");
  if (f.kind < srj::SRK_NONE || f.kind > srj::SRK_F64)
    throw std::invalid_argument(w + ": unknown value kind");
  if (f.out == nullptr) throw std::invalid_argument(w + ": null output");
  if (std::get<6>(t) % 8 != 0 && (f.fn < srj::SR_MIN || f.fn > srj::SR_MAX))
    throw std::invalid_argument(w + ": output not aligned to 8 bytes");
  if (f.fn != srj::SR_COUNT && f.kind == srj::SRK_NONE)
    throw std::invalid_argument(w + ": function needs a value column");
  if (f.kind == srj::SRK_NONE) {
    f.values = nullptr;
    f.stride = 1;
    f.width = 1;
  } else {
    if (f.values == nullptr) throw std::invalid_argument(w + ": null values");
    if (f.width != 1 && f.width != 2 && f.width != 4 && f.width != 8)
      throw std::invalid_argument(w + ": width must be 1, 2, 4 or 8");
    if ((f.kind == srj::SRK_F32 && f.width != 4) ||
        (f.kind == srj::SRK_F64 && f.width != 8) ||
        (f.kind == srj::SRK_BOOL && f.width != 1))
      throw std::invalid_argument(w + ": width does not match the kind");
    if (std::get<4>(t) % f.width != 0 || std::get<6>(t) % f.width != 0)
      throw std::invalid_argument(w + ": buffer not aligned to its element");
    if (f.stride < 1) throw std::invalid_argument(w + ": stride < 1");
  }
  return f;
}

}  // namespace

void register_seg_reduce(py::module_& m) {
  m.attr("SEG_MAX_FUNCS") = srj::SEG_MAX_FUNCS;
  m.attr("SEG_SMALL_ROWS") = srj::SEG_SMALL_ROWS;
  m.attr("SEG_TILE_ROWS") = srj::SEG_TILE_ROWS;
  m.attr("SEG_CARRY_CHUNK") = srj::SEG_CARRY_CHUNK;
  m.def("seg_reduce_work_bytes", [](int64_t rows, int32_t nfuncs) {
    return srj_seg_reduce_work_bytes(rows, nfuncs);
  });
  m.def("seg_reduce",
        [](const std::vector<Func>& funcs, uintptr_t perm, uintptr_t head,
           int64_t rows, int64_t value_rows, int64_t num_out,
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
          std::vector<SegFunc> fs;
          for (size_t i = 0; i < funcs.size(); ++i)
            fs.push_back(to_func(funcs[i], i));
          srj_seg_reduce(fs.data(), (int32_t)fs.size(),
                         as_ptr<const int64_t>(perm),
                         as_ptr<const uint8_t>(head), rows, value_rows,
                         num_out, as_ptr<int64_t>(first_rows),
                         as_ptr<int64_t>(count), as_ptr<int64_t>(work),
                         as_stream(stream));
          check_hip("seg_reduce");
        });
}
