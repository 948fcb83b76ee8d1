// Bindings for the sort-merge join.
#include "srj_bind.hpp"

extern "C" {
void srj_merge_join(const int64_t*, const int64_t*, int64_t, const int64_t*,
                    const uint8_t*, int64_t, uint64_t*, int32_t*, int64_t*,
                    int64_t, int32_t, hipStream_t);
}

void register_sort(py::module_& m) {
  m.def("merge_join", [](uintptr_t build_sorted, uintptr_t build_rows,
                         int64_t nbuild, uintptr_t probe, uintptr_t pvalid,
                         int64_t nprobe, uintptr_t counter, uintptr_t out_build,
                         uintptr_t out_probe, int64_t out_capacity, int32_t fill,
                         uintptr_t stream) {
    srj_merge_join(as_ptr<int64_t>(build_sorted), as_ptr<int64_t>(build_rows),
                   nbuild, as_ptr<int64_t>(probe), as_ptr<uint8_t>(pvalid), nprobe,
                   as_ptr<uint64_t>(counter), as_ptr<int32_t>(out_build),
                   as_ptr<int64_t>(out_probe), out_capacity, fill,
                   as_stream(stream));
    check_hip("merge_join");
  });
}
