// Bindings for the rolling window kernel.
#include "bind_seg_scan.hpp"
#include "window_rolling.hpp"

using srj::RollFunc;

extern "C" {
int32_t srj_window_rolling_staged(const RollFunc*, int32_t);
void srj_window_rolling(const RollFunc*, int32_t, const int64_t*,
                        const int64_t*, const int64_t*, int64_t, hipStream_t);
}

// (the tuple of bind_seg_scan.hpp with fn = SF_COUNT..SF_AVG or RF_SHIFT,
//  lo, hi, shift)
using RollFuncTuple = std::tuple<SegFuncTuple, int64_t, int64_t, int64_t>;

static std::vector<RollFunc> to_roll_funcs(
    const std::vector<RollFuncTuple>& funcs) {
  if (funcs.empty() || funcs.size() > (size_t)srj::SEG_MAX_FUNCS)
    throw std::invalid_argument(
        "window_rolling: 1..WINDOW_MAX_FUNCS functions per call");
  std::vector<RollFunc> fs;
  for (size_t i = 0; i < funcs.size(); ++i) {
    const std::string w = "window_rolling: funcs[" + std::to_string(i) + "]";
    SegFuncTuple t = std::get<0>(funcs[i]);
    const int32_t fn = std::get<0>(t);
    const bool shift = fn == srj::RF_SHIFT;
    if (!shift && (fn < srj::SF_COUNT || fn > srj::SF_AVG))
      throw std::invalid_argument(w + ": unknown function");
    // lag / lead take what min takes: a value column of any kind, a result
    // in its dtype
    if (shift) std::get<0>(t) = srj::SF_MIN;
    std::get<1>(t) = srj::SFR_ROWS;
    RollFunc g{};
    g.f = to_seg_func(t, i, "window_rolling", true);
    g.f.fn = fn;
    g.lo = std::get<1>(funcs[i]);
    g.hi = std::get<2>(funcs[i]);
    g.shift = std::get<3>(funcs[i]);
    if (shift) {
      if (g.f.out_valid == nullptr)
        throw std::invalid_argument(w + ": lag / lead need out_valid");
      g.lo = g.hi = g.shift;
    } else {
      g.shift = 0;
    }
    if (g.lo > g.hi) throw std::invalid_argument(w + ": lo > hi");
    if (g.lo < -srj::ROLL_MAX_OFFSET || g.hi > srj::ROLL_MAX_OFFSET)
      throw std::invalid_argument(w + ": offset beyond +-(2^31 - 1)");
    fs.push_back(g);
  }
  return fs;
}

void register_window_rolling(py::module_& m) {
  m.attr("ROLL_TILE_ROWS") = srj::ROLL_TILE_ROWS;
  m.attr("ROLL_MAX_REACH") = srj::ROLL_MAX_REACH;
  m.attr("ROLL_FN_SHIFT") = srj::RF_SHIFT;
  // whether a launch of these functions takes the staged path
  m.def("window_rolling_staged", [](const std::vector<RollFuncTuple>& funcs) {
    const std::vector<RollFunc> fs = to_roll_funcs(funcs);
    return srj_window_rolling_staged(fs.data(), (int32_t)fs.size()) != 0;
  });
  m.def("window_rolling",
        [](const std::vector<RollFuncTuple>& funcs, uintptr_t perm,
           uintptr_t rn, uintptr_t pcnt, int64_t rows, uintptr_t stream) {
          if (rows <= 0)
            throw std::invalid_argument("window_rolling: rows <= 0");
          if (rows > (int64_t(1) << 40))
            throw std::invalid_argument("window_rolling: more than 2^40 rows");
          if (perm == 0 || rn == 0 || pcnt == 0)
            throw std::invalid_argument(
                "window_rolling: null perm or partition bounds");
          if (perm % 8 != 0 || rn % 8 != 0 || pcnt % 8 != 0)
            throw std::invalid_argument(
                "window_rolling: perm or partition bounds not aligned");
          const std::vector<RollFunc> fs = to_roll_funcs(funcs);
          srj_window_rolling(fs.data(), (int32_t)fs.size(),
                             as_ptr<const int64_t>(perm),
                             as_ptr<const int64_t>(rn),
                             as_ptr<const int64_t>(pcnt), rows,
                             as_stream(stream));
          check_hip("window_rolling");
        });
}
