// Bindings for the packed-key sort order and the key-change flags.
#include "srj_bind.hpp"
#include "sort_order.hpp"

#include <tuple>
#include <vector>

using srj::SortKey;

extern "C" {
int64_t srj_sort_order_work_words(int64_t);
void srj_key_change_flags(const SortKey*, int32_t, const int64_t*, int64_t,
                          int64_t, uint8_t*, hipStream_t);
void srj_sort_order(const SortKey*, const int32_t*, const int32_t*, int32_t,
                    int64_t, int64_t*, int64_t*, hipStream_t);
}

namespace {

// (data, valid, stride, kind, width, bits, shift, flags)
using Field = std::tuple<uintptr_t, uintptr_t, int64_t, int32_t, int32_t,
                         int32_t, int32_t, int32_t>;

SortKey to_key(const Field& f, const char* what) {
  SortKey k{};
  k.data = as_ptr<const void>(std::get<0>(f));
  k.valid = as_ptr<const uint8_t>(std::get<1>(f));
  k.stride = std::get<2>(f);
  k.kind = std::get<3>(f);
  k.width = std::get<4>(f);
  k.bits = std::get<5>(f);
  k.shift = std::get<6>(f);
  k.flags = std::get<7>(f);
  const std::string w(what);
  if (k.kind < srj::SK_UINT || k.kind > srj::SK_NULL)
    throw std::invalid_argument(w + ": unknown field kind");
  if (k.width != 1 && k.width != 2 && k.width != 4 && k.width != 8)
    throw std::invalid_argument(w + ": width must be 1, 2, 4 or 8");
  if (k.kind == srj::SK_NULL) {
    if (k.valid == nullptr)
      throw std::invalid_argument(w + ": null field without validity");
    k.bits = 1;
    k.flags &= ~srj::SF_NULL_BIT;
  } else {
    if (k.data == nullptr) throw std::invalid_argument(w + ": null data");
    if (std::get<0>(f) % k.width != 0)
      throw std::invalid_argument(w + ": buffer not aligned to its element");
    if ((k.kind == srj::SK_F32 && k.width != 4) ||
        (k.kind == srj::SK_F64 && k.width != 8) ||
        (k.kind == srj::SK_BOOL && k.width != 1))
      throw std::invalid_argument(w + ": width does not match the kind");
    if (k.bits < 1 || k.bits > 8 * k.width)
      throw std::invalid_argument(w + ": bits out of range");
  }
  if (k.stride < 1) throw std::invalid_argument(w + ": stride < 1");
  int32_t span = k.bits + ((k.flags & srj::SF_NULL_BIT) ? 1 : 0);
  if ((k.flags & srj::SF_NULL_BIT) && k.valid == nullptr)
    throw std::invalid_argument(w + ": null bit without validity");
  if (k.shift < 0 || k.shift + span > 64)
    throw std::invalid_argument(w + ": field does not fit its word");
  return k;
}

}  // namespace

void register_sort_order(py::module_& m) {
  m.def("sort_order_work_words",
        [](int64_t n) { return srj_sort_order_work_words(n); });
  // words: least significant first; each a list of fields
  m.def("sort_order",
        [](const std::vector<std::vector<Field>>& words, int64_t n,
           uintptr_t work, uintptr_t out, uintptr_t stream) {
          if (n <= 0) throw std::invalid_argument("sort_order: n <= 0");
          if (words.empty()) throw std::invalid_argument("sort_order: no keys");
          std::vector<SortKey> keys;
          std::vector<int32_t> begin{0}, bits;
          for (const auto& w : words) {
            if (w.empty())
              throw std::invalid_argument("sort_order: empty word");
            int32_t used = 0;
            for (const auto& f : w) {
              SortKey k = to_key(f, "sort_order");
              int32_t top =
                  k.shift + k.bits + ((k.flags & srj::SF_NULL_BIT) ? 1 : 0);
              used = top > used ? top : used;
              keys.push_back(k);
            }
            begin.push_back((int32_t)keys.size());
            bits.push_back(used);
          }
          srj_sort_order(keys.data(), begin.data(), bits.data(),
                         (int32_t)words.size(), n, as_ptr<int64_t>(work),
                         as_ptr<int64_t>(out), as_stream(stream));
          check_hip("sort_order");
        });
  m.def("key_change_flags",
        [](const std::vector<Field>& fields, uintptr_t perm, int64_t n,
           int64_t nrows, uintptr_t out, uintptr_t stream) {
          if (n <= 0 || nrows <= 0)
            throw std::invalid_argument("key_change_flags: n <= 0");
          std::vector<SortKey> keys;
          for (const auto& f : fields) {
            SortKey k = to_key(f, "key_change_flags");
            k.shift = 0;
            keys.push_back(k);
          }
          srj_key_change_flags(keys.data(), (int32_t)keys.size(),
                               as_ptr<int64_t>(perm), n, nrows,
                               as_ptr<uint8_t>(out), as_stream(stream));
          check_hip("key_change_flags");
        });
}
