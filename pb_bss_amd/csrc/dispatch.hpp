// Runtime value -> template argument, once.  Host-only and free of HIP headers: each helper
// calls f with a constant (or a value of the selected type) and passes its status code through;
// a value that no compiled case serves is PBBSS_ERR_UNSUPPORTED and f is not called.
#pragma once
#include <type_traits>
#include <utility>
#include "pbbss.h"

namespace pbbss {

// f(std::integral_constant<int, V>{}) for the V among Vs... that equals v
template <int... Vs, class F>
inline int dispatch_list(int v, F&& f) {
  int rc = PBBSS_ERR_UNSUPPORTED;
  (void)(((v == Vs) && (rc = f(std::integral_constant<int, Vs>{}), true)) || ...);
  return rc;
}

template <int Lo, class F, int... Is>
inline int dispatch_offsets(int v, F&& f, std::integer_sequence<int, Is...>) {
  return dispatch_list<(Lo + Is)...>(v, std::forward<F>(f));
}

// f(std::integral_constant<int, V>{}) for Lo <= v <= Hi
template <int Lo, int Hi, class F>
inline int dispatch_range(int v, F&& f) {
  static_assert(Lo <= Hi, "empty range");
  return dispatch_offsets<Lo>(v, std::forward<F>(f), std::make_integer_sequence<int, Hi - Lo + 1>{});
}

// f(std::true_type{}) / f(std::false_type{})
template <class F>
inline int dispatch_bool(bool b, F&& f) {
  return b ? f(std::true_type{}) : f(std::false_type{});
}

// storage type of the observation: f(double{}) / f(float{})
template <class F>
inline int dispatch_real(bool is_f64, F&& f) {
  return is_f64 ? f(double{}) : f(float{});
}

}  // namespace pbbss
