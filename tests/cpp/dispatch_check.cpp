// Stand-alone check of csrc/dispatch.hpp (host-only, C++17): built and run by
// tests/test_host_logic.py::test_dispatch_helpers_reach_every_case.  Exit status 0 = all passed.
#include <cstdio>
#include <type_traits>
#include "dispatch.hpp"

static int failures = 0;
#define CHECK(...)                                                   \
  do {                                                               \
    if (!(__VA_ARGS__)) {                                            \
      std::printf("%s:%d: %s\n", __FILE__, __LINE__, #__VA_ARGS__);  \
      ++failures;                                                    \
    }                                                                \
  } while (0)

template <int V>
struct Tag {
  static constexpr int value = V;
};

int main() {
  using namespace pbbss;
  // every value of a range reaches the lambda with the matching CONSTANT; its code comes back
  for (int v = 2; v <= 8; ++v) {
    int calls = 0, seen = -1;
    const int rc = dispatch_range<2, 8>(v, [&](auto d) {
      ++calls;
      seen = Tag<d()>::value;  // usable as a template argument
      return 100 + decltype(d)::value;
    });
    CHECK(calls == 1 && seen == v && rc == 100 + v);
  }
  // just outside (and far outside): PBBSS_ERR_UNSUPPORTED, the lambda is not called
  for (int v : {1, 9, 0, -1, -2, 1 << 30}) {
    int calls = 0;
    CHECK(dispatch_range<2, 8>(v, [&](auto) { return ++calls; }) == PBBSS_ERR_UNSUPPORTED);
    CHECK(calls == 0);
  }
  // one-element range, and a range that starts below zero
  CHECK(dispatch_range<3, 3>(3, [](auto k) { return (int)k(); }) == 3);
  CHECK(dispatch_range<3, 3>(2, [](auto) { return 0; }) == PBBSS_ERR_UNSUPPORTED);
  CHECK(dispatch_range<3, 3>(4, [](auto) { return 0; }) == PBBSS_ERR_UNSUPPORTED);
  CHECK(dispatch_range<-1, 1>(-1, [](auto k) { return 10 + k(); }) == 9);
  // a status that happens to equal PBBSS_ERR_UNSUPPORTED is passed through after ONE call
  {
    int calls = 0;
    CHECK(dispatch_range<1, 6>(4, [&](auto) { ++calls; return PBBSS_ERR_UNSUPPORTED; }) ==
          PBBSS_ERR_UNSUPPORTED);
    CHECK(calls == 1);
  }
  // list form: members only
  for (int v = 0; v <= 40; ++v) {
    int calls = 0, seen = -1;
    const int rc = dispatch_list<10, 16, 36>(v, [&](auto n) {
      ++calls;
      seen = Tag<n()>::value;
      return PBBSS_ERR_HIP;
    });
    const bool member = v == 10 || v == 16 || v == 36;
    CHECK(calls == (member ? 1 : 0));
    CHECK(rc == (member ? PBBSS_ERR_HIP : PBBSS_ERR_UNSUPPORTED));
    CHECK(!member || seen == v);
  }
  // bool and storage-type dispatchers
  CHECK(dispatch_bool(true, [](auto b) { return b() ? 7 : 8; }) == 7);
  CHECK(dispatch_bool(false, [](auto b) { return b() ? 7 : 8; }) == 8);
  CHECK(dispatch_bool(true, [](auto b) { return (int)std::is_same<decltype(b), std::true_type>::value; }) == 1);
  CHECK(dispatch_real(true, [](auto y) { return (int)sizeof(y); }) == 8);
  CHECK(dispatch_real(false, [](auto y) { return (int)sizeof(y); }) == 4);
  CHECK(dispatch_real(1, [](auto y) { return std::is_same<decltype(y), double>::value ? PBBSS_ERR_HIP : 0; }) == PBBSS_ERR_HIP);
  CHECK(dispatch_real(0, [](auto y) { return std::is_same<decltype(y), float>::value ? PBBSS_ERR_INTERNAL : 0; }) == PBBSS_ERR_INTERNAL);
  // nested, as the launch sites use them
  {
    int D = 0, K = 0, bytes = 0;
    const int rc = dispatch_range<2, 8>(5, [&](auto d) {
      return dispatch_real(true, [&](auto y) {
        return dispatch_range<1, 6>(6, [&](auto k) {
          D = d(), K = k(), bytes = (int)sizeof(y);
          return PBBSS_OK;
        });
      });
    });
    CHECK(rc == PBBSS_OK && D == 5 && K == 6 && bytes == 8);
    CHECK(dispatch_range<2, 8>(5, [&](auto) {
            return dispatch_range<1, 6>(7, [&](auto) { return PBBSS_OK; });
          }) == PBBSS_ERR_UNSUPPORTED);
  }
  if (failures) std::printf("%d check(s) failed\n", failures);
  return failures ? 1 : 0;
}
