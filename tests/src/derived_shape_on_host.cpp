// derived_shape_on_host.cpp -- csrc/hmpc_derived_shape.h on the CPU (tests/test_derived_shape_on_host.py): the one rule from (contacts,
// horizon) to the (HMAX, NC) instantiation of the kernels launched behind a solve, and the dispatcher the launchers call, each against
// the table written here.
#include <stdio.h>

#include <type_traits>

#include "hmpc_derived_shape.h"

static int problems = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      ++problems;                              \
      printf("FAILED %s: ", #cond);            \
      printf(__VA_ARGS__);                     \
      printf("\n");                            \
    }                                          \
  } while (0)

struct Want {
  int shape, hmax, nc;  // shape < 0: unsupported
};
// (2, 1 .. 10) -> <10, 2>, (2, 11 .. 20) -> <20, 2>, (3, 1 .. 10) -> <10, 3>, nothing else
static Want want(int nc, int horizon) {
  if (nc == 2 && horizon >= 1 && horizon <= 10) return {0, 10, 2};
  if (nc == 2 && horizon >= 11 && horizon <= 20) return {1, 20, 2};
  if (nc == 3 && horizon >= 1 && horizon <= 10) return {2, 10, 3};
  return {-1, 0, 0};
}

// the rule is usable where a constant is needed
static_assert(hmpc::derived_shape(2, 10) == 0 && hmpc::derived_shape(2, 11) == 1 && hmpc::derived_shape(3, 10) == 2 &&
                  hmpc::derived_shape(3, 11) == -1,
              "constexpr");

int main() {
  constexpr int INVALID = 1, OK = 0;  // (what the launchers pass: hipErrorInvalidValue, and hipGetLastError() of a launch that went out)
  const int horizons[] = {0, 1, 10, 11, 20, 21};
  int supported = 0;
  for (int nc = 0; nc <= 4; ++nc)
    for (int horizon : horizons) {
      const Want w = want(nc, horizon);
      CHECK(hmpc::derived_shape(nc, horizon) == w.shape, "nc %d horizon %d: shape %d, want %d", nc, horizon, hmpc::derived_shape(nc, horizon),
            w.shape);
      int calls = 0, got_h = -1, got_c = -1;
      const int rc = hmpc::for_derived_shape(nc, horizon, INVALID, [&](auto H, auto C) {
        static_assert(std::is_same<decltype(H), std::integral_constant<int, H()>>::value, "HMAX arrives as a constant");
        static_assert(std::is_same<decltype(C), std::integral_constant<int, C()>>::value, "NC arrives as a constant");
        ++calls, got_h = H(), got_c = C();
        return OK;
      });
      if (w.shape < 0) {
        CHECK(calls == 0 && rc == INVALID, "nc %d horizon %d: %d calls, returned %d", nc, horizon, calls, rc);
      } else {
        ++supported;
        CHECK(calls == 1 && rc == OK && got_h == w.hmax && got_c == w.nc, "nc %d horizon %d: %d calls <%d, %d> returned %d, want <%d, %d>", nc,
              horizon, calls, got_h, got_c, rc, w.hmax, w.nc);
        CHECK(hmpc::DERIVED_SHAPES[w.shape].hmax == w.hmax && hmpc::DERIVED_SHAPES[w.shape].nc == w.nc, "row %d of DERIVED_SHAPES", w.shape);
      }
      // what the callable returns comes back as it is (a launch error reaches the caller)
      const int passed = hmpc::for_derived_shape(nc, horizon, INVALID, [&](auto, auto) { return 7; });
      CHECK(passed == (w.shape < 0 ? INVALID : 7), "nc %d horizon %d: returned %d", nc, horizon, passed);
    }
  CHECK(supported == 2 + 2 + 2, "%d supported points of the grid", supported);
  CHECK(hmpc::N_DERIVED_SHAPES == 3 && hmpc::DERIVED_NT == 128, "%d shapes, %d threads", hmpc::N_DERIVED_SHAPES, hmpc::DERIVED_NT);
  printf("%d problems\n", problems);
  return problems != 0;
}
