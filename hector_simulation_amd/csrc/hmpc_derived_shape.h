// hmpc_derived_shape.h -- THE shape rule of the kernels launched behind a solve (hmpc_derived.h): which (HMAX, NC) instantiation serves a
// handle of `nc` contacts and `horizon` steps, or that none does.  Plain functions of plain values, like hmpc_plan.h: no HIP, so that
// tests/src/derived_shape_on_host.cpp compiles this header for the CPU and checks the rule and the dispatcher.  A new shape is one row of
// DERIVED_SHAPES, one arm of derived_shape and one case of for_derived_shape; no launcher changes.
#pragma once
#include <type_traits>
#include <utility>

#pragma GCC visibility push(hidden)  // (the inline functions of this header are no exports of the library)

namespace hmpc {

// threads per workgroup of every derived kernel, one workgroup per instance: stage_a_scalars needs lanes of two waves.  (Here and not in
// hmpc_derived.h so that the families' own constants -- PREDICT_NT, FB_NT, ... -- can name it in headers that compile without the kernel.)
constexpr int DERIVED_NT = 128;

struct DerivedShape {
  int hmax, nc;
};
// two contacts up to ten steps, two contacts up to twenty, three contacts up to ten
inline constexpr DerivedShape DERIVED_SHAPES[] = {{10, 2}, {20, 2}, {10, 3}};
constexpr int N_DERIVED_SHAPES = sizeof(DERIVED_SHAPES) / sizeof(DERIVED_SHAPES[0]);

// the index into DERIVED_SHAPES of the smallest shape that holds (nc, horizon), or -1: no kernel is instantiated for it.  (The launchers
// turn horizon < 1 away with their other argument checks before they ask; the rule says the same.)
constexpr int derived_shape(int nc, int horizon) {
  if (horizon < 1) return -1;
  if (nc == 2 && horizon <= 10) return 0;
  if (nc == 2 && horizon <= 20) return 1;
  if (nc == 3 && horizon <= 10) return 2;
  return -1;
}

// f(std::integral_constant<int, HMAX>, std::integral_constant<int, NC>) of the shape of (nc, horizon), once, and what it returns; for an
// unsupported shape f is not called and the answer is `invalid`
template <class E, class F>
E for_derived_shape(int nc, int horizon, E invalid, F &&f) {
  using std::integral_constant;
  switch (derived_shape(nc, horizon)) {
    case 0: return f(integral_constant<int, DERIVED_SHAPES[0].hmax>{}, integral_constant<int, DERIVED_SHAPES[0].nc>{});
    case 1: return f(integral_constant<int, DERIVED_SHAPES[1].hmax>{}, integral_constant<int, DERIVED_SHAPES[1].nc>{});
    case 2: return f(integral_constant<int, DERIVED_SHAPES[2].hmax>{}, integral_constant<int, DERIVED_SHAPES[2].nc>{});
    default: return invalid;
  }
}
static_assert(N_DERIVED_SHAPES == 3, "one case of for_derived_shape per row of DERIVED_SHAPES");

}  // namespace hmpc

#pragma GCC visibility pop
