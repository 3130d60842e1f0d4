// sph_select.h -- run-time choices -> template arguments, for the kernel launchers.
//
// A launcher turns its run-time selectors (one type or several, the block shape, the force
// mode ...) into the template arguments of one kernel.  Each helper here turns ONE run-time
// value into a compile-time constant and calls a generic lambda with it; a launcher nests
// them, innermost the single hipLaunchKernelGGL that names the kernel and its argument list:
//
//   select_bool(nt1, [&](auto n) {
//     constexpr bool NT1 = n;
//     select_int<M_HEAT, M_TAIT, M_GAS>(mode, [&](auto m) {
//       constexpr int MODE = m;
//       hipLaunchKernelGGL((k<NT1, MODE>), ...);
//     });
//   });
//
// Every combination the lambdas can reach is instantiated, so a combination that must not
// exist is mapped to one that does with a constexpr expression, or left out with
// `if constexpr`, inside the lambda.  Plain C++17: no HIP, a host compiler builds it alone.
#pragma once
#include <type_traits>

namespace sph {

// Study builds (make STUDY=1) hold measurement variants whose outputs are meaningless; a
// launcher admits them under `if constexpr (STUDY_BUILD && ...)`, so the shipped library
// does not contain them.
#ifdef SPH_STUDY
constexpr bool STUDY_BUILD = true;
#else
constexpr bool STUDY_BUILD = false;
#endif

// f(std::true_type{}) or f(std::false_type{})
template <class F>
inline void select_bool(bool b, F &&f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}

// f(std::integral_constant<int, v>{}) for v among V...; every other value takes FALLBACK
// (which may be one of V..., or a value the lambda refuses)
template <int FALLBACK, int... V, class F>
inline void select_int(int v, F &&f) {
  const bool listed = ((v == V ? (f(std::integral_constant<int, V>{}), true) : false) || ...);
  if (!listed) f(std::integral_constant<int, FALLBACK>{});
}

// the constants of one entry of a shape table: Dims<R, G, U>::v[] = {R, G, U}
template <int... V>
struct Dims {
  static constexpr int v[sizeof...(V)] = {V...};
};

// SPH_SHAPE_SELECT(name, TABLE) defines `bool name(int k, F &&f)` over the X-macro table
// TABLE(X) = X(k0, dims...) X(k1, dims...) ..., which stays the one place where the shapes
// are listed: f(Dims<dims...>{}) of the entry with index k and true, or false (f not called)
// when no entry has that index -- the caller names its fall-back there.
#define SPH_SHAPE_CASE_(k, ...) \
  case k: f(::sph::Dims<__VA_ARGS__>{}); return true;
#define SPH_SHAPE_SELECT(name, TABLE)      \
  template <class F>                       \
  inline bool name(int k, F &&f) {         \
    switch (k) {                           \
      TABLE(SPH_SHAPE_CASE_)               \
      default: return false;               \
    }                                      \
  }

}  // namespace sph
