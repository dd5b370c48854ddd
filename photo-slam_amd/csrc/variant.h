// variant.h -- run-time flags to template arguments.  Every optional feature of a hot kernel is a template parameter, an
// instantiation of its own.  A launcher names the kernel ONCE, inside a generic lambda that these helpers call with
// the run-time values as types, and asks the kernel family's constexpr predicate -- written next to its template <...> line, the
// one statement of which instantiations exist -- whether to instantiate it:
//   return with_flags([&](auto dp, auto ab) -> int {
//       constexpr bool DEPTH = decltype(dp)::value, ABS = decltype(ab)::value, EXISTS = my_kernel_variant(DEPTH, ABS);
//       if constexpr (EXISTS) GSR_LAUNCH((my_kernel<DEPTH, ABS>), grid, block, stream, p);
//       return EXISTS ? GSR_OK : GSR_ERR_UNSUPPORTED;
//   }, p.depth != 0, p.abs_sums != 0);
// The launcher refuses the other combinations in front of its first launch.  Plain C++17, no HIP: the emulator build compiles it as is.
#pragma once
#include <type_traits>

namespace gsr {

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...) -> int
template <class F>
inline int with_flags(F&& f)
{
	return f();
}
template <class F, class... Rest>
inline int with_flags(F&& f, bool b0, Rest... rest)
{
	auto bound = [&](auto c0) { return with_flags([&](auto... cs) { return f(c0, cs...); }, rest...); };
	return b0 ? bound(std::true_type{}) : bound(std::false_type{});
}

// f(std::integral_constant<int, v>{}) -> int for Lo <= v <= Hi; `outside` for any other v
template <int Lo, int Hi, class F>
inline int with_int(F&& f, int v, int outside)
{
	if constexpr (Lo > Hi) return outside;
	else return v == Lo ? f(std::integral_constant<int, Lo>{}) : with_int<Lo + 1, Hi>(f, v, outside);
}

}  // namespace gsr
