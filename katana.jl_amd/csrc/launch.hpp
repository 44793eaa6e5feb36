// launch.hpp -- every kernel launch goes through here: the two entry points, the grid rules, and the run-time -> compile-time
// selection of a kernel's template arguments (G lanes per output first of all).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <type_traits>

#include "common.hpp"
#include "types.hpp"

namespace ktn {

// ---- grid rules (workgroups of kBlock threads); a count <= 0 gives 0 workgroups, which the launchers skip
inline unsigned grid_n(int64_t count) { return count > 0 ? (unsigned)ceil_div(count, kBlock) : 0u; }               // a thread per item
inline unsigned group_grid(int64_t count, int G, int T = 1) {                                                      // G lanes per T outputs
    return count > 0 ? (unsigned)ceil_div(count * G, kBlock * T) : 0u;
}
// G lanes per output, then one trailing workgroup per long output
inline unsigned group_grid_long(int64_t count, int G, int64_t n_long) { return group_grid(count, G) + (unsigned)n_long; }

// ---- the two entry points.  A site keeps the one it has: the Ext one where a launch can carry the kernel's own start / stop
// events (null outside profile mode), the plain one everywhere else.  A zero-size grid is skipped.
template <class... P, class... A>
inline void launch(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, A&&... args) {
    if (grid.x == 0) return;
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, static_cast<P>(args)...);
}

template <class... P, class... A>
inline void launch_ev(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, hipEvent_t e0, hipEvent_t e1,
                      A&&... args) {
    if (grid.x == 0) return;
    hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, stream, e0, e1, 0, static_cast<P>(args)...);
}

// the sites that are timed in profile mode only: the plain entry point without events, the Ext one with either of them
template <class... P, class... A>
inline void launch_timed(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, hipEvent_t e0, hipEvent_t e1,
                         A&&... args) {
    if (e0 || e1) launch_ev(kernel, grid, block, lds, stream, e0, e1, args...);
    else launch(kernel, grid, block, lds, stream, args...);
}

// a thread per item, kBlock threads per workgroup
template <class... P, class... A>
inline void launch_n(void (*kernel)(P...), int64_t count, hipStream_t stream, A&&... args) {
    launch(kernel, grid_n(count), kBlock, 0, stream, args...);
}

// ---- f(std::integral_constant<., V>) for the V of the list that equals v; the LAST entry is the fallback for any other v.
// (`auto`, not `void`: a deduced return type makes the compiler instantiate these where they are called and not at the end of
//  the translation unit, so a unit's kernels are emitted in the order its launches are written.)
template <auto V0, auto... Vs, class T, class F>
inline auto with_value(T v, F&& f) {
    if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<decltype(V0), V0>{});
    else if (v == (T)V0) f(std::integral_constant<decltype(V0), V0>{});
    else with_value<Vs...>(v, f);
}

// lanes per output: with_group(G, [&](auto g) { launch(k<g()>, group_grid(count, g()), kBlock, 0, stream, ...); })
template <class F>
inline auto with_group(int G, F&& f) { with_value<4, 8, 16, 32, 64>(G, f); }

template <class F>
inline auto with_bool(bool b, F&& f) { with_value<true, false>(b, f); }

}  // namespace ktn
