// Run-time values that select a kernel instantiation: f gets them as integral constants (a generic lambda takes `auto d`
// and reads `constexpr int DEG = d;`).  Host side of the launchers only.
#pragma once
#include <type_traits>

namespace gsr {
template <class F>
inline void dispatch_degree(int degree, F&& f) {
    switch (degree) {
        case 0: f(std::integral_constant<int, 0>{}); break;
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        default: f(std::integral_constant<int, 3>{}); break;
    }
}
template <class F>
inline void dispatch_bool(bool b, F&& f) {
    if (b) f(std::true_type{}); else f(std::false_type{});
}
// the channel counts of the three modes gsr_create admits: :rgb 3, :rgbd 5, :rgbdn 8
template <class F>
inline void dispatch_channels(int channels, F&& f) {
    switch (channels) {
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 5: f(std::integral_constant<int, 5>{}); break;
        default: f(std::integral_constant<int, 8>{}); break;
    }
}
}  // namespace gsr
