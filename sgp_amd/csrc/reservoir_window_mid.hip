// Windowed last-state reservoir (reservoir_window_impl.h): the instances for 32 < R <= 64, weights in LDS
// (their streamed twins for packs beyond the LDS: reservoir_window_mid_stream.hip).
#include "reservoir_window_impl.h"

namespace sgp_win {
WinKernel resolve_mid(int jt, int L) {
    return jt == 3 ? pick_layers<3, true>(L, std::make_integer_sequence<int, 8>{})
         : jt == 4 ? pick_layers<4, true>(L, std::make_integer_sequence<int, 6>{}) : nullptr;
}
}  // namespace sgp_win
