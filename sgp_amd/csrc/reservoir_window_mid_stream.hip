// Windowed last-state reservoir (reservoir_window_impl.h): 32 < R <= 64 with a pack beyond the LDS (deep stacks
// behind a wide input: R = 64, L = 4 with more than 176 input features) -- the fragments are read from the packed
// buffer through L2, so every L R <= 256 stack still runs in one launch.
#include "reservoir_window_impl.h"

namespace sgp_win {
WinKernel resolve_mid_stream(int jt, int L) {
    return jt == 3 ? pick_layers<3, false>(L, std::make_integer_sequence<int, 8>{})
         : jt == 4 ? pick_layers<4, false>(L, std::make_integer_sequence<int, 6>{}) : nullptr;
}
}  // namespace sgp_win
