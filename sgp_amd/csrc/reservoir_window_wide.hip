// Windowed last-state reservoir (reservoir_window_impl.h): the instances for 64 < R <= 256.  Their weights (64 KB of
// W_hh per layer at R = 128, 256 KB at R = 256) do not fit the LDS beside anything else: every wave reads the fragments
// from the packed buffer, which the whole launch shares in L2.
#include "reservoir_window_impl.h"

namespace sgp_win {
WinKernel resolve_wide(int jt, int L) {
    return jt == 8 ? pick_layers<8, false>(L, std::make_integer_sequence<int, 3>{})
         : jt == 16 ? pick_layers<16, false>(L, std::make_integer_sequence<int, 1>{}) : nullptr;
}
}  // namespace sgp_win
