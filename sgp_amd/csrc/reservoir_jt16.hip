// Instantiations of the reservoir layer kernel for 256-wide (padded) reservoirs.
#include "reservoir_impl.h"
namespace sgp_res {
ResKernel resolve_jt16(const ResPart& p, int nkx) { return resolve_nkx<16>(p, nkx); }
}
