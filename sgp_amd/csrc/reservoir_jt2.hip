// Instantiations of the reservoir layer kernel for 32-wide (padded) reservoirs.
#include "reservoir_impl.h"
namespace sgp_res {
ResKernel resolve_jt2(const ResPart& p, int nkx) { return resolve_nkx<2>(p, nkx); }
}
