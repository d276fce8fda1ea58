// Instantiations of the reservoir layer kernel for 64-wide (padded) reservoirs.
#include "reservoir_impl.h"
namespace sgp_res {
ResKernel resolve_jt4(const ResPart& p, int nkx) { return resolve_nkx<4>(p, nkx); }
}
