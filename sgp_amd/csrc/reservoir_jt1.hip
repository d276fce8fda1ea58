// Instantiations of the reservoir layer kernel for 16-wide (padded) reservoirs.
#include "reservoir_impl.h"
namespace sgp_res {
ResKernel resolve_jt1(const ResPart& p, int nkx) { return resolve_nkx<1>(p, nkx); }
}
