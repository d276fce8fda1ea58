// Instantiations of the reservoir layer kernel for 128-wide (padded) reservoirs.
#include "reservoir_impl.h"
namespace sgp_res {
ResKernel resolve_jt8(const ResPart& p, int nkx) { return resolve_nkx<8>(p, nkx); }
}
