// Instantiations of the streamed-weights reservoir kernel (R = 256: 16 output tiles, and
// R = 128 with F = 256, the one 8-tile shape whose weights exceed the LDS), one
// translation unit of its own so that it builds in parallel with reservoir_jt16.hip.
#define SGP_RES_STREAM_TU
#include "reservoir_impl.h"
namespace sgp_res {
template <> ResKernel resolve_stream_ool<8, 64>(const ResPart& p) { return resolve_stream<8, 64>(p); }
template <> ResKernel resolve_stream_ool<16, 4>(const ResPart& p) { return resolve_stream<16, 4>(p); }
template <> ResKernel resolve_stream_ool<16, 8>(const ResPart& p) { return resolve_stream<16, 8>(p); }
template <> ResKernel resolve_stream_ool<16, 16>(const ResPart& p) { return resolve_stream<16, 16>(p); }
template <> ResKernel resolve_stream_ool<16, 32>(const ResPart& p) { return resolve_stream<16, 32>(p); }
template <> ResKernel resolve_stream_ool<16, 64>(const ResPart& p) { return resolve_stream<16, 64>(p); }
}
