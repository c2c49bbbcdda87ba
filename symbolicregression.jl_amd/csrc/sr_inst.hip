// sr_inst.hip — the explicit instantiations of one unit of sr_builds.h; compiled once per unit with
// -DSR_UNIT=<unit> (the Makefile's UNITS), so the units compile in parallel.
#include "sr_tile_impl.h"
#include "sr_builds.h"

#ifndef SR_UNIT
#error "compile with -DSR_UNIT=<a unit of sr_builds.h>"
#endif
#define SR_INST_TILE(T, R, MODE, GATHER, TIER, W, LK, VSTK) \
  template hipError_t sr_launch_tile<T, R, MODE, GATHER, TIER, W, LK, VSTK>(const SrEvalArgs<T>&, int, hipStream_t);
#define SR_INST_DERIVED(T)                                                                                              \
  template hipError_t sr_launch_derived<T>(const T*, int64_t, const int64_t*, int64_t, int64_t, const SrDerivedSpec&, \
                                           T*, int64_t, hipStream_t);
#define SR_INST_UNIT_(unit) SR_BUILDS_##unit(SR_INST_TILE, SR_INST_DERIVED)
#define SR_INST_UNIT(unit) SR_INST_UNIT_(unit)
SR_INST_UNIT(SR_UNIT)
