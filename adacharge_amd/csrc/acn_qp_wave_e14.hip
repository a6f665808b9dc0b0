// Wave-per-problem kernel (acn_qp_wave.hpp): the instantiations whose P = Ghat r0 runs over 14 EVSE k-steps (sites of at
// most 56 EVSEs; wave_evse_extent, acn_qp_rank.hpp) and their launcher launch_wave_e14.  A unit of its own so that it
// compiles beside acn_qp_wave.hip, which holds the instantiations over all 16 k-steps and routes between the two.
#define ACNQP_WAVE_NE 14
#include "acn_qp_wave.hip"
