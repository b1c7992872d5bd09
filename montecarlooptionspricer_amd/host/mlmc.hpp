// Host side of the multilevel level call (include/mcgpu.h: mcg_mlmc_localvol_level_ex): what it rejects of the scheme and the
// bridge flag, and the bridge levels of a book.  Plain C++ (no HIP header): host/mlmc.cpp builds and runs without the runtime
// (tests/cpp/mlmc_bridge_host_main.cpp, under the sanitizers).
#pragma once
#include "../../include/mcgpu.h"

namespace mcg {

constexpr int MLMC_SLOT_NONE = -2;       // not a barrier contract: the payoff on the five statistics
constexpr int MLMC_SLOT_UNTOUCHED = -1;  // a down barrier at zero: P = 1 by rule, no slot

int mlmc_check_level(const mcg_mlmc_level* lv, double T);
// MCG_ERR_INVALID with a message unless scheme is one of mcg_mlmc_scheme and bridge is 0 or 1
int mlmc_check_scheme(int scheme, int bridge);
// The distinct (barrier, up) of the barrier contracts, compared bitwise, in the order of first appearance: barriers and is_up
// hold MCG_MLMC_BRIDGE_L_MAX entries, slot (may be null) n_contracts -- a level's index, or one of the two constants above.
// MCG_ERR_INVALID with a message: a kind outside [0, 9]; a barrier that is not finite; an up barrier <= 0; a down barrier < 0;
// more than MCG_MLMC_BRIDGE_L_MAX levels.
int mlmc_bridge_plan(const mcg_exotic* book, int n_contracts, double* barriers, int* is_up, int* slot, int* n_levels);

}  // namespace mcg
