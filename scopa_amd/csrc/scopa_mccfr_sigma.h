// scopa_mccfr_sigma.h -- the MCCFR solvers' regret matching, shared by the translation units that freeze a strategy from a regret row
// (scopa_mccfr.hip: every traversal kernel; scopa_chance.hip: the reduce of the chance game's MCCFR iteration, which weighs a row's visit
// count with the sigma its walks sampled from).
#pragma once
#include <hip/hip_runtime.h>

namespace scopa {

// InfoNode.current_strategy, mc_cfr.py:20-24  (np.maximum, ndarray.sum left-to-right, elementwise divide)
// (all loops over the 4 slots are unrolled with a predicate on n: indexing by a run-time n would put the arrays in scratch memory)
__device__ __forceinline__ void mc_sigma(const double *R, int n, double *sigma) {
    double pos[4];
#pragma unroll
    for (int i = 0; i < 4; i++) pos[i] = (i < n && R[i] > 0.0) ? R[i] : 0.0;
    double s = pos[0];
#pragma unroll
    for (int i = 1; i < 4; i++) if (i < n) s += pos[i];
#pragma unroll
    for (int i = 0; i < 4; i++) sigma[i] = i < n ? (s == 0.0 ? 1.0 / (double)n : pos[i] / s) : 0.0;
}

}  // namespace scopa
