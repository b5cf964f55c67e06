// Host build of the deterministic mode's grid definitions (obvi-slam_amd/csrc/ba_device.h: the grids of the kernels that leave partial
// sums and the slot size taken from them) so the CPU test-suite can hold one against the other without a GPU.  Test infrastructure only.
#include "../obvi-slam_amd/csrc/ba_device.h"
using namespace obvi;
extern "C" {
// c: P L O od n_rp n_point_waves n_long_points n_bb n_sp n_lt n_rl (DetCounts)
int64_t detslots_needed(const int64_t* c) { return det_slots_needed({c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], c[10]}); }
// g: the grids the launchers of ba_kernels.hip take from the same counts, back-substitution at `lanes` per feature
void detslots_grids(const int64_t* c, int lanes, int64_t* g) {
  const int64_t P = c[0], L = c[1], O = c[2], od = c[3], n_rp = c[4], ns = c[7] + c[8] + c[9] + c[10];
  g[0] = point_pass_grid(c[5]);
  g[1] = point_pass_long_grid(c[6]);
  g[2] = small_lin_grid(c[7], c[8] + c[9], c[10]);
  g[3] = reduced_diag_grid(P, O, od);
  g[4] = backsub_grid(L, P, O, lanes);
  g[5] = cost_grid(P, n_rp, ns);
  g[6] = eval_reproj_grid(n_rp);
  g[7] = eval_small_grid(ns);
}
}
