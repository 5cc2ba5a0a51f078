// The tree rollout kernel's RK4 instantiations (MJCF <option integrator="RK4">: MuJoCo's mj_RungeKutta, four forward
// evaluations per substep; tree_rollout_kernel's RK4 = 1) as a translation unit of their own: the 16-lane dense family for
// GEN 0, 1 and 2, compiled with the scheduling alternatives of tree_rollout_dense.hip.  TREE_DENSE_TU holds the forward
// evaluations per substep of the unit's instantiations (tree_rollout_dense.hip: 1).  Every Euler model runs the kernels it had.
#define TREE_DENSE_TU 4
#include "tree_rollout.hip"
namespace mjmpc {
MJMPC_TREE_INSTANTIATE(0)
}  // namespace mjmpc
