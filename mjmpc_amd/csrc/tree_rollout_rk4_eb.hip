// The episode batches' twins (tree_rollout_kernel's EB = 1) of the RK4 instantiations of tree_rollout_rk4.hip,
// compiled beside them with the same scheduling alternatives (mjmpc_amd/build.py).
#define TREE_DENSE_TU 4
#include "tree_rollout.hip"
namespace mjmpc {
MJMPC_TREE_INSTANTIATE(1)
}  // namespace mjmpc
