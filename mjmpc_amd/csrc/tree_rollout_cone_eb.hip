// The episode batches' twins (tree_rollout_kernel's EB = 1) of the elliptic-cone instantiations of
// tree_rollout_cone.hip, compiled beside them with the same scheduling alternatives (mjmpc_amd/build.py).
#define TREE_CONE_TU
#include "tree_rollout.hip"
namespace mjmpc {
MJMPC_TREE_INSTANTIATE(1)
}  // namespace mjmpc
