"""GPU rollout engine for kinematic-tree models - ``ArmRolloutEngine``'s sibling for models the serial-chain kernel
cannot hold (a hand on an arm; the reference's vendored swimmer and half-cheetah with their floating
roots, springs, fluid forces and frictional contacts; up to 32 hinge / slide dofs).

The state dictionary follows the model's task: the reacher's ``{qp, qv, target_pos}`` (reacher_env.py:81-99) or the
locomotion envs' ``{qpos, qvel}`` (swimmer.py:33-50, half_cheetah.py:36-51).

Same reference-shaped surface (``SubprocVecEnv.rollout / set_env_state / reset / close``,
mjmpc/envs/vec_env/subproc_vec_env.py:128-186, 235-251), so ``make_rollout_fn`` / ``make_device_rollout_fn`` and every
controller work on it unchanged:

    sim_env = TreeRolloutEngine(hand24_raw())
    controller.set_sim_state_fn = sim_env.set_env_state
    controller.rollout_fn = make_device_rollout_fn(sim_env)

One HIP launch per rollout (mjmpc_amd/csrc/tree_rollout.hip) through the C ABI (``mjmpc_tree_*``).  The host side both
engines share is ``RolloutEngine`` (envs/_engine.py); this module holds what is the tree's own: its model compiler and state
layout, the host-synchronous ``step``, ``get_state_device`` and the raw state shards of episode batches.
"""
import numpy as np

from .. import _lib
from ..models.compile_tree import TreeModel, compile_tree
from ..models.raw import TASK_FORWARD
from ._engine import RolloutEngine, SimulationUnstableError  # noqa: F401


class TreeRolloutEngine(RolloutEngine):
    _abi = "tree"
    _model_type, _compile = TreeModel, staticmethod(compile_tree)
    _layout = (78, 40, 72)          # MJMPC_TREE_STATE_LEN: qpos[40] | qvel[32] | target[3] | -
    _qpos_len = "nq"
    _fused_checks_shards = True
    _shard_states_set_state = True
    forward_task = property(lambda self: self.model.task == TASK_FORWARD)

    def _create(self, blob, n_blob, device, h_out):
        integrator = {"Euler": 0, "RK4": 1}[getattr(self.model, "integrator", "Euler")]     # (MJMPC_INTEGRATOR_*)
        return self._lib.mjmpc_tree_create_ex(blob, n_blob, device, integrator, h_out)

    def _unpack(self, state):
        kq, kv = ("qpos", "qvel") if "qpos" in state else ("qp", "qv")
        return self._checked_state(state[kq], state[kv], state.get("target_pos", self.model.target_default))

    def _start_qpos(self):
        return self.model.qpos0.copy()

    def reset(self):
        super().reset()
        return self.get_env_state()

    def _default_geom_friction(self, geom):
        return np.array([geom.friction, 0.005, 0.0001])          # (torsional / rolling: MuJoCo's defaults, unused here)

    def _default_frictionloss(self, joint):
        # (a non-zero value: friction-loss constraint rows - the general kernel instantiation, which the engine's own model
        # must already run: a model whose defaults are all zero keeps them zero under a multiplicative draw)
        return float(joint.frictionloss)

    def step(self, action):
        """Advance the engine's own state by one env step (a one-particle rollout, state round trip through the host:
        the tree engine keeps no device-resident "real env").  Returns (next_obs, reward)."""
        if self.forward_task and self.model.obs_skip:
            raise ValueError("the observation leaves out qpos[:%d]; step an engine compiled with obs_skip = 0"
                             % self.model.obs_skip)
        with self.real_step_guard("TreeRolloutEngine.step"):
            _, rew, _, _, _, nobs = self.rollout(1, 1, np.asarray(action, np.float64).reshape(1, -1), None)
        nv, nq = self.model.nv, self.model.nq
        self.set_env_state(dict(qp=nobs[0, 0, :nq], qv=nobs[0, 0, nq:nq + nv], target_pos=self._state["target_pos"]))
        return nobs[0, 0].copy(), float(rew[0, 0])

    def set_real_env_model(self, model):
        """The model ``step_state`` - the device-resident real env, also inside a captured control iteration - steps with:
        a ``RawModel`` / compiled ``TreeModel`` of the engine's topology, ``"nominal"`` for the model the engine was built
        from (the reference's pairing after ``randomize_dynamics``: a randomized ``sim_env`` that only does rollouts beside
        a nominal true env, example_mpc.py), or ``None`` for the default, shard 0's block.  Call it before
        ``enable_graph(post_step=engine.step_state)``: a captured env step keeps the block it was captured with."""
        if model is None:
            blob = None
        else:
            if isinstance(model, str):
                if model != "nominal":
                    raise ValueError("set_real_env_model takes a model, 'nominal' or None, got %r" % (model,))
                model = self.model
            elif not isinstance(model, TreeModel):
                model = self._compile(model)
            blob = np.ascontiguousarray(model.blob, np.float64)
        _lib.check(self._lib.mjmpc_tree_set_env_model(self._h, None if blob is None else blob.ctypes.data_as(_lib._dp)))
        self.real_env_blob = blob
