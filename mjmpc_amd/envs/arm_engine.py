"""GPU rollout engine for arm models - the drop-in for the reference's ``SubprocVecEnv``.

The reference fans particles out to forked CPU workers that each run ``GymEnvWrapper.rollout``
(mjmpc/envs/vec_env/subproc_vec_env.py:128-186, mjmpc/envs/gym_env_wrapper.py:89-156).  Here the
whole particle set is one HIP kernel launch (mjmpc_amd/csrc/arm_rollout.hip) reached through the C
ABI; this class keeps the reference's method names, argument meaning and return layout so that
the closures of examples/example_mpc.py:112-155 work unchanged:

    sim_env = ArmRolloutEngine(reacher7dof_raw())
    controller.set_sim_state_fn = sim_env.set_env_state
    controller.rollout_fn = make_rollout_fn(sim_env)

What the arm engine shares with ``TreeRolloutEngine`` - the reference-shaped surface, the device-resident rollouts, per-shard
models and start states - is ``RolloutEngine`` (envs/_engine.py); this module holds what is the arm's own: its model
compiler and state layout, and the fused control iteration (``mppi_step`` and its launchers).  ``make_rollout_fn`` and
``make_device_rollout_fn`` work on any engine and are re-exported from here.
"""
import numpy as np

from .. import _lib
from ..models.compile import ArmModel, compile_arm
from ._engine import (RolloutEngine, SimulationUnstableError, _ptr, _torch,  # noqa: F401
                      make_device_rollout_fn, make_rollout_fn)


class ArmRolloutEngine(RolloutEngine):
    """One GPU's worth of particles for a compiled arm model (``reacher_7dof-v0``)."""
    _abi = "arm"
    _model_type, _compile = ArmModel, staticmethod(compile_arm)
    _layout = (19, 8, 16)           # MJMPC_ARM_STATE_LEN: qpos[8] | qvel[8] | target[3]

    def _create(self, blob, n_blob, device, h_out):
        return self._lib.mjmpc_arm_create(blob, n_blob, device, h_out)

    def _unpack(self, state):
        return self._checked_state(state["qp"], state["qv"], state["target_pos"])

    def _start_qpos(self):
        return np.zeros(self.model.nv)

    def _overrides(self, rand):
        """geom_friction is accepted without effect (every contact here is frictionless condim 1), dof_frictionloss stays 0
        (the default is 0 and the randomization multiplicative: the draw is consumed), no observation reads a sensor."""
        if any(np.any(np.asarray(v) != 0) for v in rand.get("dof_frictionloss", {}).values()):
            raise NotImplementedError("a non-zero dof_frictionloss adds friction-loss constraint rows, which the "
                                      "arm kernel does not model")
        return {k: v for k, v in rand.items() if k not in ("geom_friction", "dof_frictionloss", "sensor_noise")}

    def _default_geom_friction(self, geom):
        return np.array([0.5, 0.1, 0.1])                      # sawyer.xml:6 default

    def _default_frictionloss(self, joint):
        # RawJoint carries no frictionloss here: every model this engine loads has MuJoCo's default 0 (sawyer.xml:5 sets
        # none).  The reference's randomization is multiplicative (gym_env_wrapper.py:409-411), so the randomized
        # value of a zero default is exactly 0: the draw is consumed, no friction-loss row ever appears.
        return 0.0

    # ------------------------------------------------------------------ the fused control iteration
    def mppi_step_supported(self, num_particles, horizon):
        """The fused iteration is built for launches of at most one wavefront per SIMD pair (two wavefronts per particle
        group, 4096 particles on 256 CUs) - the latency-bound regime, where the launches it saves matter; larger
        populations keep the separate sampler / rollout / update launches (their rollout kernel needs the registers and
        the LDS the fused one spends on sampling and on the action tile)."""
        torch = _torch()
        simds = 4 * torch.cuda.get_device_properties(self.device).multi_processor_count
        groups = (int(num_particles) + 7) // 8
        lds = 8 * (32 + 8 * int(horizon) * self.d_action * (8 if self.dtype == "f64" else 4) // 8)
        return 2 * groups <= simds and lds <= 40 * 1024

    def rollout_sampled(self, num_particles, horizon, mean, gamma_seq, filter_coeffs, chol, chol_full, seed, offset,
                        particle_offset, step_counter, q0_out=None):
        """A rollout whose samples are drawn in the kernel (``mjmpc_arm_rollout_sampled``): the Philox stream of
        ``DeviceUpdater.sample_noise``, coloured by the device-resident factor ``chol`` (``chol_full``: its whole lower
        triangle - CEM's adapting covariance), filtered on the fly.  Returns (costs, actions, q0) device tensors; nothing
        but the model, the state, the mean and the factor is read from memory."""
        self._refuse_with_terms("rollout_sampled")
        P, H, A = int(num_particles), int(horizon), self.d_action
        costs, act = self._buffer("costs", (P, H)), self._buffer("act", (P, H, A))
        q0 = self._q0_buffer(P, q0_out)
        _lib.check(self._lib.mjmpc_arm_rollout_sampled(self._h, self._code, P, H, _ptr(mean), _ptr(gamma_seq), _ptr(filter_coeffs),
                                                       _ptr(chol), int(bool(chol_full)), int(seed) & (2 ** 64 - 1), int(offset),
                                                       int(particle_offset), _ptr(step_counter), _ptr(costs), _ptr(act), _ptr(q0),
                                                       self._stream()))
        return costs, act, q0

    def mppi_step(self, num_particles, horizon, mean, mean_out, gamma_seq, filter_coeffs, chol, seed, offset,
                  particle_offset, step_counter, lam, step_size, shift_mode, action_out=None, action_slots=None, record=None,
                  env_step=False, want_trajectories=False):
        """One whole control iteration in two launches (``mjmpc_arm_mppi_step``): sampling (the Philox stream of
        ``DeviceUpdater.sample_noise`` for a diagonal covariance), rollout, cost-to-go | softmax update of ``mean`` into
        ``mean_out`` (a tensor of its own), action read-out, shift, and - ``env_step`` - one step of the device-resident
        real env with that action.  All tensors are CUDA tensors (``mean`` / ``mean_out`` float64 (H,A), ``gamma_seq``
        float64 (H,), ``filter_coeffs`` float64 (3,) or None, ``chol`` float64 (A,A), ``step_counter`` int64 (1,));
        ``action_slots`` is a pinned host tensor (2, A+1).  ``record`` (float64 (2 + H*A,)): sharded runs - this GPU's
        softmax record instead of the update.  Returns (costs, actions, q0) device tensors when ``want_trajectories``."""
        self._refuse_with_terms("mppi_step")
        launch, out = self.mppi_step_launcher(num_particles, horizon, mean, mean_out, gamma_seq, filter_coeffs, chol, seed,
                                              offset, particle_offset, step_counter, lam, step_size, shift_mode, action_out,
                                              action_slots, record, env_step, want_trajectories)
        launch()
        return out

    def mppi_step_launcher(self, num_particles, horizon, mean, mean_out, gamma_seq, filter_coeffs, chol, seed, offset,
                           particle_offset, step_counter, lam, step_size, shift_mode, action_out=None, action_slots=None,
                           record=None, env_step=False, want_trajectories=False, bind_stream=True):
        """``mppi_step`` with its arguments bound once: returns (launch, outputs) where ``launch()`` enqueues the
        iteration on the stream that is current NOW (one C call, nothing converted per step) - what a control loop
        calls every step.  ``bind_stream=False``: on the stream that is current when ``launch()`` is called (a launcher
        that is also called under stream capture must say so, or its kernels stay out of the graph).  The tensors must
        stay alive (and in place) while the launcher is in use."""
        self._refuse_with_terms("mppi_step_launcher")
        P, H, A = int(num_particles), int(horizon), self.d_action
        costs = act = q0 = None
        if want_trajectories:
            costs, act, q0 = self._buffer("costs", (P, H)), self._buffer("act", (P, H, A)), self._q0_buffer(P)
        scost = self._buffer("step_cost", (1,)) if env_step else None
        snobs = self._buffer("step_obs", (self.d_obs,)) if env_step else None
        keep = (mean, mean_out, gamma_seq, filter_coeffs, chol, step_counter, action_out, action_slots, record, scost, snobs,
                costs, act, q0)
        args = (self._h, self._code, P, H, _ptr(mean), _ptr(mean_out), _ptr(gamma_seq), _ptr(filter_coeffs), _ptr(chol),
                int(seed) & (2 ** 64 - 1), int(offset), int(particle_offset), _ptr(step_counter), float(lam), float(step_size),
                int(shift_mode), _ptr(action_out), _ptr(action_slots), _ptr(record), int(bool(env_step)), _ptr(scost),
                _ptr(snobs), _ptr(costs), _ptr(act), _ptr(q0))
        fn, check, stream = self._lib.mjmpc_arm_mppi_step, _lib.check, self._stream
        if bind_stream:
            args = args + (stream(),)

            def launch(_keep=keep):
                check(fn(*args))
        else:
            def launch(_keep=keep):
                check(fn(*args, stream()))

        return launch, ((costs, act, q0) if want_trajectories else None)

    def mppi_combine_launcher(self, records, n_records, horizon, mean, mean_out, step_counter, step_size, shift_mode,
                              action_out, action_slots, env_step):
        """Sharded runs: the launch behind the record all-gather (``mjmpc_arm_mppi_combine``) with its arguments bound;
        ``launch()`` enqueues it on the stream that is current WHEN IT IS CALLED (it is called under stream capture)."""
        self._refuse_with_terms("mppi_combine_launcher")
        scost = self._buffer("step_cost", (1,))         # (bound whether or not this launcher steps the env: the parameter
        snobs = self._buffer("step_obs", (self.d_obs,))  #  block of the call then never changes between launchers)
        keep = (records, mean, mean_out, step_counter, action_out, action_slots, scost, snobs)
        args = (self._h, self._code, _ptr(records), int(n_records), int(horizon), _ptr(mean), _ptr(mean_out),
                _ptr(step_counter), float(step_size), int(shift_mode), _ptr(action_out), _ptr(action_slots),
                int(bool(env_step)), _ptr(scost), _ptr(snobs))
        fn, check, stream = self._lib.mjmpc_arm_mppi_combine, _lib.check, self._stream

        def launch(_keep=keep):
            check(fn(*args, stream()))

        return launch
