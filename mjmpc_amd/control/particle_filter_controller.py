"""Particle-filter MPC with the rollout and the weights on the GPU.

Counterpart of the reference's ``PFMPC`` (mjmpc/control/particle_filter_controller.py): the control
distribution is a set of P action sequences; every iteration rolls them out, turns the discounted
costs into softmax weights, resamples systematically and (on shift) diffuses the survivors.

Split of work: rollouts and the exponentiated-cost weights are HIP kernels; the resampling itself is
a cumulative-sum search whose float summation order decides which particle survives, so it is done
on the host on the gathered weights, in the reference's order.

Sharded runs (one process per GPU): every rank holds the whole particle set, rolls out only its contiguous
block, all-gathers the (P,H) costs - the path's one exchange - and then computes the same weights and the
same resampling as every other rank (identical seeds), so the replicas stay bit-identical without a broadcast.

``noise_mode='device'`` (one GPU) keeps the particle set, its mean, the weights and the resampling on the device
(csrc/pfmpc.hip): the running sum is added strictly left to right by one lane, so the indices are the ones
``systematic_resample_indices`` returns for the same weights and pointer; the random numbers are the library's Philox
stream instead of the reference's MT19937 one (as MPPI's 'device' noise mode).  ``optimize()`` then synchronises with
the device once, to read the action; ``action_samples`` / ``mean_action`` are device tensors.
"""
import copy
import ctypes
import inspect
import random

import numpy as np

from .. import _lib
from .control_utils import generate_noise
from .controller import Controller
from .sharding import local_block


def systematic_resample_indices(weights, first_pointer):
    """Low-variance resampling: pointers ``first_pointer + m/M`` walk the running sum of ``weights``.

    Equivalent to the serial walk of particle_filter_controller.py:159-171 (``while c < u: c += w[i]``):
    ``np.cumsum`` accumulates in the same order, a pointer selects the first particle whose running sum
    reaches it, pointers beyond the total select the last particle, and a pointer at 0 selects index -1
    exactly as the reference's ``act_seq[i - 1]`` with ``i == 0`` does."""
    M = weights.shape[0]
    pointers = first_pointer + np.arange(M) * 1.0 / M * 1.0
    running = np.cumsum(weights)
    idx = np.minimum(np.searchsorted(running, pointers, side="left"), M - 1)
    idx[pointers <= 0.0] = -1
    return idx


def _check_device_rollout_fn(fn):
    if not getattr(fn, "accepts_device", False):
        raise ValueError("noise_mode='device' needs a device-resident rollout_fn (make_device_rollout_fn): this one does "
                         "not accept device tensors")


_PF_SHIFT_MODES = {'null': 0, 'repeat': 1}


class PFMPC(Controller):
    def __init__(self, d_state, d_obs, d_action, horizon, cov_shift, cov_resample, base_action, lam,
                 num_particles, gamma, n_iters, action_lows, action_highs, set_sim_state_fn=None, rollout_fn=None,
                 sample_mode="mean", batch_size=1, filter_coeffs=[1., 0., 0.], seed=0, device=0, comm=None,
                 noise_mode='host'):
        if noise_mode not in ('host', 'device'):
            raise ValueError("noise_mode must be 'host' or 'device'")
        if noise_mode == 'device':              # refused before any device memory exists
            if base_action not in _PF_SHIFT_MODES:
                raise ValueError("noise_mode='device' takes base_action 'null' or 'repeat' ('random' draws from the host's "
                                 "global generator)")
            if comm is not None and comm.world_size > 1:
                raise ValueError("noise_mode='device' runs on one GPU; sharded runs keep noise_mode='host'")
            if n_iters < 1:
                raise ValueError("noise_mode='device' needs n_iters >= 1")
            if rollout_fn is not None:
                _check_device_rollout_fn(rollout_fn)
        self.noise_mode = noise_mode
        super().__init__(d_state, d_obs, d_action, action_lows, action_highs, horizon, gamma, n_iters,
                         set_sim_state_fn, rollout_fn, sample_mode, batch_size, seed, device=device, comm=comm)
        if num_particles % self.dev.comm.world_size != 0:
            raise AssertionError("Number of particles must be divisible by number of shards")
        self.lam = lam
        self.num_particles = num_particles
        self.base_action = base_action
        self.filter_coeffs = filter_coeffs
        self.cov_shift = np.diag(np.full(self.d_action, float(cov_shift)))
        self.cov_resample = np.diag(np.full(self.d_action, float(cov_resample)))
        if noise_mode == 'device':
            self._post_step = None
            self._device_setup()
            return
        random.seed(self.seed_val)                       # the reference seeds the global `random` here (:66)
        self.mean_action = np.zeros((horizon, d_action))
        self.action_samples = self._fresh_samples()

    # -- sampling ---------------------------------------------------------------------------------
    def _fresh_samples(self):
        """Initial particle set: filtered N(0, cov_resample) draws from the controller seed (:68-70)."""
        return generate_noise(self.cov_resample, self.filter_coeffs, shape=(self.num_particles, self.horizon),
                              base_seed=self.seed_val)

    def sample_actions(self):
        return self.action_samples

    def generate_rollouts(self, state):
        """:74-90 - the particles are passed as deviations from their mean, the only form rollout_fn takes."""
        self._set_sim_state_fn(copy.deepcopy(state))
        off, n = local_block(self.num_particles, self.dev.comm.rank, self.dev.comm.world_size)
        return self._rollout_fn(n, self.horizon, self.mean_action,
                                (self.action_samples - self.mean_action)[off:off + n], mode="open_loop")

    # -- update -------------------------------------------------------------------------------------
    def _exp_util(self, costs):
        """softmax(-cost_to_go[:, 0] / lam) (:104-113), by the HIP softmax kernels."""
        costs = self.dev.to_device(costs, "costs")
        if self.dev.comm.world_size > 1:                  # the exchange: every rank sees all P cost rows
            costs = self.dev.comm.all_gather_flat(costs.reshape(-1)).reshape(self.num_particles, self.horizon)
        n = self.dev.softmax_update(costs, self.dev.zero_actions(costs.shape[0], costs), self.lam, 0.0,
                                    update_mean=False, replicated=True)
        return self.dev.softmax_weights(n).cpu().numpy()

    def _resampling(self, act_seq, weights, low_variance=True):
        if low_variance:
            M = act_seq.shape[0]
            return act_seq[systematic_resample_indices(weights, random.uniform(0.0, 1.0 / M * 1.0))]
        return np.array(random.choices(self.action_samples, weights=weights, k=self.num_particles))

    def _update_distribution(self, trajectories):
        """:92-102 - weights, reseed both global generators with seed + step, resample, recentre."""
        w = self._exp_util(trajectories["costs"])
        step_seed = self.seed_val + self.num_steps
        random.seed(step_seed)
        np.random.seed(step_seed)
        self.action_samples = self._resampling(self.action_samples, w, low_variance=True)
        self.mean_action = self.action_samples.mean(axis=0)

    def _get_next_action(self, state, mode='mean'):
        return self.action_samples.mean(axis=0)[0].copy()

    # -- time shift ---------------------------------------------------------------------------------
    def _shift(self):
        """:127-150 - advance every sequence one step, diffuse with fresh filtered noise, append the base action."""
        moved = self.action_samples
        moved[:, :-1] = moved[:, 1:]
        jitter = generate_noise(self.cov_shift, self.filter_coeffs, shape=(self.num_particles, self.horizon),
                                base_seed=self.seed_val + self.num_steps)
        moved = moved + jitter
        tails = {'null': lambda: np.zeros((self.num_particles, self.d_action)),
                 'repeat': lambda: moved[:, -2],
                 'random': lambda: np.random.normal(0, self.cov_resample, self.d_action)}
        if self.base_action not in tails:
            raise NotImplementedError("invalid option for base action during shift")
        moved[:, -1] = tails[self.base_action]()
        self.action_samples = moved

    def reset(self):
        self.num_steps = 0
        if self.noise_mode == 'device':
            self._device_reset()
            return
        self.mean_action = np.zeros((self.horizon, self.d_action))
        self.action_samples = self._fresh_samples()

    # -- device-resident mode (csrc/pfmpc.hip) ----------------------------------------------
    def _set_rollout_fn(self, fn):
        if getattr(self, "noise_mode", "host") == 'device' and fn is not None:
            _check_device_rollout_fn(fn)
        self._rollout_fn = fn

    rollout_fn = Controller.rollout_fn.setter(_set_rollout_fn)

    def set_post_step(self, fn):
        """``fn(action)`` is called in ``optimize()`` with the DEVICE action tensor (float64 [A]) before the host waits for
        the action - e.g. ``engine.step_state``: with ``set_sim_state_fn = resident_state`` the closed loop then never
        uploads a state.  Device mode only."""
        if self.noise_mode != 'device':
            raise ValueError("set_post_step needs noise_mode='device'")
        self._post_step = fn

    def _device_setup(self):
        torch, dev = self.dev.torch, self.dev.device
        M, H, A = self.num_particles, self.horizon, self.d_action
        f64 = dict(dtype=torch.float64, device=dev)
        self._set, self._set_alt, self._gathered = (torch.empty((M, H, A), **f64) for _ in range(3))
        self._mean = torch.zeros((H, A), **f64)
        self._w, self._first = torch.empty(M, **f64), torch.zeros(1, **f64)
        self._idx = torch.empty(M, dtype=torch.int32, device=dev)
        self._pf_ws = torch.empty((self.dev.lib.mjmpc_pf_workspace_bytes(M, H, A) + 7) // 8, **f64)
        self._step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self._action_dev = torch.zeros(A, **f64)
        self._action_pin = torch.zeros(A, dtype=torch.float64).pin_memory()
        # the jitter's factor: cov_shift is c I, its factor sqrt(c) I (a zero variance is a zero jitter, not an error)
        self._chol_shift = torch.from_numpy(np.sqrt(self.cov_shift)).to(dev)
        fc = np.asarray(self.filter_coeffs, np.float64)
        self._coeffs_dev = None if (fc[0] == 1.0 and fc[1] == 0.0 and fc[2] == 0.0) else torch.from_numpy(fc.copy()).to(dev)
        self._delta, self._costs, self._q0_kw_for = {}, None, None
        self._device_reset()

    def _device_reset(self):
        """The initial set: the Philox counterpart of ``_fresh_samples`` (key (seed, offset 0)); the mean starts at zero."""
        self._set.copy_(self.dev.sample_noise(self.num_particles, self.cov_resample, self.filter_coeffs, self.seed_val, 0,
                                              dtype="f64"))
        self._mean.zero_()
        self._step_dev.fill_(self.num_steps)
        self._step_host = self.num_steps
        self.action_samples, self.mean_action = self._set, self._mean

    def _device_iteration(self, shift_mode, bump):
        """delta -> rollout -> weights + first pointer -> indices -> gather (+ shift) -> mean + action: five small launches
        beside the rollout, nothing synchronises."""
        dev, lib, fn = self.dev, self.dev.lib, self._rollout_fn
        _check_device_rollout_fn(fn)
        M, H, A = self.num_particles, self.horizon, self.d_action
        vp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        seed = int(self.seed_val) & (2 ** 64 - 1)
        dtype = getattr(getattr(fn, "engine", None), "dtype", "f64")
        delta = self._delta.get(dtype)
        if delta is None:
            delta = self._delta[dtype] = dev.torch.empty((M, H, A), device=dev.device,
                                                         dtype=dev.torch.float32 if dtype == "f32" else dev.torch.float64)
        _lib.check(lib.mjmpc_pf_delta(_lib.F32 if dtype == "f32" else _lib.F64, M, H, A, vp(self._set), vp(self._mean),
                                      vp(delta), dev.stream()))
        q0 = dev.q0_destination(M)
        fused = getattr(fn, "fused", None)
        if fused is not None:           # the cost-to-go comes out of the rollout launch, where the weights read it
            if self._q0_kw_for is None or self._q0_kw_for[0] is not fused:
                self._q0_kw_for = (fused, "q0_out" in inspect.signature(fused).parameters)
            costs, _, got = fused(M, H, self._mean, delta, None, dev.gseq, **(dict(q0_out=q0) if self._q0_kw_for[1] else {}))
            if got.data_ptr() != q0.data_ptr():
                q0.copy_(got)
        else:                           # (engines without a fused launch: the cost-to-go kernel of the other controllers)
            costs = dev.to_device(fn(M, H, self._mean, delta, mode="open_loop")["costs"], "costs")
            _lib.check(lib.mjmpc_traj_cost(dev.code(costs), M, H, A, vp(costs), vp(dev.gseq), dev.gamma_zero,
                                           vp(dev.workspace(M)), dev.stream()))
        self._costs = costs
        _lib.check(lib.mjmpc_pf_weights(M, vp(q0), float(self.lam), seed, 0, vp(self._step_dev), vp(self._w), vp(self._first),
                                        dev.stream()))
        _lib.check(lib.mjmpc_pf_resample(M, vp(self._w), vp(self._first), vp(self._idx), vp(self._pf_ws), dev.stream()))
        # (keyed with offset k + 1: the reference increments num_steps before _shift)
        _lib.check(lib.mjmpc_pf_gather_shift(M, H, A, vp(self._set), vp(self._idx), int(shift_mode), vp(self._chol_shift),
                                             vp(self._coeffs_dev), seed, 1, vp(self._step_dev), vp(self._set_alt),
                                             vp(self._gathered), vp(self._pf_ws), dev.stream()))
        _lib.check(lib.mjmpc_pf_finish(M, H, A, vp(self._pf_ws), vp(self._mean), vp(self._action_dev),
                                       vp(self._step_dev) if bump else None, dev.stream()))
        self._set, self._set_alt = self._set_alt, self._set
        self.action_samples = self._set

    def _optimize_device(self, state, hotstart):
        torch = self.dev.torch
        if not getattr(self._set_sim_state_fn, "ignores_state", False):
            self._set_sim_state_fn(copy.deepcopy(state))
        if self._step_host != self.num_steps:           # num_steps was assigned from outside
            self._step_dev.fill_(self.num_steps)
        # n_iters > 1 repeats rollout .. mean with the same step count k (the reference reseeds identically); the shift
        # rides in the last gather, the step counter moves behind it
        for it in range(self.n_iters):
            last = it == self.n_iters - 1
            self._device_iteration(_PF_SHIFT_MODES[self.base_action] if (last and hotstart) else -1, last)
        if self._post_step is not None:
            self._post_step(self._action_dev)
        self._action_pin.copy_(self._action_dev, non_blocking=True)
        torch.cuda.current_stream(self.dev.device).synchronize()         # the control step's one synchronisation
        action = self._action_pin.numpy().copy()
        self.num_steps += 1
        self._step_host = self.num_steps
        self.dev.check_status()
        return action, 0.0

    def optimize(self, state, calc_val=False, hotstart=True):
        if self.noise_mode != 'device':
            return super().optimize(state, calc_val, hotstart)
        if calc_val:
            self._calc_val(None)
        return self._optimize_device(state, hotstart)

    def last_device_step(self):
        """The stages of the last iteration of the last ``optimize()`` as device tensors (valid until the next call):
        ``samples`` the set that was rolled out, ``costs`` / ``q0`` what the rollout returned, ``w``, ``first``, ``idx``,
        ``resampled`` = samples[idx], ``mean`` of it, ``shifted`` the set the next step rolls out, ``step`` the count k the
        step was keyed with."""
        if self.noise_mode != 'device' or self._costs is None:
            raise ValueError("last_device_step needs noise_mode='device' and a finished optimize()")
        return dict(samples=self._set_alt, costs=self._costs, q0=self.dev.q0_destination(self.num_particles), w=self._w,
                    first=self._first, idx=self._idx, resampled=self._gathered, mean=self._mean, shifted=self._set,
                    step=self.num_steps - 1)

    def _calc_val(self, trajectories):
        raise NotImplementedError("_calc val not implemented yet")
