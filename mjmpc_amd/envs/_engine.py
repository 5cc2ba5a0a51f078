"""The host side of a GPU rollout engine, once: ``RolloutEngine`` is what ``ArmRolloutEngine`` (arm_engine.py) and
``TreeRolloutEngine`` (tree_engine.py) have in common - the reference-shaped surface of ``SubprocVecEnv``
(mjmpc/envs/vec_env/subproc_vec_env.py:128-186, 235-256, 304-312), the device-resident rollouts, the per-shard models
and start states - over the C ABI's ``mjmpc_<_abi>_*`` entry points.  A subclass says what differs: its model compiler and
``create`` call, the layout of a shard's start state, how a state dictionary is read, and a few defaults.

Every library function is looked up when it is called (``_fn``), never kept: ``_lib.recording`` swaps the library's
attributes for recording wrappers while a launch tape is made.

torch is used only as the owner of device memory and streams.
"""
import ctypes
import time

import numpy as np

from .. import _lib
from ..models.compile import principal_inertia, require_f32_power_ratio
from ..models.raw import TASK_FORWARD, RawModel
from ._resets import EnvResetWatch, SimulationUnstableError  # noqa: F401
from .cost_terms import launch_points, refuse_mass_randomization
from .seeding import np_random

_DT = {"f32": (_lib.F32, np.float32), "f64": (_lib.F64, np.float64)}


def _torch():
    import torch
    return torch


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _same_state(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("qp", "qv", "target_pos"))


def draw_shard_models(host, param_dict, seeds, defaults, rand):
    """The draws and model blocks of ``randomize_dynamics``: shard i draws from ``np_random(seeds[i])`` a uniform value in
    ``m (1 +- noise)``, ``m = (1 + bias) * default``, for every ``{param_id: {name: [noise_scale, bias_scale]}}`` entry
    (gym_env_wrapper.py:367-416), in the order of ``param_dict``; ``defaults[i]`` / ``rand[i]`` (dicts, filled in place)
    receive its default and randomized values, and ``host`` (an engine, or ``RolloutEngine.host_only``) compiles its block.
    Returns the blocks, float64 ``[len(seeds), blob length]``.  Host only: nothing here touches the device."""
    blobs = []
    for i, seed in enumerate(seeds):
        rng, _ = np_random(int(seed))
        d, r = defaults[i], rand[i]
        for param_id, entries in param_dict.items():
            for name, (noise_scale, bias_scale) in entries.items():
                cur = d.setdefault(param_id, {}).get(name)
                if cur is None:
                    cur = d[param_id][name] = host._default_param(param_id, name)
                mean = (1.0 + bias_scale) * np.asarray(cur, float)
                r.setdefault(param_id, {})[name] = rng.uniform(mean - mean * noise_scale, mean + mean * noise_scale)
        blobs.append(host._compile(host.raw, overrides=host._overrides(r), base=host.model).blob)
    return np.ascontiguousarray(np.stack(blobs), np.float64)


class RolloutEngine(EnvResetWatch):
    """One GPU's worth of particles for a compiled model.  Subclasses set ``_abi``, ``_model_type``, ``_compile``,
    ``_layout``, ``_qpos_len`` and define ``_create``, ``_unpack``, ``_start_qpos``, ``_default_geom_friction`` and
    ``_default_frictionloss``."""
    _model_type = None              # the compiled model's class; ``_compile(raw, overrides=, base=)`` makes one
    _layout = None                  # a shard's start state in mjmpc_*_set_shard_states: (stride, qvel offset, target offset)
    _qpos_len = "nv"                # the model attribute that is the length of qpos
    forward_task = False            # the locomotion envs' {qpos, qvel} state dictionaries
    _fused_checks_shards = False    # rollout_fused refuses an indivisible population in Python (else the C layer does)
    _shard_states_set_state = False     # a per-shard set_env_state also makes shard 0's state ``_state``
    _cost_terms = None              # set_cost_terms: the builder, its table on the device, whether a row reads an action
    _terms_dev = None
    _terms_read_actions = False
    _track_ref = None               # tracked terms: the reference [N][R] and the env-time counter, on the device
    _track_step = None
    _track_periodic = 0
    _terms_rate = False             # the table holds action-rate rows or one-sided kinds: mjmpc_cost_terms_rate
    _prev_action = None             # ... with rate rows the action last applied to the controlled env, float64 [A] on the device
    _terms_quad = None              # the table holds quadratic groups or signed linear rows: mjmpc_cost_terms_quad
                                    # with this pool of matrices, float64 on the device (one zero without a group)
    _points = None                  # the table names points: (program on the device, n_rows, n_points, n_diff, n_extra,
                                    # the node rows' qvel addresses on the device - None without axes and velocities)
    _points_levels = None           # ... the saved frames of its program: a centre of mass, mjmpc_points_tree
    _points_orient = False          # ... whether it holds an orientation: mjmpc_points_orient
    _mass_randomized = None         # randomize_dynamics drew body_mass: its param_dict (DESIGN 12.6 refuses a centre of mass then)
    _points_last = None             # ... the augmented observations of the last cost launch (cost_observations)
    _closure_terms = None           # make_device_rollout_fn: whether the closures handed out were made with terms set

    def __init__(self, model, device=0, dtype="f64", num_shards=1):
        self.raw = model if isinstance(model, RawModel) else None
        if isinstance(model, RawModel):
            model = self._compile(model)
        if not isinstance(model, self._model_type):
            raise TypeError("model must be a RawModel or a compiled %s" % self._model_type.__name__)
        if dtype not in _DT:
            raise ValueError("dtype must be 'f32' or 'f64'")
        if dtype == "f32":
            require_f32_power_ratio(model)      # (a solimp power ratio beyond float32: refused)
        self.model, self.dtype = model, dtype
        self._code, self._np = _DT[dtype]
        self.num_shards = int(num_shards)       # reported like the reference's num_cpu (infos['total_time'])
        self._lib = _lib.require_gpu()
        torch = _torch()
        self.device = torch.device("cuda", device)
        self._tdtype = torch.float32 if dtype == "f32" else torch.float64
        h = ctypes.c_void_p()
        blob = np.ascontiguousarray(model.blob, np.float64)
        _lib.check(self._create(blob.ctypes.data_as(_lib._dp), blob.size, device, ctypes.byref(h)))
        self._h = h
        self.d_action, self.d_obs = model.nu, model.d_obs
        # qp, qv, qa, target_pos, timestep (reacher_env.py:81-85) or qpos, qvel
        self.d_state = self._nq + model.nv if self.forward_task else self._nq + 2 * model.nv + 3 + 1
        self.action_lows, self.action_highs = model.ctrl_lo.copy(), model.ctrl_hi.copy()
        self.closed = False
        self._buf = {}
        self.default_dyn_params = [dict() for _ in range(self.num_shards)]
        self.randomized_dyn_params = [dict() for _ in range(self.num_shards)]
        self.reset()

    def _fn(self, name):
        return getattr(self._lib, "mjmpc_%s_%s" % (self._abi, name))

    @property
    def _nq(self):
        return getattr(self.model, self._qpos_len)

    # ------------------------------------------------------------------ reference-shaped API
    def _checked_state(self, qp, qv, target_pos):
        qp, qv, tg = (np.ascontiguousarray(x, np.float64).reshape(-1) for x in (qp, qv, target_pos))
        if qp.size != self._nq or qv.size != self.model.nv or tg.size != 3:     # (qpos in MuJoCo's layout: nq entries)
            raise ValueError("state has the wrong dimensions for this model")
        return dict(qp=qp.copy(), qv=qv.copy(), target_pos=tg.copy())

    def set_env_state(self, state_dicts):
        """``SubprocVecEnv.set_env_state`` (subproc_vec_env.py:235-251): one dict (every shard starts from it), a list
        holding one dict, or one dict per shard (shard k's particles start from states[k]).  Keys as reacher_env.py:81-85;
        ``qa`` and ``timestep`` do not influence a rollout and are ignored."""
        if isinstance(state_dicts, (list, tuple)):
            if len(state_dicts) not in (1, self.num_shards):
                raise AssertionError("num states should equal 1 (same for all envs) or 1 per env")
            states = [self._unpack(s) for s in state_dicts]
            if any(not _same_state(states[0], s) for s in states[1:]):
                return self._set_shard_states(states)
            state = states[0]
        else:
            state = self._unpack(state_dicts)
        if getattr(self, "_per_shard_states", False):
            _lib.check(self._fn("set_shard_states")(self._h, None, 0, self._stream()))
            self._per_shard_states = False
        self._state = state
        _lib.check(self._fn("set_state")(self._h, state["qp"].ctypes.data_as(_lib._dp), state["qv"].ctypes.data_as(_lib._dp),
                                         state["target_pos"].ctypes.data_as(_lib._dp), self._stream()))

    def _pack_shard_states(self, states):
        """Unpacked states -> the (n, stride) array of ``mjmpc_*_set_shard_states``: qpos | qvel | target_pos at ``_layout``."""
        stride, ov, ot = self._layout
        arr = np.zeros((len(states), stride))
        for k, s in enumerate(states):
            arr[k, :self._nq], arr[k, ov:ov + self.model.nv], arr[k, ot:ot + 3] = s["qp"], s["qv"], s["target_pos"]
        return arr

    def _set_shard_states(self, states):
        arr = self._pack_shard_states(states)
        _lib.check(self._fn("set_shard_states")(self._h, arr.ctypes.data_as(_lib._dp), self.num_shards, self._stream()))
        self._per_shard_states = True
        self._shard_state_list = states
        if self._shard_states_set_state:
            self._state = states[0]

    def get_env_state(self):
        """One state dict - or, after a per-shard ``set_env_state``, one per shard (subproc_vec_env.py:253-256)."""
        states = self._shard_state_list if getattr(self, "_per_shard_states", False) else [self._state]
        if self.forward_task:
            return [dict(qpos=st["qp"].copy(), qvel=st["qv"].copy()) for st in states]
        return [dict(qp=st["qp"].copy(), qv=st["qv"].copy(), qa=np.zeros(self.model.nv),
                     target_pos=st["target_pos"].copy(), timestep=0) for st in states]

    def reset(self):
        self.set_env_state(dict(qp=self._start_qpos(), qv=np.zeros(self.model.nv),
                                target_pos=self.model.target_default.copy()))

    def close(self):
        if not self.closed:
            self._fn("destroy")(self._h)
            self._h = None              # later calls fail with "null engine" instead of touching freed memory
            self.closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def rollout(self, num_particles, horizon, mean, noise, mode="open_loop"):
        """``SubprocVecEnv.rollout``: numpy in, numpy out, reference layouts.
        Returns (obs, rew, act, done, info, next_obs); ``info`` is a list with one dict per shard."""
        t0 = time.time()
        out = self.rollout_device(num_particles, horizon, mean, noise, mode, want_obs=True)
        costs, act, obs, nobs = (x.to("cpu").numpy().astype(np.float64, copy=False) for x in out)
        done = np.zeros((num_particles, horizon))
        dt = time.time() - t0
        info = [{"total_time": dt} for _ in range(self.num_shards)]
        return obs, -costs, act, done, info, nobs

    def randomize_dynamics(self, param_dict, base_seed):
        """``SubprocVecEnv.randomize_dynamics`` (subproc_vec_env.py:304-312): shard i draws from
        ``np_random(base_seed + i*12345)`` a uniform value in ``m (1 +- noise)``, ``m = (1 + bias) * default``
        for every ``{param_id: {name: [noise_scale, bias_scale]}}`` entry (gym_env_wrapper.py:367-416) and
        from then on simulates its own model block (``mjmpc_*_set_shard_models``).  Supported: body_mass, body_inertia,
        dof_damping, geom_size (collision geoms), geom_friction, dof_frictionloss, sensor_noise (a known sensor's draw is
        consumed; no observation reads a sensor); what the engine's kernel makes of them: ``_overrides``.
        Returns (default_params, randomized_params), one dict per shard."""
        if self.raw is None:
            raise ValueError("randomize_dynamics needs the engine to be built from a RawModel")
        refuse_mass_randomization(self._cost_terms, param_dict)     # (no centre of mass over randomized masses)
        seeds = [int(base_seed) + i * 12345 for i in range(self.num_shards)]
        blobs = draw_shard_models(self, param_dict, seeds, self.default_dyn_params, self.randomized_dyn_params)
        _lib.check(self._fn("set_shard_models")(self._h, blobs.ctypes.data_as(_lib._dp), self.num_shards))
        self.shard_blobs = blobs
        if "body_mass" in param_dict:
            self._mass_randomized = {"body_mass": param_dict["body_mass"]}
        return self.default_dyn_params, self.randomized_dyn_params

    @classmethod
    def host_only(cls, raw, model=None):
        """The model-side half of an engine without a device: ``raw``, ``model``, the model compiler and the
        dynamics-randomization defaults (``draw_shard_models``) - what an episode batch draws its model blocks with."""
        self = cls.__new__(cls)
        self.raw, self.model = raw, cls._compile(raw) if model is None else model
        self.closed = True
        return self

    def _overrides(self, rand):
        """What of a shard's randomized parameters reaches the model compiler."""
        return rand

    def _default_param(self, param_id, name):
        raw, m = self.raw, self.model
        names = [b.name for b in raw.bodies]
        if param_id == "body_mass":
            return float(m.body_mass[names.index(name)])
        if param_id == "body_inertia":
            return principal_inertia(m.body_inertia[names.index(name)])[0]
        if param_id == "dof_damping":
            return float(next(b.joint.damping for b in raw.bodies if b.joint is not None and b.joint.name == name))
        if param_id in ("geom_size", "geom_friction"):
            g = next(g for b in raw.bodies for g in b.geoms if g.name == name)
            if param_id == "geom_friction":
                return self._default_geom_friction(g)
            half = 0.5 * np.linalg.norm(np.asarray(g.b, float) - np.asarray(g.a, float)) if g.type == 2 else 0.0
            return np.array([g.radius, half, 0.0])
        if param_id == "dof_frictionloss":
            return self._default_frictionloss(next(b.joint for b in raw.bodies if b.joint is not None and b.joint.name == name))
        if param_id == "sensor_noise":
            # (gym_env_wrapper.py:396-398 - model.sensor_noise: MuJoCo keeps the value for the user and adds no noise itself, and no
            # observation on the path reads a sensor: the draw is consumed, as in the reference, and changes nothing)
            if name not in raw.sensors:
                raise ValueError("no sensor named %r" % name)
            return float(raw.sensors[name])
        raise ValueError("Unknown dynamics field")

    # ------------------------------------------------------------------ device-resident API
    def rollout_device(self, num_particles, horizon, mean, noise, mode="open_loop", want_obs=False,
                       want_actions=True):
        """Launch the fused rollout.  ``mean`` / ``noise`` may be numpy arrays or CUDA tensors.
        Returns device tensors (costs, actions, obs, next_obs); buffers are reused between calls."""
        if mode not in ("open_loop", "closed_loop_linear"):
            raise ValueError("unsupported rollout mode %r ('open_loop' or 'closed_loop_linear')" % (mode,))
        if num_particles % self.num_shards != 0:
            raise AssertionError("Number of particles must be divisible by number of shards")
        torch = _torch()
        P, H, A = int(num_particles), int(horizon), self.d_action
        closed = mode == "closed_loop_linear"
        mean_d = self._as_device(mean, torch.float64, (self.d_obs + 1, A) if closed else (H, A))
        noise_d = None if noise is None else self._as_device(noise, self._tdtype, (P, H, A))
        costs = self._buffer("costs", (P, H))
        act = self._buffer("act", (P, H, A)) if want_actions else None
        obs = self._buffer("obs", (P, H, self.d_obs)) if want_obs else None
        nobs = self._buffer("nobs", (P, H, self.d_obs)) if want_obs else None
        # cost terms read the next observations (and the actions): the launch writes them whether or not the caller asked
        t_nobs, t_act = nobs, act
        if self._track_step is not None and self._in_real_step and (P, H) != (1, 1):
            raise ValueError("a rollout under real_step_guard advances the tracked cost terms' env time by one step: it must "
                             "be one particle and one step, got (%d, %d)" % (P, H))
        if self._prev_action is not None and self._in_real_step and (P, H) != (1, 1):
            raise ValueError("a rollout under real_step_guard records the action it applied for the action-rate cost terms: it "
                             "must be one particle and one step, got (%d, %d)" % (P, H))
        if self._terms_dev is not None:
            t_nobs = nobs if nobs is not None else self._buffer("terms_nobs", (P, H, self.d_obs))
            if self._terms_read_actions and act is None:
                t_act = self._buffer("terms_act", (P, H, A))
        fn = self._fn("rollout_cl" if closed else "rollout")
        _lib.check(fn(self._h, self._code, P, H, _ptr(mean_d), _ptr(noise_d), _ptr(costs), _ptr(t_act), _ptr(obs),
                      _ptr(t_nobs), self._stream()))
        if self._terms_dev is not None:
            # (a one-particle rollout under real_step_guard is the controlled env's step: never a plan's last step)
            self._launch_cost_terms(P, H, t_nobs, t_act, costs, terminal=not self._in_real_step, advance=self._in_real_step)
        return costs, act, obs, nobs

    def rollout_fused(self, num_particles, horizon, mean, raw_noise, filter_coeffs, gamma_seq, q0_out=None):
        """Device-resident rollout with the noise filter and the discounted cost-to-go fused into the
        launch (``mjmpc_*_rollout_fused``).  All arguments are CUDA tensors (``filter_coeffs`` may be
        None; ``q0_out``: a float64 [P] tensor the cost-to-go is written to instead of the engine's own
        buffer).  Returns (costs, actions, q0)."""
        self._refuse_with_terms("rollout_fused")
        if self._fused_checks_shards and num_particles % self.num_shards != 0:
            raise AssertionError("Number of particles must be divisible by number of shards")
        torch = _torch()
        P, H, A = int(num_particles), int(horizon), self.d_action
        mean_d = self._as_device(mean, torch.float64, (H, A))
        noise_d = self._as_device(raw_noise, self._tdtype, (P, H, A))
        costs = self._buffer("costs", (P, H))
        act = self._buffer("act", (P, H, A))
        q0 = self._q0_buffer(P, q0_out)
        _lib.check(self._fn("rollout_fused")(self._h, self._code, P, H, _ptr(mean_d), _ptr(noise_d), _ptr(filter_coeffs),
                                             _ptr(gamma_seq), _ptr(costs), _ptr(act), _ptr(q0), self._stream()))
        return costs, act, q0

    def step_state(self, action):
        """Advance the engine state in place by one env step (the "real env" kept on the device).
        ``action``: numpy (A,) or CUDA float64 tensor.  Returns (cost, next_obs) device tensors."""
        torch = _torch()
        a = self._as_device(action, torch.float64, (self.d_action,))
        cost = self._buffer("step_cost", (1,))
        nobs = self._buffer("step_obs", (self.d_obs,))
        _lib.check(self._fn("step_state")(self._h, self._code, _ptr(a), _ptr(cost), _ptr(nobs), self._stream()))
        if self._terms_dev is not None:
            act = None
            if self._terms_read_actions:
                act = self._buffer("step_act", (self.d_action,))
                act.copy_(a)                # (into the engine's storage type; a launch, no allocation: capturable)
            self._launch_cost_terms(1, 1, nobs, act, cost, terminal=False, advance=True)
        return cost, nobs

    # ------------------------------------------------------------------ user-defined cost terms (envs/cost_terms.py)
    def obs_layout(self):
        """Named slices of the observation, as the kernels write it.  Reach and orient tasks: ``qpos`` (nq entries,
        MuJoCo's layout), ``qvel``, ``site`` (the tracked site) and ``site_minus_target``.  Forward task: ``qpos`` - the
        entries ``qpos[obs_skip:]``, so the block's entry 0 is ``qpos[obs_skip]`` - and ``qvel``."""
        m, nq = self.model, self._nq
        if getattr(m, "task", None) == TASK_FORWARD:
            n = nq - m.obs_skip
            return dict(qpos=slice(0, n), qvel=slice(n, n + m.nv))
        n = nq + m.nv
        return dict(qpos=slice(0, nq), qvel=slice(nq, n), site=slice(n, n + 3), site_minus_target=slice(n + 3, n + 6))

    def set_cost_terms(self, terms):
        """From now on ``rollout_device`` (both modes), everything built on it (``rollout``, the env classes' ``step``) and
        ``step_state`` return the cost of ``terms`` (a ``CostTerms``; ``keep_builtin``: added to the built-in cost) instead
        of the built-in one: a second launch (``mjmpc_cost_terms``) behind the rollout on the same stream.  Rows marked
        terminal count at a rollout's last step, never in a step of the controlled env (``step_state``, a rollout under
        ``real_step_guard``).  The fused launches evaluate the built-in cost inside the rollout kernel and refuse to run
        while terms are set; ``make_device_rollout_fn`` then offers the controllers only the generic iteration - set the
        terms first, then make the ``rollout_fn``.  ``None`` restores the built-in cost.  The episode batches have their own
        ``set_cost_terms`` (``control/batched.py``, DESIGN 10.8: one table for the batch or one per episode).  Covered: both
        rollout engines and all six episode-batch classes, with constant targets, tracked references, action rates,
        one-sided bounds, quadratic forms with full matrices, signed linear rows, world positions of points on any body, world directions of body axes and world linear and angular velocities.  Not covered: the fused launches, ``AnalyticRolloutEngine``, world sizes above 1.

        Terms with a ``reference=`` are costed by ``mjmpc_cost_terms_track``: their reference goes to the device
        with an env-time counter (``track_step()``, 0 now) that every plan reads and every step of the controlled env
        (``step_state``, a ``(1, 1)`` rollout under ``real_step_guard``) advances by one inside its launch; a guarded rollout
        of another shape raises ``ValueError``.  ``set_track_step(n)`` tells an engine that only plans what time it is.

        Terms with ``action_rate=`` rows or a one-sided kind are costed by ``mjmpc_cost_terms_rate``, tracked or
        not.  With rate rows the engine keeps the action last applied to the controlled env on the device (``prev_action()``,
        all NaN now: nothing applied, the first rate is 0): every plan's first step reads it and every step of the controlled
        env records its action there inside its launch, with the same restriction on guarded rollouts.
        ``set_prev_action(a)`` tells an engine that only plans which action was applied.

        Terms with a quadratic group or a signed linear row are costed by ``mjmpc_cost_terms_quad``, which serves
        every other row too: the groups' matrices go to the device as one pool (``CostTerms.quad_table``); counter and previous
        action behave exactly as on the rate path.

        Terms that name points or differences (``CostTerms.point`` / ``difference``) put one launch,
        ``mjmpc_points``, in front of whichever cost entry the table takes: it copies the next observations into a buffer of the
        engine's with the world positions of the points, at each row's own ``qpos``, behind every row, and the cost entry reads
        that buffer with ``d_obs + n_extra`` entries a row (``cost_observations()`` returns it).  The observations a rollout
        returns keep their width; the counter, the previous action, ``terminal`` and the guard behave as without points; a table
        without points launches nothing new.  With an axis, a velocity or an angular velocity (``CostTerms.axis`` / ``velocity`` /
        ``angular_velocity``) that launch is ``mjmpc_points_motion``, which reads the row's ``qvel`` too; with a centre
        of mass (``CostTerms.com`` / ``com_velocity``) it is ``mjmpc_points_tree``, and the table is refused
        (``ValueError``) once ``randomize_dynamics`` has drawn ``body_mass``, as that call is refused after this one; with an
        orientation (``CostTerms.orientation``) it is ``mjmpc_points_orient`` for the whole program; everything
        else is as with points."""
        if self._closure_terms is not None and self._closure_terms != (terms is not None):
            raise RuntimeError("set_cost_terms: this engine has handed out a rollout_fn made %s cost terms, which offers the "
                               "controllers %s; set the terms first, then call make_device_rollout_fn"
                               % (("with", "no fused launches") if self._closure_terms else ("without", "the fused launches")))
        if terms is None:
            self._cost_terms = self._terms_dev = self._track_ref = self._track_step = self._prev_action = None
            self._terms_quad = self._points = self._points_last = self._points_levels = None
            self._terms_read_actions = self._terms_rate = self._points_orient = False
            return
        table = np.ascontiguousarray(terms.table(self), np.float64)       # (ValueError before anything reaches the device)
        refuse_mass_randomization(terms, self._mass_randomized)           # 
        ref = terms.reference_table(self)
        pool = terms.quad_table(self)
        points = terms.points_table(self)
        torch = _torch()
        self._points = self._points_last = self._points_levels = None
        self._points_orient = False
        if points is not None:
            # (every cost launch is preceded by mjmpc_points into a buffer of the engine's)
            # (with an axis or a velocity the table has a fifth entry, the node rows' qvel addresses, and the
            # launch is mjmpc_points_motion)
            dofadr = torch.from_numpy(points[4]).to(self.device) if len(points) > 4 else None
            # (with a centre of mass a sixth, the saved frames of the program, and the launch is mjmpc_points_tree)
            self._points = (torch.from_numpy(points[0]).to(self.device),) + tuple(points[1:4]) + (int(terms.n_extra), dofadr)
            self._points_levels = points[5] if len(points) > 5 else None
            # (with an orientation a seventh, and the launch is mjmpc_points_orient)
            self._points_orient = len(points) > 6
        self._terms_dev = torch.from_numpy(table).to(self.device)
        self._terms_rate = bool(terms.needs_rate_entry)
        self._terms_quad = None
        if terms.needs_quad_entry:
            # (a table with linear rows alone still hands the entry a pool: one zero nothing reads)
            self._terms_quad = torch.from_numpy(pool if pool is not None else np.zeros(1)).to(self.device)
        # (the rate and quad entries want the actions)
        self._terms_read_actions = bool(np.any(table[:, 1] != 0)) or self._terms_rate or self._terms_quad is not None
        self._cost_terms = terms
        self._track_ref = self._track_step = self._prev_action = None
        if terms.reads_action_rate:
            # rate rows: the previous action lives on the device; NaN: none has been applied yet
            self._prev_action = torch.full((self.d_action,), float("nan"), dtype=torch.float64, device=self.device)
        if ref is not None:
            # tracked terms: the reference and the env-time counter live on the device; time 0 is now
            self._track_ref = torch.from_numpy(ref).to(self.device)
            self._track_periodic = int(terms.periodic)
            self._track_step = torch.zeros(1, dtype=torch.int64, device=self.device)

    def set_track_step(self, n):
        """The env time of the tracked terms' reference becomes ``n``: a fill of the device counter in stream
        order, no synchronisation.  For loops whose controlled env is another object, whose steps this engine cannot see:
        call it before each plan.  ``step_state`` and a rollout under ``real_step_guard`` advance the counter by one
        themselves; ``set_cost_terms`` resets it to 0; ``set_env_state`` leaves it alone - a state does not say what
        time it is.  A host edit like ``set_env_state``: with a controller's ``lookahead``, ``reset()`` it first."""
        if self._track_step is None:
            raise RuntimeError("set_track_step: no tracked cost terms are set (CostTerms with reference=)")
        self._track_step.fill_(int(n))

    def track_step(self):
        """The env time of the tracked terms' reference, read back from the device (synchronises the stream)."""
        if self._track_step is None:
            raise RuntimeError("track_step: no tracked cost terms are set (CostTerms with reference=)")
        return int(self._track_step.item())

    def set_prev_action(self, action):
        """The action last applied to the controlled env, as the action-rate terms see it, becomes ``action``
        (numpy ``(A,)`` or a CUDA float64 tensor; ``None``: no action yet - an episode's start, where the first rate is 0): a
        copy or a fill in stream order, no synchronisation.  For loops whose controlled env is another object: call it before
        each plan, beside ``set_track_step``.  ``step_state`` and a rollout under ``real_step_guard`` record their action
        themselves; ``set_cost_terms`` resets it to "none"; ``set_env_state`` leaves it alone.  A host edit like
        ``set_env_state``: with a controller's ``lookahead``, ``reset()`` it first."""
        if self._prev_action is None:
            raise RuntimeError("set_prev_action: no action-rate cost terms are set (CostTerms with action_rate=)")
        if action is None:
            self._prev_action.fill_(float("nan"))
        else:
            self._prev_action.copy_(self._as_device(action, _torch().float64, (self.d_action,)), non_blocking=True)

    def prev_action(self):
        """The action-rate terms' previous action, float64 ``(A,)`` read back from the device (synchronises the stream); NaN
        entries: no action has been applied yet."""
        if self._prev_action is None:
            raise RuntimeError("prev_action: no action-rate cost terms are set (CostTerms with action_rate=)")
        return self._prev_action.cpu().numpy().copy()

    def cost_observations(self):
        """The augmented observations of the last cost launch with points: ``[P][H][d_obs + n_extra]`` (a
        ``step_state``: ``[d_obs + n_extra]``) in the engine's dtype, on the device - the next observations bit for bit, then
        three entries per point and per difference.  The engine's own buffer: the next launch of that shape rewrites it."""
        if self._points is None or self._points_last is None:
            raise RuntimeError("cost_observations: no cost terms with points have been launched (CostTerms.point)")
        return self._points_last

    def _launch_cost_terms(self, P, H, nobs, act, costs, terminal, advance=False):
        d_obs = self.d_obs
        if self._points is not None:
            #  the world positions first: the cost entry below then sees d_obs + n_extra entries a row.  The
            # controlled env's step has a buffer of its own, so a loop of plans and steps never reallocates (captures)
            program, n_rows, n_points, n_diff, n_extra, dofadr = self._points
            step = (P, H) == (1, 1)
            aug = self._buffer("points_step" if step else "points_obs",
                               (self.d_obs + n_extra,) if nobs.dim() == 1 else (P, H, self.d_obs + n_extra))
            #  with axes or velocities - a dof-address table - the launch reads qvel, the nv entries behind qpos, too
            _lib.check(launch_points(self._lib, self._code, P * H, self.d_obs, self._nq, self.model.nv, _ptr(nobs), _ptr(program),
                                     _ptr(dofadr), n_rows, n_points, n_diff, _ptr(aug), self._stream(), self._points_levels,
                                     self._points_orient))
            self._points_last = nobs = aug
            d_obs += n_extra
        t = self._terms_dev
        act = _ptr(act if self._terms_read_actions else None)
        keep = int(self._cost_terms.keep_builtin)
        if self._terms_quad is not None:
            # (the rate entry's arguments and the pool)
            r, q = self._track_ref, self._terms_quad
            _lib.check(self._lib.mjmpc_cost_terms_quad(
                self._code, P, H, d_obs, self.d_action, _ptr(nobs), act, _ptr(t), t.shape[0], keep, int(bool(terminal)),
                _ptr(r), 0 if r is None else r.shape[0], 0 if r is None else r.shape[1], self._track_periodic,
                _ptr(self._track_step), 0, int(bool(advance)), _ptr(self._prev_action), _ptr(q), q.shape[0], _ptr(costs),
                self._stream()))
            return
        if self._terms_rate:
            # (tracked or not, and as below the advance - counter and previous action - is part of the launch)
            r = self._track_ref
            _lib.check(self._lib.mjmpc_cost_terms_rate(
                self._code, P, H, d_obs, self.d_action, _ptr(nobs), act, _ptr(t), t.shape[0], keep, int(bool(terminal)),
                _ptr(r), 0 if r is None else r.shape[0], 0 if r is None else r.shape[1], self._track_periodic,
                _ptr(self._track_step), 0, int(bool(advance)), _ptr(self._prev_action), _ptr(costs), self._stream()))
            return
        if self._track_step is None:
            _lib.check(self._lib.mjmpc_cost_terms(self._code, P, H, d_obs, self.d_action, _ptr(nobs), act, _ptr(t),
                                                  t.shape[0], keep, int(bool(terminal)), _ptr(costs), self._stream()))
            return
        # (the advance is part of the library launch, not a torch op: a captured iteration keeps its launch tape)
        r = self._track_ref
        _lib.check(self._lib.mjmpc_cost_terms_track(self._code, P, H, d_obs, self.d_action, _ptr(nobs), act, _ptr(t),
                                                    t.shape[0], keep, int(bool(terminal)), _ptr(r), r.shape[0], r.shape[1],
                                                    self._track_periodic, _ptr(self._track_step), 0, int(bool(advance)),
                                                    _ptr(costs), self._stream()))

    def _refuse_with_terms(self, what):
        if self._cost_terms is not None:
            raise RuntimeError("%s evaluates the built-in cost inside the rollout kernel and cannot see the table of "
                               "set_cost_terms; use rollout_device (a rollout_fn made by make_device_rollout_fn after "
                               "set_cost_terms takes the generic iteration), or set_cost_terms(None)" % what)

    def get_state_device(self):
        """The device-resident state as the task's state dictionary (one D2H copy; synchronises the stream)."""
        qp, qv = np.zeros(self._nq), np.zeros(self.model.nv)
        _lib.check(self._fn("get_state")(self._h, qp.ctypes.data_as(_lib._dp), qv.ctypes.data_as(_lib._dp), self._stream()))
        if self.on_env_reset != "ignore":
            self.check_env_resets("the device-resident env (step_state)")     # (the host has synchronised anyway)
        if self.forward_task:
            return dict(qpos=qp, qvel=qv)
        return dict(qp=qp, qv=qv, qa=np.zeros(self.model.nv), target_pos=self._state["target_pos"].copy(), timestep=0)

    # ------------------------------------------------------------------ raw state shards (episode batches: control/batched.py)
    def set_shard_states_raw(self, states):
        """``len(states)`` unpacked states (``_unpack``) become the engine's state shards, whatever ``num_shards`` is: an
        episode batch's real envs.  ``set_env_state`` / ``get_env_state`` do not know about them."""
        arr = self._pack_shard_states(states)
        _lib.check(self._fn("set_shard_states")(self._h, arr.ctypes.data_as(_lib._dp), len(states), self._stream()))
        self._n_raw_shards = len(states)

    def get_shard_states(self):
        """The state shards of ``set_shard_states_raw`` -> (qpos [n, nq], qvel [n, nv]) (one D2H copy; synchronises the stream)."""
        qp, qv = np.zeros((self._n_raw_shards, self._nq)), np.zeros((self._n_raw_shards, self.model.nv))
        _lib.check(self._fn("get_shard_states")(self._h, qp.ctypes.data_as(_lib._dp), qv.ctypes.data_as(_lib._dp),
                                                self._stream()))
        return qp, qv

    def _counter(self, name):
        c = ctypes.c_uint32()
        _lib.check(self._fn(name)(self._h, ctypes.byref(c)))
        return int(c.value)

    def solver_failures(self):
        return self._counter("solver_failures")

    def diverged_substeps(self):
        """Resets: particle-substeps in which MuJoCo's mj_checkPos / mj_checkVel / mj_checkAcc would have called mj_resetData
        (a NaN or an entry beyond 1e10 in qpos / qvel / qacc); the kernel does the same and the particle rolls on from
        qpos0 with finite costs - counted apart from solver_failures()."""
        return self._counter("diverged")

    # ------------------------------------------------------------------ helpers
    def _stream(self):
        return ctypes.c_void_p(_torch().cuda.current_stream(self.device).cuda_stream)

    def _buffer(self, name, shape):
        torch = _torch()
        t = self._buf.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = torch.empty(shape, dtype=self._tdtype, device=self.device)
            self._buf[name] = t
        return t

    def _q0_buffer(self, P, q0_out=None):
        """Where a launch writes its cost-to-go: ``q0_out`` (float64 [P]), or the engine's own buffer of that shape."""
        torch = _torch()
        q0 = q0_out if q0_out is not None else self._buf.get("q0")
        if q0 is None or q0.shape[0] != P:
            q0 = self._buf["q0"] = torch.empty(P, dtype=torch.float64, device=self.device)
        return q0

    def _as_device(self, x, tdtype, shape):
        torch = _torch()
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(x))
        if tuple(x.shape) != tuple(shape):
            raise ValueError("expected shape %s, got %s" % (shape, tuple(x.shape)))
        return x.to(device=self.device, dtype=tdtype).contiguous()


def make_device_rollout_fn(sim_env):
    """Device-resident ``rollout_fn``: costs and actions come back as CUDA tensors (no observations,
    which the MPPI / CEM / DMD / random-shooting updates never read - SURVEY 8b), so one control
    iteration moves nothing across PCIe but the final action."""
    def rollout_fn(num_particles, horizon, mean, noise, mode):
        t0 = time.time()
        costs, act, _, _ = sim_env.rollout_device(num_particles, horizon, mean, noise, mode, want_obs=False)
        return dict(costs=costs, actions=act, observations=None, next_observations=None, dones=None,
                    infos={"total_time": np.array([time.time() - t0] * sim_env.num_shards)})
    rollout_fn.accepts_device = True          # controllers may hand over their device-resident mean
    rollout_fn.engine = sim_env
    if isinstance(sim_env, RolloutEngine):
        sim_env._closure_terms = sim_env._cost_terms is not None
        if sim_env._closure_terms:
            # the fused launches cost inside the rollout kernel and cannot see the table: without them on the closure every
            # controller takes the generic device iteration (rollout_device + its update launches), captured or eager
            return rollout_fn
    if hasattr(sim_env, "rollout_fused"):   # filter + cost-to-go fused into the launch (graph fast path)
        rollout_fn.fused = sim_env.rollout_fused
    if hasattr(sim_env, "mppi_step"):       # the whole iteration in one launch (captured iterations of MPPI / DMD-MPC)
        rollout_fn.mono = sim_env.mppi_step
        rollout_fn.sampled = sim_env.rollout_sampled     # rollouts that draw their own samples (any update that reads q0 / actions)
        rollout_fn.mono_launcher = sim_env.mppi_step_launcher
        rollout_fn.combine_launcher = sim_env.mppi_combine_launcher
    return rollout_fn


def make_rollout_fn(sim_env):
    """The ``rollout_fn`` closure of examples/example_mpc.py:112-133 over any engine with a
    reference-shaped ``rollout``: negates rewards into costs and builds the trajectory dict."""
    def rollout_fn(num_particles, horizon, mean, noise, mode):
        obs, rew, act, done, info, nobs = sim_env.rollout(num_particles, horizon, np.array(mean, copy=True),
                                                          noise, mode)
        infos = {k: np.array([d[k] for d in info]) for k in info[0]}
        return dict(observations=obs, actions=act, costs=-1.0 * rew, dones=done,
                    next_observations=nobs, infos=infos)
    return rollout_fn
