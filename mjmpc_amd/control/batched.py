"""Episode batches: E independent MPPI, CEM, PFMPC, DMD-MPC, random-shooting or MPPIQ episodes side by side on the tree engine
(DESIGN 10, 10.2 - 10.6).

The reference runs its experiments one episode after another (examples/job_script.py:80-99, the episode loop of
examples/example_mpc.py), each with its own seed (``seed + i*12345``) and start state, and its "tune" mode multiplies
that loop by a grid of hyperparameters.  One small population leaves most of the MI355X idle; ``BatchedMPPI`` runs the
episodes together instead.  A control step of the whole batch is four launches, with no host synchronisation:

    batched Philox draw -> one rollout launch (grid row = episode) -> batched fused update -> batched real-env step

Episode e computes the bits that the single-episode device path computes for it - ``MPPI(..., noise_mode='device',
seed=seeds[e])`` on a ``TreeRolloutEngine`` of its own, ``make_device_rollout_fn`` and
``enable_graph(post_step=engine.step_state)`` - so a batch replaces that loop exactly, not statistically.

    batch = BatchedMPPI(half_cheetah_raw(), num_episodes=8, horizon=32, num_particles=512, lam=0.2, step_size=1.0,
                        init_cov=0.3, gamma=1.0, filter_coeffs=[0.25, 0.8, 0.0], base_action="null",
                        seeds=[123 + i * 12345 for i in range(8)])
    batch.set_states(start_states)                  # one state dict per episode
    actions, costs, next_obs = batch.run(100)       # [T][E][A], [T][E], [T][E][d_obs]

Per episode: seed, start state (with ``target_pos``), initial mean, ``lam``, ``step_size`` and ``init_cov`` - and, after
``randomize_dynamics``, the model blocks its particle shards roll out (shared by the episodes, or a set per episode).  Shared by
the batch: the model, ``horizon``, ``num_particles`` (per episode), ``gamma``, ``filter_coeffs``, ``base_action`` and
the dtype.  The batch's E real envs are the state shards of the batch's own engine (``mjmpc_tree_step_shard_states``).

``BatchedCEM`` is the same batch for the cross-entropy method (cem.py): per episode also ``elite_frac`` and
``beta``, and a covariance that is refitted from the elites on the device.  ``BatchedPFMPC`` is the batch of particle-filter
MPC (particle_filter_controller.py, ``noise_mode='device'``): per episode ``lam``, ``cov_shift`` and
``cov_resample``, and a particle set that is resampled on the device.  ``BatchedDMDMPC`` is the batch of DMD-MPC with an
adapting covariance (gaussian_dmd.py with ``update_cov=True``): per episode ``lam``, ``step_size``, ``init_cov``
and ``beta``, and a ``'diagonal'`` or ``'full'`` covariance that is re-estimated from the weighted samples, grown by
``beta I`` and factored on the device every step (``update_cov=False`` is ``BatchedMPPI``'s arithmetic).
``BatchedRandomShooting`` is the batch of random shooting (random_shooting.py): per episode ``step_size`` and
``init_cov``, and a mean that moves towards the best sample of the step.  ``BatchedMPPIQ`` is the batch of MPPIQ (mppiq.py;
DESIGN 10.6): per episode ``beta``, ``step_size``, ``init_cov`` and ``td_lam``, TD(lambda) returns of the per-step costs and a
softmax per horizon step.

Every class takes ``engine="tree"`` (the default, all of the above) or ``engine="arm"``: the same batch on
``ArmRolloutEngine`` for the models the arm kernels run without slide joints or friction loss (``reacher_7dof-v0``), with
``num_particles`` a multiple of 8.  The sampler and the update launches are the same; the rollout and the real-env step are the
arm kernels' episode-batch twins (``mjmpc_arm_rollout_fused_batch``, ``mjmpc_arm_step_shard_states``).  Episode e's rollout rows
are, bit for bit, those of a plain ``mjmpc_arm_rollout_fused`` launch of all ``E * num_particles`` particles under its state and
mean (the arm kernels choose their launch shape from the grid), its env steps those of ``mjmpc_arm_step_state``.  Dynamics
randomization stays with ``engine="tree"``.  The classes share
``_EpisodeBatch``: the engine, the state shards, the buffers, the rollout launch, the env step, ``run``, dynamics
randomization, the step frame, the bound checks, the covariance status and ``set_cost_terms``: a user-defined
cost (``envs/cost_terms.py``) for every class on both engines, one table for the batch or one per episode with its own weights
and targets.
"""
import ctypes

import numpy as np

from .. import _lib
from ..envs.cost_terms import launch_points, refuse_mass_randomization
from ._device import noise_factor
from .controller import _SHIFT_MODES, _seed_value


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _per_episode(name, value, E, shape=(), sign=None):
    """One value for every episode, or one per episode -> float64 [E, *shape].  ``sign``: ``'positive'`` or ``'not negative'``,
    what every value must be (a NaN is neither)."""
    a = np.asarray(value, np.float64)
    if a.shape != tuple(shape) and a.shape != (E,) + tuple(shape):
        raise ValueError("%s takes one value of shape %s for every episode or %d of them, shape %s; got shape %s"
                         % (name, tuple(shape), E, (E,) + tuple(shape), a.shape))
    if sign is not None and not np.all(a > 0 if sign == "positive" else a >= 0):
        raise ValueError("%s must %s" % (name, "be positive" if sign == "positive" else "not be negative"))
    return np.broadcast_to(a, (E,) + tuple(shape)).copy()


def _cov(self):
    """The E action covariances, ``(E, A, A)`` (synchronises)."""
    out = self._covs.cpu().numpy().copy()
    self._check_status()
    return out


class _EpisodeBatch:
    """What the episode batches share: the checks of the common settings, the engine whose state shards are the E real envs,
    the device buffers of the rollout launch, the env step, ``run`` and dynamics randomization.  A subclass checks its own
    settings, calls ``_check_common`` and ``_compile`` (both raise ``ValueError`` and touch no device), then ``_setup``,
    and provides ``_launches``, its own launches of a ``step``."""

    _status = None      # int32 [E] on the device in the batches whose kernels can flag an episode's covariance
    _engine_kind = "tree"   # ``engine=``: "tree" (TreeRolloutEngine) or "arm" (ArmRolloutEngine)
    _track = None           # tracked terms: (references on the device [1 or E][N][R], N, R, per episode?, periodic)
    _track_bias = 0         # env time of the references = _step_dev + _track_bias (set_track_step)
    _rate = False           # the tables hold action-rate rows or one-sided kinds: mjmpc_cost_terms_rate_batch
    _prev_actions = None    # ... with rate rows every episode's last applied action, float64 [E][A] on the device (NaN: none yet)
    _quad = None            # the tables hold quadratic groups or signed linear rows: mjmpc_cost_terms_quad_batch with
                            # this pool of matrices on the device, one for all episodes
    _cost_terms_set = None  # set_cost_terms' argument, _mass_randomized: randomize_dynamics drew body_mass (DESIGN 12.6 refuses a
    _mass_randomized = None  # centre of mass beside it)
    _points_levels = None   # ... the saved frames of its program: a centre of mass, mjmpc_points_tree
    _points_orient = False  # ... whether it holds an orientation: mjmpc_points_orient
    _points = None          # the tables name points: (program, n_rows, n_points, n_diff, d_obs + n_extra, the augmented
                            # observations of the rollouts [E P][H][.] and of the real-env steps [E][.], the node rows' qvel
                            # addresses - None without axes and velocities)
    _terms = None           # set_cost_terms: (tables on the device, rows, per episode?, keep_builtin, a row reads an action?)
    _terms_nobs = None      # ... the rollouts' next observations [E P][H][d_obs] (only while terms are set)
    _terms_env = None       # ... the real-env step's own next observations [E][d_obs] and actions [E][A] in the batch's dtype

    def _pick_engine(self, engine, num_particles):
        """The first refusals of every constructor: the ``engine`` keyword, and what the arm engine asks of the population."""
        if engine not in ("tree", "arm"):
            raise ValueError("engine must be 'tree' or 'arm', got %r" % (engine,))
        if engine == "arm" and int(num_particles) % 8 != 0:
            raise ValueError("with engine='arm' every episode holds a multiple of 8 particles (a particle group of the arm "
                             "kernels must not straddle two episodes), got num_particles = %d" % int(num_particles))
        self._engine_kind = engine

    @staticmethod
    def _check_common(num_episodes, horizon, num_particles, n_iters, base_action, use_zero_control_seq, sample_mode, dtype,
                      gamma, filter_coeffs, what):
        """The settings every batch refuses alike -> (E, H, P, filter coefficients)."""
        E, H, P = int(num_episodes), int(horizon), int(num_particles)
        if not 1 <= E <= 65535:
            raise ValueError("num_episodes must be in [1, 65535], got %d" % E)
        if H < 1 or P < 1:
            raise ValueError("horizon and num_particles must be positive")
        if n_iters != 1:
            raise ValueError("an episode batch runs one %s iteration per control step (n_iters = 1), got %r" % (what, n_iters))
        if base_action not in ("null", "repeat"):
            raise ValueError("base_action must be 'null' or 'repeat' in an episode batch, got %r" % (base_action,))
        if use_zero_control_seq:
            raise ValueError("an episode batch does not run use_zero_control_seq")
        if sample_mode != "mean":
            raise ValueError("an episode batch acts with the mean (sample_mode 'mean'), got %r" % (sample_mode,))
        if dtype not in ("f64", "f32"):
            raise ValueError("dtype must be 'f64' or 'f32'")
        if float(gamma) == 0.0:
            raise ValueError("gamma = 0 leaves zeros in the discount sequence, which the fused update does not take")
        fc = np.asarray(filter_coeffs, np.float64).reshape(-1)
        if fc.size != 3:
            raise ValueError("filter_coeffs must hold three coefficients")
        return E, H, P, fc

    @staticmethod
    def _check_seeds(seeds, E):
        seeds = list(seeds) if isinstance(seeds, (list, tuple, np.ndarray)) else None
        if seeds is None or len(seeds) != E:
            raise ValueError("seeds must hold one seed per episode (%d)" % E)
        return [_seed_value(int(s) if isinstance(s, (np.integer,)) else s) for s in seeds]

    @staticmethod
    def _compile(raw_model):
        """The tree engine's model, or ``ValueError`` for a model it refuses."""
        from ..models.compile_tree import TreeModel, compile_tree
        try:
            model = raw_model if isinstance(raw_model, TreeModel) else compile_tree(raw_model)
        except (ValueError, NotImplementedError, TypeError, AttributeError) as e:
            raise ValueError("the tree engine cannot run this model: %s" % e) from e
        gen = int(model.field("gen")[0])
        if model.integrator == "RK4" and (model.nv > 16 or gen >= 3):
            raise ValueError("the tree engine runs RK4 models of up to 16 dofs without elliptic friction cones")
        return model

    @staticmethod
    def _compile_arm(raw_model):
        """The arm engine's model, or ``ValueError`` for a model it refuses or has no episode-batch kernels for."""
        from ..models.compile import ArmModel, compile_arm
        try:
            model = raw_model if isinstance(raw_model, ArmModel) else compile_arm(raw_model)
        except (ValueError, NotImplementedError, TypeError, AttributeError) as e:
            raise ValueError("the arm engine cannot run this model (engine='tree' runs the general models): %s" % e) from e
        if np.any(model.field("jtype") != 0) or np.any(model.field("frictionloss") > 0):
            raise ValueError("the arm engine's extended-joint kernels (slide joints, friction loss) have no episode-batch "
                             "twins: run this model with engine='tree'")
        return model

    def _seeds_and_model(self, seeds, E, raw_model):
        """The last two refusals of every constructor: ``seed_vals`` and the compiled model."""
        self.seed_vals = self._check_seeds(seeds, E)
        return self._compile_arm(raw_model) if self._engine_kind == "arm" else self._compile(raw_model)

    @staticmethod
    def _init_mean(init_mean, E, H, A):
        return np.zeros((E, H, A)) if init_mean is None else _per_episode("init_mean", init_mean, E, (H, A))

    @staticmethod
    def _diag_factors(var, A):
        """``diag(var_e)`` per episode, as the controllers take a scalar covariance, and what the sampler colours with
        (``noise_factor``) -> the covariances [E, A, A], their lower factors [E, A, A] and the factors' diagonal flags."""
        covs = np.stack([np.diag(np.full(A, c)) for c in var])
        factors = [noise_factor(c) for c in covs]
        return covs, np.stack([f[0] for f in factors]), [f[1] for f in factors]

    def _setup(self, raw_model, model, E, H, P, dtype, device, base_action, gamma, fc, init_mean):
        """The engine (its state shards are the E real envs) and the device buffers every batch has."""
        from ..models.raw import RawModel
        import torch
        self.torch = torch
        if self._engine_kind == "arm":
            from ..envs.arm_engine import ArmRolloutEngine
            self.engine = ArmRolloutEngine(model, device=device, dtype=dtype)
        else:
            from ..envs.tree_engine import TreeRolloutEngine
            self.engine = TreeRolloutEngine(model, device=device, dtype=dtype)
        self.lib = self.engine._lib
        self.model = model
        self.raw = raw_model if isinstance(raw_model, RawModel) else None
        self.engine.raw = self.raw      # (the engine was made from the compiled model; CostTerms.point reads the bodies' poses)
        self.shard_blobs = None         # randomize_dynamics: the model blocks of the rollouts, [sets][num_shards][blob length]
        A = model.nu
        self.num_episodes, self.horizon, self.num_particles, self.d_action = E, H, P, A
        self.d_obs, self.dtype = model.d_obs, dtype
        self.forward_task = self.engine.forward_task
        self.base_action, self.gamma, self.filter_coeffs = base_action, float(gamma), fc.copy()
        self.init_mean = init_mean
        self.num_steps = 0
        dev = self.device = torch.device("cuda", device)
        self._code = _lib.F32 if dtype == "f32" else _lib.F64
        tdt = self._tdtype = torch.float32 if dtype == "f32" else torch.float64
        f64 = dict(dtype=torch.float64, device=dev)
        self._means = self._upload(init_mean)
        self._gseq = self._upload(np.cumprod([1.0] + [self.gamma] * (H - 1)))     # (Controller.gamma_seq)
        self._coeffs = self._upload(fc)
        self._seeds = self._upload(np.array(self.seed_vals, np.uint64).view(np.int64))
        self._step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self._noise = torch.empty((E, P, H, A), dtype=tdt, device=dev)
        self._costs = torch.empty((E * P, H), dtype=tdt, device=dev)
        self._actions = torch.empty((E * P, H, A), dtype=tdt, device=dev)
        self._q0 = torch.empty(E * P, **f64)
        self._act = torch.empty((E, A), **f64)
        self._env_cost = torch.empty(E, dtype=tdt, device=dev)
        self._env_obs = torch.empty((E, self.d_obs), dtype=tdt, device=dev)
        self.set_states([dict(qp=self.engine._start_qpos(), qv=np.zeros(model.nv), target_pos=model.target_default.copy())] * E)
        return f64

    def _upload(self, a):
        """A host array on the batch's device (a copy: the host array stays the caller's)."""
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def _workspace(self, nbytes):
        """``nbytes`` of device workspace, as a library ``*_workspace_bytes`` call sized it (negative: that call's error)."""
        if nbytes < 0:
            _lib.check(int(nbytes))
        return self.torch.empty((nbytes + 7) // 8, dtype=self.torch.float64, device=self.device)

    def _coeffs_unless_identity(self):
        """The filter coefficients on the device, or None where the filter leaves the samples as they are."""
        fc = self.filter_coeffs
        return None if fc[0] == 1.0 and fc[1] == 0.0 and fc[2] == 0.0 else self._coeffs

    # ------------------------------------------------------------------ state of the E real envs
    @property
    def on_env_reset(self):
        """What a reset of a real env does where ``run`` / ``get_states`` synchronise (``envs/_resets.py``)."""
        return self.engine.on_env_reset

    @on_env_reset.setter
    def on_env_reset(self, mode):
        self.engine.on_env_reset = mode

    def set_states(self, states):
        """One state dict per episode, in the env classes' format: ``{qp, qv, target_pos}`` or ``{qpos, qvel}``."""
        if len(states) != self.num_episodes:
            raise ValueError("set_states takes one state per episode (%d), got %d" % (self.num_episodes, len(states)))
        unpacked = [self.engine._unpack(s) for s in states]
        self.engine.set_shard_states_raw(unpacked)
        self._targets = [s["target_pos"].copy() for s in unpacked]

    def get_states(self):
        """The E real envs' states as state dicts (one device-to-host copy; synchronises the stream)."""
        E, m = self.num_episodes, self.model
        qp, qv = self.engine.get_shard_states()
        self._check_resets()
        self._check_status()
        if self.forward_task:
            return [dict(qpos=qp[e].copy(), qvel=qv[e].copy()) for e in range(E)]
        return [dict(qp=qp[e].copy(), qv=qv[e].copy(), qa=np.zeros(m.nv), target_pos=self._targets[e].copy(), timestep=0)
                for e in range(E)]

    @property
    def mean_action(self):
        """The E means, ``(E, H, A)`` (synchronises)."""
        out = self._means.cpu().numpy().copy()
        self._check_status()
        return out

    def reset(self):
        """Every episode back to its initial mean and step 0 (the real envs keep their states: ``set_states``)."""
        self._means.copy_(self.torch.from_numpy(self.init_mean))
        self._step_dev.zero_()
        self.num_steps = 0
        self._track_bias = 0
        if self._prev_actions is not None:
            self._prev_actions.fill_(float("nan"))      # (no action has been applied in the new episodes)

    # ------------------------------------------------------------------ dynamics randomization
    def randomize_dynamics(self, param_dict, base_seed, num_shards):
        """``SubprocVecEnv.randomize_dynamics`` for every episode of the batch (the reference's ``example_mpc.py
        --dyn_randomize_config``): each episode's particles are split into ``num_shards`` shards of consecutive particles
        and shard i rolls out its own model block, while the E real envs keep the nominal model (the reference's randomized
        ``sim_env`` only does rollouts).  ``base_seed``: one int - every episode's shard i draws from
        ``np_random(base_seed + i*12345)``, one shared set of blocks, as the reference randomizes once before its episode
        loop - or one int per episode: episode e's shard i draws from ``np_random(base_seed[e] + i*12345)``.  Episode e then
        computes the bits of the single-episode path on ``TreeRolloutEngine(raw, num_shards=num_shards)`` after
        ``randomize_dynamics(param_dict, base_seed[e])`` and ``set_real_env_model('nominal')``.  Every call draws from the
        nominal model, as on a fresh engine.  Returns ``(default_params, randomized_params)``, one dict per shard - as a list
        per episode with per-episode seeds.  Raises ``ValueError`` before anything reaches the device."""
        from ..envs._engine import draw_shard_models
        from ..envs.tree_engine import TreeRolloutEngine
        self._tree_only("randomize_dynamics")
        E, K = self.num_episodes, int(num_shards)
        if not 1 <= K <= 65535 or self.num_particles % K != 0:
            raise ValueError("num_particles (%d) must divide into num_shards (%d) shards, 1 .. 65535" % (self.num_particles, K))
        if self.raw is None:
            raise ValueError("randomize_dynamics needs the batch to be built from a RawModel")
        refuse_mass_randomization(self._cost_terms_set, param_dict)      # (no centre of mass over randomized masses)
        per_episode = isinstance(base_seed, (list, tuple, np.ndarray))
        if per_episode and len(base_seed) != E:
            raise ValueError("base_seed takes one int or one per episode (%d), got %d" % (E, len(base_seed)))
        host = TreeRolloutEngine.host_only(self.raw, self.model)
        defaults, rand, blobs = [], [], []
        for seed in (base_seed if per_episode else [base_seed]):
            d, r = [dict() for _ in range(K)], [dict() for _ in range(K)]
            try:
                blobs.append(draw_shard_models(host, param_dict, [int(seed) + i * 12345 for i in range(K)], d, r))
            except (StopIteration, KeyError, IndexError) as e:
                raise ValueError("the model has no such dynamics parameter: %r" % (e,)) from e
            defaults.append(d)
            rand.append(r)
        blobs = np.ascontiguousarray(np.stack(blobs), np.float64)
        _lib.check(self.lib.mjmpc_tree_set_batch_models(self.engine._h, blobs.ctypes.data_as(_lib._dp), len(blobs), K))
        self.shard_blobs = blobs
        self._mass_randomized = {"body_mass": param_dict["body_mass"]} if "body_mass" in param_dict else None
        return (defaults, rand) if per_episode else (defaults[0], rand[0])

    def clear_dynamics(self):
        """Back to the one nominal model block for every rollout."""
        self._tree_only("clear_dynamics")
        _lib.check(self.lib.mjmpc_tree_set_batch_models(self.engine._h, None, 0, 0))
        self.shard_blobs = None
        self._mass_randomized = None

    # ------------------------------------------------------------------ user-defined cost terms
    def obs_layout(self):
        """Named slices of the observation (``RolloutEngine.obs_layout``): what ``CostTerms`` resolves ``obs=`` against."""
        return self.engine.obs_layout()

    @staticmethod
    def _resolve_cost_terms(terms, engine, E):
        """``set_cost_terms``'s argument, resolved and checked against ``engine`` on the host -> the tables float64
        ``[1 or E][K][8]`` (one ``CostTerms``: one table for every episode; a list: one per episode), ``keep_builtin`` and
        whether a row reads an action.  ``ValueError`` for anything else."""
        from ..envs.cost_terms import CostTerms
        per_episode = isinstance(terms, (list, tuple))
        each = list(terms) if per_episode else [terms]
        if per_episode and len(each) != E:
            raise ValueError("set_cost_terms takes one CostTerms for every episode or one per episode (%d), got %d"
                             % (E, len(each)))
        if not all(isinstance(t, CostTerms) for t in each):
            raise ValueError("set_cost_terms takes a CostTerms, a list of them or None")
        tables = [np.ascontiguousarray(t.table(engine), np.float64) for t in each]    # (an empty table, an index outside)
        keep, first = each[0].keep_builtin, tables[0]
        structure = [0, 1, 2, 5, 6, 7]              # kind, source, index, group, when, reserved: shared by the batch
        for e, (t, table) in enumerate(zip(each, tables)):
            if table.shape != first.shape:
                raise ValueError("set_cost_terms: episode %d's table has %d rows, episode 0's %d (the episodes share the "
                                 "rows; weights and targets may differ)" % (e, len(table), len(first)))
            if t.keep_builtin != keep:
                raise ValueError("set_cost_terms: episode %d's keep_builtin differs from episode 0's" % e)
            if not np.array_equal(table[:, structure], first[:, structure]):
                raise ValueError("set_cost_terms: episode %d's rows differ from episode 0's in kind, source, index, group or "
                                 "when (only weights and targets may differ between the episodes)" % e)
        pool = each[0].quad_table(engine)           # (one pool of matrices for the batch)
        for e, t in enumerate(each):
            other = t.quad_table(engine)
            if pool is not None and not np.array_equal(other, pool):
                raise ValueError("set_cost_terms: episode %d's quadratic matrices differ from episode 0's (the episodes share "
                                 "one pool of matrices; weights, targets and references may differ)" % e)
        points = each[0].points_table(engine)       # (one points program for the batch)
        for e, t in enumerate(each):
            other = t.points_table(engine)
            if (other is None) != (points is None) or (points is not None and (
                    len(other) != len(points) or other[1:4] != points[1:4] or not np.array_equal(other[0], points[0]))):
                # (a fifth entry, the dof addresses, follows from the program and the model)
                raise ValueError("set_cost_terms: episode %d's points or differences differ from episode 0's (the episodes "
                                 "share them; weights, targets and references may differ)" % e)
        return np.stack(tables), bool(keep), bool(np.any(first[:, 1] != 0))

    @staticmethod
    def _resolve_tracking(terms, engine, E):
        """The references of ``set_cost_terms``'s argument (already through ``_resolve_cost_terms``: the rows agree, the
        ``reserved`` column - which rows are tracked - included) -> ``(float64 [1 or E][N][R], periodic)``, or ``None`` without a
        tracked term.  The values may differ between the episodes; ``N`` and ``periodic`` are structure: ``ValueError``."""
        each = list(terms) if isinstance(terms, (list, tuple)) else [terms]
        refs = [t.reference_table(engine) for t in each]
        if refs[0] is None:
            return None
        for e, (t, r) in enumerate(zip(each, refs)):
            if r.shape[0] != refs[0].shape[0]:
                raise ValueError("set_cost_terms: episode %d's reference has %d rows, episode 0's %d (the episodes share N; "
                                 "the values may differ)" % (e, r.shape[0], refs[0].shape[0]))
            if t.periodic != each[0].periodic:
                raise ValueError("set_cost_terms: episode %d's periodic differs from episode 0's" % e)
        return np.ascontiguousarray(np.stack(refs), np.float64), bool(each[0].periodic)

    def set_track_step(self, n):
        """The env time of the tracked terms' references at the next control step becomes ``n``: reference row
        ``n + t + 1`` is the goal of the next plan's step ``t``.  Host side (``_track_bias = n - num_steps``: the device step
        counter goes on keying the noise); ``reset()`` puts the env time back to the step count, 0."""
        self._track_bias = int(n) - self.num_steps

    def set_cost_terms(self, terms):
        """From the next step on the rollouts and the real-env steps of every episode cost what ``terms`` say instead of
        the built-in cost (``envs/cost_terms.py``; ``keep_builtin``: on top of it).  ``terms``: a ``CostTerms`` for every
        episode, a list of ``num_episodes`` of them - the same rows with each episode's own weights and targets, e.g. a goal
        per episode or a sweep of the weights - or ``None``, which restores the built-in cost exactly.  The rollout launch
        then also writes the next observations (``mjmpc_<engine>_rollout_fused_batch_obs``) and one launch behind it
        (``mjmpc_cost_terms_batch``) rewrites the costs and forms the cost-to-go; the real-env step is followed by the same
        launch without the terminal rows.  Terms with a ``reference=`` (per episode the values may differ, ``N``,
        ``periodic`` and the tracked rows not) read their goals at env time ``num_steps`` (``set_track_step``: another) + the
        plan step through ``mjmpc_cost_terms_track_batch``.  Tables with ``action_rate=`` rows or one-sided kinds
        go through ``mjmpc_cost_terms_rate_batch``, tracked or not; with rate rows every episode's last applied action lives
        on the device (``_prev_actions``, NaN now and after ``reset()``: the first rate of an episode is 0) - the plans read
        it, the launch that costs the real-env step reads it and then records the step's action.  Tables with a quadratic group
        or a signed linear row go through ``mjmpc_cost_terms_quad_batch``, which serves every row: the groups'
        matrices are one pool for the batch - per episode the weights, targets and references may differ, the matrices not
        (``ValueError`` naming the episode).  Tables with points or differences put ``mjmpc_points`` over the
        ``E P H`` rows between the rollout and the cost entry, as the single engines do; the episodes share the points and
        differences (``ValueError`` naming the episode) and keep their own weights, targets and references; with axes,
        velocities or angular velocities the launch is ``mjmpc_points_motion``, shared in the same way, with a centre
        of mass ``mjmpc_points_tree`` - refused beside a ``randomize_dynamics`` of ``body_mass`` -, with an
        orientation ``mjmpc_points_orient``.  Everything is
        checked on the host first (``ValueError``); callable between steps."""
        if terms is None:
            self._terms = self._terms_nobs = self._terms_env = self._track = self._prev_actions = self._quad = None
            self._points = self._cost_terms_set = self._points_levels = None
            self._rate = self._points_orient = False
            return
        tables, keep, reads_actions = self._resolve_cost_terms(terms, self.engine, self.num_episodes)
        refuse_mass_randomization(terms, self._mass_randomized)         # 
        self._cost_terms_set = terms
        track = self._resolve_tracking(terms, self.engine, self.num_episodes)
        rate_rows = bool(np.any(tables[0][:, 1] == 2))
        kinds = tables[0][:, 0]
        self._rate = rate_rows or bool(np.any((kinds >= 4) & (kinds <= 7)))
        self._quad = None
        if np.any(kinds >= 8):
            pool = (terms[0] if isinstance(terms, (list, tuple)) else terms).quad_table(self.engine)
            self._quad = self._upload(pool if pool is not None else np.zeros(1))    # (linear rows alone: one zero nothing reads)
        reads_actions = reads_actions or self._rate or self._quad is not None       # (the rate and quad entries want the actions)
        self._track = None if track is None else (self._upload(track[0]), track[0].shape[1], track[0].shape[2],
                                                  int(track[0].shape[0] > 1), int(track[1]))
        torch, E, tdt, dev = self.torch, self.num_episodes, self._tdtype, self.device
        self._terms = (self._upload(tables), tables.shape[1], int(tables.shape[0] > 1), int(keep), reads_actions)
        self._terms_nobs = torch.empty((E * self.num_particles, self.horizon, self.d_obs), dtype=tdt, device=dev)
        # the real-env step's own next observations (a caller may pass none) and its actions in the batch's dtype
        self._terms_env = (torch.empty((E, self.d_obs), dtype=tdt, device=dev),
                           torch.empty((E, self.d_action), dtype=tdt, device=dev) if reads_actions else None)
        self._prev_actions = (torch.full((E, self.d_action), float("nan"), dtype=torch.float64, device=dev) if rate_rows
                              else None)
        self._points = self._points_levels = None
        self._points_orient = False
        first = terms[0] if isinstance(terms, (list, tuple)) else terms
        points = first.points_table(self.engine)
        if points is not None:
            #  one program for the batch; the augmented rows of the rollouts' and of the real-env steps' observations
            d_aug = self.d_obs + first.n_extra
            self._points = (self._upload(points[0]),) + tuple(points[1:4]) + (
                d_aug, torch.empty((E * self.num_particles, self.horizon, d_aug), dtype=tdt, device=dev),
                torch.empty((E, d_aug), dtype=tdt, device=dev),
                #  with axes or velocities the node rows' qvel addresses: mjmpc_points_motion
                torch.from_numpy(points[4]).to(dev) if len(points) > 4 else None)
            #  with a centre of mass the saved frames of the program: mjmpc_points_tree
            self._points_levels = points[5] if len(points) > 5 else None
            #  with an orientation the whole program goes through mjmpc_points_orient
            self._points_orient = len(points) > 6

    def _launch_cost_terms(self, P, H, nobs, act, costs, terminal, gseq, q0, s, bias=0, advance_prev=0):
        """``mjmpc_cost_terms_batch`` on ``[E P][H]`` costs with the batch's table(s); with tracked terms
        ``mjmpc_cost_terms_track_batch`` at env time ``_step_dev + bias``; with rate rows or one-sided kinds
        ``mjmpc_cost_terms_rate_batch`` (``advance_prev``: the E elements record their actions in ``_prev_actions``)."""
        tables, K, per_episode, keep, reads_actions = self._terms
        d_obs = self.d_obs
        if self._points is not None:
            #  the same launch as the single engines', over E P H rows: the cost entry reads the augmented rows
            program, n_rows, n_points, n_diff, d_aug, aug_rollout, aug_env, dofadr = self._points
            aug = aug_rollout if nobs is self._terms_nobs else aug_env
            _lib.check(launch_points(self.lib, self._code, self.num_episodes * P * H, d_obs, self.engine._nq, self.model.nv,
                                     _vp(nobs), _vp(program), _vp(dofadr), n_rows, n_points, n_diff, _vp(aug), s, self._points_levels,
                                     self._points_orient))
            nobs, d_obs = aug, d_aug
        if self._quad is not None:
            refs, N, R, ref_per_episode, periodic = self._track if self._track is not None else (None, 0, 0, 0, 0)
            _lib.check(self.lib.mjmpc_cost_terms_quad_batch(
                self._code, self.num_episodes, P, H, d_obs, self.d_action, _vp(nobs), _vp(act), _vp(tables), K, per_episode,
                keep, terminal, _vp(refs), N, R, ref_per_episode, periodic, _vp(self._step_dev) if refs is not None else None,
                bias, _vp(self._prev_actions), advance_prev, _vp(self._quad), self._quad.shape[0], _vp(costs), _vp(gseq),
                _vp(q0), s))
            return
        if self._rate:
            refs, N, R, ref_per_episode, periodic = self._track if self._track is not None else (None, 0, 0, 0, 0)
            _lib.check(self.lib.mjmpc_cost_terms_rate_batch(
                self._code, self.num_episodes, P, H, d_obs, self.d_action, _vp(nobs), _vp(act), _vp(tables), K, per_episode,
                keep, terminal, _vp(refs), N, R, ref_per_episode, periodic, _vp(self._step_dev) if refs is not None else None,
                bias, _vp(self._prev_actions), advance_prev, _vp(costs), _vp(gseq), _vp(q0), s))
            return
        if self._track is not None:
            refs, N, R, ref_per_episode, periodic = self._track
            _lib.check(self.lib.mjmpc_cost_terms_track_batch(
                self._code, self.num_episodes, P, H, d_obs, self.d_action, _vp(nobs), _vp(act) if reads_actions else None,
                _vp(tables), K, per_episode, keep, terminal, _vp(refs), N, R, ref_per_episode, periodic, _vp(self._step_dev),
                bias, _vp(costs), _vp(gseq), _vp(q0), s))
            return
        _lib.check(self.lib.mjmpc_cost_terms_batch(self._code, self.num_episodes, P, H, d_obs, self.d_action, _vp(nobs),
                                                   _vp(act) if reads_actions else None, _vp(tables), K, per_episode, keep,
                                                   terminal, _vp(costs), _vp(gseq), _vp(q0), s))

    # ------------------------------------------------------------------ control steps
    def step(self, _out=None):
        """Enqueue one control step of every episode - the subclass's ``_launches``, then the real-env step - without a host
        synchronisation.  The actions, real-env costs and next observations stay on the device."""
        act, cost, nobs = _out if _out is not None else (self._act, self._env_cost, self._env_obs)
        s = self._stream()
        self._launches(act, s)
        self._env_step(act, cost, nobs, s)
        self.num_steps += 1
        return act, cost, nobs

    def _launches(self, act, s):
        """The controller's own launches of one step on stream ``s``, up to the E actions in ``act``.  Every one is looked up
        on ``self.lib`` when it is made."""
        raise NotImplementedError

    def _rollout(self, s, noise=None, filtered=True, gseq=True, q0=True):
        """The batch's rollout launch: grid row = episode, the cost-to-go of every particle into ``_q0``.  ``noise``: the
        deviations from the means, ``_noise`` by default; ``filtered=False``: they are filtered already; ``gseq=False`` /
        ``q0=False``: no discount sequence / no cost-to-go (the update forms its own)."""
        E, P, H = self.num_episodes, self.num_particles, self.horizon
        if self._terms is not None:
            # the rollout with its next observations and no cost-to-go, then the terms: costs in place, q0 from the new costs
            _lib.check(self._fn("rollout_fused_batch_obs")(
                self.engine._h, self._code, E * P, H, _vp(self._means), _vp(self._noise if noise is None else noise),
                _vp(self._coeffs) if filtered else None, None, _vp(self._costs), _vp(self._actions), None,
                _vp(self._terms_nobs), s))
            self._launch_cost_terms(P, H, self._terms_nobs, self._actions, self._costs, 1, self._gseq if q0 else None,
                                    self._q0 if q0 else None, s, bias=self._track_bias)
            return
        _lib.check(self._fn("rollout_fused_batch")(
            self.engine._h, self._code, E * P, H, _vp(self._means), _vp(self._noise if noise is None else noise),
            _vp(self._coeffs) if filtered else None, _vp(self._gseq) if gseq else None, _vp(self._costs), _vp(self._actions),
            _vp(self._q0) if q0 else None, s))

    def _draw(self, s):
        """The batched Philox draw with the static factors ``_chols``, keyed with the step count: ``_noise``."""
        E, P, H, A = self.num_episodes, self.num_particles, self.horizon, self.d_action
        _lib.check(self.lib.mjmpc_sample_noise_batch(self._code, E, _vp(self._noise), P, H, A, _vp(self._chols), _vp(self._seeds),
                                                     0, _vp(self._step_dev), s))

    def _env_step(self, act, cost, nobs, s):
        """The E real envs take their episode's action in one launch; with cost terms a second launch costs the steps (no
        terminal rows: a real env's step is no plan's last step)."""
        if self._terms is None:
            _lib.check(self._fn("step_shard_states")(self.engine._h, self._code, _vp(act), _vp(cost), _vp(nobs), s))
            return
        own_obs, act_t = self._terms_env
        nobs = own_obs if nobs is None else nobs
        _lib.check(self._fn("step_shard_states")(self.engine._h, self._code, _vp(act), _vp(cost), _vp(nobs), s))
        if act_t is not None:
            act_t.copy_(act)                # (into the batch's dtype, as step_state does)
        # (every class's update launch has advanced _step_dev by now: the step that was planned at _step_dev - 1)
        self._launch_cost_terms(1, 1, nobs, act_t, cost, 0, None, None, s, bias=self._track_bias - 1, advance_prev=1)

    def run(self, T):
        """``T`` control steps of every episode -> actions ``[T][E][A]`` (float64), real-env costs ``[T][E]`` and next
        observations ``[T][E][d_obs]`` (the batch's dtype), brought back with one device-to-host copy at the end."""
        torch, T = self.torch, int(T)
        E, A, D = self.num_episodes, self.d_action, self.d_obs
        isz = 4 if self.dtype == "f32" else 8
        na, nc = 8 * T * E * A, isz * T * E
        buf = torch.empty(na + nc + isz * T * E * D, dtype=torch.uint8, device=self.device)
        acts = buf[:na].view(torch.float64).view(T, E, A)
        costs = buf[na:na + nc].view(self._tdtype).view(T, E)
        nobs = buf[na + nc:].view(self._tdtype).view(T, E, D)
        for t in range(T):
            self.step(_out=(acts[t], costs[t], nobs[t]))
        host = buf.cpu().numpy()
        self._check_resets()
        self._check_status()
        npt = np.float32 if self.dtype == "f32" else np.float64
        return (host[:na].view(np.float64).reshape(T, E, A).copy(), host[na:na + nc].view(npt).reshape(T, E).copy(),
                host[na + nc:].view(npt).reshape(T, E, D).copy())

    def close(self):
        self.engine.close()

    # ------------------------------------------------------------------ helpers
    def _fn(self, name):
        """The engine kind's entry point ``mjmpc_<tree|arm>_<name>``, looked up on ``self.lib`` when the launch is made."""
        return getattr(self.lib, "mjmpc_%s_%s" % (self._engine_kind, name))

    def _tree_only(self, what):
        if self._engine_kind != "tree":
            raise ValueError("%s: an arm batch rolls out one model block; per-episode model blocks need engine='tree'" % what)

    def _check_resets(self):
        if self.engine.on_env_reset != "ignore":
            self.engine.check_env_resets("an episode batch's real envs (step_shard_states)")

    def _check_status(self):
        """``DeviceUpdater.check_status`` per episode: raise for the episodes whose finish launch (``BatchedCEM``) or factor
        launch (``BatchedDMDMPC``) has flagged an indefinite or non-finite covariance (the flags are sticky on the device) and
        clear exactly the flags reported.  Nothing to check in a batch without ``_status``."""
        if self._status is None:
            return
        st = self._status.cpu().numpy()
        bad = np.nonzero(st)[0]
        if bad.size == 0:
            return
        self._status[self.torch.from_numpy(bad).to(self.device)] = 0
        raise _lib.MjmpcError("the action covariance of episode%s %s on the device is indefinite or not finite: its Cholesky "
                              "factor (sampler colouring) does not exist"
                              % ("" if bad.size == 1 else "s", ", ".join(str(int(e)) for e in bad)))

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)


class BatchedMPPI(_EpisodeBatch):
    """``num_episodes`` MPPI controllers (mppi.py, ``alpha = 1``, one iteration per step) and their real envs, stepped together.

    ``lam``, ``step_size``, ``init_cov`` (scalar covariance ``init_cov * I``, as ``MPPI`` takes it) and ``init_mean`` (``(H, A)``,
    default zeros) take one value for every episode or one per episode; ``seeds`` one seed per episode.  Settings the
    batch does not run raise ``ValueError`` before any engine or device memory exists: ``n_iters != 1``, ``alpha != 1``,
    ``time_based_weights``, ``cov_type != 'diagonal'``, ``base_action`` other than ``'null'`` / ``'repeat'``,
    ``use_zero_control_seq``, ``sample_mode != 'mean'``, ``gamma == 0`` and a model the tree engine refuses."""

    def __init__(self, raw_model, num_episodes, horizon, num_particles, lam, step_size, init_cov, gamma, filter_coeffs,
                 base_action, seeds, init_mean=None, dtype="f64", device=0, n_iters=1, alpha=1, time_based_weights=False,
                 cov_type="diagonal", use_zero_control_seq=False, sample_mode="mean", engine="tree"):
        self._pick_engine(engine, num_particles)
        # -- everything that can be refused is refused here, before the engine and its device memory exist
        if alpha != 1:
            raise ValueError("an episode batch runs MPPI without the control cost (alpha = 1), got %r" % (alpha,))
        if time_based_weights:
            raise ValueError("an episode batch does not run time_based_weights")
        if cov_type != "diagonal":
            raise ValueError("an episode batch samples with a diagonal covariance (cov_type 'diagonal'), got %r" % (cov_type,))
        E, H, P, fc = self._check_common(num_episodes, horizon, num_particles, n_iters, base_action, use_zero_control_seq,
                                         sample_mode, dtype, gamma, filter_coeffs, "MPPI")
        lam = _per_episode("lam", lam, E, sign="positive")
        step_size = _per_episode("step_size", step_size, E)
        init_cov = _per_episode("init_cov", init_cov, E, sign="positive")
        model = self._seeds_and_model(seeds, E, raw_model)
        A = model.nu
        init_mean = self._init_mean(init_mean, E, H, A)
        chols = self._diag_factors(init_cov, A)[1]                                  # (OLGaussianMPC: diag(init_cov))

        # -- the engine (its state shards are the E real envs) and the batch's device buffers
        self._setup(raw_model, model, E, H, P, dtype, device, base_action, gamma, fc, init_mean)
        self.lam, self.step_size, self.init_cov = lam, step_size, init_cov
        self._chols, self._lam, self._step = self._upload(chols), self._upload(lam), self._upload(step_size)
        self._ws = self._workspace(self.lib.mjmpc_update_batch_workspace_bytes(E, P, H, A))

    def _launches(self, act, s):
        """Enqueue one control step of every episode (sampling, rollouts, update, action, shift, real-env step) without a
        host synchronisation.  The actions, real-env costs and next observations stay on the device."""
        E, P, H, A = self.num_episodes, self.num_particles, self.horizon, self.d_action
        if self._generic is not None:           # (tracked terms; rate rows or one-sided kinds)
            return self._launches_tracked(act, s)
        self._draw(s)
        self._rollout(s)
        _lib.check(self.lib.mjmpc_mppi_fused_update_batch(self._code, E, P, H, A, _vp(self._q0), _vp(self._actions),
                                                          _vp(self._lam), _vp(self._step), _SHIFT_MODES[self.base_action],
                                                          _vp(self._means), _vp(act), _vp(self._step_dev), _vp(self._ws), s))


    _generic = None         # tracked terms: (workspace, covariances nobody reads, zero growth) of the general update

    def set_cost_terms(self, terms):
        """``_EpisodeBatch.set_cost_terms``.  With tracked terms the step takes the general softmax update - what the
        single-episode MPPI runs once its costs come from a launch behind the rollout - in place of the fused one: an episode
        of the batch stays, bit for bit, the sequential loop on an engine with the same tracked terms.  Tables with action-rate
        rows or one-sided kinds and tables with quadratic groups or linear rows take the same step,
        tracked or not, and are that loop bit for bit as well; every other table keeps the fused update."""
        super().set_cost_terms(terms)           # (every refusal of the terms themselves, before anything else)
        self._generic = None
        if self._track is None and not self._rate and self._quad is None:
            return
        E, P, H, A = self.num_episodes, self.num_particles, self.horizon, self.d_action
        nbytes = self.lib.mjmpc_dmd_batch_workspace_bytes(E, P, H, A)
        if nbytes <= 0:
            super().set_cost_terms(None)
            raise ValueError("no general-update workspace for tracked or rate terms with E = %d, P = %d, H = %d, A = %d (A <= 64)"
                             % (E, P, H, A))
        f64 = dict(dtype=self.torch.float64, device=self.device)
        self._generic = (self._workspace(nbytes), self.torch.zeros((E, A, A), **f64), self.torch.zeros(E, **f64))

    def _launches_tracked(self, act, s):
        """The step with tracked terms: draw + filter, the plain rollout costed by the terms, then ``mjmpc_dmd_update_batch`` -
        row e is ``mjmpc_softmax_stats`` + ``mjmpc_softmax_combine`` + ``mjmpc_step_tail``, the single-episode MPPI's general
        iteration - with a covariance per episode that it adapts and nobody reads (the draw keeps the static factors) and
        no growth."""
        E, P, H, A = self.num_episodes, self.num_particles, self.horizon, self.d_action
        ws, covs, beta = self._generic
        # (the draw of _draw with the filter as a pass of its own, then the plain rollout: the single path's launches)
        _lib.check(self.lib.mjmpc_sample_noise_cov_batch(self._code, E, _vp(self._noise), P, H, A, _vp(self._chols),
                                                         _vp(self._coeffs_unless_identity()), _vp(self._seeds), 0,
                                                         _vp(self._step_dev), 1, s))
        self._rollout(s, filtered=False, gseq=False, q0=False)
        _lib.check(self.lib.mjmpc_dmd_update_batch(self._code, E, P, H, A, _vp(self._costs), _vp(self._actions), _vp(self._gseq),
                                                   _vp(self._lam), _vp(self._step), 1, _vp(beta),
                                                   _SHIFT_MODES[self.base_action], _vp(self._means), _vp(covs), _vp(act),
                                                   _vp(self._step_dev), _vp(ws), s))


def _cem_limits():
    return "the batched fused CEM step takes A <= 8, A <= H + 1, P <= 32768 and 1 <= num_elite <= num_particles"


class BatchedCEM(_EpisodeBatch):
    """``num_episodes`` CEM controllers (cem.py, one iteration per step) and their real envs, stepped together.

    Episode e computes the bits of ``CEM(..., noise_mode='device', seed=seeds[e])`` on a ``TreeRolloutEngine`` of its own with
    ``make_device_rollout_fn`` and ``enable_graph(post_step=engine.step_state)``, whose step is the fused one
    (``mjmpc_cem_select_moments`` + ``mjmpc_cem_finish``).  ``init_cov`` (scalar: ``diag(init_cov)``, as ``CEM`` takes it),
    ``elite_frac``, ``step_size`` and ``beta`` take one value for every episode or one per episode (``num_elite_e =
    int(num_particles * elite_frac_e)``); ``seeds`` one seed per episode.  A control step is four launches - rollout,
    selection + moments, finish (refit, covariance growth, factor, action, shift, the next step's samples), real-env step -
    and a fifth, the first draw, on step 0.  Settings the batch does not run raise ``ValueError`` before any engine or
    device memory exists: ``n_iters != 1``, ``sample_mode != 'mean'``, ``use_zero_control_seq``, ``gamma == 0``, ``cov_type``
    other than ``'diagonal'`` / ``'full'``, ``base_action`` other than ``'null'`` / ``'repeat'``, a ``num_elite_e < 1``, a shape
    outside ``mjmpc_cem_batch_supported`` and a model the tree engine refuses.  An episode whose covariance turns indefinite
    raises ``MjmpcError`` where ``run`` / ``get_states`` / ``mean_action`` / ``cov`` synchronise."""

    def __init__(self, raw_model, num_episodes, horizon, num_particles, init_cov, elite_frac, step_size, beta, gamma,
                 filter_coeffs, base_action, seeds, cov_type="full", dtype="f64", device=0, n_iters=1, sample_mode="mean",
                 use_zero_control_seq=False, engine="tree"):
        self._pick_engine(engine, num_particles)
        # -- everything that can be refused is refused here, before the engine and its device memory exist
        if cov_type not in ("diagonal", "full"):
            raise ValueError("cov_type must be 'diagonal' or 'full' in a CEM episode batch, got %r" % (cov_type,))
        E, H, P, fc = self._check_common(num_episodes, horizon, num_particles, n_iters, base_action, use_zero_control_seq,
                                         sample_mode, dtype, gamma, filter_coeffs, "CEM")
        init_cov = _per_episode("init_cov", init_cov, E, sign="positive")
        elite_frac = _per_episode("elite_frac", elite_frac, E)
        step_size = _per_episode("step_size", step_size, E)
        beta = _per_episode("beta", beta, E)
        num_elite = np.array([int(P * f) for f in elite_frac], np.int64)          # (cem.py:18)
        if np.any(num_elite < 1) or np.any(num_elite > P):
            raise ValueError("every episode needs 1 <= num_elite = int(num_particles * elite_frac) <= num_particles, got %s"
                             % (num_elite.tolist(),))
        model = self._seeds_and_model(seeds, E, raw_model)
        A = model.nu
        lib = _lib.load()
        if not lib.mjmpc_cem_batch_supported(E, P, int(num_elite.max()), H, A):
            raise ValueError("%s; got A = %d, H = %d, P = %d, num_elite up to %d"
                             % (_cem_limits(), A, H, P, int(num_elite.max())))
        init_mean = np.zeros((E, H, A))                                            # (CEM starts from a zero mean)

        # -- the engine (its state shards are the E real envs) and the batch's device buffers
        self._setup(raw_model, model, E, H, P, dtype, device, base_action, gamma, fc, init_mean)
        self.init_cov, self.elite_frac, self.step_size, self.beta = init_cov, elite_frac, step_size, beta
        self.num_elite, self.cov_type = num_elite, cov_type
        # the first factor is the diagonal sqrt(init_cov): what the single path's first draw colours its samples with
        self._init_covs, self._init_chols, _ = self._diag_factors(init_cov, A)
        self._covs, self._chols = self._upload(self._init_covs), self._upload(self._init_chols)
        self._k, self._step = self._upload(num_elite), self._upload(step_size)
        self._grow_diag = self._upload(np.repeat(init_cov[:, None], A, axis=1))     # (cem.py:94)
        self._grow_scale = self._upload(beta)
        self._status = self.torch.zeros(E, dtype=self.torch.int32, device=self.device)
        self._ws = self._workspace(self.lib.mjmpc_cem_batch_workspace_bytes(E, P, int(num_elite.max()), H, A))
        self._noise_valid = False       # step 0 (and the step after reset) draws its own samples; later ones are drawn ahead

    cov = property(_cov)

    def reset(self):
        """Every episode back to its initial mean, covariance and factor and to step 0 (the real envs keep their states)."""
        super().reset()
        self._covs.copy_(self.torch.from_numpy(self._init_covs))
        self._chols.copy_(self.torch.from_numpy(self._init_chols))
        self._noise_valid = False

    def _launches(self, act, s):
        """Enqueue one control step of every episode (rollouts, selection + moments, refit + action + shift + the next step's
        samples, real-env step) without a host synchronisation; step 0 draws its samples first.  The actions, real-env costs
        and next observations stay on the device."""
        E, P, H, A = self.num_episodes, self.num_particles, self.horizon, self.d_action
        lib, code = self.lib, self._code
        if not self._noise_valid:
            # (the factors are diagonal here - diag(sqrt(init_cov)) -, for which the diagonal draw and the general one of the
            # single path's first step form the same 0 + l z per sample: DESIGN 10.2)
            self._draw(s)
            self._noise_valid = True
        self._rollout(s)
        _lib.check(lib.mjmpc_cem_select_moments_batch(code, E, P, H, A, _vp(self._actions), _vp(self._q0), _vp(self._k),
                                                      _vp(self._means), _vp(self._covs), _vp(self._step_dev), _vp(self._ws), s))
        _lib.check(lib.mjmpc_cem_finish_batch(code, E, P, H, A, _vp(self._k), int(self.cov_type == "full"), _vp(self._step),
                                              _SHIFT_MODES[self.base_action], _vp(self._means), _vp(self._covs),
                                              _vp(self._chols), _vp(self._status), _vp(self._grow_diag), _vp(self._grow_scale),
                                              _vp(act), _vp(self._step_dev), _vp(self._noise), _vp(self._seeds), 0,
                                              _vp(self._ws), s))


class BatchedDMDMPC(_EpisodeBatch):
    """``num_episodes`` DMD-MPC controllers that adapt their covariance (gaussian_dmd.py with ``update_cov=True``, one iteration
    per step) and their real envs, stepped together.

    Episode e computes the bits of ``DMDMPC(..., update_cov=True, cov_type=cov_type, noise_mode='device', noise_dtype=dtype,
    seed=seeds[e])`` on a ``TreeRolloutEngine`` of its own with ``make_device_rollout_fn`` and
    ``enable_graph(post_step=engine.step_state)``, whose step is the general one of ``OLGaussianMPC._device_iteration``: Cholesky
    factor, draw + filter, plain rollout, ``softmax_update`` with the covariance, ``step_tail`` with the growth ``beta I``.
    ``lam``, ``step_size``, ``init_cov`` (scalar: ``diag(init_cov)``, as ``DMDMPC`` takes it), ``beta`` and ``init_mean``
    (``(H, A)``, default zeros) take one value for every episode or one per episode; ``seeds`` one seed per episode.  A control
    step is eight launches - factors, draw, filter, rollout, weights + their maximum, partial moments, record + combine +
    tail, real-env step (seven with the identity filter) - and nothing synchronises.  Settings the batch does not run raise
    ``ValueError`` before any engine or device memory exists: ``update_cov=False`` (that arithmetic is ``BatchedMPPI``'s),
    ``n_iters != 1``, ``sample_mode != 'mean'``, ``use_zero_control_seq``, ``gamma == 0``, ``cov_type`` other than
    ``'diagonal'`` / ``'full'``, ``base_action`` other than ``'null'`` / ``'repeat'``, ``lam <= 0``, ``init_cov <= 0``,
    ``beta < 0``, more than 64 action channels (the Cholesky kernel's limit) and a model the tree engine refuses.  An episode
    whose covariance turns indefinite or non-finite raises ``MjmpcError`` where ``run`` / ``get_states`` / ``mean_action`` /
    ``cov`` synchronise."""

    def __init__(self, raw_model, num_episodes, horizon, num_particles, lam, step_size, init_cov, beta, gamma, filter_coeffs,
                 base_action, seeds, cov_type="full", update_cov=True, init_mean=None, dtype="f64", device=0, n_iters=1,
                 sample_mode="mean", use_zero_control_seq=False, engine="tree"):
        self._pick_engine(engine, num_particles)
        # -- everything that can be refused is refused here, before the engine and its device memory exist
        if not update_cov:
            raise ValueError("DMD-MPC without covariance adaptation (update_cov=False) is MPPI with alpha = 1: run it as "
                             "BatchedMPPI with the same lam, step_size and init_cov")
        if cov_type not in ("diagonal", "full"):
            raise ValueError("cov_type must be 'diagonal' or 'full' in a DMD-MPC episode batch, got %r" % (cov_type,))
        E, H, P, fc = self._check_common(num_episodes, horizon, num_particles, n_iters, base_action, use_zero_control_seq,
                                         sample_mode, dtype, gamma, filter_coeffs, "DMD-MPC")
        lam = _per_episode("lam", lam, E, sign="positive")
        step_size = _per_episode("step_size", step_size, E)
        init_cov = _per_episode("init_cov", init_cov, E, sign="positive")
        beta = _per_episode("beta", beta, E, sign="not negative")
        model = self._seeds_and_model(seeds, E, raw_model)
        A = model.nu
        if A > 64:
            raise ValueError("a DMD-MPC episode batch factors covariances of up to 64 action channels, got %d" % A)
        init_mean = self._init_mean(init_mean, E, H, A)
        nbytes = _lib.load().mjmpc_dmd_batch_workspace_bytes(E, P, H, A)
        if nbytes <= 0:
            raise ValueError("no DMD-MPC batch workspace for E = %d, P = %d, H = %d, A = %d" % (E, P, H, A))

        # -- the engine (its state shards are the E real envs) and the batch's device buffers
        f64 = self._setup(raw_model, model, E, H, P, dtype, device, base_action, gamma, fc, init_mean)
        self.lam, self.step_size, self.init_cov, self.beta, self.cov_type = lam, step_size, init_cov, beta, cov_type
        self._init_covs = self._diag_factors(init_cov, A)[0]                        # (OLGaussianMPC: diag(init_cov))
        self._covs = self._upload(self._init_covs)
        self._chols = self.torch.zeros((E, A, A), **f64)
        self._lam, self._step, self._beta = self._upload(lam), self._upload(step_size), self._upload(beta)
        self._status = self.torch.zeros(E, dtype=self.torch.int32, device=self.device)
        self._draw_coeffs = self._coeffs_unless_identity()      # (the filter pass leaves an identity's samples as they are)
        self._ws = self._workspace(nbytes)

    cov = property(_cov)

    def reset(self):
        """Every episode back to its initial mean and covariance and to step 0 (the real envs keep their states)."""
        super().reset()
        self._covs.copy_(self.torch.from_numpy(self._init_covs))

    def _launches(self, act, s):
        """Enqueue one control step of every episode (factors, draw + filter, rollouts, weights, partial moments, update +
        action + shift + covariance growth, real-env step) without a host synchronisation.  The actions, real-env costs and
        next observations stay on the device."""
        E, P, H, A = self.num_episodes, self.num_particles, self.horizon, self.d_action
        lib, code = self.lib, self._code
        _lib.check(lib.mjmpc_cholesky_lower_batch(E, _vp(self._covs), A, _vp(self._chols), _vp(self._status), s))
        _lib.check(lib.mjmpc_sample_noise_cov_batch(code, E, _vp(self._noise), P, H, A, _vp(self._chols), _vp(self._draw_coeffs),
                                                    _vp(self._seeds), 0, _vp(self._step_dev),
                                                    int(self.cov_type == "diagonal"), s))
        # (the samples are filtered already and the update forms its own cost-to-go: the single path's plain rollout)
        self._rollout(s, filtered=False, gseq=False, q0=False)
        _lib.check(lib.mjmpc_dmd_update_batch(code, E, P, H, A, _vp(self._costs), _vp(self._actions), _vp(self._gseq),
                                              _vp(self._lam), _vp(self._step), 2 if self.cov_type == "full" else 1,
                                              _vp(self._beta), _SHIFT_MODES[self.base_action], _vp(self._means),
                                              _vp(self._covs), _vp(act), _vp(self._step_dev), _vp(self._ws), s))


class BatchedMPPIQ(_EpisodeBatch):
    """``num_episodes`` MPPIQ controllers (mppiq.py, one iteration per step) and their real envs, stepped together.

    Episode e computes the bits of ``MPPIQ(..., alpha=alpha, time_based_weights=time_based_weights, noise_mode='device',
    noise_dtype=dtype, seed=seeds[e])`` on a ``TreeRolloutEngine`` of its own with ``make_device_rollout_fn``, whose step is the
    general one of ``OLGaussianMPC._device_iteration``: draw + filter with the static diagonal factor, plain rollout,
    ``mjmpc_td_lambda_returns``, ``softmax_update`` on the returns, ``step_tail`` - captured with
    ``enable_graph(post_step=engine.step_state)`` for ``alpha = 1``, eager for ``alpha = 0`` (which uploads ``cov^-1`` per step).
    ``beta`` (the temperature), ``step_size``, ``init_cov`` (scalar: ``diag(init_cov)``, as ``MPPIQ`` takes it) and ``td_lam``
    take one value for every episode or one per episode; ``seeds`` one seed per episode; ``alpha`` (1: no control cost, 0: the
    control cost with ``cov^-1 = diag(1 / init_cov_e)``), ``time_based_weights`` (a softmax per horizon step, ``MPPIQ``'s
    default) and ``gamma`` are shared.  The mean starts at zero.  A control step is seven launches - draw, filter, rollout,
    returns + weights + their maxima, partial moments, record + combine + tail, real-env step (six with the identity filter)
    - and nothing synchronises.  Out of scope: terminal Q estimates (open-loop rollouts produce no ``qvals``), ``_calc_val``
    and ``n_iters > 1``.  Settings the batch does not run raise ``ValueError`` before any engine or device memory exists:
    ``n_iters != 1``, ``sample_mode != 'mean'``, ``gamma == 0``, ``base_action`` other than ``'null'`` / ``'repeat'``, ``alpha``
    other than 0 / 1, ``beta <= 0``, ``init_cov <= 0``, ``td_lam`` outside [0, 1], a wrong seed count, a shape outside
    ``mjmpc_mppiq_batch_supported`` and a model the tree engine refuses."""

    def __init__(self, raw_model, num_episodes, horizon, num_particles, beta, step_size, init_cov, td_lam, gamma,
                 filter_coeffs, base_action, seeds, alpha=1, time_based_weights=True, dtype="f64", device=0, n_iters=1,
                 sample_mode="mean", engine="tree"):
        self._pick_engine(engine, num_particles)
        # -- everything that can be refused is refused here, before the engine and its device memory exist
        E, H, P, fc = self._check_common(num_episodes, horizon, num_particles, n_iters, base_action, False, sample_mode, dtype,
                                         gamma, filter_coeffs, "MPPIQ")
        if alpha not in (0, 1):
            raise ValueError("alpha must be 0 (control cost on) or 1 (off) in an MPPIQ episode batch, got %r" % (alpha,))
        beta = _per_episode("beta", beta, E, sign="positive")
        step_size = _per_episode("step_size", step_size, E)
        init_cov = _per_episode("init_cov", init_cov, E, sign="positive")
        td_lam = _per_episode("td_lam", td_lam, E)
        if not np.all((td_lam >= 0) & (td_lam <= 1)):
            raise ValueError("td_lam must lie in [0, 1]")
        tbw = int(bool(time_based_weights))
        lib = _lib.load()
        # (the support predicate's other limit, 1 <= A <= 64, needs the model: below)
        if not lib.mjmpc_mppiq_batch_supported(E, P, H, 1, tbw):
            raise ValueError("the batched MPPIQ step with time-based weights takes a horizon of up to 512, got %d" % H)
        model = self._seeds_and_model(seeds, E, raw_model)
        A = model.nu
        if not lib.mjmpc_mppiq_batch_supported(E, P, H, A, tbw):
            raise ValueError("the batched MPPIQ step takes up to 64 action channels, got A = %d" % A)
        # the single path's tables, by its expressions and so with its bits (DeviceUpdater.td_lambda_returns, MPPIQ._returns)
        wseq, wseq_zero = self._td_tables(td_lam, gamma, H)
        covs, chols, _ = self._diag_factors(init_cov, A)                            # (OLGaussianMPC: diag(init_cov))
        covinv = np.stack([np.linalg.inv(c) for c in covs]) if alpha == 0 else None

        # -- the engine (its state shards are the E real envs) and the batch's device buffers
        self._setup(raw_model, model, E, H, P, dtype, device, base_action, gamma, fc, np.zeros((E, H, A)))
        self.beta, self.step_size, self.init_cov, self.td_lam = beta, step_size, init_cov, td_lam
        self.alpha, self.time_based_weights = int(alpha), bool(tbw)
        self.wseq, self.wseq_zero = wseq, wseq_zero
        self._chols, self._beta, self._step = self._upload(chols), self._upload(beta), self._upload(step_size)
        self._td_lam, self._wseq, self._wseq_zero = self._upload(td_lam), self._upload(wseq), self._upload(wseq_zero)
        self._covinv = None if covinv is None else self._upload(covinv)
        self._draw_coeffs = self._coeffs_unless_identity()      # (the filter pass leaves an identity's samples as they are)
        self._ws = self._workspace(self.lib.mjmpc_mppiq_batch_workspace_bytes(E, P, H, A, tbw))

    @staticmethod
    def _td_tables(td_lam, gamma, H):
        """The TD(lambda) weight tables of the episodes, float64 ``[E][max(H - 1, 1)]``, and whether each holds a zero (int32
        ``[E]``: cost_to_go's pass-through branch) - ``DeviceUpdater.td_lambda_returns``'s expression per episode."""
        wseq = np.stack([np.cumprod([1.0] + [gamma * l] * (H - 2)) if H > 1 else np.array([1.0]) for l in td_lam])
        return wseq, np.array([int(bool(np.any(w == 0))) for w in wseq], np.int32)

    def _launches(self, act, s):
        """Enqueue one control step of every episode (draw + filter, rollouts, returns + weights, partial moments, update +
        action + shift, real-env step) without a host synchronisation.  The actions, real-env costs and next observations
        stay on the device."""
        E, P, H, A = self.num_episodes, self.num_particles, self.horizon, self.d_action
        lib, code = self.lib, self._code
        # (the static factors diag(sqrt(init_cov_e)): row e is the single path's mjmpc_sample_noise, draw then filter)
        _lib.check(lib.mjmpc_sample_noise_cov_batch(code, E, _vp(self._noise), P, H, A, _vp(self._chols), _vp(self._draw_coeffs),
                                                    _vp(self._seeds), 0, _vp(self._step_dev), 1, s))
        # (the samples are filtered already and the update forms its own returns: the single path's plain rollout)
        self._rollout(s, filtered=False, gseq=False, q0=False)
        _lib.check(lib.mjmpc_mppiq_update_batch(code, E, P, H, A, _vp(self._costs), _vp(self._actions), _vp(self._beta),
                                                _vp(self._step), _vp(self._td_lam), _vp(self._wseq), _vp(self._wseq_zero),
                                                self.gamma, self.alpha, _vp(self._covinv), int(self.time_based_weights),
                                                _SHIFT_MODES[self.base_action], _vp(self._means), _vp(act),
                                                _vp(self._step_dev), _vp(self._ws), s))


class BatchedPFMPC(_EpisodeBatch):
    """``num_episodes`` particle-filter MPC controllers (particle_filter_controller.py, one iteration per step) and their real
    envs, stepped together.

    Episode e computes the bits of ``PFMPC(..., noise_mode='device', seed=seeds[e])`` on a ``TreeRolloutEngine`` of its own with
    ``make_device_rollout_fn``, ``set_sim_state_fn = resident_state`` and ``set_post_step(engine.step_state)``, whose
    ``optimize()`` is called with ``hotstart=True``.  ``lam``, ``cov_shift`` and ``cov_resample`` (scalar variances, as ``PFMPC``
    takes them) take one value for every episode or one per episode; ``seeds`` one seed per episode.  A control step is seven
    launches - deviations, rollout, weights + first pointer, resampling, gather + shift, mean + action, real-env step - and
    nothing synchronises.  ``keep_stages=True`` also keeps the unshifted survivors, for ``last_step()``.  Settings the batch
    does not run raise ``ValueError`` before any engine or device memory exists: ``n_iters != 1``, ``sample_mode != 'mean'``,
    ``gamma == 0``, ``base_action`` other than ``'null'`` / ``'repeat'``, ``lam <= 0``, a negative ``cov_shift``,
    ``cov_resample <= 0``, a wrong seed count and a model the tree engine refuses."""

    def __init__(self, raw_model, num_episodes, horizon, num_particles, cov_shift, cov_resample, lam, gamma, filter_coeffs,
                 base_action, seeds, dtype="f64", device=0, n_iters=1, sample_mode="mean", keep_stages=False,
                 engine="tree"):
        self._pick_engine(engine, num_particles)
        # -- everything that can be refused is refused here, before the engine and its device memory exist
        E, H, P, fc = self._check_common(num_episodes, horizon, num_particles, n_iters, base_action, False, sample_mode, dtype,
                                         gamma, filter_coeffs, "PFMPC")
        if base_action == "repeat" and H < 2:
            raise ValueError("base_action 'repeat' needs a horizon of at least 2")
        lam = _per_episode("lam", lam, E, sign="positive")
        cov_shift = _per_episode("cov_shift", cov_shift, E, sign="not negative")
        cov_resample = _per_episode("cov_resample", cov_resample, E, sign="positive")
        model = self._seeds_and_model(seeds, E, raw_model)
        A = model.nu
        nbytes = _lib.load().mjmpc_pf_batch_workspace_bytes(E, P, H, A)
        if nbytes <= 0:
            raise ValueError("no particle-filter workspace for E = %d, P = %d, H = %d, A = %d" % (E, P, H, A))
        # the first sets' factors (DeviceUpdater.prepare_noise: the Cholesky factor of cov_resample I and its diagonal flag)
        _, init_chols, init_diag = self._diag_factors(cov_resample, A)

        # -- the engine (its state shards are the E real envs) and the batch's device buffers
        f64 = self._setup(raw_model, model, E, H, P, dtype, device, base_action, gamma, fc, np.zeros((E, H, A)))
        torch = self.torch
        self.lam, self.cov_shift, self.cov_resample, self.keep_stages = lam, cov_shift, cov_resample, bool(keep_stages)
        self._set, self._set_alt = (torch.empty((E, P, H, A), **f64) for _ in range(2))
        self._gathered = torch.empty((E, P, H, A), **f64) if self.keep_stages else None
        self._w, self._first = torch.empty((E, P), **f64), torch.zeros(E, **f64)
        self._idx = torch.empty((E, P), dtype=torch.int32, device=self.device)
        self._lam = self._upload(lam)
        # the jitters' factors: cov_shift is c I, its factor sqrt(c) I (a zero variance is a zero jitter, not an error)
        self._chols = self._upload(np.stack([np.sqrt(np.diag(np.full(A, c))) for c in cov_shift]))
        self._init_chols = [(self._upload(c), d) for c, d in zip(init_chols, init_diag)]
        self._shift_coeffs = self._coeffs_unless_identity()               # (as the single path hands them to the gather)
        self._ws = self._workspace(nbytes)
        self._delta = self._noise                                         # (the rollout launch's noise is set - mean)
        self._stepped = False
        self._draw_initial_sets()

    def _draw_initial_sets(self):
        """Row e <- the single path's first set: ``DeviceUpdater.sample_noise(P, cov_resample_e I, filter_coeffs, seed_e, 0,
        'f64')``, E calls of the single sampler (off the hot path)."""
        P, H, A, s = self.num_particles, self.horizon, self.d_action, self._stream()
        for e, (chol, diag) in enumerate(self._init_chols):
            _lib.check(self.lib.mjmpc_sample_noise(_lib.F64, _vp(self._set[e]), P, H, A, _vp(chol), _vp(self._coeffs),
                                                   int(self.seed_vals[e]) & (2 ** 64 - 1), 0, 0, None, diag, s))

    @property
    def action_samples(self):
        """The E particle sets the next step rolls out, ``(E, P, H, A)`` (synchronises)."""
        out = self._set.cpu().numpy().copy()
        self._check_status()
        return out

    def reset(self):
        """Every episode back to its initial set, a zero mean and step 0 (the real envs keep their states)."""
        super().reset()
        self._draw_initial_sets()
        self._stepped = False

    def step(self, _out=None):
        """Enqueue one control step of every episode (deviations, rollouts, weights, resampling, gather + shift, mean + action,
        real-env step) without a host synchronisation.  The actions, real-env costs and next observations stay on the device."""
        out = super().step(_out)
        self._set, self._set_alt = self._set_alt, self._set
        self._stepped = True
        return out

    def _launches(self, act, s):
        E, P, H, A = self.num_episodes, self.num_particles, self.horizon, self.d_action
        lib = self.lib
        _lib.check(lib.mjmpc_pf_delta_batch(self._code, E, P, H, A, _vp(self._set), _vp(self._means), _vp(self._delta), s))
        # (the set is filtered already: the rollout takes the deviations as they are, as the single path's fused(.., None, ..))
        self._rollout(s, noise=self._delta, filtered=False)
        _lib.check(lib.mjmpc_pf_weights_batch(E, P, _vp(self._q0), _vp(self._lam), _vp(self._seeds), 0, _vp(self._step_dev),
                                              _vp(self._w), _vp(self._first), s))
        _lib.check(lib.mjmpc_pf_resample_batch(E, P, _vp(self._w), _vp(self._first), _vp(self._idx), _vp(self._ws), s))
        # (keyed with offset k + 1: the reference increments num_steps before _shift)
        _lib.check(lib.mjmpc_pf_gather_shift_batch(E, P, H, A, _vp(self._set), _vp(self._idx), _SHIFT_MODES[self.base_action],
                                                   _vp(self._chols), _vp(self._shift_coeffs), _vp(self._seeds), 1,
                                                   _vp(self._step_dev), _vp(self._set_alt), _vp(self._gathered), _vp(self._ws),
                                                   s))
        _lib.check(lib.mjmpc_pf_finish_batch(E, P, H, A, _vp(self._ws), _vp(self._means), _vp(act), _vp(self._step_dev), s))

    def last_step(self):
        """The stages of the last step as device tensors with a leading E axis (valid until the next step), as
        ``PFMPC.last_device_step`` names them: ``samples`` the sets that were rolled out, ``costs`` / ``q0`` what the rollout
        returned, ``w``, ``first``, ``idx``, ``resampled`` = samples[idx], ``mean`` of it, ``shifted`` the sets the next step
        rolls out, ``step`` the count k the step was keyed with.  Needs ``keep_stages=True`` and a step."""
        if not self.keep_stages or not self._stepped:
            raise ValueError("last_step needs keep_stages=True and a finished step")
        E, P, H = self.num_episodes, self.num_particles, self.horizon
        return dict(samples=self._set_alt, costs=self._costs.view(E, P, H), q0=self._q0.view(E, P), w=self._w,
                    first=self._first, idx=self._idx, resampled=self._gathered, mean=self._means, shifted=self._set,
                    step=self.num_steps - 1)


class BatchedRandomShooting(_EpisodeBatch):
    """``num_episodes`` random-shooting controllers (random_shooting.py, one iteration per step) and their real envs, stepped
    together.

    Episode e computes the bits of ``RandomShooting(..., noise_mode='device', noise_dtype=dtype, seed=seeds[e])`` on a
    ``TreeRolloutEngine`` of its own with ``make_device_rollout_fn`` and ``enable_graph(post_step=engine.step_state)``: the
    Philox draw with the static diagonal factor, the fused rollout (filter + rollout + cost-to-go), ``mjmpc_rs_best`` +
    ``mjmpc_rs_combine`` and ``mjmpc_step_tail``.  ``step_size``, ``init_cov`` (scalar: ``diag(init_cov)``, as ``RandomShooting``
    takes it) and ``init_mean`` (``(H, A)``, default zeros) take one value for every episode or one per episode; ``seeds`` one
    seed per episode.  A control step is four launches - draw, rollout, selection + blend + action + shift, real-env step -
    and nothing synchronises.  An episode whose cost-to-go values are all ``+inf`` takes particle 0, as ``np.argmin`` does (the
    single path is undefined there).  Settings the batch does not run raise ``ValueError`` before any engine or device memory
    exists: ``n_iters != 1``, ``sample_mode != 'mean'``, ``use_zero_control_seq``, ``gamma == 0``, ``base_action`` other than
    ``'null'`` / ``'repeat'``, ``init_cov <= 0``, ``step_size < 0``, a wrong seed count, a shape outside
    ``mjmpc_rs_batch_supported`` and a model the tree engine refuses."""

    def __init__(self, raw_model, num_episodes, horizon, num_particles, step_size, init_cov, gamma, filter_coeffs, base_action,
                 seeds, init_mean=None, dtype="f64", device=0, n_iters=1, use_zero_control_seq=False, sample_mode="mean",
                 engine="tree"):
        self._pick_engine(engine, num_particles)
        # -- everything that can be refused is refused here, before the engine and its device memory exist
        E, H, P, fc = self._check_common(num_episodes, horizon, num_particles, n_iters, base_action, use_zero_control_seq,
                                         sample_mode, dtype, gamma, filter_coeffs, "random-shooting")
        step_size = _per_episode("step_size", step_size, E, sign="not negative")
        init_cov = _per_episode("init_cov", init_cov, E, sign="positive")
        model = self._seeds_and_model(seeds, E, raw_model)
        A = model.nu
        if not _lib.load().mjmpc_rs_batch_supported(E, P, H, A):
            raise ValueError("the batched random-shooting step takes up to 256 action channels, got A = %d" % A)
        init_mean = self._init_mean(init_mean, E, H, A)
        chols = self._diag_factors(init_cov, A)[1]                                  # (OLGaussianMPC: diag(init_cov))

        # -- the engine (its state shards are the E real envs) and the batch's device buffers
        self._setup(raw_model, model, E, H, P, dtype, device, base_action, gamma, fc, init_mean)
        self.step_size, self.init_cov = step_size, init_cov
        self._chols, self._step = self._upload(chols), self._upload(step_size)
        self._best = self.torch.zeros(E, dtype=self.torch.int64, device=self.device)

    @property
    def best_particle(self):
        """The particle every episode's last step moved its mean towards, ``(E,)`` int64 (synchronises)."""
        out = self._best.cpu().numpy().copy()
        self._check_status()
        return out

    def _launches(self, act, s):
        """Enqueue one control step of every episode (sampling, rollouts, selection + blend + action + shift, real-env step)
        without a host synchronisation.  The actions, real-env costs and next observations stay on the device."""
        E, P, H, A = self.num_episodes, self.num_particles, self.horizon, self.d_action
        self._draw(s)
        self._rollout(s)
        _lib.check(self.lib.mjmpc_rs_update_batch(self._code, E, P, H, A, _vp(self._q0), _vp(self._actions), _vp(self._step),
                                                  _SHIFT_MODES[self.base_action], _vp(self._means), _vp(act),
                                                  _vp(self._step_dev), _vp(self._best), s))
