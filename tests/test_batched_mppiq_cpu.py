"""CPU: ``BatchedMPPIQ`` refuses what it does not run before any engine or device memory exists, broadcasts its
per-episode settings as the other batches do, builds the single path's TD(lambda) weight tables, and its entry points are
declared, bound, built and reject bad arguments; the two ``mppiq`` config blocks name what the batched driver takes."""
import ctypes
import os
import sys

import numpy as np
import pytest

import batched_cases as bc
from batched_cases import no_engine  # noqa: F401
from mjmpc_amd import _lib
from mjmpc_amd.models.half_cheetah import half_cheetah_raw

NEW_SYMBOLS = ["mjmpc_mppiq_batch_supported", "mjmpc_mppiq_batch_workspace_bytes", "mjmpc_mppiq_update_batch"]
E_BADARG = -1               # (MJMPC_E_BADARG of include/mjmpc_amd.h)


def _kw(**over):
    kw = dict(raw_model=half_cheetah_raw(), num_episodes=4, horizon=8, num_particles=64, beta=0.2, step_size=0.8, init_cov=0.3,
              td_lam=0.9, gamma=1.0, filter_coeffs=[0.25, 0.8, 0.0], base_action="null", seeds=[1, 2, 3, 4])
    kw.update(over)
    return kw


@pytest.mark.parametrize("over", bc.COMMON_REFUSED + [
    dict(alpha=2), dict(beta=0), dict(beta=[0.2, 0.2, 0.2, -1]), dict(td_lam=1.5), dict(td_lam=-0.1), dict(init_cov=0),
    dict(horizon=513, time_based_weights=True),             # (outside mjmpc_mppiq_batch_supported: the partial launch's LDS)
    dict(raw_model=bc.rk4_hand()),
    # per-episode arrays of the wrong length, and values that are no numbers
    dict(beta=[0.2] * 3), dict(td_lam=np.ones(5)), dict(td_lam=[0.5, 0.5, 1.5, 0.5]), dict(td_lam=float("nan")),
    dict(beta=float("nan")), dict(init_cov=[0.3, 0.3, -1.0, 0.3]), dict(alpha=-1), dict(alpha=0.5),
], ids=bc.refused_id())
def test_unsupported_settings_raise_before_any_engine(no_engine, over):     # noqa: F811
    from mjmpc_amd.control import BatchedMPPIQ
    with pytest.raises(ValueError):
        BatchedMPPIQ(**_kw(**over))


def test_supported_settings_reach_the_engine(no_engine):                    # noqa: F811
    """The settings the batch runs pass the checks (and then get as far as making the engine)."""
    from mjmpc_amd.control import BatchedMPPIQ
    bc.check_reaches_the_engine(BatchedMPPIQ, [
        _kw(), _kw(alpha=0), _kw(time_based_weights=False), _kw(td_lam=0.0), _kw(td_lam=1.0), _kw(num_particles=50),
        _kw(num_episodes=1, seeds=[9]), _kw(horizon=512), _kw(horizon=513, time_based_weights=False), _kw(horizon=1),
        _kw(beta=[0.1, 0.2, 0.3, 0.4], step_size=[1.0, 0.9, 0.8, 0.7], init_cov=[0.2, 0.3, 0.4, 0.5], td_lam=[0.0, 0.5, 0.9, 1.0],
            alpha=0, base_action="repeat", dtype="f32", seeds=np.arange(4))])


def test_per_episode_broadcasting(monkeypatch):
    """One value for every episode or one per episode, as they reach the batch's set-up; the mean starts at zero."""
    from mjmpc_amd.control import BatchedMPPIQ
    seen = bc.stop_at_setup(monkeypatch)
    for P in (64, 50, 1000):
        bc.check_stops_at_setup(BatchedMPPIQ, _kw(num_particles=P), seen, 4, 8, P)
        assert seen["init_mean"].shape == (4, 8, 6) and not seen["init_mean"].any()
    bc.check_per_episode("beta", 0.2, [0.1, 0.2, 0.3, 0.4])
    bc.check_per_episode("step_size", 0.8, [1.0, 0.7, 0.4, 0.0])
    bc.check_per_episode("init_cov", 0.3, [0.2, 0.3, 0.4, 0.5])
    bc.check_per_episode("td_lam", 0.9, [0.0, 0.5, 0.9, 1.0])


def test_batched_mppiq_is_exported():
    bc.check_exported("BatchedMPPIQ",
                      ("set_states", "get_states", "mean_action", "reset", "step", "run", "close", "on_env_reset",
                       "randomize_dynamics", "clear_dynamics"),
                      # the base class's, unchanged
                      ("run", "step", "set_states", "get_states", "mean_action", "reset", "randomize_dynamics", "clear_dynamics",
                       "close", "on_env_reset"))


def test_new_entry_points_are_declared_bound_and_built():
    bc.check_entry_points(NEW_SYMBOLS, abi=4)


def test_supported_shapes_and_workspace():
    lib = _lib.load()
    ok, nbytes = lib.mjmpc_mppiq_batch_supported, lib.mjmpc_mppiq_batch_workspace_bytes
    for good in ((1, 1, 1, 1, 1), (3, 1040, 5, 3, 1), (3, 1040, 5, 3, 0), (65535, 256, 32, 6, 1), (4, 2 ** 33, 32, 6, 0),
                 (2, 17, 1, 2, 1), (1, 64, 8, 64, 1), (3, 64, 512, 6, 1), (3, 64, 513, 6, 0), (3, 64, 4000, 6, 0)):
        assert ok(*good) == 1, good
    for bad in ((0, 64, 8, 6, 1), (65536, 64, 8, 6, 1), (-1, 64, 8, 6, 0), (3, 0, 8, 6, 1), (3, -5, 8, 6, 0), (3, 64, 0, 6, 1),
                (3, 64, 8, 0, 1), (3, 64, 8, 65, 0), (3, 64, 513, 6, 1), (3, 64, 4000, 6, 1)):
        assert ok(*bad) == 0, bad
        assert nbytes(*bad) < 0, bad
    for bad in ((0, 64, 8, 6, 1), (3, 64, 8, 65, 1), (3, 64, 513, 6, 1)):       # (E = 0, A = 65, H = 513 with time-based weights)
        assert nbytes(*bad) < 0, bad
        assert len(lib.mjmpc_last_error()) > 0
    # the row layout: un[HA] | returns [P H] | x [P Hw] | xmax [Hw] | record [2 Hw + HA + AA] | partials [nb][Hw + HA + AA]
    for E, P, H, A, tbw in ((3, 1040, 5, 3, 1), (3, 1040, 5, 3, 0), (2, 17, 1, 2, 1), (16, 256, 32, 6, 1)):
        Hw, nb, HA, AA = (H if tbw else 1), (P + 15) // 16, H * A, A * A
        row = HA + P * H + P * Hw + Hw + (2 * Hw + HA + AA) + nb * (Hw + HA + AA)
        assert nbytes(E, P, H, A, tbw) == 8 * E * row


def test_update_entry_point_rejects_bad_arguments():
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)            # never dereferenced: every call below is refused on its arguments
    F = _lib.F64
    upd = lib.mjmpc_mppiq_update_batch

    def call(code=F, E=3, P=64, H=8, A=6, costs=fake, actions=fake, beta=fake, step=fake, td_lam=fake, wseq=fake, wz=fake,
             alpha=1, covinv=None, tbw=1, shift=0, means=fake, ws=fake):
        return upd(code, E, P, H, A, costs, actions, beta, step, td_lam, wseq, wz, 1.0, alpha, covinv, tbw, shift, means, None,
                   None, ws, None)
    bad = [dict(costs=None), dict(actions=None), dict(beta=None), dict(step=None), dict(td_lam=None), dict(wseq=None),
           dict(wz=None), dict(means=None), dict(ws=None), dict(E=0), dict(E=65536), dict(P=0), dict(H=0), dict(A=0), dict(A=65),
           dict(H=513), dict(code=7), dict(alpha=2), dict(alpha=0), dict(shift=2), dict(shift=-1),
           dict(E=0, costs=None, actions=None, means=None, ws=None)]
    for kw in bad:
        assert call(**kw) == E_BADARG, kw
        assert len(lib.mjmpc_last_error()) > 0, kw


def test_weight_tables_are_the_single_paths():
    """``wseq_e`` is ``oracle.controllers_ref.mppiq_returns``'s expression (and ``DeviceUpdater.td_lambda_returns``'s) for every
    episode, to the bit - a ``td_lam`` of 0 (zeros in the table: cost_to_go's pass-through branch) and of 1 among them."""
    from mjmpc_amd.control import BatchedMPPIQ
    td_lam = np.array([0.85, 0.0, 1.0, 0.3])
    for gamma in (0.97, 1.0, 1):
        for H in (1, 2, 3, 8):
            wseq, zero = BatchedMPPIQ._td_tables(td_lam, gamma, H)
            assert wseq.shape == (4, max(H - 1, 1)) and wseq.dtype == np.float64
            assert zero.shape == (4,) and zero.dtype == np.int32
            for e, lam in enumerate(td_lam):
                want = np.array([1.0]) if H == 1 else np.cumprod([1.0] + [gamma * lam] * (H - 2))     # (controllers_ref.py:125-128)
                assert np.array_equal(wseq[e], want), (H, e)
                assert bool(zero[e]) == bool(np.any(want == 0)) == (lam == 0.0 and H > 2)


@pytest.mark.parametrize("cfg,alpha,td_lam_is_one", [("half_cheetah_gpu.yml", 1, False), ("cartpole_gpu.yml", 0, True)])
def test_config_blocks_name_what_the_batched_driver_takes(cfg, alpha, td_lam_is_one):
    import yaml
    sys.path.insert(0, os.path.join(bc.ROOT, "examples"))
    try:
        from example_mpc_batched import BATCHES
    finally:
        sys.path.remove(os.path.join(bc.ROOT, "examples"))
    from mjmpc_amd.control import BatchedMPPIQ
    cls, names, optional = BATCHES["mppiq"]
    assert cls is BatchedMPPIQ and names == ("beta", "step_size", "init_cov", "td_lam")
    assert optional == dict(alpha=1, time_based_weights=True)
    with open(os.path.join(bc.ROOT, "examples", "configs", cfg)) as f:
        block = yaml.safe_load(f)["mppiq"]
    for n in names + tuple(optional) + ("horizon", "gamma", "n_iters", "filter_coeffs", "particles_per_cpu"):
        assert n in block, n
    assert block["alpha"] == alpha and block["time_based_weights"] is True and block["n_iters"] == 1
    assert (block["td_lam"] == 1.0) == td_lam_is_one and 0.0 <= block["td_lam"] <= 1.0
